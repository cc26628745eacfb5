"""The captured DRS-Net train step (R_NETWORK, mode 'drs', dp.TrainStep with use_graph) at [32, 256, 256] on the fused mask +
synthesis node (network_functions._real_step_fused: dcs_complex_abs_f32 + the dcs_rmask_apply_polar_frames pair, csrc/mask.hip)
against the op-by-op spelling it replaces (network_functions.RSTEP_FUSED off: torch.abs / atan2 / sigmoid / cos / sin / complex /
pad / transpose / irfft under autograd).  Two TrainSteps over the same seeded state and batch live in one process, each captured
under its own route; their replays are timed in alternating windows bracketed by events (at least 1 s and 10 windows of each)
and the medians compared.  No target is fixed: the op-by-op route in the same process is the yardstick.  Also recorded: the number
of kernel nodes of each route's captured graph (a second capture of each, kept as a graph, queried and never replayed).

usage: python tools/rstep_bench.py [--out profiles/rstep_bench.json] [--batch 32] [--frames 256] [--no-dropout]"""
import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'dcs-net_amd'))
from dcsnet import network_functions as nf  # noqa: E402
from dcsnet.config import config, hparams  # noqa: E402
from dcsnet.dp import TrainStep  # noqa: E402
from dcsnet.r_network import R_NETWORK  # noqa: E402
from oracle.seeded_state import fill_state_stream, seeded_input  # noqa: E402

ROUTES = (('fused', True), ('unfused', False))


HP = dict(hparams)


def _train_step(dev, fused, batch, warmup=2):
    """A TrainStep on the seeded DRS-Net, captured under the given route (the route is read while the step is issued, i.e. at the
    warm-up steps and at capture; a replay is whatever was captured)."""
    nf.RSTEP_FUSED = fused
    net = fill_state_stream(R_NETWORK(config, dict(HP), 0), 5).to(dev).train()      # the reference's dropout, batch statistics
    ts = TrainStep(net, use_graph=True, graph_warmup=warmup)
    for _ in range(warmup + 1):
        ts(batch)
    torch.cuda.synchronize()
    if ts._graph is None:
        raise RuntimeError(f'rstep_bench: the {"fused" if fused else "unfused"} step was not captured')
    return ts


def _kernel_nodes(dev, fused, batch, warmup=2):
    """Kernel nodes (and all nodes) of the route's captured graph: the step captured once more into a graph that is kept
    (torch.cuda.CUDAGraph(keep_graph=True)), asked for its nodes, and dropped without being instantiated or replayed."""
    nf.RSTEP_FUSED = fused
    net = fill_state_stream(R_NETWORK(config, dict(HP), 0), 5).to(dev).train()
    ts = TrainStep(net, use_graph=True, graph_warmup=warmup)
    for _ in range(warmup):
        ts(batch)
    plain = torch.cuda.CUDAGraph
    torch.cuda.CUDAGraph = lambda: plain(keep_graph=True)
    try:
        ts._capture(batch)
    finally:
        torch.cuda.CUDAGraph = plain
    torch.cuda.synchronize()
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), 'lib', 'libamdhip64.so'))
    graph = ctypes.c_void_p(ts._graph.raw_cuda_graph())
    n = ctypes.c_size_t(0)
    if hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) != 0:
        raise RuntimeError('hipGraphGetNodes failed')
    nodes = (ctypes.c_void_p * n.value)()
    if hip.hipGraphGetNodes(graph, nodes, ctypes.byref(n)) != 0:
        raise RuntimeError('hipGraphGetNodes failed')
    kernels = 0
    for node in nodes:
        kind = ctypes.c_int(-1)
        if hip.hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(kind)) != 0:
            raise RuntimeError('hipGraphNodeGetType failed')
        kernels += kind.value == 0                           # hipGraphNodeTypeKernel
    return {'kernel_nodes': int(kernels), 'nodes': int(n.value)}


def measure(dev, B, T, min_window_s=1.0):
    clean, noise = seeded_input(B, 256, T, 1, 0.1), seeded_input(B, 256, T, 2, 0.05)
    batch = (noise.to(dev), (clean + noise).to(dev), clean.to(dev), list(range(B)))
    steps = {name: _train_step(dev, fused, batch) for name, fused in ROUTES}
    inputs = {name: (*ts.input_buffers(), batch[3]) for name, ts in steps.items()}       # the static buffers: no staging copies
    first = {name: float(steps[name](inputs[name])) for name in steps}

    def window(name, n):
        ts, b = steps[name], inputs[name]
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            ts(b)
        e.record()
        e.synchronize()
        return s.elapsed_time(e)

    for name in steps:
        window(name, 5)
    n = max(3, math.ceil(100.0 / max(window(name, 5) / 5 for name in steps)))          # windows of about 0.1 s
    times = {name: [] for name in steps}
    total = {name: 0.0 for name in steps}
    while min(total.values()) < min_window_s or len(times['fused']) < 10:
        for name in steps:                                                               # alternating windows of n replays
            ms = window(name, n)
            times[name].append(ms / n)
            total[name] += ms / 1e3
    res = {'B': B, 'T': T, 'mode': 'drs', 'windows': len(times['fused']), 'steps_per_window': n,
           'loss_after_capture': first}
    for name in steps:
        res[name] = {'ms_per_step_median': round(float(np.median(times[name])), 4),
                     'ms_per_step_min': round(float(np.min(times[name])), 4), 'timed_s': round(total[name], 2)}
    f, u = res['fused']['ms_per_step_median'], res['unfused']['ms_per_step_median']
    res['speedup_median'] = round(u / f, 4)
    res['fused_at_least_as_fast'] = bool(f <= u)
    return res, batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rstep_bench.json'))
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--no-dropout', action='store_true', help='dropout_conv = dropout_fc = 0 instead of the configured 0.1 / 0.2')
    a = ap.parse_args()
    if a.no_dropout:
        HP['dropout_conv'], HP['dropout_fc'] = 0.0, 0.0
    sys.argv = ['train.py', 'drs', '0']                                   # the mode the step functions read (network_functions._mode)
    dev = torch.device('cuda:0')
    default_route = nf.RSTEP_FUSED
    res = {'metric': 'drs_train_step_fused_vs_unfused', 'device': torch.cuda.get_device_name(0),
           'default_route': 'fused' if default_route else 'unfused', 'dropout': [HP['dropout_conv'], HP['dropout_fc']]}

    def write():
        print(json.dumps(res))
        if a.out != '-':
            with open(a.out, 'w') as f:
                json.dump(res, f, indent=1)

    try:
        timing, batch = measure(dev, a.batch, a.frames)
        res.update(timing)
        write()                                                           # the timing is on disk before the graphs are queried
        try:
            for name, fused in ROUTES:
                res[name].update(_kernel_nodes(dev, fused, batch))
        except Exception as e:                                            # noqa: BLE001 - the timing stands without the counts
            res['kernel_nodes_error'] = f'{type(e).__name__}: {e}'
        write()
    finally:
        nf.RSTEP_FUSED = default_route


if __name__ == '__main__':
    main()
