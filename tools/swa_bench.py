"""Device time of one stochastic-weight-averaging update (ops.swa_average, csrc/swa.hip: two fp32 streams in, one out) at the
size of C_NETWORK's flat parameter bucket.  Two figures, each from HIP events around at least --seconds of calls:
  graph_us   calls captured 50 to a graph and replayed back to back: the kernel's own cost
  eager_us   one call at a time from the host, as dcsnet/swa.py issues it once per epoch (launch overhead included)
Prints one JSON line.  usage: python tools/swa_bench.py [--seconds 1.0]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'dcs-net_amd'))
from dcsnet import ops  # noqa: E402
from dcsnet.c_network import C_NETWORK  # noqa: E402
from dcsnet.config import config, hparams  # noqa: E402
from dcsnet.dp import FlatBucket  # noqa: E402


def _timed(fn, calls_per_fn, seconds):
    """ms per call over repetitions of fn() filling at least `seconds` of device time (events on the current stream)."""
    reps = 4
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= seconds * 1e3:
            return ms / (reps * calls_per_fn), reps * calls_per_fn, ms
        reps = int(reps * min(64.0, max(2.0, 1.3 * seconds * 1e3 / max(ms, 1e-3))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=1.0)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    n = FlatBucket(C_NETWORK(config, dict(hparams), 0)).numel
    g = torch.Generator().manual_seed(0)
    avg, p = torch.randn(n, generator=g).to(dev), torch.randn(n, generator=g).to(dev)
    for i in range(10):
        ops.swa_average(avg, p, i)
    torch.cuda.synchronize()
    per_graph = 50
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(per_graph):
            ops.swa_average(avg, p, 1 + i)
    graph.replay()
    torch.cuda.synchronize()
    g_ms, g_calls, g_total = _timed(graph.replay, per_graph, args.seconds)
    e_ms, e_calls, e_total = _timed(lambda: ops.swa_average(avg, p, 7), 1, args.seconds)
    moved = 3 * 4 * n
    print(json.dumps({'what': 'dcs_swa_average_f32', 'n': n, 'bytes_per_call': moved,
                      'graph_us': round(g_ms * 1e3, 3), 'graph_calls': g_calls, 'graph_total_ms': round(g_total, 1),
                      'graph_GBps': round(moved / (g_ms * 1e-3) / 1e9, 1),
                      'eager_us': round(e_ms * 1e3, 3), 'eager_calls': e_calls, 'eager_total_ms': round(e_total, 1),
                      'device': torch.cuda.get_device_name(0)}))


if __name__ == '__main__':
    main()
