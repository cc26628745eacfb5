"""What a checkpoint costs a running train step (dcsnet/checkpoint.py): a captured C_NETWORK step at [B, 256, T] (32 x 256 x 256
by default) with a checkpoint every k-th replay, three routes alternating in event-timed windows of at least --seconds:
  none    no checkpoint
  sync    save_checkpoint: device-to-host reads on the step's stream, the file written by the calling thread
  async   CheckpointWriter: one snapshot launch, the copy on a side stream, the file written by a thread
and the device time of the snapshot launch itself against one copy_ per tensor into the same slab (each captured 20 times to a
graph and replayed back to back: the kernels' own cost, not the host's launch rate).
Prints one JSON line and writes it to profiles/checkpoint_bench.json.
usage: python tools/checkpoint_bench.py [--seconds 1.0 --every 50 --rounds 3 --batch 32 --frames 256]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'dcs-net_amd'))
from dcsnet import ops  # noqa: E402
from dcsnet.c_network import C_NETWORK  # noqa: E402
from dcsnet.checkpoint import CheckpointWriter, save_checkpoint  # noqa: E402
from dcsnet.config import config, hparams  # noqa: E402
from dcsnet.dp import TrainStep, plateau_scheduler  # noqa: E402
from dcsnet.swa import StochasticWeightAveraging  # noqa: E402


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
            return ms / (reps * calls_per_fn)
        reps = int(reps * min(64.0, max(2.0, 1.3 * seconds * 1e3 / max(ms, 1e-3))))


def _window(step, batch, seconds, every, save):
    """(ms per step, steps, checkpoints) of one window: whole periods of `every` replays until `seconds` have passed."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    steps = saves = 0
    t0 = time.perf_counter()
    e0.record()
    while time.perf_counter() - t0 < seconds or steps == 0:
        for _ in range(every):
            step(batch)
        steps += every
        if save is not None:
            save()
            saves += 1
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps, steps, saves


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--every', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=256)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    net = C_NETWORK(config, dict(hparams), 0).to(dev).train()
    step = TrainStep(net, use_graph=True)
    swa = StochasticWeightAveraging(step, 2, lr_scheduler=plateau_scheduler(step.optimizer))
    swa.on_train_epoch_start(0)                                # averaging: the slab holds the average too
    g = torch.Generator().manual_seed(1)
    clean = torch.view_as_complex(0.1 * torch.randn(a.batch, 256, a.frames, 2, generator=g)).to(dev)
    noise = torch.view_as_complex(0.05 * torch.randn(a.batch, 256, a.frames, 2, generator=g)).to(dev)
    batch = (noise, clean + noise, clean, list(range(a.batch)))
    for _ in range(6):
        step(batch)
    assert step._graph is not None, 'capture did not happen'
    batch = (*step.input_buffers(), batch[3])                  # no staging copies: the step reads its own buffers
    out = tempfile.mkdtemp(prefix='checkpoint_bench_')
    try:
        writer = CheckpointWriter(step, swa)
        path = os.path.join(out, 'last.ckpt')

        def drain():
            while writer.poll():
                time.sleep(0.005)
            torch.cuda.synchronize()
        routes = {'none': None, 'sync': lambda: save_checkpoint(path, step, swa),
                  'async': lambda: writer.save(path)}
        rows = {k: [] for k in routes}
        for _ in range(a.rounds):
            for name, save in routes.items():
                ms, steps, saves = _window(step, batch, a.seconds, a.every, save)
                drain()                                         # (not timed: the next window must start idle)
                rows[name].append({'ms_per_step': round(ms, 4), 'steps': steps, 'checkpoints': saves})
        rejected = len(writer.rejected)
        # the launch itself against its copy_-per-tensor equivalent, 20 to a graph
        table, slab, counts = writer._table, writer._slab, writer._counts
        views = [table.view(slab, i) for i in range(table.n)]
        per = 20
        g_snap, g_copy = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        ops.snapshot(table, slab, counts)
        torch.cuda.synchronize()
        with torch.cuda.graph(g_snap):
            for _ in range(per):
                ops.snapshot(table, slab, counts)
        with torch.cuda.graph(g_copy):
            for _ in range(per):
                for v, t in zip(views, table.tensors):
                    v.copy_(t)
        snap_ms, copy_ms = _timed(g_snap.replay, per, a.seconds), _timed(g_copy.replay, per, a.seconds)
        nbytes = writer.bytes_per_checkpoint
        writer.close()
    finally:
        shutil.rmtree(out, ignore_errors=True)
    mean = {k: sum(r['ms_per_step'] * r['steps'] for r in v) / sum(r['steps'] for r in v) for k, v in rows.items()}
    line = {'what': 'checkpoint every k-th replay of a captured C_NETWORK step', 'shape': [a.batch, 256, a.frames], 'every': a.every,
            'step_ms': {k: round(v, 4) for k, v in mean.items()}, 'windows': rows, 'tensors': table.n,
            'bytes_per_checkpoint': nbytes, 'snapshot_launch_us': round(snap_ms * 1e3, 2),
            'snapshot_GBps': round(2 * nbytes / (snap_ms * 1e-3) / 1e9, 1),
            'copy_per_tensor_us': round(copy_ms * 1e3, 2), 'copy_launches': table.n, 'rejected': rejected,
            'device': torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text)
    with open(os.path.join(ROOT, 'profiles', 'checkpoint_bench.json'), 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
