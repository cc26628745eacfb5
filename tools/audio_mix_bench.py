"""The mixing batch (MixingAudioStore.batch_device -> ops.audio_mix_stft_batch, csrc/audio_mix.hip) against the paired batch
(ops.audio_stft_batch) on the store materialise() makes with the SAME draws, at B = 32, T = 256: the two kernels share their
frame / FFT / store sequence (csrc/audio_batch_common.h) and differ in where the noisy sample comes from — one load from the
noisy store, or one load from the noise store, a wrapped index, a multiplication and an addition.

Both run in one process.  Each is captured as a graph of --launches back-to-back launches (so the host's launch cost does not
bound the rate); the graphs are replayed in alternating event-timed windows of at least --window-s seconds each, and the
medians over the windows are reported per launch, with their ratio.  The outputs are compared with torch.equal first.
Synthetic audio from seeds: 64 clean recordings of 1 to 4 s and 8 noise recordings of 0.25 to 10 s at config.sr.

usage: python tools/audio_mix_bench.py [--out profiles/audio_mix.json]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'dcs-net_amd'))
from dcsnet.audio_store import MixingAudioStore  # noqa: E402
from dcsnet.config import config  # noqa: E402


def _stores(dev, seed=0):
    rng = np.random.default_rng(seed)
    sr = int(config.file_sr)
    clean = [(0.1 * rng.standard_normal(int(sec * sr))).astype(np.float32) for sec in rng.uniform(1.0, 4.0, 64)]
    noise = [(0.1 * rng.standard_normal(int(sec * sr))).astype(np.float32) for sec in (0.25, 0.5, 1, 2, 3, 5, 8, 10)]
    mixing = MixingAudioStore(clean, noise, config, dev)
    return mixing, mixing.materialise(generator=torch.Generator().manual_seed(seed)), mixing.last_draws


def _graph(fn, launches):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    return g


def _window(graph, replays):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(replays):
        graph.replay()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e-3                            # seconds


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'audio_mix.json'))
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--launches', type=int, default=200, help='launches per captured graph')
    ap.add_argument('--windows', type=int, default=5, help='timed windows per kernel')
    ap.add_argument('--window-s', type=float, default=1.0, help='minimum length of a window')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    mixing, fixed, draws = _stores(dev)
    B, T = a.batch, mixing.T
    idx = list(range(B))
    starts = mixing.draw_starts(idx, torch.Generator().manual_seed(1))

    def i32(v):
        return torch.tensor(v, dtype=torch.int32, device=dev)
    index, start = i32(idx), i32(starts)
    nidx, nstart = i32(draws['noise_index'][:B]), i32(draws['noise_start'][:B])
    gain = torch.from_numpy(np.asarray(draws['gain'][:B], dtype=np.float32)).to(dev)
    out_mix = tuple(torch.empty((B, 256, T), dtype=torch.complex64, device=dev) for _ in range(3))
    out_pair = tuple(torch.empty((B, 256, T), dtype=torch.complex64, device=dev) for _ in range(3))

    def mix():
        return mixing.batch_device(index, start, nidx, nstart, gain, out=out_mix)

    def pair():
        return fixed.batch_device(index, start, out=out_pair)
    mix(), pair()
    equal = all(torch.equal(x, y) for x, y in zip(out_mix, out_pair))
    graphs = {'mix': _graph(mix, a.launches), 'paired': _graph(pair, a.launches)}
    replays = {}
    for name, g in graphs.items():                             # size the windows from a short trial
        _window(g, 5)
        replays[name] = max(1, math.ceil(1.05 * a.window_s / (_window(g, 20) / 20)))
    times = {name: [] for name in graphs}
    for _ in range(a.windows):
        for name, g in graphs.items():                         # alternating
            seconds = _window(g, replays[name])
            while seconds < a.window_s:                        # (a window that came out short is taken again, longer)
                replays[name] = math.ceil(replays[name] * 1.2 * a.window_s / seconds)
                seconds = _window(g, replays[name])
            times[name].append(seconds / (replays[name] * a.launches) * 1e6)
    med = {name: float(np.median(v)) for name, v in times.items()}
    L = mixing.crop_length
    res = {'metric': 'audio_mix_stft_batch', 'device': torch.cuda.get_device_name(0), 'B': B, 'T': T, 'L': L,
           'bit_identical_to_paired_on_materialised_store': equal, 'launches_per_graph': a.launches, 'windows': a.windows,
           'window_s_min': a.window_s,
           'mix_us_median': round(med['mix'], 3), 'paired_us_median': round(med['paired'], 3),
           'mix_us_windows': [round(v, 3) for v in times['mix']], 'paired_us_windows': [round(v, 3) for v in times['paired']],
           'ratio_mix_over_paired': round(med['mix'] / med['paired'], 4),
           'bytes_written': 3 * B * 256 * T * 8, 'bytes_read_per_signal': B * L * 4}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
