"""The ITU-T P.56 active-speech-level pass over a set of recordings on the device (ops.active_level_ragged,
csrc/speech_level.hip) against the host function metrics.active_speech_level on the same set, with the whole-recording power
pass (ops.signal_power_ragged) beside it: what MixingAudioStore(level='p56') pays once per store.

The set is tools/score_bench.py's: --recordings seeded synthetic signals, lengths spread uniformly over 1 to 10 s at 16 kHz.
Timing: device events around one call over the whole set; the two device passes alternate in three rounds, in each of which a
pass repeats until it has filled its third of --min-seconds, after a warm-up call of each; medians over the calls.  The host
function: the wall clock of one loop over the set, signals already on the host.  No target is set for this time.

usage: python tools/level_bench.py [--out profiles/active_level_bench.json] [--recordings 32]"""
import argparse
import importlib.util
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'dcs-net_amd'))
from dcsnet import metrics, ops  # noqa: E402


def _score_bench():
    spec = importlib.util.spec_from_file_location('dcs_tools_score_bench', os.path.join(ROOT, 'tools', 'score_bench.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'active_level_bench.json'), help='- for none')
    ap.add_argument('--recordings', type=int, default=32)
    ap.add_argument('--min-seconds', type=float, default=1.0)
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('level_bench: needs the GPU; a time taken elsewhere says nothing about it')
    sb = _score_bench()
    dev = torch.device('cuda:0')
    fs, n = 16000, a.recordings
    clean, _ = sb.synthetic_set(n, a.seed, fs)
    off_h = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(c) for c in clean], out=off_h[1:])
    x = torch.from_numpy(np.concatenate(clean)).to(dev)
    off = torch.from_numpy(off_h).to(dev)
    methods = (('signal_power_ragged_call', lambda: ops.signal_power_ragged(x, off)),
               ('active_level_ragged_call', lambda: ops.active_level_ragged(x, off, fs, return_counts=True)))
    first = {}
    for name, fn in methods:
        first[name] = fn()
        torch.cuda.synchronize()
    times = sb.timed_rounds(methods, a.min_seconds)
    t0 = time.perf_counter()
    host = [metrics.active_speech_level(c, fs) for c in clean]
    host_s = time.perf_counter() - t0
    level, counts = (t.cpu().numpy() for t in first['active_level_ragged_call'])
    want = np.array([[h['active_power'], h['activity']] for h in host])
    power = first['signal_power_ragged_call'].cpu().numpy()
    res = {'metric': 'active_level_recordings', 'device': torch.cuda.get_device_name(0), 'recordings': n,
           'audio_seconds': round(float(off_h[-1]) / fs, 2), 'lengths_s': '1 .. 10 s at 16 kHz, uniform, seeded',
           'first_measurement': 'no earlier figure exists for this pass on the MI355X and nothing at the parent commit compares',
           'timing': 'device events around one call over the set; the two device passes alternate in 3 rounds, each filling a '
                     'third of min_seconds with repeated calls; median over the calls.  host: wall clock of one loop of '
                     'metrics.active_speech_level over the set (numpy / scipy, fp64), signals already on the host',
           'min_seconds': a.min_seconds, 'kernel_launches': {'active_level_ragged_call': 1, 'signal_power_ragged_call': 1},
           'tile_samples': ops.ACTIVE_LEVEL_TILE, 'host_loop_s': round(host_s, 4),
           'counts_equal_host': bool(np.array_equal(counts, np.array([h['counts'] for h in host]))),
           'level_max_rel_diff_vs_host': float(np.nanmax(np.abs(level / want - 1.0))),
           'nan_levels': int(np.isnan(level[:, 0]).sum()), 'nan_levels_host': int(np.isnan(want[:, 0]).sum()),
           'active_over_mean_power_db': {'min': round(float(np.nanmin(10 * np.log10(level[:, 0] / power))), 3),
                                         'max': round(float(np.nanmax(10 * np.log10(level[:, 0] / power))), 3)}}
    for name, _ in methods:
        res[name] = sb.pass_stats(times[name], n)
    ms = res['active_level_ragged_call']['ms_per_pass_median']
    res['audio_seconds_per_device_second'] = round(res['audio_seconds'] / (ms / 1e3), 1)
    res['active_level_over_signal_power_pass'] = round(ms / res['signal_power_ragged_call']['ms_per_pass_median'], 3)
    res['host_loop_over_device_pass'] = round(host_s * 1e3 / ms, 1)
    sb.write_result(res, a.out)


if __name__ == '__main__':
    main()
