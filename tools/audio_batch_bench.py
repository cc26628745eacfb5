"""The fused batch op of the resident audio store (ops.audio_stft_batch, csrc/audio_store.hip) against frontend.stft_batch on the
same pre-cropped device waveforms (B items of exactly L = hop (T - 1) samples, start 0), at B = 32 and 64, T = 256.  The two
are timed in the same process, alternating, with events around windows of back-to-back launches after warm-up (at least 1 s
of each per shape); the outputs are compared with torch.equal.  Bytes each op must move over its time, against the 6.3 TB/s
a streaming copy achieves.  Also the host path the reference's loader workers run, for reference (HOST numbers): the sinc
resampler as one fp32 conv1d of a 3 s 48 kHz utterance (the way torchaudio runs it) and the crop + three torch.stft calls of
one item, per item with clean and noisy resampled, on 1 and 4 torch threads.

usage: python tools/audio_batch_bench.py [--out profiles/audio_batch.json]
       python tools/audio_batch_bench.py --profile-run          (a few launches of each, for rocprofv3 --kernel-trace --stats)
       python tools/audio_batch_bench.py --kernel-stats CSV     (adds the kernel rows of that stats file to --out)"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'dcs-net_amd'))
from dcsnet import ops  # noqa: E402
from dcsnet.config import config  # noqa: E402
from dcsnet.frontend import stft_batch  # noqa: E402
from dcsnet.network_functions import _window_on  # noqa: E402

HBM_STREAM = 6.3e12                                       # achievable streaming-copy rate (peak 8 TB/s)


def _host_items_per_s(threads, items=200):
    torch.set_num_threads(threads)
    g = torch.Generator().manual_seed(0)
    h = torch.from_numpy(ops.sinc_resample_taps(48000, 16000).astype(np.float32))[:, None, :]     # [1, 1, 41]
    x48 = 0.1 * torch.randn(2, 3 * 48000, generator=g)
    w = config.window
    L = config.integer_win_size - config.hop_length

    def one():
        y = torch.nn.functional.conv1d(torch.nn.functional.pad(x48[:, None], (19, 19 + 3)), h, stride=3)[:, 0, :48000]
        s = int(torch.randint(0, y.shape[1] - L, (1,), generator=g))
        c, n = y[0, s:s + L], y[1, s:s + L]
        return [torch.stft(v, 512, 32, 512, w, return_complex=True, normalized=True)[1:257] for v in (c, n - c, n)]

    for _ in range(10):
        one()
    t0 = time.perf_counter()
    for _ in range(items):
        one()
    dt = time.perf_counter() - t0
    t0 = time.perf_counter()
    for _ in range(items):
        torch.nn.functional.conv1d(torch.nn.functional.pad(x48[:1, None], (19, 22)), h, stride=3)
    rs = time.perf_counter() - t0
    return {'torch_threads': threads, 'items_per_s': round(items / dt, 1), 'ms_per_item': round(dt / items * 1e3, 3),
            'resample_3s_utterance_ms': round(rs / items * 1e3, 3)}


def _setup(B, T, dev, seed):
    hop = config.hop_length
    L = hop * (T - 1)
    g = torch.Generator().manual_seed(seed)
    clean = 0.1 * torch.randn(B, L, generator=g)
    noisy = clean + 0.05 * torch.randn(B, L, generator=g)
    clean, noisy = clean.to(dev), noisy.to(dev)
    off = (torch.arange(B + 1, dtype=torch.int64) * L).to(dev)
    idx = torch.arange(B, dtype=torch.int32, device=dev)
    starts = torch.zeros(B, dtype=torch.int32, device=dev)
    out = tuple(torch.empty((B, 256, T), dtype=torch.complex64, device=dev) for _ in range(3))
    w = _window_on(config, dev)

    def fused():
        return ops.audio_stft_batch(clean.view(-1), noisy.view(-1), off, idx, starts, w, T, hop, 512 ** -0.5, out=out)

    def three():
        return stft_batch(clean, noisy, config)
    return fused, three, L


def _bytes(B, T, L):
    spec = 3 * B * 256 * T * 8                             # the three complex64 [B, 256, T] outputs
    wave = 2 * B * L * 4                                   # clean and noisy read
    frames = 3 * B * T * 512 * 4                           # stft_batch: frames written, read by the FFT
    full = 3 * B * T * 257 * 8                             # stft_batch: 257-bin spectra written, read by the bins kernel
    return {'fused': spec + wave, 'stft_batch': wave + 2 * frames + 2 * full + spec}


def measure(B, T, dev, min_window_s=1.0):
    fused, three, L = _setup(B, T, dev, B)
    a, b = fused(), three()
    equal = all(torch.equal(x, y) for x, y in zip(a, b))
    for _ in range(20):
        fused(); three()
    torch.cuda.synchronize()
    n = 50
    times = {'fused': [], 'stft_batch': []}
    total = {'fused': 0.0, 'stft_batch': 0.0}
    while min(total.values()) < min_window_s or len(times['fused']) < 10:
        for name, fn in (('fused', fused), ('stft_batch', three)):         # alternating windows of n back-to-back calls
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(n):
                fn()
            e.record()
            e.synchronize()
            ms = s.elapsed_time(e)
            times[name].append(ms * 1e3 / n)
            total[name] += ms / 1e3
    nbytes = _bytes(B, T, L)
    res = {'B': B, 'T': T, 'L': L, 'bit_identical': equal, 'windows': len(times['fused']), 'calls_per_window': n}
    for name in ('fused', 'stft_batch'):
        med = float(np.median(times[name]))
        res[name] = {'us_per_batch_median': round(med, 2), 'us_per_batch_min': round(float(np.min(times[name])), 2),
                     'timed_s': round(total[name], 2), 'bytes_moved': nbytes[name],
                     'TBps_at_median': round(nbytes[name] / (med * 1e-6) / 1e12, 3),
                     'fraction_of_6.3TBps': round(nbytes[name] / (med * 1e-6) / HBM_STREAM, 3)}
    res['speedup_median'] = round(res['stft_batch']['us_per_batch_median'] / res['fused']['us_per_batch_median'], 3)
    return res


def kernel_rows(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append({'name': r['Name'][:120], 'calls': int(r['Calls']), 'total_us': round(float(r['TotalDurationNs']) / 1e3, 1),
                         'avg_us': round(float(r['AverageNs']) / 1e3, 2), 'min_us': round(float(r['MinNs']) / 1e3, 2)})
    return rows


def per_batch_kernel_times(trace_path):
    """Median kernel time per op and batch size from the kernel trace of --profile-run (B = 32 launches first, then B = 64):
    the fused kernel alone, and stft_batch's three kernels summed."""
    ks = {}
    with open(trace_path) as f:
        for r in csv.DictReader(f):
            name = r['Kernel_Name']
            key = next((k for k in ('audio_stft_batch_kernel', 'stft_frames_kernel', 'rfft512_kernel', 'stft_bins_kernel')
                        if k in name), None)
            if key:
                ks.setdefault(key, []).append((int(r['Start_Timestamp']), int(r['End_Timestamp']) - int(r['Start_Timestamp'])))
    out = {}
    for k, v in ks.items():
        v.sort()
        half = len(v) // 2
        out[k] = {'B32_median_us': round(float(np.median([d for _, d in v[:half]])) / 1e3, 2),
                  'B64_median_us': round(float(np.median([d for _, d in v[half:]])) / 1e3, 2)}
    three = [k for k in ('stft_frames_kernel', 'rfft512_kernel', 'stft_bins_kernel') if k in out]
    if len(three) == 3:
        out['stft_batch_three_kernels'] = {f'B{b}_median_us': round(sum(out[k][f'B{b}_median_us'] for k in three), 2)
                                           for b in (32, 64)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'audio_batch.json'))
    ap.add_argument('--profile-run', action='store_true')
    ap.add_argument('--kernel-stats')
    a = ap.parse_args()
    if a.kernel_stats:
        res = json.load(open(a.out))
        res['kernel_stats'] = {'source': 'rocprofv3 --kernel-trace --stats -- python tools/audio_batch_bench.py --profile-run '
                                         '(20 calls of each op at B = 32, then at B = 64)',
                               'rows': kernel_rows(a.kernel_stats)}
        trace = a.kernel_stats.replace('kernel_stats.csv', 'kernel_trace.csv')
        if os.path.exists(trace):
            res['kernel_stats']['per_batch_size'] = per_batch_kernel_times(trace)
            for sh in res['shapes']:
                kt = res['kernel_stats']['per_batch_size']
                t = kt['audio_stft_batch_kernel'][f"B{sh['B']}_median_us"]
                sh['fused']['kernel_us_rocprof'] = t
                sh['fused']['fraction_of_6.3TBps_kernel'] = round(sh['fused']['bytes_moved'] / (t * 1e-6) / HBM_STREAM, 3)
                if 'stft_batch_three_kernels' in kt:
                    sh['stft_batch']['kernel_us_rocprof'] = kt['stft_batch_three_kernels'][f"B{sh['B']}_median_us"]
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
        return
    if a.profile_run:
        dev = torch.device('cuda:0')
        for B in (32, 64):
            fused, three, _ = _setup(B, 256, dev, B)
            for _ in range(20):
                fused(); three()
        torch.cuda.synchronize()
        return
    host = [_host_items_per_s(1), _host_items_per_s(4)]              # before the GPU is touched
    dev = torch.device('cuda:0')
    res = {'metric': 'audio_stft_batch', 'device': torch.cuda.get_device_name(0),
           'frames_per_workgroup': int(os.environ.get('DCS_AUDIO_FRAMES_PER_WG', '8')),
           'shapes': [measure(32, 256, dev), measure(64, 256, dev)],
           'host_reference': {'note': 'HOST numbers (CPU of the GPU machine): sinc resample of clean and noisy (3 s, 48 kHz, one '
                                      'fp32 conv1d each), crop, three torch.stft per item', 'runs': host}}
    print(json.dumps(res))
    if a.out != '-':
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
