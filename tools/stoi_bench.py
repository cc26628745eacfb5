"""Batched device STOI (metrics.stoi_batch, csrc/stoi.hip) against the host loop of network_functions.calc_metric
(metrics.stoi per utterance after a .cpu().numpy() copy each), at the validation shape (B = 32, L = 8160, 16 kHz) and at
B = 4 utterances of 4 s.  Prints one JSON line: per shape the device time (median of event-timed runs after warm-up), the
host loop's time on the same inputs and max |device - host|.  usage: python tools/stoi_bench.py [--runs 50]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'dcs-net_amd'))
from dcsnet import metrics  # noqa: E402


def _signals(B, L, fs, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(L) / fs
    clean = np.zeros((B, L), np.float32)
    for i in range(B):
        f0 = rng.uniform(100, 220)
        s = sum(np.sin(2 * np.pi * k * f0 * t + rng.uniform(0, 6.3)) / k for k in range(1, 9))
        s = s + 0.03 * np.std(s) * rng.standard_normal(L)                     # broadband part, 30 dB down
        env = 0.6 + 0.4 * np.sin(2 * np.pi * rng.uniform(3, 6) * t)
        clean[i] = s * env
    noise = rng.standard_normal((B, L)) * (np.linalg.norm(clean, axis=1, keepdims=True) / np.sqrt(L))
    snr = np.linspace(-10, 30, B)[:, None]
    return clean, (clean + noise * 10 ** (-snr / 20)).astype(np.float32)


def measure(B, L, fs, runs, dev):
    clean, est = _signals(B, L, fs, B * L)
    c, e = torch.from_numpy(clean).to(dev), torch.from_numpy(est).to(dev)
    for _ in range(5):
        d = metrics.stoi_batch(c, e, fs)
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        d = metrics.stoi_batch(c, e, fs)
        t.record()
        t.synchronize()
        times.append(s.elapsed_time(t) * 1e3)
    metrics.stoi(clean[0], est[0], fs)                                       # host warm-up (imports, caches)
    t0 = time.perf_counter()
    host = [metrics.stoi(c[i].cpu().numpy(), e[i].cpu().numpy(), fs) for i in range(B)]
    host_s = time.perf_counter() - t0
    dev_us = float(np.median(times))
    return {'B': B, 'L': L, 'fs': fs, 'device_us_median': round(dev_us, 2), 'device_us_min': round(float(np.min(times)), 2),
            'host_loop_ms': round(host_s * 1e3, 2), 'speedup': round(host_s * 1e6 / dev_us, 1),
            'max_abs_diff': float(np.max(np.abs(d.cpu().numpy() - np.array(host)))), 'runs': runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=50)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = [measure(32, 8160, 16000, max(a.runs, 20), dev), measure(4, 64000, 16000, max(a.runs, 20), dev)]
    print(json.dumps({'metric': 'stoi_batch', 'device': torch.cuda.get_device_name(0), 'shapes': res}))


if __name__ == '__main__':
    main()
