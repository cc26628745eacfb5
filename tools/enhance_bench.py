"""Whole-recording enhancement (dcsnet/enhance.py): recordings per second and real-time factor of the Enhancer, captured and
eager, against the loop that was possible before it — per recording, the STFT of the whole signal (frontend.stft_batch), the
network at B = 1 at that recording's own number of frames, the fused bound + mask application, polar_wave; all eager, since
no graph survives a shape change.  All three start from the same host waveforms at 48 kHz (upload and resampling included)
and end with device waveforms at config.sr.

The set is synthetic and seeded: --recordings lengths spread uniformly over 1 to 10 s at 48 kHz.  Timing: device events around
one pass over the whole set, the three methods alternating, at least --min-seconds of each after a warm-up pass of each.

usage: python tools/enhance_bench.py [--out profiles/enhance_bench.json] [--dtype f32|bf16] [--recordings 32]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'dcs-net_amd'))
from dcsnet import functional as F, ops  # noqa: E402
from dcsnet.c_network import C_NETWORK  # noqa: E402
from dcsnet.config import config, hparams  # noqa: E402
from dcsnet.enhance import Enhancer  # noqa: E402
from dcsnet.frontend import stft_batch  # noqa: E402
from dcsnet.network_functions import _polar_wave  # noqa: E402


def synthetic_set(n, seed, rate=48000):
    g = torch.Generator().manual_seed(seed)
    lengths = torch.linspace(1.0, 10.0, n)[torch.randperm(n, generator=g)]
    return [(0.1 * torch.randn(int(round(float(s) * rate)), generator=g)).numpy() for s in lengths]


def per_recording_loop(net, waves, rate, dev):
    """One recording at a time at its own T (rounded up to the network's multiple of 8, the tail zero)."""
    hop, eps = config.hop_length, hparams['atan2_eps']
    out = []
    with torch.no_grad():
        for x in waves:
            y = ops.resample_sinc(torch.from_numpy(x).to(dev), rate, config.sr)
            n = y.numel()
            T = -(-(n // hop + 1) // 8) * 8
            y = torch.nn.functional.pad(y, (0, hop * (T - 1) - n))[None]
            _, noisy, _ = stft_batch(y, y, config)
            d = net(noisy, bound=False).reshape(noisy.shape)
            _, _, speech = F.bound2_mask_apply_complex(noisy, d, eps)
            out.append(_polar_wave(speech, eps, config)[0, :n])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'enhance_bench.json'))
    ap.add_argument('--dtype', default='f32', choices=['f32', 'bf16'])
    ap.add_argument('--recordings', type=int, default=32)
    ap.add_argument('--segment-frames', type=int, default=2000)
    ap.add_argument('--overlap-frames', type=int, default=300)
    ap.add_argument('--batch-segments', type=int, default=16)
    ap.add_argument('--min-seconds', type=float, default=1.0)
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    rate = 48000
    waves = synthetic_set(a.recordings, a.seed, rate)
    audio_s = sum(len(w) for w in waves) / rate
    torch.manual_seed(0)
    net = C_NETWORK(config, hparams, 0).to(dev).eval()
    if a.dtype == 'bf16':
        net.set_activation_dtype('bf16')
    kw = dict(mode='dcs', segment_frames=a.segment_frames, overlap_frames=a.overlap_frames, batch_segments=a.batch_segments)
    captured, eager = Enhancer(net, use_graph=True, **kw), Enhancer(net, use_graph=False, **kw)
    methods = (('enhancer_captured', lambda: captured(waves, rate)), ('enhancer_eager', lambda: eager(waves, rate)),
               ('per_recording_eager', lambda: per_recording_loop(net, waves, rate, dev)))
    first = {}
    for name, fn in methods:                                 # warm-up: every shape, the capture, the weight packs
        first[name] = fn()
        torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in zip(first['enhancer_captured'], first['enhancer_eager']))
    times = {name: [] for name, _ in methods}
    while min(sum(v) for v in times.values()) < a.min_seconds or len(times['enhancer_captured']) < 3:
        for name, fn in methods:                             # alternating windows: one pass over the set each
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) / 1e3)
    from dcsnet.enhance import SegmentPlan
    plan = SegmentPlan([ops.resample_sinc_length(len(w), rate, config.sr) for w in waves], a.segment_frames, a.overlap_frames,
                       config.hop_length, a.batch_segments)
    res = {'metric': 'enhance_recordings', 'device': torch.cuda.get_device_name(0), 'dtype': a.dtype,
           'conv_precision': ops.conv_precision(), 'recordings': a.recordings, 'audio_seconds': round(audio_s, 2),
           'lengths_s': '1 .. 10 s at 48 kHz, uniform, seeded', 'segment_frames': a.segment_frames,
           'overlap_frames': a.overlap_frames, 'batch_segments': a.batch_segments, 'segments': plan.rows,
           'batches': plan.batches, 'captured_equals_eager': bool(same),
           'timing': 'device events around one pass over the set (host upload, resampling, planning included), methods '
                     'alternating, median over the passes'}
    for name, _ in methods:
        med = float(np.median(times[name]))
        res[name] = {'passes': len(times[name]), 'timed_s': round(sum(times[name]), 2), 's_per_pass_median': round(med, 4),
                     's_per_pass_min': round(min(times[name]), 4), 'recordings_per_s': round(a.recordings / med, 1),
                     'real_time_factor': round(med / audio_s, 5), 'times_real_time': round(audio_s / med, 1)}
    res['speedup_captured_vs_per_recording'] = round(res['per_recording_eager']['s_per_pass_median'] /
                                                     res['enhancer_captured']['s_per_pass_median'], 2)
    res['speedup_captured_vs_eager'] = round(res['enhancer_eager']['s_per_pass_median'] /
                                             res['enhancer_captured']['s_per_pass_median'], 2)
    print(json.dumps(res))
    if a.out != '-':
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
