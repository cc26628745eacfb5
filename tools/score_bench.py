"""Scoring a set of recordings of different lengths (metrics.stoi_ragged, csrc/stoi_ragged.hip) against the two loops that were
possible before it: per recording one metrics.stoi_batch([1, L]) call, and per recording a copy to the host and metrics.stoi
there.  All three start from the same flat device buffers at 16 kHz (what the Enhancer leaves) and end with the per-recording
scores on the device (the host loop: in a list).

The set is synthetic and seeded: --recordings lengths spread uniformly over 1 to 10 s.  Timing: device events around one pass
over the whole set; the three methods alternate in three rounds, in each of which a method repeats its pass until it has
filled its third of --min-seconds (at least 1 s of every method, after a warm-up pass of each); medians over the passes.
Launch counts are the kernels each method issues per pass (from the entry points' definitions, include/dcsnet_hip.h).

--extended times a fourth method beside them, alternating in the same rounds: the ragged call with extended='both' (STOI and
ESTOI from one pass of the resampling, keep and band kernels), and records its cost relative to the STOI-only ragged call.
--parent-json takes the JSON this tool printed on another commit in the same session and records that commit's ragged pass.

--frame-measures times another question instead: the device pass of metrics.frame_measures_ragged (segmental SNR, LLR, cepstrum
distance; csrc/frame_measures.hip) on the same seeded set beside the STOI pass, the two alternating in the same rounds, plus
the wall-clock time of the host function metrics.frame_measures over the set and the largest device - host differences ->
profiles/frame_measures_bench.json.

--spectral-measures does the same for metrics.spectral_measures_ragged (WSS, frequency-weighted segmental SNR;
csrc/spectral_measures.hip): its device pass beside the STOI pass and the frame-measures pass, the three alternating in the same
rounds, the host function metrics.spectral_measures and the largest differences -> profiles/spectral_measures_bench.json.

--sdr does the same for metrics.sdr_ragged (the BSS-eval signal-to-distortion ratio, 512 taps; csrc/sdr_ragged.hip): its device
pass with one estimate and with two estimates in one call beside the STOI pass, the three alternating in the same rounds, the
host function metrics.sdr and the largest difference -> profiles/sdr_bench.json.  --kernel-stats FILE folds in the kernel times
of a rocprofv3 --kernel-trace --stats run of this tool (taken in a run of its own): the share of the solve launch.

usage: python tools/score_bench.py [--out profiles/score_bench.json] [--recordings 32] [--extended] [--parent-json FILE]
       python tools/score_bench.py --frame-measures [--out profiles/frame_measures_bench.json] [--recordings 32]
       python tools/score_bench.py --spectral-measures [--out profiles/spectral_measures_bench.json] [--recordings 32]
       python tools/score_bench.py --sdr [--out profiles/sdr_bench.json] [--recordings 32] [--kernel-stats FILE]"""
import argparse
import csv
import json
import os
import re
import sys
import time
from typing import Callable, NamedTuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'dcs-net_amd'))
from dcsnet import metrics, ops  # noqa: E402


def synthetic_set(n, seed, rate=16000):
    """Harmonic 'speech' under a syllable-rate envelope with a broadband part 30 dB down, and a noisy copy at -5 .. 20 dB."""
    rng = np.random.default_rng(seed)
    seconds = np.linspace(1.0, 10.0, n)[rng.permutation(n)]
    clean, est = [], []
    for i, s in enumerate(seconds):
        L = int(round(s * rate))
        t = np.arange(L) / rate
        f0 = rng.uniform(100, 220)
        x = sum(np.sin(2 * np.pi * k * f0 * t + rng.uniform(0, 6.3)) / k for k in range(1, 9))
        x = (x + 0.03 * np.std(x) * rng.standard_normal(L)) * (0.6 + 0.4 * np.sin(2 * np.pi * rng.uniform(3, 6) * t))
        noise = rng.standard_normal(L) * (np.linalg.norm(x) / np.sqrt(L)) * 10 ** (-np.linspace(-5, 20, n)[i] / 20)
        clean.append((0.1 * x).astype(np.float32))
        est.append((0.1 * (x + noise)).astype(np.float32))
    return clean, est


def timed_rounds(methods, min_seconds, rounds=3):
    """{name: [seconds per pass]}: the methods alternate in rounds; in each a method repeats its pass (each pass timed by its own
    event pair) until it has filled its share of min_seconds."""
    times = {name: [] for name, _ in methods}
    for r in range(rounds):
        for name, fn in methods:
            spent = 0.0
            while spent < min_seconds / rounds:
                s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                fn()
                t.record()
                t.synchronize()
                times[name].append(s.elapsed_time(t) / 1e3)
                spent += times[name][-1]
        print(f'[score_bench] round {r + 1} of {rounds} done', file=sys.stderr, flush=True)
    return times


def pass_stats(times, n):
    med = float(np.median(times))
    return {'passes': len(times), 'timed_s': round(sum(times), 2), 'ms_per_pass_median': round(med * 1e3, 3),
            'ms_per_pass_min': round(min(times) * 1e3, 3), 'recordings_per_s': round(n / med, 1)}


FP64_VECTOR_PEAK = 78.6e12      # FLOP/s: half the FP32 vector peak of MI355X_MICROARCH (157.3 TFLOPS), AMD's published fp64 figure


class Mode(NamedTuple):
    """What --frame-measures, --spectral-measures or --sdr times beside the STOI pass and holds against the host.  name: the flag's
    attribute; the metric is '<name>_recordings', the mode's own device pass '<name>_ragged_call'.  out: the default output file
    under profiles/.  host: (x, y, fs) -> {key: float} of one recording.  keys: what is compared with the host.  methods:
    (c, e, off, fs, longest) -> ((pass name, function), ...), timed behind the STOI pass in this order.  launches: kernels per pass
    of those.  fields: (n, total, spans, fs) -> the mode's geometry and workspace.  notes: its note strings.  more: (res, first,
    a, total) -> the fields only this mode has, from the result so far and the warm-up's values."""
    name: str
    out: str
    host: Callable
    keys: tuple
    methods: Callable
    launches: dict
    fields: Callable
    notes: dict = {}
    more: Callable = lambda res, first, a, total: {}


def _frames(spans, fs):
    return int(sum(metrics.frame_count(q - p, fs) for p, q in spans))


def _frame_fields(n, total, spans, fs):
    N, S, P = metrics.frame_geometry(fs)
    return {'frames': _frames(spans, fs), 'frame': {'N': N, 'S': S, 'lpc_order': P},
            'workspace_bytes': int(ops.frame_measures_workspace_bytes(n, total, fs))}


def _spectral_fields(n, total, spans, fs):
    N, S, _ = metrics.frame_geometry(fs)
    nfft = metrics.spectral_fft_size(fs)
    return {'frames': _frames(spans, fs), 'frame': {'N': N, 'S': S, 'nfft': nfft},
            'workspace_bytes': int(ops.spectral_measures_workspace_bytes(n, total, fs)), 'frame_kernel_lds_bytes_derived': 16 * nfft}


def _spectral_more(res, first, a, total):
    return {'spectral_measures_over_frame_measures_pass': round(res['spectral_measures_ragged_call']['ms_per_pass_median'] /
                                                                res['frame_measures_ragged_call']['ms_per_pass_median'], 3)}


def _sdr_methods(c, e, off, fs, longest):
    e2 = (c + 0.5 * (e - c)).contiguous()                     # a second estimate: the same noise 6 dB down
    return (('sdr_ragged_call', lambda: metrics.sdr_ragged(c, e, off)),
            ('sdr_ragged_two_estimates_call', lambda: metrics.sdr_ragged(c, e, off, estimate2=e2)))


def _sdr_fields(n, total, spans, fs):
    K = metrics.SDR_FILTER_LENGTH
    return {'filter_length': K, 'chunk': ops.SDR_CHUNK, 'chunks': int(sum(-(-(q - p + K - 1) // ops.SDR_CHUNK) for p, q in spans)),
            'workspace_bytes': int(ops.sdr_workspace_bytes(n, total, K))}


def sdr_kernel_times(path):
    """{'one_estimate' | 'two_estimates': {pass: mean microseconds per launch}} of the sdr_<pass>_kernel<...> rows of a rocprofv3
    kernel-stats CSV (the last template argument is the number of estimates; of signals, one more, for the corr pass)."""
    out = {'one_estimate': {}, 'two_estimates': {}}
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            m = re.search(r'sdr_(\w+)_kernel<([\d, ]+)>', row.get('Name') or row.get('KernelName') or '')
            if not m:
                continue
            estimates = int(m.group(2).split(',')[-1]) - (m.group(1) == 'corr')
            out['one_estimate' if estimates == 1 else 'two_estimates'][m.group(1)] = round(
                float(row['TotalDurationNs']) / float(row['Calls']) / 1e3, 2)
    return out


def _sdr_more(res, first, a, total):
    K = metrics.SDR_FILTER_LENGTH
    one, two = res['sdr_ragged_call']['ms_per_pass_median'], res['sdr_ragged_two_estimates_call']['ms_per_pass_median']
    # operations from the shapes: the issue's count of the algorithm (5 K L multiply-adds per recording and estimate), and the
    # multiply-adds the direct form here performs (R, D and the projection: 3 K L; 5 K L with two estimates)
    out = {'two_estimates_over_two_calls': round(two / (2 * one), 3),
           'flops': {'algorithmic_fp64_flop_one_estimate': 2 * 5 * K * total, 'direct_form_fp64_flop_one_estimate': 2 * 3 * K * total,
                     'direct_form_fp64_flop_two_estimates': 2 * 5 * K * total, 'fp64_vector_peak_flops': FP64_VECTOR_PEAK,
                     'peak_source': 'half the FP32 vector peak of the MI355X guide (157.3 TFLOPS); the guide lists no fp64 figure',
                     'algorithmic_share_of_peak_whole_pass': round(2 * 5 * K * total / (one * 1e-3) / FP64_VECTOR_PEAK, 4),
                     'direct_form_share_of_peak_whole_pass': round(2 * 3 * K * total / (one * 1e-3) / FP64_VECTOR_PEAK, 4),
                     'direct_form_share_of_peak_whole_pass_two_estimates':
                         round(2 * 5 * K * total / (two * 1e-3) / FP64_VECTOR_PEAK, 4),
                     'note': 'whole-pass rates over peak (launch gaps and the serial solve included), not a kernel\'s share of peak'},
           'second_estimate_equals_its_own_call': bool(torch.equal(first['sdr_ragged_two_estimates_call'][0], first['sdr_ragged_call']))}
    if a.kernel_stats:
        out['kernel_us_rocprofv3'] = sdr_kernel_times(a.kernel_stats)
        for tag, k in out['kernel_us_rocprofv3'].items():
            if len(k) == 4:
                out[f'solve_share_of_kernel_time_{tag}'] = round(k['solve'] / sum(k.values()), 3)
    return out


def _frame_pass(c, e, off, fs, longest):
    return ('frame_measures_ragged_call', lambda: metrics.frame_measures_ragged(c, e, off, fs, longest=longest))


def _spectral_methods(c, e, off, fs, longest):
    return (_frame_pass(c, e, off, fs, longest),
            ('spectral_measures_ragged_call', lambda: metrics.spectral_measures_ragged(c, e, off, fs, longest=longest)))


MODES = (
    Mode(name='frame_measures', out='frame_measures_bench.json', host=metrics.frame_measures, keys=('ssnr', 'llr', 'cd'),
         methods=lambda *buffers: (_frame_pass(*buffers),), launches={'frame_measures_ragged_call': 3}, fields=_frame_fields),
    Mode(name='spectral_measures', out='spectral_measures_bench.json', host=metrics.spectral_measures, keys=('wss', 'fwssnr'),
         methods=_spectral_methods, launches={'spectral_measures_ragged_call': 3, 'frame_measures_ragged_call': 3},
         fields=_spectral_fields, more=_spectral_more,
         notes={'derived': 'frame_kernel_lds_bytes_derived is 16 nfft, what the launch passes as dynamic LDS (the kernel has no '
                           'static LDS), not a reading of the code object',
                'differences': 'this set (harmonic signals) does not meet the input condition of '
                               'tests/test_spectral_measures_device.py (every band slope above 1e-6 dB), and its WSS values are two '
                               'orders larger than that test\'s: the differences below are float32 roundings of those values and '
                               'are not to be read against profiles/spectral_measures_parity.json'}),
    Mode(name='sdr', out='sdr_bench.json', host=lambda x, y, fs: {'sdr': metrics.sdr(x, y)}, keys=('sdr',), methods=_sdr_methods,
         launches={'sdr_ragged_call': ops.SDR_LAUNCHES, 'sdr_ragged_two_estimates_call': ops.SDR_LAUNCHES},
         fields=_sdr_fields, more=_sdr_more,
         notes={'differences': 'this set (harmonic signals, a broadband part 30 dB down) is far worse conditioned than the set of '
                               'tests/test_sdr_device.py; the difference above is not to be read against profiles/sdr_parity.json'}),
)


def measure_bench(mode, a, c, e, off, off_h, longest, fs):
    """The device passes of one mode beside the STOI pass, and its host function on the same set."""
    n, total, own = a.recordings, int(off_h[-1]), f'{mode.name}_ragged_call'
    spans = list(zip(off_h[:-1].tolist(), off_h[1:].tolist()))
    methods = (('stoi_ragged_call', lambda: metrics.stoi_ragged(c, e, off, fs, longest=longest)),) + mode.methods(c, e, off, fs, longest)
    first = {}
    for name, fn in methods:
        first[name] = fn()
        torch.cuda.synchronize()
    times = timed_rounds(methods, a.min_seconds)
    ch, eh = c.cpu().numpy(), e.cpu().numpy()
    t0 = time.perf_counter()
    host = [mode.host(ch[p:q], eh[p:q], fs) for p, q in spans]
    host_s = time.perf_counter() - t0
    res = {'metric': f'{mode.name}_recordings', 'device': torch.cuda.get_device_name(0), 'recordings': n,
           'audio_seconds': round(total / fs, 2), 'lengths_s': '1 .. 10 s at 16 kHz, uniform, seeded',
           'first_measurement': 'no earlier figure exists for this pass on the MI355X and nothing at the parent commit compares',
           'timing': f'device events around one pass over the set; the {("two", "three")[len(methods) - 2]} device methods alternate '
                     'in 3 rounds, each filling a third of min_seconds with repeated passes; median over the passes.  host: wall '
                     f'clock of one loop of metrics.{mode.name} over the set (numpy, fp64), signals already on the host',
           'min_seconds': a.min_seconds,
           'kernel_launches': dict(mode.launches, stoi_ragged_call=2 * 2 + 4, stoi_ragged_call_fills=2),
           **mode.fields(n, total, spans, fs), 'host_loop_s': round(host_s, 4), **mode.notes}
    for name, _ in methods:
        res[name] = pass_stats(times[name], n)
    ms = res[own]['ms_per_pass_median']
    res[f'{mode.name}_over_stoi_pass'] = round(ms / res['stoi_ragged_call']['ms_per_pass_median'], 3)
    res['host_loop_over_device_pass'] = round(host_s * 1e3 / ms, 1)
    got = first[own] if isinstance(first[own], dict) else {mode.keys[0]: first[own]}
    for k in mode.keys:
        res[f'{k}_max_abs_diff_vs_host'] = float(np.nanmax(np.abs(got[k].cpu().numpy() - np.array([m[k] for m in host]))))
    res.update(mode.more(res, first, a, total))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='default: profiles/score_bench.json (--frame-measures: '
                                                'profiles/frame_measures_bench.json, --spectral-measures: '
                                                'profiles/spectral_measures_bench.json, --sdr: profiles/sdr_bench.json); - for none')
    ap.add_argument('--sdr', action='store_true',
                    help='time metrics.sdr_ragged (one and two estimates) beside the STOI pass and the host function instead')
    ap.add_argument('--kernel-stats', default=None, help='--sdr: a rocprofv3 kernel-stats CSV of a run of this tool')
    ap.add_argument('--frame-measures', action='store_true',
                    help='time metrics.frame_measures_ragged beside the STOI pass and the host function instead')
    ap.add_argument('--spectral-measures', action='store_true',
                    help='time metrics.spectral_measures_ragged beside the STOI pass, the frame-measures pass and the host function '
                         'instead')
    ap.add_argument('--recordings', type=int, default=32)
    ap.add_argument('--min-seconds', type=float, default=1.0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--extended', action='store_true', help="time stoi_ragged(extended='both') beside the STOI-only call")
    ap.add_argument('--parent-json', default=None, help="this tool's JSON of the parent commit, same box, same session")
    a = ap.parse_args()
    mode = next((m for m in reversed(MODES) if getattr(a, m.name)), None)       # of several flags, the last of MODES
    if a.out is None:
        a.out = os.path.join(ROOT, 'profiles', mode.out if mode else 'score_bench.json')
    dev = torch.device('cuda:0')
    fs = 16000
    clean, est = synthetic_set(a.recordings, a.seed, fs)
    off_h = np.zeros(a.recordings + 1, dtype=np.int64)
    np.cumsum([len(c) for c in clean], out=off_h[1:])
    c = torch.from_numpy(np.concatenate(clean)).to(dev)
    e = torch.from_numpy(np.concatenate(est)).to(dev)
    off = torch.from_numpy(off_h).to(dev)
    longest = int(np.diff(off_h).max())
    spans = list(zip(off_h[:-1].tolist(), off_h[1:].tolist()))
    if mode:
        return write_result(measure_bench(mode, a, c, e, off, off_h, longest, fs), a.out)

    def ragged():
        return metrics.stoi_ragged(c, e, off, fs, longest=longest)

    def per_recording():
        return torch.cat([metrics.stoi_batch(c[p:q][None], e[p:q][None], fs) for p, q in spans])

    def host_loop():
        return [metrics.stoi(c[p:q].cpu().numpy(), e[p:q].cpu().numpy(), fs) for p, q in spans]

    def ragged_both():
        return metrics.stoi_ragged(c, e, off, fs, longest=longest, extended='both')

    methods = (('ragged_call', ragged), ('per_recording_stoi_batch', per_recording), ('host_loop', host_loop))
    if a.extended:
        methods = methods[:1] + (('ragged_both', ragged_both),) + methods[1:]
    first = {}
    for name, fn in methods:
        first[name] = fn()
        torch.cuda.synchronize()
        print(f'[score_bench] warm-up of {name} done', file=sys.stderr, flush=True)
    # The methods differ by orders of magnitude per pass, so they alternate in ROUNDS (timed_rounds).
    times = timed_rounds(methods, a.min_seconds)
    sisnr = []
    for _ in range(20):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        metrics.sisnr_ragged(c, e, off)
        t.record()
        t.synchronize()
        sisnr.append(s.elapsed_time(t) * 1e3)
    n = a.recordings
    res = {'metric': 'score_recordings', 'device': torch.cuda.get_device_name(0), 'recordings': n,
           'audio_seconds': round(float(off_h[-1]) / fs, 2), 'lengths_s': '1 .. 10 s at 16 kHz, uniform, seeded',
           'ragged_equals_per_recording': bool(torch.equal(first['ragged_call'], first['per_recording_stoi_batch'])),
           'max_abs_diff_vs_host': float(np.max(np.abs(first['ragged_call'].cpu().numpy() - np.array(first['host_loop'])))),
           'timing': 'device events around one pass over the set; methods alternate in 3 rounds, each filling a third of '
                     'min_seconds with repeated passes; median over the passes', 'min_seconds': a.min_seconds,
           'kernel_launches': {'ragged_call': 2 * 2 + 4, 'ragged_call_fills': 2, 'per_recording_stoi_batch': 5 * n,
                               'host_loop_copies': 2 * n},
           'sisnr_ragged_us_median': round(float(np.median(sisnr)), 2)}
    for name, _ in methods:
        res[name] = pass_stats(times[name], n)
    for name in ('per_recording_stoi_batch', 'host_loop'):
        res[f'speedup_ragged_vs_{name}'] = round(res[name]['ms_per_pass_median'] / res['ragged_call']['ms_per_pass_median'], 2)
    if a.extended:
        d, est_e = first['ragged_both']
        host_e = np.array([metrics.stoi(c[p:q].cpu().numpy(), e[p:q].cpu().numpy(), fs, extended=True) for p, q in spans])
        res['kernel_launches']['ragged_both'] = 2 * 2 + 4
        res['both_d_equals_ragged_call'] = bool(torch.equal(d, first['ragged_call']))
        res['estoi_max_abs_diff_vs_host'] = float(np.max(np.abs(est_e.cpu().numpy() - host_e)))
        res['both_over_stoi_only'] = round(res['ragged_both']['ms_per_pass_median'] / res['ragged_call']['ms_per_pass_median'], 3)
    if a.parent_json:
        with open(a.parent_json) as f:
            parent = json.load(f)
        res['parent_commit_ragged_call'] = parent['ragged_call']
        res['ragged_call_over_parent_commit'] = round(res['ragged_call']['ms_per_pass_median'] /
                                                      parent['ragged_call']['ms_per_pass_median'], 3)
    write_result(res, a.out)


def write_result(res, out):
    print(json.dumps(res))
    if out != '-':
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
