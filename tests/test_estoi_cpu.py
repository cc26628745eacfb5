"""CPU-only: the extended STOI (ESTOI) of dcsnet/metrics.py::stoi(..., extended=True) — an independent route through
np.corrcoef, its defining properties, the frame-count edges, that the default branch returns what it returned before the front
end was factored out — and evaluate.summarise with and without the extended columns, and the argument handling of the two
new C entry points (dcs_stoi_ext_f32, dcs_stoi_ext_ragged_f32: every call below fails validation before any launch).

Parity with pystoi stays unpinned (there is no pystoi to compare with): what is checked is the formula of Jensen & Taal (2016)
as pystoi 0.3.3 orders it, without pystoi's EPS-sized random dither."""
import ctypes

import numpy as np
import pytest
import torch

from dcsnet import _lib
from dcsnet import metrics

BAD, WORKSPACE = -1, -3                                       # DCS_ERR_BADARG, DCS_ERR_WORKSPACE
P = ctypes.c_void_p(16)                                       # never dereferenced


# ---- the signal generator of tests/test_stoi_device.py ---------------------------------------------------------------------

def _threshold_margin(x, fs):
    """Smallest |e - (max(e) - 40)| in dB over the clean frames of the host's framing (inf without frames)."""
    x = np.asarray(x, dtype=float)
    if fs != metrics.FS:
        x = metrics.resample_oct(x, metrics.FS, fs)
    f = metrics._frames(x, metrics.N_FRAME, metrics.N_FRAME // 2) * metrics._hann(metrics.N_FRAME)
    if len(f) == 0:
        return np.inf
    e = 20 * np.log10(np.linalg.norm(f, axis=1) + metrics.EPS)
    return float(np.min(np.abs(e - (e.max() - metrics.DYN_RANGE))))


def _speech(rng, L, fs, pause_frac):
    """Modulated multi-tone 'speech': a few harmonics of a gliding pitch plus a broadband (fricative-like) component 30 dB
    down, under a syllable-rate envelope, with pauses (-60 dB) covering about pause_frac of the signal.  The broadband part
    matters: with harmonics alone the clean bands above them hold nothing but spectral leakage, and their rows are noise."""
    t = np.arange(L) / fs
    f0 = rng.uniform(100, 220) * (1 + 0.1 * np.sin(2 * np.pi * rng.uniform(0.5, 2) * t))
    ph = 2 * np.pi * np.cumsum(f0) / fs
    s = sum(rng.uniform(0.2, 1.0) / k * np.sin(k * ph + rng.uniform(0, 2 * np.pi)) for k in range(1, 9))
    s = s + 10 ** (-30 / 20) * np.std(s) * rng.standard_normal(L)
    env = 0.6 + 0.4 * np.sin(2 * np.pi * rng.uniform(3, 6) * t + rng.uniform(0, 2 * np.pi))
    gate = np.ones(L)
    if pause_frac > 0:
        n = int(pause_frac * L)
        a = int(rng.integers(0, max(L - n, 1)))
        gate[a:a + n] = 1e-3
    return (s * env * gate).astype(np.float32)


def _clean(rng, L, fs, pause_frac):
    for _ in range(50):
        x = _speech(rng, L, fs, pause_frac)
        if _threshold_margin(x, fs) > 0.05:
            return x.astype(float)
    raise AssertionError('could not draw a signal away from the keep threshold')


def _noisy(x, noise, snr):
    return x + noise * (np.linalg.norm(x) / (np.linalg.norm(noise) * 10 ** (snr / 20)))


CASES = ((8160, 16000, 0.0, 5), (16000, 16000, 0.1, 0), (32000, 16000, 0.2, 10), (6000, 10000, 0.0, -5), (24000, 48000, 0.0, 15))


@pytest.fixture(scope='module')
def pairs():
    """(clean, estimate, fs) of the five sizes, with the host ESTOI of each: computed once and left unchanged."""
    rng = np.random.default_rng(2016)
    out = []
    for L, fs, pause, snr in CASES:
        x = _clean(rng, L, fs, pause)
        y = _noisy(x, rng.standard_normal(L), snr)
        out.append((x, y, fs, metrics.stoi(x, y, fs, extended=True)))
    return out


def _route_corrcoef(x, y, fs):
    """ESTOI by another route: rows normalised with plain numpy, then np.corrcoef of each of the 30 column pairs (a correlation
    coefficient IS the inner product of the mean-removed, unit-norm columns), averaged over columns, then over segments."""
    xseg, yseg = metrics._band_segments(x, y, fs)
    per_segment = []
    for xs, ys in zip(xseg, yseg):                            # [15, 30] each
        rows = []
        for m in (xs, ys):
            m = m - m.mean(axis=1)[:, None]
            rows.append(m / np.sqrt((m * m).sum(axis=1))[:, None])
        per_segment.append(np.mean([np.corrcoef(rows[0][:, i], rows[1][:, i])[0, 1] for i in range(metrics.N_SEG)]))
    return float(np.mean(per_segment))


def test_estoi_equals_the_corrcoef_route(pairs):
    for x, y, fs, e in pairs:
        assert 0.05 < e < 1.0, e
        assert abs(e - _route_corrcoef(x, y, fs)) <= 1e-12, (len(x), fs, e, _route_corrcoef(x, y, fs))


def test_estoi_of_a_signal_with_itself_is_one(pairs):
    for x, _, fs, _ in pairs:
        assert abs(metrics.stoi(x, x, fs, extended=True) - 1.0) <= 1e-9


def test_estoi_does_not_depend_on_the_level_of_the_estimate(pairs):
    """ESTOI has no clipping stage: the level cancels in the row normalisation (up to EPS beside the norms)."""
    for x, y, fs, e in pairs:
        for gain in (0.1, 10.0):
            assert abs(metrics.stoi(x, gain * y, fs, extended=True) - e) < 1e-6, (len(x), fs, gain)


def test_estoi_rises_with_the_snr():
    rng = np.random.default_rng(7)
    x = _clean(rng, 16000, 16000, 0.0)
    noise = rng.standard_normal(16000)
    scores = [metrics.stoi(x, _noisy(x, noise, snr), 16000, extended=True) for snr in (-10, -5, 0, 5, 10, 20, 30, 60)]
    assert all(b > a for a, b in zip(scores, scores[1:])), scores
    assert scores[-1] > 0.99, scores


def test_estoi_of_independent_noise_is_near_zero(pairs):
    rng = np.random.default_rng(8)
    for x, _, fs, _ in pairs:
        if len(x) < fs:                                       # at least 1 s: enough segments to average over
            continue
        e = metrics.stoi(x, np.std(x) * rng.standard_normal(len(x)), fs, extended=True)
        assert -0.2 < e < 0.2, (len(x), fs, e)


def test_estoi_at_the_frame_count_edges():
    """A stationary signal at 10 kHz (no frame removed): 4096 samples leave 29 STFT frames (exactly 1e-5), 4224 leave 30 (one
    segment), 4352 leave 31 (two segments)."""
    rng = np.random.default_rng(9)
    for L, frames in ((4096, 29), (4224, 30), (4352, 31)):
        x = rng.standard_normal(L)
        y = x + 0.5 * rng.standard_normal(L)
        xs, _ = metrics.remove_silent_frames(x, y, metrics.DYN_RANGE, metrics.N_FRAME, metrics.N_FRAME // 2)
        assert len(metrics._stft(xs, metrics.N_FRAME, metrics.NFFT, 2)) == frames
        e = metrics.stoi(x, y, metrics.FS, extended=True)
        if frames < metrics.N_SEG:
            assert e == 1e-5 and metrics._band_segments(x, y, metrics.FS) is None
        else:
            assert metrics._band_segments(x, y, metrics.FS)[0].shape == (frames - metrics.N_SEG + 1, metrics.NUMBAND, metrics.N_SEG)
            assert np.isfinite(e) and 0.05 < e < 1.0, e
            assert abs(e - _route_corrcoef(x, y, metrics.FS)) <= 1e-12


def test_estoi_of_constant_rows_is_finite_and_nan_input_gives_nan():
    """Silence as the estimate: every row of its segments is constant, normalises to zeros, and the score is 0, not NaN (the one
    place where pystoi's dither would matter).  A NaN sample gives NaN."""
    rng = np.random.default_rng(10)
    x = rng.standard_normal(8000)
    assert metrics.stoi(x, np.zeros(8000), metrics.FS, extended=True) == 0.0
    y = x.copy()
    y[4000] = np.nan
    assert np.isnan(metrics.stoi(x, y, metrics.FS, extended=True))


def _stoi_before_the_split(x, y, fs_sig):
    """metrics.stoi's default branch as it was before its front end moved into _band_segments: the same helpers, the same
    formula."""
    x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
    if fs_sig != metrics.FS:
        x, y = metrics.resample_oct(x, metrics.FS, fs_sig), metrics.resample_oct(y, metrics.FS, fs_sig)
    x, y = metrics.remove_silent_frames(x, y, metrics.DYN_RANGE, metrics.N_FRAME, metrics.N_FRAME // 2)
    xs, ys = metrics._stft(x, metrics.N_FRAME, metrics.NFFT, 2), metrics._stft(y, metrics.N_FRAME, metrics.NFFT, 2)
    if xs.ndim != 2 or xs.shape[0] < metrics.N_SEG:
        return 1e-5
    obm, _ = metrics.thirdoct(metrics.FS, metrics.NFFT, metrics.NUMBAND, metrics.MINFREQ)
    xt = np.sqrt(obm @ (np.abs(xs.T) ** 2))
    yt = np.sqrt(obm @ (np.abs(ys.T) ** 2))
    M = xt.shape[1]
    xseg = np.stack([xt[:, m - metrics.N_SEG:m] for m in range(metrics.N_SEG, M + 1)])
    yseg = np.stack([yt[:, m - metrics.N_SEG:m] for m in range(metrics.N_SEG, M + 1)])
    norm = np.linalg.norm(xseg, axis=2, keepdims=True) / (np.linalg.norm(yseg, axis=2, keepdims=True) + metrics.EPS)
    yn = yseg * norm
    clip = 10 ** (-metrics.BETA / 20)
    yp = np.minimum(yn, xseg * (1 + clip))
    yp = yp - yp.mean(axis=2, keepdims=True)
    xz = xseg - xseg.mean(axis=2, keepdims=True)
    yp = yp / (np.linalg.norm(yp, axis=2, keepdims=True) + metrics.EPS)
    xz = xz / (np.linalg.norm(xz, axis=2, keepdims=True) + metrics.EPS)
    return float(np.sum(yp * xz) / (xseg.shape[0] * xseg.shape[1]))


def test_the_default_branch_is_bit_for_bit_what_it_was(pairs):
    for x, y, fs, e in (pairs[0], pairs[3], pairs[4]):
        d = metrics.stoi(x, y, fs)
        assert d == _stoi_before_the_split(x, y, fs) and d == metrics.stoi(x, y, fs, extended=False)
        assert d != e
    assert metrics.stoi(np.zeros(300), np.zeros(300), metrics.FS) == 1e-5
    with pytest.raises(ValueError):
        metrics.stoi(np.zeros(300), np.zeros(301), metrics.FS, extended=True)


# ---- evaluate.summarise --------------------------------------------------------------------------------------------------

def test_summarise_takes_its_columns_from_the_dict():
    from dcsnet.evaluate import RecordingScorer, summarise
    assert RecordingScorer.METRICS == ('stoi', 'stoi_noisy', 'sisnr', 'sisnr_noisy')
    four = {'stoi': torch.tensor([0.8, 0.6, 0.7]), 'stoi_noisy': torch.tensor([0.5, 0.5, 0.5]),
            'sisnr': torch.tensor([10.0, 12.0, float('nan')]), 'sisnr_noisy': torch.tensor([1.0, 2.0, 3.0])}
    out, table = summarise(four)
    assert list(out) == ['files', 'stoi', 'stoi_nan', 'stoi_noisy', 'stoi_noisy_nan', 'sisnr', 'sisnr_nan', 'sisnr_noisy',
                         'sisnr_noisy_nan', 'stoi_improvement', 'sisnr_improvement']
    assert table.shape == (3, 4) and table.dtype == np.float32
    assert out['files'] == 3 and out['sisnr_nan'] == 1 and out['sisnr'] == 11.0 and out['sisnr_improvement'] == 9.5
    assert abs(out['stoi_improvement'] - 0.2) < 1e-6
    six = dict(four, estoi=torch.tensor([0.6, float('nan'), 0.4]), estoi_noisy=torch.tensor([0.25, 0.5, 0.25]))
    out6, table6 = summarise(six)
    assert sorted(out6) == sorted(list(out) + ['estoi', 'estoi_nan', 'estoi_noisy', 'estoi_noisy_nan', 'estoi_improvement'])
    assert table6.shape == (3, 6) and np.array_equal(table6[:, :4], table, equal_nan=True)
    assert all(out6[k] == out[k] for k in out)                # the four-key summary is a part of the six-key one
    assert out6['estoi_nan'] == 1 and out6['estoi_noisy_nan'] == 0
    assert abs(out6['estoi'] - 0.5) < 1e-6                    # the NaN is counted and left out of the mean
    assert abs(out6['estoi_noisy'] - 1.0 / 3) < 1e-6
    assert abs(out6['estoi_improvement'] - 0.25) < 1e-6       # over the pairs where both sides are numbers


def test_scorer_lists_its_metrics():
    from dcsnet.evaluate import RecordingScorer
    with pytest.raises(TypeError):
        RecordingScorer(object(), extended=True)              # the enhancer is still checked first
    import inspect
    assert list(inspect.signature(RecordingScorer.__init__).parameters) == ['self', 'enhancer', 'extended']
    assert inspect.signature(RecordingScorer.__init__).parameters['extended'].default is False


# ---- the two new entry points' argument handling -------------------------------------------------------------------------

def test_stoi_ext_rejects_bad_arguments_and_short_workspaces():
    lib = _lib.load()
    ws = lib.dcs_stoi_workspace_bytes(2, 5100)
    args = [P, P, 2, 5100, P, P, P, P, P, P, ws, None]        # clean, est, B, L, lo, hi, out_d, out_e, kept, ws, bytes, stream
    for i in (0, 1, 4, 5, 8, 9):
        a = list(args)
        a[i] = None
        assert lib.dcs_stoi_ext_f32(*a) == BAD, i
    a = list(args)
    a[6] = a[7] = None                                        # either output may be null, not both
    assert lib.dcs_stoi_ext_f32(*a) == BAD
    for i, v in ((2, 0), (2, -1), (2, 40000), (3, -1)):
        a = list(args)
        a[i] = v
        assert lib.dcs_stoi_ext_f32(*a) == BAD, (i, v)
    for drop in ((), (6,), (7,)):                             # a short workspace is refused whichever outputs are asked for
        a = list(args)
        a[10] = ws - 1
        for i in drop:
            a[i] = None
        assert lib.dcs_stoi_ext_f32(*a) == WORKSPACE, drop


def test_stoi_ext_ragged_rejects_bad_arguments_and_short_workspaces():
    lib = _lib.load()
    ws = lib.dcs_stoi_ragged_workspace_bytes(3, 30000)
    args = [P, P, P, 3, 30000, 12000, P, P, P, P, P, P, ws, None]   # clean, est, offsets, n, total, longest, lo, hi, d, e, kept, ws
    for i in (0, 1, 2, 6, 7, 10, 11):
        a = list(args)
        a[i] = None
        assert lib.dcs_stoi_ext_ragged_f32(*a) == BAD, i
    a = list(args)
    a[8] = a[9] = None
    assert lib.dcs_stoi_ext_ragged_f32(*a) == BAD
    for i, v in ((3, 0), (3, -1), (3, 40000), (4, -1), (5, -1)):
        a = list(args)
        a[i] = v
        assert lib.dcs_stoi_ext_ragged_f32(*a) == BAD, (i, v)
    for drop in ((), (8,), (9,)):
        a = list(args)
        a[12] = ws - 1
        for i in drop:
            a[i] = None
        assert lib.dcs_stoi_ext_ragged_f32(*a) == WORKSPACE, drop


def test_the_ops_check_the_extended_keyword_before_anything_else():
    from dcsnet import ops
    x = torch.zeros(2, 8160)
    for bad in ('yes', 2, None):
        with pytest.raises(_lib.DcsHipError, match='extended'):
            ops.stoi(x, x, extended=bad)
        with pytest.raises(_lib.DcsHipError, match='extended'):
            ops.stoi_ragged(x[0], x[0], torch.zeros(2, dtype=torch.int64), 8160, extended=bad)
    with pytest.raises(_lib.DcsHipError):
        metrics.stoi_batch(x, x, 16000, extended='both')      # CPU tensors: no host fallback, as without the keyword
