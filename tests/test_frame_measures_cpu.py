"""CPU-only: the host contract of the three frame-based objective measures (dcsnet/metrics.py::frame_measures: segmental SNR,
LPC log-likelihood ratio, LPC cepstrum distance after Hu & Loizou) and the C ABI of their device form (csrc/frame_measures.hip;
every call here fails validation before any launch or is pure host arithmetic).

Parity with pysepm or the MATLAB originals is unpinned (neither is available), so the checks are the measures' defining
properties — the frame count, exact segmental SNRs and the clamps, gain invariance, zero for identical signals, the trimmed
mean's count and its behaviour under ties, which frames are valid — and two independent routes: the Levinson-Durbin
recursion against scipy's Toeplitz solver, the cepstrum recursion against the FFT cepstrum of 1 / A."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
from scipy.linalg import solve_toeplitz
from scipy.signal import lfilter

from dcsnet import _lib
from dcsnet import metrics

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, WORKSPACE = -1, -3                                       # DCS_ERR_BADARG, DCS_ERR_WORKSPACE
P = ctypes.c_void_p(16)                                       # never dereferenced
NEW = ('dcs_frame_measures_ragged_workspace_bytes', 'dcs_frame_measures_ragged_f32')


def _pair(L, snr_db, seed, fs=16000):
    """AR(2)-shaped noise as the clean signal, white noise added at snr_db."""
    rng = np.random.default_rng(seed)
    x = lfilter([1.0], [1.0, -1.6, 0.8], rng.standard_normal(L + 200))[200:]
    v = rng.standard_normal(L)
    v *= np.linalg.norm(x) / np.linalg.norm(v) * 10 ** (-snr_db / 20)
    return 0.1 * x, 0.1 * (x + v)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------

def test_new_entry_points_are_declared_exported_and_bound():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'dcsnet_hip.h')).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', header), f'{name} is not declared in include/dcsnet_hip.h'
        assert hasattr(lib, name), f'{name} is not exported'
        assert name in _lib.SIGNATURES


def test_workspace_query_and_argument_errors():
    lib = _lib.load()
    ws = lib.dcs_frame_measures_ragged_workspace_bytes(3, 30000, 16000)
    assert ws > 0
    for n, total, fs in ((0, 100, 16000), (-1, 100, 16000), (40000, 100, 16000), (3, -1, 16000), (3, 100, 4000), (3, 100, 7999),
                         (3, 100, 48001), (3, 100, 0)):
        assert lib.dcs_frame_measures_ragged_workspace_bytes(n, total, fs) < 0, (n, total, fs)
    for n, total, fs in ((1, 0, 8000), (1, 1, 48000), (824, 20_000_000, 16000)):
        assert lib.dcs_frame_measures_ragged_workspace_bytes(n, total, fs) > 0, (n, total, fs)
    # clean, est, offsets, n, total, fs, window, window_len, ssnr, llr, cd, workspace, bytes, stream
    args = [P, P, P, 3, 30000, 16000, P, 480, P, P, P, P, ws, None]
    call = lib.dcs_frame_measures_ragged_f32
    for i in (0, 1, 2, 6, 8, 9, 10, 11):
        a = list(args)
        a[i] = None
        assert call(*a) == BAD, i
    for i, v in ((3, 0), (3, -1), (3, 40000), (4, -1), (5, 4000), (5, 48001), (7, 479), (7, 481)):
        a = list(args)
        a[i] = v
        assert call(*a) == BAD, (i, v)
    a = list(args)
    a[12] = ws - 1
    assert call(*a) == WORKSPACE


def test_workspace_follows_the_total_length():
    """100 recordings of 2.28 M samples together need the same workspace whether one of them is long or not, a fraction of what
    100 x the longest would, and it grows with the total."""
    lib = _lib.load()
    q = lib.dcs_frame_measures_ragged_workspace_bytes
    mixed = q(100, 300_000 + 99 * 20_000, 16000)
    assert 0 < mixed < q(100, 100 * 300_000, 16000) / 6
    assert q(100, 2 * 2_280_000, 16000) > 1.9 * mixed - 4096
    assert mixed <= (3 * 8 + 4) * (2_280_000 // 120) + 101 * 8 + 3 * 256      # three doubles and a flag per frame slot


def test_python_layer_rejects_cpu_tensors_and_bad_rates():
    from dcsnet import ops
    x, off = torch.zeros(1000), torch.tensor([0, 400, 1000])
    with pytest.raises(_lib.DcsHipError):
        metrics.frame_measures_ragged(x, x, off, 16000)
    with pytest.raises(_lib.DcsHipError):
        ops.frame_measures_ragged(x, x, off, 16000)
    with pytest.raises(_lib.DcsHipError):
        ops.frame_measures_workspace_bytes(2, 1000, 4000)


# ---- framing ------------------------------------------------------------------------------------------------------------

def test_frame_count_at_16_khz():
    x, y = _pair(720, 10, 1)
    assert metrics.frame_geometry(16000) == (480, 120, 16)
    for L, frames in ((599, 0), (600, 1), (719, 1), (720, 2)):
        assert metrics.frame_count(L, 16000) == frames
        m = metrics.frame_measures(x[:L], y[:L], 16000)
        assert sorted(m) == ['cd', 'llr', 'ssnr'] and all(isinstance(v, float) for v in m.values())
        assert all(math.isnan(v) for v in m.values()) == (frames == 0), (L, m)
        assert len(metrics.frame_values(x[:L], y[:L], 16000)[0]) == frames
    for L in (0, 1):
        assert all(math.isnan(v) for v in metrics.frame_measures(x[:L], y[:L], 16000).values())


def test_geometry_at_8_khz():
    assert metrics.frame_geometry(8000) == (240, 60, 10)
    assert metrics.frame_geometry(48000) == (1440, 360, 16)
    assert metrics.frame_geometry(9999)[2] == 10 and metrics.frame_geometry(10000)[2] == 16
    x, y = _pair(480, 10, 2)
    assert metrics.frame_count(299, 8000) == 0 and metrics.frame_count(300, 8000) == 1 and metrics.frame_count(480, 8000) == 4
    m = metrics.frame_measures(x, y, 8000)
    assert all(np.isfinite(v) for v in m.values())


def test_thin_wrappers():
    x, y = _pair(3000, 5, 3)
    m = metrics.frame_measures(x, y, 16000)
    assert metrics.ssnr(x, y, 16000) == m['ssnr'] and metrics.llr(x, y, 16000) == m['llr']
    assert metrics.cepstrum_distance(x, y, 16000) == m['cd']
    with pytest.raises(ValueError):
        metrics.frame_measures(x, y[:-1], 16000)


# ---- segmental SNR: exact values and the clamps ------------------------------------------------------------------------------

def test_ssnr_of_a_scaled_copy_and_its_clamps():
    x, _ = _pair(8000, 10, 4)
    assert abs(metrics.ssnr(x, 1.1 * x, 16000) - 20.0) <= 1e-9
    assert metrics.ssnr(x, (1 + 1e-3) * x, 16000) == 35.0
    assert metrics.ssnr(x, 11.0 * x, 16000) == -10.0
    assert abs(metrics.ssnr(x, 2.0 * x, 16000)) <= 1e-9                     # g = 1: 0 dB


def test_ssnr_counts_silent_frames_as_minus_ten():
    x, _ = _pair(8000, 10, 5)
    x[2000:5000] = 0.0
    starts = 120 * np.arange(metrics.frame_count(len(x), 16000))
    silent = int(np.sum((starts >= 2000) & (starts + 480 <= 5000)))
    assert 0 < silent < len(starts)
    want = (35.0 * (len(starts) - silent) - 10.0 * silent) / len(starts)
    got = metrics.ssnr(x, x, 16000)
    assert -10.0 < got < 35.0 and abs(got - want) <= 1e-9


# ---- LLR and CD -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', [0.25, 4.0])
def test_llr_and_cd_do_not_depend_on_the_estimates_gain(c):
    x, y = _pair(6000, 10, 6)
    a, b = metrics.frame_measures(x, y, 16000), metrics.frame_measures(x, c * y, 16000)
    assert abs(a['llr'] - b['llr']) <= 1e-9 and abs(a['cd'] - b['cd']) <= 1e-9
    assert 0.0 < a['llr'] < 2.0 and 0.0 < a['cd'] < 10.0


def test_identical_signals_score_zero():
    x, _ = _pair(6000, 10, 7)
    m = metrics.frame_measures(x, x, 16000)
    assert m['llr'] == 0.0 and m['cd'] == 0.0 and m['ssnr'] == 35.0


def test_prototype_signal_lands_where_expected():
    """Not a fixture: the order of magnitude for AR(2)-shaped noise with white noise at 10 dB."""
    x, y = _pair(16000, 10, 8)
    m = metrics.frame_measures(x, y, 16000)
    assert 8.0 < m['ssnr'] < 12.0 and 0.2 < m['llr'] < 1.2 and 3.0 < m['cd'] < 7.0


# ---- independent routes ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('order', [10, 16])
def test_levinson_recursion_against_the_toeplitz_solver(order):
    rng = np.random.default_rng(9)
    f = lfilter([1.0], [1.0, -0.9], rng.standard_normal((5, 480)), axis=1) * metrics._measure_window(480)
    R = metrics._autocorrelation(f, order)
    A, E = metrics._lpc(R, order)
    for r, a, e in zip(R, A, E):
        ref = solve_toeplitz(r[:order], r[1:order + 1])
        assert a[0] == 1.0 and np.max(np.abs(-a[1:] - ref)) <= 1e-8
        assert abs(e[order] - (r[0] - ref @ r[1:order + 1])) <= 1e-8 * r[0]      # the final error energy, both ways
        assert (e > 0).all()


def test_cepstrum_recursion_against_the_fft_cepstrum():
    """A stable AR(4): two pole pairs of radii 0.9 and 0.7.  log(1 / A(e^jw)) sampled on 4096 points and transformed back gives
    the cepstrum of 1 / A up to aliasing of order 0.9^4096."""
    poles = [0.9 * np.exp(1j * 0.7), 0.7 * np.exp(1j * 2.1)]
    A = np.real(np.poly(poles + [np.conj(p) for p in poles]))
    assert A[0] == 1.0 and len(A) == 5
    c = metrics._lpc_cepstrum(A)
    w = 2 * np.pi * np.arange(4096) / 4096
    spectrum = sum(A[k] * np.exp(-1j * w * k) for k in range(5))
    ref = np.real(np.fft.ifft(-np.log(spectrum)))
    assert np.max(np.abs(c[1:] - ref[1:5])) <= 1e-6
    stacked = metrics._lpc_cepstrum(np.stack([A, A]))                       # the vectorised form used per frame
    assert np.array_equal(stacked[0], c) and np.array_equal(stacked[1], c)


# ---- the trimmed mean ---------------------------------------------------------------------------------------------------------

def test_trimmed_count():
    for V in (1, 10, 11, 30, 31):
        assert metrics.trimmed_count(V) == max(1, math.floor(0.95 * V + 0.5)), V
    assert [metrics.trimmed_count(V) for V in (1, 10, 11, 30, 31)] == [1, 10, 10, 29, 29]
    assert metrics._trimmed_mean(np.array([5.0, 1.0, 3.0])) == 3.0          # K = 3: all of them
    assert metrics._trimmed_mean(np.arange(20.0)[::-1]) == np.mean(np.arange(19.0))
    assert math.isnan(metrics._trimmed_mean(np.zeros(0)))


def test_tied_frames_return_the_common_value():
    """Every frame of a 120-periodic recording is the same frame (the hop is 120): all values tie."""
    rng = np.random.default_rng(10)
    x = np.tile(rng.standard_normal(120), 40)
    y = x + np.tile(0.3 * rng.standard_normal(120), 40)
    assert len(x) == 4800
    s, l, c, valid = metrics.frame_values(x, y, 16000)
    assert len(s) == 36 and valid.all()
    m = metrics.frame_measures(x, y, 16000)
    for key, v in (('ssnr', s), ('llr', l), ('cd', c)):
        assert np.ptp(v) <= 1e-12 * abs(v[0]) and abs(m[key] - v[0]) <= 1e-12 * abs(v[0]), key
    assert 0.0 < m['llr'] < 2.0 and 0.0 < m['cd'] < 10.0


# ---- validity -----------------------------------------------------------------------------------------------------------------

def test_silent_frames_take_no_part_in_llr_and_cd():
    x, y = _pair(8000, 10, 11)
    x[:2000], y[:2000] = 0.0, 0.0
    s, l, c, valid = metrics.frame_values(x, y, 16000)
    starts = 120 * np.arange(len(s))
    silent = starts + 480 <= 2000
    assert silent.sum() == 13 and not valid[silent].any() and valid[~silent].all()
    assert (s[silent] == -10.0).all()
    m = metrics.frame_measures(x, y, 16000)
    tail = metrics.frame_values(x[2040:], y[2040:], 16000)                  # the frames 17 .. of the whole, all sounding
    assert abs(m['ssnr'] - np.mean(s)) <= 1e-12
    K = metrics.trimmed_count(int(valid.sum()))
    assert abs(m['llr'] - np.mean(np.sort(l[valid])[:K])) <= 1e-12 and abs(m['cd'] - np.mean(np.sort(c[valid])[:K])) <= 1e-12
    assert np.allclose(tail[1], l[17:], rtol=0, atol=1e-9)


def test_an_all_zero_clean_recording():
    _, y = _pair(3000, 10, 12)
    m = metrics.frame_measures(np.zeros(3000), y, 16000)
    assert m['ssnr'] == -10.0 and math.isnan(m['llr']) and math.isnan(m['cd'])
    m = metrics.frame_measures(y, np.zeros(3000), 16000)                    # a silent estimate: 0 dB frames, no LPC model
    assert abs(m['ssnr']) <= 1e-9 and math.isnan(m['llr']) and math.isnan(m['cd'])


# ---- the scorer's summary and the tools (host side) ---------------------------------------------------------------------------------

def test_summarise_with_the_frame_measure_keys():
    from dcsnet.evaluate import RecordingScorer, summarise
    nan = float('nan')
    base = {'stoi': torch.tensor([0.5, 0.7]), 'stoi_noisy': torch.tensor([0.4, 0.5]),
            'sisnr': torch.tensor([10.0, 14.0]), 'sisnr_noisy': torch.tensor([5.0, 5.0])}
    more = {'ssnr': torch.tensor([8.0, 6.0]), 'ssnr_noisy': torch.tensor([2.0, 4.0]), 'llr': torch.tensor([0.4, nan]),
            'llr_noisy': torch.tensor([0.9, 1.0]), 'cd': torch.tensor([3.0, 4.0]), 'cd_noisy': torch.tensor([5.0, 7.0])}
    s0, t0 = summarise(base)
    s, t = summarise(dict(base, **more))
    assert t.shape == (2, 10) and np.array_equal(t[:, :4], t0)
    assert all(s[k] == v for k, v in s0.items())                            # nothing that was there moves
    assert s['ssnr_improvement'] == pytest.approx(4.0) and s['llr_improvement'] == pytest.approx(0.5)
    assert s['cd_improvement'] == pytest.approx(2.5) and s['llr_nan'] == 1 and s['cd_nan'] == 0
    assert RecordingScorer.FRAME_MEASURES == ('ssnr', 'ssnr_noisy', 'llr', 'llr_noisy', 'cd', 'cd_noisy')
    s6, t6 = summarise(dict(base, estoi=base['stoi'], estoi_noisy=base['stoi_noisy'], **more))
    assert t6.shape == (2, 12) and np.array_equal(t6[:, 6:], t[:, 4:], equal_nan=True) and s6['ssnr_improvement'] == s['ssnr_improvement']


def test_scorer_flag_names_the_keys():
    from dcsnet.enhance import Enhancer
    from dcsnet.evaluate import RecordingScorer
    enh = Enhancer.__new__(Enhancer)
    assert RecordingScorer(enh).metrics == RecordingScorer.METRICS
    for extended in (False, True):
        scorer = RecordingScorer(enh, extended=extended)
        before = scorer.metrics
        assert scorer.frame_measures is False
        scorer.frame_measures = True
        assert scorer.metrics == before + RecordingScorer.FRAME_MEASURES
        scorer.frame_measures = False
        assert scorer.metrics == before
