"""CPU-only: the host contract of the BSS-eval signal-to-distortion ratio (dcsnet/metrics.py::sdr) and the C ABI of its device
form (csrc/sdr_ragged.hip; every call here fails validation before any launch or is pure host arithmetic).

Parity with mir_eval / museval is unpinned (neither is available), so the checks are independent routes — a brute-force
least-squares projection onto the stacked shifted copies of the reference, and the filter from two other Toeplitz solvers, all
within 1e-9 dB — and the measure's defining properties: gain invariance, SDR >= SI-SNR, a short filter between the signals is
forgiven where SI-SNR is not, a delay is forgiven, the NaN cases and one exact +inf."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
from scipy.linalg import solve_toeplitz, toeplitz
from scipy.signal import lfilter

from dcsnet import _lib
from dcsnet import metrics

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, WORKSPACE = -1, -3                                       # DCS_ERR_BADARG, DCS_ERR_WORKSPACE
P = ctypes.c_void_p(16)                                       # never dereferenced
NEW = ('dcs_sdr_ragged_workspace_bytes', 'dcs_sdr_ragged_f32')
CASES = ((600, 512), (300, 16))                               # (L, K)


def _pair(L, snr_db, seed):
    """AR(2)-shaped noise as the clean signal, white noise added at snr_db."""
    rng = np.random.default_rng(seed)
    x = lfilter([1.0], [1.0, -1.6, 0.8], rng.standard_normal(L + 200))[200:]
    v = rng.standard_normal(L)
    v *= np.linalg.norm(x) / np.linalg.norm(v) * 10 ** (-snr_db / 20)
    return 0.1 * x, 0.1 * (x + v)


def _si_snr(x, y):
    """The projection onto x alone: a gain is all it forgives."""
    s = np.dot(x, y) / np.dot(x, x) * x
    return 10.0 * np.log10(np.dot(s, s) / np.dot(y - s, y - s))


def _shift_matrix(x, K):
    """(L + K - 1) x K: column k is x delayed by k samples."""
    L = len(x)
    A = np.zeros((L + K - 1, K))
    for k in range(K):
        A[k:k + L, k] = x
    return A


# ---- independent routes ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('L, K', CASES)
def test_against_a_brute_force_projection(L, K):
    x, y = _pair(L, 10, L + K)
    A = _shift_matrix(x, K)
    y_pad = np.concatenate([y, np.zeros(K - 1)])
    c = np.linalg.lstsq(A, y_pad, rcond=None)[0]
    s = A @ c
    want = 10.0 * np.log10(np.dot(s, s) / np.dot(y_pad - s, y_pad - s))
    got = metrics.sdr(x, y, K)
    print(f'[sdr] L={L} K={K}: levinson {got:.12f} dB, lstsq {want:.12f} dB, diff {abs(got - want):.2e}')
    assert abs(got - want) <= 1e-9


@pytest.mark.parametrize('L, K', CASES)
def test_against_two_other_solvers(L, K):
    x, y = _pair(L, 20, 2 * L + K)
    R, D = metrics.sdr_correlations(x, y, K)
    A = _shift_matrix(x, K)
    assert np.allclose(R, (A.T @ A)[0], rtol=1e-12, atol=1e-14) and np.allclose(D, A.T @ np.concatenate([y, np.zeros(K - 1)]),
                                                                                 rtol=1e-12, atol=1e-14)
    got = metrics.sdr(x, y, K)
    c, E = metrics.toeplitz_levinson(R, D)
    assert got == metrics.sdr_from_filter(x, y, c) and np.all(E > 0) and np.all(np.diff(E) <= 0)
    for name, c_other in (('np.linalg.solve', np.linalg.solve(toeplitz(R), D)), ('solve_toeplitz', solve_toeplitz(R, D))):
        want = metrics.sdr_from_filter(x, y, c_other)
        print(f'[sdr] L={L} K={K} {name}: diff {abs(got - want):.2e} dB')
        assert abs(got - want) <= 1e-9, name


def test_correlations_past_the_signal_are_zero():
    x, y = _pair(5, 10, 3)
    R, D = metrics.sdr_correlations(x, y, 8)
    assert np.all(R[5:] == 0) and np.all(D[5:] == 0) and R[4] == x[0] * x[4] and D[4] == x[0] * y[4]


# ---- properties ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('gain', [0.1, 7.0])
def test_a_gain_on_the_estimate_changes_nothing(gain):
    x, y = _pair(2000, 10, 4)
    assert abs(metrics.sdr(x, gain * y) - metrics.sdr(x, y)) <= 1e-9


@pytest.mark.parametrize('snr', [0, 20])
def test_sdr_is_at_least_si_snr(snr):
    x, y = _pair(3000, snr, 5)
    assert metrics.sdr(x, y) >= _si_snr(x, y) - 1e-9
    assert metrics.sdr(x, y, 1) == pytest.approx(_si_snr(x, y), abs=1e-9)         # one tap: the gain alone


def test_a_short_filter_is_forgiven_where_si_snr_is_not():
    x, _ = _pair(8000, 10, 6)
    rng = np.random.default_rng(7)
    xh = np.convolve(x, [1.0, -0.6, 0.3])[:len(x)]
    v = rng.standard_normal(len(x))
    v *= np.linalg.norm(xh) / np.linalg.norm(v) * 10 ** (-15 / 20)
    y = xh + v
    snr = 10.0 * np.log10(np.dot(xh, xh) / np.dot(v, v))
    got, si = metrics.sdr(x, y), _si_snr(x, y)
    print(f'[sdr] coloured: SNR of v against x * h {snr:.2f} dB, SDR {got:.2f} dB, SI-SNR {si:.2f} dB')
    assert abs(got - snr) < 3.0 and si < got - 1.0


def test_a_delay_is_forgiven():
    """L = 4800, y = x delayed by 100 samples.  x ends in 100 zeros, so that the delay drops nothing at the end of the recording:
    a delayed copy cut off at L lacks the last 100 samples of x, and the projection, which is L + K - 1 long, keeps them."""
    x, _ = _pair(4800, 10, 8)
    x[-100:] = 0.0
    y = np.concatenate([np.zeros(100), x[:-100]])
    got = metrics.sdr(x, y)
    print(f'[sdr] delay of 100: SDR {got:.1f} dB, SI-SNR {_si_snr(x, y):.2f} dB')
    assert got > 100.0
    assert _si_snr(x, y) < 10.0


def test_nan_cases_and_the_exact_infinity():
    x, y = _pair(700, 10, 9)
    assert math.isnan(metrics.sdr(np.zeros(0), np.zeros(0)))
    assert math.isnan(metrics.sdr(np.zeros(700), y)) and math.isnan(metrics.sdr(x, np.zeros(700)))
    bad = y.copy()
    bad[3] = np.inf
    assert math.isnan(metrics.sdr(x, bad)) and math.isnan(metrics.sdr(bad, y))
    bad[3] = np.nan
    assert math.isnan(metrics.sdr(x, bad))
    assert metrics.sdr(np.array([0.5]), np.array([0.25])) == math.inf               # every intermediate is a power of two
    assert isinstance(metrics.sdr(x, y), float)
    with pytest.raises(ValueError):
        metrics.sdr(x, y[:-1])
    for K in (0, 513):
        with pytest.raises(ValueError):
            metrics.sdr(x, y, K)


def test_summarise_and_the_scorer_attribute():
    from dcsnet.evaluate import RecordingScorer, summarise
    assert RecordingScorer.SDR == ('sdr', 'sdr_noisy')
    base = {k: torch.tensor([0.5, 0.25, 0.75]) for k in RecordingScorer.METRICS}
    plain, table = summarise(base)
    assert table.shape == (3, 4) and 'sdr' not in plain
    scores = dict(base, sdr=torch.tensor([12.0, float('inf'), float('nan')]), sdr_noisy=torch.tensor([2.0, float('inf'), 1.0]))
    s, table = summarise(scores)
    assert table.shape == (3, 6) and all(s[k] == v for k, v in plain.items())
    assert s['sdr_nan'] == 1 and s['sdr_noisy_nan'] == 0 and s['sdr_improvement'] == 10.0


# ---- the C ABI -------------------------------------------------------------------------------------------------------------

def test_new_entry_points_are_declared_exported_and_bound():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'dcsnet_hip.h')).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', header), f'{name} is not declared in include/dcsnet_hip.h'
        assert hasattr(lib, name), f'{name} is not exported'
        assert name in _lib.SIGNATURES
    assert _lib.load().dcs_abi_version() == 20                # entry points were added, nothing else changed


def test_workspace_query_and_argument_errors():
    from dcsnet import ops
    lib = _lib.load()
    query = lib.dcs_sdr_ragged_workspace_bytes
    ws = query(3, 30000, 512)
    assert ws > 0 and ops.sdr_workspace_bytes(3, 30000) == ws and ops.SDR_CHUNK == 2048
    for n, total, K in ((0, 100, 512), (-1, 100, 512), (40000, 100, 512), (3, -1, 512), (3, 100, 0), (3, 100, 513), (3, 100, -4)):
        assert query(n, total, K) < 0, (n, total, K)
    for n, total, K in ((1, 0, 1), (1, 1, 512), (824, 20_000_000, 512)):
        assert query(n, total, K) > 0, (n, total, K)
    # it does not decrease in n, total or K
    for lo, hi in (((3, 30000, 512), (4, 30000, 512)), ((3, 30000, 512), (3, 30001, 512)), ((3, 30000, 512), (3, 60000, 512)),
                   ((3, 30000, 16), (3, 30000, 17)), ((3, 30000, 1), (3, 30000, 512)), ((1, 0, 512), (32767, 0, 512))):
        assert query(*lo) <= query(*hi), (lo, hi)
    ns, totals, Ks = (1, 2, 33), (0, 2047, 2048, 100000), (1, 16, 512)
    size = np.array([[[query(n, total, K) for K in Ks] for total in totals] for n in ns])
    assert (size > 0).all() and all((np.diff(size, axis=axis) >= 0).all() for axis in range(3))
    # clean, est, est2, offsets, n, total, filter_length, out, out2, workspace, bytes, stream
    one = [P, P, None, P, 3, 30000, 512, P, None, P, ws, None]
    two = [P, P, P, P, 3, 30000, 512, P, P, P, ws, None]
    call = lib.dcs_sdr_ragged_f32
    for args in (one, two):
        for i in (0, 1, 3, 7, 9):                            # a null pointer
            a = list(args)
            a[i] = None
            assert call(*a) == BAD, i
        for i, v in ((4, 0), (4, -1), (4, 40000), (5, -1), (5, 2 ** 41), (6, 0), (6, 513), (6, -512)):
            a = list(args)
            a[i] = v
            assert call(*a) == BAD, (i, v)
        a = list(args)
        a[10] = ws - 1
        assert call(*a) == WORKSPACE
    for i in (2, 8):                                         # est2 and out2: both or neither
        a = list(two)
        a[i] = None
        assert call(*a) == BAD, i


def test_python_layer_rejects_cpu_tensors():
    """(Host offsets are checked behind the test for device signals: tests/test_sdr_device.py::test_argument_errors.)"""
    from dcsnet import ops
    x, off = torch.zeros(1000), torch.tensor([0, 400, 1000])
    with pytest.raises(_lib.DcsHipError):
        metrics.sdr_ragged(x, x, off)
    with pytest.raises(_lib.DcsHipError):
        metrics.sdr_ragged(x, x, off, estimate2=x)
    with pytest.raises(_lib.DcsHipError):
        ops.sdr_ragged(x, x, off)
    with pytest.raises(_lib.DcsHipError):
        ops.sdr_workspace_bytes(2, 1000, 513)

