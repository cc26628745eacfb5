"""CPU-only: the host contract of the weighted spectral slope and the frequency-weighted segmental SNR
(dcsnet/metrics.py::spectral_measures, after Hu & Loizou), the composite measures, and the C ABI of the device form
(csrc/spectral_measures.hip; every call here fails validation before any launch or is pure host arithmetic).

Parity with the MATLAB originals or pysepm is unpinned (neither is available), so the checks are the measures' defining
properties — the frame count, zero / 35 dB for identical signals, gain invariance, the bank's shape, the published peak search
on hand-made band profiles, the trimmed mean under ties, silence, the clamps — and one independent route: the spectra through
an explicit DFT matrix."""
import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch
from scipy.signal import lfilter

from dcsnet import _lib
from dcsnet import metrics

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, WORKSPACE = -1, -3                                       # DCS_ERR_BADARG, DCS_ERR_WORKSPACE
P = ctypes.c_void_p(16)                                       # never dereferenced
NEW = ('dcs_spectral_measures_ragged_workspace_bytes', 'dcs_spectral_measures_ragged_f32')


def _pair(L, snr_db, seed):
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
    assert _lib.load().dcs_abi_version() == 20                # entry points were added, nothing else changed


def test_workspace_query_and_argument_errors():
    lib = _lib.load()
    ws = lib.dcs_spectral_measures_ragged_workspace_bytes(3, 30000, 16000)
    assert ws > 0
    for n, total, fs in ((0, 100, 16000), (-1, 100, 16000), (40000, 100, 16000), (3, -1, 16000), (3, 100, 4000), (3, 100, 7999),
                         (3, 100, 48001), (3, 100, 0)):
        assert lib.dcs_spectral_measures_ragged_workspace_bytes(n, total, fs) < 0, (n, total, fs)
    for n, total, fs in ((1, 0, 8000), (1, 1, 48000), (824, 20_000_000, 16000)):
        assert lib.dcs_spectral_measures_ragged_workspace_bytes(n, total, fs) > 0, (n, total, fs)
    # two doubles and a flag per frame slot: it follows the total length
    assert ws <= (2 * 8 + 4) * (30000 // 120) + 4 * 8 + 3 * 256
    # clean, est, offsets, n, total, fs, window, window_len, band_first, band_offset, band_weights, their count, twiddles,
    # twiddles_len, wss, fwssnr, workspace, bytes, stream
    args = [P, P, P, 3, 30000, 16000, P, 480, P, P, P, 600, P, 1024, P, P, P, ws, None]
    call = lib.dcs_spectral_measures_ragged_f32
    for i in (0, 1, 2, 6, 8, 9, 10, 12, 14, 15, 16):
        a = list(args)
        a[i] = None
        assert call(*a) == BAD, i
    for i, v in ((3, 0), (3, -1), (3, 40000), (4, -1), (5, 4000), (5, 48001), (7, 479), (7, 481), (11, -1), (13, 512), (13, 2048)):
        a = list(args)
        a[i] = v
        assert call(*a) == BAD, (i, v)
    a = list(args)
    a[17] = ws - 1
    assert call(*a) == WORKSPACE


def test_python_layer_rejects_cpu_tensors_and_bad_rates():
    from dcsnet import ops
    x, off = torch.zeros(1000), torch.tensor([0, 400, 1000])
    with pytest.raises(_lib.DcsHipError):
        metrics.spectral_measures_ragged(x, x, off, 16000)
    with pytest.raises(_lib.DcsHipError):
        ops.spectral_measures_ragged(x, x, off, 16000)
    with pytest.raises(_lib.DcsHipError):
        ops.spectral_measures_workspace_bytes(2, 1000, 4000)


# ---- framing and the transform ------------------------------------------------------------------------------------------------

def test_frame_count_and_result_types():
    x, y = _pair(720, 10, 1)
    for L, frames in ((599, 0), (600, 1), (719, 1), (720, 2)):
        m = metrics.spectral_measures(x[:L], y[:L], 16000)
        assert sorted(m) == ['fwssnr', 'wss'] and all(isinstance(v, float) for v in m.values())
        assert all(math.isnan(v) for v in m.values()) == (frames == 0), (L, m)
        wss, fw, valid = metrics.spectral_frame_values(x[:L], y[:L], 16000)
        assert len(wss) == len(fw) == len(valid) == frames and valid.dtype == bool
    for L in (0, 1):
        assert all(math.isnan(v) for v in metrics.spectral_measures(x[:L], y[:L], 16000).values())
    assert metrics.spectral_frame_values(x[:300], y[:300], 8000)[0].shape == (1,)
    m = metrics.spectral_measures(x, y, 16000)
    assert metrics.wss(x, y, 16000) == m['wss'] and metrics.fwssnr(x, y, 16000) == m['fwssnr']
    with pytest.raises(ValueError):
        metrics.spectral_measures(x, y[:-1], 16000)


def test_fft_sizes():
    assert [metrics.spectral_fft_size(fs) for fs in (8000, 16000, 22050, 48000)] == [512, 1024, 2048, 4096]
    assert metrics.spectral_fft_size(8549) == 512 and metrics.spectral_fft_size(8550) == 1024      # N = 256 and 257


@pytest.mark.parametrize('fs', [8000, 16000, 22050, 48000])
def test_rfft_against_an_explicit_dft_matrix(fs):
    N = metrics.frame_geometry(fs)[0]
    nfft = metrics.spectral_fft_size(fs)
    rng = np.random.default_rng(2)
    f = lfilter([1.0], [1.0, -1.6, 0.8], rng.standard_normal((3, N + 200)), axis=1)[:, 200:] * metrics._measure_window(N)
    f /= np.abs(f).max()
    k, t = np.arange(nfft // 2)[:, None], np.arange(N)[None, :]
    dft = np.exp(-2j * np.pi * ((k * t) % nfft) / nfft)       # the angle reduced in integers
    assert np.max(np.abs(np.fft.rfft(f, n=nfft, axis=1)[:, :nfft // 2] - f @ dft.T)) <= 1e-10


# ---- the bank -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('fs, top', [(16000, 244), (48000, 325), (8000, 244), (22050, None)])
def test_critical_band_bank(fs, top):
    nfft = metrics.spectral_fft_size(fs)
    H = nfft // 2
    g = metrics.critical_band_bank(fs)
    assert g.shape == (25, H) and len(metrics.CRIT_CENTRES) == len(metrics.CRIT_BANDWIDTHS) == 25
    assert (g >= 0).all() and (g[g > 0] > math.exp(-30 / (2 * 2.303))).all()
    if top is not None:
        assert np.flatnonzero(g.any(axis=0)).max() == top
    for i, row in enumerate(g):
        f0 = math.floor(metrics.CRIT_CENTRES[i] / (fs / 2) * H)
        assert int(np.argmax(row)) == f0 and abs(row[f0] - 70.0 / metrics.CRIT_BANDWIDTHS[i]) <= 1e-12
        nz = np.flatnonzero(row)
        assert len(nz) == nz[-1] - nz[0] + 1 and 3 <= len(nz) <= 48          # one run of a few dozen bins at the most
        # (70 / bandwidth_i) exp(-11 d^2) clears the threshold exactly where 11 d^2 < ln(70 / bandwidth_i) + 30 / 4.606
        bw = metrics.CRIT_BANDWIDTHS[i] / (fs / 2) * H
        reach = bw * math.sqrt((30 / (2 * 2.303) + math.log(70.0 / metrics.CRIT_BANDWIDTHS[i])) / 11)
        d = np.abs(np.arange(H) - f0)
        assert (row[d < reach - 1e-6] > 0).all() and (row[d > reach + 1e-6] == 0).all()
    first, offset, weights = metrics.compact_bank(g)
    assert first.dtype == offset.dtype == np.int32 and first.shape == (25,) and offset.shape == (26,) and offset[0] == 0
    dense = np.zeros_like(g)
    for i in range(25):
        dense[i, first[i]:first[i] + offset[i + 1] - offset[i]] = weights[offset[i]:offset[i + 1]]
    assert np.array_equal(dense, g) and (weights > 0).all()


# ---- the peak search ------------------------------------------------------------------------------------------------------------

def _expect_peaks(e, index):
    e = np.asarray(e, dtype=np.float64)
    assert e.shape == (25,) and len(index) == 24
    got = metrics._nearest_peaks(e[None, :])
    assert got.shape == (1, 24) and np.array_equal(got[0], e[list(index)]), (got[0], e[list(index)])


def test_peak_search_on_hand_made_profiles():
    up = np.arange(25.0)
    _expect_peaks(up, [23] * 24)                             # rising to the end: n stops at 24, the band below it (as published)
    _expect_peaks(up[::-1], [0] * 24)                        # falling from the start: n runs down to -1
    _expect_peaks(-np.abs(np.arange(25.0) - 10), [9] * 10 + [10] * 14)      # one peak at band 10: the rising side gets band 9
    plateau = np.array([0, 1, 2, 3, 4, 5, 5, 5, 5] + list(np.arange(4.0, -12.0, -1.0)))
    _expect_peaks(plateau, [4] * 5 + [5] * 19)               # a slope of 0 counts as falling
    _expect_peaks(np.full(25, -100.0), [0] * 24)             # silence
    both = metrics._nearest_peaks(np.stack([up, up[::-1]]))  # the vectorised form, rows independent
    assert np.array_equal(both[0], np.full(24, 23.0)) and np.array_equal(both[1], np.full(24, 24.0))


def test_wss_weights_of_a_single_peak():
    e = -2.0 * np.abs(np.arange(25.0) - 10)
    W = metrics._wss_weights(e[None, :])[0]
    peak = np.where(np.arange(24) < 10, e[9], e[10])
    assert np.allclose(W, 20.0 / (20.0 - e[:24]) / (1.0 + peak - e[:24]), rtol=1e-15, atol=0)
    assert W[10] == 1.0 and (W > 0).all() and (W <= 1.0).all()


# ---- defining properties --------------------------------------------------------------------------------------------------------

def test_identical_signals():
    x, _ = _pair(6000, 10, 3)
    assert metrics.spectral_measures(x, x, 16000) == {'wss': 0.0, 'fwssnr': 35.0}


@pytest.mark.parametrize('gain', [0.25, 4.0])
def test_a_common_gain_changes_nothing(gain):
    x, y = _pair(6000, 10, 4)
    a, b = metrics.spectral_measures(x, y, 16000), metrics.spectral_measures(gain * x, gain * y, 16000)
    assert abs(a['wss'] - b['wss']) <= 1e-9 * a['wss'] and abs(a['fwssnr'] - b['fwssnr']) <= 1e-9
    assert 0.0 < a['wss'] and -10.0 < a['fwssnr'] < 35.0
    c = metrics.spectral_measures(x, gain * y, 16000)         # fwSegSNR normalises each spectrum; the slopes ignore a gain too
    assert abs(a['wss'] - c['wss']) <= 1e-9 * a['wss'] and abs(a['fwssnr'] - c['fwssnr']) <= 1e-9


def test_more_noise_scores_worse():
    scores = [metrics.spectral_measures(*_pair(16000, snr, 5), 16000) for snr in (20, 10, 0)]
    assert scores[0]['wss'] < scores[1]['wss'] < scores[2]['wss']
    assert scores[0]['fwssnr'] > scores[1]['fwssnr'] > scores[2]['fwssnr']


def test_fwssnr_clamps_from_both_sides():
    t = np.arange(8000) / 16000.0
    high, low = np.sin(2 * np.pi * 3000 * t), np.sin(2 * np.pi * 300 * t)
    _, fw, valid = metrics.spectral_frame_values(high, low, 16000)
    assert valid.all() and (fw == -10.0).all() and metrics.fwssnr(high, low, 16000) == -10.0
    x, y = _pair(8000, 10, 6)
    _, fw, valid = metrics.spectral_frame_values(x, 1.05 * x, 16000)        # equal after the normalisation: err = EPS
    assert valid.all() and (fw == 35.0).all()
    _, fw, _ = metrics.spectral_frame_values(x, y, 16000)
    assert (fw > -10.0).all() and (fw < 35.0).all()                         # and between them otherwise


# ---- the trimmed mean, ties, silence ----------------------------------------------------------------------------------------------

def test_tied_frames_return_the_common_value():
    """Every frame of a 120-periodic recording is the same frame (the hop is 120): all values tie."""
    rng = np.random.default_rng(7)
    x = np.tile(rng.standard_normal(120), 40)
    y = x + np.tile(0.3 * rng.standard_normal(120), 40)
    wss, fw, valid = metrics.spectral_frame_values(x, y, 16000)
    assert len(wss) == 36 and valid.all() and metrics.trimmed_count(36) == 34
    m = metrics.spectral_measures(x, y, 16000)
    assert np.ptp(wss) <= 1e-9 * wss[0] and abs(m['wss'] - wss[0]) <= 1e-9 * wss[0] and wss[0] > 0
    assert np.ptp(fw) <= 1e-9 and abs(m['fwssnr'] - fw[0]) <= 1e-9
    assert metrics._trimmed_mean(np.array([2.0] * 19 + [7.0])) == 2.0        # K = 19 of 20: the tie fills it
    assert metrics._trimmed_mean(np.array([7.0] + [2.0] * 9)) == 2.5         # K = 10 of 10


def test_a_zero_head():
    x, y = _pair(8000, 10, 8)
    x[:2000], y[:2000] = 0.0, 0.0
    wss, fw, valid = metrics.spectral_frame_values(x, y, 16000)
    silent = 120 * np.arange(len(wss)) + 480 <= 2000
    assert silent.sum() == 13 and not valid[silent].any() and valid[~silent].all()
    assert np.isfinite(wss).all() and (wss[silent] == 0.0).all() and (wss[~silent] > 0).all()
    m = metrics.spectral_measures(x, y, 16000)
    K = metrics.trimmed_count(len(wss))                       # of ALL frames: the silent ones are among the smallest
    assert abs(m['wss'] - np.sort(wss)[:K].sum() / K) <= 1e-12 * m['wss']
    assert abs(m['fwssnr'] - fw[~silent].mean()) <= 1e-12     # the silent frames are left out
    z = np.zeros(3000)
    m = metrics.spectral_measures(z, z, 16000)
    assert m['wss'] == 0.0 and math.isnan(m['fwssnr'])
    m = metrics.spectral_measures(x[2000:5000], z, 16000)     # a silent estimate: no valid frame, a finite slope distance
    assert math.isnan(m['fwssnr']) and np.isfinite(m['wss']) and m['wss'] > 0


# ---- the composite measures -------------------------------------------------------------------------------------------------------

def test_composite_measures():
    m = metrics.composite_measures(2.5, 0.5, 30.0, 5.0)
    assert m['csig'] == pytest.approx(3.093 - 0.5145 + 1.5075 - 0.27) == pytest.approx(3.816)
    assert m['cbak'] == pytest.approx(1.634 + 1.195 - 0.21 + 0.315) == pytest.approx(2.934)
    assert m['covl'] == pytest.approx(1.594 + 2.0125 - 0.256 - 0.21) == pytest.approx(3.1405)
    pesq, llr = np.array([2.5, 4.5, 1.0]), np.array([0.5, 0.0, 2.0])
    wss, ssnr = np.array([30.0, 0.0, 120.0]), np.array([5.0, 35.0, -10.0])
    a = metrics.composite_measures(pesq, llr, wss, ssnr)
    assert sorted(a) == ['cbak', 'covl', 'csig'] and all(v.dtype == np.float64 and v.shape == (3,) for v in a.values())
    for k, want in (('csig', [3.816, 5.0, 1.0]), ('cbak', [2.934, 5.0, 1.0]), ('covl', [3.1405, 5.0, 1.0])):
        assert np.allclose(a[k], want, rtol=0, atol=1e-12), k
    t = metrics.composite_measures(*(torch.from_numpy(v) for v in (pesq, llr, wss, ssnr)))
    for k in a:
        assert isinstance(t[k], torch.Tensor) and t[k].dtype == torch.float64 and np.allclose(t[k].numpy(), a[k], rtol=0, atol=1e-12)
    t32 = metrics.composite_measures(*(torch.from_numpy(v).float() for v in (pesq, llr, wss, ssnr)))
    assert t32['csig'].dtype == torch.float32 and np.allclose(t32['csig'].numpy(), a['csig'], rtol=0, atol=1e-5)


# ---- the scorer's summary and the tool (host side) ----------------------------------------------------------------------------------

BASE_KEYS = ['files', 'stoi', 'stoi_nan', 'stoi_noisy', 'stoi_noisy_nan', 'sisnr', 'sisnr_nan', 'sisnr_noisy', 'sisnr_noisy_nan',
             'stoi_improvement', 'sisnr_improvement']


def test_summarise_with_and_without_the_spectral_keys():
    from dcsnet.evaluate import RecordingScorer, summarise
    nan = float('nan')
    base = {'stoi': torch.tensor([0.5, 0.7]), 'stoi_noisy': torch.tensor([0.4, 0.5]),
            'sisnr': torch.tensor([10.0, 14.0]), 'sisnr_noisy': torch.tensor([5.0, 5.0])}
    frame = {'ssnr': torch.tensor([8.0, 6.0]), 'ssnr_noisy': torch.tensor([2.0, 4.0]), 'llr': torch.tensor([0.4, nan]),
             'llr_noisy': torch.tensor([0.9, 1.0]), 'cd': torch.tensor([3.0, 4.0]), 'cd_noisy': torch.tensor([5.0, 7.0])}
    more = {'wss': torch.tensor([20.0, 30.0]), 'wss_noisy': torch.tensor([50.0, 40.0]), 'fwssnr': torch.tensor([12.0, nan]),
            'fwssnr_noisy': torch.tensor([7.0, 6.0])}
    assert RecordingScorer.SPECTRAL_MEASURES == ('wss', 'wss_noisy', 'fwssnr', 'fwssnr_noisy')
    s0, t0 = summarise(base)
    assert list(s0) == BASE_KEYS and t0.shape == (2, 4)       # what it returns today, key for key
    assert s0['files'] == 2 and s0['stoi'] == pytest.approx(0.6) and s0['sisnr_improvement'] == pytest.approx(7.0)
    assert s0['stoi_improvement'] == pytest.approx(0.15) and s0['sisnr_noisy_nan'] == 0
    s1, t1 = summarise(dict(base, **{k: v for k, v in more.items() if k != 'fwssnr_noisy'}))      # not all of the new keys
    assert s1 == s0 and np.array_equal(t1, t0)
    sf, tf = summarise(dict(base, **frame))
    assert tf.shape == (2, 10) and 'wss' not in sf and 'wss_improvement' not in sf
    s, t = summarise(dict(base, **more))
    assert t.shape == (2, 8) and np.array_equal(t[:, :4], t0)
    assert all(s[k] == v for k, v in s0.items())              # nothing that was there moves
    assert s['wss'] == pytest.approx(25.0) and s['wss_improvement'] == pytest.approx(20.0)      # noisy - enhanced
    assert s['fwssnr_improvement'] == pytest.approx(5.0) and s['fwssnr_nan'] == 1 and s['wss_nan'] == 0
    s2, t2 = summarise(dict(base, **frame, **more))
    assert t2.shape == (2, 14) and np.array_equal(t2[:, :10], tf, equal_nan=True) and np.array_equal(t2[:, 10:], t[:, 4:], equal_nan=True)
    assert all(s2[k] == v or (v != v and s2[k] != s2[k]) for k, v in sf.items()) and s2['wss_improvement'] == s['wss_improvement']


def test_scorer_attribute_names_the_keys():
    from dcsnet.enhance import Enhancer
    from dcsnet.evaluate import RecordingScorer
    enh = Enhancer.__new__(Enhancer)
    scorer = RecordingScorer(enh)
    assert scorer.spectral_measures is False and scorer.metrics == RecordingScorer.METRICS
    scorer.spectral_measures = True
    assert scorer.metrics == RecordingScorer.METRICS + RecordingScorer.SPECTRAL_MEASURES
    scorer.frame_measures = True
    assert scorer.metrics == RecordingScorer.METRICS + RecordingScorer.FRAME_MEASURES + RecordingScorer.SPECTRAL_MEASURES
    scorer = RecordingScorer(enh, extended=True)
    scorer.spectral_measures = True
    assert scorer.metrics == RecordingScorer.METRICS + RecordingScorer.EXTENDED + RecordingScorer.SPECTRAL_MEASURES


def _evaluate_tool():
    spec = importlib.util.spec_from_file_location('dcs_tools_evaluate', os.path.join(REPO, 'tools', 'evaluate.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_pesq_csv_parsing_and_the_composite_columns(tmp_path):
    tool = _evaluate_tool()
    names = ['a.wav', 'b.wav', 'c.WAV']
    one = tmp_path / 'one.csv'
    one.write_text('name,pesq\n# a comment\nb.wav, 3.5\n\na,2.5\nc.WAV,1.0\nextra.wav,4.0\n')
    pesq = tool.read_pesq_csv(str(one), names)
    assert pesq.dtype == np.float64 and pesq.tolist() == [[2.5], [3.5], [1.0]]
    two = tmp_path / 'two.csv'
    two.write_text('a.wav,2.5,1.5\nb.wav,3.5,2.0\nc.wav,1.0,1.0\n')
    pesq2 = tool.read_pesq_csv(str(two), names)
    assert pesq2.tolist() == [[2.5, 1.5], [3.5, 2.0], [1.0, 1.0]]
    with pytest.raises(SystemExit) as err:
        tool.read_pesq_csv(str(two), names + ['d.wav'])
    assert 'd.wav' in str(err.value)                          # the missing file is named
    for text in ('a.wav,2.5\nb.wav,3.5,2.0\nc.wav,1.0\n', 'a.wav,high\nb.wav,1\nc.wav,1\n', 'a.wav\n'):
        bad = tmp_path / 'bad.csv'
        bad.write_text(text)
        with pytest.raises(SystemExit):
            tool.read_pesq_csv(str(bad), names)
    for text in ('a.wav,2.5\nb.wav,3.5\nc.wav,1.0\na.WAV,2.0\n', 'a.wav,2.5\nb.wav,3.5\nc.wav,1.0\nb,3.5\n'):
        twice = tmp_path / 'twice.csv'
        twice.write_text(text)
        with pytest.raises(SystemExit) as err:                # two lines for one file, with or without .wav
            tool.read_pesq_csv(str(twice), names)
        assert 'twice.csv:4' in str(err.value)
    keys = ('stoi', 'ssnr', 'ssnr_noisy', 'llr', 'llr_noisy', 'wss', 'wss_noisy')
    table = np.array([[0.9, 5.0, 1.0, 0.5, 1.0, 30.0, 60.0],
                      [0.8, 35.0, 2.0, 0.0, 1.5, 0.0, 70.0],
                      [0.7, 4.0, 3.0, np.nan, 0.8, 20.0, 50.0]], dtype=np.float32)
    summary, wide, wide_keys = tool.add_composites({'files': 3}, table, keys, pesq)
    assert wide_keys == keys + ('csig', 'cbak', 'covl') and wide.shape == (3, 10) and np.array_equal(wide[:, :7], table, equal_nan=True)
    assert wide[0, 7:].tolist() == pytest.approx([3.816, 2.934, 3.1405], abs=1e-6)
    assert np.isnan(wide[2, 7]) and not np.isnan(wide[2, 8]) and np.isnan(wide[2, 9])      # no LLR: no CSIG, no COVL
    assert summary['files'] == 3 and summary['csig_nan'] == 1 and summary['cbak_nan'] == 0
    assert summary['csig'] == pytest.approx((3.816 + min(5.0, 3.093 + 0.603 * 3.5)) / 2)
    none, _, _ = tool.add_composites({'files': 3}, np.full_like(table, np.nan), keys, pesq)
    assert math.isnan(none['csig']) and math.isnan(none['covl']) and none['cbak_nan'] == 3      # no score is not a score of 0
    summary2, wide2, keys2 = tool.add_composites({'files': 3}, table, keys, pesq2)
    assert keys2 == keys + ('csig', 'cbak', 'covl', 'csig_noisy', 'cbak_noisy', 'covl_noisy') and wide2.shape == (3, 13)
    want = metrics.composite_measures(pesq2[:, 1], table[:, 4].astype(np.float64), table[:, 6].astype(np.float64),
                                      table[:, 2].astype(np.float64))
    assert np.allclose(wide2[:, 10], want['csig'], atol=1e-6) and summary2['covl_noisy'] == pytest.approx(float(want['covl'].mean()))
