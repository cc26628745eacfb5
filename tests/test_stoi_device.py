"""Batched STOI on the device (csrc/stoi.hip through ops.resample_poly / ops.stoi / metrics.stoi_batch) against its numerics
contract, the host function dcsnet/metrics.py::stoi, utterance by utterance; its properties; graph capture; the opt-in of
network_functions.calc_metric.  The CPU tests at the bottom check the C ABI's argument handling without a GPU."""
import ctypes
import sys

import numpy as np
import pytest
import torch

from dcsnet import _lib
from dcsnet import metrics
from dcsnet import ops


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    _lib.load()
    return torch.device('cuda:0')


def _host_kept(x, fs):
    """Frames the host's silent-frame removal keeps (clean signal x at fs)."""
    x = np.asarray(x, dtype=float)
    if fs != metrics.FS:
        x = metrics.resample_oct(x, metrics.FS, fs)
    xs, _ = metrics.remove_silent_frames(x, x, metrics.DYN_RANGE, metrics.N_FRAME, metrics.N_FRAME // 2)
    return (len(xs) - metrics.N_FRAME) // (metrics.N_FRAME // 2) + 1 if len(xs) else 0


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
    matters: with harmonics alone the clean bands above them hold nothing but spectral leakage, below the fp32 spectrum's
    rounding floor, and their correlations are noise in both precisions."""
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


def _make_batch(B, L, fs, seed, pause_fracs, snrs):
    """Clean / estimate float32 [B, L]; every clean frame's energy more than 0.05 dB away from the 40 dB threshold."""
    rng = np.random.default_rng(seed)
    clean, est = np.zeros((B, L), np.float32), np.zeros((B, L), np.float32)
    for i in range(B):
        for _ in range(50):
            x = _speech(rng, L, fs, pause_fracs[i % len(pause_fracs)])
            if _threshold_margin(x, fs) > 0.05:
                break
        else:
            raise AssertionError('could not draw an utterance away from the keep threshold')
        assert _threshold_margin(x, fs) > 0.05
        noise = rng.standard_normal(L)
        snr = snrs[i % len(snrs)]
        noise *= np.linalg.norm(x) / (np.linalg.norm(noise) * 10 ** (snr / 20))
        clean[i], est[i] = x, (x + noise).astype(np.float32)
    return clean, est


def _host(clean, est, fs):
    return np.array([metrics.stoi(c.astype(float), e.astype(float), fs) for c, e in zip(clean, est)])


def _device(clean, est, fs, dev):
    return metrics.stoi_batch(torch.from_numpy(clean).to(dev), torch.from_numpy(est).to(dev), fs).cpu().numpy()


@pytest.mark.gpu
def test_stoi_batch_matches_host_validation_shape(dev):
    """B = 32 utterances of 8160 samples at 16 kHz (the validation crop), SNRs -10 .. 30 dB; some with long pauses, whose host
    score is exactly 1e-5 (fewer than 30 STFT frames kept)."""
    B, L, fs = 32, 8160, 16000
    clean, est = _make_batch(B, L, fs, 0, (0.0, 0.05, 0.0, 0.5), (-10, -5, 0, 5, 10, 20, 30))
    want = _host(clean, est, fs)
    assert (want == 1e-5).sum() >= 4 and (want > 0.05).sum() >= 16, want
    d, kept = ops.stoi(*[ops.resample_poly(torch.from_numpy(a).to(dev), *metrics.resample_taps(fs, dev))
                                 for a in (clean, est)])
    d, kept = d.cpu().numpy(), kept.cpu().numpy()
    assert list(kept) == [_host_kept(c, fs) for c in clean]
    for i in range(B):
        if want[i] == 1e-5:
            assert d[i] == np.float32(1e-5), (i, d[i])
        else:
            assert abs(d[i] - want[i]) <= 1e-4, (i, d[i], want[i])
    got = _device(clean, est, fs, dev)
    assert np.array_equal(got, d)


@pytest.mark.gpu
@pytest.mark.parametrize('fs,L,B', [(10000, 9000, 2), (48000, 43200, 2), (16000, 64000, 2), (16000, 480000, 1)])
def test_stoi_batch_other_rates_and_lengths(dev, fs, L, B):
    """No resampling (10 kHz), 48 kHz, and long utterances (4 s and 30 s at 16 kHz)."""
    clean, est = _make_batch(B, L, fs, fs + L, (0.0, 0.2), (0, 15))
    want = _host(clean, est, fs)
    got = _device(clean, est, fs, dev)
    assert np.all(want > 0.05), want
    assert np.max(np.abs(got - want)) <= 1e-4, (got, want)


@pytest.mark.gpu
@pytest.mark.parametrize('fs,L', [(10000, 0), (10000, 100), (10000, 256), (10000, 257), (10000, 384), (10000, 385),
                                  (16000, 410), (16000, 615), (48000, 1229)])
def test_stoi_batch_short_signals(dev, fs, L):
    """Below one frame and at the frame boundaries (256, 257, 384 samples after resampling): the host's 1e-5 and kept counts."""
    rng = np.random.default_rng(L)
    clean = rng.standard_normal((2, L)).astype(np.float32)
    est = (clean + 0.5 * rng.standard_normal((2, L))).astype(np.float32)
    want = _host(clean, est, fs)
    assert np.all(want == 1e-5)
    x = torch.from_numpy(clean).to(dev)
    if fs != metrics.FS:
        x = ops.resample_poly(x, *metrics.resample_taps(fs, dev))
    d, kept = ops.stoi(x, x)
    assert np.all(d.cpu().numpy() == np.float32(1e-5))
    assert list(kept.cpu().numpy()) == [_host_kept(c, fs) for c in clean]
    assert np.all(_device(clean, est, fs, dev) == np.float32(1e-5))


@pytest.mark.gpu
@pytest.mark.parametrize('fs', [16000, 48000])
def test_resample_poly_matches_resample_oct(dev, fs):
    rng = np.random.default_rng(fs)
    L = fs // 2 + 7
    x = (rng.standard_normal((3, L)) * np.linspace(0.1, 2, L)).astype(np.float32)
    h, up, down = metrics.resample_taps(fs, dev)
    got = ops.resample_poly(torch.from_numpy(x).to(dev), h, up, down).cpu().numpy()
    for i in range(3):
        want = metrics.resample_oct(x[i].astype(float), metrics.FS, fs)
        assert got[i].shape == want.shape
        assert np.max(np.abs(got[i] - want)) <= 1e-6 * np.max(np.abs(x[i])), np.max(np.abs(got[i] - want))


@pytest.mark.gpu
def test_stoi_batch_properties(dev):
    """Identical signals score 1; the level of the estimate does not matter; all-zero inputs give the host's values; two runs
    are bit-identical."""
    fs = 16000
    clean, est = _make_batch(4, 16000, fs, 7, (0.0,), (0, 10))
    c, e = torch.from_numpy(clean).to(dev), torch.from_numpy(est).to(dev)
    same = metrics.stoi_batch(c, c, fs).cpu().numpy()
    assert np.all(np.abs(same - 1.0) <= 1e-5), same
    d = metrics.stoi_batch(c, e, fs).cpu().numpy()
    d37 = metrics.stoi_batch(c, 3.7 * e, fs).cpu().numpy()
    assert np.all(np.abs(d - d37) <= 1e-5), (d, d37)
    z = np.zeros_like(clean)
    for a, b in ((z, est), (clean, z), (z, z)):
        want = _host(a, b, fs)
        got = _device(a, b, fs, dev)
        assert np.all(np.abs(got - want) <= 1e-4), (got, want)
    runs = [metrics.stoi_batch(c, e, fs) for _ in range(2)]
    assert torch.equal(runs[0], runs[1])


@pytest.mark.gpu
def test_stoi_batch_graph_capture(dev):
    """A captured stoi_batch replayed on new inputs copied into its static buffers equals the eager result bit for bit (the op
    does no host read-back or sync: a capture would fail otherwise)."""
    fs = 16000
    clean, est = _make_batch(8, 8160, fs, 11, (0.0, 0.05), (0, 10, 20))
    clean2, est2 = _make_batch(8, 8160, fs, 12, (0.0, 0.5), (-5, 5, 25))
    sc, se = torch.from_numpy(clean).to(dev), torch.from_numpy(est).to(dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        metrics.stoi_batch(sc, se, fs)                          # warm-up: tables and workspace exist before the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = metrics.stoi_batch(sc, se, fs)
    sc.copy_(torch.from_numpy(clean2))
    se.copy_(torch.from_numpy(est2))
    g.replay()
    torch.cuda.synchronize()
    eager = metrics.stoi_batch(torch.from_numpy(clean2).to(dev), torch.from_numpy(est2).to(dev), fs)
    assert torch.equal(out, eager)
    assert np.max(np.abs(out.cpu().numpy() - _host(clean2, est2, fs))) <= 1e-4


@pytest.mark.gpu
def test_calc_metric_stoi_on_device_opt_in(dev):
    """val_batch_2_metric_loss on a C_NETWORK (B = 3, 'dcs'): with config.stoi_on_device the STOI average agrees with the host
    loop within 1e-4, and the losses and the returned audio are bit-identical: the opt-in touches nothing else."""
    from dcsnet import network_functions as nf
    from dcsnet.config import config, hparams
    from dcsnet.c_network import C_NETWORK
    from oracle.seeded_state import fill_state, seeded_input
    hp = dict(hparams)
    hp['dropout_conv'], hp['dropout_fc'] = 0.0, 0.0
    net = fill_state(C_NETWORK(config, hp, 0), 7).to(dev).eval()
    clean, noise = seeded_input(3, 256, 256, 1, 0.1), seeded_input(3, 256, 256, 2, 0.05)
    batch = (noise.to(dev), (clean + noise).to(dev), clean.to(dev))
    argv, flag = sys.argv, getattr(config, 'stoi_on_device', None)
    sys.argv = ['train.py', 'dcs', '0']
    outs = []
    try:
        for on in (False, True):
            config.stoi_on_device = on
            with torch.no_grad():
                outs.append(nf.val_batch_2_metric_loss(net, batch, 0, 'complex'))
    finally:
        sys.argv = argv
        config.stoi_on_device = flag
    host, device = outs
    assert len(host) == len(device)
    stoi_h, stoi_d = host[-6], device[-6]
    assert isinstance(stoi_d, float) and 0.0 < stoi_h < 1.0
    assert abs(stoi_h - stoi_d) <= 1e-4, (stoi_h, stoi_d)
    for i, (a, b) in enumerate(zip(host, device)):
        if i == len(host) - 6:
            continue
        if isinstance(a, torch.Tensor):
            assert torch.equal(a, b), i
        else:
            assert a == b or (a != a and b != b), (i, a, b)


# ---- CPU: argument handling of the C ABI and the Python layer ---------------------------------------------------------

def test_stoi_workspace_bytes_host_arithmetic():
    lib = _lib.load()
    for B, L in ((32, 5100), (1, 0), (1, 256), (4, 40000), (2, 300000)):
        assert lib.dcs_stoi_workspace_bytes(B, L) > 0, (B, L)
    for B, L in ((0, 5100), (-1, 5100), (1, -1), (40000, 5100)):
        assert lib.dcs_stoi_workspace_bytes(B, L) < 0, (B, L)


def test_stoi_entry_points_reject_null_pointers():
    lib = _lib.load()
    bad = -1                                                   # DCS_ERR_BADARG
    p = ctypes.c_void_p(16)                                    # never dereferenced: every call below fails validation first
    assert lib.dcs_resample_poly_f32(None, p, 1, 100, p, 5, 5, 8, None) == bad
    assert lib.dcs_resample_poly_f32(p, None, 1, 100, p, 5, 5, 8, None) == bad
    assert lib.dcs_resample_poly_f32(p, p, 1, 100, None, 5, 5, 8, None) == bad
    assert lib.dcs_resample_poly_f32(p, p, 1, 100, p, 4, 5, 8, None) == bad        # even tap count
    assert lib.dcs_resample_poly_f32(p, p, 0, 100, p, 5, 5, 8, None) == bad
    assert lib.dcs_resample_poly_f32(p, p, 1, 100, p, 5, 0, 8, None) == bad
    ws = lib.dcs_stoi_workspace_bytes(2, 5100)
    args = [p, p, 2, 5100, p, p, p, p, p, ws, None]
    for i in (0, 1, 4, 5, 6, 7, 8):
        a = list(args)
        a[i] = None
        assert lib.dcs_stoi_f32(*a) == bad, i
    a = list(args)
    a[9] = ws - 1
    assert lib.dcs_stoi_f32(*a) == -3                          # DCS_ERR_WORKSPACE
    a = list(args)
    a[2] = 0
    assert lib.dcs_stoi_f32(*a) == bad


def test_stoi_batch_rejects_cpu_tensors():
    x = torch.zeros(2, 8160)
    with pytest.raises(_lib.DcsHipError):
        metrics.stoi_batch(x, x, 16000)
    with pytest.raises(_lib.DcsHipError):
        ops.stoi(x, x)
    with pytest.raises(_lib.DcsHipError):
        ops.resample_poly(x, torch.ones(5), 5, 8)


def test_stoi_band_edges_are_thirdoct_rows():
    obm, _ = metrics.thirdoct(metrics.FS, metrics.NFFT, metrics.NUMBAND, metrics.MINFREQ)
    lo, hi = metrics.stoi_band_edges(torch.device('cpu')).numpy()
    want = np.zeros_like(obm)
    for i, (a, b) in enumerate(zip(lo, hi)):
        want[i, a:b] = 1
    assert np.array_equal(obm, want)
