"""GPU: scoring whole recordings of different lengths on the device (csrc/stoi_ragged.hip through ops.*_ragged,
metrics.stoi_ragged / sisnr_ragged and dcsnet/evaluate.py::RecordingScorer).

The ragged kernels share their device code with the batched ones (csrc/stoi_common.h), so a recording's resampling, kept count
and STOI are compared BIT FOR BIT with the batched calls on that recording alone; the host function metrics.stoi stays the
numerics contract (1e-4, exactly 1e-5 where it says so), as for stoi_batch in tests/test_stoi_device.py, whose signal generators
are repeated here.  SI-SNR is compared with an fp64 numpy evaluation of the reference's formula."""
import numpy as np
import pytest
import torch

from dcsnet import _lib
from dcsnet import metrics
from dcsnet import ops

pytestmark = pytest.mark.gpu

from oracle.seeded_state import fill_state, fill_state_stream   # noqa: E402
from _ragged_helpers import flat                                 # noqa: E402


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    _lib.load()
    return torch.device('cuda:0')


# ---- the signal generators of tests/test_stoi_device.py ---------------------------------------------------------------

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
    down, under a syllable-rate envelope, with pauses (-60 dB) covering about pause_frac of the signal."""
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


def _make_set(lengths, fs, seed, pause_fracs, snrs):
    """Clean / estimate recordings (lists of float32 arrays); every clean frame's energy more than 0.05 dB away from the 40 dB
    threshold, so that the keep decision cannot hinge on the last bits of a frame energy."""
    rng = np.random.default_rng(seed)
    clean, est = [], []
    for L, pause, snr in zip(lengths, pause_fracs, snrs):
        for _ in range(50):
            x = _speech(rng, L, fs, pause)
            if _threshold_margin(x, fs) > 0.05:
                break
        assert _threshold_margin(x, fs) > 0.05, 'could not draw a recording away from the keep threshold'
        noise = rng.standard_normal(L)
        noise *= np.linalg.norm(x) / (np.linalg.norm(noise) * 10 ** (snr / 20))
        clean.append(x)
        est.append((x + noise).astype(np.float32))
    return clean, est


def _flat(recs, dev):
    """-> (flat device buffer, int64 offsets on the device, the offsets on the host)."""
    buf, off = flat(recs, dev)
    return buf, off, off.cpu().numpy()


def _ragged_stoi(clean, est, off, longest, fs, dev):
    """(d, kept) through the ops: resample_poly_ragged (unless at 10 kHz) then stoi_ragged."""
    if fs != metrics.FS:
        h, up, down = metrics.resample_taps(fs, dev)
        clean, off10 = ops.resample_poly_ragged(clean, off, h, up, down)
        est, off10b = ops.resample_poly_ragged(est, off, h, up, down)
        assert torch.equal(off10, off10b)
        off, longest = off10, -(-longest * up // down)
    return ops.stoi_ragged(clean, est, off, longest)


# ---- 1. the ragged resampler --------------------------------------------------------------------------------------------

RESAMPLE_LENGTHS = (1, 255, 410, 615, 8160, 8161, 30001)


@pytest.mark.parametrize('fs', [16000, 48000])
def test_resample_poly_ragged_equals_each_recording_alone(dev, fs):
    """One sample, below / across the tap span, one over a block of 256 outputs, many blocks: every recording's output is
    what resample_poly makes of it alone, so no tap reaches into a neighbour; the offsets are the cumulated ceil(L up / down)."""
    rng = np.random.default_rng(fs)
    recs = [(rng.standard_normal(L) * np.linspace(0.5, 2, L)).astype(np.float32) for L in RESAMPLE_LENGTHS]
    x, off, _ = _flat(recs, dev)
    h, up, down = metrics.resample_taps(fs, dev)
    y, y_off = ops.resample_poly_ragged(x, off, h, up, down)
    want_off = np.zeros(len(recs) + 1, dtype=np.int64)
    np.cumsum([-(-L * up // down) for L in RESAMPLE_LENGTHS], out=want_off[1:])
    assert y_off.cpu().numpy().tolist() == want_off.tolist()
    assert y.numel() >= want_off[-1]
    for i, r in enumerate(recs):
        alone = ops.resample_poly(torch.from_numpy(r).to(dev), h, up, down)
        assert torch.equal(y[want_off[i]:want_off[i + 1]], alone), (i, len(r))
    assert not y[want_off[-1]:].any()                        # the slack of the upper-bound allocation stays zero


# ---- 2. ragged STOI against the batched kernels and the host ------------------------------------------------------------

STOI_LENGTHS = (100, 410, 615, 8160, 8161, 20000, 64000)
STOI_PAUSES = (0.0, 0.0, 0.0, 0.0, 0.5, 0.05, 0.2)
STOI_SNRS = (0, 10, 5, -5, 20, 15, 5)


@pytest.fixture(scope='module')
def stoi_set():
    """The 16 kHz set with its host scores and kept counts, computed once and left unchanged."""
    clean, est = _make_set(STOI_LENGTHS, 16000, 21, STOI_PAUSES, STOI_SNRS)
    host = np.array([metrics.stoi(c.astype(float), e.astype(float), 16000) for c, e in zip(clean, est)])
    kept = [_host_kept(c, 16000) for c in clean]
    return clean, est, host, kept


def _check_against_both_references(clean, est, host, host_kept, fs, dev):
    c, off, off_h = _flat(clean, dev)
    e, _, _ = _flat(est, dev)
    longest = max(len(r) for r in clean)
    d, kept = _ragged_stoi(c, e, off, longest, fs, dev)
    assert torch.equal(metrics.stoi_ragged(c, e, off, fs, longest=longest), d)
    assert torch.equal(metrics.stoi_ragged(c, e, off_h, fs), d)                      # host offsets: uploaded, longest derived
    for i, (a, b) in enumerate(zip(off_h[:-1], off_h[1:])):
        ci, ei = c[a:b].reshape(1, -1), e[a:b].reshape(1, -1)
        assert torch.equal(metrics.stoi_batch(ci, ei, fs), d[i:i + 1]), i
        if fs != metrics.FS:
            ci, ei = (ops.resample_poly(v, *metrics.resample_taps(fs, dev)) for v in (ci, ei))
        d1, k1 = ops.stoi(ci, ei)
        assert torch.equal(d1, d[i:i + 1]) and torch.equal(k1, kept[i:i + 1]), i
    d, kept = d.cpu().numpy(), kept.cpu().numpy()
    assert list(kept) == list(host_kept)
    for i in range(len(clean)):
        if host[i] == 1e-5:
            assert d[i] == np.float32(1e-5), (i, d[i])
        else:
            assert abs(d[i] - host[i]) <= 1e-4, (i, d[i], host[i])


def test_stoi_ragged_equals_the_batched_call_per_recording_and_the_host(dev, stoi_set):
    """Recordings below one frame (100 samples), around one and two frames after resampling (410, 615), the validation crop and
    one sample more, 1.25 s and 4 s, in ONE call; SNRs -5 .. 20 dB; the 8161-sample one is half pause (host: exactly 1e-5)."""
    clean, est, host, kept = stoi_set
    assert (host > 0.05).sum() >= 3 and (host == 1e-5).sum() >= 4, host
    _check_against_both_references(clean, est, host, kept, 16000, dev)


def test_stoi_ragged_at_the_internal_rate(dev):
    """10 kHz: nothing is resampled."""
    clean, est = _make_set((300, 5100, 12501), metrics.FS, 22, (0.0, 0.0, 0.2), (5, 0, 10))
    host = np.array([metrics.stoi(c.astype(float), e.astype(float), metrics.FS) for c, e in zip(clean, est)])
    assert host[0] == 1e-5 and (host[1:] > 0.05).all(), host
    _check_against_both_references(clean, est, host, [_host_kept(c, metrics.FS) for c in clean], metrics.FS, dev)


# ---- 3. no leakage between neighbours ------------------------------------------------------------------------------------

def test_a_recordings_score_does_not_depend_on_its_neighbours(dev, stoi_set):
    clean, est, _, _ = stoi_set
    c, off, off_h = _flat(clean, dev)
    e, _, _ = _flat(est, dev)
    longest = max(len(r) for r in clean)
    d0, k0 = _ragged_stoi(c, e, off, longest, 16000, dev)
    s0 = ops.sisnr_ragged(c, e, off)
    mid = 3                                                  # 8160 samples, between the 615- and the 8161-sample recordings
    other_c, other_e = _make_set((STOI_LENGTHS[mid],), 16000, 23, (0.0,), (12,))
    c2, e2 = c.clone(), e.clone()
    c2[off_h[mid]:off_h[mid + 1]] = torch.from_numpy(other_c[0]).to(dev)
    e2[off_h[mid]:off_h[mid + 1]] = torch.from_numpy(other_e[0]).to(dev)
    d1, k1 = _ragged_stoi(c2, e2, off, longest, 16000, dev)
    s1 = ops.sisnr_ragged(c2, e2, off)
    rest = [i for i in range(len(clean)) if i != mid]
    assert torch.equal(d0[rest], d1[rest]) and torch.equal(k0[rest], k1[rest]) and torch.equal(s0[rest], s1[rest])
    assert d0[mid] != d1[mid] and s0[mid] != s1[mid]         # and the rewritten one did change


# ---- 4. ragged SI-SNR ----------------------------------------------------------------------------------------------------

def _sisnr_fp64(clean, est, eps=1e-8):
    """The reference's SiSNR.__call__ (network_functions.py:30-42) for one recording, in fp64, without the batch mean."""
    c, e = clean.astype(np.float64), est.astype(np.float64)
    dot, norm = np.sum(e * c), np.sum(c * c)
    s_target = (dot * c) / (norm + eps)
    e_noise = e - s_target
    return 10 * np.log10(np.sum(s_target * s_target) / (np.sum(e_noise * e_noise) + eps) + eps)


def test_sisnr_ragged_matches_the_reference_formula_in_fp64(dev):
    """Lengths 1, 37, 8160 and 64001 (one element, less than a workgroup's stride, many strides, odd) x SNRs -10, 0, 20, 40 dB,
    and one recording whose estimate IS its clean signal (the formula's finite value: e_noise is only s_target's shortfall).
    Every sum on the device is fp64, so what remains is the rounding of the result to float32: half an ulp of a value below
    128 dB in magnitude, 3.8e-6 dB; the bound leaves a margin over that."""
    rng = np.random.default_rng(31)
    clean, est = [], []
    for L in (1, 37, 8160, 64001):
        for snr in (-10, 0, 20, 40):
            x = (0.1 * rng.standard_normal(L)).astype(np.float32)
            noise = rng.standard_normal(L)
            noise *= np.linalg.norm(x) / (np.linalg.norm(noise) * 10 ** (snr / 20))
            clean.append(x)
            est.append((x + noise).astype(np.float32))
    x = (0.1 * rng.standard_normal(8160)).astype(np.float32)
    clean.append(x)
    est.append(x.copy())
    want = np.array([_sisnr_fp64(c, e) for c, e in zip(clean, est)])
    assert np.isfinite(want).all() and np.abs(want).max() < 128 and want[-1] > 90, want
    c, off, off_h = _flat(clean, dev)
    e, _, _ = _flat(est, dev)
    got = metrics.sisnr_ragged(c, e, off)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(clean),)
    assert torch.equal(got, ops.sisnr_ragged(c, e, off)) and torch.equal(got, metrics.sisnr_ragged(c, e, off_h))
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    assert err.max() <= 2e-5, (err, want)


# ---- 5. capture ------------------------------------------------------------------------------------------------------------

def test_ragged_metrics_graph_capture(dev, stoi_set):
    """stoi_ragged + sisnr_ragged captured over static buffers and replayed on new contents (same offsets) equal the eager
    result on those contents bit for bit: neither reads anything back or syncs (a capture would fail otherwise)."""
    fs = 16000
    clean, est, _, _ = stoi_set
    clean2, est2 = _make_set(STOI_LENGTHS, fs, 24, STOI_PAUSES[::-1], STOI_SNRS[::-1])
    sc, off, _ = _flat(clean, dev)
    se, _, _ = _flat(est, dev)
    longest = max(STOI_LENGTHS)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        metrics.stoi_ragged(sc, se, off, fs, longest=longest)      # warm-up: tables and workspace exist before the capture
        metrics.sisnr_ragged(sc, se, off)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_d = metrics.stoi_ragged(sc, se, off, fs, longest=longest)
        out_s = metrics.sisnr_ragged(sc, se, off)
    c2, _, _ = _flat(clean2, dev)
    e2, _, _ = _flat(est2, dev)
    sc.copy_(c2)
    se.copy_(e2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_d, metrics.stoi_ragged(c2, e2, off, fs, longest=longest))
    assert torch.equal(out_s, metrics.sisnr_ragged(c2, e2, off))
    host = np.array([metrics.stoi(a.astype(float), b.astype(float), fs) for a, b in zip(clean2, est2)])
    assert np.max(np.abs(out_d.cpu().numpy() - host)) <= 1e-4


# ---- 6. the scorer, end to end ---------------------------------------------------------------------------------------------

T, O, S = 64, 16, 4
SCORER_LENGTHS = (1500, 2017, 7000, 20000)


def _pairs(lengths, fs, seed, int16=False):
    clean, noisy = _make_set(lengths, fs, seed, (0.0,) * len(lengths), (5, 0, 10, 15))
    if int16:
        return [np.round(a * (8000 / np.abs(a).max())).astype(np.int16) for a in noisy], \
               [np.round(a * (8000 / np.abs(a).max())).astype(np.int16) for a in clean]
    return [0.1 * a for a in noisy], [0.1 * a for a in clean]


@pytest.fixture(scope='module')
def cnet(dev):
    from dcsnet.config import config, hparams
    from dcsnet.c_network import C_NETWORK
    hp = dict(hparams)
    hp['dropout_conv'], hp['dropout_fc'] = 0.0, 0.0
    return fill_state(C_NETWORK(config, hp, 3), 3).to(dev).eval()


def _check_scorer(enh, noisy, clean, rate, dev):
    """score() against the ragged metrics applied to what the enhancer returns, to the resampled input, and to the clean
    recordings resampled the same way."""
    from dcsnet.audio_store import _as_float32
    from dcsnet.evaluate import RecordingScorer
    scores, audio = RecordingScorer(enh).score(noisy, clean, rate, return_audio=True)
    speech = enh(noisy, rate)
    assert len(audio) == len(speech) and all(torch.equal(a, b) for a, b in zip(audio, speech))
    off_in = np.zeros(len(noisy) + 1, dtype=np.int64)
    np.cumsum([len(a) for a in noisy], out=off_in[1:])
    resampled = [ops.resample_sinc(torch.from_numpy(np.concatenate([_as_float32(a, 'wave') for a in side])).to(dev), rate, enh.sr,
                                   offsets=off_in) for side in (noisy, clean)]
    off = np.zeros(len(noisy) + 1, dtype=np.int64)
    np.cumsum([s.numel() for s in speech], out=off[1:])
    assert off[-1] == resampled[0].numel()
    flat = torch.cat(speech)
    want = {'stoi': metrics.stoi_ragged(resampled[1], flat, off, enh.sr),
            'stoi_noisy': metrics.stoi_ragged(resampled[1], resampled[0], off, enh.sr),
            'sisnr': metrics.sisnr_ragged(resampled[1], flat, off),
            'sisnr_noisy': metrics.sisnr_ragged(resampled[1], resampled[0], off)}
    assert sorted(scores) == sorted(want)
    for k, v in want.items():
        assert scores[k].is_cuda and scores[k].dtype == torch.float32 and tuple(scores[k].shape) == (len(noisy),), k
        assert torch.equal(scores[k], v), (k, scores[k], v)
    return scores


@pytest.mark.parametrize('use_graph', [True, False])
def test_scorer_equals_the_metrics_of_the_enhancers_output(dev, cnet, use_graph):
    """Recordings shorter than a segment, one sample over one, several segments and more than one batch of segments, at 16 kHz;
    then int16 input at 48 kHz through the same scorer's enhancer (its stores are reused)."""
    from dcsnet.enhance import Enhancer
    enh = Enhancer(cnet, mode='dcs', segment_frames=T, overlap_frames=O, batch_segments=S, use_graph=use_graph)
    noisy, clean = _pairs(SCORER_LENGTHS, 16000, 41)
    scores = _check_scorer(enh, noisy, clean, 16000, dev)
    assert bool(torch.isfinite(scores['sisnr']).all()) and bool((scores['stoi_noisy'][2:] > 0.05).all())
    noisy48, clean48 = _pairs((9001, 30000), 48000, 42, int16=True)
    _check_scorer(enh, noisy48, clean48, 48000, dev)


def test_scorer_with_the_magnitude_enhancer(dev):
    from dcsnet.config import config, hparams
    from dcsnet.r_network import R_NETWORK
    from dcsnet.enhance import MagnitudeEnhancer
    hp = dict(hparams)
    hp['dropout_conv'], hp['dropout_fc'] = 0.0, 0.0
    rnet = fill_state_stream(R_NETWORK(config, hp, 3), 5).to(dev).eval()
    enh = MagnitudeEnhancer(rnet, mode='drs', segment_frames=T, overlap_frames=O, batch_segments=S)
    noisy, clean = _pairs(SCORER_LENGTHS, 16000, 41)
    _check_scorer(enh, noisy, clean, 16000, dev)
