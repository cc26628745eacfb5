"""GPU: the extended STOI (ESTOI) on the device — csrc/stoi_common.h::score_frames_ext through dcs_stoi_ext_f32 /
dcs_stoi_ext_ragged_f32, ops.stoi / ops.stoi_ragged(extended=...), metrics.stoi_batch / stoi_ragged(extended=...) and
RecordingScorer(enhancer, extended=True) — against its numerics contract, the host function metrics.stoi(..., extended=True).

The bound against the host is the project's STOI tolerance, 1e-4 (exactly 1e-5 where the host says so): both scores come from the
same single fp32 stage, the spectrum, and every statistic behind it is fp64 on both sides.  Everything else is bit for bit: 'both'
against the separate calls, ragged against batched, a permutation of the recordings, a graph replay against the eager call.  The
signal generators are those of tests/test_stoi_device.py."""
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
    for i, L in enumerate(lengths):
        for _ in range(50):
            x = _speech(rng, L, fs, pause_fracs[i % len(pause_fracs)])
            if _threshold_margin(x, fs) > 0.05:
                break
        assert _threshold_margin(x, fs) > 0.05, 'could not draw a recording away from the keep threshold'
        noise = rng.standard_normal(L)
        noise *= np.linalg.norm(x) / (np.linalg.norm(noise) * 10 ** (snrs[i % len(snrs)] / 20))
        clean.append(x)
        est.append((x + noise).astype(np.float32))
    return clean, est


def _flat(recs, dev):
    """-> (flat device buffer, int64 offsets on the device, the offsets on the host)."""
    buf, off = flat(recs, dev)
    return buf, off, off.cpu().numpy()


def _host_e(clean, est, fs):
    return np.array([metrics.stoi(c.astype(float), e.astype(float), fs, extended=True) for c, e in zip(clean, est)])


def _check_against_host(e, want):
    """Exactly float32(1e-5) where the host says 1e-5, else within 1e-4.  -> the largest |device - host| over the scored rows."""
    worst = 0.0
    for i, (got, w) in enumerate(zip(e, want)):
        if w == 1e-5:
            assert got == np.float32(1e-5), (i, got)
        else:
            worst = max(worst, abs(float(got) - w))
            assert abs(float(got) - w) <= 1e-4, (i, got, w)
    return worst


# ---- 1. batched against the host ------------------------------------------------------------------------------------------

def test_estoi_batch_matches_host_validation_shape(dev):
    """B = 8 utterances of 8160 samples at 16 kHz (the validation crop), SNRs -10 .. 30 dB; rows 3 and 7 are half pause, which
    leaves fewer than 30 STFT frames: exactly 1e-5.  Measured max |device - host| over the other rows on an MI355X: 8.3e-7
    (printed below; DESIGN.md §6e records it)."""
    B, L, fs = 8, 8160, 16000
    clean, est = _make_set((L,) * B, fs, 0, (0.0, 0.05, 0.0, 0.5), (-10, -5, 0, 5, 10, 20, 30))
    want = _host_e(clean, est, fs)
    assert list(want == 1e-5) == [False, False, False, True] * 2 and (np.abs(want[want != 1e-5]) > 0.05).all(), want
    c, e = torch.from_numpy(np.stack(clean)).to(dev), torch.from_numpy(np.stack(est)).to(dev)
    c10, e10 = (ops.resample_poly(v, *metrics.resample_taps(fs, dev)) for v in (c, e))
    got, kept = ops.stoi(c10, e10, extended=True)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B,) and kept.dtype == torch.int32
    assert kept.cpu().tolist() == [_host_kept(x, fs) for x in clean]
    worst = _check_against_host(got.cpu().numpy(), want)
    print(f'[estoi] max |device - host| over {int((want != 1e-5).sum())} rows of 8160 samples: {worst:.3e}')
    assert torch.equal(metrics.stoi_batch(c, e, fs, extended=True), got)


# ---- 2. the segment edges ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('L,frames', [(4096, 29), (4224, 30), (4352, 31)])
def test_estoi_at_the_frame_count_edges(dev, L, frames):
    """A stationary signal at 10 kHz, nothing removed: 29 STFT frames (exactly 1e-5), 30 (one segment), 31 (two)."""
    rng = np.random.default_rng(9 + L)
    x = rng.standard_normal(L).astype(np.float32)
    y = (x + 0.5 * rng.standard_normal(L)).astype(np.float32)
    want = _host_e([x], [y], metrics.FS)
    assert _host_kept(x, metrics.FS) == frames + 1 and (want[0] == 1e-5) == (frames < 30)
    e, kept = ops.stoi(torch.from_numpy(x[None]).to(dev), torch.from_numpy(y[None]).to(dev), extended=True)
    assert kept.cpu().tolist() == [frames + 1]
    _check_against_host(e.cpu().numpy(), want)
    c, off, _ = _flat([x], dev)
    er, keptr = ops.stoi_ragged(c, torch.from_numpy(y).to(dev), off, L, extended=True)
    assert torch.equal(er, e) and torch.equal(keptr, kept)


# ---- 3. about as many segments as threads, and more ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('L,pause,many', [(64000, 0.125, False), (80000, 0.1, True)])
def test_estoi_with_more_segments_than_threads(dev, L, pause, many):
    """One 4 s recording at 16 kHz with a 0.5 s pause, so that the kept frames differ from the frames: 273 of 311 frames kept,
    243 segments, nearly every thread of the score workgroup has one.  The same at 5 s: 351 kept, 321 segments, so threads
    0 .. 64 take two (t and t + 256) and the others one."""
    fs = 16000
    clean, est = _make_set((L,), fs, 33 + many, (pause,), (5,))
    kept_h = _host_kept(clean[0], fs)
    frames = -(-(metrics.resample_oct(clean[0].astype(float), metrics.FS, fs).size - 256) // 128)
    assert kept_h < frames - 20 and (kept_h - 30 > 256) == many, (kept_h, frames)
    want = _host_e(clean, est, fs)
    c, e = torch.from_numpy(clean[0][None]).to(dev), torch.from_numpy(est[0][None]).to(dev)
    got = metrics.stoi_batch(c, e, fs, extended=True)
    worst = _check_against_host(got.cpu().numpy(), want)
    print(f'[estoi] |device - host| of a {L // fs} s recording ({kept_h - 30} segments): {worst:.3e}')
    assert torch.equal(metrics.stoi_ragged(c[0], e[0], [0, L], fs, extended=True), got)


# ---- 4, 5. 'both' against the separate calls; ragged against batched ----------------------------------------------------------

RAGGED_SECONDS = (1.0, 0.3, 4.0, 0.42)


@pytest.mark.parametrize('fs', [16000, 48000])
def test_estoi_ragged_equals_batched_and_both_equals_the_separate_calls(dev, fs):
    """Recordings of 1 s, 0.3 s (fewer than 30 frames: 1e-5), 4 s and 0.42 s (one or two segments) in one ragged call: each e is
    what stoi_batch(extended=True) makes of the recording alone; 'both' returns the default call's d and the extended call's e;
    kept is the same in all three; reversing the recordings permutes the scores and changes no bit."""
    lengths = [int(s * fs) for s in RAGGED_SECONDS]
    clean, est = _make_set(lengths, fs, fs + 5, (0.0, 0.0, 0.1, 0.0), (0, 10, 5, 15))
    c, off, off_h = _flat(clean, dev)
    e, _, _ = _flat(est, dev)
    longest = max(lengths)
    d0 = metrics.stoi_ragged(c, e, off, fs, longest=longest)
    e1 = metrics.stoi_ragged(c, e, off, fs, longest=longest, extended=True)
    d2, e2 = metrics.stoi_ragged(c, e, off, fs, longest=longest, extended='both')
    assert torch.equal(d2, d0) and torch.equal(e2, e1)
    assert e1[1] == np.float32(1e-5) and bool((e1[[0, 2, 3]] > 0.05).all()), e1
    h, up, down = metrics.resample_taps(fs, dev)
    c10, off10 = ops.resample_poly_ragged(c, off, h, up, down)
    e10, _ = ops.resample_poly_ragged(e, off, h, up, down)
    long10 = -(-longest * up // down)
    _, k0 = ops.stoi_ragged(c10, e10, off10, long10)
    _, k1 = ops.stoi_ragged(c10, e10, off10, long10, extended=True)
    dd, ee, k2 = ops.stoi_ragged(c10, e10, off10, long10, extended='both')
    assert torch.equal(k0, k1) and torch.equal(k0, k2) and torch.equal(dd, d0) and torch.equal(ee, e1)
    for i, (a, b) in enumerate(zip(off_h[:-1], off_h[1:])):
        ci, ei = c[a:b][None], e[a:b][None]
        assert torch.equal(metrics.stoi_batch(ci, ei, fs, extended=True), e1[i:i + 1]), i
        db, eb = metrics.stoi_batch(ci, ei, fs, extended='both')
        assert torch.equal(db, metrics.stoi_batch(ci, ei, fs)) and torch.equal(db, d0[i:i + 1]) and torch.equal(eb, e1[i:i + 1]), i
    cr, offr, _ = _flat(clean[::-1], dev)
    er, _, _ = _flat(est[::-1], dev)
    dr, err = metrics.stoi_ragged(cr, er, offr, fs, longest=longest, extended='both')
    assert torch.equal(err.flip(0), e1) and torch.equal(dr.flip(0), d0)
    _check_against_host(e1.cpu().numpy(), _host_e(clean, est, fs))


def test_estoi_batch_both_equals_the_separate_calls(dev):
    fs = 16000
    clean, est = _make_set((8160,) * 4, fs, 44, (0.0, 0.5), (0, 10, 20))
    c, e = torch.from_numpy(np.stack(clean)).to(dev), torch.from_numpy(np.stack(est)).to(dev)
    d0, e1 = metrics.stoi_batch(c, e, fs), metrics.stoi_batch(c, e, fs, extended=True)
    d2, e2 = metrics.stoi_batch(c, e, fs, extended='both')
    assert torch.equal(d2, d0) and torch.equal(e2, e1)
    c10, e10 = (ops.resample_poly(v, *metrics.resample_taps(fs, dev)) for v in (c, e))
    (_, k0), (_, k1), (_, _, k2) = ops.stoi(c10, e10), ops.stoi(c10, e10, extended=True), ops.stoi(c10, e10, extended='both')
    assert torch.equal(k0, k1) and torch.equal(k0, k2)
    assert e1[1] == np.float32(1e-5) and e1[3] == np.float32(1e-5) and d0[1] == np.float32(1e-5)


# ---- 6. NaN -----------------------------------------------------------------------------------------------------------------

def test_a_nan_sample_makes_that_recordings_estoi_nan_only(dev):
    fs = metrics.FS
    clean, est = _make_set((6000, 9000, 5000), fs, 55, (0.0,), (5, 0, 10))
    c, off, off_h = _flat(clean, dev)
    e, _, _ = _flat(est, dev)
    ok = metrics.stoi_ragged(c, e, off, fs, longest=9000, extended=True)
    e[off_h[1] + 4321] = float('nan')
    bad = metrics.stoi_ragged(c, e, off, fs, longest=9000, extended=True)
    assert bool(torch.isnan(bad[1])) and torch.equal(bad[[0, 2]], ok[[0, 2]]) and bool(torch.isfinite(ok).all())
    assert np.isnan(metrics.stoi(clean[1].astype(float), e[off_h[1]:off_h[2]].cpu().numpy().astype(float), fs, extended=True))


# ---- 7. capture -------------------------------------------------------------------------------------------------------------

def test_estoi_ragged_graph_capture(dev):
    """stoi_ragged(extended='both') with device offsets, captured over static buffers and replayed on new contents, equals the
    eager call on those contents bit for bit: it reads nothing back and does not sync (a capture would fail otherwise)."""
    fs, lengths = 16000, (8160, 3000, 20000)
    clean, est = _make_set(lengths, fs, 66, (0.0, 0.0, 0.05), (0, 10, 20))
    clean2, est2 = _make_set(lengths, fs, 67, (0.05, 0.0, 0.0), (15, 5, -5))
    sc, off, _ = _flat(clean, dev)
    se, _, _ = _flat(est, dev)
    longest = max(lengths)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        metrics.stoi_ragged(sc, se, off, fs, longest=longest, extended='both')     # warm-up: tables and workspace exist
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_d, out_e = metrics.stoi_ragged(sc, se, off, fs, longest=longest, extended='both')
    c2, _, _ = _flat(clean2, dev)
    e2, _, _ = _flat(est2, dev)
    sc.copy_(c2)
    se.copy_(e2)
    g.replay()
    torch.cuda.synchronize()
    eager_d, eager_e = metrics.stoi_ragged(c2, e2, off, fs, longest=longest, extended='both')
    assert torch.equal(out_d, eager_d) and torch.equal(out_e, eager_e)
    _check_against_host(out_e.cpu().numpy(), _host_e(clean2, est2, fs))


# ---- 8. the scorer ------------------------------------------------------------------------------------------------------------

T, O, S = 64, 16, 4
SCORER_LENGTHS = (28800, 45001, 72000)                        # 0.6, 0.94 and 1.5 s at 48 kHz


def _pairs48(seed):
    clean, noisy = _make_set(SCORER_LENGTHS, 48000, seed, (0.0,), (5, 0, 10))
    return [0.1 * a for a in noisy], [0.1 * a for a in clean]


def _check_extended_scorer(enh, dev):
    """RecordingScorer(enh, extended=True): the four old keys are what RecordingScorer(enh) returns on the same input, and
    estoi / estoi_noisy are metrics.stoi_ragged(extended=True) of the returned audio and of the resampled noisy input."""
    from dcsnet.audio_store import _as_float32
    from dcsnet.evaluate import RecordingScorer, summarise
    noisy, clean = _pairs48(77)
    rate = 48000
    plain = RecordingScorer(enh)
    ext = RecordingScorer(enh, extended=True)
    assert plain.metrics == RecordingScorer.METRICS == ('stoi', 'stoi_noisy', 'sisnr', 'sisnr_noisy')
    assert ext.metrics == RecordingScorer.METRICS + ('estoi', 'estoi_noisy')
    old = plain.score(noisy, clean, rate)
    scores, audio = ext.score(noisy, clean, rate, return_audio=True)
    assert tuple(old) == plain.metrics and tuple(scores) == ext.metrics
    for k in plain.metrics:
        assert torch.equal(scores[k], old[k]), k
    off_in = np.zeros(len(noisy) + 1, dtype=np.int64)
    np.cumsum([len(a) for a in noisy], out=off_in[1:])
    resampled = [ops.resample_sinc(torch.from_numpy(np.concatenate([_as_float32(a, 'wave') for a in side])).to(dev), rate, enh.sr,
                                   offsets=off_in) for side in (noisy, clean)]
    off = np.zeros(len(noisy) + 1, dtype=np.int64)
    np.cumsum([a.numel() for a in audio], out=off[1:])
    assert off[-1] == resampled[0].numel()
    want = {'estoi': metrics.stoi_ragged(resampled[1], torch.cat(audio), off, enh.sr, extended=True),
            'estoi_noisy': metrics.stoi_ragged(resampled[1], resampled[0], off, enh.sr, extended=True)}
    for k, v in want.items():
        assert scores[k].is_cuda and scores[k].dtype == torch.float32 and tuple(scores[k].shape) == (len(noisy),), k
        assert torch.equal(scores[k], v), (k, scores[k], v)
    assert bool((scores['estoi_noisy'] > 0.05).all()), scores['estoi_noisy']
    summary, table = summarise(scores)
    assert table.shape == (len(noisy), 6) and summary['estoi_noisy_nan'] == 0 and 'estoi_improvement' in summary


def test_extended_scorer_with_the_complex_network(dev):
    from dcsnet.config import config, hparams
    from dcsnet.c_network import C_NETWORK
    from dcsnet.enhance import Enhancer
    hp = dict(hparams)
    hp['dropout_conv'], hp['dropout_fc'] = 0.0, 0.0
    cnet = fill_state(C_NETWORK(config, hp, 3), 3).to(dev).eval()
    _check_extended_scorer(Enhancer(cnet, mode='dcs', segment_frames=T, overlap_frames=O, batch_segments=S), dev)


def test_extended_scorer_with_the_magnitude_enhancer(dev):
    from dcsnet.config import config, hparams
    from dcsnet.r_network import R_NETWORK
    from dcsnet.enhance import MagnitudeEnhancer
    hp = dict(hparams)
    hp['dropout_conv'], hp['dropout_fc'] = 0.0, 0.0
    rnet = fill_state_stream(R_NETWORK(config, hp, 3), 5).to(dev).eval()
    _check_extended_scorer(MagnitudeEnhancer(rnet, mode='drs', segment_frames=T, overlap_frames=O, batch_segments=S), dev)
