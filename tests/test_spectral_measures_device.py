"""GPU: weighted spectral slope and frequency-weighted segmental SNR of whole recordings on the device
(csrc/spectral_measures.hip through ops.spectral_measures_ragged, metrics.spectral_measures_ragged and the RecordingScorer) against
the host contract metrics.spectral_measures.

Tolerance: the rule of tests/test_frame_measures_device.py.  The device value lies within 2 float32 ulps of the host value plus
1e-9 absolute, and is NaN exactly where the host is NaN.  Both sides are fp64 until the final rounding to float32 (half an
ulp); before it they differ by the rounding of two different fp64 FFTs and the order of their fp64 sums.  It is not a fitted
number.  The generators assert on the host, before any device call, that in every frame and for both signals either the frame is
exact digital silence or every band slope has |s_i| > 1e-6 dB, and that both signals are silent in the same frames: no peak
search hinges on last bits (AR-shaped noise plus white noise satisfies it).  The scorer's enhanced side is the one signal no
generator makes: there the condition is asserted on the network's output before it is held to the host.

The largest observed differences go to spectral_measures_parity.json in $DCS_PARITY_DIR (default parity_out/, kept out of git); a
full run's file is committed as profiles/spectral_measures_parity.json."""
import numpy as np
import pytest
import torch

from dcsnet import _lib
from dcsnet import metrics
from dcsnet import ops

pytestmark = pytest.mark.gpu

from oracle.seeded_state import fill_state   # noqa: E402
from _ragged_helpers import ar_pair, check_against_host, flat, tied_pair   # noqa: E402

KEYS = ('wss', 'fwssnr')
LENGTHS_16K = (0, 1, 599, 600, 719, 720, 4800, 16000, 23457, 48007)      # 4800: the tied set; 23457: a 2000-sample zero head
SNRS = (0, 10, 20)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    _lib.load()
    return torch.device('cuda:0')


# ---- signals -------------------------------------------------------------------------------------------------------------------

def _assert_input_condition(x, y, fs):
    """Every frame is exact digital silence (both signals) or has every band slope |s_i| > 1e-6 dB for both.  -> the smallest
    slope of the sounding frames (inf without one)."""
    N, S, _ = metrics.frame_geometry(fs)
    F = metrics.frame_count(len(x), fs)
    if F == 0:
        return np.inf
    nfft = metrics.spectral_fft_size(fs)
    g = metrics.critical_band_bank(fs, nfft)
    idx = S * np.arange(F)[:, None] + np.arange(N)[None, :]
    w = metrics._measure_window(N)
    silent, smallest = None, np.inf
    for sig in (x, y):
        f = sig.astype(np.float64)[idx] * w
        spec = np.fft.rfft(f, n=nfft, axis=1)[:, :nfft // 2]
        e = 10.0 * np.log10(np.maximum((spec.real ** 2 + spec.imag ** 2) @ g.T, 1e-10))
        s = np.abs(np.diff(e, axis=1))
        zero = ~f.any(axis=1)
        assert (zero | (s > 1e-6).all(axis=1)).all(), 'a frame whose peak search hinges on last bits'
        assert silent is None or np.array_equal(silent, zero), 'silent in one signal only'
        silent = zero
        if (~zero).any():
            smallest = min(smallest, float(s[~zero].min()))
    return smallest


def _make_set(lengths, fs, seed):
    rng = np.random.default_rng(seed)
    clean, est, smallest = [], [], np.inf
    for i, L in enumerate(lengths):
        tied, head = fs == 16000 and L == 4800, 2000 if L == 23457 else 0
        x, y = tied_pair(rng) if tied else ar_pair(L, SNRS[i % 3], rng, zero_head=head)
        smallest = min(smallest, _assert_input_condition(x, y, fs))
        clean.append(x)
        est.append(y)
    print(f'[spectral_measures] fs {fs} seed {seed}: the smallest band slope of a sounding frame is {smallest:.3e} dB')
    host = [metrics.spectral_measures(x, y, fs) for x, y in zip(clean, est)]
    return clean, est, host


@pytest.fixture(scope='module')
def set16():
    return _make_set(LENGTHS_16K, 16000, 31)


def _score(clean, est, fs, dev):
    c, off = flat(clean, dev)
    e, _ = flat(est, dev)
    return metrics.spectral_measures_ragged(c, e, off, fs)


def _check_against_host(got, host, what):
    check_against_host(got, host, KEYS, 'spectral_measures', what, 'spectral_measures_parity.json')


# ---- 1. parity with the host contract ---------------------------------------------------------------------------------------

def test_ragged_set_at_16_khz_against_the_host_and_alone(dev, set16):
    clean, est, host = set16
    assert metrics.spectral_fft_size(16000) == 1024
    assert [np.isnan(m['wss']) for m in host] == [True] * 3 + [False] * 7          # 0, 1, 599 samples: no frame
    got = _score(clean, est, 16000, dev)
    _check_against_host(got, host, '16k')
    whole = {k: v.cpu().numpy() for k, v in got.items()}
    rev = {k: v.cpu().numpy()[::-1] for k, v in _score(clean[::-1], est[::-1], 16000, dev).items()}
    for k in KEYS:
        assert np.array_equal(whole[k].view(np.uint32), rev[k].view(np.uint32)), k
    for i, (x, y) in enumerate(zip(clean, est)):                                    # a recording alone: bit for bit
        alone = _score([x], [y], 16000, dev)
        for k in KEYS:
            assert np.array_equal(alone[k].cpu().numpy().view(np.uint32), whole[k][i:i + 1].view(np.uint32)), (i, k)


@pytest.mark.parametrize('fs, nfft, lengths, seed', [
    (8000, 512, (299, 300, 8000), 32),
    (22050, 2048, (826, 827, 11025), 33),                    # N + S = 662 + 165
    (48000, 4096, (1799, 1800, 24000), 36),
])
def test_the_other_transform_sizes_against_the_host(dev, fs, nfft, lengths, seed):
    N, S, _ = metrics.frame_geometry(fs)
    assert metrics.spectral_fft_size(fs) == nfft and lengths[1] == N + S
    clean, est, host = _make_set(lengths, fs, seed)
    assert np.isnan(host[0]['wss']) and not np.isnan(host[1]['wss']) and not np.isnan(host[2]['fwssnr'])
    _check_against_host(_score(clean, est, fs, dev), host, f'{fs}')


# ---- 2. capture -------------------------------------------------------------------------------------------------------------

def test_graph_capture(dev, set16):
    """One linear stream capture of the call (no forks), replayed twice on new contents, equals the eager result bit for bit."""
    clean, est, _ = set16
    clean2, est2, _ = _make_set(LENGTHS_16K, 16000, 34)
    c, off = flat(clean, dev)
    e, _ = flat(est, dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        metrics.spectral_measures_ragged(c, e, off, 16000)       # warm-up: the tables and the workspace exist
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = metrics.spectral_measures_ragged(c, e, off, 16000)
    c2, _ = flat(clean2, dev)
    e2, _ = flat(est2, dev)
    c.copy_(c2)
    e.copy_(e2)
    eager = metrics.spectral_measures_ragged(c2, e2, off, 16000)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(out[k].view(torch.int32), eager[k].view(torch.int32)), k


# ---- 3. the caller's buffers ------------------------------------------------------------------------------------------------

GUARD_F, GUARD_B = 12345.0, 0xA5


@pytest.mark.parametrize('offsets', [
    (0, 700, 5000, 20000),                                   # as they should be
    (0, 9000, 3000, 12000, 11000, 20000),                    # do not rise
    (-10 ** 12, -5, 700, 10 ** 12, 2 ** 62),                 # start before the buffers and run past them
])
def test_callers_out_and_workspace_with_guards(dev, offsets):
    total, fs = 20000, 16000
    x, y = ar_pair(total, 10, np.random.default_rng(35))
    well_formed = offsets[0] == 0 and list(offsets) == sorted(offsets)
    if well_formed:                                          # these spans are held to the host below
        for p, q in zip(offsets[:-1], offsets[1:]):
            _assert_input_condition(x[p:q], y[p:q], fs)
    c, e = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    off = torch.tensor(offsets, dtype=torch.int64, device=dev)
    n = len(offsets) - 1
    nbytes = ops.spectral_measures_workspace_bytes(n, total, fs)
    ws_all = torch.full((nbytes + 512,), GUARD_B, dtype=torch.uint8, device=dev)
    out_all = torch.full((2 * n + 3 * 64,), GUARD_F, dtype=torch.float32, device=dev)
    out = tuple(out_all[64 + i * (n + 64):64 + i * (n + 64) + n] for i in range(2))
    got = ops.spectral_measures_ragged(c, e, off, fs, out=out, workspace=ws_all[256:256 + nbytes])
    torch.cuda.synchronize()
    assert got[0].data_ptr() == out[0].data_ptr() and got[1].data_ptr() == out[1].data_ptr()
    assert bool((ws_all[:256] == GUARD_B).all()) and bool((ws_all[256 + nbytes:] == GUARD_B).all())
    mask = torch.ones_like(out_all, dtype=torch.bool)
    for i in range(2):
        mask[64 + i * (n + 64):64 + i * (n + 64) + n] = False
    assert bool((out_all[mask] == GUARD_F).all())
    wss, fw = (v.cpu().numpy() for v in got)
    assert (np.isnan(wss) | (wss >= 0.0)).all() and (np.isnan(fw) | ((fw >= -10.0) & (fw <= 35.0))).all()
    if well_formed:
        host = [metrics.spectral_measures(x[p:q], y[p:q], fs) for p, q in zip(offsets[:-1], offsets[1:])]
        _check_against_host(dict(zip(KEYS, got)), host, 'callers_buffers')


# ---- 4. argument errors, digital silence ------------------------------------------------------------------------------------

def test_argument_errors_and_digital_silence(dev):
    x = torch.zeros(2000)
    off = torch.tensor([0, 800, 2000])
    with pytest.raises(_lib.DcsHipError):
        metrics.spectral_measures_ragged(x, x, off, 16000)                          # CPU tensors
    xd = x.to(dev)
    with pytest.raises(_lib.DcsHipError):
        metrics.spectral_measures_ragged(xd, xd, off, 4000)
    with pytest.raises(_lib.DcsHipError):
        metrics.spectral_measures_ragged(xd, xd, off, 96000)
    with pytest.raises(ValueError):
        metrics.spectral_measures_ragged(xd, xd, [0, 800, 1999], 16000)            # host offsets are checked
    with pytest.raises(_lib.DcsHipError):
        ops.spectral_measures_ragged(xd, xd, off.to(dev), 16000, out=(torch.empty(2, device=dev),))
    with pytest.raises(_lib.DcsHipError):
        ops.spectral_measures_ragged(xd, xd, off.to(dev), 16000, workspace=torch.empty(16, dtype=torch.uint8, device=dev))
    got = metrics.spectral_measures_ragged(xd, xd, off, 16000)                      # digital silence
    host = metrics.spectral_measures(np.zeros(800), np.zeros(800), 16000)
    assert host['wss'] == 0.0 and np.isnan(host['fwssnr'])
    assert bool((got['wss'] == 0.0).all()) and bool(torch.isnan(got['fwssnr']).all())


# ---- 5. the scorer -------------------------------------------------------------------------------------------------------------

T, O, S = 64, 16, 4                                          # the segment geometry of tests/test_score_ragged.py
SCORER_LENGTHS = (1500, 2017, 7000, 20000)


def test_scorer_with_spectral_measures(dev):
    from dcsnet.config import config, hparams
    from dcsnet.c_network import C_NETWORK
    from dcsnet.enhance import Enhancer
    from dcsnet.evaluate import RecordingScorer, summarise
    hp = dict(hparams)
    hp['dropout_conv'], hp['dropout_fc'] = 0.0, 0.0
    net = fill_state(C_NETWORK(config, hp, 3), 3).to(dev).eval()
    enh = Enhancer(net, mode='dcs', segment_frames=T, overlap_frames=O, batch_segments=S, use_graph=False)
    rng = np.random.default_rng(41)
    clean, noisy = zip(*(ar_pair(L, snr, rng) for L, snr in zip(SCORER_LENGTHS, (5, 0, 10, 15))))
    clean, noisy = list(clean), list(noisy)

    plain = RecordingScorer(enh).score(noisy, clean, 16000)
    off_scorer = RecordingScorer(enh)
    assert off_scorer.spectral_measures is False
    off = off_scorer.score(noisy, clean, 16000)
    assert list(off) == list(plain) == ['stoi', 'stoi_noisy', 'sisnr', 'sisnr_noisy']
    s_plain, t_plain = summarise(plain)

    scorer = RecordingScorer(enh)
    scorer.spectral_measures = True
    scores, audio = scorer.score(noisy, clean, 16000, return_audio=True)
    assert list(scores) == list(scorer.metrics) == list(RecordingScorer.METRICS + RecordingScorer.SPECTRAL_MEASURES)
    for k in plain:
        assert torch.equal(scores[k].view(torch.int32), plain[k].view(torch.int32)), k
    offsets = np.zeros(len(audio) + 1, dtype=np.int64)
    np.cumsum([a.numel() for a in audio], out=offsets[1:])
    total = int(offsets[-1])
    c_buf, n_buf = scorer._clean[:total], enh._store[:total]
    want = metrics.spectral_measures_ragged(c_buf, torch.cat(audio), offsets, enh.sr)
    want_noisy = metrics.spectral_measures_ragged(c_buf, n_buf, offsets, enh.sr)
    for k in KEYS:
        assert scores[k].is_cuda and scores[k].dtype == torch.float32 and tuple(scores[k].shape) == (len(noisy),)
        assert torch.equal(scores[k].view(torch.int32), want[k].view(torch.int32)), k
        assert torch.equal(scores[k + '_noisy'].view(torch.int32), want_noisy[k].view(torch.int32)), k
    # the host agrees on the scorer's buffers, on both sides: the noisy side is the clean side plus white noise at a known SNR,
    # the enhanced side is what the seeded network makes of it; the input condition is asserted on each
    ch, nh, sh = c_buf.cpu().numpy(), n_buf.cpu().numpy(), torch.cat(audio).cpu().numpy()
    spans = list(zip(offsets[:-1], offsets[1:]))
    for side, suffix, what in ((nh, '_noisy', 'scorer_noisy'), (sh, '', 'scorer_enhanced')):
        smallest = min(_assert_input_condition(ch[p:q], side[p:q], enh.sr) for p, q in spans)
        print(f'[spectral_measures] {what}: the smallest band slope of a sounding frame is {smallest:.3e} dB')
        host = [metrics.spectral_measures(ch[p:q], side[p:q], enh.sr) for p, q in spans]
        _check_against_host({k: scores[k + suffix] for k in KEYS}, host, what)
    summary, table = summarise(scores)
    assert table.shape == (len(noisy), 8) and np.array_equal(table[:, :4].view(np.uint32), t_plain.view(np.uint32))
    assert all(summary[k] == v for k, v in s_plain.items())
    assert np.array_equal(table[:, 4], scores['wss'].cpu().numpy(), equal_nan=True)
    assert summary['wss_improvement'] == pytest.approx(float(np.nanmean(table[:, 5].astype(np.float64) - table[:, 4])))
    assert summary['fwssnr_improvement'] == pytest.approx(float(np.nanmean(table[:, 6].astype(np.float64) - table[:, 7])))
