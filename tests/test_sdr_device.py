"""GPU: the BSS-eval signal-to-distortion ratio of whole recordings on the device (csrc/sdr_ragged.hip through ops.sdr_ragged,
metrics.sdr_ragged and the RecordingScorer) against the host contract metrics.sdr.

Tolerance: the device value lies within 2 float32 ulps of the host value plus 1e-9 absolute, NaN and +inf in the same places.
Both sides are fp64 until the final rounding to float32 (half an ulp) and differ before it only by the order of their fp64 sums;
an error in the filter c enters the ratio of the two explicitly summed energies at second order only.  It is not a fitted number.
The generator asserts on the host that every recording (but the empty one and the exact +inf pair) has E_{K-1} / R[0] > 1e-9 and
an SDR below 80 dB, so no value hinges on last bits.

The largest observed differences go to sdr_parity.json in $DCS_PARITY_DIR (default parity_out/, kept out of git); a full run's
file is committed as profiles/sdr_parity.json."""
import numpy as np
import pytest
import torch

from dcsnet import _lib
from dcsnet import metrics
from dcsnet import ops

pytestmark = pytest.mark.gpu

from oracle.seeded_state import fill_state   # noqa: E402
from _ragged_helpers import ar_noise, ar_pair, flat, record   # noqa: E402

C = ops.SDR_CHUNK
LENGTHS = (0, 1, 513, 600, C - 1, C, C + 1, 16000, 23457, 48007, 5000)     # 1: the exact +inf pair; 23457: a 2000-sample zero
SNRS = (0, 10, 20)                                                          # head; the last one: a 3-tap colouring
TAPS = (512, 16)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    _lib.load()
    return torch.device('cuda:0')


# ---- signals -------------------------------------------------------------------------------------------------------------------

def _coloured_pair(L, snr_db, rng, colouring):
    """ar_pair with the clean signal passed through the taps `colouring` on the estimate's side."""
    x, v = ar_noise(L, snr_db, rng)
    return (0.1 * x).astype(np.float32), (0.1 * (np.convolve(x, colouring)[:L] + v)).astype(np.float32)


def _host(x, y, K):
    """metrics.sdr(x, y, K), asserting on the way that E_{K-1} / R[0] > 1e-9 and that the value lies below 80 dB."""
    R, D = metrics.sdr_correlations(x.astype(np.float64), y.astype(np.float64), K)
    c, E = metrics.toeplitz_levinson(R, D)
    assert E[K - 1] / R[0] > 1e-9, 'a recursion whose validity hinges on last bits'
    value = metrics.sdr_from_filter(x, y, c)
    assert value < 80.0, 'a near-exact fit'
    return value


def _make_set(seed):
    rng = np.random.default_rng(seed)
    clean, est = [], []
    for i, L in enumerate(LENGTHS):
        if L == 1:
            x, y = np.array([0.5], np.float32), np.array([0.25], np.float32)
        elif L == 5000:
            x, y = _coloured_pair(L, SNRS[i % 3], rng, [1.0, -0.6, 0.3])
        else:
            x, y = ar_pair(L, SNRS[i % 3], rng, zero_head=2000 if L == 23457 else 0)
        clean.append(x)
        est.append(y)
    return clean, est


@pytest.fixture(scope='module')
def the_set():
    clean, est = _make_set(51)
    host = {K: [_host(x, y, K) if len(x) > 1 else metrics.sdr(x, y, K) for x, y in zip(clean, est)] for K in TAPS}
    return clean, est, host


def _score(clean, est, dev, K=512, est2=None):
    c, off = flat(clean, dev)
    e, _ = flat(est, dev)
    return metrics.sdr_ragged(c, e, off, K, estimate2=None if est2 is None else flat(est2, dev)[0])


def _bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)).view(np.uint32)


def _check_against_host(got, host, what):
    """2 float32 ulps of the host value + 1e-9; NaN and +inf exactly where the host has them.  Prints and records the largest
    difference."""
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(host),)
    g, h = got.cpu().numpy(), np.array(host, dtype=np.float64)
    assert np.array_equal(np.isnan(g), np.isnan(h)), (what, g, h)
    assert np.array_equal(np.isposinf(g), np.isposinf(h)) and not np.isneginf(g).any() and not np.isneginf(h).any(), (what, g, h)
    ok = np.isfinite(h)
    diff = np.abs(g[ok].astype(np.float64) - h[ok])
    tol = 2.0 * np.spacing(np.abs(h[ok]).astype(np.float32)).astype(np.float64) + 1e-9
    worst = float(diff.max()) if ok.any() else 0.0
    ratio = float((diff / tol).max()) if ok.any() else 0.0
    print(f'[sdr] {what}: max |device - host| = {worst:.3e} dB, {ratio:.3f} of the tolerance')
    record('sdr_parity.json', (what,), {'max_abs_diff': worst, 'max_share_of_tolerance': ratio})
    assert (diff <= tol).all(), (what, g, h)


# ---- 1. parity with the host contract ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('K', TAPS)
def test_ragged_set_against_the_host(dev, the_set, K):
    clean, est, host = the_set
    h = host[K]
    assert np.isnan(h[0]) and h[1] == np.inf and np.isfinite(h[2:]).all()
    assert h[-1] > metrics.sdr(clean[-1], est[-1], 1) + 0.25  # the colouring: forgiven by the taps, not by one gain
    _check_against_host(_score(clean, est, dev, K), h, f'K{K}')


def test_two_estimates_in_one_call(dev, the_set):
    clean, est, host = the_set
    rng = np.random.default_rng(52)
    other = [(x + 0.05 * rng.standard_normal(len(x))).astype(np.float32) for x in clean]
    for K in TAPS:
        a, b = _score(clean, est, dev, K, est2=other)
        assert np.array_equal(_bits(a), _bits(_score(clean, est, dev, K))), K
        assert np.array_equal(_bits(b), _bits(_score(clean, other, dev, K))), K
    a, b = _score(clean, other, dev, est2=est)                # the two swapped
    assert np.array_equal(_bits(b), _bits(_score(clean, est, dev)))
    _check_against_host(b, host[512], 'second_estimate')


# ---- 2. independence, determinism, capture ------------------------------------------------------------------------------------

def test_a_recordings_value_does_not_depend_on_its_neighbours(dev, the_set):
    clean, est, _ = the_set
    whole = _bits(_score(clean, est, dev))
    assert np.array_equal(whole, _bits(_score(clean, est, dev)))                   # two runs
    assert np.array_equal(whole, _bits(_score(clean[::-1], est[::-1], dev))[::-1])
    for i, (x, y) in enumerate(zip(clean, est)):
        assert np.array_equal(_bits(_score([x], [y], dev)), whole[i:i + 1]), i
    short = _bits(_score(clean, est, dev, 16))
    for i in (3, 5, 9):
        assert np.array_equal(_bits(_score(clean[i:i + 1], est[i:i + 1], dev, 16)), short[i:i + 1]), i


def test_an_empty_recording_in_the_middle(dev, the_set):
    clean, est, _ = the_set
    pick = [3, 6, 8]
    c, e = [clean[i] for i in pick], [est[i] for i in pick]
    whole = _bits(_score(c, e, dev))
    empty = np.zeros(0, np.float32)
    got = _score(c[:1] + [empty] + c[1:2] + [empty, empty] + c[2:], e[:1] + [empty] + e[1:2] + [empty, empty] + e[2:], dev)
    g = got.cpu().numpy()
    assert np.isnan(g[[1, 3, 4]]).all()
    assert np.array_equal(_bits(g[[0, 2, 5]]), whole)


def test_graph_capture(dev, the_set):
    """One linear stream capture of both forms of the call (no forks), replayed twice on new contents, equals the eager
    results bit for bit."""
    clean, est, _ = the_set
    clean2, est2 = _make_set(53)
    c, off = flat(clean, dev)
    e, _ = flat(est, dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        metrics.sdr_ragged(c, e, off)                         # warm-up: the workspace exists
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        one = metrics.sdr_ragged(c, e, off)
        pair = metrics.sdr_ragged(c, e, off, 16, estimate2=c)
    c2, _ = flat(clean2, dev)
    e2, _ = flat(est2, dev)
    c.copy_(c2)
    e.copy_(e2)
    eager_one = metrics.sdr_ragged(c2, e2, off)
    eager_pair = metrics.sdr_ragged(c2, e2, off, 16, estimate2=c2)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(one), _bits(eager_one))
        assert np.array_equal(_bits(pair[0]), _bits(eager_pair[0])) and np.array_equal(_bits(pair[1]), _bits(eager_pair[1]))


# ---- 3. offsets that are wrong --------------------------------------------------------------------------------------------------

GUARD_F, GUARD_B = 12345.0, 0xA5


@pytest.mark.parametrize('offsets', [
    (0, 9000, 3000, 12000, 11000, 20000),                    # do not rise
    (0, 5000, 40000, 10 ** 12, 2 ** 62),                     # run past the buffers
    (-10 ** 12, -5, 700, 20000, 20000),                      # start before them
    (20000, 0),                                              # one recording, backwards
])
def test_bad_offsets_stay_inside_the_buffers(dev, offsets):
    total = 20000
    x, y = ar_pair(total, 10, np.random.default_rng(54))
    c, e = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    off = torch.tensor(offsets, dtype=torch.int64, device=dev)
    n = len(offsets) - 1
    nbytes = ops.sdr_workspace_bytes(n, total)
    ws_all = torch.full((nbytes + 512,), GUARD_B, dtype=torch.uint8, device=dev)
    out_all = torch.full((2 * n + 3 * 64,), GUARD_F, dtype=torch.float32, device=dev)
    out = tuple(out_all[64 + i * (n + 64):64 + i * (n + 64) + n] for i in range(2))
    got = ops.sdr_ragged(c, e, off, est2=c, out=out, workspace=ws_all[256:256 + nbytes])
    torch.cuda.synchronize()
    assert bool((ws_all[:256] == GUARD_B).all()) and bool((ws_all[256 + nbytes:] == GUARD_B).all())
    mask = torch.ones_like(out_all, dtype=torch.bool)
    for i in range(2):
        mask[64 + i * (n + 64):64 + i * (n + 64) + n] = False
    assert bool((out_all[mask] == GUARD_F).all())
    # every offset is moved into [0, total] and a span that does not rise is empty; where the moved offsets still rise, the
    # chunk slots do too, and every span is scored as the host scores it
    a = np.clip(np.array(offsets, dtype=np.float64), 0, total).astype(np.int64)
    first = got[0].cpu().numpy()
    for i, (p, q) in enumerate(zip(a[:-1], a[1:])):
        if q <= p:
            assert np.isnan(first[i]), (i, first)
    if (np.diff(a) >= 0).all():
        _check_against_host(got[0], [metrics.sdr(x[p:q], y[p:q]) for p, q in zip(a[:-1], a[1:])], f'bad_offsets_{offsets[1]}')


# ---- 4. argument errors --------------------------------------------------------------------------------------------------------

def test_argument_errors(dev):
    x = torch.zeros(2000)
    off = torch.tensor([0, 800, 2000])
    with pytest.raises(_lib.DcsHipError):
        metrics.sdr_ragged(x, x, off)                                                # CPU tensors
    xd = x.to(dev)
    for bad in ([0, 800, 1999], [1, 800, 2000], [0, 1200, 800, 2000], [2000]):       # host offsets are checked
        with pytest.raises(ValueError):
            metrics.sdr_ragged(xd, xd, bad)
    for K in (0, 513):
        with pytest.raises(_lib.DcsHipError):
            metrics.sdr_ragged(xd, xd, off, K)
    with pytest.raises(_lib.DcsHipError):
        ops.sdr_ragged(xd, xd, off.to(dev), out=tuple(torch.empty(2, device=dev) for _ in range(2)))       # 2 for 1
    with pytest.raises(_lib.DcsHipError):
        ops.sdr_ragged(xd, xd, off.to(dev), est2=xd[:-1])
    assert bool(torch.isnan(metrics.sdr_ragged(xd, xd, off)).all())                 # digital silence
    empty = torch.zeros(0, device=dev)
    a, b = metrics.sdr_ragged(empty, empty, [0, 0, 0], estimate2=empty)              # no sample at all
    assert bool(torch.isnan(a).all()) and bool(torch.isnan(b).all()) and a.numel() == 2


# ---- 5. the scorer -------------------------------------------------------------------------------------------------------------

T, O, S = 64, 16, 4                                          # the segment geometry of tests/test_frame_measures_device.py
SCORER_LENGTHS = (1500, 2017, 7000, 20000)


def test_scorer_with_sdr(dev):
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

    plain_scorer = RecordingScorer(enh)
    assert plain_scorer.sdr is False
    plain = plain_scorer.score(noisy, clean, 16000)
    assert list(plain) == ['stoi', 'stoi_noisy', 'sisnr', 'sisnr_noisy']             # the keys of a scorer without the attribute
    s_plain, t_plain = summarise(plain)

    scorer = RecordingScorer(enh)
    scorer.sdr = True
    scores, audio = scorer.score(noisy, clean, 16000, return_audio=True)
    assert list(scores) == list(scorer.metrics) == list(RecordingScorer.METRICS + RecordingScorer.SDR)
    for k in plain:
        assert torch.equal(scores[k].view(torch.int32), plain[k].view(torch.int32)), k
    offsets = np.zeros(len(audio) + 1, dtype=np.int64)
    np.cumsum([a.numel() for a in audio], out=offsets[1:])
    total = int(offsets[-1])
    c_buf, n_buf = scorer._clean[:total], enh._store[:total]
    want = metrics.sdr_ragged(c_buf, torch.cat(audio), offsets)
    want_noisy = metrics.sdr_ragged(c_buf, n_buf, offsets)
    for k, w in (('sdr', want), ('sdr_noisy', want_noisy)):
        assert scores[k].is_cuda and scores[k].dtype == torch.float32 and tuple(scores[k].shape) == (len(noisy),)
        assert torch.equal(scores[k].view(torch.int32), w.view(torch.int32)), k
    # the noisy side is the clean side plus white noise at a known SNR: the host agrees on the scorer's buffers
    host = [metrics.sdr(c_buf[p:q].cpu().numpy(), n_buf[p:q].cpu().numpy()) for p, q in zip(offsets[:-1], offsets[1:])]
    _check_against_host(scores['sdr_noisy'], host, 'scorer_noisy')
    assert bool((scores['sdr_noisy'] >= scores['sisnr_noisy'] - 1e-3).all())        # the larger subspace
    summary, table = summarise(scores)
    assert table.shape == (len(noisy), 6) and np.array_equal(table[:, :4].view(np.uint32), t_plain.view(np.uint32))
    assert all(summary[k] == v for k, v in s_plain.items())
    assert np.array_equal(table[:, 4], scores['sdr'].cpu().numpy(), equal_nan=True)
    assert summary['sdr_improvement'] == pytest.approx(float(np.mean(table[:, 4].astype(np.float64) - table[:, 5])))
