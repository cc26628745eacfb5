"""GPU: segmental SNR, LLR and cepstrum distance of whole recordings on the device (csrc/frame_measures.hip through
ops.frame_measures_ragged, metrics.frame_measures_ragged and the RecordingScorer) against the host contract
metrics.frame_measures.

Tolerance: the device value lies within 2 float32 ulps of the host value plus 1e-9 absolute.  Both sides are fp64 until the
final rounding to float32 (half an ulp), and differ before it only by the order of their fp64 sums; the absolute term covers the
LLR of near-identical signals, log(1 + d) with d at fp64 rounding level.  It is not a fitted number.  The generators assert on
the host that every frame is either exact digital silence or has E_P / R[0] > 1e-9 for both signals, so no validity decision
hinges on last bits (AR-shaped noise plus white noise satisfies it; pure tones would not).

The largest observed differences go to frame_measures_parity.json in $DCS_PARITY_DIR (default parity_out/, kept out of git); a
full run's file is committed as profiles/frame_measures_parity.json."""
import numpy as np
import pytest
import torch

from dcsnet import _lib
from dcsnet import metrics
from dcsnet import ops

pytestmark = pytest.mark.gpu

from oracle.seeded_state import fill_state   # noqa: E402
from _ragged_helpers import ar_pair, check_against_host, flat, tied_pair   # noqa: E402

KEYS = ('ssnr', 'llr', 'cd')
LENGTHS_16K = (0, 1, 599, 600, 719, 720, 4800, 16000, 23457, 48007)      # 4800: the tied set; 23457: a 2000-sample zero head
SNRS = (0, 10, 20)
LENGTHS_8K = (479, 480, 8000)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    _lib.load()
    return torch.device('cuda:0')


# ---- signals -------------------------------------------------------------------------------------------------------------------

def _assert_input_condition(x, y, fs):
    """Every frame is exact digital silence (both signals) or has E_P / R[0] > 1e-9 for both."""
    N, S, P = metrics.frame_geometry(fs)
    F = metrics.frame_count(len(x), fs)
    if F == 0:
        return
    idx = S * np.arange(F)[:, None] + np.arange(N)[None, :]
    w = metrics._measure_window(N)
    silent = None
    for sig in (x, y):
        f = sig.astype(np.float64)[idx] * w
        R = metrics._autocorrelation(f, P)
        _, E = metrics._lpc(R, P)
        zero = ~f.any(axis=1)
        with np.errstate(all='ignore'):
            assert (zero | (E[:, P] / R[:, 0] > 1e-9)).all(), 'a frame whose validity hinges on last bits'
        assert silent is None or np.array_equal(silent, zero), 'silent in one signal only'
        silent = zero


def _make_set(lengths, fs, seed):
    rng = np.random.default_rng(seed)
    clean, est = [], []
    for i, L in enumerate(lengths):
        x, y = tied_pair(rng) if L == 4800 else ar_pair(L, SNRS[i % 3], rng, zero_head=2000 if L == 23457 else 0)
        _assert_input_condition(x, y, fs)
        clean.append(x)
        est.append(y)
    host = [metrics.frame_measures(x, y, fs) for x, y in zip(clean, est)]
    return clean, est, host


@pytest.fixture(scope='module')
def set16():
    return _make_set(LENGTHS_16K, 16000, 31)


def _score(clean, est, fs, dev):
    c, off = flat(clean, dev)
    e, _ = flat(est, dev)
    return metrics.frame_measures_ragged(c, e, off, fs)


def _check_against_host(got, host, what):
    check_against_host(got, host, KEYS, 'frame_measures', what, 'frame_measures_parity.json')


# ---- 1. parity with the host contract ---------------------------------------------------------------------------------------

def test_ragged_set_at_16_khz_against_the_host(dev, set16):
    clean, est, host = set16
    assert [np.isnan(m['ssnr']) for m in host] == [True] * 3 + [False] * 7        # 0, 1, 599 samples: no frame
    _check_against_host(_score(clean, est, 16000, dev), host, '16k')


def test_set_at_8_khz_against_the_host(dev):
    clean, est, host = _make_set(LENGTHS_8K, 8000, 32)
    assert metrics.frame_geometry(8000) == (240, 60, 10)
    assert all(not np.isnan(m['llr']) for m in host)
    _check_against_host(_score(clean, est, 8000, dev), host, '8k')


def test_one_long_frame_rate(dev):
    """48 kHz: N = 1440, the longest frame the kernel takes."""
    clean, est, host = _make_set((1799, 1800, 9001), 48000, 33)
    assert np.isnan(host[0]['ssnr']) and not np.isnan(host[1]['ssnr'])
    _check_against_host(_score(clean, est, 48000, dev), host, '48k')


# ---- 2. independence, determinism, capture ------------------------------------------------------------------------------------

def test_a_recordings_scores_do_not_depend_on_its_neighbours(dev, set16):
    clean, est, _ = set16
    whole = {k: v.cpu().numpy() for k, v in _score(clean, est, 16000, dev).items()}
    again = _score(clean, est, 16000, dev)
    rev = {k: v.cpu().numpy()[::-1] for k, v in _score(clean[::-1], est[::-1], 16000, dev).items()}
    for k in KEYS:
        assert np.array_equal(whole[k], again[k].cpu().numpy(), equal_nan=True), k      # two runs
        assert np.array_equal(whole[k].view(np.uint32), rev[k].view(np.uint32)), k
    for i, (x, y) in enumerate(zip(clean, est)):
        alone = _score([x], [y], 16000, dev)
        for k in KEYS:
            assert np.array_equal(alone[k].cpu().numpy().view(np.uint32), whole[k][i:i + 1].view(np.uint32)), (i, k)


def test_graph_capture(dev, set16):
    """One linear stream capture of the call (no forks), replayed twice on new contents, equals the eager result bit for bit."""
    clean, est, _ = set16
    clean2, est2, _ = _make_set(LENGTHS_16K, 16000, 34)
    c, off = flat(clean, dev)
    e, _ = flat(est, dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        metrics.frame_measures_ragged(c, e, off, 16000)          # warm-up: the window table and the workspace exist
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = metrics.frame_measures_ragged(c, e, off, 16000)
    c2, _ = flat(clean2, dev)
    e2, _ = flat(est2, dev)
    c.copy_(c2)
    e.copy_(e2)
    eager = metrics.frame_measures_ragged(c2, e2, off, 16000)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(out[k].view(torch.int32), eager[k].view(torch.int32)), k


# ---- 3. offsets that are wrong --------------------------------------------------------------------------------------------------

GUARD_F, GUARD_B = 12345.0, 0xA5


@pytest.mark.parametrize('offsets', [
    (0, 9000, 3000, 12000, 11000, 20000),                    # do not rise
    (0, 5000, 40000, 10 ** 12, 2 ** 62),                     # run past the buffers
    (-10 ** 12, -5, 700, 20000, 20000),                      # start before them
    (20000, 0),                                              # one recording, backwards
])
def test_bad_offsets_stay_inside_the_buffers(dev, offsets):
    total, fs = 20000, 16000
    rng = np.random.default_rng(35)
    x, y = ar_pair(total, 10, rng)
    c, e = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    off = torch.tensor(offsets, dtype=torch.int64, device=dev)
    n = len(offsets) - 1
    nbytes = ops.frame_measures_workspace_bytes(n, total, fs)
    ws_all = torch.full((nbytes + 512,), GUARD_B, dtype=torch.uint8, device=dev)
    out_all = torch.full((3 * n + 4 * 64,), GUARD_F, dtype=torch.float32, device=dev)
    out = tuple(out_all[64 + i * (n + 64):64 + i * (n + 64) + n] for i in range(3))
    got = ops.frame_measures_ragged(c, e, off, fs, out=out, workspace=ws_all[256:256 + nbytes])
    torch.cuda.synchronize()
    assert bool((ws_all[:256] == GUARD_B).all()) and bool((ws_all[256 + nbytes:] == GUARD_B).all())
    mask = torch.ones_like(out_all, dtype=torch.bool)
    for i in range(3):
        mask[64 + i * (n + 64):64 + i * (n + 64) + n] = False
    assert bool((out_all[mask] == GUARD_F).all())
    for v, (lo, hi) in zip(got, ((-10.0, 35.0), (0.0, 2.0), (0.0, 10.0))):
        v = v.cpu().numpy()
        assert (np.isnan(v) | ((v >= lo) & (v <= hi))).all(), v
    # what the clamping does: every offset is moved into [0, total], a span that does not rise is empty, and spans that overlap
    # share the total / S frame slots the workspace has: a recording keeps the frames that still fit behind its predecessors'
    a = np.clip(np.array(offsets, dtype=np.float64), 0, total).astype(np.int64)
    spans = [(p, max(p, q)) for p, q in zip(a[:-1], a[1:])]
    base = np.minimum(np.concatenate([[0], np.cumsum([metrics.frame_count(q - p, fs) for p, q in spans])]), total // 120)
    host = []
    for (p, q), frames in zip(spans, np.diff(base)):
        s, l, c, valid = (v[:frames] for v in metrics.frame_values(x[p:q], y[p:q], fs))
        host.append({'ssnr': float(np.mean(s)) if frames else float('nan'),
                     'llr': metrics._trimmed_mean(l[valid]), 'cd': metrics._trimmed_mean(c[valid])})
    _check_against_host(dict(zip(KEYS, got)), host, 'bad_offsets')


# ---- 4. argument errors --------------------------------------------------------------------------------------------------------

def test_argument_errors(dev):
    x = torch.zeros(2000)
    off = torch.tensor([0, 800, 2000])
    with pytest.raises(_lib.DcsHipError):
        metrics.frame_measures_ragged(x, x, off, 16000)                             # CPU tensors
    xd = x.to(dev)
    with pytest.raises(_lib.DcsHipError):
        metrics.frame_measures_ragged(xd, xd, off, 4000)
    with pytest.raises(_lib.DcsHipError):
        metrics.frame_measures_ragged(xd, xd, off, 96000)
    with pytest.raises(ValueError):
        metrics.frame_measures_ragged(xd, xd, [0, 800, 1999], 16000)               # host offsets are checked
    with pytest.raises(_lib.DcsHipError):
        ops.frame_measures_ragged(xd, xd, off.to(dev), 16000, window=torch.ones(480, device=dev))       # float32 window
    with pytest.raises(_lib.DcsHipError):
        ops.frame_measures_ragged(xd, xd, off.to(dev), 16000, out=tuple(torch.empty(2, device=dev) for _ in range(4)))  # 4 for 3
    got = metrics.frame_measures_ragged(xd, xd, off, 16000)                         # digital silence
    assert bool((got['ssnr'] == -10.0).all()) and bool(torch.isnan(got['llr']).all()) and bool(torch.isnan(got['cd']).all())


# ---- 5. the scorer -------------------------------------------------------------------------------------------------------------

T, O, S = 64, 16, 4                                          # the segment geometry of tests/test_score_ragged.py
SCORER_LENGTHS = (1500, 2017, 7000, 20000)


def test_scorer_with_frame_measures(dev):
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
    off_scorer.frame_measures = False
    off = off_scorer.score(noisy, clean, 16000)
    assert list(off) == list(plain) == ['stoi', 'stoi_noisy', 'sisnr', 'sisnr_noisy']
    for k in plain:
        assert torch.equal(off[k].view(torch.int32), plain[k].view(torch.int32)), k
    s_plain, t_plain = summarise(plain)
    s_off, t_off = summarise(off)
    assert s_plain == s_off and np.array_equal(t_plain.view(np.uint32), t_off.view(np.uint32))

    scorer = RecordingScorer(enh)
    scorer.frame_measures = True
    scores, audio = scorer.score(noisy, clean, 16000, return_audio=True)
    assert list(scores) == list(scorer.metrics) == list(RecordingScorer.METRICS + RecordingScorer.FRAME_MEASURES)
    for k in plain:
        assert torch.equal(scores[k].view(torch.int32), plain[k].view(torch.int32)), k
    offsets = np.zeros(len(audio) + 1, dtype=np.int64)
    np.cumsum([a.numel() for a in audio], out=offsets[1:])
    total = int(offsets[-1])
    c_buf, n_buf = scorer._clean[:total], enh._store[:total]
    want = metrics.frame_measures_ragged(c_buf, torch.cat(audio), offsets, enh.sr)
    want_noisy = metrics.frame_measures_ragged(c_buf, n_buf, offsets, enh.sr)
    for k in KEYS:
        assert scores[k].is_cuda and scores[k].dtype == torch.float32 and tuple(scores[k].shape) == (len(noisy),)
        assert torch.equal(scores[k].view(torch.int32), want[k].view(torch.int32)), k
        assert torch.equal(scores[k + '_noisy'].view(torch.int32), want_noisy[k].view(torch.int32)), k
    # the noisy side is the clean side plus white noise at a known SNR: the host agrees on the scorer's buffers
    host = [metrics.frame_measures(c_buf[p:q].cpu().numpy(), n_buf[p:q].cpu().numpy(), enh.sr) for p, q in zip(offsets[:-1], offsets[1:])]
    _check_against_host({k: scores[k + '_noisy'] for k in KEYS}, host, 'scorer_noisy')
    summary, table = summarise(scores)
    assert table.shape == (len(noisy), 10) and np.array_equal(table[:, :4].view(np.uint32), t_plain.view(np.uint32))
    assert all(summary[k] == v for k, v in s_plain.items())
    j = 4
    assert np.array_equal(table[:, j], scores['ssnr'].cpu().numpy(), equal_nan=True)
    imp = table[:, j].astype(np.float64) - table[:, j + 1]
    assert summary['ssnr_improvement'] == pytest.approx(float(imp[~np.isnan(imp)].mean()))
    assert 'llr_improvement' in summary and 'cd_improvement' in summary
    assert summary['llr_improvement'] == pytest.approx(float(np.nanmean(table[:, j + 3].astype(np.float64) - table[:, j + 2])))
