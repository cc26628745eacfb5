"""GPU: whole recordings through the Enhancer (dcsnet/enhance.py) — the two kernels of csrc/enhance.hip against the kernels
and the op chain they are built from, bit for bit where the arithmetic is the same, and the segment geometry end to end.

Tiny shapes: segments of 64 frames (2016 samples at hop 32) overlapping by 16, 4 segments per batch; recordings of 1500,
2016, 2017 and 7000 samples at 16 kHz (shorter than, exactly, one sample over one segment, five segments) and one int16
recording at 48 kHz.  Their content is a sum of tones on STFT bin centres under a smooth envelope: the front end drops the DC
bin (data.py:118), so only a signal without DC in any frame can come back from a pass-through exactly.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.seeded_state import fill_state   # noqa: E402

T, O, S, HOP = 64, 16, 4, 32
LS, STRIDE, OV = HOP * (T - 1), HOP * (T - O), HOP * (O - 1)
LENGTHS = (1500, 2016, 2017, 7000)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from dcsnet import _lib
    _lib.load()
    return torch.device('cuda:0')


def _tones(n, rate, seed):
    """Tones on bin centres k * 16000 / 512 Hz (k >= 40) under a sin^2 envelope over the whole recording, float64."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64)
    x = torch.zeros(n, dtype=torch.float64)
    for k in (40, 67, 101, 150, 203):
        x += 0.1 * torch.cos(2 * np.pi * k * (16000 / 512) * t / rate + float(torch.rand(1, generator=g)) * 6.28)
    return x * torch.sin(np.pi * (t + 0.5) / n) ** 2


@pytest.fixture(scope='module')
def waves16():
    return [_tones(n, 16000, n).float().numpy() for n in LENGTHS]


@pytest.fixture(scope='module')
def wave48():
    return torch.round(_tones(9001, 48000, 5) * 32768).to(torch.int16)


@pytest.fixture(scope='module')
def net(dev):
    from dcsnet.config import config, hparams
    from dcsnet.c_network import C_NETWORK
    hp = dict(hparams)
    hp['dropout_conv'], hp['dropout_fc'] = 0.0, 0.0
    return fill_state(C_NETWORK(config, hp, 3), 3).to(dev).eval()        # running statistics off their defaults


def _enhancer(net, **kw):
    from dcsnet.enhance import Enhancer
    return Enhancer(net, **dict(dict(mode='dcs', segment_frames=T, overlap_frames=O, batch_segments=S), **kw))


@pytest.fixture(scope='module')
def captured(net, waves16):
    """One captured run over the 16 kHz recordings, shared (and left unchanged) by the tests below."""
    enh = _enhancer(net, use_graph=True)
    plan, tables, noise, speech = enh.enhance_segments(waves16, 16000)
    return enh, plan, tables, noise, speech


def _store(recs, dev):
    off = np.zeros(len(recs) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in recs], out=off[1:])
    return torch.from_numpy(np.concatenate(recs)).to(dev), torch.from_numpy(off).to(dev), off


def _i32(a, dev):
    return torch.tensor(list(a), dtype=torch.int32, device=dev)


# ---------------------------------------------------------------------------------------------------------- planner (host)

def test_planner_geometry():
    from dcsnet.enhance import SegmentPlan
    lens = [1, 1500, 2016, 2017, 2016 + 1536, 2016 + 1537, 7000, 100000]
    p = SegmentPlan(lens, T, O, HOP, S)
    for i, n in enumerate(lens):
        k = 0
        while HOP * (T + k * (T - O) - 1) < n:               # the smallest n >= 0 with L_i >= len_i, by search
            k += 1
        assert p.n_seg[i] == k + 1 and p.frames[i] == T + k * (T - O)
        rows = slice(int(p.seg_first[i]), int(p.seg_first[i + 1]))
        assert (p.item[rows] == i).all() and list(p.first_frame[rows]) == [s * (T - O) for s in range(k + 1)]
    assert p.item.size == p.batches * S and p.item.size - p.rows < S
    assert (p.item[p.rows:] == -1).all() and (p.first_frame[p.rows:] == 0).all()
    assert list(p.offsets) == [0] + list(np.cumsum(lens))
    with pytest.raises(ValueError):
        SegmentPlan([10, 0], T, O, HOP, S)


# ------------------------------------------------------------------------------------------------ 1. segment STFT, bit for bit

@pytest.mark.parametrize('t_seg,o_seg', [(T, O), (20, 5)])               # (20: ragged tiles, 20 = 2 * 8 + 4)
def test_segment_stft_equals_the_whole_recordings_stft(dev, t_seg, o_seg):
    from dcsnet import ops
    from dcsnet.enhance import SegmentPlan
    g = torch.Generator().manual_seed(1)
    recs = [(0.3 * torch.randn(n, generator=g)).numpy() for n in LENGTHS + (257,)]
    store, off_d, off = _store(recs, dev)
    window = torch.hann_window(512).to(dev)
    scale = 512 ** -0.5
    p = SegmentPlan([len(r) for r in recs], t_seg, o_seg, HOP, S)
    bad = [(-1, 0), (len(recs), 0), (3, -1), (3, int(p.frames[3]) - t_seg + 1), (4, 1), (-7, 5)]
    item = _i32(list(p.item[:p.rows]) + [b[0] for b in bad], dev)
    frame = _i32(list(p.first_frame[:p.rows]) + [b[1] for b in bad], dev)
    got = ops.audio_stft_segments(store, off_d, item, frame, window, t_seg, o_seg, HOP, scale)
    assert got.shape == (p.rows + len(bad), 256, t_seg)
    for i in range(len(recs)):
        whole = ops.audio_stft_batch(store, store, off_d, _i32([i], dev), _i32([0], dev), window, int(p.frames[i]), HOP, scale)[1][0]
        for r in range(int(p.seg_first[i]), int(p.seg_first[i + 1])):
            f = int(p.first_frame[r])
            assert torch.equal(torch.view_as_real(got[r]), torch.view_as_real(whole[:, f:f + t_seg])), (i, r)
    assert float(got[:p.rows].abs().max()) > 0.1
    assert not torch.view_as_real(got[p.rows:]).any()                    # every row the table does not cover: zeros
    out = torch.full((2, 256, t_seg), 1 + 1j, dtype=torch.complex64, device=dev)
    assert ops.audio_stft_segments(store, off_d, _i32([-1, 4], dev), _i32([0, 0], dev), window, t_seg, o_seg, HOP, scale,
                                   out=out) is out
    assert not torch.view_as_real(out[0]).any() and torch.equal(out[1], got[int(p.seg_first[4])])


# ----------------------------------------------------------------------------------- 2. per-segment waveforms, bit for bit

def test_segment_waveforms_equal_the_unfused_chain_captured_and_eager(dev, net, waves16, captured):
    from dcsnet import ops, functional as F
    enh, plan, tables, noise, speech = captured
    assert plan.rows == 9 and plan.batches == 3
    store, off_d, _ = _store(waves16, dev)
    item, frame = _i32(plan.item, dev), _i32(plan.first_frame, dev)
    eps = net.hparams['atan2_eps']
    for b in range(plan.batches):
        rows = slice(b * S, (b + 1) * S)
        with torch.no_grad():
            Y = ops.audio_stft_segments(store, off_d, item[rows], frame[rows], enh.window, T, O, HOP, 512 ** -0.5)
            d = net(Y, bound=False)
            _, NS = F.bound2_mask_apply_pair_complex(Y, d, eps)
            want = F.polar_wave(NS.reshape(2 * S, 256, T), enh.window, enh.inv_env, 512, HOP, 512 ** 0.5, eps)
        assert torch.equal(noise[rows], want[:S]), b
        assert torch.equal(speech[rows], want[S:]), b
    assert float(speech[:plan.rows].abs().max()) > 1e-3
    eager = _enhancer(net, use_graph=False)
    _, _, noise_e, speech_e = eager.enhance_segments(waves16, 16000)
    assert eager._graph is None and enh._graph is not None
    assert torch.equal(noise_e, noise) and torch.equal(speech_e, speech)
    assert not net.training
    net.train()
    try:
        eager.enhance_segments(waves16[:1], 16000)
        assert net.training                                              # the training flag is restored
    finally:
        net.eval()


# -------------------------------------------------------------------------------------------------------------- 3. stitch

def test_stitch_copies_outside_overlaps_and_cross_fades_inside(dev, waves16, captured):
    from dcsnet import ops
    enh, plan, tables, noise, speech = captured
    flat, pcm = enh.stitch(plan, tables, speech, pcm=True)
    assert flat.shape == pcm.shape == (sum(LENGTHS),) and pcm.dtype == torch.int16
    assert torch.equal(pcm, torch.clamp(torch.round(flat * 32768), -32767, 32767).to(torch.int16))
    seg = speech.cpu().double().numpy()
    got = flat.cpu().numpy()
    faded = 0
    for i, n in enumerate(LENGTHS):
        assert n == ops.resample_sinc_length(n, 16000, 16000)
        y = got[int(plan.offsets[i]):int(plan.offsets[i + 1])]
        assert y.size == n
        m = np.arange(n)
        s = np.minimum(m // STRIDE, plan.n_seg[i] - 1)
        j = m - s * STRIDE
        r = int(plan.seg_first[i]) + s
        cur = seg[r, j]
        inside = (s > 0) & (j < OV)
        assert np.array_equal(y[~inside], cur[~inside].astype(np.float32)), i      # the one owner's sample, unchanged
        a = seg[r[inside] - 1, j[inside] + STRIDE]
        b = cur[inside]
        want = a + (j[inside] + 0.5) / OV * (b - a)                      # fp64
        assert (np.abs(y[inside] - want) <= 2.0 ** -21 * np.maximum(np.abs(a), np.abs(b))).all(), i
        faded += int(inside.sum())
    assert faded == (1 + 4) * OV
    # PCM clipping, and the float output of a call is this launch's
    loud = speech * 1000.0
    pcm = enh.stitch(plan, tables, loud, pcm=True)
    assert torch.equal(pcm[1], torch.clamp(torch.round(pcm[0] * 32768), -32767, 32767).to(torch.int16))
    assert int(pcm[1].max()) == 32767 and int(pcm[1].min()) == -32767
    out, out_noise = enh(waves16, 16000, return_noise=True)
    assert [o.numel() for o in out] == list(LENGTHS) and all(o.is_cuda and o.dtype == torch.float32 for o in out)
    assert torch.equal(torch.cat(out), flat) and torch.equal(torch.cat(out_noise), enh.stitch(plan, tables, noise))


# ---------------------------------------------------------------------------------------------------------- 4. end to end

def test_pass_through_returns_the_resampled_recordings(dev, net, waves16, wave48, monkeypatch):
    """The per-batch step replaced by a plain resynthesis of the noisy segments (the DC bin back in front): segmenting,
    padding, the table, the graph's static buffers and the stitch must then return every resampled recording.  5e-6: the
    bound of test_hip_backward.py::test_hip_istft_equals_torch_istft_and_its_gradient on STFT -> synthesis."""
    from dcsnet import ops
    want48 = ops.resample_sinc(wave48.to(dev).float() * (1.0 / 32768), 48000, 16000)
    assert want48.numel() == ops.resample_sinc_length(9001, 48000, 16000) == 3001
    for use_graph in (True, False):
        enh = _enhancer(net, use_graph=use_graph)

        def through(Y):
            X = torch.view_as_real(torch.nn.functional.pad(Y, (0, 0, 1, 0)).transpose(1, 2).contiguous())     # [S, T, 257, 2]
            w = ops.istft_ola(ops.irfft512(X), enh.window, enh.inv_env, HOP, 512 ** 0.5 / 512)
            return torch.cat((w, w))
        monkeypatch.setattr(enh, '_batch_step', through)
        speech, noise = enh(waves16, 16000, return_noise=True)
        for x, y, z in zip(waves16, speech, noise):
            assert y.shape == (len(x),)
            assert float((y.cpu() - torch.from_numpy(x)).abs().max()) < 5e-6
            assert torch.equal(y, z)
        (y48,) = enh([wave48], 48000)                                    # int16 at 48 kHz: resampled once on the device
        assert y48.shape == want48.shape and float((y48 - want48).abs().max()) < 5e-6
        assert float(want48.abs().max()) > 0.2


def test_a_recording_does_not_depend_on_its_batch_neighbours(dev, waves16, wave48, captured):
    """Alone and among the others, same batch_segments: in eval() every row of the batch is computed on its own, so only the
    row a segment lands in differs.  2e-4 absolute: test_hip_parity.py's bound on the network forward (the bounded mask, |M| < 1;
    the estimates are Y (.) M and Y - Y (.) M of signals below 1)."""
    enh = captured[0]
    among = enh(waves16, 16000)
    for i in (0, 3):
        (alone,) = enh([waves16[i]], 16000)
        assert alone.shape == among[i].shape
        assert float((alone - among[i]).abs().max()) <= 2e-4
        assert float(among[i].abs().max()) > 1e-3


def test_replay_after_the_envelope_and_window_caches_evicted(dev, waves16, captured):
    """The captured graph reads the Enhancer's own window and envelope and the cached values _derived.collect() handed it:
    pushing the envelope and the pack caches past their capacities (64, 512) takes nothing from under it."""
    from dcsnet import network_functions as nf, functional as F
    enh, plan, tables, noise, speech = captured
    assert enh._graph is not None
    graph = enh._graph
    window = torch.hann_window(512).to(dev)
    for t in range(70):
        nf._inv_envelope(window, 16 + 8 * t, HOP)
    assert len(nf._ENVELOPES) <= 64
    pairs = [(torch.full((2, 2, 1, 1), 1.0 + i, device=dev), torch.ones(2, 2, 1, 1, device=dev)) for i in range(520)]
    for w_r, w_i in pairs:                                               # (alive: an entry goes with its owner)
        F.packed_weight(w_r, w_i, None, None, False)
    assert len(F._PACKED) == 512
    _, _, noise2, speech2 = enh.enhance_segments(waves16, 16000)
    assert enh._graph is graph                                           # replayed, not captured again
    assert torch.equal(noise2, noise) and torch.equal(speech2, speech)


def test_mask_applying_mode(dev, net, waves16):
    """'dc': the mask is applied (speech = Y (.) M) through the unfused ops; there is no noise estimate."""
    from dcsnet import ops, functional as F
    enh = _enhancer(net, mode='dc', use_graph=False)
    plan, tables, noise, speech = enh.enhance_segments(waves16[:2], 16000)
    assert noise is None and plan.rows == 2
    store, off_d, _ = _store(waves16[:2], dev)
    with torch.no_grad():
        Y = ops.audio_stft_segments(store, off_d, _i32(plan.item, dev), _i32(plan.first_frame, dev), enh.window, T, O, HOP,
                                    512 ** -0.5)
        _, applied, _ = F.bound_mask_apply_complex(Y, net(Y), net.hparams['atan2_eps'])
        want = F.polar_wave(applied, enh.window, enh.inv_env, 512, HOP, 512 ** 0.5, net.hparams['atan2_eps'])
    assert torch.equal(speech, want)
    with pytest.raises(ValueError, match='no noise estimate'):
        enh(waves16[:1], 16000, return_noise=True)


def test_errors(dev, net, waves16):
    from dcsnet import ops, DcsHipError
    from dcsnet.config import config, hparams
    from dcsnet.c_network import C_NETWORK
    from dcsnet.r_network import R_NETWORK
    from dcsnet.enhance import Enhancer
    with pytest.raises(DcsHipError, match='R_NETWORK'):
        Enhancer(R_NETWORK(config, dict(hparams), 0).to(dev))
    with pytest.raises(DcsHipError, match='no CPU fallback'):
        Enhancer(C_NETWORK(config, dict(hparams), 0))
    with pytest.raises(ValueError, match='multiple of 8'):
        Enhancer(net, segment_frames=60, overlap_frames=16)
    for o in (1, T // 2 + 1):
        with pytest.raises(ValueError, match='overlap_frames'):
            Enhancer(net, segment_frames=T, overlap_frames=o)
    with pytest.raises(ValueError, match='mode'):
        Enhancer(net, mode='drs')
    enh = _enhancer(net, use_graph=False)
    with pytest.raises(ValueError, match='empty signal'):
        enh([waves16[0], np.zeros(0, dtype=np.float32)], 16000)
    bad = waves16[0].copy()
    bad[7] = np.inf
    with pytest.raises(ValueError, match='inf, neginf or nan'):
        enh([waves16[1], bad], 16000)
    with pytest.raises(TypeError):
        enh([waves16[0].astype(np.float64)], 16000)
    cpu = torch.zeros(4096)
    idx = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(DcsHipError, match='no CPU fallback'):
        ops.audio_stft_segments(cpu, torch.tensor([0, 4096]), idx, idx, torch.hann_window(512), T, O, HOP, 1.0)
    with pytest.raises(DcsHipError, match='no CPU fallback'):
        ops.segments_stitch(torch.zeros(1, LS), torch.tensor([0, 1], dtype=torch.int32), torch.tensor([0, 100]), 100, T, O, HOP)
    seg = torch.zeros(1, LS, device=dev)
    with pytest.raises(DcsHipError, match='overlap'):
        ops.segments_stitch(seg, _i32([0, 1], dev), torch.tensor([0, 100], device=dev), 100, T, T // 2 + 1, HOP)
