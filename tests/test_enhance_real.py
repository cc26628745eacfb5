"""GPU: whole recordings through the MagnitudeEnhancer (dcsnet/enhance.py) — the real twin (R_NETWORK: DRS-Net 'drs', DR-Net 'dr')
on the fused mask + synthesis node (F.rmask_apply_polar_wave).  Planner, segment STFT and stitch are the Enhancer's own and are
covered by tests/test_enhance.py; here: what the subclass adds, end to end.

The shapes of tests/test_enhance.py: segments of 64 frames (2016 samples at hop 32) overlapping by 16, 4 segments per batch;
recordings of 1500, 2016, 2017 and 7000 samples at 16 kHz whose content is a sum of tones on STFT bin centres under a smooth
envelope (the front end drops the DC bin, so only a signal without DC in any frame can come back from a pass-through).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.seeded_state import fill_state, fill_state_stream   # noqa: E402

T, O, S, HOP = 64, 16, 4, 32
LS = HOP * (T - 1)
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
def net(dev):
    from dcsnet.config import config, hparams
    from dcsnet.r_network import R_NETWORK
    hp = dict(hparams)
    hp['dropout_conv'], hp['dropout_fc'] = 0.0, 0.0
    return fill_state_stream(R_NETWORK(config, hp, 3), 5).to(dev).eval()         # running statistics off their defaults


def _enhancer(net, **kw):
    from dcsnet.enhance import MagnitudeEnhancer
    return MagnitudeEnhancer(net, **dict(dict(mode='drs', segment_frames=T, overlap_frames=O, batch_segments=S), **kw))


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


def _by_hand(net, enh, waves, plan, dev, pair):
    """The per-batch step spelled out on the same segments' STFT: |Y|, the raw forward, the fused node."""
    from dcsnet import ops, functional as F
    store, off_d, _ = _store(waves, dev)
    item, frame = _i32(plan.item, dev), _i32(plan.first_frame, dev)
    out = []
    for b in range(plan.batches):
        rows = slice(b * S, (b + 1) * S)
        with torch.no_grad():
            Y = ops.audio_stft_segments(store, off_d, item[rows], frame[rows], enh.window, T, O, HOP, 512 ** -0.5)
            d = net(ops.complex_abs(Y), sigmoid=False)
            out.append(F.rmask_apply_polar_wave(Y, d, enh.window, enh.inv_env, 512, HOP, 512 ** 0.5, net.hparams['atan2_eps'],
                                                pair=pair, want_mask=False)[1])
    return out


def test_segment_waveforms_equal_the_node_by_hand_captured_and_eager(dev, net, waves16, captured):
    enh, plan, tables, noise, speech = captured
    assert plan.rows == 9 and plan.batches == 3
    for b, want in enumerate(_by_hand(net, enh, waves16, plan, dev, True)):
        rows = slice(b * S, (b + 1) * S)
        assert torch.equal(noise[rows], want[:S]), b
        assert torch.equal(speech[rows], want[S:]), b
    assert float(speech[:plan.rows].abs().max()) > 1e-3 and float(noise[:plan.rows].abs().max()) > 1e-3
    eager = _enhancer(net, use_graph=False)
    _, _, noise_e, speech_e = eager.enhance_segments(waves16, 16000)
    assert eager._graph is None and enh._graph is not None
    assert torch.equal(noise_e, noise) and torch.equal(speech_e, speech)
    assert not net.training
    graph = enh._graph
    _, _, noise2, speech2 = enh.enhance_segments(waves16, 16000)
    assert enh._graph is graph                                           # replayed, not captured again
    assert torch.equal(noise2, noise) and torch.equal(speech2, speech)
    net.train()
    try:
        eager.enhance_segments(waves16[:1], 16000)
        assert net.training                                              # the training flag is restored
    finally:
        net.eval()


def test_a_recording_does_not_depend_on_its_batch_neighbours(dev, waves16, captured):
    """Alone and among the others, same batch_segments: in eval() every row of the batch is computed on its own, so only the
    row a segment lands in differs.  2e-4 absolute, the bound of the same test of the complex network (tests/test_enhance.py):
    the mask is a sigmoid (< 1), the estimates are |Y| M and |Y| - |Y| M of signals below 1."""
    enh = captured[0]
    among, among_n = enh(waves16, 16000, return_noise=True)
    assert [o.numel() for o in among] == list(LENGTHS) and all(o.is_cuda and o.dtype == torch.float32 for o in among)
    for i in (0, 3):
        alone, alone_n = enh([waves16[i]], 16000, return_noise=True)
        assert alone[0].shape == among[i].shape
        assert float((alone[0] - among[i]).abs().max()) <= 2e-4
        assert float((alone_n[0] - among_n[i]).abs().max()) <= 2e-4
        assert float(among[i].abs().max()) > 1e-3


def test_replay_after_the_envelope_and_pack_caches_evicted(dev, waves16, captured):
    """tests/test_enhance.py's test of the same name for the real twin: the envelope cache and the real network's pack cache
    pushed past their capacities (64, 512) take nothing from under the captured graph."""
    from dcsnet import network_functions as nf, r_network
    enh, plan, tables, noise, speech = captured
    assert enh._graph is not None
    graph = enh._graph
    window = torch.hann_window(512).to(dev)
    for t in range(70):
        nf._inv_envelope(window, 16 + 8 * t, HOP)
    assert len(nf._ENVELOPES) <= 64
    owner, w = torch.nn.Identity(), torch.ones(2, 2, 1, 1, device=dev)
    for tag in range(520):
        r_network._packed(owner, tag, (w,), lambda: w * float(tag))
    assert len(r_network._PACKED) == 512
    _, _, noise2, speech2 = enh.enhance_segments(waves16, 16000)
    assert enh._graph is graph                                           # replayed, not captured again
    assert torch.equal(noise2, noise) and torch.equal(speech2, speech)


def _reference_fp64(x, plan, i):
    """Recording i through the reference's own chain in fp64 on the CPU, segment by segment: torch.stft of the zero-extended
    recording (centred, reflected at 0 and at L_i), bins 1..256, oracle.nf_oracle.mag_phase_2_wave of the noisy magnitude on the
    noisy phase over each segment's frames, and the linear cross-fade of DESIGN §6d."""
    from oracle.nf_oracle import mag_phase_2_wave
    eps = float(np.float32(10e-7))
    n, frames, n_seg = len(x), int(plan.frames[i]), int(plan.n_seg[i])
    xe = torch.zeros(HOP * (frames - 1), dtype=torch.float64)
    xe[:n] = torch.from_numpy(x).double()
    w = torch.hann_window(512, dtype=torch.float64)
    Y = torch.stft(xe, 512, HOP, 512, w, center=True, pad_mode='reflect', normalized=True, return_complex=True)[1:257]
    assert Y.shape == (256, frames)
    seg = []
    for s in range(n_seg):
        Ys = Y[None, :, s * (T - O):s * (T - O) + T]
        seg.append(mag_phase_2_wave(Ys.abs(), torch.atan2(Ys.imag, Ys.real + eps), 512, HOP, w)[0].numpy())
    seg = np.stack(seg)
    stride, ov = HOP * (T - O), HOP * (O - 1)
    m = np.arange(n)
    s = np.minimum(m // stride, n_seg - 1)
    j = m - s * stride
    out = seg[s, j]
    inside = (s > 0) & (j < ov)
    a = seg[s[inside] - 1, j[inside] + stride]
    out[inside] = a + (j[inside] + 0.5) / ov * (out[inside] - a)
    return out


@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
def test_a_closed_or_open_mask_returns_the_noisy_recordings_synthesis(dev, net, waves16, use_graph, monkeypatch):
    """The raw forward patched to a constant: at -40 the sigmoid is 4e-18, the noise magnitude vanishes and the speech estimate is
    the noisy magnitude on the noisy phase; at +40 the sigmoid is 1 in fp32 and the noise estimate is.  Segmenting, padding, the
    table, the static buffers and the stitch are in the loop.  5e-6: the synthesis tolerance of DESIGN §6d (the bound of
    tests/test_enhance.py::test_pass_through_returns_the_resampled_recordings).

    The yardstick is the resampled recording taken through the reference's own analysis and synthesis in fp64 (_reference_fp64),
    not the recording itself: mag_phase_2_wave appends its zero bin BEHIND bin 256 (network_functions.py:140-145, the quirk
    oracle/nf_oracle.py keeps and tests/golden pins), so bins 1..256 of the STFT come back as bins 0..255 and an all-pass mask
    returns the recording one bin lower in frequency — 0.76 away from it at these tones (asserted below), for the reference as for
    this project.  The complex Enhancer's pass-through test avoids that by replacing the whole batch step with a synthesis that
    puts the DC bin back in front; here the real synthesis is what is under test."""
    refs = None
    for level in (-40.0, 40.0):
        monkeypatch.setattr(net, 'forward', lambda x, sigmoid=True, level=level: torch.full_like(x, level))
        enh = _enhancer(net, use_graph=use_graph)
        speech, noise = enh(waves16, 16000, return_noise=True)
        if refs is None:
            plan = enh.enhance_segments(waves16, 16000)[0]
            refs = [_reference_fp64(x, plan, i) for i, x in enumerate(waves16)]
            assert max(float(np.abs(r - x).max()) for r, x in zip(refs, waves16)) > 0.1      # the one-bin shift: no identity
        same, gone = (speech, noise) if level < 0 else (noise, speech)
        worst = 0.0
        for x, r, y, z in zip(waves16, refs, same, gone):
            assert y.shape == z.shape == (len(x),)
            worst = max(worst, float(np.abs(y.cpu().double().numpy() - r).max()))
            assert float(z.abs().max()) < 5e-6
        print(f'level {level}: max |estimate - fp64 reference synthesis of the recording| = {worst:.3e}')
        assert worst < 5e-6
        assert (enh._graph is not None) == use_graph


def test_mask_applying_mode(dev, net, waves16):
    """'dr': the mask is applied (speech = |Y| M on the noisy phase); there is no noise estimate."""
    enh = _enhancer(net, mode='dr', use_graph=False)
    plan, tables, noise, speech = enh.enhance_segments(waves16[:2], 16000)
    assert noise is None and plan.rows == 2 and plan.batches == 1
    (want,) = _by_hand(net, enh, waves16[:2], plan, dev, False)
    assert want.shape == (S, LS) and torch.equal(speech, want)
    with pytest.raises(ValueError, match='no noise estimate'):
        enh(waves16[:1], 16000, return_noise=True)
    cap = _enhancer(net, mode='dr', use_graph=True)
    assert torch.equal(cap.enhance_segments(waves16[:2], 16000)[3], speech) and cap._graph is not None


def test_errors(dev, net):
    from dcsnet import DcsHipError
    from dcsnet.config import config, hparams
    from dcsnet.c_network import C_NETWORK
    from dcsnet.r_network import R_NETWORK
    from dcsnet.enhance import Enhancer, MagnitudeEnhancer
    cnet = fill_state(C_NETWORK(config, dict(hparams), 0), 3).to(dev)
    with pytest.raises(DcsHipError, match='C_NETWORK'):
        MagnitudeEnhancer(cnet, mode='drs')
    with pytest.raises(DcsHipError, match='R_NETWORK'):
        Enhancer(net)
    with pytest.raises(DcsHipError, match='MagnitudeEnhancer'):          # the message points at the class that does it
        Enhancer(net)
    with pytest.raises(DcsHipError, match='no CPU fallback'):
        MagnitudeEnhancer(R_NETWORK(config, dict(hparams), 0))
    for mode in ('dcs', 'dc'):
        with pytest.raises(ValueError, match='mode'):
            MagnitudeEnhancer(net, mode=mode)
    with pytest.raises(ValueError, match='multiple of 8'):
        MagnitudeEnhancer(net, segment_frames=60, overlap_frames=16)


def test_pcm_file_round_trip(dev, waves16, captured, tmp_path):
    from scipy.io import wavfile
    enh, plan, tables, noise, speech = captured
    src, dst = str(tmp_path / 'noisy.wav'), str(tmp_path / 'enhanced.wav')
    x = np.clip(np.round(waves16[3] * 32768), -32767, 32767).astype(np.int16)
    wavfile.write(src, 16000, x)
    assert enh.enhance_files([src], [dst]) == [dst]
    rate, y = wavfile.read(dst)
    assert rate == 16000 and y.dtype == np.int16 and y.shape == x.shape
    p1, t1, _, s1 = enh.enhance_segments([x], 16000)
    want = enh.stitch(p1, t1, s1, pcm=True)[1].cpu().numpy()
    assert np.array_equal(y, want) and int(np.abs(y).max()) > 30
