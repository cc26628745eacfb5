"""HBM-resident training audio (dcsnet/audio_store.py, csrc/audio_store.hip): the torchaudio 0.9.0 sinc resampler restated in
float64 here and pinned against scipy and analytic tones; ops.resample_sinc against that restatement; the fused batch op
against the composition it replaces (device resampling, host crop, frontend.stft_batch) bit for bit, against the oracle
front end, under graph replay and as the input of a captured TrainStep.  The CPU tests check the crop rule, the epoch
sharding and the argument checks without a GPU.  All audio is synthetic, generated from seeds."""
import math

import numpy as np
import pytest
import torch

from dcsnet import _lib, ops
from dcsnet.audio_store import DeviceAudioStore, check_indices, draw_crop_starts, epoch_batches


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    _lib.load()
    return torch.device('cuda:0')


# ---- the float64 restatement of torchaudio.transforms.Resample (0.9.0: sinc_interpolation, width 6, rolloff 0.99) ----------

def _taps64(orig, new):
    """_get_sinc_resample_kernel in float64, phase by phase as torchaudio loops over them."""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * 0.99
    width = math.ceil(6 * o / base)
    idx = np.arange(-width, width + o, dtype=np.float64)
    rows = []
    for i in range(n):
        t = np.clip((-i / n + idx / o) * base, -6, 6)
        window = np.cos(t * math.pi / 6 / 2) ** 2
        t = t * math.pi
        with np.errstate(divide='ignore', invalid='ignore'):
            k = np.where(t == 0, 1.0, np.sin(t) / t)
        rows.append(k * window)
    return np.stack(rows) * (base / o), o, n, width


def _resample64(x, orig, new):
    """pad(width, width + o), conv1d(stride o) with the once-rounded float32 taps, transpose / reshape, keep ceil(n L / o):
    evaluated in float64."""
    if orig == new:
        return np.asarray(x, dtype=np.float64)
    h, o, n, width = _taps64(orig, new)
    h = h.astype(np.float32).astype(np.float64)
    x = np.asarray(x, dtype=np.float64)
    L = x.shape[0]
    xp = np.pad(x, (width, width + o))
    win = np.lib.stride_tricks.sliding_window_view(xp, h.shape[1])[::o]              # [floor(L / o) + 1, K]
    return (win @ h.T).reshape(-1)[:-(-n * L // o)]


def _signal(rng, L, fs, amp=0.3):
    """Tones with a wandering pitch plus a broadband part: the kind of content speech has."""
    t = np.arange(L) / fs
    f0 = rng.uniform(90, 250)
    s = sum(np.sin(2 * np.pi * k * f0 * t + rng.uniform(0, 6.3)) / k for k in range(1, 12))
    s = s + 0.1 * rng.standard_normal(L)
    return (amp * s / np.max(np.abs(s))).astype(np.float32)


# ---- CPU: the restatement itself ------------------------------------------------------------------------------------------

def test_sinc_taps_of_48k_to_16k():
    h, o, n, width = _taps64(48000, 16000)
    assert (o, n, width, h.shape) == (3, 1, 19, (1, 41))
    assert abs(h.astype(np.float32).astype(np.float64).sum() - 1.000466) < 1e-6
    assert ops.sinc_resample_geometry(48000, 16000) == (3, 1, 19, 41)
    assert ops.sinc_resample_geometry(44100, 16000) == (441, 160, 17, 475)
    for orig, new in ((48000, 16000), (44100, 16000), (8000, 16000)):
        assert np.array_equal(ops.sinc_resample_taps(orig, new).astype(np.float32), _taps64(orig, new)[0].astype(np.float32))


def test_restatement_matches_scipy_upfirdn():
    """scipy applies the same filter by its own rules: that pins padding, stride and output length."""
    from scipy.signal import upfirdn
    h = _taps64(48000, 16000)[0][0].astype(np.float32).astype(np.float64)
    rng = np.random.default_rng(1)
    for L in (48000, 48001, 48002, 100):
        x = rng.standard_normal(L)
        y = _resample64(x, 48000, 16000)
        n_out = -(-L // 3)
        assert y.shape == (n_out,) == (ops.resample_sinc_length(L, 48000, 16000),)
        ref = upfirdn(h[::-1], x, 1, 3)[7:7 + n_out]
        assert np.max(np.abs(y - ref)) < 1e-12, L


def test_restatement_against_analytic_tones():
    """Zero-delay alignment: unit sines resample to the analytic 16 kHz samples; a 12 kHz tone (above 8 kHz) is stopped."""
    L = 48000
    t48, t16 = np.arange(L) / 48000, np.arange(L // 3) / 16000
    for f in (440.0, 1000.0, 3000.0):
        y = _resample64(np.sin(2 * np.pi * f * t48), 48000, 16000)
        err = np.max(np.abs(y - np.sin(2 * np.pi * f * t16))[20:-20])
        assert err < 1e-3, (f, err)
    y = _resample64(np.sin(2 * np.pi * 12000.0 * t48), 48000, 16000)
    assert np.max(np.abs(y[20:-20])) < 3e-3


def test_fp32_model_of_the_kernel_arithmetic():
    """The kernel's arithmetic (float32 taps and samples, one fp32 accumulator in tap order) stays within a few ulp of the
    float64 restatement: what bounds the device tolerance below (1e-6 max|x|)."""
    rng = np.random.default_rng(2)
    x = rng.standard_normal(30000).astype(np.float32)
    x /= np.max(np.abs(x))
    h = _taps64(48000, 16000)[0][0].astype(np.float32)
    xp = np.pad(x, (19, 22))
    win = np.lib.stride_tricks.sliding_window_view(xp, 41)[::3]
    acc = np.zeros(win.shape[0], dtype=np.float32)
    for k in range(41):
        acc = (acc + h[k] * win[:, k]).astype(np.float32)
    err = np.max(np.abs(acc[:10000].astype(np.float64) - _resample64(x, 48000, 16000)))
    assert err < 3.5e-7, err


# ---- CPU: crop rule, epochs, argument checks ------------------------------------------------------------------------------

def test_crop_starts_follow_crop_batch():
    """The store's draws equal frontend.crop_batch's for the same generator state, short items and len == L included."""
    from dcsnet.frontend import crop_batch
    L = 8160
    lengths = [4000, L, L + 1, L + 2, 16000, 240000, 100, 9000]
    items = [torch.arange(n, dtype=torch.float32) for n in lengths]
    idx = [5, 0, 1, 2, 3, 4, 6, 7, 5, 1]
    for seed in range(3):
        starts = draw_crop_starts(lengths, idx, L, torch.Generator().manual_seed(seed))
        c, _ = crop_batch([items[i] for i in idx], [items[i] for i in idx], L, generator=torch.Generator().manual_seed(seed))
        for b, i in enumerate(idx):
            if lengths[i] <= L:
                assert starts[b] == 0
            else:
                assert 0 <= starts[b] < lengths[i] - L
                assert float(c[b, 0]) == starts[b]                 # crop_batch's crop starts at sample `start`
        assert starts == [int(v[0]) if lengths[i] > L else 0 for v, i in zip(c, idx)]


def test_epoch_shards_are_disjoint_and_cover_each_global_batch():
    n, bs = 37, 8
    for drop_last in (False, True):
        full = list(epoch_batches(n, bs, torch.Generator().manual_seed(4), drop_last=drop_last))
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(4)).tolist()
        assert [i for b in full for i in b] == perm[:len(full) * bs if drop_last else n]
        assert len(full) == (n // bs if drop_last else -(-n // bs))
        for world in (2, 3, 4):
            shards = [list(epoch_batches(n, bs, torch.Generator().manual_seed(4), drop_last=drop_last, rank=r, world=world))
                      for r in range(world)]
            for k, gb in enumerate(full):
                parts = [shards[r][k] for r in range(world)]
                assert sum(parts, []) == gb                          # contiguous shares, in rank order: disjoint and covering
    assert list(epoch_batches(5, 2, shuffle=False)) == [[0, 1], [2, 3], [4]]
    with pytest.raises(ValueError):
        list(epoch_batches(5, 2, rank=2, world=2))


def test_argument_checks_raise_before_any_launch(tmp_path):
    from dcsnet.config import config
    from scipy.io import wavfile
    a = np.zeros(4800, dtype=np.float32)
    with pytest.raises(ValueError, match='not the same length'):
        DeviceAudioStore([a], [a[:-1]], config, 'cuda')
    with pytest.raises(ValueError, match='1-D'):
        DeviceAudioStore([a.reshape(2, -1)], [a.reshape(2, -1)], config, 'cuda')
    with pytest.raises(TypeError):
        DeviceAudioStore([a.astype(np.float64)], [a.astype(np.float64)], config, 'cuda')
    with pytest.raises(_lib.DcsHipError):
        DeviceAudioStore([a], [a], config, 'cpu')
    pcm = np.zeros(4800, dtype=np.int16)
    cases = {'rate.wav': (44100, pcm), 'stereo.wav': (48000, np.zeros((4800, 2), dtype=np.int16)),
             'float.wav': (48000, pcm.astype(np.float32))}
    wavfile.write(str(tmp_path / 'ok.wav'), 48000, pcm)
    for name, (rate, data) in cases.items():
        wavfile.write(str(tmp_path / name), rate, data)
        with pytest.raises(ValueError):
            DeviceAudioStore.from_wav([str(tmp_path / name)], [str(tmp_path / 'ok.wav')], config, 'cuda')
    with pytest.raises(IndexError):
        draw_crop_starts([9000, 9000], [0, 2], 8160)
    with pytest.raises(IndexError):
        check_indices([-1], 3)
    cpu = torch.zeros(96, dtype=torch.float32)
    with pytest.raises(_lib.DcsHipError):
        ops.resample_sinc(cpu, 48000, 16000)
    idx = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(_lib.DcsHipError):
        ops.audio_stft_batch(cpu, cpu, torch.tensor([0, 96]), idx, idx, torch.hann_window(512), 256, 32, 512 ** -0.5)


# ---- GPU -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_resample_sinc_matches_the_restatement(dev):
    """Ragged rows in one launch, down- and upsampling: within 1e-6 max|x| of the float64 restatement."""
    rng = np.random.default_rng(5)
    for orig, new, lengths in ((48000, 16000, [48000, 1, 2, 3, 12347, 100]), (44100, 16000, [44100, 7, 5000]),
                               (8000, 16000, [8000, 1, 333, 4097])):
        rows = [rng.standard_normal(L).astype(np.float32) for L in lengths]
        off = np.concatenate([[0], np.cumsum(lengths)])
        y = ops.resample_sinc(torch.from_numpy(np.concatenate(rows)).to(dev), orig, new, offsets=off).cpu().numpy()
        out_len = [ops.resample_sinc_length(L, orig, new) for L in lengths]
        y_off = np.concatenate([[0], np.cumsum(out_len)])
        assert y.shape == (y_off[-1],)
        for r, x in enumerate(rows):
            want = _resample64(x, orig, new)
            got = y[y_off[r]:y_off[r + 1]]
            assert got.shape == want.shape
            err = np.max(np.abs(got - want))
            assert err <= 1e-6 * np.max(np.abs(x)), (orig, new, lengths[r], err)
    x = torch.from_numpy(rng.standard_normal((3, 4800)).astype(np.float32)).to(dev)
    y = ops.resample_sinc(x, 48000, 16000)
    assert y.shape == (3, 1600)
    assert np.max(np.abs(y[1].cpu().numpy() - _resample64(x[1].cpu().numpy(), 48000, 16000))) <= 1e-6 * float(x[1].abs().max())
    assert ops.resample_sinc(x, 16000, 16000) is x                          # Resample.forward at equal rates


def _dataset(seed, lengths48, int16_noisy=False):
    rng = np.random.default_rng(seed)
    clean = [_signal(rng, L, 48000) for L in lengths48]
    noisy = [c + (0.05 * rng.standard_normal(c.shape[0])).astype(np.float32) for c in clean]
    if int16_noisy:
        noisy = [np.round(np.clip(y, -1, 1) * 32767).astype(np.int16) for y in noisy]
    return clean, noisy


# 16 kHz lengths: 4000 (shorter than the crop), 8160 (exactly the crop), 1 s, 15 s, and a spread between
_LENGTHS48 = [12000, 24480, 48000, 720000] + [24483, 24486, 30000, 60001, 99999, 150000]


@pytest.mark.gpu
def test_fused_batch_equals_the_composition(dev):
    """B = 32 drawn over ragged items: torch.equal to frontend.stft_batch of the device-resampled, host-cropped waveforms."""
    from dcsnet.config import config
    from dcsnet.frontend import crop_batch, stft_batch
    clean, noisy = _dataset(6, _LENGTHS48)
    store = DeviceAudioStore(clean, noisy, config, dev, chunk_samples=200000)   # several upload chunks
    assert store.T == 256 and store.crop_length == 8160
    assert list(store.lengths) == [-(-L // 3) for L in _LENGTHS48]
    idx = [int(i) for i in np.random.default_rng(7).integers(0, len(store), 30)] + [0, 1]    # the short and the exact item
    g_store, g_crop = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    noise, noisy_s, clean_s, starts = store.batch(idx, generator=g_store)
    off = store.offsets.cpu()
    c16 = [store.clean[off[i]:off[i + 1]].cpu() for i in idx]
    n16 = [store.noisy[off[i]:off[i + 1]].cpu() for i in idx]
    cc, nn = crop_batch(c16, n16, store.crop_length, generator=g_crop)
    want = stft_batch(cc.to(dev), nn.to(dev), config)
    for name, a, b in zip(('noise', 'noisy', 'clean'), (noise, noisy_s, clean_s), want):
        assert a.shape == (32, 256, 256) and a.is_contiguous() and a.dtype == torch.complex64, name
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    assert starts.tolist() == store.draw_starts(idx, torch.Generator().manual_seed(11))
    # the same items at explicit starts, written into given buffers
    bufs = tuple(torch.full((32, 256, 256), float('nan'), dtype=torch.complex64, device=dev) for _ in range(3))
    got = store.batch(idx, starts=starts, out=bufs)
    assert all(g is b for g, b in zip(got[:3], bufs))
    assert all(torch.equal(a, b) for a, b in zip(bufs, want))


@pytest.mark.gpu
def test_fused_batch_matches_the_oracle_front_end(dev):
    """The float64 restated resampler, the crop at the store's starts and oracle.nf_oracle.stft_frontend (torch.stft), at the
    tolerance of test_hip_parity's front-end test; int16 noisy input scaled by 1/32768."""
    from dcsnet.config import config
    from oracle.nf_oracle import stft_frontend
    clean, noisy = _dataset(8, _LENGTHS48, int16_noisy=True)
    store = DeviceAudioStore(clean, noisy, config, dev)
    idx = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 3, 3]
    got = store.batch(idx, generator=torch.Generator().manual_seed(2))
    starts = got[3].tolist()
    L = store.crop_length

    def crop(x, s):
        y = np.zeros(L, dtype=np.float32)
        seg = x[s:s + L]
        y[:seg.shape[0]] = seg
        return y
    c = np.stack([crop(_resample64(clean[i], 48000, 16000).astype(np.float32), s) for i, s in zip(idx, starts)])
    n = np.stack([crop(_resample64(noisy[i].astype(np.float64) / 32768, 48000, 16000).astype(np.float32), s)
                  for i, s in zip(idx, starts)])
    want = stft_frontend(torch.from_numpy(c), torch.from_numpy(n))
    for name, a, b in zip(('noise', 'noisy', 'clean'), got[:3], want):
        err = float((a.cpu() - b).abs().max())
        assert err <= 1e-5 * float(b.abs().max()) + 1e-7, (name, err)


@pytest.mark.gpu
def test_fused_batch_replays_in_a_graph_with_new_indices(dev):
    from dcsnet.config import config
    clean, noisy = _dataset(9, _LENGTHS48)
    store = DeviceAudioStore(clean, noisy, config, dev)
    B = 6
    index = torch.tensor([0, 1, 2, 3, 4, 5], dtype=torch.int32, device=dev)
    starts = torch.tensor([0, 0, 100, 5000, 0, 700], dtype=torch.int32, device=dev)
    bufs = tuple(torch.empty((B, 256, 256), dtype=torch.complex64, device=dev) for _ in range(3))
    store.batch_device(index, starts, out=bufs)                             # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        store.batch_device(index, starts, out=bufs)
    new_idx, new_starts = [3, 9, 8, 0, 6, 2], [40000, 3, 11, 0, 1, 0]
    index.copy_(torch.tensor(new_idx, dtype=torch.int32))
    starts.copy_(torch.tensor(new_starts, dtype=torch.int32))
    g.replay()
    want = store.batch(new_idx, starts=new_starts)
    torch.cuda.synchronize()
    for a, b in zip(bufs, want[:3]):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_captured_train_step_fed_by_the_store_equals_the_composition(dev):
    """Five steps of TrainStep(use_graph=True): one fed by store.batch(..., out=step.input_buffers()), one by crop_batch +
    stft_batch; dropout off, so losses and parameters agree bit for bit."""
    from dcsnet.config import config, hparams
    from dcsnet.c_network import C_NETWORK
    from dcsnet.dp import TrainStep
    from dcsnet.frontend import crop_batch, stft_batch
    from oracle.seeded_state import fill_state
    hp = dict(hparams)
    hp['dropout_conv'], hp['dropout_fc'] = 0.0, 0.0
    clean, noisy = _dataset(10, _LENGTHS48)
    store = DeviceAudioStore(clean, noisy, config, dev)
    batches = [b for b in store.epoch(2, torch.Generator().manual_seed(3))][:5]
    off = store.offsets.cpu()
    runs = []
    for fused in (True, False):
        net = fill_state(C_NETWORK(config, hp, 0), 2).to(dev).train()
        ts = TrainStep(net, use_graph=True, graph_warmup=1)
        g = torch.Generator().manual_seed(21)
        losses = []
        for idx in batches:
            if fused:
                noise, noisy_s, clean_s, _ = store.batch(idx, generator=g, out=ts.input_buffers())
            else:
                cc, nn = crop_batch([store.clean[off[i]:off[i + 1]].cpu() for i in idx],
                                    [store.noisy[off[i]:off[i + 1]].cpu() for i in idx], store.crop_length, generator=g)
                noise, noisy_s, clean_s = stft_batch(cc.to(dev), nn.to(dev), config)
            losses.append(float(ts((noise, noisy_s, clean_s, idx))))
        assert ts._graph is not None
        runs.append((losses, ts.bucket.flat.clone()))
    (la, pa), (lb, pb) = runs
    assert la == lb and all(math.isfinite(v) for v in la), (la, lb)
    assert torch.equal(pa, pb)
