"""GPU: mixing clean speech and noise at drawn SNRs on the device (csrc/audio_mix.hip, dcsnet/audio_store.py::MixingAudioStore).
Every result is tied bit for bit to code the suite already pins: the mixing batch to frontend.stft_batch of a host-made
mixture (two separately rounded float32 operations: a contracted FMA fails it) and, through the ragged mix kernel, to the
paired store's batch; the powers to numpy in float64.  All audio is synthetic, generated from seeds."""
import json
import math
import types

import numpy as np
import pytest
import torch

from dcsnet import _lib, ops
from dcsnet.audio_store import DeviceAudioStore, MixingAudioStore, draw_crop_starts, draw_mix, mix_gain

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda:0')


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _flat(signals, dev):
    off = np.concatenate([[0], np.cumsum([len(s) for s in signals])]).astype(np.int64)
    return torch.from_numpy(np.concatenate(signals)).to(dev), torch.from_numpy(off).to(dev)


# ---- 1. power -----------------------------------------------------------------------------------------------------------------------

def test_signal_power_against_numpy_in_float64(dev):
    """1e-12 relative: a 256-way strided fp64 sum plus an 8-level tree errs by at most (N / 256 + 9) 2^-53 < 3e-14 at N = 65536
    and numpy's pairwise sum by less; the squares are exact in fp64."""
    rng = np.random.default_rng(1)
    lengths = [1, 255, 256, 257, 4097, 65536]
    rows = [(0.3 * rng.standard_normal(L) * (1 + np.arange(L) / L)).astype(np.float32) for L in lengths]
    x, off = _flat(rows, dev)
    got = ops.signal_power_ragged(x, off)
    assert got.dtype == torch.float64 and got.shape == (6,)
    want = np.array([np.mean(np.square(r.astype(np.float64))) for r in rows])
    rel = np.abs(got.cpu().numpy() - want) / want
    print('signal_power_ragged: relative errors', rel.tolist())
    assert (rel <= 1e-12).all(), rel.tolist()
    assert torch.equal(ops.signal_power_ragged(x, off), got)  # the same bits on every run
    # an empty recording between two others gives 0 and moves nothing
    off2 = torch.tensor([0, 1, 1, 256], dtype=torch.int64, device=dev)
    p = ops.signal_power_ragged(x[:256].contiguous(), off2).cpu().numpy()
    assert p[1] == 0.0 and p[0] == float(rows[0][0]) ** 2
    assert abs(p[2] - np.mean(np.square(rows[1].astype(np.float64)))) <= 1e-12 * p[2]


# ---- 2. / 3. the kernel at the smallest shapes where it can go wrong -------------------------------------------------------------------

HOP, T, L = 32, 13, 384                                      # L = 384 > 256 (one reflection), T no multiple of the 8 frames per workgroup
CLEAN_LENGTHS = [1000, 300, 384]                             # longer than the crop, shorter (zero tail), exactly the crop
NOISE_LENGTHS = [100, 700]                                   # wraps four times inside one crop; wraps once near its end
#         clean item, crop start, noise recording, noise start
ITEMS = [(0, 200, 0, 99),                                    # start > 0, 100 samples of noise from its last one: four wraps
         (1, 0, 1, 650),                                     # the short item: zero tail; 50 samples before the noise wraps once
         (2, 0, 0, 99),                                      # exactly the crop, the short noise
         (0, 616, 1, 699),                                   # the last admissible start (616 + 384 = 1000): (699 + 616) mod 700, one wrap
         (1, 0, 1, 0)]                                       # no wrap at all
GAINS = [0.37, 1.9, 0.011, 0.73, 1.0]


def _small_config():
    from dcsnet.config import config
    return types.SimpleNamespace(fft_size=512, hop_length=HOP, window=config.window, normalise_stft=True)


@pytest.fixture(scope='module')
def small(dev):
    """The two small stores, the batch of ITEMS through the kernel, and the reference: frontend.stft_batch of the clean crops and
    of a mixture formed on the CPU in float32 as two separately rounded operations."""
    from dcsnet.frontend import stft_batch
    rng = np.random.default_rng(2)
    clean = [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in CLEAN_LENGTHS]
    noise = [(0.2 * rng.standard_normal(n)).astype(np.float32) for n in NOISE_LENGTHS]
    c = torch.zeros(len(ITEMS), L)
    n = torch.zeros(len(ITEMS), L)
    for b, (i, start, r, nstart) in enumerate(ITEMS):
        seg = clean[i][start:start + L]
        c[b, :len(seg)] = torch.from_numpy(seg)
        n[b] = torch.from_numpy(noise[r][(nstart + start + np.arange(L)) % len(noise[r])])
    g = torch.tensor(GAINS, dtype=torch.float32)
    scaled = g[:, None] * n                                   # rounded to float32
    noisy = c + scaled                                        # rounded again: no FMA
    for b, (i, start, _, _) in enumerate(ITEMS):
        noisy[b, max(0, CLEAN_LENGTHS[i] - start):] = 0.0     # zero past the clean item's end
    fused = torch.addcmul(c.double(), g[:, None].double(), n.double()).float()
    assert int((fused != c + scaled).sum()) > 0               # (the data does tell an FMA from two roundings)
    cfg = _small_config()
    want = stft_batch(c.to(dev), noisy.to(dev), cfg)
    stores = _flat(clean, dev) + _flat(noise, dev)
    window = cfg.window.to(dev)
    sel = [_i32([it[k] for it in ITEMS], dev) for k in range(4)] + [g.to(dev)]

    def run(index, start, nidx, nstart, gain):
        return ops.audio_mix_stft_batch(stores[0], stores[1], stores[2], stores[3], index, start, nidx, nstart, gain, window, T,
                                        HOP, 512 ** -0.5)
    return types.SimpleNamespace(run=run, sel=sel, want=want, got=run(*sel), stores=stores, noisy=noisy, clean=clean)


def test_mix_batch_equals_stft_batch_of_a_host_mixture(small):
    for name, a, b in zip(('noise', 'noisy', 'clean'), small.got, small.want):
        assert a.shape == (5, 256, T) and a.dtype == torch.complex64 and a.is_contiguous(), name
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    assert float(small.got[0].abs().max()) > 0 and float(small.got[1][1].abs().max()) > 0


def test_ragged_mix_equals_the_host_mixture(small, dev):
    """Whole recordings: item i with the draw of the first ITEMS row that uses it; the crop of the result is that row's mixture."""
    rows = [next(b for b, it in enumerate(ITEMS) if it[0] == i) for i in range(3)]
    nidx, nstart = _i32([ITEMS[b][2] for b in rows], dev), _i32([ITEMS[b][3] for b in rows], dev)
    gain = torch.tensor([GAINS[b] for b in rows], device=dev)
    y = ops.audio_mix_ragged(small.stores[0], small.stores[1], small.stores[2], small.stores[3], nidx, nstart, gain).cpu()
    off = small.stores[1].cpu().tolist()
    for i, b in enumerate(rows):
        start = ITEMS[b][1]
        seg = y[off[i] + start:min(off[i + 1], off[i] + start + L)]
        assert torch.equal(seg, small.noisy[b, :len(seg)]), i
    # a draw that cannot be followed leaves the clean recording
    bad = ops.audio_mix_ragged(small.stores[0], small.stores[1], small.stores[2], small.stores[3], _i32([0, 2, 1], dev),
                               _i32([99, 0, 700], dev), torch.tensor([0.5, 1.0, float('nan')], device=dev)).cpu()
    assert torch.equal(bad[off[1]:], small.stores[0].cpu()[off[1]:]) and not torch.equal(bad[:off[1]], small.stores[0].cpu()[:off[1]])


@pytest.mark.parametrize('column, value', [(2, -1), (2, len(NOISE_LENGTHS)), (3, -1), (3, 'len_n'), (4, float('inf')),
                                           (4, float('-inf')), (4, float('nan')), (0, -1), (0, len(CLEAN_LENGTHS)), (1, -1),
                                           (1, 617)])
@pytest.mark.parametrize('b', [0, 3])
def test_a_selection_that_must_not_be_followed_gives_zeros_for_that_item_alone(small, column, value, b):
    sel = [t.clone() for t in small.sel]
    if value == 'len_n':
        value = NOISE_LENGTHS[ITEMS[b][2]]
    sel[column][b] = value
    got = small.run(*sel)
    others = [k for k in range(len(ITEMS)) if k != b]
    for name, a, ref in zip(('noise', 'noisy', 'clean'), got, small.got):
        assert int(torch.count_nonzero(torch.view_as_real(a[b]))) == 0, name
        assert torch.equal(a[others], ref[others]), name


# ---- 4. store against store ------------------------------------------------------------------------------------------------------------

def _corpus(seed, lengths48, amp):
    rng = np.random.default_rng(seed)
    out = []
    for k, n in enumerate(lengths48):
        t = np.arange(n) / 48000
        out.append((amp * (np.sin(2 * np.pi * (180 + 70 * k) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * (2 + k) * t)) +
                           0.3 * rng.standard_normal(n))).astype(np.float32))
    return out


CLEAN48 = [12000, 24480, 30000, 48000, 60001, 99999]         # 16 kHz: 4000 (shorter than the crop), 8160 (the crop), ...
NOISE48 = [9000, 60000, 150000]                              # 16 kHz: 3000 (shorter than the crop), 20000, 50000


@pytest.fixture(scope='module')
def mixing(dev):
    from dcsnet.config import config
    return MixingAudioStore(_corpus(3, CLEAN48, 0.2), _corpus(4, NOISE48, 0.1), config, dev, ids=[f'c{k}' for k in range(6)],
                            chunk_samples=100000)


def test_mixing_store_equals_the_paired_store_on_its_materialised_set(mixing, dev):
    m = mixing
    assert (m.T, m.crop_length, len(m)) == (256, 8160, 6) and list(m.lengths) == [-(-n // 3) for n in CLEAN48]
    assert list(m.noise_lengths) == [3000, 20000, 50000]
    assert m.clean_power.dtype == np.float64 and m.clean_power.shape == (6,) and m.noise_power.shape == (3,)
    off = m.offsets.cpu().tolist()
    x = m.clean.cpu().numpy().astype(np.float64)
    assert np.allclose(m.clean_power, [np.mean(x[off[i]:off[i + 1]] ** 2) for i in range(6)], rtol=1e-12, atol=0)
    idx = [3, 0, 5, 1, 4, 2]
    noise, noisy, clean, starts = m.batch(idx, generator=torch.Generator().manual_seed(12))
    d = m.last_draws
    # the draws: all crop starts first (the paired store's from this seed), then draw_mix, then mix_gain
    g = torch.Generator().manual_seed(12)
    assert starts.tolist() == draw_crop_starts(m.lengths, idx, m.crop_length, g)
    assert (d['noise_index'], d['noise_start'], d['snr_db']) == draw_mix(idx, m.noise_lengths, g)
    assert np.array_equal(d['gain'], mix_gain(m.clean_power[idx], m.noise_power[d['noise_index']], np.array(d['snr_db'])))
    assert d['gain'].dtype == np.float32 and starts.dtype == torch.int64
    per_item = [[None] * 6 for _ in range(3)]
    for b, i in enumerate(idx):
        for k, key in enumerate(('noise_index', 'noise_start', 'snr_db')):
            per_item[k][i] = d[key][b]
    fixed = m.materialise(draws=per_item)
    assert isinstance(fixed, DeviceAudioStore) and fixed.clean is m.clean and fixed.ids == m.ids and len(fixed) == 6
    want = fixed.batch(idx, starts=starts)
    for name, a, b in zip(('noise', 'noisy', 'clean'), (noise, noisy, clean), want):
        assert a.shape == (6, 256, 256) and torch.equal(a, b), (name, float((a - b).abs().max()))
    assert float(noise.abs().max()) > 0 and not torch.equal(noisy, clean)
    # explicit starts and draws, written into given buffers
    bufs = tuple(torch.full((6, 256, 256), float('nan'), dtype=torch.complex64, device=dev) for _ in range(3))
    got = m.batch(idx, starts=starts, draws=(d['noise_index'], d['noise_start'], d['snr_db']), out=bufs)
    assert all(a is b for a, b in zip(got[:3], bufs)) and all(torch.equal(a, b) for a, b in zip(bufs, want))
    # a drawn materialisation is draw_mix over the items in order
    m.materialise(generator=torch.Generator().manual_seed(13))
    e = m.last_draws
    assert (e['noise_index'], e['noise_start'], e['snr_db']) == draw_mix(range(6), m.noise_lengths, torch.Generator().manual_seed(13))
    with pytest.raises(IndexError):
        m.batch([0], draws=([3], [0], [5.0]))
    with pytest.raises(IndexError):
        m.batch([0], draws=([0], [3000], [5.0]))


def test_a_silent_recording_is_named(dev):
    from dcsnet.config import config
    clean, noise = _corpus(5, [12000, 9000], 0.2), _corpus(6, [9000, 9000], 0.1)
    noise[1][:] = 0.0
    with pytest.raises(ValueError, match=r'noise\[1\] \(hum\.wav\)'):
        MixingAudioStore(clean, noise, config, dev, noise_ids=['fan.wav', 'hum.wav'])
    clean[0][:] = 0.0
    with pytest.raises(ValueError, match=r'clean\[0\]'):
        MixingAudioStore(clean, noise[:1], config, dev)


# ---- 5. realised SNR ---------------------------------------------------------------------------------------------------------------------

def test_realised_snr_of_a_materialised_mixture(dev):
    """A noise recording as long as the clean item from its sample 0: whole-recording powers apply exactly, and float32 rounding
    of the mixture moves 10 log10(sum c^2 / sum (noisy - c)^2) by less than 1e-4 dB at these SNRs; the bound is 1e-3 dB."""
    from dcsnet.config import config
    m = MixingAudioStore(_corpus(7, [36000], 0.2), _corpus(8, [36000], 0.05), config, dev)
    for snr in (0.0, 5.0, 17.5):
        fixed = m.materialise(draws=([0], [0], [snr]))
        c, y = fixed.clean.cpu().numpy().astype(np.float64), fixed.noisy.cpu().numpy().astype(np.float64)
        realised = 10 * math.log10(np.sum(c * c) / np.sum((y - c) ** 2))
        print(f'realised SNR at {snr} dB: {realised!r}')
        assert abs(realised - snr) <= 1e-3, (snr, realised)


# ---- 6. graph replay -----------------------------------------------------------------------------------------------------------------------

def test_mixing_batch_replays_in_a_graph_with_new_selections(mixing, dev):
    m, B = mixing, 6
    sel = [_i32([0, 1, 2, 3, 4, 5], dev), _i32([0, 0, 100, 5000, 0, 700], dev), _i32([0, 1, 2, 0, 1, 2], dev),
           _i32([0, 19999, 7, 2999, 0, 49000], dev), torch.tensor([1.0, 0.5, 0.25, 2.0, 0.1, 0.7], device=dev)]
    bufs = tuple(torch.empty((B, 256, 256), dtype=torch.complex64, device=dev) for _ in range(3))
    m.batch_device(*sel, out=bufs)                            # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m.batch_device(*sel, out=bufs)
    new = ([3, 5, 4, 0, 2, 2], [7000, 3, 11, 0, 1, 0], [2, 2, 0, 1, 0, 1], [49999, 0, 2999, 12345, 1500, 19999],
           [0.3, 1.5, 0.9, 0.05, 1.25, 0.6])
    for t, v in zip(sel, new):                                # all five selection tensors rewritten
        t.copy_(torch.tensor(v, dtype=t.dtype))
    g.replay()
    want = m.batch_device(*[t.clone() for t in sel])
    torch.cuda.synchronize()
    for a, b in zip(bufs, want):
        assert torch.equal(a, b) and float(a.abs().max()) > 0


# ---- 7. through fit ------------------------------------------------------------------------------------------------------------------------

EPOCHS, BATCH = 3, 2


def test_fit_trains_on_a_mixing_store_and_repeats_itself(dev, tmp_path):
    """The run of tests/test_fit_gpu.py (six recordings of 0.6 to 1.0 s, batches of 2, 3 epochs), mixed on the fly for training
    and materialised for validation; two identically seeded runs write the same loss columns."""
    from dcsnet.config import config, hparams
    from dcsnet.c_network import C_NETWORK
    from dcsnet.fit import fit
    clean = _corpus(9, [int(s * 48000) for s in (0.6, 0.7, 0.8, 0.9, 1.0, 0.75)], 0.2)
    noise = _corpus(10, [20000, 70000], 0.1)
    rows = []
    for run in ('a', 'b'):
        train = MixingAudioStore(clean[:4], noise, config, dev)
        val = MixingAudioStore(clean[4:], noise, config, dev).materialise(generator=torch.Generator().manual_seed(int(config.seed)))
        out = fit(C_NETWORK(config, dict(hparams), 0).to(dev), train, val, str(tmp_path / run), EPOCHS, BATCH, log=lambda s: None)
        assert out['finished'] and out['global_step'] == EPOCHS * 2 and not out['rejected']
        rows.append([json.loads(ln) for ln in open(tmp_path / run / 'metrics.jsonl')])
        assert train.last_draws is not None and len(train.last_draws['gain']) == BATCH
    a, b = rows
    assert len(a) == len(b) == EPOCHS
    assert all(math.isfinite(r['train_loss']) and math.isfinite(r['val_loss']) for r in a + b)
    assert [r['train_loss'] for r in a] == [r['train_loss'] for r in b]
    assert [r['val_loss'] for r in a] == [r['val_loss'] for r in b]
