"""GPU: the ITU-T P.56 active speech level on the device (csrc/speech_level.hip, ops.active_level_ragged) against its numerics
contract, the host function metrics.active_speech_level, and MixingAudioStore(level='p56') against the level='power' store
given the same gains.  One ragged call per rate; all audio is synthetic, generated from seeds."""
import types

import numpy as np
import pytest
import torch

import _level_cases as C
from dcsnet import _lib, metrics, ops
from dcsnet.audio_store import MixingAudioStore, mix_gain

pytestmark = pytest.mark.gpu

TILE = ops.ACTIVE_LEVEL_TILE


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda:0')


def _recordings(fs):
    """(name, signal) per recording: the lengths at which the kernel takes another path, and the undefined levels."""
    I = metrics.p56_hangover(fs)
    assert I == int(np.ceil(0.2 * fs))
    lengths = [1, 255, 256, 257, I, I + 1, I + 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 40000]
    rows = [(f'bursts[{n}]', C.gated_bursts(n, fs, seed=(k & 1))) for k, n in enumerate(lengths)]
    rows.insert(5, ('empty', np.zeros(0, dtype=np.float32)))
    rows.insert(9, ('zeros', np.zeros(5000, dtype=np.float32)))
    rows.append(('quiet', C.gated_bursts(5000, fs, seed=0, amplitude=1e-6, floor=1e-6)))
    square = np.where((np.arange(20000) // 37) % 2 == 0, 1.0, -1.0).astype(np.float32)
    rows.append(('square', square))
    return rows


@pytest.fixture(scope='module', params=[16000, 8000, 48000])
def case(request, dev):
    """The recordings of one rate, the host function's results (computed once) and one ragged call with the counts."""
    fs = request.param
    rows = _recordings(fs)
    want = [metrics.active_speech_level(x, fs) for _, x in rows]
    off = np.concatenate([[0], np.cumsum([len(x) for _, x in rows])]).astype(np.int64)
    x = torch.from_numpy(np.concatenate([x for _, x in rows])).to(dev)
    offsets = torch.from_numpy(off).to(dev)
    level, counts = ops.active_level_ragged(x, offsets, fs, return_counts=True)
    return types.SimpleNamespace(fs=fs, rows=rows, want=want, off=off, x=x, offsets=offsets, level=level, counts=counts)


def test_the_inputs_keep_their_distance_from_the_thresholds(case):
    """A property of the seeds, not of the code under test: no windowed maximum of the host envelope lies within 1e-9 relative
    of a threshold, so an envelope that differs from lfilter's by rounding (about 1e-14) gives the same counts."""
    thresholds = 2.0 ** (np.arange(15) - 15.0)
    closest = np.inf
    for _, x in case.rows:
        if len(x):
            m = metrics.windowed_max(metrics.p56_envelope(x, case.fs), metrics.p56_hangover(case.fs))
            closest = min(closest, float(np.abs(m[:, None] / thresholds[None, :] - 1.0).min()))
    print(f'fs {case.fs}: smallest |m / c - 1| = {closest:.3e}')
    assert closest >= 1e-9


def test_counts_and_levels_equal_the_host_function(case):
    """Counts exactly; active_power and activity to 1e-12 relative (libm's log10 and pow in fp64: six orders below the 1 / a[j]
    >= 1e-6 that one miscounted sample would move them); NaN exactly where the host has NaN."""
    assert case.level.dtype == torch.float64 and case.level.shape == (len(case.rows), 2)
    assert case.counts.dtype == torch.int64 and case.counts.shape == (len(case.rows), 15)
    level, counts = case.level.cpu().numpy(), case.counts.cpu().numpy()
    worst = 0.0
    for i, ((name, _), want) in enumerate(zip(case.rows, case.want)):
        assert counts[i].tolist() == want['counts'].tolist(), (case.fs, name)
        for k, key in enumerate(('active_power', 'activity')):
            if np.isnan(want[key]):
                assert np.isnan(level[i, k]), (case.fs, name, key, level[i, k])
            else:
                rel = abs(level[i, k] / want[key] - 1.0)
                worst = max(worst, rel)
                assert rel <= 1e-12, (case.fs, name, key, level[i, k], want[key])
    print(f'fs {case.fs}: worst relative error {worst:.3e}')
    by_name = {name: want for (name, _), want in zip(case.rows, case.want)}
    for name in ('empty', 'zeros', 'quiet'):                  # (the undefined cases are in the set ...)
        assert np.isnan(by_name[name]['active_power']) and by_name[name]['counts'][0] == 0
    assert (by_name['square']['counts'] > 0).all() and np.isfinite(by_name['square']['active_power'])   # ... and all 15 thresholds
    assert np.isfinite(by_name['bursts[40000]']['active_power'])


def test_two_runs_give_the_same_bits(case):
    level, counts = ops.active_level_ragged(case.x, case.offsets, case.fs, return_counts=True)
    assert torch.equal(level.view(torch.int64), case.level.view(torch.int64)) and torch.equal(counts, case.counts)


def test_without_counts_the_levels_are_the_same_bits(case):
    level = ops.active_level_ragged(case.x, case.offsets, case.fs)
    assert isinstance(level, torch.Tensor) and torch.equal(level.view(torch.int64), case.level.view(torch.int64))


def test_a_recording_alone_gives_the_bits_it_has_among_others(case, dev):
    for i, (name, x) in enumerate(case.rows):
        if not len(x):
            continue
        alone = torch.from_numpy(x).to(dev)
        off = torch.tensor([0, len(x)], dtype=torch.int64, device=dev)
        level, counts = ops.active_level_ragged(alone, off, case.fs, return_counts=True)
        assert torch.equal(level[0].view(torch.int64), case.level[i].view(torch.int64)), (case.fs, name)
        assert torch.equal(counts[0], case.counts[i]), (case.fs, name)


def test_rate_and_device_are_checked(dev):
    x, off = torch.zeros(100, device=dev), torch.tensor([0, 100], dtype=torch.int64, device=dev)
    for fs in (7999, 48001):
        with pytest.raises(_lib.DcsHipError):
            ops.active_level_ragged(x, off, fs)


# ---- the store -----------------------------------------------------------------------------------------------------------------------

CLEAN48 = [60000, 36000, 90000]                              # 16 kHz: 20000, 12000, 30000; the crop is 8160
NOISE48 = [30000, 75000]


def _corpus():
    clean = [C.gated_bursts(n, 48000, seed=20 + k, amplitude=0.1) for k, n in enumerate(CLEAN48)]
    noise = [C.gated_bursts(n, 48000, seed=30 + k, amplitude=0.05, floor=0.02) for k, n in enumerate(NOISE48)]
    return clean, noise


@pytest.fixture(scope='module')
def stores(dev):
    from dcsnet.config import config
    clean, noise = _corpus()
    ids = [f'c{k}.wav' for k in range(len(clean))]
    return types.SimpleNamespace(power=MixingAudioStore(clean, noise, config, dev, ids=ids),
                                 p56=MixingAudioStore(clean, noise, config, dev, ids=ids, level='p56'),
                                 both=MixingAudioStore(clean, noise, config, dev, ids=ids, level='p56', noise_level='p56'))


def test_store_levels_are_the_ops_output(stores):
    pw, p56, both = stores.power, stores.p56, stores.both
    assert pw.clean_level is pw.clean_power and pw.noise_level is pw.noise_power
    assert np.isnan(pw.clean_activity).all() and np.isnan(pw.noise_activity).all()
    want = ops.active_level_ragged(p56.clean, p56.offsets, p56.sr).cpu().numpy()
    assert np.array_equal(p56.clean_level, want[:, 0]) and np.array_equal(p56.clean_activity, want[:, 1])
    assert p56.noise_level is p56.noise_power and np.isnan(p56.noise_activity).all()
    assert np.array_equal(p56.clean_power, pw.clean_power) and np.array_equal(p56.noise_power, pw.noise_power)
    assert (p56.clean_level > p56.clean_power).all() and ((p56.clean_activity > 0) & (p56.clean_activity < 1)).all()
    want_noise = ops.active_level_ragged(both.noise, both.noise_offsets, both.sr).cpu().numpy()
    assert np.array_equal(both.noise_level, want_noise[:, 0]) and np.array_equal(both.noise_activity, want_noise[:, 1])
    assert np.array_equal(both.clean_level, p56.clean_level) and np.array_equal(both.noise_power, pw.noise_power)


def test_store_batches_are_the_power_stores_with_the_p56_gains(stores, dev):
    pw, p56 = stores.power, stores.p56
    idx = [2, 0, 1, 2]
    noise, noisy, clean, starts = p56.batch(idx, torch.Generator().manual_seed(4))
    d = p56.last_draws
    gain = mix_gain(p56.clean_level[idx], p56.noise_power[d['noise_index']], np.array(d['snr_db']))
    assert gain.dtype == np.float32 and np.array_equal(d['gain'], gain)
    assert not np.array_equal(gain, mix_gain(pw.clean_power[idx], pw.noise_power[d['noise_index']], np.array(d['snr_db'])))
    # the same draws from the same generator state: the level does not enter the draws
    pw.batch(idx, torch.Generator().manual_seed(4))
    assert all(pw.last_draws[k] == d[k] for k in ('noise_index', 'noise_start', 'snr_db'))

    def i32(v):
        return torch.tensor(v, dtype=torch.int32, device=dev)
    want = pw.batch_device(i32(idx), i32(starts.tolist()), i32(d['noise_index']), i32(d['noise_start']),
                           torch.from_numpy(gain).to(dev))
    for name, a, b in zip(('noise', 'noisy', 'clean'), (noise, noisy, clean), want):
        assert torch.equal(a, b), name
    # materialise(): the whole-recording mixtures of the power store's tensors with the p56 gains
    draws = ([1, 0, 1], [70, 0, 24999], [5.0, 0.0, 15.0])
    fixed = p56.materialise(draws=draws)
    gain = mix_gain(p56.clean_level, p56.noise_power[draws[0]], np.array(draws[2]))
    assert np.array_equal(p56.last_draws['gain'], gain)
    want = ops.audio_mix_ragged(pw.clean, pw.offsets, pw.noise, pw.noise_offsets, i32(draws[0]), i32(draws[1]),
                                torch.from_numpy(gain).to(dev))
    assert torch.equal(fixed.noisy, want) and torch.equal(fixed.clean, pw.clean)


def test_a_recording_without_a_level_is_named(dev):
    from dcsnet.config import config
    clean, noise = _corpus()
    clean[1] = C.gated_bursts(36000, 48000, seed=21, amplitude=1e-6, floor=1e-6)
    with pytest.raises(ValueError, match=r'clean\[1\] \(quiet\.wav\).*lowest threshold'):
        MixingAudioStore(clean, noise, config, dev, ids=['a.wav', 'quiet.wav', 'b.wav'], level='p56')
    MixingAudioStore(clean, noise, config, dev, level='power')          # the mean power still serves
    with pytest.raises(ValueError, match=r'noise\[0\].*lowest threshold'):
        MixingAudioStore(noise, clean[1:2], config, dev, noise_level='p56')
