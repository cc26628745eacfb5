"""CPU-only: the ITU-T P.56 active speech level on the host (dcsnet/metrics.py::active_speech_level, the numerics contract of
csrc/speech_level.hip), the argument handling of its C entry point (every call below fails validation before any launch), and
the level= / --level switches of the mixing store and the tools.  No P.56 implementation is here to compare with: the counts
are checked against a literal transcription of the published loop (tests/_level_cases.py), the level by its defining
properties."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import _level_cases as C
from dcsnet import _lib, metrics, ops
from dcsnet.audio_store import MixingAudioStore

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = -1                                                      # DCS_ERR_BADARG
P = ctypes.c_void_p(16)                                       # never dereferenced


def _bursts(n, fs, seed):
    """Gated noise bursts whose amplitudes step through 0.002 .. 0.3 from one second (or part of one) to the next."""
    x = C.gated_bursts(n, fs, seed, amplitude=1.0, floor=1e-3, on=0.4).astype(np.float64)
    amplitude = np.array([0.002, 0.3, 0.02, 0.1, 0.005])[(np.arange(n) * 5 // max(n, 1)) % 5]
    return (amplitude * x).astype(np.float32)


# ---- the counts ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n,fs', [(3000, 16000), (8000, 16000), (12000, 16000), (20000, 16000), (12000, 8000)])
def test_counts_equal_the_published_loop(n, fs):
    x = _bursts(n, fs, seed=n + fs)
    got = metrics.active_speech_level(x, fs)
    want = C.published_counts(x, fs)
    assert got['counts'].dtype == np.int64 and got['counts'].shape == (15,)
    assert got['counts'].tolist() == want.tolist()
    assert want[0] > 0 and want[0] > want[12]                 # (the signal does separate the thresholds)
    assert (np.diff(want) <= 0).all() and want[0] <= n        # nothing is counted past the end


def test_windowed_max_is_the_maximum_over_the_last_samples():
    rng = np.random.default_rng(0)
    q = rng.random(700)
    for I in (0, 1, 7, 256, 699, 700, 5000):
        want = np.array([q[max(0, k - I):k + 1].max() for k in range(len(q))])
        assert np.array_equal(metrics.windowed_max(q, I), want), I
    assert metrics.windowed_max(np.zeros(0), 5).shape == (0,)
    assert [metrics.p56_hangover(fs) for fs in (8000, 16000, 22050, 44100, 48000, 8001)] == [1600, 3200, 4410, 8820, 9600, 1601]


# ---- the level -----------------------------------------------------------------------------------------------------------------------

def test_scaling_by_a_power_of_two_shifts_the_counts_and_scales_the_level():
    """Every intermediate scales exactly in fp64, so the counts move by s thresholds exactly; the level by 4^s to 1e-12."""
    x = C.gated_bursts(24000, 16000, seed=3, amplitude=0.02)
    base = metrics.active_speech_level(x, 16000)
    assert np.isfinite(base['active_power']) and 0 < base['activity'] < 1
    for s in (1, 2):
        y = metrics.active_speech_level(x * np.float32(2 ** s), 16000)
        assert y['counts'][s:].tolist() == base['counts'][:15 - s].tolist()
        assert abs(y['active_power'] / (4 ** s * base['active_power']) - 1) <= 1e-12
        assert abs(y['activity'] / base['activity'] - 1) <= 1e-12


def test_pauses_do_not_move_the_level():
    """A one-second burst followed by 16000 or 48000 zeros: the envelope is below 2^-15 and the hangover has expired long before
    16000 samples, so the counts and the sum of squares — hence the active power, bit for bit — do not change, while the
    mean power falls by the length ratio."""
    rng = np.random.default_rng(5)
    burst = (0.1 * rng.standard_normal(16000)).astype(np.float32)
    short, long_ = (np.concatenate([burst, np.zeros(z, dtype=np.float32)]) for z in (16000, 48000))
    a, b = metrics.active_speech_level(short, 16000), metrics.active_speech_level(long_, 16000)
    assert a['counts'].tolist() == b['counts'].tolist() and a['counts'][0] < 32000
    assert a['active_power'] == b['active_power'] and np.isfinite(a['active_power'])
    assert abs(np.mean(short.astype(np.float64) ** 2) / np.mean(long_.astype(np.float64) ** 2) - 2.0) <= 1e-12
    for r, x in ((a, short), (b, long_)):
        mean_power = np.sum(x.astype(np.float64) ** 2) / len(x)
        assert abs(r['activity'] * r['active_power'] / mean_power - 1) <= 1e-15
    assert abs(a['activity'] / b['activity'] - 2.0) <= 1e-12
    # the active part is the burst plus the hangover (3200 samples) and the envelope's decay: between 16000 and 22400 samples
    # carry the burst's energy, so the active power lies within 10 log10(16000 / 22400) = -1.46 dB of the burst's own power,
    # while the recordings' mean powers are 3 and 6 dB below it
    assert -1.5 < 10 * np.log10(a['active_power'] / np.mean(burst.astype(np.float64) ** 2)) < 0.1


def test_level_is_the_margin_crossing():
    """p56_level on counts chosen by hand: D[j] = 10 log10(sq / a[j]) - 20 log10(c[j]) crosses 15.9 dB between j = 9 and j = 10."""
    counts = np.array([1000] * 9 + [900, 500, 100, 0, 0, 0], dtype=np.int64)
    sq = 1000 * 2.0 ** -10                                     # active power 2^-10 at a[j] = 1000: D[j] = 6.02 (5 - j) + ...
    A = 10 * np.log10(sq / counts[:12].astype(np.float64))
    D = A - 20 * np.log10(2.0 ** (np.arange(12) - 15.0))
    j = int(np.flatnonzero(D <= 15.9)[0])
    assert j >= 1 and D[j - 1] > 15.9
    t = (D[j - 1] - 15.9) / (D[j - 1] - D[j])
    want = 10 ** ((A[j - 1] + t * (A[j] - A[j - 1])) / 10)
    active, activity = metrics.p56_level(sq, 4000, counts)
    assert abs(active / want - 1) <= 1e-14 and abs(activity * active / (sq / 4000) - 1) <= 1e-15
    assert np.isnan(metrics.p56_level(sq, 4000, counts, margin_db=200.0)[0])          # D[0] below the margin
    assert np.isnan(metrics.p56_level(sq, 4000, counts, margin_db=-200.0)[0])         # the counts run out before a crossing
    assert np.isnan(metrics.p56_level(float('inf'), 4000, counts)[0])


def test_undefined_levels_are_nan():
    for x in (np.zeros(0, dtype=np.float32), np.zeros(5000, dtype=np.float32), C.gated_bursts(5000, 16000, 1, amplitude=1e-6, floor=1e-6)):
        r = metrics.active_speech_level(x, 16000)
        assert np.isnan(r['active_power']) and np.isnan(r['activity']) and r['counts'].tolist() == [0] * 15
    with pytest.raises(ValueError):
        metrics.active_speech_level(np.zeros((2, 100)), 16000)
    with pytest.raises(ValueError):
        metrics.active_speech_level(np.zeros(100), 16000.5)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------

def test_entry_point_is_declared_exported_and_bound():
    name = 'dcs_active_level_ragged_f64'
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'dcsnet_hip.h')).read(), flags=re.S)
    assert re.search(r'\b' + name + r'\s*\(', header), f'{name} is not declared in include/dcsnet_hip.h'
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f'{name} is not exported'
    assert name in _lib.SIGNATURES
    assert _lib.load().dcs_abi_version() == 20                # an entry point was added, nothing else changed


def test_argument_errors_come_before_any_launch():
    call = _lib.load().dcs_active_level_ragged_f64
    # x, offsets, n, total, fs, margin_db, out, counts, stream
    args = [P, P, 3, 1000, 16000, 15.9, P, P, None]
    for i in (0, 1, 6):                                       # every required pointer
        a = list(args)
        a[i] = None
        assert call(*a) == BAD, i
    for i, v in ((2, 0), (2, -1), (2, 32768), (3, -1), (4, 7999), (4, 48001), (4, 0)):
        a = list(args)
        a[i] = v
        assert call(*a) == BAD, (i, v)
    # a NULL counts passes the check: with nothing else to object to, the same call with a bad rate is still what fails
    a = list(args)
    a[7] = None
    a[4] = 7999
    assert call(*a) == BAD


def test_python_layer_rejects_before_any_launch():
    x, off = torch.zeros(1000), torch.tensor([0, 400, 1000])
    with pytest.raises(_lib.DcsHipError):
        ops.active_level_ragged(x, off, 16000)                # CPU tensors: there is no fallback
    assert ops.ACTIVE_LEVEL_TILE == 4096


# ---- the store and the tools ---------------------------------------------------------------------------------------------------------

def test_store_rejects_an_unknown_level_before_touching_the_device():
    """No device is named that exists here: the ValueError comes first."""
    from dcsnet.config import config
    x = [np.ones(9000, dtype=np.float32)]
    for kw in ({'level': 'rms'}, {'noise_level': 'P56'}, {'level': None}):
        with pytest.raises(ValueError, match='expected one of'):
            MixingAudioStore(x, x, config, 'cuda:0', **kw)


def _tool(name):
    spec = importlib.util.spec_from_file_location('dcs_tools_' + name, os.path.join(REPO, 'tools', name + '.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_tools_take_the_level_switches(capsys):
    from dcsnet.audio_store import LEVELS
    train, mix = _tool('train'), _tool('mix')
    assert train.LEVELS == mix.LEVELS == LEVELS == ('power', 'p56')
    base = ['dcs', '--clean-dir', 'c', '--out', 'o', '--noise-dir', 'd']
    a = train.parse_args(base)
    assert (a.level, a.noise_level) == ('power', 'power')
    a = train.parse_args(base + ['--level', 'p56'])
    assert (a.level, a.noise_level) == ('p56', 'power')
    a = train.parse_args(base + ['--level', 'p56', '--noise-level', 'p56'])
    assert (a.level, a.noise_level) == ('p56', 'p56')
    for extra in (['--level', 'rms'], ['--noise-level', 'P.56']):
        with pytest.raises(SystemExit) as err:
            train.parse_args(base + extra)
        assert err.value.code == 2 and 'invalid choice' in capsys.readouterr().err
    with pytest.raises(SystemExit):                           # pre-mixed pairs have no level to choose
        train.parse_args(['dcs', '--clean-dir', 'c', '--out', 'o', '--noisy-dir', 'n', '--level', 'p56'])
    assert '--noise-dir' in capsys.readouterr().err
    a = mix.parse_args(['c', 'd', '--out', 'o'])
    assert (a.level, a.noise_level) == ('power', 'power')
    a = mix.parse_args(['c', 'd', '--out', 'o', '--level', 'p56', '--noise-level', 'p56'])
    assert (a.level, a.noise_level) == ('p56', 'p56')
    for extra in (['--level', 'rms'], ['--noise-level', '']):
        with pytest.raises(SystemExit) as err:
            mix.parse_args(['c', 'd', '--out', 'o'] + extra)
        assert err.value.code == 2
    capsys.readouterr()
