"""CPU-only: the host side of mixing clean speech and noise at drawn SNRs (dcsnet/audio_store.py: draw_mix, mix_gain), the C ABI
of the device kernels (csrc/audio_mix.hip: every call here fails validation before any launch) and the command line of
tools/train.py with --noise-dir."""
import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

from dcsnet import _lib, ops
from dcsnet.audio_store import SNR_LEVELS_DB, draw_crop_starts, draw_mix, mix_gain

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = -1                                                      # DCS_ERR_BADARG
P = ctypes.c_void_p(16)                                       # never dereferenced
NEW = ('dcs_signal_power_ragged_f64', 'dcs_audio_mix_ragged_f32', 'dcs_audio_mix_stft_batch_f32')


# ---- draw_mix ------------------------------------------------------------------------------------------------------------------

NOISE_LENGTHS = [100, 48000, 7, 160001]


def test_draw_order_is_the_documented_one():
    """Per item, in batch order: the noise recording, its start, the SNR level — replayed by hand from the same seed."""
    idx = [4, 0, 4, 2, 1]
    got = draw_mix(idx, NOISE_LENGTHS, torch.Generator().manual_seed(5))
    g = torch.Generator().manual_seed(5)
    want = ([], [], [])
    for _ in idx:
        r = int(torch.randint(0, len(NOISE_LENGTHS), (1,), generator=g))
        want[0].append(r)
        want[1].append(int(torch.randint(0, NOISE_LENGTHS[r], (1,), generator=g)))
        want[2].append(float(SNR_LEVELS_DB[int(torch.randint(0, len(SNR_LEVELS_DB), (1,), generator=g))]))
    assert got == want
    assert all(0 <= r < 4 and 0 <= s < NOISE_LENGTHS[r] and v in (15.0, 10.0, 5.0, 0.0) for r, s, v in zip(*got))
    assert len(set(got[0])) > 1                               # (the seed does exercise more than one recording)


def test_draw_order_with_a_range_and_with_single_outcomes():
    idx = [0, 1, 2]
    got = draw_mix(idx, NOISE_LENGTHS, torch.Generator().manual_seed(6), snr_range=(-5.0, 20.0))
    g = torch.Generator().manual_seed(6)
    for b in range(3):
        r = int(torch.randint(0, 4, (1,), generator=g))
        s = int(torch.randint(0, NOISE_LENGTHS[r], (1,), generator=g))
        snr = -5.0 + 25.0 * float(torch.rand(1, dtype=torch.float64, generator=g))
        assert (got[0][b], got[1][b], got[2][b]) == (r, s, snr) and -5.0 <= snr < 20.0
    # one recording of one sample and one level: every draw is still made, so the generator advances as documented
    g1, g2 = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    assert draw_mix([0, 0], [1], g1, snr_db=[3.0]) == ([0, 0], [0, 0], [3.0, 3.0])
    for _ in range(2):
        torch.randint(0, 1, (1,), generator=g2), torch.randint(0, 1, (1,), generator=g2), torch.randint(0, 1, (1,), generator=g2)
    assert torch.equal(g1.get_state(), g2.get_state())
    with pytest.raises(ValueError):
        draw_mix([0], [])
    with pytest.raises(ValueError):
        draw_mix([0], [5, 0])
    with pytest.raises(ValueError):
        draw_mix([0], [5], snr_db=[])
    with pytest.raises(ValueError):
        draw_mix([0], [5], snr_range=(3.0, 1.0))


def test_a_restored_generator_repeats_the_draws():
    g = torch.Generator().manual_seed(8)
    draw_mix([0, 1, 2], NOISE_LENGTHS, g)                     # somewhere in the middle of a run
    state = g.get_state()
    first = draw_mix([3, 4, 5, 6], NOISE_LENGTHS, g)
    after = g.get_state()
    resumed = torch.Generator()
    resumed.set_state(state)
    assert draw_mix([3, 4, 5, 6], NOISE_LENGTHS, resumed) == first
    assert torch.equal(resumed.get_state(), after)
    assert draw_mix([3, 4, 5, 6], NOISE_LENGTHS, g) != first    # (and the run itself goes on to other mixtures)


def test_crop_starts_come_first_and_equal_the_paired_stores():
    """A mixing store draws all crop starts, then the mixtures: the starts are draw_crop_starts' from the same seed, and the
    mixture draws are draw_mix's from the state that leaves."""
    lengths, idx, crop = [9000, 4000, 8160, 20000, 8161], [3, 0, 1, 4, 2, 3], 8160
    g = torch.Generator().manual_seed(9)
    starts = draw_crop_starts(lengths, idx, crop, g)
    mixes = draw_mix(idx, NOISE_LENGTHS, g)
    assert starts == draw_crop_starts(lengths, idx, crop, torch.Generator().manual_seed(9))
    h = torch.Generator().manual_seed(9)
    for i in idx:                                             # by hand: crop_batch's draws, none for an item not longer than the crop
        if lengths[i] > crop:
            torch.randint(0, lengths[i] - crop, (1,), generator=h)
    assert draw_mix(idx, NOISE_LENGTHS, h) == mixes


# ---- mix_gain ----------------------------------------------------------------------------------------------------------------------

def test_mix_gain_is_the_formula_rounded_once():
    for pc, pn, snr in ((0.01, 0.0025, 0.0), (3.1e-3, 7.7e-5, 17.5), (1e-6, 0.2, -5.0), (0.02, 0.02, 15.0)):
        g = mix_gain(pc, pn, snr)
        assert isinstance(g, np.float32)
        want = math.sqrt(pc / pn) * 10.0 ** (-snr / 20.0)     # float64
        assert abs(float(g) - want) <= 2.0 ** -24 * want * (1 + 1e-9), (pc, pn, snr)      # half a float32 ulp: one rounding
        # and it does what it is for: gain^2 Pn is snr dB below Pc
        assert abs(10 * math.log10(pc / (float(g) ** 2 * pn)) - snr) <= 1e-6
    g = mix_gain(np.array([0.01, 0.02]), np.array([0.01, 0.005]), np.array([0.0, 20.0]))
    assert g.dtype == np.float32 and g.shape == (2,) and g.tolist() == [1.0, np.float32(0.2)]
    assert mix_gain(0.5, 0.5, 0) == np.float32(1.0)


@pytest.mark.parametrize('pc, pn', [(0.0, 1.0), (1.0, 0.0), (float('nan'), 1.0), (1.0, float('nan')), (-1.0, 1.0), (1.0, -1e-3),
                                    (float('inf'), 1.0), (1.0, float('inf'))])
def test_mix_gain_rejects_powers_that_give_no_snr(pc, pn):
    with pytest.raises(ValueError):
        mix_gain(pc, pn, 5.0)
    with pytest.raises(ValueError):
        mix_gain(np.array([1.0, pc]), np.array([1.0, pn]), np.array([5.0, 5.0]))


def test_mix_gain_rejects_a_bad_snr_or_a_gain_outside_float32():
    with pytest.raises(ValueError):
        mix_gain(1.0, 1.0, float('nan'))
    with pytest.raises(ValueError):
        mix_gain(1.0, 1e-300, -400.0)
    with pytest.raises(ValueError):
        mix_gain(1e-300, 1.0, 400.0)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

def test_new_entry_points_are_declared_exported_and_bound():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'dcsnet_hip.h')).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', header), f'{name} is not declared in include/dcsnet_hip.h'
        assert hasattr(lib, name), f'{name} is not exported'
        assert name in _lib.SIGNATURES
    assert _lib.load().dcs_abi_version() == 20                # entry points were added, nothing else changed


def _each_bad(call, args, pointers, values):
    assert all(args[i] is P for i in pointers)
    for i in pointers:
        a = list(args)
        a[i] = None
        assert call(*a) == BAD, i
    for i, v in values:
        a = list(args)
        a[i] = v
        assert call(*a) == BAD, (i, v)


def test_argument_errors_come_before_any_launch():
    lib = _lib.load()
    # x, offsets, n, total, out, stream
    _each_bad(lib.dcs_signal_power_ragged_f64, [P, P, 3, 1000, P, None], (0, 1, 4), ((2, 0), (2, -1), (3, -1)))
    # clean, offsets, n_items, total, noise, noise_offsets, n_noise, noise_index, noise_start, gain, noisy, stream
    _each_bad(lib.dcs_audio_mix_ragged_f32, [P, P, 3, 1000, P, P, 2, P, P, P, P, None], (0, 1, 4, 5, 7, 8, 9, 10),
              ((2, 0), (2, -1), (3, -1), (6, 0), (6, -2)))
    # clean, offsets, n_items, noise, noise_offsets, n_noise, item_index, item_start, noise_index, noise_start, gain, B, window,
    # n_fft, T, hop, scale, out_noise, out_noisy, out_clean, stream
    args = [P, P, 3, P, P, 2, P, P, P, P, P, 4, P, 512, 256, 32, 1.0, P, P, P, None]
    _each_bad(lib.dcs_audio_mix_stft_batch_f32, args, (0, 1, 3, 4, 6, 7, 8, 9, 10, 12, 17, 18, 19),
              ((2, 0), (2, -1), (5, 0), (5, -1), (11, 0), (11, -1), (11, 65536), (13, 256), (13, 1024), (14, 1), (14, 0), (15, 0),
               (15, -32), (14, 9)))                           # T = 9 at hop 32: a crop of 256 samples, not more


def test_python_layer_rejects_before_any_launch():
    x, off = torch.zeros(1000), torch.tensor([0, 400, 1000])
    i32 = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(_lib.DcsHipError):
        ops.signal_power_ragged(x, off)
    with pytest.raises(_lib.DcsHipError):
        ops.audio_mix_ragged(x, off, x, off, i32, i32, torch.ones(2))
    with pytest.raises(_lib.DcsHipError):
        ops.audio_mix_stft_batch(x, off, x, off, i32, i32, i32, i32, torch.ones(2), torch.hann_window(512), 256, 32, 512 ** -0.5)


# ---- tools/train.py --------------------------------------------------------------------------------------------------------------------

def _tool(name):
    spec = importlib.util.spec_from_file_location('dcs_tools_' + name, os.path.join(REPO, 'tools', name + '.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_train_tool_takes_exactly_one_source_of_noisy_speech(capsys):
    tool = _tool('train')
    base = ['dcs', '--clean-dir', 'c', '--out', 'o']
    a = tool.parse_args(base + ['--noisy-dir', 'n'])
    assert (a.noisy_dir, a.noise_dir, a.snr_db, a.snr_range) == ('n', None, None, None)
    a = tool.parse_args(base + ['--noise-dir', 'd'])
    assert (a.noisy_dir, a.noise_dir, a.snr_db, a.snr_range) == (None, 'd', None, None)
    a = tool.parse_args(base + ['--noise-dir', 'd', '--snr-db', '17.5,12.5,2.5'])
    assert a.snr_db == [17.5, 12.5, 2.5] and a.snr_range is None
    a = tool.parse_args(base + ['--noise-dir', 'd', '--snr-range', '-5', '20'])
    assert a.snr_range == [-5.0, 20.0] and a.snr_db is None
    for extra, word in ((['--noisy-dir', 'n', '--noise-dir', 'd'], 'exactly one'),
                        ([], 'exactly one'),
                        (['--noise-dir', 'd', '--snr-db', '15,5', '--snr-range', '0', '10'], 'exclude'),
                        (['--noisy-dir', 'n', '--snr-db', '15,5'], '--noise-dir'),
                        (['--noise-dir', 'd', '--snr-range', '10', '0'], 'LO'),
                        (['--noise-dir', 'd', '--snr-db', 'loud'], 'dB')):
        with pytest.raises(SystemExit) as err:
            tool.parse_args(base + extra)
        assert err.value.code == 2
        assert word in capsys.readouterr().err, extra
    with pytest.raises(SystemExit):                           # the mode still comes first
        tool.parse_args(['--clean-dir', 'c', 'dcs', '--noisy-dir', 'n', '--out', 'o'])
    capsys.readouterr()


def test_mix_tool_pcm_conversion_and_arguments(capsys):
    tool = _tool('mix')
    pcm, clipped = tool.to_pcm16(np.array([0.0, 0.5, -0.5, 1.0, -1.0, 1.5, 3e-5, 0.99998], dtype=np.float32))
    assert pcm.dtype == np.int16 and pcm.tolist() == [0, 16384, -16384, 32767, -32767, 32767, 1, 32767] and clipped == 3
    a = tool.parse_args(['c', 'd', '--out', 'o', '--snr-range', '0', '10', '--seed', '4'])
    assert (a.clean_dir, a.noise_dir, a.out, a.snr_range, a.seed) == ('c', 'd', 'o', [0.0, 10.0], 4)
    with pytest.raises(SystemExit):
        tool.parse_args(['c', 'd', '--out', 'o', '--snr-db', '5', '--snr-range', '0', '10'])
    capsys.readouterr()
