"""CPU-only: the argument handling of the ragged scoring entry points (csrc/stoi_ragged.hip), the host arithmetic of the ragged
STOI workspace, the RecordingScorer's pairing checks (they run before anything touches the device) and the command-line tool's
argument parser.  No launch is made here — every call fails validation first or is pure host arithmetic."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dcsnet import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, WORKSPACE = -1, -3                                       # DCS_ERR_BADARG, DCS_ERR_WORKSPACE
P = ctypes.c_void_p(16)                                       # never dereferenced


def _fails_where(call, args, positions, value=None):
    for i in positions:
        a = list(args)
        a[i] = value
        assert call(*a) == BAD, (call.__name__, i)


def test_abi_version_is_unchanged():
    assert _lib.load().dcs_abi_version() == 20


def test_resample_poly_ragged_rejects_bad_arguments():
    lib = _lib.load()
    args = [P, P, 3, 1000, P, P, 700, P, 5, 5, 8, None]        # x, offsets, n, total, y, out_offsets, capacity, h, taps, up, down
    _fails_where(lib.dcs_resample_poly_ragged_f32, args, (0, 1, 4, 5, 7))
    _fails_where(lib.dcs_resample_poly_ragged_f32, args, (2, 8, 9, 10), 0)
    _fails_where(lib.dcs_resample_poly_ragged_f32, args, (2, 3, 6), -1)
    _fails_where(lib.dcs_resample_poly_ragged_f32, args, (8,), 4)                   # even tap count
    _fails_where(lib.dcs_resample_poly_ragged_f32, args, (2,), 40000)


def test_stoi_ragged_rejects_bad_arguments_and_short_workspaces():
    lib = _lib.load()
    ws = lib.dcs_stoi_ragged_workspace_bytes(3, 30000)
    assert ws > 0
    args = [P, P, P, 3, 30000, 12000, P, P, P, P, P, ws, None]   # clean, est, offsets, n, total, longest, lo, hi, d, kept, ws, bytes
    _fails_where(lib.dcs_stoi_ragged_f32, args, (0, 1, 2, 6, 7, 8, 9, 10))
    _fails_where(lib.dcs_stoi_ragged_f32, args, (3,), 0)
    _fails_where(lib.dcs_stoi_ragged_f32, args, (3, 4, 5), -1)
    _fails_where(lib.dcs_stoi_ragged_f32, args, (3,), 40000)
    a = list(args)
    a[11] = ws - 1
    assert lib.dcs_stoi_ragged_f32(*a) == WORKSPACE
    for n, total in ((0, 100), (-1, 100), (3, -1), (40000, 100)):
        assert lib.dcs_stoi_ragged_workspace_bytes(n, total) < 0, (n, total)
    for n, total in ((1, 0), (1, 1), (5, 257), (824, 20_000_000)):
        assert lib.dcs_stoi_ragged_workspace_bytes(n, total) > 0, (n, total)


def test_sisnr_ragged_rejects_bad_arguments():
    lib = _lib.load()
    args = [P, P, P, 3, 1000, P, None]                         # clean, est, offsets, n, total, out
    _fails_where(lib.dcs_sisnr_ragged_f32, args, (0, 1, 2, 5))
    _fails_where(lib.dcs_sisnr_ragged_f32, args, (3,), 0)
    _fails_where(lib.dcs_sisnr_ragged_f32, args, (3, 4), -1)


def test_stoi_ragged_workspace_follows_the_total_length():
    """One 300,000-sample recording among 99 of 20,000 samples: the workspace is sized by the 2.28 M samples there are, not by
    100 x the longest — well under a third of what 100 recordings of 300,000 samples need, and no more than the batched
    layout's own bytes per sample."""
    lib = _lib.load()
    mixed = lib.dcs_stoi_ragged_workspace_bytes(100, 300_000 + 99 * 20_000)
    uniform = lib.dcs_stoi_ragged_workspace_bytes(100, 100 * 300_000)
    assert 0 < mixed < uniform / 3 / 2, (mixed, uniform)
    assert uniform <= 1.05 * lib.dcs_stoi_workspace_bytes(100, 300_000) + 4096
    assert lib.dcs_stoi_ragged_workspace_bytes(100, 2 * 2_280_000) > 1.9 * mixed - 4096      # grows with the total


def test_ragged_python_layer_rejects_cpu_tensors():
    from dcsnet import metrics, ops
    x, off = torch.zeros(1000), torch.tensor([0, 400, 1000])
    with pytest.raises(_lib.DcsHipError):
        metrics.stoi_ragged(x, x, off, 16000)
    with pytest.raises(_lib.DcsHipError):
        metrics.sisnr_ragged(x, x, off)
    with pytest.raises(_lib.DcsHipError):
        ops.stoi_ragged(x, x, off, 600)
    with pytest.raises(_lib.DcsHipError):
        ops.sisnr_ragged(x, x, off)
    with pytest.raises(_lib.DcsHipError):
        ops.resample_poly_ragged(x, off, torch.ones(5), 5, 8)


def test_scorer_refuses_unpaired_input_before_touching_the_device():
    from dcsnet.enhance import Enhancer
    from dcsnet.evaluate import RecordingScorer
    with pytest.raises(TypeError):
        RecordingScorer(object())
    scorer = RecordingScorer(Enhancer.__new__(Enhancer))       # no network behind it: the checks below come first
    a, b, c = (np.zeros(n, np.float32) for n in (1500, 2017, 2016))
    with pytest.raises(ValueError, match='2 noisy recordings for 1 clean'):
        scorer.score([a, b], [a], 16000)
    with pytest.raises(ValueError, match='item 1: clean_data and noisy_data are not the same length'):
        scorer.score([a, b], [a, c], 16000)
    with pytest.raises(ValueError, match='no recordings'):
        scorer.score([], [], 16000)
    with pytest.raises(ValueError, match='2 noisy files for 1 clean'):
        scorer.score_files(['a.wav', 'b.wav'], ['a.wav'])


def test_summarise_leaves_nans_out_and_counts_them():
    from dcsnet.evaluate import summarise
    nan = float('nan')
    scores = {'stoi': torch.tensor([0.5, nan, 0.7]), 'stoi_noisy': torch.tensor([0.4, 0.5, 0.5]),
              'sisnr': torch.tensor([10.0, 12.0, 14.0]), 'sisnr_noisy': torch.tensor([5.0, 5.0, nan])}
    s, table = summarise(scores)
    assert table.shape == (3, 4) and s['files'] == 3
    assert s['stoi'] == pytest.approx(0.6) and s['stoi_nan'] == 1 and s['stoi_noisy_nan'] == 0
    assert s['sisnr'] == pytest.approx(12.0) and s['sisnr_noisy'] == pytest.approx(5.0) and s['sisnr_noisy_nan'] == 1
    assert s['stoi_improvement'] == pytest.approx(0.15) and s['sisnr_improvement'] == pytest.approx(6.0)


def test_evaluate_tool_help():
    r = subprocess.run([sys.executable, os.path.join(REPO, 'tools', 'evaluate.py'), '--help'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert '--checkpoint' in r.stdout and 'noisy_dir' in r.stdout and '--csv' in r.stdout


def test_the_measure_groups_table_orders_the_keys_and_signs_the_improvements():
    """All 16 settings of the four switches: scorer.metrics is METRICS plus the switched-on groups' tuples in the table's order.
    summarise() on a dict of those keys, key number i holding i + 0.5 if it is a _noisy key and i otherwise: the columns come
    back in that order, and each improvement is enhanced - noisy, or noisy - enhanced for llr, cd and wss.  With these values
    the right answer for a measure at column i is -1.5 (+1.5 where lower is better); the operands swapped give the other sign,
    and any other column in either place an amount that is not 1.5."""
    import itertools
    from dcsnet.enhance import Enhancer
    from dcsnet.evaluate import MEASURE_GROUPS, RecordingScorer, summarise
    switches = ('extended', 'frame_measures', 'spectral_measures', 'sdr')
    tuples = (RecordingScorer.EXTENDED, RecordingScorer.FRAME_MEASURES, RecordingScorer.SPECTRAL_MEASURES, RecordingScorer.SDR)
    assert tuple(g.switch for g in MEASURE_GROUPS) == (None,) + switches
    assert tuple(g.keys for g in MEASURE_GROUPS) == (RecordingScorer.METRICS,) + tuples
    lower = {k for g in MEASURE_GROUPS for k in g.lower_is_better}
    assert lower == {'llr', 'cd', 'wss'}
    for setting in itertools.product((False, True), repeat=4):
        scorer = RecordingScorer(Enhancer.__new__(Enhancer), extended=setting[0])
        for name, on in zip(switches[1:], setting[1:]):
            setattr(scorer, name, on)
        keys = RecordingScorer.METRICS + sum((t for t, on in zip(tuples, setting) if on), ())
        assert scorer.metrics == keys, setting
        scores = {k: torch.full((3,), i + 0.5 * k.endswith('_noisy')) for i, k in enumerate(keys)}
        summary, table = summarise(dict(reversed(list(scores.items()))))              # the dict's own order does not count
        assert table.shape == (3, len(keys)) and all((table[:, i] == scores[k].numpy()).all() for i, k in enumerate(keys))
        measures = [k for k in keys if not k.endswith('_noisy')]
        assert list(summary) == ['files'] + [k + s for k in keys for s in ('', '_nan')] + [k + '_improvement' for k in measures]
        for k in measures:
            assert summary[k + '_improvement'] == (1.5 if k in lower else -1.5), (setting, k)
