"""CPU-only: the device validation route's host side — the new C entry point's declaration, export and argument handling (every
call below fails validation before any launch), the fold rule restated in dcsnet/validation.py against a transcription of the
reference's two rules, and the switches of fit / tools/train.py."""
import ctypes
import math
import os
import re
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float('nan'), float('inf')


@pytest.fixture(scope='module')
def lib():
    from dcsnet import _lib
    return _lib.load()


def test_entry_point_is_declared_exported_and_bound(lib):
    from dcsnet import _lib
    header = open(os.path.join(REPO, 'include', 'dcsnet_hip.h')).read()
    assert re.search(r'\bint\s+dcs_val_accumulate_f32\s*\(const float\* losses, int n_loss, const float\* scores, int n_scores, '
                     r'int B, double\* state,\s*dcs_stream_t stream\);', header)
    assert 'dcs_val_accumulate_f32' in _lib.SIGNATURES
    assert hasattr(lib, 'dcs_val_accumulate_f32')
    res, args = _lib.SIGNATURES['dcs_val_accumulate_f32']
    assert res is ctypes.c_int and len(args) == 7
    assert lib.dcs_abi_version() == 20                                   # a new entry point only: no signature changed


def test_header_layout_matches_the_python_constants():
    from dcsnet import ops
    header = open(os.path.join(REPO, 'include', 'dcsnet_hip.h')).read()
    want = {'DCS_VAL_STATE': ops.VAL_STATE, 'DCS_VAL_MAX_SCORES': ops.VAL_MAX_SCORES, 'DCS_VAL_LOSS_SUM': ops.VAL_LOSS_SUM,
            'DCS_VAL_SCORE_SUM': ops.VAL_SCORE_SUM, 'DCS_VAL_KEPT': ops.VAL_KEPT, 'DCS_VAL_SKIPPED': ops.VAL_SKIPPED,
            'DCS_VAL_SCORE_NAN': ops.VAL_SCORE_NAN}
    for name, value in want.items():
        m = re.search(rf'#define {name}\s+(\d+)', header)
        assert m and int(m.group(1)) == value, name
    # the fields do not overlap: 3 loss sums, 4 score sums, 2 counts, 4 NaN counts inside 16 doubles
    assert ops.VAL_LOSS_SUM + 3 <= ops.VAL_SCORE_SUM and ops.VAL_SCORE_SUM + ops.VAL_MAX_SCORES <= ops.VAL_KEPT
    assert ops.VAL_KEPT < ops.VAL_SKIPPED < ops.VAL_SCORE_NAN and ops.VAL_SCORE_NAN + ops.VAL_MAX_SCORES <= ops.VAL_STATE


@pytest.mark.parametrize('args', [
    (None, 3, 64, 1, 4, 64),            # null losses
    (64, 3, 64, 1, 4, None),            # null state
    (64, 0, 64, 1, 4, 64),              # n_loss not in {1, 3}
    (64, 2, 64, 1, 4, 64),
    (64, 4, 64, 1, 4, 64),
    (64, 3, 64, -1, 4, 64),             # n_scores outside [0, 4]
    (64, 3, 64, 5, 4, 64),
    (64, 3, None, 1, 4, 64),            # scores missing
    (64, 1, None, 2, 4, 64),
    (64, 3, 64, 1, 0, 64),              # B < 1
    (64, 3, None, 0, 0, 64),
    (64, 1, 64, 2, -3, 64),
])
def test_bad_arguments_are_refused_before_any_launch(lib, args):
    # (the non-null "device pointers" are never dereferenced: every case fails the host-side checks)
    assert lib.dcs_val_accumulate_f32(*args, None) == -1         # DCS_ERR_BADARG


# ---- the fold rule ---------------------------------------------------------------------------------------------------------

def _ref_calc_metric(scores):
    """network_functions.py:152-166 (calc_metric) over already computed per-utterance scores."""
    vals = []
    for v in scores:
        if v == v:
            vals.append(v)
    return float(sum(vals)) / max(len(vals), 1)


def _ref_epoch(rows):
    """validation_step (c_network.py:298-300: a NaN loss returns None) and _epoch_end (None outputs dropped, then the mean of the
    batch metrics), in double."""
    outs = []
    for losses, scores in rows:
        metrics = {f'loss{k}': v for k, v in enumerate(losses)}
        metrics.update({f'score{r}': _ref_calc_metric(row) for r, row in enumerate(scores)})
        if torch.any(torch.isnan(torch.tensor(losses[-1]))):
            outs.append(None)
            continue
        outs.append(metrics)
    skipped = sum(o is None for o in outs)
    outs = [o for o in outs if o is not None]
    keys = outs[0].keys() if outs else []
    return ({k: float(torch.stack([torch.as_tensor(o[k], dtype=torch.float64) for o in outs]).mean()) for k in keys}, len(outs), skipped)


ROWS3 = [
    ([1.5, -12.25, -10.75], [[0.5, 0.75, NAN, 0.25]]),
    ([NAN, NAN, NAN], [[0.9, 0.9, 0.9, 0.9]]),                   # a NaN loss: the whole batch is skipped
    ([1.25, INF, INF], [[0.125, 0.5, 0.25, 0.0]]),               # +Inf is kept and propagates
    ([1.0, -3.0, -2.0], [[NAN, NAN, NAN, NAN]]),                 # an all-NaN score row contributes 0.0
    ([0.5, -8.0, -7.5], [[0.6]]),                                # the smaller last batch counts as one batch
]


def _same(a, b):
    return (a != a and b != b) or a == b or abs(a - b) <= 1e-12 * max(abs(a), abs(b))


@pytest.mark.parametrize('rows', [ROWS3, ROWS3[:2], [ROWS3[0], ROWS3[3], ROWS3[4]], [ROWS3[4]], [ROWS3[1]], [],
                                  [([v[1]], s + [list(reversed(s[0]))]) for v, s in ROWS3]],
                         ids=['all', 'nan-skip', 'finite', 'lone', 'none-kept', 'empty', 'one-loss-two-scores'])
def test_fold_rule_is_the_references(rows):
    from dcsnet import ops
    from dcsnet.validation import epoch_means, fold_batches
    state = fold_batches(rows)
    assert len(state) == ops.VAL_STATE
    want, kept, skipped = _ref_epoch(rows)
    assert state[ops.VAL_KEPT] == kept and state[ops.VAL_SKIPPED] == skipped
    n_loss = len(rows[0][0]) if rows else 3
    n_scores = len(rows[0][1]) if rows else 1
    means = epoch_means(state, n_loss, n_scores)
    if kept == 0:
        assert means is None and not want
        assert all(v == 0 for i, v in enumerate(state) if i != ops.VAL_SKIPPED)
        return
    loss, score = means
    for k in range(n_loss):
        assert _same(loss[k], want[f'loss{k}']), (k, loss[k], want[f'loss{k}'])
    for r in range(n_scores):
        assert _same(score[r], want[f'score{r}']), (r, score[r], want[f'score{r}'])
        nans = sum(sum(v != v for v in s[r]) for lo, s in rows if lo[-1] == lo[-1])
        assert state[ops.VAL_SCORE_NAN + r] == nans


def test_fold_rule_by_hand():
    from dcsnet import ops
    from dcsnet.validation import epoch_means, fold_batches
    state = fold_batches([ROWS3[0], ROWS3[1], ROWS3[3], ROWS3[4]])
    assert (state[ops.VAL_KEPT], state[ops.VAL_SKIPPED], state[ops.VAL_SCORE_NAN]) == (3, 1, 5)
    loss, score = epoch_means(state, 3, 1)
    assert loss == [(1.5 + 1.0 + 0.5) / 3, (-12.25 - 3.0 - 8.0) / 3, (-10.75 - 2.0 - 7.5) / 3]
    assert score == [(0.5 + 0.0 + 0.6) / 3]
    assert math.isinf(epoch_means(fold_batches(ROWS3), 3, 1)[0][2])


# ---- the switches ----------------------------------------------------------------------------------------------------------

def test_fit_refuses_an_unknown_validation_route_before_any_device_work(tmp_path):
    from dcsnet.fit import fit
    out = tmp_path / 'never'
    with pytest.raises(ValueError, match='validation'):
        fit(None, None, None, str(out), 1, 2, validation='gpu')
    assert not out.exists()                                     # raised before anything was made


def test_fit_default_is_the_host_route():
    import inspect
    from dcsnet.fit import fit
    assert inspect.signature(fit).parameters['validation'].default == 'host'


def test_train_tool_lists_the_flag():
    r = subprocess.run([sys.executable, os.path.join(REPO, 'tools', 'train.py'), '--help'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert '--validation' in r.stdout and '{host,device}' in r.stdout
