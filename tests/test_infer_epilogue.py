"""The folded inference epilogue of every conv kernel — conv + bias, the eval-mode CBN's six coefficients per channel
(re' = q0 re + q1 im + q4, im' = q2 re + q3 im + q5), activation, as ONE kernel (F.cconv2d_cbn_eval -> dcs_cconv2d_fwd_affine:
encoder stages 0-6 and decoder stages 0-5 at inference) — against fp64, one epilogue copy at a time.

The epilogue is written out in seven places (cconv_mfma_kernel with one and several K waves, the 16-column kernel,
splitk_reduce_kernel, the ring kernel, the conv_enc0.hip kernels, cconv_direct_body, and the bf16-storage builds of all of
them) and has been silently wrong once (conv_mfma.hip's epilogue comment, profiles/r03_pk_fma_op_sel_hazard.txt: q1 * im
missing in ~300 of 4 M outputs, other elements every run).  The whole-network checks cannot see such a fault: their CBN
states (seeded_state.fill_state) have small cross terms, and a few hundred mid-network elements drown in 2e-4 on the mask.
So every CBN state here has LARGE cross coefficients (oracle/layer_fp64.eval_cbn_state: min(|q1|, |q2|) >= 0.25 max(|q0|, |q3|)).

  CPU   the coefficient condition; the comparator on every row of the table at batch 1 (accepts a second correct fp32
        evaluation, refuses six planted epilogue faults of 16 elements each); the oracle modules against the closed form.
  A     every element of every row of tests/_plan_probe.py's table (P1 .. P8: each epilogue copy and each way into it)
        against oracle modules in fp64, in the modes 'bf16x6', 'f32', 'bf16' (bf16-representable operands there: the
        products are then exact and the same tolerance holds), with the activations the network uses + none + sigmoid.
        The plan probe (a child process under DCS_MFMA_TRACE=1) shows that each row takes the plan it is in the table for.
  B     bf16 storage: the _h entry point's output equals the fp32 entry point's rounded once to bf16.
  C     the folded form is bit-identical to conv (no activation) followed by ops.cbn (cbn_apply_kernel), as the kernels'
        comments promise — on every tier-A row, and three times over on shapes that fill the chip (>= 768 workgroups, so
        epilogues run beside other workgroups' bf16 MFMAs), the runs bit-identical with each other.
  D     the coefficient kernel against the closed form in fp64 (C = 1, 8, 64, 128, one nearly singular state), and the
        network's wiring: C_NETWORK's own encoder / decoder stage through F.cconv2d_cbn_eval with bn.eval_coef().

Rule (oracle/rnet_layer_fp64.compare): err = max |got - ref64| / max |ref64| over every element <= 2e-5; where the fp32 CPU
evaluation of the oracle modules itself misses that, 16 x its error (recorded as a fallback).  Every figure goes to
infer_epilogue_parity.json in $DCS_PARITY_DIR (default parity_out/); a full run's file is committed as
profiles/infer_epilogue_parity.json.

Measured (MI355X, full run of the suite, profiles/infer_epilogue_parity.json): worst error / worst ratio to
the fp32 CPU evaluation's error per path over the three modes — P1 8.9e-7 / 2.0, P2 4.3e-7 / 1.8, P3 7.5e-7 / 2.8, P4 3.2e-7 /
1.5, P5 1.0e-6 / 2.3, P6 2.4e-7 / 1.4, P7 3.6e-7 / 1.2, P8 1.2e-6 / 3.6 (102 cases, the 16 x cpu32 fallback nowhere); folded ==
two-kernel form in all 99 cases that have one and in all 11 chip-filling ones, three runs each, 0 differing elements; the 11
bf16-storage rows equal; coefficient kernel 1.0e-7 .. 1.3e-7 (cpu32 6e-8 .. 1.7e-7), the nearly singular state 1.56e-5 against
1.39e-5 on the CPU — inside 2e-5, so without the fallback; wiring 2.7e-7 (enc2), 2.0e-7 (dec4).  The plan probe saw candidates
2, 3, 4, 5, 7, 8, 10, K slices 8 / 8 on both P4 rows, and no plan line on the P6 / P7 rows.  No kernel fault was found: the
copies without the scalar-FMA guard (splitk_reduce_kernel, cconv_direct_body) agree bit for bit with cbn_apply_kernel too.
"""
import functools
import os
import re
import subprocess
import sys

import pytest
import torch

from oracle import layer_fp64 as L64
from oracle import rnet_layer_fp64 as R64
import _plan_probe as P
from _ragged_helpers import record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ('bf16x6', 'f32', 'bf16')
LIVE = 0.2                     # share of the outputs each branch of an activation has to hold


_record = functools.partial(record, 'infer_epilogue_parity.json')     # figures -> $DCS_PARITY_DIR/infer_epilogue_parity.json (default parity_out/)


def _compare(got, ref, ref32):
    """The project's per-op rule on one tensor: (figures, missed?)."""
    rows, misses = R64.compare(dict(y=got), dict(y=ref), dict(y=ref32))
    return rows['y'], bool(misses)


# ------------------------------------------------------------------------------------------------ references (CPU)

_REFS = {}


def _refs(name, B=None, rounded=False):
    """{act: (y64, y32)}, pre64, case, state of one row — computed once, shared, never modified."""
    key = (name, B, rounded)
    for k in [k for k in _REFS if k[0] != name]:               # one row's references at a time (the tests run row by row)
        del _REFS[k]
    if key not in _REFS:
        row = P.ALL[name]
        case, state = P.row_case(name, B, rounded)
        out, pre = {}, {True: None, False: None}
        for act in row.acts:
            ys = []
            for wide in (True, False):
                r = L64.folded_reference(row.L, case, state, act, wide, P.EPS, pre=pre[wide])
                pre[wide] = r['pre']
                ys.append(r['y'])
            out[act] = tuple(ys)
        _REFS[key] = (out, pre[True], pre[False], case, state)
    return _REFS[key]


def _alternative_fp32(row, case, state, act):
    """A second correct fp32 evaluation in another order than the oracle modules': the four real convolutions written out,
    each as the sum of two convolutions over complementary (checkerboard) halves of the taps (test_layers_train_size.py's
    device), then the affine map with the fp32 coefficients, then the activation."""
    L = row.L
    m = ((torch.arange(L.k)[:, None] + torch.arange(L.k)[None, :]) % 2).float()
    zero = torch.zeros(L.Cout)
    xr, xi = case['x'].real, case['x'].imag
    re, im = L64.complex_conv_from_real(L, xr, xi, case['w_r'] * m, case['w_i'] * m, case['b_r'], case['b_i'])
    re2, im2 = L64.complex_conv_from_real(L, xr, xi, case['w_r'] * (1 - m), case['w_i'] * (1 - m), zero, zero)
    return L64.apply_coef(torch.complex(re + re2, im + im2), L64.eval_coef_reference(state, P.EPS, wide=False), act)


# ------------------------------------------------------------------------------------------------ CPU tests

D_CHANNELS = (1, 8, 64, 128)


def _d_state(C, hard=False):
    return L64.eval_cbn_state(C, 7000 + C + (1 if hard else 0), hard)


def test_table_respects_the_size_cap_and_names_every_path():
    assert {r.path for r in P.ROWS.values()} == set(P.PATHS)
    for name, row in P.ROWS.items():
        assert P.n_outputs(row) <= P.MAX_OUTPUTS, (name, P.n_outputs(row))
        assert row.acts[0] == ('lrelu' if row.L.transposed else 'relu'), name
        assert (row.path in ('P6', 'P7')) == (not row.cands), name
    assert any('sigmoid' in r.acts for r in P.ROWS.values()) and any('none' in r.acts for r in P.ROWS.values())
    p5 = [r.L for r in P.ROWS.values() if r.path == 'P5']
    assert all(L.Cout == 8 for L in p5) and {(L.C1 + L.C2) % 16 for L in p5} == {0, 8}
    assert all((r.L.C1 + r.L.C2) % 8 or r.L.Cout % 8 for r in P.ROWS.values() if r.path == 'P7')


def test_cross_coefficients_are_large_in_every_state_the_gpu_tests_use():
    states = {name: P.row_case(name, B=1)[1] for name in P.ALL}
    states.update({f'tier_d_C{C}': _d_state(C) for C in D_CHANNELS})
    states.update(parity_regression=L64.eval_cbn_state(128, 9), wiring_enc=L64.eval_cbn_state(32, 51), wiring_dec=L64.eval_cbn_state(16, 52))
    for name, st in states.items():
        for wide in (True, False):
            r = L64.cross_ratio(L64.eval_coef_reference(st, P.EPS, wide))
            assert r >= L64.CROSS_MIN, (name, wide, r)
    # the recipe itself: 200 draws of 128 channels (closed form, fp64)
    worst = min(L64.cross_ratio(L64.eval_coef_reference(L64.eval_cbn_state(128, s), P.EPS, True)) for s in range(200))
    assert worst >= L64.CROSS_MIN, worst
    # the hard state is hard: nearly singular covariance
    v = _d_state(64, hard=True)['running_covar']
    rho = (v[:, 2] / torch.sqrt(v[:, 0] * v[:, 1])).abs()
    assert float(rho.min()) >= 0.99 and float(rho.max()) <= 0.999
    # and fill_state's are not what this module needs: cross terms a fraction of the diagonal ones
    from oracle import cpt_oracle as cpt
    from oracle.seeded_state import fill_state
    bn = fill_state(cpt.ComplexBatchNorm2d(128), 3)
    weak = dict(weight=bn.weight.detach(), bias=bn.bias.detach(), running_mean=torch.view_as_real(bn.running_mean), running_covar=bn.running_covar)
    assert L64.cross_ratio(L64.eval_coef_reference(weak, P.EPS, True)) < L64.CROSS_MIN


@pytest.mark.parametrize('name', list(P.ROWS))
def test_comparator_accepts_a_second_fp32_evaluation_and_refuses_epilogue_faults(name):
    """Batch 1 of the row's own geometry: the written-out fp32 evaluation passes the rule, each planted fault (16 elements
    of one output row) fails it by more than ten times; both branches of the activation are live."""
    threads = L64.set_threads()
    try:
        row = P.ROWS[name]
        refs, pre64, pre32, case, state = _refs(name, B=1)
        coef64 = L64.eval_coef_reference(state, P.EPS, True)
        for act in row.acts:
            y64, y32 = refs[act]
            fig, missed = _compare(_alternative_fp32(row, case, state, act), y64, y32)
            assert not missed, (act, fig)
            faults = L64.epilogue_faults(y64, coef64, pre64, act)
            want = set(L64.EPILOGUE_FAULTS) - ({'activation_skipped'} if act == 'none' else set())
            assert set(faults) == want, (act, sorted(faults))
            for fault, y_bad in faults.items():
                assert int((y_bad != y64.to(torch.complex64)).sum()) == 16, (act, fault)
                f, missed = _compare(y_bad, y64, y32)
                assert missed and f['err'] > 10 * f['limit'], (act, fault, f)
            if act != 'none':
                hi, lo = L64.live_branches(y64, act)
                assert hi > LIVE and lo > LIVE, (act, hi, lo)
    finally:
        torch.set_num_threads(threads)


@pytest.mark.parametrize('name', list(P.ROWS))
def test_oracle_modules_equal_the_closed_form_coefficients(name):
    """folded_reference (conv_module -> ComplexBatchNorm2d.eval() -> activation) equals eval_coef_reference applied to the raw
    oracle conv output: to 1e-12 in fp64, and in fp32 to 32 roundings of the tensor's max-abs (about ten roundings on the
    way, of terms up to ~3 x the output: the centred input times the whitening matrix, times the weight)."""
    threads = L64.set_threads()
    try:
        row = P.ROWS[name]
        refs, pre64, pre32, case, state = _refs(name, B=1)
        for act in row.acts:
            y64, y32 = refs[act]
            assert L64.rel_max(L64.apply_coef(pre64, L64.eval_coef_reference(state, P.EPS, True), act), y64) <= 1e-12
            assert L64.rel_max(L64.apply_coef(pre32, L64.eval_coef_reference(state, P.EPS, False), act), y32) <= 32 * L64.EPS32
    finally:
        torch.set_num_threads(threads)


# ------------------------------------------------------------------------------------------------ GPU

gpu = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from dcsnet import _lib
    _lib.load()
    threads = L64.set_threads()
    yield torch.device('cuda:0')
    torch.set_num_threads(threads)


class _mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from dcsnet import ops
        self.default = ops.conv_precision()
        ops.set_conv_precision(self.mode)

    def __exit__(self, *a):
        from dcsnet import ops
        ops.set_conv_precision(self.default)


def _cbn_args(state, dev):
    return tuple(state[n].to(dev).contiguous() for n in ('weight', 'bias', 'running_mean', 'running_covar'))


def _two_kernel_form(row, operands, state, act, dev):
    """conv without activation, then ops.cbn in eval mode (cbn_finalize + cbn_apply_kernel): (y, coef [C,6] of that call).
    cbn_apply_kernel spreads C / 2 channel pairs over 256 threads, so it has no form for 24 or 6 channels: there the raw conv
    output is padded with zero channels to the next power of two (the map is per channel: the first C channels see the same
    arithmetic) and the result cut back."""
    from dcsnet import ops
    raw = P.launch(row, operands, 'none', None)
    C = raw.shape[3]
    Cp = C if C == 1 else max(2, 1 << (C - 1).bit_length())
    if Cp != C:
        pad = L64.eval_cbn_state(Cp, 1)
        state = {k: torch.cat((v, pad[k][C:])) for k, v in state.items()}
        raw = torch.cat((raw, torch.zeros(*raw.shape[:3], Cp - C, 2, device=dev)), dim=3).contiguous()
    y, _, coef = ops.cbn(raw, *_cbn_args(state, dev), P.EPS, -1.0, False, P.act_code(act))
    return y[:, :, :, :C].contiguous(), coef[:C].contiguous()


_PLAN_RE = re.compile(r'ncls (\d+) \| cand (\d+) tile (\d+)x(\d+) CH (\d+) S (\d+)/(\d+) cps (\d+) prec (\d+) coef (\d+)')


@pytest.fixture(scope='module')
def plans(dev):
    """One child process under DCS_MFMA_TRACE=1 launching every row once: (exit status, {row: [plan of each [mfma] line]},
    end of its stderr).  Run once; a failing child is reported by test_plan_probe and never started again."""
    env = dict(os.environ, DCS_MFMA_TRACE='1')
    for k in ('DCS_CONV_RING', 'DCS_RING_MIN_WG', 'DCS_CONV_PRECISION'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_plan_probe.py')], env=env, capture_output=True, text=True,
                       timeout=300)
    if r.returncode < 0:                                       # killed by a signal: a GPU fault or an abort — nothing more runs on this GPU
        pytest.exit(f'the plan probe died with signal {-r.returncode}:\n{r.stderr[-3000:]}', returncode=1)
    seen, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith('ROW '):
            cur = line[4:].strip()
            seen.setdefault(cur, [])
        elif line.startswith('[mfma]') and cur is not None:
            m = _PLAN_RE.search(line)
            assert m, line
            ncls, cand, th, tw, ch, s_used, s_plan, cps, prec, coef = (int(v) for v in m.groups())
            seen[cur].append(dict(ncls=ncls, cand=cand, tile=[th, tw], CH=ch, S=s_used, S_planned=s_plan, prec=prec, coef=coef))
    return r.returncode, seen, r.stderr[-3000:] + r.stdout[-500:]


@gpu
def test_plan_probe_every_row_takes_the_path_it_is_in_the_table_for(plans):
    code, seen, tail = plans
    assert code == 0, tail
    reached = set()
    for name, row in P.ALL.items():
        got = seen.get(name)
        assert got is not None, f'{name}: not launched'
        _record(('plans', name), got)
        if row.path in ('P6', 'P7') and not row.cands:
            assert got == [], (name, got)                      # conv_enc0.hip / conv_direct.hip: not an MFMA-plan launch
        else:
            assert len(got) == 1, (name, got)
            g = got[0]
            assert g['coef'] == 1 and g['cand'] in row.cands and (g['S'] > 1) == row.sliced and g['ncls'] == row.ncls, (name, row, g)
            if row.path == 'P5':
                assert row.L.Cout == 8 and g['cand'] == 3      # N = 16, cand 3: the 16-column kernel's dispatch condition
        if name in P.ROWS:
            reached.add(row.path)
    assert reached == set(P.PATHS), reached
    cands = {g['cand'] for name in P.ROWS for g in seen[name]}
    assert {4, 5, 7, 10} <= cands and cands & {6, 8}, cands      # P3's tiles and the ring


TIER_A = [(n, a, m) for n, r in P.ROWS.items() for a in r.acts for m in MODES]


@gpu
@pytest.mark.parametrize('name,act,mode', TIER_A, ids=[f'{n}-{a}-{m}' for n, a, m in TIER_A])
def test_folded_epilogue_against_fp64(dev, plans, name, act, mode):
    """Tier A (+ tier C's equality on the same launch): ops.cconv2d(..., act, coef=closed-form coefficients in fp32) against
    the oracle modules in fp64, every element; then, with the coefficient kernel's own output, folded == two-kernel form."""
    row = P.ROWS[name]
    rounded = mode == 'bf16'
    refs, _, _, case, state = _refs(name, rounded=rounded)
    y64, y32 = refs[act]
    if act != 'none':
        hi, lo = L64.live_branches(y64, act)
        assert hi > LIVE and lo > LIVE, (hi, lo)
    from dcsnet import ops
    with _mode(mode):
        operands = P.device_operands(row, case, dev)
        coef = L64.eval_coef_reference(state, P.EPS, wide=False).to(dev)
        y = P.launch(row, operands, act, coef)
        equal = None
        if act != 'sigmoid':                                   # (ops.cbn has no sigmoid: the network never asks for one)
            two, coef_dev = _two_kernel_form(row, operands, state, act, dev)
            equal = bool(torch.equal(P.launch(row, operands, act, coef_dev), two))
        torch.cuda.synchronize()
    got = ops.from_nhwc(y).cpu()
    fig, missed = _compare(got, y64, y32)
    plan = plans[1].get(name) if mode == 'bf16x6' else None      # the probe runs the default mode
    fig.update(path=row.path, folded_equals_two_kernel_form=equal, plan_default_mode=plan)
    print(f'{name} {act} {mode}: err {fig["err"]:.3e} cpu32 {fig["cpu32"]:.3e} limit {fig["limit"]:.3e}{" (fallback)" if fig["fallback"] else ""} '
          f'folded == two-kernel: {equal}')
    _record(('tier_a', name, act, mode), fig)
    assert not missed, fig
    assert equal is not False, 'the folded epilogue differs from conv + cbn_apply_kernel'


TIER_B = ['p1_16to16_k5s22', 'p2_up22_8p16to24_w40', 'p2_up22_16p16to16', 'p3_cand4_64to128', 'p3_cand7_classes_32p32to32',
          'p3_enc1_rows_8to16_k7', 'p4_plain_128to128', 'p4_classes_dec0', 'p5_dec5_ragged', 'p5_cin8_one_class_k5s22',
          'p6_enc0_ragged']


@gpu
@pytest.mark.parametrize('name', TIER_B)
def test_bf16_storage_entry_point_equals_the_fp32_one_rounded_once(dev, name):
    """Tier B: the _h build of the row's kernel with coef + activation, on bf16-representable operands in mode 'bf16'."""
    from test_hip_bf16 import _same_after_rounding
    row = P.ROWS[name]
    case, state = P.row_case(name, rounded=True)
    coef = L64.eval_coef_reference(state, P.EPS, wide=False)
    with _mode('bf16'):
        f32 = P.device_operands(row, case, dev)
        h = P.device_operands(row, case, dev, torch.bfloat16)
        assert torch.equal(h[0].float(), f32[0])               # bf16-representable: the two entry points read the same values
        for act in row.acts:
            y_f = P.launch(row, f32, act, coef.to(dev))
            y_h = P.launch(row, h, act, coef.to(dev))
            torch.cuda.synchronize()
            assert y_f.dtype == torch.float32
            _same_after_rounding(y_h, y_f, f'{name} {act}')
    _record(('tier_b', name), 'equal')


# (the ring kernel of the fp32 build runs the emulation only: no 'bf16' case for it)
TIER_C = [(n, m) for n, r in P.CHIP.items() for m in ('bf16x6', 'bf16') if not (r.ring and m == 'bf16')]


@gpu
@pytest.mark.parametrize('name,mode', TIER_C, ids=[f'{n}-{m}' for n, m in TIER_C])
def test_folded_equals_two_kernel_form_with_the_chip_filled(dev, name, mode):
    """Tier C: three folded launches, bit-identical with each other and with conv + ops.cbn, every element."""
    row = P.CHIP[name]
    case, state = P.row_case(name, rounded=(mode == 'bf16'))
    act = row.acts[0]
    with _mode(mode):
        operands = P.device_operands(row, case, dev)
        two, coef = _two_kernel_form(row, operands, state, act, dev)
        runs = [P.launch(row, operands, act, coef) for _ in range(3)]
        torch.cuda.synchronize()
    differ = [int((r != two).sum()) for r in runs]
    _record(('tier_c', name, mode), dict(outputs=two.numel(), differing_from_two_kernel_form=differ,
                                         runs_identical=all(torch.equal(r, runs[0]) for r in runs)))
    assert all(torch.equal(r, runs[0]) for r in runs), 'run-to-run differences'
    assert differ == [0, 0, 0], differ


@gpu
@pytest.mark.parametrize('C,hard', [(C, False) for C in D_CHANNELS] + [(64, True)])
def test_coefficient_kernel_against_the_closed_form(dev, C, hard):
    """Tier D: the coef [C,6] output of ops.cbn(..., use_batch_stats=False) against eval_coef_reference in fp64."""
    from dcsnet import ops
    state = _d_state(C, hard)
    x = torch.zeros(1, 2, 2, C, 2, device=dev)
    _, _, coef = ops.cbn(x, *_cbn_args(state, dev), P.EPS, -1.0, False, ops.ACT_NONE)
    ref, ref32 = (L64.eval_coef_reference(state, P.EPS, w) for w in (True, False))
    fig, missed = _compare(coef.cpu(), ref, ref32)
    print(f'coef C {C} hard {hard}: err {fig["err"]:.3e} cpu32 {fig["cpu32"]:.3e} limit {fig["limit"]:.3e}{" (fallback)" if fig["fallback"] else ""}')
    _record(('tier_d', 'coef', f'C{C}{"_hard" if hard else ""}'), fig)
    assert not missed, fig


@gpu
def test_network_stages_pass_their_cached_coefficients_to_the_folded_kernel(dev):
    """Tier D: one encoder and one decoder stage of a C_NETWORK at [2,256,32] carrying correlated CBN states, driven as
    C_NETWORK.forward drives them at inference: F.cconv2d_cbn_eval(..., bn.eval_coef(), act)."""
    from dcsnet import functional as F, ops
    from dcsnet.config import config, hparams
    from dcsnet.c_network import C_NETWORK
    from oracle.seeded_state import fill_state, seeded_input
    net = fill_state(C_NETWORK(config, dict(hparams), 0), 4)
    stages = {'enc2': (net.encoder[2][0], net.encoder[2][1], L64.eval_cbn_state(32, 51)),
              'dec4': (net.decoder[4][0], net.decoder[4][1], L64.eval_cbn_state(16, 52))}
    for conv, bn, st in stages.values():
        sd = bn.state_dict()
        sd.update(weight=st['weight'], bias=st['bias'], running_mean=torch.view_as_complex(st['running_mean'].contiguous()),
                  running_covar=st['running_covar'])
        bn.load_state_dict(sd)
    F.note_state_update()
    net = net.to(dev).eval()
    with torch.no_grad():
        for _, bn, _ in stages.values():
            assert bn.eval_coef() is None                      # nothing cached before the first eval pass
        net(seeded_input(2, 256, 32, seed=4).to(dev))
        for tag, (conv, bn, st) in stages.items():
            coef = bn.eval_coef()
            assert torch.is_tensor(coef) and tuple(coef.shape) == (st['weight'].shape[0], 6)
            tr = tag.startswith('dec')
            a, b = (conv.conv_tran_r, conv.conv_tran_i) if tr else (conv.conv_r, conv.conv_i)
            k = conv.kernel_size[0]
            up = tuple(config.upsample_scale_factor[4]) if tr else (1, 1)
            cin = a.weight.shape[0] if tr else a.weight.shape[1]
            cout = a.weight.shape[1] if tr else a.weight.shape[0]
            c1 = cin // 2 if tr else cin
            L = L64.ConvLayer(tag, 10, 12, c1, cin - c1, cout, k, (1, 1) if tr else tuple(conv.stride), up, tr)
            case = L64.conv_case(L, 2, 60 + len(tag))
            case.update(w_r=a.weight.detach().cpu(), w_i=b.weight.detach().cpu(), b_r=a.bias.detach().cpu(), b_i=b.bias.detach().cpu())
            act = 'lrelu' if tr else 'relu'
            y64, y32 = (L64.folded_reference(L, case, st, act, w, bn.eps)['y'] for w in (True, False))
            x = ops.to_nhwc(case['x'].to(dev))
            x1, x2 = x[:, :, :, :c1].contiguous(), (x[:, :, :, c1:].contiguous() if tr else None)
            y = F.cconv2d_cbn_eval(x1, x2, a.weight, b.weight, a.bias, b.bias, tr, conv.kernel_size, (1, 1) if tr else conv.stride,
                                   conv.corr_padding if tr else conv.padding, up, coef, P.act_code(act))
            fig, missed = _compare(ops.from_nhwc(y).cpu(), y64, y32)
            hi, lo = L64.live_branches(y64, act)
            assert hi > LIVE and lo > LIVE, (tag, hi, lo)
            print(f'{tag}: err {fig["err"]:.3e} cpu32 {fig["cpu32"]:.3e} limit {fig["limit"]:.3e}')
            _record(('tier_d', 'wiring', tag), fig)
            assert not missed, (tag, fig)
