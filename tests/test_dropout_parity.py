"""Dropout ON, against fp64: the oracle drops exactly what the device dropped.

The fused dropout sites draw no random numbers: an element is kept or dropped by a hash of (seed + ops.SEED_STATE, flat
index of the real element in the channels-last tensor) — csrc/dcs_common.h.  oracle/dropout_mask.py restates that hash on
the host (pinned to published splitmix64 vectors in tests/test_dropout_cpu.py), so every kernel that drops can be compared
with a plain fp64 evaluation that multiplies by the same mask:

  ops.dropout                  bit for bit (one fp32 multiply), sizes around its grid-stride loop's first wrap
  F.cbn, C = 1                 the two-pixels-per-float4 layout with its odd tail pixel, forward and backward
  F.cbn_two, F.cbn_attention   the DROP instantiations of cbn_apply_kernel and attention_apply_kernel and the mask
  F.attention_block            regenerations of cbn_bwd.hip / attention_bwd.hip, on reduced maps of the step's layers, with
                               the comparator of tests/test_layers_train_size.py (_check_block_with_ties)
  wrap cases                   the smallest maps at which the forward kernels' grids reach their caps and every workgroup loops
  C_NETWORK                    output, loss and every gradient of one training forward / backward with the reference's
                               dropout_conv = 0.1, dropout_fc = 0.2, and four optimisation steps of TrainStep, eager and as a
                               replayed graph, against the fp64 oracle replaying each step's masks (ReplayDropout)

Every test runs under a non-zero ops.SEED_STATE: a kernel that loses the device-side offset draws another mask.

Whole-network bounds: those of the dropout-off twins (tests/test_hip_backward.py, tests/test_hip_train.py) — per tensor
max-abs error <= 2e-3 of the tensor's max-abs + 1e-6, norms 2e-3, loss 1e-4, loss trajectory 2e-3 |loss| + 1e-3.  The fp32
CPU oracle runs with the same masks against the fp64 one; where IT misses a bound, the bound of that tensor becomes
layer_fp64.K_BOUND times its error (recorded as such).  No bound is computed from the HIP result.  Figures go to
dropout_parity.json in $DCS_PARITY_DIR (default parity_out/); a full run's file is profiles/dropout_parity.json.

Not pinned here: DR-Net's dropout is ATen's (no replayable mask); bf16 activation storage with dropout is compared with the
fp32 kernels only (tests/test_hip_bf16.py).
"""
import functools
import os
import re
import time
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from oracle import dropout_mask as DM
from oracle import layer_fp64 as L64
from oracle.cnet_oracle import C_NETWORK_Oracle, replay_dropout
from oracle.nf_oracle import dcs_train_losses
from oracle.seeded_state import fill_state, seeded_input

from _ragged_helpers import record
from test_dropout_cpu import miss, REL, ABS
from test_layers_train_size import (BY_NAME, _bn_params, _check_block_with_ties, _cplx, _forward, _offset_input, _operands, _seed,
                                    _sqrt2_covar)

pytestmark = pytest.mark.gpu

STATE = 5                                   # ops.SEED_STATE of the kernel tests
SEEDS = (1234, 2 ** 63 - 1)
K = L64.K_BOUND
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'dcs-net_amd', 'csrc')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from dcsnet import _lib
    _lib.load()
    threads = L64.set_threads()
    yield torch.device('cuda:0')
    torch.set_num_threads(threads)


@contextmanager
def seed_state(dev, value):
    """ops.SEED_STATE = a one-element int64 tensor holding `value` for the block; the previous one comes back afterwards."""
    from dcsnet import ops
    old = ops.SEED_STATE
    ops.SEED_STATE = torch.tensor([value], dtype=torch.int64, device=dev)
    try:
        yield ops.SEED_STATE
    finally:
        ops.SEED_STATE = old


_record = functools.partial(record, 'dropout_parity.json')     # figures -> $DCS_PARITY_DIR/dropout_parity.json (default parity_out/)


def _define(source, name):
    """The default of `#define NAME value` in a kernel source."""
    m = re.search(r'#define\s+' + name + r'\s+(\d+)', open(os.path.join(CSRC, source)).read())
    assert m, (source, name)
    return int(m.group(1))


def _keep32_nhwc(seed, shape, p, state=STATE):
    """The float32 mask of a channels-last float tensor [..., 2] as the kernels form it."""
    n = int(np.prod(shape))
    return DM.keep_scale(seed, n, p, state, wide=False).view(*shape)


# ------------------------------------------------------------------------------------------------ ops.dropout

def test_dropout_kernel_is_the_host_mask(dev):
    """dcs_dropout_fwd: y = x * keep, one fp32 multiply — bit for bit.  Its launch (attention.hip) has ceil(n / (4 * 256))
    workgroups of 256 threads, so the grid-stride loop first wraps at n = 257."""
    from dcsnet import ops
    src = open(os.path.join(CSRC, 'attention.hip')).read()
    assert 'long nb = (n + kThreads * 4 - 1) / (kThreads * 4);' in src and 'constexpr int kThreads = 256;' in src
    first_wrap = 256 + 1
    g = torch.Generator().manual_seed(3)
    with seed_state(dev, STATE):
        for n in (1, 3, 255, first_wrap, 1027):
            x = torch.randn(n, generator=g)
            for p in (0.1, 0.5):
                for seed in SEEDS:
                    y = ops.dropout(x.to(dev), p, seed).cpu()
                    want = x * DM.keep_scale(seed, n, p, STATE, wide=False)
                    assert torch.equal(y, want), (n, p, seed, int((y != want).sum()))
        # the state is part of the mask ...
        assert not torch.equal(DM.keep_scale(1234, 1027, 0.1, STATE), DM.keep_scale(1234, 1027, 0.1, 0))
    # ... and without a state tensor the by-value seed alone decides
    old = ops.SEED_STATE
    ops.SEED_STATE = None
    try:
        x = torch.randn(1027, generator=g)
        assert torch.equal(ops.dropout(x.to(dev), 0.1, 1234).cpu(), x * DM.keep_scale(1234, 1027, 0.1, 0, wide=False))
    finally:
        ops.SEED_STATE = old


# ------------------------------------------------------------------------------------------------ CBN, one channel

C1_SEEDS = (11, 12, 13, 14)
C1_P = 0.3


def _report(tag, rows):
    for k_, v in rows.items():
        print(f'{tag} {k_}: {v}')


@pytest.mark.parametrize('act', ['none', 'relu'])
@pytest.mark.parametrize('shape', [(3, 1, 5), (2, 2, 4)], ids=['P15', 'P16'])
def test_cbn_single_channel(dev, shape, act):
    """F.cbn at C = 1: two pixels per float4, and for odd P the last pixel through the scalar tail of cbn_apply_kernel and of
    both cbn_bwd kernels (its mask index is 2 (P - 1), not a float4's)."""
    from dcsnet import ops, functional as F
    B, H, W = shape
    P = B * H * W
    # over the seeds the tail pixel's real part is dropped at least once and kept at least once
    tail = [float(DM.keep_scale(s, 2 * P, C1_P, STATE)[2 * (P - 1)]) for s in C1_SEEDS]
    assert min(tail) == 0.0 and max(tail) > 1.0, tail
    misses = []
    for seed in C1_SEEDS:
        x, g = _offset_input(1, B, H, W, 40 + P)
        g = g.to(torch.complex64)
        bn = _bn_params(1, 3)
        xd = ops.to_nhwc(x.to(dev)).requires_grad_(True)
        w, b = (t.to(dev).requires_grad_(True) for t in bn)
        rm, rc = torch.zeros(1, 2, device=dev), _sqrt2_covar(1, dev)
        with seed_state(dev, STATE):
            y = F.cbn(xd, w, b, rm, rc, 1e-5, 0.1, True, F.ACT_RELU if act == 'relu' else F.ACT_NONE, C1_P, seed)
            grads = torch.autograd.grad(y, [xd, w, b], ops.to_nhwc(g.to(dev)))
            y0 = ops.cbn(xd.detach(), w.detach(), b.detach(), torch.zeros_like(rm), _sqrt2_covar(1, dev), 1e-5, 0.1, True,
                         F.ACT_RELU if act == 'relu' else F.ACT_NONE)[0]
        assert torch.equal(y.detach().cpu(), y0.cpu() * _keep32_nhwc(seed, y0.shape, C1_P)), seed
        got = dict(y=_cplx(y), gx=_cplx(grads[0]), running_mean=torch.view_as_complex(rm.cpu()), running_covar=rc.cpu(),
                   g_weight=grads[1].cpu(), g_bias=grads[2].cpu())
        decided = got['y'] if act != 'none' else None

        def make_refs(choice, seed=seed, x=x, g=g, bn=bn, decided=decided):
            return tuple(L64.block_reference(x, g, wide, bn, act, decided=decided, keep=DM.keep_nchw(seed, (B, 1, H, W), C1_P, STATE, wide))
                         for wide in (True, False))

        rows, m = _check_block_with_ties(got, make_refs)
        _report(f'cbn C=1 P={P} {act} seed {seed}', rows)
        _record(('cbn_c1', f'P{P}_{act}', f'seed{seed}'), rows)
        misses += [(seed,) + t for t in m]
    assert not misses, misses


# ------------------------------------------------------------------------------------------------ the step's CBN nodes, reduced maps

MAPS = [(6, 10), (5, 7)]                    # B = 3: P = 180, and P = 105 — no multiple of rows_per_iter = 256 / (C / 2) for C = 8, 64, 128
B_SMALL = 3
P_CONV = 0.1


def _reduced_layer(name, Ho, Wo):
    """The conv layer `name` of the step with its source map shrunk so that its output — the CBN's input — is Ho x Wo.  A
    decoder layer whose upsampling cannot produce an odd extent runs without upsampling: the conv is only the producer of
    the CBN's input and statistics rows here."""
    L = BY_NAME[name]
    if not L.transposed:
        L = L._replace(H=Ho * L.stride[0], W=Wo * L.stride[1])
    elif Ho % L.up[0] == 0 and Wo % L.up[1] == 0:
        L = L._replace(H=Ho // L.up[0], W=Wo // L.up[1])
    else:
        L = L._replace(H=Ho, W=Wo, up=(1, 1))
    assert L64.out_hw(L) == (Ho, Wo), (L, L64.out_hw(L))
    return L


def _conv_output(L, dev, seed):
    case = L64.conv_case(L, B_SMALL, seed, offset=(1.0 - 0.7j), spread=0.08)
    x1, x2, _, p = _operands(L, case, dev)
    with torch.no_grad():
        y, stat = _forward(L, x1, x2, p)
    return y, stat


def _same_pattern(y, y0, keep32):
    """The dropped output is the undropped output of the same kernel times the host mask, element by element (one fp32
    multiply): in particular its zeros are the mask's zeros and the zeros the undropped output already has."""
    y, y0 = y.detach().cpu(), y0.detach().cpu()
    assert torch.equal(y == 0, (keep32 == 0) | (y0 == 0)), int(((y == 0) != ((keep32 == 0) | (y0 == 0))).sum())
    assert torch.equal(y, y0 * keep32), int((y != y0 * keep32).sum())
    assert 0.05 < float((keep32 == 0).float().mean()) < 0.16


@pytest.mark.parametrize('Ho,Wo', MAPS, ids=[f'{h}x{w}' for h, w in MAPS])
@pytest.mark.parametrize('name', ['enc0', 'enc3', 'enc6'])
@pytest.mark.parametrize('seed', SEEDS, ids=['seed1234', 'seed2p63m1'])
def test_cbn_two_with_dropout_against_fp64(dev, seed, name, Ho, Wo):
    """The encoder stages' node: CBN + ReLU + dropout with two consumers (cbn_apply_kernel<RELU, true>, the two cbn_bwd
    kernels' mask), C = 8, 64, 128, from the HIP conv's own output and statistics rows."""
    from dcsnet import ops, functional as F
    L = _reduced_layer(name, Ho, Wo)
    C, B = L.Cout, B_SMALL
    y, stat = _conv_output(L, dev, 300 + _seed(BY_NAME[name], B) + Ho)
    if name != 'enc0':                      # (the one-input-channel kernel has no statistics epilogue on maps this small)
        assert stat is not None, 'this geometry must take the statistics epilogue'
    xc = _cplx(y)
    g = torch.Generator().manual_seed(500 + C + Ho)
    bn = _bn_params(C, C + 1)
    w, b = (t.to(dev).requires_grad_(True) for t in bn)
    rm, rc = torch.zeros(C, 2, device=dev), _sqrt2_covar(C, dev)
    yl = y.detach().requires_grad_(True)
    ga, gb = L64.randc(g, B, C, Ho, Wo), L64.randc(g, B, C, Ho, Wo)
    with seed_state(dev, STATE):
        a, a2 = F.cbn_two(yl, w, b, rm, rc, 1e-5, 0.1, True, F.ACT_RELU, P_CONV, seed, stat)
        grads = torch.autograd.grad([a, a2], [yl, w, b], [ops.to_nhwc(ga.to(dev)), ops.to_nhwc(gb.to(dev))])
        a0 = F.cbn_two(y, w.detach(), b.detach(), torch.zeros_like(rm), _sqrt2_covar(C, dev), 1e-5, 0.1, True, F.ACT_RELU, 0.0, 0, stat)[0]
    assert a2.data_ptr() == a.data_ptr()
    _same_pattern(a, a0, _keep32_nhwc(seed, a.shape, P_CONV))
    got = dict(y=_cplx(a), gx=_cplx(grads[0]), running_mean=torch.view_as_complex(rm.cpu()), running_covar=rc.cpu(),
               g_weight=grads[1].cpu(), g_bias=grads[2].cpu())
    g_out = ga.to(torch.complex128) + gb.to(torch.complex128)
    seen = {}

    def make_refs(choice):
        refs = tuple(L64.block_reference(xc, g_out, wide, bn, 'relu', decided=got['y'], max_choice=choice,
                                         keep=DM.keep_nchw(seed, (B, C, Ho, Wo), P_CONV, STATE, wide)) for wide in (True, False))
        seen['undecided'] = refs[0]['undecided_activations']
        return refs

    rows, misses = _check_block_with_ties(got, make_refs)
    _report(f'cbn_two {name} {Ho}x{Wo} seed {seed}', rows)
    assert seen['undecided'] <= 8 + 2e-5 * 2 * xc.numel(), (seen['undecided'], xc.numel())
    _record(('cbn_two', name, f'{Ho}x{Wo}', f'seed{seed}'), dict(tensors=rows, undecided_activations=seen['undecided'],
                                                                   statistics_rows=stat is not None))
    assert not misses, misses


@pytest.mark.parametrize('Ho,Wo', MAPS, ids=[f'{h}x{w}' for h, w in MAPS])
@pytest.mark.parametrize('name', ['dec5', 'dec0'])
@pytest.mark.parametrize('seed', SEEDS, ids=['seed1234', 'seed2p63m1'])
def test_cbn_attention_with_dropout_against_fp64(dev, seed, name, Ho, Wo):
    """The decoder stages' node: CBN + leaky ReLU, channel and spatial attention, dropout AFTER the spatial-attention multiply
    (attention_apply_kernel<true>; the two mask regenerations of attention_bwd.hip), C = 8 and 128."""
    from dcsnet import ops, functional as F
    L = _reduced_layer(name, Ho, Wo)
    C, B = L.Cout, B_SMALL
    y, stat = _conv_output(L, dev, 300 + _seed(BY_NAME[name], B) + Ho)
    assert stat is not None and ops.FUSE_APPLY_POOL
    xc = _cplx(y)
    g = torch.Generator().manual_seed(500 + C + Ho)
    bn = _bn_params(C, C + 1)
    att = L64.attention_params(C, 900 + C)
    w, b = (t.to(dev).requires_grad_(True) for t in bn)
    ap = [t.to(dev).requires_grad_(True) for t in att]
    rm, rc = torch.zeros(C, 2, device=dev), _sqrt2_covar(C, dev)
    yl = y.detach().requires_grad_(True)
    ga = L64.randc(g, B, C, Ho, Wo)
    with seed_state(dev, STATE):
        a = F.cbn_attention(yl, w, b, rm, rc, 1e-5, 0.1, True, F.ACT_LRELU, *ap, 7, P_CONV, seed, stat)
        a_again = ops.cbn(y, w.detach(), b.detach(), torch.zeros_like(rm), _sqrt2_covar(C, dev), 1e-5, 0.1, True, F.ACT_LRELU, stat=stat)[0]
        same = [t for t in a.grad_fn.saved_tensors
                if t is not None and t.shape == a_again.shape
                and float((t.detach() - a_again).abs().max()) <= 1e-5 * float(a_again.abs().max())]
        assert len(same) == 1, len(same)
        decided = _cplx(same[0])                               # the node's saved activation: CBN + leaky ReLU, before the attention
        grads = torch.autograd.grad(a, [yl, w, b] + ap, ops.to_nhwc(ga.to(dev)))
        a0 = F.cbn_attention(y, w.detach(), b.detach(), torch.zeros_like(rm), _sqrt2_covar(C, dev), 1e-5, 0.1, True, F.ACT_LRELU,
                             *[t.detach() for t in ap], 7, 0.0, 0, stat)
    _same_pattern(a, a0, _keep32_nhwc(seed, a.shape, P_CONV))
    got = dict(y=_cplx(a), gx=_cplx(grads[0]), running_mean=torch.view_as_complex(rm.cpu()), running_covar=rc.cpu(),
               g_weight=grads[1].cpu(), g_bias=grads[2].cpu(), g_att=[t.cpu() for t in grads[3:]])
    seen = {}

    def make_refs(choice):
        refs = tuple(L64.block_reference(xc, ga, wide, bn, 'lrelu', att, decided=decided, max_choice=choice,
                                         keep=DM.keep_nchw(seed, (B, C, Ho, Wo), P_CONV, STATE, wide)) for wide in (True, False))
        seen['undecided'] = refs[0]['undecided_activations']
        return refs

    rows, misses = _check_block_with_ties(got, make_refs)
    _report(f'cbn_attention {name} {Ho}x{Wo} seed {seed}', rows)
    assert seen['undecided'] <= 8 + 2e-5 * 2 * xc.numel(), (seen['undecided'], xc.numel())
    _record(('cbn_attention', name, f'{Ho}x{Wo}', f'seed{seed}'), dict(tensors=rows, undecided_activations=seen['undecided']))
    assert not misses, misses


@pytest.mark.parametrize('Ho,Wo', MAPS, ids=[f'{h}x{w}' for h, w in MAPS])
@pytest.mark.parametrize('name', ['dec5', 'dec0'])
def test_attention_block_with_dropout_against_fp64(dev, name, Ho, Wo):
    """F.attention_block (the stand-alone node: channel attention, spatial attention, apply + dropout) at p = 0.1 on the two
    decoder geometries: forward, g_x and the six parameter gradients."""
    from dcsnet import ops, functional as F
    C, B, seed = BY_NAME[name].Cout, B_SMALL, SEEDS[1]
    g = torch.Generator().manual_seed(60 + C + Ho)
    x = L64.nf.complex_lrelu(L64.randc(g, B, C, Ho, Wo) * 0.7 + (0.2 + 0.1j)).to(torch.complex64)
    gg = L64.randc(g, B, C, Ho, Wo)
    att = L64.attention_params(C, 700 + C)
    xd = ops.to_nhwc(x.to(dev)).requires_grad_(True)
    ap = [t.to(dev).requires_grad_(True) for t in att]
    with seed_state(dev, STATE):
        out = F.attention_block(xd, *ap, 7, P_CONV, seed)
        grads = torch.autograd.grad(out, [xd] + ap, ops.to_nhwc(gg.to(dev)))
        out0 = F.attention_block(xd.detach(), *[t.detach() for t in ap], 7, 0.0, 0)
    _same_pattern(out, out0, _keep32_nhwc(seed, out.shape, P_CONV))
    got = dict(y=_cplx(out), gx=_cplx(grads[0]), g_att=[t.cpu() for t in grads[1:]])
    rows, misses = _check_block_with_ties(got, lambda choice: tuple(
        L64.block_reference(x, gg, wide, attention=att, max_choice=choice, keep=DM.keep_nchw(seed, (B, C, Ho, Wo), P_CONV, STATE, wide))
        for wide in (True, False)))
    _report(f'attention_block {name} {Ho}x{Wo}', rows)
    _record(('attention_block', name, f'{Ho}x{Wo}'), dict(tensors=rows))
    assert not misses, misses


# ------------------------------------------------------------------------------------------------ wrap cases

def test_cbn_apply_dropout_where_its_grid_is_capped(dev):
    """cbn_apply_kernel<., true>, C = 8: the launch has one workgroup per DCS_CBN_APP_IT passes of rows_per_iter pixels, at
    most 2048 — the smallest P beyond that makes every workgroup's loop run on past its planned passes.  Element-wise: the
    dropped output is the same kernel's undropped output times the float32 host mask."""
    from dcsnet import ops, functional as F
    src = open(os.path.join(CSRC, 'cbn.hip')).read()
    assert 'nb > 2048 ? 2048 : nb' in src and 'constexpr int kThreads = 256;' in src
    C = 8
    rows_per_iter = 256 // (C // 2)
    P = 2048 * _define('cbn_geom.h', 'DCS_CBN_APP_IT') * rows_per_iter + 1
    g = torch.Generator().manual_seed(8)
    x = (torch.randn(1, 1, P, C, 2, generator=g) * 0.5 + 0.3).to(dev)
    w, b = (t.to(dev) for t in _bn_params(C, 5))
    seed = SEEDS[1]
    keep = _keep32_nhwc(seed, x.shape, P_CONV)
    with seed_state(dev, STATE):
        for act in (F.ACT_RELU, F.ACT_LRELU):
            y0 = ops.cbn(x, w, b, torch.zeros(C, 2, device=dev), _sqrt2_covar(C, dev), 1e-5, 0.1, True, act)[0].cpu()
            y = ops.cbn(x, w, b, torch.zeros(C, 2, device=dev), _sqrt2_covar(C, dev), 1e-5, 0.1, True, act, P_CONV, seed)[0].cpu()
            assert torch.equal(y, y0 * keep), (act, int((y != y0 * keep).sum()))
            assert float((y0 != 0).float().mean()) > 0.2


@pytest.mark.parametrize('form', ['small_map', 'capped_grid'])
def test_attention_apply_dropout_where_its_loop_wraps(dev, form):
    """attention_apply_kernel<true>, C = 8 (64 pixels per workgroup pass).  small_map: B = 3 and HW two pixels beyond DCS_ATT_APP_IT + 1
    passes — the launch plans DCS_ATT_APP_IT passes per workgroup, two workgroups per sample, and the first comes round again.  capped_grid: B = 1 and the
    smallest HW beyond 2048 workgroups of four passes."""
    from dcsnet import ops
    src = open(os.path.join(CSRC, 'attention.hip')).read()
    assert '(it + 3) / 4' in src and ': 2048) / (B > 0 ? B : 1)' in src
    C, rpi = 8, 256 // 4
    app_it, small_it = _define('attention.hip', 'DCS_ATT_APP_IT'), _define('cbn_geom.h', 'DCS_ATT_SMALL_IT')
    if form == 'small_map':
        B, HW = 3, (app_it + 1) * rpi + 2
        it = -(-HW // rpi)
        assert it <= small_it and -(-it // app_it) * rpi < HW
    else:
        B, HW = 1, 2048 * 4 * rpi + 1
        assert -(-HW // rpi) > small_it
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, 1, HW, C, 2, generator=g).to(dev)
    ca = (torch.rand(B, C, 2, generator=g) * 0.8 + 0.1).to(dev)
    sa = (torch.rand(B, 1, HW, 1, 2, generator=g) * 0.8 + 0.1).to(dev)
    seed = SEEDS[1]
    with seed_state(dev, STATE):
        y0 = ops.attention_apply(x, ca, sa).cpu()
        y = ops.attention_apply(x, ca, sa, P_CONV, seed).cpu()
    keep = _keep32_nhwc(seed, x.shape, P_CONV)
    assert torch.equal(y, y0 * keep), int((y != y0 * keep).sum())


# ------------------------------------------------------------------------------------------------ the whole network

def _net(dev, seed):
    """C_NETWORK with the reference hparams unchanged (dropout_conv 0.1, dropout_fc 0.2), seeded state, training mode."""
    from dcsnet.config import config, hparams
    from dcsnet.c_network import C_NETWORK
    hp = dict(hparams)
    assert hp['dropout_conv'] == 0.1 and hp['dropout_fc'] == 0.2
    return fill_state(C_NETWORK(config, hp, 0), seed).to(dev).train(), hp


def _spy_on_drop(net):
    """Wrap the instance's _drop: every (p, seed) it hands to a site with p > 0, in call order."""
    seen = []
    inner = net._drop

    def _drop(p):
        out = inner(p)
        if out[0] > 0:
            seen.append(out)
        return out

    net._drop = _drop
    return seen


_SITE_SHAPES = {}


def _site_shapes(B, Fb, T):
    """Complex shapes of the oracle's 14 dropout_conv sites and its dropout_fc site for an input [B, Fb, T]."""
    if (B, Fb, T) not in _SITE_SHAPES:
        ref = C_NETWORK_Oracle().eval()
        shapes = {'conv': [], 'fc': []}
        hooks = [ref.dropout_conv.register_forward_hook(lambda m, a, o: shapes['conv'].append(tuple(a[0].shape[:-1]))),
                 ref.dropout_fc.register_forward_hook(lambda m, a, o: shapes['fc'].append(tuple(a[0].shape[:-1])))]
        with torch.no_grad(), L64.cdtype(torch.complex64):       # (a caller may have widened the oracle's casts)
            ref(seeded_input(B, Fb, T))
        for h in hooks:
            h.remove()
        assert len(shapes['conv']) == 14 and len(shapes['fc']) == 1
        _SITE_SHAPES[(B, Fb, T)] = shapes
    return _SITE_SHAPES[(B, Fb, T)]


def _check_sites(pairs):
    assert len(pairs) == 15, len(pairs)
    assert [p for p, _ in pairs] == [0.1] * 7 + [0.2] + [0.1] * 7
    assert len({s for _, s in pairs}) == 15


def _replay(ref, pairs, state, shape, wide):
    """ReplayDropout modules in `ref` holding the host masks of the device's 15 sites: (p, seed + state) in call order —
    7 encoder sites, the latent fc site, 7 decoder sites."""
    _check_sites(pairs)
    shapes = _site_shapes(*shape)
    conv = [DM.keep_like(s, sh, p, state, wide) for (p, s), sh in zip(pairs[:7] + pairs[8:], shapes['conv'])]
    fc = [DM.keep_like(pairs[7][1], shapes['fc'][0], pairs[7][0], state, wide)]
    replay_dropout(ref, conv, fc)


def _bias_before_bn(n):
    return n.endswith('.bias') and (('.0.conv_r' in n or '.0.conv_i' in n) and n.startswith('encoder')
                                    or ('.0.conv_tran_' in n and n.startswith('decoder')))


def _quadratic(out, w):
    return (w * (out.real ** 2 + 0.5 * out.imag ** 2 + 0.25 * out.real * out.imag)).sum()


def test_one_forward_has_fifteen_sites(dev):
    net, _ = _net(dev, 0)
    seen = _spy_on_drop(net)
    with seed_state(dev, STATE), torch.no_grad():
        net(seeded_input(2, 256, 32, seed=7).to(dev))
    _check_sites(seen)
    net.eval()
    with torch.no_grad():
        net(seeded_input(2, 256, 32, seed=7).to(dev))
    assert len(seen) == 15                     # no site in eval


def _held(name, e_hip, e_cpu32, bound, what, misses, path):
    """One figure against its bound; where the fp32 CPU oracle itself misses the bound, K times ITS error."""
    row = dict(e_hip=e_hip, e_cpu32=e_cpu32, bound=bound, bound_is=what)
    if e_cpu32 > bound:
        row.update(bound=K * e_cpu32, bound_is=f'{K:g} x the fp32 CPU oracle\'s error (it misses {what}: {bound:.3e})')
    _record(path + (name,), row)
    if not e_hip <= row['bound']:
        misses.append((name, row))
    return row


def test_network_forward_and_gradients_with_dropout(dev, golden_dir):
    """net(x) with bound=True, the quadratic functional of tests/test_hip_backward.py's whole-network test, backward — all with
    the reference's dropout — against the fp64 oracle dropping the same elements at all 15 sites."""
    t0 = time.time()
    cnv = np.load(os.path.join(golden_dir, 'cnet_vectors.npz'))
    x, w = torch.from_numpy(cnv['b2t32_x']), torch.from_numpy(cnv['b2t32_loss_w'])
    net, _ = _net(dev, 0)
    seen = _spy_on_drop(net)
    state = 0x1234567
    with seed_state(dev, state):
        out = net(x.to(dev))
        loss = _quadratic(out, w.to(dev))
        loss.backward()
    _check_sites(seen)
    refs = {}
    for wide in (True, False):
        cd = torch.complex128 if wide else torch.complex64
        with L64.cdtype(cd):
            ref = fill_state(C_NETWORK_Oracle(), 0).train()
            ref = ref.double() if wide else ref
            _replay(ref, seen, state, tuple(x.shape), wide)
            o = ref(x.to(cd))
            l = _quadratic(o, w.to(torch.float64 if wide else torch.float32))
            l.backward()
        refs[wide] = (o.detach(), float(l.detach()), {n: q.grad for n, q in ref.named_parameters()})
    o64, l64, g64 = refs[True]
    o32, l32, g32 = refs[False]
    misses, path = [], ('network', 'forward_backward')
    e, b = miss(out.cpu(), o64)
    _held('output', e, miss(o32, o64)[0], b, f'{REL:g} of max-abs + {ABS:g}', misses, path)
    _held('loss', abs(float(loss.detach()) - l64), abs(l32 - l64), 1e-4 * abs(l64), '1e-4 of |loss|', misses, path)
    pd = dict(net.named_parameters())
    assert sorted(pd) == sorted(g64)
    compared = 0
    for n, want in g64.items():
        g = pd[n].grad
        if want is None:                               # decoder_attention.12 / .13 are never run
            assert g is None and n.startswith(('decoder_attention.12.', 'decoder_attention.13.')), n
            continue
        if _bias_before_bn(n):                         # analytically zero: both sides are rounding noise
            assert float(g.norm()) < 2e-3, n
            continue
        g = g.detach().cpu()
        e, b = miss(g, want)
        _held(n, e, miss(g32[n], want)[0], b, f'{REL:g} of max-abs + {ABS:g}', misses, path + ('gradients',))
        nw = float(want.norm())
        _held(n, abs(float(g.double().norm()) - nw), abs(float(g32[n].double().norm()) - nw), 2e-3 * nw + 1e-6, '2e-3 of the norm + 1e-6',
              misses, path + ('gradient_norms',))
        compared += 1
    assert compared == 198 - sum(_bias_before_bn(n) for n in g64), compared
    _record(path + ('seconds',), time.time() - t0)
    assert not misses, misses


@pytest.mark.parametrize('stepper', ['eager', 'graph'])
def test_train_steps_with_dropout_track_the_oracle(dev, stepper):
    """Four optimisation steps with the reference's dropout, TrainStep eager and as a captured graph (one eager warm-up step,
    capture at the second call, replays after).  The eager stepper draws new by-value seeds every step; a replayed graph keeps
    the seeds it was captured with and only ops.SEED_STATE moves — either way the fp64 oracle (Adam with amsgrad, clip 100)
    replays exactly the masks of each step, and every step's loss follows it."""
    from dcsnet import ops
    from dcsnet.dp import TrainStep
    t0 = time.time()
    clean, noise = seeded_input(2, 256, 32, 1, 0.1), seeded_input(2, 256, 32, 2, 0.05)
    noisy = clean + noise
    batch = (noise.to(dev), noisy.to(dev), clean.to(dev), [0, 1])
    previous = ops.SEED_STATE
    try:
        net, hp = _net(dev, 2)
        seen = _spy_on_drop(net)
        ts = TrainStep(net, use_graph=True, graph_warmup=1) if stepper == 'graph' else TrainStep(net)
        assert ops.SEED_STATE is ts.seed_state
        ts.seed_state.fill_(1000)
        got, steps, pairs = [], [], None
        for k in range(4):
            state, n0 = int(ts.seed_state), len(seen)
            got.append(float(ts((batch))))
            new = seen[n0:]
            if stepper == 'graph' and k >= 2:
                assert not new, 'a replayed graph runs no Python'       # the by-value seeds of the capture, another state
            else:
                pairs = list(new)
            steps.append((state, pairs))
        if stepper == 'graph':
            assert ts._graph is not None, 'capture did not happen (fell back to eager)'
        assert [s for s, _ in steps] == [1000, 1001, 1002, 1003]
        seeds = [tuple(s for _, s in p) for _, p in steps]
        assert len(set(seeds)) == (2 if stepper == 'graph' else 4) and seeds[0] != seeds[1]
    finally:
        ops.SEED_STATE = previous
    want = {}
    for wide in (True, False):
        cd = torch.complex128 if wide else torch.complex64
        with L64.cdtype(cd):
            ref = fill_state(C_NETWORK_Oracle(), 2).train()
            ref = ref.double() if wide else ref
            opt = torch.optim.Adam(ref.parameters(), lr=hp['lr'], eps=hp['optim_eps'], weight_decay=hp['optim_weight_decay'], amsgrad=True)
            losses = []
            for state, p in steps:
                _replay(ref, p, state, (2, 256, 32), wide)
                opt.zero_grad()
                loss = dcs_train_losses(ref, noise.to(cd), noisy.to(cd), clean.to(cd))[2]
                loss.backward()
                torch.nn.utils.clip_grad_norm_(ref.parameters(), 100.0)
                opt.step()
                losses.append(float(loss.detach()))
        want[wide] = losses
    misses = []
    for k, (a, b64, b32) in enumerate(zip(got, want[True], want[False])):
        row = _held(f'step{k}', abs(a - b64), abs(b32 - b64), 2e-3 * abs(b64) + 1e-3, '2e-3 |loss| + 1e-3', misses, ('network', f'train_step_{stepper}'))
        print(f'{stepper} step {k}: loss {a:.6f}, fp64 oracle {b64:.6f}, fp32 oracle {b32:.6f}, bound {row["bound"]:.2e}')
    _record(('network', f'train_step_{stepper}', 'losses'), dict(hip=got, oracle_fp64=want[True], oracle_fp32=want[False],
                                                                    seed_states=[s for s, _ in steps], seconds=time.time() - t0))
    assert not misses, (misses, got, want)
