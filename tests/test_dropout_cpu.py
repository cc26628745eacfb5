"""The host side of the dropout-on parity tests (tests/test_dropout_parity.py), without a GPU.

  the mask      oracle/dropout_mask.py restates dcs_hash32 / dcs_keep_scale (csrc/dcs_common.h): it has to BE splitmix64's
                output function (published vectors), wrap like uint64, and drop a share p.
  the harness   oracle/cnet_oracle.ReplayDropout fed the masks nn.Dropout drew reproduces nn.Dropout bit for bit, forward and
                all gradients; fed all-ones masks it is the dropout-off oracle.
  the bounds    the whole-network bounds of the GPU tests (max-abs error <= 2e-3 of the tensor's max-abs + 1e-6) reject each
                way a fused dropout site can be wrong — by ten times — on one encoder CBN and one decoder CBN + attention
                geometry, and accept the fp32 oracle.
"""
import math

import numpy as np
import pytest
import torch

from oracle import dropout_mask as DM
from oracle import layer_fp64 as L64
from oracle.cnet_oracle import C_NETWORK_Oracle, ReplayDropout, replay_dropout
from oracle.seeded_state import fill_state, seeded_input

REL, ABS = 2e-3, 1e-6            # per tensor: max |got - want| <= REL * max |want| + ABS (tests/test_hip_backward.py: close)


def miss(got, want, rel=REL, abs_=ABS):
    """(max-abs error, bound): the comparison of the whole-network tests."""
    want = want.detach()
    got = got.detach().to(want.dtype)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((got - want).abs().max()), rel * float(want.abs().max()) + abs_


# ------------------------------------------------------------------------------------------------ the mask

def test_hash_is_splitmix64():
    """First outputs of splitmix64 seeded with 0 (state after k steps = k * 0x9E3779B97F4A7C15): indices 1, 2, 3."""
    h = DM.hash64(0, 3, first=1)
    assert [int(v) for v in h] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    u = DM.uniform(0, 1, first=1)
    assert u.dtype == np.float32 and u[0] == np.float32((0xE220A8397B1DCDAF >> 40) / 16777216.0)
    assert abs(float(u[0]) - 0.8833108) < 5e-8
    # the same three through seed, state and index: only their wrapped combination matters
    assert [int(v) for v in DM.hash64(0x9E3779B97F4A7C15, 3)] == [int(v) for v in h]
    assert [int(v) for v in DM.hash64(0x9E3779B97F4A7C15 - 7, 3, state=7)] == [int(v) for v in h]


def test_seed_plus_state_wraps_like_uint64():
    big = 2 ** 63 - 1
    a = DM.hash64(big, 64, state=5)
    assert np.array_equal(a, DM.hash64(big + 5, 64))                  # 2^63 + 4: above int64, inside uint64
    assert np.array_equal(DM.hash64(2 ** 64 - 1, 64, state=5), DM.hash64(4, 64))      # and past 2^64
    assert np.array_equal(DM.hash64(3, 64, state=-1), DM.hash64(2, 64))              # an int64 state read as uint64
    assert not np.array_equal(a, DM.hash64(big, 64))
    k = DM.keep_scale(big, 64, 0.1, state=5)
    assert torch.equal(k, DM.keep_scale(big + 5, 64, 0.1))


@pytest.mark.parametrize('p', [0.1, 0.2, 0.5])
def test_dropped_share(p):
    n = 1 << 22
    k = DM.keep_scale(1234, n, p, state=5)
    assert k.dtype == torch.float64 and set(k.unique().tolist()) == {0.0, 1.0 / (1.0 - p)}
    share = float((k == 0).double().mean())
    sigma = math.sqrt(p * (1 - p) / n)
    print(f'p = {p}: dropped share {share:.5f}, sigma {sigma:.1e}')
    assert abs(share - p) <= 5 * sigma, (share, p, sigma)
    k32 = DM.keep_scale(1234, n, p, state=5, wide=False)
    assert k32.dtype == torch.float32 and torch.equal(k32 == 0, k == 0)
    s32 = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    assert float(k32.max()) == float(s32)


def test_keep_nchw_is_the_channels_last_mask_permuted():
    B, C, H, W = 2, 3, 4, 5
    flat = DM.keep_scale(77, B * H * W * C * 2, 0.5, state=3)
    k = DM.keep_nchw(77, (B, C, H, W), 0.5, state=3)
    assert k.shape == (B, C, H, W, 2) and k.is_contiguous()
    for b, c, h, w, r in ((0, 0, 0, 0, 1), (1, 2, 3, 4, 0), (1, 0, 2, 1, 1), (0, 1, 3, 0, 0)):
        assert k[b, c, h, w, r] == flat[(((b * H + h) * W + w) * C + c) * 2 + r]
    assert torch.equal(DM.keep_like(77, (B, C, H, W), 0.5, 3), k)
    assert torch.equal(DM.keep_like(77, (B, 7, C), 0.5, 3), DM.keep_scale(77, B * 7 * C * 2, 0.5, 3).view(B, 7, C, 2))


# ------------------------------------------------------------------------------------------------ the replay harness

def test_replay_dropout_raises_on_misuse():
    m = ReplayDropout([torch.ones(2, 3, 2)])
    with pytest.raises(ValueError):
        m(torch.zeros(2, 4, 2))
    m(torch.zeros(2, 3, 2))
    with pytest.raises(RuntimeError):
        m(torch.zeros(2, 3, 2))
    left = ReplayDropout([torch.ones(1, 2), torch.ones(1, 2)])
    left(torch.zeros(1, 2))
    with pytest.raises(RuntimeError):
        left.finish()


def _run(net, x, w):
    net.zero_grad()
    out = net(x)
    loss = (w * (out.real ** 2 + 0.5 * out.imag ** 2 + 0.25 * out.real * out.imag)).sum()
    loss.backward()
    return out.detach(), {n: (None if q.grad is None else q.grad.clone()) for n, q in net.named_parameters()}


def _recorded_masks(net, torch_seed, x, w):
    """One training forward + backward of `net` with its own nn.Dropout modules under a fixed torch seed, forward hooks
    recording each call's mask as output over input (where the input is 0 the element counts as kept)."""
    seen = {'conv': [], 'fc': []}

    def hook(key):
        def f(mod, args, out):
            v = args[0].detach()
            ratio = out.detach() / v
            dropped = (out.detach() == 0) & (v != 0)
            live = ratio[(v != 0) & ~dropped]
            s = live.flatten().mode().values                     # 1 / (1 - p) as ATen rounds it
            m = torch.where(dropped, torch.zeros_like(v), s.expand_as(v))
            assert torch.equal(v * m, out.detach()), key         # the recorded mask IS what the module applied
            seen[key].append(m)
        return f

    hooks = [net.dropout_conv.register_forward_hook(hook('conv')), net.dropout_fc.register_forward_hook(hook('fc'))]
    torch.manual_seed(torch_seed)
    try:
        res = _run(net, x, w)
    finally:
        for h in hooks:
            h.remove()
    return res, seen


def test_replay_drops_where_nn_dropout_drops():
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    x = seeded_input(2, 256, 32, seed=3)
    w = torch.rand(2, 256, 32, generator=torch.Generator().manual_seed(1))
    net = fill_state(C_NETWORK_Oracle(), 4).train()
    assert net.dropout_conv.p == 0.1 and net.dropout_fc.p == 0.2
    (out, grads), seen = _recorded_masks(net, 11, x, w)
    assert len(seen['conv']) == 14 and len(seen['fc']) == 1
    shares = [float((m == 0).float().mean()) for m in seen['conv'] + seen['fc']]
    # (a ReLU output is 0 at half its elements, and those count as kept: the encoder sites read about p / 2)
    assert all(0.03 < s < 0.15 for s in shares[:14]) and 0.15 < shares[14] < 0.25, shares
    # every parameter the forward runs has a gradient: 204 parameters, all but the six of decoder_attention.12 / .13
    assert len(grads) == 204 and sorted(n for n, g in grads.items() if g is None) == sorted(
        n for n in grads if n.startswith(('decoder_attention.12.', 'decoder_attention.13.')))
    assert sum(g is not None for g in grads.values()) == 198

    again = fill_state(C_NETWORK_Oracle(), 4).train()
    replay_dropout(again, seen['conv'], seen['fc'])
    out2, grads2 = _run(again, x, w)
    assert torch.equal(out2, out)
    assert grads.keys() == grads2.keys()
    for n, g in grads.items():
        assert (g is None) == (grads2[n] is None), n
        assert g is None or torch.equal(g, grads2[n]), n
    for (n, b), (_, b2) in zip(net.named_buffers(), again.named_buffers()):
        assert torch.equal(b, b2), n

    # all-ones masks: the dropout-off oracle
    off = fill_state(C_NETWORK_Oracle({'dropout_conv': 0.0, 'dropout_fc': 0.0}), 4).train()
    out0, grads0 = _run(off, x, w)
    assert not torch.equal(out0, out)
    ones = fill_state(C_NETWORK_Oracle(), 4).train()
    replay_dropout(ones, [torch.ones_like(m) for m in seen['conv']], [torch.ones_like(m) for m in seen['fc']])
    out1, grads1 = _run(ones, x, w)
    assert torch.equal(out1, out0)
    for n, g in grads0.items():
        assert g is None or torch.equal(g, grads1[n]), n

    # a mask too few / too many is an error, not a silently different network
    short = fill_state(C_NETWORK_Oracle(), 4).train()
    replay_dropout(short, seen['conv'][:13], seen['fc'])
    with pytest.raises(RuntimeError):
        short(x)
    long_ = fill_state(C_NETWORK_Oracle(), 4).train()
    replay_dropout(long_, seen['conv'] + seen['conv'][-1:], seen['fc'])
    with pytest.raises(RuntimeError):
        long_(x)


# ------------------------------------------------------------------------------------------------ the comparison rejects faults

FAULT_GEOMETRIES = ['enc3', 'dec3']            # one CBN-only site (cbn_apply_kernel), one CBN + attention site (attention_apply_kernel)
P_DROP, SEED, STATE = 0.1, 0x5DEECE66D1234567, 5
FAULTS = ('mask_in_nchw_order', 'imag_uses_real_mask', 'index_shifted_by_one', 'backward_without_scale',
          'dropped_before_attention', 'backward_without_state_offset')


def _block_case(name):
    from test_layers_train_size import CBN_LAYERS, _offset_input, _bn_params
    _, C, H, W, act = next(c for c in CBN_LAYERS if c[0] == name)
    x, g = _offset_input(C, 2, H, W, 91 + C)
    att = L64.attention_params(C, 900 + C) if act == 'lrelu' else None
    return (2, C, H, W), x, g, _bn_params(C, C + 2), act, att


def faulty_masks(shape, wide):
    """{fault: (keep, keep_before_attention)} for an activation of complex shape [B,C,H,W]."""
    B, C, H, W = shape
    n = B * C * H * W * 2
    nhwc = lambda flat: flat.view(B, H, W, C, 2).permute(0, 3, 1, 2, 4).contiguous()
    true = DM.keep_nchw(SEED, shape, P_DROP, STATE, wide)
    imag = true.clone()
    imag[..., 1] = imag[..., 0]
    return true, {
        'mask_in_nchw_order': (DM.keep_scale(SEED, n, P_DROP, STATE, wide).view(B, C, H, W, 2), False),
        'imag_uses_real_mask': (imag, False),
        'index_shifted_by_one': (nhwc(DM.keep_scale(SEED, n, P_DROP, STATE, wide, first=1)), False),
        'backward_without_scale': ((true, (true != 0).to(true.dtype)), False),
        'dropped_before_attention': (true, True),
        'backward_without_state_offset': ((true, DM.keep_nchw(SEED, shape, P_DROP, 0, wide)), False),
    }


def _tensors(res):
    out = {k: res[k] for k in ('y', 'gx', 'g_weight', 'g_bias')}
    for n, t in zip(L64.ATT_NAMES, res.get('g_att', ())):
        out[n] = t
    return out


@pytest.mark.parametrize('name', FAULT_GEOMETRIES)
def test_comparison_rejects_dropout_faults(name):
    """"Got" = the fp32 CPU oracle of the block with one fault in its dropout site, reference = the fp64 oracle with the true
    mask, bound = the whole-network one (REL, ABS).  The honest fp32 oracle passes on every tensor; each fault misses on at
    least one tensor by ten times the bound."""
    shape, x, g, bn, act, att = _block_case(name)
    true64, _ = faulty_masks(shape, True)
    true32, faults = faulty_masks(shape, False)
    assert sorted(faults) == sorted(FAULTS)
    ref = _tensors(L64.block_reference(x, g, True, bn, act, att, keep=true64))
    good = _tensors(L64.block_reference(x, g, False, bn, act, att, keep=true32))
    # the mask reached the output where it should: dropped elements are exact zeros
    assert bool((torch.view_as_real(ref['y'])[true64 == 0] == 0).all())
    for k, r in ref.items():
        e, b = miss(good[k], r)
        assert e <= b, (name, 'unfaulted fp32 oracle', k, e, b)
    for fault, (keep, before) in faults.items():
        if before and att is None:
            continue                                           # an encoder site has no attention to be misplaced against
        bad = _tensors(L64.block_reference(x, g, False, bn, act, att, keep=keep, keep_before_attention=before))
        ratios = {k: e / b for k, (e, b) in ((k, miss(bad[k], r)) for k, r in ref.items())}
        worst = max(ratios, key=ratios.get)
        print(f'{name} {fault}: misses {worst} by {ratios[worst]:.1f} x the bound;  y {ratios["y"]:.1f}, gx {ratios["gx"]:.1f}')
        assert ratios[worst] >= 10.0, (name, fault, ratios)
        if fault.startswith('backward_'):
            assert ratios['y'] <= 1.0, (fault, ratios['y'])     # only the backward was touched
