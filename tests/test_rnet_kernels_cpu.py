"""The real network's host algebra, and the comparator of tests/test_rnet_kernels.py, without a GPU.

1. `_RConvFn` (dcsnet/r_network.py) with its four device entries replaced by fp64 torch emulations of their DOCUMENTED
   contracts (the wrappers' docstrings, include/dcsnet_hip.h): the packed B panel's fragment order, the zero-inserted
   stride-1 correlation of the data gradient, the block sum / channel split, and the complex weight gradient
   (gradients of the four real convolutions of the complex layer, complex bias (b_r - b_i) + j (b_r + b_i)).  What is left
   is the host side: panel packing, flip / in-out swap for transposed convs, the four-block recombination
   D_rr / D_ii / D_ir / D_ri of the two complex launches (x and conj x), the bias pairing — compared with fp64 autograd
   through the stock layer.
2. The comparison rule (oracle/rnet_layer_fp64.compare): it accepts a second correct fp32 evaluation of each layer and
   rejects each seeded fault by at least ten times its bound.
"""
import pytest
import torch
from torch.nn import functional as TF

from oracle import rnet_layer_fp64 as R64


# ------------------------------------------------------------------------------------------------ emulated entries

def _unpack_panel(panel, taps, ci, co):
    """Inverse of the documented fragment order: element (tap, kg, nt, lane = 32 kk + j, e) = B[tap][8 kg + 4 kk + e][32 nt + j]
    -> B [taps, ci, co]."""
    nt = (co + 31) // 32
    b = panel.reshape(taps, ci // 8, nt, 2, 32, 4).permute(0, 1, 3, 5, 2, 4)            # [tap, kg, kk, e, nt, j]
    return b.reshape(taps, ci, nt * 32)[:, :, :co]


def _emu_rconv2d(x1, x2, panel, bias, cout, ksize, stride, pad, up=(1, 1), act=0):
    assert act == 0
    x = x1 if x2 is None else torch.cat([x1, x2], dim=-1)
    ci = x.shape[-1]
    w = _unpack_panel(panel, ksize[0] * ksize[1], ci, cout).reshape(*ksize, ci, cout).permute(3, 2, 0, 1)   # w[n, k, dy, dx]
    x = x.permute(0, 3, 1, 2).double()
    if tuple(up) != (1, 1):
        x = x.repeat_interleave(up[0], dim=2).repeat_interleave(up[1], dim=3)
    y = TF.conv2d(x, w.double(), None if bias is None else bias.double(), stride, pad)
    return y.permute(0, 2, 3, 1).contiguous()


def _emu_rconv2d_bwd_data(gy, panel_bwd, Hv, Wv, cin, ksize, stride, pad):
    """gxv = stride-1 correlation of the zero-inserted g_Y with the panel B[tap][k = output channel][n = input channel],
    padding k - 1 - p (rows / columns of the virtual input beyond the last tap's reach get no contribution)."""
    B, Ho, Wo, cout = gy.shape
    kh, kw = ksize
    w = _unpack_panel(panel_bwd, kh * kw, cout, cin).reshape(kh, kw, cout, cin).permute(3, 2, 0, 1).double()
    z = torch.zeros(B, cout, (Ho - 1) * stride[0] + 1, (Wo - 1) * stride[1] + 1, dtype=torch.float64)
    z[:, :, ::stride[0], ::stride[1]] = gy.permute(0, 3, 1, 2).double()
    pf, pt = kh - 1 - pad[0], kw - 1 - pad[1]
    rf, rt = Hv - (z.shape[2] + 2 * pf - kh + 1), Wv - (z.shape[3] + 2 * pt - kw + 1)
    assert 0 <= rf < stride[0] and 0 <= rt < stride[1]
    z = TF.pad(z, (pt, pt + rt, pf, pf + rf))
    return TF.conv2d(z, w).permute(0, 2, 3, 1).contiguous()


def _emu_upsample_cat_bwd(gxv, H, W, c1, c2, up):
    return R64.upsample_cat_bwd_reference(gxv, H, W, c1, c2, up)


def _emu_cconv2d_bwd_weight(x1, x2, gy, w_shape, has_bias, ksize, stride, pad, up=(1, 1), transposed=False, outs=None,
                            immediate=False):
    """Gradients of the complex layer's four real convolutions (y_r = conv_r x_r - conv_i x_i, y_i = conv_r x_i + conv_i x_r,
    each real conv carrying its own bias) in the [Cout,Cin,kh,kw] layout; x*, gy: [B,H,W,C,2]."""
    assert not transposed and outs is None
    x = x1 if x2 is None else torch.cat([x1, x2], dim=3)
    x = x.double().permute(0, 3, 1, 2, 4)
    if tuple(up) != (1, 1):
        x = x.repeat_interleave(up[0], dim=2).repeat_interleave(up[1], dim=3)
    xr, xi = x[..., 0].detach(), x[..., 1].detach()
    g = gy.detach().double().permute(0, 3, 1, 2, 4)
    with torch.enable_grad():                              # (called from inside a backward)
        w_r, w_i = (torch.zeros(w_shape, dtype=torch.float64, requires_grad=True) for _ in range(2))
        b_r, b_i = (torch.zeros(w_shape[0], dtype=torch.float64, requires_grad=True) for _ in range(2))
        cr = lambda t: TF.conv2d(t, w_r, b_r, stride, pad)
        ci = lambda t: TF.conv2d(t, w_i, b_i, stride, pad)
        yr, yi = cr(xr) - ci(xi), cr(xi) + ci(xr)
        (yr * g[..., 0] + yi * g[..., 1]).sum().backward()
    return w_r.grad, w_i.grad, (b_r.grad if has_bias else None), (b_i.grad if has_bias else None)


@pytest.fixture
def emulated(monkeypatch):
    from dcsnet import r_network as rn, ops
    monkeypatch.setattr(rn, 'rconv2d', _emu_rconv2d)
    monkeypatch.setattr(rn, 'rconv2d_bwd_data', _emu_rconv2d_bwd_data)
    monkeypatch.setattr(rn, 'upsample_cat_bwd', _emu_upsample_cat_bwd)
    monkeypatch.setattr(ops, 'cconv2d_bwd_weight', _emu_cconv2d_bwd_weight)
    monkeypatch.setattr(rn, '_CONJ', {})
    return rn


HOST_CASES = {   # B, H, W, c1, c2, cout, k, transposed, stride, pad, up, bias
    'plain_strided': (2, 6, 5, 32, 0, 48, 3, False, (2, 1), (1, 1), (1, 1), True),
    'plain_k5_even': (1, 6, 8, 16, 0, 16, 5, False, (2, 2), (2, 2), (1, 1), True),
    'transposed_cat_up': (2, 3, 4, 16, 16, 48, 3, True, (1, 1), (1, 1), (2, 1), True),
    'transposed_cat_up22_nobias': (1, 2, 3, 32, 16, 16, 3, True, (1, 1), (1, 1), (2, 2), False),
}


@pytest.mark.parametrize('name', list(HOST_CASES))
def test_rconv_host_algebra_against_fp64_autograd(emulated, name):
    """_RConvFn forward and backward on CPU tensors over the emulated entries: y, g_x1, g_x2, g_w (the module's layout),
    g_b against autograd through conv2d / conv_transpose2d in fp64 — to 1e-6 (g_b is stored in fp32 by the node)."""
    B, H, W, c1, c2, cout, k, transposed, stride, pad, up, bias = HOST_CASES[name]
    case = R64.rconv_case(B, H, W, c1, c2, cout, k, transposed, seed=len(name), bias=bias)
    g = torch.Generator().manual_seed(5)
    gy = torch.randn(R64.rconv_out_shape(case, transposed, stride, pad, up), generator=g)
    ref = R64.rconv_reference(case, transposed, stride, pad, up, gy, True)
    leaf = lambda t: None if t is None else t.double().requires_grad_(True)
    x1, x2, w, b = (leaf(case[n]) for n in ('x1', 'x2', 'w', 'b'))
    y = emulated._RConvFn.apply(x1, x2, w, b, transposed, stride, pad, up)
    assert y.shape == ref['y'].shape
    y.backward(gy.double())
    got = dict(y=y.detach(), g_x1=x1.grad, g_x2=None if x2 is None else x2.grad, g_w=w.grad, g_b=None if b is None else b.grad)
    for key, r in ref.items():
        if r is None:
            assert got[key] is None, key
            continue
        e = R64.rel_max(got[key].double(), r)
        print(f'{name} {key}: {e:.2e}')
        assert e <= 1e-6, (name, key, e)


# ------------------------------------------------------------------------------------------------ the comparator

CONV_SELF = dict(B=2, H=12, W=10, c1=32, c2=0, cout=64, k=5, transposed=False, stride=(2, 2), pad=(2, 2), up=(1, 1))


def _conv_self_case():
    c = CONV_SELF
    case = R64.rconv_case(c['B'], c['H'], c['W'], c['c1'], c['c2'], c['cout'], c['k'], c['transposed'], seed=11)
    gy = torch.randn(R64.rconv_out_shape(case, c['transposed'], c['stride'], c['pad'], c['up']),
                     generator=torch.Generator().manual_seed(12))
    geo = (c['transposed'], c['stride'], c['pad'], c['up'])
    return case, gy, geo


def _second_fp32_conv(case, gy, geo):
    """A second correct fp32 evaluation in another summation order: the conv as the sum of two convs over complementary
    (checkerboard) halves of the taps."""
    transposed, stride, pad, up = geo
    leaf = lambda t: t.clone().requires_grad_(True)
    x1, w, b = leaf(case['x1']), leaf(case['w']), leaf(case['b'])
    k = w.shape[2]
    m = ((torch.arange(k)[:, None] + torch.arange(k)[None, :]) % 2).float()
    y = R64.rconv_forward(x1, None, w * m, b, transposed, stride, pad, up) + R64.rconv_forward(x1, None, w * (1 - m), None, transposed, stride, pad, up)
    (y * gy).sum().backward()
    return dict(y=y.detach(), g_x1=x1.grad, g_x2=None, g_w=w.grad, g_b=b.grad)


def _assert_rejected(name, bad, ref, ref32, key, **kw):
    e, lim = R64.score(bad, ref[key], ref32[key], key, **kw)
    print(f'fault {name}: {key} err {e:.3g}, bound {lim:.3g}, ratio {e / lim:.3g}')
    assert e >= 10.0 * lim, (name, key, e, lim)


def test_comparator_accepts_fp32_and_rejects_conv_faults():
    case, gy, geo = _conv_self_case()
    ref, ref32 = R64.rconv_reference(case, *geo, gy, True), R64.rconv_reference(case, *geo, gy, False)
    rows, misses = R64.compare(_second_fp32_conv(case, gy, geo), ref, ref32)
    print({k: f'{v["err"]:.2e}' for k, v in rows.items()})
    assert not misses, misses
    assert not any(v['fallback'] for v in rows.values()), rows        # at this K = 800 stock fp32 holds the tolerance
    f32 = lambda t: t.float()
    _assert_rejected('last row of the data gradient zeroed', R64.fault_dgrad_last_row(f32(ref['g_x1'])), ref, ref32, 'g_x1')
    # (an untransposed conv: the module's layout IS the correlation layout g_corr)
    _assert_rejected('D_ir / D_ri swapped in one 16-channel block', R64.fault_wgrad_swapped_block(f32(ref['g_w'])), ref, ref32, 'g_w')
    _assert_rejected('bias-gradient sign flipped', R64.fault_bias_sign(f32(ref['g_b'])), ref, ref32, 'g_b')


def test_comparator_accepts_fp32_and_rejects_exchanged_bn_statistics():
    Cr, shape = 32, (3, 7, 5)
    x = R64.bn_input(shape, Cr, seed=21)
    w, b, rm, rv = R64.bn_params(Cr, 22)
    g = torch.randn(*shape, Cr, generator=torch.Generator().manual_seed(23))
    args = (x, w, b, rm, rv, 1e-5, 0.1, True, 'none', g)
    ref, ref32 = R64.bn_reference(*args, True), R64.bn_reference(*args, False)
    # second fp32 evaluation: the normalisation written out from fp32 moments about a pivot
    piv = x[0, 0, 0]
    d = x - piv
    mean = d.mean(dim=(0, 1, 2))
    var = (d * d).mean(dim=(0, 1, 2)) - mean * mean
    alt = (d - mean) / (var + 1e-5).sqrt() * w + b
    rows, misses = R64.compare(dict(y=alt), dict(y=ref['y']), dict(y=ref32['y']))
    print(rows)
    assert not misses, misses
    _assert_rejected('BN statistics of channels 2c / 2c+1 exchanged', R64.fault_bn_pair_statistics(x, w, b, 1e-5).float(), ref, ref32, 'y')


@pytest.mark.parametrize('hidden', [64, 128])
def test_comparator_accepts_fp32_and_rejects_lstm_faults(hidden):
    lstm = R64.lstm_module(hidden, seed=hidden)
    state = lstm.state_dict()
    g = torch.Generator().manual_seed(31)
    kw = dict(tol_fwd=R64.TOL_LSTM, tol_bwd=R64.TOL_LSTM, abs_tol=R64.ABS_LSTM)
    for B, S in ((2, 2), (2, 3)):
        x, g_out = torch.randn(B, S, 2 * hidden, generator=g), torch.randn(B, S, 2 * hidden, generator=g)
        ref, ref32 = R64.lstm_reference(state, hidden, x, g_out, True), R64.lstm_reference(state, hidden, x, g_out, False)
        hand = R64.lstm_by_hand(state, hidden, x)
        assert R64.rel_max(hand, ref['y']) <= 1e-12                  # the written-out recurrence IS nn.LSTM
        # second fp32 evaluation: the written-out recurrence rounded to fp32 at the end is exact to half an ulp; the rule
        # has to accept it and the stock fp32 layer alike
        for alt in (hand.float(), ref32['y']):
            rows, misses = R64.compare(dict(y=alt), dict(y=ref['y']), dict(y=ref32['y']), **kw)
            assert not misses, misses
        _assert_rejected(f'S={S}: reverse direction reads h_(t-1)', R64.lstm_by_hand(state, hidden, x, reverse_reads_previous=True).float(),
                         ref, ref32, 'y', **kw)
        if S == 2:
            _assert_rejected('S=2: step 0 read again', R64.lstm_by_hand(state, hidden, x, reread_first=True).float(), ref, ref32, 'y', **kw)


def test_bn_input_is_what_the_issue_asks_for():
    """Per-channel mean several times the spread, even / odd neighbours correlated at about 0.9."""
    x = R64.bn_input((3, 7, 5), 32, seed=4).double().reshape(-1, 32)
    ratio = x.mean(0).abs() / x.std(0)
    assert float(ratio.min()) >= 2.0, ratio
    c = torch.corrcoef(x.t())
    rho = torch.stack([c[2 * i, 2 * i + 1] for i in range(16)])
    assert float(rho.min()) >= 0.75 and float(rho.mean()) >= 0.85, rho
    assert float(x.std(0).max() / x.std(0).min()) >= 2.0


def test_bn_seeds_decide_every_activation():
    """The seeds of the GPU module's BatchNorm table: no pre-activation of the fp64 layer within 1e-6 of zero (relative to its
    channel's largest value), in train and in eval mode — the GPU tests assert the same before they compare."""
    cases = [(c, R64.BN_SHAPE) for c in R64.BN_CHANNELS] + [R64.BN_SMALL] + [(1, s) for s in R64.BN_ONE_CHANNEL.values()]
    for Cr, shape in cases:
        for use_batch in (True, False):
            x, (w, b, rm, rv), _ = R64.bn_case(Cr, shape, use_batch)
            margin = R64.bn_pre_activation_margin(x, w, b, rm, rv, R64.BN_EPS, use_batch)
            assert margin > 1e-6, (Cr, shape, use_batch, margin)
