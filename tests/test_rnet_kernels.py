"""The real network's (R_NETWORK: DR-Net / DRS-Net) training kernels, one at a time, against fp64 — every element.

The only other check of these entry points is the whole-network golden test (test_rnetwork_gradients_against_reference_vectors:
one shape, 3e-3 of each tensor's max, big tensors sampled, conv biases in front of a BatchNorm skipped).  Here each piece
runs alone, driven the way R_NETWORK drives it, and is compared with the stock torch layer in double on the CPU
(oracle/rnet_layer_fp64.py):

  real conv      `_RConvFn` (dcs_rconv2d_fwd, dcs_rconv2d_bwd_data, dcs_upsample_cat_bwd, two complex weight-gradient launches
                 recombined into the D_rr / D_ii / D_ir / D_ri blocks, bias pairing) over the network's geometries, shrunk: the
                 four strided encoder forms at even extents ((Hv + 2p - k) % s = 1: the last input row gets fewer taps), odd
                 extents and Hout = 1; the transposed decoder forms with cat + upsample (K = 9 * 512, the N = 16 panel, a
                 ragged column tile); bias=None; in both arithmetic modes.  No BatchNorm follows, so g_b is O(1) and its sign
                 and pairing show.  The raw wrappers `rconv2d` (activation epilogues, bias=None) and `upsample_cat_bwd`.
  BatchNorm      `_RBnFn` (dcs_rbn_fwd / dcs_rbn_bwd): y, g_x, g_weight, g_bias, running statistics (unbiased variance) at
                 Cr = 16 .. 512 with a pixel count that is no multiple of the kernels' rows per pass, three activations,
                 momentum 0.1 / cumulative average (through `_bn_act`, which resolves momentum=None to 1 / n) / eval
                 statistics, affine=None, the one-channel layout and its P % 4 rule.  Inputs: per-channel mean 3 .. 6 spreads
                 off zero, even / odd neighbours correlated at 0.9.
  LSTM           the hidden-size-128 recurrence (`_lstm`: inference entry and `_LstmRecFn` + dcs_lstm_layer_bwd) at
                 S = 1, 2, 3, 8, 64 against nn.LSTM(256, 128, 2, bidirectional) — S = 2, 3 are where the backward kernel's
                 two-step look-ahead wraps; one-step cotangents; saturated gates.
  enc0 / dec6    `_enc0`, `_dec_last`: the real-to-complex weight and bias maps, grad-enabled and cached-pack routes.

Rule: oracle/rnet_layer_fp64.compare — 2e-5 of the tensor's max-abs forward, 1e-4 gradients, the LSTM 1e-4 + 1e-6 absolute;
where the stock fp32 CPU layer itself misses the tolerance, 16 times its error (recorded).  Every figure goes to
rnet_kernel_parity.json in $DCS_PARITY_DIR (default parity_out/); a full run's file is committed as
profiles/rnet_kernel_parity.json.  The comparator is tested without a GPU in tests/test_rnet_kernels_cpu.py.

Measured (MI355X, full run, profiles/rnet_kernel_parity.json): worst error / worst ratio to the fp32 CPU
layer's error — conv forward 1.1e-6 / 1.1, data gradient 8.9e-7 / 2.0, weight + bias gradient 3.2e-7 / 2.0, BatchNorm
6.3e-6 / 8.1 (5.4e-8 against 6.6e-9), LSTM 1.4e-6 / 3.0, enc0 / dec6 7.1e-7 / 1.4; the 16 x cpu32 fallback applied nowhere.
"""
import functools
import types

import pytest
import torch

from oracle import rnet_layer_fp64 as R64
from _ragged_helpers import record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from dcsnet import _lib
    _lib.load()
    threads = R64.set_threads()
    yield torch.device('cuda:0')
    torch.set_num_threads(threads)


_record = functools.partial(record, 'rnet_kernel_parity.json')     # figures -> $DCS_PARITY_DIR/rnet_kernel_parity.json (default parity_out/)


def _judge(path, got, ref, ref32, **kw):
    rows, misses = R64.compare(got, ref, ref32, **kw)
    for k, v in rows.items():
        print(f'{"/".join(path)} {k}: err {v["err"]:.3e} cpu32 {v["cpu32"]:.3e} limit {v["limit"]:.3e}{" (fallback)" if v["fallback"] else ""}')
    _record(path, rows)
    assert not misses, misses
    return rows


def _cpu(t):
    return None if t is None else t.detach().cpu()


# ------------------------------------------------------------------------------------------------ real conv

ENC_FORMS = {'k5s22_32to64': (32, 64, 5, (2, 2)), 'k5s21_64to128': (64, 128, 5, (2, 1)),
             'k3s21_128to256': (128, 256, 3, (2, 1)), 'k3s21_256to256': (256, 256, 3, (2, 1))}
ENC_SHAPES = {'even': (2, 12, 10), 'odd': (3, 7, 9), 'hout1': (1, 2, 32)}
# name -> (B, H, W, c1, c2, cout, k, transposed, stride, pad, up, bias)
CONV_CASES = {f'enc_{f}_{s}': (*ENC_SHAPES[s], c, 0, co, k, False, st, (k // 2, k // 2), (1, 1), True)
              for f, (c, co, k, st) in ENC_FORMS.items() for s in ENC_SHAPES}
CONV_CASES.update({
    'dec_latent_512to256_up21': (1, 2, 32, 256, 256, 256, 3, True, (1, 1), (1, 1), (2, 1), True),      # K = 9 * 512
    'dec_256to64_up21': (2, 4, 16, 128, 128, 64, 3, True, (1, 1), (1, 1), (2, 1), True),
    'dec_64to16_up22': (2, 6, 5, 32, 32, 16, 3, True, (1, 1), (1, 1), (2, 2), True),                  # N = 16 panel padded to 32
    'dec_128to48_up22': (2, 5, 7, 64, 64, 48, 3, True, (1, 1), (1, 1), (2, 2), True),                 # ragged second column tile
    'enc_k5s22_32to64_even_nobias': (2, 12, 10, 32, 0, 64, 5, False, (2, 2), (2, 2), (1, 1), False),
    'dec_64to16_up22_nobias': (2, 6, 5, 32, 32, 16, 3, True, (1, 1), (1, 1), (2, 2), False),
})
_CONV_REFS = {}


def _conv_refs(name):
    if name not in _CONV_REFS:
        B, H, W, c1, c2, cout, k, transposed, stride, pad, up, bias = CONV_CASES[name]
        case = R64.rconv_case(B, H, W, c1, c2, cout, k, transposed, seed=1 + list(CONV_CASES).index(name), bias=bias)
        geo = (transposed, stride, pad, up)
        gy = torch.randn(R64.rconv_out_shape(case, *geo), generator=torch.Generator().manual_seed(case['seed'] + 500))
        _CONV_REFS[name] = (case, geo, gy, R64.rconv_reference(case, *geo, gy, True), R64.rconv_reference(case, *geo, gy, False))
    return _CONV_REFS[name]


def test_conv_table_has_the_edges_it_claims():
    for name, (B, H, W, c1, c2, cout, k, transposed, stride, pad, up, bias) in CONV_CASES.items():
        assert (c1 + c2) % 16 == 0 and cout % 16 == 0 and (c1 // 2) % 2 == 0 and (cout // 2) % 2 == 0, name
        if name.startswith('enc_'):
            rem = (H + 2 * pad[0] - k) % stride[0]
            hout = (H + 2 * pad[0] - k) // stride[0] + 1
            assert rem == (0 if name.endswith('_odd') else 1), (name, rem)
            assert (hout == 1) == name.endswith('_hout1'), (name, hout)


@pytest.mark.parametrize('mode', ['bf16x6', 'f32'])
@pytest.mark.parametrize('name', list(CONV_CASES))
def test_rconv_node_against_fp64(dev, name, mode):
    """_RConvFn forward, data gradient, weight and bias gradient for a random cotangent, in one arithmetic mode."""
    from dcsnet import ops
    from dcsnet.r_network import _RConvFn
    case, (transposed, stride, pad, up), gy, ref, ref32 = _conv_refs(name)
    leaf = lambda t: None if t is None else t.to(dev).requires_grad_(True)
    x1, x2, w, b = (leaf(case[n]) for n in ('x1', 'x2', 'w', 'b'))
    default = ops.conv_precision()
    ops.set_conv_precision(mode)
    try:
        y = _RConvFn.apply(x1, x2, w, b, transposed, stride, pad, up)
        assert tuple(y.shape) == tuple(ref['y'].shape)
        y.backward(gy.to(dev))
        torch.cuda.synchronize()
    finally:
        ops.set_conv_precision(default)
    g = lambda t: None if t is None else _cpu(t.grad)
    _judge(('conv', name, mode), dict(y=_cpu(y), g_x1=g(x1), g_x2=g(x2), g_w=g(w), g_b=g(b)), ref, ref32)


RAW_GEOMETRIES = {'strided_k5': (2, 9, 7, 32, 0, 64, 5, (2, 2), (1, 1)), 'cat_up_k3': (3, 6, 8, 16, 16, 48, 3, (1, 1), (2, 2))}


@pytest.mark.parametrize('act', ['relu', 'lrelu', 'sigmoid'])
@pytest.mark.parametrize('geometry', list(RAW_GEOMETRIES))
def test_rconv2d_activation_epilogue_and_no_bias(dev, geometry, act):
    """The raw forward wrapper: act(conv + bias) and act(conv) with bias=None."""
    from dcsnet import functional as F, r_network as rn
    B, H, W, c1, c2, cout, k, stride, up = RAW_GEOMETRIES[geometry]
    case = R64.rconv_case(B, H, W, c1, c2, cout, k, False, seed=70 + len(geometry))
    code = {'relu': F.ACT_RELU, 'lrelu': F.ACT_LRELU, 'sigmoid': F.ACT_SIGMOID}[act]
    d = lambda t: None if t is None else t.to(dev)
    panel = rn.pack_real_panel(case['w'].to(dev))
    for bias in (case['b'], None):
        refs = [R64.rconv_forward(case['x1'].to(dt), None if case['x2'] is None else case['x2'].to(dt), case['w'].to(dt),
                                  None if bias is None else bias.to(dt), False, stride, (k // 2, k // 2), up, act)
                for dt in (torch.float64, torch.float32)]
        got = rn.rconv2d(d(case['x1']), d(case['x2']), panel, d(bias), cout, (k, k), stride, (k // 2, k // 2), up, code)
        assert float((refs[0] > 0).double().mean()) > 0.2 and float((refs[0] < 0.5).double().mean()) > 0.2       # both branches live
        _judge(('rconv2d', geometry, act, 'bias' if bias is not None else 'no_bias'), dict(y=_cpu(got)), dict(y=refs[0]), dict(y=refs[1]))


@pytest.mark.parametrize('c1,c2,up', [(32, 16, (1, 1)), (32, 16, (2, 1)), (32, 16, (2, 2)), (16, 32, (2, 2))])
def test_upsample_cat_bwd_with_real_channel_counts(dev, c1, c2, up):
    from dcsnet import r_network as rn
    B, H, W = 2, 5, 7
    gxv = torch.randn(B, H * up[0], W * up[1], c1 + c2, generator=torch.Generator().manual_seed(c1 + up[0] + 2 * up[1]))
    want = R64.upsample_cat_bwd_reference(gxv, H, W, c1, c2, up)
    want32 = tuple(t.float() for t in R64.upsample_cat_bwd_reference(gxv, H, W, c1, c2, up))
    g1, g2 = rn.upsample_cat_bwd(gxv.to(dev), H, W, c1, c2, up)
    assert tuple(g1.shape) == (B, H, W, c1) and tuple(g2.shape) == (B, H, W, c2)
    _judge(('upsample_cat_bwd', f'{c1}+{c2}_up{up[0]}{up[1]}'), dict(g_x1=_cpu(g1), g_x2=_cpu(g2)),
           dict(g_x1=want[0], g_x2=want[1]), dict(g_x1=want32[0], g_x2=want32[1]))


# ------------------------------------------------------------------------------------------------ real BatchNorm

def _act_code(act):
    from dcsnet import functional as F
    return {'none': F.ACT_NONE, 'relu': F.ACT_RELU, 'lrelu': F.ACT_LRELU}[act]


def _run_bn(dev, x, params, g, momentum, use_batch, act, calls=1, affine=True):
    """`calls` consecutive train-mode passes through R_NETWORK._bn_act on a BatchNorm2d holding the case's parameters and
    running statistics (momentum None: the module's cumulative average), or one eval-mode pass; backward of the last."""
    from dcsnet.r_network import R_NETWORK
    w, b, rm, rv = params
    Cr = w.numel()
    bn = torch.nn.BatchNorm2d(Cr, eps=R64.BN_EPS, momentum=momentum, affine=affine)
    with torch.no_grad():
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
        if affine:
            bn.weight.copy_(w)
            bn.bias.copy_(b)
    bn = bn.to(dev)
    holder = types.SimpleNamespace(training=bool(use_batch))
    for _ in range(calls):
        xd = x.to(dev).requires_grad_(True)
        y = R_NETWORK._bn_act(holder, bn, xd, _act_code(act))
    return bn, xd, y


def _bn_got(bn, xd, y):
    return dict(y=_cpu(y), g_x=_cpu(xd.grad), g_weight=None if bn.weight is None else _cpu(bn.weight.grad),
                g_bias=None if bn.bias is None else _cpu(bn.bias.grad), running_mean=_cpu(bn.running_mean), running_var=_cpu(bn.running_var))


BN_MODES = {'momentum0.1': (0.1, True, 1), 'cumulative_two_calls': (None, True, 2), 'eval': (0.1, False, 1)}


@pytest.mark.parametrize('mode', list(BN_MODES))
@pytest.mark.parametrize('act', ['none', 'relu', 'lrelu'])
@pytest.mark.parametrize('Cr,shape', [(c, R64.BN_SHAPE) for c in R64.BN_CHANNELS] + [R64.BN_SMALL])
def test_rbn_against_fp64(dev, Cr, shape, act, mode):
    momentum, use_batch, calls = BN_MODES[mode]
    x, params, g = R64.bn_case(Cr, shape, use_batch)
    w, b, rm, rv = params
    # every ReLU / leaky-ReLU branch of the reference is decided: nothing needs exempting
    assert R64.bn_pre_activation_margin(x, w, b, rm, rv, R64.BN_EPS, use_batch) > 1e-6
    args = (x, w, b, rm, rv, R64.BN_EPS, momentum, use_batch, act, g)
    ref, ref32 = R64.bn_reference(*args, True, calls=calls), R64.bn_reference(*args, False, calls=calls)
    bn, xd, y = _run_bn(dev, x, params, g, momentum, use_batch, act, calls)
    y.backward(g.to(dev))
    got = _bn_got(bn, xd, y)
    if use_batch:                                       # the update uses the unbiased estimator, and the biased one would not pass
        P = x.numel() // Cr
        unb = x.double().reshape(P, Cr).var(dim=0, unbiased=True)
        f = 0.1 if momentum is not None else 1.0        # cumulative average of two identical batches: the batch's own estimate
        want = (1 - f) * rv.double() + f * unb
        assert R64.rel_max(ref['running_var'], want) <= 1e-12
        biased = want - f * unb / P
        assert R64.rel_max(biased, want) > 10 * R64.TOL_FWD
        assert int(bn.num_batches_tracked) == calls
    _judge(('bn', f'Cr{Cr}_P{x.numel() // Cr}', act, mode), got, ref, ref32)


@pytest.mark.parametrize('use_batch', [True, False])
def test_rbn_without_affine_returns_no_parameter_gradients(dev, use_batch):
    from dcsnet.r_network import _RBnFn
    Cr, shape = 32, R64.BN_SHAPE
    x, (w, b, rm, rv), g = R64.bn_case(Cr, shape, use_batch)
    args = (x, None, None, rm, rv, R64.BN_EPS, 0.1, use_batch, 'none', g)
    ref, ref32 = R64.bn_reference(*args, True), R64.bn_reference(*args, False)
    xd, rmd, rvd = x.to(dev).requires_grad_(True), rm.to(dev), rv.to(dev)
    y = _RBnFn.apply(xd, None, None, rmd, rvd, R64.BN_EPS, 0.1, use_batch, _act_code('none'))
    out = _RBnFn.backward(y.grad_fn, g.to(dev))         # the node's own return values: (g_x, g_weight, g_bias, ...)
    assert out[1] is None and out[2] is None and all(o is None for o in out[3:])
    y.backward(g.to(dev))
    got = dict(y=_cpu(y), g_x=_cpu(xd.grad), g_weight=None, g_bias=None, running_mean=_cpu(rmd), running_var=_cpu(rvd))
    assert torch.equal(out[0].cpu(), got['g_x'])
    _judge(('bn', 'no_affine', 'train' if use_batch else 'eval'), got, ref, ref32)


@pytest.mark.parametrize('mode', ['momentum0.1', 'eval'])
def test_rbn_one_channel_layout(dev, mode):
    """x.dim() == 3, P % 4 == 0: the [B,F,T] values read as P/2 (re, im) pairs of ONE channel — forward and backward."""
    momentum, use_batch, calls = BN_MODES[mode]
    shape = R64.BN_ONE_CHANNEL['p_mod4_0']
    x, params, g = R64.bn_case(1, shape, use_batch)
    assert x.dim() == 3 and x.numel() % 4 == 0
    args = (x, *params, R64.BN_EPS, momentum, use_batch, 'none', g)
    ref, ref32 = R64.bn_reference(*args, True), R64.bn_reference(*args, False)
    bn, xd, y = _run_bn(dev, x, params, g, momentum, use_batch, 'none')
    y.backward(g.to(dev))
    _judge(('bn', 'one_channel_P60', mode), _bn_got(bn, xd, y), ref, ref32)


def test_rbn_one_channel_scalar_tail_forward_and_refused_backward(dev):
    """P % 4 == 2: the forward runs (the C == 1 path's scalar tail), the backward refuses (its kernels read float4 pairs)."""
    from dcsnet._lib import DcsHipError
    shape = R64.BN_ONE_CHANNEL['p_mod4_2']
    x, params, g = R64.bn_case(1, shape, True)
    assert x.numel() % 4 == 2
    args = (x, *params, R64.BN_EPS, 0.1, True, 'none', g)
    ref, ref32 = R64.bn_reference(*args, True), R64.bn_reference(*args, False)
    bn, xd, y = _run_bn(dev, x, params, g, 0.1, True, 'none')
    keys = ('y', 'running_mean', 'running_var')
    got = _bn_got(bn, xd, y)
    _judge(('bn', 'one_channel_P18', 'forward_only'), {k: got[k] for k in keys}, {k: ref[k] for k in keys}, {k: ref32[k] for k in keys})
    with pytest.raises(DcsHipError):
        y.backward(g.to(dev))
    assert xd.grad is None


# ------------------------------------------------------------------------------------------------ LSTM, hidden size 128

LSTM_SHAPES = [(1, 1), (2, 2), (2, 3), (2, 8), (3, 64)]
HID = 128
LSTM_TOL = dict(tol_fwd=R64.TOL_LSTM, tol_bwd=R64.TOL_LSTM, abs_tol=R64.ABS_LSTM)
_LSTM = {}


def _lstm_state():
    if 'state' not in _LSTM:
        _LSTM['state'] = {k: v.clone() for k, v in R64.lstm_module(HID, seed=128).state_dict().items()}
    return _LSTM['state']


def _lstm_operands(B, S, scale=0.8, cotangent=None):
    g = torch.Generator().manual_seed(1000 * B + S)
    x, g_out = torch.randn(B, S, 2 * HID, generator=g) * scale, torch.randn(B, S, 2 * HID, generator=g)
    if cotangent is not None:                           # non-zero at one time step only
        keep = torch.zeros(S, dtype=torch.bool)
        keep[0 if cotangent == 'first' else S - 1] = True
        g_out = g_out * keep[None, :, None]
    return x, g_out


def _hip_lstm(dev, x, g_out=None):
    """R_NETWORK._lstm on a holder that carries `.lstm` (the 16 parameter tensors as the network holds them)."""
    from dcsnet.r_network import R_NETWORK
    lstm = torch.nn.LSTM(2 * HID, HID, 2, bidirectional=True, batch_first=True)
    lstm.load_state_dict(_lstm_state())
    holder = types.SimpleNamespace(lstm=lstm.to(dev))
    if g_out is None:
        with torch.no_grad():
            return dict(y=_cpu(R_NETWORK._lstm(holder, x.to(dev))))
    xd = x.to(dev).requires_grad_(True)
    y = R_NETWORK._lstm(holder, xd)
    assert y.grad_fn is not None
    y.backward(g_out.to(dev))
    got = dict(y=_cpu(y), g_x=_cpu(xd.grad))
    got.update({n: _cpu(q.grad) for n, q in lstm.named_parameters()})
    assert len(got) == 2 + 16
    return got


def _lstm_refs(x, g_out):
    return tuple(R64.lstm_reference(_lstm_state(), HID, x, g_out, wide) for wide in (True, False))


@pytest.mark.parametrize('B,S', LSTM_SHAPES)
def test_lstm128_inference_path(dev, B, S):
    x, g_out = _lstm_operands(B, S)
    ref, ref32 = _lstm_refs(x, g_out)
    _judge(('lstm128', f'B{B}_S{S}', 'inference'), _hip_lstm(dev, x), dict(y=ref['y']), dict(y=ref32['y']), **LSTM_TOL)


@pytest.mark.parametrize('B,S', LSTM_SHAPES)
def test_lstm128_training_path(dev, B, S):
    x, g_out = _lstm_operands(B, S)
    ref, ref32 = _lstm_refs(x, g_out)
    # one step: h_(t-1) = 0, so the recurrent weights get no gradient
    zero_ok = tuple(n for n in ref if n.startswith('weight_hh')) if S == 1 else ()
    _judge(('lstm128', f'B{B}_S{S}', 'training'), _hip_lstm(dev, x, g_out), ref, ref32, zero_ok=zero_ok, **LSTM_TOL)


@pytest.mark.parametrize('where', ['first', 'last'])
@pytest.mark.parametrize('B,S', [(2, 3), (2, 8)])
def test_lstm128_one_step_cotangent(dev, B, S, where):
    """A cotangent at one time step: the forward direction's gradient then flows only to earlier steps, the reverse
    direction's only to later ones — an off-by-one in the reverse direction's h_(t+-1) cannot hide in a dense sum."""
    x, g_out = _lstm_operands(B, S, cotangent=where)
    ref, ref32 = _lstm_refs(x, g_out)
    # the last layer's chain that STARTS at the cotangent's step has h = 0 behind it there: no recurrent-weight gradient
    zero_ok = ('weight_hh_l1',) if where == 'first' else ('weight_hh_l1_reverse',)
    assert all(float(ref[n].abs().max()) == 0 for n in zero_ok)
    _judge(('lstm128', f'B{B}_S{S}', f'cotangent_{where}'), _hip_lstm(dev, x, g_out), ref, ref32, zero_ok=zero_ok, **LSTM_TOL)


def test_lstm128_saturated_gates(dev):
    B, S = 2, 8
    x, g_out = _lstm_operands(B, S, scale=5.0)
    pre = R64.lstm_first_layer_preactivations(_lstm_state(), x)
    assert float(pre.max()) >= 8.0 and float((pre > 6.0).double().mean()) > 1e-3, float(pre.max())
    ref, ref32 = _lstm_refs(x, g_out)
    _judge(('lstm128', f'B{B}_S{S}', 'saturated'), _hip_lstm(dev, x, g_out), ref, ref32, **LSTM_TOL)


# ------------------------------------------------------------------------------------------------ enc0, dec6

def _both_routes(path, run, leaves, params, g_out, ref, ref32, names):
    """run(): the piece under grad mode (gradients of `leaves` + `params`) and under no_grad (cached packs)."""
    y = run()
    assert y.grad_fn is not None
    y.backward(g_out)
    got = dict(y=_cpu(y))
    got.update({n: _cpu(t.grad) for n, t in zip(names, leaves + params)})
    _judge(path + ('grad_route',), got, ref, ref32)
    with torch.no_grad():
        y2, y3 = run(), run()
    assert y2.grad_fn is None and torch.equal(y2, y3)
    _judge(path + ('no_grad_route',), dict(y=_cpu(y2)), dict(y=ref['y']), dict(y=ref32['y']))
    scale = float(ref['y'].abs().max())
    assert float((y2 - y.detach()).abs().max()) <= R64.TOL_FWD * scale


def test_enc0_against_fp64_conv2d(dev):
    from dcsnet.r_network import R_NETWORK
    torch.manual_seed(16)
    conv = torch.nn.Conv2d(1, 16, 7, stride=2, padding=3)
    with torch.no_grad():
        conv.bias.copy_(torch.randn(16) * 0.5 + torch.tensor([0.7, -0.4]).repeat(8))       # even and odd entries differ
    g = torch.Generator().manual_seed(17)
    x, g_out = torch.randn(2, 24, 20, generator=g), torch.randn(2, 12, 10, 16, generator=g)
    refs = []
    for dt in (torch.float64, torch.float32):
        xl, w, b = (t.detach().to(dt).clone().requires_grad_(True) for t in (x, conv.weight, conv.bias))
        y = torch.nn.functional.conv2d(xl.unsqueeze(1), w, b, 2, 3).permute(0, 2, 3, 1)
        (y * g_out.to(dt)).sum().backward()
        refs.append(dict(y=y.detach(), g_x=xl.grad, g_w=w.grad, g_b=b.grad))
    conv = conv.to(dev)
    xd = x.to(dev).requires_grad_(True)
    _both_routes(('enc0',), lambda: R_NETWORK._enc0(None, conv, xd), [xd], [conv.weight, conv.bias], g_out.to(dev), *refs,
                 ('g_x', 'g_w', 'g_b'))


def test_dec_last_against_fp64_conv_transpose2d(dev):
    from dcsnet.r_network import R_NETWORK
    torch.manual_seed(32)
    convt = torch.nn.ConvTranspose2d(32, 1, 3, stride=1, padding=1)
    with torch.no_grad():
        convt.bias.fill_(0.3)
    g = torch.Generator().manual_seed(33)
    d, skip = torch.randn(2, 12, 10, 16, generator=g), torch.randn(2, 12, 10, 16, generator=g)
    g_out = torch.randn(2, 24, 20, generator=g)
    refs = []
    for dt in (torch.float64, torch.float32):
        dl, sl, w, b = (t.detach().to(dt).clone().requires_grad_(True) for t in (d, skip, convt.weight, convt.bias))
        y = R64.rconv_forward(dl, sl, w, b, True, (1, 1), (1, 1), (2, 2))[..., 0]
        (y * g_out.to(dt)).sum().backward()
        refs.append(dict(y=y.detach(), g_d=dl.grad, g_skip=sl.grad, g_w=w.grad, g_b=b.grad))
    convt = convt.to(dev)
    dd, sd = d.to(dev).requires_grad_(True), skip.to(dev).requires_grad_(True)
    _both_routes(('dec6',), lambda: R_NETWORK._dec_last(None, convt, dd, sd, (2, 2)), [dd, sd], [convt.weight, convt.bias],
                 g_out.to(dev), *refs, ('g_d', 'g_skip', 'g_w', 'g_b'))
