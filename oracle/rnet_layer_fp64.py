"""ORACLE — TEST INFRASTRUCTURE ONLY. Never imported by the product path.

fp64 references of the REAL network's (R_NETWORK: DR-Net / DRS-Net) training kernels, one kernel family at a time, for
tests/test_rnet_kernels.py (GPU) and tests/test_rnet_kernels_cpu.py (host algebra + comparator self-check).

Every reference is a stock torch layer evaluated on the CPU under autograd — conv2d / conv_transpose2d over
interpolate(cat(x1, x2), mode='nearest'), batch_norm (+ ReLU / LeakyReLU), nn.LSTM — in double (`wide=True`) or, as the
yardstick of what a correct fp32 evaluation can reach, in float (`wide=False`).  Activations are channels-last
([B,H,W,Cr]) on both sides of every function here, the layout the kernels use.

Comparison rule (`compare`): per tensor, err = max |got - ref64| / max |ref64| over EVERY element; limit = the project's
per-op tolerance (TOL_FWD = 2e-5 forward, TOL_BWD = 1e-4 gradients; the LSTM 1e-4 + 1e-6 absolute).  Where the stock fp32
CPU layer itself misses that tolerance on a tensor, the tensor is held to K_BOUND (layer_fp64: 16) times the fp32 layer's
error and the row says so.  No limit is ever derived from the result under test.

The `fault_*` functions produce the seeded faults the rule exists for; each edits a correct result, so its score can be
computed anywhere.
"""
import torch
from torch.nn import functional as TF

from .layer_fp64 import K_BOUND, rel_max, set_threads        # noqa: F401  (re-exported for the tests)

TOL_FWD, TOL_BWD = 2e-5, 1e-4
TOL_LSTM, ABS_LSTM = 1e-4, 1e-6
SLOPE = 0.01                                                  # nn.LeakyReLU's default, the kernels' constant
ACT = {'none': lambda t: t, 'relu': torch.relu, 'lrelu': lambda t: TF.leaky_relu(t, SLOPE), 'sigmoid': torch.sigmoid}
FORWARD_KEYS = ('y', 'running_mean', 'running_var')


def _dt(wide):
    return torch.float64 if wide else torch.float32


def _leaf(t, wide):
    return None if t is None else t.detach().to(_dt(wide)).clone().requires_grad_(True)


# ---- comparator -------------------------------------------------------------------------------------------------------

def compare(got, ref, ref32, tol_fwd=TOL_FWD, tol_bwd=TOL_BWD, abs_tol=0.0, zero_ok=()):
    """{tensor: figures}, [misses]: every tensor of `ref` (None entries: `got` must hold None too) under the module's rule.
    zero_ok: tensors whose reference is identically zero BY CONSTRUCTION (the recurrent weights' gradient of a one-step
    sequence); the result then has to be zero to within abs_tol.  Any other all-zero reference is a dead case and an error."""
    rows, misses = {}, []
    for key, r in ref.items():
        if r is None:
            assert got[key] is None, f'{key}: expected no tensor'
            continue
        g, r32 = got[key], ref32[key]
        assert g is not None, f'{key}: missing'
        scale = float(r.abs().max())
        assert bool(torch.isfinite(g).all()), f'{key}: non-finite values'
        if scale == 0 and key in zero_ok:
            assert g.shape == r.shape
            rows[key] = dict(err=float(g.abs().max()), cpu32=float(r32.abs().max()), limit=abs_tol, limit_is='absolute: zero reference',
                             fallback=False)
            if not rows[key]['err'] <= abs_tol:
                misses.append((key, rows[key]))
            continue
        assert scale > 0, f'{key}: the reference is identically zero (a dead case checks nothing)'
        tol = (tol_fwd if key in FORWARD_KEYS else tol_bwd) + abs_tol / scale
        e, e32 = rel_max(g, r), rel_max(r32, r)
        row = dict(err=e, cpu32=e32, limit=tol, limit_is='tolerance', fallback=False)
        if e32 > tol:
            row.update(limit=K_BOUND * e32, limit_is=f'{K_BOUND:g} x cpu32 (the fp32 CPU layer misses the tolerance)', fallback=True)
        rows[key] = row
        if not e <= row['limit']:
            misses.append((key, row))
    return rows, misses


def score(got, ref, ref32, key, **kw):
    """(err, limit) of one tensor under `compare`."""
    rows, _ = compare({key: got}, {key: ref}, {key: ref32}, **kw)
    return rows[key]['err'], rows[key]['limit']


# ---- real conv ----------------------------------------------------------------------------------------------------------

def rconv_case(B, H, W, c1, c2, cout, k, transposed, seed, bias=True):
    """Seeded operands of one real conv as R_NETWORK holds them: x1 (x2) channels-last, the module's weight ([Cout,Cin,k,k],
    or [Cin,Cout,k,k] when transposed), bias."""
    g = torch.Generator().manual_seed(seed)
    cin = c1 + c2
    x1 = torch.randn(B, H, W, c1, generator=g)
    x2 = torch.randn(B, H, W, c2, generator=g) if c2 else None
    shape = (cin, cout, k, k) if transposed else (cout, cin, k, k)
    w = torch.randn(shape, generator=g) / (cin * k * k) ** 0.5
    b = torch.randn(cout, generator=g) if bias else None
    return dict(x1=x1, x2=x2, w=w, b=b, seed=seed)


def rconv_forward(x1, x2, w, b, transposed, stride, pad, up, act='none'):
    """The stock layer on channels-last operands of any float dtype: act(conv(upsample(cat(x1, x2)))) -> [B,Ho,Wo,Cout]."""
    x = x1 if x2 is None else torch.cat([x1, x2], dim=-1)
    x = x.permute(0, 3, 1, 2)
    if tuple(up) != (1, 1):
        x = TF.interpolate(x, scale_factor=tuple(float(u) for u in up), mode='nearest')
    y = TF.conv_transpose2d(x, w, b, 1, pad) if transposed else TF.conv2d(x, w, b, stride, pad)
    return ACT[act](y).permute(0, 2, 3, 1)


def rconv_reference(case, transposed, stride, pad, up, gy, wide):
    """y, g_x1, g_x2, g_w, g_b of the conv over the case's operands for the cotangent gy (None where there is no such
    operand)."""
    x1, x2, w, b = (_leaf(case[n], wide) for n in ('x1', 'x2', 'w', 'b'))
    y = rconv_forward(x1, x2, w, b, transposed, stride, pad, up)
    (y * gy.to(_dt(wide))).sum().backward()
    g = lambda t: None if t is None else t.grad
    return dict(y=y.detach(), g_x1=g(x1), g_x2=g(x2), g_w=g(w), g_b=g(b))


def rconv_out_shape(case, transposed, stride, pad, up):
    B, H, W, _ = case['x1'].shape
    k = case['w'].shape[2]
    cout = case['w'].shape[1] if transposed else case['w'].shape[0]
    if transposed:
        return B, H * up[0] + k - 1 - 2 * pad[0], W * up[1] + k - 1 - 2 * pad[1], cout
    return B, (H * up[0] + 2 * pad[0] - k) // stride[0] + 1, (W * up[1] + 2 * pad[1] - k) // stride[1] + 1, cout


def upsample_cat_bwd_reference(gxv, H, W, c1, c2, up):
    """fp64 block sum over the upsample and channel split: [B,H*uf,W*ut,c1+c2] -> ([B,H,W,c1], [B,H,W,c2] | None)."""
    B = gxv.shape[0]
    s = gxv.double().view(B, H, up[0], W, up[1], c1 + c2).sum(dim=(2, 4))
    return s[..., :c1].contiguous(), (s[..., c1:].contiguous() if c2 else None)


# ---- real BatchNorm -----------------------------------------------------------------------------------------------------

def bn_input(shape, Cr, seed, rho=0.9):
    """[.., Cr] (or [B,F,T] for Cr == 1) with a mean and a spread of its own per real channel, the mean several times the
    spread, and each even channel correlated (rho) with its odd neighbour — a kernel that whitens the (even, odd) pair
    jointly, or that loses the spread to the offset, is off by far more than any tolerance here."""
    g = torch.Generator().manual_seed(seed)
    if Cr == 1:
        return torch.randn(shape, generator=g) * 0.6 + 2.5
    z = torch.randn(*shape, Cr, generator=g)
    z[..., 1::2] = rho * z[..., 0::2] + (1.0 - rho * rho) ** 0.5 * z[..., 1::2]
    spread = 0.3 + torch.rand(Cr, generator=g) * 1.2
    sign = torch.where(torch.rand(Cr, generator=g) < 0.5, -1.0, 1.0)
    mean = sign * spread * (3.0 + 3.0 * torch.rand(Cr, generator=g))          # 3 .. 6 spreads off zero
    return z * spread + mean


def bn_params(Cr, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(Cr, generator=g) * 0.3 + 1.2, torch.randn(Cr, generator=g) * 0.5,
            torch.randn(Cr, generator=g) * 0.5, torch.rand(Cr, generator=g) + 0.5)       # weight, bias, running mean / var


def bn_pre_activation_margin(x, weight, bias, rm, rv, eps, use_batch):
    """Smallest |pre-activation| of the fp64 layer relative to its channel's largest: the ReLU / leaky-ReLU branch of every
    element is decided when this is above 1e-6."""
    xn = _channels_first(x.double())
    d = lambda t: None if t is None else t.double()
    z = TF.batch_norm(xn, d(rm).clone(), d(rv).clone(), d(weight), d(bias), use_batch, 0.0, eps)
    dims = [i for i in range(z.dim()) if i != 1]
    return float((z.abs() / z.abs().amax(dim=dims, keepdim=True)).min())


def _channels_first(x):
    return x.unsqueeze(1) if x.dim() == 3 else x.permute(0, 3, 1, 2)


def _channels_last(y, dim):
    return y.squeeze(1) if dim == 3 else y.permute(0, 2, 3, 1)


def bn_reference(x, weight, bias, rm, rv, eps, momentum, use_batch, act, g_out, wide, calls=1):
    """torch.nn.functional.batch_norm (+ activation) under autograd, `calls` consecutive times on the same input with the
    running statistics carried along (momentum None: the cumulative average, factor 1 / call number, as nn.BatchNorm2d
    applies it).  Outputs of the LAST call; running statistics after it."""
    dt = _dt(wide)
    rm, rv = rm.to(dt).clone(), rv.to(dt).clone()
    for n in range(1, calls + 1):
        xl, wl, bl = _leaf(x, wide), _leaf(weight, wide), _leaf(bias, wide)
        f = (1.0 / n if momentum is None else momentum) if use_batch else 0.0
        y = _channels_last(ACT[act](TF.batch_norm(_channels_first(xl), rm, rv, wl, bl, use_batch, f, eps)), x.dim())
    (y * g_out.to(dt)).sum().backward()
    g = lambda t: None if t is None else t.grad
    return dict(y=y.detach(), g_x=xl.grad, g_weight=g(wl), g_bias=g(bl), running_mean=rm, running_var=rv)


# ---- LSTM ---------------------------------------------------------------------------------------------------------------

def lstm_module(hidden, seed, layers=2):
    torch.manual_seed(seed)
    return torch.nn.LSTM(2 * hidden, hidden, layers, bidirectional=True, batch_first=True)


def lstm_reference(state, hidden, x, g_out, wide, layers=2):
    """nn.LSTM(2H, H, layers, bidirectional, batch_first) with `state` on x [B,S,2H]: y, g_x and every parameter's gradient."""
    m = torch.nn.LSTM(2 * hidden, hidden, layers, bidirectional=True, batch_first=True)
    m.load_state_dict(state)
    m = m.to(_dt(wide))
    xl = _leaf(x, wide)
    y = m(xl)[0]
    (y * g_out.to(_dt(wide))).sum().backward()
    out = dict(y=y.detach(), g_x=xl.grad)
    out.update({n: q.grad for n, q in m.named_parameters()})
    return out


def lstm_first_layer_preactivations(state, x):
    """|x W_ih^T + b| of layer 0 (both directions) in fp64: what the gates see before the recurrent term."""
    x = x.double()
    pre = [x @ state[f'weight_ih_l0{s}'].double().t() + state[f'bias_ih_l0{s}'].double() + state[f'bias_hh_l0{s}'].double()
           for s in ('', '_reverse')]
    return torch.cat(pre, dim=-1).abs()


# ---- seeded faults ------------------------------------------------------------------------------------------------------

def fault_dgrad_last_row(g_x):
    """The data gradient with its last input row left at zero (a border row's taps dropped)."""
    bad = g_x.clone()
    bad[:, -1] = 0
    return bad


def fault_wgrad_swapped_block(g_corr, block=0):
    """One 16 x 16 channel block of the correlation-layout weight gradient with D_ir and D_ri exchanged."""
    bad = g_corr.clone()
    o = slice(16 * block, 16 * block + 16)
    sub, src = bad[o, :16], g_corr[o, :16]
    sub[1::2, 0::2] = src[0::2, 1::2]
    sub[0::2, 1::2] = src[1::2, 0::2]
    return bad


def fault_bias_sign(g_b):
    """gb[0::2] = 0.5 (ab_r + ab_i), gb[1::2] = 0.5 (ab_r - ab_i): the pair's two sums exchanged."""
    bad = g_b.clone()
    bad[0::2], bad[1::2] = g_b[1::2], g_b[0::2]
    return bad


def fault_bn_pair_statistics(x, weight, bias, eps, act='none'):
    """Train-mode BatchNorm output in which channel 2c is normalised with channel 2c+1's batch statistics and vice versa."""
    xd = x.double()
    dims = tuple(range(x.dim() - 1))
    mean, var = xd.mean(dim=dims), xd.var(dim=dims, unbiased=False)
    swap = torch.arange(x.shape[-1]).view(-1, 2).flip(1).reshape(-1)
    y = (xd - mean[swap]) / (var[swap] + eps).sqrt() * weight.double() + bias.double()
    return ACT[act](y)


def _lstm_by_hand(state, hidden, x, reverse_reads_previous=False, reread_first=False, layers=2):
    """The bidirectional LSTM written out step by step in fp64 (i, f, g, o gate order), with the two recurrence faults:
    the reverse direction consuming the FORWARD neighbour's hidden state (h_{t-1} of its own chain laid out in time, i.e.
    it runs in the forward direction), or every chain reading its step-0 operands again at its second step."""
    inp = x.double()
    B, S, _ = inp.shape
    for layer in range(layers):
        outs = []
        for d, sfx in enumerate(('', '_reverse')):
            p = lambda n: state[f'{n}_l{layer}{sfx}'].double()
            gx = inp @ p('weight_ih').t() + p('bias_ih') + p('bias_hh')
            order = list(range(S)) if (d == 0 or reverse_reads_previous) else list(range(S - 1, -1, -1))
            h, c = torch.zeros(B, hidden, dtype=torch.float64), torch.zeros(B, hidden, dtype=torch.float64)
            out = torch.zeros(B, S, hidden, dtype=torch.float64)
            for n, t in enumerate(order):
                src = order[0] if (reread_first and n == 1) else t
                i, f, g, o = (gx[:, src] + h @ p('weight_hh').t()).chunk(4, dim=-1)
                c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
                h = torch.sigmoid(o) * torch.tanh(c)
                out[:, t] = h
            outs.append(out)
        inp = torch.cat(outs, dim=-1)
    return inp


def lstm_by_hand(state, hidden, x, **faults):
    return _lstm_by_hand(state, hidden, x, **faults)


# ---- the BatchNorm case table (shared by the GPU test and the CPU check of its seeds) ------------------------------------

BN_CHANNELS = (16, 32, 256, 512)
BN_SHAPE = (3, 7, 5)              # P = 105: no multiple of the kernels' rows per pass 256 / (Cr / 4) = 64, 32, 4, 2
BN_SMALL = (16, (1, 1, 3))        # P = 3: below a single pass of 64 rows
BN_ONE_CHANNEL = {'p_mod4_0': (2, 6, 5), 'p_mod4_2': (1, 3, 6)}
BN_EPS = 1e-5
# Seeds for which no pre-activation of the fp64 layer lies within 1e-6 of zero (relative to its channel's largest value), so
# every ReLU / leaky-ReLU branch is decided; found by counting up from 0, asserted by the tests on the reference itself.
_BN_SEED_BUMP = {(512, (3, 7, 5), True): 1}


def bn_seed(Cr, shape, use_batch):
    return 1000 + 3 * Cr + 7 * len(shape) * shape[-1] + (0 if use_batch else 500) + 100000 * _BN_SEED_BUMP.get((Cr, tuple(shape), bool(use_batch)), 0)


def bn_case(Cr, shape, use_batch):
    """x, (weight, bias, running_mean, running_var), cotangent of one BatchNorm case."""
    seed = bn_seed(Cr, shape, use_batch)
    x = bn_input(shape, Cr, seed)
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(seed + 1))
    return x, bn_params(Cr, seed + 2), g
