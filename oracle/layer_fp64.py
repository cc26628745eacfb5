"""ORACLE — TEST INFRASTRUCTURE ONLY. Never imported by the product path.

One layer at a time, in fp64: references, absolute sums and the comparator of tests/test_layers_train_size.py.

The references are this repository's own oracle modules (cpt_oracle / cnet_oracle) widened to complex128 through
``CDTYPE`` and ``.double()`` (what tests/test_full_size.py does for the whole step), differentiated by autograd.  All
tensors here are CPU tensors in the oracle's layout: complex ``[B, C, H, W]``.

The convolution comparator measures, per REAL output element, the distance to fp64 in units of one fp32 rounding of
that element's absolute sum:

    e = max |got - ref64| / (2^-24 * S),     S = sum of |term| over the terms of that element

(forward, real part: |x_r||w_r| + |x_i||w_i| over taps and input channels, + |b_r| + |b_i|; the gradients likewise, of
the cotangent's components).  S is the same convolution / gradient evaluated on absolute values: ``conv_abs_sums``.
The metric is flat over a tensor and does not depend on how much a sum cancels.

``corruptions`` produces the faults the comparator exists for (a dropped tap in one tile, a reduction that misses its
last row, a sign slip in the cross term) by editing the rounded fp64 reference, so their score can be computed on any
machine.
"""
import contextlib
import math
from collections import namedtuple

import torch
from torch.nn import functional as TF

from . import cpt_oracle as cpt
from . import nf_oracle as nf
from . import cnet_oracle as cno

EPS32 = 2.0 ** -24
# Bound: e_hip <= K_BOUND * max(e_cpu32, 1), one number for the whole table.
# An MFMA tile keeps ONE fp32 accumulator per output along K.  A correct evaluation of that kind (`single_chain_e`: random
# products summed in order in one fp32 chain) has rms e 0.47 but a long tail: its maximum over 10^6 .. 4 * 10^6 outputs is
# 5 .. 7 whatever the chain's length (400, 1600, 4608 terms), about 8 at the 1.7 * 10^7 elements of the largest tensors here.
# The CPU oracle's convolutions block the sum over many accumulators and read 0.2 .. 3.7, below one rounding on half the
# layers, so K times ITS error with K = 4 refuses a correct single chain.  K = 16 is twice the single chain's extreme.  The
# smallest fault of `corruptions` scores 163 (dec6's weight gradient at B = 64), the forward / data-gradient ones 4 * 10^5 and
# more.  (Measured margins and where the kernels' worst elements lie: DESIGN.md section 4, profiles/layer_parity.json.)
K_BOUND = 16.0
LOOSE = 4.0                    # elements above this are counted in the records (the issue's starting K)

# name, source map H x W, channels of x1 (previous stage) and x2 (skip), output channels, kernel, stride, upsample, transposed
ConvLayer = namedtuple('ConvLayer', 'name H W C1 C2 Cout k stride up transposed')


def set_threads(cap=16):
    """Cap torch's thread count at `cap` (the share of a GPU machine one command gets) — only ever lowers it, never sizes it by
    the machine's core count.  Returns the previous count for the caller to restore."""
    old = torch.get_num_threads()
    if old > cap:
        torch.set_num_threads(cap)
    return old


@contextlib.contextmanager
def cdtype(cd):
    """complexPyTorch's literal complex64 casts, widened (or not) for the duration."""
    old = (cpt.CDTYPE, nf.CDTYPE)
    cpt.CDTYPE = nf.CDTYPE = cd
    try:
        yield
    finally:
        cpt.CDTYPE, nf.CDTYPE = old


def out_hw(L):
    p = L.k // 2
    return ((L.H * L.up[0] + 2 * p - L.k) // L.stride[0] + 1, (L.W * L.up[1] + 2 * p - L.k) // L.stride[1] + 1)


def randc(g, *shape):
    return torch.complex(torch.randn(*shape, generator=g), torch.randn(*shape, generator=g))


def conv_case(L, B, seed, offset=0j, spread=0.5):
    """Seeded operands of one layer: x = cat(x1, x2) complex [B, Cin, H, W], the two real layers' weights and biases in
    the reference's parameter layout, and a cotangent gy of the output."""
    g = torch.Generator().manual_seed(seed)
    Cin = L.C1 + L.C2
    x = randc(g, B, Cin, L.H, L.W) * spread + offset
    shape = (Cin, L.Cout, L.k, L.k) if L.transposed else (L.Cout, Cin, L.k, L.k)
    s = 1.0 / math.sqrt(Cin * L.k * L.k)
    w_r, w_i = torch.randn(shape, generator=g) * s, torch.randn(shape, generator=g) * s
    b_r, b_i = torch.randn(L.Cout, generator=g) * 0.5, torch.randn(L.Cout, generator=g) * 0.5
    gy = randc(g, B, L.Cout, *out_hw(L))
    return dict(x=x, w_r=w_r, w_i=w_i, b_r=b_r, b_i=b_i, gy=gy)


def conv_module(L, case, wide):
    """The oracle layer of this geometry holding the case's parameters."""
    Cin = L.C1 + L.C2
    if L.transposed:
        m = cpt.ComplexConvTranspose2d(Cin, L.Cout, L.k, 1, L.k // 2)
        a, b = m.conv_tran_r, m.conv_tran_i
    else:
        m = cpt.ComplexConv2d(Cin, L.Cout, L.k, L.stride, L.k // 2)
        a, b = m.conv_r, m.conv_i
    with torch.no_grad():
        a.weight.copy_(case['w_r']); b.weight.copy_(case['w_i'])
        a.bias.copy_(case['b_r']); b.bias.copy_(case['b_i'])
    return (m.double() if wide else m), a, b


def conv_reference(L, case, wide, gy=None, sample=None):
    """Forward and autograd of the oracle layer in fp64 (wide) or fp32: dict(y, gx, gw_r, gw_i, gb_r, gb_i), y and gx complex.
    gy: another cotangent; sample: run one sample of the batch only (slice b:b+1)."""
    cd, rd = (torch.complex128, torch.float64) if wide else (torch.complex64, torch.float32)
    gy = case['gy'] if gy is None else gy
    x = case['x']
    if sample is not None:
        x, gy = x[sample:sample + 1], gy[sample:sample + 1]
    with cdtype(cd):
        m, a, b = conv_module(L, case, wide)
        xr, xi = x.real.to(rd).requires_grad_(True), x.imag.to(rd).requires_grad_(True)
        z = torch.complex(xr, xi)
        if tuple(L.up) != (1, 1):
            z = cpt.complex_upsample(z, scale_factor=tuple(L.up), mode='nearest')
        y = m(z)
        (torch.view_as_real(y) * torch.view_as_real(gy.to(cd))).sum().backward()
    return dict(y=y.detach(), gx=torch.complex(xr.grad, xi.grad), gw_r=a.weight.grad, gw_i=b.weight.grad,
                gb_r=a.bias.grad, gb_i=b.bias.grad)


def _real_conv(L, x, w):
    if tuple(L.up) != (1, 1):
        x = TF.interpolate(x, scale_factor=tuple(float(u) for u in L.up), mode='nearest')
    if L.transposed:
        return TF.conv_transpose2d(x, w, padding=L.k // 2)
    return TF.conv2d(x, w, stride=tuple(L.stride), padding=L.k // 2)


def complex_conv_from_real(L, xr, xi, w_r, w_i, b_r, b_i, sign=-1.0, cross_sign=1.0):
    """(re, im) of the complex layer written as its four real convolutions.  sign = -1, cross_sign = +1: the layer itself
    (apply_complex: two real layers, each with its own bias).  sign = +1 on absolute values: the absolute sums."""
    re = _real_conv(L, xr, w_r) + sign * _real_conv(L, xi, w_i) + (b_r + sign * b_i)[None, :, None, None]
    im = cross_sign * _real_conv(L, xi, w_r) + _real_conv(L, xr, w_i) + (b_r + b_i)[None, :, None, None]
    return re, im


def conv_abs_sums(L, case, gy=None):
    """S of every quantity conv_reference returns, same keys and shapes (y and gx complex: S of the real part, S of the
    imaginary part)."""
    gy = case['gy'] if gy is None else gy
    leaf = lambda t: t.abs().double().requires_grad_(True)
    xr, xi = leaf(case['x'].real), leaf(case['x'].imag)
    w_r, w_i, b_r, b_i = (leaf(case[n]) for n in ('w_r', 'w_i', 'b_r', 'b_i'))
    re, im = complex_conv_from_real(L, xr, xi, w_r, w_i, b_r, b_i, sign=1.0)
    (re * gy.real.abs().double() + im * gy.imag.abs().double()).sum().backward()
    return dict(y=torch.complex(re.detach(), im.detach()), gx=torch.complex(xr.grad, xi.grad), gw_r=w_r.grad, gw_i=w_i.grad,
                gb_r=b_r.grad, gb_i=b_i.grad)


def _real(t):
    return torch.view_as_real(t) if t.is_complex() else t


def ulp_error(got, ref, S):
    """(e, flat index of the worst element) — see the module docstring.  An element without terms must be exact."""
    got, ref, S = _real(got).double(), _real(ref).double(), _real(S).double()
    assert got.shape == ref.shape == S.shape, (got.shape, ref.shape, S.shape)
    d = (got - ref).abs_()
    q = d / (EPS32 * S.clamp_min(1e-300))
    q = torch.where((S <= 0) & (d == 0), torch.zeros_like(q), q)
    e, idx = q.flatten().max(dim=0)
    return float(e), int(idx), int((q > LOOSE).sum())


def single_chain_e(n_terms, n_outputs, seed=0):
    """e of a correct fp32 evaluation that keeps one accumulator per output: n_outputs sums of n_terms products of standard
    normal factors, accumulated in order in fp32 (fused multiply-add) — (max, rms)."""
    g = torch.Generator().manual_seed(seed)
    acc = torch.zeros(n_outputs)
    ref, S = torch.zeros(n_outputs, dtype=torch.float64), torch.zeros(n_outputs, dtype=torch.float64)
    for _ in range(n_terms):
        a, b = torch.randn(n_outputs, generator=g), torch.randn(n_outputs, generator=g)
        t = a.double() * b.double()
        acc = (acc.double() + t).float()
        ref += t
        S += t.abs()
    q = (acc.double() - ref).abs() / (EPS32 * S)
    return float(q.max()), float(q.pow(2).mean().sqrt())


def where(shape, flat_index, complex_):
    """Index tuple of ulp_error's worst element in the original tensor (+ 're' / 'im')."""
    full = tuple(shape) + ((2,) if complex_ else ())
    idx = []
    for n in reversed(full):
        idx.append(flat_index % n)
        flat_index //= n
    idx = idx[::-1]
    return tuple(idx[:-1]) + (('re', 'im')[idx[-1]],) if complex_ else tuple(idx)


QUANTITIES = {'fwd': ('y',), 'dgrad': ('gx',), 'wgrad': ('gw_r', 'gw_i', 'gb_r', 'gb_i')}


def score(got, ref, S, quantity):
    """(e, where, count): e of one quantity (the weight gradient: the worst of its four tensors), the element it sits at, and
    how many elements read above LOOSE."""
    worst, count = (-1.0, None), 0
    for key in QUANTITIES[quantity]:
        e, idx, n = ulp_error(got[key], ref[key], S[key])
        count += n
        if e > worst[0]:
            worst = (e, (key,) + where(ref[key].shape, idx, ref[key].is_complex()))
    return worst + (count,)


def bound(e_cpu32):
    return K_BOUND * max(e_cpu32, 1.0)


def accepts(e, e_cpu32):
    return e <= bound(e_cpu32)


def _tile(n, size=16):
    return slice(max(n - size, 0), n)


def corruptions(L, case, ref):
    """The faults of the comparator tests applied to the fp64 reference rounded to fp32: {name: (quantity, tensors)} where
    tensors has the keys of conv_reference for that quantity.  Each needs one more pass over ONE sample only:

      fwd_tap    the last 16x16 tile of the last output channel of the last sample computed without the centre tap
      dgrad_tap  the same tile of the last input channel's data gradient
      fwd_sign   the cross term of the last output channel with the wrong sign (x_r w_i - x_i w_r) in the last sample
      wgrad_row  the last output row of the last sample left out of the weight- and bias-gradient sums
    """
    B = case['x'].shape[0]
    f32 = lambda t: t.to(torch.complex64 if t.is_complex() else torch.float32)
    out = {}
    c = L.k // 2
    cut = dict(case)
    cut['w_r'], cut['w_i'] = case['w_r'].clone(), case['w_i'].clone()
    cut['w_r'][:, :, c, c] = 0
    cut['w_i'][:, :, c, c] = 0
    bad = conv_reference(L, cut, True, sample=B - 1)
    y = f32(ref['y']).clone()
    hs, ws = _tile(y.shape[2]), _tile(y.shape[3])
    y[B - 1, -1, hs, ws] = f32(bad['y'][0, -1, hs, ws])
    out['fwd_tap'] = ('fwd', dict(y=y))
    gx = f32(ref['gx']).clone()
    hs, ws = _tile(gx.shape[2]), _tile(gx.shape[3])
    gx[B - 1, -1, hs, ws] = f32(bad['gx'][0, -1, hs, ws])
    out['dgrad_tap'] = ('dgrad', dict(gx=gx))
    d = lambda t: t.double()
    x = case['x'][B - 1:B]
    _, im = complex_conv_from_real(L, d(x.real), d(x.imag), d(case['w_r']), d(case['w_i']), d(case['b_r']), d(case['b_i']),
                                   cross_sign=-1.0)
    y = f32(ref['y']).clone()
    y[B - 1, -1] = torch.complex(y[B - 1, -1].real, im[0, -1].float())
    out['fwd_sign'] = ('fwd', dict(y=y))
    row = torch.zeros_like(case['gy'])
    row[B - 1, :, -1, :] = case['gy'][B - 1, :, -1, :]
    part = conv_reference(L, case, True, gy=row, sample=B - 1)
    out['wgrad_row'] = ('wgrad', {k: f32(ref[k] - part[k]) for k in QUANTITIES['wgrad']})
    return out


def corruption_scores(L, case, ref, S):
    """{fault: e} — the figures the bound of every (layer, quantity) has to stay ten times below."""
    return {name: score(t, ref, S, q)[0] for name, (q, t) in corruptions(L, case, ref).items()}


def smallest_corruption(scores, quantity):
    return min(e for name, e in scores.items() if name.startswith(quantity))


def top2_gap(z, b, h, w):
    """Relative gap between the largest and the second largest channel value of z [B,C,H,W] at one pixel, real and imaginary
    part: how close the channel maximum of the spatial attention is to a tie there."""
    out = []
    for part in (z.real, z.imag):
        v = part[b, :, h, w].sort(descending=True).values
        out.append(float((v[0] - v[1]) / part.abs().max()))
    return tuple(out)


TIE = 1e-6        # relative gap below which a channel maximum is undecided in fp32 (a few roundings of the largest |z|)


def undecided(z, thr=TIE):
    """Pixels where the spatial attention's channel maximum of z is a tie to fp32 resolution: [(part, b, h, w, runner-up)]."""
    out = []
    for name, part in (('re', z.real), ('im', z.imag)):
        if part.shape[1] < 2:
            continue
        top = part.topk(2, dim=1)
        gap = (top.values[:, 0] - top.values[:, 1]) / part.abs().max()
        for b, h, w in (gap < thr).nonzero().tolist():
            out.append((name, b, h, w, int(top.indices[b, 1, h, w])))
    return out


def _spatial_with_choice(sa, z, choice):
    """cnet_oracle.ComplexSpatialAttention.forward with the maximising channel at the pixels of `choice` (entries of
    `undecided`) set to the runner-up: the other admissible resolution of a tie."""
    idx = {'re': z.real.argmax(dim=1, keepdim=True), 'im': z.imag.argmax(dim=1, keepdim=True)}
    for part, b, h, w, c in choice:
        idx[part][b, 0, h, w] = c
    mean_c = torch.mean(z, dim=1, keepdim=True)
    max_c = torch.complex(z.real.gather(1, idx['re']), z.imag.gather(1, idx['im']))
    return nf.complex_sigmoid(sa.conv1(torch.cat([mean_c, max_c], dim=1)))


# ---- CBN, attention blocks, LSTM ------------------------------------------------------------------------------------

def rel_max(got, ref):
    """The project's per-op measure: max-abs error relative to the tensor's max-abs."""
    ref = ref.detach()
    assert got.shape == ref.shape and got.is_complex() == ref.is_complex(), (got.shape, ref.shape, got.dtype, ref.dtype)
    got = got.detach().to(ref.dtype)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


_POST = {'none': lambda z: z, 'relu': cpt.complex_relu, 'lrelu': nf.complex_lrelu}
ATT_NAMES = ('fc.0.conv_r.weight', 'fc.0.conv_i.weight', 'fc.2.conv_r.weight', 'fc.2.conv_i.weight',
             'conv1.conv_r.weight', 'conv1.conv_i.weight')


def attention_params(C, seed, ratio=16, k=7):
    """Seeded parameters of one attention block in ATT_NAMES order.  The first FC's real weights lean positive: the pooled
    inputs of these blocks (post-activation maps) have positive parts, and a hidden unit that is negative for every sample
    has identically zero gradients — with C / 16 = 1 or 2 hidden units that happens to whole blocks."""
    g = torch.Generator().manual_seed(seed)
    Ch = max(C // ratio, 1)
    u = lambda *s: (torch.rand(*s, generator=g) - 0.5) * 2.0
    return [(u(Ch, C, 1, 1) + 0.6) * math.sqrt(3.0 / C), u(Ch, C, 1, 1) * 0.3 * math.sqrt(3.0 / C), u(C, Ch, 1, 1) * math.sqrt(3.0 / Ch),
            u(C, Ch, 1, 1) * math.sqrt(3.0 / Ch), u(1, 2, k, k) * 0.25, u(1, 2, k, k) * 0.25]


def _attention_modules(C, params, wide, ratio=16, k=7):
    ca, sa = cno.ComplexChannelAttention(C, ratio), cno.ComplexSpatialAttention(k)
    with torch.no_grad():
        for (n, q), v in zip(list(ca.named_parameters()) + list(sa.named_parameters()), params):
            q.copy_(v)
    return (ca.double(), sa.double()) if wide else (ca, sa)


def _act_with_decisions(z, act, decided, thr=TIE):
    """The activation of z with the reference's OWN branch per element, except where that branch is undecided in fp32:
    |Re z| (|Im z|) within `thr` of the channel's largest magnitude (a few fp32 roundings of the values the sign was taken
    from).  There — a few elements in 10^6 — two correct evaluations fall either way, the gradient on either branch is exact
    for that evaluation, and the branch is read from `decided`, the post-activation tensor of the evaluation under test.
    Returns (activation, number of undecided real elements)."""
    slope = 0.0 if act == 'relu' else 0.01          # nf_oracle.complex_lrelu: torch's default slope
    count = 0

    def f(v, d):
        nonlocal count
        scale = v.detach().abs().amax(dim=(0, 2, 3), keepdim=True)
        undecided_ = v.detach().abs() <= thr * scale
        count += int(undecided_.sum())
        pos = torch.where(undecided_, d > 0, v.detach() > 0).to(v.dtype)
        return v * pos + slope * v * (1 - pos)

    return torch.complex(f(z.real, decided.real), f(z.imag, decided.imag)), count


class _KeepFn(torch.autograd.Function):
    """v * keep_fwd forward, g * keep_bwd backward: a dropout whose backward regenerates its mask (comparator tests hand in
    two different ones: a backward that lost its scale or its seed offset)."""

    @staticmethod
    def forward(ctx, v, keep_fwd, keep_bwd):
        ctx.save_for_backward(keep_bwd)
        return v * keep_fwd

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None


def _apply_keep(a, keep, rd):
    """Complex a [B,C,H,W] times the real mask keep [B,C,H,W,2] (or the pair (forward mask, backward mask))."""
    fwd, bwd = keep if isinstance(keep, (tuple, list)) else (keep, None)
    v = torch.view_as_real(a)
    if tuple(fwd.shape) != tuple(v.shape):
        raise ValueError(f'block_reference: keep has shape {tuple(fwd.shape)}, the output {tuple(v.shape)}')
    v = v * fwd.to(rd) if bwd is None else _KeepFn.apply(v, fwd.to(rd), bwd.to(rd))
    return torch.view_as_complex(v)


def block_reference(x, g_out, wide, bn=None, act='none', attention=None, drop_last=0, decided=None, max_choice=None, keep=None,
                    keep_before_attention=False):
    """One CBN (training mode, fresh running statistics) and / or one attention block on complex64 input x with cotangent
    g_out, in fp64 (wide) or fp32, differentiated by autograd.  bn = (weight [C,3], bias [C,2]); attention = the six
    parameters in ATT_NAMES order.  Returns dict(y, gx[, running_mean, running_covar, g_weight, g_bias][, g_att: list]).

    decided: see _act_with_decisions; max_choice: see _spatial_with_choice.  drop_last = n > 0 (CBN only, comparator tests): the gradients a backward gives whose reduction sums leave out the LAST n
    pixels — every sum over pixels (the two that couple g_x to the batch statistics, and with them the parameter
    gradients) is taken over the cotangent with those pixels zeroed, the per-pixel term keeps the whole cotangent.

    keep: a dropout mask [B,C,H,W,2] of 0 and 1 / (1 - p) (oracle/dropout_mask.keep_nchw) multiplied into the block's output
    where the kernels drop — after the activation of a CBN-only block (cbn_apply_kernel), after the spatial-attention multiply
    of a block with attention (attention_apply_kernel); `y` is the dropped output.  Comparator tests only: keep = (forward
    mask, backward mask), and keep_before_attention = True (the mask between the activation and the attention)."""
    cd, rd = (torch.complex128, torch.float64) if wide else (torch.complex64, torch.float32)
    C = x.shape[1]
    out = {}
    drop_mask = keep                                 # (`keep` below is drop_last's pixel selection)
    with cdtype(cd):
        mod = None
        if bn is not None:
            mod = cpt.ComplexBatchNorm2d(C)
            with torch.no_grad():
                mod.weight.copy_(bn[0]); mod.bias.copy_(bn[1])
            mod = (mod.double() if wide else mod).train()
        ca = sa = None
        if attention is not None:
            ca, sa = _attention_modules(C, attention, wide)

        def run(g, frozen=None):
            xr, xi = x.real.to(rd).requires_grad_(True), x.imag.to(rd).requires_grad_(True)
            a = torch.complex(xr, xi).to(cd)
            if mod is not None:
                for q in mod.parameters():
                    q.grad = None
                if frozen is None:
                    mod.reset_running_stats()
                    mod.train()
                else:                               # the batch statistics as constants: the per-pixel term alone
                    mod.eval()
                    mod.running_mean = frozen[0].clone()
                    mod.running_covar.copy_(frozen[1])
                if decided is None or act == 'none':
                    a = _POST[act](mod(a))
                else:
                    a, out['undecided_activations'] = _act_with_decisions(mod(a), act, decided)
            if drop_mask is not None and keep_before_attention:
                a = _apply_keep(a, drop_mask, rd)
            if ca is not None:
                z = ca(a) * a
                a = (sa(z) if not max_choice else _spatial_with_choice(sa, z, max_choice)) * z
                out['z'] = z.detach()                # what the spatial attention takes its channel maximum of
            if drop_mask is not None and not keep_before_attention:
                a = _apply_keep(a, drop_mask, rd)
            (torch.view_as_real(a) * torch.view_as_real(g.to(cd))).sum().backward()
            return a.detach(), torch.complex(xr.grad, xi.grad)

        y, gx = run(g_out)
        out.update(y=y, gx=gx)
        if mod is not None:
            out.update(running_mean=mod.running_mean.detach().clone(), running_covar=mod.running_covar.detach().clone(),
                       g_weight=mod.weight.grad.clone(), g_bias=mod.bias.grad.clone())
        if ca is not None:
            out['g_att'] = [q.grad.clone() for q in list(ca.parameters()) + list(sa.parameters())]
        if drop_last:
            assert mod is not None and ca is None
            B, _, H, W = x.shape
            keep = torch.ones(B * H * W, dtype=torch.bool)
            keep[-drop_last:] = False
            keep = keep.view(B, 1, H, W)                         # pixel order of the channels-last kernels: b, h, w
            xc = x.to(cd)
            mean = torch.complex(xc.real.mean([0, 2, 3]), xc.imag.mean([0, 2, 3]))
            ce = xc - mean[None, :, None, None]
            cov = torch.stack((ce.real.pow(2).mean([0, 2, 3]), ce.imag.pow(2).mean([0, 2, 3]),
                               (ce.real * ce.imag).mean([0, 2, 3])), dim=1)
            _, g_kept = run(g_out * keep)                        # every term, sums without the dropped pixels
            g_w, g_b = mod.weight.grad.clone(), mod.bias.grad.clone()
            _, g_local = run(g_out * ~keep, frozen=(mean, cov))  # the dropped pixels' own per-pixel term
            out.update(gx=g_kept + g_local, g_weight=g_w, g_bias=g_b)
    return out


def lstm_reference(state, z, g_out, wide):
    """cnet_oracle.ComplexLSTM(128, 64, 2, bidirectional) with the given state_dict on complex64 z [B, S, 128]."""
    m = cno.ComplexLSTM(128, 64, 2, True)
    m.load_state_dict(state)
    cd = torch.complex128 if wide else torch.complex64
    if wide:
        m = m.double()
    zz = z.to(cd).requires_grad_(True)
    y = m(zz)
    (torch.view_as_real(y) * torch.view_as_real(g_out.to(cd))).sum().backward()
    return dict(y=y.detach(), gz=zz.grad, grads={n: q.grad for n, q in m.named_parameters()})


# ---- the folded inference epilogue: conv -> eval-mode CBN -> activation as one kernel (tests/test_infer_epilogue.py) ----

ACT_NAMES = ('none', 'relu', 'lrelu', 'sigmoid')
_POST_EVAL = dict(_POST, sigmoid=nf.complex_sigmoid)
CROSS_MIN = 0.25              # min(|q1|, |q2|) >= CROSS_MIN * max(|q0|, |q3|) in every channel of a non-hard state


def eval_cbn_state(C, seed, hard=False):
    """Seeded eval-mode CBN tensors whose folded coefficients have LARGE cross terms: dict(weight [C,3] = (W_rr, W_ii, W_ri),
    bias [C,2], running_mean float [C,2], running_covar [C,3] = (V_rr, V_ii, V_ri)).

    V_rr, V_ii ~ U[0.5, 2]; V_ri = rho sqrt(V_rr V_ii), rho = s U[0.5, 0.9] with a random sign s per channel (hard: |rho| in
    [0.99, 0.999], a nearly singular covariance); W_rr, W_ii = sqrt(2) + U[-0.3, 0.3]; W_ri = -s U[0.4, 0.9]: the whitening
    matrix's cross term R_ri has the sign of -V_ri, so the weight's cross term adds to it instead of cancelling it.  Mean
    components U[-2, 2], bias U[-0.5, 0.5].  (seeded_state.fill_state has |V_ri|, |W_ri| <= 0.3: q1, q2 a fraction of q0, q3.)"""
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi, *s: torch.rand(*s, generator=g) * (hi - lo) + lo
    vrr, vii = u(0.5, 2.0, C), u(0.5, 2.0, C)
    s = torch.where(torch.rand(C, generator=g) < 0.5, -torch.ones(C), torch.ones(C))
    rho = s * (u(0.99, 0.999, C) if hard else u(0.5, 0.9, C))
    vri = rho * torch.sqrt(vrr * vii)
    weight = torch.stack((math.sqrt(2.0) + u(-0.3, 0.3, C), math.sqrt(2.0) + u(-0.3, 0.3, C), -s * u(0.4, 0.9, C)), dim=1)
    return dict(weight=weight, bias=u(-0.5, 0.5, C, 2), running_mean=u(-2.0, 2.0, C, 2),
                running_covar=torch.stack((vrr, vii, vri), dim=1))


def eval_coef_reference(state, eps=1e-5, wide=True):
    """[C, 6] = (q0, q1, q2, q3, q4, q5) of re' = q0 re + q1 im + q4, im' = q2 re + q3 im + q5: complexPyTorch's eval-mode
    whitening (the closed-form inverse square root of the 2 x 2 covariance) followed by the affine map, evaluated in fp64
    (wide) or fp32."""
    dt = torch.float64 if wide else torch.float32
    w, b, m, v = (state[n].to(dt) for n in ('weight', 'bias', 'running_mean', 'running_covar'))
    crr, cii, cri = v[:, 0] + eps, v[:, 1] + eps, v[:, 2]
    s = torch.sqrt(crr * cii - cri * cri)
    t = torch.sqrt(cii + crr + 2 * s)
    ist = 1.0 / (s * t)
    rrr, rii, rri = (cii + s) * ist, (crr + s) * ist, -cri * ist
    q0, q1 = w[:, 0] * rrr + w[:, 2] * rri, w[:, 0] * rri + w[:, 2] * rii
    q2, q3 = w[:, 2] * rrr + w[:, 1] * rri, w[:, 2] * rri + w[:, 1] * rii
    return torch.stack((q0, q1, q2, q3, b[:, 0] - q0 * m[:, 0] - q1 * m[:, 1], b[:, 1] - q2 * m[:, 0] - q3 * m[:, 1]), dim=1)


def cross_ratio(coef):
    """min over channels of min(|q1|, |q2|) / max(|q0|, |q3|)."""
    q = coef.double().abs()
    return float((torch.minimum(q[:, 1], q[:, 2]) / torch.maximum(q[:, 0], q[:, 3])).min())


def apply_coef(pre, coef, act='none'):
    """act(A pre + c) on a complex [B,C,H,W] tensor with coef [C,6], in coef's real dtype."""
    q = coef[None, :, :, None, None]
    re, im = pre.real.to(coef.dtype), pre.imag.to(coef.dtype)
    z = torch.complex(q[:, :, 0] * re + q[:, :, 1] * im + q[:, :, 4], q[:, :, 2] * re + q[:, :, 3] * im + q[:, :, 5])
    with cdtype(z.dtype):
        return _POST_EVAL[act](z)


def eval_cbn_module(state, eps, wide):
    """cpt.ComplexBatchNorm2d in .eval() holding `state`."""
    C = state['weight'].shape[0]
    mod = cpt.ComplexBatchNorm2d(C, eps=eps)
    with torch.no_grad():
        mod.weight.copy_(state['weight']); mod.bias.copy_(state['bias'])
        mod.running_covar.copy_(state['running_covar'])
    if wide:
        mod = mod.double()
    mod.running_mean = torch.view_as_complex(state['running_mean'].to(torch.float64 if wide else torch.float32).contiguous())
    return mod.eval()


def folded_reference(L, case, state, act, wide, eps=1e-5, pre=None):
    """The oracle's own modules on the case's operands: conv_module -> ComplexBatchNorm2d.eval() holding `state` ->
    complex_relu / complex_lrelu / complex_sigmoid, in fp64 (wide) or fp32.  dict(y, pre): the output and the raw conv
    output the CBN read, complex [B, Cout, Hout, Wout].  pre: the conv output of an earlier call with the same operands and
    width (another activation of the same row)."""
    cd = torch.complex128 if wide else torch.complex64
    with cdtype(cd), torch.no_grad():
        if pre is None:
            m, _, _ = conv_module(L, case, wide)
            z = case['x'].to(cd)
            if tuple(L.up) != (1, 1):
                z = cpt.complex_upsample(z, scale_factor=tuple(L.up), mode='nearest')
            pre = m(z)
        assert pre.dtype == cd
        y = _POST_EVAL[act](eval_cbn_module(state, eps, wide)(pre))
    return dict(y=y, pre=pre)


def live_branches(y, act):
    """(share of real output components on the upper branch of the activation, on the lower one): > 0 / <= 0 after ReLU
    (the clamped ones), > 0 / < 0 after the leaky ReLU, above / below 1/2 after the sigmoid."""
    v = torch.view_as_real(y).double()
    t = 0.5 if act == 'sigmoid' else 0.0
    return float((v > t).double().mean()), float((v <= t).double().mean())


EPILOGUE_FAULTS = ('q1_im_dropped', 'q2_re_dropped', 'q1_q2_swapped', 'additive_dropped', 'neighbour_channel_coef', 'activation_skipped')


def epilogue_faults(y_ref, coef, pre, act='relu', n=16):
    """{fault: y}: the fp64 reference rounded to fp32 with one epilogue fault each in `n` elements of ONE output row (the
    last sample's middle row: all columns and channels of it) — the references the comparator has to refuse.

      q1_im_dropped / q2_re_dropped   the cross term of the real / imaginary part left out
      q1_q2_swapped                   the two cross coefficients exchanged
      additive_dropped                q4, q5 left out
      neighbour_channel_coef          channel c evaluated with channel c ^ 1's coefficients (the pairing of the kernels that
                                      keep two channels per thread)
      activation_skipped              A pre + c stored as it is

    The elements are the first n (in (column, channel) order) of those whose output changes by at least the median of the
    non-zero changes in that row: never one where im ~ 0 or where the ReLU hides the fault."""
    coef = coef.double()
    q = {name: coef.clone() for name in EPILOGUE_FAULTS}
    q['q1_im_dropped'][:, 1] = 0
    q['q2_re_dropped'][:, 2] = 0
    q['q1_q2_swapped'][:, 1], q['q1_q2_swapped'][:, 2] = coef[:, 2], coef[:, 1]
    q['additive_dropped'][:, 4:] = 0
    C = coef.shape[0]
    if C > 1:
        q['neighbour_channel_coef'] = coef[torch.arange(C) ^ 1 if C % 2 == 0 else torch.arange(C).roll(1)]
    else:
        del q['neighbour_channel_coef']            # one channel has no neighbour
    b, h = y_ref.shape[0] - 1, y_ref.shape[2] // 2
    row = pre[b:b + 1, :, h:h + 1].to(torch.complex128)
    good = y_ref[b, :, h].to(torch.complex128)
    out = {}
    for name, qq in q.items():
        if name == 'activation_skipped' and act == 'none':
            continue
        bad = apply_coef(row, qq, 'none' if name == 'activation_skipped' else act)[0, :, 0]        # [C, W]
        change = (bad - good).abs().t()                                                               # [W, C]
        live = change[change > 0]
        assert live.numel() >= n, f'{name}: the fault changes {live.numel()} elements of the row'
        pick = (change >= live.median()).flatten().nonzero().flatten()[:n]
        y = y_ref.to(torch.complex64).clone()
        for i in pick.tolist():
            w_, c_ = divmod(i, C)
            y[b, c_, h, w_] = bad[c_, w_].to(torch.complex64)
        out[name] = y
    return out
