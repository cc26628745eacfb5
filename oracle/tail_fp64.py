"""ORACLE — TEST INFRASTRUCTURE ONLY. Never imported by the product path.

fp64 references of the configured ('dcs') train step's TAIL — everything between the network's raw output D_raw and the total
loss, and the way back to g_D (csrc/mask.hip, csrc/synth.hip, csrc/fft512.hip) — and of the fused optimizer (csrc/adam.hip),
for tests/test_tail_fp64.py (GPU) and tests/test_tail_fp64_cpu.py (host algebra + comparator self-check).

References: the functions of oracle/nf_oracle.py (bound_cRM, mask_apply_subtract, _polar + mag_phase_2_wave, si_snr and the
loss assembly of dcs_train_losses) evaluated on complex128 / float64 CPU tensors under autograd (`wide=True`).  The same
functions in fp32 (`wide=False`; on the CPU in the self-checks, on the device in the GPU tests) are the yardstick of what a
correct fp32 evaluation reaches.  This torch's atan2 / abs backward are finite (zero) at the origin, the convention of the
kernels' unit_dir_bwd, so the references need no exclusions.

Comparison rule (`judge`): per tensor, err = max |got - ref64| / max |ref64| over EVERY element (a complex tensor counts as
its (re, im) floats); limit = max(4 x yardstick_err, FLOOR).  4x: both routes are a handful of fp32 roundings per element,
while an omission is O(1e-2) or more.  FLOOR = 2e-6: this project's bound for fft512.hip against torch.fft, the rule
tests/test_rstep_fused.py was merged with.  No limit is ever derived from the result under test, and an identically zero
reference is an error: a dead case checks nothing.  On a planted input set a gradient is judged twice, over the planted and
over the unplanted elements with their own max-abs scales: one near-singular plant (-eps + 1e-9j) carries |g_D| ~ 184 against
~ 3 elsewhere, and one scale over both would hide every other element.

The `fault_*` functions and AdamRef(fault=...) produce the seeded faults the rule exists for; each edits a correct result or
re-evaluates the fp64 chain with one term wrong, so its score can be computed anywhere.
"""
import math

import numpy as np
import torch
from torch.nn import functional as TF

from . import nf_oracle as nf
from .layer_fp64 import set_threads        # noqa: F401  (re-exported for the tests)

EPS = float(np.float32(10e-7))             # hparams['atan2_eps'] as the fp32 kernels and torch's fp32 add see it
SNR_EPS = 1e-8
ALPHA = 0.7
N_FFT = 512
FLOOR = 2e-6
K_YARD = 4.0

D_PLANTS = (0j, complex(-EPS, 0.0), 1e-7 - 1e-7j, -2 + 0j, 50 - 70j, 1e-3 + 1e-3j, complex(-EPS, 1e-9))
Y_PLANTS = (0j, complex(-EPS, 0.0), 1e-7 - 1e-7j, -2 + 0j)


def f32(x):
    """A hyper-parameter as the fp32 value a kernel receives."""
    return float(np.float32(x))


# ---- inputs -----------------------------------------------------------------------------------------------------------

def inputs(B, F, T, planted, seed=0):
    """(Y, D, where): complex64 [B, F, T] seeded Gaussians, |Y| ~ 0.8, |D| ~ 1.5 (means).  planted: every Y plant meets every
    D plant in bin rows 0..3 of the first item's first frames and rows F-4..F-1 of the last item's last frames; `where` marks
    those elements (None on the regular set)."""
    g = torch.Generator().manual_seed(100003 * seed + 1009 * B + 31 * T + F)

    def c(mean_abs):
        return torch.complex(torch.randn(B, F, T, generator=g), torch.randn(B, F, T, generator=g)) * (mean_abs / math.sqrt(math.pi / 2))
    Y, D = c(0.8), c(1.5)
    if not planted:
        return Y, D, None
    yp, dp = torch.tensor(Y_PLANTS, dtype=torch.complex64), torch.tensor(D_PLANTS, dtype=torch.complex64)
    n = len(dp)
    assert F >= 2 * len(yp) and T >= n
    where = torch.zeros(B, F, T, dtype=torch.bool)
    for j, v in enumerate(yp):
        for b, f, sl in ((0, j, slice(0, n)), (B - 1, F - len(yp) + j, slice(T - n, T))):
            Y[b, f, sl], D[b, f, sl], where[b, f, sl] = v, dp, True
    return Y, D, where


def randn(shape, seed, scale=1.0, cplx=False):
    g = torch.Generator().manual_seed(seed)
    if cplx:
        return torch.complex(torch.randn(shape, generator=g), torch.randn(shape, generator=g)) * scale
    return torch.randn(shape, generator=g) * scale


SNR_ROWS = ('0dB', 'zero_target', '40dB', 'scaled', '20dB', '40dB')


def sisnr_rows(B, L, seed=0, first=0, level=None):
    """(target, estimate) float32 [B, L]; row b is of kind SNR_ROWS[(first + b) % 6]: the estimate at about 0 / 40 / 20 dB of its target,
    a 20 dB row with both signals scaled by 1e-3, and a row whose target is all zeros (-80 dB, zero gradient).  Six kinds, 40 dB
    twice: over 0, -80, 40, 20, 20 dB alone the batch mean is about zero, and a mean of zero is a dead reference.
    The noise of a row is made orthogonal to its target and given the target's norm before it is scaled, so the row sits at its
    stated level at every length (independent draws leave a 3-sample row anywhere within 15 dB of it).  The '0dB' row sits at
    1 dB: at 0 dB exactly the one-row case's snr is a dead reference.  first: the kind of row 0, so that a case of two or three
    rows can be given the kinds its first rows leave out.  level: every row at that many dB instead (the high-SNR cases)."""
    g = torch.Generator().manual_seed(7919 * seed + 13 * B + L)
    c = 0.3 * torch.randn(B, L, generator=g)
    n = 0.3 * torch.randn(B, L, generator=g)
    e = torch.empty_like(c)
    for b in range(B):
        kind = SNR_ROWS[(first + b) % len(SNR_ROWS)] if level is None else 'level'
        db = {'0dB': 1.0, '40dB': 40.0, 'level': level}.get(kind, 20.0)
        cd, nd = c[b].double(), n[b].double()
        nd = nd - cd * (nd @ cd) / (cd @ cd)
        nd = nd * (cd.norm() / nd.norm())
        e[b] = (cd + nd * 10.0 ** (-db / 20.0)).float()
        if kind == 'scaled':
            c[b] *= 1e-3
            e[b] *= 1e-3
        if kind == 'zero_target':
            c[b] = 0.0
    return c, e


# ---- evaluation -------------------------------------------------------------------------------------------------------

def cast(t, wide, device='cpu'):
    if not torch.is_tensor(t):
        return t
    if t.is_complex():
        return t.detach().to(device=device, dtype=torch.complex128 if wide else torch.complex64)
    if t.is_floating_point():
        return t.detach().to(device=device, dtype=torch.float64 if wide else torch.float32)
    return t.detach().to(device)


def rdot(a, b):
    """Real inner product; a complex pair counts as its (re, im) floats, so d/d(leaf) is (d/d re, d/d im) as the kernels store it."""
    if torch.is_tensor(a) and a.is_complex():
        return (torch.view_as_real(a) * torch.view_as_real(b)).sum()
    return (a * b).sum()


def evaluate(fn, leaves, consts, cots, wide, device='cpu'):
    """fn(**leaves, **consts) -> {name: tensor or None}.  Returns the outputs (detached) and, with cotangents `cots`
    ({output name: tensor}), 'g_<leaf>' for every leaf: the gradient of sum_k <out_k, cot_k>."""
    lv = {k: cast(v, wide, device).requires_grad_(True) for k, v in leaves.items()}
    outs = fn(**lv, **{k: cast(v, wide, device) for k, v in consts.items()})
    res = {k: v.detach() for k, v in outs.items() if v is not None}
    if cots:
        loss = sum(rdot(outs[k], cast(c, wide, device)) for k, c in cots.items())
        for k, g in zip(lv, torch.autograd.grad(loss, list(lv.values()), allow_unused=True)):
            res['g_' + k] = g
    return res


# ---- the reference chain (dtype and device follow the arguments) ----------------------------------------------------------

def bound(M, eps=EPS):
    return nf.bound_cRM(M, {'atan2_eps': eps})


def drop(D, keep):
    """keep: float [..., 2] per (re, im) float, 0 or 1 / (1 - p) — what F.dropout makes of a tensor of ones."""
    return D if keep is None else torch.complex(D.real * keep[..., 0], D.imag * keep[..., 1])


def mask_apply(Y, M_in, pre=False, keep=None, eps2=EPS):
    """{M1, M, N, S}: M = bound(M_in) — or, pre, bound(M1) with M1 = bound(dropout(M_in)) — N = Y (.) M, S = Y - N.
    eps2: the eps of the last bound (a seeded fault drops it)."""
    M1 = bound(drop(M_in, keep)) if pre else None
    M = bound(M1 if pre else M_in, eps2)
    N = nf.complex_mat_mult(Y, M)
    return {'M1': M1, 'M': M, 'N': N, 'S': Y - N}


def polar(z):
    mag, ph = nf._polar(z, EPS)
    return torch.complex(mag * torch.cos(ph), mag * torch.sin(ph))


def polar_frames(z, pad=1):
    """mag_phase_2_wave's spectrum (zero bins appended), frame-major [B, T, F + pad]."""
    return TF.pad(polar(z), (0, 0, 0, pad)).transpose(1, 2)


def wave(z, hop, window):
    return nf.mag_phase_2_wave(*nf._polar(z, EPS), N_FFT, hop, window)


def ola(frames, window, hop, scale=1.0):
    """torch.istft's window / overlap-add / envelope / centre trim over real frames [B, T, n_fft], written out (differentiable
    with respect to the frames): ola(irfft(X, norm='forward'), w, hop, 1 / n_fft) == torch.istft(X) (tests/test_tail_fp64_cpu.py)."""
    B, T, n_fft = frames.shape
    full = hop * (T - 1) + n_fft

    def fold(x):
        return TF.fold(x.transpose(1, 2), (1, full), (1, n_fft), stride=(1, hop)).reshape(x.shape[0], full)
    y = fold(frames * window)
    env = fold((window * window).expand(1, T, n_fft))
    lo = n_fft // 2
    return scale * y[:, lo:lo + hop * (T - 1)] / env[:, lo:lo + hop * (T - 1)]


def envelope(window, T, hop):
    """1 / (squared-window overlap-add envelope) of torch.istft(center=True), trimmed: [hop (T - 1)]."""
    n_fft = window.numel()
    env = torch.zeros(hop * (T - 1) + n_fft, dtype=window.dtype, device=window.device)
    for f in range(T):
        env[f * hop:f * hop + n_fft] += window * window
    return 1.0 / env[n_fft // 2:n_fft // 2 + hop * (T - 1)]


def snr_rows(clean, est):
    """si_snr per utterance [B] (nf.si_snr is their mean)."""
    return torch.stack([nf.si_snr(clean[b:b + 1], est[b:b + 1], SNR_EPS) for b in range(est.shape[0])])


def losses(target, est, alpha=ALPHA):
    """dcs_train_losses' assembly on stacked signals (rows [0, B) noise, [B, 2B) speech): [noise_loss, speech_loss, total]."""
    B = est.shape[0] // 2
    noise_loss = 1 - alpha * (-nf.si_snr(target[:B], est[:B], SNR_EPS))
    speech_loss = alpha * (-nf.si_snr(target[B:], est[B:], SNR_EPS))
    return torch.stack([noise_loss, speech_loss, noise_loss + speech_loss])


def wave_written(z, hop, window):
    """wave() by another route: torch.fft.irfft of the frame-major spectrum and the written-out overlap-add, not torch.istft."""
    frames = torch.fft.irfft(polar_frames(z), n=N_FFT, dim=-1, norm='forward')
    return ola(frames, window, hop, math.sqrt(N_FFT) / N_FFT)


def losses_written(target, est, alpha=ALPHA):
    """losses() by another route: the kernels' sums (sisnr_closed's forward), not nf.si_snr."""
    B = est.shape[0] // 2
    snr = sisnr_closed(target, est)[0]
    noise_loss, speech_loss = 1 + alpha * snr[:B].mean(), -alpha * snr[B:].mean()
    return torch.stack([noise_loss, speech_loss, noise_loss + speech_loss])


def node(Y, D, window, hop, keep=None, eps2=EPS, s_sign=1.0, written=False):
    """D_raw -> {M, wave [2B, L]}: both bounds, multiply, subtract, mag_phase_2_wave of both estimates.  written: the synthesis
    by wave_written (a second evaluation whose roundings and summation order are its own)."""
    r = mask_apply(Y, D, pre=True, keep=keep, eps2=eps2)
    wv = wave_written if written else wave
    return {'M': r['M'], 'wave': torch.cat([wv(r['N'], hop, window), wv(s_sign * r['S'], hop, window)])}


def tail(Y, D, target, window, hop, keep=None, written=False):
    r = node(Y, D, window, hop, keep, written=written)
    return {'losses': (losses_written if written else losses)(target, r['wave']), 'wave': r['wave']}


def herm_weights(Fp, skip_row=None, dc=False):
    """The one-sided cotangent's weights: 2 on bins 0 < f < Fp - 1 (skip_row / dc: the seeded faults)."""
    w = torch.full((Fp,), 2.0)
    w[0], w[Fp - 1] = (2.0 if dc else 1.0), 1.0
    if skip_row is not None:
        w[skip_row] = 1.0
    return w


# ---- the closed forms the kernels use (mask.hip / synth.hip), dtype-generic -------------------------------------------------

def _inv(h):
    z = h == 0
    return torch.where(z, torch.zeros_like(h), 1 / torch.where(z, torch.ones_like(h), h))


def unit_dir(x, y):
    h = torch.hypot(x, y)
    z, ih = h == 0, _inv(h)
    return torch.where(z, torch.ones_like(x), x * ih), torch.where(z, torch.zeros_like(y), y * ih)


def unit_dir_bwd(x, y, gx, gy):
    """(g - u (u.g)) / |v|; zero where |v|^2 is below the smallest normal number of the type (the kernels: |v| < 2^-63), the
    point at which the denominator x^2 + y^2 of atan2's backward is lost."""
    h = torch.hypot(x, y)
    ih = _inv(torch.where(h * h < torch.finfo(h.dtype).tiny, torch.zeros_like(h), h))
    ux, uy = x * ih, y * ih
    d = ux * gx + uy * gy
    return (gx - ux * d) * ih, (gy - uy * d) * ih


def bound_one(mr, mi, eps=EPS):
    m = torch.tanh(torch.hypot(mr, mi))
    d1 = unit_dir(mr + eps, mi)
    d2 = unit_dir(m * d1[0] + eps, m * d1[1])
    return m * d2[0], m * d2[1]


def bound_one_bwd(mr, mi, gx, gy, eps=EPS):
    r = torch.hypot(mr, mi)
    m = torch.tanh(r)
    d1 = unit_dir(mr + eps, mi)
    v2x, v2y = m * d1[0] + eps, m * d1[1]
    d2 = unit_dir(v2x, v2y)
    gv2 = unit_dir_bwd(v2x, v2y, m * gx, m * gy)
    gm = gx * d2[0] + gy * d2[1] + gv2[0] * d1[0] + gv2[1] * d1[1]
    gv1 = unit_dir_bwd(mr + eps, mi, m * gv2[0], m * gv2[1])
    gr, ir = gm * (1 - m * m), _inv(r)
    return gv1[0] + gr * mr * ir, gv1[1] + gr * mi * ir


def polar_turn(zx, zy, eps=EPS):
    m, d = torch.hypot(zx, zy), unit_dir(zx + eps, zy)
    return m * d[0], m * d[1]


def polar_turn_bwd(zx, zy, gx, gy, eps=EPS):
    m, d = torch.hypot(zx, zy), unit_dir(zx + eps, zy)
    dot = d[0] * gx + d[1] * gy
    o = unit_dir_bwd(zx + eps, zy, m * gx, m * gy)
    im = _inv(m)
    return o[0] + dot * zx * im, o[1] + dot * zy * im


def sisnr_closed(c, e, eps=SNR_EPS, drop_tail=0, drop_a_term=False):
    """(snr [B], g [B, L] = d sum_b snr_b / d e) by the kernels' k1 c + k2 e form.  drop_tail: the last samples left out of
    every sum; drop_a_term: k1 without its a * on_r part (the seeded faults)."""
    cs, es = (c[:, :c.shape[1] - drop_tail], e[:, :e.shape[1] - drop_tail]) if drop_tail else (c, e)
    Dd, E = (es * cs).sum(-1), (cs * cs).sum(-1)
    a = Dd / (E + eps)
    tv = a[:, None] * cs
    rv = es - tv
    T, R, RC = (tv * tv).sum(-1), (rv * rv).sum(-1), (rv * cs).sum(-1)
    q = T / (R + eps)
    K, ie, ir = 10 / (math.log(10.0) * (q + eps)), 1 / (E + eps), 1 / (R + eps)
    on_c = K * (2 * a * E * ie * ir + 2 * T * RC * ie * ir * ir)
    on_r = -K * 2 * T * ir * ir
    k1 = on_c if drop_a_term else on_c - a * on_r
    return 10 * torch.log10(q + eps), k1[:, None] * c + on_r[:, None] * e


def sisnr_form_allowance(c, e, row_scale=None):
    """The stated cost of the kernels' k1 c + k2 e form, relative to max |g_ref|: the gradient is the small term k2 (e - a c) (plus
    on_c c) written as the sum of two products that cancel to 10^(-dB/20) of their size, and four fp32 roundings of that size
    reach it unreduced — k1 as stored, the product a * on_r inside it, and the products k1 c_n and k2 e_n (a fused multiply-add
    saves one; the bound does not count on it).  Each is at most 2^-24 of |k2 e_n| (|k1 c_n| equals it to 10^(-dB/20)), so the
    allowance is 4 x 2^-24 x max_n |s_b k2_b e_bn| / max |g_ref|, about 4 x 2^-24 x 10^(dB/20): 2.4e-5 at 40 dB, 2.4e-4 at 60 dB.
    Everything in it comes from the fp64 reference.  row_scale [B]: the factor s_b the loss assembly gives row b."""
    c, e = c.double(), e.double()
    E, Dd = (c * c).sum(-1), (e * c).sum(-1)
    a = Dd / (E + SNR_EPS)
    r = e - a[:, None] * c
    T, R = (a * a * E), (r * r).sum(-1)
    q = T / (R + SNR_EPS)
    k2 = -(10 / (math.log(10.0) * (q + SNR_EPS))) * 2 * T / (R + SNR_EPS) ** 2
    s = torch.ones_like(k2) if row_scale is None else row_scale.double()
    g = sisnr_closed(c, e)[1] * s[:, None]
    return 4 * 2.0 ** -24 * float(((s * k2)[:, None] * e).abs().max()) / float(g.abs().max())


# ---- comparator -------------------------------------------------------------------------------------------------------

def _flat(t, where=None):
    t = t.detach().cpu()
    t = torch.view_as_real(t.to(torch.complex128).contiguous()) if t.is_complex() else t.double()
    return t if where is None else t[where]


def score(x, ref, where=None):
    """max |x - ref| / max |ref| over the elements `where` selects (all of them by default)."""
    x, r = _flat(x, where), _flat(ref, where)
    assert x.shape == r.shape, (tuple(x.shape), tuple(r.shape))
    assert bool(torch.isfinite(x).all()), 'non-finite values'
    assert bool(torch.isfinite(r).all()), 'non-finite reference'
    scale = float(r.abs().max()) if r.numel() else 0.0
    assert scale > 0, 'the reference is identically zero (a dead case checks nothing)'
    return float((x - r).abs().max()) / scale


def limit_of(yard_err, floor=FLOOR):
    assert math.isfinite(yard_err), 'the yardstick is not finite'
    return max(K_YARD * yard_err, floor)


def plant_classes(where, Y=None):
    """{row tag: element mask} of a planted input set.  With Y, the plants with Y = -eps stand apart: there S_r + eps keeps one
    or two significant bits in fp32 (S = Y - Y M), so every fp32 evaluation sits 1e-3 ... 1e-1 from fp64, and a scale and a
    yardstick shared with them would hide every other plant."""
    if where is None or isinstance(where, dict):
        return where
    if Y is None:
        return {'[unplanted]': ~where, '[planted]': where}
    hard = where & (Y.detach().cpu().to(torch.complex64) == torch.tensor(Y_PLANTS[1], dtype=torch.complex64))
    assert bool(hard.any()) and bool((where & ~hard).any())
    return {'[unplanted]': ~where, '[planted]': where & ~hard, '[planted Y=-eps]': hard}


def judge(got, ref, yard, where=None, twice=(), floors=None):
    """({row: {err, yardstick, limit}}, [misses]) for every tensor of `ref`.  got / yard: dicts of the result under test and of
    the parent's fp32 evaluation, or `yard` a dict of its already computed scores (floats).  Tensors named in `twice` are judged
    over the planted (`where`) and the unplanted elements separately when `where` is given (a mask, or plant_classes' dict).  floors: {tensor: floor} in place of
    FLOOR (the Adam update's stated allowance)."""
    rows, misses = {}, []
    for key, r in ref.items():
        parts = [('', None)]
        if where is not None and key in twice:
            parts = list(plant_classes(where).items())
        for tag, sel in parts:
            y = yard.get(key + tag, yard.get(key))
            y_err = score(y, r, sel) if torch.is_tensor(y) else float(y)
            row = dict(err=score(got[key], r, sel), yardstick=y_err, limit=limit_of(y_err, (floors or {}).get(key, FLOOR)))
            rows[key + tag] = row
            if not row['err'] <= row['limit']:
                misses.append((key + tag, row))
    return rows, misses


def yard_scores(yard, ref, where=None, twice=()):
    """The yardstick's own scores, in judge's row names: computed once per case and shared."""
    out = {}
    for key, r in ref.items():
        if where is not None and key in twice:
            for tag, sel in plant_classes(where).items():
                out[key + tag] = score(yard[key], r, sel)
            out[key] = max(out[key + tag] for tag in plant_classes(where))
        else:
            out[key] = score(yard[key], r)
    return out


# ---- seeded faults on results -----------------------------------------------------------------------------------------

def fault_tile(spec, t0, f0):
    """One 32 x 32 tile of a frame-major [B, T, Fp] tensor written back untransposed: element (t0 + i, f0 + j) takes the value of
    (t0 + j, f0 + i) wherever both lie inside the tensor — what a tile[ty][tx] / tile[tx][ty] mix-up does at a ragged edge."""
    out = spec.clone()
    T, Fp = spec.shape[1:3]
    for i in range(min(32, T - t0)):
        for j in range(min(32, Fp - f0)):
            if t0 + j < T and f0 + i < Fp:
                out[:, t0 + i, f0 + j] = spec[:, t0 + j, f0 + i]
    return out


def fault_swap_rows(w):
    B = w.shape[0] // 2
    return torch.cat([w[B:], w[:B]])


# ---- Adam / AMSGrad -----------------------------------------------------------------------------------------------------

ADAM_FAULTS = ('bias_from_calls', 'clip_after_wd', 'no_world', 'no_vmax')


class AdamRef:
    """The fused optimizer step written out in fp64 (adam.hip's header; torch.optim.Adam(amsgrad=True) after clip_grad_norm_):
        g = g_sum / world ;  g *= min(1, max_norm / (||g|| + 1e-6)) ;  g += wd p
        m = b1 m + (1 - b1) g ;  v = b2 v + (1 - b2) g^2 ;  vmax = max(vmax, v)
        p -= lr / (1 - b1^t) m / (sqrt(vmax) / sqrt(1 - b2^t) + eps),   t = the count of updates (a skipped call is none)
    Every hyper-parameter is the fp32 value the kernel receives: 1 - beta2 alone differs by 1.3e-5 otherwise."""

    def __init__(self, p, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=0.0, fault=None, dtype=torch.float64):
        assert fault is None or fault in ADAM_FAULTS
        self.dtype = dtype                                  # float32: a second fp32 evaluation, independent of torch.optim's
        self.p = p.detach().to(dtype).cpu().clone()
        self.m, self.v, self.vmax = (torch.zeros_like(self.p) for _ in range(3))
        self.lr, self.b1, self.b2, self.eps, self.wd, self.max_norm = (f32(x) for x in (lr, betas[0], betas[1], eps, weight_decay, max_norm))
        self.t = self.calls = 0
        self.fault = fault

    def step(self, g_sum, world=1, skip=False):
        self.calls += 1
        if skip:
            return
        self.t += 1
        t = self.calls if self.fault == 'bias_from_calls' else self.t
        g = g_sum.detach().to(self.dtype).cpu() * (1.0 if self.fault == 'no_world' else f32(1.0 / world))
        clip = min(1.0, self.max_norm / (float(g.norm()) + f32(1e-6))) if self.max_norm > 0 else 1.0
        g = (g + self.wd * self.p) * clip if self.fault == 'clip_after_wd' else g * clip + self.wd * self.p
        self.m = self.b1 * self.m + (1 - self.b1) * g
        self.v = self.b2 * self.v + (1 - self.b2) * g * g
        self.vmax = self.v.clone() if self.fault == 'no_vmax' else torch.maximum(self.vmax, self.v)
        bc1, bc2 = 1 - self.b1 ** t, 1 - self.b2 ** t
        self.p = self.p - (self.lr / bc1) * self.m / (self.vmax.sqrt() / math.sqrt(bc2) + self.eps)

    def state(self):
        return {'p': self.p, 'm': self.m, 'v': self.v, 'vmax': self.vmax}


def torch_adam_states(p0, grads, world, kw, dtype, device='cpu'):
    """The parent: torch.optim.Adam(amsgrad=True) after clip_grad_norm_ on one parameter, hyper-parameters as their fp32
    values; the states after every step."""
    p = torch.nn.Parameter(p0.detach().to(device=device, dtype=dtype).clone())
    opt = torch.optim.Adam([p], lr=f32(kw['lr']), betas=tuple(f32(b) for b in kw['betas']), eps=f32(kw['eps']),
                           weight_decay=f32(kw['weight_decay']), amsgrad=True)
    out = []
    for g in grads:
        p.grad = g.detach().to(device=device, dtype=dtype) / world
        torch.nn.utils.clip_grad_norm_([p], f32(kw['max_norm']))
        opt.step()
        s = opt.state[p]
        out.append({'p': p.detach().clone(), 'm': s['exp_avg'].clone(), 'v': s['exp_avg_sq'].clone(), 'vmax': s['max_exp_avg_sq'].clone()})
    return out


def adam_dp_floor(t, beta2, p_max, dp_max):
    """The stated allowance of the update dp = p_after - p_before relative to max |dp_ref|: powf's OpenCL bound of 16 ulp on
    beta2^t, halved by the square root, over 1 - beta2^t; plus the rounding of p (4 x 2^-24 max|p|) on the update's scale."""
    u = 2.0 ** -24
    return 16 * u / (2 * (1 - f32(beta2) ** t)) + 4 * u * p_max / dp_max
