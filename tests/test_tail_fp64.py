"""GPU: the configured ('dcs') train step's tail — csrc/mask.hip, csrc/synth.hip, csrc/fft512.hip between the network's raw output
D_raw and the total loss, and the way back to g_D — and the fused optimizer (csrc/adam.hip), element by element against fp64.

References, inputs (a regular and a planted set) and the rule are oracle/tail_fp64.py's: per tensor err = max |got - ref64| /
max |ref64| over every element, limit = max(4 x yardstick, 2e-6), where the yardstick is the parent's chain — the nf_oracle
functions (torch.optim.Adam + clip_grad_norm_ for the optimizer) run in fp32 ON THE DEVICE — measured against the same fp64
result; on the planted set g_D is judged over the planted and the unplanted elements separately, and in the fused node and the
tail the plants with Y = -eps (ill-conditioned in fp32) apart from the other plants.  The Adam update dp has its stated
allowance (tl.adam_dp_floor: powf's 16 ulp on beta2^t and the rounding of p), and so has the SI-SNR gradient on rows at 60 dB
(tl.sisnr_form_allowance: the cancellation in k1 c + k2 e).  tests/test_tail_fp64_cpu.py holds the
rule against the seeded faults.  Every figure goes to $DCS_PARITY_DIR/tail_parity.json (default parity_out/, kept out of git);
a full run's file is committed as profiles/tail_parity.json.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tail_fp64 as tl            # noqa: E402
from _ragged_helpers import record            # noqa: E402

F_BINS = 256
SCALE = 512 ** 0.5                              # torch.istft(normalized=True) at n_fft = 512
DROPS = ((0.0, 0), (0.3, 4242))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from dcsnet import _lib
    _lib.load()
    old = tl.set_threads()
    yield torch.device('cuda:0')
    torch.set_num_threads(old)


_record = functools.partial(record, 'tail_parity.json')     # figures -> $DCS_PARITY_DIR/tail_parity.json (default parity_out/)


def _judge(path, got, ref, yard, **kw):
    """Record and print every figure, then return the misses."""
    rows, misses = tl.judge(got, ref, yard, **kw)
    _record(path, rows)
    print('/'.join(path), {k: f"{r['err']:.2e} (yardstick {r['yardstick']:.2e}, limit {r['limit']:.2e})" for k, r in rows.items()})
    return [(path, m) for m in misses]


def _keep(shape, drop, dev):
    """The keep mask of F.dropout for (p, seed), per (re, im) float: 0 or 1 / (1 - p); the kept share within 5 sigma of 1 - p."""
    from dcsnet import functional as F
    p, seed = drop
    if p == 0.0:
        return None
    keep = F.dropout(torch.ones(tuple(shape) + (2,), device=dev), p, seed).cpu()
    kept = keep != 0
    assert bool(((keep == 0) | (keep == tl.f32(1.0 / (1.0 - tl.f32(p))))).all())
    assert abs(float(kept.double().mean()) - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / keep.numel())
    return keep


def _drop_tag(drop):
    return 'nodrop' if drop[0] == 0.0 else f'drop{drop[0]:g}'


# ------------------------------------------------------------------------------------------------------ 1. element-wise masks

MASK_SHAPES = {'n1027': (1, 13, 79), 'b3_f256_t40': (3, F_BINS, 40)}
_ALL = [('M',), ('N',), ('S',), ('N', 'S'), ('M', 'N', 'S')]
_PAIR = [('M',), ('N', 'S'), ('M', 'N', 'S')]


def _hip_mask(entry, Y, D, drop):
    from dcsnet import functional as F
    if entry == 'bound_crm':
        return {'M': F.bound_crm_complex(D)}
    if entry == 'bound_mask_apply':
        return dict(zip('MNS', F.bound_mask_apply_complex(Y, D)))
    if entry == 'bound_mask_apply_pair':
        M, NS = F.bound_mask_apply_pair_complex(Y, D)
    else:
        M, NS = F.bound2_mask_apply_pair_complex(Y, D, drop=drop)
    return {'M': M, 'N': NS[0], 'S': NS[1]}


MASK_ENTRIES = {'bound_crm': (False, [('M',)]), 'bound_mask_apply': (False, _ALL), 'bound_mask_apply_pair': (False, _PAIR),
                'bound2_mask_apply_pair': (True, _PAIR)}
MASK_CASES = [(e, DROPS[0]) for e in MASK_ENTRIES] + [('bound2_mask_apply_pair', DROPS[1])]


def _mask_inputs(shape, flat, dev, drop):
    Y, D, where = tl.inputs(*shape, True)
    keep = _keep(shape, drop, dev)
    cots = {k: tl.randn(shape, 20 + i, cplx=True) for i, k in enumerate(('M1', 'M', 'N', 'S'))}
    if flat:                                                # n = 1027 elements: a ragged tail of the grid-stride loop
        Y, D, where = Y.reshape(-1), D.reshape(-1), where.reshape(-1)
        keep = None if keep is None else keep.reshape(-1, 2)
        cots = {k: v.reshape(-1) for k, v in cots.items()}
    return Y, D, where, keep, cots


@pytest.mark.parametrize('shape', list(MASK_SHAPES))
@pytest.mark.parametrize('entry,drop', MASK_CASES, ids=[f'{e}-{_drop_tag(d)}' for e, d in MASK_CASES])
def test_masks_forward_and_every_cotangent_combination(dev, entry, drop, shape):
    pre, combos = MASK_ENTRIES[entry]
    Y, D, where, keep, cots = _mask_inputs(MASK_SHAPES[shape], shape == 'n1027', dev, drop)
    outs = combos[-1]
    consts = {'Y': Y} if keep is None else {'Y': Y, 'keep': keep}
    ref_fn = lambda D, Y, keep=None: {k: tl.mask_apply(Y, D, pre=pre, keep=keep)[k] for k in outs}       # noqa: E731
    hip_fn = lambda D, Y, keep=None: _hip_mask(entry, Y, D, drop)                                         # noqa: E731
    misses = []
    for combo in combos:
        c = {k: cots[k] for k in combo}
        ref = tl.evaluate(ref_fn, {'D': D}, consts, c, True)
        yard = tl.evaluate(ref_fn, {'D': D}, consts, c, False, dev)
        got = tl.evaluate(hip_fn, {'D': D}, consts, c, False, dev)
        assert got['g_D'].shape == D.shape and got['g_D'].dtype == torch.complex64
        if combo is not combos[-1]:                          # the forward tensors once, with the last combination
            ref = {'g_D': ref['g_D']}
        misses += _judge(('masks', f'{entry}-{_drop_tag(drop)}', shape, 'g' + '+'.join(combo)), got, ref, yard, where=where, twice=('g_D',))
    assert not misses, misses


@pytest.mark.parametrize('shape', list(MASK_SHAPES))
def test_double_bound_inference_form_and_its_backward_with_gM1(dev, shape):
    """F.bound2_mask_apply_complex (no autograd), the once-bounded mask of ops.bound2_mask_apply(keep_m1) and
    ops.bound2_mask_apply_bwd with every cotangent combination it accepts, gM1 among them."""
    from dcsnet import ops, functional as F
    Y, D, where, _, cots = _mask_inputs(MASK_SHAPES[shape], shape == 'n1027', dev, DROPS[0])
    ref_fn = lambda D, Y: tl.mask_apply(Y, D, pre=True)                                                   # noqa: E731
    Yd, Dd = Y.to(dev), D.to(dev)
    yr, dr = torch.view_as_real(Yd), torch.view_as_real(Dd)
    fwd = dict(zip('MNS', F.bound2_mask_apply_complex(Yd, Dd)))
    M1, M, N, S = ops.bound2_mask_apply(yr, dr, 10e-7, keep_m1=True)
    fwd['M1'] = torch.view_as_complex(M1)
    assert torch.equal(torch.view_as_complex(M), fwd['M']) and torch.equal(torch.view_as_complex(S), fwd['S'])
    misses = []
    combos = [('M1',), ('M',), ('N',), ('S',), ('N', 'S'), ('M1', 'M', 'N', 'S')]
    for combo in combos:
        c = {k: cots[k] for k in combo}
        ref = tl.evaluate(ref_fn, {'D': D}, {'Y': Y}, c, True)
        yard = tl.evaluate(ref_fn, {'D': D}, {'Y': Y}, c, False, dev)
        g = [None if k not in c else torch.view_as_real(c[k].to(dev)).contiguous() for k in ('M1', 'M', 'N', 'S')]
        got = dict(fwd, g_D=torch.view_as_complex(ops.bound2_mask_apply_bwd(yr, dr, *g)))
        if combo is not combos[-1]:
            ref = {'g_D': ref['g_D']}
        misses += _judge(('masks', 'bound2_mask_apply', shape, 'g' + '+'.join(combo)), got, ref, yard, where=where, twice=('g_D',))
    assert not misses, misses


def test_masks_forward_where_the_grid_stride_loop_wraps(dev):
    """n = 2048 * 1024 + 1027 elements: ew_grid's cap of 2048 workgroups of 256 threads, four elements a thread, is passed and the
    last trip is ragged.  Forward only, every entry point."""
    from dcsnet import functional as F
    n = 2048 * 1024 + 1027
    Y, D, _ = tl.inputs(1, 1, n, False)
    Y, D = Y.reshape(-1), D.reshape(-1)
    keep = _keep((n,), DROPS[1], dev)
    Yd, Dd = Y.to(dev), D.to(dev)
    misses = []
    for pre, kp in ((False, None), (True, None), (True, keep)):
        consts = {'D': D, 'Y': Y} if kp is None else {'D': D, 'Y': Y, 'keep': kp}
        fn = lambda D, Y, keep=None: tl.mask_apply(Y, D, pre=pre, keep=keep)                              # noqa: E731
        ref, yard = tl.evaluate(fn, {}, consts, None, True), tl.evaluate(fn, {}, consts, None, False, dev)
        if not pre:
            got = dict(zip('MNS', F.bound_mask_apply_complex(Yd, Dd)))
            M, NS = F.bound_mask_apply_pair_complex(Yd, Dd)
            assert torch.equal(F.bound_crm_complex(Dd), got['M']) and torch.equal(M, got['M'])
            assert torch.equal(NS[0], got['N']) and torch.equal(NS[1], got['S'])
        else:
            drop = DROPS[0] if kp is None else DROPS[1]
            M, NS = F.bound2_mask_apply_pair_complex(Yd, Dd, drop=drop)
            got = {'M': M, 'N': NS[0], 'S': NS[1]}
            if kp is None:
                assert all(torch.equal(a, got[k]) for k, a in zip('MNS', F.bound2_mask_apply_complex(Yd, Dd)))
            ref.pop('M1'), yard.pop('M1')
        misses += _judge(('masks', 'wrap', f'pre{int(pre)}_{"nodrop" if kp is None else "drop0.3"}'), got, ref, yard)
    assert not misses, misses


# ------------------------------------------------------------------------------------------------------------ 2. polar frames

@pytest.mark.parametrize('B,F,T', [(2, 70, 45), (1, 256, 8)])
def test_polar_frames_forward_and_backward(dev, B, F, T):
    """F.polar_frames_complex under autograd, and ops.polar_frames' backward with the Hermitian x2 on and off: the reference
    doubles the rows 0 < f < Fp - 1 itself."""
    from dcsnet import ops, functional as Fn
    z, where = tl.inputs(B, F, T, True)[1:]
    G = tl.randn((B, T, F + 1), 31, cplx=True)
    misses = []
    for herm in (False, True):
        wts = tl.herm_weights(F + 1) if herm else torch.ones(F + 1)
        ref_fn = lambda z, wts: {'spec': tl.polar_frames(z), 'w': tl.polar_frames(z) * wts}              # noqa: E731
        ref = tl.evaluate(ref_fn, {'z': z}, {'wts': wts}, {'w': G}, True)
        yard = tl.evaluate(ref_fn, {'z': z}, {'wts': wts}, {'w': G}, False, dev)
        ref.pop('w'), yard.pop('w')
        zd = z.to(dev)
        if herm:
            spec = ops.polar_frames(torch.view_as_real(zd), F + 1)
            gz = ops.polar_frames(torch.view_as_real(zd), F + 1, grad=torch.view_as_real(G.to(dev)).contiguous(), hermitian=True)
            got = {'spec': torch.view_as_complex(spec), 'g_z': torch.view_as_complex(gz)}
        else:
            got = tl.evaluate(lambda z: {'spec': Fn.polar_frames_complex(z)}, {'z': z}, {}, {'spec': G}, False, dev)
        assert got['spec'].shape == (B, T, F + 1) and not bool(torch.view_as_real(got['spec'][:, :, F:]).any())
        misses += _judge(('polar_frames', f'B{B}_F{F}_T{T}', 'hermitian' if herm else 'plain'), got, ref, yard, where=where, twice=('g_z',))
    assert not misses, misses


# --------------------------------------------------------------------------------------------------------------- 3. synthesis

def _spectra(B, T, seed):
    X = tl.randn((B, T, 257), seed, cplx=True)
    X[..., 0], X[..., 256] = X[..., 0].real + 0j, X[..., 256].real + 0j     # a real signal's DC and Nyquist bins
    return X


@pytest.mark.parametrize('B,T,hop', [(3, 40, 128), (1, 2, 128), (2, 33, 64), (2, 19, 32), (1, 14, 256)])
def test_synthesis_against_torch_istft_and_fft_in_double(dev, B, T, hop):
    from dcsnet import ops, functional as F
    L = hop * (T - 1)
    tag = f'B{B}_T{T}_hop{hop}'
    w = torch.hann_window(512)
    wd, w64 = w.to(dev), w.double()
    misses = []
    # the envelope
    inv_env = ops.istft_envelope(wd, T, hop)
    misses += _judge(('synthesis', tag, 'envelope'), {'inv_env': inv_env}, {'inv_env': tl.envelope(w64, T, hop)}, {'inv_env': tl.envelope(wd, T, hop)})
    # the 512-point pair
    X = _spectra(B, T, 50 + T)
    Xd = X.to(dev)
    Xr = torch.view_as_real(Xd).contiguous()
    fr = tl.randn((B, T, 512), 60 + T)
    ref = {'irfft': torch.fft.irfft(X.to(torch.complex128), n=512, dim=-1, norm='forward'), 'rfft': torch.fft.rfft(fr.double(), dim=-1)}
    yard = {'irfft': torch.fft.irfft(Xd, n=512, dim=-1, norm='forward'), 'rfft': torch.fft.rfft(fr.to(dev), dim=-1)}
    got = {'irfft': ops.irfft512(Xr), 'rfft': torch.view_as_complex(ops.rfft512(fr.to(dev)))}
    misses += _judge(('synthesis', tag, 'fft512'), got, ref, yard)
    # window, overlap-add, envelope, trim: forward and grad=
    gy = tl.randn((B, L), 70 + T)
    frames = ref['irfft'].float()
    ola_fn = lambda frames, window: {'y': tl.ola(frames, window, hop, 1.0 / 512)}                        # noqa: E731
    ref_o = tl.evaluate(ola_fn, {'frames': frames}, {'window': w}, {'y': gy}, True)
    want = torch.istft(torch.fft.rfft(frames.double(), dim=-1, norm='forward').transpose(1, 2), n_fft=512, hop_length=hop, win_length=512,
                       window=w64)
    assert tl.score(ref_o['y'], want) <= 1e-12                                 # the written-out reference is torch.istft
    yard_o = tl.evaluate(ola_fn, {'frames': frames}, {'window': w}, {'y': gy}, False, dev)
    got_o = tl.evaluate(lambda frames, window: {'y': F.istft_ola(frames, window, inv_env, hop, 1.0 / 512)},
                        {'frames': frames}, {'window': w}, {'y': gy}, False, dev)
    misses += _judge(('synthesis', tag, 'istft_ola'), got_o, ref_o, yard_o)
    # the same two without the frames in HBM
    ref_f = {'G': torch.fft.rfft(ref_o['g_frames'], dim=-1)}
    yard_f = {'G': torch.fft.rfft(yard_o['g_frames'], dim=-1)}
    got_f = {'G': torch.view_as_complex(ops.rfft512_ola(gy.to(dev), wd, inv_env, T, hop, 1.0 / 512))}
    if ops.irfft512_ola_ok(T, hop):
        ref_f['y'] = torch.istft(X.to(torch.complex128).transpose(1, 2), n_fft=512, hop_length=hop, win_length=512, window=w64)
        yard_f['y'] = torch.istft(Xd.transpose(1, 2), n_fft=512, hop_length=hop, win_length=512, window=wd)
        got_f['y'] = ops.irfft512_ola(Xr, wd, inv_env, hop, 1.0 / 512)
    else:
        assert hop == 32
    misses += _judge(('synthesis', tag, 'fused_with_fft512'), got_f, ref_f, yard_f)
    # F.polar_wave: mag_phase_2_wave of a spectrum, forward and backward
    z, where = tl.inputs(B, F_BINS, T, T >= 7)[1:]
    wave_fn = lambda z, window: {'wave': tl.wave(z, hop, window)}                                        # noqa: E731
    ref_w = tl.evaluate(wave_fn, {'z': z}, {'window': w}, {'wave': gy}, True)
    yard_w = tl.evaluate(wave_fn, {'z': z}, {'window': w}, {'wave': gy}, False, dev)
    got_w = tl.evaluate(lambda z, window: {'wave': F.polar_wave(z, window, inv_env, 512, hop, SCALE, 10e-7)},
                        {'z': z}, {'window': w}, {'wave': gy}, False, dev)
    misses += _judge(('synthesis', tag, 'polar_wave'), got_w, ref_w, yard_w, where=where, twice=('g_z',))
    assert not misses, misses


def test_scalar_overlap_add_backward(dev):
    """n_fft = 64, hop = 6, T = 9: hop is no multiple of 4, so dcs_istft_ola_bwd takes its one-element-per-thread kernel."""
    from dcsnet import ops, functional as F
    n_fft, hop, T, B = 64, 6, 9, 2
    w = torch.hann_window(n_fft)
    inv_env = ops.istft_envelope(w.to(dev), T, hop)
    frames, gy = tl.randn((B, T, n_fft), 81), tl.randn((B, hop * (T - 1)), 82)
    ola_fn = lambda frames, window: {'y': tl.ola(frames, window, hop, 0.25)}                             # noqa: E731
    ref = tl.evaluate(ola_fn, {'frames': frames}, {'window': w}, {'y': gy}, True)
    yard = tl.evaluate(ola_fn, {'frames': frames}, {'window': w}, {'y': gy}, False, dev)
    got = tl.evaluate(lambda frames, window: {'y': F.istft_ola(frames, window, inv_env, hop, 0.25)},
                      {'frames': frames}, {'window': w}, {'y': gy}, False, dev)
    ref['inv_env'], yard['inv_env'], got['inv_env'] = tl.envelope(w.double(), T, hop), tl.envelope(w.to(dev), T, hop), inv_env
    misses = _judge(('synthesis', f'nfft{n_fft}_hop{hop}_T{T}', 'istft_ola'), got, ref, yard)
    assert not misses, misses


# ---------------------------------------------------------------------------------------------------------- 4. the fused node

NODE_SHAPES = ((3, 40), (2, 72), (1, 8))        # (B, T): ragged 32-tiles in T, several blocks, B = 1
NODE_HOPS = (128, 32)                           # (inverse FFT + overlap-add in one kernel | the configured hop: two kernels)
_node_cases = {}


def _node_case(B, T, hop, drop, dev):
    """Planted inputs, the keep mask, seeded cotangents, the fp64 result of both forms (mask wanted or not) and the parent's device
    chain's scores against it: computed once per (B, T, hop, drop), shared by the parametrised cases and left unchanged."""
    key = (B, T, hop, drop)
    if key not in _node_cases:
        Y, D, where = tl.inputs(B, F_BINS, T, True)
        where = tl.plant_classes(where, Y)                  # g_D in three parts: unplanted, the plants with Y = -eps, the other plants
        keep = _keep((B, F_BINS, T), drop, dev)
        cots = {'wave': tl.randn((2 * B, hop * (T - 1)), 7 + T + hop), 'M': tl.randn(D.shape, 8 + T + hop, cplx=True)}
        consts = {'Y': Y, 'window': torch.hann_window(512)}
        if keep is not None:
            consts['keep'] = keep
        fn = lambda D, Y, window, keep=None: tl.node(Y, D, window, hop, keep)                            # noqa: E731
        ref, yard = {}, {}
        for want_mask in (False, True):
            c = cots if want_mask else {'wave': cots['wave']}
            r = tl.evaluate(fn, {'D': D}, consts, c, True)
            y = tl.evaluate(fn, {'D': D}, consts, c, False, dev)
            if not want_mask:
                r.pop('M'), y.pop('M')
            ref[want_mask], yard[want_mask] = r, tl.yard_scores(y, r, where, ('g_D',))
        _node_cases[key] = (Y, D, where, cots, ref, yard)
    return _node_cases[key]


@pytest.mark.parametrize('want_mask', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('drop', DROPS, ids=[_drop_tag(d) for d in DROPS])
@pytest.mark.parametrize('hop', NODE_HOPS)
@pytest.mark.parametrize('B,T', NODE_SHAPES)
def test_fused_node_against_fp64(dev, B, T, hop, drop, want_mask):
    from dcsnet import ops, functional as F
    Y, D, where, cots, ref, yard = _node_case(B, T, hop, drop, dev)
    wd = torch.hann_window(512).to(dev)
    inv_env = ops.istft_envelope(wd, T, hop)

    def hip(D, Y):
        M, w = F.bound2_apply_polar_wave_pair(Y, D, wd, inv_env, 512, hop, SCALE, 10e-7, drop=drop, want_mask=want_mask)
        assert (M is None) == (not want_mask)
        return {'M': M, 'wave': w}
    c = cots if want_mask else {'wave': cots['wave']}
    got = tl.evaluate(hip, {'D': D}, {'Y': Y}, c, False, dev)
    again = tl.evaluate(hip, {'D': D}, {'Y': Y}, c, False, dev)
    assert all(torch.equal(got[k], again[k]) for k in got)                  # two runs: the same bits
    assert got['wave'].shape == (2 * B, hop * (T - 1)) and got['g_D'].shape == D.shape
    # the raw spectra: frame-major, bins >= F exactly zero (the zero bin mag_phase_2_wave pads), every row written
    M3, spec = ops.bound2_apply_polar_frames(torch.view_as_real(Y.to(dev)), torch.view_as_real(D.to(dev)), F_BINS + 1, 10e-7, drop[0], drop[1],
                                             want_mask)
    assert spec.shape == (2 * B, T, F_BINS + 1, 2) and not spec[:, :, F_BINS:].any() and bool(torch.isfinite(spec).all())
    assert (M3 is None) == (not want_mask)
    tag = f'B{B}_T{T}_hop{hop}_{_drop_tag(drop)}_{"mask" if want_mask else "nomask"}'
    misses = _judge(('node', tag), got, ref[want_mask], yard[want_mask], where=where, twice=('g_D',))
    assert not misses, misses


# ------------------------------------------------------------------------------------------------------------------ 5. SI-SNR

SNR_SHAPES = [(3, 1000), (32, 8160),            # the register kernel
              (3, 1001), (2, 8196), (4, 3),     # the two-pass kernel: L % 4 != 0, L > 8192, L < 4
              (70, 64),                         # the loss assembly's loop beyond 64 rows
              (1, 512)]


@pytest.mark.parametrize('B,L', SNR_SHAPES)
def test_sisnr_rows_gradient_and_losses(dev, B, L):
    from dcsnet import ops, functional as F
    tag = f'B{B}_L{L}'
    c, e = tl.sisnr_rows(B, L)
    # the second signal starts at the third kind (40 dB, scaled, 20 dB, ...): between them the two signals of the two- and three-row
    # cases of the two-pass kernel, (2, 8196) and (3, 1001), hold a 40 dB row and a 20 dB one (the row scaled by 1e-3 is one)
    c2, e2 = tl.sisnr_rows(B, L, seed=1, first=2)
    misses = []
    # per row, and coef through the gradient
    fn = lambda e, c: {'snr': tl.snr_rows(c, e)}                                                         # noqa: E731
    ones = torch.ones(B)
    for name, (cc, ee) in (('rows', (c, e)), ('rows_second', (c2, e2))):
        ref, yard = tl.evaluate(fn, {'e': ee}, {'c': cc}, {'snr': ones}, True), tl.evaluate(fn, {'e': ee}, {'c': cc}, {'snr': ones}, False, dev)
        cd, ed = cc.to(dev), ee.to(dev)
        snr, coef = ops.sisnr(cd, ed, 1e-8)
        got = {'snr': snr, 'g_e': ops.sisnr_bwd(cd, ed, coef, torch.ones(1, device=dev), 1.0)}
        zero = [b for b in range(B) if not bool(cc[b].any())]
        assert zero or name != 'rows' or B == 1
        for b in zero:                                    # -80 dB and a zero gradient
            assert abs(float(ref['snr'][b]) + 80.0) < 1e-6 and not bool(got['g_e'][b].any()) and not bool(ref['g_e'][b].any())
        misses += _judge(('sisnr', tag, name), got, ref, yard)
    # the batch mean
    fn = lambda e, c: {'mean': tl.snr_rows(c, e).mean().reshape(1)}                                      # noqa: E731
    cot = {'mean': torch.full((1,), -0.7)}
    ref, yard = tl.evaluate(fn, {'e': e}, {'c': c}, cot, True), tl.evaluate(fn, {'e': e}, {'c': c}, cot, False, dev)
    got = tl.evaluate(lambda e, c: {'mean': F.sisnr_mean(c, e, 1e-8).reshape(1)}, {'e': e}, {'c': c}, cot, False, dev)
    misses += _judge(('sisnr', tag, 'mean'), got, ref, yard)
    # the loss assembly: four signals, and the stacked pair; every single output picked
    tgt, est = torch.cat([c, c2]), torch.cat([e, e2])      # rows [0, B) noise, [B, 2B) speech
    fn = lambda est, tgt: {'losses': tl.losses(tgt, est)}                                                # noqa: E731
    for pick in (2, 0, 1):                                 # total, noise_loss only, speech_loss only
        cot = {'losses': torch.eye(3)[pick]}
        ref, yard = tl.evaluate(fn, {'est': est}, {'tgt': tgt}, cot, True), tl.evaluate(fn, {'est': est}, {'tgt': tgt}, cot, False, dev)
        got = tl.evaluate(lambda est, tgt: {'losses': torch.stack(F.sisnr_losses(tgt[B:], est[B:], tgt[:B], est[:B], tl.ALPHA))},
                          {'est': est}, {'tgt': tgt}, cot, False, dev)
        misses += _judge(('sisnr', tag, f'losses_pick{pick}'), got, ref, yard)
        skip = torch.full((1,), 7.0, device=dev)
        got = tl.evaluate(lambda est, tgt: {'losses': torch.stack(F.sisnr_losses_pair(tgt, est, tl.ALPHA, skip=skip))},
                          {'est': est}, {'tgt': tgt}, cot, False, dev)
        assert float(skip) == 0.0                          # the guard flag: finite input
        misses += _judge(('sisnr', tag, f'losses_pair_pick{pick}'), got, ref, yard)
    bad = est.clone()
    bad[2 * B - 1, L - 1] = float('nan')                   # one estimate sample
    skip = torch.zeros(1, device=dev)
    F.sisnr_losses_pair(tgt.to(dev), bad.to(dev), tl.ALPHA, skip=skip)
    assert float(skip) == 1.0
    assert not misses, misses


@pytest.mark.parametrize('B,L', [(2, 1000), (2, 1001), (2, 3)])
def test_sisnr_gradient_at_60_db(dev, B, L):
    """Above 40 dB the k1 c + k2 e form of the gradient loses 10^(dB/20) x 2^-24 to the cancellation of its two products.  That
    cost is held to its stated size: on rows at 60 dB the floor of the rule becomes 2e-6 + tl.sisnr_form_allowance (four fp32
    roundings of |k2 e_n|, 2.4e-4 of max |g| at 60 dB, from the fp64 reference alone); 4 x yardstick stands as everywhere.
    Both backward kernels (ops.sisnr_bwd, and the stacked pair's through F.sisnr_losses_pair), behind the register kernel and
    the two-pass one."""
    from dcsnet import ops, functional as F
    tag = f'B{B}_L{L}_60dB'
    c, e = tl.sisnr_rows(B, L, seed=2, level=60.0)
    ref = tl.evaluate(lambda e, c: {'snr': tl.snr_rows(c, e)}, {'e': e}, {'c': c}, {'snr': torch.ones(B)}, True)
    assert float((ref['snr'] - 60.0).abs().max()) < 2.0           # (the SI-SNR eps takes up to a dB off a 3-sample row)
    yard = tl.evaluate(lambda e, c: {'snr': tl.snr_rows(c, e)}, {'e': e}, {'c': c}, {'snr': torch.ones(B)}, False, dev)
    cd, ed = c.to(dev), e.to(dev)
    snr, coef = ops.sisnr(cd, ed, 1e-8)
    got = {'snr': snr, 'g_e': ops.sisnr_bwd(cd, ed, coef, torch.ones(1, device=dev), 1.0)}
    allow = tl.sisnr_form_allowance(c, e)
    assert 1e-4 < allow < 1e-3, allow
    misses = _judge(('sisnr', tag, 'rows'), got, ref, yard, floors={'g_e': tl.FLOOR + allow})
    # the stacked pair: row 0 the noise signal, row 1 the speech signal (B = 1 each), the total picked
    assert B == 2
    fn = lambda est, tgt: {'losses': tl.losses(tgt, est)}                                                # noqa: E731
    cot = {'losses': torch.eye(3)[2]}
    ref, yard = tl.evaluate(fn, {'est': e}, {'tgt': c}, cot, True), tl.evaluate(fn, {'est': e}, {'tgt': c}, cot, False, dev)
    got = tl.evaluate(lambda est, tgt: {'losses': torch.stack(F.sisnr_losses_pair(tgt, est, tl.ALPHA))}, {'est': e}, {'tgt': c}, cot, False, dev)
    allow = tl.sisnr_form_allowance(c, e, row_scale=torch.tensor([tl.ALPHA, -tl.ALPHA]))
    misses += _judge(('sisnr', tag, 'losses_pair_pick2'), got, ref, yard, floors={'g_est': tl.FLOOR + allow})
    assert not misses, misses


# ----------------------------------------------------------------------------------------------------- 6. the tail end to end

@pytest.mark.parametrize('planted', [False, True], ids=['regular', 'planted'])
@pytest.mark.parametrize('B,T,hop', [(2, 40, 32), (1, 8, 128)])
def test_tail_end_to_end(dev, B, T, hop, planted):
    """D_raw -> F.bound2_apply_polar_wave_pair -> F.sisnr_losses_pair against the fp64 chain: the three losses and g_D of the
    total; targets synthesised by F.polar_wave from seeded spectra."""
    from dcsnet import ops, functional as F
    Y, D, where = tl.inputs(B, F_BINS, T, planted)
    where = tl.plant_classes(where, Y)                      # (None on the regular set)
    w = torch.hann_window(512)
    wd = w.to(dev)
    inv_env = ops.istft_envelope(wd, T, hop)
    tn, ts = tl.inputs(B, F_BINS, T, False, seed=1)[:2]
    target = torch.cat([F.polar_wave(t.to(dev), wd, inv_env, 512, hop, SCALE, 10e-7) for t in (tn, ts)]).cpu()
    cot = {'losses': torch.eye(3)[2]}
    consts = {'Y': Y, 'window': w, 'target': target}
    fn = lambda D, Y, window, target: {'losses': tl.tail(Y, D, target, window, hop)['losses']}           # noqa: E731
    ref, yard = tl.evaluate(fn, {'D': D}, consts, cot, True), tl.evaluate(fn, {'D': D}, consts, cot, False, dev)

    def hip(D, Y, window, target):
        _, wv = F.bound2_apply_polar_wave_pair(Y, D, window, inv_env, 512, hop, SCALE, 10e-7)
        return {'losses': torch.stack(F.sisnr_losses_pair(target, wv, tl.ALPHA))}
    got = tl.evaluate(hip, {'D': D}, consts, cot, False, dev)
    misses = _judge(('tail', f'B{B}_T{T}_hop{hop}_{"planted" if planted else "regular"}'), got, ref, yard, where=where, twice=('g_D',))
    assert not misses, misses


# -------------------------------------------------------------------------------------------------------------------- 7. Adam

ADAM_KW = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-3, max_norm=0.5)
# the same as the fp32 values the kernel receives, for the parent (torch.optim.Adam keeps Python doubles: 1 - beta2 alone differs
# by 1.3e-5 between the literal and its fp32 value, and a yardstick built on the literal would measure that)
ADAM_F32 = dict(lr=tl.f32(ADAM_KW['lr']), betas=tuple(tl.f32(b) for b in ADAM_KW['betas']), eps=tl.f32(ADAM_KW['eps']),
                weight_decay=tl.f32(ADAM_KW['weight_decay']), max_norm=tl.f32(ADAM_KW['max_norm']))
N_WRAP = 2048 * 256 * 4 + 4000                  # beyond the Adam grid's 2048 x 256 float4 and grad_sumsq_parts' 512 x 256 x 4 float4


class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.small = torch.nn.Parameter(1e-2 * torch.randn(64, 33, generator=g))
        self.three = torch.nn.Parameter(torch.randn(3, generator=g))
        self.big = torch.nn.Parameter(torch.randn(N_WRAP, generator=g))


def _adam_rows(path, got, ref, yard, prev, t):
    """m, v, vmax, p under the rule; the update dp, in double from the fp32 states, under its stated allowance."""
    got, ref, yard = dict(got), dict(ref), dict(yard)
    for d, pv in ((got, prev['got']), (ref, prev['ref']), (yard, prev['yard'])):
        d['dp'] = d['p'].double().cpu() - pv.double().cpu()
    floors = {'dp': tl.adam_dp_floor(t, ADAM_KW['betas'][1], float(ref['p'].abs().max()), float(ref['dp'].abs().max()))}
    return _judge(path, got, ref, yard, floors=floors)


@pytest.mark.parametrize('world', [1, 4])
def test_fused_adam_states_after_every_step(dev, world):
    """6 steps at the production betas over a bucket of 2.1 M floats (both kernels' loops wrap): gradients alternately unclipped
    and clipped, the skip flag on step 3 (no state changes; step 4 uses update count 3), a new learning rate before step 5."""
    from dcsnet.dp import FlatBucket, FusedAdam, TorchAdam
    m1, m2 = _Toy().to(dev), _Toy().to(dev)
    b1, b2 = FlatBucket(m1), FlatBucket(m2)
    assert b1.numel == 64 * 33 + 4 + N_WRAP and b1.numel > 2048 * 256 * 4
    o1, o2 = FusedAdam(b1, **ADAM_KW), TorchAdam(b2, **ADAM_F32)
    ref = tl.AdamRef(b1.flat, **ADAM_KW)
    gen = torch.Generator().manual_seed(10 + world)
    misses = []

    def torch_state():
        out = {'p': b2.flat.clone()}
        for k, name in (('m', 'exp_avg'), ('v', 'exp_avg_sq'), ('vmax', 'max_exp_avg_sq')):
            out[k] = torch.zeros_like(b2.flat)
            for p, o in zip(b2.params, b2.offsets):
                out[k][o:o + p.numel()] = o2.opt.state[p][name].reshape(-1)
        return out
    prev = {'got': b1.flat.clone(), 'ref': ref.p.clone(), 'yard': b2.flat.clone()}
    for it in range(6):
        if it == 4:
            o1.lr = 5e-3
            o2.opt.param_groups[0]['lr'] = ref.lr = tl.f32(5e-3)
        grad = (torch.randn(b1.numel, generator=gen) * (3.0 if it % 2 else 1e-4)).to(dev)
        for b in (b1, b2):
            b.zero_grad()
            for p, o in zip(b.params, b.offsets):
                p.grad.copy_(grad[o:o + p.numel()].view(p.shape))
        clipped = float(b1.grad.double().norm()) / world > ADAM_KW['max_norm']
        assert clipped == bool(it % 2)
        skip = it == 2
        if skip:
            b1.skip.fill_(1.0), b2.skip.fill_(1.0)
        before = [t.clone() for t in (b1.flat, o1.m, o1.v, o1.vmax, o1.t_dev)]
        g_cpu = b1.grad.cpu()
        o1.step(world), o2.step(world), ref.step(g_cpu, world, skip=skip)
        if skip:                                            # no state may change, and the update count stays
            assert all(torch.equal(a, b) for a, b in zip(before, (b1.flat, o1.m, o1.v, o1.vmax, o1.t_dev)))
            assert int(o1.t_dev) == 2 and o1.t == 3
            continue
        assert int(o1.t_dev) == ref.t == it + (0 if it < 2 else -1) + 1
        got = {'p': b1.flat, 'm': o1.m, 'v': o1.v, 'vmax': o1.vmax}
        yard = torch_state()
        misses += _adam_rows(('adam', f'world{world}', f'step{it + 1}_t{ref.t}'), got, ref.state(), yard, prev, ref.t)
        prev = {'got': b1.flat.clone(), 'ref': ref.p.clone(), 'yard': b2.flat.clone()}
    assert o1.t == 6 and ref.t == 5
    assert not misses, misses


@pytest.mark.parametrize('n', [4 * 300 + 1, 4 * 300 + 2, 4 * 300 + 3, 3])
def test_adam_kernel_tails_through_the_library(dev, n):
    """dcs_adam_amsgrad_step with a device norm at sizes FlatBucket's padding never produces: the n % 4 tail, and n < 4."""
    from dcsnet import _lib
    from dcsnet._lib import check, ptr, cur_stream
    lib, world = _lib.load(), 4
    p0 = tl.randn(n, 90 + n)
    grads = [tl.randn(n, 91 + n, 3.0), tl.randn(n, 92 + n, 1e-2)]                       # clipped, unclipped
    want = tl.torch_adam_states(p0, grads, world, ADAM_KW, torch.float32, dev)
    ref = tl.AdamRef(p0, **ADAM_KW)
    p = p0.to(dev).clone()
    m, v, vmax = (torch.zeros(n, device=dev) for _ in range(3))
    lr = torch.full((1,), ADAM_KW['lr'], device=dev)
    prev = {'got': p.clone(), 'ref': ref.p.clone(), 'yard': p.clone()}
    misses = []
    for it, g in enumerate(grads):
        gd = g.to(dev)
        gn = torch.linalg.vector_norm(gd).reshape(1)
        check(lib.dcs_adam_amsgrad_step(ptr(p), ptr(gd), ptr(m), ptr(v), ptr(vmax), ptr(gn), ADAM_KW['max_norm'], 1.0 / world, n, ptr(lr),
                                        ADAM_KW['betas'][0], ADAM_KW['betas'][1], ADAM_KW['eps'], ADAM_KW['weight_decay'], it + 1,
                                        None, None, cur_stream()), 'dcs_adam_amsgrad_step')
        ref.step(g, world)
        misses += _adam_rows(('adam', 'library', f'n{n}_step{it + 1}'), {'p': p, 'm': m, 'v': v, 'vmax': vmax}, ref.state(), want[it], prev, it + 1)
        prev = {'got': p.clone(), 'ref': ref.p.clone(), 'yard': want[it]['p'].clone()}
    assert not misses, misses


@pytest.mark.parametrize('n', [4 * 300 + 3, N_WRAP, N_WRAP + 3])
def test_grad_sumsq_parts_through_the_library(dev, n):
    """The sum of dcs_grad_sumsq_parts' 512 partial sums against the fp64 sum of squares: the n % 4 tail, and the wrapping size."""
    from dcsnet import _lib
    from dcsnet._lib import check, ptr, cur_stream
    g = tl.randn(n, 95, 0.3)
    gd = g.to(dev)
    parts = torch.full((512,), float('nan'), dtype=torch.float64, device=dev)
    check(_lib.load().dcs_grad_sumsq_parts(ptr(gd), n, ptr(parts), 512, None, None, None, None, 0, cur_stream()), 'dcs_grad_sumsq_parts')
    got = {'sumsq': parts.sum().reshape(1)}
    ref = {'sumsq': (g.double() ** 2).sum().reshape(1)}
    yard = {'sumsq': (torch.linalg.vector_norm(gd) ** 2).reshape(1)}
    misses = _judge(('adam', 'library', f'sumsq_n{n}'), got, ref, yard)
    assert not misses, misses
