"""CPU: the host side of tests/test_tail_fp64.py — oracle/tail_fp64.py's written-out Adam step against torch.optim.Adam in
double, its closed forms and written-out overlap-add against autograd / torch.istft in double on the planted set, and the
comparator against itself: it accepts a correct fp32 evaluation of every case (the nf_oracle chain in fp32, and the kernels'
closed forms evaluated in fp32) and scores every seeded fault at 10x the limit of its tensor or more, at the smallest GPU
shape of each family.
"""
import numpy as np
import pytest
import torch

from oracle import nf_oracle as nf
from oracle import tail_fp64 as tl

F_BINS = 256


@pytest.fixture(scope='module', autouse=True)
def _threads():
    old = tl.set_threads()
    yield
    torch.set_num_threads(old)


def _window(n=512):
    return torch.hann_window(n)


# ------------------------------------------------------------------------------------------------------------------ Adam

KW = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-3, max_norm=0.5)


def _grads(n, steps, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) * (3.0 if it % 2 else 0.01) for it in range(steps)]       # unclipped / clipped


def _torch_adam(p0, grads, world, dtype):
    return tl.torch_adam_states(p0, grads, world, KW, dtype)


@pytest.mark.parametrize('world', [1, 4])
def test_written_out_adam_equals_torch_adam_in_double(world):
    n = 4 * 300 + 3
    p0 = tl.randn(n, 3).double()
    grads = _grads(n, 6)
    clips = [float((g.double() / world).norm()) > KW['max_norm'] for g in grads]
    assert any(clips) and not all(clips)
    want = _torch_adam(p0, grads, world, torch.float64)
    ref = tl.AdamRef(p0, **KW)
    for it, g in enumerate(grads):
        ref.step(g, world)
        for k, v in ref.state().items():
            assert tl.score(v, want[it][k]) <= 1e-12, (it, k)
    assert ref.t == 6


def test_a_skipped_step_changes_nothing_and_is_not_counted():
    n = 64
    ref, same = tl.AdamRef(tl.randn(n, 3), **KW), tl.AdamRef(tl.randn(n, 3), **KW)
    grads = _grads(n, 3)
    ref.step(grads[0]), same.step(grads[0])
    before = {k: v.clone() for k, v in ref.state().items()}
    ref.step(grads[1], skip=True)
    assert all(torch.equal(v, before[k]) for k, v in ref.state().items()) and (ref.t, ref.calls) == (1, 2)
    ref.step(grads[2]), same.step(grads[2])
    assert all(torch.equal(v, same.state()[k]) for k, v in ref.state().items())


@pytest.mark.parametrize('fault', tl.ADAM_FAULTS)
def test_the_comparator_rejects_every_seeded_adam_fault(fault):
    """6 steps, world 4, a skipped third call: the written-out step in fp32 (a second fp32 evaluation beside torch's, the
    yardstick) is accepted on every tensor after every step, the fault is at 10x the limit or more on some tensor after some
    step — the update dp included, under its stated allowance."""
    n, world = 4 * 300 + 3, 4
    p0 = tl.randn(n, 3)
    grads = _grads(n, 6, seed=2)
    ref, bad, second = tl.AdamRef(p0, **KW), tl.AdamRef(p0, fault=fault, **KW), tl.AdamRef(p0, dtype=torch.float32, **KW)
    y32 = iter(_torch_adam(p0, [g for i, g in enumerate(grads) if i != 2], world, torch.float32))
    worst, prev, yprev, sprev = 0.0, ref.state(), {'p': p0}, {'p': p0}
    for it, g in enumerate(grads):
        ref.step(g, world, skip=it == 2), bad.step(g, world, skip=it == 2), second.step(g, world, skip=it == 2)
        if it == 2:
            continue
        r, b, y, s2 = dict(ref.state()), dict(bad.state()), dict(next(y32)), dict(second.state())
        assert s2['p'].dtype == torch.float32 and s2['v'].dtype == torch.float32
        r['dp'], b['dp'], y['dp'] = r['p'] - prev['p'], b['p'] - prev['p'], y['p'].double() - yprev['p'].double()
        s2['dp'] = s2['p'].double() - sprev['p'].double()
        floors = {'dp': tl.adam_dp_floor(ref.t, KW['betas'][1], float(r['p'].abs().max()), float(r['dp'].abs().max()))}
        rows, misses = tl.judge(s2, r, y, floors=floors)
        assert not misses, (it, misses)
        rows, _ = tl.judge(b, r, y, floors=floors)
        worst = max(worst, max(row['err'] / row['limit'] for row in rows.values()))
        prev, yprev, sprev = r, y, s2
    print(fault, f'worst err / limit {worst:.1f}')
    assert worst >= 10.0, (fault, worst)


# ----------------------------------------------------------------------------------------------------- closed forms, algebra

def _c2(z):
    return z.real, z.imag


def test_closed_forms_equal_autograd_in_double_on_the_planted_set():
    Y, D, where = tl.inputs(1, F_BINS, 8, True)
    assert int(where.sum()) == 2 * len(tl.Y_PLANTS) * len(tl.D_PLANTS)
    gM, gN = tl.randn(D.shape, 5, cplx=True).to(torch.complex128), tl.randn(D.shape, 6, cplx=True).to(torch.complex128)
    D64, Y64 = D.to(torch.complex128), Y.to(torch.complex128)
    # one bound, forward and backward
    r = tl.evaluate(lambda D: {'M': tl.bound(D)}, {'D': D}, {}, {'M': gM}, True)
    assert tl.score(torch.complex(*tl.bound_one(*_c2(D64))), r['M']) <= 1e-12
    for sel in (where, ~where):
        assert tl.score(torch.complex(*tl.bound_one_bwd(*_c2(D64), *_c2(gM))), r['g_D'], sel) <= 1e-12
    # both bounds + multiply + subtract, cotangents of M, N and S
    r = tl.evaluate(lambda D, Y: tl.mask_apply(Y, D, pre=True), {'D': D}, {'Y': Y}, {'M': gM, 'N': gN, 'S': gM}, True)
    g = gN - gM                                                           # conj(Y) (gN - gS) + gM
    g = torch.complex(Y64.real * g.real + Y64.imag * g.imag, Y64.real * g.imag - Y64.imag * g.real) + gM
    m1 = tl.bound_one(*_c2(D64))
    g1 = tl.bound_one_bwd(*m1, *_c2(g))
    for sel in (where, ~where):
        assert tl.score(torch.complex(*tl.bound_one_bwd(*_c2(D64), *g1)), r['g_D'], sel) <= 1e-12
    # the polar turn
    r = tl.evaluate(lambda D: {'z': tl.polar(D)}, {'D': D}, {}, {'z': gM}, True)
    assert tl.score(torch.complex(*tl.polar_turn(*_c2(D64))), r['z']) <= 1e-12
    for sel in (where, ~where):
        assert tl.score(torch.complex(*tl.polar_turn_bwd(*_c2(D64), *_c2(gM))), r['g_D'], sel) <= 1e-12
    assert bool(torch.isfinite(torch.view_as_real(r['g_D'])).all())


@pytest.mark.parametrize('B,L', [(4, 3), (5, 1001)])
def test_sisnr_closed_form_equals_autograd_in_double(B, L):
    c, e = tl.sisnr_rows(B, L)
    r = tl.evaluate(lambda e, c: {'snr': tl.snr_rows(c, e)}, {'e': e}, {'c': c}, {'snr': torch.ones(B)}, True)
    snr, g = tl.sisnr_closed(c.double(), e.double())
    assert tl.score(snr, r['snr']) <= 1e-12 and tl.score(g, r['g_e']) <= 1e-12
    assert abs(float(r['snr'].mean()) - float(nf.si_snr(c.double(), e.double(), tl.SNR_EPS))) <= 1e-12
    zero = [b for b in range(B) if tl.SNR_ROWS[b % len(tl.SNR_ROWS)] == 'zero_target']
    assert zero and all(abs(float(r['snr'][b]) + 80.0) < 1e-6 and not r['g_e'][b].any() for b in zero)


@pytest.mark.parametrize('n_fft,hop,T', [(512, 128, 2), (512, 32, 19), (512, 256, 14), (64, 6, 9)])
def test_written_out_overlap_add_equals_torch_istft_in_double(n_fft, hop, T):
    w = torch.hann_window(n_fft, dtype=torch.float64)
    X = tl.randn((2, T, n_fft // 2 + 1), 9, cplx=True).to(torch.complex128)
    frames = torch.fft.irfft(X, n=n_fft, dim=-1, norm='forward')
    want = torch.istft(X.transpose(1, 2), n_fft=n_fft, hop_length=hop, win_length=n_fft, window=w)
    assert tl.score(tl.ola(frames, w, hop, 1.0 / n_fft), want) <= 1e-12
    assert tl.score(_ola_by_envelope(frames, w, hop, 1.0 / n_fft), want) <= 1e-12


def _ola_by_envelope(frames, w, hop, scale):
    """The kernels' spelling: the overlap-added windowed frames times envelope()'s reciprocal."""
    B, T, n_fft = frames.shape
    y = torch.zeros(B, hop * (T - 1) + n_fft, dtype=frames.dtype)
    for f in range(T):
        y[:, f * hop:f * hop + n_fft] += frames[:, f] * w
    return scale * y[:, n_fft // 2:n_fft // 2 + hop * (T - 1)] * tl.envelope(w, T, hop)


# ---------------------------------------------------------------------------------------- the comparator at the GPU shapes

def _accept(got, ref, yard, **kw):
    rows, misses = tl.judge(got, ref, yard, **kw)
    assert not misses, misses
    return rows


def _reject(bad, ref, yard, key, where=None):
    """The fault's score on tensor `key` (over `where`) is 10x the limit of that tensor or more."""
    s = tl.score(bad, ref[key], where)
    lim = tl.limit_of(tl.score(yard[key], ref[key], where))
    assert s >= 10 * lim, (key, s, lim)
    return s / lim


def test_comparator_on_the_masks_at_the_smallest_gpu_shape():
    """n = 1027 = [1, 13, 79], planted; the nf_oracle chain in fp32 and the kernels' closed forms in fp32 are accepted, the
    second bound without its eps (seen by the planted gradients) and S = N - Y are not."""
    Y, D, where = tl.inputs(1, 13, 79, True)
    cots = {k: tl.randn(D.shape, 20 + i, cplx=True) for i, k in enumerate(('M1', 'M', 'N', 'S'))}
    fn = lambda D, Y: tl.mask_apply(Y, D, pre=True)                                              # noqa: E731
    ref, yard = (tl.evaluate(fn, {'D': D}, {'Y': Y}, cots, wide) for wide in (True, False))
    # the kernels' closed forms, in fp32: a second evaluation with roundings of its own
    m1 = tl.bound_one(*_c2(D))
    m = tl.bound_one(*m1)
    Mc = torch.complex(*m)
    N = torch.complex(Y.real * m[0] - Y.imag * m[1], Y.real * m[1] + Y.imag * m[0])
    t = cots['N'] - cots['S']
    g = cots['M'] + torch.complex(Y.real * t.real + Y.imag * t.imag, Y.real * t.imag - Y.imag * t.real)
    g1 = tl.bound_one_bwd(*m1, *_c2(g))
    gd = tl.bound_one_bwd(*_c2(D), g1[0] + cots['M1'].real, g1[1] + cots['M1'].imag)
    closed = {'M1': torch.complex(*m1), 'M': Mc, 'N': N, 'S': Y - N, 'g_D': torch.complex(*gd)}
    rows = _accept(closed, ref, yard, where=where, twice=('g_D',))
    print({k: (f"{r['err']:.2e}", f"{r['limit']:.2e}") for k, r in rows.items()})
    bad = tl.evaluate(lambda D, Y: tl.mask_apply(Y, D, pre=True, eps2=0.0), {'D': D}, {'Y': Y}, cots, True)
    _reject(bad['g_D'], ref, yard, 'g_D', where)           # (on M itself the eps is 1e-6 of max |M|: the planted gradients see it)
    _reject(-ref['S'], ref, yard, 'S')


@pytest.mark.parametrize('B,F,T', [(1, 256, 8)])
def test_comparator_on_the_polar_frames_at_the_smallest_gpu_shape(B, F, T):
    z = tl.inputs(B, F, T, True)[1]
    G = tl.randn((B, T, F + 1), 31, cplx=True)
    w = tl.herm_weights(F + 1)

    def run(wide, wts):
        return tl.evaluate(lambda z, G, wts: {'spec': tl.polar_frames(z), 'gspec': tl.polar_frames(z) * wts}, {'z': z},
                           {'G': G, 'wts': wts}, {'gspec': G}, wide)
    ref, yard = run(True, w), run(False, w)
    gx, gy = tl.polar_turn_bwd(*_c2(z), *_c2((G * w)[:, :, :F].transpose(1, 2)))
    _accept({'spec': yard['spec'], 'gspec': yard['gspec'], 'g_z': torch.complex(gx, gy)}, ref, yard)
    _reject(run(True, tl.herm_weights(F + 1, skip_row=100))['g_z'], ref, yard, 'g_z')          # a missing x2 on one interior row
    _reject(run(True, tl.herm_weights(F + 1, dc=True))['g_z'], ref, yard, 'g_z')               # the x2 also on bin 0


def test_comparator_on_a_wrongly_transposed_ragged_tile():
    """[3, 256, 40]: frames 32..39 (the ragged tile row) of the last full bin tile and of an interior one."""
    z = tl.inputs(3, F_BINS, 40, False)[1]
    ref, yard = (tl.evaluate(lambda z: {'spec': tl.polar_frames(z)}, {'z': z}, {}, None, wide) for wide in (True, False))
    for f0 in (224, 96):
        bad = tl.fault_tile(ref['spec'], 32, f0)
        assert not torch.equal(bad, ref['spec'])
        _reject(bad, ref, yard, 'spec')


@pytest.mark.parametrize('planted', [False, True], ids=['regular', 'planted'])
def test_comparator_on_the_node_and_the_tail_at_the_smallest_gpu_shape(planted):
    """[1, 256, 8], hop 128: waveforms, mask, the three losses and g_D; the nf_oracle chain in fp32 is accepted; swapped rows,
    S = N - Y and the eps dropped from the second bound are not."""
    B, T, hop = 1, 8, 128
    Y, D, where = tl.inputs(B, F_BINS, T, planted)
    L = hop * (T - 1)
    window = _window()
    tn, ts = tl.inputs(B, F_BINS, T, False, seed=1)[:2]
    target = torch.cat([tl.wave(tn.to(torch.complex128), hop, window.double()), tl.wave(ts.to(torch.complex128), hop, window.double())]).float()
    cots = {'M': tl.randn(D.shape, 41, cplx=True), 'wave': tl.randn((2 * B, L), 42)}
    fn = lambda D, Y, window, **k: tl.node(Y, D, window, hop, **k)                               # noqa: E731
    ref, yard = (tl.evaluate(fn, {'D': D}, {'Y': Y, 'window': window}, cots, wide) for wide in (True, False))
    # a second fp32 evaluation by another route (torch.fft.irfft and the written-out overlap-add, not torch.istft), under the rule
    # as the GPU tests apply it: g_D over the unplanted elements, the plants with Y = -eps and the other plants
    parts = tl.plant_classes(where, Y)
    second = tl.evaluate(lambda D, Y, window: tl.node(Y, D, window, hop, written=True), {'D': D}, {'Y': Y, 'window': window}, cots, False)
    assert not torch.equal(second['wave'], yard['wave'])
    rows = _accept(second, ref, yard, where=parts, twice=('g_D',))
    print(planted, 'node', {k: (f"{r['err']:.2e}", f"{r['limit']:.2e}") for k, r in rows.items()})
    sel = None if where is None else ~where
    _reject(tl.fault_swap_rows(ref['wave']), ref, yard, 'wave')
    bad = tl.evaluate(lambda D, Y, window: tl.node(Y, D, window, hop, s_sign=-1.0), {'D': D}, {'Y': Y, 'window': window}, cots, True)
    _reject(bad['wave'], ref, yard, 'wave')
    _reject(bad['g_D'], ref, yard, 'g_D', sel)
    bad = tl.evaluate(lambda D, Y, window: tl.node(Y, D, window, hop, eps2=0.0), {'D': D}, {'Y': Y, 'window': window}, cots, True)
    if planted:                                            # (on M itself the eps is 1e-6 of max |M|: the planted gradients see it)
        _reject(bad['g_D'], ref, yard, 'g_D', where)
    # the tail end to end
    fn = lambda D, Y, window, target: {'losses': tl.tail(Y, D, target, window, hop)['losses']}   # noqa: E731
    consts = {'Y': Y, 'window': window, 'target': target}
    cot = {'losses': torch.eye(3)[2]}                       # the total, the cotangent of the GPU case
    ref, yard = (tl.evaluate(fn, {'D': D}, consts, cot, wide) for wide in (True, False))
    second = tl.evaluate(lambda D, Y, window, target: {'losses': tl.tail(Y, D, target, window, hop, written=True)['losses']},
                         {'D': D}, consts, cot, False)        # ... and the kernels' sums in place of nf.si_snr
    rows = _accept(second, ref, yard, where=parts, twice=('g_D',))
    print(planted, 'tail', {k: (f"{r['err']:.2e}", f"{r['limit']:.2e}") for k, r in rows.items()})
    swapped = tl.evaluate(fn, {'D': D}, dict(consts, target=tl.fault_swap_rows(target)), cot, True)
    _reject(swapped['losses'], ref, yard, 'losses')
    _reject(swapped['g_D'], ref, yard, 'g_D', sel)


@pytest.mark.parametrize('B,L', [(4, 3), (3, 1001), (1, 512), (5, 1000)])
def test_comparator_on_sisnr(B, L):
    """The kernels' k1 c + k2 e form in fp32 is accepted next to fp32 autograd; the last L % 4 samples left out of the sums and
    k1 without its a * on_r term are not."""
    c, e = tl.sisnr_rows(B, L)
    fn = lambda e, c: {'snr': tl.snr_rows(c, e)}                                                 # noqa: E731
    ref, yard = (tl.evaluate(fn, {'e': e}, {'c': c}, {'snr': torch.ones(B)}, wide) for wide in (True, False))
    snr, g = tl.sisnr_closed(c, e)
    rows = _accept({'snr': snr, 'g_e': g}, ref, yard)
    print(B, L, {k: (f"{r['err']:.2e}", f"{r['yardstick']:.2e}") for k, r in rows.items()})
    if L % 4:
        snr, g = tl.sisnr_closed(c.double(), e.double(), drop_tail=L % 4)
        _reject(snr, ref, yard, 'snr')
    _reject(tl.sisnr_closed(c.double(), e.double(), drop_a_term=True)[1], ref, yard, 'g_e')


@pytest.mark.parametrize('L', [3, 1000, 1001])
def test_comparator_on_sisnr_at_60_db(L):
    """The stated allowance of the k1 c + k2 e form is 4 x 2^-24 x 10^(dB/20) to a few per cent; with it the form in fp32 is
    accepted at 60 dB, and k1 without its a * on_r term is still at 10x the limit or more."""
    B = 2
    c, e = tl.sisnr_rows(B, L, seed=2, level=60.0)
    fn = lambda e, c: {'snr': tl.snr_rows(c, e)}                                                 # noqa: E731
    ref, yard = (tl.evaluate(fn, {'e': e}, {'c': c}, {'snr': torch.ones(B)}, wide) for wide in (True, False))
    allow = tl.sisnr_form_allowance(c, e)
    db = float(ref['snr'].max())
    ratio = (e.double().abs().max(-1).values / (e.double() - c.double()).abs().max(-1).values).max()     # max |e_n| / max |r_n|, about
    assert 58.0 < db < 60.01 and 0.2 < allow / (4 * 2.0 ** -24 * float(ratio)) < 5.0, (db, allow)
    snr, g = tl.sisnr_closed(c, e)
    rows, misses = tl.judge({'snr': snr, 'g_e': g}, ref, yard, floors={'g_e': tl.FLOOR + allow})
    print(L, allow, {k: (f"{r['err']:.2e}", f"{r['yardstick']:.2e}", f"{r['limit']:.2e}") for k, r in rows.items()})
    assert not misses, misses
    bad = tl.sisnr_closed(c.double(), e.double(), drop_a_term=True)[1]
    assert tl.score(bad, ref['g_e']) >= 10 * rows['g_e']['limit']


def test_an_identically_zero_reference_is_an_error():
    z = torch.zeros(4)
    with pytest.raises(AssertionError, match='dead case'):
        tl.score(z, z)
    with pytest.raises(AssertionError, match='non-finite'):
        tl.score(torch.tensor([float('nan')]), torch.ones(1))
    assert tl.limit_of(0.0) == tl.FLOOR and tl.limit_of(1e-6) == 4e-6
    assert tl.EPS == float(np.float32(10e-7))
