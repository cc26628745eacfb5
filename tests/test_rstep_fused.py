"""GPU: the real twin's fused step — dcs_complex_abs_f32 and the dcs_rmask_apply_polar_frames pair (csrc/mask.hip) through
ops.complex_abs / F.rmask_apply_polar_wave, the route network_functions._real_step takes with them, and the train step built
on it against the op-by-op spelling it replaces (RSTEP_FUSED off).

The yardstick of the kernel pair is the reference's own formula chain (network_functions.py:224-232 and
oracle.nf_oracle.mag_phase_2_wave) evaluated in fp64 on the CPU, computed once per (shape, hop) and shared by the cases; the
op-by-op chain of the parent (torch.abs / atan2 / sigmoid / cos / sin / complex / pad / irfft on the device) is measured
against the same fp64 result in the same test, and the fused node may be at most 4x as far from fp64 as that chain is, with a
floor of 2e-6 (relative to max|ref|).  4x: both routes are a handful of fp32 roundings per element, while any omission (a missed
x2 of the one-sided spectrum, a shifted bin, a sign, the order of a - n) is O(1).  2e-6: this project's bound for fft512.hip
against torch.fft.  Figures go to $DCS_PARITY_DIR/rstep_parity.json (default parity_out/, kept out of git); a full run's file
is committed as profiles/rstep_parity.json.
"""
import functools
import sys
import types
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.nf_oracle import mag_phase_2_wave as mag_phase_2_wave_oracle   # noqa: E402
from oracle.seeded_state import fill_state_stream, seeded_input            # noqa: E402
from _ragged_helpers import record                                         # noqa: E402

EPS = float(np.float32(10e-7))            # hparams['atan2_eps'] as the fp32 kernels and torch's fp32 add see it
F_BINS = 256


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from dcsnet import _lib
    _lib.load()
    return torch.device('cuda:0')


_record = functools.partial(record, 'rstep_parity.json')     # figures -> $DCS_PARITY_DIR/rstep_parity.json (default parity_out/)


# ------------------------------------------------------------------------------------------------------------ complex_abs

def test_complex_abs_against_fp64_hypot(dev):
    """n = 1027 (a ragged tail of the 256-thread grid-stride loop), with zeros, (-1e-6, 0), 1e-30-sized and 1e19-sized components
    planted: x^2 + y^2 underflows to 0 / overflows to inf there, hypot does neither.  4 ulp: the OpenCL bound for hypot, which
    the device math library follows; a wrong component or an overflow is O(1)."""
    from dcsnet import ops
    n = 1027
    g = torch.Generator().manual_seed(11)
    y = torch.randn(n, 2, generator=g)
    y[0] = 0.0
    y[1] = torch.tensor([-1e-6, 0.0])
    y[2] = torch.tensor([1e-30, -2e-30])
    y[3] = torch.tensor([0.0, 3e-30])
    y[4] = torch.tensor([1e19, 1e19])
    y[5] = torch.tensor([-3e19, 4e18])
    y[1026] = torch.tensor([2e19, -1e-30])                               # the last element of the tail
    y[300:400] *= 1e19
    y[500:600] *= 1e-30
    want = torch.hypot(y[:, 0].double(), y[:, 1].double())
    assert bool(torch.isfinite(want.float()).all()) and float(want.max()) > 1e19
    yc = torch.view_as_complex(y.contiguous()).to(dev)
    got = ops.complex_abs(yc)
    assert got.shape == (n,) and got.dtype == torch.float32
    assert torch.equal(ops.complex_abs(torch.view_as_real(yc)), got)    # the (re, im) view: the same launch
    got = got.cpu()
    assert bool(torch.isfinite(got).all()) and float(got[0]) == 0.0
    ulp = torch.from_numpy(np.spacing(want.float().numpy())).double()
    err = ((got.double() - want).abs() / ulp)
    _record(('complex_abs', 'max_err_ulp'), float(err.max()))
    print(f'complex_abs: max error {float(err.max()):.3f} ulp')
    assert float(err.max()) <= 4.0
    got3 = ops.complex_abs(yc.reshape(13, 79))                           # shape follows the input
    assert got3.shape == (13, 79) and torch.equal(got3.reshape(-1).cpu(), got)


# ------------------------------------------------------------------------------------------------- the kernel pair, via the node

SHAPES = ((3, 40), (2, 72), (1, 8))        # (B, T): ragged 32-tiles in T (40 = 32 + 8, 72 = 64 + 8, 8 < 32), several blocks, B = 1
HOPS = (128, 32)                           # (inverse FFT + overlap-add in one kernel | the configured hop: two kernels)
_cases = {}


def _inputs(B, T):
    g = torch.Generator().manual_seed(100 * B + T)
    Y = torch.complex(torch.randn(B, F_BINS, T, generator=g), torch.randn(B, F_BINS, T, generator=g))
    D = 2.0 * torch.randn(B, F_BINS, T, generator=g)
    yp = torch.tensor([0, -1e-6 + 0j, 1e-7 - 1e-7j, -2 + 0j], dtype=torch.complex64)
    dp = torch.tensor([0, -30, 30, 1e-7, -88, 89], dtype=torch.float32)
    # every planted Y meets every planted D: bin rows 0..3 (row 0 is not doubled by the one-sided weighting) of the first item's first
    # frames, and bin rows 252..255 (255: next to the zero bin) of the last item's last frames
    for j, v in enumerate(yp):
        Y[0, j, :6], D[0, j, :6] = v, dp
        Y[B - 1, F_BINS - 4 + j, T - 6:], D[B - 1, F_BINS - 4 + j, T - 6:] = v, dp
    return Y, D


def _case(B, T, hop, dev):
    """Inputs, seeded cotangents, the fp64 yardstick of both forms (pair / not) and the parent's device chain's distance to it:
    computed once per (B, T, hop), shared by the parametrised cases and left unchanged."""
    key = (B, T, hop)
    if key in _cases:
        return _cases[key]
    from dcsnet import network_functions as nf
    Y, D = _inputs(B, T)
    L = hop * (T - 1)
    g = torch.Generator().manual_seed(7 + T + hop)
    gw = torch.randn(2 * B, L, generator=g)                              # cotangent of the waveforms (rows [0, B) alone without pair)
    gM = torch.randn(B, F_BINS, T, generator=g)                           # cotangent of the mask (want_mask)
    window = torch.hann_window(512)
    ref, parent = {}, {}
    # fp64, CPU: network_functions.py:224-232 + mag_phase_2_wave
    Y64 = Y.to(torch.complex128)
    a64, ph64 = torch.abs(Y64), torch.atan2(Y64.imag, Y64.real + EPS)
    cfg = types.SimpleNamespace(fft_size=512, hop_length=hop, window=window, normalise_stft=True)
    Yd = Y.to(dev)
    for pair in (True, False):
        rows = 2 * B if pair else B
        for want_mask in (False, True):
            D64 = D.double().requires_grad_(True)
            m = torch.sigmoid(D64)
            n = a64 * m
            waves = [mag_phase_2_wave_oracle(n, ph64, 512, hop, window.double())]
            if pair:
                waves.append(mag_phase_2_wave_oracle(a64 - n, ph64, 512, hop, window.double()))
            w = torch.cat(waves)
            assert w.dtype == torch.float64 and w.shape == (rows, L)
            loss = (w * gw[:rows].double()).sum() + ((m * gM.double()).sum() if want_mask else 0.0)
            (gD,) = torch.autograd.grad(loss, D64)
            ref[pair, want_mask] = (w.detach(), gD, m.detach())
            # the parent's op-by-op chain on the device (today's _real_step)
            Dd = D.to(dev).requires_grad_(True)
            mag = torch.abs(Yd)
            phase = torch.atan2(Yd.imag, Yd.real + 10e-7)
            mk = torch.sigmoid(Dd)
            nm = mag * mk
            pw = [nf.mag_phase_2_wave(nm, phase, cfg)]
            if pair:
                pw.append(nf.mag_phase_2_wave(mag - nm, phase, cfg))
            pw = torch.cat(pw)
            ploss = (pw * gw[:rows].to(dev)).sum() + ((mk * gM.to(dev)).sum() if want_mask else 0.0)
            (pg,) = torch.autograd.grad(ploss, Dd)
            parent[pair, want_mask] = tuple(_rel(x, r) for x, r in zip((pw, pg, mk), ref[pair, want_mask]))
    _cases[key] = (Y, D, gw, gM, ref, parent)
    return _cases[key]


def _rel(x, ref):
    return float((x.detach().double().cpu() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize('want_mask', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('pair', [True, False], ids=['drs', 'dr'])
@pytest.mark.parametrize('hop', HOPS)
@pytest.mark.parametrize('B,T', SHAPES)
def test_fused_node_against_fp64_and_the_parent_chain(dev, B, T, hop, pair, want_mask):
    from dcsnet import ops, functional as F
    Y, D, gw, gM, ref, parent = _case(B, T, hop, dev)
    w_ref, g_ref, m_ref = ref[pair, want_mask]
    rows = 2 * B if pair else B
    window = torch.hann_window(512).to(dev)
    inv_env = ops.istft_envelope(window, T, hop)
    Yd = Y.to(dev)

    def run():
        Dd = D.to(dev).requires_grad_(True)
        M, w = F.rmask_apply_polar_wave(Yd, Dd, window, inv_env, 512, hop, 512 ** 0.5, 10e-7, pair=pair, want_mask=want_mask)
        loss = (w * gw[:rows].to(dev)).sum()
        if want_mask:
            loss = loss + (M * gM.to(dev)).sum()
        (gD,) = torch.autograd.grad(loss, Dd)
        return M, w.detach(), gD

    M, w, gD = run()
    M2, w2, gD2 = run()
    assert w.shape == (rows, hop * (T - 1)) and gD.shape == D.shape and gD.dtype == torch.float32
    assert torch.equal(w, w2) and torch.equal(gD, gD2)                   # two runs: the same bits
    assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(gD).all())
    if want_mask:
        assert M.shape == D.shape and torch.equal(M.detach(), M2.detach()) and bool(torch.isfinite(M).all())
    else:
        assert M is None
    errs = {'wave': _rel(w, w_ref), 'g_D': _rel(gD, g_ref)}
    if want_mask:
        errs['mask'] = _rel(M, m_ref)
    perr = dict(zip(('wave', 'g_D', 'mask'), parent[pair, want_mask]))
    tag = f'B{B}_T{T}_hop{hop}_{"drs" if pair else "dr"}_{"mask" if want_mask else "nomask"}'
    _record(('node', tag), {k: {'fused': errs[k], 'parent': perr[k]} for k in errs})
    print(tag, {k: (f'{errs[k]:.3e}', f'{perr[k]:.3e}') for k in errs})
    # the raw spectra: frame-major, bins >= F exactly zero (the zero bin mag_phase_2_wave pads), every row written
    M3, spec = ops.rmask_apply_polar_frames(torch.view_as_real(Yd), D.to(dev), F_BINS + 1, 10e-7, pair, want_mask)
    assert spec.shape == (rows, T, F_BINS + 1, 2) and not spec[:, :, F_BINS:].any() and bool(torch.isfinite(spec).all())
    assert (M3 is None) == (not want_mask)
    # ... and against fp64: rows [0, B) = |Y| m u, rows [B, 2B) = (|Y| - |Y| m) u, transposed
    Y64 = Y.to(torch.complex128)
    a64 = torch.abs(Y64)
    u64 = torch.polar(torch.ones_like(a64), torch.atan2(Y64.imag, Y64.real + EPS))
    n64 = a64 * m_ref
    want_spec = torch.cat([n64 * u64] + ([(a64 - n64) * u64] if pair else [])).transpose(1, 2)
    got_spec = torch.view_as_complex(spec[:, :, :F_BINS].contiguous()).cpu().to(torch.complex128)
    e_spec = float((got_spec - want_spec).abs().max() / want_spec.abs().max())
    _record(('node', tag, 'spectrum'), {'fused': e_spec})
    assert e_spec <= 2e-6, e_spec
    for k in errs:
        assert errs[k] <= max(4 * perr[k], 2e-6), (k, errs[k], perr[k])


# -------------------------------------------------------------------------------------------------------- the route is taken

class _Forbidden(RuntimeError):
    pass


def _forbid(name):
    def f(*a, **k):
        raise _Forbidden(f'torch.{name} on the fused route')
    return f


def _net(dev, seed=5):
    from dcsnet.config import config, hparams
    from dcsnet.r_network import R_NETWORK
    hp = dict(hparams)
    hp['dropout_conv'], hp['dropout_fc'] = 0.0, 0.0
    return fill_state_stream(R_NETWORK(config, hp, 0), seed).to(dev).train()


def _batch(dev, B=2, T=32):
    clean, noise = seeded_input(B, 256, T, 1, 0.1), seeded_input(B, 256, T, 2, 0.05)
    return (noise.to(dev), (clean + noise).to(dev), clean.to(dev), list(range(B)))


@pytest.mark.parametrize('mode', ['drs', 'dr'])
def test_the_train_step_takes_the_fused_route(dev, mode, monkeypatch):
    """No inverse FFT of the library and no atan2 on the default route; with RSTEP_FUSED off the op-by-op spelling needs both."""
    from dcsnet import network_functions as nf
    net, batch = _net(dev), _batch(dev)
    monkeypatch.setattr(sys, 'argv', ['train.py', mode, '0'])
    monkeypatch.setattr(torch.fft, 'irfft', _forbid('fft.irfft'))
    monkeypatch.setattr(torch, 'atan2', _forbid('atan2'))
    assert nf.RSTEP_FUSED
    out = nf.train_batch_2_loss(net, batch, 0, 'real')
    loss = out[2] if isinstance(out, tuple) else out
    loss.backward()
    assert bool(torch.isfinite(loss)) and float(net.encoder[0][0].weight.grad.abs().max()) > 0
    monkeypatch.setattr(nf, 'RSTEP_FUSED', False)
    with pytest.raises(_Forbidden):
        nf.train_batch_2_loss(net, batch, 0, 'real')


def test_a_batch_of_one_takes_the_fused_route(dev, monkeypatch):
    """R_NETWORK.forward squeezes a batch of one to [F, T] (r_network.py:173); the step puts the batch axis back."""
    from dcsnet import network_functions as nf
    net, batch = _net(dev), _batch(dev, B=1)
    monkeypatch.setattr(sys, 'argv', ['train.py', 'drs', '0'])
    monkeypatch.setattr(torch, 'atan2', _forbid('atan2'))
    fused = nf.train_batch_2_loss(net, batch, 0, 'real')[2]
    monkeypatch.undo()
    monkeypatch.setattr(sys, 'argv', ['train.py', 'drs', '0'])
    monkeypatch.setattr(nf, 'RSTEP_FUSED', False)
    plain = nf.train_batch_2_loss(_net(dev), batch, 0, 'real')[2]
    a, b = float(fused), float(plain)
    assert abs(a - b) <= 1e-3 * abs(b) + 1e-3, (a, b)


# ------------------------------------------------------------------------------------------------- fused against unfused step

def _loss_and_grad_norms(dev, mode, fused, monkeypatch):
    from dcsnet import network_functions as nf
    monkeypatch.setattr(sys, 'argv', ['train.py', mode, '0'])
    monkeypatch.setattr(nf, 'RSTEP_FUSED', fused)
    net = _net(dev)
    out = nf.train_batch_2_loss(net, _batch(dev), 0, 'real')
    loss = out[2] if isinstance(out, tuple) else out
    loss.backward()
    return float(loss), {n: (None if p.grad is None else float(p.grad.norm())) for n, p in net.named_parameters()}


@pytest.mark.parametrize('mode', ['drs', 'dr'])
def test_fused_step_matches_the_unfused_step(dev, mode, monkeypatch):
    """Same seeded net, same batch.  Loss: 1e-3 |a| + 1e-3, the bound of test_rnetwork_graph_replayed_train_step_matches_eager for
    this net.  Parameter-gradient norms: 3e-3 relative (+ 2e-5), the DR-Net gradient-norm bound of
    test_rnetwork_gradients_against_reference_vectors — whose form for a conv bias in front of a batch-statistics BatchNorm
    (a gradient that is rounding noise) is kept too."""
    la, ga = _loss_and_grad_norms(dev, mode, True, monkeypatch)
    lb, gb = _loss_and_grad_norms(dev, mode, False, monkeypatch)
    print(mode, 'loss fused / unfused', la, lb)
    assert abs(la - lb) <= 1e-3 * abs(lb) + 1e-3, (la, lb)
    assert sorted(ga) == sorted(gb)
    seen = 0
    for n, want in gb.items():
        got = ga[n]
        if want is None:                               # decoder_attention.12 / .13: built, never run
            assert got is None, n
        elif n.endswith('.0.bias') and not n.startswith('decoder.6'):
            assert got <= 2e-3 * max(1.0, want) + 1e-3, n
        else:
            assert abs(got - want) <= 3e-3 * want + 2e-5, (n, got, want)
            seen += want > 1e-4
    assert seen > 20


def test_captured_fused_train_step_follows_the_eager_one(dev, monkeypatch):
    from dcsnet import network_functions as nf
    from dcsnet.dp import TrainStep
    monkeypatch.setattr(sys, 'argv', ['train.py', 'drs', '0'])
    assert nf.RSTEP_FUSED
    batch = _batch(dev)
    runs = []
    for use_graph in (False, True):
        ts = TrainStep(_net(dev), use_graph=use_graph, graph_warmup=2)
        with warnings.catch_warnings():
            warnings.simplefilter('error')                               # a capture failure warns: make it fail here
            losses = [float(ts(batch)) for _ in range(5)]
        runs.append((losses, ts))
    (eager, _), (graph, ts_g) = runs
    assert ts_g._graph is not None, 'capture did not happen (fell back to eager)'
    for a, b in zip(eager, graph):
        assert abs(a - b) <= 1e-3 * abs(a) + 1e-3, (eager, graph)
    assert len(set(eager)) == 5                                          # the steps really moved the weights
