"""One layer at a time, at the train step's own shapes, against fp64 — every element of every tensor.

The train step at BASELINE configs[2] (`[32,256,256]`) is checked end to end by tests/test_full_size.py, whose bound
(rel-L2 1.5e-2 per gradient tensor: the fp32 noise of 30 chained layers) cannot see a fault confined to one tile, one slab or
one class of one kernel.  The per-op tests can, but run at toy shapes that select other launch plans.  This module runs each
layer ALONE at the shapes of the step (and the conv family at B = 64, configs[4]'s per-GPU batch, where the slab budget of the
weight gradient changes), from seeded operands, and compares whole tensors with the same layer of the repository's oracle
evaluated in fp64 on the CPU (oracle/layer_fp64.py).

  convolutions   forward (`cconv2d_stats`, the step's form, with its statistics rows), data gradient, weight + bias gradient,
                 through the functional layer exactly as the network calls it (transposed / up / C1 split / single-output
                 stage), in both arithmetic modes ('bf16x6', 'f32').  Metric per element, in fp32 roundings of its absolute
                 sum:  e = max |got - ref64| / (2^-24 S).  Bound: e_hip <= K max(e_cpu32, 1), K = 16 (layer_fp64.K_BOUND has the reasoning), e_cpu32 = the fp32 CPU
                 oracle's e against the same fp64 reference; the bound has to stay below a tenth of the e of the smallest
                 fault of `layer_fp64.corruptions` on that layer and quantity (computed here, at the same batch).
                 The weight gradient runs twice: on its own, and with all 14 layers inside one deferred-reduce scope writing
                 into views of one flat buffer (the step's gradient bucket); the two must agree bit for bit.
  CBN            the 13 ComplexBatchNorm2d layers behind those convs, training mode, on the HIP conv's own output of an input
                 whose mean is several times its spread (so is the output's, and it is not the statistics' pivot): the encoder
                 ones through the two-consumer node (two cotangents), the decoder ones through the CBN + attention node with
                 the fused channel-attention pool — which also covers the 6 decoder attention blocks.
  attention      the 7 skip blocks as one batched set of launches (the network runs 7: skip_attention.0 .. .13; only
                 decoder_attention.12 / .13 are built and never run).
  LSTM           ComplexLSTM(128, 64, 2) at B = 32, S = 64 (the step's latent is [32, 2, 32, 128]) and S = 32.
  Tolerances of these three: the project's per-op ones against fp64 — 2e-5 of the tensor's max-abs forward, 1e-4 backward
  (LSTM + 1e-6 absolute).  Where the fp32 CPU oracle itself misses the tolerance, K times its error (recorded as such), with at most 8 times
  as many elements above the tolerance as it has; a tie of the spatial attention's channel maximum (gap below 1e-6) may be
  resolved either way (_check_block_with_ties).  The CBN references take the ReLU / leaky-ReLU branch from their own
  pre-activation, except at the elements within 1e-6 of zero (relative to the channel's largest value; a few in 10^6, counted
  and asserted), where it is read from the HIP path's output (layer_fp64._act_with_decisions).

Not covered, each because the entry point does not exist:
  1. dec6 statistics rows: the single-output stage has no CBN behind it and no statistics epilogue.
(The data gradient of enc0 IS run by the step — the initial CBN's parameters need it — and is covered.)

Every figure goes to layer_parity.json in the directory $DCS_PARITY_DIR names (default: parity_out/ in the repository, kept
out of git); a full run's file is committed as profiles/layer_parity.json.

The comparator itself is tested without a GPU (the `not gpu` tests below): on real layer geometries at batch 2 it has to
accept a second correct fp32 evaluation and reject each fault.
"""
import functools
import math
import time

import pytest
import torch

from oracle import layer_fp64 as L64
from oracle.layer_fp64 import ConvLayer
from _ragged_helpers import record

gpu = pytest.mark.gpu

# The network at [B, 256, 256] (c_network.py: encoder strides (2,2) x3 then (2,1) x4, decoder upsamples mirrored).
CONV_LAYERS = [
    ConvLayer('enc0', 256, 256, 1, 0, 8, 7, (2, 2), (1, 1), False),
    ConvLayer('enc1', 128, 128, 8, 0, 16, 7, (2, 2), (1, 1), False),
    ConvLayer('enc2', 64, 64, 16, 0, 32, 5, (2, 2), (1, 1), False),
    ConvLayer('enc3', 32, 32, 32, 0, 64, 5, (2, 1), (1, 1), False),
    ConvLayer('enc4', 16, 32, 64, 0, 128, 3, (2, 1), (1, 1), False),
    ConvLayer('enc5', 8, 32, 128, 0, 128, 3, (2, 1), (1, 1), False),
    ConvLayer('enc6', 4, 32, 128, 0, 128, 3, (2, 1), (1, 1), False),
    ConvLayer('dec0', 2, 32, 128, 128, 128, 3, (1, 1), (2, 1), True),
    ConvLayer('dec1', 4, 32, 128, 128, 128, 3, (1, 1), (2, 1), True),
    ConvLayer('dec2', 8, 32, 128, 128, 64, 3, (1, 1), (2, 1), True),
    ConvLayer('dec3', 16, 32, 64, 64, 32, 3, (1, 1), (2, 1), True),
    ConvLayer('dec4', 32, 32, 32, 32, 16, 3, (1, 1), (2, 2), True),
    ConvLayer('dec5', 64, 64, 16, 16, 8, 3, (1, 1), (2, 2), True),
    ConvLayer('dec6', 128, 128, 8, 8, 1, 3, (1, 1), (2, 2), True),
]
BY_NAME = {L.name: L for L in CONV_LAYERS}
# the 13 CBN layers on the conv outputs: (conv layer, channels, H, W, activation)
CBN_LAYERS = [(L.name, L.Cout, *L64.out_hw(L), 'lrelu' if L.transposed else 'relu') for L in CONV_LAYERS[:-1]]
# attention blocks the step runs: skip block i reads the output of encoder stage 6 - i; decoder block i the output of stage i
SKIP_BLOCKS = [(i, CONV_LAYERS[6 - i].Cout, *L64.out_hw(CONV_LAYERS[6 - i])) for i in range(7)]
DEC_BLOCKS = [(i, CONV_LAYERS[7 + i].Cout, *L64.out_hw(CONV_LAYERS[7 + i])) for i in range(6)]
TRAIN_B = 32
LSTM_S = 64                     # F7 * T7 of the latent [32, 2, 32, 128]
K = L64.K_BOUND

TOL_FWD, TOL_BWD = 2e-5, 1e-4


def _seed(L, B):
    return 1000 + 17 * CONV_LAYERS.index(L) + B


# ------------------------------------------------------------------------------------------------ the table (CPU)

def test_layer_table_is_the_networks():
    """The table above against the module list of a C_NETWORK instance at input [B, 256, 256]."""
    from dcsnet.config import config, hparams
    from dcsnet.c_network import C_NETWORK
    from dcsnet.complexLayers import ComplexBatchNorm2d, ComplexReLU
    net = C_NETWORK(config, dict(hparams), 0)
    Lyr = net.hparams['no_of_layers']
    assert Lyr == 7 and len(net.encoder) == 7 and len(net.decoder) == 7
    H, W, seen, outs = 256, 256, [], []
    for i, st in enumerate(net.encoder):
        conv, bn, act = st[0], st[1], st[2]
        assert isinstance(bn, ComplexBatchNorm2d) and isinstance(act, ComplexReLU)
        c = conv.conv_r
        assert conv.padding == (c.kernel_size[0] // 2,) * 2 and c.kernel_size[0] == c.kernel_size[1]
        L = ConvLayer(f'enc{i}', H, W, c.in_channels, 0, c.out_channels, c.kernel_size[0], tuple(conv.stride), (1, 1), False)
        seen.append(L)
        assert bn.num_features == L.Cout
        H, W = L64.out_hw(L)
        outs.append((L.Cout, H, W))
    assert (net.lstm.input_dim, net.lstm.rnn_units, net.lstm.real_lstm.num_layers, net.lstm.real_lstm.bidirectional) == (128, 64, 2, True)
    assert outs[-1] == (128, 2, 32) and LSTM_S == outs[-1][1] * outs[-1][2]
    C1 = outs[-1][0]
    for i, st in enumerate(net.decoder):
        convt = st if i == Lyr - 1 else st[0]
        c = convt.conv_tran_r
        C2, Hs, Ws = outs[Lyr - 1 - i]
        assert (Hs, Ws) == (H, W) and c.in_channels == C1 + C2 and convt.corr_padding == (1, 1)
        L = ConvLayer(f'dec{i}', H, W, C1, C2, c.out_channels, c.kernel_size[0], (1, 1), tuple(config.upsample_scale_factor[i]), True)
        seen.append(L)
        if i != Lyr - 1:
            assert st[1].num_features == L.Cout and type(st[2]).__name__ == 'ComplexLReLU'
        ca = net.skip_attention[2 * i]
        assert ca.fc[0].conv_r.in_channels == C2 and net.skip_attention[2 * i + 1].kernel_size == 7
        assert SKIP_BLOCKS[i] == (i, C2, Hs, Ws)
        H, W = L64.out_hw(L)
        if i != Lyr - 1:
            assert net.decoder_attention[2 * i].fc[0].conv_r.in_channels == L.Cout and DEC_BLOCKS[i] == (i, L.Cout, H, W)
        C1 = L.Cout
    assert seen == CONV_LAYERS
    assert (H, W, C1) == (256, 256, 1)
    assert [(n, C) for n, C, *_ in CBN_LAYERS] == [(L.name, L.Cout) for L in CONV_LAYERS[:-1]]
    assert CBN_LAYERS[0][1:4] == (8, 128, 128) and CBN_LAYERS[6][1:4] == (128, 2, 32)      # 524 288 x 8 down to 2 048 x 128 at B = 32


# ------------------------------------------------------------------------------------------------ the comparator (CPU)

def _alternative_fp32(L, case):
    """A second correct fp32 evaluation of the layer in another summation order than the oracle modules': the four real
    convolutions written out, each as the sum of two convolutions over complementary (checkerboard) halves of the taps."""
    leaf = lambda t: t.clone().requires_grad_(True)
    xr, xi = leaf(case['x'].real), leaf(case['x'].imag)
    p = {n: leaf(case[n]) for n in ('w_r', 'w_i', 'b_r', 'b_i')}
    m = ((torch.arange(L.k)[:, None] + torch.arange(L.k)[None, :]) % 2).float()
    zero = torch.zeros(L.Cout)
    re, im = L64.complex_conv_from_real(L, xr, xi, p['w_r'] * m, p['w_i'] * m, p['b_r'], p['b_i'])
    re2, im2 = L64.complex_conv_from_real(L, xr, xi, p['w_r'] * (1 - m), p['w_i'] * (1 - m), zero, zero)
    re, im = re + re2, im + im2
    (re * case['gy'].real + im * case['gy'].imag).sum().backward()
    return dict(y=torch.complex(re.detach(), im.detach()), gx=torch.complex(xr.grad, xi.grad), gw_r=p['w_r'].grad, gw_i=p['w_i'].grad,
                gb_r=p['b_r'].grad, gb_i=p['b_i'].grad)


@pytest.mark.parametrize('L', CONV_LAYERS, ids=[L.name for L in CONV_LAYERS])
def test_comparator_rejects_conv_faults(L):
    """Batch 2, the layer's real geometry: the clean fp32 results pass the bound, each fault fails it by more than ten times."""
    case = L64.conv_case(L, 2, _seed(L, 2))
    ref, ref32, S = L64.conv_reference(L, case, True), L64.conv_reference(L, case, False), L64.conv_abs_sums(L, case)
    # the written-out form IS the layer (it carries the faults and the absolute sums)
    d = lambda t: t.double()
    re, im = L64.complex_conv_from_real(L, d(case['x'].real), d(case['x'].imag), *(d(case[n]) for n in ('w_r', 'w_i', 'b_r', 'b_i')))
    assert float((torch.complex(re, im) - ref['y']).abs().max()) <= 1e-12 * float(ref['y'].abs().max())
    alt = _alternative_fp32(L, case)
    faults = L64.corruptions(L, case, ref)
    assert sorted(faults) == ['dgrad_tap', 'fwd_sign', 'fwd_tap', 'wgrad_row']
    for q in ('fwd', 'dgrad', 'wgrad'):
        e_cpu32 = L64.score(ref32, ref, S, q)[0]
        e_alt = L64.score(alt, ref, S, q)[0]
        print(f'{L.name} {q}: e_cpu32 {e_cpu32:.2f}, second fp32 evaluation {e_alt:.2f}, bound {L64.bound(e_cpu32):.1f}')
        assert e_cpu32 <= 16.0, (q, e_cpu32)              # the reference fp32 itself stays within a few roundings of |sum|
        assert L64.accepts(e_alt, e_cpu32), (q, e_alt, e_cpu32)
        for name, (fq, t) in faults.items():
            if fq != q:
                continue
            e_bad, at, _ = L64.score(t, ref, S, q)
            print(f'   {name}: e {e_bad:.3g} at {at}')
            assert not L64.accepts(e_bad, e_cpu32), (name, e_bad, e_cpu32)
            assert L64.bound(e_cpu32) <= 0.1 * e_bad, (name, e_bad, e_cpu32)


def _check_block(got, ref, ref32, abs_tol=0.0):
    """Section-3 comparator: {tensor: figures} and the list of misses.  Per tensor, error = max-abs distance to fp64 over the
    tensor's max-abs; limit = the project's tolerance.  Where the fp32 CPU oracle itself misses that tolerance (at these sizes:
    one channel-maximum decision out of 10^6 falls the other way in fp32 than in fp64, which moves single elements of g_x by
    O(1) and the parameter sums that contain them), the tensor is held to K times that error AND may have at most 8 times as
    many elements above the tolerance as the CPU oracle has: decisions flip at the same rate in any two fp32 evaluations, a
    faulty tile or slab is hundreds of elements."""
    rows, misses = {}, []

    def one(name, g, r, r32, tol):
        scale = float(r.abs().max())
        assert scale > 0, f'{name}: the reference is identically zero (a dead case checks nothing)'
        tol = tol + abs_tol / scale
        e, e32 = L64.rel_max(g, r), L64.rel_max(r32, r)
        row = dict(err=e, cpu32=e32, limit=tol, limit_is='tolerance')
        if e32 <= tol:
            ok = e <= tol
        else:
            n32 = int(((r32.to(r.dtype) - r).abs() > tol * scale).sum())
            n = int(((g.to(r.dtype) - r).abs() > tol * scale).sum())
            row.update(limit=K * e32, limit_is='K x cpu32, and at most 8 x as many elements above the tolerance as cpu32 has',
                       elements_above_tolerance=n, elements_above_tolerance_cpu32=n32, elements=r.numel())
            ok = e <= K * e32 and n <= 8 * n32
        rows[name] = row
        if not ok:
            misses.append((name, row))

    for key, r in ref.items():
        if key in ('z', 'undecided_activations'):
            continue
        if key in ('g_att', 'grads'):
            names = L64.ATT_NAMES if key == 'g_att' else sorted(r)
            seq = (lambda t: t) if key == 'g_att' else (lambda t: [t[n] for n in names])
            for n, g, rr, r32 in zip(names, seq(got[key]), seq(r), seq(ref32[key])):
                one(n, g, rr, r32, TOL_BWD)
        else:
            one(key, got[key], r, ref32[key], TOL_FWD if key in ('y', 'running_mean', 'running_covar') else TOL_BWD)
    if any(m[0] == 'gx' for m in misses):                 # the error map: where, and how near a channel-maximum tie
        d = (got['gx'].to(ref['gx'].dtype) - ref['gx']).abs()
        top = d.flatten().topk(min(8, d.numel()))
        rows['gx']['worst'] = []
        for v, i in zip(top.values.tolist(), top.indices.tolist()):
            at = L64.where(d.shape, i, False)
            rows['gx']['worst'].append(dict(at=list(at), err=v / float(ref['gx'].abs().max()),
                                            top2_gap=L64.top2_gap(ref['z'], at[0], at[2], at[3]) if 'z' in ref else None))
        print('gx error map:', rows['gx']['worst'])
    return rows, misses


def _check_block_with_ties(got, make_refs):
    """_check_block; where a tensor misses, or is only held by the K x cpu32 fallback, and the fp64 reference has pixels among
    the off elements of g_x whose channel maximum (spatial attention) is a tie to fp32 resolution (layer_fp64.undecided: at
    most 3 of them), the gradient there goes to one of two channels and either is exact: the kernels' result is compared with
    the reference under the resolutions of those ties, and one under which EVERY tensor meets its plain tolerance is taken."""
    import itertools
    ref, ref32 = make_refs(None)
    rows, misses = _check_block(got, ref, ref32)
    fallback = [n for n, r in rows.items() if r.get('limit_is', 'tolerance') != 'tolerance']
    ties = []
    if (misses or fallback) and 'z' in ref:               # ties at the pixels where g_x is off (a map of 10^6 pixels has a few more)
        off = (got['gx'].to(ref['gx'].dtype) - ref['gx']).abs() > TOL_BWD * float(ref['gx'].abs().max())
        pixels = {(b, h, w) for b, _, h, w in off.nonzero().tolist()[:64]}
        ties = [t for t in L64.undecided(ref['z']) if (t[1], t[2], t[3]) in pixels]
    if 1 <= len(ties) <= 3:
        for n in range(1, len(ties) + 1):
            for choice in itertools.combinations(ties, n):
                rows2, misses2 = _check_block(got, *make_refs(list(choice)))
                if not misses2 and all(r.get('limit_is', 'tolerance') == 'tolerance' for r in rows2.values()):
                    rows2['channel_maximum_ties'] = dict(pixels=[list(t) for t in ties], matched_with_runner_up_at=[list(t) for t in choice],
                                                         err_with_first_choice={k_: rows[k_]['err'] for k_ in set(fallback) | {m[0] for m in misses}})
                    return rows2, []
    return rows, misses


def _offset_input(C, B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    mean = L64.randc(g, 1, C, 1, 1) * 1.5 + (2.0 - 1.0j)
    return (L64.randc(g, B, C, H, W) * 0.4 + mean).to(torch.complex64), L64.randc(g, B, C, H, W)


def _bn_params(C, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(C, 3, generator=g) * 0.2 + torch.tensor([1.3, 1.1, 0.1])
    return w, torch.randn(C, 2, generator=g) * 0.5


@pytest.mark.parametrize('name,C,H,W,act', CBN_LAYERS, ids=[c[0] for c in CBN_LAYERS])
def test_comparator_rejects_a_cbn_backward_that_drops_its_last_pass(name, C, H, W, act):
    """Batch 2: a CBN backward whose reduction sums miss the last rows_per_iter pixels (cbn_geom.h: 256 / (C / 2)) is rejected,
    the fp32 CPU result accepted.  (The parameter gradients catch it; in g_x alone the fault is 1/P of a sum and sits below
    1e-4 of the tensor's max-abs at these sizes.)"""
    x, g = _offset_input(C, 2, H, W, 77 + C)
    bn = _bn_params(C, C)
    ref, ref32 = L64.block_reference(x, g, True, bn, act), L64.block_reference(x, g, False, bn, act)
    rows, misses = _check_block(ref32, ref, ref32)
    assert not misses, misses
    f32 = lambda t: t.to(torch.complex64 if t.is_complex() else torch.float32)
    bad = {k: f32(v) for k, v in L64.block_reference(x, g, True, bn, act, drop_last=256 // (C // 2)).items()}
    rows, misses = _check_block(bad, ref, ref32)
    print(name, {k: f'{v["err"]:.2e}' for k, v in rows.items()})
    assert misses and {m[0] for m in misses} & {'g_weight', 'g_bias', 'gx'}, rows
    assert rows['y']['err'] <= 1e-6                    # only the backward was touched


@pytest.mark.parametrize('name,C,H,W,act', CBN_LAYERS, ids=[c[0] for c in CBN_LAYERS])
def test_comparator_rejects_a_zeroed_tile_of_a_cbn_output(name, C, H, W, act):
    """Batch 2: a CBN + activation output with one 16x16 tile of every channel of the last sample written as zeros (a skipped
    tile, a tail not applied) is rejected although the reference reads the branch of its undecided elements from that very
    output; the honest fp32 output is accepted under the same rule, and only a few elements are undecided."""
    x, g = _offset_input(C, 2, H, W, 78 + C)
    bn = _bn_params(C, C)
    good = L64.block_reference(x, g, False, bn, act)
    for zeroed in (False, True):
        got = {k_: (v.clone() if torch.is_tensor(v) else v) for k_, v in good.items()}
        if zeroed:
            got['y'][-1, :, max(H - 16, 0):, max(W - 16, 0):] = 0
        ref = L64.block_reference(x, g, True, bn, act, decided=got['y'])
        ref32 = L64.block_reference(x, g, False, bn, act, decided=got['y'])
        assert ref['undecided_activations'] <= 8 + 2e-5 * 2 * x.numel(), ref['undecided_activations']
        rows, misses = _check_block(got, ref, ref32)
        print(name, 'zeroed tile' if zeroed else 'clean', {k_: f'{v["err"]:.2e}' for k_, v in rows.items()})
        assert ('y' in {m[0] for m in misses}) == zeroed and (zeroed or not misses), (zeroed, misses)


def test_bound_admits_one_fp32_accumulator_per_output():
    """The reasoning behind K (layer_fp64.K_BOUND): a correct evaluation with ONE fp32 accumulator per output — an MFMA tile
    along K — reads e above the issue's starting K = 4 and far below K = 16 at the floor of the bound (e_cpu32 <= 1)."""
    e_max, e_rms = L64.single_chain_e(400, 1 << 20)
    print(f'one fp32 chain of 400 terms, 2^20 outputs: e max {e_max:.2f}, rms {e_rms:.2f}')
    assert 4.0 < e_max <= 0.5 * L64.bound(1.0) and 0.3 < e_rms < 0.7, (e_max, e_rms)


# ------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from dcsnet import _lib
    _lib.load()
    threads = L64.set_threads()
    yield torch.device('cuda:0')
    torch.set_num_threads(threads)


_record = functools.partial(record, 'layer_parity.json')     # figures -> $DCS_PARITY_DIR/layer_parity.json (default parity_out/)


_WGRAD_REF = {}          # (layer, B) -> weight-gradient reference, absolute sums, e_cpu32, smallest fault (small tensors)


def _conv_refs(L, B):
    case = L64.conv_case(L, B, _seed(L, B))
    ref = L64.conv_reference(L, case, True)
    S = L64.conv_abs_sums(L, case)
    ref32 = L64.conv_reference(L, case, False)
    e_cpu32 = {q: L64.score(ref32, ref, S, q)[0] for q in L64.QUANTITIES}
    del ref32
    faults = L64.corruption_scores(L, case, ref, S)
    smallest = {q: L64.smallest_corruption(faults, q) for q in L64.QUANTITIES}
    keys = L64.QUANTITIES['wgrad']
    _WGRAD_REF[(L.name, B)] = (({k: ref[k] for k in keys}, {k: S[k] for k in keys}), e_cpu32['wgrad'], smallest['wgrad'])
    return case, ref, S, e_cpu32, faults, smallest


def _cplx(t):
    """float [B,H,W,C,2] on the GPU -> complex [B,C,H,W] on the CPU."""
    return torch.view_as_complex(t.detach().cpu().contiguous()).permute(0, 3, 1, 2)


def _operands(L, case, dev, sinks=None):
    """The layer's operands on the GPU: channels-last x1 (x2), cotangent, and the four parameters as leaves — with `sinks`
    (four views of a flat buffer) registered as their gradient destinations the way dp.FlatBucket does."""
    from dcsnet import ops
    x = case['x']
    x1 = ops.to_nhwc(x[:, :L.C1].to(dev))
    x2 = ops.to_nhwc(x[:, L.C1:].to(dev)) if L.C2 else None
    gy = ops.to_nhwc(case['gy'].to(dev))
    p = [case[n].to(dev).requires_grad_(True) for n in ('w_r', 'w_i', 'b_r', 'b_i')]
    if sinks is not None:
        for q, s in zip(p, sinks):
            q.grad = s
            q._dcs_grad_sink = s
    return x1, x2, gy, p


def _forward(L, x1, x2, p):
    """The layer as C_NETWORK.forward calls it in training: (y, statistics rows or None)."""
    from dcsnet import functional as F
    k = (L.k, L.k)
    if L.Cout == 1:
        return F.cconv_single_output(x1, x2, *p, k, (L.k - 1 - L.k // 2,) * 2, L.up), None
    pad = (L.k - 1 - L.k // 2,) * 2 if L.transposed else (L.k // 2,) * 2
    return F.cconv2d_with_stats(x1, x2, *p, L.transposed, k, L.stride, pad, L.up)


def _hip_conv(L, case, dev):
    x1, x2, gy, p = _operands(L, case, dev)
    x1.requires_grad_(True)
    if x2 is not None:
        x2.requires_grad_(True)
    y, stat = _forward(L, x1, x2, p)
    g = torch.autograd.grad(y, [x1] + ([x2] if x2 is not None else []) + p, gy)
    gx = torch.cat([_cplx(t) for t in g[:-4]], dim=1)
    got = dict(y=_cplx(y), gx=gx, **{n: t.detach().cpu() for n, t in zip(('gw_r', 'gw_i', 'gb_r', 'gb_i'), g[-4:])})
    mom = None if stat is None else stat[0][:, :, :stat[1]].double().sum(dim=2).cpu()
    return got, mom


def _moments(ref, case):
    """fp64 moments of the fp64 output about the effective bias (b_r - b_i, b_r + b_i): [Cout, 5]."""
    b_r, b_i = case['b_r'].double(), case['b_i'].double()
    re = ref['y'].real - (b_r - b_i)[None, :, None, None]
    im = ref['y'].imag - (b_r + b_i)[None, :, None, None]
    s = lambda t: t.sum(dim=(0, 2, 3))
    return torch.stack((s(re), s(im), s(re * re), s(im * im), s(re * im)), dim=1)


@gpu
@pytest.mark.parametrize('L', CONV_LAYERS, ids=[L.name for L in CONV_LAYERS])
@pytest.mark.parametrize('B', [32, 64])
def test_conv_layer_against_fp64(dev, B, L):
    from dcsnet import ops
    t0 = time.time()
    case, ref, S, e_cpu32, faults, smallest = _conv_refs(L, B)
    t_ref = time.time() - t0
    want_mom = _moments(ref, case)
    default = ops.conv_precision()
    misses = []
    for mode in ('bf16x6', 'f32'):
        ops.set_conv_precision(mode)
        try:
            got, mom = _hip_conv(L, case, dev)
        finally:
            ops.set_conv_precision(default)
        for q in L64.QUANTITIES:
            e_hip, at, n_loose = L64.score(got, ref, S, q)
            lim = L64.bound(e_cpu32[q])
            print(f'{L.name} B={B} {mode} {q}: e_hip {e_hip:.2f} at {at}, e_cpu32 {e_cpu32[q]:.2f}, bound {lim:.1f}, smallest fault {smallest[q]:.3g}')
            _record((f'B{B}', L.name, q, mode), dict(e_hip=e_hip, worst_at=[str(a) for a in at], elements_above_4=n_loose, elements=sum(ref[k_].numel() * (2 if ref[k_].is_complex() else 1) for k_ in L64.QUANTITIES[q]), e_cpu32=e_cpu32[q], bound=lim,
                                                    smallest_fault=smallest[q], faults={n: e for n, e in faults.items() if n.startswith(q)}))
            if not e_hip <= lim:
                misses.append((mode, q, e_hip, at, lim))
            if not lim <= 0.1 * smallest[q]:
                misses.append((mode, q, 'bound above a tenth of the smallest fault', lim, smallest[q]))
        if L.Cout == 1:
            assert mom is None                      # (the single-output stage: no statistics epilogue — module docstring)
        else:
            assert mom is not None, 'this geometry must take the statistics epilogue'
            err = float((mom - want_mom).abs().max()) / float(want_mom.abs().max())
            per_col = ((mom - want_mom).abs().amax(dim=0) / want_mom.abs().amax(dim=0)).tolist()
            _record((f'B{B}', L.name, 'statistics_rows', mode), dict(err=err, tolerance=1e-4, per_moment=per_col))
            if not err <= 1e-4:
                misses.append((mode, 'statistics rows', err))
    _record((f'B{B}', L.name, 'seconds'), dict(fp64_references=t_ref, whole_test=time.time() - t0))
    assert not misses, misses


@gpu
@pytest.mark.parametrize('mode', ['bf16x6', 'f32'])
@pytest.mark.parametrize('B', [32, 64])
def test_weight_gradients_in_one_deferred_scope(dev, B, mode):
    """All 14 layers' weight gradients inside ONE wgrad_defer_begin / wgrad_defer_flush scope, every destination a view of one flat
    buffer (how the step batches its slab reductions), in the backward's order: bit-identical to the same launches on their
    own, and within the bound of fp64."""
    from dcsnet import ops
    default = ops.conv_precision()
    ops.set_conv_precision(mode)
    misses = []
    try:
        sizes = [(L, [math.prod(s) for s in (((L.C1 + L.C2, L.Cout, L.k, L.k) if L.transposed else (L.Cout, L.C1 + L.C2, L.k, L.k)),) * 2]
                  + [L.Cout, L.Cout]) for L in CONV_LAYERS]
        flat = torch.zeros(sum(sum(n) for _, n in sizes), device=dev)
        from dcsnet import functional as F
        own, views, graphs, o = {}, {}, [], 0
        hits = F.sink_hits
        for L, ns in sizes:
            case = L64.conv_case(L, B, _seed(L, B))
            x1, x2, gy, p = _operands(L, case, dev)
            own[L.name] = torch.autograd.grad(_forward(L, x1, x2, p)[0], p, gy)
            v = []
            for n, q in zip(ns, p):
                v.append(flat[o:o + n].view(q.shape))
                o += n
            views[L.name] = v
            x1, x2, gy, p = _operands(L, case, dev, sinks=v)
            graphs.append((_forward(L, x1, x2, p)[0], gy, p))
        assert F.sink_hits - hits == 4 * len(CONV_LAYERS)      # every parameter's gradient goes to its view of the flat buffer
        ops.wgrad_defer_begin()
        try:
            for y, gy, p in reversed(graphs):
                y.backward(gy)
            # one recorded slab reduction per layer that has one (dec6's own kernel reduces by itself): nothing ran immediately
            assert len(ops.WGRAD_DEFER.keep) == len(CONV_LAYERS) - 1, len(ops.WGRAD_DEFER.keep)
        finally:
            ops.wgrad_defer_flush()
        torch.cuda.synchronize()
        for (L, _), (y, gy, p) in zip(sizes, graphs):
            for n, a, b, q in zip(('gw_r', 'gw_i', 'gb_r', 'gb_i'), own[L.name], views[L.name], p):
                assert q.grad is b                                   # written in place, nothing handed back to autograd
                if not torch.equal(a, b):
                    misses.append((L.name, n, 'deferred != immediate', float((a - b).abs().max())))
            if (L.name, B) not in _WGRAD_REF:                        # (run on its own: the references were not made yet)
                _conv_refs(L, B)
            (ref, S), e_cpu32, smallest = _WGRAD_REF[(L.name, B)]
            got = {n: b.detach().cpu() for n, b in zip(('gw_r', 'gw_i', 'gb_r', 'gb_i'), views[L.name])}
            e_hip, at, _ = L64.score(got, ref, S, 'wgrad')
            _record((f'B{B}', L.name, 'wgrad_deferred', mode), dict(e_hip=e_hip, e_cpu32=e_cpu32, bound=L64.bound(e_cpu32), smallest_fault=smallest))
            if not e_hip <= L64.bound(e_cpu32):
                misses.append((L.name, 'wgrad deferred', e_hip, at, L64.bound(e_cpu32)))
    finally:
        ops.set_conv_precision(default)
    assert not misses, misses


def _sqrt2_covar(C, dev):
    rc = torch.zeros(C, 3, device=dev)
    rc[:, :2] = math.sqrt(2.0)
    return rc


@gpu
@pytest.mark.parametrize('name,C,H,W,act', CBN_LAYERS, ids=[c[0] for c in CBN_LAYERS])
def test_cbn_layer_against_fp64(dev, name, C, H, W, act):
    """The CBN behind each conv at B = 32, fed by the HIP conv's own output and statistics rows.  Encoder stages: the
    two-consumer node (cbn_two: two cotangents summed inside the backward kernels).  Decoder stages: the CBN + attention node
    (apply pass that pools for the channel attention, attention backward feeding the CBN backward its pool term)."""
    from dcsnet import ops, functional as F
    t0 = time.time()
    L = BY_NAME[name]
    B = TRAIN_B
    g = torch.Generator().manual_seed(500 + C + H)
    # input mean several times its spread: the conv output's per-channel mean is mu_x * sum(w) + bias, its spread |w| * spread_x
    case = L64.conv_case(L, B, 300 + _seed(L, B), offset=(1.0 - 0.7j), spread=0.08)
    x1, x2, _, p = _operands(L, case, dev)
    with torch.no_grad():
        y, stat = _forward(L, x1, x2, p)
    assert stat is not None
    xc = _cplx(y)
    ratio = (torch.complex(xc.real.mean((0, 2, 3)), xc.imag.mean((0, 2, 3))).abs()
             / (xc.real.var((0, 2, 3)) + xc.imag.var((0, 2, 3))).sqrt())
    assert float(ratio.median()) >= 2.0, ratio        # measured 2.4 .. 7 (maps of 2 - 4 rows are mostly border)
    bn = _bn_params(C, C + 1)
    w, b = (t.to(dev).requires_grad_(True) for t in bn)
    rm, rc = torch.zeros(C, 2, device=dev), _sqrt2_covar(C, dev)
    yl = y.detach().requires_grad_(True)
    ga, gb = L64.randc(g, B, C, H, W), L64.randc(g, B, C, H, W)
    att = None
    if act == 'relu':
        a, a2 = F.cbn_two(yl, w, b, rm, rc, 1e-5, 0.1, True, F.ACT_RELU, 0.0, 0, stat)
        assert a2.data_ptr() == a.data_ptr()
        decided = _cplx(a)
        grads = torch.autograd.grad([a, a2], [yl, w, b], [ops.to_nhwc(ga.to(dev)), ops.to_nhwc(gb.to(dev))])
        g_out = ga.to(torch.complex128) + gb.to(torch.complex128)
    else:
        att = L64.attention_params(C, 900 + C)
        ap = [t.to(dev).requires_grad_(True) for t in att]
        assert ops.FUSE_APPLY_POOL
        a = F.cbn_attention(yl, w, b, rm, rc, 1e-5, 0.1, True, F.ACT_LRELU, *ap, 7, 0.0, 0, stat)
        # the node's saved activation (CBN + leaky ReLU output): the saved tensor that IS that activation, found by value
        a_again = ops.cbn(y, w.detach(), b.detach(), torch.zeros_like(rm), _sqrt2_covar(C, dev), 1e-5, 0.1, True, F.ACT_LRELU, stat=stat)[0]
        same = [t for t in a.grad_fn.saved_tensors
                if t is not None and t.shape == a_again.shape and float((t - a_again).abs().max()) <= 1e-5 * float(a_again.abs().max())]
        assert len(same) == 1, len(same)
        decided = _cplx(same[0])
        grads = torch.autograd.grad(a, [yl, w, b] + ap, ops.to_nhwc(ga.to(dev)))
        g_out = ga
    got = dict(y=_cplx(a), gx=_cplx(grads[0]), running_mean=torch.view_as_complex(rm.cpu()), running_covar=rc.cpu(),
               g_weight=grads[1].cpu(), g_bias=grads[2].cpu())
    if att is not None:
        got['g_att'] = [t.cpu() for t in grads[3:]]
    seen = {}

    def make_refs(choice):
        refs = tuple(L64.block_reference(xc, g_out, wide, bn, act, att, decided=decided, max_choice=choice) for wide in (True, False))
        seen['undecided'] = refs[0]['undecided_activations']
        return refs

    rows, misses = _check_block_with_ties(got, make_refs)
    for k_, v in rows.items():
        print(f'cbn {name} {k_}: {v}')
    # the kernels' branch was taken at the undecided elements only: a few in 10^6
    n_und = seen['undecided']
    assert n_und <= 8 + 2e-5 * 2 * xc.numel(), (n_und, xc.numel())
    _record(('cbn' if att is None else 'cbn_attention', name), dict(tensors=rows, pixels=B * H * W, channels=C, undecided_activations=n_und,
            median_mean_over_spread=float(ratio.median()), seconds=time.time() - t0))
    assert not misses, misses


@gpu
def test_skip_attention_blocks_against_fp64(dev):
    """The 7 skip attention blocks of the step at B = 32 through the batched entry points (one set of launches forward, one
    backward), on ReLU outputs (exact zeros: ties in the channel maximum), g_x and all six parameter gradients per block."""
    from dcsnet import ops, functional as F
    t0 = time.time()
    B = TRAIN_B
    g = torch.Generator().manual_seed(41)
    xs, gs, params = [], [], []
    for i, C, H, W in SKIP_BLOCKS:
        xs.append(L64.cpt.complex_relu(L64.randc(g, B, C, H, W) * 0.7 + (0.2 + 0.1j)))
        gs.append(L64.randc(g, B, C, H, W))
        params.append(L64.attention_params(C, 700 + i))
    xd = [ops.to_nhwc(x.to(dev)).requires_grad_(True) for x in xs]
    pd = [[t.to(dev).requires_grad_(True) for t in pr] for pr in params]
    outs = F.attention_blocks(xd, pd, 7)
    grads = torch.autograd.grad(outs, xd + [t for pr in pd for t in pr], [ops.to_nhwc(t.to(dev)) for t in gs])
    misses = []
    for (i, C, H, W), x, gg, pr in zip(SKIP_BLOCKS, xs, gs, params):
        got = dict(y=_cplx(outs[i]), gx=_cplx(grads[i]), g_att=[t.cpu() for t in grads[7 + 6 * i:13 + 6 * i]])
        rows, m = _check_block_with_ties(got, lambda choice: tuple(
            L64.block_reference(x, gg, wide, attention=pr, max_choice=choice) for wide in (True, False)))
        print(f'skip attention {i}: {rows}')
        _record(('skip_attention', f'block{i}'), dict(tensors=rows, shape=[B, C, H, W]))
        misses += [(i,) + t for t in m]
    _record(('skip_attention', 'seconds'), time.time() - t0)
    assert not misses, misses


@gpu
@pytest.mark.parametrize('S', [32, LSTM_S])
def test_complex_lstm_against_fp64(dev, S):
    from dcsnet.c_network import ComplexLSTM
    from oracle.cnet_oracle import ComplexLSTM as OracleLSTM
    t0 = time.time()
    torch.manual_seed(S)
    state = OracleLSTM(128, 64, 2, True).state_dict()
    g = torch.Generator().manual_seed(S + 1)
    z, g_out = (L64.randc(g, TRAIN_B, S, 128) * 0.7).to(torch.complex64), L64.randc(g, TRAIN_B, S, 128)
    mod = ComplexLSTM(128, 64, 2, True, True)
    mod.load_state_dict(state)
    mod = mod.to(dev)
    zd = z.to(dev).requires_grad_(True)
    out = mod(zd)
    (torch.view_as_real(out) * torch.view_as_real(g_out.to(dev))).sum().backward()
    got = dict(y=out.detach().cpu(), gz=zd.grad.cpu(), grads={n: q.grad.cpu() for n, q in mod.named_parameters()})
    ref, ref32 = L64.lstm_reference(state, z, g_out, True), L64.lstm_reference(state, z, g_out, False)
    rows, misses = _check_block(got, ref, ref32, abs_tol=1e-6)
    print(f'lstm S={S}: {rows}')
    _record(('lstm', f'B{TRAIN_B}_S{S}'), dict(tensors=rows, seconds=time.time() - t0))
    assert not misses, misses
