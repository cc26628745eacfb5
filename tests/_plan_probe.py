"""The geometry table of tests/test_infer_epilogue.py, the operands / launch of one row, and — run as a program — the plan probe:

    DCS_MFMA_TRACE=1 python tests/_plan_probe.py

launches every row (tier A's table, then tier C's chip-filling shapes) once with folded coefficients in the default arithmetic
mode and prints `ROW <name>` to stderr before each launch, so the `[mfma] ... cand ... S .../... coef 1` line the library prints for that launch (a C static read once per
process: hence a process of its own, like tests/_switch_probe.py) follows the row it belongs to.  The parent parses stderr.

Every row is one way into one of the seven copies of the folded epilogue (conv + bias -> eval-mode CBN coefficients ->
activation); `path` names the item of the coverage contract it is claimed for:

  P1  cconv_mfma_kernel, unsliced, one K wave (cand 0-3), one class
  P2  ... with folded-upsample classes and a cat source (two and four classes, a class smaller than the tile, ragged W)
  P3  K split over the waves of a tile: cand 4, 5 (32-pixel tiles), cand 7 (64 x 64, two waves: plain and classes), cand 8 (enc1's rows)
  P4  K slices + splitk_reduce_kernel (plain and classes)
  P5  the 16-column kernel (Cout = 8): four fused classes, one class, Cin % 16 == 0 and Cin = 8 (its fp32 form)
  P6  conv_enc0.hip (no [mfma] line)
  P7  conv_direct.hip (Cin or Cout no multiple of 8; no [mfma] line)
  P8  conv_ring.hip under DCS_CONV_RING=1 / DCS_RING_MIN_WG=1 (cand 10)

make_plan (csrc/conv_mfma.hip) keeps a tile unsliced and un-split only from 512 useful workgroups on (or where the whole K
is one chunk), so the P1 / P2 / cand-7 rows sit at the size cap of 2^20 complex outputs; 24 input channels (no multiple of 16)
keep a 64 x 64 tile on the classic one-wave form, which `coef` launches otherwise trade for cand 7.  No strided forward
geometry fits the ring kernel's LDS budget (tests/test_hip_ring.py: "forward falls back"), so P8's second row is a plain
stride-1 conv beside the class row.
"""
import contextlib
import math
import os
import sys
from collections import namedtuple

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'dcs-net_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from oracle import layer_fp64 as L64   # noqa: E402
from test_hip_ring import _ring as ring   # noqa: E402  (DCS_CONV_RING / DCS_RING_MIN_WG for the calls inside the block; read per call)

EPS = 1e-5
MAX_OUTPUTS = 1 << 20
# geometry (oracle.layer_fp64.ConvLayer), batch, activations run in tier A (first: the network's own for this kind of layer),
# path of the contract, claimed plan in the default mode: candidates, K-sliced, classes; ring: run under the ring switches
Row = namedtuple('Row', 'L B acts path cands sliced ncls ring')


def _row(name, B, H, W, C1, C2, Cout, k, stride, up, transposed, acts, path, cands=(), sliced=False, ncls=1, ring=False):
    return Row(L64.ConvLayer(name, H, W, C1, C2, Cout, k, stride, up, transposed), B, acts, path, tuple(cands), sliced, ncls, ring)


E, D = ('relu',), ('lrelu',)
ROWS = {r.L.name: r for r in [
    _row('p1_16to16_k5s22', 4, 256, 256, 16, 0, 16, 5, (2, 2), (1, 1), False, E, 'P1', (3,)),
    _row('p1_24to32_k5s22', 2, 128, 512, 24, 0, 32, 5, (2, 2), (1, 1), False, ('relu', 'none'), 'P1', (2,)),
    _row('p2_up21_16p8to24_w250', 2, 40, 250, 16, 8, 24, 3, (1, 1), (2, 1), True, D, 'P2', (2,), ncls=2),
    _row('p2_up22_8p16to24_w40', 4, 56, 40, 8, 16, 24, 3, (1, 1), (2, 2), True, ('lrelu', 'none'), 'P2', (2,), ncls=4),
    _row('p2_up22_16p16to16', 4, 64, 64, 16, 16, 16, 3, (1, 1), (2, 2), True, D, 'P2', (3,), ncls=4),
    _row('p2_up21_class_below_tile', 140, 3, 40, 16, 8, 24, 3, (1, 1), (2, 1), True, D, 'P2', (2,), ncls=2),
    _row('p3_cand4_64to128', 12, 16, 32, 64, 0, 128, 3, (2, 1), (1, 1), False, E, 'P3', (4,)),
    _row('p3_cand5_1x1_128to128', 2, 4, 32, 128, 0, 128, 1, (1, 1), (1, 1), False, ('relu', 'none'), 'P3', (5,)),
    _row('p3_cand7_16to32', 2, 256, 256, 16, 0, 32, 5, (2, 2), (1, 1), False, E, 'P3', (7, 9)),
    _row('p3_cand7_classes_32p32to32', 4, 64, 64, 32, 32, 32, 3, (1, 1), (2, 1), True, D, 'P3', (7, 9), ncls=2),
    _row('p3_enc1_rows_8to16_k7', 2, 250, 500, 8, 0, 16, 7, (2, 2), (1, 1), False, E, 'P3', (6, 8)),
    _row('p4_plain_128to128', 2, 8, 32, 128, 0, 128, 3, (2, 1), (1, 1), False, ('relu', 'none'), 'P4', (0, 1, 2, 3), sliced=True),
    _row('p4_classes_dec0', 2, 2, 32, 128, 128, 128, 3, (1, 1), (2, 1), True, D, 'P4', (0, 1, 2, 3), sliced=True, ncls=2),
    _row('p5_dec5_ragged', 2, 24, 20, 16, 16, 8, 3, (1, 1), (2, 2), True, ('lrelu', 'none'), 'P5', (3,), ncls=4),
    _row('p5_tiny_tiles_outside', 1, 5, 7, 16, 16, 8, 3, (1, 1), (2, 2), True, D, 'P5', (3,), ncls=4),
    _row('p5_one_class_16to8', 2, 19, 37, 16, 0, 8, 3, (1, 1), (1, 1), False, ('relu', 'sigmoid'), 'P5', (3,)),
    _row('p5_cin8_four_classes', 2, 9, 21, 8, 0, 8, 3, (1, 1), (2, 2), True, D, 'P5', (3,), ncls=4),
    _row('p5_cin8_one_class_k5s22', 2, 20, 30, 8, 0, 8, 5, (2, 2), (1, 1), False, E, 'P5', (3,)),
    _row('p6_enc0_whole_tiles', 2, 32, 128, 1, 0, 8, 7, (2, 2), (1, 1), False, ('relu', 'none'), 'P6'),
    _row('p6_enc0_ragged', 3, 18, 22, 1, 0, 8, 7, (2, 2), (1, 1), False, ('relu', 'lrelu'), 'P6'),
    _row('p7_direct_12to8', 2, 12, 20, 12, 0, 8, 3, (1, 1), (1, 1), False, ('relu', 'none'), 'P7'),
    _row('p7_direct_4p4to6_up22', 2, 7, 9, 4, 4, 6, 3, (1, 1), (2, 2), True, D, 'P7'),
    _row('p8_ring_classes_dec1', 8, 4, 32, 128, 128, 128, 3, (1, 1), (2, 1), True, D, 'P8', (10,), ncls=2, ring=True),
    _row('p8_ring_plain_64to32', 2, 16, 32, 64, 0, 32, 3, (1, 1), (1, 1), False, ('relu', 'none'), 'P8', (10,), ring=True),
]}
PATHS = ('P1', 'P2', 'P3', 'P4', 'P5', 'P6', 'P7', 'P8')
# Tier C: one shape per MFMA epilogue copy, each with >= 768 workgroups (make_plan's min_blocks: several on every CU, so the
# epilogue of one workgroup runs while others' bf16 MFMAs are in flight) — and one K-sliced row, which by construction does
# not fill the chip (a plan is sliced BECAUSE it has too few tiles; its reduce kernel has no MFMA beside it).  The strided
# enc5 shape cannot run on the ring kernel, so the ring row is the two-class decoder shape.
CHIP = {r.L.name: r for r in [
    _row('chip_enc5_128to128', 16, 8, 250, 128, 0, 128, 3, (2, 1), (1, 1), False, E, 'P3', (7, 9)),
    _row('chip_dec5_16col_four_classes', 4, 64, 500, 16, 16, 8, 3, (1, 1), (2, 2), True, D, 'P5', (3,), ncls=4),
    _row('chip_enc0', 4, 256, 2000, 1, 0, 8, 7, (2, 2), (1, 1), False, E, 'P6'),
    _row('chip_dec2_two_classes', 16, 8, 250, 128, 128, 64, 3, (1, 1), (2, 1), True, D, 'P2', (0, 1, 2, 3), ncls=2),
    _row('chip_dec2_two_classes_ring', 16, 8, 250, 128, 128, 64, 3, (1, 1), (2, 1), True, D, 'P8', (10,), ncls=2, ring=True),
    _row('chip_enc5_sliced', 2, 8, 32, 128, 0, 128, 3, (2, 1), (1, 1), False, E, 'P4', (0, 1, 2, 3), sliced=True),
]}
ALL = dict(ROWS, **CHIP)


def n_outputs(row):
    Ho, Wo = L64.out_hw(row.L)
    return row.B * Ho * Wo * row.L.Cout


def seed_of(name):
    return 100 + list(ALL).index(name)


def bf16_representable(t):
    return t.to(torch.bfloat16).to(t.dtype) if not t.is_complex() else torch.complex(bf16_representable(t.real), bf16_representable(t.imag))


def six_bit_grid(w_r, w_i):
    """Both weights rounded to multiples of one power of two with |multiple| <= 63: bf16-representable, and so is every sum
    of up to four of them (<= 252 < 2^8) — the folded-upsample sub-kernels are such sums of taps (conv_pack.hip), and the
    packer rounds THEM to bf16 in mode 'bf16'."""
    top = max(float(w_r.abs().max()), float(w_i.abs().max()))
    q = 2.0 ** math.floor(math.log2(63.0 / top))
    return torch.round(w_r * q) / q, torch.round(w_i * q) / q


def row_case(name, B=None, rounded=False):
    """(case, state): layer_fp64.conv_case of the row (batch B, default the row's) and its correlated eval-mode CBN state.
    rounded: operands that mode 'bf16' multiplies exactly — bf16-representable activations, weights on six_bit_grid."""
    row = ALL[name]
    case = L64.conv_case(row.L, row.B if B is None else B, seed_of(name))
    if rounded:
        case['x'] = bf16_representable(case['x'])
        case['w_r'], case['w_i'] = six_bit_grid(case['w_r'], case['w_i'])
    return case, L64.eval_cbn_state(row.L.Cout, 1000 + seed_of(name))


def act_code(act):
    from dcsnet import ops
    return {'none': ops.ACT_NONE, 'relu': ops.ACT_RELU, 'lrelu': ops.ACT_LRELU, 'sigmoid': ops.ACT_SIGMOID}[act]


def device_operands(row, case, dev, dtype=torch.float32):
    """x1, x2 (channels-last, `dtype`), packed weight and bias under the CURRENT arithmetic mode, and the call's geometry."""
    from dcsnet import ops
    L = row.L
    x = ops.to_nhwc(case['x'].to(dev))
    x1 = x[:, :, :, :L.C1].contiguous().to(dtype)
    x2 = x[:, :, :, L.C1:].contiguous().to(dtype) if L.C2 else None
    wp, bias = ops.pack_conv_weight(*(case[n].to(dev) for n in ('w_r', 'w_i', 'b_r', 'b_i')), L.transposed, tuple(L.up))
    return x1, x2, wp, bias, ((L.k, L.k), tuple(L.stride), (L.k // 2, L.k // 2), tuple(L.up))


def launch(row, operands, act, coef):
    """ops.cconv2d of the row (under the ring switches where the row asks for them)."""
    from dcsnet import ops
    x1, x2, wp, bias, geo = operands
    with (ring(True) if row.ring else contextlib.nullcontext()):
        return ops.cconv2d(x1, x2, wp, bias, *geo, act_code(act), coef=coef)


def main():
    from dcsnet import _lib
    _lib.load()
    dev = torch.device('cuda:0')
    for name, row in ALL.items():
        case, state = row_case(name)
        coef = L64.eval_coef_reference(state, EPS, wide=False).to(dev)
        operands = device_operands(row, case, dev)
        torch.cuda.synchronize()
        print(f'ROW {name}', file=sys.stderr, flush=True)
        y = launch(row, operands, row.acts[0], coef)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(y).all()), name
    print('ROW -', file=sys.stderr, flush=True)
    print('ok')


if __name__ == '__main__':
    main()
