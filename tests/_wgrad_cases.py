"""Weight-gradient geometries, one per route of csrc/conv_api.hip's wgrad_plan, shared by tests/test_conv_plan_cpu.py (host
arithmetic only) and tests/test_wgrad_workspace.py (the launch inside an exactly-sized, guarded workspace).

The shapes are the smallest that still take their route: more than one pixel tile where the kernel tiles (36x40 under a
4x16 tile, 32x32 under 8x16), ragged extents (6x20, 18x22, 7x9), a concatenated source on both fold rows and on one direct
row, an upsample of 3 (which must not reach the fold's four-class tables), and 64 input channels (eight 8-channel chunks: the
threshold of the pre-split g_Y planes) on the two planes rows."""
from collections import namedtuple

FOLD, MFMA, ENC0, SMALL, DIRECT = range(5)          # WgradRoute of csrc/conv_api.hip = out[0] of dcs_cconv2d_bwd_weight_plan
ROUTE_NAMES = ('fold', 'mfma', 'enc0', 'small', 'direct')

# planes: the fp32 build pre-splits g_Y under conv precision 'bf16x6' (never under bf16 storage); h: also run under bf16 storage
Case = namedtuple('Case', 'name route B H W C1 C2 Cout k stride pad up planes h')

CASES = [
    Case('fold21_16p8to16', FOLD, 2, 6, 20, 16, 8, 16, 3, (1, 1), 1, (2, 1), False, True),
    Case('fold22_planes_32p32to32', FOLD, 1, 8, 16, 32, 32, 32, 3, (1, 1), 1, (2, 2), True, True),
    Case('mfma_16to16_k5s22', MFMA, 2, 32, 32, 16, 0, 16, 5, (2, 2), 2, (1, 1), False, True),
    Case('mfma_planes_64to32_k3s21', MFMA, 2, 16, 32, 64, 0, 32, 3, (2, 1), 1, (1, 1), True, True),
    Case('mfma_tapsplit_8to16_k7s22', MFMA, 2, 36, 40, 8, 0, 16, 7, (2, 2), 3, (1, 1), False, True),
    # upsample factors above 2 never fold (conv_pack.hip folds 1 and 2 only): the plain MFMA route over the virtual input
    Case('mfma_8to8_k3up33', MFMA, 2, 5, 7, 8, 0, 8, 3, (1, 1), 1, (3, 3), False, True),
    Case('mfma_1x1_16to8', MFMA, 2, 8, 32, 16, 0, 8, 1, (1, 1), 0, (1, 1), False, True),
    Case('enc0_1to8_k7s22', ENC0, 2, 18, 22, 1, 0, 8, 7, (2, 2), 3, (1, 1), False, True),
    Case('small_2to1_k7', SMALL, 2, 16, 64, 2, 0, 1, 7, (1, 1), 3, (1, 1), False, False),
    Case('direct_12to8_k3', DIRECT, 2, 12, 20, 12, 0, 8, 3, (1, 1), 1, (1, 1), False, True),
    Case('direct_4p4to6_k3up22', DIRECT, 2, 7, 9, 4, 4, 6, 3, (1, 1), 1, (2, 2), False, True),
]


def geo(c):
    """The 14 integers of the conv entry points."""
    return (c.B, c.H, c.W, c.C1, c.C2, c.up[0], c.up[1], c.Cout, c.k, c.k, c.stride[0], c.stride[1], c.pad, c.pad)


def align256(n):
    return (n + 255) // 256 * 256


def plan(lib, geometry, h=False):
    """dcs_cconv2d_bwd_weight_plan[_h] -> (return code, [route, slabs, slab bytes, planes bytes, total bytes])."""
    import ctypes
    out = (ctypes.c_long * 5)(*([-7] * 5))
    rc = getattr(lib, 'dcs_cconv2d_bwd_weight_plan' + ('_h' if h else ''))(*geometry, out)
    return rc, list(out)


def query(lib, geometry, h=False):
    return getattr(lib, 'dcs_cconv2d_bwd_weight_workspace_bytes' + ('_h' if h else ''))(*geometry)
