"""CPU-only: the weight-gradient workspace query (dcs_cconv2d_bwd_weight_workspace_bytes[_h]) and the plan read-out
(dcs_cconv2d_bwd_weight_plan[_h]) are one description (csrc/conv_api.hip: wgrad_plan) read twice.

These are CONSISTENCY checks, not recorded numbers: the MFMA routes size their slabs from the device's occupancy answer, and
without a GPU that call fails and falls back to one workgroup per CU, so the byte counts here are not the ones a train step
sees (those are in profiles/conv_api_refactor.txt).  What holds on any machine: the two entry points agree, the layout is
[slabs | pad to 256 | planes] with the padding only where planes exist, bf16 storage has no planes, the route of a geometry
is the one tests/_wgrad_cases.py names, and a geometry the launch rejects gives -1 from both."""
import pytest

import _plan_probe as P
import _wgrad_cases as W


def _rows():
    """Every row of the forward plan probe's table (its geometries are the networks' layer kinds) and the per-route cases."""
    rows = []
    for name, r in P.ALL.items():
        L = r.L
        rows.append((name, (r.B, L.H, L.W, L.C1, L.C2, L.up[0], L.up[1], L.Cout, L.k, L.k, L.stride[0], L.stride[1], L.k // 2,
                            L.k // 2), None))
    rows += [(c.name, W.geo(c), c) for c in W.CASES]
    # upsample factors the fold does not know (its class tables hold 2 x 2): accepted geometries of the plain MFMA route
    for up in ((3, 2), (2, 3), (4, 2), (3, 1)):
        c = W.Case(f'mfma_8to8_k3up{up[0]}{up[1]}', W.MFMA, 2, 5, 7, 8, 0, 8, 3, (1, 1), 1, up, False, True)
        rows.append((c.name, W.geo(c), c))
    return rows


ROWS = _rows()


@pytest.fixture(scope='module')
def lib():
    from dcsnet import _lib, ops
    handle = _lib.load()
    default = ops.conv_precision()
    ops.set_conv_precision('bf16x6')          # the mode in which the fp32 build pre-splits g_Y (the planes region)
    yield handle
    ops.set_conv_precision(default)


@pytest.mark.parametrize('h', [False, True], ids=['f32', 'bf16_storage'])
@pytest.mark.parametrize('name,geometry,case', ROWS, ids=[r[0] for r in ROWS])
def test_plan_and_query_are_one_description(lib, name, geometry, case, h):
    rc, (route, slabs, slab_bytes, planes_bytes, total) = W.plan(lib, geometry, h)
    assert rc == 0, (name, rc)
    assert total == W.query(lib, geometry, h)
    assert route in range(5) and slabs >= 1 and slab_bytes > 0 and planes_bytes >= 0
    if planes_bytes > 0:
        assert total == W.align256(slab_bytes) + planes_bytes
    else:
        assert total == slab_bytes
    if h:
        assert planes_bytes == 0
    if route not in (W.FOLD, W.MFMA):
        assert planes_bytes == 0
    if case is not None:
        # (the pixel-stationary 7x7 kernel serves fp32 maps only: under bf16 storage that geometry runs the direct kernel)
        want = W.DIRECT if (h and case.route == W.SMALL) else case.route
        assert route == want, (name, W.ROUTE_NAMES[route], W.ROUTE_NAMES[want])
        assert (planes_bytes > 0) == (case.planes and not h), (name, planes_bytes)


def _with(geometry, **kw):
    names = ('B', 'Hin', 'Win', 'C1', 'C2', 'up_f', 'up_t', 'Cout', 'kh', 'kw', 'sf', 'st', 'pad_f', 'pad_t')
    d = dict(zip(names, geometry), **kw)
    return tuple(d[n] for n in names)


GOOD = W.geo(W.CASES[2])
BAD = {
    'zero_batch': _with(GOOD, B=0),
    'zero_height': _with(GOOD, Hin=0),
    'negative_width': _with(GOOD, Win=-3),
    'zero_cout': _with(GOOD, Cout=0),
    'no_output_row': _with(GOOD, Hin=2, kh=7, kw=7, pad_f=0, pad_t=0, sf=1, st=1),      # Hout = 2 - 7 + 1 < 0
    'negative_pad_f': _with(GOOD, pad_f=-1),
    'negative_pad_t': _with(GOOD, pad_t=-1),
    'zero_c1': _with(GOOD, C1=0, C2=16),
    'negative_c1': _with(GOOD, C1=-8),
    'zero_stride': _with(GOOD, sf=0),
    'zero_upsample': _with(GOOD, up_t=0),
}


@pytest.mark.parametrize('h', [False, True], ids=['f32', 'bf16_storage'])
@pytest.mark.parametrize('why', sorted(BAD))
def test_rejected_geometries_give_minus_one_from_both(lib, why, h):
    assert W.plan(lib, GOOD, h)[0] == 0 and W.query(lib, GOOD, h) > 0
    rc, out = W.plan(lib, BAD[why], h)
    assert rc == -1 and out == [-7] * 5          # nothing written
    assert W.query(lib, BAD[why], h) == -1
