"""dcs_cconv2d_bwd_weight[_h] inside a workspace of EXACTLY the queried size, one case per route of the weight gradient
(tests/_wgrad_cases.py; the route is asserted through dcs_cconv2d_bwd_weight_plan before the launch).

The workspace is the middle of one larger allocation with a 1 MiB guard of 0xA5 on either side.  The guards are in-bounds
memory on purpose: a launch that addresses past what its own query reports shows as a changed guard byte, never as a fault.
Per case: both guards unchanged; the four gradients bit-equal to ops.cconv2d_bwd_weight (its shared, larger workspace) on the
same operands; and with one byte less than the slabs need the call returns DCS_ERR_WORKSPACE before any launch — outputs
(pre-filled with a sentinel) and guards untouched."""
import pytest
import torch

import _wgrad_cases as W

pytestmark = pytest.mark.gpu

GUARD = 1 << 20
FILL = 0xA5
SENTINEL = -12345.0
DCS_ERR_WORKSPACE = -3

# (the small 7x7 kernel serves fp32 maps only: no bf16-storage run of its own)
RUNS = [(c, False) for c in W.CASES] + [(c, True) for c in W.CASES if c.h]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from dcsnet import _lib
    _lib.load()
    return torch.device('cuda:0')


@pytest.fixture
def precision():
    """Conv precision for the build under test, switched and restored the way tests/test_hip_bf16.py does: 'bf16x6' (the
    mode with the pre-split g_Y planes) for fp32 activations, 'bf16' (bf16 weight panels) for bf16 storage."""
    from dcsnet import ops
    default = ops.conv_precision()
    yield lambda h: ops.set_conv_precision('bf16' if h else 'bf16x6')
    ops.set_conv_precision(default)


def _guards_intact(buf, nbytes):
    return bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + nbytes:] == FILL).all())


@pytest.mark.parametrize('case,h', RUNS, ids=[f'{c.name}-{"bf16_storage" if h else "f32"}' for c, h in RUNS])
def test_launch_stays_inside_the_queried_workspace(dev, precision, case, h):
    from dcsnet import _lib, ops
    from dcsnet._lib import ptr
    precision(h)
    lib = _lib.load()
    c = case
    geometry = W.geo(c)
    rc, (route, slabs, slab_bytes, planes_bytes, total) = W.plan(lib, geometry, h)
    assert rc == 0 and route == c.route, (c.name, W.ROUTE_NAMES[route])
    assert (planes_bytes > 0) == (c.planes and not h), planes_bytes
    nbytes = W.query(lib, geometry, h)
    assert nbytes == total and nbytes >= slab_bytes > 0

    dt = torch.bfloat16 if h else torch.float32
    g = torch.Generator().manual_seed(11 + W.CASES.index(c))
    Hout = (c.H * c.up[0] + 2 * c.pad - c.k) // c.stride[0] + 1
    Wout = (c.W * c.up[1] + 2 * c.pad - c.k) // c.stride[1] + 1
    x1 = torch.randn((c.B, c.H, c.W, c.C1, 2), generator=g).to(dt).to(dev)
    x2 = torch.randn((c.B, c.H, c.W, c.C2, 2), generator=g).to(dt).to(dev) if c.C2 else None
    gy = torch.randn((c.B, Hout, Wout, c.Cout, 2), generator=g).to(dt).to(dev)
    Cin = c.C1 + c.C2
    tr = c.up != (1, 1)                          # the decoder's layers are ComplexConvTranspose2d
    w_shape = (Cin, c.Cout, c.k, c.k) if tr else (c.Cout, Cin, c.k, c.k)

    want = ops.cconv2d_bwd_weight(x1, x2, gy, w_shape, True, (c.k, c.k), c.stride, (c.pad, c.pad), c.up, tr)

    buf = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
    ws = buf.data_ptr() + GUARD
    fn = getattr(lib, 'dcs_cconv2d_bwd_weight' + ('_h' if h else ''))

    def outputs():
        return [torch.full(w_shape, SENTINEL, device=dev), torch.full(w_shape, SENTINEL, device=dev),
                torch.full((c.Cout,), SENTINEL, device=dev), torch.full((c.Cout,), SENTINEL, device=dev)]

    def call(outs, size):
        rc_ = fn(ptr(x1), ptr(x2), ptr(gy), *(ptr(t) for t in outs), ws, size, *geometry, int(tr), _lib.cur_stream())
        torch.cuda.synchronize()
        return rc_

    got = outputs()
    assert call(got, nbytes) == 0
    assert _guards_intact(buf, nbytes), f'{c.name}: the launch wrote outside its {nbytes} queried bytes'
    for a, b, n in zip(got, want, ('gw_r', 'gw_i', 'gb_r', 'gb_i')):
        assert torch.equal(a, b), (c.name, n)

    buf.fill_(FILL)
    untouched = outputs()
    assert call(untouched, slab_bytes - 1) == DCS_ERR_WORKSPACE
    for t, n in zip(untouched, ('gw_r', 'gw_i', 'gb_r', 'gb_i')):
        assert bool((t == SENTINEL).all()), (c.name, n)
    assert bool((buf == FILL).all()), c.name
