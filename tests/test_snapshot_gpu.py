"""GPU: dcs_snapshot_words (csrc/snapshot.hip) through ops.snapshot_table / ops.snapshot — many tensors into one staging slab in
one launch, bit for bit, with a per-tensor count of non-finite words; and the same launch between graph replays."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
SIZES = (0, 1, 3, 4, 5, 63, 64, 65, 1001, 4099)
BIG = 3_000_003                    # 2930 workgroups of 1024 words under a grid of 2048: the stride loop runs twice; BIG % 4 == 3


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from dcsnet import _lib
    _lib.load()
    return torch.device('cuda:0')


def _bits(n, seed, dev, finite):
    """n float32 values from seeded bit patterns: any pattern at all (NaNs, infinities and denormals among them), or with the
    exponent's top bit cleared — finite, denormals and both zeros included."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    if finite:
        w &= ~0x40000000
    return w.view(torch.float32).to(dev)


def _sources(dev, finite):
    """The small sizes and the big one as float32, a float32 view 4 bytes and an int64 view 8 bytes past a 16-byte boundary,
    an int32 counter and a complex64 tensor."""
    src = [_bits(n, 10 + i, dev, finite) for i, n in enumerate(SIZES)]
    src.append(_bits(BIG, 50, dev, finite))
    base = _bits(1001 + 4, 51, dev, finite)
    src.append(base[1:1 + 1001])                               # 4 bytes past
    ints = torch.arange(9, dtype=torch.int64, device=dev) * 0x100000000
    ints[1], ints[2] = 0x7FC00000, 0x7F800000                   # low words that would count as NaN / Inf in a float tensor
    ints[3] = -1                                                # every bit set
    src.append(ints[1:])                                        # 8 bytes past
    src.append(torch.tensor([7], dtype=torch.int32, device=dev))
    src.append(torch.view_as_complex(_bits(2 * 37, 52, dev, finite).view(37, 2)))
    assert src[-4].data_ptr() % 16 == 4 and src[-3].data_ptr() % 16 == 8
    return src


def _special(src):
    """-0.0, denormals and payload NaNs at chosen places of the float items (bit-exactness must not depend on the value)."""
    pats = [0x80000000, 0x00000001, 0x807FFFFF, 0x7FC12345, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000]
    for t in src:
        if t.dtype == torch.float32 and t.numel() >= 5:
            w = t.view(torch.int32)
            for k, p in enumerate(pats):
                w[(k * 7919) % t.numel()] = p - (1 << 32) if p >= 1 << 31 else p


def _expected_counts(src):
    out = []
    for t in src:
        if t.dtype in (torch.float32, torch.complex64) and t.numel():
            w = (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)
            out.append(int(((w & 0x7F800000) == 0x7F800000).sum()))
        else:
            out.append(0)
    return out


def _check_slab(table, slab, src, pad):
    covered = torch.zeros(slab.numel(), dtype=torch.bool, device=slab.device)
    for i, t in enumerate(src):
        o, w = table.layout[i]
        assert o % 4 == 0 and w == t.numel() * t.element_size() // 4
        want = (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32).reshape(-1)
        assert torch.equal(slab[o:o + w], want), (i, tuple(t.shape), t.dtype)
        v = table.view(slab, i)
        assert v.shape == t.shape and v.dtype == t.dtype
        covered[o:o + w] = True
    assert int((~covered).sum()) >= pad and bool((slab[~covered] == SENTINEL).all()), 'words between or behind the items were written'


def test_one_launch_over_many_items_is_bit_exact(dev):
    from dcsnet import ops
    src = _sources(dev, finite=False)
    _special(src)
    table = ops.snapshot_table(src)
    assert table.n == len(src) and table.total_words % 4 == 0
    assert int(table.first_block[-1]) > 2048                    # more workgroups than the grid holds
    pad = 64
    slab = torch.full((table.total_words + pad,), SENTINEL, dtype=torch.int32, device=dev)
    counts = torch.full((table.n,), 123, dtype=torch.int32, device=dev)
    ops.snapshot(table, slab, counts)
    torch.cuda.synchronize()
    _check_slab(table, slab, src, pad)
    want = _expected_counts(src)
    assert sum(want) > 8 and counts.tolist() == want            # whatever the random patterns hold, counted exactly
    assert counts[len(SIZES) + 2].item() == 0                   # the int64 item: NaN-like low words are not floats


def test_counts_are_exact_and_reset_by_the_call(dev):
    from dcsnet import ops
    src = _sources(dev, finite=True)
    table = ops.snapshot_table(src)
    slab = torch.full((table.total_words,), SENTINEL, dtype=torch.int32, device=dev)
    counts = torch.zeros(table.n, dtype=torch.int32, device=dev)
    i_first, i_tail, i_mid, i_cplx = SIZES.index(1001), len(SIZES), SIZES.index(4099), len(src) - 1
    src[i_first][0] = float('nan')                              # the first word of an item
    src[i_tail][BIG - 1] = float('inf')                         # the last word of the scalar tail (BIG % 4 == 3)
    src[i_mid][2050] = float('-inf')                            # mid-item, in its third workgroup
    src[i_mid][2051] = float('nan')
    src[i_cplx][36] = complex(0.0, float('inf'))                # the imaginary half of a complex element
    ops.snapshot(table, slab, counts)
    want = [0] * table.n
    want[i_first], want[i_tail], want[i_mid], want[i_cplx] = 1, 1, 2, 1
    assert counts.tolist() == want
    _check_slab(table, slab, src, 0)
    src[i_first][0], src[i_tail][BIG - 1], src[i_mid][2050], src[i_mid][2051], src[i_cplx][36] = 1.0, 2.0, 3.0, 4.0, 0j
    ops.snapshot(table, slab, counts)
    assert counts.tolist() == [0] * table.n                     # the call zeroes its own counters
    _check_slab(table, slab, src, 0)


def test_snapshot_between_graph_replays_images_the_moment_of_the_call(dev):
    from dcsnet import ops
    g0 = torch.Generator().manual_seed(3)
    src = [torch.randint(0, 1000, (n,), generator=g0).float().to(dev) for n in (BIG, 4099, 5)]
    src.append(torch.arange(6, dtype=torch.int64, device=dev))
    start = [t.clone() for t in src]
    table = ops.snapshot_table(src)
    slab = torch.zeros(table.total_words, dtype=torch.int32, device=dev)
    counts = torch.zeros(table.n, dtype=torch.int32, device=dev)
    ops.snapshot(table, slab, counts)                           # (first use outside the timed sequence)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for t in src:
            t.add_(1)
    graph.replay()
    graph.replay()
    ops.snapshot(table, slab, counts)                           # no synchronisation before or after
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for i, (t, s0) in enumerate(zip(src, start)):
        assert torch.equal(table.view(slab, i), s0 + 2), i      # the state at the call: two replays in
        assert torch.equal(t, s0 + 4), i
    assert counts.tolist() == [0] * table.n


def test_snapshot_wrapper_refuses_what_the_kernel_must_not_see(dev):
    from dcsnet import ops, DcsHipError
    table = ops.snapshot_table([torch.zeros(10, device=dev)])
    counts = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(DcsHipError, match='needs 12'):
        ops.snapshot(table, torch.zeros(8, dtype=torch.int32, device=dev), counts)
    with pytest.raises(DcsHipError, match='aligned'):
        ops.snapshot(table, torch.zeros(20, dtype=torch.int32, device=dev)[1:], counts)
    with pytest.raises(DcsHipError, match='contiguous'):
        ops.snapshot_table([torch.zeros(4, 4, device=dev).t()])
    with pytest.raises(DcsHipError, match='dtype'):
        ops.snapshot_table([torch.zeros(4, dtype=torch.uint8, device=dev)])
