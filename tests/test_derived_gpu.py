"""GPU: the cache of derived tensors (dcsnet/_derived.py) under both networks — nothing stale is served after a weight,
a running statistic or the conv precision changed, a graph owner keeps exactly what it was served, and captured graphs hold
no packs they did not hold before.

Network input [2, 256, 16]: 16 frames is the smallest multiple of 8 whose synthesis is long enough (hop (T - 1) = 480 > 256).
Seeded weights, dropout off.  A "forward" is two eval passes under no_grad: the first leaves every CBN's coefficients
(_eval_forward), the second folds them into the convs (eval_coef + cconv2d_cbn_eval in C_NETWORK); both are compared."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.seeded_state import fill_state, fill_state_stream, seeded_input   # noqa: E402

B, T = 2, 16


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from dcsnet import _lib
    _lib.load()
    return torch.device('cuda:0')


def _hp():
    from dcsnet.config import hparams
    hp = dict(hparams)
    hp['dropout_conv'], hp['dropout_fc'] = 0.0, 0.0
    return hp


def _network(kind, dev, seed=3):
    """-> (net in eval mode, its input, one conv weight of it)."""
    from dcsnet.config import config
    if kind == 'complex':
        from dcsnet.c_network import C_NETWORK
        net = fill_state(C_NETWORK(config, _hp(), 3), seed).to(dev).eval()
        return net, seeded_input(B, 256, T, 7).to(dev), net.encoder[1][0].conv_r.weight
    from dcsnet.r_network import R_NETWORK
    net = fill_state_stream(R_NETWORK(config, _hp(), 3), seed + 2).to(dev).eval()
    return net, seeded_input(B, 256, T, 7).abs().to(dev), net.encoder[1][0].weight


def _forward(net, x):
    with torch.no_grad():
        return [net(x).clone() for _ in range(2)]


def _same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


def _mul_in_place(net, x, w):
    with torch.no_grad():
        w.mul_(1.25)


def _swap_data(net, x, w):
    version = w._version
    w.data = w.data * 0.5 + 0.01
    assert w._version == version                                 # only the address tells


def _train_pass(net, x, w):
    """A train-mode pass rewrites every running statistic in a kernel (note_state_update)."""
    stats = [b for n, b in net.named_buffers() if n.endswith(('running_covar', 'running_var'))]
    before, versions = [s.clone() for s in stats], [s._version for s in stats]
    net.train()
    net(x)
    net.eval()
    assert versions == [s._version for s in stats] and any(not torch.equal(a, s) for a, s in zip(before, stats))


def _raw_write(net, x, w):
    """A write no version counter sees (what a replayed train step does), announced by bump_param_generation()."""
    from dcsnet import functional as F
    version, address = w._version, w.data_ptr()
    w.data.mul_(0.75)
    assert w._version == version and w.data_ptr() == address
    F.bump_param_generation()


@pytest.mark.parametrize('kind', ['complex', 'real'])
def test_nothing_stale_after_a_change_of_state(dev, kind):
    from dcsnet import _derived
    net, x, w = _network(kind, dev)
    before = _forward(net, x)
    assert _same(_forward(net, x), before)
    for change in (_mul_in_place, _swap_data, _train_pass, _raw_write):
        change(net, x, w)
        after = _forward(net, x)
        _derived.clear_all()
        fresh = _forward(net, x)
        assert _same(after, fresh), change.__name__
        assert not any(torch.equal(p, q) for p, q in zip(after, before)), change.__name__
        assert all(bool(torch.isfinite(torch.view_as_real(p) if p.is_complex() else p).all()) for p in after)
        before = after


@pytest.mark.parametrize('kind', ['complex', 'real'])
def test_nothing_stale_after_a_precision_switch(dev, kind):
    """Packed panels are laid out for one conv precision (one bf16 plane against three).  The real network's pack cache used
    to survive set_conv_precision()."""
    from dcsnet import _derived, ops
    net, x, _ = _network(kind, dev)
    mode, on_purpose = ops.conv_precision(), ops.BF16_OPERANDS_ON_PURPOSE
    try:
        ops.set_conv_precision('bf16x6')
        _derived.clear_all()
        first = _forward(net, x)
        for switch_to in ('bf16', 'bf16x6'):
            ops.set_conv_precision(switch_to)
            after = _forward(net, x)
            _derived.clear_all()
            assert _same(after, _forward(net, x)), switch_to
        assert _same(after, first)
    finally:
        ops.set_conv_precision(mode)
        ops.BF16_OPERANDS_ON_PURPOSE = on_purpose


def _pointers(kept):
    out = set()
    for v in kept:
        out.update(t.data_ptr() for t in (v if isinstance(v, (tuple, list)) else (v,)) if torch.is_tensor(t))
    return out


def test_the_enhancer_keeps_exactly_what_its_graph_reads(dev):
    from dcsnet import functional as F
    from dcsnet.enhance import Enhancer

    def first_pack(n):
        c = n.encoder[0][0]
        return F.packed_weight(c.conv_r.weight, c.conv_i.weight, c.conv_r.bias, c.conv_i.bias, False, (1, 1))[0].data_ptr()
    other, x, _ = _network('complex', dev, seed=4)
    _forward(other, x)
    net, _, _ = _network('complex', dev)
    enh = Enhancer(net, mode='dcs', segment_frames=T, overlap_frames=4, batch_segments=B, use_graph=True)
    enh.enhance_segments([torch.randn(700, generator=torch.Generator().manual_seed(1)).numpy()], 16000)
    assert enh._graph is not None
    kept = _pointers(enh._keep)
    assert first_pack(net) in kept
    assert first_pack(other) not in kept


# ---- node counts -------------------------------------------------------------------------------------------------------

def _kernel_nodes(graph):
    """Kernel nodes of a captured graph that was kept (CUDAGraph(keep_graph=True)); it is never instantiated or replayed."""
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), 'lib', 'libamdhip64.so'))
    raw, n = ctypes.c_void_p(graph.raw_cuda_graph()), ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(raw, None, ctypes.byref(n)) == 0
    nodes = (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(raw, nodes, ctypes.byref(n)) == 0
    kernels = 0
    for node in nodes:
        kind = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(kind)) == 0
        kernels += kind.value == 0                               # hipGraphNodeTypeKernel
    return kernels


@pytest.mark.parametrize('kind', ['complex', 'real'])
def test_a_second_capture_of_an_enhancer_step_has_as_many_nodes(dev, kind, monkeypatch):
    """Nothing is stored while a stream is captured, so a pack the warm-up passes did not leave would be made inside the
    capture: the warm-ups of Enhancer._step_fn must leave them all.  Its capture from an empty cache is as large as the
    capture that follows it, which finds everything cached.  (The graphs are kept raw and never replayed.)"""
    from dcsnet import _derived
    from dcsnet.enhance import Enhancer, MagnitudeEnhancer
    net, _, _ = _network(kind, dev)
    cls, mode = (Enhancer, 'dcs') if kind == 'complex' else (MagnitudeEnhancer, 'drs')
    enh = cls(net, mode=mode, segment_frames=T, overlap_frames=4, batch_segments=B, use_graph=False)
    enh.enhance_segments([torch.randn(700, generator=torch.Generator().manual_seed(1)).numpy()], 16000)   # store and tables
    enh.use_graph = True
    plain = torch.cuda.CUDAGraph
    monkeypatch.setattr(torch.cuda, 'CUDAGraph', lambda: plain(keep_graph=True))
    counts = []
    with torch.no_grad():
        for empty in (True, False):
            if empty:
                _derived.clear_all()
            enh._graph = None
            enh._step_fn()
            counts.append(_kernel_nodes(enh._graph))
    enh._graph = None
    torch.cuda.synchronize()
    print(f'{cls.__name__} kernel nodes: {counts}')
    assert counts[0] == counts[1] and counts[0] > 20


# C_NETWORK step at [2, 256, 16], world 1, per conv precision: counted on the commit before the cache was unified, with this
# test's own steps (two warm steps, then _capture() twice with the graph kept raw).
TRAIN_STEP_KERNEL_NODES = {'bf16x6': 260, 'f32': 250}


def test_the_train_step_graph_has_the_nodes_it_had(dev, monkeypatch):
    """dp.TrainStep's captured step is served its packs by the pack plan (4 launches); the cache adds none.  (A change to the
    step's launches moves the constant; a pack made inside the capture must not.)"""
    from dcsnet.config import config
    from dcsnet.c_network import C_NETWORK
    from dcsnet.dp import TrainStep
    from dcsnet import network_functions as nf
    clean, noise = seeded_input(B, 256, T, 1, 0.1), seeded_input(B, 256, T, 2, 0.05)
    batch = (noise.to(dev), (clean + noise).to(dev), clean.to(dev), [0, 1])
    net = fill_state(C_NETWORK(config, _hp(), 0), 2).to(dev).train()
    ts = TrainStep(net, use_graph=True, graph_warmup=2)
    for _ in range(2):
        ts(batch)
    plain = torch.cuda.CUDAGraph
    monkeypatch.setattr(torch.cuda, 'CUDAGraph', lambda: plain(keep_graph=True))
    counts = []
    for _ in range(2):
        ts._capture(batch)
        counts.append(_kernel_nodes(ts._graph))
        window = nf._window_on(config, dev)                      # what the graph synthesises with is the step's to keep
        assert {window.data_ptr(), nf._inv_envelope(window, T, config.hop_length).data_ptr()} <= _pointers(ts._keep)
        ts._graph = ts._graph_opt = None
    torch.cuda.synchronize()
    print(f'TrainStep kernel nodes: {counts}')
    from dcsnet import ops
    assert counts[0] == counts[1] == TRAIN_STEP_KERNEL_NODES[ops.conv_precision()]
