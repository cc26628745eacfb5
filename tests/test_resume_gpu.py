"""GPU: a training run saved and continued (dcsnet/checkpoint.py) — into a live captured graph, eagerly with the reference's
dropout, for DRS-Net, from an optimizer state in the reference's format, and through the asynchronous CheckpointWriter.
C_NETWORK / R_NETWORK at [2, 256, 32] on seeded state and inputs, as tests/test_hip_train.py.

One process holds one device seed offset at a time (ops.SEED_STATE is the last TrainStep's), so the runs of a test are made one
after the other and compared through clones."""
import sys
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.seeded_state import fill_state, fill_state_stream, seeded_input   # noqa: E402


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from dcsnet import _lib
    _lib.load()
    return torch.device('cuda:0')


def _batch(dev, seed, B=2, T=32):
    clean, noise = seeded_input(B, 256, T, seed, 0.1), seeded_input(B, 256, T, seed + 100, 0.05)
    return (noise.to(dev), (clean + noise).to(dev), clean.to(dev), list(range(B)))


def _hp(dropout):
    from dcsnet.config import hparams
    hp = dict(hparams)
    if not dropout:
        hp['dropout_conv'], hp['dropout_fc'] = 0.0, 0.0
    return hp


def _net(kind, dev, seed, dropout):
    from dcsnet.config import config
    if kind == 'drs':
        from dcsnet.r_network import R_NETWORK
        return fill_state_stream(R_NETWORK(config, _hp(dropout), 0), seed).to(dev).train()
    from dcsnet.c_network import C_NETWORK
    return fill_state(C_NETWORK(config, _hp(dropout), 0), seed).to(dev).train()


def _state(ts):
    """Everything a replay rewrites, as clones."""
    torch.cuda.synchronize()
    out = {'flat': ts.bucket.flat, 'm': ts.opt.m, 'v': ts.opt.v, 'vmax': ts.opt.vmax, 't_dev': ts.opt.t_dev, 'seed_state': ts.seed_state}
    out.update({f'sd/{k}': v for k, v in ts.net.state_dict().items()})
    return {k: v.detach().clone() for k, v in out.items()}


def _same(a, b):
    assert list(a) == list(b)
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, (len(bad), bad[:6])


def _run(kind, dev, seed, calls, batches, use_graph, dropout):
    from dcsnet.dp import TrainStep
    torch.manual_seed(0)
    ts = TrainStep(_net(kind, dev, seed, dropout), use_graph=use_graph, graph_warmup=1)
    for k in range(calls):
        ts(batches[k])
    return ts


def _scheme(kind, dev, tmp_path, use_graph, dropout):
    """A: 6 calls.  A': the same again (the control).  B: 3 calls, saved.  C: another seed, its own calls first, then B's file
    loaded, then calls 4-6.  C must end where A did."""
    from dcsnet.checkpoint import save_checkpoint, load_checkpoint
    from dcsnet.dp import TrainStep
    batches = [_batch(dev, 1 + k) for k in range(6)]
    other = [_batch(dev, 50 + k) for k in range(2)]
    a = _state(_run(kind, dev, 2, 6, batches, use_graph, dropout))
    a2 = _state(_run(kind, dev, 2, 6, batches, use_graph, dropout))
    _same(a, a2)                                                # the control: a twin run is bit-identical
    assert int(a['t_dev']) == 6 and int(a['seed_state']) == 6
    path = str(tmp_path / 'b.ckpt')
    b = _run(kind, dev, 2, 3, batches, use_graph, dropout)
    save_checkpoint(path, b, epoch=0, global_step=3)
    del b
    torch.manual_seed(0)
    if use_graph:
        c = TrainStep(_net(kind, dev, 5, dropout), use_graph=True, graph_warmup=1)
        for bt in other:                                        # call 2 captures: the graph is live before the load
            c(bt)
        assert c._graph is not None, 'capture did not happen (fell back to eager)'
    else:
        c = TrainStep(_net(kind, dev, 5, dropout))              # a fresh step, nothing run
        torch.rand(3, device=dev)                               # ... in a process whose generators stand elsewhere
    graph, ptrs = c._graph, (c.bucket.flat.data_ptr(), c.opt.m.data_ptr(), c.opt.t_dev.data_ptr(), c.seed_state.data_ptr())
    got = load_checkpoint(path, c)
    assert got == {'epoch': 0, 'global_step': 3, 'extra': None}
    # (opt.t, the host's call count, stands still under replay: the device count t_dev is what the bias corrections read)
    assert int(c.opt.t_dev) == 3 and int(c.seed_state) == 3 and c.opt.t == (2 if use_graph else 3)
    for k in range(3, 6):
        c(batches[k])
    assert c._graph is graph
    assert ptrs == (c.bucket.flat.data_ptr(), c.opt.m.data_ptr(), c.opt.t_dev.data_ptr(), c.seed_state.data_ptr())
    _same(a, _state(c))


def test_resume_into_a_live_graph_is_bit_identical(dev, tmp_path):
    _scheme('dcs', dev, tmp_path, use_graph=True, dropout=False)


def test_eager_resume_with_dropout_continues_the_mask_stream(dev, tmp_path):
    """Default dropout: the masks of calls 4-6 follow from _drop_calls and the seed offset, both restored."""
    _scheme('dcs', dev, tmp_path, use_graph=False, dropout=True)


def test_eager_resume_of_drs_net(dev, tmp_path):
    argv = sys.argv
    sys.argv = ['train.py', 'drs', '0']
    try:
        _scheme('drs', dev, tmp_path, use_graph=False, dropout=True)
    finally:
        sys.argv = argv


class _Toy(torch.nn.Module):
    """tests/test_swa_gpu.py's _Toy."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.a = torch.nn.Parameter(torch.randn(37, 5, generator=g))
        self.b = torch.nn.Parameter(torch.randn(1001, generator=g))
        self.c = torch.nn.Parameter(torch.randn(3, generator=g))


def test_fused_adam_continues_a_reference_format_state(dev):
    """torch.optim.Adam(amsgrad=True) with the recipe's lr / eps / weight decay runs 2 steps on the toy; its state_dict goes into
    a FusedAdam over the same parameters; 3 further steps with the same scripted gradients to both.  Judged by the rule and
    the allowances tests/test_tail_fp64.py applies to FusedAdam against torch (err against the fp64 AdamRef <= max(4 x torch's
    own, floor)), imported from there."""
    from test_tail_fp64 import _adam_rows, tl
    from dcsnet.config import hparams
    from dcsnet.dp import FlatBucket, FusedAdam
    kw = dict(lr=hparams['lr'], betas=(0.9, 0.999), eps=hparams['optim_eps'], weight_decay=hparams['optim_weight_decay'])
    f32 = dict(lr=tl.f32(kw['lr']), betas=tuple(tl.f32(b) for b in kw['betas']), eps=tl.f32(kw['eps']),
               weight_decay=tl.f32(kw['weight_decay']))
    old = tl.set_threads()
    try:
        toy_t, toy_f = _Toy().to(dev), _Toy().to(dev)
        opt_t = torch.optim.Adam(toy_t.parameters(), amsgrad=True, **f32)
        bucket = FlatBucket(toy_f)
        ref = tl.AdamRef(bucket.flat, **kw)
        gen = torch.Generator().manual_seed(21)
        grads = [torch.randn(bucket.numel, generator=gen) * (1.0 if k % 2 else 1e-3) for k in range(5)]
        for g in grads:                                         # the padding carries no gradient
            covered = torch.zeros(bucket.numel, dtype=torch.bool)
            for o, p in zip(bucket.offsets, bucket.params):
                covered[o:o + p.numel()] = True
            g[~covered] = 0.0

        def give(params, g):
            for p, o in zip(params, bucket.offsets):
                p.grad = None
            for p, o in zip(params, bucket.offsets):
                p.grad = g[o:o + p.numel()].view(p.shape).to(dev)

        def torch_state():
            out = {k: torch.zeros(bucket.numel, device=dev) for k in ('p', 'm', 'v', 'vmax')}
            for p, o in zip(toy_t.parameters(), bucket.offsets):
                s = opt_t.state[p]
                for k, v in (('p', p.detach()), ('m', s['exp_avg']), ('v', s['exp_avg_sq']), ('vmax', s['max_exp_avg_sq'])):
                    out[k][o:o + p.numel()] = v.reshape(-1)
            return out
        assert [n for n, _ in toy_t.named_parameters()] == bucket.names       # (no LSTM here: same order, padded slices)
        for g in grads[:2]:
            give(list(toy_t.parameters()), g)
            opt_t.step()
            ref.step(g)
        fused = FusedAdam(bucket, **kw)
        with torch.no_grad():
            for p, q in zip(bucket.params, toy_t.parameters()):
                p.copy_(q)
        fused.load_state_dict(opt_t.state_dict())
        assert int(fused.t_dev) == 2
        misses = []
        prev = {'got': bucket.flat.clone(), 'ref': ref.p.clone(), 'yard': torch_state()['p']}
        for it, g in enumerate(grads[2:], start=3):
            give(list(toy_t.parameters()), g)
            opt_t.step()
            ref.step(g)
            bucket.zero_grad()
            bucket.grad.copy_(g.to(dev))
            fused.step()
            got = {'p': bucket.flat, 'm': fused.m, 'v': fused.v, 'vmax': fused.vmax}
            yard = torch_state()
            misses += _adam_rows(('resume', 'adam_reference_state', f'step{it}'), got, ref.state(), yard, prev, ref.t)
            prev = {'got': bucket.flat.clone(), 'ref': ref.p.clone(), 'yard': yard['p'].clone()}
        assert int(fused.t_dev) == ref.t == 5
        assert not misses, misses
    finally:
        torch.set_num_threads(old)


def _files_equal(a, b):
    from dcsnet.checkpoint import _walk_tensors
    fa, fb = (torch.load(p, map_location='cpu', weights_only=False) for p in (a, b))
    ta, tb = dict(_walk_tensors(fa)), dict(_walk_tensors(fb))
    assert list(ta) == list(tb) and len(ta) > 300
    bad = [k for k in ta if not (ta[k].dtype == tb[k].dtype and ta[k].shape == tb[k].shape and torch.equal(ta[k], tb[k]))]
    assert not bad, bad[:6]

    def plain(x):
        if torch.is_tensor(x):
            return None
        if isinstance(x, dict):
            return {k: plain(v) for k, v in x.items()}
        if isinstance(x, (list, tuple)):
            return [plain(v) for v in x]
        return x
    assert plain(fa) == plain(fb)


def test_checkpoint_writer_images_the_step_without_stopping_it(dev, tmp_path):
    """Replayed steps, writer.save after step 3 with no synchronisation, three more replays, close(): the file is the one a twin
    run's synchronous save_checkpoint wrote after its step 3.  A NaN planted in vmax before a second save: the file on disk
    is still the first, and `rejected` names max_exp_avg_sq."""
    from dcsnet.checkpoint import CheckpointWriter, save_checkpoint
    from dcsnet.dp import plateau_scheduler
    from dcsnet.swa import StochasticWeightAveraging
    batches = [_batch(dev, 1 + k) for k in range(6)]

    def driver():
        ts = _run('dcs', dev, 2, 0, batches, True, False)
        swa = StochasticWeightAveraging(ts, 2, lr_scheduler=plateau_scheduler(ts.optimizer))       # swa_start 0: averaging
        swa.on_train_epoch_start(0)
        for k in range(3):
            ts(batches[k])
        swa.on_train_epoch_end(0, monitored=1.0)
        swa.on_train_epoch_start(1)
        return ts, swa
    sync_path, async_path = str(tmp_path / 'sync.ckpt'), str(tmp_path / 'async.ckpt')
    ts, swa = driver()
    save_checkpoint(sync_path, ts, swa, epoch=0, global_step=3, extra={'k': 1})
    del ts, swa
    ts, swa = driver()
    assert ts._graph is not None
    writer = CheckpointWriter(ts, swa)
    writer.save(async_path, epoch=0, global_step=3, extra={'k': 1})
    for k in range(3, 6):                                       # training goes on over the image
        ts(batches[k])
    writer.poll()
    writer.close()
    assert writer.written == [async_path] and not writer.rejected
    assert int(ts.opt.t_dev) == 6
    _files_equal(sync_path, async_path)
    before = open(async_path, 'rb').read()
    writer = CheckpointWriter(ts, swa)
    ts.opt.vmax[12345] = float('nan')
    writer.save(async_path, epoch=0, global_step=6)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        writer.close()
    assert open(async_path, 'rb').read() == before
    assert len(writer.rejected) == 1 and writer.rejected[0][0] == async_path
    assert list(writer.rejected[0][1]) == ['optimizer_states/max_exp_avg_sq'] and writer.rejected[0][1]['optimizer_states/max_exp_avg_sq'] == 1
    assert any('non-finite' in str(w.message) for w in caught)
    assert sorted(p.name for p in tmp_path.iterdir()) == ['async.ckpt', 'sync.ckpt']
