"""GPU: the device learning rate of the fused Adam (a schedule reaches captured steps), the SWA average kernel against torch's
fp32 CPU evaluation of Lightning's avg_fn, and stochastic weight averaging end to end on captured C_NETWORK and R_NETWORK
training steps (dcsnet/swa.py)."""
import sys

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


class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.a = torch.nn.Parameter(torch.randn(37, 5, generator=g))
        self.b = torch.nn.Parameter(torch.randn(1001, generator=g))
        self.c = torch.nn.Parameter(torch.randn(3, generator=g))


def _lightning_average(snapshots):
    """Lightning 1.5.6's update_parameters / avg_fn on the CPU in fp32 (n_averaged a long tensor), as the callback runs it."""
    avg, n = None, torch.tensor(0, dtype=torch.long)
    for s in snapshots:
        s = s.detach().cpu()
        avg = s.clone() if n == 0 else avg + (s - avg) / (n + 1)
        n += 1
    return avg


def _hp():
    from dcsnet.config import hparams
    hp = dict(hparams)
    hp['dropout_conv'], hp['dropout_fc'] = 0.0, 0.0
    return hp


def _batch(dev, B=2, T=32, seed=1):
    clean, noise = seeded_input(B, 256, T, seed, 0.1), seeded_input(B, 256, T, seed + 100, 0.05)
    return (noise.to(dev), (clean + noise).to(dev), clean.to(dev), list(range(B)))


@pytest.mark.parametrize('max_norm', [0.5, 0.0])          # dcs_adam_amsgrad_step_sumsq / dcs_adam_amsgrad_step
def test_captured_fused_adam_step_sees_a_later_learning_rate(dev, max_norm):
    from dcsnet.dp import FlatBucket, FusedAdam
    b1, b2 = FlatBucket(_Toy().to(dev)), FlatBucket(_Toy().to(dev))
    kw = dict(lr=1e-2, eps=1e-6, weight_decay=1e-3, max_norm=max_norm)
    o1, o2 = FusedAdam(b1, **kw), FusedAdam(b2, **kw)
    g = torch.Generator().manual_seed(3)
    grad = (torch.randn(b1.numel, generator=g) * 2.0).to(dev)
    for b in (b1, b2):
        b.zero_grad()
        b.grad.copy_(grad)
    o1.step()
    o2.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o1.step()
    o1.lr = 3e-3
    o1.sync_lr()
    o2.param_groups[0]['lr'] = 3e-3
    for _ in range(2):
        graph.replay()
        o2.step()
    torch.cuda.synchronize()
    assert int(o1.t_dev) == int(o2.t_dev) == 3
    for a, b in ((b1.flat, b2.flat), (o1.m, o2.m), (o1.v, o2.v), (o1.vmax, o2.vmax)):
        assert torch.equal(a, b)
    # and the rate did change: a twin stepped at the captured 1e-2 lands elsewhere
    b3 = FlatBucket(_Toy().to(dev))
    o3 = FusedAdam(b3, **kw)
    b3.zero_grad()
    b3.grad.copy_(grad)
    for _ in range(3):
        o3.step()
    assert not torch.equal(b3.flat, b1.flat)


def test_learning_rate_changes_reach_a_replayed_train_step(dev):
    """C_NETWORK [2,256,32], graph on: at lr 0 replays leave the bucket bit-unchanged while t_dev advances; the rate restored,
    the parameters move again; under a scripted rate sequence the losses follow an eager twin."""
    from dcsnet.config import config
    from dcsnet.c_network import C_NETWORK
    from dcsnet.dp import TrainStep
    hp = _hp()
    batch = _batch(dev)
    ts_g = TrainStep(fill_state(C_NETWORK(config, hp, 0), 2).to(dev).train(), use_graph=True, graph_warmup=2)
    ts_e = TrainStep(fill_state(C_NETWORK(config, hp, 0), 2).to(dev).train())
    lrs = [1e-4, 1e-4, 1e-4, 0.0, 0.0, 1e-4, 3e-4, 5e-5, 2e-4]
    graph, eager = [], []
    for i, lr in enumerate(lrs):
        for ts in (ts_g, ts_e):
            ts.optimizer.param_groups[0]['lr'] = lr
        before, t_before = ts_g.bucket.flat.clone(), int(ts_g.opt.t_dev)
        graph.append(float(ts_g(batch)))
        eager.append(float(ts_e(batch)))
        assert int(ts_g.opt.t_dev) == t_before + 1
        if i >= 3:
            assert ts_g._graph is not None, 'capture did not happen (fell back to eager)'
            assert torch.equal(before, ts_g.bucket.flat) == (lr == 0.0), (i, lr)
    assert float(ts_g.opt.lr_dev) == pytest.approx(2e-4, rel=1e-7)
    for a, b in zip(eager, graph):
        assert abs(a - b) <= 1e-3 * abs(a) + 1e-3, (eager, graph)


def _bucket_numel():
    from dcsnet.config import config
    from dcsnet.c_network import C_NETWORK
    from dcsnet.dp import FlatBucket
    return FlatBucket(C_NETWORK(config, _hp(), 0)).numel


@pytest.mark.parametrize('n_averaged', [0, 1, 2, 40])
def test_swa_average_kernel_matches_the_cpu_formula(dev, n_averaged):
    from dcsnet import ops
    g = torch.Generator().manual_seed(n_averaged)
    for n in (1, 3, 5, 1001, _bucket_numel()):
        scale = torch.pow(10.0, torch.empty(n).uniform_(-6, 2, generator=g))
        avg = torch.randn(n, generator=g) * scale
        p = avg + torch.randn(n, generator=g) * scale * 0.1
        want = p.clone() if n_averaged == 0 else avg + (p - avg) / (torch.tensor(n_averaged, dtype=torch.long) + 1)
        got = ops.swa_average(avg.to(dev), p.to(dev), n_averaged)
        assert torch.equal(got.cpu(), want), (n, n_averaged)


def test_c_network_swa_end_to_end(dev):
    """max_epochs 5, 2 batches per epoch, graph on: the parameters end as the average of the bucket at the starts of epochs 3
    and 4, the CBN statistics stay the last step's, and an eval forward equals a fresh network's on the same state_dict."""
    from dcsnet.config import config
    from dcsnet.c_network import C_NETWORK
    from dcsnet.dp import TrainStep, plateau_scheduler
    from dcsnet.swa import StochasticWeightAveraging
    hp = _hp()
    net = fill_state(C_NETWORK(config, hp, 0), 2).to(dev).train()
    ts = TrainStep(net, use_graph=True, graph_warmup=2)
    swa = StochasticWeightAveraging(ts, 5, lr_scheduler=plateau_scheduler(ts.optimizer))
    assert swa.epochs == 5 and (swa.swa_start, swa.swa_end) == (3, 4)
    batches = [_batch(dev, seed=1), _batch(dev, seed=2)]
    snaps = {}
    for epoch in range(swa.epochs):
        snaps[epoch] = ts.bucket.flat.clone()
        swa.on_train_epoch_start(epoch)
        losses = [float(ts(b, i)) for i, b in enumerate(batches)]
        swa.on_train_epoch_end(epoch, monitored=sum(losses) / len(losses))
    assert ts._graph is not None
    buffers = {k: v.clone() for k, v in net.state_dict().items() if 'running' in k or 'num_batches' in k or 'RMS' in k}
    assert buffers
    x = batches[0][1]
    net.eval()
    with torch.no_grad():
        last = net(x).clone()                          # caches derived from the last iterate
    swa.on_train_end()
    assert swa.n_averaged == 2
    assert torch.equal(ts.bucket.flat.cpu(), _lightning_average([snaps[3], snaps[4]]))
    sd = net.state_dict()
    for k, v in buffers.items():
        assert torch.equal(sd[k], v), k
    fresh = C_NETWORK(config, hp, 0).to(dev)
    fresh.load_state_dict(sd)
    fresh.eval()
    with torch.no_grad():
        got, want = net(x), fresh(x)
    assert torch.equal(got, want)
    assert not torch.equal(got, last)


def test_r_network_statistics_epoch(dev):
    """DRS-Net, max_epochs 3 + the statistics epoch over K batches, graph on: the bucket is the average; the BatchNorm
    statistics are update_bn's on the oracle with the averaged weights and the same noisy magnitudes; counters K, momentum
    0.1, buffers where they were — and the captured step still replays into them."""
    from dcsnet.config import config
    from dcsnet.r_network import R_NETWORK
    from dcsnet.dp import TrainStep, plateau_scheduler
    from dcsnet.swa import StochasticWeightAveraging
    from oracle.rnet_oracle import R_NETWORK_Oracle
    from torch.optim.swa_utils import update_bn
    K = 3
    argv = sys.argv
    sys.argv = ['train.py', 'drs', '0']
    try:
        net = fill_state_stream(R_NETWORK(config, _hp(), 0), 5).to(dev).train()
        ts = TrainStep(net, use_graph=True, graph_warmup=1)
        swa = StochasticWeightAveraging(ts, 3, lr_scheduler=plateau_scheduler(ts.optimizer))
        assert swa.epochs == 4 and (swa.swa_start, swa.swa_end) == (1, 2)
        bns = [m for m in net.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
        assert bns
        ptrs = [(m.running_mean.data_ptr(), m.running_var.data_ptr(), m.num_batches_tracked.data_ptr()) for m in bns]
        batches = [_batch(dev, seed=10 + i) for i in range(K)]
        snaps = []
        for epoch in range(swa.epochs):
            if swa.swa_start <= epoch <= swa.swa_end:
                snaps.append(ts.bucket.flat.clone())
            swa.on_train_epoch_start(epoch)
            for i, b in enumerate(batches):
                if swa.is_bn_epoch(epoch):
                    held = ts.bucket.flat.clone()
                    swa.bn_step(b, i)
                    assert torch.equal(held, ts.bucket.flat)
                else:
                    ts(b, i)
            swa.on_train_epoch_end(epoch, monitored=1.0)
        swa.on_train_end()
        assert ts._graph is not None
        assert torch.equal(ts.bucket.flat.cpu(), _lightning_average(snaps))
        assert [(m.running_mean.data_ptr(), m.running_var.data_ptr(), m.num_batches_tracked.data_ptr()) for m in bns] == ptrs
        assert all(m.momentum == 0.1 and int(m.num_batches_tracked) == K for m in bns)

        ref = R_NETWORK_Oracle(dropout_conv=0.0, dropout_fc=0.0)
        ref.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
        update_bn([(torch.abs(b[1].cpu()),) for b in batches], ref)
        got, want = net.state_dict(), ref.state_dict()
        for k in want:
            if k.endswith(('running_mean', 'running_var')):
                a, b = got[k].cpu(), want[k]
                assert ((a - b).abs() <= 1e-6 + 1e-4 * b.abs()).all(), (k, float((a - b).abs().max()))

        stats = [(m.running_mean.clone(), m.running_var.clone()) for m in bns]
        ts(batches[0])                                      # a replay of the captured step, into the same buffers
        torch.cuda.synchronize()
        assert all(int(m.num_batches_tracked) == K + 1 for m in bns)
        assert all(not torch.equal(m.running_mean, s[0]) and torch.isfinite(m.running_var).all() for m, s in zip(bns, stats))
    finally:
        sys.argv = argv
