"""CPU: the learning-rate schedule and stochastic weight averaging of the product training driver (dcsnet/dp.py,
dcsnet/swa.py) against torch's own schedulers and Lightning 1.5.6's StochasticWeightAveraging rules, on a small module with
and without a torch BatchNorm.  The optimizer is the torch reference (TorchAdam); the HIP kernels are covered by
tests/test_swa_gpu.py."""
import copy

import pytest
import torch
from torch.optim.lr_scheduler import ReduceLROnPlateau
from torch.optim.swa_utils import SWALR, update_bn


class _Small(torch.nn.Module):
    """conv -> [BatchNorm2d] -> relu -> pool -> linear, with the attributes TrainStep touches (hparams, training_step)."""

    def __init__(self, bn, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        self.conv = torch.nn.Conv2d(2, 6, 3, padding=1)
        self.bn = torch.nn.BatchNorm2d(6) if bn else torch.nn.Identity()
        self.head = torch.nn.Linear(6, 1)
        self.hparams = {'lr': 1e-2, 'optim_eps': 1e-6, 'optim_weight_decay': 1e-4, 'gradient_clip_val': 100.0}

    def forward(self, x):
        return self.head(torch.relu(self.bn(self.conv(x))).mean(dim=(2, 3)))

    def training_step(self, batch, batch_idx):
        x, y = batch[:2]
        return ((self(x) - y) ** 2).mean()


def _batches(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(4, 2, 5, 7, generator=g) * 2 + 0.5, torch.randn(4, 1, generator=g)) for _ in range(n)]


def _lightning_average(snapshots):
    """StochasticWeightAveraging.update_parameters / avg_fn of Lightning 1.5.6, restated: n_averaged a long tensor."""
    avg, n = None, torch.tensor(0, dtype=torch.long)
    for s in snapshots:
        avg = s.clone() if n == 0 else avg + (s - avg) / (n + 1)
        n += 1
    return avg


def _step(bn, seed=0):
    from dcsnet.dp import TrainStep, TorchAdam
    return TrainStep(_Small(bn, seed), optimizer_cls=TorchAdam)


@pytest.mark.parametrize('fused', [False, True])
def test_torch_schedulers_attach_to_the_step_optimizer(fused):
    """ReduceLROnPlateau and SWALR take TrainStep.optimizer, and its single group's lr is the step's rate.  FusedAdam (built
    on a CPU bucket here: only its step needs the device) is that optimizer itself; its zero_grad keeps the gradient sinks."""
    from dcsnet.dp import TrainStep, TorchAdam, FusedAdam, plateau_scheduler
    ts = TrainStep(_Small(True), **({} if fused else {'optimizer_cls': TorchAdam}))
    opt = ts.optimizer
    assert isinstance(opt, torch.optim.Optimizer) and len(opt.param_groups) == 1
    assert opt.param_groups[0]['lr'] == 1e-2
    assert (opt is ts.opt) == fused and isinstance(ts.opt, FusedAdam) == fused
    plateau = ReduceLROnPlateau(opt, patience=10)
    assert plateau.patience == 10 and plateau_scheduler(opt).patience == 10
    for _ in range(12):
        plateau.step(1.0)
    assert opt.param_groups[0]['lr'] == pytest.approx(1e-3, rel=1e-12)
    swalr = SWALR(opt, swa_lr=5e-4, anneal_epochs=2)
    swalr.step()
    swalr.step()
    assert opt.param_groups[0]['lr'] == pytest.approx(5e-4, rel=1e-12)
    if fused:
        assert ts.opt.lr == opt.param_groups[0]['lr']
        assert float(ts.opt.lr_dev) == pytest.approx(1e-2, rel=1e-7)       # written only when a step is about to run
        ts.opt.sync_lr()
        assert torch.equal(ts.opt.lr_dev, torch.tensor([5e-4], dtype=torch.float32))
        ts.opt.lr = 3e-3
        ts.opt.sync_lr()
        assert torch.equal(ts.opt.lr_dev, torch.tensor([3e-3], dtype=torch.float32))
        g_ptrs = [p.grad.data_ptr() for p in ts.bucket.params]
        ts.bucket.grad.fill_(1.0)
        opt.zero_grad()
        assert [p.grad.data_ptr() for p in ts.bucket.params] == g_ptrs and not ts.bucket.grad.any()


def test_configure_optimizers_uses_the_shared_plateau_definition():
    from dcsnet import dp
    from dcsnet.c_network import C_NETWORK
    from dcsnet.config import config, hparams
    sch = C_NETWORK(config, dict(hparams), 0).configure_optimizers()['lr_scheduler']
    ref = ReduceLROnPlateau(torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=1.0))
    assert isinstance(sch, ReduceLROnPlateau) and dp.PLATEAU_ARGS == {'patience': 10}
    for k in ('patience', 'factor', 'threshold', 'threshold_mode', 'cooldown', 'mode', 'min_lrs', 'eps'):
        want = 10 if k == 'patience' else getattr(ref, k)
        assert getattr(sch, k) == want, k


@pytest.mark.parametrize('bn', [False, True])
def test_swa_epoch_bookkeeping(bn):
    """max_epochs = 10: averaged at the starts of epochs 7, 8, 9; the final parameters are Lightning's average of snapshots
    recorded here; a BatchNorm network gets an 11th epoch whose forwards leave update_bn's statistics, with the bucket still
    and the optimizer never called, and its momentum restored at the end."""
    from dcsnet.swa import StochasticWeightAveraging
    from dcsnet.dp import plateau_scheduler
    ts = _step(bn)
    swa = StochasticWeightAveraging(ts, 10, lr_scheduler=plateau_scheduler(ts.optimizer))
    assert (swa.swa_start, swa.swa_end) == (7, 9)
    assert swa.epochs == (11 if bn else 10) and swa.contains_batch_norm == bn
    batches = _batches(3)
    snaps, updates = [], []
    for epoch in range(swa.epochs):
        before = ts.bucket.flat.clone()
        n0 = swa.n_averaged
        swa.on_train_epoch_start(epoch)
        if swa.n_averaged != n0:
            updates.append(epoch)
            snaps.append(before)
        if swa.is_bn_epoch(epoch):
            assert bn and epoch == 10
            assert torch.equal(ts.bucket.flat, _lightning_average(snaps))
            held = ts.bucket.flat.clone()
            real_step = ts.opt.step
            ts.opt.step = lambda *a, **k: pytest.fail('optimizer called in the statistics epoch')
            try:
                for i, b in enumerate(batches):
                    swa.bn_step(b, i)
            finally:
                ts.opt.step = real_step
            assert torch.equal(ts.bucket.flat, held)
            assert ts.net.bn.momentum is None and int(ts.net.bn.num_batches_tracked) == len(batches)
        else:
            assert torch.equal(ts.bucket.flat, before)
            for i, b in enumerate(batches):
                ts(b, i)
        swa.on_train_epoch_end(epoch, monitored=1.0 / (epoch + 1))
    swa.on_train_end()
    assert updates == [7, 8, 9] and swa.n_averaged == 3
    avg = _lightning_average(snaps)
    assert torch.equal(ts.bucket.flat, avg)
    for p, o in zip(ts.bucket.params, ts.bucket.offsets):
        assert torch.equal(p.detach().reshape(-1), avg[o:o + p.numel()])
    if bn:
        assert ts.net.bn.momentum == 0.1
        ref = _Small(True)
        ref.load_state_dict(ts.net.state_dict())
        update_bn([b for b in batches], ref)
        assert torch.equal(ts.net.bn.running_mean, ref.bn.running_mean)
        assert torch.equal(ts.net.bn.running_var, ref.bn.running_var)
        assert int(ts.net.bn.num_batches_tracked) == len(batches)


@pytest.mark.parametrize('swa_lrs', [None, 5e-5])
def test_lr_sequence_follows_torch_schedulers(swa_lrs):
    """Scripted monitored values: the plateau cut lands where torch's own ReduceLROnPlateau puts it on a twin SGD, the rate
    is constant from swa_start on with swa_lrs=None, and follows SWALR's cosine sequence on the twin otherwise."""
    from dcsnet.swa import StochasticWeightAveraging
    from dcsnet.dp import plateau_scheduler
    E = 50
    ts = _step(True)
    swa = StochasticWeightAveraging(ts, E, swa_lrs=swa_lrs, lr_scheduler=plateau_scheduler(ts.optimizer))
    assert swa.swa_start == 39
    twin = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=ts.net.hparams['lr'])
    twin_sched = ReduceLROnPlateau(twin, patience=10)
    monitored = [1.0, 0.9] + [0.9] * (E - 2)          # no improvement from epoch 2 on: cuts follow epochs 12, 23, 34
    batches = _batches(1)
    got, want = [], []
    for epoch in range(swa.epochs):
        swa.on_train_epoch_start(epoch)
        if epoch == swa.swa_start:
            twin_sched = SWALR(twin, swa_lr=twin.param_groups[0]['lr'] if swa_lrs is None else swa_lrs, anneal_epochs=10,
                               anneal_strategy='cos')
        got.append(ts.optimizer.param_groups[0]['lr'])
        want.append(twin.param_groups[0]['lr'])
        if swa.is_bn_epoch(epoch):
            swa.bn_step(batches[0])
        else:
            ts(batches[0])
        swa.on_train_epoch_end(epoch, monitored=monitored[min(epoch, E - 1)])
        if isinstance(twin_sched, ReduceLROnPlateau):
            twin_sched.step(monitored[epoch])
        else:
            twin_sched.step()
    swa.on_train_end()
    assert got == want
    assert got[12] == 1e-2 and got[13] == pytest.approx(1e-3, rel=1e-12) and got[35] == pytest.approx(1e-5, rel=1e-12)
    if swa_lrs is None:
        # SWALR towards the current rate: constant up to the rounding of its interpolation (Lightning's run has the same)
        assert all(lr == pytest.approx(got[35], rel=1e-12) for lr in got[swa.swa_start:])
    else:
        assert got[swa.swa_start] == got[35] and got[-1] == pytest.approx(swa_lrs, rel=1e-12)
        assert len(set(got[swa.swa_start:swa.swa_start + 10])) == 10


def test_swa_argument_checks():
    from dcsnet.swa import StochasticWeightAveraging
    ts = _step(False)
    for kw in ({'swa_epoch_start': 0}, {'swa_epoch_start': 1.5}, {'swa_lrs': -1.0}, {'annealing_strategy': 'step'},
               {'lr_scheduler': ReduceLROnPlateau(torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=1.0))}):
        with pytest.raises(ValueError):
            StochasticWeightAveraging(ts, 10, **kw)
    swa = StochasticWeightAveraging(ts, 10, swa_epoch_start=3)
    assert (swa.swa_start, swa.swa_end, swa.epochs) == (2, 9, 10)
    with pytest.raises(RuntimeError):
        swa.bn_step(_batches(1)[0])                  # no statistics epoch without a BatchNorm
    swa = StochasticWeightAveraging(_step(True), 10)
    swa.on_train_epoch_start(0)
    with pytest.raises(RuntimeError):
        swa.bn_step(_batches(1)[0])                  # only in epoch max_epochs
    swa = StochasticWeightAveraging(copy.copy(ts), 200)
    assert (swa.swa_start, swa.swa_end) == (159, 199) and swa.swa_end - swa.swa_start + 1 == 200 - (int(200 * 0.8) - 1)
