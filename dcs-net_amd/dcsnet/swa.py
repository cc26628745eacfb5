"""Stochastic weight averaging for the product training driver (dp.TrainStep): the reference trains with
Trainer(stochastic_weight_avg=True) (train.py:147, config.py:50), i.e. PyTorch Lightning 1.5.6's StochasticWeightAveraging()
callback with its defaults.  Lightning is not a dependency; this module restates that callback (and the part of the trainer
that steps the epoch-interval schedulers) over a TrainStep, with the hooks named after the callback's:

    step = TrainStep(net, use_graph=True)
    swa = StochasticWeightAveraging(step, config.max_epochs, lr_scheduler=plateau_scheduler(step.optimizer))
    for epoch in range(swa.epochs):
        swa.on_train_epoch_start(epoch)
        for batch in ...:
            swa.bn_step(batch) if swa.is_bn_epoch(epoch) else step(batch)
        swa.on_train_epoch_end(epoch, monitored=val_loss)
    swa.on_train_end()

Semantics (E = max_epochs, epochs counted from 0):
  * swa_start = max(int(E * swa_epoch_start) - 1, 0), swa_end = E - 1 (159 and 199 for the reference's 200 epochs).
  * Before swa_start the caller's plateau scheduler steps at every epoch end with the monitored value.  At the start of epoch
    swa_start it is swapped for SWALR(swa_lr = swa_lrs, or the optimizer's current rate when None), which steps at every epoch
    end from then on; with the defaults the rate stays constant.
  * At the start of every epoch in [swa_start, swa_end] the average is updated: the first update copies the parameters, the
    n-th later one computes avg + (p - avg) / (n + 1) in fp32.  Only parameters are averaged, never buffers.
  * A network that holds a torch _BatchNorm (R_NETWORK) gets one more epoch, number E: at its start the average is copied
    into the parameters and every BatchNorm's running statistics are reset with momentum None, so the epoch's train-mode
    forwards (bn_step: no backward, no optimizer step) leave their cumulative average; on_train_end restores the momenta.
  * Any other network (C_NETWORK: its ComplexBatchNorm2d is a plain Module) takes the average into its parameters at train
    end, after epoch swa_end; its CBN running statistics stay those of the last iterate.

The average is a device buffer in the bucket's layout; on a CUDA bucket only dcs_swa_average_f32 updates it (bit for bit the
fp32 CPU evaluation Lightning makes), the torch expression serves CPU buckets (the reference path of the CPU tests, as
TorchAdam is).  Transfers and BatchNorm resets are IN PLACE: a captured TrainStep graph holds those addresses.
"""
import re
import warnings

import torch
from torch.optim.lr_scheduler import ReduceLROnPlateau
from torch.optim.swa_utils import SWALR

from . import functional


def _avg_fn(avg, p, n_averaged):
    """Lightning 1.5.6's StochasticWeightAveraging.avg_fn (n_averaged: a long tensor, as the callback keeps it)."""
    return avg + (p - avg) / (n_averaged + 1)


class StochasticWeightAveraging:
    def __init__(self, step, max_epochs, swa_epoch_start=0.8, swa_lrs=None, annealing_epochs=10, annealing_strategy='cos',
                 lr_scheduler=None):
        # argument checks of the callback's constructor
        err = None
        if isinstance(swa_epoch_start, bool) or not isinstance(swa_epoch_start, (int, float)):
            err = f'swa_epoch_start should be a >0 integer or a float between 0 and 1, got {swa_epoch_start!r}'
        elif isinstance(swa_epoch_start, int) and swa_epoch_start < 1:
            err = f'swa_epoch_start should be a >0 integer, got {swa_epoch_start}'
        elif isinstance(swa_epoch_start, float) and not 0 < swa_epoch_start <= 1:
            err = f'swa_epoch_start should be a float between 0 and 1, got {swa_epoch_start}'
        if swa_lrs is not None and not (isinstance(swa_lrs, float) and swa_lrs > 0 or isinstance(swa_lrs, list) and
                                        all(isinstance(lr, float) and lr > 0 for lr in swa_lrs)):
            err = f'swa_lrs should be a positive float or a list of positive floats, got {swa_lrs!r}'
        if not isinstance(annealing_epochs, int) or annealing_epochs < 0:
            err = f'annealing_epochs should be a non-negative integer, got {annealing_epochs!r}'
        if annealing_strategy not in ('cos', 'linear'):
            err = f'annealing_strategy should be "cos" or "linear", got {annealing_strategy!r}'
        if int(max_epochs) < 1:
            err = f'max_epochs should be >= 1, got {max_epochs!r}'
        if lr_scheduler is not None and getattr(lr_scheduler, 'optimizer', None) is not step.optimizer:
            err = 'lr_scheduler must drive the step\'s own optimizer (TrainStep.optimizer)'
        if err:
            raise ValueError(f'StochasticWeightAveraging: {err}')
        self.step = step
        self.net, self.bucket, self.optimizer = step.net, step.bucket, step.optimizer
        self._max_epochs = int(max_epochs)
        # on_fit_start: a float is a fraction of max_epochs (1-based epoch count, as an int argument is)
        self._swa_epoch_start = (int(self._max_epochs * swa_epoch_start) if isinstance(swa_epoch_start, float)
                                 else swa_epoch_start)
        self._swa_lrs = swa_lrs
        self._annealing_epochs, self._annealing_strategy = annealing_epochs, annealing_strategy
        self.lr_scheduler = lr_scheduler          # the active epoch scheduler: the plateau one until swa_start, then SWALR
        self._bns = [m for m in self.net.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
        self.average = torch.zeros_like(self.bucket.flat)
        self.n_averaged = 0
        self.momenta = {}
        self._epoch = None

    @property
    def swa_start(self):
        return max(self._swa_epoch_start - 1, 0)

    @property
    def swa_end(self):
        return self._max_epochs - 1

    @property
    def contains_batch_norm(self):
        return bool(self._bns)

    @property
    def epochs(self):
        """Epochs to run: max_epochs, plus the statistics epoch when the network holds a torch BatchNorm."""
        return self._max_epochs + (1 if self.contains_batch_norm else 0)

    def is_bn_epoch(self, epoch):
        return self.contains_batch_norm and epoch == self.swa_end + 1

    def on_train_epoch_start(self, epoch):
        self._epoch = epoch
        if epoch == self.swa_start:
            groups = self.optimizer.param_groups
            swa_lrs = self._swa_lrs
            if swa_lrs is None:
                swa_lrs = [g['lr'] for g in groups]
            if isinstance(swa_lrs, float):
                swa_lrs = [swa_lrs] * len(groups)
            for lr, g in zip(swa_lrs, groups):
                g['initial_lr'] = lr
            self.lr_scheduler = self._new_swalr(swa_lrs)
            self.n_averaged = 0
        if self.swa_start <= epoch <= self.swa_end:
            self._update_average()
        if self.is_bn_epoch(epoch):
            self._transfer()
            self._reset_batch_norm()

    def bn_step(self, batch, batch_idx=0):
        """One forward of the statistics epoch: the training step's forward in train mode (dropout on), no backward and no
        optimizer step; each BatchNorm (momentum None) folds the batch's statistics into its cumulative average.  Eager: the
        network reads the BatchNorm counters on the host."""
        if self._epoch is None or not self.is_bn_epoch(self._epoch):
            raise RuntimeError(f'StochasticWeightAveraging.bn_step: epoch {self._epoch} is not the statistics epoch '
                               f'({self.swa_end + 1 if self.contains_batch_norm else "none: no BatchNorm"})')
        self.net.train()
        loss = self.net.training_step(batch, batch_idx)
        return None if loss is None else loss.detach()

    def on_train_epoch_end(self, epoch, monitored=None):
        """Steps the active epoch scheduler: the plateau scheduler with `monitored` (val_loss in dcs / drs mode, the epoch's
        mean speech_loss in dc / dr mode), SWALR without it."""
        sch = self.lr_scheduler
        if sch is None:
            return
        if isinstance(sch, ReduceLROnPlateau):
            if monitored is None:
                raise ValueError(f'StochasticWeightAveraging.on_train_epoch_end: epoch {epoch} needs the monitored value '
                                 'for ReduceLROnPlateau')
            sch.step(float(monitored))
        else:
            # a replayed TrainStep graph runs the optimizer without calling its step(), so torch's "scheduler stepped before
            # the optimizer" check cannot see it
            with warnings.catch_warnings():
                warnings.filterwarnings('ignore', message=re.escape('Detected call of `lr_scheduler.step()` before `optimizer.step()`'))
                sch.step()

    def on_train_end(self):
        if self.contains_batch_norm and self._epoch == self.swa_end + 1:
            for m, momentum in self.momenta.items():
                m.momentum = momentum
        elif self._epoch == self.swa_end:
            self._transfer()

    def _new_swalr(self, swa_lrs):
        return SWALR(self.optimizer, swa_lr=swa_lrs, anneal_epochs=self._annealing_epochs,
                     anneal_strategy=self._annealing_strategy,
                     last_epoch=self._max_epochs if self._annealing_strategy == 'cos' else -1)

    def state_dict(self):
        """Taken at an epoch boundary, after on_train_epoch_end: the average as {parameter name: CPU tensor} (independent of
        the bucket's layout; None before the first update), n_averaged, the last epoch, and the active epoch scheduler as
        {'kind': 'plateau' | 'swalr' | None, 'state': its state_dict()}."""
        sd = self.host_state()
        if self.n_averaged > 0:
            sd['average'] = self.average_dict(self.average.detach().cpu())
        return sd

    def host_state(self):
        """state_dict() without the average: host values only, no device read (checkpoint.CheckpointWriter takes the average
        from its snapshot and adds it with average_dict)."""
        import copy
        sch = self.lr_scheduler
        kind = None if sch is None else 'plateau' if isinstance(sch, ReduceLROnPlateau) else 'swalr'
        return {'average': None, 'n_averaged': int(self.n_averaged), 'epoch': self._epoch,
                'scheduler': {'kind': kind, 'state': None if sch is None else copy.deepcopy(sch.state_dict())}}

    def average_dict(self, host_flat):
        """{parameter name: tensor} from a CPU image of the average in the bucket's layout."""
        b = self.bucket
        return {n: host_flat[o:o + p.numel()].clone().view(p.shape) for n, o, p in zip(b.names, b.offsets, b.params)}

    def load_state_dict(self, sd):
        """In place (the average keeps its address).  A stored SWALR is rebuilt with the arguments on_train_epoch_start uses —
        the rates the optimizer's group holds, restored before this by TrainStep.load_state_dict — and then loaded; a stored
        plateau state is loaded into the caller's plateau scheduler."""
        b = self.bucket
        self.n_averaged = int(sd['n_averaged'])
        self._epoch = sd.get('epoch')
        with torch.no_grad():
            if sd.get('average') is None:
                self.average.zero_()
            else:
                missing = [n for n in b.names if n not in sd['average']]
                if missing:
                    raise ValueError(f'StochasticWeightAveraging.load_state_dict: the average lacks {missing[:3]} ... ({len(missing)})')
                host = torch.zeros(b.numel, dtype=self.average.dtype)
                for n, o, p in zip(b.names, b.offsets, b.params):
                    host[o:o + p.numel()].copy_(sd['average'][n].reshape(-1))
                self.average.copy_(host)
        kind, state = sd['scheduler']['kind'], sd['scheduler']['state']
        if kind == 'swalr':
            groups = self.optimizer.param_groups
            for g in groups:
                g.setdefault('initial_lr', g['lr'])
            rates = [g['lr'] for g in groups]
            self.lr_scheduler = self._new_swalr([float(g.get('swa_lr', g['lr'])) for g in groups])
            self.lr_scheduler.load_state_dict(state)
            for g, lr in zip(groups, rates):                # (the constructor's initial step rewrote the groups' rate)
                g['lr'] = lr
        elif kind == 'plateau':
            if not isinstance(self.lr_scheduler, ReduceLROnPlateau):
                raise ValueError('StochasticWeightAveraging.load_state_dict: the state holds a plateau scheduler; construct with '
                                 'lr_scheduler=plateau_scheduler(step.optimizer)')
            self.lr_scheduler.load_state_dict(state)
        else:
            self.lr_scheduler = None

    def _update_average(self):
        flat = self.bucket.flat
        if flat.is_cuda:
            from . import ops
            ops.swa_average(self.average, flat, self.n_averaged)
        elif self.n_averaged == 0:
            self.average.copy_(flat)
        else:
            self.average.copy_(_avg_fn(self.average, flat, torch.tensor(self.n_averaged, dtype=torch.long)))
        self.n_averaged += 1

    def _transfer(self):
        """The average into the parameters, in place (the bucket's address is what a captured step reads and writes)."""
        with torch.no_grad():
            self.bucket.flat.copy_(self.average)
        functional.bump_param_generation()

    def _reset_batch_norm(self):
        """running_mean 0, running_var 1, num_batches_tracked 0, momentum None — in place, where Lightning assigns new
        tensors: the captured step holds these buffers' addresses."""
        self.momenta = {}
        with torch.no_grad():
            for m in self._bns:
                if m.track_running_stats:
                    m.running_mean.zero_()
                    m.running_var.fill_(1.0)
                    m.num_batches_tracked.zero_()
                self.momenta[m] = m.momentum
                m.momentum = None
        functional.note_state_update()        # whatever eval mode derived from the old statistics is stale
