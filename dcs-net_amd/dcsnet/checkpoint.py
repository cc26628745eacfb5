"""Checkpoint and resume of a training run (dp.TrainStep + swa.StochasticWeightAveraging): DESIGN.md §6f.

The file is PyTorch Lightning 1.5.6's checkpoint layout — what the reference's Trainer writes (train.py:141-150) — so that
C_NETWORK.load_from_checkpoint / R_NETWORK.load_from_checkpoint, tools/enhance.py and tools/evaluate.py read it unchanged, and
so that a checkpoint of the reference's own training (its 'optimizer_states' and 'lr_schedulers' included) continues here:

    epoch, global_step, pytorch-lightning_version '1.5.6', state_dict, optimizer_states [torch.optim.Adam's state_dict],
    lr_schedulers [the active epoch scheduler's state_dict], callbacks {}, hyper_parameters dict(net.hparams)

plus ONE project key, 'dcsnet': {format, counters (TrainStep.state_dict), swa (StochasticWeightAveraging.state_dict), generator
(the data generator's get_state()), rng (torch's CPU and device generator states), mode, conv_precision, activation_dtype, extra}.

  save_checkpoint    synchronous: reads the device, refuses non-finite state (NonFiniteState, nothing written), writes to a
                     temporary file and os.replace()s it — a reader never sees half a file, a crash never costs the last one
  load_checkpoint    restores everything IN PLACE (a captured graph holds the addresses); returns epoch / global_step / extra
  CheckpointWriter   the same file without stopping the stream: ONE dcs_snapshot_words launch images the step's device state
                     into a staging slab between two graph replays, a side stream copies the slab to pinned memory, and a
                     writer thread — which never calls into the HIP runtime — assembles and writes the file

What resuming promises (and what it does not) is stated in DESIGN.md §6f: bit-for-bit continuation within one execution schedule
(replay against replay, eager against eager), not across them.
"""
import os
import threading
import warnings

import torch

from . import _lib

FORMAT = 1
LIGHTNING_VERSION = '1.5.6'


class NonFiniteState(RuntimeError):
    """A tensor of the state to be saved holds NaN or +-Inf; `counts` = {tensor path: number of non-finite values}."""

    def __init__(self, counts):
        self.counts = dict(counts)
        super().__init__('refusing to write a checkpoint with non-finite state: ' +
                         ', '.join(f'{k} ({v})' for k, v in list(self.counts.items())[:6]) +
                         (' ...' if len(self.counts) > 6 else ''))


def _walk_tensors(obj, path=''):
    if torch.is_tensor(obj):
        yield path, obj
    elif isinstance(obj, dict):
        for k, v in obj.items():
            yield from _walk_tensors(v, f'{path}/{k}' if path else str(k))
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from _walk_tensors(v, f'{path}/{i}')


def nonfinite_counts(ckpt):
    """{path: count} over the float tensors of the trained state (weights, buffers, moments, the SWA average)."""
    counts = {}
    for part in ('state_dict', 'optimizer_states'):
        for path, t in _walk_tensors(ckpt.get(part), part):
            if t.is_floating_point() or t.is_complex():
                n = int((~torch.isfinite(torch.view_as_real(t) if t.is_complex() else t)).sum())
                if n:
                    counts[path] = n
    swa = (ckpt.get('dcsnet') or {}).get('swa') or {}
    for path, t in _walk_tensors(swa.get('average'), 'dcsnet/swa/average'):
        n = int((~torch.isfinite(t)).sum())
        if n:
            counts[path] = n
    return counts


def _meta(step):
    """The settings a checkpoint is only valid under: host values."""
    from . import ops
    from .network_functions import _mode
    return {'mode': _mode(), 'conv_precision': ops.conv_precision() if step.bucket.flat.is_cuda else None,
            'activation_dtype': str(getattr(step.net, 'activation_dtype', torch.float32)), 'rng': _rng_state(step)}


def _rng_state(step):
    """torch's generators: DR-Net's dropout is ATen's and draws from the device generator (C_NETWORK's masks come from the
    counters), and a data pipeline may draw from the CPU one.  Host values: reading a generator's state touches no stream."""
    flat = step.bucket.flat
    return {'cpu': torch.get_rng_state(), 'cuda': torch.cuda.get_rng_state(flat.device) if flat.is_cuda else None}


def _assemble(net_sd, opt_sd, counters, swa_sd, hparams, meta, epoch, global_step, generator_state, extra):
    """The checkpoint dict from CPU values only (the writer thread runs this)."""
    sched = (swa_sd or {}).get('scheduler') or {}
    return {'epoch': int(epoch), 'global_step': int(global_step), 'pytorch-lightning_version': LIGHTNING_VERSION,
            'state_dict': net_sd, 'optimizer_states': [opt_sd],
            'lr_schedulers': [sched['state']] if sched.get('state') is not None else [],
            'callbacks': {}, 'hyper_parameters': hparams,
            'dcsnet': dict(meta, format=FORMAT, counters=counters, swa=swa_sd, generator=generator_state, extra=extra)}


def _write(ckpt, path):
    tmp = f'{path}.tmp.{os.getpid()}'
    try:
        torch.save(ckpt, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def save_checkpoint(path, step, swa=None, epoch=0, global_step=0, generator=None, extra=None):
    """Synchronous.  Raises NonFiniteState and writes nothing when a float tensor of the state is not finite: a checkpoint of
    NaN weights must never replace the last good one."""
    from collections import OrderedDict
    net = step.net
    net_sd = OrderedDict((k, v.detach().cpu().clone()) for k, v in net.state_dict().items())
    ts = step.state_dict()
    ckpt = _assemble(net_sd, ts['optimizer'], ts['counters'], None if swa is None else swa.state_dict(), dict(net.hparams),
                     _meta(step), epoch, global_step, None if generator is None else generator.get_state().clone(), extra)
    bad = nonfinite_counts(ckpt)
    if bad:
        raise NonFiniteState(bad)
    _write(ckpt, path)
    return path


def load_checkpoint(path, step, swa=None, generator=None):
    """Restore weights, buffers, optimizer, counters, SWA, scheduler and generator IN PLACE from `path`; returns
    {'epoch', 'global_step', 'extra'}.  A file without the 'dcsnet' key (the reference's own checkpoint) restores the weights,
    the optimizer, the scheduler and the epoch, and sets the counters to updates = the optimizer's step, seed_state = 0.
    Refuses a file whose mode, activation dtype or set of state_dict names differs from the live step's."""
    ckpt = torch.load(path, map_location='cpu', weights_only=False)
    if not isinstance(ckpt, dict) or 'state_dict' not in ckpt:
        raise KeyError(f"{path}: not a Lightning checkpoint (no 'state_dict')")
    net = step.net
    own = ckpt.get('dcsnet')
    live = set(net.state_dict())
    if set(ckpt['state_dict']) != live:
        diff = sorted(set(ckpt['state_dict']) ^ live)
        raise ValueError(f'{path}: the parameter names differ from the network\'s ({len(diff)}: {diff[:4]} ...)')
    if own is not None:
        if own.get('format') != FORMAT:
            raise ValueError(f"{path}: checkpoint format {own.get('format')!r}, this build reads {FORMAT}")
        meta = _meta(step)
        for k in ('mode', 'activation_dtype'):
            if own.get(k) != meta[k]:
                raise ValueError(f'{path}: saved with {k} = {own.get(k)!r}, the live step runs {meta[k]!r}')
        if own.get('conv_precision') != meta['conv_precision'] and None not in (own.get('conv_precision'), meta['conv_precision']):
            warnings.warn(f"{path}: saved with conv precision {own.get('conv_precision')!r}, the process runs "
                          f"{meta['conv_precision']!r}; training continues at the latter")
    if not ckpt.get('optimizer_states'):
        raise KeyError(f"{path}: no 'optimizer_states'; load weights alone with load_from_checkpoint")
    net.load_state_dict(ckpt['state_dict'], strict=True)            # copy_ in place: the bucket's views keep their storage
    step.load_state_dict({'optimizer': ckpt['optimizer_states'][0],
                          'counters': own['counters'] if own is not None else {'seed_state': 0}})
    if swa is not None:
        if own is not None and own.get('swa') is not None:
            swa.load_state_dict(own['swa'])
        elif ckpt.get('lr_schedulers') and swa.lr_scheduler is not None:
            swa.lr_scheduler.load_state_dict(ckpt['lr_schedulers'][0])
    if generator is not None and own is not None and own.get('generator') is not None:
        generator.set_state(own['generator'])
    rng = None if own is None else own.get('rng')
    if rng is not None:
        torch.set_rng_state(rng['cpu'])
        if rng.get('cuda') is not None and step.bucket.flat.is_cuda:
            torch.cuda.set_rng_state(rng['cuda'], step.bucket.flat.device)
    return {'epoch': ckpt.get('epoch', 0), 'global_step': ckpt.get('global_step', 0),
            'extra': None if own is None else own.get('extra')}


class _Job:
    def __init__(self, path, host):
        self.path, self.host = path, host
        self.cloned, self.done = threading.Event(), threading.Event()
        self.counts, self.error, self.written = None, None, False


class CheckpointWriter:
    """Checkpoints of a live, graph-replaying TrainStep without stopping its stream.

        writer = CheckpointWriter(step, swa)
        ...
        writer.save(path, epoch=e, global_step=g)       # returns at once; training continues
        ...
        writer.close()                                  # waits for the last file

    save() issues ONE snapshot launch (ops.snapshot) on the current stream into the device slab — the bucket's four buffers,
    the SWA average, every state_dict entry outside the bucket, t_dev and the seed offset — records an event, has a side
    stream copy slab and non-finite counters to pinned memory behind it, and returns without synchronising.  The main thread
    polls the copy's event in poll(), the next save() and close(); once it has landed the pinned image goes to the writer
    thread, which clones it, assembles the dict, torch.save()s to a temporary file and os.replace()s it.  The thread touches
    CPU memory only and never calls into the HIP runtime: a call from a second thread would break a graph capture that other
    code of this project makes in the global capture mode.

    There is ONE slab and ONE pinned image: a second save() while one is in flight first WAITS (event.synchronize() on the
    calling thread, then the thread's clone) until the earlier image has been handed over — checkpoints closer together than
    one device-to-host copy cost that copy's time.  A non-zero non-finite count means nothing is written and the previous
    file stays: (path, {tensor: count}) is appended to `rejected`, with a warning, when the main thread next polls.
    Small host-side state (scheduler dicts, generator state, epoch, learning rate, call counts) is captured at the save() call.
    asynchronous=False makes save() wait for its own file."""

    def __init__(self, step, swa=None, asynchronous=True):
        from .dp import FusedAdam
        if not step.bucket.flat.is_cuda or not isinstance(step.opt, FusedAdam):
            raise _lib.DcsHipError('CheckpointWriter: needs a CUDA (HIP) TrainStep with FusedAdam; the snapshot has no CPU fallback '
                                   '(use save_checkpoint)')
        self.step, self.swa, self.asynchronous = step, swa, bool(asynchronous)
        self.rejected, self.written = [], []
        self._table = None
        self._side = torch.cuda.Stream(device=step.bucket.flat.device)
        self._copied = torch.cuda.Event()
        self._pending = None            # a job whose device-to-host copy has been issued and not yet handed over
        self._jobs = []                 # handed over, not yet reaped
        self._queue, self._thread = [], None
        self._cv = threading.Condition()
        self._closed = False
        self._build()

    # ---- device side (calling thread only) ---------------------------------------------------------------------------
    def _sources(self):
        step, opt = self.step, self.step.opt
        hot = set(step.bucket.names)
        sd = step.net.state_dict()
        self._order = list(sd)
        self._others = [(k, v) for k, v in sd.items() if k not in hot]
        named = [('state_dict (parameters)', step.bucket.flat), ('optimizer_states/exp_avg', opt.m),
                 ('optimizer_states/exp_avg_sq', opt.v), ('optimizer_states/max_exp_avg_sq', opt.vmax)]
        if self.swa is not None:
            named.append(('dcsnet/swa/average', self.swa.average))
        named += [(f'state_dict/{k}', v) for k, v in self._others]
        named += [('t_dev', opt.t_dev), ('seed_state', step.seed_state)]
        return named

    def _build(self):
        from . import ops
        named = self._sources()
        self._names = [n for n, _ in named]
        self._table = ops.snapshot_table([t for _, t in named])
        dev = self.step.bucket.flat.device
        words = max(self._table.total_words, 4)
        self._slab = torch.empty(words, dtype=torch.int32, device=dev)
        self._counts = torch.zeros(self._table.n, dtype=torch.int32, device=dev)
        self._host_slab = torch.empty(words, dtype=torch.int32, pin_memory=True)
        self._host_counts = torch.zeros(self._table.n, dtype=torch.int32, pin_memory=True)

    def _stale(self):
        """A buffer that was replaced rather than updated in place since the table was built (load_state_dict(assign=True),
        .to()): its old address must not be read."""
        now = self._sources()
        return [n for n, _ in now] != self._names or any(a.data_ptr() != b.data_ptr() or a.shape != b.shape
                                                         for (_, a), b in zip(now, self._table.tensors))

    @property
    def bytes_per_checkpoint(self):
        return 4 * self._table.total_words

    def save(self, path, epoch=0, global_step=0, generator=None, extra=None):
        if self._closed:
            raise RuntimeError('CheckpointWriter.save after close()')
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('CheckpointWriter.save under stream capture')
        from . import ops
        self._hand_over(wait=True)                      # one slab, one pinned image: the earlier one must be out of both
        for job in self._jobs:
            job.cloned.wait()
        self._reap()
        if self._stale():
            torch.cuda.current_stream().synchronize()
            self._build()
        step, opt, swa = self.step, self.step.opt, self.swa
        # host-side state, as of this call
        host = {'group': opt.export_group(),
                'counters': {'calls': int(opt.t), 'drop_calls': getattr(step.net, '_drop_calls', None),
                             'torch_initial_seed': torch.initial_seed()},
                'swa': None if swa is None else swa.host_state(), 'hparams': dict(step.net.hparams), 'meta': _meta(step),
                'epoch': epoch, 'global_step': global_step, 'extra': extra,
                'generator': None if generator is None else generator.get_state().clone()}
        main = torch.cuda.current_stream()
        main.wait_event(self._copied)                   # (the slab's previous copy: long done, see _hand_over above)
        ops.snapshot(self._table, self._slab, self._counts)
        taken = torch.cuda.Event()
        taken.record(main)
        self._side.wait_event(taken)
        with torch.cuda.stream(self._side):
            self._host_slab.copy_(self._slab, non_blocking=True)
            self._host_counts.copy_(self._counts, non_blocking=True)
            self._copied.record(self._side)
        self._pending = _Job(path, host)
        if not self.asynchronous:
            self._hand_over(wait=True)
            self._jobs[-1].done.wait()
            self._reap()

    def poll(self):
        """Hand a landed image to the writer thread and report finished files; never blocks.  True while work is in flight."""
        self._hand_over(wait=False)
        self._reap()
        return self._pending is not None or bool(self._jobs)

    def close(self):
        """Wait for everything in flight, stop the thread, raise what it raised."""
        if self._closed:
            return
        self._hand_over(wait=True)
        with self._cv:
            self._closed = True
            self._cv.notify_all()
        if self._thread is not None:
            self._thread.join()
        self._reap()

    def _hand_over(self, wait):
        job = self._pending
        if job is None:
            return
        if wait:
            self._copied.synchronize()
        elif not self._copied.query():
            return
        self._pending = None
        self._jobs.append(job)
        if self._thread is None:
            self._thread = threading.Thread(target=self._run, name='dcsnet-checkpoint-writer', daemon=True)
            self._thread.start()
        with self._cv:
            self._queue.append(job)
            self._cv.notify_all()
        if wait:
            job.cloned.wait()                           # the pinned image is free for the next copy

    def _reap(self):
        for job in [j for j in self._jobs if j.done.is_set()]:
            self._jobs.remove(job)
            if job.error is not None:
                raise job.error
            if job.written:
                self.written.append(job.path)
            else:
                self.rejected.append((job.path, job.counts))
                warnings.warn(f'CheckpointWriter: {job.path} not written, non-finite state: {job.counts}; the previous file stays')

    # ---- writer thread: CPU memory only, no call into the HIP runtime -----------------------------------------------------
    def _run(self):
        while True:
            with self._cv:
                while not self._queue and not self._closed:
                    self._cv.wait()
                if not self._queue:
                    return
                job = self._queue.pop(0)
            try:
                self._write_job(job)
            except BaseException as e:                  # noqa: BLE001 - handed to the calling thread (_reap)
                job.error = e
            finally:
                job.cloned.set()
                job.done.set()

    def _write_job(self, job):
        from collections import OrderedDict
        table, names, step, swa = self._table, self._names, self.step, self.swa
        slab = torch.empty(self._host_slab.shape, dtype=torch.int32).copy_(self._host_slab)       # pageable CPU copies
        counts = torch.empty(self._host_counts.shape, dtype=torch.int32).copy_(self._host_counts)
        job.cloned.set()
        image = {n: table.view(slab, i) for i, n in enumerate(names)}
        host = job.host
        averaging = swa is not None and host['swa']['n_averaged'] > 0
        bad = {n: int(c) for n, c in zip(names, counts.tolist()) if c != 0 and (n != 'dcsnet/swa/average' or averaging)}
        if bad:
            job.counts = bad
            return
        b = step.bucket
        flat = image['state_dict (parameters)']
        where = {n: (o, p.numel(), p.shape) for n, o, p in zip(b.names, b.offsets, b.params)}
        net_sd = OrderedDict()
        for k in self._order:                           # the network's own state_dict order
            if k in where:
                o, n, shape = where[k]
                net_sd[k] = flat[o:o + n].clone().view(shape)
            else:
                net_sd[k] = image[f'state_dict/{k}'].clone()
        updates = int(image['t_dev'][0])
        opt_sd = step.opt.export_images(image['optimizer_states/exp_avg'], image['optimizer_states/exp_avg_sq'],
                                        image['optimizer_states/max_exp_avg_sq'], updates, host['group'])
        swa_sd = host['swa']
        if averaging:
            swa_sd['average'] = swa.average_dict(image['dcsnet/swa/average'])
        counters = dict(host['counters'], updates=updates, seed_state=int(image['seed_state'][0]))
        ckpt = _assemble(net_sd, opt_sd, counters, swa_sd, host['hparams'], host['meta'], host['epoch'], host['global_step'],
                         host['generator'], host['extra'])
        _write(ckpt, job.path)
        job.written = True
