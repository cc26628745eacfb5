"""The training loop of the recipe over device-resident audio, with checkpoints: store -> step -> schedule -> SWA -> files.

    fit(net, train_store, val_store, out_dir, max_epochs, batch_size, resume='auto')

is what the reference's Trainer.fit does for this model (train.py:141-150), restated over dp.TrainStep,
swa.StochasticWeightAveraging and checkpoint.CheckpointWriter.  Per epoch: on_train_epoch_start; the training batches
(audio_store.DeviceAudioStore.epoch / .batch, written straight into the captured step's input buffers; the statistics epoch
of a network with a torch BatchNorm runs swa.bn_step instead); validation in eval() under no_grad through net.validation_step
over val_store, unshuffled, crop starts from a generator seeded by (seed, epoch); the monitored value as the reference chooses
it (mean val_loss in dcs / drs mode, the epoch's mean speech_loss in dc / dr mode); on_train_epoch_end; last.ckpt through the
writer, best.ckpt when the monitored value improved; one JSON line appended to metrics.jsonl.  After the last epoch
on_train_end() and a synchronous final.ckpt: it holds the SWA weights and is what the enhancement tools should load.

validation='device' replaces the validation pass by validation.DeviceValidator: the same crops, losses, STOI and the epoch's
means on the device, one host read per epoch; 'host', the default, is the pass described above.

Checkpoints are taken at epoch boundaries; resume='auto' continues from out_dir/last.ckpt when it exists (a path: from that
file).  In a multi-rank run every rank loads and rank 0 writes (untested: one GPU per machine).  What a resumed run reproduces
is stated in DESIGN.md §6f.
"""
import json
import os

import torch
import torch.distributed as dist

from .config import config as _config


def _rank_world():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _mean(values):
    """Mean of the finite entries of a list of 0-dim tensors (a NaN loss skipped its update: c_network.py:257-261); one host
    read per epoch."""
    vals = [v.detach().float().reshape(()) for v in values if v is not None]
    if not vals:
        return float('nan')
    t = torch.stack(vals)
    ok = torch.isfinite(t)
    return float(t[ok].mean()) if bool(ok.any()) else float('nan')


def validate(net, val_store, batch_size, seed, epoch):
    """The validation epoch: {metric: mean over the batches}.  Unshuffled; crop starts from a generator seeded by (seed, epoch),
    so every run — resumed or not — validates epoch e on the same crops."""
    gen = torch.Generator().manual_seed((int(seed) * 1000003 + int(epoch)) & 0x7FFFFFFFFFFFFFFF)
    was_training = net.training
    net.eval()
    outs = []
    try:
        with torch.no_grad():
            for i, idx in enumerate(val_store.epoch(batch_size, shuffle=False)):
                noise, noisy, clean, _ = val_store.batch(idx, generator=gen)
                out = net.validation_step((noise, noisy, clean, idx), i)
                if out is not None:
                    outs.append(out[1])
    finally:
        net.train(was_training)
    keys = outs[0].keys() if outs else []
    return {k: float(torch.stack([torch.as_tensor(o[k]).float().cpu() for o in outs]).mean()) for k in keys}


VALIDATION = ('host', 'device')


def fit(net, train_store, val_store, out_dir, max_epochs, batch_size, use_graph=True, resume=None, seed=_config.seed,
        stop_after_epoch=None, log=print, validation='host'):
    """Train `net` for max_epochs (plus the statistics epoch where SWA needs one); returns a summary dict: epoch (the last one
    run), global_step, lr, scheduler ('plateau' | 'swalr' | None), n_averaged, best, finished, and the live `step` / `swa`.
    stop_after_epoch: return after that epoch's checkpoint — the process can stop at any epoch boundary.
    validation: 'host' — validate() below, the reference's procedure — or 'device': one validation.DeviceValidator for the run (the
    same crops; losses, STOI and the epoch's means on the device, one host read per epoch, val_pesq NaN); the metrics line then
    also carries val_skipped."""
    if validation not in VALIDATION:
        raise ValueError(f'fit: validation={validation!r}: expected one of {VALIDATION}')
    from ._pl_compat import seed_everything
    from .checkpoint import CheckpointWriter, load_checkpoint, save_checkpoint
    from .dp import TrainStep, plateau_scheduler
    from .network_functions import _mode
    from .swa import StochasticWeightAveraging
    rank, world = _rank_world()
    os.makedirs(out_dir, exist_ok=True)
    seed_everything(seed)
    step = TrainStep(net.train(), use_graph=use_graph)
    swa = StochasticWeightAveraging(step, max_epochs, lr_scheduler=plateau_scheduler(step.optimizer))
    gen = torch.Generator().manual_seed(int(seed))             # the epoch orders and the training crops
    last, best_path, final = (os.path.join(out_dir, n) for n in ('last.ckpt', 'best.ckpt', 'final.ckpt'))
    metrics_path = os.path.join(out_dir, 'metrics.jsonl')
    start, global_step, best = 0, 0, None
    if resume == 'auto':
        resume = last if os.path.exists(last) else None
    if resume is not None:
        info = load_checkpoint(resume, step, swa, generator=gen)
        start, global_step = int(info['epoch']) + 1, int(info['global_step'])
        best = (info['extra'] or {}).get('best')
        log(f'[fit] resumed {resume}: epoch {start}, step {global_step}, lr {step.optimizer.param_groups[0]["lr"]:g}')
        if rank == 0 and os.path.exists(metrics_path):          # lines of epochs the checkpoint does not hold are run again
            kept = [ln for ln in open(metrics_path) if ln.strip() and json.loads(ln)['epoch'] < start]
            with open(metrics_path, 'w') as f:
                f.writelines(kept)
    elif rank == 0 and os.path.exists(metrics_path):
        os.remove(metrics_path)
    writer = CheckpointWriter(step, swa) if rank == 0 and step.bucket.flat.is_cuda else None
    validates = _mode() in ('dcs', 'drs')
    validator = None
    if validation == 'device' and val_store is not None:
        from .validation import DeviceValidator
        validator = DeviceValidator(net, val_store, batch_size, seed=seed)
    epoch = start - 1
    try:
        for epoch in range(start, swa.epochs):
            swa.on_train_epoch_start(epoch)
            net.train()
            statistics = swa.is_bn_epoch(epoch)
            losses = []
            for i, idx in enumerate(train_store.epoch(batch_size, generator=gen, rank=rank, world=world)):
                if not idx:
                    continue
                bufs = step.input_buffers()
                fits = bufs is not None and tuple(bufs[0].shape) == (len(idx), 256, train_store.T)
                out = bufs if fits and not statistics else None           # (a partial last batch runs eagerly on its own tensors)
                noise, noisy, clean, _ = train_store.batch(idx, generator=gen, out=out)
                batch = (noise, noisy, clean, idx)
                if statistics:
                    losses.append(swa.bn_step(batch, i))
                else:
                    losses.append(step(batch, i))
                    global_step += 1
                if writer is not None:
                    writer.poll()
            train_loss = _mean(losses)
            if validator is not None:
                val = dict(validator.run(epoch), val_skipped=validator.counts['skipped'])
            else:
                val = validate(net, val_store, batch_size, seed, epoch) if val_store is not None else {}
            monitored = val.get('val_loss', train_loss) if validates else train_loss
            swa.on_train_epoch_end(epoch, monitored=monitored)
            improved = monitored == monitored and (best is None or monitored < best)
            if improved:
                best = monitored
            lr = step.optimizer.param_groups[0]['lr']
            if rank == 0:
                extra = {'best': best, 'monitored': monitored}
                for path in (last, best_path) if improved else (last,):
                    if writer is not None:
                        writer.save(path, epoch=epoch, global_step=global_step, generator=gen, extra=extra)
                    else:
                        save_checkpoint(path, step, swa, epoch=epoch, global_step=global_step, generator=gen, extra=extra)
                with open(metrics_path, 'a') as f:
                    f.write(json.dumps(dict(val, epoch=epoch, global_step=global_step, train_loss=train_loss,
                                            monitored=monitored, lr=lr, n_averaged=swa.n_averaged, improved=improved)) + '\n')
            log(f'[fit] epoch {epoch}: train {train_loss:.4f}, monitored {monitored:.4f}, lr {lr:g}' +
                (' (statistics epoch)' if statistics else ''))
            if stop_after_epoch is not None and epoch >= stop_after_epoch:
                break
    finally:
        if writer is not None:
            writer.close()
    finished = epoch >= swa.epochs - 1
    if finished:
        swa.on_train_end()
        if rank == 0:
            save_checkpoint(final, step, swa, epoch=epoch, global_step=global_step, generator=gen, extra={'best': best})
    sch = swa.host_state()['scheduler']['kind']
    return {'epoch': epoch, 'global_step': global_step, 'lr': step.optimizer.param_groups[0]['lr'], 'scheduler': sch,
            'n_averaged': swa.n_averaged, 'best': best, 'finished': finished, 'step': step, 'swa': swa,
            'rejected': [] if writer is None else list(writer.rejected)}
