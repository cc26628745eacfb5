"""The validation epoch on the device: one host read per epoch.

    v = DeviceValidator(net, val_store, batch_size, seed=config.seed, prefix='val', use_graph=False, extended=False)
    metrics = v.run(epoch)          # {'val_loss', 'val_noise_loss', 'val_speech_loss', 'val_pesq', 'val_stoi'[, 'val_estoi']}
    v.counts                        # {'batches', 'skipped', 'nan_scores'} of that run

fit.validate is the reference's host procedure: per batch the unfused step (five waveforms synthesised one by one, the target
mask), five [B, L] waveforms copied to the host for a logger that is not there, and STOI utterance by utterance in numpy.  Here
a batch is: audio_store's one launch into the validator's own static buffers; the train step's fused pair route
(network_functions._step with need_noisy_audio=False) and calc_loss; metrics.stoi_batch; and ops.val_accumulate, which folds the
batch into a 16-double device state by the reference's rule (fold_batches below restates it on the host).  Nothing in the
batch loop reads from the device; run() ends with one copy of the state.

Same data as fit.validate: val_store.epoch(batch_size, shuffle=False) and crops from a generator seeded by (seed, epoch), so epoch
e is validated on the same crops by either route.  {prefix}_pesq is ALWAYS NaN on this route: there is no device PESQ (the host
route gives NaN as well wherever pypesq is not installed).  extended=True adds {prefix}_estoi (metrics.stoi_batch(...,
extended='both'): a second score row in the same accumulator launch); the host route has no ESTOI.

Graph capture (use_graph=True): the full-batch path — step, losses, STOI, accumulate — is one graph; store.batch stays outside,
as in training.  Captured as enhance.Enhancer._step_fn captures: one eager warm pass, a second inside _derived.collect() whose
list is kept alive, then the capture; the graph is valid for one state key (F.state_generation(), the conv precision, the
activation dtype, the mode, (id, _version, data_ptr) of every parameter and buffer).  Training rewrites parameters, running
statistics and packed weights behind torch's back at every step, so the key differs at every epoch and run() recaptures: a graph
is never replayed over a stale key.  A partial last batch runs eagerly on its own tensors into the same state.
use_graph defaults to False: a recapture costs about 19 ms (two warm passes and the capture) and a replay saves about 1.4 ms
per batch over the eager launches, so at the 8 batches of tools/validation_bench.py the captured route loses (30.6 ms against
22.5 ms) and only from about 14 full batches on does it win (32 batches: 61.6 ms against 74.2 ms; profiles/validation_bench.json,
DESIGN.md §6f).  Pass use_graph=True for long validation sets.

Validation leaves training alone: its own generator, no dropout draw in eval() (no _drop_calls advance), net._dcs_skip_flag is
neither set nor written, the train graph's static buffers are not used.
"""
import math

import torch

from . import _derived
from . import functional as F
from . import metrics as _metrics
from . import ops
from .config import config as _config
from .network_functions import _mode, _step, calc_loss

LOSS_SUM, SCORE_SUM, KEPT, SKIPPED, SCORE_NAN = (ops.VAL_LOSS_SUM, ops.VAL_SCORE_SUM, ops.VAL_KEPT, ops.VAL_SKIPPED,
                                                 ops.VAL_SCORE_NAN)


def fold_batches(rows):
    """The fold rule of dcs_val_accumulate_f32 on the host, in double: rows = [(losses, scores), ...] per batch, losses a
    sequence of 3 (noise, speech, total) or 1 (speech) numbers, scores a sequence of per-utterance score rows.  -> the state
    as a list of ops.VAL_STATE floats (layout: include/dcsnet_hip.h).  A NaN monitored loss (the last component) skips the batch;
    a kept batch adds its losses and, per score row, the mean of the non-NaN entries over max(their count, 1)."""
    state = [0.0] * ops.VAL_STATE
    for losses, scores in rows:
        losses = [float(v) for v in losses]
        if losses[-1] != losses[-1]:
            state[SKIPPED] += 1.0
            continue
        state[KEPT] += 1.0
        for k, v in enumerate(losses):
            state[LOSS_SUM + k] += v
        for r, row in enumerate(scores):
            row = [float(v) for v in row]
            vals = [v for v in row if v == v]
            state[SCORE_SUM + r] += math.fsum(vals) / max(len(vals), 1)
            state[SCORE_NAN + r] += float(len(row) - len(vals))
    return state


def epoch_means(state, n_loss, n_scores):
    """(loss means, score means) = sums / kept, in double; None when no batch was kept."""
    kept = float(state[KEPT])
    if kept == 0:
        return None
    return ([float(state[LOSS_SUM + k]) / kept for k in range(n_loss)],
            [float(state[SCORE_SUM + r]) / kept for r in range(n_scores)])


class DeviceValidator:
    """net: a C_NETWORK or R_NETWORK on a CUDA (HIP) device; val_store: an audio_store.DeviceAudioStore on the same device.
    The mode ('dcs' / 'drs': three losses; 'dc' / 'dr': the speech loss) is read from sys.argv[1] at every run, as the model code
    reads it."""

    def __init__(self, net, val_store, batch_size, seed=_config.seed, prefix='val', use_graph=False, extended=False):
        if int(batch_size) < 1:
            raise ValueError(f'DeviceValidator: batch_size={batch_size}')
        self.net, self.store, self.batch_size = net, val_store, int(batch_size)
        self.seed, self.prefix, self.use_graph, self.extended = int(seed), str(prefix), bool(use_graph), bool(extended)
        self.device = dev = val_store.device
        self.counts = {'batches': 0, 'skipped': 0, 'nan_scores': 0}
        self._state = torch.zeros(ops.VAL_STATE, dtype=torch.float64, device=dev)
        self._warm_state = torch.zeros_like(self._state)            # the warm passes before a capture keep their own books
        # noise | clean | noisy in one allocation, as dp.TrainStep lays out its inputs: the two targets are synthesised as one
        # batch of 2B signals without a concatenation (network_functions._stacked)
        buf = torch.zeros((3, self.batch_size, 256, val_store.T), dtype=torch.complex64, device=dev)
        self._static = (buf[0], buf[2], buf[1])                     # (noise, noisy, clean)
        self._graph = self._graph_key = self._keep = None

    # ---- one batch -------------------------------------------------------------------------------------------------------

    def _batch(self, noise, noisy, clean, state):
        """Step, losses, STOI, accumulate: device work only."""
        net = self.net
        a = _step(net, net._step_dtype, noise, noisy, clean, need_noisy_audio=False)
        out = calc_loss(net, **a)
        parts = out if isinstance(out, (tuple, list)) else (out,)
        losses = torch.stack([t.detach().reshape(()) for t in parts]).to(torch.float32)
        scores = _metrics.stoi_batch(a['clean_audio'], a['predict_clean_audio'], net.config.sr,
                                     extended='both' if self.extended else False)
        scores = torch.stack(scores) if self.extended else scores.unsqueeze(0)
        ops.val_accumulate(losses, scores, state)

    def _run_static(self, state):
        self._batch(*self._static, state)

    def _state_key(self):
        net = self.net
        tensors = list(net.parameters()) + list(net.buffers())
        return (F.state_generation(), ops.conv_precision(), getattr(net, 'activation_dtype', None), _mode(), self.extended,
                tuple((id(t), t._version, t.data_ptr()) for t in tensors))

    def _step_fn(self):
        """The full-batch callable on the static buffers (which hold a real batch by now).  Captured once per state key, as
        Enhancer._step_fn: two eager warm passes first — the first fills the cache of packed weights and inference constants, the
        second is served from it exactly what the graph will read."""
        if not self.use_graph:
            return lambda: self._run_static(self._state)
        key = self._state_key()
        if self._graph is None or key != self._graph_key:
            self._graph = None
            self._run_static(self._warm_state)
            with _derived.collect() as kept:
                self._run_static(self._warm_state)
            torch.cuda.synchronize(self.device)
            self._keep = kept
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._run_static(self._state)
            self._graph, self._graph_key = g, self._state_key()
        return self._graph.replay

    # ---- public ----------------------------------------------------------------------------------------------------------

    def run(self, epoch):
        """One validation epoch -> {metric: mean over the kept batches} as Python floats ({} when no batch was kept)."""
        gen = torch.Generator().manual_seed((self.seed * 1000003 + int(epoch)) & 0x7FFFFFFFFFFFFFFF)
        net, store, B = self.net, self.store, self.batch_size
        pair = _mode() in ('dcs', 'drs')
        was_training = net.training
        net.eval()
        try:
            with torch.no_grad():
                self._state.zero_()
                step = None
                for idx in store.epoch(B, shuffle=False):
                    if not idx:
                        continue
                    if len(idx) == B:
                        store.batch(idx, generator=gen, out=self._static)
                        if step is None:
                            step = self._step_fn()
                        step()
                    else:                                          # the partial last batch: eagerly, on its own tensors
                        noise, noisy, clean, _ = store.batch(idx, generator=gen)
                        self._batch(noise, noisy, clean, self._state)
                state = self._state.cpu().tolist()                 # the epoch's one host read
        finally:
            net.train(was_training)
        n_loss, n_scores = (3 if pair else 1), (2 if self.extended else 1)
        self.counts = {'batches': int(state[KEPT]), 'skipped': int(state[SKIPPED]),
                       'nan_scores': int(sum(state[SCORE_NAN:SCORE_NAN + n_scores]))}
        means = epoch_means(state, n_loss, n_scores)
        if means is None:
            return {}
        loss, score = means
        p = self.prefix
        if pair:
            out = {f'{p}_loss': loss[2], f'{p}_noise_loss': loss[0], f'{p}_speech_loss': loss[1]}
        else:
            out = {f'{p}_speech_loss': loss[0]}
        out[f'{p}_pesq'] = float('nan')                            # no device PESQ
        out[f'{p}_stoi'] = score[0]
        if self.extended:
            out[f'{p}_estoi'] = score[1]
        return out
