"""Whole recordings in, enhanced waveforms out, on the device.

    enh = Enhancer(net, mode='dcs', segment_frames=2000, overlap_frames=300, batch_segments=16, use_graph=True)
    speech = enh(waves, sample_rate=48000)             list of 1-D float32 / int16 arrays or tensors
                                                        -> list of 1-D float32 device tensors at config.sr
    speech, noise = enh(waves, 48000, return_noise=True)
    enh.enhance_files(in_paths, out_paths)             mono 16-bit PCM in, mono 16-bit PCM at config.sr out
    enh = MagnitudeEnhancer(rnet, mode='drs', ...)     the same for the real twin (R_NETWORK: DRS-Net 'drs', DR-Net 'dr')

The network's forward runs at any number of frames, but a pass at a recording's own length is a few hundred launches bound
by latency and no captured graph survives a shape change.  So every recording is cut into segments of `segment_frames` frames
that overlap by `overlap_frames` (csrc/enhance.hip states the geometry): one static [batch_segments, 256, segment_frames]
input serves recordings of any length and fills its rows with segments of different files.  The reference's data path never
shows the network more than 256 frames either (data.py crops train, validation and test items alike).

Per call: the input is uploaded in chunks and resampled once (ops.resample_sinc); the planner — host integer arithmetic only
— emits the (item, first_frame) table, which reaches the device as ONE pinned copy; per batch of segments (1) the segment STFT
kernel writes the static input, (2) net(Y, bound=False) runs in eval() under no_grad, (3) the fused mask + polar + synthesis
path makes both estimates; then ONE stitch launch cross-fades all segment waveforms into the recordings.  With use_graph the
steps 1-3 are captured once and replayed per batch; the replays read the batch's rows of the table from the same device tensor.

Lifetime of what a captured graph reads.  A graph holds addresses, not references, and the package's cache of derived
tensors (_derived: packed weights, inference constants, windows) may evict any entry.  The one rule: whoever captures keeps
what its graph reads.  The Enhancer owns its window, inverse envelope, store, table and output buffers; its last warm-up
pass runs inside _derived.collect(), which hands it a reference to every cached value that pass was served; and it captures
again whenever the network's state or one of those buffers changes.
"""
import numpy as np
import torch

from . import _derived
from . import functional as F
from . import ops
from ._lib import DcsHipError
from .audio_store import _as_float32, _signal_shape


def read_pcm16(paths, rate0=None):
    """Mono 16-bit PCM WAV files of one sample rate (scipy.io.wavfile) -> (list of int16 arrays, the rate).  rate0: the rate
    of files read before these."""
    from scipy.io import wavfile
    waves = []
    for p in paths:
        rate, data = wavfile.read(p)
        if data.dtype != np.int16:
            raise ValueError(f'{p}: {data.dtype} samples; only 16-bit PCM WAV is decoded')
        if data.ndim != 1:
            raise ValueError(f'{p}: {data.shape[1]} channels; only mono WAV is read')
        if rate0 is not None and rate != rate0:
            raise ValueError(f'{p}: {rate} Hz, the files before it {rate0} Hz; one sample rate per call')
        rate0 = rate
        waves.append(data)
    return waves, rate0


class SegmentPlan:
    """Host-side geometry of one call (integers only).  lengths[i]: samples of recording i at config.sr; n_seg[i] its
    segments; frames[i] = Tp_i, the frames of the zero-extended recording; item / first_frame: the segment table, padded with
    (-1, 0) rows to a whole number of batches; seg_first[i]: recording i's first row (int32 [n + 1])."""

    def __init__(self, lengths, T, O, hop, batch):
        lengths = np.asarray(lengths, dtype=np.int64)
        if lengths.ndim != 1 or lengths.size == 0 or (lengths <= 0).any():
            raise ValueError('SegmentPlan: needs the positive lengths of at least one recording')
        self.lengths, self.T, self.O, self.hop, self.batch = lengths, int(T), int(O), int(hop), int(batch)
        Ls, stride = self.hop * (self.T - 1), self.hop * (self.T - self.O)
        extra = np.where(lengths <= Ls, 0, -(-(lengths - Ls) // stride))
        self.n_seg = extra + 1
        self.frames = self.T + extra * (self.T - self.O)
        self.seg_first = np.zeros(lengths.size + 1, dtype=np.int64)
        np.cumsum(self.n_seg, out=self.seg_first[1:])
        self.rows = int(self.seg_first[-1])
        self.batches = -(-self.rows // self.batch)
        if self.batches * self.batch >= 2 ** 31:
            raise ValueError(f'SegmentPlan: {self.rows} segments')
        self.item = np.full(self.batches * self.batch, -1, dtype=np.int32)
        self.first_frame = np.zeros(self.batches * self.batch, dtype=np.int32)
        self.item[:self.rows] = np.repeat(np.arange(lengths.size, dtype=np.int32), self.n_seg)
        self.first_frame[:self.rows] = (np.arange(self.rows) - np.repeat(self.seg_first[:-1], self.n_seg)) * (self.T - self.O)
        self.offsets = np.zeros(lengths.size + 1, dtype=np.int64)
        np.cumsum(lengths, out=self.offsets[1:])


class Enhancer:
    """net: a C_NETWORK on a CUDA (HIP) device.  mode: 'dcs' (the noise estimate is subtracted: speech = Y - Y (.) M) or 'dc'
    (the mask is applied: speech = Y (.) M, through the unfused ops) — an argument, not sys.argv.  segment_frames: a multiple
    of 8 (the network's time strides); 2 <= overlap_frames <= segment_frames / 2.  The network's activation dtype is followed
    as is (set_activation_dtype); its training flag is restored when a call returns."""

    MODES = ('dcs', 'dc')                 # (subtractive: speech and noise estimates, mask applied: speech only)

    @staticmethod
    def _check_network(net):
        if getattr(net, '_step_dtype', None) != 'complex' or not getattr(net, 'supports_unbounded_forward', False):
            raise DcsHipError('Enhancer: the complex network (C_NETWORK) only — the real twin (R_NETWORK) goes through '
                              'MagnitudeEnhancer')

    def __init__(self, net, mode='dcs', segment_frames=2000, overlap_frames=300, batch_segments=16, use_graph=True,
                 chunk_samples=1 << 24):
        if mode not in self.MODES:
            raise ValueError(f"{type(self).__name__}: mode {mode!r}: {self.MODES[0]!r} (subtractive) or {self.MODES[1]!r} "
                             f"(mask applied)")
        self._check_network(net)
        cfg = net.config
        if int(cfg.fft_size) != 512 or int(cfg.window_length) != 512:
            raise DcsHipError(f'Enhancer: n_fft = 512 only, got {cfg.fft_size}')
        T, O, S = int(segment_frames), int(overlap_frames), int(batch_segments)
        hop = int(cfg.hop_length)
        if T <= 0 or T % 8:
            raise ValueError(f'Enhancer: segment_frames={T} must be a positive multiple of 8 (the network halves time three times)')
        if hop * (T - 1) <= 256:
            raise ValueError(f'Enhancer: segment_frames={T} at hop {hop}: the synthesis needs hop (T - 1) > 256 samples')
        if not 2 <= O <= T // 2:
            raise ValueError(f'Enhancer: overlap_frames={O} outside [2, segment_frames / 2 = {T // 2}]')
        if not 1 <= S <= 65535:
            raise ValueError(f'Enhancer: batch_segments={S} outside [1, 65535]')
        dev = next(net.parameters()).device
        if dev.type != 'cuda':
            raise DcsHipError('Enhancer: the network must be on a CUDA (HIP) device; the HIP path has no CPU fallback')
        self.net, self.mode, self.config, self.device = net, mode, cfg, dev
        self.T, self.O, self.S, self.hop, self.use_graph = T, O, S, hop, bool(use_graph)
        self.Ls = hop * (T - 1)
        self.sr = int(cfg.sr)
        self.chunk_samples = int(chunk_samples)
        self.eps = float(net.hparams['atan2_eps'])
        self.scale = 512 ** -0.5 if cfg.normalise_stft else 1.0                    # analysis (stft_bins) ...
        self.synth_scale = 512 ** 0.5 if cfg.normalise_stft else 1.0               # ... and synthesis (network_functions._polar_wave)
        # the Enhancer's own window and inverse envelope: a captured graph reads them at these addresses for its whole life
        self.window = cfg.window.detach().to(device=dev, dtype=torch.float32).clone()
        self.inv_env = ops.istft_envelope(self.window, T, hop)
        self._Y = torch.zeros((S, 256, T), dtype=torch.complex64, device=dev)        # static input of the per-batch step
        self._sel = torch.full((2 * S,), -1, dtype=torch.int32, device=dev)         # the current batch's [items | first frames]
        self._sel[S:] = 0
        self._store = self._offsets = None                   # config.sr audio of the current call, capacity kept across calls
        self._graph = self._graph_key = self._graph_out = self._keep = None

    # ---- input ---------------------------------------------------------------------------------------------------------

    def _load(self, waves, sample_rate):
        """Validate, upload in chunks of whole recordings, resample on the device into the resident store.  -> SegmentPlan."""
        waves = list(waves)
        if not waves:
            raise ValueError('Enhancer: no recordings')
        sample_rate = int(sample_rate)
        if sample_rate <= 0:
            raise ValueError(f'Enhancer: sample_rate={sample_rate}')
        len_in = np.array([_signal_shape(a, f'waves[{i}]') for i, a in enumerate(waves)], dtype=np.int64)
        lengths = np.array([ops.resample_sinc_length(L, sample_rate, self.sr) for L in len_in], dtype=np.int64)
        plan = SegmentPlan(lengths, self.T, self.O, self.hop, self.S)
        n, total = len(waves), int(plan.offsets[-1])
        if self._store is None or self._store.numel() < total or self._offsets.numel() < n + 1:
            # grown with headroom, so a run of similar calls keeps its addresses (and its captured graph)
            cap_s = max(total, 2 * (0 if self._store is None else self._store.numel()))
            cap_n = max(n, 2 * (0 if self._offsets is None else self._offsets.numel() - 1))
            self._store = torch.zeros(cap_s, dtype=torch.float32, device=self.device)
            self._offsets = torch.zeros(cap_n + 1, dtype=torch.int64, device=self.device)
        self._resample_into(waves, len_in, sample_rate, plan, self._store)
        return plan

    def _resample_into(self, waves, len_in, sample_rate, plan, store, what='waves'):
        """Upload in chunks of whole recordings and resample each chunk in one launch into store[:plan.offsets[-1]] (also
        the RecordingScorer's path for the clean recordings: both sides of a score go through the same resampler)."""
        a, n = 0, len(waves)
        while a < n:
            b, acc = a, 0
            while b < n and (b == a or acc + len_in[b] <= self.chunk_samples):
                acc += int(len_in[b])
                b += 1
            off_in = np.zeros(b - a + 1, dtype=np.int64)
            np.cumsum(len_in[a:b], out=off_in[1:])
            parts = [_as_float32(waves[i], f'{what}[{i}]') for i in range(a, b)]
            for i, p in zip(range(a, b), parts):
                if not np.isfinite(p).all():
                    raise ValueError(f'{what}[{i}]: found inf, neginf or nan in the audio')
            x = torch.from_numpy(np.concatenate(parts)).to(self.device)
            ops.resample_sinc(x, sample_rate, self.sr, offsets=off_in, out=store[int(plan.offsets[a]):int(plan.offsets[b])])
            a = b

    def _upload_tables(self, plan):
        """ONE pinned host-to-device copy of everything the kernels index with: [offsets (int64, the unused tail = total) |
        per batch (items, first frames) | seg_first] -> (sel int32 [batches, 2 S], seg_first int32 [n + 1], offsets int64 [n + 1])."""
        n, cap = plan.lengths.size, self._offsets.numel()
        off = np.full(cap, plan.offsets[-1], dtype=np.int64)                         # recordings past n: empty
        off[:n + 1] = plan.offsets
        sel = np.concatenate([plan.item.reshape(plan.batches, 1, self.S), plan.first_frame.reshape(plan.batches, 1, self.S)],
                             axis=1).reshape(-1)
        host = torch.from_numpy(np.concatenate([off.view(np.int32), sel, plan.seg_first.astype(np.int32)])).pin_memory()
        tab = torch.empty(host.numel(), dtype=torch.int32, device=self.device)
        tab.copy_(host, non_blocking=True)
        self._offsets.copy_(tab[:2 * cap].view(torch.int64))                          # into the address the graph reads
        a = 2 * cap
        return tab[a:a + sel.size].view(plan.batches, 2 * self.S), tab[a + sel.size:], tab[:2 * (n + 1)].view(torch.int64)

    # ---- the per-batch step --------------------------------------------------------------------------------------------

    def _batch_step(self, Y):
        """Y complex64 [S, 256, T] -> waveforms [2 S, hop (T - 1)] ('dcs': rows [0, S) the noise, [S, 2 S) the speech
        estimates) or [S, hop (T - 1)] ('dc': speech)."""
        net, S = self.net, Y.shape[0]
        if self.mode == 'dcs':
            d_raw = net(Y, bound=False).reshape(Y.shape)                              # (forward squeezes a batch of one)
            net.__dict__.pop('_pending_dropout', None)                               # eval: (0, 0)
            return F.bound2_apply_polar_wave_pair(Y, d_raw, self.window, self.inv_env, 512, self.hop, self.synth_scale,
                                                  self.eps, (0.0, 0), want_mask=False)[1]
        mask = net(Y).reshape(Y.shape)
        _, applied, _ = F.bound_mask_apply_complex(Y, mask, self.eps)
        return F.polar_wave(applied, self.window, self.inv_env, 512, self.hop, self.synth_scale, self.eps)

    def _run_batch(self):
        """Steps 1-3 on the static buffers: what a graph captures and what the eager form runs."""
        S = self.S
        ops.audio_stft_segments(self._store, self._offsets, self._sel[:S], self._sel[S:], self.window, self.T, self.O, self.hop,
                                self.scale, out=self._Y)
        return self._batch_step(self._Y)

    def _state_key(self):
        net = self.net
        tensors = list(net.parameters()) + list(net.buffers())
        return (F.state_generation(), ops.conv_precision(), getattr(net, 'activation_dtype', None), self._batch_step, self._store.data_ptr(),
                self._offsets.data_ptr(), tuple((id(t), t._version, t.data_ptr()) for t in tensors))

    def _step_fn(self):
        """The per-batch callable -> static or fresh waveforms.  Captured once per state (two eager warm-ups first: the first
        fills the cache of packed weights and inference constants, the second is served from it exactly what the graph will read)."""
        if not self.use_graph:
            return self._run_batch
        key = self._state_key()
        if self._graph is None or key != self._graph_key:
            self._graph = self._graph_out = None
            self._run_batch()
            with _derived.collect() as kept:
                self._run_batch()
            torch.cuda.synchronize(self.device)
            self._keep = kept
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = self._run_batch()
            self._graph, self._graph_out, self._graph_key = g, out, self._state_key()

        def replay():
            self._graph.replay()
            return self._graph_out
        return replay

    # ---- public --------------------------------------------------------------------------------------------------------

    def enhance_segments(self, waves, sample_rate):
        """The segment level of __call__: -> (plan, tables, noise_segments or None, speech_segments), the waveforms float32
        [plan.batches * batch_segments, hop (T - 1)] in the table's row order (padding rows: silence in, whatever the network
        makes of silence out; never stitched)."""
        net = self.net
        was_training = net.training
        plan = self._load(waves, sample_rate)
        sel, seg_first, offsets = self._upload_tables(plan)
        rows = plan.batches * self.S
        speech = torch.empty((rows, self.Ls), dtype=torch.float32, device=self.device)
        noise = torch.empty_like(speech) if self.mode == self.MODES[0] else None
        try:
            net.eval()
            with torch.no_grad():
                step = self._step_fn()
                for b in range(plan.batches):
                    self._sel.copy_(sel[b])
                    w = step()
                    if noise is None:
                        speech[b * self.S:(b + 1) * self.S].copy_(w)
                    else:
                        noise[b * self.S:(b + 1) * self.S].copy_(w[:self.S])
                        speech[b * self.S:(b + 1) * self.S].copy_(w[self.S:])
        finally:
            net.train(was_training)
        return plan, (sel, seg_first, offsets), noise, speech

    def stitch(self, plan, tables, segments, pcm=False):
        """One launch: segment waveforms -> the concatenated recordings float32 [sum of lengths] (with pcm: and int16)."""
        _, seg_first, offsets = tables
        return ops.segments_stitch(segments, seg_first, offsets, int(plan.offsets[-1]), self.T, self.O, self.hop, pcm=pcm)

    def _split(self, plan, flat):
        return [flat[int(a):int(b)] for a, b in zip(plan.offsets[:-1], plan.offsets[1:])]

    def __call__(self, waves, sample_rate, return_noise=False):
        if return_noise and self.mode != self.MODES[0]:
            raise ValueError(f"{type(self).__name__}: mode {self.mode!r} applies the mask and has no noise estimate")
        plan, tables, noise, speech = self.enhance_segments(waves, sample_rate)
        out = self._split(plan, self.stitch(plan, tables, speech))
        if return_noise:
            return out, self._split(plan, self.stitch(plan, tables, noise))
        return out

    def enhance_files(self, in_paths, out_paths):
        """Mono 16-bit PCM WAV files of one sample rate in (scipy.io.wavfile) -> mono 16-bit PCM at config.sr out."""
        from scipy.io import wavfile
        in_paths, out_paths = list(in_paths), list(out_paths)
        if len(in_paths) != len(out_paths) or not in_paths:
            raise ValueError(f'enhance_files: {len(in_paths)} inputs for {len(out_paths)} outputs')
        waves, rate0 = read_pcm16(in_paths)
        plan, tables, _, speech = self.enhance_segments(waves, rate0)
        pcm = self.stitch(plan, tables, speech, pcm=True)[1].cpu().numpy()
        for p, a, b in zip(out_paths, plan.offsets[:-1], plan.offsets[1:]):
            wavfile.write(p, self.sr, pcm[int(a):int(b)])
        return out_paths


class MagnitudeEnhancer(Enhancer):
    """The Enhancer of the real twin.  net: an R_NETWORK on a CUDA (HIP) device.  mode: 'drs' (DRS-Net: the noise magnitude
    |Y| M is subtracted from |Y|) or 'dr' (DR-Net: the mask is applied, no noise estimate); both estimates keep the noisy
    phase (network_functions.py:224-232, :261-267).  Per batch of segments: ops.complex_abs(Y), the network's raw last-stage
    output (forward(sigmoid=False)), then sigmoid, mask, subtraction and synthesis as one fused pass
    (F.rmask_apply_polar_wave).  Planner, segment STFT, stitch, graph lifetime and keying are the Enhancer's."""

    MODES = ('drs', 'dr')

    def __init__(self, net, mode='drs', *args, **kw):
        super().__init__(net, mode, *args, **kw)

    @staticmethod
    def _check_network(net):
        if getattr(net, '_step_dtype', None) != 'real' or not getattr(net, 'supports_raw_forward', False):
            raise DcsHipError('MagnitudeEnhancer: the real network (R_NETWORK) only — the complex network (C_NETWORK) goes '
                              'through Enhancer')

    def _batch_step(self, Y):
        """Y complex64 [S, 256, T] -> waveforms [2 S, hop (T - 1)] ('drs': rows [0, S) the noise, [S, 2 S) the speech
        estimates) or [S, hop (T - 1)] ('dr': speech)."""
        d_raw = self.net(ops.complex_abs(Y), sigmoid=False).reshape(Y.shape)       # (forward squeezes a batch of one)
        return F.rmask_apply_polar_wave(Y, d_raw, self.window, self.inv_env, 512, self.hop, self.synth_scale, self.eps,
                                        pair=self.mode == 'drs', want_mask=False)[1]
