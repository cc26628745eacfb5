"""HBM-resident training audio: the reference Dataset's load_data_into_RAM mode (data.py:68-143) with the audio in device memory.

    DeviceAudioStore(clean, noisy, config, device)   utterance pairs at config.file_sr (float32, or int16 scaled by 1/32768 as
                                                      torchaudio's normalize=True does), resampled ONCE on the device to
                                                      config.sr (ops.resample_sinc: torchaudio 0.9.0's Resample, data.py:84-85)
                                                      and kept as two float32 tensors with shared int64 offsets
    store.batch(indices, generator)                   per step the host draws B crop starts (frontend.crop_batch's rule), copies
                                                      B indices and B starts into persistent device buffers and makes ONE launch
                                                      (ops.audio_stft_batch): crop, noise = noisy - clean, three STFTs, the
                                                      network's [B, 256, T] layout — optionally straight into a captured
                                                      TrainStep's input buffers
    store.epoch(batch_size, generator)                DataLoader(shuffle=True)'s batches of item indices, sharded per rank
    MixingAudioStore(clean, noise, config, device)    a clean-speech corpus and a noise corpus instead of pairs: per item a
                                                      noise recording, a noise start and an SNR are drawn on the host
                                                      (draw_mix, mix_gain) and the mixture is formed inside the batch launch
                                                      (ops.audio_mix_stft_batch); materialise() fixes one mixture per item
                                                      as a DeviceAudioStore

After construction no audio crosses PCIe.  A DataLoader cannot serve this: its workers are forked processes without device
tensors, so the store is driven from the training process itself."""
import numpy as np
import torch

from . import ops
from ._lib import DcsHipError
from .network_functions import _window_on


def _as_float32(a, what):
    """A 1-D float32 numpy view / copy of one signal: float32 as is, int16 / 32768."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.dtype == np.int16:
        return a.astype(np.float32) * np.float32(1.0 / 32768)
    if a.dtype != np.float32:
        raise TypeError(f'{what}: expected float32 or int16 samples, got {a.dtype}')
    return a


def _signal_shape(a, what):
    shape = tuple(a.shape)
    if len(shape) != 1:
        raise ValueError(f'{what}: expected a 1-D signal, got shape {shape}')
    if shape[0] == 0:
        raise ValueError(f'{what}: empty signal')
    dtype = a.dtype
    if dtype not in (np.float32, np.int16, torch.float32, torch.int16):
        raise TypeError(f'{what}: expected float32 or int16 samples, got {dtype}')
    return shape[0]


def check_indices(indices, n):
    """The batch's item indices as a list of ints; IndexError outside [0, n)."""
    idx = [int(i) for i in (indices.tolist() if isinstance(indices, torch.Tensor) else indices)]
    if not idx:
        raise ValueError('DeviceAudioStore: empty batch')
    for i in idx:
        if not 0 <= i < n:
            raise IndexError(f'DeviceAudioStore: item {i} out of range [0, {n})')
    return idx


def draw_crop_starts(lengths, indices, crop_length, generator=None):
    """frontend.crop_batch's crop starts (data.py:90-104) for the items `indices` of lengths `lengths`, in item order: 0 when
    an item is not longer than the crop, otherwise int(torch.randint(0, len - crop_length, (1,), generator=generator)) —
    no draw when len == crop_length.  The same generator state gives crop_batch's draws."""
    starts = []
    for i in check_indices(indices, len(lengths)):
        span = int(lengths[i]) - int(crop_length)
        starts.append(int(torch.randint(0, span, (1,), generator=generator)) if span > 0 else 0)
    return starts


def epoch_batches(n, batch_size, generator=None, shuffle=True, drop_last=False, rank=0, world=1):
    """DataLoader(batch_size, shuffle, drop_last)'s batches of item indices for one epoch over n items (torch.randperm order;
    a smaller last batch unless drop_last).  With world > 1 every rank passes the same generator state, so all draw the same
    permutation, and takes its contiguous share torch.tensor_split(global_batch, world)[rank] of every global batch of
    batch_size items (a share of a small last batch may be empty).  Yields lists of ints."""
    batch_size, rank, world = int(batch_size), int(rank), int(world)
    if batch_size <= 0 or world <= 0 or not 0 <= rank < world:
        raise ValueError(f'epoch: batch_size={batch_size}, rank={rank}, world={world}')
    order = torch.randperm(n, generator=generator) if shuffle else torch.arange(n)
    for a in range(0, n, batch_size):
        b = order[a:a + batch_size]
        if drop_last and b.numel() < batch_size:
            break
        yield torch.tensor_split(b, world)[rank].tolist()


def _set_geometry(store, config, who):
    """The fields a store derives from config: hop, crop_length (data.py:91), T, scale, file_sr, sr."""
    if int(config.fft_size) != 512 or int(config.window_length) != 512:
        raise DcsHipError(f'{who}: n_fft = 512 only, got {config.fft_size}')
    store.config = config
    store.hop = int(config.hop_length)
    store.crop_length = int(config.integer_win_size) - store.hop           # data.py:91
    if store.crop_length <= 256 or store.crop_length % store.hop:
        raise DcsHipError(f'{who}: crop of {store.crop_length} samples at hop {store.hop}')
    store.T = store.crop_length // store.hop + 1
    store.scale = 512 ** -0.5 if config.normalise_stft else 1.0
    store.file_sr, store.sr = int(config.file_sr), int(config.sr)


def _hip_device(device, who):
    device = torch.device(device)
    if device.type != 'cuda':
        raise DcsHipError(f'{who}: needs a CUDA (HIP) device; the HIP path has no CPU fallback')
    return device


def upload_resampled(sources, len_in, file_sr, sr, device, chunk_samples):
    """sources: ((name, signals), ...), every list with the input lengths len_in (int64 [n]).  Uploads them in chunks of whole
    items, about chunk_samples input samples per signal, and resamples each chunk on the device (ops.resample_sinc) into one
    flat float32 tensor per source.  -> (lengths int64 [n] at sr, offsets int64 [n + 1] (host), [tensor per source])."""
    n = len(len_in)
    lengths = np.array([ops.resample_sinc_length(L, file_sr, sr) for L in len_in], dtype=np.int64)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    stores = [torch.empty(int(off[-1]), dtype=torch.float32, device=device) for _ in sources]
    a = 0
    while a < n:                                             # chunks of whole items, ~chunk_samples input samples each
        b, acc = a, 0
        while b < n and (b == a or acc + len_in[b] <= chunk_samples):
            acc += int(len_in[b])
            b += 1
        off_in = np.zeros(b - a + 1, dtype=np.int64)
        np.cumsum(len_in[a:b], out=off_in[1:])
        for (name, src), dst in zip(sources, stores):
            x = np.concatenate([_as_float32(src[i], f'{name}[{i}]') for i in range(a, b)])
            if not np.isfinite(x).all():
                bad = next(i for i in range(a, b) if not np.isfinite(_as_float32(src[i], name)).all())
                raise ValueError(f'{name}[{bad}]: found inf, neginf or nan in the audio')
            ops.resample_sinc(torch.from_numpy(x).to(device), file_sr, sr, offsets=off_in, out=dst[int(off[a]):int(off[b])])
        a = b
    return lengths, off, stores


def read_wav(path, config):
    """One mono 16-bit PCM WAV file at config.file_sr through scipy.io.wavfile; any other format, channel count or rate raises."""
    from scipy.io import wavfile
    rate, data = wavfile.read(path)
    if data.dtype != np.int16:
        raise ValueError(f'{path}: {data.dtype} samples; only 16-bit PCM WAV is decoded')
    if data.ndim != 1:
        raise ValueError(f'{path}: {data.shape[1]} channels; only mono WAV is read')
    if rate != int(config.file_sr):
        raise ValueError(f'{path}: {rate} Hz, expected config.file_sr = {config.file_sr}')
    return data


class DeviceAudioStore:
    """clean / noisy: equally long lists of 1-D numpy arrays or tensors at config.file_sr (float32 or int16); each pair of
    equal length (data.py:87-88) and finite.  ids: optional names of the items (the reference's list_IDs), kept as self.ids.
    The audio is uploaded in chunks of about chunk_samples input samples per signal and resampled on the device; only the
    config.sr store (self.clean, self.noisy float32, self.offsets int64 [n + 1]) and the host copy of its lengths stay."""

    def __init__(self, clean, noisy, config, device, ids=None, chunk_samples=1 << 24):
        clean, noisy = list(clean), list(noisy)
        if len(clean) != len(noisy):
            raise ValueError(f'DeviceAudioStore: {len(clean)} clean and {len(noisy)} noisy signals')
        if not clean:
            raise ValueError('DeviceAudioStore: no utterances')
        if ids is not None:
            ids = list(ids)
            if len(ids) != len(clean):
                raise ValueError(f'DeviceAudioStore: {len(ids)} ids for {len(clean)} utterances')
        self.ids = ids
        _set_geometry(self, config, 'DeviceAudioStore')
        len_in = np.zeros(len(clean), dtype=np.int64)
        for i, (c, n) in enumerate(zip(clean, noisy)):
            lc, ln = _signal_shape(c, f'clean[{i}]'), _signal_shape(n, f'noisy[{i}]')
            if lc != ln:
                raise ValueError(f'item {i}: clean_data and noisy_data are not the same length ({lc} vs {ln})')
            len_in[i] = lc
        self.device = _hip_device(device, 'DeviceAudioStore')
        self.lengths, off, (self.clean, self.noisy) = upload_resampled(
            (('clean', clean), ('noisy', noisy)), len_in, self.file_sr, self.sr, self.device, chunk_samples)
        self.offsets = torch.from_numpy(off).to(self.device)
        self._sel = torch.zeros(2 * 64, dtype=torch.int32, device=self.device)     # persistent [indices | starts]

    @classmethod
    def from_resident(cls, clean, noisy, offsets, lengths, config, ids=None):
        """A store over tensors that are already resident at config.sr: clean / noisy float32 [N] on one HIP device, offsets
        int64 [n + 1] on it, lengths the host copy of the item lengths (int64 [n]).  Nothing is copied, so a store made from a
        MixingAudioStore shares its clean tensor."""
        lengths = np.asarray(lengths, dtype=np.int64)
        if (clean.dtype != torch.float32 or noisy.dtype != torch.float32 or clean.dim() != 1 or clean.shape != noisy.shape or
                not clean.is_contiguous() or not noisy.is_contiguous()):
            raise ValueError('DeviceAudioStore.from_resident: clean and noisy must be contiguous float32 [N] tensors of one size')
        if (offsets.dtype != torch.int64 or tuple(offsets.shape) != (len(lengths) + 1,) or len(lengths) == 0 or
                int(lengths.sum()) != clean.numel() or (lengths <= 0).any()):
            raise ValueError(f'DeviceAudioStore.from_resident: {tuple(offsets.shape)} offsets, {len(lengths)} lengths for '
                             f'{clean.numel()} samples')
        if ids is not None:
            ids = list(ids)
            if len(ids) != len(lengths):
                raise ValueError(f'DeviceAudioStore: {len(ids)} ids for {len(lengths)} utterances')
        self = cls.__new__(cls)
        self.ids = ids
        _set_geometry(self, config, 'DeviceAudioStore')
        self.device = _hip_device(clean.device, 'DeviceAudioStore')
        if noisy.device != self.device or offsets.device != self.device:
            raise ValueError(f'DeviceAudioStore.from_resident: every tensor on {self.device}')
        self.lengths, self.clean, self.noisy, self.offsets = lengths, clean, noisy, offsets
        self._sel = torch.zeros(2 * 64, dtype=torch.int32, device=self.device)
        return self

    @classmethod
    def from_wav(cls, clean_paths, noisy_paths, config, device, ids=None, **kw):
        """Reads mono 16-bit PCM WAV files at config.file_sr through scipy.io.wavfile; any other format, channel count or rate
        raises."""
        return cls([read_wav(p, config) for p in clean_paths], [read_wav(p, config) for p in noisy_paths], config, device,
                   ids=ids, **kw)

    def __len__(self):
        return len(self.lengths)

    def draw_starts(self, indices, generator=None):
        """Crop starts for these items by crop_batch's rule on the config.sr lengths (draw_crop_starts)."""
        return draw_crop_starts(self.lengths, indices, self.crop_length, generator)

    def batch(self, indices, generator=None, starts=None, out=None):
        """(noise, noisy, clean) complex64 [B, 256, T] of the items `indices` at crop starts drawn as crop_batch draws them (or
        the given `starts`), plus the starts (int64 [B], host) — data.py:140-141 logs them with the IDs.  One host-to-device copy
        of 2 B int32 and one launch; out=step.input_buffers() writes into a captured TrainStep's static inputs."""
        idx = check_indices(indices, len(self))
        if starts is None:
            starts = self.draw_starts(idx, generator)
        else:
            starts = [int(s) for s in (starts.tolist() if isinstance(starts, torch.Tensor) else starts)]
            if len(starts) != len(idx):
                raise ValueError(f'DeviceAudioStore: {len(starts)} starts for {len(idx)} items')
            for i, s in zip(idx, starts):
                if s < 0 or (s > 0 and s + self.crop_length > int(self.lengths[i])):
                    raise IndexError(f'DeviceAudioStore: start {s} of item {i} ({int(self.lengths[i])} samples) leaves the item')
        B = len(idx)
        if self._sel.numel() < 2 * B:
            self._sel = torch.zeros(2 * B, dtype=torch.int32, device=self.device)
        host = torch.tensor(idx + starts, dtype=torch.int32).pin_memory()    # freed by the host allocator after the copy
        sel = self._sel[:2 * B]
        sel.copy_(host, non_blocking=True)
        noise, noisy, clean = self.batch_device(sel[:B], sel[B:], out=out)
        return noise, noisy, clean, torch.tensor(starts, dtype=torch.int64)

    def batch_device(self, index, starts, out=None):
        """The launch alone, from device-resident int32 [B] index and start tensors (ops.audio_stft_batch): capturable in a
        hipGraph, which then replays with whatever the caller has written into those tensors since."""
        return ops.audio_stft_batch(self.clean, self.noisy, self.offsets, index, starts, _window_on(self.config, self.device),
                                    self.T, self.hop, self.scale, out=out)

    def epoch(self, batch_size, generator=None, shuffle=True, drop_last=False, rank=0, world=1):
        """One epoch's batches of item indices (epoch_batches): DataLoader(shuffle=True)'s order, each rank's contiguous share."""
        return epoch_batches(len(self), batch_size, generator, shuffle, drop_last, rank, world)


# ---- clean speech + noise recordings, mixed on the device ----------------------------------------------------------------------

SNR_LEVELS_DB = (15, 10, 5, 0)                               # the levels VoiceBank+DEMAND's training set was mixed at


LEVELS = ('power', 'p56')                                    # how a store measures a recording's level


def mix_gain(clean_power, noise_power, snr_db):
    """The gain g that puts g * noise at snr_db below the clean signal, given the LEVEL of each as a power — the whole-recording
    mean square, or the ITU-T P.56 active power (MixingAudioStore's level= / noise_level=; the function is the same for
    both): sqrt(Pc / Pn) * 10 ** (-snr_db / 20), evaluated in float64 numpy and rounded once to float32 (a
    numpy.float32 for scalars, a float32 array otherwise).  ValueError for a power that is zero, negative or not finite, a
    non-finite SNR, or a gain that float32 does not hold."""
    pc, pn, snr = (np.asarray(v, dtype=np.float64) for v in (clean_power, noise_power, snr_db))
    for name, p in (('clean', pc), ('noise', pn)):
        if not (np.isfinite(p).all() and (p > 0).all()):
            raise ValueError(f'mix_gain: {name} power must be positive and finite, got {p.tolist()}')
    if not np.isfinite(snr).all():
        raise ValueError(f'mix_gain: SNR must be finite, got {snr.tolist()}')
    with np.errstate(over='ignore'):
        g = (np.sqrt(pc / pn) * 10.0 ** (-snr / 20.0)).astype(np.float32)
    if not (np.isfinite(g).all() and (g > 0).all()):
        raise ValueError(f'mix_gain: gain {g.tolist()} is outside float32')
    return g if g.ndim else np.float32(g)


def _snr_choice(snr_db, snr_range):
    """(levels, None) or (None, (lo, hi)), validated."""
    if snr_range is not None:
        lo, hi = (float(v) for v in snr_range)
        if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
            raise ValueError(f'snr_range: need finite lo <= hi, got {snr_range}')
        return None, (lo, hi)
    levels = [float(v) for v in snr_db]
    if not levels or not np.isfinite(levels).all():
        raise ValueError(f'snr_db: need at least one finite level, got {snr_db}')
    return levels, None


def draw_mix(indices, noise_lengths, generator=None, snr_db=SNR_LEVELS_DB, snr_range=None):
    """The mixture draws for the items `indices` of a batch -> (noise_index, noise_start, snr_db): two lists of ints and one
    of floats, in batch order.  The order of the draws is part of the contract (fit checkpoints the generator, so a resumed
    run continues with the same mixtures).  For each item in batch order, three draws:
        1. the noise recording   r   = int(torch.randint(0, n_noise, (1,), generator=generator))
        2. the noise start       s   = int(torch.randint(0, noise_lengths[r], (1,), generator=generator))
        3. the SNR               snr = snr_db[int(torch.randint(0, len(snr_db), (1,), generator=generator))]
           or, with snr_range = (lo, hi),
                                 snr = lo + (hi - lo) * float(torch.rand(1, dtype=torch.float64, generator=generator))
    Every draw is made even where it has one outcome (one noise recording, one level).  Which items are in the batch does not
    enter: `indices` gives the count.  A store draws ALL crop starts of the batch first (draw_crop_starts), then calls this."""
    count = len(indices.tolist() if isinstance(indices, torch.Tensor) else list(indices))
    noise_lengths = [int(n) for n in noise_lengths]
    if not noise_lengths or min(noise_lengths) < 1:
        raise ValueError('draw_mix: needs at least one noise recording, none of them empty')
    levels, span = _snr_choice(snr_db, snr_range)
    noise_index, noise_start, snr = [], [], []
    for _ in range(count):
        r = int(torch.randint(0, len(noise_lengths), (1,), generator=generator))
        noise_index.append(r)
        noise_start.append(int(torch.randint(0, noise_lengths[r], (1,), generator=generator)))
        if span is None:
            snr.append(levels[int(torch.randint(0, len(levels), (1,), generator=generator))])
        else:
            snr.append(span[0] + (span[1] - span[0]) * float(torch.rand(1, dtype=torch.float64, generator=generator)))
    return noise_index, noise_start, snr


class MixingAudioStore:
    """A clean-speech corpus and a noise corpus, both resident at config.sr, mixed per batch on the device:
    noisy[q] = clean[q] + g * noise_r[(s + q) mod len_r] with the recording r, the start s and the SNR drawn per item
    (draw_mix) and g = mix_gain(level of the clean recording, level of the noise recording, SNR).  level / noise_level say
    what a recording's level is, per side: 'power' (the default), its whole-recording mean square, or 'p56', its ITU-T P.56
    active power (ops.active_level_ragged at config.sr, margin 15.9 dB: the mean square over the active part of the signal,
    pauses left out — how VoiceBank+DEMAND was mixed).  The noise loops and is aligned to the clean RECORDING's sample 0, so a
    crop at start t hears noise_r[(s + t + ...) mod len_r]: what the crop of the materialised mixture holds.

    clean / noise: lists of 1-D signals at config.file_sr (float32 or int16), uploaded and resampled as DeviceAudioStore does
    (upload_resampled).  snr_db: the levels to draw from; snr_range=(lo, hi): a uniform SNR instead.  clean_power / noise_power
    (numpy float64) are the per-recording mean squares, clean_level / noise_level what the gains use (the same arrays under
    'power', the active powers under 'p56') and clean_activity / noise_activity the P.56 activity factors (NaN under 'power');
    all are measured once, on the device, and read back in one transfer.  A silent recording raises here and is named, and so
    does one without a P.56 level (an envelope that never reaches 2^-15 of full scale, or no margin crossing).  The level is
    a property of the store, like the SNR choice: a resumed run must be given the same one.

    The duck type is DeviceAudioStore's (__len__, lengths, ids, T, crop_length, device, epoch, draw_starts, batch,
    batch_device), so fit, DeviceValidator and the SWA loop take it unchanged; materialise() gives a DeviceAudioStore with one
    fixed mixture per item, for validation and test sets."""

    def __init__(self, clean, noise, config, device, snr_db=SNR_LEVELS_DB, snr_range=None, ids=None, noise_ids=None,
                 chunk_samples=1 << 24, level='power', noise_level='power'):
        for name, kind in (('level', level), ('noise_level', noise_level)):
            if kind not in LEVELS:
                raise ValueError(f'MixingAudioStore: {name}={kind!r}, expected one of {LEVELS}')
        self.level_kind, self.noise_level_kind = level, noise_level
        clean, noise = list(clean), list(noise)
        if not clean or not noise:
            raise ValueError(f'MixingAudioStore: {len(clean)} clean and {len(noise)} noise recordings')
        for name, these, n in (('ids', ids, len(clean)), ('noise_ids', noise_ids, len(noise))):
            if these is not None and len(list(these)) != n:
                raise ValueError(f'MixingAudioStore: {len(list(these))} {name} for {n} recordings')
        self.ids = None if ids is None else list(ids)
        self.noise_ids = None if noise_ids is None else list(noise_ids)
        self.snr_db, self.snr_range = _snr_choice(snr_db, snr_range)
        _set_geometry(self, config, 'MixingAudioStore')
        len_c = np.array([_signal_shape(c, f'clean[{i}]') for i, c in enumerate(clean)], dtype=np.int64)
        len_n = np.array([_signal_shape(n, f'noise[{i}]') for i, n in enumerate(noise)], dtype=np.int64)
        self.device = _hip_device(device, 'MixingAudioStore')
        self.lengths, off, (self.clean,) = upload_resampled((('clean', clean),), len_c, self.file_sr, self.sr, self.device,
                                                            chunk_samples)
        self.noise_lengths, noff, (self.noise,) = upload_resampled((('noise', noise),), len_n, self.file_sr, self.sr,
                                                                   self.device, chunk_samples)
        if int(self.noise_lengths.max()) >= 1 << 31 or int(self.lengths.max()) >= 1 << 31:
            raise ValueError('MixingAudioStore: a recording of 2^31 samples or more')
        self.offsets = torch.from_numpy(off).to(self.device)
        self.noise_offsets = torch.from_numpy(noff).to(self.device)
        sides = (('clean', self.clean, self.offsets, len(clean), level, self.ids),
                 ('noise', self.noise, self.noise_offsets, len(noise), noise_level, self.noise_ids))
        parts = [ops.signal_power_ragged(x, o) for _, x, o, _, _, _ in sides]
        parts += [ops.active_level_ragged(x, o, self.sr).reshape(-1) for _, x, o, _, kind, _ in sides if kind == 'p56']
        rest = torch.cat(parts).cpu().numpy()                                                            # the one read-back
        power, levels, activity = [], [], []
        for _, _, _, n, _, _ in sides:                           # the mean powers first ...
            power.append(rest[:n].copy())
            rest = rest[n:]
        for k, (_, _, _, n, kind, _) in enumerate(sides):        # ... then (active_power, activity) rows of the 'p56' sides
            if kind == 'p56':
                levels.append(rest[0:2 * n:2].copy())
                activity.append(rest[1:2 * n:2].copy())
                rest = rest[2 * n:]
            else:
                levels.append(power[k])
                activity.append(np.full(n, np.nan))
        self.clean_power, self.noise_power = power
        self.clean_level, self.noise_level = levels
        self.clean_activity, self.noise_activity = activity
        for k, (name, _, _, _, _, these) in enumerate(sides):
            for p, why in ((power[k], ' is silent: no gain gives it an SNR'),
                           (levels[k], ' has no ITU-T P.56 active speech level: its envelope never reaches the lowest threshold '
                                       '(2^-15 of full scale), or its levels never cross the margin')):
                bad = np.flatnonzero(~(p > 0))
                if len(bad):
                    i = int(bad[0])
                    raise ValueError(f'MixingAudioStore: {name}[{i}]' + (f' ({these[i]})' if these is not None else '') + why)
        self.last_draws = None
        self._sel = torch.zeros(5 * 64, dtype=torch.int32, device=self.device)   # persistent [index | start | noise | nstart | gain]

    @classmethod
    def from_wav(cls, clean_paths, noise_paths, config, device, **kw):
        """Reads mono 16-bit PCM WAV files at config.file_sr (read_wav); any other format, channel count or rate raises."""
        return cls([read_wav(p, config) for p in clean_paths], [read_wav(p, config) for p in noise_paths], config, device, **kw)

    def __len__(self):
        return len(self.lengths)

    def draw_starts(self, indices, generator=None):
        """Crop starts for these items by crop_batch's rule on the config.sr lengths (draw_crop_starts)."""
        return draw_crop_starts(self.lengths, indices, self.crop_length, generator)

    def draw_mix(self, indices, generator=None):
        """draw_mix with this store's noise lengths and SNR choice."""
        return draw_mix(indices, self.noise_lengths, generator, self.snr_db or SNR_LEVELS_DB, self.snr_range)

    def _checked_draws(self, idx, draws):
        """(noise_index, noise_start, snr, gain float32 [len(idx)]) of given draws for the clean items idx, validated."""
        noise_index, noise_start, snr = ([v for v in (d.tolist() if isinstance(d, (torch.Tensor, np.ndarray)) else d)] for d in draws)
        noise_index, noise_start, snr = [int(r) for r in noise_index], [int(s) for s in noise_start], [float(v) for v in snr]
        if not len(noise_index) == len(noise_start) == len(snr) == len(idx):
            raise ValueError(f'MixingAudioStore: draws of {len(noise_index)}, {len(noise_start)}, {len(snr)} for {len(idx)} items')
        for r, s in zip(noise_index, noise_start):
            if not 0 <= r < len(self.noise_lengths):
                raise IndexError(f'MixingAudioStore: noise recording {r} out of range [0, {len(self.noise_lengths)})')
            if not 0 <= s < int(self.noise_lengths[r]):
                raise IndexError(f'MixingAudioStore: noise start {s} outside recording {r} ({int(self.noise_lengths[r])} samples)')
        gain = mix_gain(self.clean_level[idx], self.noise_level[noise_index], np.array(snr, dtype=np.float64))
        return noise_index, noise_start, snr, gain

    def _upload(self, ints, gain):
        """One pinned host-to-device copy of the int32 columns and the float32 gains into the persistent buffer -> its views."""
        B = len(gain)
        if self._sel.numel() < (len(ints) + 1) * B:
            self._sel = torch.zeros((len(ints) + 1) * B, dtype=torch.int32, device=self.device)
        host = torch.empty((len(ints) + 1) * B, dtype=torch.int32).pin_memory()    # freed by the host allocator after the copy
        host[:len(ints) * B] = torch.tensor([v for column in ints for v in column], dtype=torch.int32)
        host[len(ints) * B:].view(torch.float32).copy_(torch.from_numpy(np.ascontiguousarray(gain, dtype=np.float32)))
        sel = self._sel[:(len(ints) + 1) * B]
        sel.copy_(host, non_blocking=True)
        return [sel[k * B:(k + 1) * B] for k in range(len(ints))] + [sel[len(ints) * B:].view(torch.float32)]

    def batch(self, indices, generator=None, starts=None, draws=None, out=None):
        """(noise, noisy, clean) complex64 [B, 256, T] of the items `indices`, plus the crop starts (int64 [B], host).  Draws,
        in this order: ALL crop starts (draw_crop_starts — the same generator state gives the paired store's starts), then
        draw_mix's three draws per item; then mix_gain.  starts / draws = (noise_index, noise_start, snr_db) replace the
        respective draws.  One pinned host-to-device copy of 4 B int32 + B float32 and one launch; out as for
        DeviceAudioStore.batch.  The draws and gains of the last call stay in self.last_draws."""
        idx = check_indices(indices, len(self))
        if starts is None:
            starts = self.draw_starts(idx, generator)
        else:
            starts = [int(s) for s in (starts.tolist() if isinstance(starts, torch.Tensor) else starts)]
            if len(starts) != len(idx):
                raise ValueError(f'MixingAudioStore: {len(starts)} starts for {len(idx)} items')
            for i, s in zip(idx, starts):
                if s < 0 or (s > 0 and s + self.crop_length > int(self.lengths[i])):
                    raise IndexError(f'MixingAudioStore: start {s} of item {i} ({int(self.lengths[i])} samples) leaves the item')
        noise_index, noise_start, snr, gain = self._checked_draws(idx, self.draw_mix(idx, generator) if draws is None else draws)
        self.last_draws = {'noise_index': noise_index, 'noise_start': noise_start, 'snr_db': snr, 'gain': gain}
        sel = self._upload((idx, starts, noise_index, noise_start), gain)
        noise, noisy, clean = self.batch_device(*sel, out=out)
        return noise, noisy, clean, torch.tensor(starts, dtype=torch.int64)

    def batch_device(self, index, starts, noise_index, noise_start, gain, out=None):
        """The launch alone, from device-resident int32 [B] index, start, noise index and noise start tensors and float32 [B]
        gains (ops.audio_mix_stft_batch): capturable in a hipGraph, which then replays with whatever the caller has written
        into those tensors since."""
        return ops.audio_mix_stft_batch(self.clean, self.offsets, self.noise, self.noise_offsets, index, starts, noise_index,
                                        noise_start, gain, _window_on(self.config, self.device), self.T, self.hop, self.scale,
                                        out=out)

    def materialise(self, generator=None, draws=None):
        """A DeviceAudioStore with ONE mixture per item (whole recordings, one launch: ops.audio_mix_ragged), sharing this
        store's clean tensor: a fixed validation or test set for every consumer of the paired store.  The draws are draw_mix's
        for the items 0 .. n - 1 in order, or the given draws = (noise_index, noise_start, snr_db) per item; they stay in
        self.last_draws.  Its batches at the same starts are bit for bit this store's batches with the same draws."""
        idx = list(range(len(self)))
        noise_index, noise_start, snr, gain = self._checked_draws(idx, self.draw_mix(idx, generator) if draws is None else draws)
        self.last_draws = {'noise_index': noise_index, 'noise_start': noise_start, 'snr_db': snr, 'gain': gain}
        r, s, g = self._upload((noise_index, noise_start), gain)
        noisy = ops.audio_mix_ragged(self.clean, self.offsets, self.noise, self.noise_offsets, r, s, g)
        return DeviceAudioStore.from_resident(self.clean, noisy, self.offsets, self.lengths, self.config, ids=self.ids)

    def epoch(self, batch_size, generator=None, shuffle=True, drop_last=False, rank=0, world=1):
        """One epoch's batches of item indices (epoch_batches): DataLoader(shuffle=True)'s order, each rank's contiguous share."""
        return epoch_batches(len(self), batch_size, generator, shuffle, drop_last, rank, world)
