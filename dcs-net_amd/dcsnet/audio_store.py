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
        if int(config.fft_size) != 512 or int(config.window_length) != 512:
            raise DcsHipError(f'DeviceAudioStore: n_fft = 512 only, got {config.fft_size}')
        self.config, self.ids = config, ids
        self.hop = int(config.hop_length)
        self.crop_length = int(config.integer_win_size) - self.hop           # data.py:91
        if self.crop_length <= 256 or self.crop_length % self.hop:
            raise DcsHipError(f'DeviceAudioStore: crop of {self.crop_length} samples at hop {self.hop}')
        self.T = self.crop_length // self.hop + 1
        self.scale = 512 ** -0.5 if config.normalise_stft else 1.0
        self.file_sr, self.sr = int(config.file_sr), int(config.sr)
        len_in = np.zeros(len(clean), dtype=np.int64)
        for i, (c, n) in enumerate(zip(clean, noisy)):
            lc, ln = _signal_shape(c, f'clean[{i}]'), _signal_shape(n, f'noisy[{i}]')
            if lc != ln:
                raise ValueError(f'item {i}: clean_data and noisy_data are not the same length ({lc} vs {ln})')
            len_in[i] = lc
        device = torch.device(device)
        if device.type != 'cuda':
            raise DcsHipError('DeviceAudioStore: needs a CUDA (HIP) device; the HIP path has no CPU fallback')
        self.device = device
        self.lengths = np.array([ops.resample_sinc_length(L, self.file_sr, self.sr) for L in len_in], dtype=np.int64)
        off = np.zeros(len(clean) + 1, dtype=np.int64)
        np.cumsum(self.lengths, out=off[1:])
        self.clean = torch.empty(int(off[-1]), dtype=torch.float32, device=device)
        self.noisy = torch.empty(int(off[-1]), dtype=torch.float32, device=device)
        a = 0
        while a < len(clean):                                # chunks of whole items, ~chunk_samples input samples each
            b, acc = a, 0
            while b < len(clean) and (b == a or acc + len_in[b] <= chunk_samples):
                acc += int(len_in[b])
                b += 1
            off_in = np.zeros(b - a + 1, dtype=np.int64)
            np.cumsum(len_in[a:b], out=off_in[1:])
            for src, dst, name in ((clean, self.clean, 'clean'), (noisy, self.noisy, 'noisy')):
                x = np.concatenate([_as_float32(src[i], f'{name}[{i}]') for i in range(a, b)])
                if not np.isfinite(x).all():
                    bad = next(i for i in range(a, b) if not np.isfinite(_as_float32(src[i], name)).all())
                    raise ValueError(f'{name}[{bad}]: found inf, neginf or nan in the audio')
                ops.resample_sinc(torch.from_numpy(x).to(device), self.file_sr, self.sr, offsets=off_in,
                                  out=dst[int(off[a]):int(off[b])])
            a = b
        self.offsets = torch.from_numpy(off).to(device)
        self._sel = torch.zeros(2 * 64, dtype=torch.int32, device=device)     # persistent [indices | starts]

    @classmethod
    def from_wav(cls, clean_paths, noisy_paths, config, device, ids=None, **kw):
        """Reads mono 16-bit PCM WAV files at config.file_sr through scipy.io.wavfile; any other format, channel count or rate
        raises."""
        from scipy.io import wavfile

        def read(path):
            rate, data = wavfile.read(path)
            if data.dtype != np.int16:
                raise ValueError(f'{path}: {data.dtype} samples; only 16-bit PCM WAV is decoded')
            if data.ndim != 1:
                raise ValueError(f'{path}: {data.shape[1]} channels; only mono WAV is read')
            if rate != int(config.file_sr):
                raise ValueError(f'{path}: {rate} Hz, expected config.file_sr = {config.file_sr}')
            return data
        return cls([read(p) for p in clean_paths], [read(p) for p in noisy_paths], config, device, ids=ids, **kw)

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
