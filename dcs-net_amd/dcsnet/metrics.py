"""Evaluation metrics of the reference's validation / test steps (network_functions.py:152-166, test.py:18-27).

The reference scores every utterance on the CPU with two third-party packages, `pystoi.stoi` (pystoi==0.3.3,
requirements.txt:166) and `pypesq.pesq` (pypesq==1.2.4, requirements.txt:162).  Neither is in this image and neither
can be installed.

STOI.  `stoi()` below restates the PUBLISHED algorithm — C. H. Taal, R. C. Hendriks, R. Heusdens, J. Jensen, "An
Algorithm for Intelligibility Prediction of Time-Frequency Weighted Noisy Speech", IEEE TASLP 19(7), 2011 — with the
constants and processing order of pystoi 0.3.3 (10 kHz internal rate through its Octave-style polyphase resampler,
256-sample Hann frames at 50 % overlap, removal of frames more than 40 dB below the loudest clean frame, 512-point FFT,
15 one-third-octave bands from 150 Hz, 30-frame segments, clipping at -15 dB SDR, mean correlation).  It is host-side
numpy, as in the reference (which calls `.cpu().numpy()` per utterance), and is used when `pystoi` itself cannot be
imported.  PARITY UNPINNED: there is no pystoi here to compare with and the reference holds no STOI vectors; the
tests check the algorithm's defining properties only (tests/test_host_cpu.py).

ESTOI.  `stoi(..., extended=True)` is the extended STOI of Jensen & Taal (2016), pystoi's `extended=True`: the same front
end, then every 15 x 30 segment normalised by rows and by columns instead of clipped and correlated per band.  It leaves out
pystoi's EPS-sized random dither (see stoi()); parity is unpinned for the same reason (tests/test_estoi_cpu.py: properties and
an independent route).  On the device it is `extended=True` / `'both'` of `stoi_batch` and `stoi_ragged` (one more score stage,
csrc/stoi_common.h::score_frames_ext; tests/test_estoi_device.py).

STOI on the device.  `stoi_batch()` restates `stoi()` below for a whole batch of device tensors [B, L] (csrc/stoi.hip,
through ops.resample_poly and ops.stoi): the same resampler (its closed polyphase form with the same normalised window), the
same framing, silent-frame test, window, band edges, clipping and segment statistics, with the frame energies and the keep
test in fp64.  `stoi()` is its numerics contract (tests/test_stoi_device.py); parity with pystoi itself stays unpinned.
`network_functions.calc_metric` uses it when `config.stoi_on_device` is set (default off: the host loop).

Whole recordings.  `stoi_ragged()` / `sisnr_ragged()` score recordings of DIFFERENT lengths that lie in one flat device buffer
with an int64 offset table (what dcsnet/enhance.py returns; csrc/stoi_ragged.hip): per recording bit-equal to `stoi_batch` of
that recording alone, resp. the reference's SiSNR (network_functions.py:30-42) in fp64 without its batch mean.
dcsnet/evaluate.py builds the scorer of enhanced recordings on them.

PESQ.  ITU-T P.862 is ~2 k lines of reference C with psychoacoustic tables; it is not restated.  `pesq` stays the
imported package when present, else None (calc_metric then reports NaN, as in round 1)."""
import numpy as np

FS = 10000            # internal sample rate
N_FRAME = 256         # window length
NFFT = 512
NUMBAND = 15          # one-third-octave bands
MINFREQ = 150         # centre frequency of the first band
N_SEG = 30            # frames per intermediate-intelligibility segment (384 ms)
BETA = -15.0          # lower SDR bound
DYN_RANGE = 40        # speech dynamic range kept by the silent-frame removal
EPS = np.finfo('float').eps


def _resample_window_oct(p, q):
    """Octave / Matlab `resample` anti-aliasing window (Kaiser-windowed sinc), as pystoi.utils._resample_window_oct."""
    g = np.gcd(p, q)
    p, q = p // g, q // g
    log10_rejection = -3.0
    stopband_cutoff_f = 1.0 / (2 * max(p, q))
    roll_off_width = stopband_cutoff_f / 10
    rejection_db = -20 * log10_rejection
    L = np.ceil((rejection_db - 8) / (28.714 * roll_off_width))
    t = np.arange(-L, L + 1)
    ideal = 2 * p * stopband_cutoff_f * np.sinc(2 * stopband_cutoff_f * t)
    if 21 <= rejection_db <= 50:
        beta = 0.5842 * (rejection_db - 21) ** 0.4 + 0.07886 * (rejection_db - 21)
    elif rejection_db > 50:
        beta = 0.1102 * (rejection_db - 8.7)
    else:
        beta = 0.0
    return np.kaiser(int(2 * L + 1), beta) * ideal


def resample_oct(x, p, q):
    from scipy.signal import resample_poly
    h = _resample_window_oct(p, q)
    return resample_poly(x, p, q, window=h / np.sum(h))


def thirdoct(fs, nfft, num_bands, min_freq):
    """One-third-octave band matrix [num_bands, nfft/2 + 1] and the centre frequencies."""
    f = np.linspace(0, fs, nfft + 1)[:nfft // 2 + 1]
    k = np.arange(num_bands, dtype=float)
    cf = np.power(2.0 ** (1.0 / 3), k) * min_freq
    lo = min_freq * np.power(2.0, (2 * k - 1) / 6)
    hi = min_freq * np.power(2.0, (2 * k + 1) / 6)
    obm = np.zeros((num_bands, len(f)))
    for i in range(num_bands):
        a = int(np.argmin(np.square(f - lo[i])))
        b = int(np.argmin(np.square(f - hi[i])))
        obm[i, a:b] = 1
    return obm, cf


def _hann(n):
    return np.hanning(n + 2)[1:-1]


def _frames(x, framelen, hop):
    idx = range(0, len(x) - framelen, hop)
    return np.array([x[i:i + framelen] for i in idx]) if len(x) > framelen else np.zeros((0, framelen))


def remove_silent_frames(x, y, dyn_range, framelen, hop):
    """Drop the frames whose CLEAN energy is more than dyn_range dB below the loudest one; overlap-add the rest."""
    w = _hann(framelen)
    xf, yf = _frames(x, framelen, hop) * w, _frames(y, framelen, hop) * w
    if len(xf) == 0:
        return x[:0], y[:0]
    e = 20 * np.log10(np.linalg.norm(xf, axis=1) + EPS)
    keep = (np.max(e) - dyn_range - e) < 0
    xf, yf = xf[keep], yf[keep]
    n = (len(xf) - 1) * hop + framelen if len(xf) else 0
    xs, ys = np.zeros(n), np.zeros(n)
    for i in range(len(xf)):
        xs[i * hop:i * hop + framelen] += xf[i]
        ys[i * hop:i * hop + framelen] += yf[i]
    return xs, ys


def _stft(x, win, nfft, overlap):
    hop = win // overlap
    return np.array([np.fft.rfft(_hann(win) * x[i:i + win], n=nfft) for i in range(0, len(x) - win, hop)])


def _band_segments(x, y, fs_sig):
    """What both scores share: resampling to 10 kHz, silent-frame removal, STFT and one-third-octave band envelopes of the clean
    signal x and the processed signal y -> the two stacks [segments, NUMBAND, N_SEG] of all 30-frame segments, or None when
    fewer than N_SEG STFT frames remain."""
    x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
    if x.shape != y.shape or x.ndim != 1:
        raise ValueError(f'stoi: x {x.shape} and y {y.shape} must be 1-D signals of equal length')
    if fs_sig != FS:
        x, y = resample_oct(x, FS, fs_sig), resample_oct(y, FS, fs_sig)
    x, y = remove_silent_frames(x, y, DYN_RANGE, N_FRAME, N_FRAME // 2)
    xs, ys = _stft(x, N_FRAME, NFFT, 2), _stft(y, N_FRAME, NFFT, 2)
    if xs.ndim != 2 or xs.shape[0] < N_SEG:
        return None                                        # pystoi: "Not enough STFT frames to compute intermediate intelligibility"
    obm, _ = thirdoct(FS, NFFT, NUMBAND, MINFREQ)
    xt = np.sqrt(obm @ (np.abs(xs.T) ** 2))                # [bands, frames]
    yt = np.sqrt(obm @ (np.abs(ys.T) ** 2))
    M = xt.shape[1]
    xseg = np.stack([xt[:, m - N_SEG:m] for m in range(N_SEG, M + 1)])      # [segments, bands, N_SEG]
    yseg = np.stack([yt[:, m - N_SEG:m] for m in range(N_SEG, M + 1)])
    return xseg, yseg


def _row_col_normalise(seg):
    """[segments, bands, frames]: every row (a band over its 30 frames), then every column of the result (a frame over the 15
    bands), to zero mean and unit norm, dividing by (norm + EPS): a constant row or column becomes zeros, not NaN."""
    seg = seg - seg.mean(axis=2, keepdims=True)
    seg = seg / (np.linalg.norm(seg, axis=2, keepdims=True) + EPS)
    seg = seg - seg.mean(axis=1, keepdims=True)
    return seg / (np.linalg.norm(seg, axis=1, keepdims=True) + EPS)


def stoi(x, y, fs_sig, extended=False):
    """Short-Time Objective Intelligibility of the processed signal y against the clean signal x (1-D, equal length).
    Same call as pystoi.stoi.

    extended=True: the extended STOI (ESTOI; J. Jensen, C. H. Taal, "An Algorithm for Predicting the Intelligibility of Speech
    Masked by Modulated Noise Maskers", IEEE/ACM TASLP 24(11), 2016) in pystoi 0.3.3's processing order: the same resampling,
    silent-frame removal, STFT, bands and segments, then every segment normalised by rows and by columns and
    d = sum(x_n * y_n / 30) / segments; no clipping stage.  ONE deliberate difference from pystoi: it adds EPS * standard_normal
    noise before each of the two normalisations to dodge 0 / 0 on constant rows; that is left out here, because a metric must
    be deterministic and the noise moves a score by about 1e-15.  A constant row then normalises to zeros (the norms are
    divided as norm + EPS), without a NaN.  PARITY UNPINNED, for the same reason as for STOI: there is no pystoi here to compare
    with; tests/test_estoi_cpu.py checks the defining properties and an independent route through np.corrcoef."""
    segs = _band_segments(x, y, fs_sig)
    if segs is None:
        return 1e-5
    xseg, yseg = segs
    if extended:
        xn, yn = _row_col_normalise(xseg), _row_col_normalise(yseg)
        return float(np.sum(xn * yn / N_SEG) / xseg.shape[0])
    norm = np.linalg.norm(xseg, axis=2, keepdims=True) / (np.linalg.norm(yseg, axis=2, keepdims=True) + EPS)
    yn = yseg * norm
    clip = 10 ** (-BETA / 20)
    yp = np.minimum(yn, xseg * (1 + clip))
    yp = yp - yp.mean(axis=2, keepdims=True)
    xz = xseg - xseg.mean(axis=2, keepdims=True)
    yp = yp / (np.linalg.norm(yp, axis=2, keepdims=True) + EPS)
    xz = xz / (np.linalg.norm(xz, axis=2, keepdims=True) + EPS)
    return float(np.sum(yp * xz) / (xseg.shape[0] * xseg.shape[1]))


# ---- the device path -------------------------------------------------------------------------------------------------

_device_tables = {}


def stoi_band_edges(device):
    """thirdoct(10000, 512, 15, 150)'s rows as bin ranges [lo, hi): int32 [2, 15] on `device` (cached)."""
    key = ('bands', str(device))
    t = _device_tables.get(key)
    if t is None:
        import torch
        obm, _ = thirdoct(FS, NFFT, NUMBAND, MINFREQ)
        lo, hi = [], []
        for row in obm:
            nz = np.flatnonzero(row)
            a = int(nz[0]) if len(nz) else 0
            b = int(nz[-1]) + 1 if len(nz) else 0
            assert len(nz) == b - a, 'thirdoct rows are contiguous bin ranges'
            lo.append(a)
            hi.append(b)
        t = torch.tensor([lo, hi], dtype=torch.int32).to(device)
        _device_tables[key] = t
    return t


def resample_taps(fs_sig, device):
    """(h float32 [taps] on `device` = the normalised window of resample_oct(., FS, fs_sig), up, down) (cached)."""
    fs_sig = int(fs_sig)
    key = ('taps', fs_sig, str(device))
    t = _device_tables.get(key)
    if t is None:
        import torch
        g = int(np.gcd(FS, fs_sig))
        h = _resample_window_oct(FS, fs_sig)
        t = (torch.tensor(h / np.sum(h), dtype=torch.float32).to(device), FS // g, fs_sig // g)
        _device_tables[key] = t
    return t


def _extended_result(out, extended):
    """ops.stoi / ops.stoi_ragged's tuple without its kept counts: the score, or the pair (stoi, estoi) for 'both'."""
    return out[0] if extended is False or extended is True else (out[0], out[1])


def stoi_batch(clean, estimate, fs_sig, extended=False):
    """stoi(clean[i], estimate[i], fs_sig) for every row of two device tensors [B, L] of equal shape: a float32 [B] device
    tensor, computed by the HIP kernels of csrc/stoi.hip without a host read-back (capturable).  extended=True: ESTOI,
    stoi(..., extended=True), instead; extended='both': the pair (stoi, estoi) from one resampling and one pass of the keep
    and band kernels.  CPU tensors raise DcsHipError: there is no host fallback here (stoi() is the host function)."""
    from . import ops
    from ._lib import DcsHipError
    import torch
    if not (isinstance(clean, torch.Tensor) and isinstance(estimate, torch.Tensor) and clean.is_cuda and estimate.is_cuda):
        raise DcsHipError('stoi_batch: expected CUDA (HIP) tensors; the device path has no CPU fallback (use stoi())')
    if clean.shape != estimate.shape or clean.dim() != 2:
        raise ValueError(f'stoi_batch: clean {tuple(clean.shape)} and estimate {tuple(estimate.shape)} must be [B, L] of equal shape')
    clean = clean.to(torch.float32).contiguous()
    estimate = estimate.to(torch.float32).contiguous()
    bands = stoi_band_edges(clean.device)
    if int(fs_sig) != FS:
        h, up, down = resample_taps(fs_sig, clean.device)
        clean, estimate = ops.resample_poly(clean, h, up, down), ops.resample_poly(estimate, h, up, down)
    if extended is False:
        return ops.stoi(clean, estimate, bands)[0]
    return _extended_result(ops.stoi(clean, estimate, bands, extended=extended), extended)


# ---- whole recordings of different lengths ---------------------------------------------------------------------------

def _ragged_args(what, clean, estimate, offsets, longest):
    """-> (clean, estimate, offsets int64 [n + 1] on the device, longest).  offsets on the device are never read back: longest
    (a host integer >= the longest recording) then defaults to the buffer's size, which is correct and slow (it sizes a
    grid).  offsets on the host (a sequence, an array or a CPU tensor) are checked, uploaded, and give longest themselves."""
    from ._lib import DcsHipError
    import torch
    if not (isinstance(clean, torch.Tensor) and isinstance(estimate, torch.Tensor) and clean.is_cuda and estimate.is_cuda):
        raise DcsHipError(f'{what}: expected CUDA (HIP) tensors; the device path has no CPU fallback (use stoi())')
    if clean.shape != estimate.shape or clean.dim() != 1:
        raise ValueError(f'{what}: clean {tuple(clean.shape)} and estimate {tuple(estimate.shape)} must be flat buffers of '
                         f'equal size')
    clean = clean.to(torch.float32).contiguous()
    estimate = estimate.to(torch.float32).contiguous()
    if not (isinstance(offsets, torch.Tensor) and offsets.is_cuda):
        off = np.asarray(offsets.numpy() if isinstance(offsets, torch.Tensor) else offsets, dtype=np.int64).reshape(-1)
        if off.size < 2 or off[0] != 0 or off[-1] != clean.numel() or (np.diff(off) < 0).any():
            raise ValueError(f'{what}: offsets must rise from 0 to the buffers\' size {clean.numel()}')
        if longest is None:
            longest = int(np.diff(off).max())
        offsets = torch.from_numpy(off).to(clean.device)
    return clean, estimate, offsets, clean.numel() if longest is None else int(longest)


def stoi_ragged(clean, estimate, offsets, fs_sig, longest=None, extended=False):
    """stoi(clean[a:b], estimate[a:b], fs_sig) for every recording [a, b) = offsets[i:i + 2] of two flat device buffers: a
    float32 [n] device tensor, recording by recording bit-equal to stoi_batch of that recording alone as [1, L], in a
    handful of launches whatever n is (csrc/stoi_ragged.hip) and without a host read-back (capturable when offsets are on
    the device).  offsets: int64 [n + 1], on the device or on the host; longest: see _ragged_args.  extended: as for
    stoi_batch (True: ESTOI; 'both': the pair (stoi, estoi) from one resampling and one pass).  CPU signals raise DcsHipError."""
    from . import ops
    clean, estimate, offsets, longest = _ragged_args('stoi_ragged', clean, estimate, offsets, longest)
    bands = stoi_band_edges(clean.device)
    if int(fs_sig) != FS:
        h, up, down = resample_taps(fs_sig, clean.device)
        clean, off10 = ops.resample_poly_ragged(clean, offsets, h, up, down)
        estimate, _ = ops.resample_poly_ragged(estimate, offsets, h, up, down)
        offsets, longest = off10, -(-longest * up // down)
    if extended is False:
        return ops.stoi_ragged(clean, estimate, offsets, longest, bands)[0]
    return _extended_result(ops.stoi_ragged(clean, estimate, offsets, longest, bands, extended=extended), extended)


def sisnr_ragged(clean, estimate, offsets):
    """The reference's SiSNR (network_functions.py:30-42) of every recording of two flat device buffers, without the batch
    mean: float32 [n] dB on the device (one launch, fp64 sums; capturable when offsets are on the device)."""
    from . import ops
    clean, estimate, offsets, _ = _ragged_args('sisnr_ragged', clean, estimate, offsets, None)
    return ops.sisnr_ragged(clean, estimate, offsets)
