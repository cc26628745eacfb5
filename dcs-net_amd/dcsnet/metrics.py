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

Segmental SNR, LLR, cepstrum distance.  `frame_measures()` below restates the three frame-based objective measures of
Y. Hu, P. C. Loizou, "Evaluation of Objective Quality Measures for Speech Enhancement", IEEE TASLP 16(1), 2008, that are
defined by formulae alone, after their published `comp_snr.m` / `comp_llr.m` / `comp_cep.m` (30 ms frames at 75 % overlap with
the published frame count, a Hann-shaped window, segmental SNR clamped to [-10, 35] dB and averaged over all frames; order-16
(order-10 below 10 kHz) LPC by the published Levinson-Durbin recursion, LLR clamped to [0, 2], LPC-cepstrum distance clamped
to [0, 10], each averaged over the 95 % smallest frame values), at the signals' own rate.  It is host-side numpy in fp64.
PARITY UNPINNED: neither pysepm nor the MATLAB originals are here to compare with; the tests check the defining properties and
independent routes only (tests/test_frame_measures_cpu.py).  On the device it is `frame_measures_ragged()`
(csrc/frame_measures.hip: fp64 until the final rounding; `frame_measures()` is its numerics contract,
tests/test_frame_measures_device.py).  WSS and the composite measures (CSIG / CBAK / COVL) are not restated: the composites
need PESQ, and WSS a filter-bank table that nothing here can verify.

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


# ---- segmental SNR, LLR, cepstrum distance (Hu & Loizou) -------------------------------------------------------------------

SSNR_RANGE = (-10.0, 35.0)      # dB, per frame
LLR_RANGE = (0.0, 2.0)
CD_RANGE = (0.0, 10.0)
TRIM = 0.95                     # the share of the smallest frame values that LLR and CD average


def frame_geometry(fs):
    """(N, S, P) at rate fs: the frame length round(0.03 fs) (in integers, halves up), the hop N // 4 and the LPC order."""
    fs = int(fs)
    if fs <= 0:
        raise ValueError(f'frame_geometry: fs={fs}')
    N = (3 * fs + 50) // 100
    return N, N // 4, 16 if fs >= 10000 else 10


def frame_count(L, fs):
    """The published frame count (it leaves out the last full frame): (L - N) // S for L >= N + S, else 0."""
    N, S, _ = frame_geometry(fs)
    return (L - N) // S if L >= N + S else 0


def _measure_window(N):
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * (np.arange(N) + 1.0) / (N + 1.0)))


def trimmed_count(V):
    """K = max(1, floor(0.95 V + 0.5)) for V valid frames, in integers (0.95 V + 0.5 = (19 V + 10) / 20 exactly)."""
    return max(1, (19 * int(V) + 10) // 20)


def _trimmed_mean(values):
    """The mean of the trimmed_count(V) smallest of V values; NaN for none."""
    values = np.asarray(values, dtype=np.float64)
    if values.size == 0:
        return float('nan')
    return float(np.mean(np.sort(values)[:trimmed_count(values.size)]))


def _lpc(R, P):
    """The published lpcoeff on autocorrelations R [..., P + 1] -> (A [..., P + 1] = [1, -a], E [..., P + 1] the prediction
    error energies E_0 = R[0] .. E_P).  Rows whose E reaches 0 carry inf / NaN: the caller's validity test drops them."""
    R = np.asarray(R, dtype=np.float64)
    lead = R.shape[:-1]
    E = np.empty(lead + (P + 1,))
    E[..., 0] = R[..., 0]
    a = np.zeros(lead + (P,))
    with np.errstate(all='ignore'):
        for i in range(P):
            prev = a.copy()
            k = (R[..., i + 1] - np.sum(prev[..., :i] * R[..., i:0:-1], axis=-1)) / E[..., i]
            a[..., i] = k
            if i:
                a[..., :i] = prev[..., :i] - k[..., None] * prev[..., i - 1::-1]
            E[..., i + 1] = (1.0 - k * k) * E[..., i]
    return np.concatenate([np.ones(lead + (1,)), -a], axis=-1), E


def _lpc_cepstrum(A):
    """LPC cepstrum c [..., P + 1] (c[0] = 0, unused) of 1 / A(z), A [..., P + 1] with A[0] = 1."""
    A = np.asarray(A, dtype=np.float64)
    P = A.shape[-1] - 1
    c = np.zeros_like(A)
    with np.errstate(all='ignore'):
        c[..., 1] = -A[..., 1]
        for k in range(2, P + 1):
            i = np.arange(1, k)
            c[..., k] = -(A[..., k] + np.sum(i * c[..., 1:k] * A[..., k - 1:0:-1], axis=-1) / k)
    return c


def _autocorrelation(frames, P):
    """R[..., k] = sum_{n = 0}^{N - 1 - k} f[n] f[n + k], k = 0 .. P, of frames [F, N]."""
    N = frames.shape[1]
    return np.stack([np.sum(frames[:, :N - k] * frames[:, k:], axis=1) for k in range(P + 1)], axis=1)


def frame_values(x, y, fs):
    """The per-frame values of the clean signal x and the estimate y (1-D, equal length) at rate fs: (ssnr [F], llr [F], cd [F],
    valid bool [F]), clamped; llr and cd are meaningful where valid (both signals: R[0] > 0 and every E_i > 0)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.shape != y.shape or x.ndim != 1:
        raise ValueError(f'frame_measures: x {x.shape} and y {y.shape} must be 1-D signals of equal length')
    N, S, P = frame_geometry(fs)
    F = frame_count(len(x), fs)
    if F == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0, dtype=bool)
    w = _measure_window(N)
    idx = S * np.arange(F)[:, None] + np.arange(N)[None, :]
    xw, yw = x[idx] * w, y[idx] * w
    with np.errstate(all='ignore'):
        se, ne = np.sum(xw * xw, axis=1), np.sum((xw - yw) ** 2, axis=1)
        ssnr = np.clip(10.0 * np.log10(se / (ne + EPS) + EPS), *SSNR_RANGE)
        Rx, Ry = _autocorrelation(xw, P), _autocorrelation(yw, P)
        (Ax, Ex), (Ay, Ey) = _lpc(Rx, P), _lpc(Ry, P)
        valid = np.all(Ex > 0, axis=1) & np.all(Ey > 0, axis=1)
        T = Rx[:, np.abs(np.arange(P + 1)[:, None] - np.arange(P + 1)[None, :])]           # [F, P + 1, P + 1]
        num, den = np.einsum('fi,fij,fj->f', Ay, T, Ay), np.einsum('fi,fij,fj->f', Ax, T, Ax)
        llr = np.clip(np.log(num / den), *LLR_RANGE)
        cx, cy = _lpc_cepstrum(Ax), _lpc_cepstrum(Ay)
        cd = np.clip(10.0 / np.log(10.0) * np.sqrt(2.0 * np.sum((cx[:, 1:] - cy[:, 1:]) ** 2, axis=1)), *CD_RANGE)
    return ssnr, llr, cd, valid


def frame_measures(x, y, fs):
    """Segmental SNR (dB), LPC log-likelihood ratio and LPC cepstrum distance of the estimate y against the clean signal x
    (1-D, equal length, both at rate fs), after Hu & Loizou's comp_snr.m / comp_llr.m / comp_cep.m -> {'ssnr', 'llr', 'cd'} as
    Python floats.  Frames of N = round(0.03 fs) samples at hop N // 4, the published count (L - N) // (N // 4) (0 below
    N + N // 4 samples), window 0.5 (1 - cos(2 pi (i + 1) / (N + 1))).  ssnr: the mean over ALL frames of 10 log10(se / (ne +
    EPS) + EPS) clamped to [-10, 35] (digital silence counts as -10, as published); NaN without a frame.  llr, cd: per frame
    log(A_y T A_y' / A_x T A_x') clamped to [0, 2] and (10 / ln 10) sqrt(2 sum (c_x - c_y)^2) clamped to [0, 10] from the
    order-P LPC models (P = 16 for fs >= 10000, else 10), over the frames where both recursions keep every error energy
    positive; the score is the mean of the max(1, floor(0.95 V + 0.5)) smallest of those V values, NaN for V = 0.  PARITY
    UNPINNED (see the module docstring): tests/test_frame_measures_cpu.py checks the defining properties and independent
    routes."""
    ssnr, llr, cd, valid = frame_values(x, y, fs)
    return {'ssnr': float(np.mean(ssnr)) if len(ssnr) else float('nan'),
            'llr': _trimmed_mean(llr[valid]), 'cd': _trimmed_mean(cd[valid])}


def ssnr(x, y, fs):
    """frame_measures(x, y, fs)['ssnr']."""
    return frame_measures(x, y, fs)['ssnr']


def llr(x, y, fs):
    """frame_measures(x, y, fs)['llr']."""
    return frame_measures(x, y, fs)['llr']


def cepstrum_distance(x, y, fs):
    """frame_measures(x, y, fs)['cd']."""
    return frame_measures(x, y, fs)['cd']


def measure_window(fs, device):
    """_measure_window(N) of rate fs as float64 [N] on `device` (cached): the host function's own bits."""
    N = frame_geometry(fs)[0]
    key = ('measure_window', N, str(device))
    t = _device_tables.get(key)
    if t is None:
        import torch
        t = torch.from_numpy(_measure_window(N)).to(device)
        _device_tables[key] = t
    return t


def frame_measures_ragged(clean, estimate, offsets, fs, longest=None):
    """frame_measures(clean[a:b], estimate[a:b], fs) for every recording [a, b) = offsets[i:i + 2] of two flat device buffers ->
    {'ssnr', 'llr', 'cd'}: float32 [n] device tensors (NaN where the host function has NaN), fp64 until that rounding, in three
    launches whatever n is (csrc/frame_measures.hip) and without a host read-back (capturable when offsets are on the
    device).  No resampling: the measures are taken at the signals' own rate fs, 8000 .. 48000 (DcsHipError otherwise).
    offsets, longest: as for stoi_ragged (no grid here depends on longest).  CPU signals raise DcsHipError."""
    from . import ops
    clean, estimate, offsets, _ = _ragged_args('frame_measures_ragged', clean, estimate, offsets, longest)
    s, l, c = ops.frame_measures_ragged(clean, estimate, offsets, fs)
    return {'ssnr': s, 'llr': l, 'cd': c}
