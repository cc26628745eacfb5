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
tests/test_frame_measures_device.py).

WSS, fwSegSNR, composites.  `spectral_measures()` restates the weighted spectral slope and the frequency-weighted segmental
SNR of the same paper after `comp_wss.m` / `comp_fwseg.m`: the frame measures' framing, a zero-padded FFT, 25 Gaussian-shaped
critical bands.  PARITY UNPINNED for the same reason (tests/test_spectral_measures_cpu.py: defining properties and
independent routes).  On the device it is `spectral_measures_ragged()` (csrc/spectral_measures.hip, an fp64 FFT in LDS;
tests/test_spectral_measures_device.py).  `composite_measures()` is Hu & Loizou's CSIG / CBAK / COVL regression on PESQ,
LLR, WSS and segmental SNR; the PESQ values come from the caller.

BSS-eval SDR.  `sdr()` restates the signal-to-distortion ratio of Vincent, Gribonval & Fevotte (2006) as
`mir_eval.separation.bss_eval_sources` computes it for one source: the estimate projected onto 512 delayed copies of the
reference (Toeplitz normal equations by a Levinson recursion written out here, both energies summed explicitly).  PARITY
UNPINNED, as for STOI: mir_eval is not here; tests/test_sdr_cpu.py checks a brute-force projection, two other solvers and the
defining properties.  On the device it is `sdr_ragged()` (csrc/sdr_ragged.hip, fp64; tests/test_sdr_device.py).

Active speech level.  `active_speech_level()` restates ITU-T P.56 method B after the published `asl_P56` of Hu & Loizou (two
one-pole envelope smoothers, 15 power-of-two thresholds with a 0.2 s hangover, the 15.9 dB margin), taking the margin crossing
itself where the published code bisects to 0.5 dB.  PARITY UNPINNED, as for STOI; tests/test_active_level_cpu.py checks the
counts against a literal transcription of the published loop.  On the device it is ops.active_level_ragged
(csrc/speech_level.hip, fp64; tests/test_active_level.py), which MixingAudioStore(level='p56') reads once per store.

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


def _device_table(key, build):
    """_device_tables[key], made by build() on the first call."""
    t = _device_tables.get(key)
    if t is None:
        t = _device_tables[key] = build()
    return t


def stoi_band_edges(device):
    """thirdoct(10000, 512, 15, 150)'s rows as bin ranges [lo, hi): int32 [2, 15] on `device` (cached)."""
    def build():
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
        return torch.tensor([lo, hi], dtype=torch.int32).to(device)
    return _device_table(('bands', str(device)), build)


def resample_taps(fs_sig, device):
    """(h float32 [taps] on `device` = the normalised window of resample_oct(., FS, fs_sig), up, down) (cached)."""
    fs_sig = int(fs_sig)

    def build():
        import torch
        g = int(np.gcd(FS, fs_sig))
        h = _resample_window_oct(FS, fs_sig)
        return torch.tensor(h / np.sum(h), dtype=torch.float32).to(device), FS // g, fs_sig // g
    return _device_table(('taps', fs_sig, str(device)), build)


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

    def build():
        import torch
        return torch.from_numpy(_measure_window(N)).to(device)
    return _device_table(('measure_window', N, str(device)), build)


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


# ---- weighted spectral slope, frequency-weighted segmental SNR, the composite measures (Hu & Loizou) ----------------------------

CRIT_CENTRES = np.array([50.0, 120.0, 190.0, 260.0, 330.0, 400.0, 470.0, 540.0, 617.372, 703.378, 798.717, 904.128, 1020.38,
                         1148.30, 1288.72, 1442.54, 1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17,
                         3597.63])                            # Hz
CRIT_BANDWIDTHS = np.array([70.0] * 7 + [77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423, 153.823, 168.154,
                                         183.457, 199.776, 217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136])
NUM_CRIT = 25
CRIT_MIN_FACTOR = float(np.exp(-30.0 / (2.0 * 2.303)))      # band weights at or below it are 0
WSS_FLOOR = 1e-10                                             # of a band's power, before the logarithm
FWSSNR_RANGE = (-10.0, 35.0)                                  # dB, per frame
FWSSNR_GAMMA = 0.2


def spectral_fft_size(fs):
    """The smallest power of two >= 2 N, N = round(0.03 fs): 512 at 8 kHz, 1024 at 16 kHz, 2048 at 22.05 kHz, 4096 at 48 kHz."""
    nfft = 1
    while nfft < 2 * frame_geometry(fs)[0]:
        nfft *= 2
    return nfft


def critical_band_bank(fs, nfft=None):
    """g [25, H], H = nfft / 2: band i is exp(-11 ((j - f0) / bw)^2 + ln 70 - ln bandwidth_i) over the bins j, with
    f0 = floor(centre_i / (fs / 2) H) and bw = bandwidth_i / (fs / 2) H, and 0 wherever that does not exceed CRIT_MIN_FACTOR."""
    H = (spectral_fft_size(fs) if nfft is None else int(nfft)) // 2
    half = float(fs) / 2.0
    f0 = np.floor(CRIT_CENTRES / half * H)
    bw = CRIT_BANDWIDTHS / half * H
    j = np.arange(H, dtype=np.float64)
    g = np.exp(-11.0 * ((j[None, :] - f0[:, None]) / bw[:, None]) ** 2 + (np.log(70.0) - np.log(CRIT_BANDWIDTHS))[:, None])
    g[g <= CRIT_MIN_FACTOR] = 0.0
    return g


def compact_bank(g):
    """The bank's non-zero runs: (first int32 [25], offset int32 [26], weights float64 [offset[25]]); band i is
    g[i, first[i]:first[i] + offset[i + 1] - offset[i]] == weights[offset[i]:offset[i + 1]], and 0 elsewhere."""
    first, offset, weights = [], [0], []
    for row in g:
        nz = np.flatnonzero(row)
        a, b = (int(nz[0]), int(nz[-1]) + 1) if len(nz) else (0, 0)
        assert len(nz) == b - a, 'a band is one contiguous run of bins'
        first.append(a)
        offset.append(offset[-1] + b - a)
        weights.append(row[a:b])
    return np.array(first, dtype=np.int32), np.array(offset, dtype=np.int32), np.concatenate(weights)


def _nearest_peaks(e):
    """The published search for the band energy of the nearest spectral peak: e [F, 25] dB -> peak [F, 24], one per slope
    s_i = e_{i+1} - e_i.  Rising (s_i > 0): n = i, advance n while n < 24 and s_n > 0, peak_i = e_{n-1} — the band BELOW the one
    the search stops at: the published code's off-by-one, kept.  Otherwise: n = i, step n down while n >= 0 and s_n <= 0,
    peak_i = e_{n+1}."""
    e = np.asarray(e, dtype=np.float64)
    F, rows = e.shape[0], np.arange(e.shape[0])
    s = e[:, 1:] - e[:, :-1]
    peak = np.empty((F, NUM_CRIT - 1))
    for i in range(NUM_CRIT - 1):
        rising = s[:, i] > 0
        up = np.full(F, i)
        down = np.full(F, i)
        for _ in range(NUM_CRIT):
            go = rising & (up < NUM_CRIT - 1)
            go[go] = s[rows[go], up[go]] > 0
            up = up + go
            go = ~rising & (down >= 0)
            go[go] = s[rows[go], down[go]] <= 0
            down = down - go
        peak[:, i] = np.where(rising, e[rows, np.maximum(up - 1, 0)], e[rows, down + 1])
    return peak


def _wss_weights(e):
    """W [F, 24] of one signal: 20 / (20 + max_k e_k - e_i) times 1 / (1 + peak_i - e_i)."""
    peak = _nearest_peaks(e)
    return (20.0 / (20.0 + np.max(e, axis=1, keepdims=True) - e[:, :-1])) * (1.0 / (1.0 + peak - e[:, :-1]))


def spectral_frame_values(x, y, fs):
    """The per-frame values of the clean signal x and the estimate y (1-D, equal length) at rate fs: (wss [F], fwssnr [F], valid
    bool [F]); fwssnr is clamped and meaningful where valid (both magnitude spectra have a positive sum), wss is finite in
    every frame."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.shape != y.shape or x.ndim != 1:
        raise ValueError(f'spectral_measures: x {x.shape} and y {y.shape} must be 1-D signals of equal length')
    N, S, _ = frame_geometry(fs)
    F = frame_count(len(x), fs)
    if F == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0, dtype=bool)
    nfft = spectral_fft_size(fs)
    H = nfft // 2
    g = critical_band_bank(fs, nfft)
    w = _measure_window(N)
    wss, fw, valid = np.empty(F), np.zeros(F), np.zeros(F, dtype=bool)
    for a in range(0, F, 2048):                              # bounded memory for long recordings
        b = min(a + 2048, F)
        idx = S * np.arange(a, b)[:, None] + np.arange(N)[None, :]
        power, mag, energy = [], [], []
        for sig in (x, y):
            spec = np.fft.rfft(sig[idx] * w, n=nfft, axis=1)[:, :H]
            p = spec.real ** 2 + spec.imag ** 2
            power.append(p)
            mag.append(np.sqrt(p))
            energy.append(10.0 * np.log10(np.maximum(p @ g.T, WSS_FLOOR)))
        ex, ey = energy
        sx, sy = ex[:, 1:] - ex[:, :-1], ey[:, 1:] - ey[:, :-1]
        W = 0.5 * (_wss_weights(ex) + _wss_weights(ey))
        wss[a:b] = np.sum(W * (sx - sy) ** 2, axis=1) / np.sum(W, axis=1)
        tx, ty = np.sum(mag[0], axis=1), np.sum(mag[1], axis=1)
        ok = (tx > 0) & (ty > 0)
        valid[a:b] = ok
        with np.errstate(all='ignore'):
            c = (mag[0][ok] / tx[ok, None]) @ g.T
            p = (mag[1][ok] / ty[ok, None]) @ g.T
            err = np.maximum((c - p) ** 2, EPS)
            wgt = c ** FWSSNR_GAMMA
            fw[a:b][ok] = np.clip(np.sum(wgt * 10.0 * np.log10(c * c / err), axis=1) / np.sum(wgt, axis=1), *FWSSNR_RANGE)
    return wss, fw, valid


def spectral_measures(x, y, fs):
    """Weighted spectral slope (WSS) and frequency-weighted segmental SNR (fwSegSNR, dB) of the estimate y against the clean
    signal x (1-D, equal length, both at rate fs), after Hu & Loizou's comp_wss.m / comp_fwseg.m -> {'wss', 'fwssnr'} as Python
    floats.  The frame measures' framing (frame_geometry, frame_count, _measure_window); per frame |FFT(frame w, nfft)| on the
    bins 0 .. nfft / 2 - 1, nfft = spectral_fft_size(fs); the 25 bands of critical_band_bank.  wss: band energies
    e_i = 10 log10(max(sum |X|^2 g_i, 1e-10)), slopes s_i = e_{i+1} - e_i, weights from the distance to the largest band and
    to the nearest peak (_nearest_peaks: the published rising search and its off-by-one are KEPT as published), averaged over
    both signals; the frame value is sum W_i (s_i^x - s_i^y)^2 / sum W_i, and the score the mean of the
    max(1, floor(0.95 F + 0.5)) smallest of ALL F frame values (the floor makes silence finite); NaN without a frame.  fwssnr:
    magnitude spectra normalised to unit sum, band values c_i (clean) and p_i (estimate), frame value
    sum c_i^0.2 10 log10(c_i^2 / max((c_i - p_i)^2, EPS)) / sum c_i^0.2 clamped to [-10, 35]; the score is the mean over the
    frames where both magnitude sums are positive, NaN for none.  The formulae leave one case undefined and it is kept as it
    falls: a band on which the clean magnitude is exactly 0 while the frame is not silent (band-limited synthetic input; no
    signal with a noise floor) has c_i = 0, its term is 0 x log10(0) = NaN, and with it the frame's and the recording's
    fwssnr — on the device as here.  PARITY UNPINNED (see the module docstring): neither the
    MATLAB originals nor pysepm are here to compare with; tests/test_spectral_measures_cpu.py checks the defining properties
    and independent routes."""
    wss, fw, valid = spectral_frame_values(x, y, fs)
    return {'wss': _trimmed_mean(wss), 'fwssnr': float(np.mean(fw[valid])) if valid.any() else float('nan')}


def wss(x, y, fs):
    """spectral_measures(x, y, fs)['wss']."""
    return spectral_measures(x, y, fs)['wss']


def fwssnr(x, y, fs):
    """spectral_measures(x, y, fs)['fwssnr']."""
    return spectral_measures(x, y, fs)['fwssnr']


def composite_measures(pesq, llr, wss, ssnr):
    """Hu & Loizou's composite measures from PESQ, LLR, WSS and segmental SNR -> {'csig', 'cbak', 'covl'} (signal distortion,
    background intrusiveness, overall quality), each clamped to [1, 5].  Elementwise on numbers, numpy arrays or torch tensors
    of any device."""
    import torch
    if any(isinstance(v, torch.Tensor) for v in (pesq, llr, wss, ssnr)):
        def clamp(v):
            return v.clamp(1.0, 5.0)
    else:
        pesq, llr, wss, ssnr = (np.asarray(v, dtype=np.float64) for v in (pesq, llr, wss, ssnr))

        def clamp(v):
            return np.clip(v, 1.0, 5.0)
    return {'csig': clamp(3.093 - 1.029 * llr + 0.603 * pesq - 0.009 * wss),
            'cbak': clamp(1.634 + 0.478 * pesq - 0.007 * wss + 0.063 * ssnr),
            'covl': clamp(1.594 + 0.805 * pesq - 0.512 * llr - 0.007 * wss)}


def spectral_tables(fs, device):
    """What the device pass reads, on `device` (cached): (window float64 [N], band_first int32 [25], band_offset int32 [26],
    band_weights float64, twiddles float64 [nfft, 2] = (cos, -sin)(2 pi m / nfft)); the window and the weights are the host
    function's own bits."""
    fs = int(fs)

    def build():
        import torch
        nfft = spectral_fft_size(fs)
        first, offset, weights = compact_bank(critical_band_bank(fs, nfft))
        angle = 2.0 * np.pi * np.arange(nfft) / nfft
        twiddles = np.stack([np.cos(angle), -np.sin(angle)], axis=1)
        return (measure_window(fs, device),) + tuple(torch.from_numpy(np.ascontiguousarray(v)).to(device)
                                                     for v in (first, offset, weights, twiddles))
    return _device_table(('spectral', fs, str(device)), build)


def spectral_measures_ragged(clean, estimate, offsets, fs, longest=None):
    """spectral_measures(clean[a:b], estimate[a:b], fs) for every recording [a, b) = offsets[i:i + 2] of two flat device buffers
    -> {'wss', 'fwssnr'}: float32 [n] device tensors (NaN where the host function has NaN), fp64 until that rounding, in three
    launches whatever n is (csrc/spectral_measures.hip) and without a host read-back (capturable when offsets are on the
    device).  At the signals' own rate fs, 8000 .. 48000 (DcsHipError otherwise).  offsets, longest: as for stoi_ragged (no grid
    here depends on longest).  CPU signals raise DcsHipError."""
    from . import ops
    clean, estimate, offsets, _ = _ragged_args('spectral_measures_ragged', clean, estimate, offsets, longest)
    w, f = ops.spectral_measures_ragged(clean, estimate, offsets, fs)
    return {'wss': w, 'fwssnr': f}


# ---- the signal-to-distortion ratio of BSS-eval ---------------------------------------------------------------------------------

SDR_FILTER_LENGTH = 512         # bss_eval_sources' flen


def sdr_correlations(x, y, filter_length=SDR_FILTER_LENGTH):
    """(R [K], D [K]) of 1-D float64 signals of equal length L: R[k] = sum_t x[t] x[t + k], D[k] = sum_t x[t] y[t + k] over
    the samples that exist (0 for k >= L)."""
    L, K = len(x), int(filter_length)
    R, D = np.zeros(K), np.zeros(K)
    for k in range(min(K, L)):
        R[k] = np.dot(x[:L - k], x[k:])
        D[k] = np.dot(x[:L - k], y[k:])
    return R, D


def toeplitz_levinson(R, D):
    """Solve the symmetric Toeplitz system T(R) c = D (T[i, j] = R[|i - j|]) by the Levinson recursion in fp64 -> (c [K], E [K]):
    E[m] is the forward prediction error energy after step m (E[0] = R[0]); the recursion stops at the first E[m] that is not a
    positive finite number, leaving the rest of E as NaN (c is then meaningless)."""
    R, D = np.asarray(R, dtype=np.float64), np.asarray(D, dtype=np.float64)
    K = len(R)
    a, c, E = np.zeros(K), np.zeros(K), np.full(K, np.nan)      # a[1 .. m - 1]: the forward predictor of order m - 1
    E[0] = R[0]
    if not (E[0] > 0 and np.isfinite(E[0])):
        return c, E
    c[0] = D[0] / R[0]
    with np.errstate(all='ignore'):
        for m in range(1, K):
            kappa = (R[m] - np.dot(a[1:m], R[m - 1:0:-1])) / E[m - 1]
            a[1:m] = a[1:m] - kappa * a[m - 1:0:-1]
            a[m] = kappa
            E[m] = E[m - 1] * (1.0 - kappa * kappa)
            if not (E[m] > 0 and np.isfinite(E[m])):
                return c, E
            delta = (D[m] - np.dot(c[:m], R[m:0:-1])) / E[m]
            c[:m] -= delta * a[m:0:-1]
            c[m] = delta
    return c, E


def sdr_from_filter(x, y, c):
    """10 log10(sum s^2 / sum (y_pad - s)^2) with s = c * x on its L + K - 1 positions and y padded with K - 1 zeros: both
    energies summed explicitly (num = c'D and den = |y|^2 - c'D cancel at high SDR).  +inf for den == 0 < num; NaN when either
    energy is not finite or both are 0."""
    x, y, c = (np.asarray(v, dtype=np.float64) for v in (x, y, c))
    with np.errstate(all='ignore'):
        s = np.convolve(x, c)
        e = -s
        e[:len(y)] += y
        num, den = float(np.dot(s, s)), float(np.dot(e, e))
        if not (np.isfinite(num) and np.isfinite(den)) or (num == 0.0 and den == 0.0):
            return float('nan')
        if den == 0.0:
            return float('inf')
        return float(10.0 * np.log10(num / den))


def sdr(x, y, filter_length=SDR_FILTER_LENGTH):
    """The signal-to-distortion ratio of BSS-eval (E. Vincent, R. Gribonval, C. Fevotte, "Performance Measurement in Blind Audio
    Source Separation", IEEE TASLP 14(4), 2006) of the estimate y against the reference x (1-D, equal length L, taken as
    float64), in dB: y is projected onto the span of the K = filter_length (1 .. 512) delayed copies x[t - k], k < K, and the
    energy of the projection s is set against the energy of y - s.  R, D: sdr_correlations; the filter c: toeplitz_levinson;
    the energies: sdr_from_filter.  In exact arithmetic this is mir_eval.separation.bss_eval_sources for one source (SDR = SAR,
    SIR = +inf, flen = 512).  Unlike SI-SNR, which forgives a gain only, it forgives any filter of up to K taps between the two
    signals, a delay among them.  +inf when the residual is exactly 0; NaN for L == 0, for an all-zero x or y (mir_eval raises
    there), for an input that is not finite, and when an error energy E_m of the recursion is <= 0 or not finite.  PARITY
    UNPINNED, as for STOI: neither mir_eval nor museval is here to compare with; tests/test_sdr_cpu.py checks it against a
    brute-force least-squares projection, two other solvers and its defining properties."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    K = int(filter_length)
    if x.shape != y.shape or x.ndim != 1:
        raise ValueError(f'sdr: x {x.shape} and y {y.shape} must be 1-D signals of equal length')
    if not 1 <= K <= SDR_FILTER_LENGTH:
        raise ValueError(f'sdr: filter_length={filter_length} (1 .. {SDR_FILTER_LENGTH})')
    if len(x) == 0 or not (np.all(np.isfinite(x)) and np.all(np.isfinite(y))) or not x.any() or not y.any():
        return float('nan')
    c, E = toeplitz_levinson(*sdr_correlations(x, y, K))
    if not np.all(E > 0):                                    # NaN where the recursion stopped
        return float('nan')
    return sdr_from_filter(x, y, c)


def sdr_ragged(clean, estimate, offsets, filter_length=SDR_FILTER_LENGTH, estimate2=None):
    """sdr(clean[a:b], estimate[a:b], filter_length) for every recording [a, b) = offsets[i:i + 2] of two flat device buffers: a
    float32 [n] device tensor (NaN and +inf where the host function has them), fp64 until that rounding, in four launches
    whatever n is (csrc/sdr_ragged.hip) and without a host read-back (capturable when offsets are on the device).  A
    recording's value is bit-equal to that recording scored alone.  estimate2: a second estimate against the same clean buffer
    (the unprocessed signal beside the enhanced one) in the same launches -> the pair of tensors, each bit-equal to a call of
    its own; the correlation of the clean signal and the forward recursion are shared.  The measure is rate-free.  offsets: as
    for stoi_ragged.  CPU signals raise DcsHipError."""
    from . import ops
    clean, estimate, offsets, _ = _ragged_args('sdr_ragged', clean, estimate, offsets, None)
    if estimate2 is None:
        return ops.sdr_ragged(clean, estimate, offsets, filter_length=filter_length)
    _, estimate2, _, _ = _ragged_args('sdr_ragged', clean, estimate2, offsets, None)
    return ops.sdr_ragged(clean, estimate, offsets, est2=estimate2, filter_length=filter_length)


# ---- ITU-T P.56 active speech level (method B) -------------------------------------------------------------------------------------

P56_T = 0.03                    # s, time constant of each of the two envelope smoothers
P56_H = 0.2                     # s, hangover
P56_THRESHOLDS = 15             # c[j] = 2 ** (j - 15): the 16-bit thresholds of the published code, on a full scale of 1
P56_MARGIN_DB = 15.9


def p56_hangover(fs):
    """I = ceil(0.2 fs) samples, in integers."""
    fs = int(fs)
    if fs <= 0:
        raise ValueError(f'p56_hangover: fs={fs}')
    return -(-fs // 5)


def p56_envelope(x, fs):
    """q: |x| through the one-pole smoother g = exp(-1 / (0.03 fs)) twice, each from zero state (scipy.signal.lfilter, fp64)."""
    from scipy.signal import lfilter
    g = np.exp(-1.0 / (int(fs) * P56_T))
    p = lfilter([1.0 - g], [1.0, -g], np.abs(np.asarray(x, dtype=np.float64)))
    return lfilter([1.0 - g], [1.0, -g], p)


def windowed_max(q, I):
    """m[k] = max(q[max(0, k - I) .. k]) by block prefix and suffix maxima (van Herk) over blocks of I + 1 samples: exact."""
    q = np.asarray(q, dtype=np.float64)
    n, W = len(q), int(I) + 1
    if n == 0:
        return q.copy()
    blocks = -(-n // W)
    b = np.full(blocks * W, -np.inf)
    b[:n] = q
    b = b.reshape(blocks, W)
    prefix = np.maximum.accumulate(b, axis=1).reshape(-1)[:n]
    suffix = np.maximum.accumulate(b[:, ::-1], axis=1)[:, ::-1].reshape(-1)[:n]
    m = prefix.copy()
    if n > I:                                                # the window [k - I, k] lies in at most two blocks
        m[I:] = np.maximum(prefix[I:], suffix[:n - I])
    return m


def p56_level(sq, n, counts, margin_db=P56_MARGIN_DB):
    """(active_power, activity) from the sum of squares, the length and the 15 activity counts: the level arithmetic of
    active_speech_level, in the order of operations the device kernel repeats."""
    nan = (float('nan'), float('nan'))
    if n == 0 or counts[0] == 0 or not np.isfinite(sq):
        return nan
    M = float(margin_db)
    with np.errstate(all='ignore'):
        a_prev = 10.0 * np.log10(sq / float(counts[0]))
        d_prev = a_prev - 20.0 * np.log10(2.0 ** -15)
        if d_prev < M:
            return nan
        for j in range(1, P56_THRESHOLDS):
            if counts[j] == 0:
                return nan
            a_j = 10.0 * np.log10(sq / float(counts[j]))
            d_j = a_j - 20.0 * np.log10(2.0 ** (j - 15))
            if d_j <= M:
                t = (d_prev - M) / (d_prev - d_j)
                level_db = a_prev + t * (a_j - a_prev)
                active = float(10.0 ** (level_db / 10.0))
                return active, float((sq / n) / active)
            a_prev, d_prev = a_j, d_j
    return nan


def active_speech_level(x, fs, margin_db=P56_MARGIN_DB):
    """The ITU-T P.56 (method B) active speech level of the 1-D signal x at the integer rate fs, after the published asl_P56 of
    Hu & Loizou with its 16-bit thresholds on a full scale of 1 -> {'active_power', 'activity', 'counts'}: the mean square over
    the ACTIVE part of the signal, the share of it that is active (activity * active_power = mean(x^2)) and the 15 activity
    counts (int64).  Host-side numpy / scipy in fp64.

    q = |x| smoothed twice by y[k] = g y[k - 1] + (1 - g) u[k], g = exp(-1 / (0.03 fs)), from zero state.  counts[j] is the
    number of samples k with max(q[max(0, k - I) .. k]) >= c[j] = 2 ** (j - 15), I = ceil(0.2 fs): the published hangover
    counter (reset where q[k] >= c[j], counting while below I, expired at the start) in closed form; nothing is counted past
    the end of the signal.  With A[j] = 10 log10(sum(x^2) / counts[j]) and D[j] = A[j] - 20 log10(c[j]), the level is where
    D crosses the margin: for the first j >= 1 with D[j] <= margin_db, A is interpolated linearly in dB between j - 1 and j to
    D = margin_db, and active_power = 10 ** (A / 10).  The published code bisects to within 0.5 dB of that crossing; this takes
    the crossing itself, so the result carries no tolerance parameter.  Both values are NaN for an empty signal, a signal that
    never reaches c[0] (counts[0] = 0), D[0] < margin_db, a sum of squares that is not finite, or no crossing before the
    counts run out.

    PARITY UNPINNED, as for STOI: no ITU or MATLAB implementation is here to compare with; tests/test_active_level_cpu.py
    checks the counts against a literal transcription of the published loop and the defining properties.  On the device it is
    ops.active_level_ragged (csrc/speech_level.hip); this function is its numerics contract (tests/test_active_level.py)."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 1:
        raise ValueError(f'active_speech_level: expected a 1-D signal, got shape {x.shape}')
    if int(fs) != fs or int(fs) <= 0:
        raise ValueError(f'active_speech_level: fs={fs} must be a positive integer')
    n = len(x)
    counts = np.zeros(P56_THRESHOLDS, dtype=np.int64)
    if n:
        m = windowed_max(p56_envelope(x, fs), p56_hangover(fs))
        counts[:] = [np.count_nonzero(m >= 2.0 ** (j - 15)) for j in range(P56_THRESHOLDS)]
    with np.errstate(all='ignore'):
        sq = float(np.sum(x * x))
    active, activity = p56_level(sq, n, counts, margin_db)
    return {'active_power': active, 'activity': activity, 'counts': counts}
