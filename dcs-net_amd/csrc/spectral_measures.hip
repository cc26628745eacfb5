// spectral_measures.hip — the weighted spectral slope (WSS) and the frequency-weighted segmental SNR (fwSegSNR) of Hu & Loizou
// of whole recordings of different lengths, for the project's ragged convention (ragged_common.h).  The host function
// dcsnet/metrics.py::spectral_measures is the numerics contract; everything here is fp64 until the two float32 outputs.
//
// Framing, workspace (2 value planes) and the prefix launch are ragged_frames.h's, shared with frame_measures.hip; the window
// double[N] comes from the host.  nfft = 2^LOG = the smallest power of two >= 2 N (LOG = 9 .. 12), H = nfft / 2 bins.  25 critical
// bands as a compact table from the host (metrics.compact_bank: first bin, offset into the weights, the weights' own bits).
// This source owns the Stockham passes, the band sums and the peak search, and:
//
//   spectral_frame_kernel<LOG>                  one workgroup of 256 per frame slot g < fbase[n] (frame_slot finds its samples):
//       z = x w + i y w, zero-padded, into LDS (double2[nfft], the kernel's only LDS: 8 KiB .. 64 KiB);
//       one complex Stockham transform in that buffer: a radix-2 pass when LOG is odd, then radix-4 passes; every thread reads
//       the inputs of its butterflies into registers, the workgroup synchronises, and it writes their outputs (autosort, no
//       second buffer); twiddles (cos, -sin)(2 pi m / nfft) from the host's double table;
//       X[k] = (Z[k] + conj Z[nfft - k]) / 2, Y[k] = (Z[k] - conj Z[nfft - k]) / (2 i) for k < H, and slot k <- (|X[k]|^2, |Y[k]|^2)
//       (slot k is read by its own thread only); the upper half of the buffer is free from here on and holds the sums below;
//       the two magnitude sums (a thread adds k = t, t + 256, ... in ascending order, a wave butterfly, the 4 waves in order);
//       the 2 x 2 x 25 band sums: 8 lanes per band (lane l adds the band's bins l, l + 8, ... in ascending order, a 3-step
//       butterfly): power for WSS, magnitude / magnitude sum for fwSegSNR;
//       band i's first lane: e_i of both signals, and the band's fwSegSNR weight and term; threads 0 .. 23: the two peak
//       searches of slope i and its weighted term; thread 0: the two sums over the bands in ascending order ->
//       vals[0][g] = the frame's WSS, vals[1][g] = its fwSegSNR clamped to [-10, 35] dB, valid[g] = both magnitude sums > 0
//       (a band with c_i = 0 in a valid frame gives 0 x log10(0) = NaN for the frame, as in the host function: the formulae
//       leave it undefined);
//       the grid is the capacity Fcap = total / S, not the frame count (the host does not read the offsets): per recording
//       about N / S = 4 slots, and all L / S of one shorter than N + S, go to workgroups that exit at once
//   spectral_recording_kernel                   one workgroup per recording: the mean of the valid fwSegSNR values; the WSS
//       trimmed mean over ALL F frames (K = max(1, floor(0.95 F + 0.5))) by trimmed_means<1, false> (WSS values are
//       non-negative doubles); NaN for both without a frame, for fwSegSNR without a valid one
//
// Three launches whatever n is (two when total < S).  No atomics, no cross-workgroup synchronisation, no host read-back:
// capturable, bit-reproducible, and a recording's scores do not depend on its neighbours.
#include "ragged_frames.h"

namespace {

using namespace dcs_ragged;

constexpr int kBands = 25;
constexpr int kThreads = 256;
constexpr double kEps = 2.220446049250313e-16;                // np.finfo(np.float64).eps
constexpr double kFloor = 1e-10;                              // of a band's power, before the logarithm

inline int log_nfft(int N) {                                  // fs <= 48000: N <= 1440, nfft <= 4096
    int log = 9;
    while ((1 << log) < 2 * N) ++log;
    return log;
}

__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// One Stockham pass of radix R (2 or 4) over buf[2^LOG] with Ns = the product of the radices before it: butterfly j < 2^LOG / R
// takes buf[j + r 2^LOG / R] times w^(k r), k = j mod Ns, w = exp(-2 pi i / (Ns R)), and leaves its outputs at
// (j - k) R + k + r Ns.  Every thread holds the inputs of its butterflies in registers across the barrier, so the pass works in
// one buffer.
template <int LOG, int R>
__device__ __forceinline__ void stockham_pass(double2* __restrict__ buf, const double2* __restrict__ tw, int Ns, int t) {
    constexpr int N = 1 << LOG, NB = N / R, BPT = NB > kThreads ? NB / kThreads : 1;
    double2 v[BPT][R];
#pragma unroll
    for (int b = 0; b < BPT; ++b) {
        const int j = t + kThreads * b;
        if (j < NB) {
#pragma unroll
            for (int r = 0; r < R; ++r) v[b][r] = buf[j + r * NB];
        }
    }
    __syncthreads();
    const int step = N / (R * Ns);                           // w^(k r) = tw[k r step]; k r step < N
#pragma unroll
    for (int b = 0; b < BPT; ++b) {
        const int j = t + kThreads * b;
        if (j < NB) {
            const int k = j & (Ns - 1);
            double2* __restrict__ o = buf + (j - k) * R + k;
            if constexpr (R == 2) {                           // only as the first pass: Ns = 1, no twiddle
                o[0] = cadd(v[b][0], v[b][1]);
                o[Ns] = csub(v[b][0], v[b][1]);
            } else {
                const double2 v1 = cmul(v[b][1], tw[k * step]), v2 = cmul(v[b][2], tw[2 * k * step]),
                              v3 = cmul(v[b][3], tw[3 * k * step]);
                const double2 a0 = cadd(v[b][0], v2), a1 = csub(v[b][0], v2), a2 = cadd(v1, v3), d = csub(v1, v3);
                const double2 a3 = make_double2(d.y, -d.x);  // -i d
                o[0] = cadd(a0, a2);
                o[Ns] = cadd(a1, a3);
                o[2 * Ns] = csub(a0, a2);
                o[3 * Ns] = csub(a1, a3);
            }
        }
    }
    __syncthreads();
}

// the band energy of the nearest peak of slope i (metrics._nearest_peaks: the published search, its off-by-one kept)
__device__ __forceinline__ double nearest_peak(const double* __restrict__ e, int i) {
    if (e[i + 1] - e[i] > 0.0) {
        int n = i;
        while (n < kBands - 1 && e[n + 1] - e[n] > 0.0) ++n;
        return e[n - 1];                                     // n > i >= 0
    }
    int n = i;
    while (n >= 0 && e[n + 1] - e[n] <= 0.0) --n;
    return e[n + 1];
}

// dynamic LDS: double2[2^LOG]
template <int LOG>
__global__ __launch_bounds__(kThreads) void spectral_frame_kernel(
    const float* __restrict__ clean, const float* __restrict__ est, const long* __restrict__ offsets, int n, long total,
    const long* __restrict__ fbase, const double* __restrict__ window, int N, int S, const int* __restrict__ band_first,
    const int* __restrict__ band_offset, const double* __restrict__ band_weights, int n_weights,
    const double2* __restrict__ tw, long Fcap, double* __restrict__ vals, int* __restrict__ valid) {
    constexpr int NFFT = 1 << LOG, H = NFFT / 2;
    extern __shared__ double2 buf[];
    const long g = blockIdx.x;
    long base;
    if (!frame_slot(offsets, n, total, fbase, g, S, &base)) return;
    const float* __restrict__ c = clean + base;
    const float* __restrict__ e = est + base;
    const int t = threadIdx.x;
    for (int i = t; i < NFFT; i += kThreads) {               // N <= NFFT / 2 (the host checks it)
        double2 z = make_double2(0.0, 0.0);
        if (i < N) {
            const double w = window[i];
            z = make_double2(w * (double)c[i], w * (double)e[i]);
        }
        buf[i] = z;
    }
    __syncthreads();
    int Ns = 1;
    if constexpr (LOG & 1) {
        stockham_pass<LOG, 2>(buf, tw, 1, t);
        Ns = 2;
    }
    for (; Ns < NFFT; Ns *= 4) stockham_pass<LOG, 4>(buf, tw, Ns, t);

    // the two power spectra into the lower half, the two magnitude sums
    double mx = 0.0, my = 0.0;
    for (int k = t; k < H; k += kThreads) {
        const double2 a = buf[k], b = buf[(NFFT - k) & (NFFT - 1)];
        const double xr = 0.5 * (a.x + b.x), xi = 0.5 * (a.y - b.y);       // X = (Z[k] + conj Z[-k]) / 2
        const double yr = 0.5 * (a.y + b.y), yi = 0.5 * (b.x - a.x);       // Y = (Z[k] - conj Z[-k]) / (2 i)
        const double px = xr * xr + xi * xi, py = yr * yr + yi * yi;
        buf[k] = make_double2(px, py);
        mx += sqrt(px);
        my += sqrt(py);
    }
    mx = dcs_wave_sum_d(mx);
    my = dcs_wave_sum_d(my);
    __syncthreads();                                         // the upper half is free now
    double* __restrict__ up = reinterpret_cast<double*>(buf + H);           // double[NFFT], NFFT >= 512
    double* __restrict__ wave_x = up;                        // [4]
    double* __restrict__ wave_y = up + 4;                    // [4]
    double* __restrict__ ex = up + 8;                        // [25] band energies of the clean signal, dB
    double* __restrict__ ey = ex + kBands;                   // [25] of the estimate
    double* __restrict__ fw_w = ey + kBands;                 // [25] c_i^0.2
    double* __restrict__ fw_t = fw_w + kBands;               // [25] c_i^0.2 10 log10(c_i^2 / err_i)
    double* __restrict__ ws_w = fw_t + kBands;               // [24] W_i
    double* __restrict__ ws_t = ws_w + kBands;               // [24] W_i (s_i^x - s_i^y)^2
    if ((t & 63) == 0) {
        wave_x[t >> 6] = mx;
        wave_y[t >> 6] = my;
    }
    __syncthreads();
    const double tx = ((wave_x[0] + wave_x[1]) + wave_x[2]) + wave_x[3];
    const double ty = ((wave_y[0] + wave_y[1]) + wave_y[2]) + wave_y[3];
    const bool ok = tx > 0.0 && ty > 0.0;                    // uniform over the workgroup

    const int band = t >> 3, l = t & 7;                      // bands 25 .. 31 idle along (the butterfly stays inside 8 lanes)
    double s_px = 0.0, s_py = 0.0, s_mx = 0.0, s_my = 0.0;
    if (band < kBands) {
        // clamped into the spectrum and into the weights, whatever the tables hold
        int f0 = band_first[band], w0 = band_offset[band], cnt = band_offset[band + 1] - w0;
        f0 = f0 < 0 ? 0 : (f0 > H ? H : f0);
        w0 = w0 < 0 ? 0 : (w0 > n_weights ? n_weights : w0);
        cnt = cnt < 0 ? 0 : cnt;
        cnt = cnt > H - f0 ? H - f0 : cnt;
        cnt = cnt > n_weights - w0 ? n_weights - w0 : cnt;
        for (int j = l; j < cnt; j += 8) {
            const double gw = band_weights[w0 + j];
            const double2 p = buf[f0 + j];
            s_px = fma(p.x, gw, s_px);
            s_py = fma(p.y, gw, s_py);
            if (ok) {
                s_mx = fma(sqrt(p.x) / tx, gw, s_mx);
                s_my = fma(sqrt(p.y) / ty, gw, s_my);
            }
        }
    }
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) {
        s_px += __shfl_xor(s_px, o, 64);
        s_py += __shfl_xor(s_py, o, 64);
        s_mx += __shfl_xor(s_mx, o, 64);
        s_my += __shfl_xor(s_my, o, 64);
    }
    if (band < kBands && l == 0) {
        ex[band] = 10.0 * log10(s_px > kFloor ? s_px : kFloor);
        ey[band] = 10.0 * log10(s_py > kFloor ? s_py : kFloor);
        double w = 0.0, term = 0.0;
        if (ok) {
            const double d = s_mx - s_my, err = d * d > kEps ? d * d : kEps;
            w = pow(s_mx, 0.2);
            term = w * (10.0 * log10(s_mx * s_mx / err));
        }
        fw_w[band] = w;
        fw_t[band] = term;
    }
    __syncthreads();
    if (t < kBands - 1) {
        double max_x = ex[0], max_y = ey[0];
        for (int i = 1; i < kBands; ++i) {
            max_x = ex[i] > max_x ? ex[i] : max_x;
            max_y = ey[i] > max_y ? ey[i] : max_y;
        }
        const double wx = (20.0 / (20.0 + max_x - ex[t])) * (1.0 / (1.0 + nearest_peak(ex, t) - ex[t]));
        const double wy = (20.0 / (20.0 + max_y - ey[t])) * (1.0 / (1.0 + nearest_peak(ey, t) - ey[t]));
        const double W = 0.5 * (wx + wy), d = (ex[t + 1] - ex[t]) - (ey[t + 1] - ey[t]);
        ws_w[t] = W;
        ws_t[t] = W * (d * d);
    }
    __syncthreads();
    if (t == 0) {
        double num = 0.0, den = 0.0;
        for (int i = 0; i < kBands - 1; ++i) {
            num += ws_t[i];
            den += ws_w[i];
        }
        vals[g] = num / den;
        double fnum = 0.0, fden = 0.0;
        for (int i = 0; i < kBands; ++i) {
            fnum += fw_t[i];
            fden += fw_w[i];
        }
        vals[Fcap + g] = ok ? clampd(fnum / fden, -10.0, 35.0) : 0.0;
        valid[g] = ok ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void spectral_recording_kernel(const long* __restrict__ fbase, long Fcap,
                                                                 const double* __restrict__ vals, const int* __restrict__ valid,
                                                                 float* __restrict__ out_wss, float* __restrict__ out_fwssnr) {
    __shared__ double red[256];
    __shared__ unsigned long long red4[4];
    const long b = blockIdx.x;
    const int t = threadIdx.x;
    const long fb = fbase[b], F = fbase[b + 1] - fb;         // fb + F <= Fcap
    const float nan = __builtin_nanf("");
    if (F <= 0) {                                            // uniform over the workgroup
        if (t == 0) {
            out_wss[b] = nan;
            out_fwssnr[b] = nan;
        }
        return;
    }
    const double* __restrict__ fw = vals + Fcap + fb;
    const int* __restrict__ ok = valid + fb;
    double s = 0.0;
    unsigned long long cnt = 0;
    for (long i = t; i < F; i += 256) {
        if (!ok[i]) continue;
        s += fw[i];
        cnt += 1;
    }
    s = block_sum(s, red);
    const long V = (long)block_sum_ull(cnt, red4);
    if (t == 0) out_fwssnr[b] = V > 0 ? (float)(s / (double)V) : nan;
    const long K0 = (19 * F + 10) / 20;                      // floor(0.95 F + 0.5), exactly
    double mean[1];                                          // of the K smallest WSS values (plane 0), valid or not
    trimmed_means<1, false>(vals + fb, Fcap, nullptr, F, K0 > 1 ? K0 : 1, red, red4, mean);
    if (t == 0) out_wss[b] = (float)mean[0];
}

template <int LOG>
void launch_frames(const FrameLayout& s, hipStream_t st, const float* clean, const float* est, const long* offsets, int n, long total,
                   const double* window, const FrameGeometry& g, const int* band_first, const int* band_offset,
                   const double* band_weights, int n_weights, const double* twiddles) {
    DCS_LAUNCH(spectral_frame_kernel<LOG>, dim3((unsigned)s.Fcap), dim3(kThreads), sizeof(double2) << LOG, st, clean, est, offsets,
               n, total, s.fbase, window, g.N, g.S, band_first, band_offset, band_weights, n_weights,
               reinterpret_cast<const double2*>(twiddles), s.Fcap, s.vals, s.valid);
}

}  // namespace

extern "C" long dcs_spectral_measures_ragged_workspace_bytes(int n, long total, int fs) {
    return frame_workspace_bytes(n, total, fs, 2);
}

extern "C" int dcs_spectral_measures_ragged_f32(const float* clean, const float* est, const long* offsets, int n, long total, int fs,
                                                const double* window, int window_len, const int* band_first,
                                                const int* band_offset, const double* band_weights, int band_weights_len,
                                                const double* twiddles, int twiddles_len, float* out_wss, float* out_fwssnr,
                                                void* workspace, long workspace_bytes, dcs_stream_t stream) {
    if (bad_rate(fs) || !band_first || !band_offset || !band_weights || !twiddles || !out_wss || !out_fwssnr) return DCS_ERR_BADARG;
    const int log = log_nfft(frame_geometry(fs).N);
    if (twiddles_len != (1 << log) || band_weights_len < 0) return DCS_ERR_BADARG;
    FrameGeometry g;
    FrameLayout s;
    hipStream_t st;
    const int rc = frame_slots_begin(clean, est, offsets, n, total, fs, window, window_len, 2, workspace, workspace_bytes, stream,
                                     &g, &s, &st);
    if (rc != DCS_OK) return rc;
    if (s.Fcap > 0) {
        switch (log) {
            case 9: launch_frames<9>(s, st, clean, est, offsets, n, total, window, g, band_first, band_offset, band_weights,
                                     band_weights_len, twiddles); break;
            case 10: launch_frames<10>(s, st, clean, est, offsets, n, total, window, g, band_first, band_offset, band_weights,
                                       band_weights_len, twiddles); break;
            case 11: launch_frames<11>(s, st, clean, est, offsets, n, total, window, g, band_first, band_offset, band_weights,
                                       band_weights_len, twiddles); break;
            default: launch_frames<12>(s, st, clean, est, offsets, n, total, window, g, band_first, band_offset, band_weights,
                                       band_weights_len, twiddles); break;
        }
        DCS_CHECK_LAUNCH();
    }
    DCS_LAUNCH(spectral_recording_kernel, dim3(n), dim3(256), 0, st, s.fbase, s.Fcap, s.vals, s.valid, out_wss, out_fwssnr);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}
