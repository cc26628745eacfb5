// frame_measures.hip — the three frame-based objective measures of Hu & Loizou that are defined by formulae alone (segmental
// SNR, the LPC log-likelihood ratio, the LPC cepstrum distance) of whole recordings of different lengths, for the project's
// ragged convention (ragged_common.h: one flat float buffer + int64 offsets[n + 1] on the device).  The host function
// dcsnet/metrics.py::frame_measures is the numerics contract; everything here is fp64 until the three float32 outputs.
//
// Framing, workspace (3 value planes) and the prefix launch are ragged_frames.h's; the window double[N] comes from the host
// (metrics._measure_window: the same bits as the host function's).  LPC order P = 16 for fs >= 10000, else 10.  This source
// owns the LPC recursion, the cepstrum and the Toeplitz forms, and:
//
//   frame_measures_kernel<P>                    one wave64 per frame slot g < fbase[n] (grid Fcap, from the host integer
//                                                 total; frame_slot finds its samples): both windowed
//                                                 frames into LDS (2 N doubles), the two energies and the 2 (P + 1)
//                                                 autocorrelation lags with the samples split over the 64 lanes (lane t adds
//                                                 t, t + 64, ... in ascending order, then a fixed butterfly), the two
//                                                 Levinson-Durbin recursions and cepstra on lanes 0 and 1 (registers, unrolled),
//                                                 the two quadratic forms on lane 0 -> vals[0..2][g] = the frame's segmental
//                                                 SNR (clamped to [-10, 35] dB), LLR (clamped to [0, 2]), CD (clamped to
//                                                 [0, 10]); valid[g] = both recursions kept R[0] > 0 and every E_i > 0
//   recording_measures_kernel                   one workgroup per recording, any number of frames: the SSNR mean over all F
//                                                 frames; for LLR and CD the mean of the K smallest valid values
//                                                 (K = max(1, floor(0.95 V + 0.5)), V valid frames) by trimmed_means<2, true>;
//                                                 NaN for all three without a frame, for LLR and CD without a valid one
//
// Three launches whatever n is (two when total < S).  No atomics, no cross-workgroup synchronisation, no host read-back:
// capturable, bit-reproducible, and a recording's scores do not depend on its neighbours.
#include "ragged_frames.h"

namespace {

using namespace dcs_ragged;

constexpr int kMaxOrder = 16;
constexpr double kEps = 2.220446049250313e-16;                // np.finfo(np.float64).eps

inline int lpc_order(int fs) { return fs >= 10000 ? kMaxOrder : 10; }

// the published lpcoeff on R[0 .. P]: A[0 .. P] = [1, -a], c[1 .. P] the LPC cepstrum of A; returns R[0] > 0 and every E_i > 0
template <int P>
__device__ __forceinline__ bool lpc_cepstrum(const double* __restrict__ R, double* __restrict__ A_out, double* __restrict__ c_out) {
    double r[P + 1], a[P], prev[P], c[P + 1], A[P + 1];
#pragma unroll
    for (int i = 0; i <= P; ++i) r[i] = R[i];
#pragma unroll
    for (int i = 0; i < P; ++i) a[i] = 0.0;
    double E = r[0];
    bool ok = E > 0.0;
#pragma unroll
    for (int i = 0; i < P; ++i) {
#pragma unroll
        for (int j = 0; j < P; ++j) prev[j] = a[j];
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < i; ++j) s = fma(prev[j], r[i - j], s);
        const double k = (r[i + 1] - s) / E;
        a[i] = k;
#pragma unroll
        for (int j = 0; j < i; ++j) a[j] = prev[j] - k * prev[i - 1 - j];
        E = (1.0 - k * k) * E;
        ok = ok && E > 0.0;
    }
    A[0] = 1.0;
#pragma unroll
    for (int i = 0; i < P; ++i) A[i + 1] = -a[i];
    c[0] = 0.0;
    c[1] = -A[1];
#pragma unroll
    for (int k = 2; k <= P; ++k) {
        double s = 0.0;
#pragma unroll
        for (int i = 1; i < k; ++i) s = fma((double)i * c[i], A[k - i], s);
        c[k] = -(A[k] + s / (double)k);
    }
#pragma unroll
    for (int i = 0; i <= P; ++i) {
        A_out[i] = A[i];
        c_out[i] = c[i];
    }
    return ok;
}

// A T A^T, T the Toeplitz matrix of R[0 .. P]
template <int P>
__device__ __forceinline__ double toeplitz_form(const double* __restrict__ A, const double* __restrict__ R) {
    double q = 0.0;
#pragma unroll
    for (int i = 0; i <= P; ++i) {
        double row = 0.0;
#pragma unroll
        for (int j = 0; j <= P; ++j) row = fma(A[j], R[i > j ? i - j : j - i], row);
        q = fma(A[i], row, q);
    }
    return q;
}

// dynamic LDS: double[2 N], the windowed clean frame and the windowed estimate
template <int P>
__global__ __launch_bounds__(64) void frame_measures_kernel(const float* __restrict__ clean, const float* __restrict__ est,
                                                            const long* __restrict__ offsets, int n, long total,
                                                            const long* __restrict__ fbase, const double* __restrict__ window,
                                                            int N, int S, long Fcap, double* __restrict__ vals,
                                                            int* __restrict__ valid) {
    extern __shared__ double frames[];
    __shared__ double R[2][P + 1], A[2][P + 1], C[2][P + 1];
    __shared__ int ok[2];
    const long g = blockIdx.x;
    long base;
    if (!frame_slot(offsets, n, total, fbase, g, S, &base)) return;
    const float* __restrict__ c = clean + base;
    const float* __restrict__ e = est + base;
    double* fx = frames;
    double* fy = frames + N;
    const int t = threadIdx.x;
    double se = 0.0, ne = 0.0;
    for (int i = t; i < N; i += 64) {
        const double w = window[i];
        const double a = w * (double)c[i], b = w * (double)e[i], d = a - b;
        fx[i] = a;
        fy[i] = b;
        se = fma(a, a, se);
        ne = fma(d, d, ne);
    }
    se = dcs_wave_sum_d(se);
    ne = dcs_wave_sum_d(ne);
    __syncthreads();
    for (int k = 0; k <= P; ++k) {
        double ax = 0.0, ay = 0.0;
        for (int i = t; i < N - k; i += 64) {
            ax = fma(fx[i], fx[i + k], ax);
            ay = fma(fy[i], fy[i + k], ay);
        }
        ax = dcs_wave_sum_d(ax);
        ay = dcs_wave_sum_d(ay);
        if (t == 0) {
            R[0][k] = ax;
            R[1][k] = ay;
        }
    }
    __syncthreads();
    if (t < 2) ok[t] = lpc_cepstrum<P>(R[t], A[t], C[t]) ? 1 : 0;
    __syncthreads();
    if (t == 0) {
        const double snr = 10.0 * log10(se / (ne + kEps) + kEps);
        const bool v = ok[0] && ok[1];
        double llr = 0.0, cd = 0.0;
        if (v) {
            llr = clampd(log(toeplitz_form<P>(A[1], R[0]) / toeplitz_form<P>(A[0], R[0])), 0.0, 2.0);
            double s = 0.0;
#pragma unroll
            for (int k = 1; k <= P; ++k) {
                const double d = C[0][k] - C[1][k];
                s = fma(d, d, s);
            }
            cd = clampd(4.342944819032518 * sqrt(2.0 * s), 0.0, 10.0);      // 10 / ln 10
        }
        vals[g] = clampd(snr, -10.0, 35.0);
        vals[Fcap + g] = llr;
        vals[2 * Fcap + g] = cd;
        valid[g] = v ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void recording_measures_kernel(const long* __restrict__ fbase, long Fcap,
                                                                 const double* __restrict__ vals, const int* __restrict__ valid,
                                                                 float* __restrict__ out_ssnr, float* __restrict__ out_llr,
                                                                 float* __restrict__ out_cd) {
    __shared__ double red[256];
    __shared__ unsigned long long red4[4];
    const long b = blockIdx.x;
    const int t = threadIdx.x;
    const long fb = fbase[b], F = fbase[b + 1] - fb;         // fb + F <= Fcap
    const float nan = __builtin_nanf("");
    if (F <= 0) {                                            // uniform over the workgroup
        if (t == 0) {
            out_ssnr[b] = nan;
            out_llr[b] = nan;
            out_cd[b] = nan;
        }
        return;
    }
    const double* __restrict__ snr = vals + fb;
    const int* __restrict__ ok = valid + fb;
    double s = 0.0;
    unsigned long long cnt = 0;
    for (long i = t; i < F; i += 256) {
        s += snr[i];
        cnt += ok[i] ? 1 : 0;
    }
    s = block_sum(s, red);
    const long V = (long)block_sum_ull(cnt, red4);
    if (t == 0) out_ssnr[b] = (float)(s / (double)F);
    if (V == 0) {                                            // uniform over the workgroup
        if (t == 0) {
            out_llr[b] = nan;
            out_cd[b] = nan;
        }
        return;
    }
    const long K0 = (19 * V + 10) / 20;                      // floor(0.95 V + 0.5), exactly
    double mean[2];                                          // of the K smallest valid LLR (plane 1) and CD (plane 2) values
    trimmed_means<2, true>(vals + Fcap + fb, Fcap, ok, F, K0 > 1 ? K0 : 1, red, red4, mean);
    if (t == 0) {
        out_llr[b] = (float)mean[0];
        out_cd[b] = (float)mean[1];
    }
}

}  // namespace

extern "C" long dcs_frame_measures_ragged_workspace_bytes(int n, long total, int fs) {
    return frame_workspace_bytes(n, total, fs, 3);
}

extern "C" int dcs_frame_measures_ragged_f32(const float* clean, const float* est, const long* offsets, int n, long total, int fs,
                                             const double* window, int window_len, float* out_ssnr, float* out_llr, float* out_cd,
                                             void* workspace, long workspace_bytes, dcs_stream_t stream) {
    if (!out_ssnr || !out_llr || !out_cd) return DCS_ERR_BADARG;
    FrameGeometry g;
    FrameLayout s;
    hipStream_t st;
    const int rc = frame_slots_begin(clean, est, offsets, n, total, fs, window, window_len, 3, workspace, workspace_bytes, stream,
                                     &g, &s, &st);
    if (rc != DCS_OK) return rc;
    if (s.Fcap > 0) {
        const size_t lds = 2 * (size_t)g.N * sizeof(double);
        if (lpc_order(fs) == kMaxOrder)
            DCS_LAUNCH(frame_measures_kernel<16>, dim3((unsigned)s.Fcap), dim3(64), lds, st, clean, est, offsets, n, total, s.fbase,
                       window, g.N, g.S, s.Fcap, s.vals, s.valid);
        else
            DCS_LAUNCH(frame_measures_kernel<10>, dim3((unsigned)s.Fcap), dim3(64), lds, st, clean, est, offsets, n, total, s.fbase,
                       window, g.N, g.S, s.Fcap, s.vals, s.valid);
        DCS_CHECK_LAUNCH();
    }
    DCS_LAUNCH(recording_measures_kernel, dim3(n), dim3(256), 0, st, s.fbase, s.Fcap, s.vals, s.valid, out_ssnr, out_llr, out_cd);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}
