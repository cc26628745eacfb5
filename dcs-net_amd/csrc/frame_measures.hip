// frame_measures.hip — the three frame-based objective measures of Hu & Loizou that are defined by formulae alone (segmental
// SNR, the LPC log-likelihood ratio, the LPC cepstrum distance) of whole recordings of different lengths, for the project's
// ragged convention (ragged_common.h: one flat float buffer + int64 offsets[n + 1] on the device).  The host function
// dcsnet/metrics.py::frame_measures is the numerics contract; everything here is fp64 until the three float32 outputs.
//
// Framing at rate fs: N = round(0.03 fs) samples, hop S = N / 4, F = (L - N) / S frames for L >= N + S (else 0), frame k at
// k S, window double[N] from the host (metrics._measure_window: the same bits as the host function's).  LPC order P = 16 for
// fs >= 10000, else 10.
//
//   ragged_prefix_kernel<PrefixMeasureFrames>   one workgroup: fbase[i] = the frames of the recordings before i, clamped to
//                                                 Fcap = total / S >= the frames of all recordings together
//   frame_measures_kernel<P>                    one wave64 per frame slot g < fbase[n] (grid Fcap, from the host integer
//                                                 total; the workgroup finds its recording by bisection of fbase): both windowed
//                                                 frames into LDS (2 N doubles), the two energies and the 2 (P + 1)
//                                                 autocorrelation lags with the samples split over the 64 lanes (lane t adds
//                                                 t, t + 64, ... in ascending order, then a fixed butterfly), the two
//                                                 Levinson-Durbin recursions and cepstra on lanes 0 and 1 (registers, unrolled),
//                                                 the two quadratic forms on lane 0 -> vals[0..2][g] = the frame's segmental
//                                                 SNR (clamped to [-10, 35] dB), LLR (clamped to [0, 2]), CD (clamped to
//                                                 [0, 10]); valid[g] = both recursions kept R[0] > 0 and every E_i > 0
//   recording_measures_kernel                   one workgroup per recording, any number of frames: the SSNR mean; for LLR and
//                                                 CD the K-th smallest valid value t (K = max(1, floor(0.95 V + 0.5)), V valid
//                                                 frames) by binary radix selection on the bit patterns (non-negative doubles:
//                                                 bit order = numeric order; one pass per bit, both measures in one pass,
//                                                 counts by a fixed integer reduction), then (sum of the v < t + (K - #{v < t})
//                                                 t) / K, the sum over the frame slots in a fixed order: no sort, ties handled
//
// Workspace: frame base long[n + 1] | vals double[3][Fcap] | valid int[Fcap]: it follows the total length.
// Three launches whatever n is (two when total < S).  No atomics, no cross-workgroup synchronisation, no host read-back:
// capturable, bit-reproducible, and a recording's scores do not depend on its neighbours.
#include "ragged_common.h"

namespace {

using namespace dcs_ragged;

constexpr int kMinRate = 8000, kMaxRate = 48000;
constexpr int kMaxOrder = 16;
constexpr double kEps = 2.220446049250313e-16;                // np.finfo(np.float64).eps
constexpr unsigned long long kMagnitude = 0x7fffffffffffffffull;

struct Geometry {
    int N, S, P;
};
inline Geometry geometry(int fs) {
    Geometry g;
    g.N = (3 * fs + 50) / 100;                                // round(0.03 fs)
    g.S = g.N / 4;
    g.P = fs >= 10000 ? 16 : 10;
    return g;
}
inline bool bad_rate(int fs) { return fs < kMinRate || fs > kMaxRate; }
inline long align256(long n) { return (n + 255) & ~255L; }

struct PrefixMeasureFrames {                                  // v = (L - N) / S for L >= N + S
    long N, S;
    __device__ __forceinline__ long operator()(long L) const { return L >= N + S ? (L - N) / S : 0; }
};

struct Layout {
    long Fcap, off_vals, off_valid, bytes;
};
inline Layout layout(long n, long total, const Geometry& g) {
    Layout s;
    s.Fcap = total / g.S;
    s.off_vals = align256((n + 1) * (long)sizeof(long));
    s.off_valid = s.off_vals + align256(3 * s.Fcap * (long)sizeof(double));
    s.bytes = s.off_valid + align256(s.Fcap * (long)sizeof(int));
    return s;
}

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

__device__ __forceinline__ double clampd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

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
    if (g >= fbase[n]) return;                               // uniform over the workgroup; fbase[n] <= Fcap
    int lo = 0, hi = n;                                      // fbase[lo] <= g < fbase[hi]: the LAST recording that starts at or before g
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (fbase[mid] <= g) lo = mid; else hi = mid;
    }
    long first;
    rec_span(offsets, lo, total, &first);
    // frame k = g - fbase[lo] < fbase[lo + 1] - fbase[lo] <= (L - N) / S: its samples end before the recording's
    const long base = first + (g - fbase[lo]) * S;
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

// every thread of a 256-thread workgroup returns the sum of v over it (integers; red: LDS [4])
__device__ __forceinline__ unsigned long long block_sum_ull(unsigned long long v, unsigned long long* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();                                         // red may still be read from the previous sum
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ unsigned long long magnitude_bits(double v) {
    return (unsigned long long)__double_as_longlong(v) & kMagnitude;       // -0.0 orders as 0.0
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
    const double* __restrict__ llr = vals + Fcap + fb;
    const double* __restrict__ cd = vals + 2 * Fcap + fb;
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
    const long K = K0 > 1 ? K0 : 1;
    // the K-th smallest valid value of each measure, one bit per pass from the top: among the values that share the bits
    // found so far, count those whose next bit is 0 (LLR's count in the low word, CD's in the high word: F < 2^31)
    unsigned long long pl = 0, pc = 0;
    long kl = K, kc = K;
    for (int bit = 62; bit >= 0; --bit) {
        unsigned long long c0 = 0;
        for (long i = t; i < F; i += 256) {
            if (!ok[i]) continue;
            const unsigned long long ul = magnitude_bits(llr[i]), uc = magnitude_bits(cd[i]);
            if ((ul >> bit) == (pl >> bit)) c0 += 1ull;      // the bits above `bit` agree and bit `bit` is 0 (pl's still is)
            if ((uc >> bit) == (pc >> bit)) c0 += 1ull << 32;
        }
        c0 = block_sum_ull(c0, red4);
        const long zl = (long)(c0 & 0xffffffffull), zc = (long)(c0 >> 32);
        if (kl > zl) {
            kl -= zl;
            pl |= 1ull << bit;
        }
        if (kc > zc) {
            kc -= zc;
            pc |= 1ull << bit;
        }
    }
    double sl = 0.0, sc = 0.0;
    unsigned long long below = 0;
    for (long i = t; i < F; i += 256) {
        if (!ok[i]) continue;
        const double vl = llr[i], vc = cd[i];
        if (magnitude_bits(vl) < pl) {
            sl += vl;
            below += 1ull;
        }
        if (magnitude_bits(vc) < pc) {
            sc += vc;
            below += 1ull << 32;
        }
    }
    sl = block_sum(sl, red);
    sc = block_sum(sc, red);
    below = block_sum_ull(below, red4);
    if (t == 0) {
        const double tl = __longlong_as_double((long long)pl), tc = __longlong_as_double((long long)pc);
        out_llr[b] = (float)((sl + (double)(K - (long)(below & 0xffffffffull)) * tl) / (double)K);
        out_cd[b] = (float)((sc + (double)(K - (long)(below >> 32)) * tc) / (double)K);
    }
}

}  // namespace

extern "C" long dcs_frame_measures_ragged_workspace_bytes(int n, long total, int fs) {
    if (n <= 0 || n > kMaxRecordings || total < 0 || total > kMaxTotal || bad_rate(fs)) return DCS_ERR_BADARG;
    const Layout s = layout(n, total, geometry(fs));
    if (s.Fcap > 0x7fffffffL) return DCS_ERR_BADARG;          // one workgroup per frame slot
    return s.bytes;
}

extern "C" int dcs_frame_measures_ragged_f32(const float* clean, const float* est, const long* offsets, int n, long total, int fs,
                                             const double* window, int window_len, float* out_ssnr, float* out_llr, float* out_cd,
                                             void* workspace, long workspace_bytes, dcs_stream_t stream) {
    if (bad_ragged(offsets, n, total) || bad_rate(fs) || !window || !out_ssnr || !out_llr || !out_cd || !workspace ||
        (total > 0 && (!clean || !est)))
        return DCS_ERR_BADARG;
    const Geometry g = geometry(fs);
    const Layout s = layout(n, total, g);
    if (window_len != g.N || s.Fcap > 0x7fffffffL) return DCS_ERR_BADARG;
    if (workspace_bytes < s.bytes) return DCS_ERR_WORKSPACE;
    char* ws = static_cast<char*>(workspace);
    long* fbase = reinterpret_cast<long*>(ws);
    double* vals = reinterpret_cast<double*>(ws + s.off_vals);
    int* valid = reinterpret_cast<int*>(ws + s.off_valid);
    hipStream_t st = dcs_stream(stream);
    DCS_LAUNCH(ragged_prefix_kernel<PrefixMeasureFrames>, dim3(1), dim3(256), 0, st, offsets, n, total,
               PrefixMeasureFrames{g.N, g.S}, s.Fcap, fbase);
    DCS_CHECK_LAUNCH();
    if (s.Fcap > 0) {
        const size_t lds = 2 * (size_t)g.N * sizeof(double);
        if (g.P == kMaxOrder)
            DCS_LAUNCH(frame_measures_kernel<16>, dim3((unsigned)s.Fcap), dim3(64), lds, st, clean, est, offsets, n, total, fbase,
                       window, g.N, g.S, s.Fcap, vals, valid);
        else
            DCS_LAUNCH(frame_measures_kernel<10>, dim3((unsigned)s.Fcap), dim3(64), lds, st, clean, est, offsets, n, total, fbase,
                       window, g.N, g.S, s.Fcap, vals, valid);
        DCS_CHECK_LAUNCH();
    }
    DCS_LAUNCH(recording_measures_kernel, dim3(n), dim3(256), 0, st, fbase, s.Fcap, vals, valid, out_ssnr, out_llr, out_cd);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}
