// sdr_ragged.hip — the signal-to-distortion ratio of BSS-eval (bss_eval_sources for one source: the estimate projected onto
// the span of K <= 512 delayed copies of the reference) of whole recordings of different lengths, for the project's ragged
// convention (ragged_common.h: flat float buffers + int64 offsets[n + 1] on the device).  The host function
// dcsnet/metrics.py::sdr is the numerics contract; everything here is fp64 until the float32 output.  One or two estimates
// are scored against the same reference in one call (the second shares R and the forward recursion).
//
// Chunks.  A recording of L > 0 samples is cut, from its OWN first sample, into chunks of kChunk = 2048 positions
// t = 0 .. L + K - 2 (the projection is K - 1 samples longer than the recording): nch(L) = ceil((L + K - 1) / kChunk) of
// them, of which the first ceil(L / kChunk) hold samples.  Recording i owns the chunk slots from
// slot0(i) = first_i / kChunk + 2 i on (first_i from rec_span); nch(L) <= L / kChunk + 2 keeps the recordings' slots apart, and
// every slot lies below Ccap = total / kChunk + 2 n, the grid of the two chunk kernels and the capacity of the two partial
// tables.  slot0 rises with i, so owner_by() finds a slot's recording from the offsets alone: there is no table launch.  A slot
// that no recording uses ends its workgroup at once.  Whatever offsets[] holds, the slots derived from it are tested against
// nch(L) and Ccap, and every sample index against L from rec_span: no kernel leaves its buffers.
//
//   sdr_corr_kernel<NS>      one workgroup of 256 per slot that holds samples: the chunk and its 512-sample halo of the NS (2 or
//                              3) signals as doubles into LDS, de-interleaved by position mod 8 (8 planes: lane g reads plane p
//                              at index base + g, free of bank conflicts); lane g of wave w owns the 8 lags 8 g .. 8 g + 7 over
//                              the w-th quarter of the chunk: per 8 positions 8 x 8 FMAs per signal on a sliding 16-value
//                              window (8 new LDS reads); the 4 quarters are added in a fixed order ->
//                              part[slot][s][k] = sum_{t in chunk} x[t] sig_s[t + k] (R, D, D2)
//   sdr_solve_kernel<T>      one workgroup of T = 64 per recording: the chunks' partials added in ascending order, then the
//                              Levinson recursion of metrics.sdr with element i of a / c / c2 on lane i % 64, slot i / 64:
//                              one reduction per step for the three dot products (the delta sums do not depend on
//                              kappa; DPP butterflies, no LDS crossbar), the reversed vector through a double-buffered LDS
//                              copy, a'_{m - i} recomputed from the pair (a_i, a_{m - i}) a lane already holds ->
//                              c[rec][e][K], ok[rec] (every E_m > 0 and finite)
//   sdr_project_kernel<NE>   one workgroup of 256 per used slot: thread q forms s[t], t = 8 q .. 8 q + 7 of the chunk, over all
//                              K taps with the same planes and window (x once for both estimates), then the chunk's
//                              sum s^2 and sum (y_pad - s)^2 over t < L + K - 1 by block_sum -> pen[slot][e][2]
//   sdr_finish_kernel        one wave per recording: the chunks' energies in a fixed order, the NaN / inf rules, 10 log10, float
//
// Four launches whatever n is.  No atomics, no cross-workgroup synchronisation, no host read-back: capturable,
// bit-reproducible, and a recording's value does not depend on the other recordings of the call (its chunks, partial sums and
// recursion see its own samples only, in an order fixed by its own length).
#include "ragged_common.h"

#ifndef DCS_SDR_SOLVE_THREADS
#define DCS_SDR_SOLVE_THREADS 64                              // 256: the block_sum variant it was measured against
#endif

namespace {

using namespace dcs_ragged;

constexpr int kMaxTaps = 512;
constexpr int kChunk = 2048;                                  // dcsnet/ops.py::SDR_CHUNK
constexpr int kHalo = 512;                                    // >= kMaxTaps - 1, a multiple of 8
constexpr int kPlane = (kChunk + kHalo) / 8;                  // 320 doubles per plane
constexpr int kSolveThreads = DCS_SDR_SOLVE_THREADS;
static_assert(kSolveThreads == 64 || kSolveThreads == 256, "one wave, or block_sum's 256");

inline bool bad_taps(int K) { return K < 1 || K > kMaxTaps; }

struct SdrLayout {
    long Ccap, off_c, off_ok, off_pen, bytes;
    double *part, *c, *pen;                                   // set by carve()
    int* ok;
    void carve(void* workspace) {
        char* ws = static_cast<char*>(workspace);
        part = reinterpret_cast<double*>(ws);
        c = reinterpret_cast<double*>(ws + off_c);
        ok = reinterpret_cast<int*>(ws + off_ok);
        pen = reinterpret_cast<double*>(ws + off_pen);
    }
};
// part double[Ccap][3][K] | c double[n][2][K] | ok int[n] | pen double[Ccap][2][2]
inline SdrLayout layout(long n, long total, int K) {
    SdrLayout s{};
    s.Ccap = total / kChunk + 2 * n;
    s.off_c = align256(s.Ccap * 3 * K * (long)sizeof(double));
    s.off_ok = s.off_c + align256(n * 2 * K * (long)sizeof(double));
    s.off_pen = s.off_ok + align256(n * (long)sizeof(int));
    s.bytes = s.off_pen + align256(s.Ccap * 4 * (long)sizeof(double));
    return s;
}

__device__ __forceinline__ long chunks_of(long L, int K) { return L > 0 ? (L + K - 1 + kChunk - 1) / kChunk : 0; }

// owner() of ragged_common.h over a rising function at(i) of the index instead of a stored table: the last i in [0, n) with
// at(i) <= g (the same bisection, the same precondition at(0) <= g < at(n), the same guard duty of the caller)
template <typename At>
__device__ __forceinline__ int owner_by(At at, int n, long g) {
    int lo = 0, hi = n;                                      // at(lo) <= g < at(hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (at(mid) <= g) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ long slot0(const long* __restrict__ offsets, int i, long total) {
    long first;
    rec_span(offsets, i, total, &first);
    return first / kChunk + 2L * i;
}

// slot g -> false when no recording uses it (uniform over the workgroup); else its recording, that recording's first sample
// and length, and the chunk's first position t0 < L + K - 1 in the recording
__device__ __forceinline__ bool chunk_slot(const long* __restrict__ offsets, int n, long total, int K, long g, int* rec,
                                           long* first, long* L, long* t0) {
    const int r = owner_by([offsets, total](int i) { return slot0(offsets, i, total); }, n, g);
    *L = rec_span(offsets, r, total, first);
    const long j = g - (*first / kChunk + 2L * r);
    if (j < 0 || j >= chunks_of(*L, K)) return false;
    *rec = r;
    *t0 = j * kChunk;
    return true;
}

// a recording's first slot and how many of them hold partials (`used` of chunks_of), both kept below Ccap
__device__ __forceinline__ long slots_of(const long* __restrict__ offsets, int rec, long total, long Ccap, long want, long* base) {
    long b = slot0(offsets, rec, total);
    b = b < Ccap ? b : Ccap;
    *base = b;
    return want < Ccap - b ? want : Ccap - b;
}

// positions t0 - lead .. t0 - lead + 8 kPlane - 1 of a recording's signal as doubles, zero outside [0, L): p -> planes[p & 7][p >> 3]
__device__ __forceinline__ void fill_planes(double (*planes)[kPlane], const float* __restrict__ src, long L, long t0, int lead) {
    for (int p = threadIdx.x; p < 8 * kPlane; p += 256) {
        const long t = t0 - lead + p;
        planes[p & 7][p >> 3] = (t >= 0 && t < L) ? (double)src[t] : 0.0;
    }
}

template <int NS>
__global__ __launch_bounds__(256) void sdr_corr_kernel(const float* __restrict__ clean, const float* __restrict__ est,
                                                       const float* __restrict__ est2, const long* __restrict__ offsets, int n,
                                                       long total, int K, double* __restrict__ part) {
    __shared__ double sig[NS][8][kPlane];
    const long g = blockIdx.x;
    int rec;
    long first, L, t0;
    if (!chunk_slot(offsets, n, total, K, g, &rec, &first, &L, &t0) || t0 >= L) return;      // the tail chunk holds no sample
    fill_planes(sig[0], clean + first, L, t0, 0);
    fill_planes(sig[1], est + first, L, t0, 0);
    if (NS == 3) fill_planes(sig[NS - 1], est2 + first, L, t0, 0);
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double acc[NS][8];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[s][j] = 0.0;
    if (8 * lane < K) {                                      // lags 8 lane + j; positions 512 w + 8 it + i
        const int xb = 64 * w, base = xb + lane;
        double lo[NS][8], hi[NS][8], xt[8];
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int m = 0; m < 8; ++m) lo[s][m] = sig[s][m][base];
        for (int it = 0; it < 64; ++it) {
#pragma unroll
            for (int s = 0; s < NS; ++s)
#pragma unroll
                for (int m = 0; m < 8; ++m) hi[s][m] = sig[s][m][base + it + 1];
#pragma unroll
            for (int i = 0; i < 8; ++i) xt[i] = sig[0][i][xb + it];
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int s = 0; s < NS; ++s)
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        acc[s][j] = fma(xt[i], i + j < 8 ? lo[s][i + j] : hi[s][i + j - 8], acc[s][j]);
#pragma unroll
            for (int s = 0; s < NS; ++s)
#pragma unroll
                for (int m = 0; m < 8; ++m) lo[s][m] = hi[s][m];
        }
    }
    __syncthreads();
    double* red = &sig[0][0][0];                             // [4][NS][512] <= NS * 8 * kPlane doubles
    if (8 * lane < K) {
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) red[(w * NS + s) * kMaxTaps + 8 * lane + j] = acc[s][j];
    }
    __syncthreads();
    double* __restrict__ out = part + g * 3 * K;             // g < Ccap, the grid
    for (int idx = threadIdx.x; idx < NS * K; idx += 256) {
        const int s = idx / K, k = idx - s * K;
        const double* r = red + s * kMaxTaps + k;
        out[idx] = ((r[0] + r[NS * kMaxTaps]) + r[2 * NS * kMaxTaps]) + r[3 * NS * kMaxTaps];
    }
}

// The sum of v over a wave64 whose 64 lanes are all active, the same bits in every lane: inside each row of 16 lanes four DPP
// butterflies (quad_perm [1,0,3,2] and [2,3,0,1], row_half_mirror, row_mirror: VALU moves, no LDS crossbar), then the four row
// sums read as wave-uniform values and added in a fixed order.  As six __shfl_xor steps (ds_bpermute round trips) the three
// sums of a recursion step were most of the step.
template <int CTRL>
__device__ __forceinline__ double dpp_mov_d(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = dcs_dpp_mov_i<CTRL>((int)b), hi = dcs_dpp_mov_i<CTRL>((int)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
__device__ __forceinline__ double lane_value_d(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, lane), hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
__device__ __forceinline__ double wave_sum_uniform(double v) {
    v += dpp_mov_d<0xB1>(v);
    v += dpp_mov_d<0x4E>(v);
    v += dpp_mov_d<0x141>(v);
    v += dpp_mov_d<0x140>(v);
    return (lane_value_d(v, 0) + lane_value_d(v, 16)) + (lane_value_d(v, 32) + lane_value_d(v, 48));
}

// every thread returns the sums of v[0 .. M) over the workgroup, in a fixed order
template <int T, int M>
__device__ __forceinline__ void solve_sums(double (&v)[M], double* red) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
        if constexpr (T == 64) v[m] = wave_sum_uniform(v[m]);
        else v[m] = block_sum(v[m], red);
    }
}

template <int T, int NE>
__global__ __launch_bounds__(T) void sdr_solve_kernel(const long* __restrict__ offsets, int n, long total, int K, long Ccap,
                                                      const double* __restrict__ part, double* __restrict__ cws,
                                                      int* __restrict__ okws) {
    constexpr int SL = kMaxTaps / T;                         // elements per thread: i = t + T s
    __shared__ double Rl[kMaxTaps], Dl[NE][kMaxTaps], ab[2][kMaxTaps], red[256];
    const int rec = blockIdx.x, t = threadIdx.x;
    long first, base;
    const long L = rec_span(offsets, rec, total, &first);
    const long used = slots_of(offsets, rec, total, Ccap, (L + kChunk - 1) / kChunk, &base);
#pragma unroll
    for (int s = 0; s < SL; ++s) {
        const int k = t + T * s;
        double r = 0.0, d[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) d[e] = 0.0;
        if (k < K) {
            const double* __restrict__ p = part + base * 3 * K + k;
#pragma unroll 4
            for (long ch = 0; ch < used; ++ch, p += 3 * K) {
                r += p[0];
#pragma unroll
                for (int e = 0; e < NE; ++e) d[e] += p[(e + 1) * K];
            }
        }
        Rl[k] = r;
        ab[0][k] = 0.0;
        ab[1][k] = 0.0;
#pragma unroll
        for (int e = 0; e < NE; ++e) Dl[e][k] = d[e];
    }
    __syncthreads();
    double E = Rl[0];
    bool ok = E > 0.0 && E <= 1.79769313486231570e308;
    double a[SL], c[NE][SL];
#pragma unroll
    for (int s = 0; s < SL; ++s) {
        a[s] = 0.0;
#pragma unroll
        for (int e = 0; e < NE; ++e) c[e][s] = 0.0;
    }
    if (ok) {                                                // uniform over the workgroup
        if (t == 0)
#pragma unroll
            for (int e = 0; e < NE; ++e) c[e][0] = Dl[e][0] / E;
        for (int m = 1; m < K; ++m) {
            const double* __restrict__ cur = ab[(m & 1) ^ 1];                // a of step m - 1
            double* __restrict__ nxt = ab[m & 1];
            double ar[SL], sum[1 + NE];
#pragma unroll
            for (int q = 0; q <= NE; ++q) sum[q] = 0.0;
#pragma unroll
            for (int s = 0; s < SL; ++s) {
                const int i = t + T * s;
                ar[s] = 0.0;
                if (T * s < m && i < m) {
                    const double r = Rl[m - i];
                    ar[s] = cur[m - i];                      // a_{m - i}; cur[m] is still 0 for i = 0
                    sum[0] = fma(a[s], r, sum[0]);           // a_0 = 0
#pragma unroll
                    for (int e = 0; e < NE; ++e) sum[1 + e] = fma(c[e][s], r, sum[1 + e]);
                }
            }
            solve_sums<T, 1 + NE>(sum, red);
            const double kappa = (Rl[m] - sum[0]) / E;
            E = E * fma(-kappa, kappa, 1.0);
            ok = ok && E > 0.0 && E <= 1.79769313486231570e308;
            double delta[NE];
#pragma unroll
            for (int e = 0; e < NE; ++e) delta[e] = (Dl[e][m] - sum[1 + e]) / E;
#pragma unroll
            for (int s = 0; s < SL; ++s) {
                const int i = t + T * s;
                if (T * s <= m && i <= m) {
                    const double an = i == m ? kappa : (i == 0 ? 0.0 : fma(-kappa, ar[s], a[s]));      // a'_i
                    const double rev = i == 0 ? kappa : fma(-kappa, a[s], ar[s]);                    // a'_{m - i}, i < m
#pragma unroll
                    for (int e = 0; e < NE; ++e) c[e][s] = i == m ? delta[e] : fma(-delta[e], rev, c[e][s]);
                    a[s] = an;
                    nxt[i] = an;
                }
            }
            __syncthreads();                                 // nxt is the next step's cur (one wave: no s_barrier is issued)
        }
    }
#pragma unroll
    for (int s = 0; s < SL; ++s) {
        const int k = t + T * s;
        if (k < K)
#pragma unroll
            for (int e = 0; e < NE; ++e) cws[((long)rec * 2 + e) * K + k] = ok ? c[e][s] : 0.0;
    }
    if (t == 0) okws[rec] = ok ? 1 : 0;
}

template <int NE>
__global__ __launch_bounds__(256) void sdr_project_kernel(const float* __restrict__ clean, const float* __restrict__ est,
                                                          const float* __restrict__ est2, const long* __restrict__ offsets, int n,
                                                          long total, int K, const double* __restrict__ cws,
                                                          double* __restrict__ pen) {
    __shared__ double X[8][kPlane], cl[NE][kMaxTaps], red[256];
    const long g = blockIdx.x;
    int rec;
    long first, L, t0;
    if (!chunk_slot(offsets, n, total, K, g, &rec, &first, &L, &t0)) return;
    fill_planes(X, clean + first, L, t0, kHalo);             // plane index p = t - t0 + 512
    for (int k = threadIdx.x; k < kMaxTaps; k += 256)
#pragma unroll
        for (int e = 0; e < NE; ++e) cl[e][k] = k < K ? cws[((long)rec * 2 + e) * K + k] : 0.0;
    __syncthreads();
    const int q = threadIdx.x;                               // s[t0 + 8 q + r] = sum_k c[k] x[t0 + 8 q + r - k]
    double acc[NE][8], hi[8], lo[8];
#pragma unroll
    for (int e = 0; e < NE; ++e)
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[e][r] = 0.0;
#pragma unroll
    for (int m = 0; m < 8; ++m) hi[m] = X[m][64 + q];
    const int blocks = (K + 7) / 8;
    for (int kb = 0; kb < blocks; ++kb) {                    // taps 8 kb + kk: p = 8 (64 + q - kb) + (r - kk)
#pragma unroll
        for (int m = 0; m < 8; ++m) lo[m] = X[m][63 + q - kb];
#pragma unroll
        for (int kk = 0; kk < 8; ++kk)
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const double ck = cl[e][8 * kb + kk];
#pragma unroll
                for (int r = 0; r < 8; ++r) acc[e][r] = fma(ck, r >= kk ? hi[r - kk] : lo[8 + r - kk], acc[e][r]);
            }
#pragma unroll
        for (int m = 0; m < 8; ++m) hi[m] = lo[m];
    }
    double num[NE], den[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) num[e] = den[e] = 0.0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const long t = t0 + 8 * q + r;
        if (t < L + K - 1) {
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const float* __restrict__ y = e ? est2 : est;
                const double d = (t < L ? (double)y[first + t] : 0.0) - acc[e][r];
                num[e] = fma(acc[e][r], acc[e][r], num[e]);
                den[e] = fma(d, d, den[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const double a = block_sum(num[e], red), b = block_sum(den[e], red);
        if (threadIdx.x == 0) {
            pen[g * 4 + 2 * e] = a;                          // g < Ccap, the grid
            pen[g * 4 + 2 * e + 1] = b;
        }
    }
}

template <int NE>
__global__ __launch_bounds__(64) void sdr_finish_kernel(const long* __restrict__ offsets, int n, long total, int K, long Ccap,
                                                        const double* __restrict__ pen, const int* __restrict__ okws,
                                                        float* __restrict__ out, float* __restrict__ out2) {
    const int rec = blockIdx.x, t = threadIdx.x;
    long first, base;
    const long L = rec_span(offsets, rec, total, &first);
    const long used = slots_of(offsets, rec, total, Ccap, chunks_of(L, K), &base);
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        double num = 0.0, den = 0.0;
        for (long ch = t; ch < used; ch += 64) {
            num += pen[(base + ch) * 4 + 2 * e];
            den += pen[(base + ch) * 4 + 2 * e + 1];
        }
        num = wave_sum_uniform(num);
        den = wave_sum_uniform(den);
        if (t == 0) {
            const double big = 1.79769313486231570e308;
            float v;
            if (!okws[rec] || !(num <= big) || !(den <= big) || (num == 0.0 && den == 0.0))
                v = __builtin_nanf("");                      // no sample, a silent signal, a value that is not finite, E_m <= 0
            else if (den == 0.0)
                v = __builtin_inff();
            else
                v = (float)(10.0 * log10(num / den));
            (e ? out2 : out)[rec] = v;
        }
    }
}

template <int NE>
int launch(const float* clean, const float* est, const float* est2, const long* offsets, int n, long total, int K, float* out,
           float* out2, const SdrLayout& s, hipStream_t st) {
    constexpr auto solve = sdr_solve_kernel<kSolveThreads, NE>;
    if (total > 0) {                                         // Ccap >= 2
        DCS_LAUNCH(sdr_corr_kernel<NE + 1>, dim3((unsigned)s.Ccap), dim3(256), 0, st, clean, est, est2, offsets, n, total, K, s.part);
        DCS_CHECK_LAUNCH();
    }
    DCS_LAUNCH(solve, dim3(n), dim3(kSolveThreads), 0, st, offsets, n, total, K, s.Ccap, s.part,
               s.c, s.ok);
    DCS_CHECK_LAUNCH();
    if (total > 0) {
        DCS_LAUNCH(sdr_project_kernel<NE>, dim3((unsigned)s.Ccap), dim3(256), 0, st, clean, est, est2, offsets, n, total, K, s.c,
                   s.pen);
        DCS_CHECK_LAUNCH();
    }
    DCS_LAUNCH(sdr_finish_kernel<NE>, dim3(n), dim3(64), 0, st, offsets, n, total, K, s.Ccap, s.pen, s.ok, out, out2);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}

}  // namespace

extern "C" long dcs_sdr_ragged_workspace_bytes(int n, long total, int filter_length) {
    if (n <= 0 || n > kMaxRecordings || total < 0 || total > kMaxTotal || bad_taps(filter_length)) return DCS_ERR_BADARG;
    return layout(n, total, filter_length).bytes;
}

extern "C" int dcs_sdr_ragged_f32(const float* clean, const float* est, const float* est2, const long* offsets, int n, long total,
                                  int filter_length, float* out, float* out2, void* workspace, long workspace_bytes,
                                  dcs_stream_t stream) {
    if (bad_ragged(offsets, n, total) || bad_taps(filter_length) || !out || !workspace || (est2 != nullptr) != (out2 != nullptr) ||
        (total > 0 && (!clean || !est)))
        return DCS_ERR_BADARG;
    SdrLayout s = layout(n, total, filter_length);
    if (workspace_bytes < s.bytes) return DCS_ERR_WORKSPACE;
    s.carve(workspace);
    const hipStream_t st = dcs_stream(stream);
    return est2 ? launch<2>(clean, est, est2, offsets, n, total, filter_length, out, out2, s, st)
                : launch<1>(clean, est, est2, offsets, n, total, filter_length, out, out2, s, st);
}
