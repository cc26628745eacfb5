// speech_level.hip — the ITU-T P.56 (method B) active speech level of every recording of a ragged store, in fp64
// (dcsnet/metrics.py::active_speech_level is the numerics contract; dcsnet/audio_store.py::MixingAudioStore(level='p56')
// is the consumer: measured once per store, beside dcs_signal_power_ragged_f64).
//
//   active_level_ragged_kernel   one workgroup of 256 threads per recording, walking it in tiles of kTile = 256 x kPer samples;
//                                thread t owns the kPer CONSECUTIVE samples [t kPer, (t + 1) kPer) of the tile.
//
// Per tile:
//   1. the envelope q = |x| through y[k] = g y[k - 1] + (1 - g) u[k] twice.  One step maps the state (p, q) by the matrix
//      M = [[g, 0], [(1 - g) g, g]] plus an input term, and M^s = [[g^s, 0], [s (1 - g) g^s, g^s]].  Each thread runs the
//      recurrence over its own samples from zero state (thread 0 from the state the previous tile ended in), the 256 end
//      states are combined by an inclusive scan of the affine maps in LDS (Hillis-Steele: E_t += M^(kPer 2^d) E_(t - 2^d)),
//      and each thread runs its samples again from the state its left neighbour ended in.  That is the exact recurrence up to
//      the association of the scan — no warm-up approximation — and the tile's end state is carried to the next tile.
//   2. the activity counts.  counts[j] is the number of samples k whose window [k - I, k] holds a q >= c[j] = 2^(j - 15), i.e.
//      k - last_j(k) <= I for last_j(k) the LAST sample at or before k that reaches c[j].  The kernel keeps no history of q: it
//      turns q[k] into the number of thresholds it reaches (0 .. 15, from the exponent: the thresholds are powers of two, so
//      the comparison is exact), finds each thread's last such sample per threshold, takes an exclusive max-scan of those
//      positions over the workgroup (wave shuffles, then the four wave totals through LDS) and counts in integers.  The
//      positions are relative to the tile; the 15 positions a tile hands to the next are rebased and saturate at kNone.
//   3. sum(x^2) with fma(v, v, acc), per thread in ascending order, reduced once by ragged_common.h's block_sum.
// At the end the counts are reduced (integers) and thread 0 does the level arithmetic of metrics.p56_level in fp64.
//
// Everything a recording's result depends on is relative to its own first sample, the additions have a fixed order and there
// is no atomic: the same bits on every run, and for a recording alone or among others.  Samples past the recording's end
// enter as zeros after every counted sample and are not counted; rec_span keeps every read inside [0, total).
#include <cmath>
#include "ragged_common.h"

namespace {

using dcs_ragged::rec_span;

constexpr int kPer = 16;                                     // consecutive samples per thread and tile
constexpr int kTile = 256 * kPer;
constexpr int kThresholds = 15;
constexpr int kNone = -(1 << 30);                            // "never reached": further back than any hangover
constexpr int kScanLevels = 8;                               // 256 threads

struct ScanCoef {                                            // M^(kPer 2^d): g^s and s (1 - g) g^s for s = kPer 2^d
    double gs[kScanLevels], cross[kScanLevels];
};

// how many of the thresholds 2^-15 .. 2^-1 the value reaches: 0 for q < 2^-15 (and NaN), else min(exponent + 16, 15)
__device__ __forceinline__ int thresholds_reached(double q) {
    if (!(q >= 0x1p-15)) return 0;
    const int e = (int)((__double_as_longlong(q) >> 52) & 0x7ff) - 1023;
    return e + 16 < kThresholds ? e + 16 : kThresholds;
}

// lv > j ? a : b without a comparison (the 240 selections per pass stay on the vector unit: as compares, their masks
// filled the scalar registers)
__device__ __forceinline__ int select_if_above(int lv, int j, int a, int b) {
    const int m = (j - lv) >> 31;                            // all ones where lv > j
    return (a & m) | (b & ~m);
}

// x float[total], recording i = [offsets[i], offsets[i + 1]) -> out double[n][2], counts long[n][15] (or NULL); grid n
__global__ __launch_bounds__(256) void active_level_ragged_kernel(const float* __restrict__ x, const long* __restrict__ offsets,
                                                                  long total, double g, int hang, ScanCoef coef, double margin_db,
                                                                  double* __restrict__ out, long* __restrict__ counts) {
    __shared__ double red[256];
    __shared__ double2 scan[256];
    __shared__ int wave_last[4][kThresholds];
    __shared__ unsigned long long wave_count[4][kThresholds];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    long first;
    const long len = rec_span(offsets, blockIdx.x, total, &first);
    const double omg = 1.0 - g;

    double acc = 0.0;
    double2 tile_in = make_double2(0.0, 0.0);                // thread 0: the state the previous tile ended in
    int carry[kThresholds];                                  // per threshold: the last reaching sample so far, tile-relative
    unsigned long long cnt[kThresholds];
#pragma unroll
    for (int j = 0; j < kThresholds; ++j) {
        carry[j] = kNone;
        cnt[j] = 0;
    }

    for (long base = 0; base < len; base += kTile) {
        const long k0 = base + (long)t * kPer;
        float a[kPer];
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const float v = k0 + i < len ? x[first + k0 + i] : 0.f;
            acc = fma((double)v, (double)v, acc);
            a[i] = fabsf(v);
        }
        // 1. this thread's end state from zero state (thread 0: from the tile's incoming state), then the scan
        double p = t == 0 ? tile_in.x : 0.0, q = t == 0 ? tile_in.y : 0.0;
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            p = g * p + omg * (double)a[i];
            q = g * q + omg * p;
        }
        scan[t] = make_double2(p, q);
        __syncthreads();
#pragma unroll
        for (int d = 0; d < kScanLevels; ++d) {
            const int off = 1 << d;
            double2 o = make_double2(0.0, 0.0);
            if (t >= off) o = scan[t - off];
            __syncthreads();
            if (t >= off) {
                q = coef.gs[d] * o.y + (coef.cross[d] * o.x + q);
                p = coef.gs[d] * o.x + p;
                scan[t] = make_double2(p, q);
            }
            __syncthreads();
        }
        const double2 in = t == 0 ? tile_in : scan[t - 1];
        if (t == 0) tile_in = scan[255];
        // the samples again from the true incoming state: q[k] -> the number of thresholds it reaches, 4 bits each
        p = in.x;
        q = in.y;
        unsigned long long levels = 0;
        int mine[kThresholds];
#pragma unroll
        for (int j = 0; j < kThresholds; ++j) mine[j] = kNone;
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            p = g * p + omg * (double)a[i];
            q = g * q + omg * p;
            const int lv = thresholds_reached(q);
            levels |= (unsigned long long)lv << (4 * i);
#pragma unroll
            for (int j = 0; j < kThresholds; ++j) mine[j] = select_if_above(lv, j, t * kPer + i, mine[j]);
        }
        // 2. exclusive max-scan of the last reaching positions over the workgroup
        int incl[kThresholds];
#pragma unroll
        for (int j = 0; j < kThresholds; ++j) {
            int v = mine[j];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int u = __shfl_up(v, o, 64);
                if (lane >= o) v = max(v, u);
            }
            incl[j] = v;
            if (lane == 63) wave_last[wave][j] = v;
        }
        __syncthreads();
        int last[kThresholds];
        unsigned tile_cnt[kThresholds];                      // at most kPer per tile
#pragma unroll
        for (int j = 0; j < kThresholds; ++j) {
            tile_cnt[j] = 0;
            const int left = __shfl_up(incl[j], 1, 64);
            int v = carry[j], all = carry[j];
            if (lane > 0) v = max(v, left);
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int wl = wave_last[w][j];
                if (w < wave) v = max(v, wl);
                all = max(all, wl);
            }
            last[j] = v;
            carry[j] = max(all - kTile, kNone);              // rebased to the next tile
        }
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int k = t * kPer + i;
            const int lv = (int)((levels >> (4 * i)) & 15);
            const unsigned inside = k0 + i < len ? 1u : 0u;
#pragma unroll
            for (int j = 0; j < kThresholds; ++j) {
                last[j] = select_if_above(lv, j, k, last[j]);
                tile_cnt[j] += inside & ((unsigned)~(hang - (k - last[j])) >> 31);      // k - last[j] <= hang
            }
        }
#pragma unroll
        for (int j = 0; j < kThresholds; ++j) cnt[j] += tile_cnt[j];
        // the next tile writes scan[] and wave_last[] only after its own barriers, which every thread reaches after these reads
    }

    const double sq = dcs_ragged::block_sum(acc, red);
#pragma unroll
    for (int j = 0; j < kThresholds; ++j) {
        unsigned long long v = cnt[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) wave_count[wave][j] = v;
    }
    __syncthreads();
    if (t != 0) return;
    long a_cnt[kThresholds];
    for (int j = 0; j < kThresholds; ++j) {
        a_cnt[j] = (long)(wave_count[0][j] + wave_count[1][j] + wave_count[2][j] + wave_count[3][j]);
        if (counts) counts[(long)blockIdx.x * kThresholds + j] = a_cnt[j];
    }
    // metrics.p56_level, in its order of operations
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double active = nan, activity = nan;
    if (len > 0 && a_cnt[0] > 0 && isfinite(sq)) {
        double a_prev = 10.0 * log10(sq / (double)a_cnt[0]);
        double d_prev = a_prev - 20.0 * log10(0x1p-15);
        if (!(d_prev < margin_db)) {
            for (int j = 1; j < kThresholds; ++j) {
                if (a_cnt[j] == 0) break;
                const double a_j = 10.0 * log10(sq / (double)a_cnt[j]);
                const double d_j = a_j - 20.0 * log10(ldexp(1.0, j - 15));
                if (d_j <= margin_db) {
                    const double frac = (d_prev - margin_db) / (d_prev - d_j);
                    const double level_db = a_prev + frac * (a_j - a_prev);
                    active = pow(10.0, level_db / 10.0);
                    activity = (sq / (double)len) / active;
                    break;
                }
                a_prev = a_j;
                d_prev = d_j;
            }
        }
    }
    out[2 * (long)blockIdx.x] = active;
    out[2 * (long)blockIdx.x + 1] = activity;
}

}  // namespace

extern "C" int dcs_active_level_ragged_f64(const float* x, const long* offsets, int n, long total, int fs, double margin_db,
                                           double* out, long* counts, dcs_stream_t stream) {
    if (dcs_ragged::bad_ragged(offsets, n, total) || !x || !out || fs < 8000 || fs > 48000) return DCS_ERR_BADARG;
    // (a NULL counts is accepted: the kernel then writes the levels alone)
    const double g = std::exp(-1.0 / ((double)fs * 0.03));
    const int hang = (fs + 4) / 5;                           // ceil(0.2 fs)
    ScanCoef coef;
    double gs = 1.0;
    for (int i = 0; i < kPer; ++i) gs *= g;
    for (int d = 0; d < kScanLevels; ++d) {
        coef.gs[d] = gs;
        coef.cross[d] = (double)(kPer << d) * (1.0 - g) * gs;
        gs *= gs;
    }
    DCS_LAUNCH(active_level_ragged_kernel, dim3((unsigned)n), dim3(256), 0, dcs_stream(stream), x, offsets, total, g, hang, coef,
               margin_db, out, counts);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}
