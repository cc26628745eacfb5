// ragged_common.h — what the kernels of the project's ragged convention share: one flat float buffer + int64 offsets[n + 1] on
// the device, recording i = [offsets[i], offsets[i + 1]).  Included by stoi_ragged.hip, frame_measures.hip and
// spectral_measures.hip (the latter two through ragged_frames.h), speech_level.hip, audio_mix.hip, validation.hip, and for
// owner() alone by audio_store.hip, enhance.hip and snapshot.hip; stoi_common.h takes align256 from here.
// Every per-recording size is taken from rec_span (offsets clamped into the buffer) or from the differences of a
// ragged_prefix_kernel table (clamped to the capacity the host sized the buffers for), so no value in offsets[] makes a kernel
// leave its buffers.
#pragma once
#include "dcs_common.h"

namespace dcs_ragged {

constexpr int kMaxRecordings = 32767;                        // 2 n workgroup rows of the STOI band kernel's grid
constexpr long kMaxTotal = 1L << 40;
constexpr unsigned long long kMagnitude = 0x7fffffffffffffffull;

inline long align256(long n) { return (n + 255) & ~255L; }  // workspace sections of the ragged / STOI family

__device__ __forceinline__ double clampd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the bit pattern of |v|: for doubles without NaN, bit order = numeric order of the magnitudes (-0.0 orders as 0.0)
__device__ __forceinline__ unsigned long long magnitude_bits(double v) {
    return (unsigned long long)__double_as_longlong(v) & kMagnitude;
}

// Which item owns flat position g: the LAST i in [0, n) with table[i] <= g, by bisection of the rising prefix table
// table[n + 1] (item i = [table[i], table[i + 1])).  Precondition: table[0] <= g < table[n], which the caller tests (or which
// its grid guarantees) before the call.  An item of length zero (table[i] == table[i + 1]) never owns a position: the last
// entry at or before g is then a later one.  Whatever the table holds the result lies in [0, n); a caller that reads an
// untrusted table guards what it derives from g - table[i].
__device__ __forceinline__ int owner(const long* __restrict__ table, int n, long g) {
    int lo = 0, hi = n;                                      // table[lo] <= g < table[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (table[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// recording i of offsets[n + 1], clamped into the buffer [0, total): first sample and length (0 for offsets that do not rise)
__device__ __forceinline__ long rec_span(const long* __restrict__ offsets, long i, long total, long* first) {
    long a = offsets[i], b = offsets[i + 1];
    a = a < 0 ? 0 : (a > total ? total : a);
    b = b < 0 ? 0 : (b > total ? total : b);
    *first = a;
    return b > a ? b - a : 0;
}

// out long[n + 1]: the exclusive prefix sums of v(L_i), each clamped to cap (integers: the order of the additions is immaterial)
template <typename V>
__global__ __launch_bounds__(256) void ragged_prefix_kernel(const long* __restrict__ offsets, int n, long total, V v, long cap,
                                                            long* __restrict__ out) {
    __shared__ long scan[256];
    const int t = threadIdx.x;
    const int chunk = (n + 255) / 256;
    const int a = min(t * chunk, n), b = min(a + chunk, n);
    long first, s = 0;
    for (int i = a; i < b; ++i) s += v(rec_span(offsets, i, total, &first));
    scan[t] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const long add = t >= off ? scan[t - off] : 0;
        __syncthreads();
        scan[t] += add;
        __syncthreads();
    }
    long run = scan[t] - s;
    for (int i = a; i < b; ++i) {
        out[i] = run < cap ? run : cap;
        run += v(rec_span(offsets, i, total, &first));
    }
    if (t == 255) out[n] = scan[255] < cap ? scan[255] : cap;
}

// every thread of a 256-thread workgroup returns the sum of v over it; additions in a fixed order (red: LDS double[256])
__device__ __forceinline__ double block_sum(double v, double* red) {
    const int t = threadIdx.x;
    __syncthreads();                                         // red may still be read from the previous sum
    red[t] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    return red[0];
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

inline bool bad_ragged(const long* offsets, int n, long total) {
    return !offsets || n <= 0 || n > kMaxRecordings || total < 0 || total > kMaxTotal;
}

}  // namespace dcs_ragged
