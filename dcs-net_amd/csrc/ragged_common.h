// ragged_common.h — what the kernels of the project's ragged convention share (stoi_ragged.hip, frame_measures.hip): one flat
// float buffer + int64 offsets[n + 1] on the device, recording i = [offsets[i], offsets[i + 1]).  Every per-recording size is
// taken from rec_span (offsets clamped into the buffer) or from the differences of a ragged_prefix_kernel table (clamped to the
// capacity the host sized the buffers for), so no value in offsets[] makes a kernel leave its buffers.
#pragma once
#include "dcs_common.h"

namespace dcs_ragged {

constexpr int kMaxRecordings = 32767;                        // 2 n workgroup rows of the STOI band kernel's grid
constexpr long kMaxTotal = 1L << 40;

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

inline bool bad_ragged(const long* offsets, int n, long total) {
    return !offsets || n <= 0 || n > kMaxRecordings || total < 0 || total > kMaxTotal;
}

}  // namespace dcs_ragged
