// swa.hip — the parameter average of stochastic weight averaging (Trainer(stochastic_weight_avg=True), train.py:147;
// config.py:50), i.e. Lightning 1.5.6's StochasticWeightAveraging.update_parameters with its avg_fn, over the flat fp32
// parameter bucket (2.9 M floats):
//     n_averaged == 0:  avg = p
//     otherwise:        avg = avg + (p - avg) / (float)(n_averaged + 1)
// Lightning keeps the average on the CPU and evaluates that expression with torch's fp32 CPU kernels: true division, no
// fused multiply-add.  The kernel does the same operations in the same order (a division, not a reciprocal product), so its
// result is that average bit for bit.  Once per epoch, outside any graph; HBM-bound: two streams in, one out.
#include "dcs_common.h"

namespace {
constexpr int kThreads = 256;

__device__ __forceinline__ float swa_avg(float a, float p, float d, bool first) { return first ? p : a + (p - a) / d; }

__global__ __launch_bounds__(kThreads) void swa_average_kernel(float4* __restrict__ avg, const float4* __restrict__ p, long n4,
                                                                long n, float d, int first) {
    const bool f = first != 0;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (long)gridDim.x * kThreads) {
        float4 a = avg[i];
        const float4 q = p[i];
        a.x = swa_avg(a.x, q.x, d, f);
        a.y = swa_avg(a.y, q.y, d, f);
        a.z = swa_avg(a.z, q.z, d, f);
        a.w = swa_avg(a.w, q.w, d, f);
        avg[i] = a;
    }
    // tail (n not a multiple of 4)
    if (blockIdx.x == 0) {
        float* as = reinterpret_cast<float*>(avg);
        const float* ps = reinterpret_cast<const float*>(p);
        for (long i = n4 * 4 + threadIdx.x; i < n; i += kThreads) as[i] = swa_avg(as[i], ps[i], d, f);
    }
}
}  // namespace

extern "C" int dcs_swa_average_f32(float* avg, const float* p, long n, long n_averaged, dcs_stream_t stream) {
    if (!avg || !p || n <= 0 || n_averaged < 0) return DCS_ERR_BADARG;
    if (((uintptr_t)avg | (uintptr_t)p) & 15) return DCS_ERR_BADARG;
    // torch promotes the long count to the float32 of the tensor: (float)(n + 1), rounded once
    const float d = (float)(n_averaged + 1);
    const long n4 = n / 4;
    long nb = (n4 + kThreads * 2 - 1) / (kThreads * 2);
    const int grid = (int)(nb < 1 ? 1 : (nb > 2048 ? 2048 : nb));
    DCS_LAUNCH(swa_average_kernel, dim3(grid), dim3(kThreads), 0, dcs_stream(stream), (float4*)avg, (const float4*)p, n4, n, d,
               n_averaged == 0 ? 1 : 0);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}
