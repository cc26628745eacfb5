// validation.hip — the books of a validation epoch on the device (dcsnet/validation.py): one launch per batch folds that batch's
// losses and per-utterance scores into a small fp64 state by the reference's rule (validation_step's NaN skip, c_network.py:298-300;
// calc_metric's NaN filter with max(len, 1), network_functions.py:152-166; _epoch_end's mean of batch metrics), so the epoch
// ends with ONE host read.  One workgroup of 256 threads: the work is B <= a few thousand floats, and launches on one stream are
// ordered, so thread 0's read-modify-write of `state` needs no atomic.  Sums in fp64 through dcs_ragged::block_sum: a fixed order,
// bit-reproducible.  State layout: DCS_VAL_* of include/dcsnet_hip.h.
#include "ragged_common.h"

namespace {
constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void val_accumulate_kernel(const float* __restrict__ losses, int n_loss,
                                                                  const float* __restrict__ scores, int n_scores, int B,
                                                                  double* __restrict__ state) {
    __shared__ double red[kThreads];
    const int t = threadIdx.x;
    const float monitored = losses[n_loss - 1];
    if (monitored != monitored) {                                // NaN only: +-Inf is kept (uniform over the workgroup)
        if (t == 0) state[DCS_VAL_SKIPPED] += 1.0;
        return;
    }
    for (int r = 0; r < n_scores; ++r) {
        const float* row = scores + (long)r * B;
        double s = 0.0, c = 0.0;
        for (int i = t; i < B; i += kThreads) {
            const float v = row[i];
            if (v == v) {
                s += (double)v;
                c += 1.0;
            }
        }
        s = dcs_ragged::block_sum(s, red);
        c = dcs_ragged::block_sum(c, red);                      // (integers below 2^53: exact)
        if (t == 0) {
            state[DCS_VAL_SCORE_SUM + r] += s / (c > 1.0 ? c : 1.0);
            state[DCS_VAL_SCORE_NAN + r] += (double)B - c;
        }
    }
    if (t == 0) {
        state[DCS_VAL_KEPT] += 1.0;
        for (int k = 0; k < n_loss; ++k) state[DCS_VAL_LOSS_SUM + k] += (double)losses[k];
    }
}
}  // namespace

extern "C" int dcs_val_accumulate_f32(const float* losses, int n_loss, const float* scores, int n_scores, int B, double* state,
                                      dcs_stream_t stream) {
    if (!losses || !state || (n_loss != 1 && n_loss != 3) || n_scores < 0 || n_scores > DCS_VAL_MAX_SCORES || B < 1)
        return DCS_ERR_BADARG;
    if (n_scores > 0 && !scores) return DCS_ERR_BADARG;
    hipStream_t st = dcs_stream(stream);
    DCS_LAUNCH(val_accumulate_kernel, dim3(1), dim3(kThreads), 0, st, losses, n_loss, scores, n_scores, B, state);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}
