// stoi_ragged.hip — scoring whole recordings of different lengths on the device: the kernels of stoi.hip for the project's ragged
// convention (one flat float buffer + int64 offsets[n + 1] on the device, recording i = [offsets[i], offsets[i + 1])), and the
// reference's SiSNR (network_functions.py:30-42) per recording.  What stoi.hip's kernels do to one row, these do to one
// recording, through the same device functions (stoi_common.h): a recording's score is bit-equal to dcs_stoi_f32 with B = 1.
//
//   ragged_prefix_kernel          (ragged_common.h) one workgroup: out[i] = sum over j < i of v_j, v_j = the resampled length ceil(L_j up / down) or the
//                                   frame count of recording j, clamped to the capacity the host sized the buffers for — the
//                                   later kernels take every per-recording size from the differences of this table, so no
//                                   value in offsets[] makes them write outside their buffers
//   resample_poly_ragged_kernel   resample_poly_kernel, one thread per output sample of the flat output; a thread finds its
//                                   recording by owner() of the output offsets (as resample_sinc_kernel does); taps stop at the
//                                   recording's own ends
//   stoi_keep_ragged_kernel       one workgroup per recording: stoi_keep_kernel on its samples and frame slots
//   stoi_bands_ragged_kernel      grid (frames of the LONGEST recording / 4, 2 n): stoi_bands_kernel; workgroups past a recording's
//                                   kept frames exit
//   stoi_score_ragged_kernel      one workgroup per recording: stoi_score_kernel
//   stoi_score_ext_ragged_kernel  one workgroup per recording, in its place in dcs_stoi_ext_ragged_f32: stoi_score_ext_kernel (STOI
//                                   and / or ESTOI, whichever is asked for, from the same band envelopes)
//   sisnr_ragged_kernel           one workgroup per recording, two passes over its samples, every sum in fp64: thread t adds the
//                                   elements t, t + 256, ... in ascending order, then a fixed LDS tree
//
// Workspace of dcs_stoi_ragged_f32: frame base long[n + 1] | energies double[Fcap] | kept frame indices int[Fcap] | band
// envelopes float[2][Fcap][15], Fcap = total / 128 >= the frames of all recordings together (a recording of L > 256 samples
// has ceil((L - 256) / 128) <= L / 128 - 1 frames): recording i owns the slots [base_i, base_{i + 1}) of each array, so the
// allocation follows the total length, not n x the longest.
//
// Grids are sized from host integers (n, total, the longest recording); everything per recording is read from the offsets on the
// device.  No atomics, no cross-workgroup synchronisation, no host read-back: capturable, bit-reproducible.
#include "ragged_common.h"
#include "stoi_common.h"

namespace {

using namespace dcs_stoi;
using namespace dcs_ragged;                                  // owner, rec_span, ragged_prefix_kernel, block_sum, bad_ragged

constexpr int kMaxRatio = 1 << 16;                           // up, down: total * up and n_out * down stay inside int64
constexpr double kSisnrEps = 1e-8;                           // SiSNR.__call__'s default, network_functions.py:31

struct PrefixResample {                                       // v = ceil(L up / down)
    long up, down;
    __device__ __forceinline__ long operator()(long L) const { return (L * up + down - 1) / down; }
};
struct PrefixFrames {                                         // v = STOI frames of the first max_len samples
    long max_len;
    __device__ __forceinline__ long operator()(long L) const { return stoi_frames(L < max_len ? L : max_len); }
};

// x float[total] (ragged) -> y float[y_off[n]] (ragged); y_off from ragged_prefix_kernel<PrefixResample>
__global__ __launch_bounds__(256) void resample_poly_ragged_kernel(const float* __restrict__ x, const long* __restrict__ offsets, int n,
                                                                   long total, float* __restrict__ y, const long* __restrict__ y_off,
                                                                   const float* __restrict__ h, int taps, int up, int down) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= y_off[n]) return;
    const int lo = owner(y_off, n, g);
    long first;
    const long L = rec_span(offsets, lo, total, &first);
    y[g] = resample_poly_sample(x + first, L, g - y_off[lo], h, taps, up, down);
}

__global__ __launch_bounds__(256) void stoi_keep_ragged_kernel(const float* __restrict__ clean, const long* __restrict__ offsets,
                                                               long total, const long* __restrict__ fbase, double* __restrict__ e_ws,
                                                               int* __restrict__ idx_ws, int* __restrict__ kept) {
    __shared__ double win[kFrame];
    __shared__ double red[256];
    __shared__ int wave_cnt[4];
    const long b = blockIdx.x;
    const long fb = fbase[b], F = fbase[b + 1] - fb;
    if (F <= 0) {                                            // at most one frame's worth of samples: nothing to keep
        if (threadIdx.x == 0) kept[b] = 0;
        return;
    }
    long first;
    rec_span(offsets, b, total, &first);
    const int running = keep_frames(clean + first, F, e_ws + fb, idx_ws + fb, win, red, wave_cnt);
    if (threadIdx.x == 0) kept[b] = running;
}

// band float[2][Fcap][15]: recording b's rows of signal sig start at (sig Fcap + fbase[b]) * 15
__global__ __launch_bounds__(256) void stoi_bands_ragged_kernel(const float* __restrict__ clean, const float* __restrict__ est,
                                                                const long* __restrict__ offsets, long total,
                                                                const long* __restrict__ fbase, long Fcap,
                                                                const int* __restrict__ idx_ws, const int* __restrict__ kept,
                                                                const int* __restrict__ band_lo, const int* __restrict__ band_hi,
                                                                float* __restrict__ band_ws) {
    const long b = blockIdx.y >> 1;
    const int sig = blockIdx.y & 1;
    const int K = kept[b];
    const long Mb = K > 0 ? K - 1 : 0;
    const long m0 = (long)blockIdx.x * kFramesPerWg;
    if (m0 >= Mb) return;                                    // uniform over the workgroup
    long first;
    rec_span(offsets, b, total, &first);
    const long fb = fbase[b];
    band_frames((sig ? est : clean) + first, idx_ws + fb, Mb, m0, band_lo, band_hi, band_ws + (sig * Fcap + fb) * kBands);
}

__global__ __launch_bounds__(256) void stoi_score_ragged_kernel(const float* __restrict__ band_ws, const long* __restrict__ fbase,
                                                                long Fcap, const int* __restrict__ kept, float* __restrict__ out_d) {
    __shared__ double red[256];
    const long b = blockIdx.x;
    const float* X = band_ws + fbase[b] * kBands;
    score_frames(X, X + Fcap * kBands, kept[b], red, out_d + b);
}

// out_d / out_e: null = not asked for (not both)
__global__ __launch_bounds__(256) void stoi_score_ext_ragged_kernel(const float* __restrict__ band_ws, const long* __restrict__ fbase,
                                                                    long Fcap, const int* __restrict__ kept, float* __restrict__ out_d,
                                                                    float* __restrict__ out_e) {
    __shared__ double red[256];
    const long b = blockIdx.x;
    const float* X = band_ws + fbase[b] * kBands;
    score_frames_both(X, X + Fcap * kBands, kept[b], red, out_d ? out_d + b : nullptr, out_e ? out_e + b : nullptr);
}

// SiSNR.__call__ per recording, without its batch mean: dot = <est, clean>, norm = <clean, clean>, s_target = dot clean /
// (norm + eps), e_noise = est - s_target (per element), out = 10 log10(|s_target|^2 / (|e_noise|^2 + eps) + eps)
__global__ __launch_bounds__(256) void sisnr_ragged_kernel(const float* __restrict__ clean, const float* __restrict__ est,
                                                           const long* __restrict__ offsets, long total, float* __restrict__ out) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    long first;
    const long L = rec_span(offsets, blockIdx.x, total, &first);
    const float* c = clean + first;
    const float* e = est + first;
    double dot = 0.0, norm = 0.0;
    for (long i = t; i < L; i += 256) {
        const double cv = c[i], ev = e[i];
        dot = fma(ev, cv, dot);
        norm = fma(cv, cv, norm);
    }
    dot = block_sum(dot, red);
    norm = block_sum(norm, red);
    const double den = norm + kSisnrEps;
    double tn = 0.0, nn = 0.0;
    for (long i = t; i < L; i += 256) {
        const double st = (dot * (double)c[i]) / den;
        const double en = (double)e[i] - st;
        tn = fma(st, st, tn);
        nn = fma(en, en, nn);
    }
    tn = block_sum(tn, red);
    nn = block_sum(nn, red);
    if (t == 0) out[blockIdx.x] = (float)(10.0 * log10(tn / (nn + kSisnrEps) + kSisnrEps));
}

struct RaggedLayout {
    long Fcap, off_e, off_idx, off_band, bytes;
};

inline RaggedLayout ragged_layout(long n, long total) {
    RaggedLayout s;
    s.Fcap = total / kHop;
    s.off_e = align256((n + 1) * (long)sizeof(long));
    s.off_idx = s.off_e + align256(s.Fcap * (long)sizeof(double));
    s.off_band = s.off_idx + align256(s.Fcap * (long)sizeof(int));
    s.bytes = s.off_band + align256(2 * s.Fcap * kBands * (long)sizeof(float));
    return s;
}

inline bool bad_stoi_ragged(const float* clean10, const float* est10, const long* offsets, int n, long total10, long longest10,
                            const int* band_lo, const int* band_hi, const int* out_kept, const void* workspace) {
    return bad_ragged(offsets, n, total10) || longest10 < 0 || longest10 > (1L << 31) || !band_lo || !band_hi || !out_kept ||
           !workspace || (total10 > 0 && (!clean10 || !est10));
}

// the prefix, keep and band launches of both entry points, arguments checked by the caller: -> out_kept, the frame bases and
// the band envelopes in ws
int launch_prefix_keep_bands(const float* clean10, const float* est10, const long* offsets, int n, long total10, long longest10,
                             const int* band_lo, const int* band_hi, int* out_kept, const RaggedLayout& s, char* ws, hipStream_t st) {
    long* fbase = reinterpret_cast<long*>(ws);
    double* e_ws = reinterpret_cast<double*>(ws + s.off_e);
    int* idx_ws = reinterpret_cast<int*>(ws + s.off_idx);
    float* band_ws = reinterpret_cast<float*>(ws + s.off_band);
    DCS_LAUNCH(ragged_prefix_kernel<PrefixFrames>, dim3(1), dim3(256), 0, st, offsets, n, total10, PrefixFrames{longest10}, s.Fcap,
               fbase);
    DCS_CHECK_LAUNCH();
    DCS_LAUNCH(stoi_keep_ragged_kernel, dim3(n), dim3(256), 0, st, clean10, offsets, total10, fbase, e_ws, idx_ws, out_kept);
    DCS_CHECK_LAUNCH();
    const long Mmax = stoi_frames(longest10 < total10 ? longest10 : total10) - 1;      // STFT frames of the longest recording
    if (Mmax > 0) {
        DCS_LAUNCH(stoi_bands_ragged_kernel, dim3((unsigned)((Mmax + kFramesPerWg - 1) / kFramesPerWg), 2 * n), dim3(256), 0, st, clean10,
                   est10, offsets, total10, fbase, s.Fcap, idx_ws, out_kept, band_lo, band_hi, band_ws);
        DCS_CHECK_LAUNCH();
    }
    return DCS_OK;
}

}  // namespace

extern "C" int dcs_resample_poly_ragged_f32(const float* x, const long* offsets, int n, long total, float* y, long* out_offsets,
                                            long out_capacity, const float* h, int taps, int up, int down, dcs_stream_t stream) {
    if (bad_ragged(offsets, n, total) || !out_offsets || !h || taps <= 0 || !(taps & 1) || up <= 0 || up > kMaxRatio ||
        down <= 0 || down > kMaxRatio || out_capacity < 0 || out_capacity > kMaxTotal || (total > 0 && !x) || (out_capacity > 0 && !y))
        return DCS_ERR_BADARG;
    hipStream_t st = dcs_stream(stream);
    DCS_LAUNCH(ragged_prefix_kernel<PrefixResample>, dim3(1), dim3(256), 0, st, offsets, n, total, PrefixResample{up, down},
               out_capacity, out_offsets);
    DCS_CHECK_LAUNCH();
    if (out_capacity > 0) {
        DCS_LAUNCH(resample_poly_ragged_kernel, dim3((unsigned)((out_capacity + 255) / 256)), dim3(256), 0, st, x, offsets, n, total, y,
                   out_offsets, h, taps, up, down);
        DCS_CHECK_LAUNCH();
    }
    return DCS_OK;
}

extern "C" long dcs_stoi_ragged_workspace_bytes(int n, long total10) {
    if (n <= 0 || n > kMaxRecordings || total10 < 0 || total10 > kMaxTotal) return DCS_ERR_BADARG;
    return ragged_layout(n, total10).bytes;
}

extern "C" int dcs_stoi_ragged_f32(const float* clean10, const float* est10, const long* offsets, int n, long total10,
                                   long longest10, const int* band_lo, const int* band_hi, float* out_d, int* out_kept,
                                   void* workspace, long workspace_bytes, dcs_stream_t stream) {
    if (bad_stoi_ragged(clean10, est10, offsets, n, total10, longest10, band_lo, band_hi, out_kept, workspace) || !out_d)
        return DCS_ERR_BADARG;
    const RaggedLayout s = ragged_layout(n, total10);
    if (workspace_bytes < s.bytes) return DCS_ERR_WORKSPACE;
    char* ws = static_cast<char*>(workspace);
    hipStream_t st = dcs_stream(stream);
    const int rc = launch_prefix_keep_bands(clean10, est10, offsets, n, total10, longest10, band_lo, band_hi, out_kept, s, ws, st);
    if (rc != DCS_OK) return rc;
    DCS_LAUNCH(stoi_score_ragged_kernel, dim3(n), dim3(256), 0, st, reinterpret_cast<const float*>(ws + s.off_band),
               reinterpret_cast<const long*>(ws), s.Fcap, out_kept, out_d);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}

extern "C" int dcs_stoi_ext_ragged_f32(const float* clean10, const float* est10, const long* offsets, int n, long total10,
                                       long longest10, const int* band_lo, const int* band_hi, float* out_d, float* out_e,
                                       int* out_kept, void* workspace, long workspace_bytes, dcs_stream_t stream) {
    if (bad_stoi_ragged(clean10, est10, offsets, n, total10, longest10, band_lo, band_hi, out_kept, workspace) || (!out_d && !out_e))
        return DCS_ERR_BADARG;
    const RaggedLayout s = ragged_layout(n, total10);
    if (workspace_bytes < s.bytes) return DCS_ERR_WORKSPACE;
    char* ws = static_cast<char*>(workspace);
    hipStream_t st = dcs_stream(stream);
    const int rc = launch_prefix_keep_bands(clean10, est10, offsets, n, total10, longest10, band_lo, band_hi, out_kept, s, ws, st);
    if (rc != DCS_OK) return rc;
    DCS_LAUNCH(stoi_score_ext_ragged_kernel, dim3(n), dim3(256), 0, st, reinterpret_cast<const float*>(ws + s.off_band),
               reinterpret_cast<const long*>(ws), s.Fcap, out_kept, out_d, out_e);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}

extern "C" int dcs_sisnr_ragged_f32(const float* clean, const float* est, const long* offsets, int n, long total, float* out,
                                    dcs_stream_t stream) {
    if (bad_ragged(offsets, n, total) || !out || (total > 0 && (!clean || !est))) return DCS_ERR_BADARG;
    DCS_LAUNCH(sisnr_ragged_kernel, dim3(n), dim3(256), 0, dcs_stream(stream), clean, est, offsets, total, out);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}
