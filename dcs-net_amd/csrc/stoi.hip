// stoi.hip — STOI of a whole batch on the device: dcsnet/metrics.py::stoi (the published algorithm with pystoi 0.3.3's
// constants) restated for B utterances of one length, in the host function's order.  The reference scores every validation /
// test utterance on the CPU (network_functions.py:152-166: .cpu().numpy() per utterance); here one call per batch, no host
// read-back, no sync inside, so the op can be captured in a graph.
//
//   resample_poly_kernel  the Octave-style polyphase resampler (metrics.resample_oct) in closed form, one thread per output:
//                           y[n] = up * sum_k h[k] x[(n down + half - k) / up],  over the k where n down + half - k is a
//                           multiple of up and the index lies in [0, L);  half = (taps - 1) / 2
//   stoi_keep_kernel      one workgroup per utterance: the clean frames' energies 20 log10(|w x_f| + eps) in fp64 (a keep
//                           decision that flips between fp64 and fp32 changes the frame count), their maximum, the strict keep
//                           test (max - 40 - e) < 0 and the compaction of the kept frame indices (ballot + wave prefix)
//   stoi_bands_kernel     one wavefront per (utterance, signal, STFT frame): frame m of the overlap-added kept frames, read on the
//                           fly (kept frame m - 1's second half + kept frame m + kept frame m + 1's first half), Hann window,
//                           zero-pad to 512, real FFT (fft512_common.h), |X|^2 summed over the 15 bands [lo, hi), sqrt
//   stoi_score_kernel     one workgroup per utterance: the 30-frame segments (normalise, clip, remove the mean, correlate) in
//                           fp64 and their mean; exactly 1e-5 when fewer than 30 STFT frames remain
//   stoi_score_ext_kernel one workgroup per utterance, in place of stoi_score_kernel in dcs_stoi_ext_f32: that score and / or the
//                           extended one (ESTOI: each segment normalised by rows, then by columns, in fp64; thread t takes the
//                           segments t, t + 256, ...), whichever the caller asked for, from the same band envelopes
//
// Grids are sized from (B, L) alone; every kernel reads the device-side kept count and exits where there is no work.  No float
// atomics, no cross-workgroup synchronisation: every reduction has a fixed order, results are bit-reproducible.
// The stages themselves are device functions of stoi_common.h, shared with the ragged form of these kernels (stoi_ragged.hip).
#include "stoi_common.h"

namespace {

using namespace dcs_stoi;                                    // constants and the per-recording stages: stoi_common.h

struct StoiLayout {
    long F, Mmax, off_idx, off_band, bytes;
};

// workspace: energies double[B][F] | kept frame indices int[B][F] | band envelopes float[B][2][Mmax][15]
inline StoiLayout stoi_layout(long B, long L) {
    StoiLayout s;
    s.F = stoi_frames(L);
    s.Mmax = s.F > 0 ? s.F - 1 : 0;
    s.off_idx = align256(B * s.F * (long)sizeof(double));
    s.off_band = s.off_idx + align256(B * s.F * (long)sizeof(int));
    s.bytes = s.off_band + align256(B * 2 * s.Mmax * kBands * (long)sizeof(float));
    if (s.bytes < 256) s.bytes = 256;
    return s;
}

// x float[rows][L] -> y float[rows][n_out]
__global__ __launch_bounds__(256) void resample_poly_kernel(const float* __restrict__ x, float* __restrict__ y, long L, long n_out,
                                                            const float* __restrict__ h, int taps, int up, int down) {
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= n_out) return;
    y[(long)blockIdx.y * n_out + n] = resample_poly_sample(x + (long)blockIdx.y * L, L, n, h, taps, up, down);
}

// clean float[B][L] -> e double[B][F] (scratch), idx int[B][F] (kept frame indices, ascending), kept int[B]
__global__ __launch_bounds__(256) void stoi_keep_kernel(const float* __restrict__ clean, long L, long F, double* __restrict__ e_ws,
                                                        int* __restrict__ idx_ws, int* __restrict__ kept) {
    __shared__ double win[kFrame];
    __shared__ double red[256];
    __shared__ int wave_cnt[4];
    const long b = blockIdx.x;
    const int running = keep_frames(clean + b * L, F, e_ws + b * F, idx_ws + b * F, win, red, wave_cnt);
    if (threadIdx.x == 0) kept[b] = running;
}

// -> band float[B][2][Mmax][15]: sqrt of the band sums of |rfft512(hann * frame m)|^2 for m < kept[b] - 1
__global__ __launch_bounds__(256) void stoi_bands_kernel(const float* __restrict__ clean, const float* __restrict__ est, long L, long F,
                                                         long Mmax, const int* __restrict__ idx_ws, const int* __restrict__ kept,
                                                         const int* __restrict__ band_lo, const int* __restrict__ band_hi,
                                                         float* __restrict__ band_ws) {
    const long b = blockIdx.y >> 1;
    const int sig = blockIdx.y & 1;
    const int K = kept[b];
    const long Mb = K > 0 ? K - 1 : 0;
    const long m0 = (long)blockIdx.x * kFramesPerWg;
    if (m0 >= Mb) return;                                    // uniform over the workgroup
    band_frames((sig ? est : clean) + b * L, idx_ws + b * F, Mb, m0, band_lo, band_hi, band_ws + (b * 2 + sig) * Mmax * kBands);
}

__global__ __launch_bounds__(256) void stoi_score_kernel(const float* __restrict__ band_ws, const int* __restrict__ kept, long Mmax,
                                                         float* __restrict__ out_d) {
    __shared__ double red[256];
    const long b = blockIdx.x;
    const float* X = band_ws + (b * 2) * Mmax * kBands;
    score_frames(X, X + Mmax * kBands, kept[b], red, out_d + b);
}

// out_d / out_e: null = not asked for (not both)
__global__ __launch_bounds__(256) void stoi_score_ext_kernel(const float* __restrict__ band_ws, const int* __restrict__ kept, long Mmax,
                                                             float* __restrict__ out_d, float* __restrict__ out_e) {
    __shared__ double red[256];
    const long b = blockIdx.x;
    const float* X = band_ws + (b * 2) * Mmax * kBands;
    score_frames_both(X, X + Mmax * kBands, kept[b], red, out_d ? out_d + b : nullptr, out_e ? out_e + b : nullptr);
}

// the keep and band launches of both entry points, arguments checked by the caller: -> out_kept, the band envelopes in ws
int launch_keep_bands(const float* clean10, const float* est10, int B, long L10, const int* band_lo, const int* band_hi,
                      int* out_kept, const StoiLayout& s, char* ws, hipStream_t st) {
    double* e_ws = reinterpret_cast<double*>(ws);
    int* idx_ws = reinterpret_cast<int*>(ws + s.off_idx);
    float* band_ws = reinterpret_cast<float*>(ws + s.off_band);
    DCS_LAUNCH(stoi_keep_kernel, dim3(B), dim3(256), 0, st, clean10, L10, s.F, e_ws, idx_ws, out_kept);
    DCS_CHECK_LAUNCH();
    if (s.Mmax > 0) {
        DCS_LAUNCH(stoi_bands_kernel, dim3((unsigned)((s.Mmax + kFramesPerWg - 1) / kFramesPerWg), 2 * B), dim3(256), 0, st, clean10,
                   est10, L10, s.F, s.Mmax, idx_ws, out_kept, band_lo, band_hi, band_ws);
        DCS_CHECK_LAUNCH();
    }
    return DCS_OK;
}

inline bool bad_stoi(const float* clean10, const float* est10, int B, long L10, const int* band_lo, const int* band_hi,
                     const int* out_kept, const void* workspace) {
    return B <= 0 || B > 32767 || L10 < 0 || L10 > (1L << 31) || !band_lo || !band_hi || !out_kept || !workspace ||
           (L10 > 0 && (!clean10 || !est10));
}

}  // namespace

extern "C" int dcs_resample_poly_f32(const float* x, float* y, int rows, long L, const float* h, int taps, int up, int down,
                                     dcs_stream_t stream) {
    if (!x || !y || !h || rows <= 0 || rows > 65535 || L <= 0 || L > (1L << 40) || taps <= 0 || !(taps & 1) || up <= 0 ||
        down <= 0)
        return DCS_ERR_BADARG;
    const long n_out = (L * up + down - 1) / down;
    const long blocks = (n_out + 255) / 256;
    if (blocks > (1L << 31) - 1) return DCS_ERR_BADARG;
    DCS_LAUNCH(resample_poly_kernel, dim3((unsigned)blocks, (unsigned)rows), dim3(256), 0, dcs_stream(stream), x, y, L, n_out, h, taps,
               up, down);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}

extern "C" long dcs_stoi_workspace_bytes(int B, long L10) {
    if (B <= 0 || B > 32767 || L10 < 0 || L10 > (1L << 31)) return DCS_ERR_BADARG;
    return stoi_layout(B, L10).bytes;
}

extern "C" int dcs_stoi_f32(const float* clean10, const float* est10, int B, long L10, const int* band_lo, const int* band_hi,
                            float* out_d, int* out_kept, void* workspace, long workspace_bytes, dcs_stream_t stream) {
    if (bad_stoi(clean10, est10, B, L10, band_lo, band_hi, out_kept, workspace) || !out_d) return DCS_ERR_BADARG;
    const StoiLayout s = stoi_layout(B, L10);
    if (workspace_bytes < s.bytes) return DCS_ERR_WORKSPACE;
    char* ws = static_cast<char*>(workspace);
    hipStream_t st = dcs_stream(stream);
    const int rc = launch_keep_bands(clean10, est10, B, L10, band_lo, band_hi, out_kept, s, ws, st);
    if (rc != DCS_OK) return rc;
    DCS_LAUNCH(stoi_score_kernel, dim3(B), dim3(256), 0, st, reinterpret_cast<const float*>(ws + s.off_band), out_kept, s.Mmax, out_d);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}

extern "C" int dcs_stoi_ext_f32(const float* clean10, const float* est10, int B, long L10, const int* band_lo, const int* band_hi,
                                float* out_d, float* out_e, int* out_kept, void* workspace, long workspace_bytes,
                                dcs_stream_t stream) {
    if (bad_stoi(clean10, est10, B, L10, band_lo, band_hi, out_kept, workspace) || (!out_d && !out_e)) return DCS_ERR_BADARG;
    const StoiLayout s = stoi_layout(B, L10);
    if (workspace_bytes < s.bytes) return DCS_ERR_WORKSPACE;
    char* ws = static_cast<char*>(workspace);
    hipStream_t st = dcs_stream(stream);
    const int rc = launch_keep_bands(clean10, est10, B, L10, band_lo, band_hi, out_kept, s, ws, st);
    if (rc != DCS_OK) return rc;
    DCS_LAUNCH(stoi_score_ext_kernel, dim3(B), dim3(256), 0, st, reinterpret_cast<const float*>(ws + s.off_band), out_kept, s.Mmax,
               out_d, out_e);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}
