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
//
// Grids are sized from (B, L) alone; every kernel reads the device-side kept count and exits where there is no work.  No float
// atomics, no cross-workgroup synchronisation: every reduction has a fixed order, results are bit-reproducible.
#include "fft512_common.h"

namespace {

using namespace dcs_fft512;

constexpr int kFrame = 256, kHop = 128, kBands = 15, kSeg = 30, kFramesPerWg = 4;
constexpr double kEps = 2.220446049250313e-16;              // np.finfo(float).eps
constexpr double kDynRange = 40.0;
constexpr double kClip = 5.623413251903491;                 // 10 ** (15 / 20)
constexpr double kPi = 3.141592653589793;

// frames of range(0, L - 256, 128): both framings of the host function
inline long stoi_frames(long L) { return L > kFrame ? (L - kFrame + kHop - 1) / kHop : 0; }

inline long align256(long n) { return (n + 255) & ~255L; }

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

// hanning(258)[1:-1]
__device__ __forceinline__ double hann256(int n) { return 0.5 - 0.5 * cos(2.0 * kPi * (double)(n + 1) / 257.0); }

// x float[rows][L] -> y float[rows][n_out]
__global__ __launch_bounds__(256) void resample_poly_kernel(const float* __restrict__ x, float* __restrict__ y, long L, long n_out,
                                                            const float* __restrict__ h, int taps, int up, int down) {
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= n_out) return;
    const float* xr = x + (long)blockIdx.y * L;
    const long t = n * down + (taps - 1) / 2;
    const int k0 = (int)(t % up);
    const long i0 = (t - k0) / up;                           // x index of tap k0; tap k0 + j up reads x[i0 - j]
    long j_lo = i0 - (L - 1);
    if (j_lo < 0) j_lo = 0;
    long j_hi = k0 < taps ? (taps - 1 - k0) / up : -1;       // last tap of this phase
    if (j_hi > i0) j_hi = i0;
    float acc = 0.f;
    for (long j = j_lo; j <= j_hi; ++j) acc = fmaf(h[k0 + j * up], xr[i0 - j], acc);
    y[(long)blockIdx.y * n_out + n] = (float)up * acc;
}

// numpy's max / minimum: a NaN operand wins (fmax / fmin would drop it)
__device__ __forceinline__ double nan_max(double a, double b) { return (a != a || b != b) ? (double)NAN : fmax(a, b); }
__device__ __forceinline__ double nan_min(double a, double b) { return (a != a || b != b) ? (double)NAN : fmin(a, b); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// clean float[B][L] -> e double[B][F] (scratch), idx int[B][F] (kept frame indices, ascending), kept int[B]
__global__ __launch_bounds__(256) void stoi_keep_kernel(const float* __restrict__ clean, long L, long F, double* __restrict__ e_ws,
                                                        int* __restrict__ idx_ws, int* __restrict__ kept) {
    __shared__ double win[kFrame];
    __shared__ double red[256];
    __shared__ int wave_cnt[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long b = blockIdx.x;
    win[t] = hann256(t);
    __syncthreads();
    const float* x = clean + b * L;
    double* e = e_ws + b * F;
    int* idx = idx_ws + b * F;
    for (long f = wave; f < F; f += 4) {
        const float* xf = x + f * kHop;
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double v = win[lane + 64 * r] * (double)xf[lane + 64 * r];
            s = fma(v, v, s);
        }
        s = wave_sum(s);
        if (lane == 0) e[f] = 20.0 * log10(sqrt(s) + kEps);
    }
    __syncthreads();                                         // e[] written by the other waves of this workgroup
    double m = -INFINITY;
    for (long f = t; f < F; f += 256) m = nan_max(m, e[f]);
    red[t] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] = nan_max(red[t], red[t + w]);
        __syncthreads();
    }
    const double thr = red[0] - kDynRange;                   // (max(e) - dyn_range - e) < 0, in the host's order (NaN: none kept)
    int running = 0;
    for (long base = 0; base < F; base += 256) {
        const long f = base + t;
        const bool keep = f < F && (thr - e[f]) < 0.0;
        const unsigned long long bal = __ballot(keep);
        const int before = __popcll(bal & ((1ULL << lane) - 1ULL));
        if (lane == 0) wave_cnt[wave] = __popcll(bal);
        __syncthreads();
        int off = running;
        for (int w = 0; w < wave; ++w) off += wave_cnt[w];
        if (keep) idx[off + before] = (int)f;
        running += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();                                     // wave_cnt is rewritten by the next chunk
    }
    if (t == 0) kept[b] = running;
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
    __shared__ float2 tw[M], tw512[M];
    __shared__ float win[kFrame];
    __shared__ float2 buf[kFramesPerWg][2][M];
    __shared__ float pw[kFramesPerWg][M + 1];
    build_twiddles(tw, tw512);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    win[t] = (float)hann256(t);
    __syncthreads();
    const long m = m0 + wave;
    const bool live = m < Mb;
    float2* a = buf[wave][0];
    float2* bb = buf[wave][1];
    if (live) {
        const float* x = (sig ? est : clean) + b * L;
        const int* idx = idx_ws + b * F;
        const float* cur = x + (long)idx[m] * kHop;
        const float* nxt = x + (long)idx[m + 1] * kHop;
        const float* prv = m > 0 ? x + (long)idx[m - 1] * kHop : nullptr;
#pragma unroll
        for (int r = 0; r < 2; ++r) {                        // samples 2 q, 2 q + 1 < 256; 256..511 are the zero padding
            const int q = lane + 64 * r;
            float g[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int p = 2 * q + u;
                float s;
                if (p < kHop) s = (prv ? win[p + kHop] * prv[p + kHop] : 0.f) + win[p] * cur[p];
                else s = win[p] * cur[p] + win[p - kHop] * nxt[p - kHop];
                g[u] = win[p] * s;
            }
            a[q] = make_float2(g[0], g[1]);
            a[q + 128] = make_float2(0.f, 0.f);
        }
    }
    __syncthreads();
    fft256<false>(a, bb, tw, lane);
    float* P = pw[wave];
    if (live) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float2 G = rfft512_bin(a, tw512, lane + 64 * r);
            P[lane + 64 * r] = G.x * G.x + G.y * G.y;
        }
        if (lane == 0) {
            const float2 G = rfft512_nyquist(a);
            P[M] = G.x * G.x;
        }
    }
    __syncthreads();
    if (live && lane < kBands) {
        const int lo = min(max(band_lo[lane], 0), M + 1), hi = min(max(band_hi[lane], lo), M + 1);
        float s = 0.f;
        for (int k = lo; k < hi; ++k) s += P[k];
        band_ws[((b * 2 + sig) * Mmax + m) * kBands + lane] = sqrtf(s);
    }
}

// one (segment, band) pair of the intermediate intelligibility: frames s .. s + 29 of band j
__device__ __forceinline__ double segment_corr(const float* __restrict__ X, const float* __restrict__ Y, long s, int j) {
    const float* xs = X + s * kBands + j;
    const float* ys = Y + s * kBands + j;
    double sx2 = 0.0, sy2 = 0.0;
    for (int i = 0; i < kSeg; ++i) {
        const double xv = xs[i * kBands], yv = ys[i * kBands];
        sx2 = fma(xv, xv, sx2);
        sy2 = fma(yv, yv, sy2);
    }
    const double norm = sqrt(sx2) / (sqrt(sy2) + kEps);
    double sp = 0.0, sx = 0.0;
    for (int i = 0; i < kSeg; ++i) {
        const double xv = xs[i * kBands], yv = ys[i * kBands];
        sp += nan_min(yv * norm, xv * (1.0 + kClip));
        sx += xv;
    }
    const double mp = sp / kSeg, mx = sx / kSeg;
    double spp = 0.0, sxx = 0.0, spx = 0.0;
    for (int i = 0; i < kSeg; ++i) {
        const double xv = xs[i * kBands], yv = ys[i * kBands];
        const double pc = nan_min(yv * norm, xv * (1.0 + kClip)) - mp, xc = xv - mx;
        spp = fma(pc, pc, spp);
        sxx = fma(xc, xc, sxx);
        spx = fma(pc, xc, spx);
    }
    return spx / ((sqrt(spp) + kEps) * (sqrt(sxx) + kEps));
}

__global__ __launch_bounds__(256) void stoi_score_kernel(const float* __restrict__ band_ws, const int* __restrict__ kept, long Mmax,
                                                         float* __restrict__ out_d) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    const long b = blockIdx.x;
    const int K = kept[b];
    const long Mb = K > 0 ? K - 1 : 0;
    if (Mb < kSeg) {                                         // pystoi: "Not enough STFT frames"
        if (t == 0) out_d[b] = 1e-5f;
        return;
    }
    const float* X = band_ws + (b * 2) * Mmax * kBands;
    const float* Y = X + Mmax * kBands;
    const long nseg = Mb - kSeg + 1, pairs = nseg * kBands;
    double acc = 0.0;
    for (long p = t; p < pairs; p += 256) acc += segment_corr(X, Y, p / kBands, (int)(p % kBands));
    red[t] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) out_d[b] = (float)(red[0] / (double)pairs);
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
    if (B <= 0 || B > 32767 || L10 < 0 || L10 > (1L << 31) || !band_lo || !band_hi || !out_d || !out_kept || !workspace)
        return DCS_ERR_BADARG;
    if (L10 > 0 && (!clean10 || !est10)) return DCS_ERR_BADARG;
    const StoiLayout s = stoi_layout(B, L10);
    if (workspace_bytes < s.bytes) return DCS_ERR_WORKSPACE;
    char* ws = static_cast<char*>(workspace);
    double* e_ws = reinterpret_cast<double*>(ws);
    int* idx_ws = reinterpret_cast<int*>(ws + s.off_idx);
    float* band_ws = reinterpret_cast<float*>(ws + s.off_band);
    hipStream_t st = dcs_stream(stream);
    DCS_LAUNCH(stoi_keep_kernel, dim3(B), dim3(256), 0, st, clean10, L10, s.F, e_ws, idx_ws, out_kept);
    DCS_CHECK_LAUNCH();
    if (s.Mmax > 0) {
        DCS_LAUNCH(stoi_bands_kernel, dim3((unsigned)((s.Mmax + kFramesPerWg - 1) / kFramesPerWg), 2 * B), dim3(256), 0, st, clean10,
                   est10, L10, s.F, s.Mmax, idx_ws, out_kept, band_lo, band_hi, band_ws);
        DCS_CHECK_LAUNCH();
    }
    DCS_LAUNCH(stoi_score_kernel, dim3(B), dim3(256), 0, st, band_ws, out_kept, s.Mmax, out_d);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}
