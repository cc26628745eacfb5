// stoi_common.h — the device code that stoi.hip (B utterances of one length) and stoi_ragged.hip (recordings of any lengths in
// one flat buffer) share: the constants, the resampler's output sample, and the three per-recording stages of STOI (with the
// score stage's extended sibling, ESTOI), each written against ONE recording's pointers.  A kernel of either file only works out where its recording's samples, frame slots and band
// rows lie and then calls the stage, so a recording goes through the same operations in the same order whichever entry point
// scores it: dcs_stoi_ragged_f32 is bit-equal to dcs_stoi_f32 with B = 1 on the same samples.
#pragma once
#include "fft512_common.h"
#include "ragged_common.h"

namespace dcs_stoi {

using namespace dcs_fft512;

constexpr int kFrame = 256, kHop = 128, kBands = 15, kSeg = 30, kFramesPerWg = 4;
constexpr double kEps = 2.220446049250313e-16;              // np.finfo(float).eps
constexpr double kDynRange = 40.0;
constexpr double kClip = 5.623413251903491;                 // 10 ** (15 / 20)
constexpr double kPi = 3.141592653589793;

// frames of range(0, L - 256, 128): both framings of the host function
__host__ __device__ inline long stoi_frames(long L) { return L > kFrame ? (L - kFrame + kHop - 1) / kHop : 0; }

using dcs_ragged::align256;                                  // the one definition of the ragged / STOI family

// hanning(258)[1:-1]
__device__ __forceinline__ double hann256(int n) { return 0.5 - 0.5 * cos(2.0 * kPi * (double)(n + 1) / 257.0); }

// numpy's max / minimum: a NaN operand wins (fmax / fmin would drop it)
__device__ __forceinline__ double nan_max(double a, double b) { return (a != a || b != b) ? (double)NAN : fmax(a, b); }
__device__ __forceinline__ double nan_min(double a, double b) { return (a != a || b != b) ? (double)NAN : fmin(a, b); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// output sample n of the polyphase resampler for one row xr float[L]
__device__ __forceinline__ float resample_poly_sample(const float* __restrict__ xr, long L, long n, const float* __restrict__ h,
                                                      int taps, int up, int down) {
    const long t = n * down + (taps - 1) / 2;
    const int k0 = (int)(t % up);
    const long i0 = (t - k0) / up;                           // x index of tap k0; tap k0 + j up reads x[i0 - j]
    long j_lo = i0 - (L - 1);
    if (j_lo < 0) j_lo = 0;
    long j_hi = k0 < taps ? (taps - 1 - k0) / up : -1;       // last tap of this phase
    if (j_hi > i0) j_hi = i0;
    float acc = 0.f;
    for (long j = j_lo; j <= j_hi; ++j) acc = fmaf(h[k0 + j * up], xr[i0 - j], acc);
    return (float)up * acc;
}

// The keep stage of one recording, by one workgroup of 256 threads: x float[> 128 (F - 1) + 255] -> e double[F] (scratch),
// idx int[F] (kept frame indices, ascending); returns the kept count (every thread).  win / red / wave_cnt: the workgroup's LDS.
__device__ __forceinline__ int keep_frames(const float* __restrict__ x, long F, double* __restrict__ e, int* __restrict__ idx,
                                           double* win, double* red, int* wave_cnt) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    win[t] = hann256(t);
    __syncthreads();
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
    return running;
}

// The band stage of one signal of one recording, by one workgroup (one wavefront per STFT frame): frames m0 .. m0 + 3 (< Mb) of
// the overlap-added kept frames of x -> band float[Mb][15], sqrt of the band sums of |rfft512(hann * frame m)|^2.  The caller
// has checked m0 < Mb for the whole workgroup.
__device__ __forceinline__ void band_frames(const float* __restrict__ x, const int* __restrict__ idx, long Mb, long m0,
                                            const int* __restrict__ band_lo, const int* __restrict__ band_hi,
                                            float* __restrict__ band) {
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
        band[m * kBands + lane] = sqrtf(s);
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

// The score stage of one recording, by one workgroup of 256 threads: the band envelopes X (clean), Y (estimate) float[Mb][15]
// of its K kept frames (Mb = K - 1 STFT frames) -> *out_d; exactly 1e-5 when fewer than 30 STFT frames remain.  red: LDS.
__device__ __forceinline__ void score_frames(const float* __restrict__ X, const float* __restrict__ Y, int K, double* red,
                                             float* __restrict__ out_d) {
    const int t = threadIdx.x;
    const long Mb = K > 0 ? K - 1 : 0;
    if (Mb < kSeg) {                                         // pystoi: "Not enough STFT frames"
        if (t == 0) *out_d = 1e-5f;
        return;
    }
    const long nseg = Mb - kSeg + 1, pairs = nseg * kBands;
    double acc = 0.0;
    for (long p = t; p < pairs; p += 256) acc += segment_corr(X, Y, p / kBands, (int)(p % kBands));
    red[t] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) *out_d = (float)(red[0] / (double)pairs);
}

// The row statistics of one signal of one segment of the extended score: frames 0 .. 29 of xs float[30][15] -> per band its mean
// over the 30 frames and 1 / (norm of the centred row + eps).  Direct sums in ascending frame order, all in registers (the band
// loops unroll).  A constant row has norm 0: its centred values are zeros and stay zeros, no NaN.
__device__ __forceinline__ void segment_rows(const float* __restrict__ xs, double (&mean)[kBands], double (&rinv)[kBands]) {
    double s[kBands];
#pragma unroll
    for (int j = 0; j < kBands; ++j) s[j] = 0.0;
    for (int i = 0; i < kSeg; ++i) {
#pragma unroll
        for (int j = 0; j < kBands; ++j) s[j] += (double)xs[i * kBands + j];
    }
#pragma unroll
    for (int j = 0; j < kBands; ++j) {
        mean[j] = s[j] / kSeg;
        s[j] = 0.0;
    }
    for (int i = 0; i < kSeg; ++i) {
#pragma unroll
        for (int j = 0; j < kBands; ++j) {
            const double c = (double)xs[i * kBands + j] - mean[j];
            s[j] = fma(c, c, s[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < kBands; ++j) rinv[j] = 1.0 / (sqrt(s[j]) + kEps);
}

// one segment of the extended intermediate intelligibility (ESTOI, Jensen & Taal 2016): frames s .. s + 29 of all 15 bands.
// Rows first (each band over its 30 frames: remove the mean, divide by norm + eps), then columns of the result (each frame
// over the 15 bands: the same), then sum(x_n y_n) / 30.  A column's sum(x_n y_n) is formed as sum(x_c y_c) / ((|x_c| + eps)
// (|y_c| + eps)) from its centred values: one division per column.
__device__ __forceinline__ double segment_ext(const float* __restrict__ X, const float* __restrict__ Y, long s) {
    const float* xs = X + s * kBands;
    const float* ys = Y + s * kBands;
    double mx[kBands], rx[kBands], my[kBands], ry[kBands];
    segment_rows(xs, mx, rx);
    segment_rows(ys, my, ry);
    double acc = 0.0;
    for (int i = 0; i < kSeg; ++i) {
        double a[kBands], b[kBands], sa = 0.0, sb = 0.0;
#pragma unroll
        for (int j = 0; j < kBands; ++j) {
            a[j] = ((double)xs[i * kBands + j] - mx[j]) * rx[j];
            b[j] = ((double)ys[i * kBands + j] - my[j]) * ry[j];
            sa += a[j];
            sb += b[j];
        }
        const double ma = sa / kBands, mb = sb / kBands;
        double saa = 0.0, sbb = 0.0, sab = 0.0;
#pragma unroll
        for (int j = 0; j < kBands; ++j) {
            const double ac = a[j] - ma, bc = b[j] - mb;
            saa = fma(ac, ac, saa);
            sbb = fma(bc, bc, sbb);
            sab = fma(ac, bc, sab);
        }
        acc += sab / ((sqrt(saa) + kEps) * (sqrt(sbb) + kEps));
    }
    return acc / kSeg;
}

// The extended score stage of one recording (metrics.stoi(..., extended=True)), by one workgroup of 256 threads: score_frames'
// inputs -> *out_e; exactly 1e-5 when fewer than 30 STFT frames remain.  Thread t takes the segments t, t + 256, ... in
// ascending order, each from its own direct sums (no sums sliding from one segment to the next: their rounding would depend
// on the history), then the fixed LDS tree of score_frames.  A NaN in a segment makes the score NaN.  red: LDS, free to write.
__device__ __forceinline__ void score_frames_ext(const float* __restrict__ X, const float* __restrict__ Y, int K, double* red,
                                                 float* __restrict__ out_e) {
    const int t = threadIdx.x;
    const long Mb = K > 0 ? K - 1 : 0;
    if (Mb < kSeg) {
        if (t == 0) *out_e = 1e-5f;
        return;
    }
    const long nseg = Mb - kSeg + 1;
    double acc = 0.0;
    for (long s = t; s < nseg; s += 256) acc += segment_ext(X, Y, s);
    red[t] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) *out_e = (float)(red[0] / (double)nseg);
}

// Either or both scores of one recording from one pass over its band envelopes (out_d / out_e: null = not asked for).  *out_d
// is score_frames' value, bit for bit.
__device__ __forceinline__ void score_frames_both(const float* __restrict__ X, const float* __restrict__ Y, int K, double* red,
                                                  float* __restrict__ out_d, float* __restrict__ out_e) {
    if (out_d) score_frames(X, Y, K, red, out_d);
    __syncthreads();                                         // red[0] has been read before the next tree overwrites it
    if (out_e) score_frames_ext(X, Y, K, red, out_e);
}

}  // namespace dcs_stoi
