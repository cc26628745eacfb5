// fft512_common.h — the 512-point real FFT's building blocks, one wavefront per frame: complex helpers, the twiddle tables,
// the 256-point radix-4 Stockham transform over two LDS buffers and the forward real-FFT twist.  Shared by the waveform
// synthesis (fft512.hip) and the on-device STOI (stoi.hip).
//   * a real transform of length N = 512 is a complex one of length M = 256 plus an O(M) twist: forward
//       z[m] = g[2m] + j g[2m+1],  Zf = DFT_M(z),  G[k] = 1/2 [(Zf[k] + conj Zf[M-k]) - j W^k (Zf[k] - conj Zf[M-k])],  W = e^{-2 pi j / N}
//     and inverse (unnormalised; the imaginary parts of the DC and Nyquist bins are ignored as every c2r transform does)
//       Z[k] = (X[k] + conj X[M-k]) + j W^{-k} (X[k] - conj X[M-k]),  z = IDFT_M(Z) (no 1/M),  y[2m] = Re z[m], y[2m+1] = Im z[m];
//   * the 256-point complex transform is four radix-4 Stockham passes over two LDS buffers: 64 lanes x one butterfly per
//     pass, twiddles from a 256-entry table built once per workgroup (256 threads) with sincospif.
#pragma once
#include "dcs_common.h"

namespace dcs_fft512 {

constexpr int N = 512, M = 256;

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cconj(float2 a) { return make_float2(a.x, -a.y); }
__device__ __forceinline__ float2 mulj(float2 a) { return make_float2(-a.y, a.x); }      // j * a

// tw[i] = e^{+2 pi j i / 256}; a forward transform conjugates on use
__device__ __forceinline__ void build_twiddles(float2* tw, float2* tw512) {
    const int t = threadIdx.x;
    float s, c;
    sincospif(2.f * (float)t / (float)M, &s, &c);
    tw[t] = make_float2(c, s);
    sincospif(2.f * (float)t / (float)N, &s, &c);
    tw512[t] = make_float2(c, s);                            // e^{+2 pi j t / 512}, t < 256
}

// In-place (result back in a) 256-point complex DFT over LDS buffers a, b of one wavefront; INV: e^{+...}, unnormalised.
// Stockham radix 4: pass Ns = 1, 4, 16, 64; lane j: inputs a[j + 64 r] * tw^(r (j % Ns) 64 / Ns), outputs b[expand(j) + r Ns].
template <bool INV>
__device__ __forceinline__ void fft256(float2* a, float2* b, const float2* tw, int lane) {
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int Ns = 1 << (2 * pass);
        const int k = lane & (Ns - 1);
        float2 v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float2 w = tw[(r * k * (64 / Ns)) & (M - 1)];
            if (!INV) w.y = -w.y;
            v[r] = cmul(a[lane + 64 * r], w);
        }
        const float2 s02 = cadd(v[0], v[2]), d02 = csub(v[0], v[2]), s13 = cadd(v[1], v[3]), d13 = csub(v[1], v[3]);
        const float2 jd = INV ? mulj(d13) : make_float2(d13.y, -d13.x);            // +j d13 (inverse) or -j d13 (forward)
        const int j0 = ((lane >> (2 * pass)) << (2 * pass + 2)) + k;               // (lane / Ns) * 4 Ns + k
        // (b was last READ one pass ago, before that pass's barrier: no barrier needed before overwriting it)
        b[j0] = cadd(s02, s13);
        b[j0 + Ns] = cadd(d02, jd);
        b[j0 + 2 * Ns] = csub(s02, s13);
        b[j0 + 3 * Ns] = csub(d02, jd);
        __syncthreads();
        float2* tmp = a; a = b; b = tmp;
    }
}

// Forward twist: bin k in [0, 256) of the real 512-point transform from a = DFT_256(z) (fft256<false>'s result).
__device__ __forceinline__ float2 rfft512_bin(const float2* a, const float2* tw512, int k) {
    const float2 zk = a[k], zm = cconj(a[(M - k) & (M - 1)]);
    const float2 e = cadd(zk, zm), o = cmul(csub(zk, zm), cconj(tw512[k]));       // W^k = conj(tw512[k])
    // G = 1/2 (e - j o)
    return make_float2(0.5f * (e.x + o.y), 0.5f * (e.y - o.x));
}

// Bin k = M: W^M = -1, Zf[M] = Zf[0]
__device__ __forceinline__ float2 rfft512_nyquist(const float2* a) {
    const float2 z0 = a[0];
    return make_float2(z0.x - z0.y, 0.f);
}

}  // namespace dcs_fft512
