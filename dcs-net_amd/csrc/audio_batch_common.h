// audio_batch_common.h — the one definition of the training batch's frame, FFT and store sequence, shared by
// audio_stft_batch_kernel (audio_store.hip: clean / noisy pairs) and audio_mix_stft_batch_kernel (audio_mix.hip: clean + gain *
// noise).  A kernel decides whether its item is valid, builds a Source — load(q, want_noisy, c, y): the clean and (where
// want_noisy: the clean pass does not use it) the noisy sample at position q of the crop, zero past the utterance's end — and
// calls stft_batch_body.  Whatever the Source, every element
// goes through the operations of stft_frames_kernel (synth.hip), rfft512_kernel (fft512.hip) and stft_bins_kernel in the same
// order, so the result is bit for bit what frontend.stft_batch makes of the waveforms the Source describes.
#pragma once
#include "fft512_common.h"

#ifndef DCS_AUDIO_FRAMES_PER_WG
#define DCS_AUDIO_FRAMES_PER_WG 8
#endif

namespace dcs_audio_batch {

using namespace dcs_fft512;

constexpr int kFrames = DCS_AUDIO_FRAMES_PER_WG;              // frames per workgroup: bins stored as runs of kFrames * 8 B
static_assert(kFrames % 4 == 0 && kFrames >= 8 && kFrames <= 32, "frames per workgroup: a multiple of 4 waves, runs >= 64 B");
constexpr int kPitch = M + 32 / kFrames;                     // row pitch (float2): the bin reads below hit 64 distinct banks

// torch.stft(center=True, pad_mode='reflect') index of a crop of L samples (L > 256: one reflection suffices)
__device__ __forceinline__ int reflect_index(int n, int L) {
    if (n < 0) n = -n;
    if (n >= L) n = 2 * (L - 1) - n;
    return n;
}

// the existing rule for an item of a resident store: index inside [0, n_items), start 0 or a crop that stays inside the utterance
__device__ __forceinline__ bool crop_of_item(const long* __restrict__ off, int n_items, int item, int start, int L, long* base,
                                             long* len) {
    *base = 0;
    *len = 0;
    if (item < 0 || item >= n_items || start < 0) return false;
    *base = off[item];
    *len = off[item + 1] - *base;
    return start == 0 || (long)start + L <= *len;            // crop_batch's starts: 0 when len <= L, else start + L < len
}

// One workgroup (256 threads) of grid (ceil(T / kFrames), B): frames [blockIdx.x * kFrames, + kFrames) of item blockIdx.y; outputs
// complex[B][256][T].  ok must be uniform over the workgroup (no barrier skipped by a part of it): an item that is not ok gets zeros.
template <typename Source>
__device__ __forceinline__ void stft_batch_body(const Source& src, bool ok, const float* __restrict__ w,
                                                float2* __restrict__ out_noise, float2* __restrict__ out_noisy,
                                                float2* __restrict__ out_clean, int T, int hop, int L, float scale) {
    __shared__ float2 tw[M], tw512[M];
    __shared__ float2 fa[kFrames][kPitch];                   // frame t0 + slot of the current signal, transformed in place
    __shared__ float2 fb[4][M];                              // a wave's second Stockham buffer
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long b = blockIdx.y;
    const int t0 = (int)blockIdx.x * kFrames;
    if (!ok) {
        for (int e = threadIdx.x; e < M * kFrames; e += 256) {
            const int t = t0 + e % kFrames, f = e / kFrames;
            if (t < T) {
                const long o = (b * M + f) * T + t;
                out_noise[o] = out_noisy[o] = out_clean[o] = make_float2(0.f, 0.f);
            }
        }
        return;
    }
    build_twiddles(tw, tw512);
#pragma unroll 1
    for (int s = 0; s < 3; ++s) {                            // 0 clean, 1 noise = noisy - clean, 2 noisy (stft_frames_kernel's order)
#pragma unroll 1
        for (int i = 0; i < kFrames / 4; ++i) {
            const int slot = wave * (kFrames / 4) + i, t = t0 + slot;
            float2* a = fa[slot];
            if (t < T) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = lane + 64 * r, k = 2 * m, n = t * hop + k - N / 2;
                    float c0, c1, y0, y1;
                    src.load(reflect_index(n, L), s != 0, c0, y0);     // (the clean pass does not use the noisy sample)
                    src.load(reflect_index(n + 1, L), s != 0, c1, y1);
                    const float2 wk = *reinterpret_cast<const float2*>(w + k);
                    float2 v;
                    if (s == 0) v = make_float2(wk.x * c0, wk.y * c1);
                    else if (s == 1) v = make_float2(wk.x * (y0 - c0), wk.y * (y1 - c1));
                    else v = make_float2(wk.x * y0, wk.y * y1);
                    a[m] = v;                                // (g[2m], g[2m + 1]): rfft512_kernel's load of the stored frame
                }
            }
            __syncthreads();                                 // (first round: the twiddle tables as well)
            fft256<false>(a, fb[wave], tw, lane);            // frames past T transform stale LDS: never stored below
        }
        // fft256 ends on a barrier: every transform of this signal is in fa
        float2* out = s == 0 ? out_clean : (s == 1 ? out_noise : out_noisy);
        for (int e = threadIdx.x; e < M * kFrames; e += 256) {
            const int tt = e % kFrames, f = e / kFrames, t = t0 + tt;
            if (t < T) {
                const int k = f + 1;                         // the DC bin dropped (data.py:118)
                const float2 v = k < M ? rfft512_bin(fa[tt], tw512, k) : rfft512_nyquist(fa[tt]);
                out[(b * M + f) * T + t] = make_float2(v.x * scale, v.y * scale);      // stft_bins_kernel's scaling
            }
        }
        __syncthreads();                                     // before the next signal's frames overwrite fa
    }
}

}  // namespace dcs_audio_batch
