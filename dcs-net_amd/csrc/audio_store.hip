// audio_store.hip — the data path of an HBM-resident training set (dcsnet/audio_store.py): what the reference's Dataset does per
// item on CPU loader workers (data.py:68-143), on the device.
//
//   resample_sinc_kernel      torchaudio.transforms.Resample(orig, new) of torchaudio 0.9.0 (sinc_interpolation, lowpass filter
//                               width 6, rolloff 0.99; config.py:61, data.py:84-85), run once per utterance when the store is
//                               loaded.  With o = orig / g, n = new / g (g = gcd) and width = ceil(6 o / (0.99 min(o, n))):
//                               y[j n + i] = sum_k h_i[k] x[j o + k - width],  k = 0 .. K - 1 ascending,  K = 2 width + o,
//                               x = 0 outside [0, L), j n + i < ceil(n L / o) — pad(width, width + o), conv1d(stride o) and the
//                               transpose / reshape of _apply_sinc_resample_kernel.  The taps h float[n][K] are computed on the
//                               host in fp64 and rounded once (ops.sinc_resample_taps).  One thread per output sample, fp32
//                               accumulation in tap order: the result does not depend on the launch geometry.  Rows are ragged
//                               (x_off / y_off, int64 prefix offsets); a thread finds its row by bisection of y_off.
//   audio_stft_batch_kernel   one training batch from the resident 16 kHz store in one launch: per item b the crop
//                               [start_b, start_b + L) of utterance idx_b (zero past its end: data.py:90-104), the reflect padding
//                               of torch.stft(center=True), the windowed frames of clean, noise = noisy - clean (time domain,
//                               data.py:104) and noisy, the 512-point real FFT, the DC bin dropped, 1 / sqrt(512) and the
//                               network's [B][256][T] layout (data.py:104-134).  The frames and their spectra never leave LDS.
//                               Every element goes through the operations of stft_frames_kernel (synth.hip), rfft512_kernel
//                               (fft512.hip, through fft512_common.h) and stft_bins_kernel in the same order, so the result is
//                               bit for bit what frontend.stft_batch makes of the cropped waveforms.
//
// audio_stft_batch_kernel: a workgroup owns kFrames consecutive frames of one item; for each of the three signals in turn every wave
// transforms kFrames / 4 of them (frames held transformed in LDS, one padded row per frame), then the workgroup writes the 256
// bins x kFrames frames as runs of kFrames * 8 bytes along T.  The index and start of an item are read from device memory (a
// captured graph replays with what the host wrote there since); an index outside [0, n_items) or a start whose crop would leave
// the utterance yields zeros for that item, so no value in those buffers makes the kernel read outside the store.
#include "fft512_common.h"

#ifndef DCS_AUDIO_FRAMES_PER_WG
#define DCS_AUDIO_FRAMES_PER_WG 8
#endif

namespace {

using namespace dcs_fft512;

// x float[x_off[rows]] (ragged rows) -> y float[y_off[rows]]; y_off[r + 1] - y_off[r] = ceil(n (x_off[r + 1] - x_off[r]) / o)
__global__ __launch_bounds__(256) void resample_sinc_kernel(const float* __restrict__ x, const long* __restrict__ x_off,
                                                            float* __restrict__ y, const long* __restrict__ y_off, int rows,
                                                            long total, const float* __restrict__ h, int o, int n, int K,
                                                            int width) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    int lo = 0, hi = rows;                                   // y_off[lo] <= g < y_off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (y_off[mid] <= g) lo = mid; else hi = mid;
    }
    const long xb = x_off[lo], L = x_off[lo + 1] - xb;
    const long m = g - y_off[lo], j = m / n;
    const int i = (int)(m - j * n);
    const long p0 = j * o - width;
    const float* hi_ = h + (long)i * K;
    float acc = 0.f;
    for (int k = 0; k < K; ++k) {
        const long p = p0 + k;
        if (p >= 0 && p < L) acc = fmaf(hi_[k], x[xb + p], acc);
    }
    y[g] = acc;
}

constexpr int kFrames = DCS_AUDIO_FRAMES_PER_WG;              // frames per workgroup: bins stored as runs of kFrames * 8 B
static_assert(kFrames % 4 == 0 && kFrames >= 8 && kFrames <= 32, "frames per workgroup: a multiple of 4 waves, runs >= 64 B");
constexpr int kPitch = M + 32 / kFrames;                     // row pitch (float2): the bin reads below hit 64 distinct banks

// torch.stft(center=True, pad_mode='reflect') index of a crop of L samples (L > 256: one reflection suffices)
__device__ __forceinline__ int reflect_index(int n, int L) {
    if (n < 0) n = -n;
    if (n >= L) n = 2 * (L - 1) - n;
    return n;
}

// grid (ceil(T / kFrames), B); outputs complex[B][256][T]
__global__ __launch_bounds__(256) void audio_stft_batch_kernel(const float* __restrict__ clean, const float* __restrict__ noisy,
                                                               const long* __restrict__ off, int n_items,
                                                               const int* __restrict__ item_idx, const int* __restrict__ item_start,
                                                               const float* __restrict__ w, float2* __restrict__ out_noise,
                                                               float2* __restrict__ out_noisy, float2* __restrict__ out_clean,
                                                               int T, int hop, int L, float scale) {
    __shared__ float2 tw[M], tw512[M];
    __shared__ float2 fa[kFrames][kPitch];                   // frame t0 + slot of the current signal, transformed in place
    __shared__ float2 fb[4][M];                              // a wave's second Stockham buffer
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long b = blockIdx.y;
    const int t0 = (int)blockIdx.x * kFrames;
    const int item = item_idx[b], start = item_start[b];
    long base = 0, len = 0;
    bool ok = item >= 0 && item < n_items && start >= 0;
    if (ok) {
        base = off[item];
        len = off[item + 1] - base;
        ok = start == 0 || (long)start + L <= len;           // crop_batch's starts: 0 when len <= L, else start + L < len
    }
    if (!ok) {                                               // (uniform over the workgroup: no barrier skipped by a part of it)
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
    const float* cs = clean + base;
    const float* ns = noisy + base;
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
                    const long p0 = (long)start + reflect_index(n, L), p1 = (long)start + reflect_index(n + 1, L);
                    const float c0 = p0 < len ? cs[p0] : 0.f, c1 = p1 < len ? cs[p1] : 0.f;     // zero past the end (crop_batch)
                    const float y0 = p0 < len ? ns[p0] : 0.f, y1 = p1 < len ? ns[p1] : 0.f;
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

}  // namespace

extern "C" int dcs_resample_sinc_f32(const float* x, const long* x_off, float* y, const long* y_off, int rows, long total_out,
                                     const float* taps, int orig, int new_, int width, dcs_stream_t stream) {
    if (!x || !x_off || !y || !y_off || !taps || rows <= 0 || total_out < 0 || orig <= 0 || new_ <= 0 || width < 0 ||
        (total_out + 255) / 256 > 0x7fffffffL)
        return DCS_ERR_BADARG;
    if (total_out == 0) return DCS_OK;
    DCS_LAUNCH(resample_sinc_kernel, dim3((unsigned)((total_out + 255) / 256)), dim3(256), 0, dcs_stream(stream), x, x_off, y, y_off,
               rows, total_out, taps, orig, new_, 2 * width + orig, width);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}

extern "C" int dcs_audio_stft_batch_f32(const float* clean, const float* noisy, const long* offsets, int n_items,
                                        const int* item_index, const int* item_start, int B, const float* window, int n_fft,
                                        int T, int hop, float scale, float* out_noise, float* out_noisy, float* out_clean,
                                        dcs_stream_t stream) {
    if (!clean || !noisy || !offsets || !item_index || !item_start || !window || !out_noise || !out_noisy || !out_clean ||
        n_items <= 0 || B <= 0 || B > 65535 || n_fft != N || T < 2 || hop <= 0)
        return DCS_ERR_BADARG;
    const long L = (long)hop * (T - 1);
    if (L <= N / 2 || L > 0x7fffffffL - N) return DCS_ERR_BADARG;      // one reflection reaches every padded index
    DCS_LAUNCH(audio_stft_batch_kernel, dim3((unsigned)((T + kFrames - 1) / kFrames), B), dim3(256), 0, dcs_stream(stream), clean, noisy,
               offsets, n_items, item_index, item_start, window, (float2*)out_noise, (float2*)out_noisy, (float2*)out_clean, T, hop,
               (int)L, scale);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}
