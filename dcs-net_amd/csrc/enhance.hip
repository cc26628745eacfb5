// enhance.hip — whole recordings through a fixed-shape network pass (dcsnet/enhance.py): a recording of any length is cut into
// segments of T frames that overlap by O frames, every segment goes through the network as one row of a static [S][256][T]
// batch, and the segment waveforms are cross-faded back into one waveform per recording.
//
//   Geometry.  Recording i of len_i samples is treated as zero-extended to L_i = hop (Tp_i - 1) samples, Tp_i = T + n (T - O)
//   for the smallest n >= 0 with L_i >= len_i: it has n + 1 segments, segment s covers frames [s (T - O), s (T - O) + T) of the
//   extended recording's centred STFT and samples [s (T - O) hop, s (T - O) hop + hop (T - 1)) of its waveform.  Consecutive
//   segments share hop (O - 1) samples; with 2 <= O <= T / 2 no sample belongs to more than two segments.
//
//   audio_stft_segments_kernel   the noisy-only STFT of S segments named by device-resident (item, first_frame) pairs, from a
//                                  ragged store (float samples + int64 offsets: DeviceAudioStore's layout).  Reflection happens
//                                  at 0 and at L_i only — a segment edge inside the recording reads its neighbours' real audio —
//                                  and samples at or past len_i read as zero.  Per element the operations of
//                                  audio_stft_batch_kernel (audio_store.hip) in the same order: window, Stockham pass in LDS,
//                                  bins 1..256, scale; so frames [f, f + T) equal that kernel's frames of the whole extended
//                                  recording bit for bit.  One transform per frame (no clean signal), grid (ceil(T / 8), S),
//                                  64-byte output runs along T.  An item outside [0, n_items), a negative first frame or a window
//                                  leaving [0, Tp_i) yields zeros and reads nothing: the last batch is padded with such rows,
//                                  and no value in the table makes the kernel read outside the store.
//   segments_stitch_kernel       segment waveforms [rows][hop (T - 1)] -> one ragged row per recording (len_i samples, the
//                                  store's offsets).  One thread per output sample finds its recording by owner() of the
//                                  offsets (ragged_common.h), then its segment; inside an overlap of n samples, sample j
//                                  is a + w (b - a), w = (j + 0.5) / n, a the earlier and b the later segment's sample;
//                                  everywhere else the one covering segment's sample is copied unchanged.  Plain stores, no
//                                  atomics: bit-reproducible.  Optionally the same thread writes the sample as 16-bit PCM.
#include "fft512_common.h"
#include "ragged_common.h"

#ifndef DCS_AUDIO_FRAMES_PER_WG
#define DCS_AUDIO_FRAMES_PER_WG 8
#endif

namespace {

using namespace dcs_fft512;

constexpr int kFrames = DCS_AUDIO_FRAMES_PER_WG;              // frames per workgroup: bins stored as runs of kFrames * 8 B
static_assert(kFrames % 4 == 0 && kFrames >= 8 && kFrames <= 32, "frames per workgroup: a multiple of 4 waves, runs >= 64 B");
constexpr int kPitch = M + 32 / kFrames;                     // row pitch (float2): the bin reads below hit 64 distinct banks

// torch.stft(center=True, pad_mode='reflect') index in a signal of L samples (L > 256: one reflection suffices)
__device__ __forceinline__ long reflect_index(long n, long L) {
    if (n < 0) n = -n;
    if (n >= L) n = 2 * (L - 1) - n;
    return n;
}

// frames of recording `len` samples long in segments of T frames overlapping by O: Tp = T + n (T - O), hop (Tp - 1) >= len
__device__ __forceinline__ long padded_frames(long len, int T, int O, int hop) {
    const long Ls = (long)hop * (T - 1), stride = (long)hop * (T - O);
    const long n = len <= Ls ? 0 : (len - Ls + stride - 1) / stride;
    return T + n * (T - O);
}

// grid (ceil(T / kFrames), S); out complex[S][256][T]
__global__ __launch_bounds__(256) void audio_stft_segments_kernel(const float* __restrict__ noisy, const long* __restrict__ off,
                                                                  int n_items, const int* __restrict__ seg_item,
                                                                  const int* __restrict__ seg_frame, const float* __restrict__ w,
                                                                  float2* __restrict__ out, int T, int O, int hop, float scale) {
    __shared__ float2 tw[M], tw512[M];
    __shared__ float2 fa[kFrames][kPitch];                   // frame t0 + slot, transformed in place
    __shared__ float2 fb[4][M];                              // a wave's second Stockham buffer
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long b = blockIdx.y;
    const int t0 = (int)blockIdx.x * kFrames;
    const int item = seg_item[b], f0 = seg_frame[b];
    long base = 0, len = 0, L = 0;
    bool ok = item >= 0 && item < n_items && f0 >= 0;
    if (ok) {
        base = off[item];
        len = off[item + 1] - base;
        const long Tp = padded_frames(len, T, O, hop);
        ok = len >= 0 && (long)f0 + T <= Tp;
        L = (long)hop * (Tp - 1);
    }
    if (!ok) {                                               // (uniform over the workgroup: no barrier skipped by a part of it)
        for (int e = threadIdx.x; e < M * kFrames; e += 256) {
            const int t = t0 + e % kFrames, f = e / kFrames;
            if (t < T) out[(b * M + f) * T + t] = make_float2(0.f, 0.f);
        }
        return;
    }
    build_twiddles(tw, tw512);
    const float* ns = noisy + base;
#pragma unroll 1
    for (int i = 0; i < kFrames / 4; ++i) {
        const int slot = wave * (kFrames / 4) + i, t = t0 + slot;
        float2* a = fa[slot];
        if (t < T) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = lane + 64 * r, k = 2 * m;
                const long n = ((long)f0 + t) * hop + k - N / 2;
                const long p0 = reflect_index(n, L), p1 = reflect_index(n + 1, L);
                const float y0 = p0 < len ? ns[p0] : 0.f, y1 = p1 < len ? ns[p1] : 0.f;     // zero past the recording's end
                const float2 wk = *reinterpret_cast<const float2*>(w + k);
                a[m] = make_float2(wk.x * y0, wk.y * y1);    // (g[2m], g[2m + 1]): rfft512_kernel's load of the stored frame
            }
        }
        __syncthreads();                                     // (first round: the twiddle tables as well)
        fft256<false>(a, fb[wave], tw, lane);                // frames past T transform stale LDS: never stored below
    }
    // fft256 ends on a barrier: every transform is in fa
    for (int e = threadIdx.x; e < M * kFrames; e += 256) {
        const int tt = e % kFrames, f = e / kFrames, t = t0 + tt;
        if (t < T) {
            const int k = f + 1;                             // the DC bin dropped (data.py:118)
            const float2 v = k < M ? rfft512_bin(fa[tt], tw512, k) : rfft512_nyquist(fa[tt]);
            out[(b * M + f) * T + t] = make_float2(v.x * scale, v.y * scale);      // stft_bins_kernel's scaling
        }
    }
}

// seg float[rows][Ls] (Ls = hop (T - 1)); recording r owns rows [seg_first[r], seg_first[r + 1]) and y[y_off[r], y_off[r + 1])
__global__ __launch_bounds__(256) void segments_stitch_kernel(const float* __restrict__ seg, const int* __restrict__ seg_first,
                                                              const long* __restrict__ y_off, int recs, long total, long rows,
                                                              float* __restrict__ y, short* __restrict__ pcm, long Ls,
                                                              long stride, int ov) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int lo = dcs_ragged::owner(y_off, recs, g);
    const long m = g - y_off[lo];
    const long r0 = seg_first[lo], nseg = seg_first[lo + 1] - r0;
    long s = m / stride;
    if (s > nseg - 1) s = nseg - 1;                          // the last segment runs hop (O - 1) samples past its stride
    const long j = m - s * stride;
    float v = 0.f;
    // a table that does not cover the sample (too few segments, rows outside the buffer) yields silence, never a stray read
    if (nseg > 0 && r0 >= 0 && r0 + nseg <= rows && j < Ls) {
        const float* cur = seg + (r0 + s) * Ls;
        v = cur[j];
        if (s > 0 && j < ov) {
            const float a = cur[j + stride - Ls], wgt = ((float)j + 0.5f) / (float)ov;       // the earlier segment's row ends at cur
            v = a + wgt * (v - a);
        }
    }
    y[g] = v;
    if (pcm) pcm[g] = (short)fminf(fmaxf(rintf(v * 32768.f), -32767.f), 32767.f);
}

}  // namespace

extern "C" int dcs_audio_stft_segments_f32(const float* noisy, const long* offsets, int n_items, const int* seg_item,
                                           const int* seg_first_frame, int S, const float* window, int n_fft, int T, int overlap,
                                           int hop, float scale, float* out, dcs_stream_t stream) {
    if (!noisy || !offsets || !seg_item || !seg_first_frame || !window || !out || n_items <= 0 || S <= 0 || S > 65535 ||
        n_fft != N || T < 2 || hop <= 0 || overlap < 0 || overlap >= T)
        return DCS_ERR_BADARG;
    const long Ls = (long)hop * (T - 1);
    if (Ls <= N / 2 || Ls > 0x7fffffffL - N) return DCS_ERR_BADARG;     // one reflection reaches every padded index
    DCS_LAUNCH(audio_stft_segments_kernel, dim3((unsigned)((T + kFrames - 1) / kFrames), S), dim3(256), 0, dcs_stream(stream), noisy,
               offsets, n_items, seg_item, seg_first_frame, window, (float2*)out, T, overlap, hop, scale);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}

extern "C" int dcs_segments_stitch_f32(const float* seg, long seg_rows, const int* seg_first, const long* offsets, int n_items,
                                       long total_out, int T, int overlap, int hop, float* y, short* pcm, dcs_stream_t stream) {
    if (!seg || !seg_first || !offsets || !y || seg_rows <= 0 || n_items <= 0 || total_out < 0 || hop <= 0 || T < 4 ||
        overlap < 2 || 2 * overlap > T || (total_out + 255) / 256 > 0x7fffffffL)
        return DCS_ERR_BADARG;
    if (total_out == 0) return DCS_OK;
    DCS_LAUNCH(segments_stitch_kernel, dim3((unsigned)((total_out + 255) / 256)), dim3(256), 0, dcs_stream(stream), seg, seg_first,
               offsets, n_items, total_out, seg_rows, y, pcm, (long)hop * (T - 1), (long)hop * (T - overlap), hop * (overlap - 1));
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}
