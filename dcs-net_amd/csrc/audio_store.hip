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
//                               (x_off / y_off, int64 prefix offsets); a thread finds its row by owner() of y_off.
//   audio_stft_batch_kernel   one training batch from the resident 16 kHz store in one launch: per item b the crop
//                               [start_b, start_b + L) of utterance idx_b (zero past its end: data.py:90-104), the reflect padding
//                               of torch.stft(center=True), the windowed frames of clean, noise = noisy - clean (time domain,
//                               data.py:104) and noisy, the 512-point real FFT, the DC bin dropped, 1 / sqrt(512) and the
//                               network's [B][256][T] layout (data.py:104-134).  The frames and their spectra never leave LDS.
//                               Every element goes through the operations of stft_frames_kernel (synth.hip), rfft512_kernel
//                               (fft512.hip, through fft512_common.h) and stft_bins_kernel in the same order, so the result is
//                               bit for bit what frontend.stft_batch makes of the cropped waveforms.
//
// audio_stft_batch_kernel (its body: audio_batch_common.h, shared with audio_mix.hip): a workgroup owns kFrames consecutive frames of one item; for each of the three signals in turn every wave
// transforms kFrames / 4 of them (frames held transformed in LDS, one padded row per frame), then the workgroup writes the 256
// bins x kFrames frames as runs of kFrames * 8 bytes along T.  The index and start of an item are read from device memory (a
// captured graph replays with what the host wrote there since); an index outside [0, n_items) or a start whose crop would leave
// the utterance yields zeros for that item, so no value in those buffers makes the kernel read outside the store.
#include "audio_batch_common.h"
#include "ragged_common.h"

namespace {

using namespace dcs_audio_batch;

// x float[x_off[rows]] (ragged rows) -> y float[y_off[rows]]; y_off[r + 1] - y_off[r] = ceil(n (x_off[r + 1] - x_off[r]) / o)
__global__ __launch_bounds__(256) void resample_sinc_kernel(const float* __restrict__ x, const long* __restrict__ x_off,
                                                            float* __restrict__ y, const long* __restrict__ y_off, int rows,
                                                            long total, const float* __restrict__ h, int o, int n, int K,
                                                            int width) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int lo = dcs_ragged::owner(y_off, rows, g);
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

// the paired store's samples: clean and noisy at the same position of the same utterance, zero past its end (crop_batch)
struct PairedSource {
    const float* cs;
    const float* ns;
    long len;
    int start;
    __device__ __forceinline__ void load(int q, bool, float& c, float& y) const {
        const long p = (long)start + q;
        c = p < len ? cs[p] : 0.f;
        y = p < len ? ns[p] : 0.f;
    }
};

// grid (ceil(T / kFrames), B); outputs complex[B][256][T]
__global__ __launch_bounds__(256) void audio_stft_batch_kernel(const float* __restrict__ clean, const float* __restrict__ noisy,
                                                               const long* __restrict__ off, int n_items,
                                                               const int* __restrict__ item_idx, const int* __restrict__ item_start,
                                                               const float* __restrict__ w, float2* __restrict__ out_noise,
                                                               float2* __restrict__ out_noisy, float2* __restrict__ out_clean,
                                                               int T, int hop, int L, float scale) {
    const int start = item_start[blockIdx.y];
    long base, len;
    const bool ok = crop_of_item(off, n_items, item_idx[blockIdx.y], start, L, &base, &len);
    stft_batch_body(PairedSource{clean + base, noisy + base, len, start}, ok, w, out_noise, out_noisy, out_clean, T, hop, L, scale);
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
