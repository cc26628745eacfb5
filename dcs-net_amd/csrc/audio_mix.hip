// audio_mix.hip — training on a clean-speech corpus and a noise corpus (dcsnet/audio_store.py::MixingAudioStore): the mixture
// noisy = clean + gain * noise is formed on the device, at an SNR, a noise recording and a noise start drawn per item.
//
// The mixture rule (mix_sample, noise_at): for clean item i of len_c samples, noise recording r of len_n >= 1 samples, a noise
// start s in [0, len_n) and a float32 gain g, the noise that belongs to clean position q is noise_r[(s + q) mod len_n] — the
// noise loops and is aligned to the RECORDING's sample 0, not to a crop — and noisy[q] = clean[q] + g * noise[...], the product
// and the sum each rounded to float32 (no FMA), for q < len_c; 0 for q >= len_c (the reference zero-pads both signals of a
// short item: data.py:95-97).
//
//   signal_power_ragged_kernel   out[i] = mean(x_i^2) per recording, squares and sums in fp64: one workgroup per recording,
//                                  thread t adds samples t, t + 256, ... in ascending order, then ragged_common.h's block_sum
//                                  (a fixed tree): the same bits on every run; 0 for an empty recording
//   audio_mix_ragged_kernel      whole-recording mixtures for a materialised set: one thread per sample of the flat clean
//                                  store; it finds its item by owner() of the offsets (as resample_sinc_kernel does); an item
//                                  whose draw cannot be followed gets noisy = clean
//   audio_mix_stft_batch_kernel  audio_stft_batch_kernel (audio_store.hip) with the noisy sample replaced by the mixture rule at
//                                  q = start_b + reflect_index(...): grid, LDS, the order clean -> noise -> noisy and the bin
//                                  store are audio_batch_common.h's, the one definition both kernels instantiate.  noise stays
//                                  what the reference defines, noisy - clean in the time domain (data.py:105), not g * n.
//
// A draw is followed only if the noise index is inside [0, n_noise), the recording has 1 <= len_n < 2^31 samples, the start
// is inside [0, len_n) and the gain is finite; every noise index a kernel forms is reduced into [0, len_n), so no value in the
// selection buffers makes a kernel read outside either store (the offsets themselves are the caller's invariant, as for
// audio_stft_batch_kernel).  The 64-bit modulo is taken once per thread; after it the position advances in 32-bit unsigned
// arithmetic (phase < len_n < 2^31 and a crop offset < 2^31: the sum fits) and is wrapped by a multiplication with
// floor(2^32 / len_n) and one conditional subtraction (noise_at), not by a division per sample.
#include "audio_batch_common.h"
#include "ragged_common.h"

namespace {

using namespace dcs_audio_batch;

// clean + gain * noise in two float32 roundings.  hipcc contracts c + g * n into an FMA by default, and in this toolchain
// __fmul_rn / __fadd_rn are the plain operators (so they contract as well once inlined): the pragma keeps both operations
// of THIS function uncontracted, which is what a host float32 `c + g * n` (two separately rounded ops) computes.
__device__ __forceinline__ float mix_sample(float c, float g, float n) {
#pragma clang fp contract(off)
    const float gn = g * n;
    return c + gn;
}

struct NoiseDraw {                                            // one item's noise recording, start and gain
    const float* nz;
    unsigned len_n, start;
    float g;
    bool ok;
};

__device__ __forceinline__ NoiseDraw noise_draw(const float* __restrict__ noise, const long* __restrict__ noff, int n_noise, int rec,
                                                int nstart, float g) {
    NoiseDraw d{noise, 1u, 0u, 0.f, false};
    if (rec < 0 || rec >= n_noise) return d;
    const long base = noff[rec], len = noff[rec + 1] - base;
    const bool finite = (__float_as_uint(g) & 0x7f800000u) != 0x7f800000u;
    if (len < 1 || len > 0x7fffffffL || nstart < 0 || nstart >= len || !finite) return d;
    return NoiseDraw{noise + base, (unsigned)len, (unsigned)nstart, g, true};
}

// floor(2^32 / len_n), saturated (len_n = 1): the multiplier of noise_at, one 64-bit division per thread
__device__ __forceinline__ unsigned wrap_magic(unsigned len_n) {
    const unsigned long m = (1ul << 32) / len_n;
    return m > 0xfffffffful ? 0xffffffffu : (unsigned)m;
}

// (phase + q) mod len_n for phase < len_n < 2^31 and q < 2^31, without a division: with m = wrap_magic(len_n),
// u / len_n - 1 < u m / 2^32 <= u / len_n for every u < 2^32, so the high product is the quotient or one less and one conditional
// subtraction finishes the remainder (< 2 len_n < 2^32) — however often a short noise recording wraps inside the crop.
__device__ __forceinline__ unsigned noise_at(unsigned phase, unsigned q, unsigned len_n, unsigned magic) {
    const unsigned u = phase + q;
    unsigned r = u - __umulhi(u, magic) * len_n;
    if (r >= len_n) r -= len_n;
    return r;
}

// x float[total], recording i = [offsets[i], offsets[i + 1]) -> out double[n]; grid n
__global__ __launch_bounds__(256) void signal_power_ragged_kernel(const float* __restrict__ x, const long* __restrict__ offsets,
                                                                  long total, double* __restrict__ out) {
    __shared__ double red[256];
    long first;
    const long len = dcs_ragged::rec_span(offsets, blockIdx.x, total, &first);
    double acc = 0.0;
    for (long j = threadIdx.x; j < len; j += 256) {
        const double v = (double)x[first + j];
        acc = fma(v, v, acc);                                // v * v is exact in fp64: one rounding per addition either way
    }
    const double sum = dcs_ragged::block_sum(acc, red);
    if (threadIdx.x == 0) out[blockIdx.x] = len > 0 ? sum / (double)len : 0.0;
}

// clean float[total] with offsets[n_items + 1] -> noisy float[total]; per item a noise recording, start and gain
__global__ __launch_bounds__(256) void audio_mix_ragged_kernel(const float* __restrict__ clean, const long* __restrict__ off,
                                                               int n_items, long total, const float* __restrict__ noise,
                                                               const long* __restrict__ noff, int n_noise,
                                                               const int* __restrict__ noise_idx, const int* __restrict__ noise_start,
                                                               const float* __restrict__ gain, float* __restrict__ noisy) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int lo = dcs_ragged::owner(off, n_items, g);       // off[0] <= g is the caller's invariant; q >= 0 is tested below
    const float c = clean[g];
    const long q = g - off[lo];
    const NoiseDraw d = noise_draw(noise, noff, n_noise, noise_idx[lo], noise_start[lo], gain[lo]);
    float y = c;
    if (d.ok && q >= 0) y = mix_sample(c, d.g, d.nz[(unsigned)(((long)d.start + q) % (long)d.len_n)]);
    noisy[g] = y;
}

// the mixing store's samples: clean from the utterance, noisy by the mixture rule, both zero past the utterance's end
struct MixSource {
    const float* cs;
    const float* nz;
    long len;
    int start;
    unsigned len_n, phase, magic;                            // phase = (noise start + crop start) mod len_n; wrap_magic(len_n)
    float g;
    __device__ __forceinline__ void load(int q, bool want_noisy, float& c, float& y) const {
        const long p = (long)start + q;
        c = 0.f;
        y = 0.f;
        if (p < len) {
            c = cs[p];
            if (want_noisy) y = mix_sample(c, g, nz[noise_at(phase, (unsigned)q, len_n, magic)]);
        }
    }
};

// grid (ceil(T / kFrames), B); outputs complex[B][256][T]
__global__ __launch_bounds__(256) void audio_mix_stft_batch_kernel(
    const float* __restrict__ clean, const long* __restrict__ off, int n_items, const float* __restrict__ noise,
    const long* __restrict__ noff, int n_noise, const int* __restrict__ item_idx, const int* __restrict__ item_start,
    const int* __restrict__ noise_idx, const int* __restrict__ noise_start, const float* __restrict__ gain,
    const float* __restrict__ w, float2* __restrict__ out_noise, float2* __restrict__ out_noisy, float2* __restrict__ out_clean, int T,
    int hop, int L, float scale) {
    const int b = blockIdx.y, start = item_start[b];
    long base, len;
    bool ok = crop_of_item(off, n_items, item_idx[b], start, L, &base, &len);
    const NoiseDraw d = noise_draw(noise, noff, n_noise, noise_idx[b], noise_start[b], gain[b]);
    ok = ok && d.ok;                                         // (every term is per item: uniform over the workgroup)
    const unsigned phase = ok ? (unsigned)(((long)d.start + (long)start) % (long)d.len_n) : 0u;
    stft_batch_body(MixSource{clean + base, d.nz, len, start, d.len_n, phase, wrap_magic(d.len_n), d.g}, ok, w, out_noise,
                    out_noisy, out_clean, T, hop, L, scale);
}

}  // namespace

extern "C" int dcs_signal_power_ragged_f64(const float* x, const long* offsets, int n, long total, double* out,
                                           dcs_stream_t stream) {
    if (!x || !offsets || !out || n <= 0 || total < 0 || total > dcs_ragged::kMaxTotal) return DCS_ERR_BADARG;
    DCS_LAUNCH(signal_power_ragged_kernel, dim3((unsigned)n), dim3(256), 0, dcs_stream(stream), x, offsets, total, out);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}

extern "C" int dcs_audio_mix_ragged_f32(const float* clean, const long* offsets, int n_items, long total, const float* noise,
                                        const long* noise_offsets, int n_noise, const int* noise_index, const int* noise_start,
                                        const float* gain, float* noisy, dcs_stream_t stream) {
    if (!clean || !offsets || !noise || !noise_offsets || !noise_index || !noise_start || !gain || !noisy || n_items <= 0 ||
        n_noise <= 0 || total < 0 || (total + 255) / 256 > 0x7fffffffL)
        return DCS_ERR_BADARG;
    if (total == 0) return DCS_OK;
    DCS_LAUNCH(audio_mix_ragged_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, dcs_stream(stream), clean, offsets,
               n_items, total, noise, noise_offsets, n_noise, noise_index, noise_start, gain, noisy);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}

extern "C" int dcs_audio_mix_stft_batch_f32(const float* clean, const long* offsets, int n_items, const float* noise,
                                            const long* noise_offsets, int n_noise, const int* item_index, const int* item_start,
                                            const int* noise_index, const int* noise_start, const float* gain, int B,
                                            const float* window, int n_fft, int T, int hop, float scale, float* out_noise,
                                            float* out_noisy, float* out_clean, dcs_stream_t stream) {
    if (!clean || !offsets || !noise || !noise_offsets || !item_index || !item_start || !noise_index || !noise_start || !gain ||
        !window || !out_noise || !out_noisy || !out_clean || n_items <= 0 || n_noise <= 0 || B <= 0 || B > 65535 || n_fft != N ||
        T < 2 || hop <= 0)
        return DCS_ERR_BADARG;
    const long L = (long)hop * (T - 1);
    if (L <= N / 2 || L > 0x7fffffffL - N) return DCS_ERR_BADARG;      // one reflection reaches every padded index
    DCS_LAUNCH(audio_mix_stft_batch_kernel, dim3((unsigned)((T + kFrames - 1) / kFrames), B), dim3(256), 0, dcs_stream(stream), clean,
               offsets, n_items, noise, noise_offsets, n_noise, item_index, item_start, noise_index, noise_start, gain, window,
               (float2*)out_noise, (float2*)out_noisy, (float2*)out_clean, T, hop, (int)L, scale);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}
