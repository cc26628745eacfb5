// ragged_frames.h — the skeleton of a measure that is defined per frame and averaged per recording (frame_measures.hip,
// spectral_measures.hip), on top of ragged_common.h.  A source of this family owns its per-frame mathematics, its frame
// kernel and the means and NaN rules of its recording kernel; everything else is here:
//
//   framing     at rate fs (8000 .. 48000): N = round(0.03 fs) samples, hop S = N / 4, F = (L - N) / S frames for
//               L >= N + S (else 0), frame k at k S
//   workspace   frame base long[n + 1] | vals double[planes][Fcap] | valid int[Fcap], Fcap = total / S >= the frames of all
//               recordings together: it follows the total length, and the frame kernel's grid is Fcap (< 2^31) workgroups
//   launches    frame_slots_begin: the checks both entry points make and ragged_prefix_kernel<PrefixFrameSlots> (one workgroup:
//               fbase[i] = the frames of the recordings before i, clamped to Fcap); then the source's own frame kernel, whose
//               workgroup g takes its samples from frame_slot; then its recording kernel, one workgroup of 256 per recording
//               around trimmed_means
#pragma once
#include "ragged_common.h"

namespace dcs_ragged {

constexpr int kMinRate = 8000, kMaxRate = 48000;
inline bool bad_rate(int fs) { return fs < kMinRate || fs > kMaxRate; }

struct FrameGeometry {
    int N, S;
};
inline FrameGeometry frame_geometry(int fs) {
    FrameGeometry g;
    g.N = (3 * fs + 50) / 100;                                // round(0.03 fs)
    g.S = g.N / 4;
    return g;
}

struct PrefixFrameSlots {                                     // v = (L - N) / S for L >= N + S
    long N, S;
    __device__ __forceinline__ long operator()(long L) const { return L >= N + S ? (L - N) / S : 0; }
};

struct FrameLayout {
    long Fcap, off_vals, off_valid, bytes;
    long* fbase;                                              // set by carve(): the three sections of the caller's workspace
    double* vals;
    int* valid;
    void carve(void* workspace) {
        char* ws = static_cast<char*>(workspace);
        fbase = reinterpret_cast<long*>(ws);
        vals = reinterpret_cast<double*>(ws + off_vals);
        valid = reinterpret_cast<int*>(ws + off_valid);
    }
};
inline FrameLayout layout(long n, long total, int S, int planes) {
    FrameLayout s{};
    s.Fcap = total / S;
    s.off_vals = align256((n + 1) * (long)sizeof(long));
    s.off_valid = s.off_vals + align256(planes * s.Fcap * (long)sizeof(double));
    s.bytes = s.off_valid + align256(s.Fcap * (long)sizeof(int));
    return s;
}

// dcs_*_measures_ragged_workspace_bytes
inline long frame_workspace_bytes(int n, long total, int fs, int planes) {
    if (n <= 0 || n > kMaxRecordings || total < 0 || total > kMaxTotal || bad_rate(fs)) return DCS_ERR_BADARG;
    const FrameLayout s = layout(n, total, frame_geometry(fs).S, planes);
    if (s.Fcap > 0x7fffffffL) return DCS_ERR_BADARG;          // one workgroup per frame slot
    return s.bytes;
}

// The head of an entry point, after the checks of what only that entry point takes (all of them DCS_ERR_BADARG): the shared
// argument checks, the layout, its limits and its pointers into the workspace, and the prefix launch -> s->fbase on *st.  The
// caller launches its frame kernel (when s->Fcap > 0) and its recording kernel.
inline int frame_slots_begin(const float* clean, const float* est, const long* offsets, int n, long total, int fs,
                             const double* window, int window_len, int planes, void* workspace, long workspace_bytes,
                             dcs_stream_t stream, FrameGeometry* g, FrameLayout* s, hipStream_t* st) {
    if (bad_ragged(offsets, n, total) || bad_rate(fs) || !window || !workspace || (total > 0 && (!clean || !est)))
        return DCS_ERR_BADARG;
    *g = frame_geometry(fs);
    *s = layout(n, total, g->S, planes);
    if (window_len != g->N || s->Fcap > 0x7fffffffL) return DCS_ERR_BADARG;
    if (workspace_bytes < s->bytes) return DCS_ERR_WORKSPACE;
    s->carve(workspace);
    *st = dcs_stream(stream);
    DCS_LAUNCH(ragged_prefix_kernel<PrefixFrameSlots>, dim3(1), dim3(256), 0, *st, offsets, n, total,
               PrefixFrameSlots{g->N, g->S}, s->Fcap, s->fbase);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}

// Frame slot g (one workgroup each, g = blockIdx.x < Fcap) -> false when no recording has a frame there (uniform over the
// workgroup; fbase[n] <= Fcap); else *base = its first sample in the flat buffers.  In its recording rec it is frame
// k = g - fbase[rec] < fbase[rec + 1] - fbase[rec] <= (L - N) / S: its N samples end before the recording's.
__device__ __forceinline__ bool frame_slot(const long* __restrict__ offsets, int n, long total, const long* __restrict__ fbase,
                                           long g, int S, long* base) {
    if (g >= fbase[n]) return false;
    const int rec = owner(fbase, n, g);
    long first;
    rec_span(offsets, rec, total, &first);
    *base = first + (g - fbase[rec]) * S;
    return true;
}

// Per recording, for a workgroup of 256: the mean of the K smallest of the F >= 1 frame values v[m plane + i], i < F, of each
// of M (1 or 2) measures — those with ok[i] != 0 when MASKED (then 1 <= K <= their number; else ok is not read and
// 1 <= K <= F).  Values are non-negative doubles, so bit order = numeric order: the K-th smallest value t is found by binary
// radix selection on the bit patterns, one pass per bit from the top: among the values that share the bits found so far,
// count those whose next bit is 0 (all measures in one pass and one integer reduction, measure m's count in the 32-bit word
// m: F < 2^31).  Then mean = (sum of the v < t + (K - #{v < t}) t) / K, thread t adding i = t, t + 256, ... in ascending
// order, then block_sum: no sort, ties handled.  Every thread returns the means in out.  red: LDS double[256], red4: LDS [4].
template <int M, bool MASKED>
__device__ __forceinline__ void trimmed_means(const double* __restrict__ v, long plane, const int* __restrict__ ok, long F, long K,
                                              double* red, unsigned long long* red4, double (&out)[M]) {
    static_assert(M == 1 || M == 2, "one 32-bit word of the count per measure");
    const int t = threadIdx.x;
    const auto word = [](unsigned long long c, int m) { return M == 1 ? c : (m ? c >> 32 : c & 0xffffffffull); };
    unsigned long long p[M];
    long k[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        p[m] = 0;
        k[m] = K;
    }
    for (int bit = 62; bit >= 0; --bit) {
        unsigned long long c0 = 0;
        for (long i = t; i < F; i += 256) {
            if (MASKED && !ok[i]) continue;
#pragma unroll
            for (int m = 0; m < M; ++m)                      // the bits above `bit` agree and bit `bit` is 0 (p[m]'s still is)
                if ((magnitude_bits(v[m * plane + i]) >> bit) == (p[m] >> bit)) c0 += 1ull << (32 * m);
        }
        c0 = block_sum_ull(c0, red4);
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const long z = (long)word(c0, m);
            if (k[m] > z) {
                k[m] -= z;
                p[m] |= 1ull << bit;
            }
        }
    }
    double s[M];
#pragma unroll
    for (int m = 0; m < M; ++m) s[m] = 0.0;
    unsigned long long below = 0;
    for (long i = t; i < F; i += 256) {
        if (MASKED && !ok[i]) continue;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const double x = v[m * plane + i];
            if (magnitude_bits(x) < p[m]) {
                s[m] += x;
                below += 1ull << (32 * m);
            }
        }
    }
#pragma unroll
    for (int m = 0; m < M; ++m) s[m] = block_sum(s[m], red);
    below = block_sum_ull(below, red4);
#pragma unroll
    for (int m = 0; m < M; ++m)
        out[m] = (s[m] + (double)(K - (long)word(below, m)) * __longlong_as_double((long long)p[m])) / (double)K;
}

}  // namespace dcs_ragged
