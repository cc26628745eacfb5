// snapshot.hip — the checkpoint snapshot: every tensor a graph replay rewrites (the bucket's parameters and Adam moments, the SWA
// average, ~45 small running-statistics buffers, the device counters) gathered bit for bit into ONE staging slab by ONE
// launch, between two replays, without a host synchronisation.  One copy_ per tensor would put ~50 dependent kernel boundaries
// on the step's stream; this is one, HBM-bound (one stream in, one out).  The same pass counts non-finite words per tensor, so
// a checkpoint that holds NaN weights is known as such before anything is written (dcsnet/checkpoint.py).
//
// The item table and the cumulative workgroup table are DEVICE memory: the host entry point reads neither.  What can only be
// known from the table is checked where it is read: an item that breaks a rule of include/dcsnet_hip.h is not copied at all.
#include "ragged_common.h"                                   // owner(): which item a block of the cumulative table belongs to

namespace {
constexpr int kThreads = 256;
constexpr long kBlockWords = DCS_SNAPSHOT_BLOCK_WORDS;
static_assert(kBlockWords == 4 * kThreads, "one 16-byte access per thread and workgroup");

__device__ __forceinline__ bool item_ok(const dcs_snapshot_item& it, long dst_words) {
    return it.src != nullptr && !((uintptr_t)it.src & 3) && it.words >= 0 && it.dst_word >= 0 && !(it.dst_word & 3) &&
           it.words <= dst_words && it.dst_word <= dst_words - it.words;
}
__device__ __forceinline__ int nonfinite_word(uint32_t w) { return (w & 0x7F800000u) == 0x7F800000u; }

// A source address comes out of the table as a generic pointer, which compiles to flat loads; every source is device global
// memory, so it is read through the global address space (global_load_dword / _dwordx4).
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) uint32_t* gsrc1_t;
typedef const __attribute__((address_space(1))) u32x4* gsrc4_t;

__global__ __launch_bounds__(kThreads) void snapshot_kernel(const dcs_snapshot_item* __restrict__ items, int n,
                                                            const long* __restrict__ first_block, uint32_t* __restrict__ dst,
                                                            long dst_words, int* __restrict__ nonfinite) {
    if (blockIdx.x == 0)                                       // a rule-breaking item is reported, never copied
        for (int i = threadIdx.x; i < n; i += kThreads)
            if (!item_ok(items[i], dst_words)) nonfinite[i] = -1;
    const long total = first_block[n];
    for (long vb = blockIdx.x; vb < total; vb += gridDim.x) {          // (uniform over the workgroup)
        const int lo = dcs_ragged::owner(first_block, n, vb);
        const dcs_snapshot_item it = items[lo];
        const long w0 = (vb - first_block[lo]) * kBlockWords + 4 * (long)threadIdx.x;
        // a table whose block counts disagree with its items leaves words uncopied; it cannot make an access leave src or dst
        const bool ok = item_ok(it, dst_words) && vb >= first_block[lo];
        const long left = ok ? it.words - w0 : 0;
        const gsrc1_t s = (gsrc1_t)(uintptr_t)it.src + w0;
        uint32_t* d = dst + it.dst_word + w0;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (left >= 4) {
            if (!((uintptr_t)it.src & 15)) {
                const u32x4 q = *(gsrc4_t)s;
                v = make_uint4(q.x, q.y, q.z, q.w);
            } else {                                             // (a view 4 or 8 bytes past a 16-byte boundary)
                v.x = s[0]; v.y = s[1]; v.z = s[2]; v.w = s[3];
            }
            *reinterpret_cast<uint4*>(d) = v;                    // dst 16-byte aligned, dst_word and w0 multiples of 4
        } else if (left > 0) {                                   // the item's last words % 4
            v.x = s[0]; d[0] = v.x;
            if (left > 1) { v.y = s[1]; d[1] = v.y; }
            if (left > 2) { v.z = s[2]; d[2] = v.z; }
        }
        if (it.is_f32) {                                         // (uniform: one item per workgroup and pass)
            const bool a = left > 0, b = left > 1, c = left > 2, e = left > 3;
            const int cnt = __popcll(__ballot(a && nonfinite_word(v.x))) + __popcll(__ballot(b && nonfinite_word(v.y))) +
                            __popcll(__ballot(c && nonfinite_word(v.z))) + __popcll(__ballot(e && nonfinite_word(v.w)));
            if (cnt && (threadIdx.x & (DCS_WAVE - 1)) == 0) atomicAdd(nonfinite + lo, cnt);
        }
    }
}
}  // namespace

extern "C" int dcs_snapshot_words(const dcs_snapshot_item* items, int n, const long* first_block, void* dst, long dst_words,
                                  int* nonfinite, dcs_stream_t stream) {
    if (!items || !first_block || !dst || !nonfinite || n < 1 || n > 1024 || dst_words < 0) return DCS_ERR_BADARG;
    if ((uintptr_t)dst & 15) return DCS_ERR_BADARG;
    hipStream_t st = dcs_stream(stream);
    if (hipMemsetAsync(nonfinite, 0, sizeof(int) * (size_t)n, st) != hipSuccess) return DCS_ERR_LAUNCH;
    DCS_LAUNCH(snapshot_kernel, dim3(DCS_SNAPSHOT_GRID), dim3(kThreads), 0, st, items, n, first_block, (uint32_t*)dst, dst_words,
               nonfinite);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}
