// conv_epilogue.h — the tail every forward conv kernel ends with, defined once: the eval-mode ComplexBatchNorm2d map folded
// into the conv that feeds it (conv_common.h Args::coef, six floats {a0, a1, a2, a3, c0, c1} per channel) in its three
// register layouts, and the training-mode CBN sums of the un-biased output (Args::stat).  Bias add, activation, addressing
// and stores stay with the kernels.  Callers: cconv_mfma_kernel, cconv_mfma16_kernel, splitk_reduce_kernel,
// splitk_reduce_stats_kernel (conv_mfma.hip), cconv_ring_kernel (conv_ring.hip), both kernels of conv_enc0.hip,
// cconv_direct_body (conv_direct.hip), cbn_apply_kernel and cbn_apply_pool_kernel (cbn.hip).
#pragma once
#include "conv_common.h"

namespace conv {

// ---- the map ---------------------------------------------------------------------------------------------------------------
// (re, im) <- (a0 re + a1 im + c0, a2 re + a3 im + c1) as out = fma(a_re, re, fma(a_im, im, c)) per component.  THE association
// order of the library: the conv epilogues and cbn.hip's apply kernels all come here, so a conv with the map folded in and
// the same conv followed by dcs_cbn agree bit for bit (tests/test_infer_epilogue.py).
__device__ __forceinline__ float2 affine2(float re, float im, const float* q) {
    return make_float2(fmaf(q[0], re, fmaf(q[1], im, q[4])), fmaf(q[2], re, fmaf(q[3], im, q[5])));
}

// float4 form: a lane owns two complex channels (x, y) and (z, w), q[0..5] and q[6..11].
// SEP: scalar FMAs kept apart by empty asm statements.  Paired by the compiler into v_pk_fma_f32 with op_sel (low half =
// q1 * u.y + q4 taking the HIGH half of the {u.x, u.y} pair) the low half sporadically came out as q4 alone beside other
// workgroups' bf16 MFMAs (profiles/r03_pk_fma_op_sel_hazard.txt); the kernels that issue MFMAs keep the
// separators on top of the library-wide -fno-slp-vectorize (tests/test_host_cpu.py scans every kernel for the pairing).
// SEP = false: the streaming kernels (cbn.hip, splitk_reduce_kernel), whose schedule the separators would pin.
template <bool SEP = true>
__device__ __forceinline__ float4 affine4(float4 u, const float* q) {
    float4 v;
    v.x = fmaf(q[0], u.x, fmaf(q[1], u.y, q[4]));
    if (SEP) asm volatile("" : "+v"(v.x));
    v.y = fmaf(q[2], u.x, fmaf(q[3], u.y, q[5]));
    if (SEP) asm volatile("" : "+v"(v.y));
    v.z = fmaf(q[6], u.z, fmaf(q[7], u.w, q[10]));
    if (SEP) asm volatile("" : "+v"(v.z));
    v.w = fmaf(q[8], u.z, fmaf(q[9], u.w, q[11]));
    return v;
}

// the twelve coefficients of the two channels that own columns n0 .. n0 + 3 (n0 a multiple of 4)
__device__ __forceinline__ void load_affine4(const float* coef, int n0, float q[12]) {
#pragma unroll
    for (int e = 0; e < 12; ++e) q[e] = coef[6 * (n0 >> 1) + e];
}

// One-column form (16-column C/D maps: a lane owns ONE real column n, re of channel n / 2 if n is even, im if odd): the
// column's row of the 2x2 map, own term first; the partner column is the neighbouring lane (quad_perm [1,0,3,2]).
struct ColAffine { float c_re, c_im, c_add; };
__device__ __forceinline__ ColAffine load_col_affine(const float* coef, int n) {
    ColAffine ca = {1.f, 0.f, 0.f};                        // (no coef: identity, never applied)
    if (coef) {
        const float* q = coef + 6 * (n >> 1);
        if (n & 1) { ca.c_re = q[2]; ca.c_im = q[3]; ca.c_add = q[5]; } else { ca.c_re = q[0]; ca.c_im = q[1]; ca.c_add = q[4]; }
    }
    return ca;
}
// (applied where there is a map: `coef` is the pointer load_col_affine was given)
__device__ __forceinline__ float col_affine(const float* coef, float v, int n, const ColAffine& ca) {
    if (coef) {
        const float pv = dcs_dpp_term<0xB1, 0xf>(v);
        v = (n & 1) ? fmaf(ca.c_re, pv, fmaf(ca.c_im, v, ca.c_add)) : fmaf(ca.c_re, v, fmaf(ca.c_im, pv, ca.c_add));
    }
    return v;
}

// ---- CBN sums of the raw output -------------------------------------------------------------------------------------------
// {S_r, S_i, S_rr, S_ii, S_ri} of a lane's two channels, of the UN-biased value (pivot = bias); the caller's own predicate
__device__ __forceinline__ void stat10_add(float s[10], float4 v) {
    s[0] += v.x; s[1] += v.y;
    s[2] = fmaf(v.x, v.x, s[2]); s[3] = fmaf(v.y, v.y, s[3]); s[4] = fmaf(v.x, v.y, s[4]);
    s[5] += v.z; s[6] += v.w;
    s[7] = fmaf(v.z, v.z, s[7]); s[8] = fmaf(v.w, v.w, s[8]); s[9] = fmaf(v.z, v.w, s[9]);
}
// ... of a lane's one column: sum, sum of squares, sum of re * im (both columns of a channel accumulate the last)
__device__ __forceinline__ void col_stat_add(float st[3], float raw) {
    st[0] += raw; st[1] = fmaf(raw, raw, st[1]); st[2] = fmaf(raw, dcs_dpp_term<0xB1, 0xf>(raw), st[2]);
}
// One row of partial sums of a 256-thread workgroup of 16-column tiles (Cout = 8: 40 sums), row[t * stride]: column li of
// 4 row groups (lanes li + 16 g) x 4 waves — shuffles over the row groups, then LDS (red: 192 floats) over the waves.
// (conv_enc0.hip; cconv_mfma16_kernel keeps col_stat_add and this written out — as calls they cost it registers)
__device__ __forceinline__ void col_stat_rows_out(float st[3], float* red, float* row, int stride, int t, int lane, int wave,
                                                  int li) {
#pragma unroll
    for (int e = 0; e < 3; ++e) { st[e] += __shfl_xor(st[e], 16, 64); st[e] += __shfl_xor(st[e], 32, 64); }
    __syncthreads();                                        // every wave is done with what `red` held
    if (lane < 16) { red[(wave * 16 + li) * 3] = st[0]; red[(wave * 16 + li) * 3 + 1] = st[1]; red[(wave * 16 + li) * 3 + 2] = st[2]; }
    __syncthreads();
    if (t < 40) {                                           // channel c: {S_r, S_i, S_rr, S_ii, S_ri}
        const int c = t / 5, e = t % 5;
        const int colx = 2 * c + (e == 1 || e == 3), which = e < 2 ? 0 : (e < 4 ? 1 : 2);
        float sum = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) sum += red[(w * 16 + colx) * 3 + which];
        row[(long)t * stride] = sum;
    }
}
// 32-column tiles behind the transpose: lanes c4 + 8 r8 (c4 = lane & 7) hold the same two channels.  Sum a wave's ten lane
// sums over r8 through its own transpose tile tsm (>= 640 floats; in-order LDS, no barrier) into row `slot` of comb[][80]:
// [0..39] = {5 sums} x {8 column groups} of each group's first channel, [40..79] of its second.
__device__ __forceinline__ void tile_stat_reduce(const float s[10], float* tsm, float* comb, int slot, int lane, int c4) {
#pragma unroll
    for (int e = 0; e < 10; ++e) tsm[e * 64 + lane] = s[e];
    float r0 = 0.f, r1 = 0.f;
    const int k5 = lane >> 3;
    if (lane < 40) {
#pragma unroll
        for (int q8 = 0; q8 < 8; ++q8) {
            r0 += tsm[k5 * 64 + c4 + 8 * q8];
            r1 += tsm[(5 + k5) * 64 + c4 + 8 * q8];
        }
        comb[slot * 80 + lane] = r0;
        comb[slot * 80 + 40 + lane] = r1;
    }
}

}  // namespace conv
