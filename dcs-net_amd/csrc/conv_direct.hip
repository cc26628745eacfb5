// conv_direct.hip — direct (non-GEMM) complex correlation and its weight gradient: the kernels and their launchers
// (declared in conv_common.h).  The entry points, the routing among the conv kernels and the workspace contracts are
// conv_api.hip's.
//
// Forward use: enc0 (Cin=1, K=98: SURVEY.md §7 "small-channel ends"), dec6 (Cout=1), the 7x7 2->1
// spatial-attention conv (c_network.py:74), and the generic fallback for any geometry the MFMA
// implicit-GEMM kernel (conv_mfma.hip) does not take.  These stages are HBM-bound (SURVEY.md
// §8d): one haloed input tile per workgroup is staged in LDS (each input element is read from
// HBM once per tile), COB output channels per thread live in VGPRs, weights come through the
// scalar cache (wave-uniform addresses).
//
// The virtual input (nearest upsample of cat(x1, x2): c_network.py:214-216) is resolved in the
// LDS gather, so neither the concatenated nor the upsampled tensor ever exists in HBM.
//
// Backward (what autograd does for the reference through 4 real convs per complex conv):
//   data   g_X = conj(W) (*)^T g_Y : the SAME kernel run on g_Y with zero-insertion (stride) in the
//          gather and the flipped / conjugated / in-out-swapped weight (dcs_pack_conv_weight_bwd)
//   weight g_W[tap,ci,co] = sum_p g_Y[p,co] conj(X[p*s-pad+tap, ci]) : per-tile partial slabs
//          (no atomics: bitwise reproducible) + a reduce that writes the reference's parameter
//          layout (conv_r / conv_i or conv_tran_r / conv_tran_i, and the two biases).
// Also here: the block sum / channel split of a virtual-input gradient (upsample_cat_bwd_kernel).
#include "conv_common.h"
#include "conv_epilogue.h"
#include "wgrad_reduce.h"

namespace {

constexpr int TH = 16, TW = 16;      // output tile (pixels) per workgroup
constexpr int CHUNK = 8;             // input channels staged per LDS pass

using ConvArgs = conv::Args;
using conv::gather;

template <int COB>
__device__ __forceinline__ void cconv_direct_body(const ConvArgs& a, int tile_id, int co0, int b) {
    extern __shared__ __attribute__((aligned(16))) float2 tile[];   // [CHUNK][rows][colsp]
    const int t = threadIdx.x;
    const int tx = t % TW, ty = t / TW;
    const int oy0 = (tile_id / a.tiles_w) * TH, ox0 = (tile_id % a.tiles_w) * TW;
    const int Cin = a.C1 + a.C2;
    const int vy0 = oy0 * a.sf - a.pad_f, vx0 = ox0 * a.st - a.pad_t;

    float accr[COB], acci[COB];
#pragma unroll
    for (int i = 0; i < COB; ++i) { accr[i] = 0.f; acci[i] = 0.f; }

    for (int c0 = 0; c0 < Cin; c0 += CHUNK) {
        const int nc = min(CHUNK, Cin - c0);
        __syncthreads();                                   // previous pass finished reading
        const int total = a.rows * a.cols * nc;
        for (int idx = t; idx < total; idx += TH * TW) {
            const int ci = idx % nc;
            const int px = idx / nc;
            const int ix = px % a.cols, iy = px / a.cols;
            tile[ci * a.plane + iy * a.colsp + ix] = gather(a, b, vy0 + iy, vx0 + ix, c0 + ci);
        }
        __syncthreads();
        for (int ci = 0; ci < nc; ++ci) {
            const float2* pl = tile + ci * a.plane + (ty * a.sf) * a.colsp + tx * a.st;
            for (int dy = 0; dy < a.kh; ++dy) {
                for (int dx = 0; dx < a.kw; ++dx) {
                    const float2 xv = pl[dy * a.colsp + dx];
                    const float2* w = a.wp + ((long)(dy * a.kw + dx) * Cin + (c0 + ci)) * a.Cout + co0;
#pragma unroll
                    for (int i = 0; i < COB; ++i) {
                        const float2 wv = w[i];
                        accr[i] = fmaf(wv.x, xv.x, accr[i]);
                        accr[i] = fmaf(-wv.y, xv.y, accr[i]);
                        acci[i] = fmaf(wv.x, xv.y, acci[i]);
                        acci[i] = fmaf(wv.y, xv.x, acci[i]);
                    }
                }
            }
        }
    }
    const int oy = oy0 + ty, ox = ox0 + tx;
    if (oy < a.Hout && ox < a.Wout) {
        act2_t* out = a.y + (((long)b * a.Hout + oy) * a.Wout + ox) * a.Cout + co0;
#pragma unroll
        for (int i = 0; i < COB; ++i) {
            const float2 bv = a.bias ? a.bias[co0 + i] : make_float2(0.f, 0.f);
            float vr = accr[i] + bv.x, vi = acci[i] + bv.y;
            if (a.coef) {                                  // folded eval-mode CBN
                const float2 u = conv::affine2(vr, vi, a.coef + 6 * (co0 + i));
                vr = u.x; vi = u.y;
            }
            conv::stc(out + i, make_float2(dcs_act(vr, a.act), dcs_act(vi, a.act)));
        }
    }
}

template <int COB>
__global__ __launch_bounds__(TH * TW) void cconv_direct_kernel(ConvArgs a) {
    cconv_direct_body<COB>(a, blockIdx.x, blockIdx.y * COB, blockIdx.z);
}

// several problems whose Cout == COB (one output-channel block each) in one launch: problem = blockIdx.y
constexpr int kDirectBatch = 8;
struct DirectTable { ConvArgs p[kDirectBatch]; };

template <int COB>
__global__ __launch_bounds__(TH * TW) void cconv_direct_multi_kernel(DirectTable t) {
    const ConvArgs& a = t.p[blockIdx.y];
    if ((int)blockIdx.x >= a.tiles_w * a.tiles_h) return;
    cconv_direct_body<COB>(a, blockIdx.x, 0, blockIdx.z);
}

// ---- weight gradient ---------------------------------------------------------------------------
constexpr int WG_CO = 8;             // output channels per workgroup (g_Y tile columns)
constexpr int WG_TAPS = 13;          // taps per thread: ceil(49 / 4) covers k = 7

struct WgradArgs {
    const act2_t* x1; const act2_t* x2; const act2_t* gy; float2* slab_w; float2* slab_b;
    int n_slabs, total_tiles, n_co_chunks;
    ConvArgs c;                      // forward geometry (y/wp/bias unused)
};

// grid: (n_slabs, ci_chunks * co_chunks).  The (tap, ci, co) outputs of the workgroup's chunk pair are
// flattened over the 256 threads (<= WG_TAPS each), so the small-channel layers this kernel serves
// (enc0: 49x1x8, dec6: 9x16x1, the 7x7 2->1 attention convs: 49x2x1) keep most lanes busy.
template <int SLOTS>
__global__ __launch_bounds__(TH * TW) void cconv_wgrad_kernel(WgradArgs w) {
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    const ConvArgs& a = w.c;
    float2* tile = lds;                                   // [CHUNK][plane]
    float2* gt = lds + CHUNK * a.plane;                   // [TH*TW][WG_CO]
    const int t = threadIdx.x;
    const int ci0 = (blockIdx.y / w.n_co_chunks) * CHUNK, co0 = (blockIdx.y % w.n_co_chunks) * WG_CO;
    const int Cin = a.C1 + a.C2;
    const int ntaps = a.kh * a.kw;
    const int tiles_per_img = a.tiles_w * a.tiles_h;
    const int nc = min(CHUNK, Cin - ci0), nco = min(WG_CO, a.Cout - co0);
    const int per_tap = nc * nco, n_out = ntaps * per_tap;

    // few outputs (Cout = 1 layers: 72..98): Q thread groups take every Q-th pixel of a tile each and are
    // combined through LDS once, after the last tile, so all 256 lanes work
    int Q = 1, q = 0, o0 = t;
    if (SLOTS == 1 && 2 * n_out <= TH * TW) {
        Q = (TH * TW) / n_out;
        q = t / n_out;
        o0 = q < Q ? t % n_out : n_out;                   // lanes beyond Q * n_out stay idle
    }

    float accr[SLOTS], acci[SLOTS];
    int xoff[SLOTS], goff[SLOTS];
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
        accr[i] = 0.f; acci[i] = 0.f;
        const int o = o0 + TH * TW * i;
        const int tap = o < n_out ? o / per_tap : 0, r = o < n_out ? o % per_tap : 0;
        xoff[i] = (r / nco) * a.plane + (tap / a.kw) * a.colsp + (tap % a.kw);
        goff[i] = r % nco;
    }
    float br = 0.f, bi = 0.f;

    for (int tl = blockIdx.x; tl < w.total_tiles; tl += w.n_slabs) {
        const int b = tl / tiles_per_img, tile_id = tl % tiles_per_img;
        const int oy0 = (tile_id / a.tiles_w) * TH, ox0 = (tile_id % a.tiles_w) * TW;
        const int vy0 = oy0 * a.sf - a.pad_f, vx0 = ox0 * a.st - a.pad_t;
        __syncthreads();
        const int total = a.rows * a.cols * nc;
        for (int idx = t; idx < total; idx += TH * TW) {
            const int ci = idx % nc, px = idx / nc;
            const int ix = px % a.cols, iy = px / a.cols;
            tile[ci * a.plane + iy * a.colsp + ix] = gather(a, b, vy0 + iy, vx0 + ix, ci0 + ci);
        }
        for (int idx = t; idx < TH * TW * WG_CO; idx += TH * TW) {
            const int co = idx % WG_CO, p = idx / WG_CO;
            const int oy = oy0 + p / TW, ox = ox0 + p % TW;
            float2 v = make_float2(0.f, 0.f);
            if (oy < a.Hout && ox < a.Wout && co0 + co < a.Cout)
                v = conv::ldc(w.gy + (((long)b * a.Hout + oy) * a.Wout + ox) * a.Cout + co0 + co);
            gt[p * WG_CO + co] = v;
        }
        __syncthreads();
#pragma unroll 4
        for (int p = q; p < TH * TW; p += Q) {
            const int base = ((p / TW) * a.sf) * a.colsp + (p % TW) * a.st;
#pragma unroll
            for (int i = 0; i < SLOTS; ++i) {
                if (o0 + TH * TW * i < n_out) {
                    const float2 g = gt[p * WG_CO + goff[i]];
                    const float2 xv = tile[xoff[i] + base];
                    // g * conj(x)
                    accr[i] = fmaf(g.x, xv.x, accr[i]);
                    accr[i] = fmaf(g.y, xv.y, accr[i]);
                    acci[i] = fmaf(g.y, xv.x, acci[i]);
                    acci[i] = fmaf(-g.x, xv.y, acci[i]);
                }
            }
        }
        if (ci0 == 0 && t < WG_CO) {                      // bias: column sums of g_Y, once per co chunk
            for (int p = 0; p < TH * TW; ++p) {
                const float2 g = gt[p * WG_CO + t];
                br += g.x; bi += g.y;
            }
        }
    }
    const long wsz = (long)ntaps * Cin * a.Cout;
    if (Q > 1) {                                          // combine the pixel shares (SLOTS == 1 here)
        __syncthreads();
        if (o0 < n_out) lds[q * n_out + o0] = make_float2(accr[0], acci[0]);
        __syncthreads();
        if (q == 0) {
            for (int k = 1; k < Q; ++k) { const float2 v = lds[k * n_out + o0]; accr[0] += v.x; acci[0] += v.y; }
        } else {
            o0 = n_out;                                   // only group 0 writes the slab
        }
    }
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
        const int o = o0 + TH * TW * i;
        if (o < n_out) {
            const int tap = o / per_tap, r = o % per_tap;
            w.slab_w[(long)blockIdx.x * wsz + ((long)tap * Cin + ci0 + r / nco) * a.Cout + co0 + r % nco] =
                make_float2(accr[i], acci[i]);
        }
    }
    if (ci0 == 0 && t < WG_CO && co0 + t < a.Cout) w.slab_b[(long)blockIdx.x * a.Cout + co0 + t] = make_float2(br, bi);
}

// g_x1[b][y][x][c] = sum over the up_f x up_t block of g_Xv[b][..][..][c]; channels >= C1 go to g_x2
__global__ void upsample_cat_bwd_kernel(const act2_t* __restrict__ gxv, act2_t* __restrict__ gx1,
                                        act2_t* __restrict__ gx2, int B, int Hin, int Win, int C1, int C2, int up_f,
                                        int up_t) {
    const int C = C1 + C2;
    const long n = (long)B * Hin * Win * C;
    const int Wv = Win * up_t, Hv = Hin * up_f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        long p = i / C;
        const int x = (int)(p % Win); p /= Win;
        const int y = (int)(p % Hin);
        const int b = (int)(p / Hin);
        float sr = 0.f, si = 0.f;
        for (int dy = 0; dy < up_f; ++dy)
            for (int dx = 0; dx < up_t; ++dx) {
                const float2 v = conv::ldc(gxv + (((long)b * Hv + y * up_f + dy) * Wv + x * up_t + dx) * C + c);
                sr += v.x; si += v.y;
            }
        const long sp = ((long)b * Hin + y) * Win + x;
        if (c < C1) conv::stc(gx1 + sp * C1 + c, make_float2(sr, si));
        else        conv::stc(gx2 + sp * C2 + (c - C1), make_float2(sr, si));
    }
}

bool conv_geometry(ConvArgs& a) {
    if (a.Hout <= 0 || a.Wout <= 0) return false;
    a.tiles_w = (a.Wout + TW - 1) / TW;
    a.tiles_h = (a.Hout + TH - 1) / TH;
    a.rows = (TH - 1) * a.sf + a.kh;
    a.cols = (TW - 1) * a.st + a.kw;
    a.colsp = a.cols | 1;                       // odd row pitch (in float2) spreads LDS banks
    a.plane = a.rows * a.colsp + 1;
    return true;
}

// n plain correlations with the same batch size and Cout in {1, 2} (the spatial-attention convs and their data
// gradients) as one launch; `a`: geometry with Hout / Wout set (tiling is filled in here)
int launch_direct_multi(ConvArgs* a, int n, hipStream_t stream) {
    if (n < 1 || n > kDirectBatch) return DCS_ERR_BADARG;
    if (dcs_conv_k7_ok(a, n)) return dcs_conv_k7_launch(a, n, stream);          // the attention convs: conv_k7.hip
    DirectTable t;
    size_t lds = 0;
    int tiles = 0;
    const int cob = a[0].Cout;
    for (int i = 0; i < n; ++i) {
        if (!conv_geometry(a[i]) || a[i].Cout != cob || a[i].B != a[0].B || (cob != 1 && cob != 2)) return DCS_ERR_BADARG;
        const int Cin = a[i].C1 + a[i].C2;
        const size_t l = (size_t)(Cin < CHUNK ? Cin : CHUNK) * a[i].plane * sizeof(float2);
        lds = l > lds ? l : lds;
        tiles = a[i].tiles_w * a[i].tiles_h > tiles ? a[i].tiles_w * a[i].tiles_h : tiles;
        t.p[i] = a[i];
    }
    if (lds > 64 * 1024 || a[0].B > 65535) return DCS_ERR_BADARG;
    dim3 grid(tiles, n, a[0].B);
    if (cob == 1) DCS_LAUNCH(cconv_direct_multi_kernel<1>, grid, dim3(TH * TW), lds, stream, t);
    else DCS_LAUNCH(cconv_direct_multi_kernel<2>, grid, dim3(TH * TW), lds, stream, t);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}

}  // namespace

int dcs_conv_direct_launch(ConvArgs& a, hipStream_t stream) {
    if (!DCS_ACT_IS_BF16 && dcs_conv_k7_ok(&a, 1)) return dcs_conv_k7_launch(&a, 1, stream);        // the attention convs: conv_k7.hip (fp32 maps)
    if (dcs_conv_enc0_ok(a)) return dcs_conv_enc0_launch(a, stream);            // the first encoder conv: conv_enc0.hip
    if (!conv_geometry(a)) return DCS_ERR_BADARG;
    const int Cin = a.C1 + a.C2;
    const size_t lds = (size_t)(Cin < CHUNK ? Cin : CHUNK) * a.plane * sizeof(float2);
    if (lds > 150 * 1024) return DCS_ERR_BADARG;
    const int Cout = a.Cout;
    int cob = (Cout % 8 == 0) ? 8 : (Cout % 4 == 0) ? 4 : (Cout % 2 == 0) ? 2 : 1;
    if (lds > 64 * 1024) {   // above the default dynamic-LDS limit: raise it for this instantiation
        const void* fn = cob == 8 ? (const void*)cconv_direct_kernel<8> : cob == 4 ? (const void*)cconv_direct_kernel<4>
                       : cob == 2 ? (const void*)cconv_direct_kernel<2> : (const void*)cconv_direct_kernel<1>;
        if (dcs_ensure_dynamic_lds(fn, lds) != hipSuccess) return DCS_ERR_LAUNCH;
    }
    dim3 grid(a.tiles_w * a.tiles_h, Cout / cob, a.B);
    if (grid.y > 65535 || grid.z > 65535) return DCS_ERR_BADARG;
    switch (cob) {
        case 8: DCS_LAUNCH(cconv_direct_kernel<8>, grid, dim3(TH * TW), lds, stream, a); break;
        case 4: DCS_LAUNCH(cconv_direct_kernel<4>, grid, dim3(TH * TW), lds, stream, a); break;
        case 2: DCS_LAUNCH(cconv_direct_kernel<2>, grid, dim3(TH * TW), lds, stream, a); break;
        default: DCS_LAUNCH(cconv_direct_kernel<1>, grid, dim3(TH * TW), lds, stream, a); break;
    }
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}

// a: forward geometry with x1 / x2 and the tiling set; slab_w float2[n_slabs][taps][Cin][Cout], slab_b float2[n_slabs][Cout]
int dcs_conv_direct_wgrad_launch(const ConvArgs& a, const act_t* gy, float2* slab_w, float2* slab_b, int n_slabs, float* gw_r,
                                 float* gw_i, float* gb_r, float* gb_i, int transposed, hipStream_t s) {
    static_assert(4 * WG_TAPS == conv::kWgradMaxTaps, "the widest instance covers the taps the entry point admits");
    WgradArgs w{};
    w.c = a;
    w.x1 = a.x1; w.x2 = a.x2; w.gy = (const act2_t*)gy;
    w.slab_w = slab_w; w.slab_b = slab_b; w.n_slabs = n_slabs;
    w.total_tiles = a.tiles_w * a.tiles_h * a.B;
    const int Cin = a.C1 + a.C2, Cout = a.Cout;
    const int n_ci = (Cin + CHUNK - 1) / CHUNK;
    w.n_co_chunks = (Cout + WG_CO - 1) / WG_CO;
    const size_t lds = ((size_t)CHUNK * w.c.plane + (size_t)TH * TW * WG_CO) * sizeof(float2);
    if (lds > 150 * 1024) return DCS_ERR_BADARG;
    // outputs per thread: taps * min(Cin,8) * min(Cout,8) spread over 256 threads
    const int n_out = a.kh * a.kw * (Cin < CHUNK ? Cin : CHUNK) * (Cout < WG_CO ? Cout : WG_CO);
    const int slots = (n_out + TH * TW - 1) / (TH * TW);
    auto fn = slots <= 1 ? cconv_wgrad_kernel<1> : slots <= 2 ? cconv_wgrad_kernel<2>
            : slots <= 4 ? cconv_wgrad_kernel<4> : cconv_wgrad_kernel<WG_TAPS>;
    if (dcs_ensure_dynamic_lds((const void*)fn, lds) != hipSuccess) return DCS_ERR_LAUNCH;
    dim3 grid(w.n_slabs, n_ci * w.n_co_chunks);
    if (grid.y > 65535) return DCS_ERR_BADARG;
    DCS_LAUNCH(fn, grid, dim3(TH * TW), lds, s, w);
    DCS_CHECK_LAUNCH();
    return dcs_conv_wgrad_reduce(slab_w, slab_b, n_slabs, gw_r, gw_i, gb_r, gb_i, Cout, Cin, a.kh, a.kw, transposed, s);
}

int dcs_upsample_cat_bwd_launch(const act_t* gxv, act_t* gx1, act_t* gx2, int B, int Hin, int Win, int C1, int C2, int up_f,
                                int up_t, hipStream_t s) {
    const long n = (long)B * Hin * Win * (C1 + C2);
    long nb = (n + 255) / 256;
    if (nb > 4096) nb = 4096;
    DCS_LAUNCH(upsample_cat_bwd_kernel, dim3((int)nb), dim3(256), 0, s, (const act2_t*)gxv, (act2_t*)gx1, (act2_t*)gx2, B, Hin,
               Win, C1, C2, up_f, up_t);
    DCS_CHECK_LAUNCH();
    return DCS_OK;
}

// the launchers that touch no activation: once, from the fp32 build
#ifndef DCS_ACT_BF16
bool dcs_conv_geometry(conv::Args& a) { return conv_geometry(a); }

int dcs_conv_direct_multi(conv::Args* a, int n, hipStream_t stream) { return launch_direct_multi(a, n, stream); }

// sum the slabs and scatter into the reference's parameter layout (wgrad_reduce.hip: immediate, or deferred + batched)
int dcs_conv_wgrad_reduce(const float2* slab_w, const float2* slab_b, int n_slabs, float* gw_r, float* gw_i, float* gb_r,
                          float* gb_i, int Cout, int Cin, int kh, int kw, int transposed, hipStream_t s) {
    wreduce::Job j{};
    j.slab_w = slab_w; j.slab_b = slab_b; j.gw_r = gw_r; j.gw_i = gw_i; j.gb_r = gb_r; j.gb_i = gb_i;
    j.n_slabs = n_slabs; j.Cout = Cout; j.Cin = Cin; j.kh = kh; j.kw = kw; j.transposed = transposed;
    return wreduce::emit(j, s);
}
#endif
