// conv_api.hip — host side of the conv family: every dcs_cconv2d_* / dcs_rconv2d_* / dcs_pack_conv_weight* /
// dcs_packed_weight* entry point, the routing among the kernels (conv_mfma, conv_enc0, conv_small, conv_k7,
// conv_wgrad_mfma, conv_wgrad_small, conv_direct) and the workspace contracts.  No kernel lives here.
//
// Every entry point fills one conv::Geom from its 14 integers and checks it with conv::geom_ok.  Forward, data
// gradient and weight gradient each have ONE launch description (FwdPlan, DgradPlan, WgradPlan) that the workspace
// query and the launch both read, so the two cannot disagree about a route, a slab count or an offset.
// Compiled in both builds (build.py: ACT_SOURCES); entry points without activations exist in the fp32 build only.
#include "conv_common.h"
#include "pack_jobs.h"

namespace {

using ConvArgs = conv::Args;
using conv::Geom;
using conv::align256;

// direct + MFMA panels of a (CoutRole, CinRole) weight
long base_floats(int CoutRole, int CinRole, int taps) {
    return conv::direct_floats(CoutRole, CinRole, taps) + conv::mfma_floats(CoutRole, CinRole, taps);
}

ConvArgs fwd_args(const void* x1, const void* x2, const Geom& g) {
    ConvArgs a{};
    a.x1 = (const act2_t*)x1; a.x2 = (const act2_t*)x2;
    a.B = g.B; a.Hin = g.Hin; a.Win = g.Win; a.C1 = g.C1; a.C2 = g.C2; a.up_f = g.up_f; a.up_t = g.up_t; a.zero_ins = 0;
    a.Cout = g.Cout; a.kh = g.kh; a.kw = g.kw; a.sf = g.sf; a.st = g.st; a.pad_f = g.pad_f; a.pad_t = g.pad_t;
    a.act = DCS_ACT_NONE;
    a.Hv = g.Hin * g.up_f; a.Wv = g.Win * g.up_t;
    a.Hout = (a.Hv + 2 * g.pad_f - g.kh) / g.sf + 1;
    a.Wout = (a.Wv + 2 * g.pad_t - g.kw) / g.st + 1;
    return a;
}

// a forward-shaped call: valid integers, x1 present, x2 present exactly when it has channels
bool fwd_geom_ok(const void* x1, const void* x2, const Geom& g) {
    return x1 && conv::geom_ok(g) && (g.C2 > 0) == (x2 != nullptr);
}

}  // namespace

#ifndef DCS_ACT_BF16
extern "C" int dcs_pack_conv_weight(const float* w_r, const float* w_i, const float* b_r, const float* b_i, float* wp,
                                    float* bias_out, int Cout, int Cin, int kh, int kw, int transposed, int up_f,
                                    int up_t, dcs_stream_t stream) {
    if (up_f < 1 || up_t < 1) return DCS_ERR_BADARG;
    if (!w_r || !w_i || !wp || !bias_out || Cout <= 0 || Cin <= 0 || kh <= 0 || kw <= 0) return DCS_ERR_BADARG;
    if ((b_r == nullptr) != (b_i == nullptr)) return DCS_ERR_BADARG;
    long n = (long)kh * kw * Cin * Cout;
    if (n < Cout) n = Cout;
    packjob::Job j{};
    j.kind = packjob::DIRECT;
    j.Cout = Cout; j.Cin = Cin; j.kh = kh; j.kw = kw; j.flag = transposed;
    j.total = n;
    j.dst_bytes = (long)kh * kw * Cin * Cout * (long)sizeof(float2);
    j.src0 = w_r; j.src1 = w_i; j.src2 = b_r; j.src3 = b_i;
    j.dst0 = wp; j.dst1 = bias_out;
    {
        const int rc = packjob::emit(j, dcs_stream(stream));
        if (rc != DCS_OK) return rc;
    }
    if (conv::mfma_ok(Cin, Cout)) {    // second panel: MFMA fragment order (conv_mfma.hip)
        const int rc = dcs_conv_mfma_pack(wp, wp + conv::direct_floats(Cout, Cin, kh * kw), Cout, Cin, kh * kw,
                                          dcs_stream(stream));
        if (rc != DCS_OK) return rc;
    }
    if (conv::fold_ok(Cin, Cout, kh, kw, 1, 1, 1, 1, up_f, up_t))   // third: per-parity folded sub-kernels (conv_pack.hip)
        return conv::pack_fold(wp, wp + base_floats(Cout, Cin, kh * kw), Cout, Cin, up_f, up_t, dcs_stream(stream));
    return DCS_OK;
}
#endif

#ifndef DCS_ACT_BF16
extern "C" long dcs_packed_weight_floats(int Cout, int Cin, int kh, int kw, int up_f, int up_t) {
    if (Cout <= 0 || Cin <= 0 || kh <= 0 || kw <= 0 || up_f < 1 || up_t < 1) return -1;
    long n = base_floats(Cout, Cin, kh * kw);
    if (conv::fold_ok(Cin, Cout, kh, kw, 1, 1, 1, 1, up_f, up_t)) n += conv::fold_floats(Cout, Cin, up_f, up_t);
    return n;
}
#endif

#ifndef DCS_ACT_BF16
extern "C" long dcs_packed_weight_bwd_floats(int Cout, int Cin, int kh, int kw, int sf, int st, int pad_f, int pad_t,
                                             int up_f, int up_t) {
    if (Cout <= 0 || Cin <= 0 || kh <= 0 || kw <= 0 || sf < 1 || st < 1 || up_f < 1 || up_t < 1) return -1;
    long n = base_floats(Cin, Cout, kh * kw);
    if (conv::fold_ok(Cin, Cout, kh, kw, sf, st, pad_f, pad_t, up_f, up_t)) n += conv::upfold_bwd_floats(Cout, Cin, up_f, up_t);
    else if (up_f * up_t == 1 && conv::stride_ok(Cin, Cout, kh, kw, sf, st, pad_f, pad_t))
        n += conv::stride_bwd_floats(Cout, Cin, kh, kw, sf, st, pad_f, pad_t);
    return n;
}
#endif

#ifndef DCS_ACT_BF16
extern "C" int dcs_pack_conv_weight_bwd(const float* wp, float* wp_bwd, int Cout, int Cin, int kh, int kw, int sf,
                                        int st, int pad_f, int pad_t, int up_f, int up_t, dcs_stream_t stream) {
    if (!wp || !wp_bwd || Cout <= 0 || Cin <= 0 || kh <= 0 || kw <= 0 || sf < 1 || st < 1 || up_f < 1 || up_t < 1)
        return DCS_ERR_BADARG;
    const long n = (long)kh * kw * Cin * Cout;
    hipStream_t s = dcs_stream(stream);
    packjob::Job j{};
    j.kind = packjob::BWD;
    j.Cout = Cout; j.Cin = Cin; j.kh = kh * kw;
    j.total = n;
    j.dst_bytes = n * (long)sizeof(float2);
    j.src0 = wp; j.dst0 = wp_bwd;
    {
        const int rc = packjob::emit(j, s);
        if (rc != DCS_OK) return rc;
    }
    // in the data-gradient GEMM the roles swap: K runs over the forward Cout, N over the forward Cin
    if (conv::mfma_ok(Cout, Cin)) {
        const int rc = dcs_conv_mfma_pack(wp_bwd, wp_bwd + conv::direct_floats(Cin, Cout, kh * kw), Cin, Cout, kh * kw, s);
        if (rc != DCS_OK) return rc;
    }
    float* extra = wp_bwd + base_floats(Cin, Cout, kh * kw);
    if (conv::fold_ok(Cin, Cout, kh, kw, sf, st, pad_f, pad_t, up_f, up_t))
        return conv::pack_upfold_bwd(wp, extra, Cout, Cin, up_f, up_t, s);
    if (up_f * up_t == 1 && conv::stride_ok(Cin, Cout, kh, kw, sf, st, pad_f, pad_t))
        return conv::pack_stride_bwd(wp_bwd, extra, Cout, Cin, kh, kw, sf, st, pad_f, pad_t, s);
    return DCS_OK;
}
#endif

// forward launch description shared by the workspace query and the launch itself
struct FwdPlan { ConvArgs a; int path, ncls, os_f, os_t; conv::Cls cls[4]; };   // path 0: folded classes, 1: plain MFMA, 2: direct

static FwdPlan fwd_plan(const void* x1, const void* x2, const Geom& g) {
    const auto [B, Hin, Win, C1, C2, up_f, up_t, Cout, kh, kw, sf, st, pad_f, pad_t] = g;
    FwdPlan p{};
    if (!(C1 & 1) && conv::fold_ok(C1 + C2, Cout, kh, kw, sf, st, pad_f, pad_t, up_f, up_t)) {
        // nearest upsample folded into per-parity sub-kernels on the SOURCE tensors (conv_pack.hip)
        Geom src = g;
        src.up_f = src.up_t = src.sf = src.st = 1;
        p.a = fwd_args(x1, x2, src);
        p.a.Hout = Hin * up_f; p.a.Wout = Win * up_t;
        p.path = 0; p.ncls = up_f * up_t; p.os_f = up_f; p.os_t = up_t;
        conv::fold_classes(Cout, C1 + C2, up_f, up_t, Hin, Win, p.cls);
        return p;
    }
    p.a = fwd_args(x1, x2, g);
    p.path = (conv::mfma_ok(C1 + C2, Cout) && !(C1 & 1)) ? 1 : 2;
    return p;
}

#ifndef DCS_ACT_BF16
extern "C" long dcs_cconv2d_fwd_workspace_bytes(int B, int Hin, int Win, int C1, int C2, int up_f, int up_t, int Cout,
                                                int kh, int kw, int sf, int st, int pad_f, int pad_t) {
    const Geom g{B, Hin, Win, C1, C2, up_f, up_t, Cout, kh, kw, sf, st, pad_f, pad_t};
    if (!conv::geom_ok(g)) return -1;
    const FwdPlan p = fwd_plan(nullptr, nullptr, g);
    if (p.a.Hout <= 0 || p.a.Wout <= 0) return -1;
    if (p.path == 0) return dcs_conv_mfma_workspace_bytes(p.a, p.ncls, p.cls);
    if (p.path == 1) return dcs_conv_mfma_workspace_bytes_plain(p.a);
    return 0;
}
#endif

extern "C" int DCS_SYM(dcs_cconv2d_fwd_affine)(const act_t* x1, const act_t* x2, const float* wp, const float* bias, const float* coef,
                                      act_t* y, void* workspace, long workspace_bytes, int B, int Hin, int Win, int C1, int C2,
                                      int up_f, int up_t, int Cout, int kh, int kw, int sf, int st, int pad_f, int pad_t,
                                      int act, dcs_stream_t stream);
extern "C" int DCS_SYM(dcs_cconv2d_fwd)(const act_t* x1, const act_t* x2, const float* wp, const float* bias, act_t* y,
                               void* workspace, long workspace_bytes, int B, int Hin, int Win, int C1, int C2, int up_f,
                               int up_t, int Cout, int kh, int kw, int sf, int st, int pad_f, int pad_t, int act,
                               dcs_stream_t stream) {
    return DCS_SYM(dcs_cconv2d_fwd_affine)(x1, x2, wp, bias, nullptr, y, workspace, workspace_bytes, B, Hin, Win, C1, C2, up_f, up_t, Cout,
                                  kh, kw, sf, st, pad_f, pad_t, act, stream);
}

extern "C" int DCS_SYM(dcs_cconv2d_fwd_affine)(const act_t* x1, const act_t* x2, const float* wp, const float* bias, const float* coef,
                                      act_t* y, void* workspace, long workspace_bytes, int B, int Hin, int Win, int C1, int C2,
                                      int up_f, int up_t, int Cout, int kh, int kw, int sf, int st, int pad_f, int pad_t,
                                      int act, dcs_stream_t stream) {
    if (!wp || !bias || !y) return DCS_ERR_BADARG;
    const Geom g{B, Hin, Win, C1, C2, up_f, up_t, Cout, kh, kw, sf, st, pad_f, pad_t};
    if (!fwd_geom_ok(x1, x2, g)) return DCS_ERR_BADARG;
    if (act < DCS_ACT_NONE || act > DCS_ACT_SIGMOID) return DCS_ERR_BADARG;
    FwdPlan p = fwd_plan(x1, x2, g);
    p.a.wp = (const float2*)wp; p.a.bias = (const float2*)bias; p.a.y = (act2_t*)y; p.a.act = act; p.a.coef = coef;
    if (p.path == 0)
        return dcs_conv_mfma_launch_classes(p.a, wp + base_floats(Cout, C1 + C2, kh * kw), p.ncls, p.cls, p.os_f, p.os_t,
                                            nullptr, 0, workspace, workspace_bytes, dcs_stream(stream));
    if (p.path == 1)
        return dcs_conv_mfma_launch(p.a, wp + conv::direct_floats(Cout, C1 + C2, kh * kw), workspace, workspace_bytes,
                                    dcs_stream(stream));
    return dcs_conv_direct_launch(p.a, dcs_stream(stream));
}

// Rows of CBN partial sums (float[rows][Cout][5]) dcs_cconv2d_fwd_stats writes for this geometry when handed the split-K
// scratch dcs_cconv2d_fwd_workspace_bytes asks for; 0: the geometry has no statistics epilogue (run dcs_cbn_fwd instead).
static int fwd_stat_rows(const FwdPlan& p, bool have_ws) {
    if (p.path == 0) return dcs_conv_mfma_stat_rows(p.a, p.ncls, p.cls, have_ws);
    if (p.path == 1) {
        conv::Cls c;
        c.kh = p.a.kh; c.kw = p.a.kw; c.pad_f = p.a.pad_f; c.pad_t = p.a.pad_t; c.oo_f = 0; c.oo_t = 0;
        c.Hc = p.a.Hout; c.Wc = p.a.Wout; c.bm_off = 0;
        return dcs_conv_mfma_stat_rows(p.a, 1, &c, have_ws);
    }
    if (!dcs_conv_k7_ok(&p.a, 1) && p.a.C2 == 0) return dcs_conv_enc0_stat_rows(p.a);
    return 0;
}

#ifndef DCS_ACT_BF16
extern "C" int dcs_cconv2d_fwd_stats_rows(int B, int Hin, int Win, int C1, int C2, int up_f, int up_t, int Cout, int kh,
                                          int kw, int sf, int st, int pad_f, int pad_t) {
    const Geom g{B, Hin, Win, C1, C2, up_f, up_t, Cout, kh, kw, sf, st, pad_f, pad_t};
    if (!conv::geom_ok(g)) return -1;
    const FwdPlan p = fwd_plan(nullptr, nullptr, g);
    if (p.a.Hout <= 0 || p.a.Wout <= 0) return -1;
    return fwd_stat_rows(p, true);
}
#endif

// dcs_cconv2d_fwd (no activation) that ALSO leaves the training-mode CBN statistics of its raw output: stat =
// float[Cout][5][stat_rows], column r = one workgroup's partial {S_r, S_i, S_rr, S_ii, S_ri} of (y - bias), fixed order;
// *rows_used (host int) = the rows actually written (<= stat_rows = dcs_cconv2d_fwd_stats_rows).  Feeds dcs_cbn_fwd_slabs
// with pivot = bias: the CBN's statistics pass over y (c_network.py:107-114: conv, CBN back to back) disappears.
extern "C" int DCS_SYM(dcs_cconv2d_fwd_stats)(const act_t* x1, const act_t* x2, const float* wp, const float* bias, act_t* y,
                                     float* stat, int stat_rows, int* rows_used, void* workspace, long workspace_bytes, int B,
                                     int Hin, int Win, int C1, int C2, int up_f, int up_t, int Cout, int kh, int kw, int sf,
                                     int st, int pad_f, int pad_t, dcs_stream_t stream) {
    if (!wp || !bias || !y || !stat || !rows_used || stat_rows < 1) return DCS_ERR_BADARG;
    const Geom g{B, Hin, Win, C1, C2, up_f, up_t, Cout, kh, kw, sf, st, pad_f, pad_t};
    if (!fwd_geom_ok(x1, x2, g)) return DCS_ERR_BADARG;
    FwdPlan p = fwd_plan(x1, x2, g);
    const long need = p.path == 0 ? dcs_conv_mfma_workspace_bytes(p.a, p.ncls, p.cls)
                    : p.path == 1 ? dcs_conv_mfma_workspace_bytes_plain(p.a) : 0;
    const bool have_ws = need > 0 && workspace != nullptr && workspace_bytes >= need;
    const int rows = fwd_stat_rows(p, have_ws);
    if (rows < 1 || rows > stat_rows) return DCS_ERR_BADARG;
    *rows_used = rows;
    p.a.wp = (const float2*)wp; p.a.bias = (const float2*)bias; p.a.y = (act2_t*)y; p.a.act = DCS_ACT_NONE; p.a.coef = nullptr;
    p.a.stat = stat; p.a.stat_stride = stat_rows;
    if (p.path == 0)
        return dcs_conv_mfma_launch_classes(p.a, wp + base_floats(Cout, C1 + C2, kh * kw), p.ncls, p.cls, p.os_f, p.os_t,
                                            nullptr, 0, workspace, workspace_bytes, dcs_stream(stream));
    if (p.path == 1)
        return dcs_conv_mfma_launch(p.a, wp + conv::direct_floats(Cout, C1 + C2, kh * kw), workspace, workspace_bytes,
                                    dcs_stream(stream));
    return dcs_conv_enc0_launch(p.a, dcs_stream(stream));
}

// ---- real-valued convolution on the same MFMA kernel (DR-Net: r_network.py:60-66, :90-102) -------------------------
// A real NHWC activation with an even channel count IS an interleaved "complex" one with half as many channels, and the
// complex kernel's GEMM is a plain real GEMM over K = taps x real input channels, N = real output channels whose B
// panel happens to have a 2x2 block structure.  A real conv only needs a B panel WITHOUT that structure: the caller
// packs B[tap][k][n] = w[n][k][tap] into the 32-column fragment order (dcsnet/r_network.py) and this entry runs it.
static bool rconv_ok(int C1r, int C2r, int Coutr) {
    if ((C1r & 1) || (C2r & 1) || (Coutr & 1)) return false;
    return conv::mfma_ok((C1r + C2r) / 2, Coutr / 2) && !((C1r / 2) & 1);
}

#ifndef DCS_ACT_BF16
extern "C" long dcs_rconv2d_fwd_workspace_bytes(int B, int Hin, int Win, int C1r, int C2r, int up_f, int up_t, int Coutr,
                                                int kh, int kw, int sf, int st, int pad_f, int pad_t) {
    if (!rconv_ok(C1r, C2r, Coutr) || B <= 0 || Hin <= 0 || Win <= 0) return -1;
    const ConvArgs a = fwd_args(nullptr, nullptr, Geom{B, Hin, Win, C1r / 2, C2r / 2, up_f, up_t, Coutr / 2, kh, kw, sf, st, pad_f, pad_t});
    return dcs_conv_mfma_workspace_bytes_plain(a);
}
#endif

#ifndef DCS_ACT_BF16
extern "C" int dcs_rconv2d_fwd(const float* x1, const float* x2, const float* bm, const float* bias, float* y,
                               void* workspace, long workspace_bytes, int B, int Hin, int Win, int C1r, int C2r, int up_f,
                               int up_t, int Coutr, int kh, int kw, int sf, int st, int pad_f, int pad_t, int act,
                               dcs_stream_t stream) {
    if (!bm || !y || !rconv_ok(C1r, C2r, Coutr)) return DCS_ERR_BADARG;
    const Geom g{B, Hin, Win, C1r / 2, C2r / 2, up_f, up_t, Coutr / 2, kh, kw, sf, st, pad_f, pad_t};
    if (!fwd_geom_ok(x1, x2, g)) return DCS_ERR_BADARG;
    if (act < DCS_ACT_NONE || act > DCS_ACT_SIGMOID) return DCS_ERR_BADARG;
    ConvArgs a = fwd_args(x1, x2, g);
    a.wp = nullptr; a.bias = (const float2*)bias; a.y = (float2*)y; a.act = act;
    return dcs_conv_mfma_launch_wide(a, bm, workspace, workspace_bytes, dcs_stream(stream));
}
#endif

// Gradient of dcs_rconv2d_fwd's VIRTUAL input (the upsampled concatenation), float[B][Hv][Wv][Cinr]: a stride-1
// correlation of the zero-inserted g_Y with the caller-packed panel of the flipped, in/out-swapped kernel
// (B[tap][k = real output channel][n = real input channel]), padding k-1-p.  The block sum over an upsample and the
// channel split of a concatenation are dcs_upsample_cat_bwd's (complex channel counts Cr/2).
#ifndef DCS_ACT_BF16
static conv::Args rconv_dgrad_args(const float* gy, float* gxv, int B, int Hv, int Wv, int Cinr, int Coutr, int kh, int kw,
                                   int sf, int st, int pad_f, int pad_t) {
    ConvArgs a{};
    const int Hout = (Hv + 2 * pad_f - kh) / sf + 1, Wout = (Wv + 2 * pad_t - kw) / st + 1;
    a.x1 = (const float2*)gy; a.x2 = nullptr; a.bias = nullptr; a.wp = nullptr; a.y = (float2*)gxv;
    a.B = B; a.Hin = Hout; a.Win = Wout; a.C1 = Coutr / 2; a.C2 = 0; a.Cout = Cinr / 2; a.act = DCS_ACT_NONE;
    a.up_f = sf; a.up_t = st; a.zero_ins = 1;
    a.kh = kh; a.kw = kw; a.sf = 1; a.st = 1; a.pad_f = kh - 1 - pad_f; a.pad_t = kw - 1 - pad_t;
    a.Hv = (Hout - 1) * sf + 1; a.Wv = (Wout - 1) * st + 1;
    a.Hout = Hv; a.Wout = Wv;
    return a;
}
#endif

#ifndef DCS_ACT_BF16
extern "C" long dcs_rconv2d_bwd_data_workspace_bytes(int B, int Hv, int Wv, int Cinr, int Coutr, int kh, int kw, int sf,
                                                     int st, int pad_f, int pad_t) {
    if (B <= 0 || Hv <= 0 || Wv <= 0 || !rconv_ok(Coutr, 0, Cinr) || kh < 1 || kw < 1 || sf < 1 || st < 1 || pad_f < 0 ||
        pad_t < 0 || pad_f > kh - 1 || pad_t > kw - 1)
        return -1;
    const ConvArgs a = rconv_dgrad_args(nullptr, nullptr, B, Hv, Wv, Cinr, Coutr, kh, kw, sf, st, pad_f, pad_t);
    if (a.Hin <= 0 || a.Win <= 0) return -1;
    return dcs_conv_mfma_workspace_bytes_plain(a);
}
#endif

#ifndef DCS_ACT_BF16
extern "C" int dcs_rconv2d_bwd_data(const float* gy, const float* bm_bwd, float* gxv, void* workspace, long workspace_bytes,
                                    int B, int Hv, int Wv, int Cinr, int Coutr, int kh, int kw, int sf, int st, int pad_f,
                                    int pad_t, dcs_stream_t stream) {
    if (!gy || !bm_bwd || !gxv || B <= 0 || Hv <= 0 || Wv <= 0 || !rconv_ok(Coutr, 0, Cinr)) return DCS_ERR_BADARG;
    if (kh < 1 || kw < 1 || sf < 1 || st < 1 || pad_f < 0 || pad_t < 0 || pad_f > kh - 1 || pad_t > kw - 1)
        return DCS_ERR_BADARG;
    ConvArgs a = rconv_dgrad_args(gy, gxv, B, Hv, Wv, Cinr, Coutr, kh, kw, sf, st, pad_f, pad_t);
    if (a.Hin <= 0 || a.Win <= 0) return DCS_ERR_BADARG;
    return dcs_conv_mfma_launch_wide(a, bm_bwd, workspace, workspace_bytes, dcs_stream(stream));
}
#endif

// data-gradient launch description shared by the workspace query and the launch itself
struct DgradPlan {
    ConvArgs a{};
    int path;                  // 0: gradient of the upsample-folded conv, 1: enc0 class kernel, 2: stride classes (MFMA),
                               // 3: zero-insertion MFMA, 4: zero-insertion direct
    int ncls, os_f, os_t;
    conv::Cls cls[4];
    long gxv_bytes;            // gradient of the virtual (upsampled / concatenated) input, 0 when written straight to g_x1
    bool split;                // path 3 writes g_x1 | g_x2 from its epilogue
    int Hv, Wv, Hout, Wout;
};

static DgradPlan dgrad_plan(const void* gy, const Geom& g) {
    const auto [B, Hin, Win, C1, C2, up_f, up_t, Cout, kh, kw, sf, st, pad_f, pad_t] = g;
    DgradPlan p{};
    const int Cin = C1 + C2;
    p.Hv = Hin * up_f; p.Wv = Win * up_t;
    p.Hout = (p.Hv + 2 * pad_f - kh) / sf + 1; p.Wout = (p.Wv + 2 * pad_t - kw) / st + 1;
    ConvArgs& a = p.a;
    a.x1 = (const act2_t*)gy; a.x2 = nullptr; a.bias = nullptr;
    a.B = B; a.Hin = p.Hout; a.Win = p.Wout; a.C1 = Cout; a.C2 = 0; a.Cout = Cin; a.act = DCS_ACT_NONE;
    p.ncls = 1; p.os_f = 1; p.os_t = 1;
    if (!(C1 & 1) && conv::fold_ok(Cin, Cout, kh, kw, sf, st, pad_f, pad_t, up_f, up_t)) {
        // gradient w.r.t. the SOURCE of the upsampled conv: stride-up correlation over g_Y with the effective
        // 4-tap kernel; columns split into g_x1 | g_x2 in the epilogue (no g_Xv, no block-sum pass)
        a.up_f = 1; a.up_t = 1; a.zero_ins = 0; a.Hv = p.Hout; a.Wv = p.Wout;
        a.kh = up_f == 2 ? 4 : 3; a.kw = up_t == 2 ? 4 : 3; a.sf = up_f; a.st = up_t; a.pad_f = 1; a.pad_t = 1;
        a.Hout = Hin; a.Wout = Win;
        conv::Cls& c = p.cls[0];
        c.kh = a.kh; c.kw = a.kw; c.pad_f = 1; c.pad_t = 1; c.oo_f = 0; c.oo_t = 0; c.Hc = Hin; c.Wc = Win;
        c.bm_off = conv::direct_floats(Cin, Cout, a.kh * a.kw);
        p.path = 0;
        return p;
    }
    // stride-1 conv over a plain concatenation (no upsample): the MFMA epilogue splits its columns into g_x1 | g_x2, so the
    // gradient of the virtual input is never materialised (dec6's 1x1 tap conv: a 67 MB round trip + a split kernel)
    p.split = up_f * up_t == 1 && sf == 1 && st == 1 && C2 > 0 && conv::mfma_ok(Cout, Cin) && !(C1 & 1);
    if ((up_f * up_t > 1 || C2 > 0) && !p.split) p.gxv_bytes = (long)B * p.Hv * p.Wv * Cin * (long)sizeof(float2);
    if (C2 == 0 && dcs_conv_small_dgrad_ok(Cin, Cout, kh, kw, sf, st, pad_f, pad_t, up_f, up_t)) { p.path = 1; return p; }
    if (conv::stride_ok(Cin, Cout, kh, kw, sf, st, pad_f, pad_t)) {
        // one compact sub-kernel per residue class of the input pixel instead of zero insertion
        a.up_f = 1; a.up_t = 1; a.zero_ins = 0; a.Hv = p.Hout; a.Wv = p.Wout;
        a.kh = kh; a.kw = kw; a.sf = 1; a.st = 1; a.pad_f = 0; a.pad_t = 0;
        a.Hout = p.Hv; a.Wout = p.Wv;
        conv::stride_classes(Cout, Cin, kh, kw, sf, st, pad_f, pad_t, p.Hv, p.Wv, p.cls);
        p.ncls = sf * st; p.os_f = sf; p.os_t = st;
        p.path = 2;
        return p;
    }
    a.up_f = sf; a.up_t = st; a.zero_ins = 1;
    a.kh = kh; a.kw = kw; a.sf = 1; a.st = 1; a.pad_f = kh - 1 - pad_f; a.pad_t = kw - 1 - pad_t;
    a.Hv = (p.Hout - 1) * sf + 1; a.Wv = (p.Wout - 1) * st + 1;
    a.Hout = p.Hv; a.Wout = p.Wv;                          // explicit: rows past the last tap get zeros
    p.path = conv::mfma_ok(Cout, Cin) ? 3 : 4;
    return p;
}

static long dgrad_split_bytes(const DgradPlan& p) {
    if (p.path == 0 || p.path == 2) return dcs_conv_mfma_workspace_bytes(p.a, p.ncls, p.cls);
    if (p.path == 3) return dcs_conv_mfma_workspace_bytes_plain(p.a);
    return 0;
}

#ifndef DCS_ACT_BF16
extern "C" long dcs_cconv2d_bwd_data_workspace_bytes(int B, int Hin, int Win, int C1, int C2, int up_f, int up_t,
                                                     int Cout, int kh, int kw, int sf, int st, int pad_f, int pad_t) {
    const Geom g{B, Hin, Win, C1, C2, up_f, up_t, Cout, kh, kw, sf, st, pad_f, pad_t};
    if (!conv::geom_ok(g) || !conv::dgrad_pad_ok(g)) return -1;
    const DgradPlan p = dgrad_plan(nullptr, g);
    if (p.Hout <= 0 || p.Wout <= 0) return -1;
    return align256(p.gxv_bytes) + dgrad_split_bytes(p);     // [g_Xv | split-K slices]
}
#endif

extern "C" int DCS_SYM(dcs_cconv2d_bwd_data)(const act_t* gy, const float* wp_bwd, act_t* gx1, act_t* gx2, void* workspace,
                                    long workspace_bytes, int B, int Hin, int Win, int C1, int C2, int up_f, int up_t,
                                    int Cout, int kh, int kw, int sf, int st, int pad_f, int pad_t,
                                    dcs_stream_t stream) {
    const Geom g{B, Hin, Win, C1, C2, up_f, up_t, Cout, kh, kw, sf, st, pad_f, pad_t};
    if (!gy || !wp_bwd || !gx1 || !conv::geom_ok(g) || !conv::dgrad_pad_ok(g)) return DCS_ERR_BADARG;
    if ((C2 > 0) != (gx2 != nullptr)) return DCS_ERR_BADARG;
    const int Cin = C1 + C2, taps = kh * kw;
    DgradPlan p = dgrad_plan(gy, g);
    if (p.Hout <= 0 || p.Wout <= 0) return DCS_ERR_BADARG;
    hipStream_t s = dcs_stream(stream);
    const float* extra = wp_bwd + base_floats(Cin, Cout, taps);
    act_t* gxv = gx1;
    if (p.gxv_bytes > 0) {                                  // generic: gradient of the virtual input, then fold it
        if (!workspace || workspace_bytes < p.gxv_bytes) return DCS_ERR_WORKSPACE;
        gxv = (act_t*)workspace;
    }
    // whatever follows g_Xv in the workspace is split-K scratch (optional: too small just means no slicing)
    const long used = align256(p.gxv_bytes);
    void* ws2 = (workspace && workspace_bytes > used) ? (void*)((char*)workspace + used) : nullptr;
    const long ws2_bytes = ws2 ? workspace_bytes - used : 0;
    p.a.y = (act2_t*)gxv;
    int rc;
    switch (p.path) {
        case 0:
            return dcs_conv_mfma_launch_classes(p.a, extra, 1, p.cls, 1, 1, C2 ? gx2 : nullptr, 2 * C1, ws2, ws2_bytes, s);
        case 1:
            return dcs_conv_small_dgrad_launch(gy, wp_bwd, gx1, B, p.Hv, p.Wv, p.Hout, p.Wout, pad_f, pad_t, s);   // enc0
        case 2:
            rc = dcs_conv_mfma_launch_classes(p.a, extra, p.ncls, p.cls, p.os_f, p.os_t, nullptr, 0, ws2, ws2_bytes, s);
            break;
        case 3:
            p.a.wp = (const float2*)wp_bwd;
            if (p.split)
                return dcs_conv_mfma_launch_split(p.a, wp_bwd + conv::direct_floats(Cin, Cout, taps), gx2, 2 * C1, ws2, ws2_bytes, s);
            rc = dcs_conv_mfma_launch(p.a, wp_bwd + conv::direct_floats(Cin, Cout, taps), ws2, ws2_bytes, s);
            break;
        default:
            p.a.wp = (const float2*)wp_bwd;
            rc = dcs_conv_direct_launch(p.a, s);
            break;
    }
    if (rc != DCS_OK || gxv == gx1) return rc;
    return dcs_upsample_cat_bwd_launch(gxv, gx1, gx2, B, Hin, Win, C1, C2, up_f, up_t, s);
}

// ---- weight gradient ---------------------------------------------------------------------------
// Launch description shared by the workspace query, the plan read-out and the launch itself.  The workspace of every
// route is conv::WgradLayout's: [ weight slabs | bias slabs | pad to 256 | pre-split g_Y planes (MFMA routes only) ].
enum WgradRoute { WG_FOLD = 0, WG_MFMA = 1, WG_ENC0 = 2, WG_SMALL = 3, WG_DIRECT = 4 };   // in order of precedence
struct WgradPlan {
    bool ok;                   // false: no weight gradient for this geometry (DCS_ERR_BADARG / -1)
    WgradRoute route;
    ConvArgs a;                // forward geometry; the three non-MFMA routes have conv_direct.hip's 16x16 tiling filled in
    conv::WgradLayout m;       // slab count and byte offsets (MFMA routes: conv_wgrad_mfma.hip's, with its tile and classes)
};

static WgradPlan wgrad_plan(const Geom& g) {
    WgradPlan p{};
    p.a = fwd_args(nullptr, nullptr, g);             // (the launch sets the operands)
    if (g.kh * g.kw > conv::kWgradMaxTaps || p.a.Hout <= 0 || p.a.Wout <= 0) return p;
    if (dcs_conv_wgrad_mfma_ok(g.C1 + g.C2, g.Cout, g.kh, g.kw, g.C1)) {          // MFMA GEMM over the pixel axis
        p.m = dcs_conv_wgrad_mfma_plan(p.a);
        p.route = p.m.fold ? WG_FOLD : WG_MFMA;         // (fold: decoder stages, per parity class at source resolution)
        p.ok = true;
        return p;
    }
    // one slab per 16x16 tile up to 32 MB of them: the count the three remaining kernels are handed (enc0 and small use fewer)
    if (!dcs_conv_geometry(p.a)) return p;
    p.m.ncls = 1;
    p.m.wsz = (long)g.kh * g.kw * (g.C1 + g.C2) * g.Cout;
    const long total_tiles = (long)p.a.tiles_w * p.a.tiles_h * g.B;
    long cap = (32L << 20) / (p.m.wsz * (long)sizeof(float2));
    if (cap < 1) cap = 1;
    if (cap > 1024) cap = 1024;
    p.m.n_slabs = (int)(total_tiles < cap ? total_tiles : cap);
    p.m.slab_bytes = (long)p.m.n_slabs * (p.m.wsz + g.Cout) * (long)sizeof(float2);
    p.m.planes_off = align256(p.m.slab_bytes);
    p.m.bytes = p.m.slab_bytes;
    p.route = dcs_conv_enc0_wgrad_ok(p.a) ? WG_ENC0         // 7x7 1->8 stride 2: taps x pixels on the MFMA units (conv_enc0.hip)
            // 7x7 2->1 / 1->8: pixel-stationary kernel (conv_wgrad_small.hip; fp32 maps only: the attention convs' operands
            // stay fp32 in either mode)
            : (!DCS_ACT_IS_BF16 && dcs_conv_wgrad_small_ok(p.a)) ? WG_SMALL : WG_DIRECT;
    p.ok = true;
    return p;
}

extern "C" long DCS_SYM(dcs_cconv2d_bwd_weight_workspace_bytes)(int B, int Hin, int Win, int C1, int C2, int up_f, int up_t,
                                                                int Cout, int kh, int kw, int sf, int st, int pad_f, int pad_t) {
    const Geom g{B, Hin, Win, C1, C2, up_f, up_t, Cout, kh, kw, sf, st, pad_f, pad_t};
    if (!conv::geom_ok(g)) return -1;
    const WgradPlan p = wgrad_plan(g);
    return p.ok ? p.m.bytes : -1;
}

// out = {route (WgradRoute), slabs, slab bytes, planes bytes, total bytes}: what the launch of this geometry will do
extern "C" int DCS_SYM(dcs_cconv2d_bwd_weight_plan)(int B, int Hin, int Win, int C1, int C2, int up_f, int up_t, int Cout, int kh,
                                                    int kw, int sf, int st, int pad_f, int pad_t, long* out) {
    const Geom g{B, Hin, Win, C1, C2, up_f, up_t, Cout, kh, kw, sf, st, pad_f, pad_t};
    if (!out || !conv::geom_ok(g)) return -1;
    const WgradPlan p = wgrad_plan(g);
    if (!p.ok) return -1;
    out[0] = p.route; out[1] = p.m.n_slabs; out[2] = p.m.slab_bytes; out[3] = p.m.planes_bytes; out[4] = p.m.bytes;
    return 0;
}

extern "C" int DCS_SYM(dcs_cconv2d_bwd_weight)(const act_t* x1, const act_t* x2, const act_t* gy, float* gw_r, float* gw_i,
                                      float* gb_r, float* gb_i, void* workspace, long workspace_bytes, int B, int Hin,
                                      int Win, int C1, int C2, int up_f, int up_t, int Cout, int kh, int kw, int sf,
                                      int st, int pad_f, int pad_t, int transposed, dcs_stream_t stream) {
    if (!gy || !gw_r || !gw_i || !workspace) return DCS_ERR_BADARG;
    if ((gb_r == nullptr) != (gb_i == nullptr)) return DCS_ERR_BADARG;
    const Geom g{B, Hin, Win, C1, C2, up_f, up_t, Cout, kh, kw, sf, st, pad_f, pad_t};
    if (!fwd_geom_ok(x1, x2, g)) return DCS_ERR_BADARG;
    WgradPlan p = wgrad_plan(g);
    if (!p.ok) return DCS_ERR_BADARG;
    p.a.x1 = (const act2_t*)x1; p.a.x2 = (const act2_t*)x2;
    // the slabs must fit; without room for the planes the kernels split g_Y themselves
    const conv::WgradLayout& m = p.m;
    if (workspace_bytes < m.slab_bytes) return DCS_ERR_WORKSPACE;
    float2* slab_w = (float2*)workspace;
    float2* slab_b = slab_w + (long)m.n_slabs * m.ncls * m.wsz;
    void* planes = (m.planes_bytes > 0 && workspace_bytes >= m.planes_off + m.planes_bytes) ? (char*)workspace + m.planes_off
                                                                                             : nullptr;
    hipStream_t s = dcs_stream(stream);
    const int Cin = C1 + C2;
    int ns = m.n_slabs, rc;
    switch (p.route) {
        case WG_FOLD:
            return dcs_conv_wgrad_fold_run(p.a, m, gy, slab_w, slab_b, planes, gw_r, gw_i, gb_r, gb_i, transposed, s);
        case WG_MFMA:
            rc = dcs_conv_wgrad_mfma_launch(p.a, m, gy, slab_w, (float*)slab_b, planes, s);
            break;
        case WG_ENC0:
            rc = dcs_conv_enc0_wgrad_launch(p.a, gy, slab_w, slab_b, m.n_slabs, &ns, s);
            break;
#ifndef DCS_ACT_BF16
        case WG_SMALL: {
            // two resident workgroups per CU.  The 2 -> 1 attention convs run batched (13 problems in one launch inside a
            // train step): ~8 tiles per workgroup there, so that the fixed cross-lane reduction of the 196 accumulators at the
            // end of a workgroup (~2.5 us) is paid per 8 tiles (~6 us of FMAs) rather than per 2
            const int total_tiles = p.a.tiles_w * p.a.tiles_h * B;
            ns = ns < 512 ? ns : 512;
            if (Cin == 2 && Cout == 1) { ns = total_tiles / 8; ns = ns < 1 ? 1 : (ns > 512 ? 512 : ns); }   // = ~2 of its 16 x 64 tiles
            rc = dcs_conv_wgrad_small_launch(p.a, gy, slab_w, slab_b, ns, s);
            break;
        }
#endif
        default:
            return dcs_conv_direct_wgrad_launch(p.a, gy, slab_w, slab_b, ns, gw_r, gw_i, gb_r, gb_i, transposed, s);
    }
    if (rc != DCS_OK) return rc;
    return dcs_conv_wgrad_reduce(slab_w, slab_b, ns, gw_r, gw_i, gb_r, gb_i, Cout, Cin, kh, kw, transposed, s);
}

#ifndef DCS_ACT_BF16
extern "C" int dcs_upsample_cat_bwd(const float* gxv, float* gx1, float* gx2, int B, int Hin, int Win, int C1, int C2,
                                    int up_f, int up_t, dcs_stream_t stream) {
    if (!gxv || !gx1 || B <= 0 || Hin <= 0 || Win <= 0 || C1 <= 0 || C2 < 0 || up_f < 1 || up_t < 1) return DCS_ERR_BADARG;
    if ((C2 > 0) != (gx2 != nullptr)) return DCS_ERR_BADARG;
    return dcs_upsample_cat_bwd_launch(gxv, gx1, gx2, B, Hin, Win, C1, C2, up_f, up_t, dcs_stream(stream));
}
#endif
