// tests/kshim/kshim.hip — test-only launch shim: ONE launch of the reduced-precision convolution kernels, of the fragment-operand
// softmax attention kernels, of the fused DiT row chain and of the linear attention (fused and fp32) of libdexamd.so from a flat descriptor (tests/kshim/__init__.py mirrors the structs with ctypes).  Host
// code only, no kernels: every entry point fills the library's parameter struct by member name, sets the split-weight flag as
// dex_api.hip does for a call, runs the library's own launcher on the given stream and returns the instantiation it picked
// (dex::g_last_symbol; the attention launchers leave none: their entries return the kernel and the plan, recomputed here).
//
// A descriptor the library's shape predicates reject, or one whose launcher would abort or pick a kernel built for another shape,
// is an ERROR CODE (KS_E_*), never a launch: a mistyped test case must not reach the device.  Buffer sizes are the caller's side
// of the contract (the Python loader checks every tensor against the extent the descriptor implies before it calls).
#include "../../dex_tts_amd/csrc/kernels.h"
#include <cstdio>
#include <cstring>

using namespace dex;

namespace {

enum { KS_OK = 0, KS_E_PREC = -1, KS_E_NULL = -2, KS_E_SHAPE = -3, KS_E_UNSUPPORTED = -4, KS_E_FORM = -5, KS_E_STRIDE = -6 };

struct WsplitScope {          // the predicates of lp_dispatch.hip answer for the mode of the call being built on this thread
    bool prev;
    explicit WsplitScope(int precision) : prev(g_lp_wsplit) { g_lp_wsplit = prec_wsplit(precision); }
    ~WsplitScope() { g_lp_wsplit = prev; }
};

bool lp_prec(int p) { return p == PREC_BF16 || p == PREC_FP16 || p == PREC_FP16X2; }

void put_symbol(char* sym, int n) {
    if (!sym || n <= 0) return;
    const char* s = g_last_symbol ? g_last_symbol : "";
    strncpy(sym, s, (size_t)n - 1);
    sym[n - 1] = 0;
}

}  // namespace

extern "C" {

// ---- descriptors (8-byte members first: no padding to mirror) --------------------------------------------------------------
struct KsConv3 {
    const void *X, *Wbf, *Wfrag, *bias, *mask; void* Y;
    const void *pro_stats, *pro_gamma, *pro_beta, *pro_tadd, *pro_res; void* pro_xout;
    const void *res2_w, *res2_b, *res2_mu, *res2_x, *res2_spk, *res2_scal;
    const void *res_w, *res_b, *res_wfrag; void* res_y;
    void* gn_stats;
    long long mask_bstride, w_lo_off, res_lo_off;
    int precision, H, W, Cin, Cout, B, ldx, x_coff, mask_ws, step, row_bstride, x_bf16, y_bf16, xout_lp, res2_scal_stride, res2_planes;
};
struct KsConvDown {
    const void *X, *Wfrag, *bias, *inmask; void* Y;
    long long xb, mask_bstride;
    int precision, a_lp, c_lp, ldx, x_coff, H, W, ldy, y_coff, inmask_ws, B, C;
};
struct KsConvTUp {
    const void *X, *Wfrag0, *Wfrag1, *Wfrag2, *Wfrag3, *bias, *inmask; void* Y;
    long long xb, mask_bstride;
    int precision, a_lp, c_lp, ldx, x_coff, H, W, ldy, y_coff, inmask_ws, B, C;
};

struct KsAttn {               // mirrors AttnDirectP (csrc/kernels.h); xcd_map, half plans of the automatic kind and dbg are the launchers' own
    const void *Qh, *Kh, *Vt; void *O, *ml;
    long long o_sstride;
    int N, Npad, B, ksplit, o_lp, tail_g, tail_ks, half_g, half_n, precision;
};

// mirrors DitChainP (csrc/kernels.h).  heads = 2, M = B * N, xcd_map and xcds are the launcher's / dex_api.hip's own; there is no
// hand-off drop knob here (xdrop is always 0).  A null next_shift is the last block (no qkv stage); xslab / xflag given = the cluster
// form, whose xerr word is the one behind the flag words of every cluster the launch grids for.
struct KsRowChain {
    void* X; const void *O, *ml, *Wp, *W1, *W2, *Wq, *bp, *b1, *b2, *bq, *ada, *next_shift, *next_scale;
    void *Qh, *Kh, *Vt; const void *Qin, *Kin, *Vin; void *xslab, *xflag;
    long long o_sstride, next_step_stride;
    int precision, B, N, Npad, ksplit, qkv_only, attn_inline, step, row_bstride, o_lp, tail_row0, tail_ks, xlocal;
    unsigned epoch; float qscale;
};

// mirror LinKvCtxP, LinMergeP, LinOut2P, LinAttnCtxP and LinAttnCombineP (csrc/kernels.h).  Everything the sampler derives from its
// knobs (nsub, nblk, headwaves, rows, hw and the storage flags) is a member; only DEX_OUT2_MIN stays a knob (the launcher reads it).
struct KsLinKvCtx {
    const void *X, *Wkv, *H2, *gn_stats, *gamma, *beta, *res, *mask; void *part_m, *part_s, *part_c, *Xout;
    long long xb, resb, mask_bstride, wkv_lo_off;
    int precision, npix, C, B, ldx, x_coff, nsub, nblk, headwaves, rows, ldres, res_under_mask, mask_ws, W, h2_bf16, res_lp, xout_lp, reserved;
};
struct KsLinMerge { const void *part_m, *part_s, *part_c, *Wout, *g; void* W2; int precision, nblk, C, B; };
struct KsLinOut2 {
    const void *X, *Wq, *W2, *bias; void *Y, *Y2;
    long long xb, yb, y2b, wq_lo_off;
    int precision, npix, C, B, ldx, x_coff, ldy, y_coff, ldy2, y2_coff, x_lp, y_lp, hw, rows;
};
struct KsLinCtx { const void* qkv; void *part_m, *part_s, *part_c; long long bstride; int ld, n, heads, chunk, nchunks, B; };
struct KsLinCombine { const void *part_m, *part_s, *part_c, *Wout, *g; void* Weff; int nchunks, heads, C, B; };

int ks_struct_bytes(int which) {
    switch (which) {
        case 0: return (int)sizeof(KsConv3);
        case 1: return (int)sizeof(KsConvDown);
        case 2: return (int)sizeof(KsConvTUp);
        case 3: return (int)sizeof(KsAttn);
        case 4: return (int)sizeof(KsRowChain);
        case 5: return (int)sizeof(KsLinKvCtx);
        case 6: return (int)sizeof(KsLinMerge);
        case 7: return (int)sizeof(KsLinOut2);
        case 8: return (int)sizeof(KsLinCtx);
        case 9: return (int)sizeof(KsLinCombine);
    }
    return KS_E_SHAPE;
}

// ---- shape predicates of the library, for the mode `precision` -------------------------------------------------------------
// which: 0 conv3x3_bf16_supported(a, b)   1 conv3x3_bf16_tail_supported(a)   2 conv3x3_bf16_res_supported(a, b)
//        3 conv3x3_bf16_xb_supported(a, b)   4 conv3x3_plain_lp_in_supported(a, b, c, d, e)   5 conv3x3_cat_lp_in_supported(a, b, c, d, e)
//        6 conv3x3_res2_form(a, b, c)   7 conv_down_supported(a, b, c, d, e, f)   8 convt_up_supported(a, b, c, d, e)
//        9 dit_rowchain_supported(a, b)   10 dit_rowchain64_form(a, b, c)   11 dit_rowchain_cluster_form(a, b)
//        12 dit_rowchain_cluster_local_fits(a, b)   13 dit_rowchain_cluster_xcds(a, b) (a count, not a truth value)
int ks_predicate(int which, int precision, int a, int b, int c, int d, int e, int f) {
    if (!lp_prec(precision)) return KS_E_PREC;
    WsplitScope ws(precision);
    switch (which) {
        case 0: return conv3x3_bf16_supported(a, b);
        case 1: return conv3x3_bf16_tail_supported(a);
        case 2: return conv3x3_bf16_res_supported(a, b);
        case 3: return conv3x3_bf16_xb_supported(a, b);
        case 4: return conv3x3_plain_lp_in_supported(a, b, c, d, e);
        case 5: return conv3x3_cat_lp_in_supported(a, b, c, d, e);
        case 6: return conv3x3_res2_form(a, b, c);
        case 7: return conv_down_supported(a, b, c, d, e, f);
        case 8: return convt_up_supported(a, b, c, d, e);
        case 9: return dit_rowchain_supported(a, b);
        case 10: return dit_rowchain64_form(a, b, c);
        case 11: return dit_rowchain_cluster_form(a, b);
        case 12: return dit_rowchain_cluster_local_fits(a, b);
        case 13: return dit_rowchain_cluster_xcds(a, b);
    }
    return KS_E_SHAPE;
}

// ---- weight packing by the library's own code ------------------------------------------------------------------------------
// kind: 0 launch_pack_lp_nk (fp32 [K][N] -> 16-bit [N][K])   1 launch_pack_lp_frag (fp32 [K][N] -> MFMA fragment order)
//       2 launch_pack_lp_frag_nk (fp32 [N][K] -> the same fragment order: Wq of the linear attention's tail)
//       3 launch_f32_to_lp (the row-major 16-bit cast of K * N elements: Wkv of its context pass).
// The split-weight mode packs the fp16 rounding of the weight, then what that rounding lost (through `scratch`, K*N floats), in the
// same layout `lo_off` elements behind - dex_api.hip's pack3.  lo_off is ignored in the other modes.
int ks_pack(int kind, const void* src, void* dst, void* scratch, int K, int N, long long lo_off, int precision, void* stream) {
    if (!lp_prec(precision)) return KS_E_PREC;
    if (!src || !dst || (precision == PREC_FP16X2 && !scratch)) return KS_E_NULL;
    if (K <= 0 || N <= 0 || kind < 0 || kind > 3) return KS_E_SHAPE;
    if ((kind == 1 || kind == 2) && (K % 16 != 0 || N % 32 != 0)) return KS_E_SHAPE;
    if (precision == PREC_FP16X2 && lo_off < (long long)K * N) return KS_E_STRIDE;
    hipStream_t st = (hipStream_t)stream;
    const float* s = (const float*)src;
    unsigned short* d = (unsigned short*)dst;
    auto pack = [&](const float* from, unsigned short* to, int prec) {
        if (kind == 0) launch_pack_lp_nk(from, to, K, N, prec, st);
        else if (kind == 1) launch_pack_lp_frag(from, to, K, N, prec, st);
        else if (kind == 2) launch_pack_lp_frag_nk(from, to, K, N, prec, st);
        else launch_f32_to_lp(from, to, (long)K * N, prec, st);
    };
    if (precision != PREC_FP16X2) { pack(s, d, precision); return KS_OK; }
    pack(s, d, PREC_FP16);
    launch_f32_residual_lp(s, (float*)scratch, (long)K * N, PREC_FP16, st);
    pack((const float*)scratch, d + lo_off, PREC_FP16);
    return KS_OK;
}

// ---- 3x3 / s1 / p1 Block convolution ----------------------------------------------------------------------------------------
static int conv3_fill(const KsConv3& d, Conv3P& p) {
    if (!lp_prec(d.precision)) return KS_E_PREC;
    if (d.H <= 0 || d.W <= 0 || d.B <= 0 || d.mask_ws < 1 || d.mask_bstride < 0) return KS_E_SHAPE;
    if (!d.X || !d.Wbf || !d.bias || !d.mask || !d.Y) return KS_E_NULL;
    if (d.ldx % 8 != 0 || d.x_coff % 8 != 0 || d.x_coff < 0 || d.ldx < d.x_coff + d.Cin) return KS_E_STRIDE;
    if (!conv3x3_bf16_supported(d.Cin, d.Cout)) return KS_E_UNSUPPORTED;
    if (d.Cin == 256 && d.Cout != 64) return KS_E_UNSUPPORTED;               // (256 input channels: the up path's 2C -> C only)
    if (d.precision == PREC_FP16X2 && (d.w_lo_off < 9LL * d.Cin * d.Cout)) return KS_E_STRIDE;
    const bool tail = d.pro_res || d.res2_w;
    if (d.pro_stats) {      // GroupNorm prologue: the model's Cin == Cout convs only (no kernel form pairs it with the fused shortcut)
        if (!d.pro_gamma || !d.pro_beta) return KS_E_NULL;
        if (d.Cin != d.Cout || d.res_w || !conv3x3_bf16_tail_supported(d.Cin)) return KS_E_UNSUPPORTED;
    } else if (tail || d.pro_tadd || d.pro_gamma || d.pro_beta) return KS_E_FORM;
    if (d.pro_res && d.res2_w) return KS_E_FORM;
    if (tail && d.pro_tadd) return KS_E_FORM;                                  // (the fused tail carries no time bias: diffusion.py:66-71)
    if (tail && !d.pro_xout) return KS_E_NULL;
    if (!tail && (d.pro_xout || d.xout_lp)) return KS_E_FORM;
    if (d.res_w) {
        if (!d.res_b || !d.res_y) return KS_E_NULL;
        if (!conv3x3_bf16_res_supported(d.Cin, d.Cout)) return KS_E_UNSUPPORTED;
        if (d.precision == PREC_FP16X2 && d.res_lo_off < (long long)d.Cin * d.Cout) return KS_E_STRIDE;
    } else if (d.res_b || d.res_y || d.res_wfrag) return KS_E_FORM;
    if (d.Cin != d.Cout && !d.res_w && !(d.Cin == 64 || d.Cin == 128 || d.Cin == 256)) return KS_E_UNSUPPORTED;

    p = Conv3P{};
    p.X = (const float*)d.X; p.ldx = d.ldx; p.x_coff = d.x_coff; p.H = d.H; p.W = d.W; p.Cin = d.Cin; p.Cout = d.Cout;
    p.Wbf = d.Wbf; p.bias = (const float*)d.bias; p.Y = (float*)d.Y;
    p.Wfrag = d.Wfrag;
    p.mask = (const float*)d.mask; p.mask_ws = d.mask_ws; p.mask_bstride = (long)d.mask_bstride;
    p.pro_stats = (const gnfix_t*)d.pro_stats; p.pro_gamma = (const float*)d.pro_gamma; p.pro_beta = (const float*)d.pro_beta;
    p.pro_tadd = (const float*)d.pro_tadd;
    p.pro_res = (const float*)d.pro_res; p.pro_xout = (float*)d.pro_xout;
    p.xout_lp = d.xout_lp ? 1 : 0;
    p.res2_w = (const float*)d.res2_w; p.res2_b = (const float*)d.res2_b; p.res2_mu = (const float*)d.res2_mu; p.res2_x = (const float*)d.res2_x;
    p.res2_spk = (const float*)d.res2_spk; p.res2_scal = (const float*)d.res2_scal;
    p.res2_scal_stride = d.res2_scal_stride; p.res2_planes = d.res2_planes;
    p.res_w = d.res_w; p.res_b = (const float*)d.res_b; p.res_y = (float*)d.res_y;
    p.res_wfrag = d.res_wfrag;
    p.step = d.step; p.gn_stats = (gnfix_t*)d.gn_stats; p.B = d.B;
    p.dbg = nullptr;
    p.x_bf16 = d.x_bf16 ? 1 : 0; p.y_bf16 = d.y_bf16 ? 1 : 0;
    p.w_lo_off = (long)d.w_lo_off; p.res_lo_off = (long)d.res_lo_off;
    p.row_bstride = d.row_bstride;
    p.skip_dead = 0;                                          // (set by the launchers)

    // forms that exist at some grids only (the struct-level predicates above cannot see them)
    if (d.res2_w) {         // the recomputed shortcut: the ping-pong strip form, contiguous 64-channel input
        if (!d.res2_b || !d.res2_mu || !d.res2_x || !d.res2_scal) return KS_E_NULL;
        if (d.res2_planes != 2 && d.res2_planes != 3) return KS_E_SHAPE;
        if (d.res2_planes == 3 && !d.res2_spk) return KS_E_NULL;
        if (d.res2_scal_stride < 3) return KS_E_STRIDE;
        if (d.Cin != 64 || d.Cout != 64 || d.ldx != 64 || d.x_coff != 0) return KS_E_UNSUPPORTED;
        if (!conv3x3_res2_form(d.H, d.W, d.B)) return KS_E_FORM;
    }
    if (p.xout_lp && !conv3x3_strip_form(p)) return KS_E_FORM;                // written by the strip forms only
    if (p.x_bf16) {
        if (d.pro_stats) { if (!conv3x3_bf16_xb_supported(d.Cin, d.Cout)) return KS_E_UNSUPPORTED; }
        else if (d.res_w && d.Cout == 128) { if (!conv3x3_plain_lp_in_supported(d.H, d.W, d.B, d.Cin, d.Cout) && !conv3x3_strip_form(p)) return KS_E_FORM; }
        else if (d.res_w) { if (!conv3x3_cat_lp_in_supported(d.H, d.W, d.B, d.Cin, d.Cout)) return KS_E_FORM; }
        else if (!(d.Cin == 64 && d.Cout == 64 && conv3x3_strip_form(p))) return KS_E_FORM;      // plain 16-bit input: the ping-pong form
    }
    return KS_OK;
}

// 1 = this descriptor is valid AND runs on one of the strip-walking forms (conv3x3_strip_form); 0 = valid, a patch form; < 0 = error
int ks_conv3x3_strip_form(const KsConv3* d) {
    if (!d) return KS_E_NULL;
    if (!lp_prec(d->precision)) return KS_E_PREC;
    WsplitScope ws(d->precision);
    Conv3P p;
    const int rc = conv3_fill(*d, p);
    if (rc != KS_OK) return rc;
    return conv3x3_strip_form(p) ? 1 : 0;
}

int ks_conv3x3(const KsConv3* d, void* stream, char* sym, int sym_len) {
    if (!d) return KS_E_NULL;
    if (!lp_prec(d->precision)) return KS_E_PREC;
    WsplitScope ws(d->precision);
    Conv3P p;
    const int rc = conv3_fill(*d, p);
    if (rc != KS_OK) return rc;
    g_last_symbol = nullptr;
    launch_conv3x3_lp(p, d->precision, (hipStream_t)stream);
    put_symbol(sym, sym_len);
    return KS_OK;
}

// ---- Downsample: Conv2d(64, 64, 3, 2, 1) on x * mask ------------------------------------------------------------------------
int ks_conv_down(const KsConvDown* d, void* stream, char* sym, int sym_len) {
    if (!d) return KS_E_NULL;
    if (!lp_prec(d->precision)) return KS_E_PREC;
    WsplitScope ws(d->precision);
    if (d->H <= 0 || d->W <= 0 || d->B <= 0 || d->inmask_ws < 1 || d->mask_bstride < 0) return KS_E_SHAPE;
    if (!d->X || !d->Wfrag || !d->bias || !d->inmask || !d->Y) return KS_E_NULL;
    if (d->x_coff < 0 || d->y_coff < 0 || d->y_coff % 8 != 0 || d->ldx < d->x_coff + d->C || d->ldy < d->y_coff + d->C) return KS_E_STRIDE;
    if (d->xb < (long long)d->H * d->W * d->ldx) return KS_E_STRIDE;
    if (!conv_down_supported(d->C, d->H, d->W, d->ldx, d->ldy, d->x_coff)) return KS_E_UNSUPPORTED;
    ConvDownP p{};
    p.X = d->X; p.a_lp = d->a_lp ? 1 : 0; p.ldx = d->ldx; p.xb = (long)d->xb; p.x_coff = d->x_coff; p.H = d->H; p.W = d->W;
    p.Wfrag = d->Wfrag; p.bias = (const float*)d->bias;
    p.Y = d->Y; p.c_lp = d->c_lp ? 1 : 0; p.ldy = d->ldy; p.y_coff = d->y_coff;
    p.inmask = (const float*)d->inmask; p.inmask_ws = d->inmask_ws; p.mask_bstride = (long)d->mask_bstride; p.B = d->B;
    g_last_symbol = nullptr;
    launch_conv_down(p, d->precision, (hipStream_t)stream);
    put_symbol(sym, sym_len);
    return KS_OK;
}

// ---- Upsample: ConvTranspose2d(64, 64, 4, 2, 1) on x * mask -----------------------------------------------------------------
int ks_convt_up(const KsConvTUp* d, void* stream, char* sym, int sym_len) {
    if (!d) return KS_E_NULL;
    if (!lp_prec(d->precision)) return KS_E_PREC;
    WsplitScope ws(d->precision);
    if (d->H <= 0 || d->W <= 0 || d->B <= 0 || d->inmask_ws < 1 || d->mask_bstride < 0) return KS_E_SHAPE;
    if (!d->X || !d->Wfrag0 || !d->Wfrag1 || !d->Wfrag2 || !d->Wfrag3 || !d->bias || !d->inmask || !d->Y) return KS_E_NULL;
    if (d->x_coff < 0 || d->y_coff < 0 || d->x_coff % 8 != 0 || d->y_coff % 8 != 0 || d->ldx < d->x_coff + d->C || d->ldy < d->y_coff + d->C) return KS_E_STRIDE;
    if (d->xb < (long long)d->H * d->W * d->ldx) return KS_E_STRIDE;
    if (!convt_up_supported(d->C, d->H, d->W, d->ldx, d->ldy)) return KS_E_UNSUPPORTED;
    ConvTUpP p{};
    p.X = d->X; p.a_lp = d->a_lp ? 1 : 0; p.ldx = d->ldx; p.xb = (long)d->xb; p.x_coff = d->x_coff; p.H = d->H; p.W = d->W;
    p.Wfrag[0] = d->Wfrag0; p.Wfrag[1] = d->Wfrag1; p.Wfrag[2] = d->Wfrag2; p.Wfrag[3] = d->Wfrag3; p.bias = (const float*)d->bias;
    p.Y = d->Y; p.c_lp = d->c_lp ? 1 : 0; p.ldy = d->ldy; p.y_coff = d->y_coff;
    p.inmask = (const float*)d->inmask; p.inmask_ws = d->inmask_ws; p.mask_bstride = (long)d->mask_bstride; p.B = d->B;
    g_last_symbol = nullptr;
    launch_convt_up(p, d->precision, (hipStream_t)stream);
    put_symbol(sym, sym_len);
    return KS_OK;
}

// ---- softmax attention on fragment-ordered 16-bit operands (attention_direct.hip, attention_q64.hip) ---------------------------
// Every plan outside what the launchers document is an error code: a workgroup whose waves disagree on barrier counts, or a split
// without key tiles, must not be tried on the device.  nt32 = 32-key tiles, nT = 64-key tiles, ng = groups of 256 queries.
static int attn_fill(const KsAttn& d, AttnDirectP& p, int& ks) {
    if (!lp_prec(d.precision)) return KS_E_PREC;
    if (!d.Qh || !d.Kh || !d.Vt || !d.O) return KS_E_NULL;
    if (d.N <= 0 || d.B <= 0 || d.N > (1 << 16) || d.B > (1 << 12) || d.ksplit < 0) return KS_E_SHAPE;
    if (d.Npad != (d.N + 31) / 32 * 32) return KS_E_SHAPE;
    ks = d.ksplit > 1 ? d.ksplit : 1;
    if (ks > 1 && !d.ml) return KS_E_NULL;
    if (d.o_lp && ks > 1) return KS_E_FORM;                                     // 16-bit rows exist for a single split only
    if (d.o_sstride < (long long)d.B * d.N * 256) return KS_E_STRIDE;
    p = AttnDirectP{};
    p.Qh = d.Qh; p.Kh = d.Kh; p.Vt = d.Vt; p.N = d.N; p.Npad = d.Npad; p.B = d.B;
    p.O = (float*)d.O; p.o_sstride = (long)d.o_sstride; p.ml = (float*)d.ml; p.ksplit = d.ksplit; p.dbg = nullptr;
    p.o_lp = d.o_lp ? 1 : 0; p.xcd_map = 0;
    p.tail_g = d.tail_g; p.tail_ks = d.tail_ks; p.half_g = d.half_g; p.half_n = d.half_n;
    return KS_OK;
}

// which: 0 attention_direct_batch_regime(N, B)   1 attention_direct_ksplit(N, B)   2 attention_q64_ksplit(N, B, a)
int ks_attn_plan(int which, int precision, int N, int B, int a) {
    if (!lp_prec(precision)) return KS_E_PREC;
    if (N <= 0 || B <= 0) return KS_E_SHAPE;
    WsplitScope ws(precision);
    switch (which) {
        case 0: return attention_direct_batch_regime(N, B);
        case 1: return attention_direct_ksplit(N, B);
        case 2: return attention_q64_ksplit(N, B, a);
    }
    return KS_E_SHAPE;
}

// launch_attention_direct: the key-splitting waves (few query tiles) or the shared-ring kernel (many).  form: the kernel, and the
// ring kernel's xcd_map as the launcher computes it.
int ks_attn_direct(const KsAttn* d, void* stream, char* form, int form_len) {
    if (!d) return KS_E_NULL;
    if (!lp_prec(d->precision)) return KS_E_PREC;
    WsplitScope ws(d->precision);
    AttnDirectP p; int ks = 1;
    const int rc = attn_fill(*d, p, ks);
    if (rc != KS_OK) return rc;
    const int nt32 = (d->N + 31) / 32;
    if (d->tail_g || d->tail_ks || d->half_g || d->half_n) return KS_E_FORM;    // the 64-query form's plans
    if (ks > nt32) return KS_E_SHAPE;                                           // (these kernels split by 32-key tiles)
    const bool ring = attention_direct_batch_regime(d->N, d->B);
    if (ring && ks != 1 && ks != attention_direct_ksplit(d->N, d->B)) return KS_E_FORM;
    if (!ring && d->o_lp) return KS_E_FORM;                                     // 16-bit rows: the ring kernel only
    const int xcd_map = (2 * d->B * ks) % 8 == 0 && !knob_off("DEX_XCD_MAP") ? 1 : 0;
    launch_attention_direct(p, d->precision, (hipStream_t)stream);
    if (form && form_len > 0) {
        if (ring) snprintf(form, (size_t)form_len, "attn_direct_ring_kernel xcd_map=%d", xcd_map);
        else snprintf(form, (size_t)form_len, "attn_direct_kernel");
    }
    return KS_OK;
}

// launch_attention_q64.  half_n < 0: whole units only; 0: the launcher's automatic half plan; > 0: that plan, forced.
// form: the unit plan as launch_attention_q64 derives it, recomputed here from the library's public functions.
int ks_attn_q64(const KsAttn* d, void* stream, char* form, int form_len) {
    if (!d) return KS_E_NULL;
    if (!lp_prec(d->precision)) return KS_E_PREC;
    WsplitScope ws(d->precision);
    AttnDirectP p; int ks = 1;
    const int rc = attn_fill(*d, p, ks);
    if (rc != KS_OK) return rc;
    const int nt32 = (d->N + 31) / 32, nT = (nt32 + 1) / 2, ng = (nt32 + 7) / 8;
    if (ks > nT) return KS_E_SHAPE;
    int tks = 1, tg = ng;
    if (d->tail_ks > 1) {
        if (d->tail_ks > (nT < 4 ? nT : 4) || d->tail_g < 1 || d->tail_g > ng - 1) return KS_E_SHAPE;
        if (ks > 1) return KS_E_FORM;
        if (!d->ml) return KS_E_NULL;
        tks = d->tail_ks; tg = d->tail_g;
    } else if (d->tail_ks < 0 || d->tail_g != 0) return KS_E_SHAPE;
    int hg = 0, hn = 0;
    if (d->half_n > 0) {
        if (ks > 1 || tks > 1) return KS_E_FORM;
        if (d->half_g < 0 || d->half_g > nt32 / 8 || d->half_n != (nt32 - 8 * d->half_g + 3) / 4) return KS_E_SHAPE;
        hg = d->half_g; hn = d->half_n;
    } else {
        if (d->half_g != 0) return KS_E_SHAPE;
        const bool automatic = d->half_n == 0 && ks == 1 && tks == 1 && knob_or("DEX_ATTN_Q64_HALF", 1);
        if (!(automatic && attention_q64_half_plan(d->N, d->B, &hg, &hn))) hg = hn = 0;
    }
    const long nunits = hn > 0 ? 2L * d->B * (hg + hn) : 2L * d->B * ((long)tg * ks + (long)(ng - tg) * tks);
    if (nunits >= (1L << 22) || (long)tg * ks >= 4096 || (long)(ng - tg) * tks >= 4096) return KS_E_SHAPE;      // (the kernel's division-free unit decode)
    const int xcd_mode = (2 * d->B) % 8 == 0 ? 1 : 0;
    launch_attention_q64(p, d->precision, (hipStream_t)stream);
    if (form && form_len > 0)
        snprintf(form, (size_t)form_len, "attn_q64_kernel nunits=%ld grid=%ld ks=%d tail_g=%d tail_ks=%d half_g=%d half_n=%d xcd_mode=%d",
                 nunits, nunits < 256 ? nunits : 256L, ks, tg, tks, hg, hn, xcd_mode);
    return KS_OK;
}

// ---- fused DiT row chain (dit_rowchain.hip) -------------------------------------------------------------------------------------
// One launch_dit_rowchain.  Every descriptor the launcher would run on another form than the members ask for, and every one the
// kernels' index arithmetic does not cover, is an error code.  form: g_last_symbol (the launcher names every branch).
int ks_dit_rowchain(const KsRowChain* d, void* stream, char* form, int form_len) {
    if (!d) return KS_E_NULL;
    if (!lp_prec(d->precision)) return KS_E_PREC;
    WsplitScope ws(d->precision);
    if (!dit_rowchain_supported(256, 512)) return KS_E_UNSUPPORTED;
    if (d->N <= 0 || d->B <= 0 || d->N > (1 << 16) || d->B > (1 << 12) || d->step < 0 || d->row_bstride < 0) return KS_E_SHAPE;
    if (d->Npad % 32 != 0 || d->Npad < (d->N + 31) / 32 * 32) return KS_E_SHAPE;
    if (d->ksplit < 0 || d->ksplit > 8 || d->tail_ks < 0 || d->tail_ks > 8) return KS_E_SHAPE;
    const bool has_q = d->next_shift != nullptr;
    const bool chain = !d->qkv_only;
    if (!d->X || !d->ada) return KS_E_NULL;
    if (d->qkv_only && (!has_q || d->attn_inline)) return KS_E_FORM;
    if (has_q) { if (!d->next_scale || !d->Wq || !d->bq || !d->Qh || !d->Kh || !d->Vt) return KS_E_NULL; if (d->next_step_stride < 0 || d->next_step_stride % 4 != 0) return KS_E_STRIDE; }
    else if (d->next_scale || d->Wq || d->bq) return KS_E_FORM;
    if (chain && (!d->Wp || !d->W1 || !d->W2 || !d->bp || !d->b1 || !d->b2)) return KS_E_NULL;
    if (chain && d->attn_inline && (!d->Qin || !d->Kin || !d->Vin)) return KS_E_NULL;
    if (chain && d->attn_inline && (d->ksplit > 1 || d->o_lp || d->tail_ks > 1)) return KS_E_FORM;
    const bool sep = chain && !d->attn_inline;
    if (sep) {
        if (!d->O) return KS_E_NULL;
        if ((d->ksplit > 1 || d->tail_ks > 1) && !d->ml) return KS_E_NULL;
        if (d->o_sstride < (long long)d->B * d->N * 256) return KS_E_STRIDE;
    }
    const bool form64 = dit_rowchain64_form(d->N, d->B, d->attn_inline);
    if (d->o_lp && (!sep || d->ksplit > 1 || !form64)) return KS_E_FORM;          // 16-bit O rows: the 64-row form, one key split
    if (d->tail_ks > 1) {                                                            // the tail merge: the round-3 64-row kernel only
        if (!sep || !form64 || d->ksplit > 1) return KS_E_FORM;
        if (d->tail_row0 <= 0 || d->tail_row0 % 64 != 0 || d->tail_row0 >= d->N) return KS_E_SHAPE;
    } else if (d->tail_row0 != 0 || d->tail_ks == 1) return KS_E_SHAPE;
    const bool slabs = d->xslab || d->xflag;
    if (slabs) {
        if (!d->xslab || !d->xflag) return KS_E_NULL;
        if (!(d->attn_inline || d->qkv_only) || !dit_rowchain_cluster_form(d->N, d->B)) return KS_E_FORM;
        if (d->epoch == 0) return KS_E_SHAPE;
        if (d->xlocal && d->epoch >= (1u << 24)) return KS_E_SHAPE;
        if (d->xlocal && !dit_rowchain_cluster_local_fits(d->N, d->B)) return KS_E_UNSUPPORTED;
    } else if (d->xlocal || d->epoch) return KS_E_FORM;

    DitChainP p{};
    p.O = (const float*)d->O; p.ksplit = d->ksplit; p.o_sstride = (long)d->o_sstride; p.ml = (const float*)d->ml; p.heads = 2;
    p.rows_per_batch = d->N; p.X = (float*)d->X;
    p.Wp = d->Wp; p.W1 = d->W1; p.W2 = d->W2; p.Wq = d->Wq;
    p.bp = (const float*)d->bp; p.b1 = (const float*)d->b1; p.b2 = (const float*)d->b2; p.bq = (const float*)d->bq;
    p.ada = (const float*)d->ada; p.next_shift = (const float*)d->next_shift; p.next_scale = (const float*)d->next_scale;
    p.next_step_stride = (long)d->next_step_stride;
    p.Qh = d->Qh; p.Kh = d->Kh; p.Vt = d->Vt; p.Npad = d->Npad; p.qscale = d->qscale;
    p.Qin = d->Qin; p.Kin = d->Kin; p.Vin = d->Vin;
    p.qkv_only = d->qkv_only ? 1 : 0; p.attn_inline = d->attn_inline ? 1 : 0;
    p.step = d->step; p.M = d->B * d->N; p.B = d->B; p.dbg = nullptr;
    p.o_lp = d->o_lp ? 1 : 0; p.xcd_map = 0; p.xdrop = 0;
    p.tail_row0 = d->tail_row0; p.tail_ks = d->tail_ks; p.row_bstride = d->row_bstride;
    if (slabs) {
        const long tiles = (long)d->B * ((d->N + 31) / 32);
        p.xcds = dit_rowchain_cluster_xcds(d->N, d->B);
        p.xlocal = d->xlocal ? 1 : 0;
        const long grid_tiles = p.xlocal ? (tiles + p.xcds - 1) / p.xcds * 8 : tiles;      // the clusters launch_dit_rowchain grids for
        p.xslab = (float*)d->xslab; p.xflag = (unsigned*)d->xflag; p.epoch = d->epoch;
        p.xerr = reinterpret_cast<int*>((unsigned*)d->xflag + grid_tiles * (long)DIT_CLUSTER_FLAG_WORDS);
    }
    g_last_symbol = nullptr;
    launch_dit_rowchain(p, d->precision, (hipStream_t)stream);
    put_symbol(form, form_len);
    return KS_OK;
}

// ---- linear attention of the U-Net stages (linattn_fused.hip; linattn.hip in the fp32 mode) --------------------------------------
// One launch each.  form: g_last_form, the whole instantiation as the launcher names it (the fp32 kernels have one form each).
static void put_form(char* form, int n) {
    if (!form || n <= 0) return;
    const char* s = g_last_form ? g_last_form : "";
    strncpy(form, s, (size_t)n - 1);
    form[n - 1] = 0;
}
static int lin_common(int precision, int C, int B) {
    if (!lp_prec(precision)) return KS_E_PREC;
    if (C != 64 && C != 128) return KS_E_SHAPE;
    if (B <= 0 || B > 65535) return KS_E_SHAPE;
    if (!linattn_fused_supported(C)) return KS_E_UNSUPPORTED;
    return KS_OK;
}

int ks_linattn_kvctx(const KsLinKvCtx* d, void* stream, char* form, int form_len) {
    if (!d) return KS_E_NULL;
    if (!lp_prec(d->precision)) return KS_E_PREC;
    WsplitScope ws(d->precision);
    const int rc = lin_common(d->precision, d->C, d->B);
    if (rc != KS_OK) return rc;
    const int C = d->C;
    if (d->npix <= 0 || d->nsub < 1 || d->nsub > 8) return KS_E_SHAPE;
    if ((long long)d->nblk != ((long long)d->npix + 128LL * d->nsub - 1) / (128LL * d->nsub)) return KS_E_SHAPE;
    if (!d->Wkv || !d->part_m || !d->part_s || !d->part_c) return KS_E_NULL;
    if (d->precision == PREC_FP16X2 && (d->wkv_lo_off < 256LL * C || d->wkv_lo_off % 8 != 0)) return KS_E_STRIDE;
    if (d->headwaves && d->precision == PREC_FP16X2 && C == 128) return KS_E_UNSUPPORTED;      // (two weight images + the x image: LDS)
    if (d->rows && !d->headwaves) return KS_E_FORM;
    const bool pro = d->H2 != nullptr;
    if (pro) {
        if (!d->gn_stats || !d->gamma || !d->beta || !d->mask || !d->Xout) return KS_E_NULL;
        if (d->W <= 0 || d->npix % d->W != 0 || d->mask_ws < 1 || d->mask_bstride < 0) return KS_E_SHAPE;
        if (d->res) {
            if (d->ldres < C || d->ldres % (d->res_lp ? 8 : 4) != 0 || d->resb < (long long)d->npix * d->ldres) return KS_E_STRIDE;
        } else if (d->ldres || d->resb) return KS_E_FORM;
    } else {
        if (!d->X) return KS_E_NULL;
        if (d->gn_stats || d->gamma || d->beta || d->res || d->mask || d->Xout) return KS_E_FORM;
        if (d->h2_bf16 || d->res_lp || d->xout_lp || d->res_under_mask || d->W || d->ldres) return KS_E_FORM;
        if (d->x_coff < 0 || d->x_coff % 4 != 0 || d->ldx % 4 != 0 || d->ldx < d->x_coff + C) return KS_E_STRIDE;
        if (d->xb < (long long)d->npix * d->ldx) return KS_E_STRIDE;
    }
    LinKvCtxP p{};
    p.X = (const float*)d->X; p.ldx = d->ldx; p.x_coff = d->x_coff; p.xb = (long)d->xb; p.npix = d->npix; p.C = C; p.Wkv = d->Wkv;
    p.nsub = d->nsub; p.nblk = d->nblk; p.part_m = (float*)d->part_m; p.part_s = (float*)d->part_s; p.part_c = (float*)d->part_c; p.B = d->B;
    p.H2 = (const float*)d->H2; p.gn_stats = (const gnfix_t*)d->gn_stats; p.gamma = (const float*)d->gamma; p.beta = (const float*)d->beta;
    p.res = (const float*)d->res; p.ldres = d->ldres; p.resb = (long)d->resb; p.res_under_mask = d->res_under_mask ? 1 : 0;
    p.mask = (const float*)d->mask; p.mask_ws = d->mask_ws; p.mask_bstride = (long)d->mask_bstride; p.W = d->W; p.Xout = (float*)d->Xout;
    p.h2_bf16 = d->h2_bf16 ? 1 : 0; p.res_lp = d->res_lp ? 1 : 0; p.xout_lp = d->xout_lp ? 1 : 0; p.wkv_lo_off = (long)d->wkv_lo_off;
    p.headwaves = d->headwaves ? 1 : 0; p.rows = d->rows ? 1 : 0; p.dbg = nullptr;
    g_last_form = nullptr;
    launch_linattn_kvctx(p, d->precision, (hipStream_t)stream);
    put_form(form, form_len);
    return KS_OK;
}

int ks_linattn_merge(const KsLinMerge* d, void* stream, char* form, int form_len) {
    if (!d) return KS_E_NULL;
    if (!lp_prec(d->precision)) return KS_E_PREC;
    WsplitScope ws(d->precision);
    const int rc = lin_common(d->precision, d->C, d->B);
    if (rc != KS_OK) return rc;
    if (d->nblk < 1) return KS_E_SHAPE;
    if (!d->part_m || !d->part_s || !d->part_c || !d->Wout || !d->g || !d->W2) return KS_E_NULL;
    LinMergeP p{(const float*)d->part_m, (const float*)d->part_s, (const float*)d->part_c, d->nblk, (const float*)d->Wout,
                (const float*)d->g, d->C, d->W2, d->B};
    launch_linattn_merge(p, d->precision, (hipStream_t)stream);
    if (form && form_len > 0) snprintf(form, (size_t)form_len, "linattn_merge_kernel merge_fold<%d>", (d->nblk + 7) / 8 <= 8 ? 8 : (d->nblk + 7) / 8 <= 16 ? 16 : 24);
    return KS_OK;
}

int ks_linattn_out2(const KsLinOut2* d, void* stream, char* form, int form_len) {
    if (!d) return KS_E_NULL;
    if (!lp_prec(d->precision)) return KS_E_PREC;
    WsplitScope ws(d->precision);
    const int rc = lin_common(d->precision, d->C, d->B);
    if (rc != KS_OK) return rc;
    const int C = d->C;
    if (d->npix <= 0) return KS_E_SHAPE;
    if (!d->X || !d->Wq || !d->W2 || !d->bias || !d->Y) return KS_E_NULL;
    const bool lp_io = d->x_lp || d->y_lp || d->Y2;
    if (d->hw && lp_io) return KS_E_FORM;                                         // the wave-split form: fp32 X and Y only
    if (d->rows && !d->hw) return KS_E_FORM;
    if (lp_io && !linattn_out2_lp_out_supported(d->npix, d->B)) return KS_E_FORM;  // 16-bit I/O: the throughput form only
    const int xa = d->x_lp ? 8 : 4;
    if (d->x_coff < 0 || d->x_coff % xa != 0 || d->ldx % xa != 0 || d->ldx < d->x_coff + C || d->xb < (long long)d->npix * d->ldx) return KS_E_STRIDE;
    if (d->y_coff < 0 || d->y_coff % 4 != 0 || d->ldy % 4 != 0 || d->ldy < d->y_coff + C || d->yb < (long long)d->npix * d->ldy) return KS_E_STRIDE;
    if (d->Y2) {
        if (d->y2_coff < 0 || d->y2_coff % 4 != 0 || d->ldy2 % 4 != 0 || d->ldy2 < d->y2_coff + C || d->y2b < (long long)d->npix * d->ldy2) return KS_E_STRIDE;
    } else if (d->ldy2 || d->y2_coff || d->y2b) return KS_E_FORM;
    if (d->precision == PREC_FP16X2 && (d->wq_lo_off < 128LL * C || d->wq_lo_off % 8 != 0)) return KS_E_STRIDE;
    LinOut2P p{};
    p.X = (const float*)d->X; p.ldx = d->ldx; p.x_coff = d->x_coff; p.xb = (long)d->xb; p.npix = d->npix; p.C = C; p.Wq = d->Wq; p.W2 = d->W2;
    p.bias = (const float*)d->bias; p.Y = (float*)d->Y; p.ldy = d->ldy; p.y_coff = d->y_coff; p.yb = (long)d->yb; p.B = d->B;
    p.y_lp = d->y_lp ? 1 : 0; p.Y2 = d->Y2; p.ldy2 = d->ldy2; p.y2_coff = d->y2_coff; p.y2b = (long)d->y2b; p.x_lp = d->x_lp ? 1 : 0;
    p.wq_lo_off = (long)d->wq_lo_off; p.hw = d->hw ? 1 : 0; p.rows = d->rows ? 1 : 0; p.dbg = nullptr;
    g_last_form = nullptr;
    launch_linattn_out2(p, d->precision, (hipStream_t)stream);
    put_form(form, form_len);
    return KS_OK;
}

// the fp32 mode's pair (linattn.hip): chunks of LA_CHUNK = 512 positions (dex_api.hip), four heads of 32
int ks_linattn_ctx(const KsLinCtx* d, void* stream, char* form, int form_len) {
    if (!d) return KS_E_NULL;
    if (!d->qkv || !d->part_m || !d->part_s || !d->part_c) return KS_E_NULL;
    if (d->n <= 0 || d->B <= 0 || d->B > 65535 || d->heads != 4 || d->chunk != 512) return KS_E_SHAPE;
    if (d->nchunks != (d->n + d->chunk - 1) / d->chunk) return KS_E_SHAPE;
    if (d->ld % 4 != 0 || d->ld < 3 * d->heads * 32 || d->bstride < (long long)d->n * d->ld) return KS_E_STRIDE;
    LinAttnCtxP p{(const float*)d->qkv, d->ld, (long)d->bstride, d->n, d->heads, d->chunk, d->nchunks,
                  (float*)d->part_m, (float*)d->part_s, (float*)d->part_c, d->B};
    launch_linattn_ctx(p, (hipStream_t)stream);
    if (form && form_len > 0) snprintf(form, (size_t)form_len, "linattn_ctx_kernel");
    return KS_OK;
}

int ks_linattn_combine(const KsLinCombine* d, void* stream, char* form, int form_len) {
    if (!d) return KS_E_NULL;
    if (!d->part_m || !d->part_s || !d->part_c || !d->Wout || !d->g || !d->Weff) return KS_E_NULL;
    if (d->nchunks <= 0 || d->B <= 0 || d->B > 65535 || d->heads != 4 || d->C <= 0 || d->C > 256) return KS_E_SHAPE;
    LinAttnCombineP p{(const float*)d->part_m, (const float*)d->part_s, (const float*)d->part_c, d->nchunks, d->heads,
                      (const float*)d->Wout, (const float*)d->g, d->C, (float*)d->Weff, d->B};
    launch_linattn_combine(p, (hipStream_t)stream);
    if (form && form_len > 0) snprintf(form, (size_t)form_len, "linattn_combine_kernel");
    return KS_OK;
}

}  // extern "C"
