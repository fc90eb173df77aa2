// patch_embed.hip — PatchEmbed2D of the DiT bottleneck (dit.py:57-58: overlapping depthwise k x k conv, SiLU, pointwise C -> hidden) as
// ONE launch for small grids (reduced-precision modes).  At B = 1 the two separate kernels are 7.0 + 8.4 us of pure latency for 2 MFLOP
// of depthwise work and a 650 x 128 x 256 GEMM; here a workgroup owns EIGHT tokens: its 256 threads compute the depthwise outputs of
// the 8 x C/4 (token, channel quad) items (all 49 taps of an item unconditional loads in flight together, as in dwconv_silu_direct_kernel),
// round SiLU(.) to the MFMA operand type into an LDS A tile [32 rows, 8 live][C] and the four waves run the pointwise GEMM on it —
// the weight fragments (requested at kernel entry, independent of the depthwise phase) come straight from the packed [hidden][C]
// 16-bit twin.  Same arithmetic in the same order as dwconv_silu + igemm_lp_ss (depthwise in fp32, one rounding, K order 0..C):
// bit-identical output.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "lp_util.h"
#include "kernels_lp.h"

namespace dex {
namespace DEX_LP_NS {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned short u16;
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Phase stamps (-DDEX_TIMING builds only, tools/dit_ends_stamps): cycles of thread 0 of a workgroup between consecutive stamps,
// written to pe_dbg[workgroup * 8 + k] (k = 7: the whole workgroup); the tool sets the pointer (pe_set_dbg).
#ifdef DEX_TIMING
__device__ long long* pe_dbg = nullptr;
void pe_set_dbg(long long* d) { (void)hipMemcpyToSymbol(HIP_SYMBOL(pe_dbg), &d, sizeof d); }
#define PSTAMP_DECL long long tk[8] = {0, 0, 0, 0, 0, 0, 0, 0}; const long long tk0 = __builtin_readcyclecounter(); long long tlast = tk0;
#define PSTAMP(k) do { const long long now_ = __builtin_readcyclecounter(); tk[k] += now_ - tlast; tlast = now_; } while (0)
#define PSTAMP_STORE()                                                                                                \
    if (pe_dbg && threadIdx.x == 0) {                                                                                 \
        tk[7] = __builtin_readcyclecounter() - tk0;                                                                   \
        for (int k_ = 0; k_ < 8; ++k_) pe_dbg[(long)blockIdx.x * 8 + k_] = tk[k_];                                    \
    }
// Cut-grid timing (the same builds): pe_set_cut(n) runs the UNCHANGED 8-token body with n live tokens per workgroup on a grid of
// ceil(tokens / n) workgroups - the grid effect alone, without the small tiles' mask and weight changes.
__device__ int pe_cut = 0;
static int pe_cut_host = 0;
void pe_set_cut(int n) { pe_cut_host = n; (void)hipMemcpyToSymbol(HIP_SYMBOL(pe_cut), &n, sizeof n); }
#define PE_LIVE(TOK) ((TOK) == PE_TOK && pe_cut > 0 ? pe_cut : (TOK))
#define PE_LIVE_HOST(TOK) ((TOK) == PE_TOK && pe_cut_host > 0 ? pe_cut_host : (TOK))
#else
#define PSTAMP_DECL
#define PSTAMP(k) do {} while (0)
#define PSTAMP_STORE()
#define PE_LIVE(TOK) (TOK)
#define PE_LIVE_HOST(TOK) (TOK)
#endif

namespace {
constexpr int PE_TOK = 8;
constexpr int PE_TOK_MIN = 4;          // smallest tile the launcher takes by itself (2 is built: DEX_PE_TOK=2)
__device__ __forceinline__ float silu_pe(float x) { return x * __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
}

// TOK tokens per workgroup: 8 (the form the head of this file describes) or, at grids of less than one round of the CUs, 4 (2 is built and
// reached with DEX_PE_TOK=2 only: measured slower) - the A tile stays 32 rows with TOK live
// ones, the depthwise phase runs on the first TOK * C/4 threads, the four waves still split the column tiles and the epilogue stores
// rows < TOK.  The forms below 8 also fetch the mask once per tap COLUMN (it depends on the column only: KS loads per item instead of
// KS * KS); the value that enters the product is still inb ? mk : 0, so every output is the 8-token form's to the bit.
template <int KS, int C, int TOK = PE_TOK>
__global__ __launch_bounds__(256) void patch_embed_fused_kernel(const DwConvP p, const u16* __restrict__ Wb, const float* __restrict__ bias, float* __restrict__ emb, int hid) {
    constexpr int C4 = C / 4, LD = C + 8, KSTEPS = C / 16;
    static_assert(TOK == 8 || TOK == 4 || TOK == 2, "tokens per workgroup");
    __shared__ __attribute__((aligned(16))) u16 As[32 * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, hh = lane >> 5;
    PSTAMP_DECL
    const long ntok = (long)p.B * p.Hf * p.Wt;
    const long tok0 = (long)blockIdx.x * PE_LIVE(TOK);
    // pointwise weight fragments of this wave's column tiles: B operand lane = (column i, K half hh), 8 consecutive k
    const int ntile = hid / 32, per_wave = ntile / 4;       // hid % 128 == 0
    union Fr { uint4 u; lp8 v; };
    Fr wf[2][KSTEPS];                                       // up to two column tiles in flight per pass (hidden 256: all of them)
#ifdef DEX_LP_WSPLIT
    Fr wl[2][KSTEPS];                                       // split weights: the lo halves, hid * C elements behind (the twin's second pack)
#endif
    auto wload_tile = [&](int slot, int nt) __attribute__((always_inline)) {
        const u16* src = Wb + (long)(nt * 32 + i) * C + hh * 8;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) wf[slot][ks].u = *reinterpret_cast<const uint4*>(src + ks * 16);
    };
    // (the lo halves are requested after the depthwise phase: next to its 49 taps in flight they would not fit the register file)
    auto wload_lo = [&](int slot, int nt) __attribute__((always_inline)) {
#ifdef DEX_LP_WSPLIT
        const u16* src = Wb + (long)hid * C + (long)(nt * 32 + i) * C + hh * 8;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) wl[slot][ks].u = *reinterpret_cast<const uint4*>(src + ks * 16);
#endif
    };
    wload_tile(0, wave * per_wave);
    if (per_wave > 1) wload_tile(1, wave * per_wave + 1);
    // zero rows TOK..31 of the A tile (the MFMA reads 32 rows)
    for (int q = tid; q < (32 - TOK) * LD / 8; q += 256) *reinterpret_cast<uint4*>(As + TOK * LD + q * 8) = make_uint4(0, 0, 0, 0);
    // ---- depthwise conv + SiLU of this workgroup's tokens
    if constexpr (TOK != PE_TOK) {
        // small tiles: the waves WITH depthwise items (the first TOK * C/4 threads: one or two waves) request the KS mask columns and all
        // KS * KS taps of X; the other waves meanwhile pass the depthwise weights - the same KS * KS * C floats for every token - through
        // registers into LDS in one coalesced sweep (instead of KS * KS float4 requests per item), and the chain reads them back as 16-byte
        // LDS reads behind an LDS-only barrier, the taps still in flight.  Explicit phases on separate waves: as straight-line code the
        // scheduler waited for every load in turn, and a wave that issues both kinds of request waits for its taps at the join.
        __shared__ __attribute__((aligned(16))) float Wds[KS * KS * C];
        constexpr int NW4 = KS * KS * C4, DWW = (TOK * C4 + 63) / 64, NST = 256 - DWW * 64, WIT = (NW4 + NST - 1) / NST;
        static_assert(DWW <= 2, "at least two waves stage the weights");
        const bool dw = tid < TOK * C4;
        const int cq = tid % C4, tl = tid / C4;
        const long tok = min(tok0 + tl, ntok - 1);
        const int wt = (int)(tok % p.Wt);
        const int f = (int)((tok / p.Wt) % p.Hf);
        const int b = (int)(tok / ((long)p.Wt * p.Hf));
        const float* X = p.X + (long)b * p.xb;
        const float* mrow = p.mask ? p.mask + (long)b * p.mask_bstride : nullptr;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), a4 = make_float4(1.f, 1.f, 1.f, 1.f), c4 = acc;
        float mkc[KS];                                      // the mask of each tap column, addressed by the column clamp alone
        f32x4 xv[KS * KS];
        if (dw) {
            acc = *reinterpret_cast<const float4*>(p.bd + cq * 4);
            if (p.aff) {
                a4 = *reinterpret_cast<const float4*>(p.aff + ((long)b * 2 + 0) * p.C + cq * 4);
                c4 = *reinterpret_cast<const float4*>(p.aff + ((long)b * 2 + 1) * p.C + cq * 4);
            }
#pragma unroll
            for (int kw = 0; kw < KS; ++kw) {
                const int wi = wt * p.s + kw - p.pad;
                const int wcc = (unsigned)wi < (unsigned)p.Wi ? wi : 0;
                mkc[kw] = mrow ? mrow[wcc * p.mask_ws] : 1.f;
            }
#pragma unroll
            for (int kh = 0; kh < KS; ++kh) {
                const int hi = f * p.s + kh - p.pad;
#pragma unroll
                for (int kw = 0; kw < KS; ++kw) {
                    const int wi = wt * p.s + kw - p.pad;
                    const bool inb = (unsigned)hi < (unsigned)p.Hi && (unsigned)wi < (unsigned)p.Wi;
                    const int hc = inb ? hi : 0, wc = inb ? wi : 0;          // clamped: loads are unconditional
                    xv[kh * KS + kw] = *reinterpret_cast<const f32x4*>(X + ((long)hc * p.Wi + wc) * p.ldx + cq * 4);
                }
            }
        }
        if (wave >= DWW) {                                  // (wave-uniform)
            const int t0 = tid - DWW * 64;
            f32x4 ws[WIT];                                  // (native vectors: arrays of float4 structs ended up in scratch)
#pragma unroll
            for (int j = 0; j < WIT; ++j) ws[j] = *reinterpret_cast<const f32x4*>(p.Wd + min(t0 + NST * j, NW4 - 1) * 4);
#pragma unroll
            for (int j = 0; j < WIT; ++j)
                if (t0 + NST * j < NW4) *reinterpret_cast<f32x4*>(Wds + (t0 + NST * j) * 4) = ws[j];
        }
        PSTAMP(0);                                          // requests issued (staging waves: weights passed to LDS)
        lds_barrier();                                      // (LDS only: the taps stay in flight)
        PSTAMP(1);
        if (dw) {
#pragma unroll
            for (int kh = 0; kh < KS; ++kh) {
                const int hi = f * p.s + kh - p.pad;
#pragma unroll
                for (int kw = 0; kw < KS; ++kw) {
                    const int wi = wt * p.s + kw - p.pad;
                    const bool inb = (unsigned)hi < (unsigned)p.Hi && (unsigned)wi < (unsigned)p.Wi;
                    f32x4 v = xv[kh * KS + kw];
                    if (p.aff) { v.x = fmaf(v.x, a4.x, c4.x); v.y = fmaf(v.y, a4.y, c4.y); v.z = fmaf(v.z, a4.z, c4.z); v.w = fmaf(v.w, a4.w, c4.w); }
                    const float4 w = *reinterpret_cast<const float4*>(Wds + (kh * KS + kw) * C + cq * 4);
                    const float mk = inb ? mkc[kw] : 0.f;
                    acc.x = fmaf(v.x * mk, w.x, acc.x); acc.y = fmaf(v.y * mk, w.y, acc.y);
                    acc.z = fmaf(v.z * mk, w.z, acc.z); acc.w = fmaf(v.w * mk, w.w, acc.w);
                }
            }
            uint2 o;
            o.x = pack2_lp(silu_pe(acc.x), silu_pe(acc.y)); o.y = pack2_lp(silu_pe(acc.z), silu_pe(acc.w));
            *reinterpret_cast<uint2*>(As + tl * LD + cq * 4) = o;
        }
    } else {
        if (tid < PE_LIVE(TOK) * C4) {
            const int cq = tid % C4, tl = tid / C4;
            const long tok = min(tok0 + tl, ntok - 1);
            const int wt = (int)(tok % p.Wt);
            const int f = (int)((tok / p.Wt) % p.Hf);
            const int b = (int)(tok / ((long)p.Wt * p.Hf));
            const float* X = p.X + (long)b * p.xb;
            const float* mrow = p.mask ? p.mask + (long)b * p.mask_bstride : nullptr;
            float4 acc = *reinterpret_cast<const float4*>(p.bd + cq * 4);
            // (DwConvP::aff: the DEX TIV adaptor's per-channel affine applied on load, as in dit_elem.hip)
            const float4 a4 = p.aff ? *reinterpret_cast<const float4*>(p.aff + ((long)b * 2 + 0) * p.C + cq * 4) : make_float4(1.f, 1.f, 1.f, 1.f);
            const float4 c4 = p.aff ? *reinterpret_cast<const float4*>(p.aff + ((long)b * 2 + 1) * p.C + cq * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int kh = 0; kh < KS; ++kh) {
                const int hi = f * p.s + kh - p.pad;
#pragma unroll
                for (int kw = 0; kw < KS; ++kw) {
                    const int wi = wt * p.s + kw - p.pad;
                    const bool inb = (unsigned)hi < (unsigned)p.Hi && (unsigned)wi < (unsigned)p.Wi;
                    const int hc = inb ? hi : 0, wc = inb ? wi : 0;              // clamped: loads are unconditional
                    float4 v = *reinterpret_cast<const float4*>(X + ((long)hc * p.Wi + wc) * p.ldx + cq * 4);
                    if (p.aff) { v.x = fmaf(v.x, a4.x, c4.x); v.y = fmaf(v.y, a4.y, c4.y); v.z = fmaf(v.z, a4.z, c4.z); v.w = fmaf(v.w, a4.w, c4.w); }
                    const float4 w = *reinterpret_cast<const float4*>(p.Wd + (kh * KS + kw) * p.C + cq * 4);
                    float mk = mrow ? mrow[wc * p.mask_ws] : 1.f;
                    mk = inb ? mk : 0.f;
                    acc.x = fmaf(v.x * mk, w.x, acc.x); acc.y = fmaf(v.y * mk, w.y, acc.y);
                    acc.z = fmaf(v.z * mk, w.z, acc.z); acc.w = fmaf(v.w * mk, w.w, acc.w);
                }
            }
            uint2 o;
            o.x = pack2_lp(silu_pe(acc.x), silu_pe(acc.y)); o.y = pack2_lp(silu_pe(acc.z), silu_pe(acc.w));
            *reinterpret_cast<uint2*>(As + tl * LD + cq * 4) = o;
        }
    }
    PSTAMP(2);                                              // depthwise chain done, A rows written
    wload_lo(0, wave * per_wave);
    if (per_wave > 1) wload_lo(1, wave * per_wave + 1);
    __syncthreads();
    PSTAMP(3);
    // ---- pointwise GEMM: this wave's column tiles, K = C
    const u16* a_lane = As + i * LD + hh * 8;
    for (int t0 = 0; t0 < per_wave; t0 += 2) {
#pragma unroll
        for (int s_ = 0; s_ < 2; ++s_) {
            if (t0 + s_ >= per_wave) break;
            const int nt = wave * per_wave + t0 + s_;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ++ks) {
                const lp8 af = *reinterpret_cast<const lp8*>(a_lane + ks * 16);
                acc = DEX_MFMA_LP(af, wf[s_][ks].v, acc, 0, 0, 0);
#ifdef DEX_LP_WSPLIT
                acc = DEX_MFMA_LP(af, wl[s_][ks].v, acc, 0, 0, 0);
#endif
            }
            PSTAMP(4);                                      // MFMA chain (with the wait for the weight fragments)
            const float bv = bias ? bias[nt * 32 + i] : 0.f;
            // accumulator rows (r & 3) + 8 (r >> 2) + 4 hh: rows 0..7 are r = 0..3 of both lane halves
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rowl = r + 4 * hh;
                if (rowl < PE_LIVE(TOK) && tok0 + rowl < ntok) emb[(tok0 + rowl) * hid + nt * 32 + i] = acc[r] + bv;
            }
        }
        if (t0 + 2 < per_wave) {                           // hidden > 256: next pair of column tiles
            wload_tile(0, wave * per_wave + t0 + 2); wload_lo(0, wave * per_wave + t0 + 2);
            if (t0 + 3 < per_wave) { wload_tile(1, wave * per_wave + t0 + 3); wload_lo(1, wave * per_wave + t0 + 3); }
        }
    }
    PSTAMP(5);                                              // bias + stores issued
    PSTAMP_STORE()
}

bool patch_embed_fused_supported(int k, int C, int hid, long ntok) {
#if defined(DEX_LP_WSPLIT) && !defined(DEX_WS_HAVE_PE)
    return false;            // no split-weight form yet (lp_config.h)
#endif
   
    // the small-grid regime: measured (fused vs depthwise kernel + GEMM, us) 1 015 tokens (T = 800) 14.1 vs 16.1, 5 010 tokens (T = 4000) 41.6 vs 35.0,
    // 20 800 tokens (B = 32) 153 vs 94 - the one launch pays off up to a few thousand tokens
    return (k == 3 || k == 7) && (C == 64 || C == 128) && hid % 128 == 0 && (ntok * (C / 4) + 255) / 256 < 320;
}

template <int TOK>
static void pe_launch(const DwConvP& p, const u16* w, const float* bias, float* emb, int hid, long ntok, hipStream_t st) {
    const dim3 grid((unsigned)((ntok + PE_LIVE_HOST(TOK) - 1) / PE_LIVE_HOST(TOK)));
    if (p.k == 7 && p.C == 128) hipLaunchKernelGGL((patch_embed_fused_kernel<7, 128, TOK>), grid, dim3(256), 0, st, p, w, bias, emb, hid);
    else if (p.k == 7) hipLaunchKernelGGL((patch_embed_fused_kernel<7, 64, TOK>), grid, dim3(256), 0, st, p, w, bias, emb, hid);
    else if (p.C == 128) hipLaunchKernelGGL((patch_embed_fused_kernel<3, 128, TOK>), grid, dim3(256), 0, st, p, w, bias, emb, hid);
    else hipLaunchKernelGGL((patch_embed_fused_kernel<3, 64, TOK>), grid, dim3(256), 0, st, p, w, bias, emb, hid);
}

// tokens per workgroup: the smallest of 4 / 8 (PE_TOK_MIN; 2 only when forced) whose grid is at most one round of the CUs (B = 1, T = 512: 650 tokens, 163 workgroups
// of 4; T = 800: 1 015 tokens, 254 of 4), 8 where no grid fits a round and at B >= 4 (the batch regime keeps its instructions whatever
// the width).  DEX_PE_TOK forces a value (8 = the form of every grid before).
static int pe_tokens(long ntok, int B) {
    const int forced = knob_or("DEX_PE_TOK", 0);
    if (forced == 2 || forced == 4 || forced == 8) return forced;
    const long ncu = device_cus();
    if (B >= 4) return PE_TOK;
    for (int t = PE_TOK_MIN; t < PE_TOK; t *= 2)
        if ((ntok + t - 1) / t <= ncu) return t;
    return PE_TOK;
}

void launch_patch_embed_fused(const DwConvP& p, const void* Wb, const float* bias, float* emb, int hid, hipStream_t st) {
    const long ntok = (long)p.B * p.Hf * p.Wt;
    const u16* w = reinterpret_cast<const u16*>(Wb);
    switch (pe_tokens(ntok, p.B)) {
    case 2: g_last_symbol = "patch_embed_fused_kernel<2>"; pe_launch<2>(p, w, bias, emb, hid, ntok, st); break;
    case 4: g_last_symbol = "patch_embed_fused_kernel<4>"; pe_launch<4>(p, w, bias, emb, hid, ntok, st); break;
    default: g_last_symbol = "patch_embed_fused_kernel"; pe_launch<PE_TOK>(p, w, bias, emb, hid, ntok, st); break;
    }
}

}  // namespace DEX_LP_NS
}  // namespace dex
