// linattn_fused.hip — LinearAttention (diffusion.py:74-92) without ever materialising q, k or v (bf16-MFMA mode).
//
// Algebra: q enters linearly (out[e,n] = sum_d ctx[d,e] q[d,n], q = Wq x), so the whole Residual(Rezero(
// LinearAttention)) collapses to   y = x + M_b x + g*b_out   with a per-utterance C x C matrix
//     M_b = g * Wout * blockdiag_h(ctx_h^T) * Wq,      ctx_h[d,e] = sum_n softmax_n(k)[d,n] v[e,n].
// Kernel 1 (this file) streams x once: per 32-pixel sub-tile a wave computes k and v (8 tiles of 32x32) with
// v_mfma_f32_32x32x16_bf16, keeps an online per-channel max, and accumulates ctx^T with a SECOND MFMA whose A
// and B operands are the k/v accumulator registers themselves (C-layout: lane = channel, registers = pixels ->
// exactly the A[e][px] / B[px][d] fragment shape; both use the same pixel order, so no shuffle and no LDS).
// Kernel 2 merges the workgroup partials (flash-style) into normalised ctx and folds it with Wout and g into
// W2 = g Wout blockdiag(ctx^T) (C x 128, bf16); kernel 3 is the tail  y = x + W2 (Wq x) + g b  (two chained MFMA
// GEMMs per 32-pixel wave tile, M_b itself is never formed).
// HBM traffic per call: x read twice + y written, instead of writing q,k,v (6x the size of x) and re-reading them.
#include "kernels.h"
#include "lp_util.h"
#include "kernels_lp.h"

namespace dex {
namespace DEX_LP_NS {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned short u16;
union LFrag { uint4 u; lp8 v; };
constexpr float LOG2E_F = 1.4426950408889634f;


// Phase stamps of the context pass (-DDEX_TIMING builds only, tools/kvctx_stamps): cycles spent by thread 0 of a workgroup between
// consecutive stamps, accumulated per phase, written to p.dbg[workgroup * 8 + k] (k = 7: the whole workgroup).
#ifdef DEX_TIMING
#define KSTAMP_DECL long long tk[8] = {0, 0, 0, 0, 0, 0, 0, 0}; const long long tk0 = __builtin_readcyclecounter(); long long tlast = tk0;
#define KSTAMP(k) do { const long long now_ = __builtin_readcyclecounter(); tk[k] += now_ - tlast; tlast = now_; } while (0)
#define KSTAMP_STORE(n)                                                                                               \
    if (p.dbg && threadIdx.x == 0) {                                                                                  \
        long long* d_ = p.dbg + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 8;                                      \
        for (int k_ = 0; k_ < (n); ++k_) d_[k_] = tk[k_];                                                             \
        d_[7] = __builtin_readcyclecounter() - tk0;                                                                   \
    }
#else
#define KSTAMP_DECL
#define KSTAMP(k) do {} while (0)
#define KSTAMP_STORE(n)
#endif

// The prologue of one K-step of a lane's x fragment (PRO forms): the 8 raw values in xa / xc (16-bit H2: xa holds all 8) become
// x = mask * (Mish(GN(h2)) + r)  (identity shortcut)  or  mask * Mish(GN(h2)) + r  (res_conv shortcut), are written to Xout when
// `live`, and replace xa / xc.  The head-parallel form's copy of the 4-wave form's inline prologue (that form keeps its own code, so the
// batch sizes run the same instructions as before): the same operations, and the same bits (tests/test_gpu_linattn_headwaves.py).
__device__ __forceinline__ void kv_prologue8(const LinKvCtxP& p, float4& xa, float4& xc, const float4& ra, const float4& rc, const float* gsc_s,
                                             const float* gsh_s, int ch, bool hb, bool rlp, bool has_r, bool under, bool xlp, float mkv,
                                             bool live, long orow) {
    // Products and sums fuse only where written (fmaf).  Left to the backend, the choice depended on the surrounding code: here it fused
    // (y + r) less often than in the 4-wave form, and 2.8 % of the fp32 x at 40x256 C = 128 differed in the last bit.  Written out below
    // are exactly the fusions the backend gives the 4-wave form in every instantiation: (y + r) = fma(t, q, r) under the mask, nothing else.
#pragma clang fp contract(on)
    float v[8] = {xa.x, xa.y, xa.z, xa.w, xc.x, xc.y, xc.z, xc.w};
    if (hb) {
        const unsigned u0 = __float_as_uint(xa.x), u1 = __float_as_uint(xa.y), u2 = __float_as_uint(xa.z), u3 = __float_as_uint(xa.w);
        v[0] = lp_lo(u0); v[1] = lp_hi(u0); v[2] = lp_lo(u1); v[3] = lp_hi(u1);
        v[4] = lp_lo(u2); v[5] = lp_hi(u2); v[6] = lp_lo(u3); v[7] = lp_hi(u3);
    }
    float r_[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float4 sc0 = *reinterpret_cast<const float4*>(gsc_s + ch), sc1 = *reinterpret_cast<const float4*>(gsc_s + ch + 4);
    const float4 sh0 = *reinterpret_cast<const float4*>(gsh_s + ch), sh1 = *reinterpret_cast<const float4*>(gsh_s + ch + 4);
    const float gsc[8] = {sc0.x, sc0.y, sc0.z, sc0.w, sc1.x, sc1.y, sc1.z, sc1.w};
    const float gsh[8] = {sh0.x, sh0.y, sh0.z, sh0.w, sh1.x, sh1.y, sh1.z, sh1.w};
    if (has_r) {
        if (rlp) {
            const unsigned u0 = __float_as_uint(ra.x), u1 = __float_as_uint(ra.y), u2 = __float_as_uint(ra.z), u3 = __float_as_uint(ra.w);
            r_[0] = lp_lo(u0); r_[1] = lp_hi(u0); r_[2] = lp_lo(u1); r_[3] = lp_hi(u1); r_[4] = lp_lo(u2); r_[5] = lp_hi(u2); r_[6] = lp_lo(u3); r_[7] = lp_hi(u3);
        } else { r_[0] = ra.x; r_[1] = ra.y; r_[2] = ra.z; r_[3] = ra.w; r_[4] = rc.x; r_[5] = rc.y; r_[6] = rc.z; r_[7] = rc.w; }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float t = fmaf(v[j], gsc[j], gsh[j]);
        const float e = __expf(fminf(t, 20.f));
        const float n = e * (e + 2.f);
        const float q = n * __builtin_amdgcn_rcpf(n + 2.f);         // Mish = t * q (rcp: 1 ulp, bf16 consumers)
        v[j] = under ? fmaf(t, q, r_[j]) * mkv : fmaf(t * q, mkv, r_[j]);
    }
    xa = make_float4(v[0], v[1], v[2], v[3]); xc = make_float4(v[4], v[5], v[6], v[7]);
    if (live) {
        if (xlp) {       // 16-bit x for the tail kernel: its q operand rounds x the same way, its residual term reads the rounded value
            u16* xh = reinterpret_cast<u16*>(p.Xout) + orow * p.C + ch;
            *reinterpret_cast<uint4*>(xh) = make_uint4(pack2_lp(v[0], v[1]), pack2_lp(v[2], v[3]), pack2_lp(v[4], v[5]), pack2_lp(v[6], v[7]));
        } else {
            float* xo = p.Xout + orow * p.C + ch;
            *reinterpret_cast<float4*>(xo) = xa;
            *reinterpret_cast<float4*>(xo + 4) = xc;
        }
    }
}

// One head of one 32-pixel sub-tile: k_h and v_h tiles from the x fragments `af` and the k | v rows in LDS (2 x 16 accumulator registers),
// the running softmax statistics of the head's 32 channels, then ctx_h^T += v_h^T p_h from those registers.  The body of the 4-wave
// form's head loop, the same operations in the same order, so a (sub-tile, head) state is the same bits in either form.
// KG > 0: a scheduling fence after every KG K-steps, so the k | v fragments of at most KG steps are in flight (128-register budgets).
template <int C, bool SEED, int KG = 0>
__device__ __forceinline__ void kv_head_step(const u16* Ws, int h, int i, int hh, const LFrag* af, const f32x16& kseed, int px0, int npix,
                                             f32x16& ctx, float& m_run, float& s_run) {
    constexpr int LDW = C + 8, KS = C / 16;
    f32x16 kh, vh;
#pragma unroll
    for (int r = 0; r < 16; ++r) { kh[r] = SEED ? kseed[r] : 0.f; vh[r] = 0.f; }
    const u16* bk = Ws + (h * 32 + i) * LDW + hh * 8;
    const u16* bv = Ws + ((4 + h) * 32 + i) * LDW + hh * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        LFrag fk, fv; fk.u = *reinterpret_cast<const uint4*>(bk + ks * 16); fv.u = *reinterpret_cast<const uint4*>(bv + ks * 16);
        kh = DEX_MFMA_LP(af[ks].v, fk.v, kh, 0, 0, 0);
        vh = DEX_MFMA_LP(af[ks].v, fv.v, vh, 0, 0, 0);
#ifdef DEX_LP_WSPLIT
        LFrag lk, lv; lk.u = *reinterpret_cast<const uint4*>(bk + 256 * LDW + ks * 16); lv.u = *reinterpret_cast<const uint4*>(bv + 256 * LDW + ks * 16);
        kh = DEX_MFMA_LP(af[ks].v, lk.v, kh, 0, 0, 0);
        vh = DEX_MFMA_LP(af[ks].v, lv.v, vh, 0, 0, 0);
#endif
        if constexpr (KG > 0) { if ((ks + 1) % KG == 0) __builtin_amdgcn_sched_barrier(0); }
    }
    // column (channel d = lane&31) max over the 32 pixels of the sub-tile
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if constexpr (!SEED) { if (px0 + (r & 3) + 8 * (r >> 2) + 4 * hh >= npix) kh[r] = -INFINITY; }
        mx = fmaxf(mx, kh[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    // fp16 operands: the softmax reference sits 14 octaves BELOW the running maximum, so p = exp(k - ref) spans
    // [.., 2^14] and a position 2^-38 below the maximum still survives the fp16 rounding of the MFMA operand (over
    // n = 80*T positions nearly all of them sit far below the maximum); the partial's (m, s, ctx) are consistent
    // with that reference, so nothing downstream changes.  bf16 has fp32's exponent range: no shift.
    constexpr float KSHIFT = LP_IS_F16 ? 14.f * 0.69314718056f : 0.f;
    const float mn = fmaxf(m_run, mx - KSHIFT);
    const float alpha = __expf(m_run - mn);
    m_run = mn;
    const float nmn2 = -mn * LOG2E_F;
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { kh[r] = __builtin_amdgcn_exp2f(fmaf(kh[r], LOG2E_F, nmn2)); ps += kh[r]; }
    s_run = s_run * alpha + ps;
#pragma unroll
    for (int r = 0; r < 16; ++r) ctx[r] *= alpha;
    // ctx^T[e][d] += sum_px v[px][e] * p[px][d]   (A = v tile regs, B = p tile regs, same pixel order)
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
        LFrag va, pb;
        va.u.x = pack2_lp(vh[8 * k2 + 0], vh[8 * k2 + 1]); va.u.y = pack2_lp(vh[8 * k2 + 2], vh[8 * k2 + 3]);
        va.u.z = pack2_lp(vh[8 * k2 + 4], vh[8 * k2 + 5]); va.u.w = pack2_lp(vh[8 * k2 + 6], vh[8 * k2 + 7]);
        pb.u.x = pack2_lp(kh[8 * k2 + 0], kh[8 * k2 + 1]); pb.u.y = pack2_lp(kh[8 * k2 + 2], kh[8 * k2 + 3]);
        pb.u.z = pack2_lp(kh[8 * k2 + 4], kh[8 * k2 + 5]); pb.u.w = pack2_lp(kh[8 * k2 + 6], kh[8 * k2 + 7]);
        ctx = DEX_MFMA_LP(va.v, pb.v, ctx, 0, 0, 0);
    }
}

// grid (nblk, B); 256 threads; each wave owns `nsub` consecutive 32-pixel sub-tiles.
// part_m/part_s: [B][4][nblk][32], part_c: [B][4][nblk][32 d][32 e]   (same layout linattn_combine reads)
// FL >= 0 (round 5): the flags of the PRO form as COMPILE-TIME constants - bit 0 h2_bf16, bit 1 res_lp, bit 2 xout_lp, bit 3 res_under_mask.  As
// run-time (uniform) flags they became ~180 v_cndmask + both sides of every select per 32-pixel sub-tile of a VALU-bound loop; the
// launcher instantiates every combination with 16-bit h2 (the default of the reduced-precision modes) and keeps FL = -1 for the rest
// (DEX_H_BF16=0).
template <int C, bool PRO, int FL = -1>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(C == 64 ? 2 : 1, C == 64 ? 2 : 8))) void linattn_kvctx_kernel(const LinKvCtxP p) {
    constexpr int LDW = C + 8, KS = C / 16;
    extern __shared__ __attribute__((aligned(16))) u16 smem_la[];
    u16* Ws = smem_la;                                       // [256][LDW]  rows: k(4x32) then v(4x32)
    KSTAMP_DECL
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, hh = lane >> 5;
    const int blk = blockIdx.x, b = blockIdx.y;
    const u16* Wg = reinterpret_cast<const u16*>(p.Wkv);     // bf16 [256][C]
    {   // all weight loads in flight together, then the LDS stores (a load->store loop serialises 8-16 round trips)
        uint4 wr[C / 8];
#pragma unroll
        for (int j = 0; j < C / 8; ++j) {
            const int it = tid + 256 * j;
            wr[j] = *reinterpret_cast<const uint4*>(Wg + (long)(it / (C / 8)) * C + (it % (C / 8)) * 8);
        }
#pragma unroll
        for (int j = 0; j < C / 8; ++j) {
            const int it = tid + 256 * j;
            *reinterpret_cast<uint4*>(Ws + (it / (C / 8)) * LDW + (it % (C / 8)) * 8) = wr[j];
        }
#ifdef DEX_LP_WSPLIT
        // the lo halves of the same rows (p.wkv_lo_off elements behind), a second LDS image behind the first
#pragma unroll
        for (int j = 0; j < C / 8; ++j) {
            const int it = tid + 256 * j;
            wr[j] = *reinterpret_cast<const uint4*>(Wg + p.wkv_lo_off + (long)(it / (C / 8)) * C + (it % (C / 8)) * 8);
        }
#pragma unroll
        for (int j = 0; j < C / 8; ++j) {
            const int it = tid + 256 * j;
            *reinterpret_cast<uint4*>(Ws + 256 * LDW + (it / (C / 8)) * LDW + (it % (C / 8)) * 8) = wr[j];
        }
#endif
    }
    const float* X = PRO ? p.H2 + (long)b * p.npix * C : p.X + (long)b * p.xb + p.x_coff;
    const int ldx = PRO ? C : p.ldx;
    const float* R = (PRO && p.res) ? p.res + (long)b * p.resb : nullptr;
    const float* mrow = PRO ? p.mask + (long)b * p.mask_bstride : nullptr;
    const int px_base = (blk * 4 + wave) * p.nsub * 32;

    f32x16 ctxT[4];
    float m_run[4], s_run[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        m_run[h] = -INFINITY; s_run[h] = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) ctxT[h][r] = 0.f;
    }
    // x rows of the first sub-tile go out before the barrier (beside the weight loads); later sub-tiles are
    // prefetched one iteration ahead.  PRO: the rows are the raw conv output + the residual, turned into x below.
    float4 xa[KS], xc[KS], ra[PRO ? KS : 1], rc[PRO ? KS : 1];
    float mkv = 1.f;
    float ga_pre = 0.f, be_pre = 0.f;                       // GroupNorm affine of channel tid, requested with the first loads
    if constexpr (PRO) { if (tid < C) { ga_pre = p.gamma[tid]; be_pre = p.beta[tid]; } }
    const bool hb = FL >= 0 ? (FL & 1) != 0 : (PRO && p.h2_bf16 != 0);      // H2 stored as bf16: xa holds the 8 raw values until they are used
    const bool rlp = FL >= 0 ? (FL & 2) != 0 : (PRO && p.res_lp != 0);      // the residual rows likewise (ra holds 8 raw 16-bit values)
    const bool xlp = FL >= 0 ? (FL & 4) != 0 : (p.xout_lp != 0);            // x leaves in the mode's 16-bit type
    const unsigned short* Rh = (PRO && p.res) ? reinterpret_cast<const unsigned short*>(p.res) + (long)b * p.resb : nullptr;
    const unsigned short* Xh = PRO ? reinterpret_cast<const unsigned short*>(p.H2) + (long)b * p.npix * C : nullptr;
    {
        const int pxr = min(px_base + i, p.npix - 1);
        const float* xr = X + (long)pxr * ldx + hh * 8;
        if (hb) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) { xa[ks] = *reinterpret_cast<const float4*>(Xh + (long)pxr * C + hh * 8 + ks * 16); xc[ks] = xa[ks]; }
        } else {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                xa[ks] = *reinterpret_cast<const float4*>(xr + ks * 16);
                xc[ks] = *reinterpret_cast<const float4*>(xr + ks * 16 + 4);
            }
        }
        if constexpr (PRO) {
            if (R) {
                if (rlp) {
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) { ra[ks] = *reinterpret_cast<const float4*>(Rh + (long)pxr * p.ldres + hh * 8 + ks * 16); rc[ks] = ra[ks]; }
                } else {
                    const float* rr = R + (long)pxr * p.ldres + hh * 8;
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        ra[ks] = *reinterpret_cast<const float4*>(rr + ks * 16);
                        rc[ks] = *reinterpret_cast<const float4*>(rr + ks * 16 + 4);
                    }
                }
            }
            mkv = mrow[(pxr % p.W) * p.mask_ws];
        }
    }
    KSTAMP(0);
    __shared__ float smean[8], srstd[8];
    __shared__ __attribute__((aligned(16))) float gsc_s[PRO ? C : 4], gsh_s[PRO ? C : 4];   // GroupNorm folded to x*gsc + gsh per channel
    if constexpr (PRO) {
        {   // 8 groups x GN_SLOTS partials == 256 threads
            const int g = tid / GN_SLOTS;
            const longlong2 sv = *reinterpret_cast<const longlong2*>(p.gn_stats + (((long)b * 8 + g) * GN_SLOTS + (tid % GN_SLOTS)) * 2);
            long long s1 = sv.x, s2 = sv.y;
            gn_slots_reduce<GN_SLOTS>(s1, s2);
            if ((tid % GN_SLOTS) == 0) gn_moments(s1, s2, 1e-5, smean[g], srstd[g]);
        }
    }
    __syncthreads();
    if constexpr (PRO) {
        if (tid < C) {
            const float ga = ga_pre * srstd[tid / (C / 8)];
            gsc_s[tid] = ga;
            gsh_s[tid] = be_pre - smean[tid / (C / 8)] * ga;
        }
        __syncthreads();
    }
    KSTAMP(1);
    for (int sub = 0; sub < p.nsub; ++sub) {
        const int px0 = px_base + sub * 32;
        if (px0 >= p.npix) break;
        if constexpr (PRO) {
            // x = mask * (Mish(GN(h2)) + r)   (identity shortcut)   or   mask * Mish(GN(h2)) + r   (res_conv shortcut)
            const bool under = FL >= 0 ? (FL & 8) != 0 : (p.res_under_mask != 0);
            const bool live = px0 + i < p.npix;
            float* xo = p.Xout + ((long)b * p.npix + min(px0 + i, p.npix - 1)) * C + hh * 8;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                float v[8] = {xa[ks].x, xa[ks].y, xa[ks].z, xa[ks].w, xc[ks].x, xc[ks].y, xc[ks].z, xc[ks].w};
                if (hb) {
                    const unsigned u0 = __float_as_uint(xa[ks].x), u1 = __float_as_uint(xa[ks].y), u2 = __float_as_uint(xa[ks].z), u3 = __float_as_uint(xa[ks].w);
                    v[0] = lp_lo(u0); v[1] = lp_hi(u0); v[2] = lp_lo(u1); v[3] = lp_hi(u1);
                    v[4] = lp_lo(u2); v[5] = lp_hi(u2); v[6] = lp_lo(u3); v[7] = lp_hi(u3);
                }
                float r_[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                const float4 sc0 = *reinterpret_cast<const float4*>(gsc_s + ks * 16 + hh * 8), sc1 = *reinterpret_cast<const float4*>(gsc_s + ks * 16 + hh * 8 + 4);
                const float4 sh0 = *reinterpret_cast<const float4*>(gsh_s + ks * 16 + hh * 8), sh1 = *reinterpret_cast<const float4*>(gsh_s + ks * 16 + hh * 8 + 4);
                const float gsc[8] = {sc0.x, sc0.y, sc0.z, sc0.w, sc1.x, sc1.y, sc1.z, sc1.w};
                const float gsh[8] = {sh0.x, sh0.y, sh0.z, sh0.w, sh1.x, sh1.y, sh1.z, sh1.w};
                if (R) {
                    if (rlp) {
                        const unsigned u0 = __float_as_uint(ra[ks].x), u1 = __float_as_uint(ra[ks].y), u2 = __float_as_uint(ra[ks].z), u3 = __float_as_uint(ra[ks].w);
                        r_[0] = lp_lo(u0); r_[1] = lp_hi(u0); r_[2] = lp_lo(u1); r_[3] = lp_hi(u1); r_[4] = lp_lo(u2); r_[5] = lp_hi(u2); r_[6] = lp_lo(u3); r_[7] = lp_hi(u3);
                    } else { r_[0] = ra[ks].x; r_[1] = ra[ks].y; r_[2] = ra[ks].z; r_[3] = ra[ks].w; r_[4] = rc[ks].x; r_[5] = rc[ks].y; r_[6] = rc[ks].z; r_[7] = rc[ks].w; }
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float t = fmaf(v[j], gsc[j], gsh[j]);
                    const float e = __expf(fminf(t, 20.f));
                    const float n = e * (e + 2.f);
                    const float y = t * (n * __builtin_amdgcn_rcpf(n + 2.f));   // Mish (rcp: 1 ulp, bf16 consumers)
                    v[j] = under ? (y + r_[j]) * mkv : fmaf(y, mkv, r_[j]);
                }
                xa[ks] = make_float4(v[0], v[1], v[2], v[3]); xc[ks] = make_float4(v[4], v[5], v[6], v[7]);
                if (live) {
                    if (xlp) {       // 16-bit x for the tail kernel: its q operand rounds x the same way, its residual term reads the rounded value
                        u16* xh = reinterpret_cast<u16*>(p.Xout) + ((long)b * p.npix + min(px0 + i, p.npix - 1)) * C + hh * 8 + ks * 16;
                        *reinterpret_cast<uint4*>(xh) = make_uint4(pack2_lp(v[0], v[1]), pack2_lp(v[2], v[3]), pack2_lp(v[4], v[5]), pack2_lp(v[6], v[7]));
                    } else {
                        *reinterpret_cast<float4*>(xo + ks * 16) = xa[ks];
                        *reinterpret_cast<float4*>(xo + ks * 16 + 4) = xc[ks];
                    }
                }
            }
        }
        // A fragments of x: lane (pixel i, half hh) holds x[px][ks*16 + hh*8 .. +8]
        LFrag af[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            af[ks].u.x = pack2_lp(xa[ks].x, xa[ks].y); af[ks].u.y = pack2_lp(xa[ks].z, xa[ks].w);
            af[ks].u.z = pack2_lp(xc[ks].x, xc[ks].y); af[ks].u.w = pack2_lp(xc[ks].z, xc[ks].w);
        }
        if (sub + 1 < p.nsub) {
            const int pxr = min(px0 + 32 + i, p.npix - 1);
            const float* xr = X + (long)pxr * ldx + hh * 8;
            if (hb) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) { xa[ks] = *reinterpret_cast<const float4*>(Xh + (long)pxr * C + hh * 8 + ks * 16); xc[ks] = xa[ks]; }
            } else {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    xa[ks] = *reinterpret_cast<const float4*>(xr + ks * 16);
                    xc[ks] = *reinterpret_cast<const float4*>(xr + ks * 16 + 4);
                }
            }
            if constexpr (PRO) {
                if (R) {
                    if (rlp) {
#pragma unroll
                        for (int ks = 0; ks < KS; ++ks) { ra[ks] = *reinterpret_cast<const float4*>(Rh + (long)pxr * p.ldres + hh * 8 + ks * 16); rc[ks] = ra[ks]; }
                    } else {
                        const float* rr = R + (long)pxr * p.ldres + hh * 8;
#pragma unroll
                        for (int ks = 0; ks < KS; ++ks) {
                            ra[ks] = *reinterpret_cast<const float4*>(rr + ks * 16);
                            rc[ks] = *reinterpret_cast<const float4*>(rr + ks * 16 + 4);
                        }
                    }
                }
                mkv = mrow[(pxr % p.W) * p.mask_ws];
            }
        }
        KSTAMP(2);
        // head by head: k_h and v_h tiles (2 x 16 accumulator registers live instead of the 128 of all eight tiles at once -
        // the kernel sat at one wave per SIMD), softmax statistics, then ctx_h += v_h^T p_h from those registers
        // (round 6) SEED forms: the ragged last sub-tile's pixels >= npix enter as -inf seeds of the k accumulators, once per sub-tile,
        // instead of a compare + select per element and head (124 of the 537 vector instructions of this block); the 16 seed registers
        // fit beside a 16-bit residual prefetch (the batch forms), with an fp32 one the 64-channel form would spill (12 registers).
        constexpr bool SEED = C == 128 || (FL >= 0 && (FL & 2) != 0);
        f32x16 kseed;
#pragma unroll
        for (int r = 0; r < 16; ++r) kseed[r] = (SEED && px0 + (r & 3) + 8 * (r >> 2) + 4 * hh >= p.npix) ? -INFINITY : 0.f;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            f32x16 kh, vh;
#pragma unroll
            for (int r = 0; r < 16; ++r) { kh[r] = SEED ? kseed[r] : 0.f; vh[r] = 0.f; }
            const u16* bk = Ws + (h * 32 + i) * LDW + hh * 8;
            const u16* bv = Ws + ((4 + h) * 32 + i) * LDW + hh * 8;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                LFrag fk, fv; fk.u = *reinterpret_cast<const uint4*>(bk + ks * 16); fv.u = *reinterpret_cast<const uint4*>(bv + ks * 16);
                kh = DEX_MFMA_LP(af[ks].v, fk.v, kh, 0, 0, 0);
                vh = DEX_MFMA_LP(af[ks].v, fv.v, vh, 0, 0, 0);
#ifdef DEX_LP_WSPLIT
                LFrag lk, lv; lk.u = *reinterpret_cast<const uint4*>(bk + 256 * LDW + ks * 16); lv.u = *reinterpret_cast<const uint4*>(bv + 256 * LDW + ks * 16);
                kh = DEX_MFMA_LP(af[ks].v, lk.v, kh, 0, 0, 0);
                vh = DEX_MFMA_LP(af[ks].v, lv.v, vh, 0, 0, 0);
#endif
            }
            // column (channel d = lane&31) max over the 32 pixels of the sub-tile
            float mx = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if constexpr (!SEED) { if (px0 + (r & 3) + 8 * (r >> 2) + 4 * hh >= p.npix) kh[r] = -INFINITY; }
                mx = fmaxf(mx, kh[r]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            // fp16 operands: the softmax reference sits 14 octaves BELOW the running maximum, so p = exp(k - ref) spans
            // [.., 2^14] and a position 2^-38 below the maximum still survives the fp16 rounding of the MFMA operand (over
            // n = 80*T positions nearly all of them sit far below the maximum); the partial's (m, s, ctx) are consistent
            // with that reference, so nothing downstream changes.  bf16 has fp32's exponent range: no shift.
            constexpr float KSHIFT = LP_IS_F16 ? 14.f * 0.69314718056f : 0.f;
            const float mn = fmaxf(m_run[h], mx - KSHIFT);
            const float alpha = __expf(m_run[h] - mn);
            m_run[h] = mn;
            const float nmn2 = -mn * LOG2E_F;
            float ps = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) { kh[r] = __builtin_amdgcn_exp2f(fmaf(kh[r], LOG2E_F, nmn2)); ps += kh[r]; }
            s_run[h] = s_run[h] * alpha + ps;
#pragma unroll
            for (int r = 0; r < 16; ++r) ctxT[h][r] *= alpha;
            // ctx^T[e][d] += sum_px v[px][e] * p[px][d]   (A = v tile regs, B = p tile regs, same pixel order)
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2) {
                LFrag va, pb;
                va.u.x = pack2_lp(vh[8 * k2 + 0], vh[8 * k2 + 1]); va.u.y = pack2_lp(vh[8 * k2 + 2], vh[8 * k2 + 3]);
                va.u.z = pack2_lp(vh[8 * k2 + 4], vh[8 * k2 + 5]); va.u.w = pack2_lp(vh[8 * k2 + 6], vh[8 * k2 + 7]);
                pb.u.x = pack2_lp(kh[8 * k2 + 0], kh[8 * k2 + 1]); pb.u.y = pack2_lp(kh[8 * k2 + 2], kh[8 * k2 + 3]);
                pb.u.z = pack2_lp(kh[8 * k2 + 4], kh[8 * k2 + 5]); pb.u.w = pack2_lp(kh[8 * k2 + 6], kh[8 * k2 + 7]);
                ctxT[h] = DEX_MFMA_LP(va.v, pb.v, ctxT[h], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);            // keep the heads sequential: interleaving them brings all tiles back to life
        }
        KSTAMP(4);
    }
    // ---- merge the 4 waves of the workgroup through LDS, write one partial per head
    __syncthreads();                                          // weights no longer needed
    float* mS = reinterpret_cast<float*>(smem_la);            // [4 waves][4 heads][32 d][33]  ctx as [d][e]
    float* mm = mS + 4 * 4 * 32 * 33;                         // [4][4][32] m
    float* ms = mm + 4 * 4 * 32;                              // [4][4][32] s
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const float st = s_run[h] + __shfl_xor(s_run[h], 32);
        float* dst = mS + ((wave * 4 + h) * 32 + i) * 33;     // row d = lane&31
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[(r & 3) + 8 * (r >> 2) + 4 * hh] = ctxT[h][r];   // column e
        if (hh == 0) { mm[(wave * 4 + h) * 32 + i] = m_run[h]; ms[(wave * 4 + h) * 32 + i] = st; }
    }
    __syncthreads();
    KSTAMP(5);
    for (int idx = tid; idx < 4 * 1024; idx += 256) {
        const int h = idx >> 10, d = (idx >> 5) & 31, e = idx & 31;
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w) M = fmaxf(M, mm[(w * 4 + h) * 32 + d]);
        float acc = 0.f, s = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float mw = mm[(w * 4 + h) * 32 + d];
            const float f = (mw == -INFINITY) ? 0.f : __expf(mw - M);
            acc = fmaf(f, mS[((w * 4 + h) * 32 + d) * 33 + e], acc);
            s = fmaf(f, ms[(w * 4 + h) * 32 + d], s);
        }
        const long pidx = ((long)b * 4 + h) * p.nblk + blk;
        p.part_c[pidx * 1024 + d * 32 + e] = acc;
        if (e == 0) { p.part_m[pidx * 32 + d] = M; p.part_s[pidx * 32 + d] = s; }
    }
    KSTAMP(6);
    KSTAMP_STORE(7)
}

// Head-parallel form of the same pass for grids below one round of the chip's workgroup slots (B = 1..3: the form above is one long
// dependent chain per wave - prologue, then four head chains back to back - on 80-160 of the 256 CUs).  The workgroup owns the same
// 4 x nsub sub-tiles and writes the same partials; it runs 16 waves, wave = (slot, head): slot = the pixel range the form above gives
// wave `slot`, head = the one head this wave carries through every sub-tile.  Per sub-tile the prologue (GN + Mish + shortcut + mask,
// the Xout store) is split by channel quarter over the slot's four head-waves, and the bf16 x fragments go through an LDS image
// [4 slots][2 sub-tile buffers][32 px][C + 8] (double-buffered: one barrier per sub-tile).  Each head-wave then runs kv_head_step for
// its head - the same instructions on the same fragments as the form above, so every (slot, head) state and every partial is the same
// bits - and the LDS merge walks the same (h, d, e) space in the same wave order with four times the threads.
// Not in the split-weight build at C = 128: two weight images (139 KB) and the x image do not fit in the 160 KB of LDS.
// grid (nblk, B); 1024 threads.
// ROWS (launcher: DEX_KVCTX_ROWS): the prologue's 8-channel items dealt in memory order instead of lane = pixel.  The slot's four
// head-waves (256 lanes) take the sub-tile's 32 * C / 8 items as it = k * 256 + hd * 64 + lane, pixel it / (C / 8), channels
// 8 * (it % (C / 8)): a wave instruction on 16-bit rows is one contiguous 1 KB (8 lines, all of each used) where lane = pixel touches 32
// lines for 32 B of each - and so does each of the slot's other three head-waves.  The prologue is elementwise, so every element sees the
// same operations, and the x image, Xout and everything after the barrier are the same bits.
template <int C, bool PRO, int FL = -1, bool ROWS = false>
__global__ __launch_bounds__(1024) void linattn_kvctx_hw_kernel(const LinKvCtxP p) {
    constexpr int LDW = C + 8, KS = C / 16, KQ = KS / 4;      // KQ: K-steps (ROWS: items) of the prologue per head-wave lane
    constexpr int O8 = C / 8;                                  // 8-channel items per pixel row
#ifdef DEX_LP_WSPLIT
    constexpr int NWI = 2;                                     // hi + lo weight images
#else
    constexpr int NWI = 1;
#endif
    extern __shared__ __attribute__((aligned(16))) u16 smem_la[];
    u16* Ws = smem_la;                                         // [NWI][256][LDW]  rows: k(4x32) then v(4x32)
    u16* Xs = smem_la + NWI * 256 * LDW;                       // [4 slots][2][32][LDW]  bf16 x fragments of the current sub-tile
    KSTAMP_DECL
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hd = wave & 3, slot = wave >> 2;
    const int i = lane & 31, hh = lane >> 5;
    const int blk = blockIdx.x, b = blockIdx.y;
    const u16* Wg = reinterpret_cast<const u16*>(p.Wkv);       // bf16 [256][C]
    // the GroupNorm statistics and affine are requested first: they return ahead of the weights and rows, and the reduce below runs
    // while the rows are in flight (it waited behind every row before: loads return in order)
    uint4 sv = make_uint4(0u, 0u, 0u, 0u);
    float ga_pre = 0.f, be_pre = 0.f;
    if constexpr (PRO) {
        if (tid < 8 * GN_SLOTS) sv = *reinterpret_cast<const uint4*>(p.gn_stats + (((long)b * 8 + tid / GN_SLOTS) * GN_SLOTS + (tid % GN_SLOTS)) * 2);
        if (tid < C) { ga_pre = p.gamma[tid]; be_pre = p.beta[tid]; }
    }
    {
        uint4 wr[C / 32];
#pragma unroll
        for (int j = 0; j < C / 32; ++j) {
            const int it = tid + 1024 * j;
            wr[j] = *reinterpret_cast<const uint4*>(Wg + (long)(it / (C / 8)) * C + (it % (C / 8)) * 8);
        }
#pragma unroll
        for (int j = 0; j < C / 32; ++j) {
            const int it = tid + 1024 * j;
            *reinterpret_cast<uint4*>(Ws + (it / (C / 8)) * LDW + (it % (C / 8)) * 8) = wr[j];
        }
#ifdef DEX_LP_WSPLIT
#pragma unroll
        for (int j = 0; j < C / 32; ++j) {
            const int it = tid + 1024 * j;
            wr[j] = *reinterpret_cast<const uint4*>(Wg + p.wkv_lo_off + (long)(it / (C / 8)) * C + (it % (C / 8)) * 8);
        }
#pragma unroll
        for (int j = 0; j < C / 32; ++j) {
            const int it = tid + 1024 * j;
            *reinterpret_cast<uint4*>(Ws + 256 * LDW + (it / (C / 8)) * LDW + (it % (C / 8)) * 8) = wr[j];
        }
#endif
    }
    const float* X = PRO ? p.H2 + (long)b * p.npix * C : p.X + (long)b * p.xb + p.x_coff;
    const int ldx = PRO ? C : p.ldx;
    const float* R = (PRO && p.res) ? p.res + (long)b * p.resb : nullptr;
    const float* mrow = PRO ? p.mask + (long)b * p.mask_bstride : nullptr;
    const int px_base = (blk * 4 + slot) * p.nsub * 32;
    const int ch0 = hd * KQ * 16 + hh * 8;                     // this lane's first prologue channel
    // item k of this lane: pixel (of the sub-tile) and first channel
    auto ipx = [&](int k) { return ROWS ? (hd * 64 + lane) / O8 + k * (256 / O8) : i; };
    auto ich = [&](int k) { return ROWS ? 8 * (lane % O8) : ch0 + k * 16; };

    f32x16 ctxT;
    float m_run = -INFINITY, s_run = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) ctxT[r] = 0.f;
    float4 xa[KQ], xc[KQ], ra[PRO ? KQ : 1], rc[PRO ? KQ : 1];
    float mkv[ROWS ? KQ : 1];                                  // the mask value of each item's pixel (lane = pixel: one)
#pragma unroll
    for (int k = 0; k < (ROWS ? KQ : 1); ++k) mkv[k] = 1.f;
    const bool hb = FL >= 0 ? (FL & 1) != 0 : (PRO && p.h2_bf16 != 0);
    const bool rlp = FL >= 0 ? (FL & 2) != 0 : (PRO && p.res_lp != 0);
    const bool xlp = FL >= 0 ? (FL & 4) != 0 : (p.xout_lp != 0);
    const unsigned short* Rh = (PRO && p.res) ? reinterpret_cast<const unsigned short*>(p.res) + (long)b * p.resb : nullptr;
    const unsigned short* Xh = PRO ? reinterpret_cast<const unsigned short*>(p.H2) + (long)b * p.npix * C : nullptr;
    // this lane's items of the raw rows of one sub-tile (lane = pixel: pixel px0 + i, channels ch0 + 16 ks .. +8), addresses clamped
    auto load_rows = [&](int px0) {
        int pxr[KQ];
#pragma unroll
        for (int k = 0; k < KQ; ++k) pxr[k] = min(px0 + ipx(k), p.npix - 1);
        if (hb) {
#pragma unroll
            for (int k = 0; k < KQ; ++k) { xa[k] = *reinterpret_cast<const float4*>(Xh + (long)pxr[k] * C + ich(k)); xc[k] = xa[k]; }
        } else {
#pragma unroll
            for (int k = 0; k < KQ; ++k) {
                const float* xr = X + (long)pxr[k] * ldx + ich(k);
                xa[k] = *reinterpret_cast<const float4*>(xr);
                xc[k] = *reinterpret_cast<const float4*>(xr + 4);
            }
        }
        if constexpr (PRO) {
            if (R) {
                if (rlp) {
#pragma unroll
                    for (int k = 0; k < KQ; ++k) { ra[k] = *reinterpret_cast<const float4*>(Rh + (long)pxr[k] * p.ldres + ich(k)); rc[k] = ra[k]; }
                } else {
#pragma unroll
                    for (int k = 0; k < KQ; ++k) {
                        const float* rr = R + (long)pxr[k] * p.ldres + ich(k);
                        ra[k] = *reinterpret_cast<const float4*>(rr);
                        rc[k] = *reinterpret_cast<const float4*>(rr + 4);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < (ROWS ? KQ : 1); ++k) mkv[k] = mrow[(pxr[k] % p.W) * p.mask_ws];
        }
    };
    load_rows(px_base);
    KSTAMP(0);
    __shared__ float smean[8], srstd[8];
    __shared__ __attribute__((aligned(16))) float gsc_s[PRO ? C : 4], gsh_s[PRO ? C : 4];
    if constexpr (PRO) {
        if (tid < 8 * GN_SLOTS) {   // 8 groups x GN_SLOTS partials == the first 4 waves
            const int g = tid / GN_SLOTS;
            // first touch through a pinned instruction (conv_gn.h, cv_gn_finish): as a plain move it is hoisted behind the load, and
            // its s_waitcnt would stall the wave before the weight and row loads are issued
            long long s1 = (long long)(((unsigned long long)mov_pinned(sv.y) << 32) | mov_pinned(sv.x));
            long long s2 = (long long)(((unsigned long long)mov_pinned(sv.w) << 32) | mov_pinned(sv.z));
            gn_slots_reduce<GN_SLOTS>(s1, s2);
            if ((tid % GN_SLOTS) == 0) gn_moments(s1, s2, 1e-5, smean[g], srstd[g]);
        }
    }
    lds_barrier();                                             // LDS only (weight image, moments): the rows stay in flight
    if constexpr (PRO) {
        if (tid < C) {
            const float ga = ga_pre * srstd[tid / (C / 8)];
            gsc_s[tid] = ga;
            gsh_s[tid] = be_pre - smean[tid / (C / 8)] * ga;
        }
        lds_barrier();
    }
    KSTAMP(1);
    constexpr bool SEED = C == 128 || (FL >= 0 && (FL & 2) != 0);
    // every wave runs all nsub iterations (the barrier is workgroup-wide); a slot past the end skips the work
    for (int sub = 0; sub < p.nsub; ++sub) {
        const int px0 = px_base + sub * 32;
        const bool act = px0 < p.npix;
        u16* xsb = Xs + (slot * 2 + (sub & 1)) * 32 * LDW;     // the slot's image of this sub-tile; xs: this lane's fragment row
        const u16* xs = xsb + i * LDW;
        if (act) {
            if constexpr (PRO) {
                const bool under = FL >= 0 ? (FL & 8) != 0 : (p.res_under_mask != 0);
#pragma unroll
                for (int k = 0; k < KQ; ++k) {
                    const bool live = px0 + ipx(k) < p.npix;
                    const long orow = (long)b * p.npix + min(px0 + ipx(k), p.npix - 1);
                    kv_prologue8(p, xa[k], xc[k], ra[k], rc[k], gsc_s, gsh_s, ich(k), hb, rlp, R != nullptr, under, xlp, mkv[ROWS ? k : 0], live, orow);
                }
            }
#pragma unroll
            for (int k = 0; k < KQ; ++k)
                *reinterpret_cast<uint4*>(xsb + ipx(k) * LDW + ich(k)) =
                    make_uint4(pack2_lp(xa[k].x, xa[k].y), pack2_lp(xa[k].z, xa[k].w), pack2_lp(xc[k].x, xc[k].y), pack2_lp(xc[k].z, xc[k].w));
            if (sub + 1 < p.nsub) load_rows(px0 + 32);
        }
        KSTAMP(2);
        __syncthreads();                                       // the slot's x image is complete (and the image of sub - 1 is free)
        KSTAMP(3);
        if (!act) continue;
        LFrag af[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) af[ks].u = *reinterpret_cast<const uint4*>(xs + ks * 16 + hh * 8);
        f32x16 kseed;
#pragma unroll
        for (int r = 0; r < 16; ++r) kseed[r] = (SEED && px0 + (r & 3) + 8 * (r >> 2) + 4 * hh >= p.npix) ? -INFINITY : 0.f;
        kv_head_step<C, SEED, (C == 128 ? 4 : 0)>(Ws, hd, i, hh, af, kseed, px0, p.npix, ctxT, m_run, s_run);   // (C = 128: 128 registers, no spill)
        KSTAMP(4);
    }
    // ---- merge: the same LDS layout and walk as the form above, wave `slot` of that form = slot here
    __syncthreads();
    float* mS = reinterpret_cast<float*>(smem_la);             // [4 slots][4 heads][32 d][33]  ctx as [d][e]
    float* mm = mS + 4 * 4 * 32 * 33;
    float* ms = mm + 4 * 4 * 32;
    {
        const float st = s_run + __shfl_xor(s_run, 32);
        float* dst = mS + ((slot * 4 + hd) * 32 + i) * 33;
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[(r & 3) + 8 * (r >> 2) + 4 * hh] = ctxT[r];
        if (hh == 0) { mm[(slot * 4 + hd) * 32 + i] = m_run; ms[(slot * 4 + hd) * 32 + i] = st; }
    }
    __syncthreads();
    KSTAMP(5);
    for (int idx = tid; idx < 4 * 1024; idx += 1024) {
        const int h = idx >> 10, d = (idx >> 5) & 31, e = idx & 31;
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w) M = fmaxf(M, mm[(w * 4 + h) * 32 + d]);
        float acc = 0.f, s = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float mw = mm[(w * 4 + h) * 32 + d];
            const float f = (mw == -INFINITY) ? 0.f : __expf(mw - M);
            acc = fmaf(f, mS[((w * 4 + h) * 32 + d) * 33 + e], acc);
            s = fmaf(f, ms[(w * 4 + h) * 32 + d], s);
        }
        const long pidx = ((long)b * 4 + h) * p.nblk + blk;
        p.part_c[pidx * 1024 + d * 32 + e] = acc;
        if (e == 0) { p.part_m[pidx * 32 + d] = M; p.part_s[pidx * 32 + d] = s; }
    }
    KSTAMP(6);
    KSTAMP_STORE(7)
}

// The instantiation a context-pass launch takes, as text (g_last_form): kernel, C, PRO, FL, and ROWS of the head-parallel form.
static const char* kvctx_form(bool hw, int C, bool pro, int fl, bool rows) {
#define KVF_ROW(K, CC, RW)                                                                                                            \
    { K " C=" #CC " PRO=0 FL=-1" RW, K " C=" #CC " PRO=1 FL=-1" RW, K " C=" #CC " PRO=1 FL=1" RW, K " C=" #CC " PRO=1 FL=3" RW,        \
      K " C=" #CC " PRO=1 FL=5" RW, K " C=" #CC " PRO=1 FL=7" RW, K " C=" #CC " PRO=1 FL=9" RW, K " C=" #CC " PRO=1 FL=11" RW,         \
      K " C=" #CC " PRO=1 FL=13" RW, K " C=" #CC " PRO=1 FL=15" RW }
    static const char* const names[6][10] = {
        KVF_ROW("linattn_kvctx_kernel", 64, ""), KVF_ROW("linattn_kvctx_kernel", 128, ""),
        KVF_ROW("linattn_kvctx_hw_kernel", 64, " ROWS=0"), KVF_ROW("linattn_kvctx_hw_kernel", 128, " ROWS=0"),
        KVF_ROW("linattn_kvctx_hw_kernel", 64, " ROWS=1"), KVF_ROW("linattn_kvctx_hw_kernel", 128, " ROWS=1") };
#undef KVF_ROW
    const int col = !pro ? 0 : (fl >= 1 && fl <= 15 && (fl & 1)) ? 2 + fl / 2 : 1;       // the launchers' switch: odd FL = 16-bit H2
    return names[(hw ? 2 + (rows ? 2 : 0) : 0) + (C == 128 ? 1 : 0)][col];
}
// the head-parallel form exists for every C of every build but the split-weight one at C = 128 (LDS)
static bool kvctx_hw_supported(int C) {
#ifdef DEX_LP_WSPLIT
    return C == 64;
#else
    return C == 64 || C == 128;
#endif
}
template <int CC, bool ROWS>
static void launch_kvctx_hw(const LinKvCtxP& p, int fl, bool pro, dim3 grid, size_t lds, hipStream_t st) {
    constexpr int LDS_HW = 144 * 1024;
    static bool attr = false;
    if (!attr) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&linattn_kvctx_hw_kernel<CC, false, -1, ROWS>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_HW);
        hipFuncSetAttribute(reinterpret_cast<const void*>(&linattn_kvctx_hw_kernel<CC, true, -1, ROWS>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_HW);
#define KVHW_ATTR(F) hipFuncSetAttribute(reinterpret_cast<const void*>(&linattn_kvctx_hw_kernel<CC, true, F, ROWS>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_HW);
        KVHW_ATTR(1) KVHW_ATTR(3) KVHW_ATTR(5) KVHW_ATTR(7) KVHW_ATTR(9) KVHW_ATTR(11) KVHW_ATTR(13) KVHW_ATTR(15)
#undef KVHW_ATTR
        attr = true;
    }
#define KVHW_CASE(F) case F: hipLaunchKernelGGL((linattn_kvctx_hw_kernel<CC, true, F, ROWS>), grid, dim3(1024), lds, st, p); break;
    switch (fl) {
        KVHW_CASE(1) KVHW_CASE(3) KVHW_CASE(5) KVHW_CASE(7) KVHW_CASE(9) KVHW_CASE(11) KVHW_CASE(13) KVHW_CASE(15)
        default:
            if (pro) hipLaunchKernelGGL((linattn_kvctx_hw_kernel<CC, true, -1, ROWS>), grid, dim3(1024), lds, st, p);
            else hipLaunchKernelGGL((linattn_kvctx_hw_kernel<CC, false, -1, ROWS>), grid, dim3(1024), lds, st, p);
    }
#undef KVHW_CASE
}
// p.rows (DEX_KVCTX_ROWS): the memory-order deal of the prologue's items; 0 = lane = pixel
template <int CC>
static void launch_kvctx_hw(const LinKvCtxP& p, int fl, bool pro, dim3 grid, size_t lds, hipStream_t st) {
    if (p.rows) launch_kvctx_hw<CC, true>(p, fl, pro, grid, lds, st);
    else launch_kvctx_hw<CC, false>(p, fl, pro, grid, lds, st);
}

void launch_linattn_kvctx(const LinKvCtxP& p, hipStream_t st) {
#ifdef DEX_LP_WSPLIT
    const size_t lds_w = (size_t)2 * 256 * (p.C + 8) * sizeof(u16);          // hi + lo images of the k | v rows
    constexpr int LDS_MAX = 144 * 1024;
#else
    const size_t lds_w = (size_t)256 * (p.C + 8) * sizeof(u16);
    constexpr int LDS_MAX = 96 * 1024;
#endif
    const size_t lds_m = (size_t)(4 * 4 * 32 * 33 + 2 * 4 * 4 * 32) * sizeof(float);
    const size_t lds = lds_w > lds_m ? lds_w : lds_m;
    static bool attr = false;
    if (!attr) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&linattn_kvctx_kernel<64, false>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
        hipFuncSetAttribute(reinterpret_cast<const void*>(&linattn_kvctx_kernel<128, false>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
        hipFuncSetAttribute(reinterpret_cast<const void*>(&linattn_kvctx_kernel<64, true>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
        hipFuncSetAttribute(reinterpret_cast<const void*>(&linattn_kvctx_kernel<128, true>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
#define KVCTX_ATTR(CC, F) hipFuncSetAttribute(reinterpret_cast<const void*>(&linattn_kvctx_kernel<CC, true, F>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
        KVCTX_ATTR(64, 1) KVCTX_ATTR(64, 3) KVCTX_ATTR(64, 5) KVCTX_ATTR(64, 7) KVCTX_ATTR(64, 9) KVCTX_ATTR(64, 11) KVCTX_ATTR(64, 13) KVCTX_ATTR(64, 15)
        KVCTX_ATTR(128, 1) KVCTX_ATTR(128, 3) KVCTX_ATTR(128, 5) KVCTX_ATTR(128, 7) KVCTX_ATTR(128, 9) KVCTX_ATTR(128, 11) KVCTX_ATTR(128, 13) KVCTX_ATTR(128, 15)
#undef KVCTX_ATTR
        attr = true;
    }
    dim3 grid(p.nblk, p.B);
    const bool pro = p.H2 != nullptr;
    const int fl = pro ? (p.h2_bf16 != 0 ? 1 : 0) | (p.res_lp != 0 ? 2 : 0) | (p.xout_lp != 0 ? 4 : 0) | (p.res_under_mask != 0 ? 8 : 0) : -1;
    if (p.headwaves && kvctx_hw_supported(p.C)) {
        g_last_symbol = "linattn_kvctx_hw_kernel";
        g_last_form = kvctx_form(true, p.C, pro, fl, p.rows != 0);
        // weight image(s) + the x image [4][2][32][C + 8]; the merge reuses the same bytes
        const size_t lds_hw = lds_w + (size_t)4 * 2 * 32 * (p.C + 8) * sizeof(u16);
        const size_t lds2 = lds_hw > lds_m ? lds_hw : lds_m;
#ifdef DEX_LP_WSPLIT
        launch_kvctx_hw<64>(p, fl, pro, grid, lds2, st);
#else
        if (p.C == 64) launch_kvctx_hw<64>(p, fl, pro, grid, lds2, st);
        else launch_kvctx_hw<128>(p, fl, pro, grid, lds2, st);
#endif
        return;
    }
#define KVCTX_CASE(CC, F) case F: hipLaunchKernelGGL((linattn_kvctx_kernel<CC, true, F>), grid, dim3(256), lds, st, p); break;
#define KVCTX_LAUNCH(CC)                                                                                                              \
    switch (fl) {                                                                                                                      \
        KVCTX_CASE(CC, 1) KVCTX_CASE(CC, 3) KVCTX_CASE(CC, 5) KVCTX_CASE(CC, 7) KVCTX_CASE(CC, 9) KVCTX_CASE(CC, 11) KVCTX_CASE(CC, 13) KVCTX_CASE(CC, 15)   \
        default:                                                                                                                       \
            if (pro) hipLaunchKernelGGL((linattn_kvctx_kernel<CC, true>), grid, dim3(256), lds, st, p);                                \
            else hipLaunchKernelGGL((linattn_kvctx_kernel<CC, false>), grid, dim3(256), lds, st, p);                                   \
    }
    g_last_symbol = "linattn_kvctx_kernel";
    g_last_form = kvctx_form(false, p.C, pro, fl, false);
    if (p.C == 64) { KVCTX_LAUNCH(64) } else { KVCTX_LAUNCH(128) }
#undef KVCTX_LAUNCH
#undef KVCTX_CASE
}

// grid (4 heads, B, 32 rows d): merge the workgroup partials of ONE context row -> normalised ctx[b][h][d][:], then
// fold it with the output projection:  W2[co][h*32+d] = g * sum_e Wout[co][h*32+e] * ctx[h][d][e]   (one column of
// W2 = g * Wout * blockdiag(ctx^T) per workgroup).  W2 is written as bf16 in the A-fragment order the tail kernel
// consumes: he index permuted to the accumulator row order of the q^T tiles (see linattn_out2_kernel).
// thread = (column e = tid%32, partial lane pl = tid/32): 8 lanes stride the partial list with independent loads.
template <int MC>
__device__ __forceinline__ void merge_fold(const LinMergeP& p, long pbase, int d, int e, int pl, float& m, float& acc, float& s) {
    for (int c0 = 0; c0 < p.nblk; c0 += 8 * MC) {
        float pm[MC], ps[MC], pc[MC];
#pragma unroll
        for (int k = 0; k < MC; ++k) {
            const int c = min(c0 + pl + 8 * k, p.nblk - 1);           // clamped: loads are unconditional
            pm[k] = p.part_m[(pbase + c) * 32 + d];
            ps[k] = p.part_s[(pbase + c) * 32 + d];
            pc[k] = p.part_c[(pbase + c) * 1024 + d * 32 + e];
        }
#pragma unroll
        for (int k = 0; k < MC; ++k) {
            if (c0 + pl + 8 * k < p.nblk) {
                const float mn = fmaxf(m, pm[k]);
                const float a = (m == -INFINITY) ? 0.f : __expf(m - mn);
                const float w = (pm[k] == -INFINITY) ? 0.f : __expf(pm[k] - mn);
                acc = fmaf(acc, a, w * pc[k]);
                s = fmaf(s, a, w * ps[k]);
                m = mn;
            }
        }
    }
}

__global__ __launch_bounds__(256) void linattn_merge_kernel(const LinMergeP p) {
    __shared__ float redm[8], reda[8][32], reds[8], cvec[32];
    const int tid = threadIdx.x, h = blockIdx.x, b = blockIdx.y, d = blockIdx.z;
    const int C = p.C;
    // this thread's Wout row slice (co = tid): 32 floats, in flight under the partial merge
    float4 wo[8];
    if (tid < C) {
#pragma unroll
        for (int j = 0; j < 8; ++j) wo[j] = *reinterpret_cast<const float4*>(p.Wout + (long)tid * 128 + h * 32 + j * 4);
    }
    const float g = p.g[0];
    const long pbase = ((long)b * 4 + h) * p.nblk;
    const int e = tid & 31, pl = tid >> 5;
    // ONE pass: every lane first requests its whole share of the partial list (up to MC entries per round, all loads
    // in flight together), then folds them with a running maximum (flash-style).  The two-pass form (maximum, then
    // weighted sum) walked the list twice in rounds of 8 dependent-latency loads: 9.3 us at 160 partials, B=1.
    float m = -INFINITY, acc = 0.f, s = 0.f;
    const int per_lane = (p.nblk + 7) / 8;
    if (per_lane <= 8) merge_fold<8>(p, pbase, d, e, pl, m, acc, s);
    else if (per_lane <= 16) merge_fold<16>(p, pbase, d, e, pl, m, acc, s);
    else merge_fold<24>(p, pbase, d, e, pl, m, acc, s);
    if (e == 0) { redm[pl] = m; reds[pl] = s; }
    reda[pl][e] = acc;
    __syncthreads();
    if (pl == 0) {
        float M = redm[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) M = fmaxf(M, redm[k]);
        float a = 0.f, ss = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float w = (redm[k] == -INFINITY) ? 0.f : __expf(redm[k] - M);
            a = fmaf(w, reda[k][e], a); ss = fmaf(w, reds[k], ss);
        }
        cvec[e] = a / ss;
    }
    __syncthreads();
    if (tid < C) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            a = fmaf(wo[j].x, cvec[j * 4 + 0], a); a = fmaf(wo[j].y, cvec[j * 4 + 1], a);
            a = fmaf(wo[j].z, cvec[j * 4 + 2], a); a = fmaf(wo[j].w, cvec[j * 4 + 3], a);
        }
        a *= g;
        // fragment slot of (co = tid, he = h*32 + d):  d = (j&3) + 8*(2*ksl + (j>>2)) + 4*hh
        const int co = tid, hh = (d >> 2) & 1, j = (d & 3) + 4 * ((d >> 3) & 1), ks = 2 * h + (d >> 4);
        const long dst = ((((long)b * (C / 32) + (co >> 5)) * 8 + ks) * 64 + hh * 32 + (co & 31)) * 8 + j;
        reinterpret_cast<u16*>(p.W2)[dst] = (u16)(pack2_lp(a, 0.f) & 0xffffu);
    }
}
void launch_linattn_merge(const LinMergeP& p, hipStream_t st) {
    hipLaunchKernelGGL(linattn_merge_kernel, dim3(4, p.B, 32), dim3(256), 0, st, p);
}

// Tail, latency form (small grids): y = x + W2 (Wq x) + g*b per pixel, as two chained MFMA GEMMs computed TRANSPOSED so that no operand ever
// needs a layout change:  q^T[he][px] = Wq[he][:] . x[px][:]  (A = Wq rows, B = x rows),  then
// y^T[co][px] = sum_he W2[co][he] q^T[he][px]  (A = W2, B = the q^T accumulators re-used in place: a lane already
// holds, for its pixel column, 8 he values per K-step — in accumulator row order, which is why W2 is stored with
// that permutation).  Each wave owns 32 pixels end to end: no LDS, no barrier, every global load issued up front
// (at B=1 the LDS-staged form below costs 1.5 % end to end: one more dependent round trip in a latency-bound chain).
// grid (ceil(npix/128), B), 256 threads.
template <int C>
__global__ __launch_bounds__(256) void linattn_out2_direct_kernel(const LinOut2P p) {
    constexpr int KS1 = C / 16, CT = C / 32;
    KSTAMP_DECL
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, hh = lane >> 5;
    const int b = blockIdx.y;
    const int px0 = (blockIdx.x * 4 + wave) * 32;
    if (px0 >= p.npix) return;
    const float* X = p.X + (long)b * p.xb + p.x_coff;
    const int px = min(px0 + i, p.npix - 1);
    // B fragments of GEMM1: lane (pixel column i, half hh) holds x[px][ks*16 + hh*8 .. +8]
    const float* xr = X + (long)px * p.ldx + hh * 8;
    float4 xa[KS1], xc[KS1];
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks) {
        xa[ks] = *reinterpret_cast<const float4*>(xr + ks * 16);
        xc[ks] = *reinterpret_cast<const float4*>(xr + ks * 16 + 4);
    }
    // A fragments of GEMM2 (all of W2 for this utterance: CT x 8 K-steps)
    const uint4* w2 = reinterpret_cast<const uint4*>(p.W2) + (long)b * CT * 8 * 64 + lane;
    uint4 w2f[CT][8];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) w2f[ct][ks] = w2[(ct * 8 + ks) * 64];
    KSTAMP(0);
    LFrag xf[KS1];
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks) {
        xf[ks].u.x = pack2_lp(xa[ks].x, xa[ks].y); xf[ks].u.y = pack2_lp(xa[ks].z, xa[ks].w);
        xf[ks].u.z = pack2_lp(xc[ks].x, xc[ks].y); xf[ks].u.w = pack2_lp(xc[ks].z, xc[ks].w);
    }
    // ---- GEMM1: q^T, four 32-row he tiles; converted to bf16 B fragments tile by tile
    const uint4* wq = reinterpret_cast<const uint4*>(p.Wq) + lane;                  // bf16, fragment order [he tile][K-step][lane][8]
    LFrag qf[8];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        f32x16 q;
#pragma unroll
        for (int r = 0; r < 16; ++r) q[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS1; ++ks) {
            LFrag af; af.u = wq[(t * KS1 + ks) * 64];
            q = DEX_MFMA_LP(af.v, xf[ks].v, q, 0, 0, 0);
#ifdef DEX_LP_WSPLIT
            LFrag al; al.u = wq[(t * KS1 + ks) * 64 + p.wq_lo_off / 8];       // the lo half of the same fragment
            q = DEX_MFMA_LP(al.v, xf[ks].v, q, 0, 0, 0);
#endif
        }
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
            qf[t * 2 + k2].u.x = pack2_lp(q[8 * k2 + 0], q[8 * k2 + 1]); qf[t * 2 + k2].u.y = pack2_lp(q[8 * k2 + 2], q[8 * k2 + 3]);
            qf[t * 2 + k2].u.z = pack2_lp(q[8 * k2 + 4], q[8 * k2 + 5]); qf[t * 2 + k2].u.w = pack2_lp(q[8 * k2 + 6], q[8 * k2 + 7]);
        }
    }
    KSTAMP(2);
    // ---- GEMM2 + epilogue: rows co = ct*32 + (r&3) + 8*(r>>2) + 4*hh  ->  4 consecutive channels per register quad
    float* Y = p.Y + (long)b * p.yb + p.y_coff;
    const bool ok = px0 + i < p.npix;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        f32x16 y;
#pragma unroll
        for (int r = 0; r < 16; ++r) y[r] = 0.f;
        float4 res[4], bia[4];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int co = ct * 32 + 8 * g4 + 4 * hh;
            res[g4] = *reinterpret_cast<const float4*>(X + (long)px * p.ldx + co);
            bia[g4] = *reinterpret_cast<const float4*>(p.bias + co);
        }
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            LFrag af; af.u = w2f[ct][ks];
            y = DEX_MFMA_LP(af.v, qf[ks].v, y, 0, 0, 0);
        }
        KSTAMP(4);
        if (ok) {
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int co = ct * 32 + 8 * g4 + 4 * hh;
                float4 o;
                o.x = y[g4 * 4 + 0] + res[g4].x + bia[g4].x; o.y = y[g4 * 4 + 1] + res[g4].y + bia[g4].y;
                o.z = y[g4 * 4 + 2] + res[g4].z + bia[g4].z; o.w = y[g4 * 4 + 3] + res[g4].w + bia[g4].w;
                *reinterpret_cast<float4*>(Y + (long)(px0 + i) * p.ldy + co) = o;
            }
        }
        KSTAMP(5);
    }
    KSTAMP_STORE(7)
}

// Tail, wave-split latency form (small grids): the direct form's work for one 32-pixel slot spread over the four waves of a workgroup.
//   x:     wave t loads and rounds K-quarter t of the slot's x fragments (the direct form's pack2_lp), shared through LDS;
//   GEMM1: wave t computes q^T he tile t - the direct form's chain, same K order and operands (split-weight build: hi then lo per
//          fragment) - and packs it to the same B fragments, shared through LDS;
//   GEMM2: wave t < C/32 runs the whole 8-K-step chain of co tile t, then that tile's epilogue (y + residual + bias in the same order).
// Every output is the direct form's bits.  Each wave fetches only its own Wq tile and W2 co tile (C = 128: 8 + 8 KB instead of 64 KB), all
// issued at entry; the bias comes through the scalar cache, and at C = 128 the residual of co tile t is wave t's own x quarter (the two
// pixel halves trade the other half of their 8-channel runs), so that form issues 20 vector loads per wave where the direct one issues 112.
// At 40x256 the grid covers the CUs instead of 80 of them.  (Four slots per 16-wave workgroup, the same 80 workgroups as the direct form,
// measured slower: 10.4 against 6.4 us at 40x256 C = 128 - DESIGN.md section 8.)
// fp32 X and Y only (no x_lp / y_lp / Y2: the direct form's regime).  grid (ceil(npix / 32), B), 256 threads.
// ROWS (launcher: DEX_OUT2_ROWS): x and y move as whole pixel rows.  Wave t takes pixels 8t .. 8t + 7 of the slot: lane = (pixel, channel
// octet) in memory order, so a wave instruction covers contiguous rows (8 x 512 B at C = 128 in two instructions per half octet) where
// lane = pixel touches 32 lines per instruction.  It rounds each octet with the same pack2_lp into the same fragment image (the halves of
// a K-step 33 entries apart: the octets of one pixel land on different banks), keeps its fp32 rows as the residual, and the epilogue goes
// the same way back: the co tiles are staged as an fp32 image [32 px][C + 4], then every wave forms (y + residual) + bias for its eight
// rows and stores them as contiguous requests.  The GEMM chains are untouched, the sums are the direct form's in the direct form's order.
template <int C, bool ROWS = false>
__global__ __launch_bounds__(256) void linattn_out2_hw_kernel(const LinOut2P p) {
    constexpr int KS1 = C / 16, CT = C / 32, KQ = KS1 / 4;     // KQ: x K-steps (ROWS: row octets) loaded per wave lane
    constexpr int O8 = C / 8, XH = ROWS ? 33 : 32, LDY = C + 4;
    __shared__ uint4 xs[KS1][2 * XH], qs[8][64];               // lane-indexed fragment images: conflict-free b128
    __shared__ __attribute__((aligned(16))) float ys[ROWS ? 32 * LDY : 4];      // ROWS: the y^T tiles as pixel rows
    KSTAMP_DECL
    const int tid = threadIdx.x, lane = tid & 63;
    const int t = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, hh = lane >> 5;
    const int fi = hh * XH + i;                                // this lane's entry of a fragment image row
    const int b = blockIdx.y;
    const int px0 = blockIdx.x * 32;
    if (px0 >= p.npix) return;
    const float* X = p.X + (long)b * p.xb + p.x_coff;
    const int px = min(px0 + i, p.npix - 1);
    // ROWS: item k of this lane = pixel 8t + rp0 + k * (64 / O8) of the slot, channels rch .. rch + 7
    const int rp0 = 8 * t + lane / O8, rch = 8 * (lane % O8);
    // every global load of the wave at entry: its x quarter, its Wq tile, its W2 co tile (+ C = 64: its residual rows), the bias
    float4 xa[KQ], xc[KQ];
    if constexpr (ROWS) {
#pragma unroll
        for (int k = 0; k < KQ; ++k) {
            const float* xr = X + (long)min(px0 + rp0 + k * (64 / O8), p.npix - 1) * p.ldx + rch;
            xa[k] = *reinterpret_cast<const float4*>(xr);
            xc[k] = *reinterpret_cast<const float4*>(xr + 4);
        }
    } else {
        const float* xr = X + (long)px * p.ldx + hh * 8;
#pragma unroll
        for (int k = 0; k < KQ; ++k) {
            const int ks = t * KQ + k;
            xa[k] = *reinterpret_cast<const float4*>(xr + ks * 16);
            xc[k] = *reinterpret_cast<const float4*>(xr + ks * 16 + 4);
        }
    }
    const uint4* wq = reinterpret_cast<const uint4*>(p.Wq) + lane;                  // bf16, fragment order [he tile][K-step][lane][8]
    uint4 wqf[KS1];
#ifdef DEX_LP_WSPLIT
    uint4 wql[KS1];
#endif
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks) {
        wqf[ks] = wq[(t * KS1 + ks) * 64];
#ifdef DEX_LP_WSPLIT
        wql[ks] = wq[(t * KS1 + ks) * 64 + p.wq_lo_off / 8];                         // the lo half of the same fragment
#endif
    }
    const bool g2 = t < CT;                                     // (uniform) this wave owns co tile t
    const int ct = g2 ? t : 0;
    const uint4* w2 = reinterpret_cast<const uint4*>(p.W2) + (long)b * CT * 8 * 64 + lane;
    uint4 w2f[8];
    float4 res[4], bia[4];
    if (g2) {
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) w2f[ks] = w2[(ct * 8 + ks) * 64];
    }
    if constexpr (ROWS) {
        // the bias of this lane's octet (every item of a lane has the same channels)
        bia[0] = *reinterpret_cast<const float4*>(p.bias + rch);
        bia[1] = *reinterpret_cast<const float4*>(p.bias + rch + 4);
    } else if (g2) {
        if constexpr (C != 128) {
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) res[g4] = *reinterpret_cast<const float4*>(X + (long)px * p.ldx + ct * 32 + 8 * g4 + 4 * hh);
        }
        // the bias through the scalar cache: a uniform load of the tile's 32 channels, then each half keeps its 4 of every 8 (a bit blend:
        // written as a select, the pair of loads was folded into ONE load from a selected address - a private array in scratch)
        const float4* bt = reinterpret_cast<const float4*>(p.bias + ct * 32);
        const unsigned hm = 0u - (unsigned)hh;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const float4 b0 = bt[2 * g4], b1 = bt[2 * g4 + 1];
            bia[g4] = make_float4(__uint_as_float((__float_as_uint(b1.x) & hm) | (__float_as_uint(b0.x) & ~hm)),
                                  __uint_as_float((__float_as_uint(b1.y) & hm) | (__float_as_uint(b0.y) & ~hm)),
                                  __uint_as_float((__float_as_uint(b1.z) & hm) | (__float_as_uint(b0.z) & ~hm)),
                                  __uint_as_float((__float_as_uint(b1.w) & hm) | (__float_as_uint(b0.w) & ~hm)));
        }
    }
    KSTAMP(0);
    // ---- x quarter (ROWS: x rows) -> the slot's fragment image
#pragma unroll
    for (int k = 0; k < KQ; ++k) {
        LFrag f;
        f.u.x = pack2_lp(xa[k].x, xa[k].y); f.u.y = pack2_lp(xa[k].z, xa[k].w);
        f.u.z = pack2_lp(xc[k].x, xc[k].y); f.u.w = pack2_lp(xc[k].z, xc[k].w);
        if constexpr (ROWS) xs[rch >> 4][((rch >> 3) & 1) * XH + rp0 + k * (64 / O8)] = f.u;
        else xs[t * KQ + k][fi] = f.u;
    }
    if constexpr (C == 128 && !ROWS) {
        // wave t's x quarter is channels 32t .. 32t + 31 of its pixel = the residual of co tile t: lane half hh holds channels
        // 16k + 8hh + 0..7 (k = 0, 1) and needs 8 g4 + 4hh + 0..3; the halves swap the 4 channels the other one needs (exact copies)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float4 snd = hh ? xa[k] : xc[k];
            float4 rcv;
            rcv.x = __shfl_xor(snd.x, 32); rcv.y = __shfl_xor(snd.y, 32); rcv.z = __shfl_xor(snd.z, 32); rcv.w = __shfl_xor(snd.w, 32);
            res[2 * k] = hh ? rcv : xa[k];
            res[2 * k + 1] = hh ? xc[k] : rcv;
        }
    }
    lds_barrier();                                             // LDS only: the Wq, W2, residual and bias loads stay in flight
    KSTAMP(1);
    // ---- GEMM1: q^T he tile t
    {
        f32x16 q;
#pragma unroll
        for (int r = 0; r < 16; ++r) q[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS1; ++ks) {
            LFrag af, xf; af.u = wqf[ks]; xf.u = xs[ks][fi];
            q = DEX_MFMA_LP(af.v, xf.v, q, 0, 0, 0);
#ifdef DEX_LP_WSPLIT
            LFrag al; al.u = wql[ks];
            q = DEX_MFMA_LP(al.v, xf.v, q, 0, 0, 0);
#endif
        }
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
            LFrag f;
            f.u.x = pack2_lp(q[8 * k2 + 0], q[8 * k2 + 1]); f.u.y = pack2_lp(q[8 * k2 + 2], q[8 * k2 + 3]);
            f.u.z = pack2_lp(q[8 * k2 + 4], q[8 * k2 + 5]); f.u.w = pack2_lp(q[8 * k2 + 6], q[8 * k2 + 7]);
            qs[t * 2 + k2][lane] = f.u;
        }
    }
    KSTAMP(2);
    lds_barrier();
    KSTAMP(3);
    if constexpr (!ROWS) { if (!g2) return; }
    // ---- GEMM2 + epilogue of co tile t: rows co = ct*32 + (r&3) + 8*(r>>2) + 4*hh  ->  4 consecutive channels per register quad
    f32x16 y;
    if (g2) {
#pragma unroll
        for (int r = 0; r < 16; ++r) y[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            LFrag af, qf; af.u = w2f[ks]; qf.u = qs[ks][lane];
            y = DEX_MFMA_LP(af.v, qf.v, y, 0, 0, 0);
        }
    }
    KSTAMP(4);
    float* Y = p.Y + (long)b * p.yb + p.y_coff;
    if constexpr (ROWS) {
        if (g2) {
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *reinterpret_cast<float4*>(ys + i * LDY + ct * 32 + 8 * g4 + 4 * hh) = make_float4(y[g4 * 4 + 0], y[g4 * 4 + 1], y[g4 * 4 + 2], y[g4 * 4 + 3]);
        }
        lds_barrier();                                         // the slot's y image is complete
#pragma unroll
        for (int k = 0; k < KQ; ++k) {
            const int rp = rp0 + k * (64 / O8);
            const float4 ya = *reinterpret_cast<const float4*>(ys + rp * LDY + rch), yc = *reinterpret_cast<const float4*>(ys + rp * LDY + rch + 4);
            if (px0 + rp < p.npix) {
                float4 oa, oc;
                oa.x = ya.x + xa[k].x + bia[0].x; oa.y = ya.y + xa[k].y + bia[0].y; oa.z = ya.z + xa[k].z + bia[0].z; oa.w = ya.w + xa[k].w + bia[0].w;
                oc.x = yc.x + xc[k].x + bia[1].x; oc.y = yc.y + xc[k].y + bia[1].y; oc.z = yc.z + xc[k].z + bia[1].z; oc.w = yc.w + xc[k].w + bia[1].w;
                float* yr = Y + (long)(px0 + rp) * p.ldy + rch;
                *reinterpret_cast<float4*>(yr) = oa;
                *reinterpret_cast<float4*>(yr + 4) = oc;
            }
        }
    } else if (px0 + i < p.npix) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int co = ct * 32 + 8 * g4 + 4 * hh;
            float4 o;
            o.x = y[g4 * 4 + 0] + res[g4].x + bia[g4].x; o.y = y[g4 * 4 + 1] + res[g4].y + bia[g4].y;
            o.z = y[g4 * 4 + 2] + res[g4].z + bia[g4].z; o.w = y[g4 * 4 + 3] + res[g4].w + bia[g4].w;
            *reinterpret_cast<float4*>(Y + (long)(px0 + i) * p.ldy + co) = o;
        }
    }
    KSTAMP(5);
    KSTAMP_STORE(7)
}
// Tail, throughput form (large grids: +1.2 % end to end at B=32): y = x + W2 (Wq x) + g*b per pixel, two chained MFMA GEMMs computed TRANSPOSED so that no operand ever
// needs a layout change:  q^T[he][px] = Wq[he][:] . x[px][:]  (A = Wq rows, B = x rows),  then
// y^T[co][px] = sum_he W2[co][he] q^T[he][px]  (A = W2, B = the q^T accumulators re-used in place: a lane already
// holds, for its pixel column, 8 he values per K-step — in accumulator row order, which is why W2 is stored with
// that permutation).  Each wave owns 32 pixels end to end, no workgroup barrier.
// The x tile goes through a WAVE-PRIVATE LDS image: the MFMA layouts have a lane own 8 (operand) or 4 (result) channels
// of ONE pixel, so direct loads/stores touch 32 cache lines per instruction and use 16-32 bytes of each (x: 8 loads,
// residual re-read: 4*CT, y: 4*CT stores — ~770 line touches per tile for 128 lines of data, and this kernel is bound by
// the CU's address/line rate).  Through LDS every global instruction moves 1 KB of contiguous pixels (8 lines), the
// residual comes from the image, and y is staged in place over it.
// grid (ceil(npix/128), B), 256 threads, dynamic LDS 4 * 32 * (C + 4) floats.
template <int C>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, C == 64 ? 4 : 2))) void linattn_out2_kernel(const LinOut2P p) {
    constexpr int KS1 = C / 16, CT = C / 32;
    constexpr int LDX = C + 4;                          // floats: row stride 4 mod 64 dwords -> conflict-free b128 rows
    constexpr int NCH = 32 * C / 4 / 64;                // 16-byte chunks of the tile per lane (8 for C = 64)
    extern __shared__ __attribute__((aligned(16))) float smem_o2[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, hh = lane >> 5;
    const int b = blockIdx.y;
    const int px0 = (blockIdx.x * 4 + wave) * 32;
    if (px0 >= p.npix) return;
    float* xs = smem_o2 + wave * 32 * LDX;
    const float* X = p.X + (long)b * p.xb + p.x_coff;
    // coalesced tile load: chunk c = lane + 64k covers pixel c / (C/4), channels (c % (C/4)) * 4 .. +4
    float4 xin[NCH];
    const bool xlp = p.x_lp != 0;                       // 16-bit X: chunk c = lane + 64k (k < NCH / 2) covers pixel c / (C/8), channels (c % (C/8)) * 8 .. +8
    if (xlp) {
        const u16* Xh = reinterpret_cast<const u16*>(p.X) + (long)b * p.xb + p.x_coff;
#pragma unroll
        for (int k = 0; k < NCH / 2; ++k) {
            const int c = lane + 64 * k, px = c / (C / 8), ch = (c % (C / 8)) * 8;
            xin[k] = *reinterpret_cast<const float4*>(Xh + (long)min(px0 + px, p.npix - 1) * p.ldx + ch);
        }
    } else {
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int c = lane + 64 * k, px = c / (C / 4), ch = (c % (C / 4)) * 4;
            xin[k] = *reinterpret_cast<const float4*>(X + (long)min(px0 + px, p.npix - 1) * p.ldx + ch);
        }
    }
    // A fragments of GEMM2 (all of W2 for this utterance: CT x 8 K-steps)
    const uint4* w2 = reinterpret_cast<const uint4*>(p.W2) + (long)b * CT * 8 * 64 + lane;
    uint4 w2f[CT][8];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) w2f[ct][ks] = w2[(ct * 8 + ks) * 64];
    if (xlp) {
#pragma unroll
        for (int k = 0; k < NCH / 2; ++k) {
            const int c = lane + 64 * k, px = c / (C / 8), ch = (c % (C / 8)) * 8;
            const unsigned u0 = __float_as_uint(xin[k].x), u1 = __float_as_uint(xin[k].y), u2 = __float_as_uint(xin[k].z), u3 = __float_as_uint(xin[k].w);
            *reinterpret_cast<float4*>(xs + px * LDX + ch) = make_float4(lp_lo(u0), lp_hi(u0), lp_lo(u1), lp_hi(u1));
            *reinterpret_cast<float4*>(xs + px * LDX + ch + 4) = make_float4(lp_lo(u2), lp_hi(u2), lp_lo(u3), lp_hi(u3));
        }
    } else {
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int c = lane + 64 * k, px = c / (C / 4), ch = (c % (C / 4)) * 4;
            *reinterpret_cast<float4*>(xs + px * LDX + ch) = xin[k];
        }
    }
    __builtin_amdgcn_wave_barrier();
    // B fragments of GEMM1: lane (pixel column i, half hh) holds x[px][ks*16 + hh*8 .. +8]
    LFrag xf[KS1];
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks) {
        const float4 xa = *reinterpret_cast<const float4*>(xs + i * LDX + ks * 16 + hh * 8);
        const float4 xc = *reinterpret_cast<const float4*>(xs + i * LDX + ks * 16 + hh * 8 + 4);
        xf[ks].u.x = pack2_lp(xa.x, xa.y); xf[ks].u.y = pack2_lp(xa.z, xa.w);
        xf[ks].u.z = pack2_lp(xc.x, xc.y); xf[ks].u.w = pack2_lp(xc.z, xc.w);
    }
    // ---- GEMM1: q^T, four 32-row he tiles; converted to bf16 B fragments tile by tile
    const uint4* wq = reinterpret_cast<const uint4*>(p.Wq) + lane;                  // bf16, fragment order [he tile][K-step][lane][8]
    LFrag qf[8];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        f32x16 q;
#pragma unroll
        for (int r = 0; r < 16; ++r) q[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS1; ++ks) {
            LFrag af; af.u = wq[(t * KS1 + ks) * 64];
            q = DEX_MFMA_LP(af.v, xf[ks].v, q, 0, 0, 0);
#ifdef DEX_LP_WSPLIT
            LFrag al; al.u = wq[(t * KS1 + ks) * 64 + p.wq_lo_off / 8];       // the lo half of the same fragment
            q = DEX_MFMA_LP(al.v, xf[ks].v, q, 0, 0, 0);
#endif
        }
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
            qf[t * 2 + k2].u.x = pack2_lp(q[8 * k2 + 0], q[8 * k2 + 1]); qf[t * 2 + k2].u.y = pack2_lp(q[8 * k2 + 2], q[8 * k2 + 3]);
            qf[t * 2 + k2].u.z = pack2_lp(q[8 * k2 + 4], q[8 * k2 + 5]); qf[t * 2 + k2].u.w = pack2_lp(q[8 * k2 + 6], q[8 * k2 + 7]);
        }
    }
    // ---- GEMM2 + epilogue: rows co = ct*32 + (r&3) + 8*(r>>2) + 4*hh  ->  4 consecutive channels per register quad;
    // y = result + x (from the image) + bias replaces x in the image, location by location
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        f32x16 y;
#pragma unroll
        for (int r = 0; r < 16; ++r) y[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            LFrag af; af.u = w2f[ct][ks];
            y = DEX_MFMA_LP(af.v, qf[ks].v, y, 0, 0, 0);
        }
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int co = ct * 32 + 8 * g4 + 4 * hh;
            float* slot = xs + i * LDX + co;
            const float4 res = *reinterpret_cast<const float4*>(slot);
            const float4 bia = *reinterpret_cast<const float4*>(p.bias + co);
            float4 o;
            o.x = y[g4 * 4 + 0] + res.x + bia.x; o.y = y[g4 * 4 + 1] + res.y + bia.y;
            o.z = y[g4 * 4 + 2] + res.z + bia.z; o.w = y[g4 * 4 + 3] + res.w + bia.w;
            *reinterpret_cast<float4*>(slot) = o;
        }
    }
    __builtin_amdgcn_wave_barrier();
    float* Y = p.Y + (long)b * p.yb + p.y_coff;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int c = lane + 64 * k, px = c / (C / 4), ch = (c % (C / 4)) * 4;
        const float4 o = *reinterpret_cast<const float4*>(xs + px * LDX + ch);
        if (px0 + px < p.npix) {
            if (p.y_lp) {     // every consumer of this tensor rounds it to the operand type: store it that way (half the bytes)
                u16* yh = reinterpret_cast<u16*>(p.Y) + (long)b * p.yb + p.y_coff + (long)(px0 + px) * p.ldy + ch;
                *reinterpret_cast<uint2*>(yh) = make_uint2(pack2_lp(o.x, o.y), pack2_lp(o.z, o.w));
            } else *reinterpret_cast<float4*>(Y + (long)(px0 + px) * p.ldy + ch) = o;
            if (p.Y2) {       // (uniform) a 16-bit copy for the reader that rounds it anyway (the up path's conv reads the concatenation buffer)
                u16* y2 = reinterpret_cast<u16*>(p.Y2) + (long)b * p.y2b + p.y2_coff + (long)(px0 + px) * p.ldy2 + ch;
                *reinterpret_cast<uint2*>(y2) = make_uint2(pack2_lp(o.x, o.y), pack2_lp(o.z, o.w));
            }
        }
    }
}
bool linattn_fused_supported(int C) {
#if defined(DEX_LP_WSPLIT) && !defined(DEX_WS_HAVE_LINATTN)
    return false;            // no split-weight form yet (lp_config.h)
#endif
    return C == 64 || C == 128;
}
// the throughput form below takes grids of at least this many workgroups (DEX_OUT2_MIN)
static long out2_min_wgs() { return knob_or("DEX_OUT2_MIN", 256); }
bool linattn_out2_lp_out_supported(int npix, int B) { return (long)((npix + 127) / 128) * B >= out2_min_wgs(); }       // == the throughput form below
void launch_linattn_out2(const LinOut2P& p, hipStream_t st) {
    dim3 grid((p.npix + 127) / 128, p.B);
    const size_t lds = (size_t)4 * 32 * (p.C + 4) * sizeof(float);
    static bool attr = false;
    if (!attr) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&linattn_out2_kernel<128>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)4 * 32 * 132 * sizeof(float)));
        attr = true;
    }
    const bool lp_io = p.x_lp || p.y_lp || p.Y2;
    if (p.hw && !lp_io) {                              // the wave-split latency form (launcher: DEX_LINATTN_OUT2_HW)
        g_last_symbol = "linattn_out2_hw_kernel";
        g_last_form = p.C == 64 ? (p.rows ? "linattn_out2_hw_kernel C=64 rows=1" : "linattn_out2_hw_kernel C=64 rows=0")
                                : (p.rows ? "linattn_out2_hw_kernel C=128 rows=1" : "linattn_out2_hw_kernel C=128 rows=0");
        const dim3 g1((p.npix + 31) / 32, p.B);
        if (p.rows) {                                  // x and y as whole pixel rows (launcher: DEX_OUT2_ROWS)
            if (p.C == 64) hipLaunchKernelGGL((linattn_out2_hw_kernel<64, true>), g1, dim3(256), 0, st, p);
            else hipLaunchKernelGGL((linattn_out2_hw_kernel<128, true>), g1, dim3(256), 0, st, p);
            return;
        }
        if (p.C == 64) hipLaunchKernelGGL((linattn_out2_hw_kernel<64, false>), g1, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((linattn_out2_hw_kernel<128, false>), g1, dim3(256), 0, st, p);
        return;
    }
    if ((long)grid.x * p.B < out2_min_wgs()) {        // latency regime: the direct form
        g_last_form = p.C == 64 ? "linattn_out2_direct_kernel C=64" : "linattn_out2_direct_kernel C=128";
        if (p.C == 64) hipLaunchKernelGGL(linattn_out2_direct_kernel<64>, grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL(linattn_out2_direct_kernel<128>, grid, dim3(256), 0, st, p);
        return;
    }
    g_last_form = p.C == 64 ? "linattn_out2_kernel C=64 (throughput)" : "linattn_out2_kernel C=128 (throughput)";
    if (p.C == 64) hipLaunchKernelGGL(linattn_out2_kernel<64>, grid, dim3(256), lds, st, p);
    else hipLaunchKernelGGL(linattn_out2_kernel<128>, grid, dim3(256), lds, st, p);
}

}  // namespace DEX_LP_NS
}  // namespace dex
