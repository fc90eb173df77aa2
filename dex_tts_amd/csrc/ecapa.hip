// ecapa.hip — WavLM-large + ECAPA-TDNN speaker similarity (the SIM-o of zero-shot TTS tables) on the device: the WavLM-large trunk
// (HF's WavLMModel: layer-norm feature extractor, stable-layer-norm encoder, head_dim 64, gated relative-position bias) feeding the
// ECAPA-TDNN head of the UniSpeech speaker-verification recipe, in eval mode.  fp32 throughout, channels-last [B][T][C].  C ABI
// dex_ecapa_*.  Row b of a batch is the network applied to row b alone at its own length.
//
//   ecapa_norm_kernel      F.layer_norm(wav, wav.shape) of the s3prl upstream: mean and biased variance over the row's own length in
//                          fp64, eps 1e-5 (wav_encoder.h's asr_norm_kernel is Wav2Vec2FeatureExtractor's, eps 1e-7).
//   the trunk              composed from wav_layernorm.h / wav_trunk.h / wav_gated_attn.h: asr.hip's front end, h = y + GELU(pos_conv(y))
//                          with NO LayerNorm before the layers, the shared encoder layer in its pre-norm order with the gated attention
//                          (the gate reads LayerNorm(h), as the attention does), encoder.layer_norm after the last layer.  The hidden
//                          states are the inputs of layers 0 .. L - 1 and that normed output, mixed as they appear (wavlm_mix_kernel).
//   ecapa_inorm_kernel     InstanceNorm1d(x + 1e-6) over the row's own frames per channel: two passes in fp64, 0 past the frames.
//   launch_igemm           (igemm.hip, exact-fp32 MFMA) layer1 (k = 5), the 1 x 1 convolutions, the two Linears of the pooling's
//                          attention and the embedding Linear, ReLU in the epilogue where one follows.
//   ecapa_bn_kernel        the eval-mode BatchNorm that FOLLOWS a ReLU: x scale[c] + shift[c] (folded in fp64 at finalize), 0 past the frames.
//   ecapa_res2_kernel      the seven dependent w x w x 3 dilated convolutions of a Res2 block in ONE launch.  A workgroup owns
//                          RES2_TILE = 72 frames and computes a span of 128 (28 = 7 stages x the largest dilation each side; the halo
//                          is recomputed).  A stage's input lives in LDS as [channel][position]; its weights [3 w][w] stream through
//                          LDS stage by stage (all seven are 344 KB at w = 64); out = W x in on v_mfma_f32_32x32x2_f32, one 32-position
//                          tile per wave, k = tap w + channel ascending: the order is fixed by the config.  Every stage zero-pads ITS OWN
//                          input at the row's true ends, so after each stage the positions outside [0, frames) are forced to 0 (they
//                          are not what the convolution makes of padded neighbours), and the next stage's input is that plus the next
//                          slice.  Positions the span does not hold read as 0: the error this makes travels one dilation per stage and
//                          after seven stages has not reached the 72 frames that are stored.
//   ecapa_tstats_kernel    per (row, channel) over the row's frames, fp64, 16 frame lanes added in order: the mean (squeeze-excitation),
//                          or mean | sqrt(unbiased variance + 1e-10) (the pooling's global context).
//   ecapa_se_fc_kernel     gate = sigmoid(W2 relu(W1 mean + b1) + b2), fmaf chains, k ascending; one workgroup per row.
//   ecapa_se_apply_kernel  out = x gate + residual into a channel slice of the [B][T][3 C] buffer the 1 x 1 convolution after the blocks
//                          reads: no concat copy.
//   ecapa_cbias_kernel     global_context_att: the context is constant over time, so [T][3 x 3C] is never built - its share of linear1
//                          is a per-row bias, as mos.hip folds its conditioning.
//   ecapa_pool_kernel      attentive statistics pooling per (row, 64 channels): the max of the logits over the row's frames, then
//                          sum e, sum e x, sum e x^2 in fp64 (e = exp(logit - max)); mean = S1 / S0, deviation = sqrt(max(S2 / S0 -
//                          mean^2, 1e-9)); the BatchNorm before the embedding Linear is applied on the way out.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dex_amd.h"
#include "kernels.h"
#include "wav_gated_attn.h"
#include "wav_layernorm.h"
#include "wav_trunk.h"
#include "weight_store.h"

using namespace dex::wavenc;

namespace {

static_assert(MAXC == DEX_ECAPA_MAX_CONV, "ConvSpec holds DEX_ECAPA_MAX_CONV layers");
static_assert(MAXF == DEX_ECAPA_MAX_FRAMES, "the bucket table holds DEX_ECAPA_MAX_FRAMES frames");
constexpr int NBLK = DEX_ECAPA_BLOCKS;          // SE-Res2 blocks
constexpr int NST = 7;                          // convolutions of a Res2 chain (scale - 1)
constexpr float BN_EPS = 1e-5f;
constexpr int TL = 16;                          // frame lanes of the per-channel statistics workgroups (x 64 channels)
constexpr int SE_MAX = 256, CH_MAX = 1024;      // ecapa_se_fc_kernel's LDS

// a = row lengths; rows r0 .. r0 + n of wav / out [.][ld]: (x - mean) / sqrt(var + eps) over the row's own length, 0 past it
__global__ __launch_bounds__(NORM_T) void ecapa_norm_kernel(const float* wav, float* out, long ld, double eps, int r0, const Tab R) {
    __shared__ double red[NORM_T];
    const int r = blockIdx.x, tid = threadIdx.x, L = R.a[r];
    const float* w = wav + (long)(r0 + r) * ld;
    float* o = out + (long)(r0 + r) * ld;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < L; i += 4 * NORM_T) {
#pragma unroll
        for (int u = 0; u < 4; ++u) s[u] += i + u * NORM_T < L ? (double)w[i + u * NORM_T] : 0.0;
    }
    const double mean = block_sum<NORM_T>((s[0] + s[1]) + (s[2] + s[3]), red) / (double)L;
    double q[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < L; i += 4 * NORM_T) {
#pragma unroll
        for (int u = 0; u < 4; ++u) { const double d = i + u * NORM_T < L ? (double)w[i + u * NORM_T] - mean : 0.0; q[u] = fma(d, d, q[u]); }
    }
    const double sd = sqrt(block_sum<NORM_T>((q[0] + q[1]) + (q[2] + q[3]), red) / (double)L + eps);
    for (long i = tid; i < ld; i += NORM_T) o[i] = i < L ? (float)(((double)w[i] - mean) / sd) : 0.f;
}

// X [B][T][C] -> Y [B][T][C]: InstanceNorm1d(x + 1e-6) per (row, channel) over the first len[b] frames (the constant leaves with the
// mean), biased variance, eps 1e-5; 0 past them.  grid (C / 64, B)
__global__ __launch_bounds__(TL * 64) void ecapa_inorm_kernel(const float* X, float* Y, int T, int C, const int* len) {
    __shared__ double red[TL][64];
    const int cl = threadIdx.x & 63, ts = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl, b = blockIdx.y;
    const int n = min(len[b], T);
    const float* x = X + (long)b * T * C + c;
    float* y = Y + (long)b * T * C + c;
    double s = 0.0;
    for (int t = ts; t < n; t += TL) s += (double)x[(long)t * C];
    red[ts][cl] = s;
    __syncthreads();
    double tot = 0.0;
    for (int u = 0; u < TL; ++u) tot += red[u][cl];
    const double mean = tot / (double)n;
    __syncthreads();
    double q = 0.0;
    for (int t = ts; t < n; t += TL) { const double d = (double)x[(long)t * C] - mean; q = fma(d, d, q); }
    red[ts][cl] = q;
    __syncthreads();
    double qt = 0.0;
    for (int u = 0; u < TL; ++u) qt += red[u][cl];
    const double rstd = 1.0 / sqrt(qt / (double)n + 1e-5);
    for (int t = ts; t < T; t += TL) y[(long)t * C] = t < n ? (float)(((double)x[(long)t * C] - mean) * rstd) : 0.f;
}

// X [B][T][C] in place: x scale[c] + shift[c]; 0 at or past len[b]
__global__ __launch_bounds__(256) void ecapa_bn_kernel(float4* X, int T, int C4, const int* len, const float4* scale, const float4* shift, long n4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const long row = i / C4;
    const int c = (int)(i - row * C4), b = (int)(row / T), t = (int)(row - (long)b * T);
    if (t >= len[b]) { X[i] = make_float4(0.f, 0.f, 0.f, 0.f); return; }
    const float4 v = X[i], sc = scale[c], sh = shift[c];
    X[i] = make_float4(fmaf(v.x, sc.x, sh.x), fmaf(v.y, sc.y, sh.y), fmaf(v.z, sc.z, sh.z), fmaf(v.w, sc.w, sh.w));
}

// X [B][T][C] in place: tanh
__global__ __launch_bounds__(256) void ecapa_tanh_kernel(float4* X, long n4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const float4 v = X[i];
    X[i] = make_float4(tanhf(v.x), tanhf(v.y), tanhf(v.z), tanhf(v.w));
}

// scale = gamma / sqrt(var + eps), shift = beta - mean scale, in fp64
__global__ __launch_bounds__(256) void ecapa_bnfold_kernel(const float* gamma, const float* beta, const float* mean, const float* var, float* scale,
                                                          float* shift, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double sc = (double)gamma[i] / sqrt((double)var[i] + (double)BN_EPS);
    scale[i] = (float)sc;
    shift[i] = (float)((double)beta[i] - (double)mean[i] * sc);
}

// ---- the Res2 chain
constexpr int R2_TILE = DEX_ECAPA_RES2_TILE;     // frames a workgroup stores
constexpr int R2_DMAX = 4;                       // the largest dilation
constexpr int R2_HALO = NST * R2_DMAX;           // 28
constexpr int R2_SPAN = R2_TILE + 2 * R2_HALO;   // 128 positions a workgroup computes: one 32-position MFMA tile per wave
constexpr int R2_LD = R2_SPAN + 2 * R2_DMAX + 1; // a channel's row in LDS: R2_DMAX zeros either side of the span
static_assert(R2_SPAN == 128, "four waves x 32 positions");

// X, Y [B][T][8 w]; Wt [7][3 w][w] (row = tap w + ci); par [7][3][w]: bias | BN scale | BN shift
struct Res2P { const float* X; float* Y; const float* Wt; const float* par; int T, dil; };
size_t res2_lds(int w) { return (size_t)(3 * w * w + w * R2_LD + 3 * w) * sizeof(float); }

// frames [R2_TILE blockIdx.x, + R2_TILE) of row r0 + blockIdx.y (R.a: the rows' frame counts).  Y must not overlap X
template <int W>
__global__ __launch_bounds__(256) void ecapa_res2_kernel(const Res2P p, int r0, const Tab R) {
    extern __shared__ __attribute__((aligned(16))) float r2_smem[];
    constexpr int MT = W / 32, C = 8 * W;
    constexpr int LPP = W / 4, PPP = 256 / LPP;            // lanes per position of the cooperative passes (a float4 each), positions per pass
    float* Wl = r2_smem;                                    // [3 W][W]
    float* cur = Wl + 3 * W * W;                            // [W][R2_LD]: the stage's input, then its output
    float* par = cur + W * R2_LD;                           // [3][W]
    const int tid = threadIdx.x, lane = tid & 63, nt = tid >> 6, i = lane & 31, hh = lane >> 5;
    const int b = r0 + blockIdx.y, Tb = min(R.a[blockIdx.y], p.T), t0 = blockIdx.x * R2_TILE;
    const float* Xb = p.X + (long)b * p.T * C;
    float* Yb = p.Y + (long)b * p.T * C;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t0 >= Tb) {                                         // the whole tile lies past the row's frames
        const int np = min(R2_TILE, p.T - t0);
        for (int idx = tid; idx < np * (C / 4); idx += 256) reinterpret_cast<float4*>(Yb + (long)t0 * C)[idx] = zero4;
        return;
    }
    const int c4 = (tid % LPP) * 4, ps = tid / LPP;
    for (int idx = tid; idx < W * 2 * R2_DMAX; idx += 256) {
        const int c = idx / (2 * R2_DMAX), m = idx - c * 2 * R2_DMAX;
        cur[c * R2_LD + (m < R2_DMAX ? m : R2_SPAN + m)] = 0.f;
    }
    // slice 0 (0 outside the row), and the pass-through slice 7
    for (int s = ps; s < R2_SPAN; s += PPP) {
        const int pos = t0 - R2_HALO + s;
        const bool in_row = pos >= 0 && pos < Tb;
        const float4 v = in_row ? *reinterpret_cast<const float4*>(Xb + (long)pos * C + c4) : zero4;
        float* d = cur + c4 * R2_LD + R2_DMAX + s;
        d[0] = v.x; d[R2_LD] = v.y; d[2 * R2_LD] = v.z; d[3 * R2_LD] = v.w;
        if (s >= R2_HALO && s < R2_HALO + R2_TILE && pos < p.T)
            *reinterpret_cast<float4*>(Yb + (long)pos * C + 7 * W + c4) = in_row ? *reinterpret_cast<const float4*>(Xb + (long)pos * C + 7 * W + c4) : zero4;
    }
    const int pcol = t0 - R2_HALO + nt * 32 + i;            // the position of this lane's accumulator column
    const bool col_in_row = pcol >= 0 && pcol < Tb;
    for (int st = 0; st < NST; ++st) {
        {
            const float4* src = reinterpret_cast<const float4*>(p.Wt + (long)st * 3 * W * W);
            for (int idx = tid; idx < 3 * W * W / 4; idx += 256) reinterpret_cast<float4*>(Wl)[idx] = src[idx];
            for (int idx = tid; idx < 3 * W; idx += 256) par[idx] = p.par[st * 3 * W + idx];
        }
        __syncthreads();
        f32x16 acc[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
        const float* bq = cur + hh * R2_LD + R2_DMAX + nt * 32 + i;
        const float* aq = Wl + hh * W + i;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int off = (j - 1) * p.dil;
#pragma unroll 8
            for (int ci = 0; ci < W; ci += 2) {
                const float bf = bq[ci * R2_LD + off];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[(j * W + ci) * W + mt * 32], bf, acc[mt], 0, 0, 0);
            }
        }
        __syncthreads();                                    // every wave has read the stage's input
        // bias, ReLU, the BatchNorm after it; 0 outside the row: the next stage pads its own input there
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                const float v = fmaf(fmaxf(acc[mt][r] + par[co], 0.f), par[W + co], par[2 * W + co]);
                cur[co * R2_LD + R2_DMAX + nt * 32 + i] = col_in_row ? v : 0.f;
            }
        __syncthreads();
        // store the tile's frames of slice st; the next stage's input = this output + slice st + 1
        for (int s = ps; s < R2_SPAN; s += PPP) {
            const int pos = t0 - R2_HALO + s;
            float* d = cur + c4 * R2_LD + R2_DMAX + s;
            const float4 o = make_float4(d[0], d[R2_LD], d[2 * R2_LD], d[3 * R2_LD]);
            if (s >= R2_HALO && s < R2_HALO + R2_TILE && pos < p.T) *reinterpret_cast<float4*>(Yb + (long)pos * C + st * W + c4) = o;
            if (st + 1 < NST) {
                const float4 v = (pos >= 0 && pos < Tb) ? *reinterpret_cast<const float4*>(Xb + (long)pos * C + (st + 1) * W + c4) : zero4;
                d[0] = o.x + v.x; d[R2_LD] = o.y + v.y; d[2 * R2_LD] = o.z + v.z; d[3 * R2_LD] = o.w + v.w;
            }
        }
    }
}

// X [B][T][C] -> out [B][C]: the mean per channel over the first len[b] frames; STD: out [B][2 C] = mean | sqrt(unbiased variance +
// 1e-10), two passes.  fp64, the 16 frame lanes added in order.  grid (C / 64, B)
template <bool STD>
__global__ __launch_bounds__(TL * 64) void ecapa_tstats_kernel(const float* X, int T, int C, const int* len, float* out) {
    __shared__ double red[TL][64];
    const int cl = threadIdx.x & 63, ts = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl, b = blockIdx.y;
    const int n = min(len[b], T);
    const float* x = X + (long)b * T * C + c;
    double s = 0.0;
    for (int t = ts; t < n; t += TL) s += (double)x[(long)t * C];
    red[ts][cl] = s;
    __syncthreads();
    double tot = 0.0;
    for (int u = 0; u < TL; ++u) tot += red[u][cl];
    const double mean = tot / (double)n;
    if (!STD) {
        if (ts == 0) out[(long)b * C + c] = (float)mean;
        return;
    }
    __syncthreads();
    double q = 0.0;
    for (int t = ts; t < n; t += TL) { const double d = (double)x[(long)t * C] - mean; q = fma(d, d, q); }
    red[ts][cl] = q;
    __syncthreads();
    if (ts == 0) {
        double qt = 0.0;
        for (int u = 0; u < TL; ++u) qt += red[u][cl];
        out[(long)b * 2 * C + c] = (float)mean;
        out[(long)b * 2 * C + C + c] = (float)sqrt(qt / (double)(n - 1) + 1e-10);
    }
}

// mean [B][C] -> gate [B][C] = sigmoid(W2 relu(W1 mean + b1) + b2); w1 [C][S], w2 [S][C].  One workgroup per row
__global__ __launch_bounds__(256) void ecapa_se_fc_kernel(const float* mean, const float* w1, const float* b1, const float* w2, const float* b2, float* gate,
                                                         int C, int S) {
    __shared__ float sm[CH_MAX];
    __shared__ float hs[SE_MAX];
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int c = tid; c < C; c += 256) sm[c] = mean[(long)b * C + c];
    __syncthreads();
    if (tid < S) {
        float a = b1[tid];
        for (int c = 0; c < C; ++c) a = fmaf(sm[c], w1[(long)c * S + tid], a);
        hs[tid] = fmaxf(a, 0.f);
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        float a = b2[c];
        for (int j = 0; j < S; ++j) a = fmaf(hs[j], w2[(long)j * C + c], a);
        gate[(long)b * C + c] = 1.f / (1.f + expf(-a));
    }
}

// out[b][t][c] = y[b][t][c] gate[b][c] + res[b][t][c] (0 at or past len[b]); y [B][T][C], res / out with row strides ldr / ldo
__global__ __launch_bounds__(256) void ecapa_se_apply_kernel(const float4* y, const float* gate, const float* res, int ldr, float* out, int ldo, int T, int C4,
                                                            const int* len, long n4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const long row = i / C4;
    const int c = (int)(i - row * C4), b = (int)(row / T), t = (int)(row - (long)b * T);
    float4* o = reinterpret_cast<float4*>(out + row * ldo) + c;
    if (t >= len[b]) { *o = make_float4(0.f, 0.f, 0.f, 0.f); return; }
    const float4 v = y[i], g = reinterpret_cast<const float4*>(gate + (long)b * C4 * 4)[c], r = reinterpret_cast<const float4*>(res + row * ldr)[c];
    *o = make_float4(fmaf(v.x, g.x, r.x), fmaf(v.y, g.y, r.y), fmaf(v.z, g.z, r.z), fmaf(v.w, g.w, r.w));
}

// ctx [B][2 C] (mean | deviation) -> cb [B][A] = (b1 + sum_c mean[c] wc[c]) + sum_c dev[c] wc[C + c]; wc [2 C][A]: linear1's rows past
// its first C.  grid B, A threads
__global__ void ecapa_cbias_kernel(const float* ctx, const float* wc, const float* b1, float* cb, int C, int A) {
    const int b = blockIdx.x, j = threadIdx.x;
    if (j >= A) return;
    const float* cv = ctx + (long)b * 2 * C;
    float am = 0.f, as = 0.f;
    for (int c = 0; c < C; ++c) am = fmaf(cv[c], wc[(long)c * A + j], am);
    for (int c = 0; c < C; ++c) as = fmaf(cv[C + c], wc[(long)(C + c) * A + j], as);
    cb[(long)b * A + j] = (b1[j] + am) + as;
}

// logits, X [B][T][C] -> out [B][2 C] = BN(mean | deviation) of the attentive statistics over the first len[b] frames.  grid (C / 64, B)
__global__ __launch_bounds__(TL * 64) void ecapa_pool_kernel(const float* Lg, const float* X, int T, int C, const int* len, const float* scale,
                                                            const float* shift, float* out) {
    __shared__ double red[3][TL][64];
    __shared__ float mx[TL][64];
    const int cl = threadIdx.x & 63, ts = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl, b = blockIdx.y;
    const int n = min(len[b], T);
    const float* lg = Lg + (long)b * T * C + c;
    const float* x = X + (long)b * T * C + c;
    float m = -INFINITY;
    for (int t = ts; t < n; t += TL) m = fmaxf(m, lg[(long)t * C]);
    mx[ts][cl] = m;
    __syncthreads();
    for (int u = 0; u < TL; ++u) m = fmaxf(m, mx[u][cl]);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int t = ts; t < n; t += TL) {
        const double e = (double)expf(lg[(long)t * C] - m), xv = (double)x[(long)t * C];
        s0 += e; s1 = fma(e, xv, s1); s2 = fma(e * xv, xv, s2);
    }
    red[0][ts][cl] = s0; red[1][ts][cl] = s1; red[2][ts][cl] = s2;
    __syncthreads();
    if (ts == 0) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int u = 0; u < TL; ++u) { a0 += red[0][u][cl]; a1 += red[1][u][cl]; a2 += red[2][u][cl]; }
        const double mean = a1 / a0, var = a2 / a0 - mean * mean;
        const float dev = (float)sqrt(var > 1e-9 ? var : 1e-9);
        float* o = out + (long)b * 2 * C;
        o[c] = fmaf((float)mean, scale[c], shift[c]);
        o[C + c] = fmaf(dev, scale[C + c], shift[C + c]);
    }
}

DexEcapaConfig default_config() {
    DexEcapaConfig c;
    std::memset(&c, 0, sizeof c);
    default_trunk_geometry(c);
    c.conv_bias = 1; c.feat_extract_norm_layer = 1;
    c.hidden = 1024; c.n_layers = 24; c.n_heads = 16; c.intermediate = 4096; c.do_stable_layer_norm = 1;
    c.num_buckets = 320; c.max_bucket_distance = 800;
    c.channels = 512; c.emb_dim = 256; c.res2_scale = 8; c.se_bottleneck_dim = 128; c.attention_channels = 128; c.global_context_att = 0;
    for (int i = 0; i < NBLK; ++i) c.dilations[i] = 2 + i;
    return c;
}

// the family that is built; names the first field outside it
int check_config(const DexEcapaConfig& c) {
    if (c.feat_extract_norm_layer != 1) return create_fail("%s: only 'layer' is built", "feat_extract_norm");
    if (c.do_stable_layer_norm != 1) return create_fail("%s: only True is built", "do_stable_layer_norm");
    if (int rc = check_trunk(trunk_of(c), 32)) return rc;
    if (c.num_buckets < 4 || c.num_buckets % 4 || c.num_buckets > 65536) return create_fail("%s: a multiple of 4 in 4 .. 65536", "num_buckets");
    if (c.max_bucket_distance <= c.num_buckets / 4 || c.max_bucket_distance > (1 << 24)) return create_fail("%s: above num_buckets / 4", "max_bucket_distance");
    if (c.res2_scale != 8) return create_fail("%s: only 8 is built", "res2_scale");
    if (c.channels != 8 * 32 && c.channels != 8 * 64) return create_fail("%s: only slices of 32 or 64 channels are built (channels 256 or 512)", "channels / scale");
    if (c.emb_dim < 32 || c.emb_dim % 32 || c.emb_dim > 4096) return create_fail("%s: a multiple of 32 up to 4096", "emb_dim");
    if (c.se_bottleneck_dim < 1 || c.se_bottleneck_dim > SE_MAX) return create_fail("%s: 1 .. 256", "se_bottleneck_dim");
    if (c.attention_channels < 32 || c.attention_channels % 32 || c.attention_channels > 1024) return create_fail("%s: a multiple of 32 up to 1024", "attention_channels");
    if (c.global_context_att != 0 && c.global_context_att != 1) return create_fail("%s: 0 or 1", "global_context_att");
    for (int i = 0; i < NBLK; ++i)
        if (c.dilations[i] < 1 || c.dilations[i] > R2_DMAX) return create_fail("%s: 1 .. 4", "dilations");
    return DEX_OK;
}

long min_samples(const DexEcapaConfig& c) { return samples_for(trunk_of(c), 2); }      // InstanceNorm1d needs two frames
const TrunkKeys KEYS("wavlm.");
const char* const BN_KEYS[4] = {"weight", "bias", "running_mean", "running_var"};
std::string blk(int n, const std::string& what) { return "layer" + std::to_string(n + 2) + "." + what; }

}  // namespace

struct DexEcapa : TrunkStore {
    DexEcapa() : TrunkStore("ecapa ", "dex_ecapa") {}
    DexEcapaConfig c;
    std::vector<GateW> gates;
    const float *rel_embed = nullptr, *lw = nullptr;
    const int* buckets = nullptr;
    std::vector<int32_t> buckets_host;
    struct Affine { const float *scale, *shift; };          // a folded eval-mode BatchNorm
    struct Conv { const float *w, *b; Affine bn; };
    Conv l1;
    struct Block { Conv c1, c2; const float *r2w, *r2par, *se_w1, *se_b1, *se_w2, *se_b2; } blocks[NBLK];
    const float *cat_w = nullptr, *cat_b = nullptr, *att_w1 = nullptr, *att_b1 = nullptr, *att_w2 = nullptr, *att_b2 = nullptr;
    Affine bn{};
    const float *emb_w = nullptr, *emb_b = nullptr;
};

namespace {

void add_bn(DexEcapa* s, const std::string& p, int n) {
    for (const char* k : BN_KEYS) s->add(p + k, {n});
}

void register_keys(DexEcapa* s) {
    const DexEcapaConfig& c = s->c;
    s->t = trunk_of(c);
    s->why = "too short, the instance norm needs two frames (" + std::to_string(min_samples(c)) + " samples)";
    s->rule = WavRule{min_samples(c), s->why.c_str(), 0, MAXF};
    register_trunk_keys(s, KEYS, s->t, true, [&](int l) {
        s->add(KEYS.lk(l, "attention.gru_rel_pos_const"), {1, c.n_heads, 1, 1});
        s->add(KEYS.lk(l, "attention.gru_rel_pos_linear.weight"), {8, 64}); s->add(KEYS.lk(l, "attention.gru_rel_pos_linear.bias"), {8});
        if (l == 0) s->add(KEYS.lk(0, "attention.rel_attn_embed.weight"), {c.num_buckets, c.n_heads});
    });
    const int C = c.channels, w = C / 8, C3 = 3 * C, A = c.attention_channels;
    s->add("feature_weight", {c.n_layers + 1});
    s->add("layer1.conv.weight", {C, c.hidden, 5}); s->add("layer1.conv.bias", {C}); add_bn(s, "layer1.bn.", C);
    for (int n = 0; n < NBLK; ++n) {
        s->add(blk(n, "Conv1dReluBn1.conv.weight"), {C, C, 1}); s->add(blk(n, "Conv1dReluBn1.conv.bias"), {C}); add_bn(s, blk(n, "Conv1dReluBn1.bn."), C);
        for (int i = 0; i < NST; ++i) {
            s->add(blk(n, "Res2Conv1dReluBn.convs.") + std::to_string(i) + ".weight", {w, w, 3});
            s->add(blk(n, "Res2Conv1dReluBn.convs.") + std::to_string(i) + ".bias", {w});
        }
        for (int i = 0; i < NST; ++i) add_bn(s, blk(n, "Res2Conv1dReluBn.bns.") + std::to_string(i) + ".", w);
        s->add(blk(n, "Conv1dReluBn2.conv.weight"), {C, C, 1}); s->add(blk(n, "Conv1dReluBn2.conv.bias"), {C}); add_bn(s, blk(n, "Conv1dReluBn2.bn."), C);
        s->add(blk(n, "SE_Connect.linear1.weight"), {c.se_bottleneck_dim, C}); s->add(blk(n, "SE_Connect.linear1.bias"), {c.se_bottleneck_dim});
        s->add(blk(n, "SE_Connect.linear2.weight"), {C, c.se_bottleneck_dim}); s->add(blk(n, "SE_Connect.linear2.bias"), {C});
    }
    s->add("conv.weight", {C3, C3, 1}); s->add("conv.bias", {C3});
    s->add("pooling.linear1.weight", {A, c.global_context_att ? 3 * C3 : C3, 1}); s->add("pooling.linear1.bias", {A});
    s->add("pooling.linear2.weight", {C3, A, 1}); s->add("pooling.linear2.bias", {C3});
    add_bn(s, "bn.", 2 * C3);
    s->add("linear.weight", {c.emb_dim, 2 * C3}); s->add("linear.bias", {c.emb_dim});
}

// the BatchNorm under prefix p folded into dst[0 .. n) (scale) and dst[n .. 2 n) (shift)
DexEcapa::Affine fold_bn_into(DexEcapa* s, const std::string& p, int n, float* scale, float* shift, hipStream_t st) {
    if (scale && shift)
        hipLaunchKernelGGL(ecapa_bnfold_kernel, dim3((n + 255) / 256), dim3(256), 0, st, s->R(p + "weight"), s->R(p + "bias"), s->R(p + "running_mean"),
                           s->R(p + "running_var"), scale, shift, n);
    return {scale, shift};
}
DexEcapa::Affine fold_bn(DexEcapa* s, const std::string& p, int n, hipStream_t st) {
    float* d = s->alloc(2L * up64(n));
    return fold_bn_into(s, p, n, d, d ? d + up64(n) : nullptr, st);
}
DexEcapa::Conv pack_conv(DexEcapa* s, const std::string& p, int cout, int cin, int k, hipStream_t st) {
    return {pack(s, p + "conv.weight", 1, cout, cin, k, nullptr, st), s->R(p + "conv.bias"), fold_bn(s, p + "bn.", cout, st)};
}

int pack_all(DexEcapa* s, hipStream_t st) {
    const DexEcapaConfig& c = s->c;
    const Trunk& t = s->t;
    auto pack_pos = [&](const double* scale) {
        const int G = t.pos_groups, cg = t.hidden / G;
        if (scale) s->w.pos_w = pack(s, KEYS.ENC + "pos_conv_embed.conv.weight_v", G, cg, cg, t.pos_k, scale, st);
        s->w.pos_b = s->R(KEYS.ENC + "pos_conv_embed.conv.bias");
    };
    if (int rc = finalize_trunk(s, KEYS, t, true, s->w, pack_pos, st)) return rc;
    s->rel_embed = s->R(KEYS.lk(0, "attention.rel_attn_embed.weight"));
    s->gates.clear();
    for (int l = 0; l < t.n_layers; ++l)
        s->gates.push_back({s->R(KEYS.lk(l, "attention.gru_rel_pos_linear.weight")), s->R(KEYS.lk(l, "attention.gru_rel_pos_linear.bias")),
                            s->R(KEYS.lk(l, "attention.gru_rel_pos_const"))});
    {
        float* lw = s->alloc(up64(c.n_layers + 1));
        if (lw) hipLaunchKernelGGL(wavlm_softmax_kernel, dim3(1), dim3(64), 0, st, s->R("feature_weight"), lw, c.n_layers + 1);
        s->lw = lw;
    }
    {   // the bucket of every distance one call can meet, computed here on the host
        s->buckets_host.resize(2 * MAXF - 1);
        for (int d = -(MAXF - 1); d <= MAXF - 1; ++d) s->buckets_host[d + MAXF - 1] = bucket_of(c.num_buckets, c.max_bucket_distance, d);
        int* bk = (int*)s->alloc(up64(2 * MAXF - 1));
        if (bk) DEX_HIPCHK(s, hipMemcpyAsync(bk, s->buckets_host.data(), (2 * MAXF - 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
        s->buckets = bk;
    }
    const int C = c.channels, w = C / 8, C3 = 3 * C, A = c.attention_channels, S = c.se_bottleneck_dim;
    s->l1 = pack_conv(s, "layer1.", C, c.hidden, 5, st);
    for (int n = 0; n < NBLK && s->alloc_rc == DEX_OK; ++n) {
        DexEcapa::Block& b = s->blocks[n];
        b.c1 = pack_conv(s, blk(n, "Conv1dReluBn1."), C, C, 1, st);
        b.c2 = pack_conv(s, blk(n, "Conv1dReluBn2."), C, C, 1, st);
        float* rw = s->alloc((long)NST * 3 * w * w);
        float* rp = s->alloc((long)NST * 3 * w);
        if (!rw || !rp) return s->alloc_rc;
        for (int i = 0; i < NST; ++i) {
            const std::string cv = blk(n, "Res2Conv1dReluBn.convs.") + std::to_string(i), bn = blk(n, "Res2Conv1dReluBn.bns.") + std::to_string(i) + ".";
            pack_into(s->R(cv + ".weight"), rw + (long)i * 3 * w * w, 1, w, w, 3, w, 0, nullptr, st);
            DEX_HIPCHK(s, hipMemcpyAsync(rp + (long)i * 3 * w, s->R(cv + ".bias"), w * sizeof(float), hipMemcpyDeviceToDevice, st));
            fold_bn_into(s, bn, w, rp + (long)i * 3 * w + w, rp + (long)i * 3 * w + 2 * w, st);
        }
        b.r2w = rw; b.r2par = rp;
        b.se_w1 = pack(s, blk(n, "SE_Connect.linear1.weight"), 1, S, C, 1, nullptr, st); b.se_b1 = s->R(blk(n, "SE_Connect.linear1.bias"));
        b.se_w2 = pack(s, blk(n, "SE_Connect.linear2.weight"), 1, C, S, 1, nullptr, st); b.se_b2 = s->R(blk(n, "SE_Connect.linear2.bias"));
    }
    s->cat_w = pack(s, "conv.weight", 1, C3, C3, 1, nullptr, st); s->cat_b = s->R("conv.bias");
    s->att_w1 = pack(s, "pooling.linear1.weight", 1, A, c.global_context_att ? 3 * C3 : C3, 1, nullptr, st); s->att_b1 = s->R("pooling.linear1.bias");
    s->att_w2 = pack(s, "pooling.linear2.weight", 1, C3, A, 1, nullptr, st); s->att_b2 = s->R("pooling.linear2.bias");
    s->bn = fold_bn(s, "bn.", 2 * C3, st);
    s->emb_w = pack(s, "linear.weight", 1, c.emb_dim, 2 * C3, 1, nullptr, st); s->emb_b = s->R("linear.bias");
    return DEX_OK;
}

// workspace: the trunk's prefix | mix [B][T][H] | gate [B][heads][T] | rel [heads][2T - 1] | mask [B][T] | lens (int) [n_conv + 1][B] |
// x [B][T][H] (the instance-normed mix) | a1, ta, tb [B][T][C] | cat, xc, lg [B][T][3C] | att [B][T][A] | sem, seg [B][C] | ctx [B][6C] |
// cb [B][A] | pool [B][6C]
struct Ws : TrunkWs { float *mix, *gate, *rel, *x, *a1, *ta, *tb, *cat, *xc, *lg, *att, *sem, *seg, *ctx, *cb, *pool; size_t bytes; };
Ws plan(const DexEcapa* s, void* ws, long B, long n) {
    const DexEcapaConfig& c = s->c;
    Ws w{};
    Taker tk(ws);
    plan_trunk(s->t, tk, B, n, w);
    const long T = w.T, H = c.hidden, C = c.channels, C3 = 3 * C, A = c.attention_channels;
    w.mix = tk.take(B * T * H);
    w.gate = tk.take(B * c.n_heads * T); w.rel = tk.take((long)c.n_heads * (2 * T - 1)); w.mask = tk.take(B * T);
    w.lens = (int*)tk.take((long)(c.n_conv + 1) * B);
    w.x = tk.take(B * T * H);
    w.a1 = tk.take(B * T * C); w.ta = tk.take(B * T * C); w.tb = tk.take(B * T * C);
    w.cat = tk.take(B * T * C3); w.xc = tk.take(B * T * C3); w.lg = tk.take(B * T * C3); w.att = tk.take(B * T * A);
    w.sem = tk.take(B * C); w.seg = tk.take(B * C); w.ctx = tk.take(B * 2 * C3); w.cb = tk.take(B * A); w.pool = tk.take(B * 2 * C3);
    w.bytes = tk.bytes();
    return w;
}

// the trunk, the layer mix and the instance norm: `hidden` [B][T][H] (0 past a row's frames)
int enqueue_encoder(DexEcapa* s, const float* wav, const int32_t* lengths_host, int B, int n, int do_normalize, float* hidden, const Ws& w, hipStream_t st) {
    const DexEcapaConfig& c = s->c;
    const Trunk& t = s->t;
    const TrunkWeights& W = s->w;
    const int T = w.T, H = c.hidden;
    enqueue_front(t, w, wav, lengths_host, B, n, false, st);
    if (do_normalize)
        for_each_row_table<Tab>(B, [&](Tab& R, int e, int b) { R.a[e] = lengths_host[b]; }, [&](int r0, const Tab& R) {
            hipLaunchKernelGGL(ecapa_norm_kernel, dim3(R.n), dim3(NORM_T), 0, st, wav, w.xn, (long)n, 1e-5, r0, R);
        });
    enqueue_conv0_layernorm(t, W, w, do_normalize ? w.xn : wav, B, n, st);
    enqueue_projection(t, W, w, enqueue_conv_tail<true>(t, W, w, B, 0, st), B, st);
    // h = y + GELU(pos_conv(y)) without its last frame; no LayerNorm before the layers
    gemm(w.y, H, T, H / t.pos_groups, t.pos_k, 1, -(t.pos_k / 2), T, W.pos_w, H / t.pos_groups, t.pos_groups, W.pos_b, w.h, 1, w.y, nullptr, B, st);
    const long n4 = (long)B * T * H / 4;
    auto mix = [&](int l, const float* h) {
        hipLaunchKernelGGL(wavlm_mix_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, (const float4*)h, (const float4*)w.mix, (float4*)w.mix, s->lw, l,
                           l == 0 ? 1 : 0, (const float*)nullptr, n4, H / 4);
    };
    hipLaunchKernelGGL(wavlm_rel_kernel, dim3((2 * T - 1 + 255) / 256, c.n_heads), dim3(256), 0, st, s->rel_embed, s->buckets, w.rel, T, c.n_heads);
    const int* kv_len = w.lens + (long)t.n_conv * B;
    for (int l = 0; l < c.n_layers; ++l) {
        mix(l, w.h);                                        // hidden state l is the INPUT of layer l
        enqueue_layer<true>(layer_dims(t), W.layers[l], w, B, [&](const float* qkv, float* out) {       // pre-norm; the gate reads LayerNorm(h) = y
            enqueue_gated_attention(w.y, s->gates[l], qkv, out, w.gate, w.rel, kv_len, B, T, c.n_heads, st);
        }, st);
    }
    layer_norm<false>(w.h, w.y, (long)B * T, T, H, W.enc_g, W.enc_be, t.layer_norm_eps, nullptr, st);
    mix(c.n_layers, w.y);
    hipLaunchKernelGGL(ecapa_inorm_kernel, dim3(H / 64, B), dim3(TL * 64), 0, st, w.mix, hidden, T, H, kv_len);
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

// one Res2 chain: X [B][T][C] -> Y [B][T][C], row b frames_host[b] frames
int enqueue_res2(DexEcapa* s, int block, const float* X, const int32_t* frames_host, int B, int T, float* Y, hipStream_t st) {
    const int w = s->c.channels / 8;
    // 85 KB of LDS at w = 64: above what a launch gets without asking
    if (w == 64) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ecapa_res2_kernel<64>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)res2_lds(64));
    const Res2P p{X, Y, s->blocks[block].r2w, s->blocks[block].r2par, T, s->c.dilations[block]};
    for_each_row_table<Tab>(B, [&](Tab& R, int e, int b) { R.a[e] = frames_host[b]; }, [&](int r0, const Tab& R) {
        const dim3 grid((T + R2_TILE - 1) / R2_TILE, R.n);
        if (w == 64) hipLaunchKernelGGL(ecapa_res2_kernel<64>, grid, dim3(256), res2_lds(64), st, p, r0, R);
        else hipLaunchKernelGGL(ecapa_res2_kernel<32>, grid, dim3(256), res2_lds(32), st, p, r0, R);
    });
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

// out = BN(ReLU(conv(A))) in place of `out`: the convolution with ReLU in its epilogue, then the BatchNorm (0 past the frames)
void conv_relu_bn(const DexEcapa::Conv& cv, const float* A, int lda, int cin, int k, int cout, float* out, int B, int T, const int* len, hipStream_t st) {
    gemm(A, lda, T, cin, k, 1, -(k / 2), T, cv.w, cout, 1, cv.b, out, 2, nullptr, nullptr, B, st);
    const long n4 = (long)B * T * cout / 4;
    hipLaunchKernelGGL(ecapa_bn_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, (float4*)out, T, cout / 4, len, (const float4*)cv.bn.scale,
                       (const float4*)cv.bn.shift, n4);
}

// the ECAPA-TDNN head after the instance norm: x [B][T][H] -> embed [B][emb_dim]
int enqueue_head(DexEcapa* s, const float* x, const int32_t* frames_host, int B, float* embed, const Ws& w, hipStream_t st) {
    const DexEcapaConfig& c = s->c;
    const int T = w.T, H = c.hidden, C = c.channels, C3 = 3 * C, A = c.attention_channels;
    const int* len = w.lens + (long)c.n_conv * B;
    conv_relu_bn(s->l1, x, H, H, 5, C, w.a1, B, T, len, st);
    const long n4 = (long)B * T * C / 4;
    for (int n = 0; n < NBLK; ++n) {
        const DexEcapa::Block& b = s->blocks[n];
        const float* xin = n ? w.cat + (long)(n - 1) * C : w.a1;
        const int ldx = n ? C3 : C;
        conv_relu_bn(b.c1, xin, ldx, C, 1, C, w.ta, B, T, len, st);
        if (int rc = enqueue_res2(s, n, w.ta, frames_host, B, T, w.tb, st)) return rc;
        conv_relu_bn(b.c2, w.tb, C, C, 1, C, w.ta, B, T, len, st);
        hipLaunchKernelGGL(ecapa_tstats_kernel<false>, dim3(C / 64, B), dim3(TL * 64), 0, st, w.ta, T, C, len, w.sem);
        hipLaunchKernelGGL(ecapa_se_fc_kernel, dim3(B), dim3(256), 0, st, w.sem, b.se_w1, b.se_b1, b.se_w2, b.se_b2, w.seg, C, c.se_bottleneck_dim);
        hipLaunchKernelGGL(ecapa_se_apply_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, (const float4*)w.ta, w.seg, xin, ldx, w.cat + (long)n * C,
                           C3, T, C / 4, len, n4);
    }
    gemm(w.cat, C3, T, C3, 1, 1, 0, T, s->cat_w, C3, 1, s->cat_b, w.xc, 2, nullptr, nullptr, B, st);
    {   // att = tanh(linear1([x | context])): the context's share is a per-row bias
        const float* bias = s->att_b1;
        long bias_bstride = 0;
        if (c.global_context_att) {
            hipLaunchKernelGGL(ecapa_tstats_kernel<true>, dim3(C3 / 64, B), dim3(TL * 64), 0, st, w.xc, T, C3, len, w.ctx);
            hipLaunchKernelGGL(ecapa_cbias_kernel, dim3(B), dim3(A), 0, st, w.ctx, s->att_w1 + (long)C3 * A, s->att_b1, w.cb, C3, A);
            bias = w.cb; bias_bstride = A;
        }
        dex::IGemmP g{};
        g.A = w.xc; g.lda = C3; g.a_bstride = (long)T * C3;
        g.Hi = 1; g.Wi = T; g.Cin = C3;
        g.KH = 1; g.KW = 1; g.sh = 1; g.sw = 1; g.step_h = 1; g.step_w = 1;
        g.Ho = 1; g.Wo = T;
        g.W = s->att_w1; g.w_gstride = (long)C3 * A; g.N = A; g.K = C3; g.ksplit = 1; g.groups = 1;
        g.bias = bias; g.bias_bstride = bias_bstride;
        g.C = w.att; g.ldc = A; g.c_bstride = (long)T * A; g.c_sstride = (long)B * T * A;
        g.OHf = 1; g.OWf = T; g.osh = 1; g.osw = 1;
        g.inmask_ws = 1; g.outmask_ws = 1; g.mask_bstride = T; g.gate_nstride = 1;
        g.ldres = A; g.res_bstride = (long)T * A;
        g.B = B;
        dex::launch_igemm(g, dex::PREC_FP32, st);
        const long a4 = (long)B * T * A / 4;
        hipLaunchKernelGGL(ecapa_tanh_kernel, dim3((unsigned)((a4 + 255) / 256)), dim3(256), 0, st, (float4*)w.att, a4);
    }
    linear(w.att, A, s->att_w2, C3, s->att_b2, w.lg, 0, nullptr, nullptr, T, B, st);
    hipLaunchKernelGGL(ecapa_pool_kernel, dim3(C3 / 64, B), dim3(TL * 64), 0, st, w.lg, w.xc, T, C3, len, s->bn.scale, s->bn.shift, w.pool);
    linear(w.pool, 2 * C3, s->emb_w, c.emb_dim, s->emb_b, embed, 0, nullptr, nullptr, B, 1, st);
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

typedef Entry<DexEcapa> E;

int run(DexEcapa* s, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, int do_normalize, float* hidden_dev, float* embed_dev,
        void* workspace_dev, size_t workspace_bytes, hipStream_t st) {
    return E::call(s, wav_dev, lengths_host, B, n_samples, hidden_dev || embed_dev, workspace_dev, workspace_bytes, plan, no_further_check,
                   [&](const Ws& w, int) {
        float* hidden = hidden_dev ? hidden_dev : w.x;
        int rc = enqueue_encoder(s, wav_dev, lengths_host, B, n_samples, do_normalize, hidden, w, st);
        if (rc == DEX_OK && embed_dev) {
            std::vector<int32_t> frames(B);
            for (int b = 0; b < B; ++b) frames[b] = frames_of(s->t, lengths_host[b], s->t.n_conv);
            rc = enqueue_head(s, hidden, frames.data(), B, embed_dev, w, st);
        }
        return rc;
    });
}

bool geometry_ok(const DexEcapaConfig& c) { return conv_ok(c); }

}  // namespace

extern "C" {

int dex_ecapa_create(const DexEcapaConfig* cfg, DexEcapa** out) { return E::create(cfg, out, default_config, check_config, register_keys); }
void dex_ecapa_destroy(DexEcapa* s) { E::destroy(s); }
const char* dex_ecapa_last_error(const DexEcapa* s) { return E::last_error(s); }
int dex_ecapa_load(DexEcapa* s, const char* key, const float* w_dev, const int64_t* shape, int ndim, dex_stream_t stream) {
    return E::load(s, key, w_dev, shape, ndim, stream);
}
int dex_ecapa_finalize(DexEcapa* s, dex_stream_t stream) { return E::finalize(s, stream, pack_all, "packing the ecapa weights failed"); }
int dex_ecapa_num_weights(const DexEcapa* s) { return E::num_weights(s); }
int dex_ecapa_weight_info(const DexEcapa* s, int i, const char** key, int64_t shape[4], int* ndim) { return E::weight_info(s, i, key, shape, ndim); }

int dex_ecapa_num_frames(const DexEcapaConfig* cfg, int n_samples) { return E::num_frames(cfg, n_samples, default_config, geometry_ok); }
int dex_ecapa_min_samples(const DexEcapaConfig* cfg) { return E::min_samples(cfg, default_config, geometry_ok, min_samples); }
size_t dex_ecapa_workspace_bytes(const DexEcapa* s, int B, int max_samples) { return E::workspace_bytes(s, B, max_samples, plan); }

int dex_ecapa_hidden(DexEcapa* s, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, int do_normalize, float* hidden_dev,
                     void* workspace_dev, size_t workspace_bytes, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!hidden_dev) return s->fail(DEX_ERR_ARG, "null pointer argument");
    return run(s, wav_dev, lengths_host, B, n_samples, do_normalize, hidden_dev, nullptr, workspace_dev, workspace_bytes, (hipStream_t)stream);
}

int dex_ecapa_embed(DexEcapa* s, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, int do_normalize, float* embed_dev,
                    void* workspace_dev, size_t workspace_bytes, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!embed_dev) return s->fail(DEX_ERR_ARG, "null pointer argument");
    return run(s, wav_dev, lengths_host, B, n_samples, do_normalize, nullptr, embed_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
}

int dex_ecapa_res2(DexEcapa* s, int block, const float* x_dev, const int32_t* frames_host, int B, int T, float* out_dev, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!x_dev || !frames_host || !out_dev) return s->fail(DEX_ERR_ARG, "null pointer argument");
    if (x_dev == out_dev) return s->fail(DEX_ERR_ARG, "out_dev must not be x_dev");
    if (block < 0 || block >= NBLK) return s->fail(DEX_ERR_ARG, "block must lie in [0, %d)", NBLK);
    if (B < 1 || B > MAX_B) return s->fail(DEX_ERR_ARG, "B must lie in [1, %d]", MAX_B);
    if (T < 1 || T > MAXF) return s->fail(DEX_ERR_ARG, "T must lie in [1, %d]", MAXF);
    for (int b = 0; b < B; ++b)
        if (frames_host[b] < 1 || frames_host[b] > T) return s->fail(DEX_ERR_ARG, "frame counts must lie in [1, T]");
    if (!s->finalized) return s->fail(DEX_ERR_STATE, "the ecapa weights are not finalized (dex_ecapa_finalize)");
    const int rc = enqueue_res2(s, block, x_dev, frames_host, B, T, out_dev, (hipStream_t)stream);
    return rc ? s->fail(rc, "kernel launch failed") : DEX_OK;
}

}  // extern "C"
