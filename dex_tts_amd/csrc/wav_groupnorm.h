// wav_groupnorm.h — the first layer of the group-norm feature extractor (feat_extract_norm = "group": wavlm.hip's WavLM x-vector
// network and mos.hip's UTMOS trunk) and the positional convolution with padded groups that both of them run:
//
//   wavlm_conv0_kernel     the first convolution (Cin = 1), raw: 8 frames x all channels per workgroup, the sample window in LDS.
//   wavlm_gn_part_kernel,  GroupNorm(C, C) of layer 0: per (row, channel) over the row's OWN frames, two passes - the sums of 512-frame
//   wavlm_gn_final_kernel, chunks in fp64, added in chunk order, first of x (mean), then of (x - mean)^2 (biased variance): a DC offset
//   wavlm_gn_apply_kernel  cancels nothing; then (x - mean) * rstd * gamma + beta -> GELU in place, 0 at or past the row's frames.
//   wavlm_pack_pos_kernel, groups of the positional convolution that are no multiple of 32 channels wide (768 / 16 = 48) are padded to
//   wavlm_pad_vec_kernel,  64 for the exact-fp32 implicit GEMM (zeros in the padding) and come back onto the residual through
//   wavlm_unpad_add_kernel wavlm_unpad_add_kernel.
// with the workspace pieces (GnWs, PosWs), the enqueue steps around them, and the whole front end of such a network up to its first
// encoder layer (enqueue_groupnorm_front).  Includes wav_trunk.h; everything has internal linkage.
#pragma once
#include "wav_trunk.h"

namespace dex {
namespace wavenc {
namespace {

constexpr int GN_CHUNK = 512;            // frames per partial sum of the group norm

struct Conv0P { const float* x; long x_ld; const float* w; const float* bias; float* out; int T0, C, k, s; };

// frames [F0 blockIdx.x, + F0) of utterance blockIdx.y: out[b][t][c] = bias[c] + sum_j w[c][j] x[b][t s + j] (taps ascending, fmaf)
__global__ __launch_bounds__(256) void wavlm_conv0_kernel(const Conv0P p) {
    __shared__ float xs[(F0 - 1) * S0_MAX + K0_MAX];
    const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * F0;
    const int nwin = (F0 - 1) * p.s + p.k;
    const float* x = p.x + (long)b * p.x_ld;
    for (int i = tid; i < nwin; i += 256) {
        const long idx = (long)t0 * p.s + i;
        xs[i] = idx < p.x_ld ? x[idx] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int ci = 0; ci < 2; ++ci) {
        const int c = tid + 256 * ci;
        if (c >= p.C) continue;
        float w[K0_MAX];
#pragma unroll
        for (int j = 0; j < K0_MAX; ++j) w[j] = j < p.k ? p.w[(long)c * p.k + j] : 0.f;
        const float bs = p.bias ? p.bias[c] : 0.f;
#pragma unroll
        for (int f = 0; f < F0; ++f) {
            float v = bs;
#pragma unroll
            for (int j = 0; j < K0_MAX; ++j)
                if (j < p.k) v = fmaf(w[j], xs[f * p.s + j], v);
            if (t0 + f < p.T0) p.out[((long)b * p.T0 + t0 + f) * p.C + c] = v;
        }
    }
}

// part[b][chunk][c] = sum over the chunk's frames below len0[b] of x (SQ: of (x - mean[b][c])^2), fp64; 64 channels x 4 frame lanes
// per workgroup, the four lanes added in a fixed order.  grid (chunks, ceil(C / 64), B)
template <bool SQ>
__global__ __launch_bounds__(256) void wavlm_gn_part_kernel(const float* X, int T0, int C, const int* len0, const double* mean, double* part) {
    __shared__ double red[4][64];
    const int cl = threadIdx.x & 63, ts = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + cl, b = blockIdx.z, ch = blockIdx.x;
    const int L = min(len0[b], T0);
    const int tbeg = ch * GN_CHUNK, tend = min(tbeg + GN_CHUNK, L);
    double s = 0.0;
    if (c < C) {
        const double m = SQ ? mean[(long)b * C + c] : 0.0;
        const float* x = X + (long)b * T0 * C + c;
        for (int t = tbeg + ts; t < tend; t += 4) {
            const double v = (double)x[(long)t * C] - m;
            s = SQ ? fma(v, v, s) : s + v;
        }
    }
    red[ts][cl] = s;
    __syncthreads();
    if (ts == 0 && c < C) part[((long)b * gridDim.x + ch) * C + c] = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
}

// the chunks of a row in order: mean[b][c] = sum / L (SQ: rstd[b][c] = 1 / sqrt(sum / L + eps))
template <bool SQ>
__global__ __launch_bounds__(256) void wavlm_gn_final_kernel(const double* part, int nchunk, int T0, int C, const int* len0, double* mean, float* rstd,
                                                            float eps) {
    const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (c >= C) return;
    const int L = min(len0[b], T0), nc = (L + GN_CHUNK - 1) / GN_CHUNK;
    double s = 0.0;
    for (int ch = 0; ch < nc; ++ch) s += part[((long)b * nchunk + ch) * C + c];
    if (SQ) rstd[(long)b * C + c] = (float)(1.0 / sqrt(s / (double)L + (double)eps));
    else mean[(long)b * C + c] = s / (double)L;
}

// X [B][T0][C] in place: GELU((x - mean) rstd gamma + beta), the difference in fp64; 0 at or past len0[b]
__global__ __launch_bounds__(256) void wavlm_gn_apply_kernel(float* X, int T0, int C, const int* len0, const double* mean, const float* rstd,
                                                            const float* gamma, const float* beta, long n4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const long e = i * 4, row = e / C;
    const int c = (int)(e - row * C);
    const int b = (int)(row / T0), t = (int)(row - (long)b * T0);
    float4* x4 = reinterpret_cast<float4*>(X) + i;
    if (t >= len0[b]) { *x4 = make_float4(0.f, 0.f, 0.f, 0.f); return; }
    const float4 v = *x4;
    const float xv[4] = {v.x, v.y, v.z, v.w};
    float r[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const long sc = (long)b * C + c + u;
        const float d = (float)((double)xv[u] - mean[sc]);
        r[u] = gelu_erf_(d * rstd[sc] * gamma[c + u] + beta[c + u]);
    }
    *x4 = make_float4(r[0], r[1], r[2], r[3]);
}

// h[row][g cg + c] = y[row][g cg + c] + pp[row][g cgp + c]: the padded groups of the positional convolution back onto the residual
__global__ __launch_bounds__(256) void wavlm_unpad_add_kernel(const float* y, const float* pp, float* h, long rows, int G, int cg, int cgp) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int H = G * cg;
    if (i >= rows * H) return;
    const long row = i / H;
    const int ch = (int)(i - row * H), g = ch / cg, c = ch - g * cg;
    h[i] = y[i] + pp[(row * G + g) * cgp + c];
}

// positional convolution v [G cg][cg][k] times scale[tap] (fp64) -> per group [k cgp][cgp] (row = tap cgp + ci), zeros in the padding
__global__ __launch_bounds__(256) void wavlm_pack_pos_kernel(const float* v, const double* scale, float* dst, int G, int cg, int cgp, int k) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)G * k * cgp * cgp) return;
    const int co = (int)(idx % cgp);
    long r = idx / cgp;
    const int ci = (int)(r % cgp); r /= cgp;
    const int tap = (int)(r % k), g = (int)(r / k);
    dst[idx] = (co < cg && ci < cg) ? (float)((double)v[((long)(g * cg + co) * cg + ci) * k + tap] * scale[tap]) : 0.f;
}

// dst [G cgp] = src [G cg] with zeros in the padding
__global__ __launch_bounds__(256) void wavlm_pad_vec_kernel(const float* src, float* dst, int G, int cg, int cgp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= G * cgp) return;
    const int g = i / cgp, c = i - g * cgp;
    dst[i] = c < cg ? src[g * cg + c] : 0.f;
}

int pad32(int n) { return (n + 31) & ~31; }
// channels of a positional-convolution group as the GEMM takes them
int pos_group_pad(const Trunk& t) { const int cg = t.hidden / t.pos_groups; return cg % 32 ? (cg + 63) & ~63 : cg; }

const float* pad_vec(WeightStore* s, const std::string& key, int G, int cg, int cgp, hipStream_t st) {
    if (cg == cgp) return s->R(key);
    float* d = s->alloc((long)G * cgp);
    if (d) hipLaunchKernelGGL(wavlm_pad_vec_kernel, dim3((G * cgp + 255) / 256), dim3(256), 0, st, s->R(key), d, G, cg, cgp);
    return d;
}

// finalize_trunk's pack_pos of these networks: the positional convolution with its groups padded to what the GEMM takes (zeros in
// the padding) into W.pos_w / W.pos_b
void pack_pos_padded(WeightStore* s, const TrunkKeys& k, const Trunk& t, TrunkWeights& W, const double* scale, hipStream_t st) {
    const int G = t.pos_groups, K = t.pos_k, cg = t.hidden / G, cgp = pos_group_pad(t);
    const long n = (long)G * K * cgp * cgp;
    float* pw = s->alloc(n);
    if (scale && pw)
        hipLaunchKernelGGL(wavlm_pack_pos_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s->R(k.ENC + "pos_conv_embed.conv.weight_v"), scale, pw,
                           G, cg, cgp, K);
    W.pos_w = pw;
    W.pos_b = pad_vec(s, k.ENC + "pos_conv_embed.conv.bias", G, cg, cgp, st);
}

// ---- workspace pieces: gnpart (fp64) [B][chunks][C_0] | gnmean (fp64) [B][C_0] | gnrstd [B][C_0], and yp, pp [B][T][G cgp] (the
// padded positional groups; empty where the groups need no padding)
struct GnWs { double *gnpart, *gnmean; float* gnrstd; int nchunk; };
struct PosWs { float *yp, *pp; };

void plan_groupnorm(Taker& tk, long B, int T0, int C0, GnWs& g) {
    g.nchunk = (T0 + GN_CHUNK - 1) / GN_CHUNK;
    g.gnpart = (double*)tk.take(2 * B * g.nchunk * C0); g.gnmean = (double*)tk.take(2 * B * C0); g.gnrstd = tk.take(B * C0);
}
void plan_pos_padded(const Trunk& t, Taker& tk, long B, long T, PosWs& p) {
    const long cgp = pos_group_pad(t), G = t.pos_groups, padded = cgp * G != t.hidden;
    p.yp = tk.take(padded ? B * T * G * cgp : 0); p.pp = tk.take(padded ? B * T * G * cgp : 0);
}

// layer 0 into fa: the raw convolution of x (row stride n), then the group norm over each row's own frames, GELU
void enqueue_conv0_groupnorm(const Trunk& c, const TrunkWeights& W, const TrunkWs& w, const GnWs& g, const float* x, int B, int n, hipStream_t st) {
    const int T0 = w.Tl[0], C0 = c.conv_dim[0];
    const int* len0 = w.lens + B;
    const Conv0P p{x, (long)n, W.conv_w[0], W.conv_b[0], w.fa, T0, C0, c.conv_kernel[0], c.conv_stride[0]};
    hipLaunchKernelGGL(wavlm_conv0_kernel, dim3((T0 + F0 - 1) / F0, B), dim3(256), 0, st, p);
    const dim3 pg(g.nchunk, (C0 + 63) / 64, B), fg((C0 + 255) / 256, B);
    hipLaunchKernelGGL(wavlm_gn_part_kernel<false>, pg, dim3(256), 0, st, w.fa, T0, C0, len0, nullptr, g.gnpart);
    hipLaunchKernelGGL(wavlm_gn_final_kernel<false>, fg, dim3(256), 0, st, g.gnpart, g.nchunk, T0, C0, len0, g.gnmean, nullptr, 0.f);
    hipLaunchKernelGGL(wavlm_gn_part_kernel<true>, pg, dim3(256), 0, st, w.fa, T0, C0, len0, g.gnmean, g.gnpart);
    hipLaunchKernelGGL(wavlm_gn_final_kernel<true>, fg, dim3(256), 0, st, g.gnpart, g.nchunk, T0, C0, len0, nullptr, g.gnrstd, 1e-5f);
    const long n4 = (long)B * T0 * C0 / 4;
    hipLaunchKernelGGL(wavlm_gn_apply_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, w.fa, T0, C0, len0, g.gnmean, g.gnrstd, W.conv_g[0],
                       W.conv_be[0], n4);
}

// h = y + GELU(pos_conv(y)) without its last frame (the LayerNorm that follows is enqueue_groupnorm_front's)
void enqueue_pos_padded(const Trunk& t, const TrunkWeights& W, const TrunkWs& w, const PosWs& p, int B, hipStream_t st) {
    const int T = w.T, H = t.hidden, G = t.pos_groups, K = t.pos_k, cg = H / G, cgp = pos_group_pad(t);
    const long rows = (long)B * T;
    if (cgp == cg) {
        gemm(w.y, H, T, cg, K, 1, -(K / 2), T, W.pos_w, cg, G, W.pos_b, w.h, 1, w.y, nullptr, B, st);
    } else {
        dex::launch_group_pad(w.y, p.yp, rows, G, cg, cgp, st);
        gemm(p.yp, G * cgp, T, cgp, K, 1, -(K / 2), T, W.pos_w, cgp, G, W.pos_b, p.pp, 1, nullptr, nullptr, B, st);
        hipLaunchKernelGGL(wavlm_unpad_add_kernel, dim3((unsigned)((rows * H + 255) / 256)), dim3(256), 0, st, w.y, p.pp, w.h, rows, G, cg, cgp);
    }
}

// everything before the encoder layers of a group-norm network: the frame plan (normalize: and the input normalisation), layer 0
// with its group norm, the GELU convolutions, the feature projection, and h = LN(y + GELU(pos_conv(y)))
void enqueue_groupnorm_front(const Trunk& t, const TrunkWeights& W, const TrunkWs& w, const GnWs& g, const PosWs& p, const float* wav,
                             const int32_t* lengths_host, int B, int n, bool normalize, hipStream_t st) {
    enqueue_front(t, w, wav, lengths_host, B, n, normalize, st);
    enqueue_conv0_groupnorm(t, W, w, g, normalize ? w.xn : wav, B, n, st);
    enqueue_projection(t, W, w, enqueue_conv_tail<false>(t, W, w, B, 1, st), B, st);
    enqueue_pos_padded(t, W, w, p, B, st);
    layer_norm<false>(w.h, w.h, (long)B * w.T, w.T, t.hidden, W.enc_g, W.enc_be, t.layer_norm_eps, nullptr, st);
}

}  // namespace
}  // namespace wavenc
}  // namespace dex
