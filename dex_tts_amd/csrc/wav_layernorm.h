// wav_layernorm.h — the first layer of the layer-norm feature extractor (feat_extract_norm = "layer": asr.hip's wav2vec 2.0 CTC
// network and ecapa.hip's WavLM-large trunk):
//
//   asr_conv0_kernel     the first convolution (Cin = 1, k = 10, s = 5) with its LayerNorm and GELU: 8 frames x all channels per
//                        workgroup, the sample window in LDS, a thread's taps in registers; the 3200 frames/s x 512 tensor is written once.
// Includes wav_trunk.h; everything has internal linkage.
#pragma once
#include "wav_trunk.h"

namespace dex {
namespace wavenc {
namespace {

struct LnConv0P { const float* x; long x_ld; const float* w; const float* bias; const float* gamma; const float* beta; float eps;
                float* out; int T0, C, k, s; const int* len1; };

// frames [F0 blockIdx.x, + F0) of utterance blockIdx.y: conv (taps ascending, fmaf) -> LayerNorm over the C channels -> GELU; frames at
// or past len1[b] are stored as 0, frames at or past T0 are not stored
__global__ __launch_bounds__(256) void asr_conv0_kernel(const LnConv0P p) {
    __shared__ float xs[(F0 - 1) * S0_MAX + K0_MAX];
    __shared__ float red[4][F0];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y, t0 = blockIdx.x * F0;
    const int nwin = (F0 - 1) * p.s + p.k;
    const float* x = p.x + (long)b * p.x_ld;
    for (int i = tid; i < nwin; i += 256) {
        const long idx = (long)t0 * p.s + i;
        xs[i] = idx < p.x_ld ? x[idx] : 0.f;
    }
    float w[2][K0_MAX], v[2][F0], g[2], be[2];
    bool cv[2];
#pragma unroll
    for (int ci = 0; ci < 2; ++ci) {
        const int c = tid + 256 * ci;
        cv[ci] = c < p.C;
#pragma unroll
        for (int j = 0; j < K0_MAX; ++j) w[ci][j] = (cv[ci] && j < p.k) ? p.w[(long)c * p.k + j] : 0.f;
        const float bs = (cv[ci] && p.bias) ? p.bias[c] : 0.f;
        g[ci] = cv[ci] ? p.gamma[c] : 0.f;
        be[ci] = cv[ci] ? p.beta[c] : 0.f;
#pragma unroll
        for (int f = 0; f < F0; ++f) v[ci][f] = bs;
    }
    __syncthreads();
#pragma unroll
    for (int f = 0; f < F0; ++f) {
#pragma unroll
        for (int j = 0; j < K0_MAX; ++j) {
            if (j < p.k) {
                const float xv = xs[f * p.s + j];
                v[0][f] = fmaf(w[0][j], xv, v[0][f]);
                v[1][f] = fmaf(w[1][j], xv, v[1][f]);
            }
        }
    }
    // mean, then the centred sum of squares: two fixed-order reductions (butterfly in the wave, then the four waves in order)
    float mean[F0], rstd[F0];
#pragma unroll
    for (int f = 0; f < F0; ++f) {
        float s = (cv[0] ? v[0][f] : 0.f) + (cv[1] ? v[1][f] : 0.f);
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) red[wave][f] = s;
    }
    __syncthreads();
#pragma unroll
    for (int f = 0; f < F0; ++f) mean[f] = (((red[0][f] + red[1][f]) + red[2][f]) + red[3][f]) / (float)p.C;
    __syncthreads();
#pragma unroll
    for (int f = 0; f < F0; ++f) {
        const float d0 = cv[0] ? v[0][f] - mean[f] : 0.f, d1 = cv[1] ? v[1][f] - mean[f] : 0.f;
        float q = fmaf(d1, d1, d0 * d0);
        for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
        if (lane == 0) red[wave][f] = q;
    }
    __syncthreads();
#pragma unroll
    for (int f = 0; f < F0; ++f) rstd[f] = 1.f / sqrtf((((red[0][f] + red[1][f]) + red[2][f]) + red[3][f]) / (float)p.C + p.eps);
    const int L1 = p.len1[b];
#pragma unroll
    for (int f = 0; f < F0; ++f) {
        const int t = t0 + f;
        if (t >= p.T0) break;
        float* o = p.out + ((long)b * p.T0 + t) * p.C;
#pragma unroll
        for (int ci = 0; ci < 2; ++ci)
            if (cv[ci]) o[tid + 256 * ci] = t < L1 ? gelu_erf_((v[ci][f] - mean[f]) * rstd[f] * g[ci] + be[ci]) : 0.f;
    }
}

// layer 0 into fa: the convolution of x (row stride n) with its LayerNorm and GELU
void enqueue_conv0_layernorm(const Trunk& c, const TrunkWeights& W, const TrunkWs& w, const float* x, int B, int n, hipStream_t st) {
    const LnConv0P p{x, (long)n, W.conv_w[0], W.conv_b[0], W.conv_g[0], W.conv_be[0], c.layer_norm_eps, w.fa, w.Tl[0], c.conv_dim[0],
                     c.conv_kernel[0], c.conv_stride[0], w.lens + B};
    hipLaunchKernelGGL(asr_conv0_kernel, dim3((w.Tl[0] + F0 - 1) / F0, B), dim3(256), 0, st, p);
}

}  // namespace
}  // namespace wavenc
}  // namespace dex
