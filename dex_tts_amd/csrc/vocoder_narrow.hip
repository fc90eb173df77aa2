// vocoder_narrow.hip — the generator's narrow stages: widths that are multiples of 8, at most 64, and not multiples of 32 (the 48- and
// 24-channel tail of BigVGAN 22 kHz / 80 bands, the 16- and 8-channel tail of HiFi-GAN V2), which the implicit GEMM's 32-wide tiles
// cannot take.  Activations are channels-last fp32 [B][L][C], as on the wide path.
//
// The stages hold few channels at many samples, so each layer's weights are small (48 x 48 x 11 floats = 101 KB at most) and every
// output sample needs the whole of them.  The kernels are direct fp32 convolutions on the vector ALU: a thread owns one output sample
// and CO output channels in registers, reads its input rows with 16-byte loads, and the weights — the same address in every lane,
// so they come through scalar loads into SGPRs — feed fmaf chains in (tap, input channel) order.  Exact fp32 in every precision
// mode (dex_voc_set_precision's bf16 / fp16 modes round only the wide stages' operands); no atomics, so bitwise repeatable.
#include "kernels.h"
#include "vocoder_len.h"

namespace dex {

namespace {

// output channels per thread: 12 at widths 24 and 48, else 8.  The weights of one input-channel quad (4 x CO floats) sit in SGPRs; more
// than 12 channels would spill them.
template <int C> constexpr int narrow_co() { return C % 12 == 0 ? 12 : 8; }

__device__ __forceinline__ float lrelu(float v, float sl) { return v > 0.f ? v : v * sl; }

// Conv1d(C -> C, k, dilation dil, padding dil * (k - 1) / 2) on leaky_relu(x, slope) (slope 0: x as stored), + bias, + residual.
//   y[l][co] = (sum_{tap, ci} x[l + tap * dil - pad][ci] * w[tap][ci][co] + bias[co]) + res[l][co]
// W packed [tap][ci][co] (dex_voc_finalize).  Grid: x = sample tiles of 256, y = C / CO output-channel chunks, z = batch.
template <int C>
__global__ __launch_bounds__(256) void narrow_conv1d_kernel(const float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ bias,
                                                            const float* __restrict__ res, float* __restrict__ Y, int L, int k, int dil, float slope,
                                                            const int* __restrict__ len, int R) {
    constexpr int CO = narrow_co<C>();
    static_assert(C % 8 == 0 && CO % 4 == 0, "narrow widths");
    const int l = blockIdx.x * 256 + threadIdx.x;
    const int co0 = blockIdx.y * CO, b = blockIdx.z;
    const float* Xb = X + (long)b * L * C;
    const int Lb = voc_valid_len(len, b, R, L);                       // ragged batch: the utterance ends here (kernels.h)
    const long row = ((long)b * L + l) * C + co0;
    if (l >= Lb) {         // past the utterance's end: zeros, nothing loaded (a block wholly past it leaves here as one)
        if (l < L) {
#pragma unroll
            for (int o = 0; o < CO; o += 4) *reinterpret_cast<float4*>(Y + row + o) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
    const int half = dil * ((k - 1) / 2);
    float acc[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) acc[o] = 0.f;
    for (int tap = 0; tap < k; ++tap) {
        const int li = l + tap * dil - half;
        const bool ok = (unsigned)li < (unsigned)Lb;                  // zero padding outside [0, Lb)  (l < Lb <= L here)
        const float* xr = Xb + (long)(ok ? li : 0) * C;
        const float* wt = W + (long)tap * C * C + co0;
#pragma unroll 1
        for (int c4 = 0; c4 < C; c4 += 4) {
            float4 v = ok ? *reinterpret_cast<const float4*>(xr + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (slope != 0.f) { v.x = lrelu(v.x, slope); v.y = lrelu(v.y, slope); v.z = lrelu(v.z, slope); v.w = lrelu(v.w, slope); }
            const float xv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int o = 0; o < CO; ++o) acc[o] = fmaf(xv[q], wt[(c4 + q) * C + o], acc[o]);
        }
    }
#pragma unroll
    for (int o = 0; o < CO; o += 4) {
        float4 r = make_float4(acc[o] + bias[co0 + o], acc[o + 1] + bias[co0 + o + 1], acc[o + 2] + bias[co0 + o + 2], acc[o + 3] + bias[co0 + o + 3]);
        if (res) {
            const float4 x = *reinterpret_cast<const float4*>(res + row + o);
            r.x += x.x; r.y += x.y; r.z += x.z; r.w += x.w;
        }
        *reinterpret_cast<float4*>(Y + row + o) = r;
    }
}

// ConvTranspose1d(Cin -> C, k, stride u, padding pad) on leaky_relu(x, slope), GEMM and overlap-add in one pass:
//   y[t][co] = bias[co] + sum_{j = (t+pad) mod u, +u, .. < k} ( sum_ci x[(t+pad-j)/u][ci] * w[ci][j][co] )     (0 <= (t+pad-j)/u < L)
// the per-tap sums added to the bias in ascending j, as the wide path's GEMM + launch_convt_fold do.  W packed [ci][j][co].
// A block owns one phase r = (t + pad) mod u, so the taps j = r, r + u, .. and their weights are the same in every lane: thread q
// computes t = q u + r - pad.  Grid: x = q tiles of 256, y = u * (C / CO) (phase fastest), z = batch.
template <int C>
__global__ __launch_bounds__(256) void narrow_convt_kernel(const float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ bias,
                                                           float* __restrict__ Y, int L, int Cin, int k, int u, int pad, float slope,
                                                           const int* __restrict__ len, int R) {
    constexpr int CO = narrow_co<C>();
    const int q = blockIdx.x * 256 + threadIdx.x;
    const int r = blockIdx.y % u, co0 = (blockIdx.y / u) * CO, b = blockIdx.z;
    const long Lo = (long)L * u;
    const long t = (long)q * u + r - pad;
    const bool valid = t >= 0 && t < Lo;
    const float* Xb = X + (long)b * L * Cin;
    const int Lb = voc_valid_len(len, b, R, L);                       // the utterance's input samples; its output ends at Lb * u
    float* yr = Y + ((long)b * Lo + t) * C + co0;
    if (t >= (long)Lb * u) {          // past the utterance's end: zeros, nothing loaded
        if (valid) {
#pragma unroll
            for (int o = 0; o < CO; o += 4) *reinterpret_cast<float4*>(yr + o) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
    float acc[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) acc[o] = bias[co0 + o];
    for (int j = r; j < k; j += u) {
        const int l = q - (j - r) / u;
        const bool ok = valid && l >= 0 && l < Lb;
        const float* xr = Xb + (long)(ok ? l : 0) * Cin;
        const float* wj = W + (long)j * C + co0;
        float s[CO];
#pragma unroll
        for (int o = 0; o < CO; ++o) s[o] = 0.f;
#pragma unroll 1
        for (int c4 = 0; c4 < Cin; c4 += 4) {
            float4 v = ok ? *reinterpret_cast<const float4*>(xr + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (slope != 0.f) { v.x = lrelu(v.x, slope); v.y = lrelu(v.y, slope); v.z = lrelu(v.z, slope); v.w = lrelu(v.w, slope); }
            const float xv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
                const float* w = wj + (long)(c4 + qq) * k * C;
#pragma unroll
                for (int o = 0; o < CO; ++o) s[o] = fmaf(xv[qq], w[o], s[o]);
            }
        }
        if (ok) {
#pragma unroll
            for (int o = 0; o < CO; ++o) acc[o] += s[o];
        }
    }
    if (!valid) return;
#pragma unroll
    for (int o = 0; o < CO; o += 4) *reinterpret_cast<float4*>(yr + o) = make_float4(acc[o], acc[o + 1], acc[o + 2], acc[o + 3]);
}

// The anti-aliased activation of vocoder_elem.hip's aa_snake_kernel with the channel lanes packed: a block of 256 threads is G = 256 / C
// groups of C channel lanes (aa_snake_kernel: 4 groups of 64, of which C are busy).  Per element the same arithmetic in the same order.
constexpr int ASN_T = 64, ASN_S = 2 * ASN_T + 11;
template <int C>
__global__ __launch_bounds__(256) void aa_snake_narrow_kernel(const AaSnakeP p) {
    constexpr int G = 256 / C;
    __shared__ float s[ASN_S][C];
    __shared__ float f[12];
    const int tid = threadIdx.x, c = tid % C, grp = tid / C;
    const int t0 = blockIdx.x * ASN_T, b = blockIdx.y;
    const bool act = grp < G;
    const int Lb = voc_valid_len(p.len, b, p.R, p.L);
    if (t0 >= Lb) {        // (uniform, before any barrier) a tile wholly past the utterance's end: zeros
        if (act)
            for (int t = t0 + grp; t < min(t0 + ASN_T, p.L); t += G) p.Y[((long)b * p.L + t) * C + c] = 0.f;
        return;
    }
    if (tid < 12) f[tid] = p.filt[tid];
    __syncthreads();
    const float a = p.a[c], ib = p.inv_b[c];
    const float* X = p.X + (long)b * p.L * C + c;
    const int L2 = 2 * Lb;
    if (act)
        for (int qi = grp; qi < ASN_S; qi += G) {
            const int m = min(max(2 * t0 - 5 + qi, 0), L2 - 1);
            float up = 0.f;
            const int j0 = (m + 5) >> 1;
#pragma unroll
            for (int jj = 0; jj < 6; ++jj) {
                const int j = j0 + jj, kk = m + 15 - 2 * j;
                const int xi = min(max(j - 5, 0), Lb - 1);
                if (kk >= 0) up = fmaf(X[(long)xi * C], f[kk], up);
            }
            up *= 2.f;
            const float sn = sinf(up * a);
            s[qi][c] = up + ib * (sn * sn);
        }
    __syncthreads();
    if (!act) return;
    float* Y = p.Y + (long)b * p.L * C + c;
    for (int tt = grp; tt < ASN_T; tt += G) {
        const int t = t0 + tt;
        if (t >= p.L) break;
        float acc = 0.f;
#pragma unroll
        for (int kk = 0; kk < 12; ++kk) acc = fmaf(s[2 * tt + kk][c], f[kk], acc);
        Y[(long)t * C] = t < Lb ? acc : 0.f;
    }
}

template <int C>
void conv1d_w(const NarrowConvP& p, hipStream_t st) {
    constexpr int CO = narrow_co<C>();
    hipLaunchKernelGGL(narrow_conv1d_kernel<C>, dim3((unsigned)((p.L + 255) / 256), C / CO, p.B), dim3(256), 0, st,
                       p.X, p.W, p.bias, p.res, p.Y, p.L, p.k, p.dil, p.slope, p.len, p.R);
}
template <int C>
void convt_w(const NarrowConvTP& p, hipStream_t st) {
    constexpr int CO = narrow_co<C>();
    const long nq = (long)p.L + (p.pad + p.u - 1) / p.u + 1;      // q = (t + pad - r) / u over t in [0, L u)
    hipLaunchKernelGGL(narrow_convt_kernel<C>, dim3((unsigned)((nq + 255) / 256), p.u * (C / CO), p.B), dim3(256), 0, st,
                       p.X, p.W, p.bias, p.Y, p.L, p.Cin, p.k, p.u, p.pad, p.slope, p.len, p.R);
}
template <int C>
void aa_w(const AaSnakeP& p, hipStream_t st) {
    hipLaunchKernelGGL(aa_snake_narrow_kernel<C>, dim3((unsigned)((p.L + ASN_T - 1) / ASN_T), p.B), dim3(256), 0, st, p);
}

}  // namespace

bool voc_narrow_width(int C) { return C % 8 == 0 && C <= 64 && C % 32 != 0; }

#define DEX_NARROW_SWITCH(C, F, p, st)                                                                    \
    switch (C) {                                                                                          \
        case 8: F<8>(p, st); break;   case 16: F<16>(p, st); break; case 24: F<24>(p, st); break;         \
        case 40: F<40>(p, st); break; case 48: F<48>(p, st); break; case 56: F<56>(p, st); break;         \
        default: break;                                                                                   \
    }

void launch_narrow_conv1d(const NarrowConvP& p, hipStream_t st) { DEX_NARROW_SWITCH(p.C, conv1d_w, p, st) }
void launch_narrow_convt(const NarrowConvTP& p, hipStream_t st) { DEX_NARROW_SWITCH(p.C, convt_w, p, st) }
void launch_aa_snake_narrow(const AaSnakeP& p, hipStream_t st) { DEX_NARROW_SWITCH(p.C, aa_w, p, st) }

}  // namespace dex
