// wav_encoder.h — the kernels the waveform networks of the C ABI share (asr.hip: wav2vec 2.0 CTC; wavlm.hip: WavLM x-vector; ecapa.hip:
// WavLM-large + ECAPA-TDNN; mos.hip: UTMOS; whisper.hip: the Whisper encoder) and their launches: the input normalisation, the ragged-batch plan, row LayerNorm, the
// weight packing (weight norm folded in fp64), the k-split sum of fc2, the host wrappers that spell a 1 x k convolution / Linear as
// a launch of the exact-fp32 implicit GEMM, and the walk over a batch in tables of rows that travel as kernel arguments.  Every
// per-row sum has a fixed order that does not depend on the batch.  The host layer above them (geometry, keys, packing, workspace,
// the encoder layer, entry points) is wav_trunk.h, which includes this file; everything has internal linkage.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "kernels.h"
#include "weight_store.h"

namespace dex {
namespace wavenc {
namespace {

constexpr int TAB = 128;                 // table entries per launch (they travel as kernel arguments)
constexpr int MAXC = 8;                  // feature-extractor layers (DEX_ASR_MAX_CONV, DEX_WAVLM_MAX_CONV)

struct Tab { int n; int a[TAB]; };
struct ConvSpec { int n; int k[MAXC], s[MAXC]; };

__device__ __forceinline__ float gelu_erf_(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// deterministic sum of one double per thread over an N-thread workgroup (LDS tree); every thread gets the total
template <int N>
__device__ __forceinline__ double block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = N / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double t = red[0];
    __syncthreads();
    return t;
}

constexpr int NORM_T = 1024;             // threads of the normalisation's workgroup (one utterance each)

// a = utterance lengths; rows r0 .. r0 + n of wav / out [.][ld].  Thread t owns samples t, t + 1024, ...; four of them are in flight
// at a time, in four partial sums that meet in a fixed order
__global__ __launch_bounds__(NORM_T) void asr_norm_kernel(const float* wav, float* out, long ld, int r0, const Tab R) {
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
    const double sd = sqrt(block_sum<NORM_T>((q[0] + q[1]) + (q[2] + q[3]), red) / (double)L + 1e-7);
    for (long i = tid; i < ld; i += NORM_T) o[i] = i < L ? (float)(((double)w[i] - mean) / sd) : 0.f;
}

// lens [n_conv + 1][B]: row 0 the samples, row l + 1 the frames after convolution l; mask [B][T] = frame < the utterance's last count
__global__ __launch_bounds__(256) void asr_plan_kernel(int* lens, float* mask, int B, int T, int r0, const ConvSpec cs, const Tab R) {
    const int b = r0 + blockIdx.x;
    int L = R.a[blockIdx.x];
    if (threadIdx.x == 0) lens[b] = L;
    for (int l = 0; l < cs.n; ++l) {
        L = L >= cs.k[l] ? (L - cs.k[l]) / cs.s[l] + 1 : 0;
        if (threadIdx.x == 0) lens[(long)(l + 1) * B + b] = L;
    }
    if (mask)
        for (int t = threadIdx.x; t < T; t += 256) mask[(long)b * T + t] = t < L ? 1.f : 0.f;
}

struct LnP { const float* X; float* Y; long rows; int T, C; const float* gamma; const float* beta; float eps; const int* len; };

// one wave per row of C channels (C % 4 == 0), Y may be X.  GELU: the activation follows, and rows at or past len[b] are stored as 0
template <bool GELU>
__global__ __launch_bounds__(256) void asr_ln_kernel(const LnP p) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.rows) return;
    const float4* x = reinterpret_cast<const float4*>(p.X + row * p.C);
    float4* y = reinterpret_cast<float4*>(p.Y + row * p.C);
    const int n4 = p.C >> 2;
    if (GELU && p.len) {
        const long b = row / p.T;
        if ((int)(row - b * p.T) >= p.len[b]) {
            for (int c = lane; c < n4; c += 64) y[c] = make_float4(0.f, 0.f, 0.f, 0.f);
            return;
        }
    }
    float s = 0.f;
    for (int c = lane; c < n4; c += 64) { const float4 v = x[c]; s += (v.x + v.y) + (v.z + v.w); }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)p.C;
    float q = 0.f;
    for (int c = lane; c < n4; c += 64) {
        const float4 v = x[c];
        const float a = v.x - mean, b = v.y - mean, cc = v.z - mean, d = v.w - mean;
        q += fmaf(a, a, b * b) + fmaf(cc, cc, d * d);
    }
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = 1.f / sqrtf(q / (float)p.C + p.eps);
    const float4* g4 = reinterpret_cast<const float4*>(p.gamma);
    const float4* b4 = reinterpret_cast<const float4*>(p.beta);
    for (int c = lane; c < n4; c += 64) {
        const float4 v = x[c], g = g4[c], be = b4[c];
        float4 r = make_float4((v.x - mean) * rstd * g.x + be.x, (v.y - mean) * rstd * g.y + be.y, (v.z - mean) * rstd * g.z + be.z,
                               (v.w - mean) * rstd * g.w + be.w);
        if (GELU) { r.x = gelu_erf_(r.x); r.y = gelu_erf_(r.y); r.z = gelu_erf_(r.z); r.w = gelu_erf_(r.w); }
        y[c] = r;
    }
}

// scale[tap] = g[tap] / ||v[:, :, tap]||, the norm over the n = cout x cin_g entries of the tap in fp64; one workgroup per tap
__global__ __launch_bounds__(256) void asr_wn_scale_kernel(const float* v, const float* g, double* scale, long n, int k) {
    __shared__ double red[256];
    const int tap = blockIdx.x;
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) { const double x = (double)v[i * k + tap]; s = fma(x, x, s); }
    const double tot = block_sum<256>(s, red);
    if (threadIdx.x == 0) scale[tap] = (double)g[tap] / sqrt(tot);
}

// Conv1d / Linear weight [G cout_g][cin_g][k] -> the GEMM operand of each group [k cin_g][ldn] at column coff (row = tap cin_g + ci),
// times scale[tap] in fp64 where given
__global__ __launch_bounds__(256) void asr_pack_kernel(const float* src, float* dst, int G, int cout_g, int cin_g, int k, int ldn, int coff,
                                                       const double* scale) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)G * k * cin_g * cout_g) return;
    const int co = (int)(idx % cout_g);
    long r = idx / cout_g;
    const int ci = (int)(r % cin_g); r /= cin_g;
    const int tap = (int)(r % k);
    const int g = (int)(r / k);
    const float sv = src[((long)(g * cout_g + co) * cin_g + ci) * k + tap];
    dst[((long)(g * k + tap) * cin_g + ci) * ldn + coff + co] = scale ? (float)((double)sv * scale[tap]) : sv;
}

// h += ((p_0 + p_1) + ... + p_{ks-1}) + bias: the k-split slabs of fc2 ([ks][n] floats, n % 4 == 0), in slab order
__global__ __launch_bounds__(256) void asr_ksum_kernel(const float4* part, long n4, int ks, const float4* bias, int c4, float4* h) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    float4 a = part[i];
    for (int s = 1; s < ks; ++s) { const float4 v = part[(long)s * n4 + i]; a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
    const float4 b = bias[i % c4], r = h[i];
    h[i] = make_float4(r.x + (a.x + b.x), r.y + (a.y + b.y), r.z + (a.z + b.z), r.w + (a.w + b.w));
}

// [G cout_g][cin_g][k] -> [G][k cin_g][ldn] at column coff of dst (already allocated)
void pack_into(const float* src, float* dst, int G, int cout_g, int cin_g, int k, int ldn, int coff, const double* scale, hipStream_t st) {
    const long n = (long)G * k * cin_g * cout_g;
    hipLaunchKernelGGL(asr_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, dst, G, cout_g, cin_g, k, ldn, coff, scale);
}
const float* pack(WeightStore* s, const std::string& key, int G, int cout_g, int cin_g, int k, const double* scale, hipStream_t st) {
    float* d = s->alloc((long)G * k * cin_g * cout_g);
    if (d) pack_into(s->R(key), d, G, cout_g, cin_g, k, cout_g, 0, scale, st);
    return d;
}

long up64(long n) { return (n + 63) & ~63L; }

// C [B][To][ldc] = epi(conv1d(A [B][Ti][lda])): kernel k, stride s, left offset off, taps dil apart, `groups` groups of cin -> N channels each
void gemm(const float* A, int lda, int Ti, int cin, int k, int stride, int off, int To, const float* W, int N, int groups, const float* bias,
          float* C, int act, const float* res, const float* outmask, int B, hipStream_t st, int ksplit = 1, int dil = 1, bool res_shared = false) {
    dex::IGemmP g{};
    const int ldc = N * groups;
    g.A = A; g.lda = lda; g.a_bstride = (long)Ti * lda;
    g.Hi = 1; g.Wi = Ti; g.Cin = cin;
    g.KH = 1; g.KW = k; g.sh = 1; g.sw = stride; g.off_w = off; g.step_h = 1; g.step_w = dil;
    g.Ho = 1; g.Wo = To;
    g.W = W; g.w_gstride = (long)k * cin * N; g.N = N; g.K = k * cin; g.ksplit = ksplit; g.groups = groups; g.bias = bias;
    g.C = C; g.ldc = ldc; g.c_bstride = (long)To * ldc; g.c_sstride = (long)B * To * ldc;
    g.OHf = 1; g.OWf = To; g.osh = 1; g.osw = 1;
    g.inmask_ws = 1; g.outmask = outmask; g.outmask_ws = 1; g.mask_bstride = To; g.gate_nstride = 1;
    g.act = act;
    g.res = res; g.ldres = ldc; g.res_bstride = res_shared ? 0 : (long)To * ldc;      // res_shared: one [To][ldc] table for every row
    g.B = B;
    dex::launch_igemm(g, dex::PREC_FP32, st);
}
void linear(const float* A, int K, const float* W, int N, const float* bias, float* C, int act, const float* res, const float* outmask, int T, int B,
            hipStream_t st) {
    gemm(A, K, T, K, 1, 1, 0, T, W, N, 1, bias, C, act, res, outmask, B, st);
}
template <bool GELU>
void layer_norm(const float* X, float* Y, long rows, int T, int C, const float* g, const float* b, float eps, const int* len, hipStream_t st) {
    const LnP p{X, Y, rows, T, C, g, b, eps, len};
    hipLaunchKernelGGL(asr_ln_kernel<GELU>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, p);
}

// the batch in tables of TAB rows: fill(R, e, b) sets entry e of a zeroed table to row b = r0 + e, launch(r0, R) takes the R.n rows
template <class T, class Fill, class Launch>
void for_each_row_table(int B, Fill fill, Launch launch) {
    for (int r0 = 0; r0 < B; r0 += TAB) {
        T R;
        std::memset(&R, 0, sizeof R);
        R.n = B - r0 < TAB ? B - r0 : TAB;
        for (int e = 0; e < R.n; ++e) fill(R, e, r0 + e);
        launch(r0, R);
    }
}

void enqueue_norm(const float* wav, const int32_t* lengths_host, int B, int n, float* out, hipStream_t st) {
    for_each_row_table<Tab>(B, [&](Tab& R, int e, int b) { R.a[e] = lengths_host[b]; }, [&](int r0, const Tab& R) {
        hipLaunchKernelGGL(asr_norm_kernel, dim3(R.n), dim3(NORM_T), 0, st, wav, out, (long)n, r0, R);
    });
}

// the per-layer frame counts of every row of the batch, and the encoder's frame mask (asr_plan_kernel)
void enqueue_plan(const ConvSpec& cs, const int32_t* lengths_host, int B, int T, int* lens, float* mask, hipStream_t st) {
    for_each_row_table<Tab>(B, [&](Tab& R, int e, int b) { R.a[e] = lengths_host[b]; }, [&](int r0, const Tab& R) {
        hipLaunchKernelGGL(asr_plan_kernel, dim3(R.n), dim3(256), 0, st, lens, mask, B, T, r0, cs, R);
    });
}

}  // namespace
}  // namespace wavenc
}  // namespace dex
