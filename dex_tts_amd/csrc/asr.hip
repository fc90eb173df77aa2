// asr.hip — the reference's ASR score on the device (src/metric.py:21-67, Evaluater.transcribe / calculate_asr_score): the forward pass
// of HF's Wav2Vec2ForCTC in eval mode (facebook/wav2vec2-large-960h-lv60-self: layer-norm feature extractor, stable layer norm,
// head_dim 64) and greedy CTC.  fp32 throughout, channels-last [B][T][C].  C ABI dex_asr_*.
//
//   asr_norm_kernel      Wav2Vec2FeatureExtractor's do_normalize, one workgroup per utterance: mean and biased variance over the row's
//                        own length in fp64 (two passes, fixed-order trees), (x - mean) / sqrt(var + 1e-7) rounded to fp32 once, 0 past it.
//   asr_plan_kernel      the per-layer frame counts of every utterance (floor((L - k) / s) + 1 chained) and the encoder's frame mask,
//                        on the device: the lengths arrive as kernel arguments, nothing is copied from host memory.
//   asr_conv0_kernel     the first convolution (Cin = 1, k = 10, s = 5) with its LayerNorm and GELU: 8 frames x all channels per
//                        workgroup, the sample window in LDS, a thread's taps in registers; the 3200 frames/s x 512 tensor is written once.
//   launch_igemm         (igemm.hip, exact-fp32 MFMA) every other contraction: the strided 1 x k convolutions of layers 1-6, the feature
//                        projection, the grouped positional convolution (bias, GELU and the residual in its epilogue), q|k|v as one
//                        GEMM, out_proj and fc2 with the residual, fc1 with GELU, lm_head.  ksplit = 1 everywhere but fc2, whose K =
//                        intermediate_size is split intermediate / hidden ways (4 in the default config: 64 workgroups of 128 K tiles
//                        become 256 of 32 at one utterance) - a number fixed by the config alone, like the order in which
//                        asr_ksum_kernel adds the slabs; the two tile forms walk K in the same order: a row's sums do not depend on B or T.
//   asr_ln_kernel        affine LayerNorm over the channels of a row, one wave per row, any C % 4 == 0 (launch_ln_cl stops at 256
//                        channels; these rows are 512 / 1024 wide); <GELU> adds the activation and zeroes the rows at or past an
//                        utterance's frame count (feature-extractor layers 1-6).
//   launch_attention     (attention.hip) the generic fp32 kernel at head_dim 64, q scaled by 1/8 on load, keys masked by kv_len.
//   asr_wn_scale_kernel, asr_pack_kernel     weight_norm(dim = 2) of the positional convolution folded once at load - g[k] / ||v[:, :, k]||
//                        with the norm in fp64 - and every weight transposed to the GEMM's [K][N] operand.
//   asr_ctc_kernel       greedy CTC, one workgroup per utterance: the first index of each frame's maximum, repeats collapsed, blanks
//                        dropped, compacted with a block scan; ids and counts are all that travels to the host.
// Every per-row sum has a fixed order that does not depend on the batch: a row's logits are bitwise the row run alone.
// What the WavLM x-vector network (wavlm.hip) shares - asr_norm / plan / ln / wn_scale / pack / ksum and the launch_igemm wrappers -
// lives in wav_encoder.h; the first convolution and the CTC kernel are here.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dex_amd.h"
#include "kernels.h"
#include "wav_encoder.h"
#include "weight_store.h"

using namespace dex::wavenc;      // the pieces shared with wavlm.hip: norm, plan, LayerNorm, packing, the GEMM wrappers

namespace {

static_assert(MAXC == DEX_ASR_MAX_CONV, "ConvSpec holds DEX_ASR_MAX_CONV layers");
constexpr int F0 = 8;                   // frames per workgroup of the first convolution
constexpr int K0_MAX = 16, S0_MAX = 16;  // its kernel and stride bounds (taps in registers, window in LDS)
constexpr int C0_MAX = 512;              // its channels: two per thread
constexpr int MAX_B = 1024;              // grid z = B x 16 groups stays inside 65535
constexpr int MAX_SAMPLES = 1 << 24;     // 17 minutes at 16 kHz
constexpr long MAX_ROWS = 1L << 26;      // B x frames of the first layer: every grid inside 2^31, every element index inside 2^63

struct Conv0P { const float* x; long x_ld; const float* w; const float* bias; const float* gamma; const float* beta; float eps;
                float* out; int T0, C, k, s; const int* len1; };

// frames [F0 blockIdx.x, + F0) of utterance blockIdx.y: conv (taps ascending, fmaf) -> LayerNorm over the C channels -> GELU; frames at
// or past len1[b] are stored as 0, frames at or past T0 are not stored
__global__ __launch_bounds__(256) void asr_conv0_kernel(const Conv0P p) {
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

// a = frame counts; utterances r0 .. r0 + n of logits [.][T][V] -> ids [.][T], counts [.]
__global__ __launch_bounds__(256) void asr_ctc_kernel(const float* logits, int T, int V, int* ids, int* counts, int r0, const Tab R) {
    __shared__ int arg[257];
    __shared__ int scan[256];
    const int tid = threadIdx.x, b = r0 + blockIdx.x, F = R.a[blockIdx.x];
    const float* lg = logits + (long)b * T * V;
    int* out = ids + (long)b * T;
    int base = 0, carry = -1;
    for (int t0 = 0; t0 < F; t0 += 256) {
        const int t = t0 + tid;
        int a = -1;
        if (t < F) {
            const float* row = lg + (long)t * V;
            float best = row[0];
            a = 0;
            for (int j = 1; j < V; ++j) { const float x = row[j]; if (x > best) { best = x; a = j; } }
        }
        arg[tid + 1] = a;
        if (tid == 0) arg[0] = carry;
        __syncthreads();
        const int keep = (t < F && a != 0 && a != arg[tid]) ? 1 : 0;
        scan[tid] = keep;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int add = tid >= o ? scan[tid - o] : 0;
            __syncthreads();
            scan[tid] += add;
            __syncthreads();
        }
        if (keep) out[base + scan[tid] - 1] = a;
        base += scan[255];
        carry = arg[256];
        __syncthreads();
    }
    for (int t = base + tid; t < T; t += 256) out[t] = 0;
    if (tid == 0) counts[b] = base;
}

thread_local std::string g_create_err;

int create_fail(const char* fmt, const char* field) {
    char buf[256];
    snprintf(buf, sizeof buf, fmt, field);
    g_create_err = buf;
    return DEX_ERR_ARG;
}

DexAsrConfig default_config() {
    DexAsrConfig c;
    std::memset(&c, 0, sizeof c);
    const int k[7] = {10, 3, 3, 3, 3, 2, 2}, s[7] = {5, 2, 2, 2, 2, 2, 2};
    c.n_conv = 7;
    for (int i = 0; i < 7; ++i) { c.conv_dim[i] = 512; c.conv_kernel[i] = k[i]; c.conv_stride[i] = s[i]; }
    c.conv_bias = 1; c.feat_extract_norm_layer = 1;
    c.hidden = 1024; c.n_layers = 24; c.n_heads = 16; c.intermediate = 4096; c.do_stable_layer_norm = 1;
    c.num_conv_pos_embeddings = 128; c.num_conv_pos_embedding_groups = 16; c.layer_norm_eps = 1e-5f; c.vocab = 32;
    return c;
}

// the family that is built; names the first field outside it
int check_config(const DexAsrConfig& c) {
    if (c.feat_extract_norm_layer != 1) return create_fail("%s: only 'layer' is built", "feat_extract_norm");
    if (c.do_stable_layer_norm != 1) return create_fail("%s: only True is built", "do_stable_layer_norm");
    if (c.n_conv < 1 || c.n_conv > MAXC) return create_fail("%s: 1 .. 8 feature-extractor layers", "conv_dim");
    for (int l = 0; l < c.n_conv; ++l) {
        if (c.conv_dim[l] < 32 || c.conv_dim[l] % 32 || c.conv_dim[l] > 4096) return create_fail("%s: every width a multiple of 32 in 32 .. 4096", "conv_dim");
        if (c.conv_kernel[l] < 1 || c.conv_kernel[l] > 64) return create_fail("%s: 1 .. 64", "conv_kernel");
        if (c.conv_stride[l] < 1 || c.conv_stride[l] > 64) return create_fail("%s: 1 .. 64", "conv_stride");
    }
    if (c.conv_dim[0] > C0_MAX) return create_fail("%s: the first layer has at most 512 channels", "conv_dim");
    if (c.conv_kernel[0] > K0_MAX) return create_fail("%s: the first layer's kernel is at most 16", "conv_kernel");
    if (c.conv_stride[0] > S0_MAX) return create_fail("%s: the first layer's stride is at most 16", "conv_stride");
    if (c.n_heads < 1 || c.n_heads > 1024) return create_fail("%s: 1 .. 1024", "num_attention_heads");
    if (c.hidden < 64 || c.hidden > 16384 || c.hidden != 64 * c.n_heads) return create_fail("%s: hidden_size / num_attention_heads must be 64", "hidden_size");
    if (c.n_layers < 1 || c.n_layers > 256) return create_fail("%s: 1 .. 256", "num_hidden_layers");
    if (c.intermediate < 32 || c.intermediate % 32 || c.intermediate > 65536) return create_fail("%s: a multiple of 32 up to 65536", "intermediate_size");
    const int G = c.num_conv_pos_embedding_groups, K = c.num_conv_pos_embeddings;
    if (G < 1 || G > 16 || c.hidden % G || (c.hidden / G) % 32) return create_fail("%s: 1 .. 16 groups of a multiple of 32 channels", "num_conv_pos_embedding_groups");
    if (K < 2 || K % 2 || K > 1024) return create_fail("%s: even, 2 .. 1024", "num_conv_pos_embeddings");
    if (!(c.layer_norm_eps > 0.f) || !(c.layer_norm_eps < 1.f)) return create_fail("%s: in (0, 1)", "layer_norm_eps");
    if (c.vocab < 32 || c.vocab % 32 || c.vocab > 4096) return create_fail("%s: a multiple of 32 up to 4096", "vocab_size");
    return DEX_OK;
}

// the k-split of fc2: intermediate / hidden where that is 2, 4 or 8 (and the slices stay multiples of the GEMM's K tile), else none
int fc2_ksplit(const DexAsrConfig& c) {
    const int r = c.intermediate / c.hidden;
    return (r * c.hidden == c.intermediate && (r == 2 || r == 4 || r == 8) && (c.intermediate / r) % 32 == 0) ? r : 1;
}

int frames_of(const DexAsrConfig& c, long n, int upto) {
    for (int l = 0; l < upto; ++l) n = n >= c.conv_kernel[l] ? (n - c.conv_kernel[l]) / c.conv_stride[l] + 1 : 0;
    return (int)n;
}

}  // namespace

struct DexAsr : dex::WeightStore {
    DexAsr() : WeightStore("wav2vec2 ") {}
    DexAsrConfig c;
    const float* conv_w[MAXC] = {}; const float* conv_b[MAXC] = {}; const float* conv_g[MAXC] = {}; const float* conv_be[MAXC] = {};
    const float *fp_g = nullptr, *fp_be = nullptr, *fp_w = nullptr, *fp_b = nullptr, *pos_w = nullptr, *pos_b = nullptr;
    const float *enc_g = nullptr, *enc_be = nullptr, *lm_w = nullptr, *lm_b = nullptr;
    struct Layer { const float *ln1g, *ln1b, *wqkv, *bqkv, *wo, *bo, *ln2g, *ln2b, *w1, *b1, *w2, *b2; };
    std::vector<Layer> layers;
};

namespace {

const std::string FE = "wav2vec2.feature_extractor.conv_layers.", ENC = "wav2vec2.encoder.", FP = "wav2vec2.feature_projection.";
std::string lk(int l, const char* what) { return ENC + "layers." + std::to_string(l) + "." + what; }
std::string ck(int l, const char* what) { return FE + std::to_string(l) + "." + what; }

void register_keys(DexAsr* s) {
    const DexAsrConfig& c = s->c;
    for (int l = 0; l < c.n_conv; ++l) {
        s->add(ck(l, "conv.weight"), {c.conv_dim[l], l ? c.conv_dim[l - 1] : 1, c.conv_kernel[l]});
        if (c.conv_bias) s->add(ck(l, "conv.bias"), {c.conv_dim[l]});
        s->add(ck(l, "layer_norm.weight"), {c.conv_dim[l]});
        s->add(ck(l, "layer_norm.bias"), {c.conv_dim[l]});
    }
    const int C = c.conv_dim[c.n_conv - 1], H = c.hidden, I = c.intermediate;
    s->add(FP + "layer_norm.weight", {C}); s->add(FP + "layer_norm.bias", {C});
    s->add(FP + "projection.weight", {H, C}); s->add(FP + "projection.bias", {H});
    s->add(ENC + "pos_conv_embed.conv.bias", {H});
    s->add(ENC + "pos_conv_embed.conv.weight_g", {1, 1, c.num_conv_pos_embeddings});
    s->add(ENC + "pos_conv_embed.conv.weight_v", {H, H / c.num_conv_pos_embedding_groups, c.num_conv_pos_embeddings});
    s->add(ENC + "layer_norm.weight", {H}); s->add(ENC + "layer_norm.bias", {H});
    for (int l = 0; l < c.n_layers; ++l) {
        for (const char* pr : {"attention.q_proj", "attention.k_proj", "attention.v_proj", "attention.out_proj"}) {
            s->add(lk(l, pr) + ".weight", {H, H}); s->add(lk(l, pr) + ".bias", {H});
        }
        s->add(lk(l, "layer_norm.weight"), {H}); s->add(lk(l, "layer_norm.bias"), {H});
        s->add(lk(l, "feed_forward.intermediate_dense.weight"), {I, H}); s->add(lk(l, "feed_forward.intermediate_dense.bias"), {I});
        s->add(lk(l, "feed_forward.output_dense.weight"), {H, I}); s->add(lk(l, "feed_forward.output_dense.bias"), {H});
        s->add(lk(l, "final_layer_norm.weight"), {H}); s->add(lk(l, "final_layer_norm.bias"), {H});
    }
    s->add("lm_head.weight", {c.vocab, H}); s->add("lm_head.bias", {c.vocab});
}

int finalize(DexAsr* s, hipStream_t st) {
    if (int rc = s->begin_finalize()) return rc;
    const DexAsrConfig& c = s->c;
    const int H = c.hidden, I = c.intermediate, C = c.conv_dim[c.n_conv - 1];
    for (int l = 0; l < c.n_conv; ++l) {
        s->conv_w[l] = l ? pack(s, ck(l, "conv.weight"), 1, c.conv_dim[l], c.conv_dim[l - 1], c.conv_kernel[l], nullptr, st) : s->R(ck(0, "conv.weight"));
        s->conv_b[l] = c.conv_bias ? s->R(ck(l, "conv.bias")) : nullptr;
        s->conv_g[l] = s->R(ck(l, "layer_norm.weight")); s->conv_be[l] = s->R(ck(l, "layer_norm.bias"));
    }
    s->fp_g = s->R(FP + "layer_norm.weight"); s->fp_be = s->R(FP + "layer_norm.bias");
    s->fp_w = pack(s, FP + "projection.weight", 1, H, C, 1, nullptr, st); s->fp_b = s->R(FP + "projection.bias");
    {
        const int G = c.num_conv_pos_embedding_groups, K = c.num_conv_pos_embeddings;
        double* scale = (double*)s->alloc(2L * K);
        if (scale) {
            hipLaunchKernelGGL(asr_wn_scale_kernel, dim3(K), dim3(256), 0, st, s->R(ENC + "pos_conv_embed.conv.weight_v"),
                               s->R(ENC + "pos_conv_embed.conv.weight_g"), scale, (long)H * (H / G), K);
            s->pos_w = pack(s, ENC + "pos_conv_embed.conv.weight_v", G, H / G, H / G, K, scale, st);
        }
        s->pos_b = s->R(ENC + "pos_conv_embed.conv.bias");
    }
    s->enc_g = s->R(ENC + "layer_norm.weight"); s->enc_be = s->R(ENC + "layer_norm.bias");
    s->layers.assign(c.n_layers, DexAsr::Layer{});
    for (int l = 0; l < c.n_layers && s->alloc_rc == DEX_OK; ++l) {
        DexAsr::Layer& L = s->layers[l];
        float* wqkv = s->alloc(3L * H * H); float* bqkv = s->alloc(3L * H);
        if (!wqkv || !bqkv) break;
        const char* pr[3] = {"attention.q_proj", "attention.k_proj", "attention.v_proj"};
        for (int j = 0; j < 3; ++j) {
            pack_into(s->R(lk(l, pr[j]) + ".weight"), wqkv, 1, H, H, 1, 3 * H, j * H, nullptr, st);
            DEX_HIPCHK(s, hipMemcpyAsync(bqkv + (long)j * H, s->R(lk(l, pr[j]) + ".bias"), H * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
        L.wqkv = wqkv; L.bqkv = bqkv;
        L.wo = pack(s, lk(l, "attention.out_proj") + ".weight", 1, H, H, 1, nullptr, st); L.bo = s->R(lk(l, "attention.out_proj") + ".bias");
        L.ln1g = s->R(lk(l, "layer_norm.weight")); L.ln1b = s->R(lk(l, "layer_norm.bias"));
        L.w1 = pack(s, lk(l, "feed_forward.intermediate_dense.weight"), 1, I, H, 1, nullptr, st); L.b1 = s->R(lk(l, "feed_forward.intermediate_dense.bias"));
        L.w2 = pack(s, lk(l, "feed_forward.output_dense.weight"), 1, H, I, 1, nullptr, st); L.b2 = s->R(lk(l, "feed_forward.output_dense.bias"));
        L.ln2g = s->R(lk(l, "final_layer_norm.weight")); L.ln2b = s->R(lk(l, "final_layer_norm.bias"));
    }
    s->lm_w = pack(s, "lm_head.weight", 1, c.vocab, H, 1, nullptr, st); s->lm_b = s->R("lm_head.bias");
    if (s->alloc_rc != DEX_OK) return s->alloc_rc;
    if (hipGetLastError() != hipSuccess) return s->fail(DEX_ERR_HIP, "packing the wav2vec2 weights failed");
    s->finalized = true;
    return DEX_OK;
}

// workspace (floats, every piece a multiple of 64): xn [B][n] | fa [B][T_0][C_0] (even layers) | fb [B][T_1][C_1] (odd layers) |
// h, y [B][T][H] | qkv [B][T][3H] | ff [B][T][I] | part [ksplit][B][T][H] (fc2's slabs) | logits [B][T][V] | mask [B][T] | lens (int) [n_conv + 1][B]
struct Ws { float *xn, *fa, *fb, *h, *y, *qkv, *ff, *part, *logits, *mask; int* lens; size_t bytes; int Tl[MAXC]; int T; };
Ws plan(const DexAsrConfig& c, void* ws, long B, long n) {
    Ws w{};
    long fa = 0, fb = 0;
    for (int l = 0; l < c.n_conv; ++l) {
        w.Tl[l] = frames_of(c, n, l + 1);
        long& m = (l & 1) ? fb : fa;
        const long sz = (long)w.Tl[l] * c.conv_dim[l];
        m = sz > m ? sz : m;
    }
    w.T = w.Tl[c.n_conv - 1];
    const long T = w.T, H = c.hidden;
    // the LayerNorm of the feature projection writes the OTHER ping-pong buffer: both hold a [T][C_last] tensor
    const long last = T * c.conv_dim[c.n_conv - 1];
    fa = fa > last ? fa : last; fb = fb > last ? fb : last;
    float* f = (float*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    long off = 0;
    auto take = [&](long cnt) { float* p = f + off; off += up64(cnt); return p; };
    w.xn = take(B * n); w.fa = take(B * fa); w.fb = take(B * fb);
    w.h = take(B * T * H); w.y = take(B * T * H); w.qkv = take(B * T * 3 * H); w.ff = take(B * T * c.intermediate);
    w.part = take(fc2_ksplit(c) > 1 ? fc2_ksplit(c) * B * T * H : 0);
    w.logits = take(B * T * c.vocab); w.mask = take(B * T); w.lens = (int*)take((long)(c.n_conv + 1) * B);
    w.bytes = (size_t)off * sizeof(float) + 256;
    return w;
}

// the shared argument checks of the calls that take wavs; frames of the padded batch into *T
int check_wavs(DexAsr* s, const void* wav, const int32_t* lengths_host, int B, int n_samples, int* T) {
    if (!wav || !lengths_host) return s->fail(DEX_ERR_ARG, "null pointer argument");
    if (B < 1 || B > MAX_B) return s->fail(DEX_ERR_ARG, "B must lie in [1, %d]", MAX_B);
    if (n_samples < 1 || n_samples > MAX_SAMPLES) return s->fail(DEX_ERR_ARG, "n_samples must lie in [1, %d]", MAX_SAMPLES);
    for (int b = 0; b < B; ++b) {
        if (lengths_host[b] < 1 || lengths_host[b] > n_samples) return s->fail(DEX_ERR_ARG, "row lengths must lie in [1, n_samples]");
        if (frames_of(s->c, lengths_host[b], s->c.n_conv) < 1)
            return s->fail(DEX_ERR_ARG, "row %d has %d samples: too short for one frame of the feature extractor", b, lengths_host[b]);
    }
    if ((long)B * frames_of(s->c, n_samples, 1) > MAX_ROWS) return s->fail(DEX_ERR_ARG, "B x frames must not exceed %ld", MAX_ROWS);
    *T = frames_of(s->c, n_samples, s->c.n_conv);
    return DEX_OK;
}

int enqueue_network(DexAsr* s, const float* wav, const int32_t* lengths_host, int B, int n, float* logits, const Ws& w, hipStream_t st) {
    const DexAsrConfig& c = s->c;
    const int T = w.T, H = c.hidden, nc = c.n_conv;
    ConvSpec cs;
    std::memset(&cs, 0, sizeof cs);
    cs.n = nc;
    for (int l = 0; l < nc; ++l) { cs.k[l] = c.conv_kernel[l]; cs.s[l] = c.conv_stride[l]; }
    enqueue_plan(cs, lengths_host, B, T, w.lens, w.mask, st);
    enqueue_norm(wav, lengths_host, B, n, w.xn, st);
    // feature extractor: layer l lives in fa (l even) / fb (l odd)
    {
        const Conv0P p{w.xn, (long)n, s->conv_w[0], s->conv_b[0], s->conv_g[0], s->conv_be[0], c.layer_norm_eps, w.fa, w.Tl[0], c.conv_dim[0],
                       c.conv_kernel[0], c.conv_stride[0], w.lens + B};
        hipLaunchKernelGGL(asr_conv0_kernel, dim3((w.Tl[0] + F0 - 1) / F0, B), dim3(256), 0, st, p);
    }
    float* cur = w.fa;
    for (int l = 1; l < nc; ++l) {
        float* nxt = (l & 1) ? w.fb : w.fa;
        gemm(cur, c.conv_dim[l - 1], w.Tl[l - 1], c.conv_dim[l - 1], c.conv_kernel[l], c.conv_stride[l], 0, w.Tl[l], s->conv_w[l], c.conv_dim[l], 1,
             s->conv_b[l], nxt, 0, nullptr, nullptr, B, st);
        layer_norm<true>(nxt, nxt, (long)B * w.Tl[l], w.Tl[l], c.conv_dim[l], s->conv_g[l], s->conv_be[l], c.layer_norm_eps, w.lens + (long)(l + 1) * B, st);
        cur = nxt;
    }
    const long rows = (long)B * T;
    const int C = c.conv_dim[nc - 1];
    float* fpn = cur == w.fa ? w.fb : w.fa;
    layer_norm<false>(cur, fpn, rows, T, C, s->fp_g, s->fp_be, c.layer_norm_eps, nullptr, st);
    linear(fpn, C, s->fp_w, H, s->fp_b, w.y, 0, nullptr, w.mask, T, B, st);            // rows at or past the frame count: 0
    // h = y + GELU(pos_conv(y)) without its last frame
    {
        const int G = c.num_conv_pos_embedding_groups, K = c.num_conv_pos_embeddings;
        gemm(w.y, H, T, H / G, K, 1, -(K / 2), T, s->pos_w, H / G, G, s->pos_b, w.h, 1, w.y, nullptr, B, st);
    }
    const int* kv_len = w.lens + (long)nc * B;
    const int ks = fc2_ksplit(c);
    for (int l = 0; l < c.n_layers; ++l) {
        const DexAsr::Layer& L = s->layers[l];
        layer_norm<false>(w.h, w.y, rows, T, H, L.ln1g, L.ln1b, c.layer_norm_eps, nullptr, st);
        linear(w.y, H, L.wqkv, 3 * H, L.bqkv, w.qkv, 0, nullptr, nullptr, T, B, st);
        dex::AttnP a{};
        a.Q = w.qkv; a.ldq = 3 * H; a.qb = (long)T * 3 * H;
        a.K = w.qkv + H; a.ldk = 3 * H; a.kb = a.qb;
        a.V = w.qkv + 2 * H; a.ldv = 3 * H; a.vb = a.qb;
        a.O = w.y; a.ldo = H; a.ob = (long)T * H;
        a.Nq = T; a.Nk = T; a.kv_len = kv_len; a.kv_len_add = 0; a.heads = c.n_heads; a.scale = 0.125f; a.B = B; a.head_dim = 64;
        dex::launch_attention(a, dex::PREC_FP32, st);
        linear(w.y, H, L.wo, H, L.bo, w.h, 0, w.h, nullptr, T, B, st);                  // h += out_proj(attn)
        layer_norm<false>(w.h, w.y, rows, T, H, L.ln2g, L.ln2b, c.layer_norm_eps, nullptr, st);
        linear(w.y, H, L.w1, c.intermediate, L.b1, w.ff, 1, nullptr, nullptr, T, B, st);
        if (ks > 1) {                                                                   // h += fc2(GELU(fc1)), K in ks slabs
            gemm(w.ff, c.intermediate, T, c.intermediate, 1, 1, 0, T, L.w2, H, 1, nullptr, w.part, 0, nullptr, nullptr, B, st, ks);
            const long n4 = rows * H / 4;
            hipLaunchKernelGGL(asr_ksum_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, (const float4*)w.part, n4, ks, (const float4*)L.b2,
                               H / 4, (float4*)w.h);
        } else {
            linear(w.ff, c.intermediate, L.w2, H, L.b2, w.h, 0, w.h, nullptr, T, B, st);
        }
    }
    layer_norm<false>(w.h, w.y, rows, T, H, s->enc_g, s->enc_be, c.layer_norm_eps, nullptr, st);
    linear(w.y, H, s->lm_w, c.vocab, s->lm_b, logits, 0, nullptr, w.mask, T, B, st);
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

int enqueue_ctc(const float* logits, const int32_t* frames_host, const int* lengths_host, const DexAsrConfig* c, int B, int T, int V, int32_t* ids,
                int32_t* counts, hipStream_t st) {
    for (int r0 = 0; r0 < B; r0 += TAB) {
        Tab R;
        std::memset(&R, 0, sizeof R);
        R.n = B - r0 < TAB ? B - r0 : TAB;
        for (int e = 0; e < R.n; ++e) R.a[e] = frames_host ? frames_host[r0 + e] : frames_of(*c, lengths_host[r0 + e], c->n_conv);
        hipLaunchKernelGGL(asr_ctc_kernel, dim3(R.n), dim3(256), 0, st, logits, T, V, ids, counts, r0, R);
    }
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

}  // namespace

extern "C" {

int dex_asr_create(const DexAsrConfig* cfg, DexAsr** out) {
    if (!out) return DEX_ERR_ARG;
    *out = nullptr;
    const DexAsrConfig c = cfg ? *cfg : default_config();
    if (int rc = check_config(c)) return rc;
    DexAsr* s = new DexAsr();
    s->c = c;
    register_keys(s);
    *out = s;
    return DEX_OK;
}

void dex_asr_destroy(DexAsr* s) {
    if (!s) return;
    s->release();
    delete s;
}

const char* dex_asr_last_error(const DexAsr* s) { return s ? s->err.c_str() : g_create_err.c_str(); }

int dex_asr_load(DexAsr* s, const char* key, const float* w_dev, const int64_t* shape, int ndim, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!key || !w_dev || !shape) return s->fail(DEX_ERR_ARG, "null pointer argument");
    return s->load(key, w_dev, shape, ndim, (hipStream_t)stream, false);
}

int dex_asr_finalize(DexAsr* s, dex_stream_t stream) { return s ? finalize(s, (hipStream_t)stream) : DEX_ERR_ARG; }
int dex_asr_num_weights(const DexAsr* s) { return s ? (int)s->keys.size() : 0; }
int dex_asr_weight_info(const DexAsr* s, int i, const char** key, int64_t shape[4], int* ndim) { return s ? s->info(i, key, shape, ndim) : DEX_ERR_ARG; }

int dex_asr_num_frames(const DexAsrConfig* cfg, int n_samples) {
    const DexAsrConfig c = cfg ? *cfg : default_config();
    if (n_samples < 0 || c.n_conv < 1 || c.n_conv > MAXC) return DEX_ERR_ARG;
    for (int l = 0; l < c.n_conv; ++l)
        if (c.conv_kernel[l] < 1 || c.conv_stride[l] < 1) return DEX_ERR_ARG;
    return frames_of(c, n_samples, c.n_conv);
}

size_t dex_asr_workspace_bytes(const DexAsr* s, int B, int max_samples) {
    if (!s || B < 1 || B > MAX_B || max_samples < 1 || max_samples > MAX_SAMPLES) return 0;
    if (frames_of(s->c, max_samples, s->c.n_conv) < 1 || (long)B * frames_of(s->c, max_samples, 1) > MAX_ROWS) return 0;
    return plan(s->c, nullptr, B, max_samples).bytes;
}

int dex_asr_normalize(DexAsr* s, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, float* out_dev, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!wav_dev || !lengths_host || !out_dev) return s->fail(DEX_ERR_ARG, "null pointer argument");
    if (B < 1 || n_samples < 1 || n_samples > MAX_SAMPLES) return s->fail(DEX_ERR_ARG, "B must be >= 1 and n_samples lie in [1, %d]", MAX_SAMPLES);
    for (int b = 0; b < B; ++b)
        if (lengths_host[b] < 1 || lengths_host[b] > n_samples) return s->fail(DEX_ERR_ARG, "row lengths must lie in [1, n_samples]");
    enqueue_norm(wav_dev, lengths_host, B, n_samples, out_dev, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? DEX_OK : s->fail(DEX_ERR_HIP, "kernel launch failed");
}

int dex_asr_logits(DexAsr* s, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, float* logits_dev, void* workspace_dev,
                   size_t workspace_bytes, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    int T = 0;
    if (int rc = check_wavs(s, wav_dev, lengths_host, B, n_samples, &T)) return rc;
    if (!logits_dev || !workspace_dev) return s->fail(DEX_ERR_ARG, "null pointer argument");
    if (!s->finalized) return s->fail(DEX_ERR_STATE, "the wav2vec2 weights are not finalized (dex_asr_finalize)");
    const Ws w = plan(s->c, workspace_dev, B, n_samples);
    if (workspace_bytes < w.bytes) return s->fail(DEX_ERR_WORKSPACE, "workspace too small (dex_asr_workspace_bytes)");
    const int rc = enqueue_network(s, wav_dev, lengths_host, B, n_samples, logits_dev, w, (hipStream_t)stream);
    return rc ? s->fail(rc, "kernel launch failed") : DEX_OK;
}

int dex_asr_transcribe(DexAsr* s, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, int32_t* ids_dev, int32_t* counts_dev,
                       void* workspace_dev, size_t workspace_bytes, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    int T = 0;
    if (int rc = check_wavs(s, wav_dev, lengths_host, B, n_samples, &T)) return rc;
    if (!ids_dev || !counts_dev || !workspace_dev) return s->fail(DEX_ERR_ARG, "null pointer argument");
    if (!s->finalized) return s->fail(DEX_ERR_STATE, "the wav2vec2 weights are not finalized (dex_asr_finalize)");
    const Ws w = plan(s->c, workspace_dev, B, n_samples);
    if (workspace_bytes < w.bytes) return s->fail(DEX_ERR_WORKSPACE, "workspace too small (dex_asr_workspace_bytes)");
    int rc = enqueue_network(s, wav_dev, lengths_host, B, n_samples, w.logits, w, (hipStream_t)stream);
    if (rc == DEX_OK) rc = enqueue_ctc(w.logits, nullptr, lengths_host, &s->c, B, T, s->c.vocab, ids_dev, counts_dev, (hipStream_t)stream);
    return rc ? s->fail(rc, "kernel launch failed") : DEX_OK;
}

int dex_asr_ctc(DexAsr* s, const float* logits_dev, const int32_t* frames_host, int B, int T, int V, int32_t* ids_dev, int32_t* counts_dev,
                dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!logits_dev || !frames_host || !ids_dev || !counts_dev) return s->fail(DEX_ERR_ARG, "null pointer argument");
    if (B < 1 || T < 1 || V < 1) return s->fail(DEX_ERR_ARG, "B, T and V must be >= 1");
    if ((long)B * T > MAX_ROWS || V > 65536) return s->fail(DEX_ERR_ARG, "B x T must not exceed %ld and V 65536", MAX_ROWS);
    for (int b = 0; b < B; ++b)
        if (frames_host[b] < 0 || frames_host[b] > T) return s->fail(DEX_ERR_ARG, "frame counts must lie in [0, T]");
    const int rc = enqueue_ctc(logits_dev, frames_host, nullptr, nullptr, B, T, V, ids_dev, counts_dev, (hipStream_t)stream);
    return rc ? s->fail(rc, "kernel launch failed") : DEX_OK;
}

}  // extern "C"
