// wavlm.hip — WavLM x-vector speaker similarity on the device: the embeddings of HF's WavLMForXVector in eval mode with no attention
// mask (microsoft/wavlm-base-plus-sv: group-norm feature extractor, post-layer-norm encoder, head_dim 64, gated relative-position
// bias, TDNN / statistics-pooling head).  fp32 throughout, channels-last [B][T][C].  C ABI dex_wavlm_*.  Row b of a batch is the
// network applied to row b alone at its own length.
//
// (the next four kernels and the padded positional convolution are in wav_groupnorm.h, shared with mos.hip)
//   wavlm_conv0_kernel     the first convolution (Cin = 1), raw: 8 frames x all channels per workgroup, the sample window in LDS.
//   wavlm_gn_part_kernel,  GroupNorm(C, C) of layer 0: per (row, channel) over the row's OWN frames, two passes - the sums of 512-frame
//   wavlm_gn_final_kernel, chunks in fp64, added in chunk order, first of x (mean), then of (x - mean)^2 (biased variance): a DC offset
//   wavlm_gn_apply_kernel  cancels nothing; then (x - mean) * rstd * gamma + beta -> GELU in place, 0 at or past the row's frames.
//   launch_igemm           (igemm.hip, exact-fp32 MFMA) the convolutions of layers 1 .. (GELU in the epilogue), the feature projection,
//                          the grouped positional convolution, q|k|v, out_proj, fc1, fc2 (k-split as in asr.hip), the projector, the
//                          TDNN layers (a dilated unpadded 1 x k convolution with ReLU) and the embedding Linear.  Groups of the
//                          positional convolution that are no multiple of 32 channels wide (768 / 16 = 48) are padded to 64.
// (the gate, rel, attention and mix kernels below are in wav_gated_attn.h, shared with ecapa.hip)
//   wavlm_gate_kernel      gate[b][h][t] = a (b const[h] - 1) + 2 with (a, b) = sigmoid of the two grouped sums of
//                          gru_rel_pos_linear(x[t][64 h .. 64 h + 64]) - the layer INPUT, one thread per (frame, head).
//   wavlm_rel_kernel       rel[h][d + N - 1] = rel_attn_embed[bucket(d)][h], d = -(N - 1) .. N - 1, once per call from the bucket table
//                          the host computed at finalize.
//   wavlm_attn_kernel      softmax((q / 8) k^T + gate[b][h][i] rel[h][j - i]) v on v_mfma_f32_32x32x2_f32 in the transposed flash
//                          formulation of attention.hip's generic kernel; the bias is formed in registers from the two tables - no
//                          [B H][N][N] tensor exists.
//   asr_ln_kernel          (wav_encoder.h) every LayerNorm; the post-norm order h = LN(h + attn(h)); h = LN(h + ffn(h)).
//   wavlm_mix_kernel       the softmax(layer_weights)-weighted sum of the hidden states, accumulated as the layers finish (one buffer).
//   wavlm_pool_kernel      statistics pooling: mean and unbiased deviation per channel over the row's own TDNN frames, two passes in
//                          fp64; a channel that is 0 on every frame has deviation exactly 0.
// This file holds what is the x-vector network's own: the gate + biased attention handed to the shared encoder layer in its post-norm
// order, where the layer mix happens, the pooling kernel and the x-vector head.  What it shares with the other waveform networks - geometry, key inventory, packing, workspace
// prefix, the enqueue steps, the layer, the entry points with the skeleton of a call - is wav_trunk.h; the group-norm front end it
// shares with mos.hip is wav_groupnorm.h, the gated attention and the layer mix it shares with ecapa.hip are wav_gated_attn.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dex_amd.h"
#include "kernels.h"
#include "wav_gated_attn.h"
#include "wav_groupnorm.h"
#include "wav_trunk.h"
#include "weight_store.h"

using namespace dex::wavenc;

namespace {

static_assert(MAXC == DEX_WAVLM_MAX_CONV, "ConvSpec holds DEX_WAVLM_MAX_CONV layers");
constexpr int MAXT = DEX_WAVLM_MAX_TDNN;
static_assert(MAXF == DEX_WAVLM_MAX_FRAMES, "the bucket table holds DEX_WAVLM_MAX_FRAMES frames");

constexpr int POOL_TL = 16;              // frame lanes of the pooling workgroup (x 64 channels)

// X [B][Tt][C] -> out [B][2 C]: mean | unbiased deviation per channel over the first len[b] - shrink frames (>= 2), two passes in fp64,
// the 16 frame lanes added in order.  grid (ceil(C / 64), B)
__global__ __launch_bounds__(POOL_TL * 64) void wavlm_pool_kernel(const float* X, int Tt, int C, const int* len, int shrink, float* out) {
    __shared__ double red[POOL_TL][64];
    const int cl = threadIdx.x & 63, ts = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl, b = blockIdx.y;
    const int n = min(len[b] - shrink, Tt);
    const float* x = X + (long)b * Tt * C + min(c, C - 1);
    double s = 0.0;
    for (int t = ts; t < n; t += POOL_TL) s += (double)x[(long)t * C];
    red[ts][cl] = s;
    __syncthreads();
    double tot = 0.0;
    for (int u = 0; u < POOL_TL; ++u) tot += red[u][cl];
    const double mean = tot / (double)n;
    __syncthreads();
    double q = 0.0;
    for (int t = ts; t < n; t += POOL_TL) { const double d = (double)x[(long)t * C] - mean; q = fma(d, d, q); }
    red[ts][cl] = q;
    __syncthreads();
    if (ts == 0 && c < C) {
        double qt = 0.0;
        for (int u = 0; u < POOL_TL; ++u) qt += red[u][cl];
        out[(long)b * 2 * C + c] = (float)mean;
        out[(long)b * 2 * C + C + c] = (float)sqrt(qt / (double)(n - 1));
    }
}

// Linear weight src [N][nseg seg] -> the GEMM operand dst [nseg segpad][Npad] (row = s segpad + c), zeros in the padding
__global__ __launch_bounds__(256) void wavlm_pack_pad_kernel(const float* src, float* dst, int N, int Npad, int seg, int segpad, int nseg) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)nseg * segpad * Npad) return;
    const int n = (int)(idx % Npad);
    const long kd = idx / Npad;
    const int sg = (int)(kd / segpad), c = (int)(kd - (long)sg * segpad);
    dst[idx] = (n < N && c < seg) ? src[(long)n * nseg * seg + (long)sg * seg + c] : 0.f;
}

DexWavlmConfig default_config() {
    DexWavlmConfig c;
    std::memset(&c, 0, sizeof c);
    default_trunk_geometry(c);
    c.conv_bias = 0; c.feat_extract_norm_group = 1;
    c.hidden = 768; c.n_layers = 12; c.n_heads = 12; c.intermediate = 3072; c.do_stable_layer_norm = 0;
    c.num_buckets = 320; c.max_bucket_distance = 800; c.use_weighted_layer_sum = 1;
    const int td[5] = {512, 512, 512, 512, 1500}, tk[5] = {5, 3, 3, 1, 1}, tl[5] = {1, 2, 3, 1, 1};
    c.n_tdnn = 5;
    for (int i = 0; i < 5; ++i) { c.tdnn_dim[i] = td[i]; c.tdnn_kernel[i] = tk[i]; c.tdnn_dilation[i] = tl[i]; }
    c.xvector_output_dim = 512;
    return c;
}

// the family that is built; names the first field outside it.  The positional groups are padded for the GEMM: any multiple of 4
int check_config(const DexWavlmConfig& c) {
    if (c.feat_extract_norm_group != 1) return create_fail("%s: only 'group' is built", "feat_extract_norm");
    if (c.do_stable_layer_norm != 0) return create_fail("%s: only False is built", "do_stable_layer_norm");
    if (int rc = check_trunk(trunk_of(c), 4)) return rc;
    if (c.num_buckets < 4 || c.num_buckets % 4 || c.num_buckets > 65536) return create_fail("%s: a multiple of 4 in 4 .. 65536", "num_buckets");
    if (c.max_bucket_distance <= c.num_buckets / 4 || c.max_bucket_distance > (1 << 24)) return create_fail("%s: above num_buckets / 4", "max_bucket_distance");
    if (c.n_tdnn < 1 || c.n_tdnn > MAXT) return create_fail("%s: 1 .. 8 TDNN layers", "tdnn_dim");
    for (int i = 0; i < c.n_tdnn; ++i) {
        if (c.tdnn_dim[i] < 1 || c.tdnn_dim[i] > 8192 || (i + 1 < c.n_tdnn && c.tdnn_dim[i] % 32))
            return create_fail("%s: every width but the last a multiple of 32, all in 1 .. 8192", "tdnn_dim");
        if (c.tdnn_kernel[i] < 1 || c.tdnn_kernel[i] > 16) return create_fail("%s: 1 .. 16", "tdnn_kernel");
        if (c.tdnn_dilation[i] < 1 || c.tdnn_dilation[i] > 16) return create_fail("%s: 1 .. 16", "tdnn_dilation");
    }
    if (c.xvector_output_dim < 32 || c.xvector_output_dim % 32 || c.xvector_output_dim > 8192) return create_fail("%s: a multiple of 32 up to 8192", "xvector_output_dim");
    return DEX_OK;
}

// the geometry alone (the host-only entry points take configs that were never created)
bool geometry_ok(const DexWavlmConfig& c) {
    if (!conv_geometry_ok(trunk_of(c)) || c.n_tdnn < 1 || c.n_tdnn > MAXT) return false;
    for (int i = 0; i < c.n_tdnn; ++i)
        if (c.tdnn_kernel[i] < 1 || c.tdnn_dilation[i] < 1) return false;
    return true;
}

// frames the TDNN layers take off a row
int tdnn_shrink(const DexWavlmConfig& c) {
    int s = 0;
    for (int i = 0; i < c.n_tdnn; ++i) s += (c.tdnn_kernel[i] - 1) * c.tdnn_dilation[i];
    return s;
}
// two frames after the TDNN layers: the unbiased deviation exists
long min_samples(const DexWavlmConfig& c) { return samples_for(trunk_of(c), tdnn_shrink(c) + 2); }
int bucket_of(const DexWavlmConfig& c, long d) { return dex::wavenc::bucket_of(c.num_buckets, c.max_bucket_distance, d); }
const TrunkKeys KEYS("wavlm.");
std::string tk(int i, const char* what) { return "tdnn." + std::to_string(i) + ".kernel." + what; }

}  // namespace

struct DexWavlm : TrunkStore {             // w.conv_g[0] / conv_be[0]: the group norm's affine; w.pos_w / pos_b: the padded groups
    DexWavlm() : TrunkStore("wavlm ", "dex_wavlm") {}
    DexWavlmConfig c;
    std::vector<GateW> gates;               // gru_rel_pos_linear and gru_rel_pos_const per encoder layer
    const float *rel_embed = nullptr, *lw = nullptr;
    const int* buckets = nullptr;
    std::vector<int32_t> buckets_host;
    const float *proj_w = nullptr, *proj_b = nullptr, *emb_w = nullptr, *emb_b = nullptr;
    const float* tdnn_w[MAXT] = {}; const float* tdnn_b[MAXT] = {};
};

namespace {

void register_keys(DexWavlm* s) {
    const DexWavlmConfig& c = s->c;
    s->t = trunk_of(c);
    s->why = "too short, statistics pooling needs two TDNN frames (" + std::to_string(min_samples(c)) + " samples)";
    s->rule = WavRule{min_samples(c), s->why.c_str(), 0, MAXF};
    register_trunk_keys(s, KEYS, s->t, false, [&](int l) {
        s->add(KEYS.lk(l, "attention.gru_rel_pos_const"), {1, c.n_heads, 1, 1});
        s->add(KEYS.lk(l, "attention.gru_rel_pos_linear.weight"), {8, 64}); s->add(KEYS.lk(l, "attention.gru_rel_pos_linear.bias"), {8});
        if (l == 0) s->add(KEYS.lk(0, "attention.rel_attn_embed.weight"), {c.num_buckets, c.n_heads});
    });
    if (c.use_weighted_layer_sum) s->add("layer_weights", {c.n_layers + 1});
    s->add("projector.weight", {c.tdnn_dim[0], c.hidden}); s->add("projector.bias", {c.tdnn_dim[0]});
    for (int i = 0; i < c.n_tdnn; ++i) {
        const int din = c.tdnn_dim[i ? i - 1 : 0];
        s->add(tk(i, "weight"), {c.tdnn_dim[i], din * c.tdnn_kernel[i]}); s->add(tk(i, "bias"), {c.tdnn_dim[i]});
    }
    s->add("feature_extractor.weight", {c.xvector_output_dim, 2 * c.tdnn_dim[c.n_tdnn - 1]}); s->add("feature_extractor.bias", {c.xvector_output_dim});
}

// Linear [N][nseg seg] -> operand [nseg segpad][Npad]
const float* pack_pad(DexWavlm* s, const std::string& key, int N, int Npad, int seg, int segpad, int nseg, hipStream_t st) {
    const long n = (long)nseg * segpad * Npad;
    float* d = s->alloc(n);
    if (d) hipLaunchKernelGGL(wavlm_pack_pad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s->R(key), d, N, Npad, seg, segpad, nseg);
    return d;
}

int pack_all(DexWavlm* s, hipStream_t st) {
    const DexWavlmConfig& c = s->c;
    const Trunk& t = s->t;
    auto pack_pos = [&](const double* scale) { pack_pos_padded(s, KEYS, t, s->w, scale, st); };
    if (int rc = finalize_trunk(s, KEYS, t, false, s->w, pack_pos, st)) return rc;
    s->rel_embed = s->R(KEYS.lk(0, "attention.rel_attn_embed.weight"));
    s->gates.clear();
    for (int l = 0; l < t.n_layers; ++l)
        s->gates.push_back({s->R(KEYS.lk(l, "attention.gru_rel_pos_linear.weight")), s->R(KEYS.lk(l, "attention.gru_rel_pos_linear.bias")),
                            s->R(KEYS.lk(l, "attention.gru_rel_pos_const"))});
    if (c.use_weighted_layer_sum) {
        float* lw = s->alloc(up64(c.n_layers + 1));
        if (lw) hipLaunchKernelGGL(wavlm_softmax_kernel, dim3(1), dim3(64), 0, st, s->R("layer_weights"), lw, c.n_layers + 1);
        s->lw = lw;
    } else {
        s->lw = nullptr;
    }
    {   // the bucket of every distance one call can meet, computed here on the host
        s->buckets_host.resize(2 * MAXF - 1);
        for (int d = -(MAXF - 1); d <= MAXF - 1; ++d) s->buckets_host[d + MAXF - 1] = bucket_of(c, d);
        int* bk = (int*)s->alloc(up64(2 * MAXF - 1));
        if (bk) DEX_HIPCHK(s, hipMemcpyAsync(bk, s->buckets_host.data(), (2 * MAXF - 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
        s->buckets = bk;
    }
    s->proj_w = pack_pad(s, "projector.weight", c.tdnn_dim[0], c.tdnn_dim[0], t.hidden, t.hidden, 1, st); s->proj_b = s->R("projector.bias");
    for (int i = 0; i < c.n_tdnn; ++i) {
        const int din = c.tdnn_dim[i ? i - 1 : 0], K = din * c.tdnn_kernel[i], N = c.tdnn_dim[i], Np = pad32(N);
        s->tdnn_w[i] = pack_pad(s, tk(i, "weight"), N, Np, K, K, 1, st);
        s->tdnn_b[i] = pad_vec(s, tk(i, "bias"), 1, N, Np, st);
    }
    {
        const int Cl = c.tdnn_dim[c.n_tdnn - 1];
        s->emb_w = pack_pad(s, "feature_extractor.weight", c.xvector_output_dim, c.xvector_output_dim, Cl, pad32(Cl), 2, st);
        s->emb_b = s->R("feature_extractor.bias");
    }
    return DEX_OK;
}

// workspace: the trunk's prefix | mix [B][T][H] | yp, pp [B][T][G cgp] (padded positional groups) | gate [B][heads][T] |
// rel [heads][2T - 1] | mask [B][T] | gnpart (fp64) [B][chunks][C_0] | gnmean (fp64) [B][C_0] | gnrstd [B][C_0] |
// ta, tb [B][T][max tdnn width] | stats [B][2 Cpad] | lens (int) [n_conv + 1][B]
struct Ws : TrunkWs, GnWs, PosWs { float *mix, *gate, *rel, *ta, *tb, *stats; size_t bytes; };
Ws plan(const DexWavlm* s, void* ws, long B, long n) {
    const DexWavlmConfig& c = s->c;
    Ws w{};
    Taker tk(ws);
    plan_trunk(s->t, tk, B, n, w);
    const long T = w.T, H = c.hidden;
    long tdw = 0;
    for (int i = 0; i < c.n_tdnn; ++i) tdw = pad32(c.tdnn_dim[i]) > tdw ? pad32(c.tdnn_dim[i]) : tdw;
    w.mix = tk.take(B * T * H);
    plan_pos_padded(s->t, tk, B, T, w);
    w.gate = tk.take(B * c.n_heads * T); w.rel = tk.take((long)c.n_heads * (2 * T - 1)); w.mask = tk.take(B * T);
    plan_groupnorm(tk, B, w.Tl[0], c.conv_dim[0], w);
    w.ta = tk.take(B * T * tdw); w.tb = tk.take(B * T * tdw); w.stats = tk.take(B * 2 * pad32(c.tdnn_dim[c.n_tdnn - 1]));
    w.lens = (int*)tk.take((long)(c.n_conv + 1) * B);
    w.bytes = tk.bytes();
    return w;
}

// everything up to the layer-mixed hidden states, stored at `hidden` [B][T][H] (0 past a row's frames)
int enqueue_encoder(DexWavlm* s, const float* wav, const int32_t* lengths_host, int B, int n, int do_normalize, float* hidden, const Ws& w, hipStream_t st) {
    const DexWavlmConfig& c = s->c;
    const Trunk& t = s->t;
    const TrunkWeights& W = s->w;
    const int T = w.T, H = c.hidden;
    enqueue_groupnorm_front(t, W, w, w, w, wav, lengths_host, B, n, do_normalize, st);
    const long rows = (long)B * T;
    const long n4 = rows * H / 4;
    const dim3 mg((unsigned)((n4 + 255) / 256));
    auto mix = [&](int l, bool last) {
        if (!c.use_weighted_layer_sum && !last) return;
        const bool first = l == 0 || !c.use_weighted_layer_sum;
        hipLaunchKernelGGL(wavlm_mix_kernel, mg, dim3(256), 0, st, (const float4*)w.h, (const float4*)w.mix, (float4*)(last ? hidden : w.mix), s->lw, l,
                           first ? 1 : 0, last ? w.mask : nullptr, n4, H / 4);
    };
    mix(0, false);
    hipLaunchKernelGGL(wavlm_rel_kernel, dim3((2 * T - 1 + 255) / 256, c.n_heads), dim3(256), 0, st, s->rel_embed, s->buckets, w.rel, T, c.n_heads);
    const int* kv_len = w.lens + (long)t.n_conv * B;
    for (int l = 0; l < c.n_layers; ++l) {
        const GateW& g = s->gates[l];
        enqueue_layer<false>(layer_dims(t), W.layers[l], w, B, [&](const float* qkv, float* out) {      // post-norm; the gate reads the layer's input
            enqueue_gated_attention(w.h, g, qkv, out, w.gate, w.rel, kv_len, B, T, c.n_heads, st);
        }, st);
        mix(l + 1, l + 1 == c.n_layers);
    }
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

// projector, TDNN layers, statistics pooling, the embedding Linear: hidden [B][T][H] -> embed [B][xvector_output_dim]
int enqueue_head(DexWavlm* s, const float* hidden, int B, float* embed, const Ws& w, hipStream_t st) {
    const DexWavlmConfig& c = s->c;
    const int T = w.T, H = c.hidden;
    linear(hidden, H, s->proj_w, c.tdnn_dim[0], s->proj_b, w.ta, 0, nullptr, nullptr, T, B, st);
    float* cur = w.ta;
    int Ti = T, din = c.tdnn_dim[0];
    for (int i = 0; i < c.n_tdnn; ++i) {
        float* nxt = cur == w.ta ? w.tb : w.ta;
        const int k = c.tdnn_kernel[i], dil = c.tdnn_dilation[i], To = Ti - (k - 1) * dil, Np = pad32(c.tdnn_dim[i]);
        gemm(cur, din, Ti, din, k, 1, 0, To, s->tdnn_w[i], Np, 1, s->tdnn_b[i], nxt, 2, nullptr, nullptr, B, st, 1, dil);
        cur = nxt; Ti = To; din = Np;
    }
    hipLaunchKernelGGL(wavlm_pool_kernel, dim3((din + 63) / 64, B), dim3(POOL_TL * 64), 0, st, cur, Ti, din, w.lens + (long)c.n_conv * B, tdnn_shrink(c),
                       w.stats);
    linear(w.stats, 2 * din, s->emb_w, c.xvector_output_dim, s->emb_b, embed, 0, nullptr, nullptr, B, 1, st);
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

typedef Entry<DexWavlm> E;

int run(DexWavlm* s, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, int do_normalize, float* hidden_dev, float* embed_dev,
        void* workspace_dev, size_t workspace_bytes, hipStream_t st) {
    return E::call(s, wav_dev, lengths_host, B, n_samples, hidden_dev || embed_dev, workspace_dev, workspace_bytes, plan, no_further_check,
                   [&](const Ws& w, int) {
        float* hidden = hidden_dev ? hidden_dev : w.mix;
        const int rc = enqueue_encoder(s, wav_dev, lengths_host, B, n_samples, do_normalize, hidden, w, st);
        return rc == DEX_OK && embed_dev ? enqueue_head(s, hidden, B, embed_dev, w, st) : rc;
    });
}

}  // namespace

extern "C" {

int dex_wavlm_create(const DexWavlmConfig* cfg, DexWavlm** out) { return E::create(cfg, out, default_config, check_config, register_keys); }
void dex_wavlm_destroy(DexWavlm* s) { E::destroy(s); }
const char* dex_wavlm_last_error(const DexWavlm* s) { return E::last_error(s); }
int dex_wavlm_load(DexWavlm* s, const char* key, const float* w_dev, const int64_t* shape, int ndim, dex_stream_t stream) {
    return E::load(s, key, w_dev, shape, ndim, stream);
}
int dex_wavlm_finalize(DexWavlm* s, dex_stream_t stream) { return E::finalize(s, stream, pack_all, "packing the wavlm weights failed"); }
int dex_wavlm_num_weights(const DexWavlm* s) { return E::num_weights(s); }
int dex_wavlm_weight_info(const DexWavlm* s, int i, const char** key, int64_t shape[4], int* ndim) { return E::weight_info(s, i, key, shape, ndim); }

int dex_wavlm_num_frames(const DexWavlmConfig* cfg, int n_samples) { return E::num_frames(cfg, n_samples, default_config, geometry_ok); }
int dex_wavlm_min_samples(const DexWavlmConfig* cfg) { return E::min_samples(cfg, default_config, geometry_ok, min_samples); }

int dex_wavlm_rel_buckets(const DexWavlmConfig* cfg, int n, int32_t* out) {
    const DexWavlmConfig c = cfg ? *cfg : default_config();
    if (!out || n < 1 || n > (1 << 24) || c.num_buckets < 4 || c.num_buckets % 4 || c.max_bucket_distance <= c.num_buckets / 4) return DEX_ERR_ARG;
    for (int d = -(n - 1); d <= n - 1; ++d) out[d + n - 1] = bucket_of(c, d);
    return DEX_OK;
}

size_t dex_wavlm_workspace_bytes(const DexWavlm* s, int B, int max_samples) { return E::workspace_bytes(s, B, max_samples, plan); }

int dex_wavlm_hidden(DexWavlm* s, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, int do_normalize, float* hidden_dev,
                     void* workspace_dev, size_t workspace_bytes, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!hidden_dev) return s->fail(DEX_ERR_ARG, "null pointer argument");
    return run(s, wav_dev, lengths_host, B, n_samples, do_normalize, hidden_dev, nullptr, workspace_dev, workspace_bytes, (hipStream_t)stream);
}

int dex_wavlm_embed(DexWavlm* s, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, int do_normalize, float* embed_dev,
                    void* workspace_dev, size_t workspace_bytes, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!embed_dev) return s->fail(DEX_ERR_ARG, "null pointer argument");
    return run(s, wav_dev, lengths_host, B, n_samples, do_normalize, nullptr, embed_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
