// wav_trunk.h — the host layer of the waveform networks (asr.hip: wav2vec 2.0 CTC; wavlm.hip: WavLM x-vector; ecapa.hip: WavLM-large
// + ECAPA-TDNN; mos.hip: UTMOS; whisper.hip: the Whisper encoder).  Four of them run the wav2vec-family trunk: a feature extractor
// of 1 x k convolutions, the feature projection, a grouped weight-normed positional convolution, and N encoder layers of
// qkv | out_proj | fc1 | fc2.  Here,
// once: the trunk's geometry (Trunk) with its defaults and refusals, the HF key inventory in registration order, the packed weights
// (TrunkWeights, pack_side, finalize_trunk), the shared prefix of the workspace (plan_trunk), the enqueue steps a network composes
// its forward pass from, the encoder layer in both norm orders (enqueue_layer) with the plain self-attention over a packed q | k | v
// (enqueue_self_attention), the argument checks of a call that takes wavs, and the entry points (Entry: the boilerplate, the
// host-only frame counts, and the skeleton of a network call).  What differs stays with the network: its first convolution and its
// norm (wav_layernorm.h, wav_groupnorm.h), which norm order it instantiates, an attention that is not the plain one (WavLM's gated
// bias, wav_gated_attn.h), and its head.  Whisper has no trunk: its encoder takes the layer (LayerDims, LayerWs,
// TrunkWeights::Layer, pack_side) and the handle's boilerplate.  The kernels are in wav_encoder.h; everything has internal linkage.
#pragma once
#include <vector>

#include "wav_encoder.h"

namespace dex {
namespace wavenc {
namespace {

constexpr int F0 = 8;                    // frames per workgroup of a first convolution
constexpr int K0_MAX = 16, S0_MAX = 16;  // its kernel and stride bounds (taps in registers, window in LDS)
constexpr int C0_MAX = 512;              // its channels: two per thread
constexpr int MAX_B = 1024;              // grid z = B x 16 groups stays inside 65535
constexpr long MAX_ROWS = 1L << 26;      // B x frames of the first layer: every grid inside 2^31, every element index inside 2^63

// ---- geometry
struct Trunk {
    int n_conv, conv_dim[MAXC], conv_kernel[MAXC], conv_stride[MAXC], conv_bias;
    int hidden, n_layers, n_heads, intermediate, pos_k, pos_groups;
    float layer_norm_eps;
};

template <class Cfg>
Trunk trunk_of(const Cfg& c) {
    Trunk t{};
    t.n_conv = c.n_conv;
    for (int l = 0; l < MAXC; ++l) { t.conv_dim[l] = c.conv_dim[l]; t.conv_kernel[l] = c.conv_kernel[l]; t.conv_stride[l] = c.conv_stride[l]; }
    t.conv_bias = c.conv_bias;
    t.hidden = c.hidden; t.n_layers = c.n_layers; t.n_heads = c.n_heads; t.intermediate = c.intermediate;
    t.pos_k = c.num_conv_pos_embeddings; t.pos_groups = c.num_conv_pos_embedding_groups;
    t.layer_norm_eps = c.layer_norm_eps;
    return t;
}

// what the default configs of the family agree on: the 7-layer feature extractor, the positional convolution, eps
template <class Cfg>
void default_trunk_geometry(Cfg& c) {
    const int k[7] = {10, 3, 3, 3, 3, 2, 2}, s[7] = {5, 2, 2, 2, 2, 2, 2};
    c.n_conv = 7;
    for (int i = 0; i < 7; ++i) { c.conv_dim[i] = 512; c.conv_kernel[i] = k[i]; c.conv_stride[i] = s[i]; }
    c.num_conv_pos_embeddings = 128; c.num_conv_pos_embedding_groups = 16; c.layer_norm_eps = 1e-5f;
}

thread_local std::string g_create_err;   // the refusal of the last *_create of this thread (there is no handle to hold it)

int create_fail(const char* fmt, const char* field) {
    char buf[256];
    snprintf(buf, sizeof buf, fmt, field);
    g_create_err = buf;
    return DEX_ERR_ARG;
}

// the trunks that are built; names the first field outside them.  group_mult: the channels of a positional-convolution group are a
// multiple of it (the GEMM's 32, or 4 where the network pads the groups)
int check_trunk(const Trunk& c, int group_mult) {
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
    const int G = c.pos_groups, K = c.pos_k;
    if (G < 1 || G > 16 || c.hidden % G || (c.hidden / G) % group_mult)
        return create_fail(("%s: 1 .. 16 groups of a multiple of " + std::to_string(group_mult) + " channels").c_str(), "num_conv_pos_embedding_groups");
    if (K < 2 || K % 2 || K > 1024) return create_fail("%s: even, 2 .. 1024", "num_conv_pos_embeddings");
    if (!(c.layer_norm_eps > 0.f) || !(c.layer_norm_eps < 1.f)) return create_fail("%s: in (0, 1)", "layer_norm_eps");
    return DEX_OK;
}

// kernels and strides a frame count can be chained over (the host-only entry points take configs that were never created)
bool conv_geometry_ok(const Trunk& c) {
    if (c.n_conv < 1 || c.n_conv > MAXC) return false;
    for (int l = 0; l < c.n_conv; ++l)
        if (c.conv_kernel[l] < 1 || c.conv_stride[l] < 1) return false;
    return true;
}

// the k-split of fc2: intermediate / hidden where that is 2, 4 or 8 (and the slices stay multiples of the GEMM's K tile), else none
int fc2_ksplit(const Trunk& c) {
    const int r = c.intermediate / c.hidden;
    return (r * c.hidden == c.intermediate && (r == 2 || r == 4 || r == 8) && (c.intermediate / r) % 32 == 0) ? r : 1;
}

// what an encoder layer reads of a geometry: the widths, the k-split of fc2 (1: one launch, no `part` buffer), the LayerNorms' eps
struct LayerDims { int hidden, heads, intermediate, ksplit; float eps; };
LayerDims layer_dims(const Trunk& c) { return {c.hidden, c.n_heads, c.intermediate, fc2_ksplit(c), c.layer_norm_eps}; }

// frames after the first `upto` convolutions of n samples
int frames_of(const Trunk& c, long n, int upto) {
    for (int l = 0; l < upto; ++l) n = n >= c.conv_kernel[l] ? (n - c.conv_kernel[l]) / c.conv_stride[l] + 1 : 0;
    return (int)n;
}

// the fewest samples the feature extractor makes `frames` (>= 1) frames of
long samples_for(const Trunk& c, long frames) {
    long n = frames;
    for (int l = c.n_conv - 1; l >= 0; --l) n = (n - 1) * c.conv_stride[l] + c.conv_kernel[l];
    return n;
}

ConvSpec conv_spec(const Trunk& c) {
    ConvSpec cs;
    std::memset(&cs, 0, sizeof cs);
    cs.n = c.n_conv;
    for (int l = 0; l < c.n_conv; ++l) { cs.k[l] = c.conv_kernel[l]; cs.s[l] = c.conv_stride[l]; }
    return cs;
}

// ---- the HF keys of the trunk under a model prefix ("wav2vec2." / "wavlm.")
struct TrunkKeys {
    explicit TrunkKeys(const std::string& p) : FE(p + "feature_extractor.conv_layers."), ENC(p + "encoder."), FP(p + "feature_projection.") {}
    const std::string FE, ENC, FP;
    std::string lk(int l, const char* what) const { return ENC + "layers." + std::to_string(l) + "." + what; }
    std::string ck(int l, const char* what) const { return FE + std::to_string(l) + "." + what; }
};

// The registration order is observable (weight_info(i), the wrappers' state_dict_shapes and their 'missing keys' texts).
// conv_norm_every: every feature-extractor layer has layer_norm keys (the layer-norm family), else layer 0 alone (the group norm);
// attn_extra(l) registers what a network keeps between the attention and the layer_norm keys of encoder layer l.
template <class Extra>
void register_trunk_keys(WeightStore* s, const TrunkKeys& k, const Trunk& c, bool conv_norm_every, Extra attn_extra) {
    for (int l = 0; l < c.n_conv; ++l) {
        s->add(k.ck(l, "conv.weight"), {c.conv_dim[l], l ? c.conv_dim[l - 1] : 1, c.conv_kernel[l]});
        if (c.conv_bias) s->add(k.ck(l, "conv.bias"), {c.conv_dim[l]});
        if (conv_norm_every || l == 0) { s->add(k.ck(l, "layer_norm.weight"), {c.conv_dim[l]}); s->add(k.ck(l, "layer_norm.bias"), {c.conv_dim[l]}); }
    }
    const int C = c.conv_dim[c.n_conv - 1], H = c.hidden, I = c.intermediate;
    s->add(k.FP + "layer_norm.weight", {C}); s->add(k.FP + "layer_norm.bias", {C});
    s->add(k.FP + "projection.weight", {H, C}); s->add(k.FP + "projection.bias", {H});
    s->add(k.ENC + "pos_conv_embed.conv.bias", {H});
    s->add(k.ENC + "pos_conv_embed.conv.weight_g", {1, 1, c.pos_k});
    s->add(k.ENC + "pos_conv_embed.conv.weight_v", {H, H / c.pos_groups, c.pos_k});
    s->add(k.ENC + "layer_norm.weight", {H}); s->add(k.ENC + "layer_norm.bias", {H});
    for (int l = 0; l < c.n_layers; ++l) {
        for (const char* pr : {"attention.q_proj", "attention.k_proj", "attention.v_proj", "attention.out_proj"}) {
            s->add(k.lk(l, pr) + ".weight", {H, H}); s->add(k.lk(l, pr) + ".bias", {H});
        }
        attn_extra(l);
        s->add(k.lk(l, "layer_norm.weight"), {H}); s->add(k.lk(l, "layer_norm.bias"), {H});
        s->add(k.lk(l, "feed_forward.intermediate_dense.weight"), {I, H}); s->add(k.lk(l, "feed_forward.intermediate_dense.bias"), {I});
        s->add(k.lk(l, "feed_forward.output_dense.weight"), {H, I}); s->add(k.lk(l, "feed_forward.output_dense.bias"), {H});
        s->add(k.lk(l, "final_layer_norm.weight"), {H}); s->add(k.lk(l, "final_layer_norm.bias"), {H});
    }
}

// ---- the trunk's operands as the launches take them
struct TrunkWeights {
    const float* conv_w[MAXC] = {}; const float* conv_b[MAXC] = {}; const float* conv_g[MAXC] = {}; const float* conv_be[MAXC] = {};
    const float *fp_g = nullptr, *fp_be = nullptr, *fp_w = nullptr, *fp_b = nullptr, *pos_w = nullptr, *pos_b = nullptr;
    const float *enc_g = nullptr, *enc_be = nullptr;
    // ln1 = the layer's layer_norm, ln2 = its final_layer_norm: before attention / the feed-forward (pre-norm) or after them (post-norm)
    struct Layer { const float *ln1g, *ln1b, *wqkv, *bqkv, *wo, *bo, *ln2g, *ln2b, *w1, *b1, *w2, *b2; };
    std::vector<Layer> layers;
};

// the [K = d][N = n d] operand of the n projections `p + name` side by side (q | k | v, k | v), and (bias) their biases in one
// vector with 0 where a projection has none.  Null where an alloc failed
const float* pack_side(WeightStore* s, const std::string& p, std::initializer_list<const char*> names, int d, hipStream_t st, const float** bias) {
    const int n = (int)names.size();
    float* w = s->alloc((long)n * d * d);
    float* b = bias ? s->alloc((long)n * d) : nullptr;
    if (!w || (bias && !b)) return nullptr;
    if (b) hipMemsetAsync(b, 0, (size_t)n * d * sizeof(float), st);
    int j = 0;
    for (const char* nm : names) {
        pack_into(s->R(p + nm + ".weight"), w, 1, d, d, 1, n * d, j * d, nullptr, st);
        if (b && s->raw.count(p + nm + ".bias")) hipMemcpyAsync(b + (long)j * d, s->R(p + nm + ".bias"), d * sizeof(float), hipMemcpyDeviceToDevice, st);
        ++j;
    }
    if (bias) *bias = b;
    return w;
}

// Every weight transposed to the GEMM's [K][N] operand, q | k | v as one; weight_norm(dim = 2) of the positional convolution folded
// as scale[tap] (fp64), which pack_pos(scale) turns into pos_w / pos_b in the network's own layout.  Norm parameters and biases are
// read where they were uploaded.
template <class PackPos>
int finalize_trunk(WeightStore* s, const TrunkKeys& k, const Trunk& c, bool conv_norm_every, TrunkWeights& W, PackPos pack_pos, hipStream_t st) {
    const int H = c.hidden, I = c.intermediate, C = c.conv_dim[c.n_conv - 1];
    for (int l = 0; l < c.n_conv; ++l) {
        W.conv_w[l] = l ? pack(s, k.ck(l, "conv.weight"), 1, c.conv_dim[l], c.conv_dim[l - 1], c.conv_kernel[l], nullptr, st) : s->R(k.ck(0, "conv.weight"));
        W.conv_b[l] = c.conv_bias ? s->R(k.ck(l, "conv.bias")) : nullptr;
        const bool norm = conv_norm_every || l == 0;
        W.conv_g[l] = norm ? s->R(k.ck(l, "layer_norm.weight")) : nullptr; W.conv_be[l] = norm ? s->R(k.ck(l, "layer_norm.bias")) : nullptr;
    }
    W.fp_g = s->R(k.FP + "layer_norm.weight"); W.fp_be = s->R(k.FP + "layer_norm.bias");
    W.fp_w = pack(s, k.FP + "projection.weight", 1, H, C, 1, nullptr, st); W.fp_b = s->R(k.FP + "projection.bias");
    {
        double* scale = (double*)s->alloc(2L * c.pos_k);
        if (scale)
            hipLaunchKernelGGL(asr_wn_scale_kernel, dim3(c.pos_k), dim3(256), 0, st, s->R(k.ENC + "pos_conv_embed.conv.weight_v"),
                               s->R(k.ENC + "pos_conv_embed.conv.weight_g"), scale, (long)H * (H / c.pos_groups), c.pos_k);
        pack_pos(scale);
    }
    W.enc_g = s->R(k.ENC + "layer_norm.weight"); W.enc_be = s->R(k.ENC + "layer_norm.bias");
    W.layers.assign(c.n_layers, TrunkWeights::Layer{});
    for (int l = 0; l < c.n_layers && s->alloc_rc == DEX_OK; ++l) {
        TrunkWeights::Layer& L = W.layers[l];
        L.wqkv = pack_side(s, k.lk(l, "attention."), {"q_proj", "k_proj", "v_proj"}, H, st, &L.bqkv);
        L.wo = pack(s, k.lk(l, "attention.out_proj") + ".weight", 1, H, H, 1, nullptr, st); L.bo = s->R(k.lk(l, "attention.out_proj") + ".bias");
        L.ln1g = s->R(k.lk(l, "layer_norm.weight")); L.ln1b = s->R(k.lk(l, "layer_norm.bias"));
        L.w1 = pack(s, k.lk(l, "feed_forward.intermediate_dense.weight"), 1, I, H, 1, nullptr, st); L.b1 = s->R(k.lk(l, "feed_forward.intermediate_dense.bias"));
        L.w2 = pack(s, k.lk(l, "feed_forward.output_dense.weight"), 1, H, I, 1, nullptr, st); L.b2 = s->R(k.lk(l, "feed_forward.output_dense.bias"));
        L.ln2g = s->R(k.lk(l, "final_layer_norm.weight")); L.ln2b = s->R(k.lk(l, "final_layer_norm.bias"));
    }
    return DEX_OK;
}

// ---- workspace.  Floats, every piece a multiple of 64.  The trunk's prefix: xn [B][n] | fa [B][T_0][C_0] (even layers) |
// fb [B][T_1][C_1] (odd layers) | h, y [B][T][H] | qkv [B][T][3H] | ff [B][T][I] | part [ksplit][B][T][H] (fc2's slabs); a network
// takes its own pieces after it, and mask [B][T] and lens (int) [n_conv + 1][B] among them.  LayerWs: what an encoder layer touches,
// with T the frames of a row (part may be null where fc2 is not split)
struct LayerWs { float *h, *y, *qkv, *ff, *part; int T; };
struct TrunkWs : LayerWs { float *xn, *fa, *fb, *mask; int* lens; int Tl[MAXC]; };

struct Taker {
    explicit Taker(void* ws) : f((float*)(((uintptr_t)ws + 255) & ~(uintptr_t)255)) {}
    float* f;
    long off = 0;
    float* take(long cnt) { float* p = f + off; off += up64(cnt); return p; }
    size_t bytes() const { return (size_t)off * sizeof(float) + 256; }
};

void plan_trunk(const Trunk& c, Taker& tk, long B, long n, TrunkWs& w) {
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
    w.xn = tk.take(B * n); w.fa = tk.take(B * fa); w.fb = tk.take(B * fb);
    w.h = tk.take(B * T * H); w.y = tk.take(B * T * H); w.qkv = tk.take(B * T * 3 * H); w.ff = tk.take(B * T * c.intermediate);
    w.part = tk.take(fc2_ksplit(c) > 1 ? fc2_ksplit(c) * B * T * H : 0);
}

// ---- the argument checks of a call that takes wavs; frames of the padded batch into *T.  The network's two rules: a row needs
// `need` samples (`why` ends the refusal), and one call takes at most max_frames frames (0: bounded by max_samples alone)
struct WavRule { long need; const char* why; int max_samples, max_frames; };

int check_wavs(WeightStore* s, const Trunk& c, const WavRule& r, const void* wav, const int32_t* lengths_host, int B, int n_samples, int* T) {
    if (!wav || !lengths_host) return s->fail(DEX_ERR_ARG, "null pointer argument");
    if (B < 1 || B > MAX_B) return s->fail(DEX_ERR_ARG, "B must lie in [1, %d]", MAX_B);
    if (r.max_samples && (n_samples < 1 || n_samples > r.max_samples)) return s->fail(DEX_ERR_ARG, "n_samples must lie in [1, %d]", r.max_samples);
    if (n_samples < 1) return s->fail(DEX_ERR_ARG, "n_samples must be >= 1");
    *T = frames_of(c, n_samples, c.n_conv);
    if (r.max_frames && *T > r.max_frames) return s->fail(DEX_ERR_ARG, "%d samples are %d frames: one call takes at most %d", n_samples, *T, r.max_frames);
    for (int b = 0; b < B; ++b) {
        if (lengths_host[b] < 1 || lengths_host[b] > n_samples) return s->fail(DEX_ERR_ARG, "row lengths must lie in [1, n_samples]");
        if (lengths_host[b] < r.need) return s->fail(DEX_ERR_ARG, "row %d has %d samples: %s", b, lengths_host[b], r.why);
    }
    if ((long)B * frames_of(c, n_samples, 1) > MAX_ROWS) return s->fail(DEX_ERR_ARG, "B x frames must not exceed %ld", MAX_ROWS);
    return DEX_OK;
}

// what the handle of a trunk network holds beside its config S::c.  prefix: of its C symbols ("dex_asr"); rule (with `why`, where
// the network composes that text) is set when the keys are registered
struct TrunkStore : WeightStore {
    TrunkStore(const char* noun, const char* prefix) : WeightStore(noun), prefix(prefix) {}
    const char* prefix;
    Trunk t;
    TrunkWeights w;
    std::string why;
    WavRule rule{};
};

// kernels and strides of a config as conv_geometry_ok sees them
template <class Cfg>
bool conv_ok(const Cfg& c) { return conv_geometry_ok(trunk_of(c)); }

inline int no_further_check() { return DEX_OK; }

// ---- the steps a network's forward pass is composed of
// the per-layer frame counts and the frame mask; normalize: the input normalisation into xn
void enqueue_front(const Trunk& c, const TrunkWs& w, const float* wav, const int32_t* lengths_host, int B, int n, bool normalize, hipStream_t st) {
    enqueue_plan(conv_spec(c), lengths_host, B, w.T, w.lens, w.mask, st);
    if (normalize) enqueue_norm(wav, lengths_host, B, n, w.xn, st);
}

// feature-extractor layers 1 ..: layer l lives in fa (l even) / fb (l odd), layer 0 is in fa.  act: the epilogue activation of the
// convolution (0 none, 1 GELU); LN_GELU: each is followed by its LayerNorm + GELU.  Returns the last layer's buffer
template <bool LN_GELU>
float* enqueue_conv_tail(const Trunk& c, const TrunkWeights& W, const TrunkWs& w, int B, int act, hipStream_t st) {
    float* cur = w.fa;
    for (int l = 1; l < c.n_conv; ++l) {
        float* nxt = (l & 1) ? w.fb : w.fa;
        gemm(cur, c.conv_dim[l - 1], w.Tl[l - 1], c.conv_dim[l - 1], c.conv_kernel[l], c.conv_stride[l], 0, w.Tl[l], W.conv_w[l], c.conv_dim[l], 1,
             W.conv_b[l], nxt, act, nullptr, nullptr, B, st);
        if constexpr (LN_GELU)
            layer_norm<true>(nxt, nxt, (long)B * w.Tl[l], w.Tl[l], c.conv_dim[l], W.conv_g[l], W.conv_be[l], c.layer_norm_eps, w.lens + (long)(l + 1) * B, st);
        cur = nxt;
    }
    return cur;
}

// y = projection(LayerNorm(cur)), rows at or past the frame count: 0.  The LayerNorm writes the ping-pong buffer cur is not
void enqueue_projection(const Trunk& c, const TrunkWeights& W, const TrunkWs& w, float* cur, int B, hipStream_t st) {
    const int C = c.conv_dim[c.n_conv - 1];
    float* fpn = cur == w.fa ? w.fb : w.fa;
    layer_norm<false>(cur, fpn, (long)B * w.T, w.T, C, W.fp_g, W.fp_be, c.layer_norm_eps, nullptr, st);
    linear(fpn, C, W.fp_w, c.hidden, W.fp_b, w.y, 0, nullptr, w.mask, w.T, B, st);
}

// ---- the encoder layer
// h += fc2(GELU(fc1(x))): fc2 in one launch, or its K in d.ksplit slabs that asr_ksum_kernel adds in slab order
void enqueue_ffn(const LayerDims& d, const TrunkWeights::Layer& L, const LayerWs& w, const float* x, int B, hipStream_t st) {
    const int T = w.T, H = d.hidden, I = d.intermediate;
    linear(x, H, L.w1, I, L.b1, w.ff, 1, nullptr, nullptr, T, B, st);
    if (d.ksplit > 1) {
        gemm(w.ff, I, T, I, 1, 1, 0, T, L.w2, H, 1, nullptr, w.part, 0, nullptr, nullptr, B, st, d.ksplit);
        const long n4 = (long)B * T * H / 4;
        hipLaunchKernelGGL(asr_ksum_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, (const float4*)w.part, n4, d.ksplit,
                           (const float4*)L.b2, H / 4, (float4*)w.h);
    } else {
        linear(w.ff, I, L.w2, H, L.b2, w.h, 0, w.h, nullptr, T, B, st);
    }
}

// out [B][T][H] = softmax((q / 8) k^T) v per head of 64 over the packed qkv [B][T][3 H] (attention.hip's generic fp32 kernel); the
// keys of row b end at kv_len[b] (null: all T)
void enqueue_self_attention(const float* qkv, float* out, int T, int H, int heads, const int* kv_len, int B, hipStream_t st) {
    dex::AttnP a{};
    a.Q = qkv; a.ldq = 3 * H; a.qb = (long)T * 3 * H;
    a.K = qkv + H; a.ldk = 3 * H; a.kb = a.qb;
    a.V = qkv + 2 * H; a.ldv = 3 * H; a.vb = a.qb;
    a.O = out; a.ldo = H; a.ob = (long)T * H;
    a.Nq = T; a.Nk = T; a.kv_len = kv_len; a.kv_len_add = 0; a.heads = heads; a.scale = 0.125f; a.B = B; a.head_dim = 64;
    dex::launch_attention(a, dex::PREC_FP32, st);
}

// One layer on h.  attn(qkv, out) enqueues the attention over the packed q | k | v; it may read h, which still holds the layer's input.
//   PRE_NORM:  y = LN1(h); qkv = y Wqkv; y = attn; h += y Wo; y = LN2(h); h += ffn(y)
//   post-norm: qkv = h Wqkv; y = attn; h += y Wo; h = LN1(h); h += ffn(h); h = LN2(h)
template <bool PRE_NORM, class Attn>
void enqueue_layer(const LayerDims& d, const TrunkWeights::Layer& L, const LayerWs& w, int B, Attn attn, hipStream_t st) {
    const int T = w.T, H = d.hidden;
    const long rows = (long)B * T;
    float* x = PRE_NORM ? w.y : w.h;                      // what the GEMMs read: the normed copy, or h normed in place
    if (PRE_NORM) layer_norm<false>(w.h, x, rows, T, H, L.ln1g, L.ln1b, d.eps, nullptr, st);
    linear(x, H, L.wqkv, 3 * H, L.bqkv, w.qkv, 0, nullptr, nullptr, T, B, st);
    attn(w.qkv, w.y);
    linear(w.y, H, L.wo, H, L.bo, w.h, 0, w.h, nullptr, T, B, st);
    layer_norm<false>(w.h, x, rows, T, H, PRE_NORM ? L.ln2g : L.ln1g, PRE_NORM ? L.ln2b : L.ln1b, d.eps, nullptr, st);
    enqueue_ffn(d, L, w, x, B, st);
    if (!PRE_NORM) layer_norm<false>(w.h, w.h, rows, T, H, L.ln2g, L.ln2b, d.eps, nullptr, st);
}
// the layer with the plain attention
template <bool PRE_NORM>
void enqueue_plain_layer(const LayerDims& d, const TrunkWeights::Layer& L, const LayerWs& w, const int* kv_len, int B, hipStream_t st) {
    enqueue_layer<PRE_NORM>(d, L, w, B, [&](const float* qkv, float* out) { enqueue_self_attention(qkv, out, w.T, d.hidden, d.heads, kv_len, B, st); }, st);
}

// ---- the entry points every handle of the family has: S derives from WeightStore and holds its config as S::c
template <class S>
struct Entry {
    typedef decltype(S::c) Cfg;
    static int create(const Cfg* cfg, S** out, Cfg (*default_config)(), int (*check_config)(const Cfg&), void (*register_keys)(S*)) {
        if (!out) return DEX_ERR_ARG;
        *out = nullptr;
        const Cfg c = cfg ? *cfg : default_config();
        if (int rc = check_config(c)) return rc;
        S* s = new S();
        s->c = c;
        register_keys(s);
        *out = s;
        return DEX_OK;
    }
    static void destroy(S* s) {
        if (!s) return;
        s->release();
        delete s;
    }
    static const char* last_error(const S* s) { return s ? s->err.c_str() : g_create_err.c_str(); }
    static int load(S* s, const char* key, const float* w_dev, const int64_t* shape, int ndim, dex_stream_t stream) {
        if (!s) return DEX_ERR_ARG;
        if (!key || !w_dev || !shape) return s->fail(DEX_ERR_ARG, "null pointer argument");
        return s->load(key, w_dev, shape, ndim, (hipStream_t)stream, false);
    }
    // begin_finalize, the network's packing, and what every finalize ends with
    static int finalize(S* s, dex_stream_t stream, int (*pack_all)(S*, hipStream_t), const char* failed) {
        if (!s) return DEX_ERR_ARG;
        if (int rc = s->begin_finalize()) return rc;
        if (int rc = pack_all(s, (hipStream_t)stream)) return rc;
        if (s->alloc_rc != DEX_OK) return s->alloc_rc;
        if (hipGetLastError() != hipSuccess) return s->fail(DEX_ERR_HIP, "%s", failed);
        s->finalized = true;
        return DEX_OK;
    }
    static int num_weights(const S* s) { return s ? (int)s->keys.size() : 0; }
    static int weight_info(const S* s, int i, const char** key, int64_t shape[4], int* ndim) { return s ? s->info(i, key, shape, ndim) : DEX_ERR_ARG; }

    // ---- for S a TrunkStore.  The host-only entry points take configs that were never created: ok is the network's own predicate
    // of a geometry it can chain frame counts over, need its fewest samples of a row
    static int num_frames(const Cfg* cfg, int n_samples, Cfg (*default_config)(), bool (*ok)(const Cfg&)) {
        const Cfg c = cfg ? *cfg : default_config();
        if (n_samples < 0 || !ok(c)) return DEX_ERR_ARG;
        const Trunk t = trunk_of(c);
        return frames_of(t, n_samples, t.n_conv);
    }
    static int min_samples(const Cfg* cfg, Cfg (*default_config)(), bool (*ok)(const Cfg&), long (*need)(const Cfg&)) {
        const Cfg c = cfg ? *cfg : default_config();
        if (!ok(c)) return DEX_ERR_ARG;
        const long n = need(c);
        return n > 0x7fffffffL ? DEX_ERR_ARG : (int)n;
    }
    // the bytes plan(s, nullptr, B, max_samples) lays out; 0 for a batch the handle's rule refuses
    template <class Plan>
    static size_t workspace_bytes(const S* s, int B, int max_samples, Plan plan) {
        if (!s || B < 1 || B > MAX_B || max_samples < s->rule.need || (s->rule.max_samples && max_samples > s->rule.max_samples)) return 0;
        const int T = frames_of(s->t, max_samples, s->t.n_conv);
        if ((s->rule.max_frames && T > s->rule.max_frames) || (long)B * frames_of(s->t, max_samples, 1) > MAX_ROWS) return 0;
        return plan(s, nullptr, B, max_samples).bytes;
    }
    // A network call that takes wavs.  The checks come in an order a caller can observe: the wavs under the handle's rule, the output
    // and workspace pointers (outputs_ok: none of the outputs asked for is null), more() (the network's further argument checks),
    // finalized, the workspace's size; then enqueue(w, T) with the planned workspace and the frames of the padded batch
    template <class Plan, class More, class Enqueue>
    static int call(S* s, const float* wav, const int32_t* lengths_host, int B, int n_samples, bool outputs_ok, void* ws, size_t ws_bytes, Plan plan,
                    More more, Enqueue enqueue) {
        int T = 0;
        if (int rc = check_wavs(s, s->t, s->rule, wav, lengths_host, B, n_samples, &T)) return rc;
        if (!outputs_ok || !ws) return s->fail(DEX_ERR_ARG, "null pointer argument");
        if (int rc = more()) return rc;
        if (!s->finalized) return s->fail(DEX_ERR_STATE, "the %sweights are not finalized (%s_finalize)", s->noun, s->prefix);
        const auto w = plan(s, ws, B, n_samples);
        if (ws_bytes < w.bytes) return s->fail(DEX_ERR_WORKSPACE, "workspace too small (%s_workspace_bytes)", s->prefix);
        const int rc = enqueue(w, T);
        return rc ? s->fail(rc, "kernel launch failed") : DEX_OK;
    }
};

}  // namespace
}  // namespace wavenc
}  // namespace dex
