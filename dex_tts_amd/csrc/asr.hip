// asr.hip — the reference's ASR score on the device (src/metric.py:21-67, Evaluater.transcribe / calculate_asr_score): the forward pass
// of HF's Wav2Vec2ForCTC in eval mode (facebook/wav2vec2-large-960h-lv60-self: layer-norm feature extractor, stable layer norm,
// head_dim 64) and greedy CTC.  fp32 throughout, channels-last [B][T][C].  C ABI dex_asr_*.
//
//   asr_norm_kernel      Wav2Vec2FeatureExtractor's do_normalize, one workgroup per utterance: mean and biased variance over the row's
//                        own length in fp64 (two passes, fixed-order trees), (x - mean) / sqrt(var + 1e-7) rounded to fp32 once, 0 past it.
//   asr_plan_kernel      the per-layer frame counts of every utterance (floor((L - k) / s) + 1 chained) and the encoder's frame mask,
//                        on the device: the lengths arrive as kernel arguments, nothing is copied from host memory.
//   asr_conv0_kernel     (wav_layernorm.h, shared with ecapa.hip) the first convolution (Cin = 1, k = 10, s = 5) with its LayerNorm and GELU: 8 frames x all channels per
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
// This file holds what is wav2vec 2.0's own: the CTC kernel, the checks of the layer-norm family and lm_head.
// What it shares with the other waveform networks (wavlm.hip, mos.hip, whisper.hip) is elsewhere: asr_norm /
// plan / ln / wn_scale / pack / ksum and the launch_igemm wrappers in wav_encoder.h; geometry, key inventory, packing, workspace
// prefix, the enqueue steps, the encoder layer (instantiated pre-norm here, with the plain attention) and the entry points with the
// skeleton of a call in wav_trunk.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "../../include/dex_amd.h"
#include "kernels.h"
#include "wav_layernorm.h"
#include "wav_trunk.h"
#include "weight_store.h"

using namespace dex::wavenc;

namespace {

static_assert(MAXC == DEX_ASR_MAX_CONV, "ConvSpec holds DEX_ASR_MAX_CONV layers");
constexpr int MAX_SAMPLES = 1 << 24;     // 17 minutes at 16 kHz

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

DexAsrConfig default_config() {
    DexAsrConfig c;
    std::memset(&c, 0, sizeof c);
    default_trunk_geometry(c);
    c.conv_bias = 1; c.feat_extract_norm_layer = 1;
    c.hidden = 1024; c.n_layers = 24; c.n_heads = 16; c.intermediate = 4096; c.do_stable_layer_norm = 1;
    c.vocab = 32;
    return c;
}

// the family that is built; names the first field outside it
int check_config(const DexAsrConfig& c) {
    if (c.feat_extract_norm_layer != 1) return create_fail("%s: only 'layer' is built", "feat_extract_norm");
    if (c.do_stable_layer_norm != 1) return create_fail("%s: only True is built", "do_stable_layer_norm");
    if (int rc = check_trunk(trunk_of(c), 32)) return rc;
    if (c.vocab < 32 || c.vocab % 32 || c.vocab > 4096) return create_fail("%s: a multiple of 32 up to 4096", "vocab_size");
    return DEX_OK;
}

const TrunkKeys KEYS("wav2vec2.");

}  // namespace

struct DexAsr : TrunkStore {
    DexAsr() : TrunkStore("wav2vec2 ", "dex_asr") {}
    DexAsrConfig c;
    const float *lm_w = nullptr, *lm_b = nullptr;
};

namespace {

void register_keys(DexAsr* s) {
    s->t = trunk_of(s->c);
    s->rule = WavRule{samples_for(s->t, 1), "too short for one frame of the feature extractor", MAX_SAMPLES, 0};      // a row needs one frame
    register_trunk_keys(s, KEYS, s->t, true, [](int) {});
    s->add("lm_head.weight", {s->c.vocab, s->c.hidden}); s->add("lm_head.bias", {s->c.vocab});
}

int pack_all(DexAsr* s, hipStream_t st) {
    const Trunk& t = s->t;
    auto pack_pos = [&](const double* scale) {
        const int G = t.pos_groups, cg = t.hidden / G;
        if (scale) s->w.pos_w = pack(s, KEYS.ENC + "pos_conv_embed.conv.weight_v", G, cg, cg, t.pos_k, scale, st);
        s->w.pos_b = s->R(KEYS.ENC + "pos_conv_embed.conv.bias");
    };
    if (int rc = finalize_trunk(s, KEYS, t, true, s->w, pack_pos, st)) return rc;
    s->lm_w = pack(s, "lm_head.weight", 1, s->c.vocab, t.hidden, 1, nullptr, st); s->lm_b = s->R("lm_head.bias");
    return DEX_OK;
}

// workspace: the trunk's prefix | logits [B][T][V] | mask [B][T] | lens (int) [n_conv + 1][B]
struct Ws : TrunkWs { float* logits; size_t bytes; };
Ws plan(const DexAsr* s, void* ws, long B, long n) {
    Ws w{};
    Taker tk(ws);
    plan_trunk(s->t, tk, B, n, w);
    w.logits = tk.take(B * w.T * s->c.vocab); w.mask = tk.take(B * w.T); w.lens = (int*)tk.take((long)(s->t.n_conv + 1) * B);
    w.bytes = tk.bytes();
    return w;
}

int enqueue_network(DexAsr* s, const float* wav, const int32_t* lengths_host, int B, int n, float* logits, const Ws& w, hipStream_t st) {
    const Trunk& c = s->t;
    const TrunkWeights& W = s->w;
    const int T = w.T, H = c.hidden;
    enqueue_front(c, w, wav, lengths_host, B, n, true, st);
    enqueue_conv0_layernorm(c, W, w, w.xn, B, n, st);
    enqueue_projection(c, W, w, enqueue_conv_tail<true>(c, W, w, B, 0, st), B, st);
    // h = y + GELU(pos_conv(y)) without its last frame
    gemm(w.y, H, T, H / c.pos_groups, c.pos_k, 1, -(c.pos_k / 2), T, W.pos_w, H / c.pos_groups, c.pos_groups, W.pos_b, w.h, 1, w.y, nullptr, B, st);
    const int* kv_len = w.lens + (long)c.n_conv * B;
    for (const TrunkWeights::Layer& L : W.layers) enqueue_plain_layer<true>(layer_dims(c), L, w, kv_len, B, st);      // pre-norm
    layer_norm<false>(w.h, w.y, (long)B * T, T, H, W.enc_g, W.enc_be, c.layer_norm_eps, nullptr, st);
    linear(w.y, H, s->lm_w, s->c.vocab, s->lm_b, logits, 0, nullptr, w.mask, T, B, st);
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

// frames_host, or (null) the frame counts of the lengths under trunk c
int enqueue_ctc(const float* logits, const int32_t* frames_host, const int* lengths_host, const Trunk* c, int B, int T, int V, int32_t* ids,
                int32_t* counts, hipStream_t st) {
    for_each_row_table<Tab>(B, [&](Tab& R, int e, int b) { R.a[e] = frames_host ? frames_host[b] : frames_of(*c, lengths_host[b], c->n_conv); },
                            [&](int r0, const Tab& R) { hipLaunchKernelGGL(asr_ctc_kernel, dim3(R.n), dim3(256), 0, st, logits, T, V, ids, counts, r0, R); });
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

typedef Entry<DexAsr> E;

}  // namespace

extern "C" {

int dex_asr_create(const DexAsrConfig* cfg, DexAsr** out) { return E::create(cfg, out, default_config, check_config, register_keys); }
void dex_asr_destroy(DexAsr* s) { E::destroy(s); }
const char* dex_asr_last_error(const DexAsr* s) { return E::last_error(s); }
int dex_asr_load(DexAsr* s, const char* key, const float* w_dev, const int64_t* shape, int ndim, dex_stream_t stream) {
    return E::load(s, key, w_dev, shape, ndim, stream);
}
int dex_asr_finalize(DexAsr* s, dex_stream_t stream) { return E::finalize(s, stream, pack_all, "packing the wav2vec2 weights failed"); }
int dex_asr_num_weights(const DexAsr* s) { return E::num_weights(s); }
int dex_asr_weight_info(const DexAsr* s, int i, const char** key, int64_t shape[4], int* ndim) { return E::weight_info(s, i, key, shape, ndim); }

int dex_asr_num_frames(const DexAsrConfig* cfg, int n_samples) { return E::num_frames(cfg, n_samples, default_config, conv_ok<DexAsrConfig>); }
size_t dex_asr_workspace_bytes(const DexAsr* s, int B, int max_samples) { return E::workspace_bytes(s, B, max_samples, plan); }

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
    return E::call(s, wav_dev, lengths_host, B, n_samples, logits_dev != nullptr, workspace_dev, workspace_bytes, plan, no_further_check,
                   [&](const Ws& w, int) { return enqueue_network(s, wav_dev, lengths_host, B, n_samples, logits_dev, w, (hipStream_t)stream); });
}

int dex_asr_transcribe(DexAsr* s, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, int32_t* ids_dev, int32_t* counts_dev,
                       void* workspace_dev, size_t workspace_bytes, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    return E::call(s, wav_dev, lengths_host, B, n_samples, ids_dev && counts_dev, workspace_dev, workspace_bytes, plan, no_further_check, [&](const Ws& w, int T) {
        const int rc = enqueue_network(s, wav_dev, lengths_host, B, n_samples, w.logits, w, (hipStream_t)stream);
        return rc ? rc : enqueue_ctc(w.logits, nullptr, lengths_host, &s->t, B, T, s->c.vocab, ids_dev, counts_dev, (hipStream_t)stream);
    });
}

int dex_asr_align(DexAsr* s, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, const int32_t* targets_host,
                  const int32_t* target_lengths_host, int Lmax, int32_t* states_dev, int32_t* spans_dev, double* token_scores_dev, double* score_dev,
                  double* nll_dev, void* ctc_workspace_dev, size_t ctc_workspace_bytes, void* workspace_dev, size_t workspace_bytes,
                  dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    int32_t frames[DEX_CTC_MAX_ROWS];
    const auto more = [&]() {
        if (!target_lengths_host || !ctc_workspace_dev || (Lmax > 0 && !targets_host)) return s->fail(DEX_ERR_ARG, "null pointer argument");
        const int T = frames_of(s->t, n_samples, s->t.n_conv);
        if (B > DEX_CTC_MAX_ROWS || T > DEX_CTC_MAX_FRAMES)
            return s->fail(DEX_ERR_ARG, "an alignment takes at most %d rows of %d frames", DEX_CTC_MAX_ROWS, DEX_CTC_MAX_FRAMES);
        for (int b = 0; b < B; ++b) frames[b] = frames_of(s->t, lengths_host[b], s->t.n_conv);
        const size_t need = dex_ctc_workspace_bytes(B, T, s->c.vocab, Lmax);
        if (need == 0) return s->fail(DEX_ERR_ARG, "Lmax must lie in [0, %d]", DEX_CTC_MAX_TARGET);
        if (ctc_workspace_bytes < need) return s->fail(DEX_ERR_WORKSPACE, "CTC workspace too small (dex_ctc_workspace_bytes)");
        for (int b = 0; b < B; ++b) {
            if (target_lengths_host[b] < 0 || target_lengths_host[b] > Lmax) return s->fail(DEX_ERR_ARG, "target lengths must lie in [0, Lmax]");
            for (int l = 0; l < target_lengths_host[b]; ++l) {
                const int v = targets_host[(long)b * Lmax + l];
                if (v < 1 || v >= s->c.vocab) return s->fail(DEX_ERR_ARG, "target ids must lie in [1, vocab): id 0 is the blank");
            }
        }
        return (int)DEX_OK;
    };
    return E::call(s, wav_dev, lengths_host, B, n_samples, states_dev && spans_dev && token_scores_dev && score_dev, workspace_dev, workspace_bytes, plan,
                   more, [&](const Ws& w, int T) {
        const int rc = enqueue_network(s, wav_dev, lengths_host, B, n_samples, w.logits, w, (hipStream_t)stream);
        return rc ? rc : dex_ctc_align(w.logits, frames, B, T, s->c.vocab, targets_host, target_lengths_host, Lmax, 0, states_dev, spans_dev,
                                       token_scores_dev, score_dev, nll_dev, ctc_workspace_dev, ctc_workspace_bytes, stream);
    });
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
