// dex_vocoder.hip — C ABI of the HiFi-GAN generator (include/dex_amd.h, dex_voc_*): GeDEX-TTS/hifigan/models.py:112-173.
//
//   x = conv_pre(mel)                                            Conv1d(80 -> C0, 7, pad 3)
//   per stage i:  x = ups[i](leaky_relu(x, 0.1))                 ConvTranspose1d(C -> C/2, k_i, stride u_i, pad (k_i-u_i)/2)
//                 x = (rb_0(x) + rb_1(x) + rb_2(x)) / 3          ResBlock(k_j, dilations d_j): 3 x [lrelu, conv(k,d), lrelu, conv(k,1), + x]
//   wav = tanh(conv_post(leaky_relu(x, 0.01)))                   Conv1d(C_last -> 1, 7, pad 3)
//
// Every Conv1d is an implicit GEMM over channels-last activations [B][L][C] (H = 1, KW = k, step_w = dilation) on the
// exact-fp32 MFMA kernel (igemm.hip), with the leaky_relu applied while the A tile is gathered and the residual added in
// the epilogue.  A ConvTranspose1d is one GEMM Y[l][j*Cout + co] = lrelu(x)[l][:] . w[:, co, j] followed by an overlap-add
// (k/u terms per output).  conv_post (one output channel) and the tanh are one element-wise kernel.
//
// BigVGAN (DEX-TTS/bigvgan/models.py:138-211; DexVocoderConfig::activation != 0) is the same network with AMPBlock1: the leaky_relu
// in front of every ResBlock conv and of conv_post becomes the anti-aliased Snake / SnakeBeta activation (alias_free_torch/act.py;
// one aa_snake launch into a scratch tensor), the transposed convs take x as it is.
//
// Narrow stages (vocoder_narrow.hip): a stage whose width is a multiple of 8, at most 64 and not a multiple of 32 (BigVGAN 22 kHz / 80
// bands: 48 and 24; HiFi-GAN V2: 16 and 8) runs its ResBlock convs and the transposed conv into it on direct exact-fp32 kernels, and
// its anti-aliased activations on the lane-packed aa_snake; those kernels stay fp32 in the bf16 / fp16 modes.  Every other width
// takes the implicit GEMM as before.
//
// Ragged batches (dex_vocode_ragged): utterance b of a batch ends at lengths[b] frames, i.e. at Lb = lengths[b] * R samples in a layer
// whose cumulative rate is R, and is vocoded as if it had been passed alone.  Every producer stores zeros at positions >= Lb - the
// implicit GEMMs through their output mask (one 0 / 1 row per rate, built on the device from the lengths), the element-wise and narrow
// kernels from the lengths themselves - so the next layer's taps read the zero padding the alone run sees (leaky_relu(0) = 0, the
// residual is zero there too); the anti-aliased activation also ends its two replicate paddings at Lb.  Same kernels, same per-element
// operation order as dex_vocode, which is this call without lengths.
#include <hip/hip_runtime.h>
#include <string>
#include <vector>

#include "../../include/dex_amd.h"
#include "kernels.h"
#include "weight_store.h"

using namespace dex;

namespace {
// (w.nk: the same matrix as bf16 [0] / fp16 [1], [N][K] with K contiguous - the reduced-precision GEMM's weight operand; the vocoder has no split-weight mode)
struct VConv { PackedW w; const float* b = nullptr; int cin, cout, k, dil; bool narrow = false; };  // packed [k*cin][cout]
struct VUp { PackedW w; const float* b = nullptr; int cin, cout, k, u, pad; bool narrow = false; };   // packed [cin][k*cout]
constexpr int MEL_LD = 96;          // num_mels padded to a multiple of 32 (K tiles of the implicit GEMM do not straddle taps)
}  // namespace

struct DexVoc : WeightStore {
    DexVoc() : WeightStore("vocoder ") {}
    DexVocoderConfig cfg{};
    int precision = DEX_PREC_FP32;      // DEX_PREC_BF16 / DEX_PREC_FP16: the convolutions' operands (fp32 accumulation, fp32 activations in HBM)
    VConv pre;
    std::vector<VUp> ups;
    std::vector<VConv> rb;              // [stage][j][c1_0, c2_0, c1_1, c2_1, c1_2, c2_2] flattened
    const float *post_w = nullptr, *post_b = nullptr;
    // BigVGAN: per activation layer (a, 1/b) coefficient pairs: [stage][block j][layer l] then the post activation; the shared filter
    std::vector<const float*> act_a, act_ib;
    const float* filt = nullptr;
    bool big() const { return cfg.activation != 0; }
};

namespace {
int stage_ch(const DexVocoderConfig& c, int i) { return c.upsample_initial_channel >> (i + 1); }
long total_up(const DexVocoderConfig& c) { long u = 1; for (int i = 0; i < c.n_upsamples; ++i) u *= c.upsample_rates[i]; return u; }
}  // namespace

extern "C" {

int dex_voc_create(const DexVocoderConfig* cfg, DexVoc** out) {
    if (!cfg || !out) return DEX_ERR_ARG;
    DexVoc* v = new DexVoc();
    v->cfg = *cfg;
    *out = v;
    const DexVocoderConfig& c = v->cfg;
    if (c.num_mels < 1 || c.num_mels > MEL_LD) return v->fail(DEX_ERR_ARG, "num_mels must be in [1, %d]", MEL_LD);
    if (c.n_upsamples < 1 || c.n_upsamples > 6) return v->fail(DEX_ERR_ARG, "n_upsamples must be in [1, 6]");
    if (c.n_resblock_kernels != 3) return v->fail(DEX_ERR_ARG, "three ResBlock kernel sizes are expected (hifigan/config.json)");
    if (c.upsample_initial_channel % 64) return v->fail(DEX_ERR_ARG, "upsample_initial_channel must be a multiple of 64");
    for (int i = 0; i < c.n_upsamples; ++i) {
        const int k = c.upsample_kernel_sizes[i], u = c.upsample_rates[i], co = stage_ch(c, i);
        if (u < 1 || k < u || (k - u) % 2) return v->fail(DEX_ERR_ARG, "upsample %d: kernel %d / rate %d unsupported (needs k >= u, k - u even)", i, k, u);
        if (voc_narrow_width(co)) continue;          // the narrow kernels take any k, u that passed above
        if (co % 32 || co < 32)
            return v->fail(DEX_ERR_ARG, "stage %d has %d channels: the implicit GEMM needs multiples of 32, the narrow kernels multiples of 8 up to 64", i, co);
        if ((k * co) % 64) return v->fail(DEX_ERR_ARG, "stage %d: k * channels must be a multiple of 64", i);
    }
    if (stage_ch(c, c.n_upsamples - 1) > 64) return v->fail(DEX_ERR_ARG, "conv_post kernel handles <= 64 input channels");
    for (int j = 0; j < 3; ++j) if (c.resblock_kernel_sizes[j] % 2 == 0) return v->fail(DEX_ERR_ARG, "ResBlock kernel sizes must be odd");
    if (c.activation < 0 || c.activation > 2) return v->fail(DEX_ERR_ARG, "activation must be 0 (HiFi-GAN), 1 (BigVGAN snake) or 2 (BigVGAN snakebeta)");
    const bool big = c.activation != 0, beta = c.activation == 2;
    const std::string upsfx = big ? ".0" : "";                      // BigVGAN nests each transposed conv in a ModuleList
    const int c0 = c.upsample_initial_channel;
    v->add("conv_pre.weight", {c0, c.num_mels, 7}); v->add("conv_pre.bias", {c0});
    for (int i = 0; i < c.n_upsamples; ++i) {
        const int ci = c0 >> i, co = c0 >> (i + 1);
        v->add("ups." + std::to_string(i) + upsfx + ".weight", {ci, co, c.upsample_kernel_sizes[i]});      // ConvTranspose1d: [in, out, k]
        v->add("ups." + std::to_string(i) + upsfx + ".bias", {co});
    }
    for (int i = 0; i < c.n_upsamples; ++i)
        for (int j = 0; j < 3; ++j) {
            const int ch = stage_ch(c, i), k = c.resblock_kernel_sizes[j];
            const std::string p = "resblocks." + std::to_string(i * 3 + j);
            for (const char* cs : {".convs1.", ".convs2."})
                for (int m = 0; m < 3; ++m) {
                    v->add(p + cs + std::to_string(m) + ".weight", {ch, ch, k});
                    v->add(p + cs + std::to_string(m) + ".bias", {ch});
                }
            if (big)
                for (int l = 0; l < 6; ++l) {
                    v->add(p + ".activations." + std::to_string(l) + ".act.alpha", {ch});
                    if (beta) v->add(p + ".activations." + std::to_string(l) + ".act.beta", {ch});
                }
        }
    if (big) {
        const int cl = stage_ch(c, c.n_upsamples - 1);
        v->add("activation_post.act.alpha", {cl});
        if (beta) v->add("activation_post.act.beta", {cl});
        v->add("activation_post.upsample.filter", {1, 1, 12}); v->add("activation_post.downsample.lowpass.filter", {1, 1, 12});
    }
    v->add("conv_post.weight", {1, stage_ch(c, c.n_upsamples - 1), 7}); v->add("conv_post.bias", {1});
    return DEX_OK;
}

void dex_voc_destroy(DexVoc* v) { if (v) { v->release(); delete v; } }
const char* dex_voc_last_error(const DexVoc* v) { return v ? v->err.c_str() : "null vocoder context"; }
int dex_voc_num_weights(const DexVoc* v) { return v ? (int)v->keys.size() : 0; }
int dex_voc_weight_info(const DexVoc* v, int i, const char** key, int64_t shape[4], int* ndim) { return v ? v->info(i, key, shape, ndim) : DEX_ERR_ARG; }
int dex_voc_load_weight_async(DexVoc* v, const char* key, const float* w_dev, const int64_t* shape, int ndim, dex_stream_t stream) {
    return v ? v->load(key, w_dev, shape, ndim, (hipStream_t)stream, false) : DEX_ERR_ARG;
}

int dex_voc_finalize(DexVoc* v, dex_stream_t stream) {
    if (!v) return DEX_ERR_ARG;
    if (int rc = v->begin_finalize()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const DexVocoderConfig& c = v->cfg;
    // reduced-precision copies of a packed fp32 [K][N] matrix: bf16 and fp16, [N][K]
    auto lp_copies = [&](PackedW& w, int K, int N) {
        for (int t = 0; t < 2; ++t) {
            void* d = v->alloc(((long)K * N + 1) / 2);
            if (d) launch_pack_lp_nk(w.f32, d, K, N, t ? DEX_PREC_FP16 : DEX_PREC_BF16, st);
            w.nk[t].p = d;
        }
    };
    // Conv1d [Cout][Cin][k] -> [(tap*Cin_pad + ci)][Cout]
    auto conv = [&](const std::string& name, int cin, int cout, int k, int dil, int cin_pad) {
        VConv o{}; o.cin = cin_pad; o.cout = cout; o.k = k; o.dil = dil; o.narrow = voc_narrow_width(cout);
        o.w = conv1d_operand(*v, v->R(name + ".weight"), cin, cout, k, cin_pad, st);
        o.b = v->R(name + ".bias");
        if (o.w && !o.narrow) lp_copies(o.w, k * cin_pad, cout);      // (the narrow kernels read fp32 weights in every mode)
        return o;
    };
    v->pre = conv("conv_pre", c.num_mels, c.upsample_initial_channel, 7, 1, MEL_LD);
    v->ups.clear(); v->rb.clear();
    for (int i = 0; i < c.n_upsamples; ++i) {
        const int ci = c.upsample_initial_channel >> i, co = stage_ch(c, i), k = c.upsample_kernel_sizes[i], u = c.upsample_rates[i];
        VUp up{}; up.cin = ci; up.cout = co; up.k = k; up.u = u; up.pad = (k - u) / 2; up.narrow = voc_narrow_width(co);
        float* d = v->alloc((long)ci * k * co);
        const std::string upn = "ups." + std::to_string(i) + (v->big() ? ".0" : "");
        if (d) launch_permute4(v->R(upn + ".weight"), d, ci, co, k, 1, 0, 2, 1, 3, st);   // [ci][co][k] -> [ci][k][co]
        up.w = d; up.b = v->R(upn + ".bias");
        if (d && !up.narrow) lp_copies(up.w, ci, k * co);
        v->ups.push_back(up);
        for (int j = 0; j < 3; ++j) {
            const std::string p = "resblocks." + std::to_string(i * 3 + j);
            for (int m = 0; m < 3; ++m) {
                v->rb.push_back(conv(p + ".convs1." + std::to_string(m), co, co, c.resblock_kernel_sizes[j], c.resblock_dilation_sizes[j][m], co));
                v->rb.push_back(conv(p + ".convs2." + std::to_string(m), co, co, c.resblock_kernel_sizes[j], 1, co));
            }
        }
    }
    v->act_a.clear(); v->act_ib.clear(); v->filt = nullptr;
    if (v->big()) {
        const bool beta = c.activation == 2;
        auto coeffs = [&](const std::string& p, int ch) {
            float* a = v->alloc(ch); float* ib = v->alloc(ch);
            if (a && ib) launch_snake_coeffs(v->R(p + ".alpha"), v->R(p + (beta ? ".beta" : ".alpha")), a, ib, ch, c.snake_logscale, st);
            v->act_a.push_back(a); v->act_ib.push_back(ib);
        };
        for (int i = 0; i < c.n_upsamples; ++i)
            for (int j = 0; j < 3; ++j)
                for (int l = 0; l < 6; ++l)
                    coeffs("resblocks." + std::to_string(i * 3 + j) + ".activations." + std::to_string(l) + ".act", stage_ch(c, i));
        coeffs("activation_post.act", stage_ch(c, c.n_upsamples - 1));
        v->filt = v->R("activation_post.upsample.filter");      // (the host checks that every resampling filter of the checkpoint equals it)
    }
    {   // conv_post [1][C][7] -> [tap][c]
        const int cl = stage_ch(c, c.n_upsamples - 1);
        float* d = v->alloc(7L * cl);
        if (d) launch_permute4(v->R("conv_post.weight"), d, 1, cl, 7, 1, 0, 2, 1, 3, st);
        v->post_w = d; v->post_b = v->R("conv_post.bias");
    }
    if (v->alloc_rc != DEX_OK) return v->alloc_rc;
    DEX_HIPCHK(v, hipStreamSynchronize(st));
    DEX_HIPCHK(v, hipGetLastError());
    v->finalized = true;
    return DEX_OK;
}

int dex_voc_samples(const DexVoc* v, int T) { return v ? (int)(T * total_up(v->cfg)) : 0; }

int dex_voc_set_precision(DexVoc* v, int precision) {
    if (!v) return DEX_ERR_ARG;
    if (precision != DEX_PREC_FP32 && precision != DEX_PREC_BF16 && precision != DEX_PREC_FP16) return v->fail(DEX_ERR_ARG, "unknown precision %d", precision);
    v->precision = precision;
    return DEX_OK;
}

}  // extern "C"

namespace {
struct VPlan { float *mel, *x, *y, *a, *q, *s, *p[3], *mask[7]; size_t bytes; };      // mask[i]: [B][T R_i], R_0 = 1 (conv_pre), R_i = rate of stage i - 1
void voc_plan(const DexVoc* v, int B, int T, bool ragged, void* ws, VPlan& P) {
    const DexVocoderConfig& c = v->cfg;
    // largest activation [B][L][C] and ConvTranspose GEMM output [B][L_in][k*Cout] over the stages
    size_t act = (size_t)B * T * c.upsample_initial_channel, ymax = 0;
    long L = T;
    for (int i = 0; i < c.n_upsamples; ++i) {
        if (!voc_narrow_width(stage_ch(c, i)))            // (the narrow transposed conv writes its stage input directly)
            ymax = std::max(ymax, (size_t)B * L * c.upsample_kernel_sizes[i] * stage_ch(c, i));
        L *= c.upsample_rates[i];
        act = std::max(act, (size_t)B * L * stage_ch(c, i));
    }
    char* base = (char*)ws; size_t off = 0;
    auto take = [&](size_t n) { off = (off + 255) & ~size_t(255); float* p = ws ? (float*)(base + off) : nullptr; off += n * sizeof(float); return p; };
    P.mel = take((size_t)B * T * MEL_LD);
    P.x = take(act); P.a = take(act); P.q = take(act);
    P.s = v->big() ? take(act) : nullptr;                 // output of the anti-aliased activation in front of a conv
    for (int j = 0; j < 3; ++j) P.p[j] = take(act);
    P.y = take(ymax);
    long R = 1;
    for (int i = 0; i <= 6; ++i) {                         // (behind everything else: the plain call's plan is a prefix of the ragged one)
        const bool used = ragged && i <= c.n_upsamples && (i == 0 || !voc_narrow_width(stage_ch(c, i - 1)));
        if (i > 0 && i <= c.n_upsamples) R *= c.upsample_rates[i - 1];
        P.mask[i] = used ? take((size_t)B * T * R) : nullptr;
    }
    P.bytes = (off + 255) & ~size_t(255);
}
// the weight operands of a GEMM in mode `prec`: the fp32 pack, and in the bf16 / fp16 modes its 16-bit copy
void voc_weight(IGemmP& g, const PackedW& w, int prec) {
    g.W = w.f32; g.Wbf = prec == DEX_PREC_BF16 ? w.nk[0].p : prec == DEX_PREC_FP16 ? w.nk[1].p : nullptr;
}
IGemmP conv1d(const float* X, int L, int B, const VConv& c, float slope, float* out, const float* res, int prec, const float* mask) {
    IGemmP g{};
    g.A = X; g.lda = c.cin; g.a_bstride = (long)L * c.cin; g.a_coff = 0;
    g.Hi = 1; g.Wi = L; g.Cin = c.cin;
    g.KH = 1; g.KW = c.k; g.sh = 1; g.sw = 1; g.off_h = 0; g.off_w = -c.dil * (c.k - 1) / 2; g.step_h = 1; g.step_w = c.dil;
    g.Ho = 1; g.Wo = L;
    voc_weight(g, c.w, prec); g.N = c.cout; g.K = c.k * c.cin; g.ksplit = 1; g.groups = 1;
    g.bias = c.b;
    g.C = out; g.ldc = c.cout; g.c_bstride = (long)L * c.cout; g.c_coff = 0;
    g.OHf = 1; g.OWf = L; g.osh = 1; g.osw = 1;
    g.inmask_ws = 1; g.outmask_ws = 1; g.gate_nstride = 1;
    g.outmask = mask; g.mask_bstride = L;               // ragged: zeros past the utterance's end (applied after bias and residual)
    g.act_in_slope = slope;
    g.res = res; g.ldres = c.cout; g.res_bstride = (long)L * c.cout;
    g.B = B;
    return g;
}
// a ragged batch's lengths at one layer: the device frame counts (null: full length), the layer's rate, its GEMM output mask
struct VLen { const int* len; int R; const float* mask; };
// one ResBlock conv: the implicit GEMM, or the direct kernel at a narrow width
void voc_conv(const float* X, int L, int B, const VConv& c, float slope, float* out, const float* res, int prec, const VLen& vl, hipStream_t st) {
    if (c.narrow) {
        NarrowConvP n{X, c.w.f32, c.b, res, out, L, c.cout, c.k, c.dil, B, slope, vl.len, vl.R};
        launch_narrow_conv1d(n, st);
    } else {
        launch_igemm(conv1d(X, L, B, c, slope, out, res, prec, vl.mask), prec, st);
    }
}
void voc_aa_snake(const AaSnakeP& s, hipStream_t st) {
    if (voc_narrow_width(s.C)) launch_aa_snake_narrow(s, st); else launch_aa_snake(s, st);
}
// the generator from conv_pre to the tanh on the channels-last mel in P.mel ([B][T][MEL_LD], zero past each utterance's length);
// wav [B][T * hop].  `len` null: the plain call.
void voc_layers(const DexVoc* v, const VPlan& P, int B, int T, const int* len, float* wav_dev, hipStream_t st) {
    const bool ragged = len != nullptr;
    const DexVocoderConfig& c = v->cfg;
    const int prec = v->precision;
    if (ragged) {          // the GEMMs' output masks, one per rate (the narrow stages read the lengths themselves)
        int R = 1;
        for (int i = 0; i <= c.n_upsamples; ++i) {
            if (i > 0) R *= c.upsample_rates[i - 1];
            if (P.mask[i]) launch_voc_len_mask(len, P.mask[i], B, T, R, st);
        }
    }
    launch_igemm(conv1d(P.mel, T, B, v->pre, 0.f, P.x, nullptr, prec, P.mask[0]), prec, st);       // conv_pre
    long L = T;
    int R = 1;               // cumulative rate: the layer holds L = T * R samples, utterance b's end at lengths[b] * R
    for (int i = 0; i < c.n_upsamples; ++i) {
        const VUp& up = v->ups[i];
        if (up.narrow) {     // ConvTranspose1d into a narrow stage: one direct kernel
            NarrowConvTP n{P.x, up.w.f32, up.b, P.a, (int)L, up.cin, up.cout, up.k, up.u, up.pad, B, v->big() ? 0.f : 0.1f, len, R};
            launch_narrow_convt(n, st);
        } else {   // ConvTranspose1d(leaky_relu(x, 0.1)): GEMM + overlap-add
            IGemmP g{};
            g.A = P.x; g.lda = up.cin; g.a_bstride = L * up.cin; g.Hi = 1; g.Wi = (int)L; g.Cin = up.cin;
            g.KH = 1; g.KW = 1; g.sh = 1; g.sw = 1; g.step_h = 1; g.step_w = 1; g.Ho = 1; g.Wo = (int)L;
            voc_weight(g, up.w, prec); g.N = up.k * up.cout; g.K = up.cin; g.ksplit = 1; g.groups = 1;
            g.C = P.y; g.ldc = g.N; g.c_bstride = L * g.N; g.OHf = 1; g.OWf = (int)L; g.osh = 1; g.osw = 1;
            g.inmask_ws = 1; g.outmask_ws = 1; g.gate_nstride = 1; g.act_in_slope = v->big() ? 0.f : 0.1f; g.B = B;     // BigVGAN: no activation here
            launch_igemm(g, prec, st);          // (ragged: x is zero past the utterance's end and the GEMM has no bias, so Y is zero there)
            ConvTFoldP f{P.y, up.b, P.a, (int)L, up.cout, up.k, up.u, up.pad, B, len, R};
            launch_convt_fold(f, st);
        }
        L *= up.u; R *= up.u;
        const VLen vl{len, R, P.mask[i + 1]};
        // three ResBlocks on the stage input P.a; block j's result ends in P.p[j]
        for (int j = 0; j < 3; ++j) {
            const VConv* cv = &v->rb[(size_t)(i * 3 + j) * 6];
            const float* cur = P.a;
            for (int m = 0; m < 3; ++m) {
                float* dst = (m == 1) ? P.q : P.p[j];                   // x -> p[j] -> q -> p[j]
                if (v->big()) {      // AMPBlock1 (bigvgan/models.py:76-85): xt = c1(a_{2m}(x)); x = c2(a_{2m+1}(xt)) + x
                    const size_t ai = ((size_t)(i * 3 + j) * 6) + 2 * m;
                    AaSnakeP s1{cur, P.s, (int)L, up.cout, B, v->act_a[ai], v->act_ib[ai], v->filt, len, R};
                    voc_aa_snake(s1, st);
                    voc_conv(P.s, (int)L, B, cv[2 * m], 0.f, P.x, nullptr, prec, vl, st);
                    AaSnakeP s2{P.x, P.s, (int)L, up.cout, B, v->act_a[ai + 1], v->act_ib[ai + 1], v->filt, len, R};
                    voc_aa_snake(s2, st);
                    voc_conv(P.s, (int)L, B, cv[2 * m + 1], 0.f, dst, cur, prec, vl, st);
                } else {
                    voc_conv(cur, (int)L, B, cv[2 * m], 0.1f, P.x, nullptr, prec, vl, st);          // xt = c1(lrelu(x))
                    voc_conv(P.x, (int)L, B, cv[2 * m + 1], 0.1f, dst, cur, prec, vl, st);          // x = c2(lrelu(xt)) + x
                }
                cur = dst;
            }
        }
        launch_avg3(P.p[0], P.p[1], P.p[2], P.x, (long)B * L * up.cout, st);
    }
    const float* xin = P.x;
    if (v->big()) {          // activation_post (models.py:205) replaces the leaky_relu in front of conv_post
        AaSnakeP sp{P.x, P.s, (int)L, stage_ch(c, c.n_upsamples - 1), B, v->act_a.back(), v->act_ib.back(), v->filt, len, R};
        voc_aa_snake(sp, st);
        xin = P.s;
    }
    ConvPostP cp{xin, v->post_w, v->post_b, wav_dev, (int)L, stage_ch(c, c.n_upsamples - 1), B, v->big() ? 1.f : 0.01f, len, R};
    launch_conv_post_tanh(cp, st);
}

long floor_div(long a, long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
long ceil_div(long a, long b) { return -floor_div(-a, b); }
// The receptive field in mel frames: the generator is walked from conv_post back to conv_pre with the radius (l, r), in
// samples of the current layer, of the inputs one output sample depends on.  A Conv1d(k, dilation d, same padding) adds d (k - 1) / 2 to
// both; a stage adds its widest ResBlock; ConvTranspose1d(k, u, p) maps outputs [n u + phi - l, n u + phi + r] of input sample n's u
// outputs to inputs [ceil((n u + phi - l + p - k + 1) / u), floor((n u + phi + r + p) / u)], worst at phi = 0 on the left and phi = u - 1
// on the right; the anti-aliased activation adds the reach of its up-sampler and low-pass, from the two filters' lengths.
int voc_halo(const DexVoc* v) {
    const DexVocoderConfig& c = v->cfg;
    long aa_l = 0, aa_r = 0;
    if (v->big()) {
        // y[t] = sum_k s[2 t + k - (Kd / 2 - 1)], k < Kd;  s[m] = 2 sum_j x[j - pad] f[m + pl - 2 j], 0 <= m + pl - 2 j < Ku
        const long Ku = v->raw.at("activation_post.upsample.filter").shape.back(), Kd = v->raw.at("activation_post.downsample.lowpass.filter").shape.back();
        const long pad = Ku / 2 - 1, pl = 2 * pad + (Ku - 2) / 2;
        aa_l = pad - ceil_div(-(Kd / 2 - 1) + pl - Ku + 1, 2);
        aa_r = floor_div(Kd / 2 + pl, 2) - pad;
    }
    long l = 3 + aa_l, r = 3 + aa_r;                      // conv_post: 7 taps behind leaky_relu / activation_post
    for (int i = c.n_upsamples - 1; i >= 0; --i) {
        long conv = 0;                                   // the widest ResBlock: three dilated and three plain convs
        for (int j = 0; j < 3; ++j) {
            long s = 0;
            for (int m = 0; m < 3; ++m) s += (long)(c.resblock_dilation_sizes[j][m] + 1) * (c.resblock_kernel_sizes[j] - 1) / 2;
            conv = std::max(conv, s);
        }
        l += conv + 6 * aa_l; r += conv + 6 * aa_r;
        const long k = c.upsample_kernel_sizes[i], u = c.upsample_rates[i], p = (k - u) / 2;
        l = floor_div(l + k - 1 - p, u);
        r = floor_div(r + p + u - 1, u);
    }
    return (int)(std::max(l, r) + 3);                    // conv_pre: 7 taps
}
// workspace of a window of W frames: the ragged plan of a [B, W] call, the window-local lengths, the window's waveform
struct VWin { VPlan P; int* len; float* wav; size_t bytes; };
void voc_window_plan(const DexVoc* v, int B, long W, void* ws, VWin& w) {
    voc_plan(v, B, (int)W, true, ws, w.P);
    size_t off = w.P.bytes;
    w.len = ws ? (int*)((char*)ws + off) : nullptr;
    off += ((size_t)B * sizeof(int) + 255) & ~size_t(255);
    w.wav = ws ? (float*)((char*)ws + off) : nullptr;
    off += ((size_t)B * W * total_up(v->cfg) * sizeof(float) + 255) & ~size_t(255);
    w.bytes = off;
}
}  // namespace

extern "C" {

size_t dex_voc_workspace_bytes(const DexVoc* v, int B, int T) {
    if (!v || B < 1 || T < 1) return 0;
    VPlan P; voc_plan(v, B, T, false, nullptr, P);
    return P.bytes;
}

size_t dex_voc_ragged_workspace_bytes(const DexVoc* v, int B, int T) {
    if (!v || B < 1 || T < 1) return 0;
    VPlan P; voc_plan(v, B, T, true, nullptr, P);
    return P.bytes;
}

int dex_vocode(DexVoc* v, const float* mel_dev, int B, int T, float* wav_dev, void* ws, size_t ws_bytes, dex_stream_t stream) {
    return dex_vocode_ragged(v, mel_dev, nullptr, B, T, wav_dev, ws, ws_bytes, stream);
}

int dex_vocode_ragged(DexVoc* v, const float* mel_dev, const int32_t* len, int B, int T, float* wav_dev, void* ws, size_t ws_bytes,
                      dex_stream_t stream) {
    if (!v || !mel_dev || !wav_dev || !ws) return DEX_ERR_ARG;
    if (!v->finalized) return v->fail(DEX_ERR_STATE, "dex_voc_finalize has not been called");
    if (B < 1 || T < 1) return v->fail(DEX_ERR_ARG, "B and T must be >= 1");
    if (((uintptr_t)ws & 255) != 0) return v->fail(DEX_ERR_ARG, "workspace must be 256-byte aligned");
    const bool ragged = len != nullptr;
    VPlan P; voc_plan(v, B, T, ragged, nullptr, P);
    if (P.bytes > ws_bytes) return v->fail(DEX_ERR_WORKSPACE, "vocoder workspace too small: need %zu bytes, got %zu", P.bytes, ws_bytes);
    voc_plan(v, B, T, ragged, ws, P);
    hipStream_t st = (hipStream_t)stream;
    launch_mel_to_cl(mel_dev, P.mel, B, v->cfg.num_mels, T, MEL_LD, st, len);
    voc_layers(v, P, B, T, len, wav_dev, st);
    DEX_HIPCHK(v, hipGetLastError());
    return DEX_OK;
}

int dex_voc_halo_frames(const DexVoc* v) { return v ? voc_halo(v) : 0; }

size_t dex_voc_window_workspace_bytes(const DexVoc* v, int B, int n_frames) {
    if (!v || B < 1 || n_frames < 1) return 0;
    VWin w; voc_window_plan(v, B, (long)n_frames + 2L * voc_halo(v), nullptr, w);
    return w.bytes;
}

int dex_vocode_window(DexVoc* v, const float* mel_dev, const int32_t* len, int B, int T, int t0, int n_frames, float* wav_dev,
                      int64_t wav_bstride, void* ws, size_t ws_bytes, dex_stream_t stream) {
    if (!v || !mel_dev || !wav_dev || !ws) return DEX_ERR_ARG;
    if (!v->finalized) return v->fail(DEX_ERR_STATE, "dex_voc_finalize has not been called");
    if (B < 1 || T < 1) return v->fail(DEX_ERR_ARG, "B and T must be >= 1");
    if (t0 < 0 || n_frames < 1 || (long)t0 + n_frames > T)
        return v->fail(DEX_ERR_ARG, "window [%d, %ld) is not inside the %d frames of the mel", t0, (long)t0 + n_frames, T);
    const long hop = total_up(v->cfg);
    if (wav_bstride < n_frames * hop) return v->fail(DEX_ERR_ARG, "wav_bstride %lld is less than the window's %ld samples", (long long)wav_bstride, n_frames * hop);
    if (((uintptr_t)ws & 255) != 0) return v->fail(DEX_ERR_ARG, "workspace must be 256-byte aligned");
    const size_t need = dex_voc_window_workspace_bytes(v, B, n_frames);
    if (need > ws_bytes) return v->fail(DEX_ERR_ARG, "vocoder window workspace too small: need %zu bytes, got %zu", need, ws_bytes);
    const int H = voc_halo(v);
    const int lo = std::max(0, t0 - H), hi = (int)std::min((long)T, (long)t0 + n_frames + H), W = hi - lo;       // W <= n_frames + 2 H
    VWin w; voc_window_plan(v, B, W, ws, w);
    hipStream_t st = (hipStream_t)stream;
    launch_voc_window_len(len, w.len, B, T, lo, W, st);
    launch_mel_window_to_cl(mel_dev, w.P.mel, B, v->cfg.num_mels, T, lo, W, MEL_LD, w.len, st);
    voc_layers(v, w.P, B, W, w.len, w.wav, st);       // always with lengths: the window's own ends are the true ends only at lo = 0 and hi = T
    launch_voc_window_crop(w.wav, W * hop, (t0 - lo) * hop, wav_dev, wav_bstride, n_frames * hop, B, st);
    DEX_HIPCHK(v, hipGetLastError());
    return DEX_OK;
}

}  // extern "C"
