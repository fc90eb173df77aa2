// mos.hip — the UTMOS naturalness score (MOS prediction) on the device: the UTMOS22 "strong learner" in eval mode as its public demo
// scores a wav - the wav2vec 2.0 base trunk (group-norm feature extractor, post-layer-norm encoder, head_dim 64, plain softmax
// attention; last_hidden_state), every frame conditioned on a domain and a listener embedding, a bidirectional single-layer LSTM,
// Linear - ReLU - Linear per frame, mean over the frames x 2 + 3.  fp32 throughout, channels-last [B][T][C].  C ABI dex_mos_*.
// Row b of a batch is the network applied to row b alone at its own length.
//
//   the trunk              composed from wav_groupnorm.h / wav_trunk.h: the group-norm front end (enqueue_groupnorm_front), then the
//                          shared encoder layer in its post-norm order, h = LN(h + attn(h)); h = LN(h + ffn(h)), with the plain
//                          attention (dex::launch_attention, PREC_FP32, keys ending at the row's frames).
//   mos_cond_kernel        the embeddings are constant over time, so [T][hidden + domain_dim + judge_dim] is never built: once per call
//                          cbias[b][2 x 4H] = ((b_ih + b_hh) + dom[domain_b] . W_ih[:, hidden : hidden + dd]^T) + judge[judge_b] . W_ih[:, hidden + dd :]^T,
//                          two fmaf chains, k ascending.
//   input projections      hidden [B T][hidden] x W_ih[:, : hidden]^T of BOTH directions and all steps as one exact-fp32 implicit GEMM
//                          (N = 2 x 4H), cbias as its per-row bias.
//   mos_lstm_kernel        the recurrence.  One workgroup owns one direction and ROWS = 4 rows for all steps and never waits for another.
//                          h stays in LDS, c in registers.  Thread n owns gate columns n and n + 1024 of the 4H (H = 512: 2048 columns, two
//                          per thread of a 1024-thread workgroup): per step it streams its columns of W_hh (packed [k / 4][4H][4]: one
//                          16-byte load per lane per column per 4 k, a wave's load is 1 KB contiguous) and runs fixed-order fmaf chains,
//                          k ascending, seeded with the input projection.  The columns meet in LDS once per step; thread n then owns
//                          the (row, unit) pairs n and n + 1024 of the 4 x H for the gate update.  The forward direction walks t = 0 ..
//                          L - 1, the reverse t = L - 1 .. 0 with L the row's OWN frame count (pack_padded_sequence).  W_hh of one
//                          direction at H = 512 is 4 MiB, an XCD's whole L2: every step streams it once per workgroup, whatever the
//                          rows in it, so the workgroups of one direction are dealt to the same four XCDs (for speed only), and a
//                          group with fewer than ROWS live rows (the last of a batch; B = 1) runs a body without the dead ones.
//   the projection         two launches of the implicit GEMM (ReLU in the epilogue of the first; the second's single column padded to 32).
//   mos_mean_kernel        frames[b][t] = the score of frame t (0 past the row's frames); score[b] = mean x 2 + 3, the sum in fp64 in a
//                          fixed order (256 strided partials, an LDS tree).
// This file holds what is UTMOS's own: the head and its kernels.  Geometry, keys, packing, workspace prefix, the layer and the
// entry points with the skeleton of a call are wav_trunk.h's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dex_amd.h"
#include "kernels.h"
#include "wav_groupnorm.h"
#include "wav_trunk.h"
#include "weight_store.h"

using namespace dex::wavenc;

namespace {

static_assert(MAXC == DEX_MOS_MAX_CONV, "ConvSpec holds DEX_MOS_MAX_CONV layers");
constexpr int MAXF = DEX_MOS_MAX_FRAMES;
constexpr int MAXH = DEX_MOS_MAX_LSTM;
constexpr int ROWS = 4;                  // rows per workgroup of the recurrence
constexpr int LSTM_T = 1024;             // its threads (fewer where 4H is smaller)
constexpr int OUT_LD = 32;               // the last Linear's single column as the GEMM takes it

struct RowTab { int n; int dom[TAB], judge[TAB], frames[TAB]; };

// rows r0 .. r0 + n: cbias[b][col] = (bias[col] + sum_k dom[domain_b][k] wc[k][col]) + sum_k judge[judge_b][k] wc[dd + k][col] over the
// 2 x 4H columns (grid.y x 256), and the row's frame count into lens
__global__ __launch_bounds__(256) void mos_cond_kernel(const float* dom, const float* judge, const float* wc, const float* bias, float* cbias, int* lens,
                                                      int dd, int jd, int N, int r0, const RowTab R) {
    const int e = blockIdx.x, b = r0 + e, col = blockIdx.y * 256 + threadIdx.x;
    if (col == 0) lens[b] = R.frames[e];
    if (col >= N) return;
    const float* dv = dom + (long)R.dom[e] * dd;
    const float* jv = judge + (long)R.judge[e] * jd;
    float ad = 0.f, aj = 0.f;
    for (int k = 0; k < dd; ++k) ad = fmaf(dv[k], wc[(long)k * N + col], ad);
    for (int k = 0; k < jd; ++k) aj = fmaf(jv[k], wc[(long)(dd + k) * N + col], aj);
    cbias[(long)b * N + col] = (bias[col] + ad) + aj;
}

__device__ __forceinline__ float sigmoidf_(float x) { return __fdiv_rn(1.f, 1.f + expf(-x)); }

// gi [B][T][2 G] (G = 4H; direction d at column d G), whh [2][H / 4][G] float4, len [B] -> y [B][T][2 H] (direction d at column d H)
struct LstmP { const float* gi; const float4* whh; const int* len; float* y; int B, T, H; };

// the recurrence of one workgroup with NR live rows (the last group of a batch has fewer than ROWS: the dead rows cost nothing).
// NC: gate columns (and (row, unit) pairs) per thread.  A row's chains do not depend on NR
template <int NC, int NR>
__device__ __forceinline__ void mos_lstm_rows(const LstmP& p, int group, int dir, float (*hs)[MAXH], float (*gs)[NC * LSTM_T]) {
    const int tid = threadIdx.x, nt = blockDim.x, row0 = group * ROWS;
    const int H = p.H, G = 4 * H, T = p.T;
    int len[NR], nsteps = 0;
    const float* gp[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        len[r] = min(p.len[row0 + r], T);
        nsteps = max(nsteps, len[r]);
        gp[r] = p.gi + (long)(row0 + r) * T * 2 * G + (long)dir * G;
    }
    // the columns this thread owns, and the (row, unit) pairs it updates
    int ur[NC], uj[NC], ulen[NC];
    bool cv[NC], pv[NC];
    float c[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int q = tid + j * nt;
        cv[j] = q < G; pv[j] = q < NR * H;
        ur[j] = pv[j] ? q / H : 0; uj[j] = pv[j] ? q - ur[j] * H : 0;
        c[j] = 0.f;
        ulen[j] = 0;
#pragma unroll
        for (int r = 0; r < NR; ++r) ulen[j] = ur[j] == r ? len[r] : ulen[j];
        if (pv[j]) hs[ur[j]][uj[j]] = 0.f;
    }
    // 0 past a row's frames
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        float* yr = p.y + (long)(row0 + r) * T * 2 * H + (long)dir * H;
        for (long i = (long)len[r] * H + tid; i < (long)T * H; i += nt) { const long t = i / H; yr[t * 2 * H + (i - t * H)] = 0.f; }
    }
    auto frame = [&](int r, int s) { return max(0, min(dir ? len[r] - 1 - s : s, T - 1)); };      // step s of row r (clamped where the row is over)
    float gn[NC][NR];
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
        for (int r = 0; r < NR; ++r) gn[j][r] = cv[j] ? gp[r][(long)frame(r, 0) * 2 * G + tid + j * nt] : 0.f;
    const float4* wp = p.whh + (long)dir * (H / 4) * G + tid;
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        float acc[NC][NR];
#pragma unroll
        for (int j = 0; j < NC; ++j)
#pragma unroll
            for (int r = 0; r < NR; ++r) acc[j][r] = gn[j][r];
        if (s + 1 < nsteps) {                                   // the next step's input projection travels under this step's chain
#pragma unroll
            for (int j = 0; j < NC; ++j)
#pragma unroll
                for (int r = 0; r < NR; ++r) gn[j][r] = cv[j] ? gp[r][(long)frame(r, s + 1) * 2 * G + tid + j * nt] : 0.f;
        }
        // U x 16 B of every column in flight per lane, then their k of the chains (k ascending within every column).  One column: 8, as
        // spk_lstm_kernel.  Two columns: fewer - a 1024-thread workgroup leaves a lane 128 registers, and 4 each with 4 rows spills 12
        // of them; with fewer live rows there is room for more
        constexpr int U = NC == 1 ? 8 : (NR == 1 ? 8 : (NR == 2 ? 4 : 2));
#pragma unroll 1
        for (int q0 = 0; q0 < H / 4; q0 += U) {
            float4 w[NC][U];
#pragma unroll
            for (int j = 0; j < NC; ++j)
#pragma unroll
                for (int u = 0; u < U; ++u) w[j][u] = cv[j] ? wp[(long)(q0 + u) * G + j * nt] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    const float4 hv = *reinterpret_cast<const float4*>(&hs[r][4 * (q0 + u)]);
#pragma unroll
                    for (int j = 0; j < NC; ++j) {
                        acc[j][r] = fmaf(hv.x, w[j][u].x, acc[j][r]);
                        acc[j][r] = fmaf(hv.y, w[j][u].y, acc[j][r]);
                        acc[j][r] = fmaf(hv.z, w[j][u].z, acc[j][r]);
                        acc[j][r] = fmaf(hv.w, w[j][u].w, acc[j][r]);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NC; ++j)
            if (cv[j])
#pragma unroll
                for (int r = 0; r < NR; ++r) gs[r][tid + j * nt] = acc[j][r];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int r = ur[j], u = uj[j];
            if (!pv[j] || s >= ulen[j]) continue;                // the row is over: its state is read by nothing
            const float ig = sigmoidf_(gs[r][u]), fg = sigmoidf_(gs[r][H + u]), gg = tanhf(gs[r][2 * H + u]), og = sigmoidf_(gs[r][3 * H + u]);
            c[j] = fmaf(fg, c[j], ig * gg);
            const float hn = og * tanhf(c[j]);
            hs[r][u] = hn;
            const int t = dir ? ulen[j] - 1 - s : s;
            p.y[((long)(row0 + r) * T + t) * 2 * H + (long)dir * H + u] = hn;
        }
        __syncthreads();
    }
}

// blockDim.x = min(4H, 1024); grid 8 x ceil(groups / 4) with groups = ceil(B / ROWS): 4 groups x 2 directions per 8 blocks
template <int NC>
__global__ __launch_bounds__(LSTM_T) void mos_lstm_kernel(const LstmP p) {
    __shared__ __attribute__((aligned(16))) float hs[ROWS][MAXH];
    __shared__ float gs[ROWS][NC * LSTM_T];
    // workgroups are dealt to the 8 XCDs in turn: blocks 0 - 3 of every 8 take the forward direction, 4 - 7 the reverse, so an XCD's
    // L2 (4 MiB) is asked for ONE direction's W_hh (4 MiB at H = 512), not both.  Placement is for speed only: nothing depends on it
    const int l8 = blockIdx.x & 7, dir = l8 >> 2, group = (blockIdx.x >> 3) * 4 + (l8 & 3);
    if (group * ROWS >= p.B) return;
    switch (min(ROWS, p.B - group * ROWS)) {
    case 1: mos_lstm_rows<NC, 1>(p, group, dir, hs, gs); break;
    case 2: mos_lstm_rows<NC, 2>(p, group, dir, hs, gs); break;
    case 3: mos_lstm_rows<NC, 3>(p, group, dir, hs, gs); break;
    default: mos_lstm_rows<NC, 4>(p, group, dir, hs, gs); break;
    }
}

// fs [B][T][OUT_LD] (column 0 the frame's score), len [B] -> frames [B][T] (0 past the row's frames; may be null),
// score [B] = mean x 2 + 3 (may be null).  One workgroup per row
__global__ __launch_bounds__(256) void mos_mean_kernel(const float* fs, const int* len, int T, float* frames, float* score) {
    __shared__ double red[256];
    const int b = blockIdx.x, tid = threadIdx.x, L = min(len[b], T);
    const float* f = fs + (long)b * T * OUT_LD;
    double s = 0.0;
    for (int t = tid; t < T; t += 256) {
        const float v = t < L ? f[(long)t * OUT_LD] : 0.f;
        if (t < L) s += (double)v;
        if (frames) frames[(long)b * T + t] = v;
    }
    const double tot = block_sum<256>(s, red);
    if (score && tid == 0) score[b] = (float)(tot / (double)L * 2.0 + 3.0);
}

// dst[i] = mask[i / H4] != 0 ? src[i] : 0 (float4s)
__global__ __launch_bounds__(256) void mos_mask_kernel(const float4* src, const float* mask, float4* dst, long n4, int H4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    dst[i] = mask[i / H4] != 0.f ? src[i] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// Linear weight src [N][ld], columns k0 .. k0 + K -> dst [K][ldn] at column coff
__global__ __launch_bounds__(256) void mos_pack_t_kernel(const float* src, float* dst, int N, int ld, int k0, int K, int ldn, int coff) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)K * N) return;
    const int n = (int)(i % N), k = (int)(i / N);
    dst[(long)k * ldn + coff + n] = src[(long)n * ld + k0 + k];
}
// W_hh [4H][H] -> [H / 4][4H] float4
__global__ __launch_bounds__(256) void mos_pack_hh_kernel(const float4* w, float4* out, int H) {
    const int i = blockIdx.x * 256 + threadIdx.x, G = 4 * H;      // = q G + col
    if (i >= (H / 4) * G) return;
    const int q = i / G, col = i - q * G;
    out[i] = w[(long)col * (H / 4) + q];
}
__global__ __launch_bounds__(256) void mos_add_kernel(const float* a, const float* b, float* out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = __fadd_rn(a[i], b[i]);
}

DexMosConfig default_config() {
    DexMosConfig c;
    std::memset(&c, 0, sizeof c);
    default_trunk_geometry(c);
    c.conv_bias = 0; c.feat_extract_norm_group = 1;
    c.hidden = 768; c.n_layers = 12; c.n_heads = 12; c.intermediate = 3072; c.do_stable_layer_norm = 0;
    c.num_domains = 3; c.domain_dim = 128; c.num_judges = 3000; c.judge_dim = 128; c.lstm_hidden = 512; c.proj_hidden = 2048;
    return c;
}

// the family that is built; names the first field outside it
int check_config(const DexMosConfig& c) {
    if (c.feat_extract_norm_group != 1) return create_fail("%s: only 'group' is built", "feat_extract_norm");
    if (c.do_stable_layer_norm != 0) return create_fail("%s: only False is built", "do_stable_layer_norm");
    if (int rc = check_trunk(trunk_of(c), 4)) return rc;
    if (c.hidden % 32) return create_fail("%s: a multiple of 32", "hidden_size");
    if (c.num_domains < 1 || c.num_domains > (1 << 20)) return create_fail("%s: 1 .. 2^20", "num_domains");
    if (c.num_judges < 1 || c.num_judges > (1 << 20)) return create_fail("%s: 1 .. 2^20", "num_judges");
    if (c.domain_dim < 1 || c.domain_dim > 4096) return create_fail("%s: 1 .. 4096", "domain_dim");
    if (c.judge_dim < 1 || c.judge_dim > 4096) return create_fail("%s: 1 .. 4096", "judge_dim");
    if (c.lstm_hidden < 64 || c.lstm_hidden % 64 || c.lstm_hidden > MAXH) return create_fail("%s: a multiple of 64 up to 512", "lstm_hidden");
    if (c.proj_hidden < 32 || c.proj_hidden % 32 || c.proj_hidden > 16384) return create_fail("%s: a multiple of 32 up to 16384", "proj_hidden");
    return DEX_OK;
}

long min_samples(const DexMosConfig& c) { return samples_for(trunk_of(c), 1); }      // one encoder frame

const TrunkKeys KEYS("wav2vec2.");
const char* const DIRS[2] = {"", "_reverse"};
std::string rk(const char* what, int d) { return std::string("decoder_rnn.") + what + "_l0" + DIRS[d]; }

}  // namespace

struct DexMos : TrunkStore {
    DexMos() : TrunkStore("utmos ", "dex_mos") {}
    DexMosConfig c;
    const float *dom = nullptr, *judge = nullptr;
    const float *wih = nullptr, *wcond = nullptr, *bias = nullptr;       // [hidden][2 G], [dd + jd][2 G], [2 G] = b_ih + b_hh
    const float4* whh = nullptr;                                          // [2][H / 4][G]
    const float *p0w = nullptr, *p0b = nullptr, *p3w = nullptr, *p3b = nullptr;
};

namespace {

void register_keys(DexMos* s) {
    const DexMosConfig& c = s->c;
    s->t = trunk_of(c);
    s->why = "too short for one frame of the feature extractor (" + std::to_string(min_samples(c)) + " samples)";
    s->rule = WavRule{min_samples(c), s->why.c_str(), 0, MAXF};
    register_trunk_keys(s, KEYS, s->t, false, [](int) {});
    const int H = c.lstm_hidden, in = c.hidden + c.domain_dim + c.judge_dim;
    s->add("domain_embedding.weight", {c.num_domains, c.domain_dim});
    s->add("judge_embedding.weight", {c.num_judges, c.judge_dim});
    for (int d = 0; d < 2; ++d) {
        s->add(rk("weight_ih", d), {4 * H, in}); s->add(rk("weight_hh", d), {4 * H, H});
        s->add(rk("bias_ih", d), {4 * H}); s->add(rk("bias_hh", d), {4 * H});
    }
    s->add("projection.0.weight", {c.proj_hidden, 2 * H}); s->add("projection.0.bias", {c.proj_hidden});
    s->add("projection.3.weight", {1, c.proj_hidden}); s->add("projection.3.bias", {1});
}

int pack_all(DexMos* s, hipStream_t st) {
    const DexMosConfig& c = s->c;
    const Trunk& t = s->t;
    auto pack_pos = [&](const double* scale) { pack_pos_padded(s, KEYS, t, s->w, scale, st); };
    if (int rc = finalize_trunk(s, KEYS, t, false, s->w, pack_pos, st)) return rc;
    s->dom = s->R("domain_embedding.weight"); s->judge = s->R("judge_embedding.weight");
    const int H = c.lstm_hidden, G = 4 * H, nc = c.domain_dim + c.judge_dim, in = c.hidden + nc, P = c.proj_hidden;
    float* wih = s->alloc((long)c.hidden * 2 * G); float* wc = s->alloc((long)nc * 2 * G); float* bias = s->alloc(2L * G);
    float* whh = s->alloc(2L * H * G);
    float* p0 = s->alloc(2L * H * P); float* p3 = s->alloc((long)P * OUT_LD); float* p3b = s->alloc(OUT_LD);
    if (s->alloc_rc != DEX_OK) return s->alloc_rc;
    auto pack_t = [&](const float* src, float* dst, int N, int ld, int k0, int K, int ldn, int coff) {
        hipLaunchKernelGGL(mos_pack_t_kernel, dim3((unsigned)(((long)K * N + 255) / 256)), dim3(256), 0, st, src, dst, N, ld, k0, K, ldn, coff);
    };
    for (int d = 0; d < 2; ++d) {
        pack_t(s->R(rk("weight_ih", d)), wih, G, in, 0, c.hidden, 2 * G, d * G);
        pack_t(s->R(rk("weight_ih", d)), wc, G, in, c.hidden, nc, 2 * G, d * G);
        hipLaunchKernelGGL(mos_add_kernel, dim3((G + 255) / 256), dim3(256), 0, st, s->R(rk("bias_ih", d)), s->R(rk("bias_hh", d)), bias + (long)d * G, G);
        hipLaunchKernelGGL(mos_pack_hh_kernel, dim3(((H / 4) * G + 255) / 256), dim3(256), 0, st, (const float4*)s->R(rk("weight_hh", d)),
                           (float4*)whh + (long)d * (H / 4) * G, H);
    }
    pack_t(s->R("projection.0.weight"), p0, P, 2 * H, 0, 2 * H, P, 0);
    DEX_HIPCHK(s, hipMemsetAsync(p3, 0, (size_t)P * OUT_LD * sizeof(float), st));
    DEX_HIPCHK(s, hipMemsetAsync(p3b, 0, OUT_LD * sizeof(float), st));
    pack_t(s->R("projection.3.weight"), p3, 1, P, 0, P, OUT_LD, 0);
    DEX_HIPCHK(s, hipMemcpyAsync(p3b, s->R("projection.3.bias"), sizeof(float), hipMemcpyDeviceToDevice, st));
    s->wih = wih; s->wcond = wc; s->bias = bias; s->whh = (const float4*)whh;
    s->p0w = p0; s->p0b = s->R("projection.0.bias"); s->p3w = p3; s->p3b = p3b;
    return DEX_OK;
}

// the head's workspace: cbias [B][2 G] | gi [B][T][2 G] | lo [B][T][2 H] | p1 [B][T][P] | fs [B][T][OUT_LD] | flens (int) [B]
struct HeadWs { float *cbias, *gi, *lo, *p1, *fs; int* flens; };
void plan_head(const DexMosConfig& c, Taker& tk, long B, long T, bool recurrence_only, HeadWs& h) {
    const long H = c.lstm_hidden, G = 4 * H;
    h.cbias = tk.take(B * 2 * G); h.gi = tk.take(B * T * 2 * G);
    h.lo = tk.take(recurrence_only ? 0 : B * T * 2 * H);
    h.p1 = tk.take(recurrence_only ? 0 : B * T * c.proj_hidden); h.fs = tk.take(recurrence_only ? 0 : B * T * OUT_LD);
    h.flens = (int*)tk.take(B);
}

// workspace: the trunk's prefix | yp, pp (padded positional groups) | mask [B][T] | the group norm's pieces | lens (int) [n_conv + 1][B] |
// hid [B][T][hidden] | the head's pieces
struct Ws : TrunkWs, GnWs, PosWs, HeadWs { float* hid; size_t bytes; };
Ws plan(const DexMos* s, void* ws, long B, long n) {
    const DexMosConfig& c = s->c;
    Ws w{};
    Taker tk(ws);
    plan_trunk(s->t, tk, B, n, w);
    const long T = w.T;
    plan_pos_padded(s->t, tk, B, T, w);
    w.mask = tk.take(B * T);
    plan_groupnorm(tk, B, w.Tl[0], c.conv_dim[0], w);
    w.lens = (int*)tk.take((long)(c.n_conv + 1) * B);
    w.hid = tk.take(B * T * c.hidden);
    plan_head(c, tk, B, T, false, w);
    w.bytes = tk.bytes();
    return w;
}
struct BiWs : HeadWs { size_t bytes; };
BiWs plan_bilstm(const DexMos* s, void* ws, long B, long T) {
    BiWs w{};
    Taker tk(ws);
    plan_head(s->c, tk, B, T, true, w);
    w.bytes = tk.bytes();
    return w;
}

// the trunk: last_hidden_state at `hidden` [B][T][H] (0 past a row's frames)
int enqueue_trunk(DexMos* s, const float* wav, const int32_t* lengths_host, int B, int n, int do_normalize, float* hidden, const Ws& w, hipStream_t st) {
    const Trunk& t = s->t;
    const TrunkWeights& W = s->w;
    const int H = t.hidden;
    enqueue_groupnorm_front(t, W, w, w, w, wav, lengths_host, B, n, do_normalize, st);
    const int* kv_len = w.lens + (long)t.n_conv * B;
    for (const TrunkWeights::Layer& L : W.layers) enqueue_plain_layer<false>(layer_dims(t), L, w, kv_len, B, st);      // post-norm
    const long n4 = (long)B * w.T * H / 4;
    hipLaunchKernelGGL(mos_mask_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, (const float4*)w.h, w.mask, (float4*)hidden, n4, H / 4);
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

// features [B][T][hidden], row b frames_host[b] frames -> out [B][T][2 H]: the conditioning, the input projections, the recurrence
int enqueue_bilstm(DexMos* s, const float* feat, const int32_t* frames_host, const int32_t* domain_host, const int32_t* judge_host, int B, int T,
                   float* out, const HeadWs& w, hipStream_t st) {
    const DexMosConfig& c = s->c;
    const int H = c.lstm_hidden, G = 4 * H, N = 2 * G;
    for_each_row_table<RowTab>(B, [&](RowTab& R, int e, int b) { R.dom[e] = domain_host[b]; R.judge[e] = judge_host[b]; R.frames[e] = frames_host[b]; },
                               [&](int r0, const RowTab& R) {
        hipLaunchKernelGGL(mos_cond_kernel, dim3(R.n, (N + 255) / 256), dim3(256), 0, st, s->dom, s->judge, s->wcond, s->bias, w.cbias, w.flens,
                           c.domain_dim, c.judge_dim, N, r0, R);
    });
    {   // gi = feat W_ih[:, : hidden]^T + cbias[b]: the GEMM of wav_encoder.h's linear() with a per-row bias
        dex::IGemmP g{};
        g.A = feat; g.lda = c.hidden; g.a_bstride = (long)T * c.hidden;
        g.Hi = 1; g.Wi = T; g.Cin = c.hidden;
        g.KH = 1; g.KW = 1; g.sh = 1; g.sw = 1; g.step_h = 1; g.step_w = 1;
        g.Ho = 1; g.Wo = T;
        g.W = s->wih; g.w_gstride = (long)c.hidden * N; g.N = N; g.K = c.hidden; g.ksplit = 1; g.groups = 1;
        g.bias = w.cbias; g.bias_bstride = N;
        g.C = w.gi; g.ldc = N; g.c_bstride = (long)T * N; g.c_sstride = (long)B * T * N;
        g.OHf = 1; g.OWf = T; g.osh = 1; g.osw = 1;
        g.inmask_ws = 1; g.outmask_ws = 1; g.mask_bstride = T; g.gate_nstride = 1;
        g.ldres = N; g.res_bstride = (long)T * N;
        g.B = B;
        dex::launch_igemm(g, dex::PREC_FP32, st);
    }
    const int groups = (B + ROWS - 1) / ROWS;
    const LstmP lp{w.gi, s->whh, w.flens, out, B, T, H};
    const dim3 grid(8 * ((groups + 3) / 4)), block(G < LSTM_T ? G : LSTM_T);
    if (G > LSTM_T) hipLaunchKernelGGL(mos_lstm_kernel<2>, grid, block, 0, st, lp);
    else hipLaunchKernelGGL(mos_lstm_kernel<1>, grid, block, 0, st, lp);
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

// lo [B][T][2 H] -> frames [B][T] and / or score [B]
int enqueue_projection_head(DexMos* s, int B, int T, float* frames, float* score, const HeadWs& w, hipStream_t st) {
    const DexMosConfig& c = s->c;
    linear(w.lo, 2 * c.lstm_hidden, s->p0w, c.proj_hidden, s->p0b, w.p1, 2, nullptr, nullptr, T, B, st);
    linear(w.p1, c.proj_hidden, s->p3w, OUT_LD, s->p3b, w.fs, 0, nullptr, nullptr, T, B, st);
    hipLaunchKernelGGL(mos_mean_kernel, dim3(B), dim3(256), 0, st, w.fs, w.flens, T, frames, score);
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

int check_ids(DexMos* s, const int32_t* domain_host, const int32_t* judge_host, int B) {
    if (!domain_host || !judge_host) return s->fail(DEX_ERR_ARG, "null pointer argument");
    for (int b = 0; b < B; ++b) {
        if (domain_host[b] < 0 || domain_host[b] >= s->c.num_domains) return s->fail(DEX_ERR_ARG, "row %d: domain %d is outside [0, %d)", b, domain_host[b], s->c.num_domains);
        if (judge_host[b] < 0 || judge_host[b] >= s->c.num_judges) return s->fail(DEX_ERR_ARG, "row %d: judge %d is outside [0, %d)", b, judge_host[b], s->c.num_judges);
    }
    return DEX_OK;
}

typedef Entry<DexMos> E;

// hidden_dev, frames_dev, score_dev: whichever is asked for (the ids are read only where the head runs)
int run(DexMos* s, const float* wav_dev, const int32_t* lengths_host, const int32_t* domain_host, const int32_t* judge_host, int B, int n_samples,
        int do_normalize, float* hidden_dev, float* frames_dev, float* score_dev, void* workspace_dev, size_t workspace_bytes, hipStream_t st) {
    const bool head = frames_dev || score_dev;
    return E::call(s, wav_dev, lengths_host, B, n_samples, hidden_dev || head, workspace_dev, workspace_bytes, plan,
                   [&] { return head ? check_ids(s, domain_host, judge_host, B) : DEX_OK; }, [&](const Ws& w, int T) {
        float* hidden = hidden_dev ? hidden_dev : w.hid;
        int rc = enqueue_trunk(s, wav_dev, lengths_host, B, n_samples, do_normalize, hidden, w, st);
        if (rc == DEX_OK && head) {
            std::vector<int32_t> frames(B);
            for (int b = 0; b < B; ++b) frames[b] = frames_of(s->t, lengths_host[b], s->t.n_conv);
            rc = enqueue_bilstm(s, hidden, frames.data(), domain_host, judge_host, B, T, w.lo, w, st);
            if (rc == DEX_OK) rc = enqueue_projection_head(s, B, T, frames_dev, score_dev, w, st);
        }
        return rc;
    });
}

}  // namespace

extern "C" {

int dex_mos_create(const DexMosConfig* cfg, DexMos** out) { return E::create(cfg, out, default_config, check_config, register_keys); }
void dex_mos_destroy(DexMos* s) { E::destroy(s); }
const char* dex_mos_last_error(const DexMos* s) { return E::last_error(s); }
int dex_mos_load(DexMos* s, const char* key, const float* w_dev, const int64_t* shape, int ndim, dex_stream_t stream) {
    return E::load(s, key, w_dev, shape, ndim, stream);
}
int dex_mos_finalize(DexMos* s, dex_stream_t stream) { return E::finalize(s, stream, pack_all, "packing the utmos weights failed"); }
int dex_mos_num_weights(const DexMos* s) { return E::num_weights(s); }
int dex_mos_weight_info(const DexMos* s, int i, const char** key, int64_t shape[4], int* ndim) { return E::weight_info(s, i, key, shape, ndim); }

int dex_mos_num_frames(const DexMosConfig* cfg, int n_samples) { return E::num_frames(cfg, n_samples, default_config, conv_ok<DexMosConfig>); }
int dex_mos_min_samples(const DexMosConfig* cfg) { return E::min_samples(cfg, default_config, conv_ok<DexMosConfig>, min_samples); }
size_t dex_mos_workspace_bytes(const DexMos* s, int B, int max_samples) { return E::workspace_bytes(s, B, max_samples, plan); }

size_t dex_mos_bilstm_workspace_bytes(const DexMos* s, int B, int T) {
    if (!s || B < 1 || B > MAX_B || T < 1 || T > MAXF) return 0;
    return plan_bilstm(s, nullptr, B, T).bytes;
}

int dex_mos_hidden(DexMos* s, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, int do_normalize, float* hidden_dev,
                   void* workspace_dev, size_t workspace_bytes, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!hidden_dev) return s->fail(DEX_ERR_ARG, "null pointer argument");
    return run(s, wav_dev, lengths_host, nullptr, nullptr, B, n_samples, do_normalize, hidden_dev, nullptr, nullptr, workspace_dev, workspace_bytes,
               (hipStream_t)stream);
}

int dex_mos_bilstm(DexMos* s, const float* feat_dev, const int32_t* frames_host, const int32_t* domain_host, const int32_t* judge_host, int B, int T,
                   float* out_dev, void* workspace_dev, size_t workspace_bytes, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!feat_dev || !frames_host || !out_dev || !workspace_dev) return s->fail(DEX_ERR_ARG, "null pointer argument");
    if (B < 1 || B > MAX_B) return s->fail(DEX_ERR_ARG, "B must lie in [1, %d]", MAX_B);
    if (T < 1 || T > MAXF) return s->fail(DEX_ERR_ARG, "T must lie in [1, %d]", MAXF);
    for (int b = 0; b < B; ++b)
        if (frames_host[b] < 1 || frames_host[b] > T) return s->fail(DEX_ERR_ARG, "frame counts must lie in [1, T]");
    if (int rc = check_ids(s, domain_host, judge_host, B)) return rc;
    if (!s->finalized) return s->fail(DEX_ERR_STATE, "the utmos weights are not finalized (dex_mos_finalize)");
    const BiWs w = plan_bilstm(s, workspace_dev, B, T);
    if (workspace_bytes < w.bytes) return s->fail(DEX_ERR_WORKSPACE, "workspace too small (dex_mos_bilstm_workspace_bytes)");
    const int rc = enqueue_bilstm(s, feat_dev, frames_host, domain_host, judge_host, B, T, out_dev, w, (hipStream_t)stream);
    return rc ? s->fail(rc, "kernel launch failed") : DEX_OK;
}

int dex_mos_frames(DexMos* s, const float* wav_dev, const int32_t* lengths_host, const int32_t* domain_host, const int32_t* judge_host, int B,
                   int n_samples, int do_normalize, float* frames_dev, void* workspace_dev, size_t workspace_bytes, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!frames_dev) return s->fail(DEX_ERR_ARG, "null pointer argument");
    return run(s, wav_dev, lengths_host, domain_host, judge_host, B, n_samples, do_normalize, nullptr, frames_dev, nullptr, workspace_dev,
               workspace_bytes, (hipStream_t)stream);
}

int dex_mos_score(DexMos* s, const float* wav_dev, const int32_t* lengths_host, const int32_t* domain_host, const int32_t* judge_host, int B,
                  int n_samples, int do_normalize, float* score_dev, void* workspace_dev, size_t workspace_bytes, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!score_dev) return s->fail(DEX_ERR_ARG, "null pointer argument");
    return run(s, wav_dev, lengths_host, domain_host, judge_host, B, n_samples, do_normalize, nullptr, nullptr, score_dev, workspace_dev,
               workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
