// whisper.hip — the Whisper ASR score on the device: HF's WhisperForConditionalGeneration in eval mode (log-mel front end of
// WhisperFeatureExtractor, encoder, decoder with a key/value cache, greedy decoding).  fp32 throughout, channels-last.  C ABI
// dex_whisper_*; dex_tts_amd/whisper.py states the definitions.
//
//   wsp_mel_long_kernel  the front end up to log10: 8 frames per workgroup; the zero-padded, reflect-padded, Hann-windowed frames in
//                        LDS as fp64, the 400-point DFT as a direct sum in fp64 (400 is no power of two; one thread per bin walks the
//                        twiddle table by k n mod 400), power, the mel matrix (fp64, built on the host), log10(max(., 1e-10)).  A row of
//                        at most one chunk is zero-padded to the chunk and has its frames; a longer row has its own ends reflected and
//                        len / 160 frames.
//   wsp_mel_floor_long_kernel  one workgroup per row: the maximum over all of the row's frames (a maximum has no summation order), the
//                        floor at max - 8, (x + 4) / 4, rounded to fp32 once and stored [n_mels][frames], 0 behind the row's frames.
//   wsp_gather_kernel    the cut of a 30 s window at a row's seek.
//   launch_igemm         (igemm.hip, exact-fp32 MFMA) every wide contraction: conv1 (the mel channels padded to a multiple of 32,
//                        GELU in the epilogue), conv2 (stride 2, GELU and + embed_positions in the epilogue), the encoder's q|k|v,
//                        out_proj, fc1, fc2, and the cross-attention k|v of every decoder layer, once per utterance.  The encoder
//                        layer is wav_trunk.h's, pre-norm with the plain attention (attention.hip's generic fp32 kernel at
//                        head_dim 64, no mask) and fc2 as one launch.
//   wsp_skinny_kernel    the decoder step's linears at M = B <= 32 rows: every weight element is read from HBM once for the whole
//                        batch.  A lane owns one output column, a wave 64 rows of K (all 64 loads issued before the first wait), the rows
//                        of x sit in LDS and are read as broadcasts; the four waves of a workgroup meet in LDS in wave order and the
//                        K slabs of a launch (KS = ceil(K / 256)) land as partials [KS][B][N] that the consumer adds in slab order.
//   wsp_finish_kernel    consumer of the partials, one workgroup per row: + bias, GELU, + residual, and the LayerNorm that follows.
//   wsp_attend_kernel    cached single-query attention at head_dim 64, one workgroup per (row, head).  Self-attention appends the
//                        step's k and v (finished from the q|k|v partials) at position p and attends over 0 .. p; cross-attention
//                        attends over the encoder frames.  Four lanes share a key's dot product (16 dims each, two shuffles), the
//                        scores sit in LDS, the maximum is exact, the sum of exponentials and the weighted sum of V (one lane per
//                        channel, keys dealt to the four waves) are reduced in a fixed order.
//   tail_first_sweep     the one pass over a row's logits that every greedy and policy tail starts with, plain or (rule_ranges: the
//                        masks of WhisperTimeStampLogitsProcessor as index ranges from the row's own state - its last two ids, its
//                        last timestamp, its new-token count, all on the device) under the timestamp rule of long-form decoding:
//                        logits finished from the partials, suppression, the best text id, the best timestamp id and
//                        logsumexp(timestamps), reduced in a fixed order, the lowest index on ties.
//   wsp_pick_kernel      the greedy step tail, one workgroup per row: the plain sweep, then pick_commit: finished / length
//                        bookkeeping and the gather of the next step's embed_tokens + embed_positions row.  A step needs no host value.
//   wsp_pick_ts_kernel   the same tail under the timestamp rule: the rule's sweep, then pick_commit.
//   wsp_pick_policy_kernel, wsp_nospeech_kernel, wsp_attend_rows_kernel
//                        fallback decoding (DecodingPolicy).  The tail in its plain and timestamp-rule forms: the same sweep (so
//                        the same ids at T = 0), then the fp64 log-sum-exp of the surviving ids, at T > 0 the
//                        Gumbel-max sample on Philox4x32-10 noise, and the chosen id's log-probability added to the row's sums.
//                        The probe: the fp64 softmax of the unprocessed logits of prompt position 0 at <|nospeech|>.  The rows
//                        form of the cross-attention reads the cache row of the encoded batch a retried row came from: a retry
//                        never runs the encoder again.
//   wsp_attend_anc_kernel, wsp_attend_cross_beam_kernel, wsp_beam_lse_kernel, wsp_beam_top_kernel, wsp_beam_pick_kernel
//                        beam search (U utterances of K beams = U x K rows of the step).  The self-attention form reads key t of row r
//                        from row anc[r][t] of the cache - no cache element moves when beams are reordered - and shares its body
//                        (attend_row) with wsp_attend_kernel; the cross form streams an utterance's K / V once for its K queries,
//                        K score rows in LDS, per query the plain kernel's operations in the plain kernel's order; the tail is three
//                        launches: the fp64 log-softmax sums by chunk of 2048 ids, every chunk's 2K best by score, and per
//                        utterance the top 2K of those, the running set, the pool, the stop, the ancestry and the next embeddings.
// Host: decode_loop is the one loop of the greedy, rule, policy and beam decoders (prompt fill, steps, the early exit on a device
// counter); each hands it the launch of its tail.  check_decode_args refuses what they all refuse; pick_over_logits and pick_in_step
// build the tail's parameters for the dex_whisper_pick* entry points and for a step of a decode.
// Every per-row sum has an order fixed by the config and the position: a row's logits and ids are bitwise those of the row alone.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dex_amd.h"
#include "kernels.h"
#include "wav_trunk.h"
#include "weight_store.h"

using namespace dex::wavenc;      // the GEMM wrappers, LayerNorm, packing, the encoder layer, Taker and Entry of the waveform networks

namespace {

constexpr int WB = DEX_WHISPER_MAX_B;
constexpr int NFFT = DEX_WHISPER_N_FFT, HOP = DEX_WHISPER_HOP, NBIN = NFFT / 2 + 1;
constexpr int MELF = 8;                  // frames per workgroup of the front end
constexpr int MAX_KEYS = 4096;           // keys of a single-query attention (their scores sit in LDS)
constexpr float LN_EPS = 1e-5f;

struct Lens { int a[WB]; };

// ------------------------------------------------------------------------------------------------------------ log-mel front end
struct MelP { const float* wav; long ld; Lens len; long N; int T, n_mels; const double *win, *cs, *sn, *filt; double* out; };

// frames t0 .. t0 + MELF - 1 of one row: x its samples, L of them stored, reflected at N (centre = True), T frames in the row; out the
// row's [T][n_mels]
__device__ __forceinline__ void mel_frames(const MelP& p, const float* x, int L, long N, int T, int t0, double* out) {
    __shared__ double xs[MELF][NFFT];
    __shared__ double cs[NFFT], sn[NFFT];
    __shared__ double pw[MELF][NBIN];
    const int tid = threadIdx.x;
    for (int i = tid; i < MELF * NFFT; i += 256) {
        const int f = i / NFFT, n = i - f * NFFT, t = t0 + f;
        long j = (long)t * HOP + n - NFFT / 2;                      // centre = True, reflect padding of the N samples (the zero-padded chunk, or a long row)
        if (j < 0) j = -j;
        if (j >= N) j = 2 * (N - 1) - j;
        xs[f][n] = (t < T && j < L) ? (double)x[j] * p.win[n] : 0.0;
    }
    for (int i = tid; i < NFFT; i += 256) { cs[i] = p.cs[i]; sn[i] = p.sn[i]; }
    __syncthreads();
    if (tid < NBIN) {
        double re[MELF], im[MELF];
#pragma unroll
        for (int f = 0; f < MELF; ++f) re[f] = im[f] = 0.0;
        int idx = 0;
        for (int n = 0; n < NFFT; ++n) {
            const double c = cs[idx], s = sn[idx];
#pragma unroll
            for (int f = 0; f < MELF; ++f) { const double v = xs[f][n]; re[f] = fma(v, c, re[f]); im[f] = fma(v, s, im[f]); }
            idx += tid;
            if (idx >= NFFT) idx -= NFFT;
        }
#pragma unroll
        for (int f = 0; f < MELF; ++f) pw[f][tid] = fma(re[f], re[f], im[f] * im[f]);
    }
    __syncthreads();
    for (int o = tid; o < MELF * p.n_mels; o += 256) {
        const int f = o / p.n_mels, m = o - f * p.n_mels, t = t0 + f;
        if (t >= T) continue;
        double a = 0.0;
        for (int k = 0; k < NBIN; ++k) a = fma(p.filt[(long)k * p.n_mels + m], pw[f][k], a);
        out[(long)t * p.n_mels + m] = log10(fmax(a, 1e-10));
    }
}

// the frames of a row: at most one chunk (p.N samples) -> the chunk's p.T frames of the zero-padded row; longer -> len / 160 frames
// of the row reflected at its own ends
__device__ __forceinline__ int long_frames(int L, long chunk, int T) { return L <= chunk ? T : L / HOP; }

// rows of any length: p.T = the frames of a chunk, p.N its samples; out [B][Fmax][n_mels]
__global__ __launch_bounds__(256) void wsp_mel_long_kernel(const MelP p, int Fmax) {
    const int b = blockIdx.y, L = p.len.a[b], t0 = blockIdx.x * MELF;
    const int T = long_frames(L, p.N, p.T);
    if (t0 >= T) return;
    mel_frames(p, p.wav + (long)b * p.ld, L, L <= p.N ? p.N : (long)L, T, t0, p.out + (long)b * Fmax * p.n_mels);
}

// feat [B][n_mels][T] -> cl [B][T][Mp], the channels past n_mels 0
__global__ __launch_bounds__(256) void wsp_feat_cl_kernel(const float* feat, float* cl, long total, int T, int n_mels, int Mp) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % Mp);
    const long bt = i / Mp;
    const long b = bt / T, t = bt - b * T;
    cl[i] = c < n_mels ? feat[(b * n_mels + c) * T + t] : 0.f;
}

// logspec [B][Fmax][n_mels] (fp64), row b of long_frames(len[b]) frames -> out [B][n_mels][Fmax]: the floor at the maximum over all of
// the row's frames - 8, (x + 4) / 4; 0 behind the row's frames
__global__ __launch_bounds__(1024) void wsp_mel_floor_long_kernel(const double* logspec, float* out, Lens len, long chunk, int Tc, int Fmax, int n_mels) {
    __shared__ double red[1024];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int T = long_frames(len.a[b], chunk, Tc);
    const long n = (long)T * n_mels, all = (long)Fmax * n_mels;
    const double* x = logspec + (long)b * all;
    double m = -1e300;
    for (long i = tid; i < n; i += 1024) m = fmax(m, x[i]);
    red[tid] = m;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
        __syncthreads();
    }
    const double lo = red[0] - 8.0;
    for (long i = tid; i < all; i += 1024) {
        const int mel = (int)(i / Fmax), t = (int)(i - (long)mel * Fmax);
        out[(long)b * all + i] = t < T ? (float)((fmax(x[(long)t * n_mels + mel], lo) + 4.0) / 4.0) : 0.f;
    }
}

// out [a][n_mels][W] = feat [row[a]][n_mels][seek[a] .. seek[a] + n[a]), 0.0 behind n[a]
struct GatherP { const float* feat; float* out; int Fmax, n_mels, W; Lens row, seek, n; };
__global__ __launch_bounds__(256) void wsp_gather_kernel(const GatherP p) {
    const int a = blockIdx.z, mel = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.W) return;
    const float* src = p.feat + ((long)p.row.a[a] * p.n_mels + mel) * p.Fmax + p.seek.a[a];
    p.out[((long)a * p.n_mels + mel) * p.W + t] = t < p.n.a[a] ? src[t] : 0.f;
}

// ------------------------------------------------------------------------------------------------------------ the step's linears
// A workgroup takes SK_ROWS rows of K, 64 per wave: a wave issues all of its loads before it waits for any.  KS = ceil(K / SK_ROWS)
// slabs, a function of K alone.  Measured per token at whisper-large-v3, B = 1 / 32: 64 rows per wave 6.06 / 10.7 ms,
// 32 rows per wave (twice the slabs, twice the partials the consumer reads) 7.75 / 12.3 ms, 16-load batches over 48-64 rows 6.47 / 11.4 ms
constexpr int SK_ROWS = 256, SK_WAVE = SK_ROWS / 4;
int slabs(int K) { return (K + SK_ROWS - 1) / SK_ROWS; }

struct SkP { const float* X; int ldx; const float* W; int ldw; int K, N; float* P; int B; };

// P [slab blockIdx.y][b][n] = sum over the slab's rows k of X[b][k] W[k][n], n = 64 blockIdx.x + lane; K % 64 == 0, ldw >= 64 gridDim.x.
// RB >= B rows are carried; a row's sum is the same fmaf chain whatever RB is
template <int RB>
__global__ __launch_bounds__(256) void wsp_skinny_kernel(const SkP p) {
    extern __shared__ float sm[];
    float* xs = sm;                                  // [SK_ROWS][RB]
    float* red = sm + SK_ROWS * RB;                  // [4][RB][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.x * 64 + lane, k0 = blockIdx.y * SK_ROWS;
    const int rows = p.K - k0 < SK_ROWS ? p.K - k0 : SK_ROWS;           // a multiple of 64: a wave has all of its rows or none
    const int kb = wave * SK_WAVE;
    const bool live = kb < rows;
    float w[SK_WAVE];
    if (live) {
        const float* W = p.W + (long)(k0 + kb) * p.ldw + n;
#pragma unroll
        for (int u = 0; u < SK_WAVE; ++u) w[u] = W[(long)u * p.ldw];
    }
    for (int i = tid; i < SK_ROWS * RB; i += 256) {
        const int b = i / SK_ROWS, k = i - b * SK_ROWS;
        xs[k * RB + b] = (b < p.B && k < rows) ? p.X[(long)b * p.ldx + k0 + k] : 0.f;
    }
    __syncthreads();
    float acc[RB];
#pragma unroll
    for (int b = 0; b < RB; ++b) acc[b] = 0.f;
    if (live) {
#pragma unroll
        for (int u = 0; u < SK_WAVE; ++u) {
            if constexpr (RB >= 4) {
                const float4* xr = reinterpret_cast<const float4*>(xs + (kb + u) * RB);
#pragma unroll
                for (int q = 0; q < RB / 4; ++q) {
                    const float4 x = xr[q];
                    acc[4 * q] = fmaf(x.x, w[u], acc[4 * q]); acc[4 * q + 1] = fmaf(x.y, w[u], acc[4 * q + 1]);
                    acc[4 * q + 2] = fmaf(x.z, w[u], acc[4 * q + 2]); acc[4 * q + 3] = fmaf(x.w, w[u], acc[4 * q + 3]);
                }
            } else {
                acc[0] = fmaf(xs[kb + u], w[u], acc[0]);
            }
        }
    }
#pragma unroll
    for (int b = 0; b < RB; ++b) red[(wave * RB + b) * 64 + lane] = acc[b];
    __syncthreads();
    for (int b = wave; b < RB; b += 4) {
        if (b >= p.B || n >= p.N) continue;
        const float v = ((red[b * 64 + lane] + red[(RB + b) * 64 + lane]) + red[(2 * RB + b) * 64 + lane]) + red[(3 * RB + b) * 64 + lane];
        p.P[((long)blockIdx.y * p.B + b) * p.N + n] = v;
    }
}

// the value a launch of wsp_skinny_kernel left for (row offset `at`): its slabs in order, then the bias
__device__ __forceinline__ float finished(const float* P, int KS, long ss, long at, const float* bias, int c) {
    float v = P[at];
    for (int s = 1; s < KS; ++s) v += P[(long)s * ss + at];
    return bias ? v + bias[c] : v;
}

// sum of one float per thread over the 256 threads: butterfly in the wave, the four waves in order; every thread gets the total
__device__ __forceinline__ float block_sum256(float v, float* red4) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red4[0] + red4[1]) + red4[2]) + red4[3];
}

struct FinP { const float* P; int KS; long ss; int N; const float* bias; const float* res; float* out; int act;
              const float* g; const float* be; float* y; };

// row blockIdx.x: out = res + act(partials + bias) (P null: out = res); g: y = LayerNorm(out)
__global__ __launch_bounds__(256) void wsp_finish_kernel(const FinP p) {
    __shared__ float red4[4];
    const int tid = threadIdx.x;
    const long row = (long)blockIdx.x * p.N;
    float s = 0.f;
    for (int c = tid; c < p.N; c += 256) {
        float v;
        if (p.P) {
            v = finished(p.P, p.KS, p.ss, row + c, p.bias, c);
            if (p.act) v = gelu_erf_(v);
            if (p.res) v = p.res[row + c] + v;
            p.out[row + c] = v;
        } else {
            v = p.res[row + c];
        }
        s += v;
    }
    if (!p.g) return;
    const float* o = p.P ? p.out : p.res;
    const float mean = block_sum256(s, red4) / (float)p.N;
    float q = 0.f;
    for (int c = tid; c < p.N; c += 256) { const float d = o[row + c] - mean; q = fmaf(d, d, q); }
    const float rstd = 1.f / sqrtf(block_sum256(q, red4) / (float)p.N + LN_EPS);
    for (int c = tid; c < p.N; c += 256) p.y[row + c] = (o[row + c] - mean) * rstd * p.g[c] + p.be[c];
}

// ------------------------------------------------------------------------------------------------------------ cached attention
// q, kn, vn: slabs of partials (KS, ss) with row stride ldq, or plain rows (KS = 1); kn / vn (or null) are appended at key n - 1
struct AtP { const float* q; const float* kn; const float* vn; int KS; long ss; int ldq; const float *qbias, *kbias, *vbias;
             float* K; float* V; int ldk; long kb; int n; float* out; int ldo; float scale; };

// The body of the single-query attention of row blockIdx.y, head blockIdx.x.  ANC: key t is read from row base + anc[t] of the
// cache (the row's own at the appended position); otherwise from the row's own, and the code is that of the plain kernel
template <bool ANC>
__device__ __forceinline__ void attend_row(const AtP& p, const int* anc, int base, int beams, int kvb) {
    __shared__ float sc[MAX_KEYS];
    __shared__ float qs[64];
    __shared__ float red[4][64];
    __shared__ float red4[4];
    __shared__ int ancs[ANC ? MAX_KEYS : 1];         // the row's ancestry, staged once: a key's address must not wait for a global load
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = blockIdx.x, b = blockIdx.y;
    float* Kb = p.K + (long)kvb * p.kb + h * 64;          // kvb: the row of the cache that holds this row's keys (its own, but in the rows form)
    float* Vb = p.V + (long)kvb * p.kb + h * 64;
    if constexpr (ANC)
        for (int j = tid; j < p.n; j += 256) ancs[j] = anc[j];
    // the offset of key j's row from the row's own (0 without ancestry); an entry outside the utterance's beams reads the row's own
    auto hop = [&](int j) -> long {
        if constexpr (ANC) {
            if (p.kn && j == p.n - 1) return 0;
            const int a = ancs[j];
            return a >= 0 && a < beams ? (long)(base + a - b) * p.kb : 0;
        } else {
            return 0;
        }
    };
    {
        const int c = h * 64 + lane;
        const long at = (long)b * p.ldq + c;
        if (wave == 0) qs[lane] = p.scale * finished(p.q, p.KS, p.ss, at, p.qbias, c);
        else if (wave == 1 && p.kn) Kb[(long)(p.n - 1) * p.ldk + lane] = finished(p.kn, p.KS, p.ss, at, p.kbias, c);
        else if (wave == 2 && p.vn) Vb[(long)(p.n - 1) * p.ldk + lane] = finished(p.vn, p.KS, p.ss, at, p.vbias, c);
    }
    __syncthreads();
    // scores: four lanes per key, 16 dims each
    const int part = tid & 3, kk = tid >> 2;
    float qr[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) qr[i] = qs[part * 16 + i];
    for (int j0 = 0; j0 < p.n; j0 += 64) {
        const int j = j0 + kk;
        float s = 0.f;
        if (j < p.n) {
            const float4* kr = reinterpret_cast<const float4*>(Kb + hop(j) + (long)j * p.ldk + part * 16);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 k4 = kr[i];
                s = fmaf(qr[4 * i], k4.x, s); s = fmaf(qr[4 * i + 1], k4.y, s); s = fmaf(qr[4 * i + 2], k4.z, s); s = fmaf(qr[4 * i + 3], k4.w, s);
            }
        }
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        if (part == 0 && j < p.n) sc[j] = s;
    }
    __syncthreads();
    float m = -INFINITY;
    for (int j = tid; j < p.n; j += 256) m = fmaxf(m, sc[j]);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) red4[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red4[0], red4[1]), fmaxf(red4[2], red4[3]));
    float l = 0.f;
    for (int j = tid; j < p.n; j += 256) { const float e = expf(sc[j] - m); sc[j] = e; l += e; }
    l = block_sum256(l, red4);                       // (its barriers also publish the exponentials)
    float acc = 0.f;
#pragma unroll 8
    for (int j = wave; j < p.n; j += 4) acc = fmaf(sc[j], Vb[hop(j) + (long)j * p.ldk + lane], acc);
    red[wave][lane] = acc;
    __syncthreads();
    if (wave == 0) p.out[(long)b * p.ldo + h * 64 + lane] = (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]) / l;
}

__global__ __launch_bounds__(256) void wsp_attend_kernel(const AtP p) { attend_row<false>(p, nullptr, 0, 0, blockIdx.y); }

// The rows form of the cross-attention: query row blockIdx.y attends over cache row rows.a[blockIdx.y].  A retry of some rows of an
// encoded batch decodes them from the cross K / V where the encoder left it; per query the arithmetic is the plain kernel's
__global__ __launch_bounds__(256) void wsp_attend_rows_kernel(const AtP p, const Lens rows) { attend_row<false>(p, nullptr, 0, 0, rows.a[blockIdx.y]); }

// ------------------------------------------------------------------------------------------------------------ beam attention
// The self form: row blockIdx.y = u beams + r appends its k and v in its own row and reads the earlier positions through its ancestry
// anc [rows][ld_anc] (beam indices within the utterance).  No cache element moves when the beams are reordered
__global__ __launch_bounds__(256) void wsp_attend_anc_kernel(const AtP p, const int* anc, int ld_anc, int beams) {
    const int b = blockIdx.y;
    attend_row<true>(p, anc + (long)b * ld_anc, b / beams * beams, beams, b);
}

// The cross form: workgroup (head blockIdx.x, utterance blockIdx.y) streams the utterance's K / V (p.K, p.V, row stride p.kb per
// UTTERANCE) once for its KB queries, rows u KB + q of q and out.  KB sets of scores sit in dynamic LDS [KB][n].  Per query the
// operations and their order are those of attend_row: four lanes per key with 16 dims each, the same max and sum reductions, V
// accumulated by wave with stride 4 - a row is bitwise the plain kernel's
template <int KB>
__global__ __launch_bounds__(256) void wsp_attend_cross_beam_kernel(const AtP p) {
    extern __shared__ float scb[];                   // [KB][n]
    __shared__ float qs[KB][64];
    __shared__ float red[KB][4][64];
    __shared__ float red4[KB][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = blockIdx.x, u = blockIdx.y, n = p.n;
    const float* Kb = p.K + (long)u * p.kb + h * 64;
    const float* Vb = p.V + (long)u * p.kb + h * 64;
    for (int q = wave; q < KB; q += 4) {
        const int c = h * 64 + lane;
        qs[q][lane] = p.scale * finished(p.q, p.KS, p.ss, (long)(u * KB + q) * p.ldq + c, p.qbias, c);
    }
    __syncthreads();
    const int part = tid & 3, kk = tid >> 2;
    float qr[KB][16];
#pragma unroll
    for (int q = 0; q < KB; ++q)
#pragma unroll
        for (int i = 0; i < 16; ++i) qr[q][i] = qs[q][part * 16 + i];
    // KT tiles of 64 keys per trip, all 4 KT loads of a lane issued before the first is used: the workgroups are few (heads x
    // utterances) and each waits on HBM, so the loads in flight per lane set the pace
    constexpr int KT = 4;
    for (int j0 = 0; j0 < n; j0 += 64 * KT) {
        float4 k4[KT][4];
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            const int j = j0 + 64 * t + kk;
            const float4* kr = reinterpret_cast<const float4*>(Kb + (long)(j < n ? j : 0) * p.ldk + part * 16);
#pragma unroll
            for (int i = 0; i < 4; ++i) k4[t][i] = kr[i];
        }
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            const int j = j0 + 64 * t + kk;
#pragma unroll
            for (int q = 0; q < KB; ++q) {
                float s = 0.f;
                if (j < n) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        s = fmaf(qr[q][4 * i], k4[t][i].x, s); s = fmaf(qr[q][4 * i + 1], k4[t][i].y, s);
                        s = fmaf(qr[q][4 * i + 2], k4[t][i].z, s); s = fmaf(qr[q][4 * i + 3], k4[t][i].w, s);
                    }
                }
                s += __shfl_xor(s, 1);
                s += __shfl_xor(s, 2);
                if (part == 0 && j < n) scb[q * n + j] = s;
            }
        }
    }
    __syncthreads();
    float m[KB], l[KB];
#pragma unroll
    for (int q = 0; q < KB; ++q) {
        float v = -INFINITY;
        for (int j = tid; j < n; j += 256) v = fmaxf(v, scb[q * n + j]);
        for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
        if (lane == 0) red4[q][wave] = v;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < KB; ++q) {
        m[q] = fmaxf(fmaxf(red4[q][0], red4[q][1]), fmaxf(red4[q][2], red4[q][3]));
        float v = 0.f;
        for (int j = tid; j < n; j += 256) { const float e = expf(scb[q * n + j] - m[q]); scb[q * n + j] = e; v += e; }
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        l[q] = v;
    }
    __syncthreads();                                 // the maxima are read; the exponentials are published
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < KB; ++q) red4[q][wave] = l[q];
    __syncthreads();
    float acc[KB];
#pragma unroll
    for (int q = 0; q < KB; ++q) { l[q] = ((red4[q][0] + red4[q][1]) + red4[q][2]) + red4[q][3]; acc[q] = 0.f; }
    constexpr int VU = 32;                            // V rows in flight per wave; a query's sum still runs over j in steps of 4
    for (int j0 = wave; j0 < n; j0 += 4 * VU) {
        float v[VU];
#pragma unroll
        for (int t = 0; t < VU; ++t) { const int j = j0 + 4 * t; v[t] = Vb[(long)(j < n ? j : 0) * p.ldk + lane]; }
#pragma unroll
        for (int t = 0; t < VU; ++t) {
            const int j = j0 + 4 * t;
            if (j < n) {
#pragma unroll
                for (int q = 0; q < KB; ++q) acc[q] = fmaf(scb[q * n + j], v[t], acc[q]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < KB; ++q) red[q][wave][lane] = acc[q];
    __syncthreads();
    for (int q = wave; q < KB; q += 4)
        p.out[(long)(u * KB + q) * p.ldo + h * 64 + lane] = (((red[q][0][lane] + red[q][1][lane]) + red[q][2][lane]) + red[q][3][lane]) / l[q];
}

// ------------------------------------------------------------------------------------------------------------ greedy step tail
struct PickP { const float* P; int KS; long ss; int V; const uint8_t* mask; float* logits; long ldl; int pick, eos;
               int *finished, *lengths, *count, *ids; int ld_ids, step;
               const float *emb, *pos; int d, next_pos; float* h; };

__device__ __forceinline__ void better(float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// The end of a step for row b.  Thread 0 commits the id it chose (arg >= V: nothing competed - a row of NaN compares with nothing -
// and the id is 0; a finished row emits eos): the finished / count / lengths bookkeeping, under the timestamp rule (n_new given) the
// row's last timestamp (ids from tb on) and its new-token count, and the id store.  Then every thread gathers the next step's
// h = embed_tokens[id] + embed_positions[next_pos] (next_pos >= 0).  One writer per row
__device__ __forceinline__ void pick_commit(const PickP& p, int b, int arg, int* chosen, int tb, int* last_ts, int* n_new) {
    if (threadIdx.x == 0) {
        if (arg >= p.V) arg = 0;
        const int fin = p.finished[b];
        const int id = fin ? p.eos : arg;
        if (!fin) {
            if (id == p.eos) { p.finished[b] = 1; atomicAdd(p.count, 1); }
            else p.lengths[b] += 1;
            if (n_new && id >= tb) last_ts[b] = id;
        }
        if (n_new) n_new[b] += 1;
        p.ids[(long)b * p.ld_ids + p.step] = id;
        *chosen = id;
    }
    __syncthreads();
    if (p.next_pos < 0) return;
    const float* e = p.emb + (long)*chosen * p.d;
    const float* q = p.pos + (long)p.next_pos * p.d;
    for (int c = threadIdx.x; c < p.d; c += 1024) p.h[(long)b * p.d + c] = e[c] + q[c];
}

// The timestamp rule of long-form decoding (WhisperTimeStampLogitsProcessor) in a tail's parameters.  tb = the first timestamp id
// (no_timestamps + 1), max_init >= 0: the cap of the first timestamp; last_ts [B] the row's last emitted timestamp id (-1: none),
// n_new [B] its new-token count; its last two new ids are read from `ids` at columns step - 1 and step - 2
struct RuleP { int nots, tb, max_init; int *last_ts, *n_new; };
struct PickTsP { PickP k; RuleP r; };

// (m, s): a maximum and sum exp(x - m) over a set of values; the union of two sets.  Symmetric in its operands, bit for bit
__device__ __forceinline__ void lse_join(float& m, float& s, float om, float os) {
    const float M = fmaxf(m, om);
    const float a = m == -INFINITY ? 0.f : s * expf(m - M), c = om == -INFINITY ? 0.f : os * expf(om - M);
    m = M; s = a + c;
}

// Every mask of the rule is an index range fixed by the row's state, so a thread decides an id's fate from registers: text ids
// (below tb) live in [text_lo, tb), timestamps in [ts_lo, ts_hi], no_timestamps never.  The state: the row's new-token count, its
// last timestamp `seen`, its last and penultimate new ids.  Without the rule tb = V: every id is text
struct Ranges { int text_lo, ts_lo, ts_hi; };
__device__ __forceinline__ Ranges rule_ranges(int V, int tb, int eos, int max_init, int n_new, int seen, int last, int pen) {
    const bool last_ts = n_new >= 1 && last >= tb, pen_ts = n_new < 2 || pen >= tb;
    Ranges g{0, tb, V - 1};
    if (last_ts) {
        if (pen_ts) g.ts_lo = V;                     // a pair is closed: text next
        else g.text_lo = eos;                        // a lone timestamp: its partner (or eos) next
    }
    if (seen >= 0) {                                 // timestamps never decrease, and only a pair's partner may repeat
        const int lo = (last_ts && !pen_ts) ? seen : seen + 1;
        g.ts_lo = g.ts_lo > lo ? g.ts_lo : lo;
    }
    if (n_new == 0) {
        g.text_lo = tb;
        if (max_init >= 0 && tb + max_init < g.ts_hi) g.ts_hi = tb + max_init;
    }
    return g;
}

// the ranges of row b at this step (TS false: the plain tail's, every id open)
template <bool TS>
__device__ __forceinline__ Ranges row_ranges(const PickP& p, const RuleP& r, int b) {
    if constexpr (TS) {
        const int i = r.n_new[b];
        const int* at = p.ids + (long)b * p.ld_ids + p.step;
        return rule_ranges(p.V, r.tb, p.eos, r.max_init, i, r.last_ts[b], i >= 1 ? at[-1] : -1, i >= 2 ? at[-2] : -1);
    } else {
        return Ranges{0, p.V, p.V - 1};
    }
}

// whether id v competes before the rule's last part
template <bool TS>
__device__ __forceinline__ bool open_id(const PickP& p, const RuleP& r, const Ranges& g, int v) {
    if (p.mask && p.mask[v]) return false;
    if constexpr (TS) return v != r.nots && (v < r.tb ? v >= g.text_lo : (v >= g.ts_lo && v <= g.ts_hi));
    return true;
}

// The first sweep of every tail over row b's logits, finished from the partials.  Thread t owns ids t, t + 1024, ...; the wave
// butterfly and the 16 waves in order fix the order of every reduction from V alone.  TS: the best text id, the best timestamp id
// and logsumexp(timestamps) in one pass; a closed id does not compete.  Plain: the logits are stored where `logits` is given, a
// masked id competes as -inf at its own index, and false is returned before any reduction where pick is 0.  Thread 0 leaves the
// greedy id `arg` (>= V: nothing competed, a row of NaN), its logit `top`, and `force`: logsumexp(timestamps) > max(text), the
// timestamps' summed probability beats every text id (no normaliser is needed) and the id is the best timestamp
struct Sweep { int arg; float top; bool force; };
template <bool TS>
__device__ __forceinline__ bool tail_first_sweep(const PickP& p, const RuleP& r, const Ranges& g, int b, Sweep& out) {
    __shared__ float tv[16], sv[TS ? 16 : 1], mv[TS ? 16 : 1], lv[TS ? 16 : 1];
    __shared__ int ti[16], si[TS ? 16 : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = p.V;
    float bt = -INFINITY, bs = -INFINITY, m = -INFINITY, s = 0.f;
    int at = 0x7fffffff, as = 0x7fffffff;
    for (int v = tid; v < V; v += 1024) {
        if constexpr (TS) {
            if (!open_id<true>(p, r, g, v)) continue;
            const float x = finished(p.P, p.KS, p.ss, (long)b * V + v, nullptr, 0);
            if (v < r.tb) better(bt, at, x, v);
            else { better(bs, as, x, v); lse_join(m, s, x, 1.f); }
        } else {
            float x = finished(p.P, p.KS, p.ss, (long)b * V + v, nullptr, 0);
            if (p.logits) p.logits[(long)b * p.ldl + v] = x;
            if (!open_id<false>(p, r, g, v)) x = -INFINITY;
            better(bt, at, x, v);
        }
    }
    if constexpr (!TS)
        if (!p.pick) return false;
    for (int o = 32; o > 0; o >>= 1) {
        better(bt, at, __shfl_xor(bt, o), __shfl_xor(at, o));
        if constexpr (TS) {
            better(bs, as, __shfl_xor(bs, o), __shfl_xor(as, o));
            lse_join(m, s, __shfl_xor(m, o), __shfl_xor(s, o));
        }
    }
    if (lane == 0) {
        tv[wave] = bt; ti[wave] = at;
        if constexpr (TS) { sv[wave] = bs; si[wave] = as; mv[wave] = m; lv[wave] = s; }
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w) {
            better(bt, at, tv[w], ti[w]);
            if constexpr (TS) { better(bs, as, sv[w], si[w]); lse_join(m, s, mv[w], lv[w]); }
        }
        out = Sweep{at, bt, false};
        if constexpr (TS) {
            out.force = m + logf(s) > bt;
            if (out.force) { out.arg = as; out.top = bs; }
            else better(out.top, out.arg, bs, as);
        }
    }
    return true;
}

// row blockIdx.x: the first sweep in its plain form (the logits stored where `logits` is given); pick: the id of this step and the
// bookkeeping; next_pos >= 0: h = embed_tokens[id] + embed_positions[next_pos]
__global__ __launch_bounds__(1024) void wsp_pick_kernel(const PickP p) {
    __shared__ int chosen;
    const int b = blockIdx.x;
    Sweep w{};
    if (!tail_first_sweep<false>(p, RuleP{}, row_ranges<false>(p, RuleP{}, b), b, w)) return;
    pick_commit(p, b, w.arg, &chosen, 0, nullptr, nullptr);
}

// row blockIdx.x, as wsp_pick_kernel with the rule of WhisperTimeStampLogitsProcessor between the masks and the argmax
__global__ __launch_bounds__(1024) void wsp_pick_ts_kernel(const PickTsP q) {
    __shared__ int chosen;
    const int b = blockIdx.x;
    Sweep w{};
    tail_first_sweep<true>(q.k, q.r, row_ranges<true>(q.k, q.r, b), b, w);
    pick_commit(q.k, b, w.arg, &chosen, q.r.tb, q.r.last_ts, q.r.n_new);
}

// ------------------------------------------------------------------------------------------------------------ policy step tail
// The tail of decoding under a DecodingPolicy (temperature fallback with the log-prob statistics), plain (TS false) and under the
// timestamp rule.  Sweep 1 is tail_first_sweep, the body of wsp_pick_kernel / wsp_pick_ts_kernel: the rule's decision and at T = 0
// the id are theirs because the code is.  It fixes the surviving ids and their maximum M.
// Sweep 2 (the row now sits in L2) sums exp(x - M) over the survivors in fp64 - a thread's ids
// in order, the wave butterfly, the 16 waves in order: fixed by V alone - and at T > 0 takes the argmax of x / T + g, lowest index on
// ties, g = -log(-log(u)) the Gumbel noise of id v: u = (w + 0.5) 2^-32, w word v & 3 of Philox4x32-10 at counter (v >> 2, step,
// attempt + 16 seek, row key) under the key (seed low, seed high).  The chosen id's log-probability x - M - log(sum) is added to the
// row's sum_lp and one to n_scored unless the row had finished; the bookkeeping is pick_commit's.
struct RowKeys { uint32_t key[WB], c2[WB]; };
struct PolP { PickP k; RuleP r; double T; uint32_t k0, k1; RowKeys rk; double* sum_lp; int* n_scored; };

__device__ __forceinline__ uint32_t philox_word(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, int word) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return word == 0 ? c0 : word == 1 ? c1 : word == 2 ? c2 : c3;
}

__device__ __forceinline__ void better64(double& v, int& i, double ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

template <bool TS>
__global__ __launch_bounds__(1024) void wsp_pick_policy_kernel(const PolP q) {
    __shared__ int di[16];
    __shared__ double dv[16], ds[16];
    __shared__ int chosen, s_force, s_arg, s_fin;
    __shared__ float s_max;
    __shared__ double s_lse;
    const PickP& p = q.k;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x, V = p.V, tb = TS ? q.r.tb : V;
    const Ranges g = row_ranges<TS>(p, q.r, b);
    Sweep w{};
    tail_first_sweep<TS>(p, q.r, g, b, w);
    if (tid == 0) { s_force = w.force; s_arg = w.arg; s_max = w.top; s_fin = p.finished[b]; }
    __syncthreads();
    const bool force = s_force != 0, sample = q.T > 0.0;
    const double M = (double)s_max;
    const uint32_t c1 = (uint32_t)p.step, c2 = q.rk.c2[b], c3 = q.rk.key[b];
    double sum = 0.0, best = -INFINITY;
    int arg = 0x7fffffff;
    for (int v = tid; v < V; v += 1024) {
        if (!open_id<TS>(p, q.r, g, v) || (force && v < tb)) continue;
        const double x = (double)finished(p.P, p.KS, p.ss, (long)b * V + v, nullptr, 0);
        sum += exp(x - M);
        if (sample) {
            const double u = ((double)philox_word((uint32_t)v >> 2, c1, c2, c3, q.k0, q.k1, v & 3) + 0.5) * 0x1p-32;
            better64(best, arg, x / q.T - log(-log(u)), v);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o);
        better64(best, arg, __shfl_xor(best, o), __shfl_xor(arg, o));
    }
    if (lane == 0) { ds[wave] = sum; dv[wave] = best; di[wave] = arg; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w) { sum += ds[w]; better64(best, arg, dv[w], di[w]); }
        s_lse = M + log(sum);
        if (!sample) arg = s_arg;
    }
    pick_commit(p, b, arg, &chosen, TS ? tb : 0, TS ? q.r.last_ts : nullptr, TS ? q.r.n_new : nullptr);
    if (tid == 0 && !s_fin) {
        q.sum_lp[b] += (double)finished(p.P, p.KS, p.ss, (long)b * V + chosen, nullptr, 0) - s_lse;
        q.n_scored[b] += 1;
    }
}

// The no-speech probe: row blockIdx.x's unprocessed logits (the partials of the output projection at prompt position 0) -> the fp64
// softmax at id `ns`.  The maximum is exact, the sum runs in the policy tail's order
struct ProbeP { const float* P; int KS; long ss; int V, ns; double* out; };
__global__ __launch_bounds__(1024) void wsp_nospeech_kernel(const ProbeP p) {
    __shared__ float mv[16];
    __shared__ double ds[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    float m = -INFINITY;
    for (int v = tid; v < p.V; v += 1024) m = fmaxf(m, finished(p.P, p.KS, p.ss, (long)b * p.V + v, nullptr, 0));
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) mv[wave] = m;
    __syncthreads();
    for (int w = 0; w < 16; ++w) m = fmaxf(m, mv[w]);
    double sum = 0.0;
    for (int v = tid; v < p.V; v += 1024) sum += exp((double)finished(p.P, p.KS, p.ss, (long)b * p.V + v, nullptr, 0) - (double)m);
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) ds[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w) sum += ds[w];
        p.out[b] = exp((double)finished(p.P, p.KS, p.ss, (long)b * p.V + p.ns, nullptr, 0) - (double)m) / sum;
    }
}

// ------------------------------------------------------------------------------------------------------------ beam step tail
constexpr int KMAX = DEX_WHISPER_MAX_BEAMS;

constexpr int BCH = 2048, BPT = BCH / 256;      // ids per scan workgroup, and per thread of it
int beam_chunks(int V) { return (V + BCH - 1) / BCH; }

// The tail is three launches.  C = beam_chunks(V) chunks per row.  lg (or null where P is the logits, KS = 1): the finished fp32
// logits [U K][V].  part [U K][C][2] fp64: a chunk's maximum and sum exp(x - maximum).  cand_s (fp64) / cand_f [U K][C][2K]: a
// chunk's 2K best scores in order and their flat indices r V + id (-1: nothing was left).  div = (step + 1)^length_penalty.  tok /
// par / trace (or null): the step's new running set.  next_pos >= 0: h = embed_tokens + embed_positions of every row's next input
struct BeamP { const float* P; int KS; long ss; int V, K, C; const uint8_t* mask; float* lg; double *part, *cand_s; int* cand_f;
               int eos, step, pos, last; double div; DexWhisperBeamState s; int *tok, *par; double* trace;
               const float *emb, *posw; int d, next_pos; float* h; };

// chunk blockIdx.x of row blockIdx.y: the logits finished from the partials (stored where lg is given), the chunk's maximum and its
// sum exp(x - maximum) in fp64: per thread in id order, the wave butterfly, the four waves in order
__global__ __launch_bounds__(256) void wsp_beam_lse_kernel(const BeamP p) {
    __shared__ float rm[4];
    __shared__ double rs[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = blockIdx.x, row = blockIdx.y, V = p.V;
    if (p.s.done[row / p.K]) return;
    const long at = (long)row * V;
    float x[BPT], m = -INFINITY;
#pragma unroll
    for (int e = 0; e < BPT; ++e) {
        const int v = c * BCH + e * 256 + tid;
        x[e] = v < V ? finished(p.P, p.KS, p.ss, at + v, nullptr, 0) : -INFINITY;
        if (v < V && p.lg) p.lg[at + v] = x[e];
        m = fmaxf(m, x[e]);
    }
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) rm[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(rm[0], rm[1]), fmaxf(rm[2], rm[3]));
    double sum = 0.0;
#pragma unroll
    for (int e = 0; e < BPT; ++e)
        if (c * BCH + e * 256 + tid < V && m > -INFINITY) sum += exp((double)x[e] - (double)m);
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) rs[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        double* o = p.part + ((long)row * p.C + c) * 2;
        o[0] = (double)m; o[1] = ((rs[0] + rs[1]) + rs[2]) + rs[3];
    }
}

// chunk blockIdx.x of row blockIdx.y: the row's log-softmax normaliser from its chunks in chunk order (every workgroup of the row
// computes the same), score = running + (x - normaliser) in fp64 of the chunk's unmasked ids in registers, and 2K rounds of the
// block-wide best in the order (score descending, flat index ascending): the chunk's 2K best, of which the row's, and the
// utterance's, 2K best are a subset
__global__ __launch_bounds__(256) void wsp_beam_top_kernel(const BeamP p) {
    __shared__ double rs[4], lse;
    __shared__ int ri[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = blockIdx.x, row = blockIdx.y, V = p.V, T = 2 * p.K;
    if (p.s.done[row / p.K]) return;
    if (tid == 0) {
        const double* q = p.part + (long)row * p.C * 2;
        double M = -INFINITY, t = 0.0;
        for (int i = 0; i < p.C; ++i) M = fmax(M, q[2 * i]);
        for (int i = 0; i < p.C; ++i)
            if (q[2 * i] > -INFINITY) t += q[2 * i + 1] * exp(q[2 * i] - M);
        lse = M + log(t);
    }
    __syncthreads();
    const float* lg = (p.lg ? p.lg : p.P) + (long)row * V;
    const double base = p.s.run_score[row], nrm = lse;
    const int f0 = (row % p.K) * V;
    double sc[BPT];
#pragma unroll
    for (int e = 0; e < BPT; ++e) {
        const int v = c * BCH + e * 256 + tid;
        sc[e] = v < V && !(p.mask && p.mask[v]) ? base + ((double)lg[v] - nrm) : -INFINITY;          // -inf (and NaN) never competes
    }
    unsigned taken = 0;
    double* os = p.cand_s + ((long)row * p.C + c) * T;
    int* of = p.cand_f + ((long)row * p.C + c) * T;
    for (int j = 0; j < T; ++j) {
        double best = -INFINITY;
        int arg = 0x7fffffff, be = -1;
#pragma unroll
        for (int e = 0; e < BPT; ++e) {
            const int flat = f0 + c * BCH + e * 256 + tid;
            if (!((taken >> e) & 1) && (sc[e] > best || (sc[e] == best && flat < arg))) { best = sc[e]; arg = flat; be = e; }
        }
        const int mine = arg;
        for (int o = 32; o > 0; o >>= 1) { const double ov = __shfl_xor(best, o); const int oi = __shfl_xor(arg, o); better64(best, arg, ov, oi); }
        if (lane == 0) { rs[wave] = best; ri[wave] = arg; }
        __syncthreads();
        best = rs[0]; arg = ri[0];
        for (int w = 1; w < 4; ++w) better64(best, arg, rs[w], ri[w]);
        if (be >= 0 && mine == arg) taken |= 1u << be;
        if (tid == 0) { os[j] = best; of[j] = arg == 0x7fffffff ? -1 : arg; }
        __syncthreads();
    }
}

// Utterance blockIdx.x (whisper.py states the rule).  2K rounds over the utterance's K x C x 2K chunk candidates, each the block-wide
// best among those that come after the previous round's winner in the order (score descending, flat index ascending): the 2K
// candidates in order, ties to the lowest flat index.  Thread 0 then walks them (running set, pool merge through the slot order, the
// stop), and all threads gather the sequences and the ancestry by parent into the _out buffers, copy the pooled hypotheses into
// their slots and gather the next step's embedding rows.  A done utterance only carries its state across
__global__ __launch_bounds__(1024) void wsp_beam_pick_kernel(const BeamP p) {
    __shared__ double rs[16], cs[2 * KMAX], nsc[KMAX];
    __shared__ int ri[16], cf[2 * KMAX], npar[KMAX], nid[KMAX], pslot[KMAX], ppar[KMAX], pid[KMAX], n_pool, frozen;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = blockIdx.x, K = p.K, V = p.V, r0 = u * K;
    const DexWhisperBeamState& s = p.s;
    if (tid == 0) { frozen = s.done[u] != 0; n_pool = 0; }
    __syncthreads();
    if (!frozen) {
        const int n = K * p.C * 2 * K;
        const double* qs = p.cand_s + (long)r0 * p.C * 2 * K;
        const int* qf = p.cand_f + (long)r0 * p.C * 2 * K;
        for (int c = 0; c < 2 * K; ++c) {
            const double ps = c ? cs[c - 1] : 0.0;
            const int pf = c ? cf[c - 1] : -1;
            double best = -INFINITY;
            int arg = 0x7fffffff;
            if (c == 0 || pf >= 0) {
                for (int i = tid; i < n; i += 1024) {
                    const int flat = qf[i];
                    const double sc = qs[i];
                    if (flat < 0 || (c && !(sc < ps || (sc == ps && flat > pf)))) continue;
                    better64(best, arg, sc, flat);
                }
            }
            for (int o = 32; o > 0; o >>= 1) { const double ov = __shfl_xor(best, o); const int oi = __shfl_xor(arg, o); better64(best, arg, ov, oi); }
            if (lane == 0) { rs[wave] = best; ri[wave] = arg; }
            __syncthreads();
            if (tid == 0) {
                for (int w = 1; w < 16; ++w) better64(best, arg, rs[w], ri[w]);
                cs[c] = best; cf[c] = arg == 0x7fffffff ? -1 : arg;          // -1: nothing is left to compete
            }
            __syncthreads();
        }
        if (tid == 0) {
            int pn = s.pool_n[u], nr = 0, order[KMAX];
            for (int t = 0; t < pn; ++t) order[t] = s.pool_order[r0 + t];
            for (int c = 0; c < 2 * K; ++c) {
                if (cf[c] < 0) continue;
                const int r = cf[c] / V, id = cf[c] - r * V;
                if (!p.last && id != p.eos) {
                    if (nr < K) { npar[nr] = r; nid[nr] = id; nsc[nr] = cs[c]; ++nr; }
                    continue;
                }
                if (c >= K) continue;                                        // a finished candidate of rank >= K is dropped
                const double sc = cs[c] / p.div;
                int t = 0;
                while (t < pn && !(s.pool_score[r0 + order[t]] < sc)) ++t;  // behind every entry that is at least as good
                if (t >= K) continue;
                const int slot = pn < K ? pn : order[K - 1];
                for (int x = pn < K ? pn : K - 1; x > t; --x) order[x] = order[x - 1];
                order[t] = slot;
                if (pn < K) ++pn;
                s.pool_score[r0 + slot] = sc;
                s.pool_len[r0 + slot] = id == p.eos ? p.step : p.step + 1;
                pslot[n_pool] = slot; ppar[n_pool] = r; pid[n_pool] = id; ++n_pool;
            }
            for (int t = 0; t < pn; ++t) s.pool_order[r0 + t] = order[t];
            s.pool_n[u] = pn;
            bool done = p.last != 0;
            if (!p.last) {
                for (; nr < K; ++nr) { npar[nr] = nr; nid[nr] = p.eos; nsc[nr] = -INFINITY; }      // only where nothing was left to compete
                for (int x = 0; x < K; ++x) {
                    s.run_score[r0 + x] = nsc[x];
                    if (p.tok) { p.tok[r0 + x] = nid[x]; p.par[r0 + x] = npar[x]; }
                    if (p.trace) p.trace[r0 + x] = nsc[x];
                }
                done = pn == K && nsc[0] / p.div <= s.pool_score[r0 + order[K - 1]];
            } else {
                frozen = 1;
            }
            if (done) { s.done[u] = 1; atomicAdd(s.count, 1); }
        }
        __syncthreads();
    }
    const int ls = s.ld_seq, la = s.ld_anc;
    for (int x = 0; x < K; ++x) {
        const int par = frozen ? x : npar[x];
        const int* si = s.seq_in + (long)(r0 + par) * ls;
        const int* ai = s.anc_in + (long)(r0 + par) * la;
        int* so = s.seq_out + (long)(r0 + x) * ls;
        int* ao = s.anc_out + (long)(r0 + x) * la;
        if (frozen) {
            for (int t = tid; t < ls; t += 1024) so[t] = si[t];
            for (int t = tid; t < la; t += 1024) ao[t] = ai[t];
        } else {
            for (int t = tid; t < ls; t += 1024) so[t] = t < p.step ? si[t] : (t == p.step ? nid[x] : p.eos);
            for (int t = tid; t < la; t += 1024) ao[t] = t <= p.pos ? ai[t] : x;
        }
    }
    for (int e = 0; e < n_pool; ++e) {
        const int* si = s.seq_in + (long)(r0 + ppar[e]) * ls;
        int* po = s.pool_ids + (long)(r0 + pslot[e]) * ls;
        for (int t = tid; t < ls; t += 1024) po[t] = t < p.step ? si[t] : (t == p.step ? pid[e] : p.eos);
    }
    if (p.next_pos < 0) return;
    const float* q = p.posw + (long)p.next_pos * p.d;
    for (int x = 0; x < K; ++x) {
        const float* e = p.emb + (long)(frozen ? p.eos : nid[x]) * p.d;
        for (int c = tid; c < p.d; c += 1024) p.h[(long)(r0 + x) * p.d + c] = e[c] + q[c];
    }
}

// the state before the first step: identity ancestry in both buffers, running scores 0, -1e9, ..., empty pools, nothing done
__global__ __launch_bounds__(256) void wsp_beam_init_kernel(const DexWhisperBeamState s, int U, int K) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x, rows = (long)U * K;
    if (i < rows * s.ld_anc) { const int r = (int)(i / s.ld_anc); s.anc_in[i] = r % K; s.anc_out[i] = r % K; }
    if (i < rows) { s.run_score[i] = i % K ? -1e9 : 0.0; s.pool_score[i] = -INFINITY; s.pool_len[i] = 0; s.pool_order[i] = (int)(i % K); }
    if (i < U) { s.pool_n[i] = 0; s.done[i] = 0; }
    if (i == 0) *s.count = 0;
}

// The best pooled hypothesis of utterance blockIdx.x -> ids [U][max_new] (eos behind it), lengths, scores; pool_* (or null): the
// pool best first, ids [U K][max_new]
struct BeamOutP { DexWhisperBeamState s; int K, eos, max_new; int *ids, *lengths; double* scores; int *pool_ids, *pool_len; double* pool_scores; int* pool_n; };
__global__ __launch_bounds__(256) void wsp_beam_result_kernel(const BeamOutP p) {
    const int u = blockIdx.x, r0 = u * p.K, pn = p.s.pool_n[u], tid = threadIdx.x;
    for (int k = 0; k < p.K; ++k) {
        if (k && !p.pool_ids) break;
        const int slot = k < pn ? p.s.pool_order[r0 + k] : -1;
        const int* src = slot >= 0 ? p.s.pool_ids + (long)(r0 + slot) * p.s.ld_seq : nullptr;
        for (int t = tid; t < p.max_new; t += 256) {
            const int id = src && t < p.s.ld_seq ? src[t] : p.eos;
            if (k == 0) p.ids[(long)u * p.max_new + t] = id;
            if (p.pool_ids) p.pool_ids[(long)(r0 + k) * p.max_new + t] = id;
        }
        if (tid == 0) {
            const int len = slot >= 0 ? p.s.pool_len[r0 + slot] : 0;
            const double sc = slot >= 0 ? p.s.pool_score[r0 + slot] : -INFINITY;
            if (k == 0) { p.lengths[u] = len; p.scores[u] = sc; }
            if (p.pool_ids) { p.pool_len[r0 + k] = len; p.pool_scores[r0 + k] = sc; }
        }
    }
    if (tid == 0 && p.pool_n) p.pool_n[u] = pn;
}

// h[b] = embed_tokens[id] + embed_positions[pos], id = ids[b ld + pos] (clamped into the vocabulary) or, ids null, `id`
__global__ __launch_bounds__(256) void wsp_embed_kernel(const int* ids, int ld, int id, int pos, int V, const float* emb, const float* posw, int d, float* h) {
    const int b = blockIdx.x;
    if (ids) id = ids[(long)b * ld + pos];
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);
    for (int c = threadIdx.x; c < d; c += 256) h[(long)b * d + c] = emb[(long)id * d + c] + posw[(long)pos * d + c];
}

__global__ __launch_bounds__(256) void wsp_fill_kernel(int* dst, long n, int v) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = v;
}

// ------------------------------------------------------------------------------------------------------------ host: tables
void mel_filters(int n_mels, double* out) {
    const double logstep = 27.0 / std::log(6.4);
    auto hz2mel = [&](double f) { return f >= 1000.0 ? 15.0 + std::log(f / 1000.0) * logstep : 3.0 * f / 200.0; };
    auto mel2hz = [&](double m) { return m >= 15.0 ? 1000.0 * std::exp((std::log(6.4) / 27.0) * (m - 15.0)) : 200.0 * m / 3.0; };
    const double lo = hz2mel(0.0), hi = hz2mel(8000.0), step = (hi - lo) / (n_mels + 1);
    std::vector<double> ff(n_mels + 2);
    for (int i = 0; i < n_mels + 2; ++i) ff[i] = mel2hz(i == n_mels + 1 ? hi : lo + i * step);
    for (int k = 0; k < NBIN; ++k) {
        const double f = k == NBIN - 1 ? 8000.0 : k * (8000.0 / (NBIN - 1));
        for (int m = 0; m < n_mels; ++m) {
            const double down = -(ff[m] - f) / (ff[m + 1] - ff[m]), up = (ff[m + 2] - f) / (ff[m + 2] - ff[m + 1]);
            const double v = down < up ? down : up;
            out[(long)k * n_mels + m] = (v > 0.0 ? v : 0.0) * (2.0 / (ff[m + 2] - ff[m]));
        }
    }
}

DexWhisperConfig default_config() {
    DexWhisperConfig c;
    std::memset(&c, 0, sizeof c);
    c.vocab_size = 51866; c.num_mel_bins = 128; c.d_model = 1280;
    c.encoder_layers = 32; c.encoder_attention_heads = 20; c.encoder_ffn_dim = 5120;
    c.decoder_layers = 32; c.decoder_attention_heads = 20; c.decoder_ffn_dim = 5120;
    c.max_source_positions = 1500; c.max_target_positions = 448;
    c.scale_embedding = 0; c.activation_gelu = 1;
    return c;
}

// the family that is built; names the first field outside it
int check_config(const DexWhisperConfig& c) {
    if (c.activation_gelu != 1) return create_fail("%s: only 'gelu' (erf) is built", "activation_function");
    if (c.scale_embedding != 0) return create_fail("%s: only False is built", "scale_embedding");
    if (c.num_mel_bins < 1 || c.num_mel_bins > 128) return create_fail("%s: 1 .. 128", "num_mel_bins");
    if (c.d_model < 64 || c.d_model % 64 || c.d_model > 8192) return create_fail("%s: a multiple of 64 in 64 .. 8192", "d_model");
    if (c.encoder_attention_heads * 64 != c.d_model) return create_fail("%s: d_model / encoder_attention_heads must be 64", "encoder_attention_heads");
    if (c.decoder_attention_heads * 64 != c.d_model) return create_fail("%s: d_model / decoder_attention_heads must be 64", "decoder_attention_heads");
    if (c.encoder_layers < 1 || c.encoder_layers > 64) return create_fail("%s: 1 .. 64", "encoder_layers");
    if (c.decoder_layers < 1 || c.decoder_layers > 64) return create_fail("%s: 1 .. 64", "decoder_layers");
    if (c.encoder_ffn_dim < 64 || c.encoder_ffn_dim % 64 || c.encoder_ffn_dim > 65536) return create_fail("%s: a multiple of 64 up to 65536", "encoder_ffn_dim");
    if (c.decoder_ffn_dim < 64 || c.decoder_ffn_dim % 64 || c.decoder_ffn_dim > 65536) return create_fail("%s: a multiple of 64 up to 65536", "decoder_ffn_dim");
    if (c.vocab_size < 2 || c.vocab_size > (1 << 20)) return create_fail("%s: 2 .. 1048576", "vocab_size");
    if (c.max_source_positions < 1 || c.max_source_positions > MAX_KEYS) return create_fail("%s: 1 .. 4096", "max_source_positions");
    if (c.max_target_positions < 1 || c.max_target_positions > MAX_KEYS) return create_fail("%s: 1 .. 4096", "max_target_positions");
    return DEX_OK;
}

}  // namespace

struct DexWhisper : dex::WeightStore {
    DexWhisper() : WeightStore("whisper ") {}
    DexWhisperConfig c;
    struct DecLayer { const float *ln1g, *ln1b, *wqkv, *bq, *bv, *wo, *bo, *ln2g, *ln2b, *wcq, *bcq, *wckv, *bckv, *wco, *bco,
                      *ln3g, *ln3b, *w1, *b1, *w2, *b2; };
    const float *conv1_w = nullptr, *conv1_b = nullptr, *conv2_w = nullptr, *conv2_b = nullptr, *enc_pos = nullptr, *enc_g = nullptr, *enc_be = nullptr;
    const float *emb = nullptr, *embT = nullptr, *dec_pos = nullptr, *dec_g = nullptr, *dec_be = nullptr;
    std::vector<TrunkWeights::Layer> enc;      // ln1 = self_attn_layer_norm, ln2 = final_layer_norm
    std::vector<DecLayer> dec;
    std::vector<double> tab_host;            // window | cos | sin | mel matrix
    double* tab_dev = nullptr;
    int mel_pad() const { return (c.num_mel_bins + 31) / 32 * 32; }
    int vocab_pad() const { return (c.vocab_size + 63) / 64 * 64; }
};

namespace {

const std::string ENC = "model.encoder.", DEC = "model.decoder.";
std::string ek(int l, const char* what) { return ENC + "layers." + std::to_string(l) + "." + what; }
std::string dk(int l, const char* what) { return DEC + "layers." + std::to_string(l) + "." + what; }

void add_attn(DexWhisper* s, const std::string& p, int d) {
    s->add(p + "k_proj.weight", {d, d});
    s->add(p + "v_proj.weight", {d, d}); s->add(p + "v_proj.bias", {d});
    s->add(p + "q_proj.weight", {d, d}); s->add(p + "q_proj.bias", {d});
    s->add(p + "out_proj.weight", {d, d}); s->add(p + "out_proj.bias", {d});
}
void add_ln(DexWhisper* s, const std::string& p, int d) { s->add(p + ".weight", {d}); s->add(p + ".bias", {d}); }

// HF's own order (WhisperForConditionalGeneration.state_dict() without proj_out.weight, which is the token embedding)
void register_keys(DexWhisper* s) {
    const DexWhisperConfig& c = s->c;
    const int d = c.d_model;
    s->add(ENC + "conv1.weight", {d, c.num_mel_bins, 3}); s->add(ENC + "conv1.bias", {d});
    s->add(ENC + "conv2.weight", {d, d, 3}); s->add(ENC + "conv2.bias", {d});
    s->add(ENC + "embed_positions.weight", {c.max_source_positions, d});
    for (int l = 0; l < c.encoder_layers; ++l) {
        add_attn(s, ek(l, "self_attn."), d); add_ln(s, ek(l, "self_attn_layer_norm"), d);
        s->add(ek(l, "fc1.weight"), {c.encoder_ffn_dim, d}); s->add(ek(l, "fc1.bias"), {c.encoder_ffn_dim});
        s->add(ek(l, "fc2.weight"), {d, c.encoder_ffn_dim}); s->add(ek(l, "fc2.bias"), {d});
        add_ln(s, ek(l, "final_layer_norm"), d);
    }
    add_ln(s, ENC + "layer_norm", d);
    s->add(DEC + "embed_tokens.weight", {c.vocab_size, d});
    s->add(DEC + "embed_positions.weight", {c.max_target_positions, d});
    for (int l = 0; l < c.decoder_layers; ++l) {
        add_attn(s, dk(l, "self_attn."), d); add_ln(s, dk(l, "self_attn_layer_norm"), d);
        add_attn(s, dk(l, "encoder_attn."), d); add_ln(s, dk(l, "encoder_attn_layer_norm"), d);
        s->add(dk(l, "fc1.weight"), {c.decoder_ffn_dim, d}); s->add(dk(l, "fc1.bias"), {c.decoder_ffn_dim});
        s->add(dk(l, "fc2.weight"), {d, c.decoder_ffn_dim}); s->add(dk(l, "fc2.bias"), {d});
        add_ln(s, dk(l, "final_layer_norm"), d);
    }
    add_ln(s, DEC + "layer_norm", d);
}

int pack_all(DexWhisper* s, hipStream_t st) {
    const DexWhisperConfig& c = s->c;
    const int d = c.d_model;
    s->conv1_w = dex::conv1d_operand(*s, s->R(ENC + "conv1.weight"), c.num_mel_bins, d, 3, s->mel_pad(), st); s->conv1_b = s->R(ENC + "conv1.bias");
    s->conv2_w = pack(s, ENC + "conv2.weight", 1, d, d, 3, nullptr, st); s->conv2_b = s->R(ENC + "conv2.bias");
    s->enc_pos = s->R(ENC + "embed_positions.weight");
    s->enc_g = s->R(ENC + "layer_norm.weight"); s->enc_be = s->R(ENC + "layer_norm.bias");
    s->enc.assign(c.encoder_layers, TrunkWeights::Layer{});
    for (int l = 0; l < c.encoder_layers && s->alloc_rc == DEX_OK; ++l) {
        TrunkWeights::Layer& L = s->enc[l];
        L.wqkv = pack_side(s, ek(l, "self_attn."), {"q_proj", "k_proj", "v_proj"}, d, st, &L.bqkv);
        L.wo = pack(s, ek(l, "self_attn.out_proj.weight"), 1, d, d, 1, nullptr, st); L.bo = s->R(ek(l, "self_attn.out_proj.bias"));
        L.ln1g = s->R(ek(l, "self_attn_layer_norm.weight")); L.ln1b = s->R(ek(l, "self_attn_layer_norm.bias"));
        L.w1 = pack(s, ek(l, "fc1.weight"), 1, c.encoder_ffn_dim, d, 1, nullptr, st); L.b1 = s->R(ek(l, "fc1.bias"));
        L.w2 = pack(s, ek(l, "fc2.weight"), 1, d, c.encoder_ffn_dim, 1, nullptr, st); L.b2 = s->R(ek(l, "fc2.bias"));
        L.ln2g = s->R(ek(l, "final_layer_norm.weight")); L.ln2b = s->R(ek(l, "final_layer_norm.bias"));
    }
    s->emb = s->R(DEC + "embed_tokens.weight"); s->dec_pos = s->R(DEC + "embed_positions.weight");
    s->dec_g = s->R(DEC + "layer_norm.weight"); s->dec_be = s->R(DEC + "layer_norm.bias");
    {
        const int Vp = s->vocab_pad();
        float* t = s->alloc((long)d * Vp);
        if (t) {
            hipMemsetAsync(t, 0, (size_t)d * Vp * sizeof(float), st);
            pack_into(s->emb, t, 1, c.vocab_size, d, 1, Vp, 0, nullptr, st);
        }
        s->embT = t;
    }
    s->dec.assign(c.decoder_layers, DexWhisper::DecLayer{});
    for (int l = 0; l < c.decoder_layers && s->alloc_rc == DEX_OK; ++l) {
        DexWhisper::DecLayer& L = s->dec[l];
        L.wqkv = pack_side(s, dk(l, "self_attn."), {"q_proj", "k_proj", "v_proj"}, d, st, nullptr);
        L.bq = s->R(dk(l, "self_attn.q_proj.bias")); L.bv = s->R(dk(l, "self_attn.v_proj.bias"));
        L.wo = pack(s, dk(l, "self_attn.out_proj.weight"), 1, d, d, 1, nullptr, st); L.bo = s->R(dk(l, "self_attn.out_proj.bias"));
        L.ln1g = s->R(dk(l, "self_attn_layer_norm.weight")); L.ln1b = s->R(dk(l, "self_attn_layer_norm.bias"));
        L.wcq = pack(s, dk(l, "encoder_attn.q_proj.weight"), 1, d, d, 1, nullptr, st); L.bcq = s->R(dk(l, "encoder_attn.q_proj.bias"));
        L.wckv = pack_side(s, dk(l, "encoder_attn."), {"k_proj", "v_proj"}, d, st, &L.bckv);
        L.wco = pack(s, dk(l, "encoder_attn.out_proj.weight"), 1, d, d, 1, nullptr, st); L.bco = s->R(dk(l, "encoder_attn.out_proj.bias"));
        L.ln2g = s->R(dk(l, "encoder_attn_layer_norm.weight")); L.ln2b = s->R(dk(l, "encoder_attn_layer_norm.bias"));
        L.w1 = pack(s, dk(l, "fc1.weight"), 1, c.decoder_ffn_dim, d, 1, nullptr, st); L.b1 = s->R(dk(l, "fc1.bias"));
        L.w2 = pack(s, dk(l, "fc2.weight"), 1, d, c.decoder_ffn_dim, 1, nullptr, st); L.b2 = s->R(dk(l, "fc2.bias"));
        L.ln3g = s->R(dk(l, "final_layer_norm.weight")); L.ln3b = s->R(dk(l, "final_layer_norm.bias"));
    }
    return DEX_OK;
}

// workspace (floats, every piece a multiple of 64): logspec (fp64) [B][T][n_mels] | mel [B][T][Mp] | c1 [B][T][d] | he, ye [B][S][d]
// | qkv [B][S][3d] | ffe [B][S][ffn_e] | enc [B][S][d] | ckv [Ld][B][S][2d] | ck, cv [Ld][B][Tmax][d] | h, y, a [B][d] | ff [B][ffn_d]
// | P (the largest [KS][B][N] of a step) | state (int): finished [B], count, new-token count [B], last timestamp [B]
// the floats per row of the largest [KS][B][N] of a step
long step_partials(const DexWhisperConfig& c) {
    const long d = c.d_model;
    long pn = (long)slabs((int)d) * 3 * d, q = (long)slabs((int)d) * c.decoder_ffn_dim;
    pn = q > pn ? q : pn; q = (long)slabs(c.decoder_ffn_dim) * d;
    pn = q > pn ? q : pn; q = (long)slabs((int)d) * c.vocab_size;
    return q > pn ? q : pn;
}

struct Ws { double* logspec; float *mel, *c1, *he, *ye, *qkv, *ffe, *enc, *ckv, *ck, *cv, *h, *y, *a, *ff, *P; int *fin, *count, *n_new, *last_ts; size_t bytes; };
Ws plan(const DexWhisper* s, void* ws, long B) {
    const DexWhisperConfig& c = s->c;
    const long S = c.max_source_positions, T = 2 * S, d = c.d_model, Tm = c.max_target_positions, Ld = c.decoder_layers;
    Ws w{};
    Taker tk(ws);
    w.logspec = (double*)tk.take(2 * B * T * c.num_mel_bins);
    w.mel = tk.take(B * T * s->mel_pad()); w.c1 = tk.take(B * T * d);
    w.he = tk.take(B * S * d); w.ye = tk.take(B * S * d); w.qkv = tk.take(B * S * 3 * d); w.ffe = tk.take(B * S * c.encoder_ffn_dim);
    w.enc = tk.take(B * S * d);
    w.ckv = tk.take(Ld * B * S * 2 * d); w.ck = tk.take(Ld * B * Tm * d); w.cv = tk.take(Ld * B * Tm * d);
    w.h = tk.take(B * d); w.y = tk.take(B * d); w.a = tk.take(B * d); w.ff = tk.take(B * c.decoder_ffn_dim);
    w.P = tk.take(B * step_partials(c));
    w.fin = (int*)tk.take(3 * B + 64); w.count = w.fin + B; w.n_new = w.count + 1; w.last_ts = w.n_new + B;
    w.bytes = tk.bytes();
    return w;
}

// P = X [B][ldx] (K columns) x W [K][ldw] (N columns); returns the slabs
int skinny(const float* X, int ldx, const float* W, int ldw, int K, int N, float* P, int B, hipStream_t st) {
    const SkP p{X, ldx, W, ldw, K, N, P, B};
    const dim3 grid((N + 63) / 64, slabs(K));
    auto lds = [&](int rb) { return (size_t)(SK_ROWS * rb + 4 * rb * 64) * sizeof(float); };
    if (B == 1) hipLaunchKernelGGL(wsp_skinny_kernel<1>, grid, dim3(256), lds(1), st, p);
    else if (B <= 4) hipLaunchKernelGGL(wsp_skinny_kernel<4>, grid, dim3(256), lds(4), st, p);
    else if (B <= 8) hipLaunchKernelGGL(wsp_skinny_kernel<8>, grid, dim3(256), lds(8), st, p);
    else if (B <= 16) hipLaunchKernelGGL(wsp_skinny_kernel<16>, grid, dim3(256), lds(16), st, p);
    else hipLaunchKernelGGL(wsp_skinny_kernel<32>, grid, dim3(256), lds(32), st, p);
    return grid.y;
}

void finish(const float* P, int KS, int N, const float* bias, const float* res, float* out, int act, const float* g, const float* be, float* y,
            int B, hipStream_t st) {
    const FinP p{P, KS, (long)B * N, N, bias, res, out, act, g, be, y};
    hipLaunchKernelGGL(wsp_finish_kernel, dim3(B), dim3(256), 0, st, p);
}

// log-mel features of rows of any length (the tables are up): logspec fp64 [B][Fmax][n_mels] -> out [B][n_mels][Fmax], F the frames
// of the longest row.  Rows of at most one chunk have the chunk's frames: Fmax = F = those is the one-chunk front end
void enqueue_log_mel(DexWhisper* s, const float* wav, const int32_t* lengths_host, int B, int n, double* logspec, float* out, int F, int Fmax, hipStream_t st) {
    const DexWhisperConfig& c = s->c;
    MelP p{};
    p.wav = wav; p.ld = n; p.T = 2 * c.max_source_positions; p.N = (long)p.T * HOP; p.n_mels = c.num_mel_bins;
    for (int b = 0; b < B; ++b) p.len.a[b] = lengths_host[b];
    p.win = s->tab_dev; p.cs = s->tab_dev + NFFT; p.sn = s->tab_dev + 2 * NFFT; p.filt = s->tab_dev + 3 * NFFT; p.out = logspec;
    hipLaunchKernelGGL(wsp_mel_long_kernel, dim3((F + MELF - 1) / MELF, B), dim3(256), 0, st, p, Fmax);
    hipLaunchKernelGGL(wsp_mel_floor_long_kernel, dim3(B), dim3(1024), 0, st, (const double*)logspec, out, p.len, p.N, p.T, Fmax, p.n_mels);
}

// the window, the twiddles and the mel matrix, on the device from the first front-end call on
int ensure_tables(DexWhisper* s, hipStream_t st) {
    if (s->tab_dev) return DEX_OK;
    const int M = s->c.num_mel_bins;
    s->tab_host.assign(3 * NFFT + (size_t)NBIN * M, 0.0);
    for (int n = 0; n < NFFT; ++n) {
        const double a = 2.0 * M_PI * n / NFFT;
        s->tab_host[n] = 0.5 - 0.5 * std::cos(a); s->tab_host[NFFT + n] = std::cos(a); s->tab_host[2 * NFFT + n] = -std::sin(a);
    }
    mel_filters(M, s->tab_host.data() + 3 * NFFT);
    DEX_HIPCHK(s, hipMalloc((void**)&s->tab_dev, s->tab_host.size() * sizeof(double)));
    DEX_HIPCHK(s, hipMemcpyAsync(s->tab_dev, s->tab_host.data(), s->tab_host.size() * sizeof(double), hipMemcpyHostToDevice, st));
    return DEX_OK;
}

// mark (or null): an event recorded between the encoder and the cross-attention projections
void enqueue_encoder(DexWhisper* s, const float* feat, int B, float* enc_out, const Ws& w, hipStream_t st, hipEvent_t mark = nullptr) {
    const DexWhisperConfig& c = s->c;
    const int S = c.max_source_positions, T = 2 * S, d = c.d_model, Mp = s->mel_pad();
    const long total = (long)B * T * Mp;
    hipLaunchKernelGGL(wsp_feat_cl_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, feat, w.mel, total, T, c.num_mel_bins, Mp);
    gemm(w.mel, Mp, T, Mp, 3, 1, -1, T, s->conv1_w, d, 1, s->conv1_b, w.c1, 1, nullptr, nullptr, B, st);
    gemm(w.c1, d, T, d, 3, 2, -1, S, s->conv2_w, d, 1, s->conv2_b, w.he, 1, s->enc_pos, nullptr, B, st, 1, 1, true);
    const LayerDims ld{d, c.encoder_attention_heads, c.encoder_ffn_dim, 1, LN_EPS};      // fc2 as one launch
    const LayerWs lw{w.he, w.ye, w.qkv, w.ffe, nullptr, S};
    for (const TrunkWeights::Layer& L : s->enc) enqueue_plain_layer<true>(ld, L, lw, nullptr, B, st);
    const long rows = (long)B * S;
    layer_norm<false>(w.he, w.enc, rows, S, d, s->enc_g, s->enc_be, LN_EPS, nullptr, st);
    if (enc_out) hipMemcpyAsync(enc_out, w.enc, (size_t)rows * d * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (mark) hipEventRecord(mark, st);
    for (int l = 0; l < c.decoder_layers; ++l)                                           // the cross-attention k | v, once per utterance
        linear(w.enc, d, s->dec[l].wckv, 2 * d, s->dec[l].bckv, w.ckv + (long)l * B * S * 2 * d, 0, nullptr, nullptr, S, B, st);
}

// the beams of a step: B = U x K rows, row u K + r beam r of utterance u; the cross K / V is per utterance, the self-attention
// cache is read through the ancestry anc [B][ld_anc]
struct BeamAt { int U, K; const int* anc; int ld_anc; };

void attend_cross_beam(const AtP& x, int H, const BeamAt& bm, hipStream_t st) {
    const dim3 grid(H, bm.U);
    const size_t lds = (size_t)bm.K * x.n * sizeof(float);
    switch (bm.K) {
#define DEX_BEAM_CASE(k) case k: hipLaunchKernelGGL(wsp_attend_cross_beam_kernel<k>, grid, dim3(256), lds, st, x); break;
        DEX_BEAM_CASE(2) DEX_BEAM_CASE(3) DEX_BEAM_CASE(4) DEX_BEAM_CASE(5) DEX_BEAM_CASE(6) DEX_BEAM_CASE(7) DEX_BEAM_CASE(8)
#undef DEX_BEAM_CASE
    }
}

// the rows of a step that decodes some rows of an encoded batch: row b's cross K / V is row `row.a[b]` of the `encoded` rows' layout
struct CrossRows { int encoded; Lens row; };

// one decoder position: w.h holds embed_tokens + embed_positions of position p; logits: leaves the partials of the logits in w.P
// and returns their slabs.  bm: the step of U x K beams (the two attention launches take their beam forms)
int enqueue_step(DexWhisper* s, int p, int B, const Ws& w, hipStream_t st, bool logits = true, const BeamAt* bm = nullptr, const CrossRows* cr = nullptr) {
    const DexWhisperConfig& c = s->c;
    const int d = c.d_model, H = c.decoder_attention_heads, S = c.max_source_positions, Tm = c.max_target_positions, F = c.decoder_ffn_dim;
    finish(nullptr, 0, d, nullptr, w.h, w.h, 0, s->dec[0].ln1g, s->dec[0].ln1b, w.y, B, st);
    for (int l = 0; l < c.decoder_layers; ++l) {
        const DexWhisper::DecLayer& L = s->dec[l];
        int ks = skinny(w.y, d, L.wqkv, 3 * d, d, 3 * d, w.P, B, st);
        AtP a{};
        a.q = w.P; a.kn = w.P + d; a.vn = w.P + 2 * d; a.KS = ks; a.ss = (long)B * 3 * d; a.ldq = 3 * d; a.qbias = L.bq; a.kbias = nullptr; a.vbias = L.bv;
        a.K = w.ck + (long)l * B * Tm * d; a.V = w.cv + (long)l * B * Tm * d; a.ldk = d; a.kb = (long)Tm * d; a.n = p + 1;
        a.out = w.a; a.ldo = d; a.scale = 0.125f;
        if (bm) hipLaunchKernelGGL(wsp_attend_anc_kernel, dim3(H, B), dim3(256), 0, st, a, bm->anc, bm->ld_anc, bm->K);
        else hipLaunchKernelGGL(wsp_attend_kernel, dim3(H, B), dim3(256), 0, st, a);
        ks = skinny(w.a, d, L.wo, d, d, d, w.P, B, st);
        finish(w.P, ks, d, L.bo, w.h, w.h, 0, L.ln2g, L.ln2b, w.y, B, st);
        ks = skinny(w.y, d, L.wcq, d, d, d, w.P, B, st);
        AtP x{};
        x.q = w.P; x.KS = ks; x.ss = (long)B * d; x.ldq = d; x.qbias = L.bcq;
        x.K = w.ckv + (long)l * (bm ? bm->U : cr ? cr->encoded : B) * S * 2 * d; x.V = x.K + d; x.ldk = 2 * d; x.kb = (long)S * 2 * d; x.n = S;
        x.out = w.a; x.ldo = d; x.scale = 0.125f;
        if (bm) attend_cross_beam(x, H, *bm, st);
        else if (cr) hipLaunchKernelGGL(wsp_attend_rows_kernel, dim3(H, B), dim3(256), 0, st, x, cr->row);
        else hipLaunchKernelGGL(wsp_attend_kernel, dim3(H, B), dim3(256), 0, st, x);
        ks = skinny(w.a, d, L.wco, d, d, d, w.P, B, st);
        finish(w.P, ks, d, L.bco, w.h, w.h, 0, L.ln3g, L.ln3b, w.y, B, st);
        ks = skinny(w.y, d, L.w1, F, d, F, w.P, B, st);
        finish(w.P, ks, F, L.b1, nullptr, w.ff, 1, nullptr, nullptr, nullptr, B, st);
        ks = skinny(w.ff, F, L.w2, d, F, d, w.P, B, st);
        const bool last = l + 1 == c.decoder_layers;
        finish(w.P, ks, d, L.b2, w.h, w.h, 0, last ? s->dec_g : s->dec[l + 1].ln1g, last ? s->dec_be : s->dec[l + 1].ln1b, w.y, B, st);
    }
    return logits ? skinny(w.y, d, s->embT, s->vocab_pad(), d, c.vocab_size, w.P, B, st) : 0;
}

int ready(DexWhisper* s, int B, void* ws, size_t bytes, Ws* w) {
    if (B < 1 || B > WB) return s->fail(DEX_ERR_ARG, "B must lie in [1, %d]", WB);
    if (!ws) return s->fail(DEX_ERR_ARG, "null pointer argument");
    *w = plan(s, ws, B);
    if (bytes < w->bytes) return s->fail(DEX_ERR_WORKSPACE, "workspace too small (dex_whisper_workspace_bytes)");
    return DEX_OK;
}

// the timestamp ids of a spec: eos below no_timestamps, and one id per 20 ms of a window and its end behind it
int check_timestamps(DexWhisper* s, int eos, int nots, int max_init) {
    const DexWhisperConfig& c = s->c;
    if (nots >= c.vocab_size - 1) return s->fail(DEX_ERR_ARG, "no_timestamps_token_id %d is outside the vocabulary of %d", nots, c.vocab_size);
    if (eos > nots) return s->fail(DEX_ERR_ARG, "eos_token_id %d lies above no_timestamps_token_id %d", eos, nots);
    if (c.vocab_size - (nots + 1) < c.max_source_positions + 1)
        return s->fail(DEX_ERR_ARG, "%d timestamp ids behind no_timestamps_token_id: max_source_positions + 1 = %d are needed", c.vocab_size - (nots + 1),
                       c.max_source_positions + 1);
    if (max_init < -1) return s->fail(DEX_ERR_ARG, "max_initial_timestamp_index must be >= 0, or -1 for none");
    return DEX_OK;
}

// Beam search workspace: the layout of U rows (the encoder's pieces and the cross K / V of the U utterances) and behind it the step of
// R = U x K rows: ck, cv [Ld][R][Tmax][d] | h, y, a [R][d] | ff [R][ffn_d] | P | logits [R][V] | run, pool scores (fp64) [R] |
// chunk maxima and sums (fp64) [R][C][2] | chunk candidates: scores (fp64), flat indices [R][C][2K] | seq, anc, pool ids (int)
// 2 x [R][Tmax] each but the last | pool len, order [R] | pool n, done [U], count
struct BeamWs { Ws w; float* lg; double *part, *cand_s; int* cand_f; DexWhisperBeamState s; int *seq[2], *anc[2]; size_t bytes; };
BeamWs plan_beam(const DexWhisper* s, void* ws, long U, long K) {
    const DexWhisperConfig& c = s->c;
    const long R = U * K, d = c.d_model, Tm = c.max_target_positions, Ld = c.decoder_layers;
    BeamWs b{};
    b.w = plan(s, ws, U);
    Taker tk(ws);
    tk.off = (long)((b.w.bytes - 256) / sizeof(float));
    b.w.ck = tk.take(Ld * R * Tm * d); b.w.cv = tk.take(Ld * R * Tm * d);
    b.w.h = tk.take(R * d); b.w.y = tk.take(R * d); b.w.a = tk.take(R * d); b.w.ff = tk.take(R * c.decoder_ffn_dim);
    b.w.P = tk.take(R * step_partials(c));
    b.lg = tk.take(R * c.vocab_size);
    const long C = beam_chunks(c.vocab_size);
    b.part = (double*)tk.take(4 * R * C); b.cand_s = (double*)tk.take(2 * R * C * 2 * K); b.cand_f = (int*)tk.take(R * C * 2 * K);
    b.s.run_score = (double*)tk.take(2 * R); b.s.pool_score = (double*)tk.take(2 * R);
    for (int i = 0; i < 2; ++i) { b.seq[i] = (int*)tk.take(R * Tm); b.anc[i] = (int*)tk.take(R * Tm); }
    b.s.pool_ids = (int*)tk.take(R * Tm);
    b.s.pool_len = (int*)tk.take(R); b.s.pool_order = (int*)tk.take(R);
    b.s.pool_n = (int*)tk.take(2 * U + 64); b.s.done = b.s.pool_n + U; b.s.count = b.s.done + U;
    b.s.ld_seq = b.s.ld_anc = (int)Tm;
    b.bytes = tk.bytes();
    return b;
}

bool beams_ok(const DexWhisper* s, int U, int K) {
    return U >= 1 && K >= DEX_WHISPER_MIN_BEAMS && K <= DEX_WHISPER_MAX_BEAMS && U * K <= WB && (long)K * s->c.max_source_positions <= DEX_WHISPER_BEAM_KEYS;
}

// the three launches of a step's tail
void launch_beam_pick(const BeamP& k, int U, hipStream_t st) {
    hipLaunchKernelGGL(wsp_beam_lse_kernel, dim3(k.C, U * k.K), dim3(256), 0, st, k);
    hipLaunchKernelGGL(wsp_beam_top_kernel, dim3(k.C, U * k.K), dim3(256), 0, st, k);
    hipLaunchKernelGGL(wsp_beam_pick_kernel, dim3(U), dim3(1024), 0, st, k);
}

// ------------------------------------------------------------------------------------------------------------ host: decoding
// what every decoder refuses before any launch
int check_decode_args(DexWhisper* s, const int32_t* prompt_host, int n_prompt, int eos, int max_new, int sync_every) {
    if (!s->finalized) return s->fail(DEX_ERR_STATE, "the whisper weights are not finalized (dex_whisper_finalize)");
    const DexWhisperConfig& c = s->c;
    if (n_prompt < 1 || n_prompt > c.max_target_positions)
        return s->fail(DEX_ERR_ARG, "a prompt of %d ids: 1 .. max_target_positions = %d", n_prompt, c.max_target_positions);
    for (int i = 0; i < n_prompt; ++i)
        if (prompt_host[i] < 0 || prompt_host[i] >= c.vocab_size) return s->fail(DEX_ERR_ARG, "prompt id %d is outside the vocabulary of %d", prompt_host[i], c.vocab_size);
    if (eos < 0 || eos >= c.vocab_size) return s->fail(DEX_ERR_ARG, "eos_token_id %d is outside the vocabulary of %d", eos, c.vocab_size);
    if (max_new < 1 || sync_every < 0) return s->fail(DEX_ERR_ARG, "max_new must be >= 1 and sync_every >= 0");
    return DEX_OK;
}

// a tail over finished fp32 logits [B][V] (the dex_whisper_pick* entry points): one slab, no next embedding
PickP pick_over_logits(const float* logits, int V, const uint8_t* mask, int eos, int* finished, int* lengths, int* count, int* ids, int ld_ids, int step) {
    PickP k{};
    k.P = logits; k.KS = 1; k.V = V; k.mask = mask; k.pick = 1; k.eos = eos; k.finished = finished; k.lengths = lengths; k.count = count;
    k.ids = ids; k.ld_ids = ld_ids; k.step = step; k.next_pos = -1;
    return k;
}

// what a greedy or policy decode of B rows is given: the masks, eos, the prompt's length and ids [B][max_new], lengths [B]
struct RowsOut { const uint8_t *suppress, *begin; int eos, n_prompt, max_new; int32_t *ids, *lengths; };

// the tail of step i of n_new inside such a decode: the logits' partials (ks slabs) in w.P, the begin mask at step 0, and the
// embedding of the next position where a step follows
PickP pick_in_step(const DexWhisper* s, const Ws& w, const RowsOut& o, int B, int ks, int i, int n_new) {
    const DexWhisperConfig& c = s->c;
    PickP k = pick_over_logits(w.P, c.vocab_size, i == 0 ? o.begin : o.suppress, o.eos, w.fin, o.lengths, w.count, o.ids, o.max_new, i);
    k.KS = ks; k.ss = (long)B * c.vocab_size;
    k.emb = s->emb; k.pos = s->dec_pos; k.d = c.d_model; k.next_pos = i + 1 < n_new ? o.n_prompt + i : -1; k.h = w.h;
    return k;
}

// the rows' state before the first step: ids all eos, lengths 0, nothing finished (the count sits behind `flags` flags), and under the
// timestamp rule no new token and no timestamp yet
int reset_rows(DexWhisper* s, const Ws& w, const RowsOut& o, int B, int flags, bool rule, hipStream_t st) {
    if (rule) {
        DEX_HIPCHK(s, hipMemsetAsync(w.n_new, 0, B * sizeof(int), st));
        hipLaunchKernelGGL(wsp_fill_kernel, dim3(1), dim3(256), 0, st, w.last_ts, (long)B, -1);
    }
    const long n_ids = (long)B * o.max_new;
    hipLaunchKernelGGL(wsp_fill_kernel, dim3((unsigned)((n_ids + 255) / 256)), dim3(256), 0, st, o.ids, n_ids, o.eos);
    DEX_HIPCHK(s, hipMemsetAsync(o.lengths, 0, B * sizeof(int32_t), st));
    DEX_HIPCHK(s, hipMemsetAsync(w.fin, 0, (flags + 1) * sizeof(int), st));
    return DEX_OK;
}

// One decode: `rows` rows of the step (bm: U x K beams, the ancestry of the step to come in bm->anc; cr: rows of an encoded batch).
// It ends early once the device counter `count`, polled every sync_every steps, has reached `enough`.
struct LoopP { const int32_t* prompt; int n_prompt, max_new, sync_every, rows, enough; const int* count; const BeamAt* bm; const CrossRows* cr; bool probe0; };

// The prompt fills the cache (its logits are not needed, but position 0's where probe0), then n_new = min(max_new, the room in the
// cache) steps, each ended by tail(i, n_new, ks), which leaves the next position's embedding in w.h.  after_prompt(p, ks) follows
// the step of every prompt position p (ks: its logits' slabs, 0 where it has none).  Returns the steps taken in *steps
template <class After, class Tail>
int decode_loop(DexWhisper* s, const Ws& w, const LoopP& L, hipStream_t st, After after_prompt, Tail tail, int* steps) {
    const DexWhisperConfig& c = s->c;
    const int room = c.max_target_positions - L.n_prompt, n_new = L.max_new < room ? L.max_new : room;      // never past the cache
    *steps = 0;
    if (n_new <= 0) return DEX_OK;
    for (int p = 0; p < L.n_prompt; ++p) {
        hipLaunchKernelGGL(wsp_embed_kernel, dim3(L.rows), dim3(256), 0, st, (const int*)nullptr, 0, L.prompt[p], p, c.vocab_size, s->emb, s->dec_pos, c.d_model, w.h);
        if (p < L.n_prompt - 1) after_prompt(p, enqueue_step(s, p, L.rows, w, st, p == 0 && L.probe0, L.bm, L.cr));
    }
    for (int i = 0; i < n_new; ++i) {
        const int ks = enqueue_step(s, L.n_prompt - 1 + i, L.rows, w, st, true, L.bm, L.cr);
        if (i == 0) after_prompt(L.n_prompt - 1, ks);
        tail(i, n_new, ks);
        *steps = i + 1;
        if (L.sync_every && *steps % L.sync_every == 0 && *steps < n_new) {
            int done = 0;
            DEX_HIPCHK(s, hipMemcpyAsync(&done, L.count, sizeof(int), hipMemcpyDeviceToHost, st));
            DEX_HIPCHK(s, hipStreamSynchronize(st));
            if (done >= L.enough) break;
        }
    }
    return DEX_OK;
}

// the end of a decoding call: it waits for the stream
int decode_done(DexWhisper* s, hipStream_t st) {
    DEX_HIPCHK(s, hipStreamSynchronize(st));
    return hipGetLastError() == hipSuccess ? DEX_OK : s->fail(DEX_ERR_HIP, "kernel launch failed");
}

typedef Entry<DexWhisper> E;

}  // namespace

extern "C" {

int dex_whisper_create(const DexWhisperConfig* cfg, DexWhisper** out) { return E::create(cfg, out, default_config, check_config, register_keys); }
void dex_whisper_destroy(DexWhisper* s) {
    if (s && s->tab_dev) hipFree(s->tab_dev);
    E::destroy(s);
}
const char* dex_whisper_last_error(const DexWhisper* s) { return E::last_error(s); }
int dex_whisper_load(DexWhisper* s, const char* key, const float* w_dev, const int64_t* shape, int ndim, dex_stream_t stream) {
    return E::load(s, key, w_dev, shape, ndim, stream);
}
int dex_whisper_finalize(DexWhisper* s, dex_stream_t stream) { return E::finalize(s, stream, pack_all, "packing the whisper weights failed"); }
int dex_whisper_num_weights(const DexWhisper* s) { return E::num_weights(s); }
int dex_whisper_weight_info(const DexWhisper* s, int i, const char** key, int64_t shape[4], int* ndim) { return E::weight_info(s, i, key, shape, ndim); }

size_t dex_whisper_workspace_bytes(const DexWhisper* s, int B) {
    if (!s || B < 1 || B > WB) return 0;
    return plan(s, nullptr, B).bytes;
}

int dex_whisper_mel_filters(int n_mels, double* out) {
    if (n_mels < 1 || n_mels > 128 || !out) return DEX_ERR_ARG;
    mel_filters(n_mels, out);
    return DEX_OK;
}

int dex_whisper_log_mel(DexWhisper* s, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, float* out_dev, void* workspace_dev,
                        size_t workspace_bytes, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!wav_dev || !lengths_host || !out_dev) return s->fail(DEX_ERR_ARG, "null pointer argument");
    const long chunk = 2L * s->c.max_source_positions * HOP;
    if (n_samples < 1 || n_samples > chunk) return s->fail(DEX_ERR_ARG, "n_samples must lie in [1, %ld] (one chunk; long-form audio is not built)", chunk);
    Ws w;
    if (int rc = ready(s, B, workspace_dev, workspace_bytes, &w)) return rc;
    for (int b = 0; b < B; ++b)
        if (lengths_host[b] < 1 || lengths_host[b] > n_samples) return s->fail(DEX_ERR_ARG, "row lengths must lie in [1, n_samples]");
    if (int rc = ensure_tables(s, (hipStream_t)stream)) return rc;
    const int T = 2 * s->c.max_source_positions;
    enqueue_log_mel(s, wav_dev, lengths_host, B, n_samples, w.logspec, out_dev, T, T, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? DEX_OK : s->fail(DEX_ERR_HIP, "kernel launch failed");
}

int dex_whisper_encode(DexWhisper* s, const float* feat_dev, int B, float* enc_out_dev, float* ms_host, void* workspace_dev, size_t workspace_bytes,
                       dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!feat_dev) return s->fail(DEX_ERR_ARG, "null pointer argument");
    Ws w;
    if (int rc = ready(s, B, workspace_dev, workspace_bytes, &w)) return rc;
    if (!s->finalized) return s->fail(DEX_ERR_STATE, "the whisper weights are not finalized (dex_whisper_finalize)");
    if (!ms_host) {
        enqueue_encoder(s, feat_dev, B, enc_out_dev, w, (hipStream_t)stream);
        return hipGetLastError() == hipSuccess ? DEX_OK : s->fail(DEX_ERR_HIP, "kernel launch failed");
    }
    hipEvent_t ev[3];                                           // the measuring form (tools/whisper_bench.py): waits for the stream
    for (hipEvent_t& e : ev) DEX_HIPCHK(s, hipEventCreate(&e));
    hipEventRecord(ev[0], (hipStream_t)stream);
    enqueue_encoder(s, feat_dev, B, enc_out_dev, w, (hipStream_t)stream, ev[1]);
    hipEventRecord(ev[2], (hipStream_t)stream);
    const hipError_t rc = hipEventSynchronize(ev[2]);
    if (rc == hipSuccess) { hipEventElapsedTime(ms_host, ev[0], ev[1]); hipEventElapsedTime(ms_host + 1, ev[1], ev[2]); }
    for (hipEvent_t& e : ev) hipEventDestroy(e);
    return rc == hipSuccess && hipGetLastError() == hipSuccess ? DEX_OK : s->fail(DEX_ERR_HIP, "the encoder failed");
}

int dex_whisper_forward(DexWhisper* s, const int32_t* ids_dev, int B, int L, float* logits_dev, void* workspace_dev, size_t workspace_bytes,
                        dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!ids_dev || !logits_dev) return s->fail(DEX_ERR_ARG, "null pointer argument");
    Ws w;
    if (int rc = ready(s, B, workspace_dev, workspace_bytes, &w)) return rc;
    if (!s->finalized) return s->fail(DEX_ERR_STATE, "the whisper weights are not finalized (dex_whisper_finalize)");
    const DexWhisperConfig& c = s->c;
    if (L < 1 || L > c.max_target_positions) return s->fail(DEX_ERR_ARG, "%d decoder positions: 1 .. max_target_positions = %d", L, c.max_target_positions);
    hipStream_t st = (hipStream_t)stream;
    for (int p = 0; p < L; ++p) {
        hipLaunchKernelGGL(wsp_embed_kernel, dim3(B), dim3(256), 0, st, ids_dev, L, 0, p, c.vocab_size, s->emb, s->dec_pos, c.d_model, w.h);
        const int ks = enqueue_step(s, p, B, w, st);
        PickP k{};
        k.P = w.P; k.KS = ks; k.ss = (long)B * c.vocab_size; k.V = c.vocab_size; k.logits = logits_dev + (long)p * c.vocab_size; k.ldl = (long)L * c.vocab_size;
        k.next_pos = -1;
        hipLaunchKernelGGL(wsp_pick_kernel, dim3(B), dim3(1024), 0, st, k);
    }
    return hipGetLastError() == hipSuccess ? DEX_OK : s->fail(DEX_ERR_HIP, "kernel launch failed");
}

// the body of dex_whisper_generate (nots < 0) and dex_whisper_generate_ts
static int generate(DexWhisper* s, const int32_t* prompt_host, int n_prompt, const uint8_t* suppress_dev, const uint8_t* begin_dev, int eos, int nots,
                    int max_init, int B, int max_new, int sync_every, int32_t* ids_dev, int32_t* lengths_dev, int* steps_host, void* workspace_dev,
                    size_t workspace_bytes, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!prompt_host || !ids_dev || !lengths_dev || !steps_host) return s->fail(DEX_ERR_ARG, "null pointer argument");
    Ws w;
    if (int rc = ready(s, B, workspace_dev, workspace_bytes, &w)) return rc;
    if (int rc = check_decode_args(s, prompt_host, n_prompt, eos, max_new, sync_every)) return rc;
    if (nots >= 0)
        if (int rc = check_timestamps(s, eos, nots, max_init)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const RowsOut o{suppress_dev, begin_dev, eos, n_prompt, max_new, ids_dev, lengths_dev};
    if (int rc = reset_rows(s, w, o, B, B, nots >= 0, st)) return rc;
    const RuleP rule{nots, nots + 1, max_init, w.last_ts, w.n_new};
    auto tail = [&](int i, int n_new, int ks) {
        const PickP k = pick_in_step(s, w, o, B, ks, i, n_new);
        if (nots >= 0) hipLaunchKernelGGL(wsp_pick_ts_kernel, dim3(B), dim3(1024), 0, st, PickTsP{k, rule});
        else hipLaunchKernelGGL(wsp_pick_kernel, dim3(B), dim3(1024), 0, st, k);
    };
    const LoopP loop{prompt_host, n_prompt, max_new, sync_every, B, B, w.count, nullptr, nullptr, false};
    if (int rc = decode_loop(s, w, loop, st, [](int, int) {}, tail, steps_host)) return rc;
    return decode_done(s, st);
}

int dex_whisper_generate(DexWhisper* s, const int32_t* prompt_host, int n_prompt, const uint8_t* suppress_dev, const uint8_t* begin_dev, int eos, int B,
                         int max_new, int sync_every, int32_t* ids_dev, int32_t* lengths_dev, int* steps_host, void* workspace_dev,
                         size_t workspace_bytes, dex_stream_t stream) {
    return generate(s, prompt_host, n_prompt, suppress_dev, begin_dev, eos, -1, -1, B, max_new, sync_every, ids_dev, lengths_dev, steps_host, workspace_dev,
                    workspace_bytes, stream);
}

int dex_whisper_generate_ts(DexWhisper* s, const int32_t* prompt_host, int n_prompt, const uint8_t* suppress_dev, const uint8_t* begin_dev, int eos,
                            int no_timestamps_token_id, int max_initial_timestamp_index, int B, int max_new, int sync_every, int32_t* ids_dev,
                            int32_t* lengths_dev, int* steps_host, void* workspace_dev, size_t workspace_bytes, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (no_timestamps_token_id < 0) return s->fail(DEX_ERR_ARG, "no_timestamps_token_id %d is outside the vocabulary of %d", no_timestamps_token_id, s->c.vocab_size);
    return generate(s, prompt_host, n_prompt, suppress_dev, begin_dev, eos, no_timestamps_token_id, max_initial_timestamp_index, B, max_new, sync_every,
                    ids_dev, lengths_dev, steps_host, workspace_dev, workspace_bytes, stream);
}

// the Philox key and the per-row counter words of an attempt
static void policy_noise(PolP* q, double temperature, uint64_t seed, int attempt, const uint32_t* row_keys_host, const int32_t* seek_host, int B) {
    q->T = temperature; q->k0 = (uint32_t)seed; q->k1 = (uint32_t)(seed >> 32);
    for (int b = 0; b < B; ++b) { q->rk.key[b] = row_keys_host[b]; q->rk.c2[b] = (uint32_t)attempt + 16u * (uint32_t)seek_host[b]; }
}

int dex_whisper_generate_policy(DexWhisper* s, const int32_t* prompt_host, int n_prompt, const uint8_t* suppress_dev, const uint8_t* begin_dev, int eos,
                                int timestamps, int no_timestamps_token_id, int max_initial_timestamp_index, double temperature, uint64_t seed,
                                int attempt, const uint32_t* row_keys_host, const int32_t* seek_host, int encoded, const int32_t* rows_host, int B,
                                int max_new, int sync_every, int32_t* ids_dev, int32_t* lengths_dev, double* sum_logprob_dev, int32_t* n_scored_dev,
                                int no_speech_token_id, double* no_speech_prob_dev, int* steps_host, void* workspace_dev, size_t workspace_bytes,
                                dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!prompt_host || !ids_dev || !lengths_dev || !steps_host || !row_keys_host || !seek_host || !rows_host || !sum_logprob_dev || !n_scored_dev)
        return s->fail(DEX_ERR_ARG, "null pointer argument");
    Ws w;
    if (int rc = ready(s, encoded, workspace_dev, workspace_bytes, &w)) return rc;
    const DexWhisperConfig& c = s->c;
    if (B < 1 || B > encoded) return s->fail(DEX_ERR_ARG, "B must lie in [1, encoded = %d]", encoded);
    CrossRows cr{};
    cr.encoded = encoded;
    for (int b = 0; b < B; ++b) {
        if (rows_host[b] < 0 || rows_host[b] >= encoded) return s->fail(DEX_ERR_ARG, "row %d is outside the %d encoded rows", rows_host[b], encoded);
        if (seek_host[b] < 0) return s->fail(DEX_ERR_ARG, "a row's seek must be >= 0");
        cr.row.a[b] = rows_host[b];
    }
    if (int rc = check_decode_args(s, prompt_host, n_prompt, eos, max_new, sync_every)) return rc;
    if (!(temperature >= 0.0) || !std::isfinite(temperature)) return s->fail(DEX_ERR_ARG, "temperature must be finite and >= 0");
    if (attempt < 0 || attempt > 15) return s->fail(DEX_ERR_ARG, "attempt must lie in [0, 15]");
    if (no_speech_prob_dev && (no_speech_token_id < 0 || no_speech_token_id >= c.vocab_size))
        return s->fail(DEX_ERR_ARG, "no_speech_token_id %d is outside the vocabulary of %d", no_speech_token_id, c.vocab_size);
    if (timestamps) {
        if (no_timestamps_token_id < 0) return s->fail(DEX_ERR_ARG, "no_timestamps_token_id %d is outside the vocabulary of %d", no_timestamps_token_id, c.vocab_size);
        if (int rc = check_timestamps(s, eos, no_timestamps_token_id, max_initial_timestamp_index)) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    const RowsOut o{suppress_dev, begin_dev, eos, n_prompt, max_new, ids_dev, lengths_dev};
    if (int rc = reset_rows(s, w, o, B, encoded, timestamps != 0, st)) return rc;           // the count sits behind the encoded rows' flags
    DEX_HIPCHK(s, hipMemsetAsync(sum_logprob_dev, 0, B * sizeof(double), st));
    DEX_HIPCHK(s, hipMemsetAsync(n_scored_dev, 0, B * sizeof(int32_t), st));
    PolP q{};
    policy_noise(&q, temperature, seed, attempt, row_keys_host, seek_host, B);
    q.r = RuleP{no_timestamps_token_id, no_timestamps_token_id + 1, max_initial_timestamp_index, w.last_ts, w.n_new};
    q.sum_lp = sum_logprob_dev; q.n_scored = n_scored_dev;
    auto probe = [&](int p, int ks) {                                                     // the unprocessed logits of prompt position 0 are in w.P
        if (p == 0 && no_speech_prob_dev)
            hipLaunchKernelGGL(wsp_nospeech_kernel, dim3(B), dim3(1024), 0, st, ProbeP{w.P, ks, (long)B * c.vocab_size, c.vocab_size, no_speech_token_id, no_speech_prob_dev});
    };
    auto tail = [&](int i, int n_new, int ks) {
        q.k = pick_in_step(s, w, o, B, ks, i, n_new);
        if (timestamps) hipLaunchKernelGGL(wsp_pick_policy_kernel<true>, dim3(B), dim3(1024), 0, st, q);
        else hipLaunchKernelGGL(wsp_pick_policy_kernel<false>, dim3(B), dim3(1024), 0, st, q);
    };
    const LoopP loop{prompt_host, n_prompt, max_new, sync_every, B, B, w.count, nullptr, &cr, no_speech_prob_dev != nullptr};
    if (int rc = decode_loop(s, w, loop, st, probe, tail, steps_host)) return rc;
    return decode_done(s, st);
}

int dex_whisper_log_mel_long(DexWhisper* s, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, float* out_dev, int max_frames,
                             int32_t* frames_host, void* scratch_dev, size_t scratch_bytes, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!wav_dev || !lengths_host || !out_dev || !frames_host || !scratch_dev) return s->fail(DEX_ERR_ARG, "null pointer argument");
    if (B < 1 || B > WB) return s->fail(DEX_ERR_ARG, "B must lie in [1, %d]", WB);
    if (n_samples < 1 || n_samples > DEX_WHISPER_MAX_LONG_SAMPLES) return s->fail(DEX_ERR_ARG, "n_samples must lie in [1, %d] (the cap of a long row)", DEX_WHISPER_MAX_LONG_SAMPLES);
    const DexWhisperConfig& c = s->c;
    const int Tc = 2 * c.max_source_positions, M = c.num_mel_bins;
    const long chunk = (long)Tc * HOP;
    int F = 0;
    for (int b = 0; b < B; ++b) {
        if (lengths_host[b] < 1 || lengths_host[b] > n_samples) return s->fail(DEX_ERR_ARG, "row lengths must lie in [1, n_samples]");
        frames_host[b] = lengths_host[b] <= chunk ? Tc : lengths_host[b] / HOP;
        F = frames_host[b] > F ? frames_host[b] : F;
    }
    if (max_frames < F) return s->fail(DEX_ERR_ARG, "max_frames %d is below the longest row's %d frames", max_frames, F);
    if (scratch_bytes < (size_t)B * max_frames * M * sizeof(double)) return s->fail(DEX_ERR_WORKSPACE, "scratch too small (B x max_frames x num_mel_bins doubles)");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = ensure_tables(s, st)) return rc;
    enqueue_log_mel(s, wav_dev, lengths_host, B, n_samples, (double*)scratch_dev, out_dev, F, max_frames, st);
    return hipGetLastError() == hipSuccess ? DEX_OK : s->fail(DEX_ERR_HIP, "kernel launch failed");
}

int dex_whisper_gather_windows(DexWhisper* s, const float* feat_dev, int rows, int max_frames, const int32_t* row_host, const int32_t* seek_host,
                               const int32_t* n_host, int active, float* out_dev, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!feat_dev || !row_host || !seek_host || !n_host || !out_dev) return s->fail(DEX_ERR_ARG, "null pointer argument");
    if (active < 1 || active > WB) return s->fail(DEX_ERR_ARG, "B must lie in [1, %d]", WB);
    const int W = 2 * s->c.max_source_positions;
    GatherP p{};
    if (rows < 1 || max_frames < 1) return s->fail(DEX_ERR_ARG, "rows and max_frames must be >= 1");
    for (int a = 0; a < active; ++a) {
        if (row_host[a] < 0 || row_host[a] >= rows) return s->fail(DEX_ERR_ARG, "row index %d is outside the %d rows", row_host[a], rows);
        if (seek_host[a] < 0 || n_host[a] < 1 || n_host[a] > W || (long)seek_host[a] + n_host[a] > max_frames)
            return s->fail(DEX_ERR_ARG, "a window [seek, seek + n) must lie in the row's %d frames, n in [1, %d]", max_frames, W);
        p.row.a[a] = row_host[a]; p.seek.a[a] = seek_host[a]; p.n.a[a] = n_host[a];
    }
    p.feat = feat_dev; p.out = out_dev; p.Fmax = max_frames; p.n_mels = s->c.num_mel_bins; p.W = W;
    hipLaunchKernelGGL(wsp_gather_kernel, dim3((W + 255) / 256, p.n_mels, active), dim3(256), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? DEX_OK : s->fail(DEX_ERR_HIP, "kernel launch failed");
}

int dex_whisper_attend(const float* q_dev, float* k_dev, float* v_dev, const float* new_k_dev, const float* new_v_dev, float* out_dev, int B, int heads,
                       int n_keys, int cap, dex_stream_t stream) {
    if (!q_dev || !k_dev || !v_dev || !out_dev || (new_k_dev == nullptr) != (new_v_dev == nullptr)) return DEX_ERR_ARG;
    if (B < 1 || B > 65535 || heads < 1 || heads > 1024 || n_keys < 1 || n_keys > cap || cap > MAX_KEYS) return DEX_ERR_ARG;
    AtP a{};
    a.q = q_dev; a.kn = new_k_dev; a.vn = new_v_dev; a.KS = 1; a.ss = 0; a.ldq = heads * 64;
    a.K = k_dev; a.V = v_dev; a.ldk = heads * 64; a.kb = (long)cap * heads * 64; a.n = n_keys; a.out = out_dev; a.ldo = heads * 64; a.scale = 0.125f;
    hipLaunchKernelGGL(wsp_attend_kernel, dim3(heads, B), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

int dex_whisper_step_linear(const float* x_dev, const float* w_dev, float* y_dev, float* scratch_dev, size_t scratch_floats, int M, int K, int N, int form,
                            dex_stream_t stream) {
    if (!x_dev || !w_dev || !y_dev || M < 1 || M > WB || K < 64 || K % 64 || N < 64 || N % 64 || (form != 0 && form != 1)) return DEX_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (form == 1) {
        linear(x_dev, K, w_dev, N, nullptr, y_dev, 0, nullptr, nullptr, M, 1, st);
    } else {
        if (!scratch_dev || scratch_floats < (size_t)slabs(K) * M * N) return DEX_ERR_WORKSPACE;
        const int ks = skinny(x_dev, K, w_dev, N, K, N, scratch_dev, M, st);
        finish(scratch_dev, ks, N, nullptr, nullptr, y_dev, 0, nullptr, nullptr, nullptr, M, st);
    }
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

int dex_whisper_pick(const float* logits_dev, int B, int V, const uint8_t* mask_dev, int eos, int32_t* finished_dev, int32_t* lengths_dev,
                     int32_t* count_dev, int32_t* ids_dev, int ld_ids, int step, dex_stream_t stream) {
    if (!logits_dev || !finished_dev || !lengths_dev || !count_dev || !ids_dev) return DEX_ERR_ARG;
    if (B < 1 || B > 65535 || V < 1 || eos < 0 || eos >= V || step < 0 || step >= ld_ids) return DEX_ERR_ARG;
    const PickP k = pick_over_logits(logits_dev, V, mask_dev, eos, finished_dev, lengths_dev, count_dev, ids_dev, ld_ids, step);
    hipLaunchKernelGGL(wsp_pick_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, k);
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

int dex_whisper_pick_ts(const float* logits_dev, int B, int V, const uint8_t* mask_dev, int eos, int no_timestamps_token_id,
                        int max_initial_timestamp_index, int32_t* finished_dev, int32_t* lengths_dev, int32_t* count_dev, int32_t* ids_dev, int ld_ids,
                        int step, int32_t* last_timestamp_dev, int32_t* n_new_dev, dex_stream_t stream) {
    if (!logits_dev || !finished_dev || !lengths_dev || !count_dev || !ids_dev || !last_timestamp_dev || !n_new_dev) return DEX_ERR_ARG;
    if (B < 1 || B > 65535 || V < 1 || eos < 0 || eos >= V || step < 2 || step >= ld_ids) return DEX_ERR_ARG;
    if (no_timestamps_token_id < eos || no_timestamps_token_id >= V - 1 || max_initial_timestamp_index < -1) return DEX_ERR_ARG;
    const PickP k = pick_over_logits(logits_dev, V, mask_dev, eos, finished_dev, lengths_dev, count_dev, ids_dev, ld_ids, step);
    hipLaunchKernelGGL(wsp_pick_ts_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream,
                       PickTsP{k, RuleP{no_timestamps_token_id, no_timestamps_token_id + 1, max_initial_timestamp_index, last_timestamp_dev, n_new_dev}});
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

int dex_whisper_pick_policy(const float* logits_dev, int B, int V, const uint8_t* mask_dev, int eos, int timestamps, int no_timestamps_token_id,
                            int max_initial_timestamp_index, double temperature, uint64_t seed, int attempt, const uint32_t* row_keys_host,
                            const int32_t* seek_host, int32_t* finished_dev, int32_t* lengths_dev, int32_t* count_dev, int32_t* ids_dev, int ld_ids,
                            int step, int32_t* last_timestamp_dev, int32_t* n_new_dev, double* sum_logprob_dev, int32_t* n_scored_dev,
                            dex_stream_t stream) {
    if (!logits_dev || !finished_dev || !lengths_dev || !count_dev || !ids_dev || !row_keys_host || !seek_host || !sum_logprob_dev || !n_scored_dev)
        return DEX_ERR_ARG;
    if (B < 1 || B > WB || V < 1 || eos < 0 || eos >= V || step < 0 || step >= ld_ids) return DEX_ERR_ARG;
    if (!(temperature >= 0.0) || !std::isfinite(temperature) || attempt < 0 || attempt > 15) return DEX_ERR_ARG;
    for (int b = 0; b < B; ++b)
        if (seek_host[b] < 0) return DEX_ERR_ARG;
    PolP q{};
    q.k = pick_over_logits(logits_dev, V, mask_dev, eos, finished_dev, lengths_dev, count_dev, ids_dev, ld_ids, step);
    policy_noise(&q, temperature, seed, attempt, row_keys_host, seek_host, B);
    q.sum_lp = sum_logprob_dev; q.n_scored = n_scored_dev;
    if (timestamps) {
        if (!last_timestamp_dev || !n_new_dev || step < 2) return DEX_ERR_ARG;
        if (no_timestamps_token_id < eos || no_timestamps_token_id >= V - 1 || max_initial_timestamp_index < -1) return DEX_ERR_ARG;
        q.r = RuleP{no_timestamps_token_id, no_timestamps_token_id + 1, max_initial_timestamp_index, last_timestamp_dev, n_new_dev};
        hipLaunchKernelGGL(wsp_pick_policy_kernel<true>, dim3(B), dim3(1024), 0, (hipStream_t)stream, q);
    } else {
        hipLaunchKernelGGL(wsp_pick_policy_kernel<false>, dim3(B), dim3(1024), 0, (hipStream_t)stream, q);
    }
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

int dex_whisper_attend_beam(const float* q_dev, float* k_dev, float* v_dev, const float* new_k_dev, const float* new_v_dev, const int32_t* anc_dev,
                            int ld_anc, float* out_dev, int U, int K, int heads, int n_keys, int cap, dex_stream_t stream) {
    if (!q_dev || !k_dev || !v_dev || !out_dev || (new_k_dev == nullptr) != (new_v_dev == nullptr)) return DEX_ERR_ARG;
    if (U < 1 || K < DEX_WHISPER_MIN_BEAMS || K > DEX_WHISPER_MAX_BEAMS || (long)U * K > 65535 || heads < 1 || heads > 1024) return DEX_ERR_ARG;
    if (n_keys < 1 || n_keys > cap || cap > MAX_KEYS) return DEX_ERR_ARG;
    AtP a{};
    a.q = q_dev; a.KS = 1; a.ss = 0; a.ldq = heads * 64;
    a.K = k_dev; a.V = v_dev; a.ldk = heads * 64; a.kb = (long)cap * heads * 64; a.n = n_keys; a.out = out_dev; a.ldo = heads * 64; a.scale = 0.125f;
    if (anc_dev) {
        if (ld_anc < n_keys) return DEX_ERR_ARG;
        a.kn = new_k_dev; a.vn = new_v_dev;
        hipLaunchKernelGGL(wsp_attend_anc_kernel, dim3(heads, U * K), dim3(256), 0, (hipStream_t)stream, a, (const int*)anc_dev, ld_anc, K);
    } else {
        if (new_k_dev || (long)K * n_keys > DEX_WHISPER_BEAM_KEYS) return DEX_ERR_ARG;
        attend_cross_beam(a, heads, BeamAt{U, K, nullptr, 0}, (hipStream_t)stream);
    }
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

size_t dex_whisper_beam_pick_scratch_bytes(int U, int K, int V) {
    if (U < 1 || K < DEX_WHISPER_MIN_BEAMS || K > DEX_WHISPER_MAX_BEAMS || V < 1) return 0;
    const size_t RC = (size_t)U * K * beam_chunks(V);
    return RC * (2 * sizeof(double) + 2 * K * (sizeof(double) + sizeof(int)));
}

int dex_whisper_beam_pick(const float* logits_dev, int U, int K, int V, const uint8_t* mask_dev, int eos, int step, int pos, int last,
                          double length_penalty, const DexWhisperBeamState* state, int32_t* tokens_dev, int32_t* parents_dev, void* scratch_dev,
                          size_t scratch_bytes, dex_stream_t stream) {
    if (!logits_dev || !state || !scratch_dev || (tokens_dev == nullptr) != (parents_dev == nullptr)) return DEX_ERR_ARG;
    const DexWhisperBeamState& s = *state;
    if (!s.run_score || !s.pool_score || !s.seq_in || !s.seq_out || !s.anc_in || !s.anc_out || !s.pool_ids || !s.pool_len || !s.pool_order || !s.pool_n ||
        !s.done || !s.count)
        return DEX_ERR_ARG;
    if (U < 1 || U > 65535 || K < DEX_WHISPER_MIN_BEAMS || K > DEX_WHISPER_MAX_BEAMS || V < 2 * K || (long)K * V > 0x7fffffffL || eos < 0 || eos >= V)
        return DEX_ERR_ARG;
    if (step < 0 || step >= s.ld_seq || pos < 0 || pos >= s.ld_anc) return DEX_ERR_ARG;
    BeamP k{};
    k.P = logits_dev; k.KS = 1; k.V = V; k.K = K; k.mask = mask_dev; k.eos = eos; k.step = step; k.pos = pos; k.last = last != 0;
    k.div = std::pow((double)(step + 1), length_penalty); k.s = s; k.tok = tokens_dev; k.par = parents_dev; k.next_pos = -1;
    if (((uintptr_t)scratch_dev & 7) || scratch_bytes < dex_whisper_beam_pick_scratch_bytes(U, K, V)) return DEX_ERR_WORKSPACE;
    const long RC = (long)U * K * beam_chunks(V);
    k.C = beam_chunks(V); k.part = (double*)scratch_dev; k.cand_s = k.part + 2 * RC; k.cand_f = (int*)(k.cand_s + RC * 2 * K);
    launch_beam_pick(k, U, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

size_t dex_whisper_beam_workspace_bytes(const DexWhisper* s, int U, int K) {
    if (!s || !beams_ok(s, U, K)) return 0;
    return plan_beam(s, nullptr, U, K).bytes;
}

int dex_whisper_generate_beam(DexWhisper* s, const int32_t* prompt_host, int n_prompt, const uint8_t* suppress_dev, const uint8_t* begin_dev, int eos, int U,
                              int K, double length_penalty, int max_new, int sync_every, int32_t* ids_dev, int32_t* lengths_dev, double* scores_dev,
                              int* steps_host, float* trace_logits_dev, int32_t* trace_tokens_dev, int32_t* trace_parents_dev, double* trace_scores_dev,
                              int32_t* pool_ids_dev, int32_t* pool_len_dev, double* pool_scores_dev, int32_t* pool_n_dev, void* workspace_dev,
                              size_t workspace_bytes, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!prompt_host || !ids_dev || !lengths_dev || !scores_dev || !steps_host || !workspace_dev) return s->fail(DEX_ERR_ARG, "null pointer argument");
    const bool trace = trace_logits_dev != nullptr, pool = pool_ids_dev != nullptr;
    if (trace != (trace_tokens_dev != nullptr) || trace != (trace_parents_dev != nullptr) || trace != (trace_scores_dev != nullptr))
        return s->fail(DEX_ERR_ARG, "the trace buffers come all or none");
    if (pool != (pool_len_dev != nullptr) || pool != (pool_scores_dev != nullptr) || pool != (pool_n_dev != nullptr))
        return s->fail(DEX_ERR_ARG, "the pool buffers come all or none");
    const DexWhisperConfig& c = s->c;
    if (!beams_ok(s, U, K))
        return s->fail(DEX_ERR_ARG, "num_beams must lie in [%d, %d], utterances x num_beams in [1, %d] and num_beams x max_source_positions within %d",
                       DEX_WHISPER_MIN_BEAMS, DEX_WHISPER_MAX_BEAMS, WB, DEX_WHISPER_BEAM_KEYS);
    BeamWs b = plan_beam(s, workspace_dev, U, K);
    if (workspace_bytes < b.bytes) return s->fail(DEX_ERR_WORKSPACE, "workspace too small (dex_whisper_beam_workspace_bytes)");
    if (int rc = check_decode_args(s, prompt_host, n_prompt, eos, max_new, sync_every)) return rc;
    if (c.vocab_size < 2 * K) return s->fail(DEX_ERR_ARG, "a vocabulary of %d ids is below 2 x num_beams", c.vocab_size);
    if (!(length_penalty == length_penalty)) return s->fail(DEX_ERR_ARG, "length_penalty is NaN");
    hipStream_t st = (hipStream_t)stream;
    const int R = U * K, V = c.vocab_size, Tm = c.max_target_positions;
    const long init = (long)R * Tm;
    hipLaunchKernelGGL(wsp_beam_init_kernel, dim3((unsigned)((init + 255) / 256)), dim3(256), 0, st, [&] { DexWhisperBeamState t = b.s; t.anc_in = b.anc[0]; t.anc_out = b.anc[1]; return t; }(), U, K);
    if (trace) {
        const long n = (long)max_new * R;
        hipLaunchKernelGGL(wsp_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, trace_tokens_dev, n, -1);
        hipLaunchKernelGGL(wsp_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, trace_parents_dev, n, -1);
        DEX_HIPCHK(s, hipMemsetAsync(trace_scores_dev, 0, n * sizeof(double), st));
        DEX_HIPCHK(s, hipMemsetAsync(trace_logits_dev, 0, n * V * sizeof(float), st));
    }
    // the prompt is fed on all K rows of an utterance: identical rows, and the identity ancestry the first step starts from
    BeamAt bm{U, K, b.anc[0], Tm};
    auto tail = [&](int i, int n_new, int ks) {
        BeamP k{};
        k.P = b.w.P; k.KS = ks; k.ss = (long)R * V; k.V = V; k.K = K; k.mask = i == 0 ? begin_dev : suppress_dev;
        k.lg = trace ? trace_logits_dev + (long)i * R * V : b.lg; k.C = beam_chunks(V); k.part = b.part; k.cand_s = b.cand_s; k.cand_f = b.cand_f;
        k.eos = eos; k.step = i; k.pos = n_prompt - 1 + i; k.last = i + 1 == n_new; k.div = std::pow((double)(i + 1), length_penalty);
        k.s = b.s;
        if (trace) { k.tok = trace_tokens_dev + (long)i * R; k.par = trace_parents_dev + (long)i * R; k.trace = trace_scores_dev + (long)i * R; }
        k.emb = s->emb; k.posw = s->dec_pos; k.d = c.d_model; k.next_pos = i + 1 < n_new ? n_prompt + i : -1; k.h = b.w.h;
        k.s.seq_in = b.seq[i & 1]; k.s.seq_out = b.seq[(i & 1) ^ 1]; k.s.anc_in = b.anc[i & 1]; k.s.anc_out = b.anc[(i & 1) ^ 1];
        launch_beam_pick(k, U, st);
        bm.anc = k.s.anc_out;                                                             // the swap: the next step reads what this one wrote
    };
    const LoopP loop{prompt_host, n_prompt, max_new, sync_every, R, U, b.s.count, &bm, nullptr, false};
    if (int rc = decode_loop(s, b.w, loop, st, [](int, int) {}, tail, steps_host)) return rc;
    BeamOutP o{};
    o.s = b.s; o.K = K; o.eos = eos; o.max_new = max_new; o.ids = ids_dev; o.lengths = lengths_dev; o.scores = scores_dev;
    o.pool_ids = pool_ids_dev; o.pool_len = pool_len_dev; o.pool_scores = pool_scores_dev; o.pool_n = pool_n_dev;
    hipLaunchKernelGGL(wsp_beam_result_kernel, dim3(U), dim3(256), 0, st, o);
    return decode_done(s, st);
}

}  // extern "C"
