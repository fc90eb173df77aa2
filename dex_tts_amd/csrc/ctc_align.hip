// ctc_align.hip — CTC forced alignment and text likelihood on the device: for logits [B, T, V] and a known text per row, the Viterbi
// path over the 2 L + 1 states of the CTC trellis (word / character timings) and the negative log-likelihood of the text
// (F.ctc_loss), for a ragged batch.  The contract is the docstring of dex_tts_amd/ctc_align.py; tests/ctc_ref.py restates it.
//
// lse:      one wave per frame: the maximum, then sum exp(x - max) in fp64, lane-strided in a fixed order, one xor butterfly each.
// trellis:  one workgroup per utterance, two modes.  max: a' = max3(stay, step, skip) + (double)x, candidates in that order, the first
//           maximal one wins; one fp64 add and two compares per cell, so the path is the restatement's bit for bit.  sum: a =
//           logsumexp3 + (x - lse) in fp64.  A thread owns R consecutive states and keeps them in registers for the whole utterance.
//           Register form (S <= 512): one wave, R = 1 .. 8, the state below a lane's first comes by one __shfl_up per frame (two for
//           R = 1), no barrier; the logits of the lane's labels are prefetched through a ring.  LDS form (S <= 2047): up to 1024
//           threads of one or two states, the running column double-buffered in LDS, one barrier per frame; a wave wholly outside
//           the reachable band writes -inf and skips the arithmetic.  Both forms are one kernel body.
// pointers: two bits per cell (0 stay, 1 step, 2 skip), packed by state over 16 frames a word, word (t / 16, s) at (t / 16) S + s —
//           in LDS while S ceil(T / 16) words fit beside the column, else in the workspace, same layout.  Thread 0 walks them back
//           from the final state with s clamped to [0, S), writing states and spans; thread l then averages the posteriors of
//           target position l over its span in frame order.
// Nothing here depends on the batch: a row's outputs are bitwise those of the row alone, whichever form the batch selects.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/dex_amd.h"

#pragma clang fp contract(off)

namespace {

constexpr int LDS_BYTES = 160 * 1024;      // what one workgroup may allocate on gfx950
constexpr int HEAD_BYTES = 32;             // final a[S - 1], a[S - 2] and the has-alignment flag, in front of the dynamic LDS
constexpr int REG_STATES = 512;            // register form: 64 lanes x 8 states
constexpr int MAX_V = 65536;
constexpr double NEG_INF = -__builtin_inf();

struct CtcGeo {
    int T, V, Lmax, blank;
    int NS;                                // LDS form: states per column buffer (threads x R); 0 in the register form
    long bp_stride;                        // back-pointer words per utterance in the workspace; 0: they live in LDS
};

// ---------------------------------------------------------------------------------------------------------------- lse
// lse[b, t] = m + log(sum_v exp((double)x[v] - m)), m the frame's maximum (0 where that is not finite); 0 past a row's frames
__global__ __launch_bounds__(256) void ctc_lse_kernel(const float* __restrict__ x, const int32_t* __restrict__ frames, int B, int T, int V,
                                                      double* __restrict__ lse) {
    const long f = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (f >= (long)B * T) return;
    const int b = (int)(f / T), t = (int)(f % T);
    if (t >= frames[b]) {
        if (lane == 0) lse[f] = 0.0;
        return;
    }
    const float* r = x + f * V;
    float m = -INFINITY;
    for (int v = lane; v < V; v += 64) m = fmaxf(m, r[v]);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    const double mm = (m - m == 0.f) ? (double)m : 0.0;
    double s = 0.0;
    for (int v = lane; v < V; v += 64) s += exp((double)r[v] - mm);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) lse[f] = mm + log(s);
}

// ---------------------------------------------------------------------------------------------------------------- trellis
// one cell.  MODE 1: the first maximal candidate in the order stay, step, skip, its index in k.  MODE 0: logsumexp of the three, -inf
// where all are.
template <int MODE>
__device__ __forceinline__ double ctc_cell(double stay, double step, double skip, double e, int& k) {
    double m = stay;
    k = 0;
    if (step > m) { m = step; k = 1; }
    if (skip > m) { m = skip; k = 2; }
    if (MODE == 1) return m + e;
    if (stay == NEG_INF && step == NEG_INF && skip == NEG_INF) return NEG_INF;      // (a NaN term is not -inf: it reaches the result)
    return m + log(exp(stay - m) + exp(step - m) + exp(skip - m)) + e;
}

template <int R> struct Ring { static constexpr int P = R <= 4 ? 8 : 4; };

template <int R, bool LDSF, int MODE>
__global__ __launch_bounds__(LDSF ? 1024 : 64) void ctc_trellis_kernel(const float* __restrict__ logits, const double* __restrict__ lse,
                                                                       const int32_t* __restrict__ frames, const int32_t* __restrict__ targets,
                                                                       const int32_t* __restrict__ tlens, const CtcGeo g, uint32_t* __restrict__ gbp,
                                                                       double* __restrict__ nll, int32_t* __restrict__ states,
                                                                       int32_t* __restrict__ spans, double* __restrict__ tok,
                                                                       double* __restrict__ score) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int P = Ring<R>::P;
    double* fin = (double*)smem;
    int* okp = (int*)(smem + 16);
    double* abuf = (double*)(smem + HEAD_BYTES);
    uint32_t* sbp = (uint32_t*)(smem + HEAD_BYTES + (LDSF ? (size_t)2 * g.NS * sizeof(double) : 0));
    const int tid = threadIdx.x, b = blockIdx.x, nthr = blockDim.x;
    const int Tb = frames[b], L = tlens[b], S = 2 * L + 1;
    const int Lm = g.Lmax > 0 ? g.Lmax : 1;
    const float* X = logits + (long)b * g.T * g.V;
    const double* LS = lse + (long)b * g.T;
    const int32_t* Y = targets + (long)b * Lm;
    uint32_t* bp = g.bp_stride ? gbp + (long)b * g.bp_stride : sbp;
    const int s0 = tid * R;
    auto label = [&](int l) { const int v = Y[l]; return v < 0 ? 0 : (v >= g.V ? g.V - 1 : v); };      // validated on the host; clamped anyway

    int lab[R];
    bool can[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int s = s0 + r;
        lab[r] = g.blank;
        can[r] = false;
        if (s < S && (s & 1)) {
            const int l = (s - 1) >> 1;
            lab[r] = label(l);
            if (l >= 1) can[r] = lab[r] != label(l - 1);
        }
    }

    auto load = [&](int t, float (&c)[R], double& l) {
#pragma unroll
        for (int r = 0; r < R; ++r) c[r] = t < Tb ? X[(long)t * g.V + lab[r]] : 0.f;
        if (MODE == 0) l = t < Tb ? LS[t] : 0.0;
    };

    double a[R], pl[P];
    float pf[P][R];
    uint32_t word[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { a[r] = NEG_INF; word[r] = 0u; }
#pragma unroll
    for (int j = 0; j < P; ++j) { pl[j] = 0.0; load(j, pf[j], pl[j]); }

    const int w0 = (tid & ~63) * R, w1 = w0 + 64 * R - 1;              // the states of this wave
    for (int t0 = 0; t0 < Tb; t0 += P) {
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int t = t0 + j;
            if (t < Tb) {
                float c[R];
                const double l = pl[j];
#pragma unroll
                for (int r = 0; r < R; ++r) c[r] = pf[j][r];
                load(t + P, pf[j], pl[j]);
                const int hi = 2 * t + 1, lo = S - 2 * (Tb - t);      // the band: reachable from the start, and the end from it
                if (t == 0) {
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int s = s0 + r;
                        const double e = MODE == 0 ? (double)c[r] - l : (double)c[r];
                        a[r] = (s <= 1 && s < S && s >= lo) ? e : NEG_INF;
                    }
                } else {
                    double old[R], up1 = NEG_INF, up2 = NEG_INF;
#pragma unroll
                    for (int r = 0; r < R; ++r) old[r] = a[r];
                    if (LDSF) {
                        const double* prev = abuf + (size_t)((t - 1) & 1) * g.NS;
                        if (s0 >= 1) up1 = prev[s0 - 1];
                        if (R == 1 && s0 >= 2) up2 = prev[s0 - 2];
                    } else {
                        const double u1 = __shfl_up(old[R - 1], 1);
                        if (tid >= 1) up1 = u1;
                        if (R == 1) {
                            const double u2 = __shfl_up(old[0], 2);
                            if (tid >= 2) up2 = u2;
                        }
                    }
                    const bool live = !LDSF || (w0 <= hi && w1 >= lo && w0 < S);
                    if (live) {
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            const int s = s0 + r;
                            const double step = r >= 1 ? old[r >= 1 ? r - 1 : 0] : up1;
                            const double back = r >= 2 ? old[r >= 2 ? r - 2 : 0] : (r == 1 ? up1 : up2);
                            const double e = MODE == 0 ? (double)c[r] - l : (double)c[r];
                            int k;
                            const double v = ctc_cell<MODE>(old[r], step, can[r] ? back : NEG_INF, e, k);
                            const bool in = s < S && s <= hi && s >= lo;
                            a[r] = in ? v : NEG_INF;
                            if (MODE == 1) word[r] |= (uint32_t)(in ? k : 0) << (2 * (t & 15));
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < R; ++r) a[r] = NEG_INF;
                    }
                }
                if (LDSF) {
                    double* cur = abuf + (size_t)(t & 1) * g.NS;
#pragma unroll
                    for (int r = 0; r < R; ++r) cur[s0 + r] = a[r];
                    __syncthreads();
                }
                if (MODE == 1 && ((t & 15) == 15 || t == Tb - 1)) {
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if (s0 + r < S) bp[(long)(t >> 4) * S + s0 + r] = word[r];
                        word[r] = 0u;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (s0 + r == S - 1) fin[0] = a[r];
        if (s0 + r == S - 2) fin[1] = a[r];
    }
    __syncthreads();

    if (MODE == 0) {
        if (tid != 0) return;
        const double a1 = fin[0];
        double out;
        if (L == 0) {
            out = -a1;
        } else {
            const double a2 = fin[1];
            double m = a1;
            if (a2 > m) m = a2;
            out = (a1 == NEG_INF && a2 == NEG_INF) ? -NEG_INF : -(m + log(exp(a1 - m) + exp(a2 - m)));
        }
        nll[b] = out;
        return;
    }

    int32_t* St = states + (long)b * g.T;
    int32_t* Sp = spans + (long)b * g.Lmax * 2;
    double* Tk = tok + (long)b * g.Lmax;
    const double qnan = __builtin_nan("");
    for (int t = Tb + tid; t < g.T; t += nthr) St[t] = -1;
    for (int l = L + tid; l < g.Lmax; l += nthr) { Sp[2 * l] = -1; Sp[2 * l + 1] = -1; Tk[l] = qnan; }
    if (tid == 0) {
        int fs = S - 1;
        double best = fin[0];
        if (L > 0 && fin[1] > fin[0]) { fs = S - 2; best = fin[1]; }
        double sl = 0.0;
        for (int t = 0; t < Tb; ++t) sl += LS[t];
        const double sc = best - sl;
        score[b] = sc;
        const bool ok = !(sc == NEG_INF || sc != sc);
        *okp = ok ? 1 : 0;
        if (ok) {
            int s = fs, ck = -1, cs = -1;
            uint32_t w = 0u;
            if (s & 1) Sp[s] = Tb;                                    // target position (s - 1) / 2 ends at the last frame
            for (int t = Tb - 1; t >= 0; --t) {
                St[t] = s;
                int ns = s;
                if (t > 0) {
                    const int kw = t >> 4;
                    if (kw != ck || s != cs) { w = bp[(long)kw * S + s]; ck = kw; cs = s; }
                    ns = s - (int)((w >> (2 * (t & 15))) & 3u);
                    ns = ns < 0 ? 0 : (ns > S - 1 ? S - 1 : ns);
                }
                if (t == 0 || ns != s) {
                    if (s & 1) Sp[s - 1] = t;                        // first frame of (s - 1) / 2
                    if (t > 0 && (ns & 1)) Sp[ns] = t;               // one past the last frame of (ns - 1) / 2
                }
                s = ns;
            }
        }
    }
    __syncthreads();
    if (!*okp) {
        for (int t = tid; t < Tb; t += nthr) St[t] = -1;
        for (int l = tid; l < L; l += nthr) { Sp[2 * l] = -1; Sp[2 * l + 1] = -1; Tk[l] = qnan; }
        return;
    }
    for (int l = tid; l < L; l += nthr) {
        const int t0 = Sp[2 * l], t1 = Sp[2 * l + 1], v = label(l);
        double p = qnan;
        if (t0 >= 0 && t1 > t0 && t1 <= Tb) {
            p = 0.0;
            for (int t = t0; t < t1; ++t) p += exp((double)X[(long)t * g.V + v] - LS[t]);
            p = p / (double)(t1 - t0);
        }
        Tk[l] = p;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
struct Plan {
    bool ldsf;
    int R, threads, NS;
    size_t lds_fixed;                      // dynamic LDS without the back-pointers
};

Plan plan_for(int Smax) {
    Plan p{};
    if (Smax <= REG_STATES) {
        p.ldsf = false; p.R = 1; p.threads = 64;
        while (p.R * 64 < Smax) p.R *= 2;
        p.NS = 0;
    } else {
        p.ldsf = true; p.R = Smax <= 1024 ? 1 : 2;
        p.threads = ((Smax + p.R - 1) / p.R + 63) / 64 * 64;
        p.NS = p.threads * p.R;
    }
    p.lds_fixed = HEAD_BYTES + (size_t)2 * p.NS * sizeof(double);
    return p;
}

long bp_words(int S, int T) { return (long)S * ((T + 15) / 16); }

size_t up256(size_t n) { return (n + 255) / 256 * 256; }

bool dims_ok(int B, int T, int V, int Lmax) {
    return B >= 1 && B <= DEX_CTC_MAX_ROWS && T >= 1 && T <= DEX_CTC_MAX_FRAMES && V >= 1 && V <= MAX_V && Lmax >= 0 && Lmax <= DEX_CTC_MAX_TARGET;
}

// workspace: lse [B][T] fp64 | targets [B][max(Lmax, 1)] | target lengths [B] | frames [B] | back-pointers [B][(2 Lmax + 1) ceil(T / 16)]
// (the last only where the worst row of these dimensions does not fit LDS)
struct Ws {
    double* lse; int32_t *targets, *tlens, *frames; uint32_t* bp;
    long bp_stride; size_t bytes;
};

Ws layout(void* base, int B, int T, int Lmax) {
    Ws w{};
    size_t off = 0;
    auto take = [&](size_t bytes) { void* p = base ? (char*)base + off : nullptr; off += up256(bytes); return p; };
    w.lse = (double*)take((size_t)B * T * sizeof(double));
    w.targets = (int32_t*)take((size_t)B * (Lmax > 0 ? Lmax : 1) * sizeof(int32_t));
    w.tlens = (int32_t*)take((size_t)B * sizeof(int32_t));
    w.frames = (int32_t*)take((size_t)B * sizeof(int32_t));
    const int Smax = 2 * Lmax + 1;
    const long words = bp_words(Smax, T);
    if (plan_for(Smax).lds_fixed + (size_t)words * 4 > (size_t)LDS_BYTES) {
        w.bp_stride = words;
        w.bp = (uint32_t*)take((size_t)B * words * 4);
    }
    w.bytes = off;
    return w;
}

template <int R, bool LDSF, int MODE>
void launch(int B, int threads, size_t lds, const float* logits, const Ws& w, const CtcGeo& g, double* nll, int32_t* states, int32_t* spans, double* tok,
            double* score, hipStream_t st) {
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ctc_trellis_kernel<R, LDSF, MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
        attr = true;
    }
    ctc_trellis_kernel<R, LDSF, MODE><<<B, threads, lds, st>>>(logits, w.lse, w.frames, w.targets, w.tlens, g, w.bp, nll, states, spans, tok, score);
}

template <int MODE>
void dispatch(const Plan& p, int B, size_t lds, const float* logits, const Ws& w, const CtcGeo& g, double* nll, int32_t* states, int32_t* spans,
              double* tok, double* score, hipStream_t st) {
    if (p.ldsf) {
        if (p.R == 1) launch<1, true, MODE>(B, p.threads, lds, logits, w, g, nll, states, spans, tok, score, st);
        else launch<2, true, MODE>(B, p.threads, lds, logits, w, g, nll, states, spans, tok, score, st);
        return;
    }
    switch (p.R) {
        case 1: launch<1, false, MODE>(B, 64, lds, logits, w, g, nll, states, spans, tok, score, st); break;
        case 2: launch<2, false, MODE>(B, 64, lds, logits, w, g, nll, states, spans, tok, score, st); break;
        case 4: launch<4, false, MODE>(B, 64, lds, logits, w, g, nll, states, spans, tok, score, st); break;
        default: launch<8, false, MODE>(B, 64, lds, logits, w, g, nll, states, spans, tok, score, st); break;
    }
}

int run(const float* logits, const int32_t* frames, int B, int T, int V, const int32_t* targets, const int32_t* tlens, int Lmax, int blank,
        bool align, int32_t* states, int32_t* spans, double* tok, double* score, double* nll, void* ws, size_t ws_bytes, hipStream_t st) {
    if (!logits || !frames || !tlens || !ws || !dims_ok(B, T, V, Lmax) || (Lmax > 0 && !targets)) return DEX_ERR_ARG;
    if (blank < 0 || blank >= V) return DEX_ERR_ARG;
    if (align ? (!states || !spans || !tok || !score) : !nll) return DEX_ERR_ARG;
    int Smax = 1;
    long words = 0;
    for (int b = 0; b < B; ++b) {
        const int L = tlens[b];
        if (frames[b] < 1 || frames[b] > T || L < 0 || L > Lmax) return DEX_ERR_ARG;
        for (int l = 0; l < L; ++l) {
            const int v = targets[(long)b * Lmax + l];
            if (v < 0 || v >= V || v == blank) return DEX_ERR_ARG;
        }
        const int S = 2 * L + 1;
        Smax = S > Smax ? S : Smax;
        const long wd = bp_words(S, frames[b]);
        words = wd > words ? wd : words;
    }
    const Ws w = layout(ws, B, T, Lmax);
    if (ws_bytes < w.bytes) return DEX_ERR_WORKSPACE;

    if (Lmax > 0 && hipMemcpyAsync(w.targets, targets, (size_t)B * Lmax * sizeof(int32_t), hipMemcpyHostToDevice, st) != hipSuccess) return DEX_ERR_HIP;
    if (hipMemcpyAsync(w.tlens, tlens, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st) != hipSuccess) return DEX_ERR_HIP;
    if (hipMemcpyAsync(w.frames, frames, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st) != hipSuccess) return DEX_ERR_HIP;
    const long nf = (long)B * T;
    ctc_lse_kernel<<<(unsigned)((nf + 3) / 4), 256, 0, st>>>(logits, w.frames, B, T, V, w.lse);

    const Plan p = plan_for(Smax);
    CtcGeo g{};
    g.T = T; g.V = V; g.Lmax = Lmax; g.blank = blank; g.NS = p.NS; g.bp_stride = 0;
    if (nll) dispatch<0>(p, B, p.lds_fixed, logits, w, g, nll, nullptr, nullptr, nullptr, nullptr, st);
    if (align) {
        size_t lds = p.lds_fixed + (size_t)words * 4;
        if (lds > (size_t)LDS_BYTES) {                                 // (then the worst row of these dimensions does not fit either)
            if (!w.bp) return DEX_ERR_WORKSPACE;
            g.bp_stride = w.bp_stride;
            lds = p.lds_fixed;
        }
        dispatch<1>(p, B, lds, logits, w, g, nullptr, states, spans, tok, score, st);
    }
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

}  // namespace

extern "C" {

size_t dex_ctc_workspace_bytes(int B, int T, int V, int Lmax) { return dims_ok(B, T, V, Lmax) ? layout(nullptr, B, T, Lmax).bytes : 0; }

int dex_ctc_nll(const float* logits_dev, const int32_t* frames_host, int B, int T, int V, const int32_t* targets_host,
                const int32_t* target_lengths_host, int Lmax, int blank, double* nll_dev, void* workspace_dev, size_t workspace_bytes,
                dex_stream_t stream) {
    return run(logits_dev, frames_host, B, T, V, targets_host, target_lengths_host, Lmax, blank, false, nullptr, nullptr, nullptr, nullptr, nll_dev,
               workspace_dev, workspace_bytes, (hipStream_t)stream);
}

int dex_ctc_align(const float* logits_dev, const int32_t* frames_host, int B, int T, int V, const int32_t* targets_host,
                  const int32_t* target_lengths_host, int Lmax, int blank, int32_t* states_dev, int32_t* spans_dev, double* token_scores_dev,
                  double* score_dev, double* nll_dev, void* workspace_dev, size_t workspace_bytes, dex_stream_t stream) {
    return run(logits_dev, frames_host, B, T, V, targets_host, target_lengths_host, Lmax, blank, true, states_dev, spans_dev, token_scores_dev,
               score_dev, nll_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
