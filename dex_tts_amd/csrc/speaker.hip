// speaker.hip — the reference's speaker-similarity score on the device (src/metric.py:69-95, 115-142, Evaluater.calculate_accept /
// calculate_asv_score): the d-vector of resemblyzer's VoiceEncoder and the cosine of two of them.  C ABI dex_spk_*.
//
//   normalize_volume     one workgroup per utterance: mean(wav^2) in fp64 (a fixed-order tree), the gain rounded to fp32, wav x gain.
//   spk_mel_kernel       one mel frame per workgroup: the 400 windowed samples (zero outside the utterance: center = True's zero pad
//                        and embed_utterance's pad to the last slice) against a 400-entry twiddle table indexed by k n mod 400 - the
//                        dense real-DFT basis [400] x [400, 402] without materialising it - in fp64, |X|^2 of 201 bins, the Slaney
//                        triangles of 40 channels.  400 = 16 x 25 is no power of two; the dense form is 161 k multiply-adds per frame,
//                        all parallel, against the LSTM's 1.35 M per frame in 480 dependent steps: a mixed-radix transform buys nothing.
//   input projections    x W_ih^T + (b_ih + b_hh) of a layer for ALL steps as one exact-fp32 MFMA GEMM (launch_igemm) ahead of that
//                        layer's recurrence; layer 0's K = 40 is zero-padded to 64.
//   spk_lstm_kernel      the recurrence.  One workgroup of 1024 threads owns ROWS = 4 rows (partials) for all T steps; h and c never
//                        leave the chip (h in LDS, c in a register).  Thread n owns gate column n of the 1024: per step it streams its
//                        column of W_hh (packed [k / 4][1024][4]: one 16-byte load per lane per 4 k, a wave's load is 1 KB contiguous)
//                        from L2 and runs 4 independent 256-term fmaf chains, k ascending, seeded with the input projection.  The
//                        columns meet in LDS once per step; thread n then owns (row n / 256, unit n % 256) for the gate update.
//                        No workgroup ever waits for another.
//   spk_head_kernel      Linear(256, 256) + ReLU + L2 normalisation of the top layer's final hidden state, one row per workgroup.
//   spk_utt_kernel       mean over an utterance's partial embeddings (ascending), L2 normalisation.
//   spk_cosine_kernel    <a, b> / (|a| |b|), one row per workgroup.
// Every per-row sum has a fixed order that does not depend on the batch: a row's result is bitwise the row run alone.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dex_amd.h"
#include "kernels.h"
#include "weight_store.h"

namespace {

constexpr int SR = 16000, NFFT = 400, HOP = 160, NB = 201, NMEL = DEX_SPK_MELS, PT = DEX_SPK_PARTIAL_FRAMES;
constexpr int H = DEX_SPK_EMBED, G = 4 * H, LAYERS = 3;
constexpr int MEL_LD = 64;           // layer 0's input row: 40 mels + 24 zeros (the GEMM's K is a multiple of 32)
constexpr int ROWS = 4;              // rows per workgroup of the recurrence: ROWS x 256 (row, unit) pairs = its 1024 threads
constexpr int TAB = 128;             // table entries per launch (they travel as kernel arguments: 2 KB)
constexpr long MAX_ROWS_T = 1L << 24;   // P x T of one call: keeps every element index of the workspace far inside 2^63 and grids inside 2^31

struct Tab { int n; int a[TAB], b[TAB], c[TAB], d[TAB]; };

// deterministic sum of one double per thread over a 256-thread workgroup (LDS tree); every thread gets the total
__device__ __forceinline__ double block_sum256(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double t = red[0];
    __syncthreads();
    return t;
}
__device__ __forceinline__ float block_sum256f(float v, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = __fadd_rn(red[tid], red[tid + s]);
        __syncthreads();
    }
    const float t = red[0];
    __syncthreads();
    return t;
}

// a = utterance lengths; rows r0 .. r0 + n of wav / out [.][ld]
__global__ __launch_bounds__(256) void spk_volume_kernel(const float* wav, float* out, long ld, int r0, double target, const Tab R) {
    __shared__ double red[256];
    const int r = blockIdx.x, tid = threadIdx.x, L = R.a[r];
    const float* w = wav + (long)(r0 + r) * ld;
    float* o = out + (long)(r0 + r) * ld;
    double s = 0.0;
    for (int i = tid; i < L; i += 256) { const double x = (double)w[i]; s += x * x; }
    const double mean = block_sum256(s, red) / (double)L;
    const double change = target - 10.0 * log10(mean);
    const float gain = change < 0.0 ? 1.f : (float)pow(10.0, change / 20.0);       // (mean = 0: change = +inf, gain = inf, 0 x inf = NaN as numpy)
    for (int i = tid; i < ld; i += 256) o[i] = i < L ? (change < 0.0 ? w[i] : __fmul_rn(w[i], gain)) : 0.f;
}

struct MelP { const float* wav; long wav_ld; const double* tw; const double* win; const double* filt; const int2* range;
              float* out; long out_rows; int ld; int e0; };

// entry e of the table: utterance a[e] (length c[e]), first mel frame b[e]; frame f of it -> out[((e0 + e) out_rows + f) ld + m].
// frames at or past d[e] (dex_spk_mel's rows shorter than the batch) are 0.
__global__ __launch_bounds__(256) void spk_mel_kernel(const MelP p, const Tab R) {
    __shared__ double xs[NFFT], cs[NFFT], sn[NFFT], pw[NB];
    const int f = blockIdx.x, e = blockIdx.y, tid = threadIdx.x;
    float* o = p.out + ((long)(p.e0 + e) * p.out_rows + f) * p.ld;
    if (f >= R.d[e]) {
        if (tid < p.ld) o[tid] = 0.f;
        return;
    }
    const int L = R.c[e];
    const float* w = p.wav + (long)R.a[e] * p.wav_ld;
    const long base = (long)(R.b[e] + f) * HOP - NFFT / 2;
    for (int n = tid; n < NFFT; n += 256) {
        const long i = base + n;
        xs[n] = (i >= 0 && i < L) ? (double)w[i] * p.win[n] : 0.0;
        cs[n] = p.tw[2 * n]; sn[n] = p.tw[2 * n + 1];
    }
    __syncthreads();
    if (tid < NB) {
        double re = 0.0, im = 0.0;
        int idx = 0;
        for (int n = 0; n < NFFT; ++n) {
            re = fma(xs[n], cs[idx], re);
            im = fma(xs[n], sn[idx], im);
            idx += tid; if (idx >= NFFT) idx -= NFFT;
        }
        pw[tid] = re * re + im * im;
    }
    __syncthreads();
    if (tid < NMEL) {
        const int2 rg = p.range[tid];
        double acc = 0.0;
        for (int k = rg.x; k < rg.y; ++k) acc = fma(p.filt[tid * NB + k], pw[k], acc);
        o[tid] = (float)acc;
    } else if (tid < p.ld) o[tid] = 0.f;
}

// [rows][40] -> [rows][64], zero padded
__global__ __launch_bounds__(256) void spk_pad_kernel(const float* in, float* out, long rows) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * MEL_LD) return;
    const long r = i / MEL_LD; const int c = (int)(i - r * MEL_LD);
    out[i] = c < NMEL ? in[r * NMEL + c] : 0.f;
}

__device__ __forceinline__ float sigmoidf_(float x) { return __fdiv_rn(1.f, 1.f + expf(-x)); }

struct LstmP { const float* gi; const float4* whh; float* y; float* hT; int P, T; };

__global__ __launch_bounds__(1024) void spk_lstm_kernel(const LstmP p) {
    __shared__ __attribute__((aligned(16))) float hs[ROWS][H];
    __shared__ float gs[ROWS][G];
    const int tid = threadIdx.x, row0 = blockIdx.x * ROWS;
    const int ur = tid >> 8, uj = tid & (H - 1);               // the (row, unit) this thread updates
    const bool uvalid = row0 + ur < p.P;
    float c = 0.f;
    hs[ur][uj] = 0.f;
    const float* gp[ROWS];
    bool valid[ROWS];
    float gn[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        valid[r] = row0 + r < p.P;
        gp[r] = p.gi + (long)(valid[r] ? row0 + r : 0) * p.T * G + tid;
        gn[r] = valid[r] ? gp[r][0] : 0.f;
    }
    const float4* wp = p.whh + tid;
    __syncthreads();
    for (int t = 0; t < p.T; ++t) {
        float acc[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) acc[r] = gn[r];
        auto chain = [&](const float4 (&w)[8], int q) {          // k = 4 q .. 4 q + 31, ascending
#pragma unroll
            for (int u = 0; u < 8; ++u) {
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    const float4 hv = *reinterpret_cast<const float4*>(&hs[r][4 * (q + u)]);
                    acc[r] = fmaf(hv.x, w[u].x, acc[r]);
                    acc[r] = fmaf(hv.y, w[u].y, acc[r]);
                    acc[r] = fmaf(hv.z, w[u].z, acc[r]);
                    acc[r] = fmaf(hv.w, w[u].w, acc[r]);
                }
            }
        };
        if (t + 1 < p.T) {                                      // the next step's input projection travels under this step's chain
#pragma unroll
            for (int r = 0; r < ROWS; ++r) gn[r] = valid[r] ? gp[r][(long)(t + 1) * G] : 0.f;
        }
        // 8 x 16 B of the column in flight per lane, then their 32 k of the chain; the other three waves of the SIMD cover the wait.
        // (Two such groups alternating, the second loading under the first's multiplies, took 126 registers and ran 13-19 % SLOWER.)
#pragma unroll 1
        for (int q0 = 0; q0 < H / 4; q0 += 8) {
            float4 w[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) w[u] = wp[(q0 + u) * G];
            chain(w, q0);
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) gs[r][tid] = acc[r];
        __syncthreads();
        const float ig = sigmoidf_(gs[ur][uj]), fg = sigmoidf_(gs[ur][H + uj]), gg = tanhf(gs[ur][2 * H + uj]), og = sigmoidf_(gs[ur][3 * H + uj]);
        c = fmaf(fg, c, ig * gg);
        const float hn = og * tanhf(c);
        hs[ur][uj] = hn;
        if (uvalid) {
            if (p.y) p.y[((long)(row0 + ur) * p.T + t) * H + uj] = hn;
            if (p.hT && t == p.T - 1) p.hT[(long)(row0 + ur) * H + uj] = hn;
        }
        __syncthreads();
    }
}

// embeds[row] = l2norm(relu(h W^T + b)); wT [k][j]
__global__ __launch_bounds__(256) void spk_head_kernel(const float* hT, const float* wT, const float* b, float* out) {
    __shared__ float hsh[H];
    __shared__ float red[256];
    const int j = threadIdx.x; const long row = blockIdx.x;
    hsh[j] = hT[row * H + j];
    __syncthreads();
    float acc = b[j];
    for (int k = 0; k < H; ++k) acc = fmaf(hsh[k], wT[k * H + j], acc);
    const float v = fmaxf(acc, 0.f);
    const float n2 = block_sum256f(v * v, red);
    out[row * H + j] = __fdiv_rn(v, __fsqrt_rn(n2));
}

// utterance e: partial embeddings a[e] .. a[e] + b[e] -> out[u0 + e] = l2norm(mean)
__global__ __launch_bounds__(256) void spk_utt_kernel(const float* pe, float* out, int u0, const Tab R) {
    __shared__ float red[256];
    const int j = threadIdx.x, e = blockIdx.x, n = R.b[e];
    const float* s = pe + (long)R.a[e] * H + j;
    float acc = 0.f;
    for (int i = 0; i < n; ++i) acc = __fadd_rn(acc, s[(long)i * H]);
    const float m = __fdiv_rn(acc, (float)n);
    const float n2 = block_sum256f(m * m, red);
    out[(long)(u0 + e) * H + j] = __fdiv_rn(m, __fsqrt_rn(n2));
}

__global__ __launch_bounds__(256) void spk_cosine_kernel(const float* a, const float* b, int D, float* out) {
    __shared__ double red[256];
    const long row = blockIdx.x;
    double ab = 0.0, aa = 0.0, bb = 0.0;
    for (int i = threadIdx.x; i < D; i += 256) {
        const double x = a[row * D + i], y = b[row * D + i];
        ab += x * y; aa += x * x; bb += y * y;
    }
    ab = block_sum256(ab, red); aa = block_sum256(aa, red); bb = block_sum256(bb, red);
    if (threadIdx.x == 0) out[row] = (float)(ab / (sqrt(aa) * sqrt(bb)));
}

// W [N][K] row-major -> [Kpad][N] (rows past K zero)
__global__ __launch_bounds__(256) void spk_pack_t_kernel(const float* w, float* out, int N, int K, int Kpad) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Kpad * N) return;
    const int k = i / N, n = i - k * N;
    out[i] = k < K ? w[(long)n * K + k] : 0.f;
}
// W_hh [1024][256] -> [k / 4][1024][4]
__global__ __launch_bounds__(256) void spk_pack_hh_kernel(const float4* w, float4* out) {
    const int i = blockIdx.x * 256 + threadIdx.x;      // = q * G + col
    if (i >= (H / 4) * G) return;
    const int q = i / G, col = i - q * G;
    out[i] = w[col * (H / 4) + q];
}
__global__ __launch_bounds__(256) void spk_add_kernel(const float* a, const float* b, float* out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = __fadd_rn(a[i], b[i]);
}

// librosa.filters.mel(sr = 16000, n_fft = 400, n_mels = 40, fmin = 0, fmax = 8000, htk = False, norm = 'slaney'), fp64, rounded to
// fp32 as librosa returns it
double hz_to_mel(double f) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
double mel_to_hz(double m) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}
void mel_basis(std::vector<double>& filt, std::vector<int2>& range) {
    filt.assign((size_t)NMEL * NB, 0.0); range.assign(NMEL, make_int2(0, 0));
    std::vector<double> pts(NMEL + 2);
    const double lo = hz_to_mel(0.0), hi = hz_to_mel(SR / 2.0);
    for (int i = 0; i < NMEL + 2; ++i) pts[i] = mel_to_hz(lo + (hi - lo) * (double)i / (NMEL + 1));
    for (int m = 0; m < NMEL; ++m) {
        const double enorm = 2.0 / (pts[m + 2] - pts[m]);
        int k0 = NB, k1 = 0;
        for (int k = 0; k < NB; ++k) {
            const double f = (double)k * SR / NFFT;
            const double lower = (f - pts[m]) / (pts[m + 1] - pts[m]), upper = (pts[m + 2] - f) / (pts[m + 2] - pts[m + 1]);
            const double w = std::fmax(0.0, std::fmin(lower, upper)) * enorm;
            filt[(size_t)m * NB + k] = (double)(float)w;
            if (w != 0.0) { k0 = k < k0 ? k : k0; k1 = k + 1; }
        }
        if (k0 < k1) range[m] = make_int2(k0, k1);
    }
}

bool rows_ok(const int32_t* v, int B, int lo, int hi) {
    if (!v || B < 1) return false;
    for (int b = 0; b < B; ++b)
        if (v[b] < lo || v[b] > hi) return false;
    return true;
}

}  // namespace

struct DexSpk : dex::WeightStore {
    DexSpk() : WeightStore("speaker-encoder ") {}
    void* tables = nullptr;
    const double* tw = nullptr; const double* win = nullptr; const double* filt = nullptr; const int2* range = nullptr;
    const float* wih[LAYERS] = {}; const float4* whh[LAYERS] = {}; const float* bias[LAYERS] = {};
    const float* lin_wT = nullptr; const float* lin_b = nullptr;
};

namespace {

constexpr size_t TW_OFF = 0, WIN_OFF = TW_OFF + 2 * NFFT * sizeof(double), FILT_OFF = WIN_OFF + NFFT * sizeof(double),
                 RANGE_OFF = FILT_OFF + (size_t)NMEL * NB * sizeof(double), TABLES_BYTES = RANGE_OFF + NMEL * sizeof(int2);

std::string lkey(const char* what, int l) { return std::string("lstm.") + what + "_l" + std::to_string(l); }

int in_width(int l) { return l == 0 ? NMEL : H; }
int in_pad(int l) { return l == 0 ? MEL_LD : H; }

int finalize(DexSpk* s, hipStream_t st) {
    if (int rc = s->begin_finalize()) return rc;
    for (int l = 0; l < LAYERS; ++l) {
        float* wih = s->alloc((long)in_pad(l) * G); float* whh = s->alloc((long)H * G); float* b = s->alloc(G);
        if (s->alloc_rc != DEX_OK) return s->alloc_rc;
        hipLaunchKernelGGL(spk_pack_t_kernel, dim3((in_pad(l) * G + 255) / 256), dim3(256), 0, st, s->R(lkey("weight_ih", l)), wih, G, in_width(l), in_pad(l));
        hipLaunchKernelGGL(spk_pack_hh_kernel, dim3((H / 4) * G / 256), dim3(256), 0, st, (const float4*)s->R(lkey("weight_hh", l)), (float4*)whh);
        hipLaunchKernelGGL(spk_add_kernel, dim3(G / 256), dim3(256), 0, st, s->R(lkey("bias_ih", l)), s->R(lkey("bias_hh", l)), b, G);
        s->wih[l] = wih; s->whh[l] = (const float4*)whh; s->bias[l] = b;
    }
    float* lw = s->alloc((long)H * H);
    if (s->alloc_rc != DEX_OK) return s->alloc_rc;
    hipLaunchKernelGGL(spk_pack_t_kernel, dim3(H * H / 256), dim3(256), 0, st, s->R("linear.weight"), lw, H, H, H);
    s->lin_wT = lw; s->lin_b = s->R("linear.bias");
    if (hipGetLastError() != hipSuccess) return s->fail(DEX_ERR_HIP, "packing the speaker-encoder weights failed");
    s->finalized = true;
    return DEX_OK;
}

// workspace: x0 [rows][64] | gi [rows][1024] | ya, yb [rows][256] | hT [P][256] | partial embeddings [P][256]
struct Ws { float *x0, *gi, *ya, *yb, *hT, *pe; };
size_t ws_bytes(long P, long T) {
    const long rows = P * T;
    return (size_t)(rows * (MEL_LD + G + 2 * H) + 2 * P * H) * sizeof(float) + 256;
}
Ws carve(void* ws, long P, long T) {
    float* f = (float*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    const long rows = P * T;
    Ws w;
    w.x0 = f; w.gi = w.x0 + rows * MEL_LD; w.ya = w.gi + rows * G; w.yb = w.ya + rows * H; w.hT = w.yb + rows * H; w.pe = w.hT + P * H;
    return w;
}

// the network on x0 [P T][64] -> out [P][256]
int enqueue_network(DexSpk* s, const Ws& w, int P, int T, float* out, hipStream_t st) {
    const long rows = (long)P * T;
    const float* cur = w.x0;
    float* ys[2] = {w.ya, w.yb};
    for (int l = 0; l < LAYERS; ++l) {
        dex::IGemmP g{};          // gi = x W_ih^T + (b_ih + b_hh): [P T][1024]
        g.A = cur; g.lda = in_pad(l); g.a_bstride = 0; g.Hi = 1; g.Wi = (int)rows; g.Cin = in_pad(l);
        g.KH = 1; g.KW = 1; g.sh = 1; g.sw = 1; g.step_h = 1; g.step_w = 1; g.Ho = 1; g.Wo = (int)rows;
        g.W = s->wih[l]; g.N = G; g.K = in_pad(l); g.ksplit = 1; g.groups = 1; g.bias = s->bias[l];
        g.C = w.gi; g.ldc = G; g.c_bstride = 0; g.OHf = 1; g.OWf = (int)rows; g.osh = 1; g.osw = 1;
        g.inmask_ws = 1; g.outmask_ws = 1; g.gate_nstride = 1; g.B = 1;
        dex::launch_igemm(g, dex::PREC_FP32, st);
        const bool last = l == LAYERS - 1;
        LstmP lp{w.gi, s->whh[l], last ? nullptr : ys[l & 1], last ? w.hT : nullptr, P, T};
        hipLaunchKernelGGL(spk_lstm_kernel, dim3((P + ROWS - 1) / ROWS), dim3(1024), 0, st, lp);
        cur = ys[l & 1];
    }
    hipLaunchKernelGGL(spk_head_kernel, dim3(P), dim3(256), 0, st, w.hT, s->lin_wT, s->lin_b, out);
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

}  // namespace

extern "C" {

int dex_spk_create(DexSpk** out) {
    if (!out) return DEX_ERR_ARG;
    *out = nullptr;
    std::vector<unsigned char> host(TABLES_BYTES, 0);
    double* tw = (double*)(host.data() + TW_OFF); double* win = (double*)(host.data() + WIN_OFF);
    for (int n = 0; n < NFFT; ++n) {
        const double a = 2.0 * M_PI * (double)n / NFFT;
        tw[2 * n] = cos(a); tw[2 * n + 1] = -sin(a);
        win[n] = 0.5 - 0.5 * cos(a);                              // periodic Hann
    }
    std::vector<double> filt; std::vector<int2> range;
    mel_basis(filt, range);
    std::memcpy(host.data() + FILT_OFF, filt.data(), filt.size() * sizeof(double));
    std::memcpy(host.data() + RANGE_OFF, range.data(), range.size() * sizeof(int2));
    DexSpk* s = new DexSpk();
    if (hipMalloc(&s->tables, TABLES_BYTES) != hipSuccess || hipMemcpy(s->tables, host.data(), TABLES_BYTES, hipMemcpyHostToDevice) != hipSuccess) {
        if (s->tables) (void)hipFree(s->tables);
        delete s;
        return DEX_ERR_HIP;
    }
    unsigned char* d = (unsigned char*)s->tables;
    s->tw = (const double*)(d + TW_OFF); s->win = (const double*)(d + WIN_OFF); s->filt = (const double*)(d + FILT_OFF);
    s->range = (const int2*)(d + RANGE_OFF);
    for (int l = 0; l < LAYERS; ++l) {
        s->add(lkey("weight_ih", l), {G, in_width(l)});
        s->add(lkey("weight_hh", l), {G, H});
        s->add(lkey("bias_ih", l), {G});
        s->add(lkey("bias_hh", l), {G});
    }
    s->add("linear.weight", {H, H});
    s->add("linear.bias", {H});
    *out = s;
    return DEX_OK;
}

void dex_spk_destroy(DexSpk* s) {
    if (!s) return;
    s->release();
    if (s->tables) (void)hipFree(s->tables);
    delete s;
}

const char* dex_spk_last_error(const DexSpk* s) { return s ? s->err.c_str() : "null speaker-encoder context"; }

int dex_spk_load(DexSpk* s, const char* key, const float* w_dev, const int64_t* shape, int ndim, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!key || !w_dev || !shape) return s->fail(DEX_ERR_ARG, "null pointer argument");
    if (int rc = s->load(key, w_dev, shape, ndim, (hipStream_t)stream, false)) return rc;
    for (const auto& k : s->keys)
        if (!s->raw.at(k).loaded) return DEX_OK;
    return finalize(s, (hipStream_t)stream);
}

size_t dex_spk_forward_workspace_bytes(int P, int T) {
    if (P < 1 || T < 1 || (long)P * T > MAX_ROWS_T) return 0;
    return ws_bytes(P, T);
}

size_t dex_spk_workspace_bytes(int P, int max_samples) {
    if (max_samples < 1) return 0;
    return dex_spk_forward_workspace_bytes(P, PT);
}

int dex_spk_mel(DexSpk* s, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, float* mel_dev, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!wav_dev || !mel_dev || !lengths_host) return s->fail(DEX_ERR_ARG, "null pointer argument");
    if (B < 1 || n_samples < 1) return s->fail(DEX_ERR_ARG, "B and n_samples must be >= 1");
    if (!rows_ok(lengths_host, B, 1, n_samples)) return s->fail(DEX_ERR_ARG, "row lengths must lie in [1, n_samples]");
    const int F = n_samples / HOP + 1;
    for (int e0 = 0; e0 < B; e0 += TAB) {
        Tab R;
        std::memset(&R, 0, sizeof R);
        R.n = B - e0 < TAB ? B - e0 : TAB;
        for (int e = 0; e < R.n; ++e) { R.a[e] = e0 + e; R.b[e] = 0; R.c[e] = lengths_host[e0 + e]; R.d[e] = lengths_host[e0 + e] / HOP + 1; }
        MelP p{wav_dev, n_samples, s->tw, s->win, s->filt, s->range, mel_dev, F, NMEL, e0};
        hipLaunchKernelGGL(spk_mel_kernel, dim3(F, R.n), dim3(256), 0, (hipStream_t)stream, p, R);
    }
    return hipGetLastError() == hipSuccess ? DEX_OK : s->fail(DEX_ERR_HIP, "kernel launch failed");
}

int dex_spk_forward(DexSpk* s, const float* mels_dev, int P, int T, float* embeds_dev, void* workspace_dev, size_t workspace_bytes,
                    dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!mels_dev || !embeds_dev || !workspace_dev) return s->fail(DEX_ERR_ARG, "null pointer argument");
    if (P < 1 || T < 1) return s->fail(DEX_ERR_ARG, "P and T must be >= 1");
    if ((long)P * T > MAX_ROWS_T) return s->fail(DEX_ERR_ARG, "P x T must not exceed %ld", MAX_ROWS_T);
    if (!s->finalized) return s->fail(DEX_ERR_STATE, "the speaker-encoder weights are not loaded");
    if (workspace_bytes < ws_bytes(P, T)) return s->fail(DEX_ERR_WORKSPACE, "workspace too small (dex_spk_forward_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    const Ws w = carve(workspace_dev, P, T);
    const long rows = (long)P * T;
    hipLaunchKernelGGL(spk_pad_kernel, dim3((unsigned)((rows * MEL_LD + 255) / 256)), dim3(256), 0, st, mels_dev, w.x0, rows);
    const int rc = enqueue_network(s, w, P, T, embeds_dev, st);
    return rc ? s->fail(rc, "kernel launch failed") : DEX_OK;
}

int dex_spk_embed(DexSpk* s, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, const int32_t* slices_host,
                  const int32_t* slice_start_host, int P, float* embeds_dev, float* partials_dev, void* workspace_dev, size_t workspace_bytes,
                  dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!wav_dev || !lengths_host || !slices_host || !slice_start_host || !embeds_dev || !workspace_dev)
        return s->fail(DEX_ERR_ARG, "null pointer argument");
    if (B < 1 || n_samples < 1 || P < 1) return s->fail(DEX_ERR_ARG, "B, n_samples and P must be >= 1");
    if (!rows_ok(lengths_host, B, 1, n_samples)) return s->fail(DEX_ERR_ARG, "row lengths must lie in [1, n_samples]");
    long total = 0;
    for (int b = 0; b < B; ++b) {
        if (slices_host[b] < 1) return s->fail(DEX_ERR_ARG, "every utterance needs at least one slice");
        total += slices_host[b];
    }
    if (total != P) return s->fail(DEX_ERR_ARG, "the slice counts add up to %ld, not P = %d", total, P);
    if ((long)P * PT > MAX_ROWS_T) return s->fail(DEX_ERR_ARG, "too many partials");
    for (int i = 0; i < P; ++i)
        if (slice_start_host[i] < 0 || slice_start_host[i] > (1 << 24)) return s->fail(DEX_ERR_ARG, "slice starts must lie in [0, 2^24]");
    if (!s->finalized) return s->fail(DEX_ERR_STATE, "the speaker-encoder weights are not loaded");
    if (workspace_bytes < ws_bytes(P, PT)) return s->fail(DEX_ERR_WORKSPACE, "workspace too small (dex_spk_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    const Ws w = carve(workspace_dev, P, PT);
    // mel frames of every partial straight into layer 0's input rows
    {
        int b = 0, left = slices_host[0];
        for (int e0 = 0; e0 < P; e0 += TAB) {
            Tab R;
            std::memset(&R, 0, sizeof R);
            R.n = P - e0 < TAB ? P - e0 : TAB;
            for (int e = 0; e < R.n; ++e) {
                while (left == 0) { ++b; left = slices_host[b]; }
                --left;
                R.a[e] = b; R.b[e] = slice_start_host[e0 + e]; R.c[e] = lengths_host[b]; R.d[e] = PT;
            }
            MelP p{wav_dev, n_samples, s->tw, s->win, s->filt, s->range, w.x0, PT, MEL_LD, e0};
            hipLaunchKernelGGL(spk_mel_kernel, dim3(PT, R.n), dim3(256), 0, st, p, R);
        }
    }
    float* pe = partials_dev ? partials_dev : w.pe;
    int rc = enqueue_network(s, w, P, PT, pe, st);
    int first = 0;
    for (int u0 = 0; u0 < B && rc == DEX_OK; u0 += TAB) {
        Tab R;
        std::memset(&R, 0, sizeof R);
        R.n = B - u0 < TAB ? B - u0 : TAB;
        for (int e = 0; e < R.n; ++e) { R.a[e] = first; R.b[e] = slices_host[u0 + e]; first += slices_host[u0 + e]; }
        hipLaunchKernelGGL(spk_utt_kernel, dim3(R.n), dim3(256), 0, st, pe, embeds_dev, u0, R);
        if (hipGetLastError() != hipSuccess) rc = DEX_ERR_HIP;
    }
    return rc ? s->fail(rc, "kernel launch failed") : DEX_OK;
}

int dex_spk_normalize_volume(DexSpk* s, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, double target_dbfs,
                             float* out_dev, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!wav_dev || !out_dev || !lengths_host) return s->fail(DEX_ERR_ARG, "null pointer argument");
    if (B < 1 || n_samples < 1) return s->fail(DEX_ERR_ARG, "B and n_samples must be >= 1");
    if (!rows_ok(lengths_host, B, 1, n_samples)) return s->fail(DEX_ERR_ARG, "row lengths must lie in [1, n_samples]");
    if (!(target_dbfs == target_dbfs)) return s->fail(DEX_ERR_ARG, "target_dbfs is NaN");
    for (int r0 = 0; r0 < B; r0 += TAB) {
        Tab R;
        std::memset(&R, 0, sizeof R);
        R.n = B - r0 < TAB ? B - r0 : TAB;
        for (int e = 0; e < R.n; ++e) R.a[e] = lengths_host[r0 + e];
        hipLaunchKernelGGL(spk_volume_kernel, dim3(R.n), dim3(256), 0, (hipStream_t)stream, wav_dev, out_dev, (long)n_samples, r0, target_dbfs, R);
    }
    return hipGetLastError() == hipSuccess ? DEX_OK : s->fail(DEX_ERR_HIP, "kernel launch failed");
}

int dex_spk_cosine(DexSpk* s, const float* a_dev, const float* b_dev, int B, int D, float* cos_dev, dex_stream_t stream) {
    if (!s) return DEX_ERR_ARG;
    if (!a_dev || !b_dev || !cos_dev) return s->fail(DEX_ERR_ARG, "null pointer argument");
    if (B < 1 || D < 1) return s->fail(DEX_ERR_ARG, "B and D must be >= 1");
    hipLaunchKernelGGL(spk_cosine_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a_dev, b_dev, D, cos_dev);
    return hipGetLastError() == hipSuccess ? DEX_OK : s->fail(DEX_ERR_HIP, "kernel launch failed");
}

}  // extern "C"
