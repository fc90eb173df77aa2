// f0.hip — the DEX f0 tracker on the device: WORLD's DIO + StoneMask (M. Morise) with the arguments DEX-TTS/synthesize.py:50-52
// passes, for a ragged batch of utterances in one call.  The contract is the docstring of tests/world_f0.py (a float64 numpy
// restatement of it is the tests' oracle); it is NOT pinned to pyworld, which this project cannot run: parity with pyworld is
// unmeasured.  Everything is fp64; every reduction has a fixed order and there are no atomics, so a row's result is bitwise
// reproducible and independent of the other rows of the batch.  No FFT: both filters are direct linear convolutions, and StoneMask
// evaluates the handful of DFT bins it reads directly.
//
// DIO:  taps (once per call) -> mean / fp64 copy -> low-cut FIR -> per band: Nuttall FIR -> per (band, event kind): ordered event
//       positions -> per (band, frame): interpolated candidate + score -> per row: best band + the four fix steps.
// StoneMask: one wave per (row, frame).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/dex_amd.h"

// the restatement evaluates every expression as written, one rounding per operation: so does this file
#pragma clang fp contract(off)

namespace {

constexpr int NB_MAX = 16;          // bands (1 + int(log2(ceil / floor) * cio))
constexpr int ROWS = 128;           // rows per launch (their lengths travel as kernel arguments)
constexpr int TILE = 256;           // FIR outputs per workgroup
constexpr int TAPS_MAX = 3900;      // (TILE + 2 * taps + 2) doubles of LDS <= 64 KB
constexpr int FIX_LDS_FRAMES = 2048;  // the fix kernel keeps its frame arrays in LDS up to here, in the workspace beyond
constexpr double EPS = 1e-12;

__host__ __device__ inline int mround(double v) { return v > 0 ? (int)(v + 0.5) : (int)(v - 0.5); }
__host__ __device__ inline int f0_frames(int L, double fs, double fp) { return (int)(1000.0 * L / fs / fp) + 1; }

struct Opts {
    double fs, fp, floor, ceil, cio, ar;
};

// geometry of one call (host-computed, kernel argument)
struct Geo {
    Opts o;
    int nb, Fm, Fc, Lpm, N;          // bands, output row stride F(n_samples), frames of the longest row F(max L), max(L) + 1, low-cut taps
    int T[NB_MAX + 1], off[NB_MAX + 1];   // FIR j = 0: low-cut, j = 1..nb: band j - 1
    long tap[NB_MAX + 1];            // offsets of the taps in the tap region
    double bnd[NB_MAX];              // band boundaries
    long EC;                         // event capacity per (band, kind)
    long RS;                         // doubles per row
    long o_y, o_z, o_s, o_ev, o_cnt, o_cand, o_score, o_fa, o_fb, o_list;   // offsets inside a row
    int n_samples;                   // wav row stride
};

struct Rows {
    int r0, n;                       // first row of this launch, rows in it
    int L[ROWS];
};

__device__ inline double* row_ws(const Geo& g, double* rows, int r) { return rows + (long)r * g.RS; }

// ---- taps: low-cut h = delta - w / sum(w) (centred), Nuttall windows per band; sum(w) in a fixed (sequential) order
__global__ __launch_bounds__(256) void f0_taps_kernel(const Geo g, double* taps) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* red = (double*)smem;
    const int N = g.N;
    const double two_pi = 2.0 * M_PI;
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 1; k <= N; ++k) s += 0.5 - 0.5 * cos(two_pi * k / (N + 1));
        red[0] = s;
    }
    __syncthreads();
    const double sw = red[0];
    for (int k = threadIdx.x; k < N; k += blockDim.x) {
        const double w = 0.5 - 0.5 * cos(two_pi * (k + 1) / (N + 1));
        double h = -w / sw;
        if (k == (N - 1) / 2) h += 1.0;
        taps[k] = h;
    }
    for (int b = 0; b < g.nb; ++b) {
        const int T = g.T[b + 1];
        double* out = taps + g.tap[b + 1];
        for (int n = threadIdx.x; n < T; n += blockDim.x) {
            const double u = (double)n / (T - 1);
            out[n] = 0.355768 - 0.487396 * cos(two_pi * u) + 0.144232 * cos(2.0 * M_PI * 2.0 * u) - 0.012604 * cos(2.0 * M_PI * 3.0 * u);
        }
    }
}

// ---- y = [x, 0] - mean over L + 1 samples (fp32 promoted exactly); one workgroup per row, fixed-order reduction
__global__ __launch_bounds__(256) void f0_mean_kernel(const float* __restrict__ wav, const Geo g, const Rows R, double* rows) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* red = (double*)smem;
    const int r = R.r0 + blockIdx.x, L = R.L[blockIdx.x];
    const float* x = wav + (long)r * g.n_samples;
    double s = 0.0;
    for (int i = threadIdx.x; i < L; i += 256) s += (double)x[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    const double mean = red[0] / (L + 1);
    double* y = row_ws(g, rows, r) + g.o_y;
    for (int i = threadIdx.x; i <= L; i += 256) y[i] = (i < L ? (double)x[i] : 0.0) - mean;
}

// ---- direct linear FIR: out[n] = sum_m h[m] in[n + off - m], n in [0, L + 1), in zero outside.  Grid (tiles, rows, filters):
// filter j of the set is g.T / g.off / g.tap [j0 + j]; its input is the row's slot in_o, its output out_o + j * Lpm.
// The tile's input window and the taps are staged in LDS; the window load is coalesced (consecutive lanes, consecutive samples).
__global__ __launch_bounds__(TILE) void f0_fir_kernel(const Geo g, const Rows R, const double* __restrict__ taps, double* rows,
                                                      int j0, long in_o, long out_o) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int j = j0 + blockIdx.z, T = g.T[j], off = g.off[j];
    const int Lp = R.L[blockIdx.y] + 1;
    const int n0 = blockIdx.x * TILE;
    if (n0 >= Lp) return;
    double* ws = row_ws(g, rows, R.r0 + blockIdx.y);
    const double* in = ws + in_o;
    double* out = ws + out_o + (long)blockIdx.z * g.Lpm;
    double* h = (double*)smem;
    double* win = h + ((T + 1) & ~1);
    const double* tp = taps + g.tap[j];
    for (int m = threadIdx.x; m < T; m += TILE) h[m] = tp[m];
    const int p0 = n0 + off - (T - 1), W = TILE + T - 1;
    for (int q = threadIdx.x; q < W; q += TILE) {
        const int p = p0 + q;
        win[q] = (p >= 0 && p < Lp) ? in[p] : 0.0;
    }
    __syncthreads();
    const int n = n0 + threadIdx.x;
    if (n >= Lp) return;
    const double* wv = win + threadIdx.x + T - 1;
    double acc = 0.0;
    for (int m = 0; m < T; ++m) acc += h[m] * wv[-m];
    out[n] = acc;
}

// ---- events of one (row, band, kind): kind 0: s, 1: -s, 2: d, 3: -d (d_i = s_i - s_{i+1}).  One workgroup walks the signal in
// chunks of 256; a block-wide integer scan (wave ballots) places each event at its ordinal, so the positions come out in order.
__device__ inline double ev_val(const double* s, int kind, int i) {
    const double v = kind < 2 ? s[i] : s[i] - s[i + 1];
    return (kind & 1) ? -v : v;
}

__global__ __launch_bounds__(256) void f0_events_kernel(const Geo g, const Rows R, double* rows) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* wtot = (int*)smem;                 // [4] wave totals
    const int band = blockIdx.x >> 2, kind = blockIdx.x & 3;
    const int L = R.L[blockIdx.y];
    double* ws = row_ws(g, rows, R.r0 + blockIdx.y);
    const double* s = ws + g.o_s + (long)band * g.Lpm;
    double* ev = ws + g.o_ev + (long)blockIdx.x * g.EC;
    const int len = kind < 2 ? L + 1 : L;   // samples of v
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int c0 = 0; c0 < len - 1; c0 += 256) {
        const int i = c0 + threadIdx.x;
        bool hit = false;
        double e = 0.0;
        if (i < len - 1) {
            const double a = ev_val(s, kind, i), b = ev_val(s, kind, i + 1);
            hit = a > 0 && b <= 0;
            if (hit) e = (i + 1) - a / (b - a);
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) wtot[wave] = __popcll(m);
        __syncthreads();
        int before = base;
        for (int w = 0; w < wave; ++w) before += wtot[w];
        const int tot = wtot[0] + wtot[1] + wtot[2] + wtot[3];
        if (hit) {
            const int k = before + __popcll(m & ((1ull << lane) - 1ull));
            if (k < g.EC) ev[k] = e;
        }
        base += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) ((int*)(ws + g.o_cnt))[blockIdx.x] = base;
}

// ---- candidates: per (row, band, frame) the four interval sequences interpolated at t (histc + interp1: segment k = #(x <= t) - 1
// clamped to [0, n - 2]), their mean and spread, the range check, score / (cand + eps)
__device__ inline double ev_interp(const double* e, int n, double fs, double t) {
    // locations x_k = (e_k + e_{k+1}) / 2 / fs, k = 0..n-2 (increasing): count those <= t
    int lo = 0, hi = n - 1;                 // answer in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((e[mid] + e[mid + 1]) / 2.0 / fs <= t) lo = mid + 1; else hi = mid;
    }
    int k = lo - 1;
    k = k < 0 ? 0 : (k > n - 3 ? n - 3 : k);
    const double x0 = (e[k] + e[k + 1]) / 2.0 / fs, x1 = (e[k + 1] + e[k + 2]) / 2.0 / fs;
    const double y0 = fs / (e[k + 1] - e[k]), y1 = fs / (e[k + 2] - e[k + 1]);
    return y0 + (t - x0) * (y1 - y0) / (x1 - x0);
}

__global__ __launch_bounds__(256) void f0_cand_kernel(const Geo g, const Rows R, double* rows) {
    const int i = blockIdx.x * 256 + threadIdx.x, band = blockIdx.z;
    const int L = R.L[blockIdx.y], F = f0_frames(L, g.o.fs, g.o.fp);
    if (i >= F) return;
    double* ws = row_ws(g, rows, R.r0 + blockIdx.y);
    const int* cnt = (const int*)(ws + g.o_cnt) + band * 4;
    const double* ev = ws + g.o_ev + (long)band * 4 * g.EC;
    double c = 0.0, sc = 1e5;
    if (cnt[0] >= 3 && cnt[1] >= 3 && cnt[2] >= 3 && cnt[3] >= 3) {
        const double t = i * g.o.fp / 1000.0;
        double I[4];
        for (int k = 0; k < 4; ++k) I[k] = ev_interp(ev + k * g.EC, cnt[k], g.o.fs, t);
        c = (I[0] + I[1] + I[2] + I[3]) / 4.0;
        const double d0 = I[0] - c, d1 = I[1] - c, d2 = I[2] - c, d3 = I[3] - c;
        sc = sqrt((d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3) / 3.0);
        const double bnd = g.bnd[band];
        if (c > bnd || c < bnd / 2.0 || c > g.o.ceil || c < g.o.floor) { c = 0.0; sc = 1e5; }
    }
    ws[g.o_cand + (long)band * g.Fc + i] = c;
    ws[g.o_score + (long)band * g.Fc + i] = sc / (c + EPS);
}

// ---- best band + fix: steps 0-2 frame-parallel, steps 3-4 (sequential walks) on lane 0.  Frame arrays in LDS up to
// FIX_LDS_FRAMES frames, in the row's workspace beyond.
__device__ inline double f0_select(const double* cand, long Fc, int nb, double cur, double past, int j, double ar) {
    const double ref = (3.0 * cur - past) / 2.0;
    double best = cand[j], bd = fabs(cand[j] - ref);
    for (int b = 1; b < nb; ++b) {
        const double c = cand[(long)b * Fc + j], d = fabs(c - ref);
        if (d < bd) { bd = d; best = c; }
    }
    return fabs(1.0 - best / ref) > ar ? 0.0 : best;
}

__global__ __launch_bounds__(256) void f0_fix_kernel(const Geo g, const Rows R, double* rows, double* f0_out, int lds) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int r = R.r0 + blockIdx.x, L = R.L[blockIdx.x], F = f0_frames(L, g.o.fs, g.o.fp);
    double* ws = row_ws(g, rows, r);
    double* out = f0_out + (long)r * g.Fm;
    double* fa = lds ? (double*)smem : ws + g.o_fa;                   // best, then the running f0
    double* fb = lds ? (double*)smem + FIX_LDS_FRAMES : ws + g.o_fb;  // step-1 values
    int* list = lds ? (int*)((double*)smem + 2 * FIX_LDS_FRAMES) : (int*)(ws + g.o_list);
    const double* cand = ws + g.o_cand;
    const double* score = ws + g.o_score;
    const double ar = g.o.ar;
    const int vrm = (int)(0.5 + 1000.0 / g.o.fp / g.o.floor) * 2 + 1;
    for (int i = F + threadIdx.x; i < g.Fm; i += 256) out[i] = 0.0;
    if (F <= vrm) {
        for (int i = threadIdx.x; i < F; i += 256) out[i] = 0.0;
        return;
    }
    for (int i = threadIdx.x; i < F; i += 256) {
        int bi = 0;
        for (int b = 1; b < g.nb; ++b)
            if (score[(long)bi * g.Fc + i] > score[(long)b * g.Fc + i]) bi = b;
        fa[i] = cand[(long)bi * g.Fc + i];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < F; i += 256)        // step 1
        fb[i] = (i < vrm || i >= F - vrm) ? 0.0 : (fabs((fa[i] - fa[i - 1]) / (EPS + fa[i])) < ar ? fa[i] : 0.0);
    __syncthreads();
    const int c = (vrm - 1) / 2;
    for (int i = threadIdx.x; i < F; i += 256) {      // step 2
        double v = fb[i];
        if (i >= c && i < F - c)
            for (int k = i - c; k <= i + c; ++k)
                if (fb[k] == 0.0) v = 0.0;
        fa[i] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // step 3: voiced -> unvoiced boundaries of the step-2 values, then the forward walks
        int ne = 0;
        for (int n = 0; n < F - 1; ++n)
            if (fa[n] != 0.0 && fa[n + 1] == 0.0) list[ne++] = n;
        for (int q = 0; q < ne; ++q) {
            const int n = list[q], limit = q + 1 < ne ? list[q + 1] : F - 1;
            for (int j = n; j < limit; ++j) {
                const double v = f0_select(cand, g.Fc, g.nb, fa[j], j >= 1 ? fa[j - 1] : fa[j], j + 1, ar);
                fa[j + 1] = v;
                if (v == 0.0) break;
            }
        }
        // step 4: unvoiced -> voiced boundaries of the step-3 values, last to first, backward walks
        int np = 0;
        for (int p = 1; p < F; ++p)
            if (fa[p] != 0.0 && fa[p - 1] == 0.0) list[np++] = p;
        for (int q = np - 1; q >= 0; --q) {
            const int p = list[q], limit = q > 0 ? list[q - 1] : 1;
            for (int j = p; j > limit; --j) {
                const double v = f0_select(cand, g.Fc, g.nb, fa[j], j + 1 < F ? fa[j + 1] : fa[j], j - 1, ar);
                fa[j - 1] = v;
                if (v == 0.0) break;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < F; i += 256) out[i] = fa[i];
}

// ---- StoneMask: one wave per (row, frame).  Window sample k reads x[clamp(r_k - 1, 0, L - 1)], r_k = round((t + (k - hw) / fs) * fs);
// M and D at the bins fix() reads are direct DFT sums (twiddle angle reduced exactly: (j k) mod nfft), per lane in k order, then a
// butterfly over the wave: a fixed order.
struct SmGeo {
    double t, fs, W;
    int hw, L;
    long nfft;
};

__device__ inline double sm_mw(const SmGeo& q, int k) {
    const int r = mround((q.t + (double)(k - q.hw) / q.fs) * q.fs);
    const double tau = (r - 1) / q.fs - q.t;
    return 0.42 + 0.5 * cos(2.0 * M_PI * tau / q.W) + 0.08 * cos(4.0 * M_PI * tau / q.W);
}

template <int NBIN>
__device__ void sm_bins(const SmGeo& q, const float* x, const long* j, double* acc /* [NBIN][4]: Re M, Im M, Re D, Im D */) {
    double a[NBIN][4];
    for (int b = 0; b < NBIN; ++b) a[b][0] = a[b][1] = a[b][2] = a[b][3] = 0.0;
    const int n = 2 * q.hw + 1;
    for (int k = threadIdx.x; k < n; k += 64) {
        const int r = mround((q.t + (double)(k - q.hw) / q.fs) * q.fs);
        const int idx = r - 1 < 0 ? 0 : (r - 1 > q.L - 1 ? q.L - 1 : r - 1);
        const double xv = (double)x[idx];
        const double mw = sm_mw(q, k);
        double dw;
        if (k == 0) dw = -sm_mw(q, 1) / 2.0;
        else if (k == n - 1) dw = sm_mw(q, n - 2) / 2.0;
        else dw = -(sm_mw(q, k + 1) - sm_mw(q, k - 1)) / 2.0;
        const double xm = xv * mw, xd = xv * dw;
        for (int b = 0; b < NBIN; ++b) {
            const long ph = (j[b] * (long)k) % q.nfft;
            double sn, cs;
            sincospi(-2.0 * (double)ph / (double)q.nfft, &sn, &cs);
            a[b][0] += xm * cs; a[b][1] += xm * sn; a[b][2] += xd * cs; a[b][3] += xd * sn;
        }
    }
    for (int b = 0; b < NBIN; ++b)
        for (int c = 0; c < 4; ++c) {
            double v = a[b][c];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            acc[b * 4 + c] = v;
        }
}

__device__ inline long sm_bin(double f, const SmGeo& q, int k) {
    long j = mround(f * q.nfft / q.fs * k) % q.nfft;
    return j;
}

__device__ inline double sm_fix(const SmGeo& q, const double* acc, const long* j, int nh) {
    double num = 0.0, den = 0.0;
    for (int k = 1; k <= nh; ++k) {
        const double* m = acc + (k - 1) * 4;
        const double P = m[0] * m[0] + m[1] * m[1];
        const double ifr = P == 0.0 ? 0.0 : j[k - 1] * q.fs / q.nfft + (m[0] * m[3] - m[1] * m[2]) / P * q.fs / (2.0 * M_PI);
        const double a = sqrt(P);
        num += a * ifr;
        den += a * k;
    }
    return num / (den + EPS);
}

__global__ __launch_bounds__(64) void f0_stonemask_kernel(const float* __restrict__ wav, const Geo g, const Rows R,
                                                          const double* __restrict__ f0_in, double* f0_out) {
    const int i = blockIdx.x, r = R.r0 + blockIdx.y, L = R.L[blockIdx.y];
    const int F = f0_frames(L, g.o.fs, g.o.fp);
    double* out = f0_out + (long)r * g.Fm + i;
    if (i >= F) { if (threadIdx.x == 0) *out = 0.0; return; }
    const double f0 = f0_in[(long)r * g.Fm + i];
    const double fs = g.o.fs;
    if (!(f0 > 40.0 && f0 <= fs / 12.0)) { if (threadIdx.x == 0) *out = 0.0; return; }
    SmGeo q;
    q.t = i * g.o.fp / 1000.0; q.fs = fs; q.L = L;
    q.hw = (int)(1.5 * fs / f0 + 1);
    q.W = (2 * q.hw + 1) / fs;
    q.nfft = 1L << (2 + (int)log2((double)(2 * q.hw + 1)));
    const float* x = wav + (long)r * g.n_samples;
    long j[6];
    double acc[24];
    j[0] = sm_bin(f0, q, 1); j[1] = sm_bin(f0, q, 2);
    sm_bins<2>(q, x, j, acc);
    const double f1 = sm_fix(q, acc, j, 2);
    double res = 0.0;
    if (f1 > 0.0 && f1 <= 2.0 * f0) {
        const int nh = min((int)(fs / 2.0 / f0), 6);
        for (int k = 0; k < 6; ++k) j[k] = sm_bin(f1, q, k + 1 <= nh ? k + 1 : 1);
        sm_bins<6>(q, x, j, acc);
        const double f2 = sm_fix(q, acc, j, nh);
        res = fabs(f2 - f0) > 0.2 * f0 ? f0 : f2;
    }
    if (threadIdx.x == 0) *out = res;
}

// ---- peak normalisation (synthesize.py:46): out = float(x / max|x|) per row in fp64, 0 past the row's length and for a silent row
__global__ __launch_bounds__(256) void f0_peak_kernel(const float* __restrict__ wav, const Rows R, int n_samples, float* out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* red = (double*)smem;
    const int r = R.r0 + blockIdx.x, L = R.L[blockIdx.x];
    const float* x = wav + (long)r * n_samples;
    float* o = out + (long)r * n_samples;
    double m = 0.0;
    for (int i = threadIdx.x; i < L; i += 256) m = fmax(m, fabs((double)x[i]));
    red[threadIdx.x] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    const double pk = red[0];
    for (int i = threadIdx.x; i < n_samples; i += 256) o[i] = (i < L && pk > 0.0) ? (float)((double)x[i] / pk) : 0.0f;
}

// ---- host side
Opts opts_of(const DexF0Opts* p) {
    if (!p) return Opts{22050.0, 256.0 / 22050.0 * 1000.0, 71.0, 800.0, 2.0, 0.1};
    return Opts{p->fs, p->frame_period_ms, p->f0_floor, p->f0_ceil, p->channels_in_octave, p->allowed_range};
}

bool opts_ok(const Opts& o) {
    if (!(o.fs > 0) || !(o.fp > 0) || !(o.floor > 0) || !(o.floor < o.ceil) || !(o.cio > 0) || !(o.ar >= 0)) return false;
    if (!std::isfinite(o.fs) || !std::isfinite(o.fp) || !std::isfinite(o.ceil) || !std::isfinite(o.cio) || !std::isfinite(o.ar)) return false;
    const double nbd = 1.0 + std::floor(std::log2(o.ceil / o.floor) * o.cio);
    return nbd <= NB_MAX;
}

bool lengths_ok(const int* lengths, int B, int n_samples) {
    if (!lengths || B < 1 || n_samples < 1) return false;
    for (int b = 0; b < B; ++b)
        if (lengths[b] < 1 || lengths[b] > n_samples) return false;
    return true;
}

// geometry for rows of at most Lmax samples; false if a filter is out of range
bool make_geo(const Opts& o, int Lmax, int n_samples, Geo& g) {
    std::memset(&g, 0, sizeof g);
    g.o = o;
    g.n_samples = n_samples;
    g.nb = 1 + (int)(std::log2(o.ceil / o.floor) * o.cio);
    g.Fm = f0_frames(n_samples, o.fs, o.fp);
    g.Fc = f0_frames(Lmax, o.fs, o.fp);
    g.Lpm = Lmax + 1;
    g.N = 2 * mround(o.fs / 50.0) + 1;
    if (g.nb < 1 || g.nb > NB_MAX || g.N < 1 || g.N > TAPS_MAX || g.Fm < 1) return false;
    g.T[0] = g.N; g.off[0] = (g.N - 1) / 2; g.tap[0] = 0;
    long tp = (g.N + 1) & ~1L;
    for (int b = 0; b < g.nb; ++b) {
        g.bnd[b] = o.floor * std::pow(2.0, (b + 1) / o.cio);
        const int hl = mround(o.fs / g.bnd[b] / 2.0);
        if (hl < 1 || 4 * hl > TAPS_MAX) return false;
        g.T[b + 1] = 4 * hl; g.off[b + 1] = 2 * hl; g.tap[b + 1] = tp;
        tp += 4 * hl;
    }
    g.EC = g.Lpm / 2 + 2;
    const long Fr = g.Fc;
    long off = 0;
    auto take = [&](long n) { const long at = off; off += (n + 1) & ~1L; return at; };
    g.o_y = take(g.Lpm);
    g.o_z = take(g.Lpm);
    g.o_s = take((long)g.nb * g.Lpm);
    g.o_ev = take((long)g.nb * 4 * g.EC);
    g.o_cnt = take((g.nb * 4 + 1) / 2);
    g.o_cand = take((long)g.nb * Fr);
    g.o_score = take((long)g.nb * Fr);
    g.o_fa = take(Fr);
    g.o_fb = take(Fr);
    g.o_list = take((Fr + 1) / 2);
    g.RS = off;
    return true;
}

long tap_doubles(const Geo& g) { return g.tap[g.nb] + g.T[g.nb] + 2; }

int max_len(const int* lengths, int B) {
    int m = 0;
    for (int b = 0; b < B; ++b) m = lengths[b] > m ? lengths[b] : m;
    return m;
}

template <class Fn>
int for_row_chunks(const int* lengths, int B, Fn fn) {
    for (int r0 = 0; r0 < B; r0 += ROWS) {
        Rows R;
        R.r0 = r0; R.n = B - r0 < ROWS ? B - r0 : ROWS;
        for (int k = 0; k < R.n; ++k) R.L[k] = lengths[r0 + k];
        fn(R);
        if (hipGetLastError() != hipSuccess) return DEX_ERR_HIP;
    }
    return DEX_OK;
}

}  // namespace

extern "C" {

int dex_f0_frames(int n_samples, const DexF0Opts* opts) {
    const Opts o = opts_of(opts);
    if (n_samples < 1 || !opts_ok(o)) return DEX_ERR_ARG;
    return f0_frames(n_samples, o.fs, o.fp);
}

size_t dex_f0_workspace_bytes(int B, const int* lengths_host, const DexF0Opts* opts) {
    const Opts o = opts_of(opts);
    if (B < 1 || !lengths_host || !opts_ok(o)) return 0;
    for (int b = 0; b < B; ++b)
        if (lengths_host[b] < 1) return 0;
    const int Lmax = max_len(lengths_host, B);
    Geo g;
    if (!make_geo(o, Lmax, Lmax, g)) return 0;
    return (size_t)(tap_doubles(g) + (long)B * g.RS) * sizeof(double) + 256;
}

int dex_f0_peak_normalize(const float* wav_dev, const int* lengths_host, int B, int n_samples, float* out_dev, dex_stream_t s) {
    if (!wav_dev || !out_dev || !lengths_ok(lengths_host, B, n_samples)) return DEX_ERR_ARG;
    return for_row_chunks(lengths_host, B, [&](const Rows& R) {
        f0_peak_kernel<<<R.n, 256, 256 * sizeof(double), (hipStream_t)s>>>(wav_dev, R, n_samples, out_dev);
    });
}

int dex_f0_dio(const float* wav_dev, const int* lengths_host, int B, int n_samples, const DexF0Opts* opts, double* f0_dev, void* ws,
               size_t ws_bytes, dex_stream_t s) {
    const Opts o = opts_of(opts);
    if (!wav_dev || !f0_dev || !ws || !opts_ok(o) || !lengths_ok(lengths_host, B, n_samples)) return DEX_ERR_ARG;
    const int Lmax = max_len(lengths_host, B);
    Geo g;
    if (!make_geo(o, Lmax, n_samples, g)) return DEX_ERR_ARG;
    if (ws_bytes < dex_f0_workspace_bytes(B, lengths_host, opts)) return DEX_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)s;
    double* taps = (double*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    double* rows = taps + tap_doubles(g);
    int Tmax = 0;
    for (int j = 1; j <= g.nb; ++j) Tmax = g.T[j] > Tmax ? g.T[j] : Tmax;
    const int tiles = (g.Lpm + TILE - 1) / TILE;
    const int Fmax = g.Fc, use_lds = Fmax <= FIX_LDS_FRAMES;
    const size_t fix_lds = use_lds ? (size_t)2 * FIX_LDS_FRAMES * sizeof(double) + (FIX_LDS_FRAMES / 2 + 1) * sizeof(int) : 16;
    f0_taps_kernel<<<1, 256, 16, st>>>(g, taps);
    if (hipGetLastError() != hipSuccess) return DEX_ERR_HIP;
    return for_row_chunks(lengths_host, B, [&](const Rows& R) {
        f0_mean_kernel<<<R.n, 256, 256 * sizeof(double), st>>>(wav_dev, g, R, rows);
        f0_fir_kernel<<<dim3(tiles, R.n, 1), TILE, (size_t)(2 * g.N + TILE + 2) * sizeof(double), st>>>(g, R, taps, rows, 0, g.o_y, g.o_z);
        f0_fir_kernel<<<dim3(tiles, R.n, g.nb), TILE, (size_t)(2 * Tmax + TILE + 2) * sizeof(double), st>>>(g, R, taps, rows, 1, g.o_z, g.o_s);
        f0_events_kernel<<<dim3(g.nb * 4, R.n), 256, 16, st>>>(g, R, rows);
        f0_cand_kernel<<<dim3((Fmax + 255) / 256, R.n, g.nb), 256, 0, st>>>(g, R, rows);
        f0_fix_kernel<<<R.n, 256, fix_lds, st>>>(g, R, rows, f0_dev, use_lds);
    });
}

int dex_f0_stonemask(const float* wav_dev, const int* lengths_host, int B, int n_samples, const DexF0Opts* opts, const double* f0_in_dev,
                     double* f0_out_dev, void* ws, size_t ws_bytes, dex_stream_t s) {
    (void)ws; (void)ws_bytes;
    const Opts o = opts_of(opts);
    if (!wav_dev || !f0_in_dev || !f0_out_dev || f0_in_dev == f0_out_dev || !opts_ok(o) || !lengths_ok(lengths_host, B, n_samples))
        return DEX_ERR_ARG;
    Geo g;
    if (!make_geo(o, max_len(lengths_host, B), n_samples, g)) return DEX_ERR_ARG;
    return for_row_chunks(lengths_host, B, [&](const Rows& R) {
        f0_stonemask_kernel<<<dim3(g.Fm, R.n), 64, 0, (hipStream_t)s>>>(wav_dev, g, R, f0_in_dev, f0_out_dev);
    });
}

}  // extern "C"
