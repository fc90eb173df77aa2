// wavprep.hip — the reference wav preparation of DEX-TTS/synthesize.py:40-47 on the device, for a ragged, mixed-rate batch:
// librosa.effects.trim (top_db = 30), resampy.resample (kaiser_best) and the fp64 peak normalisation.  The contract is the docstring
// of tests/wav_prep.py (a float64 numpy restatement of it is the tests' oracle); it is NOT pinned to librosa or resampy, which this
// project cannot run: parity with them is unmeasured.  Everything is fp64; every reduction has a fixed order (or is a max / min,
// exact in any order) and there are no atomics, so a row's result is bitwise reproducible and independent of the other rows.
//
// Trim:      per (row, hop block) one wave sums x^2 -> per row: frame mse = sum of frame/hop blocks, max, dB test, first / last.
// Resample:  window table (built once by the caller, dex_wav_resample_table) -> per (row, tile of 256 outputs): the tile's input
//            span staged in LDS, outputs sorted by table offset, each running resampy's two wings in its order.
// Peak:      per (row, tile) max|x| -> per (row, tile) the row max from the tile maxima and float(x / max).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>

#include "../../include/dex_amd.h"

// the restatement evaluates every expression as written, one rounding per operation: so does this file
#pragma clang fp contract(off)

namespace {

constexpr int ROWS = 64;            // rows per launch (their geometry travels as kernel arguments)
constexpr int TILE = 256;           // resampler outputs per workgroup, one per thread
constexpr int RS_THREADS = 256;
// input samples a resampler tile may stage in LDS: 64 KB minus the tile's sort keys; beyond, the taps read global memory
constexpr int LDS_SPAN = (65536 - TILE * (int)sizeof(int)) / (int)sizeof(double);
constexpr int PEAK_TILE = 2048;     // samples per peak-normalisation workgroup (8 per thread)
constexpr int TABLE_MAX = 1 << 22;  // window table entries

struct Rows {
    int r0, n;                      // first row of this launch, rows in it
    int L[ROWS], off[ROWS], sr[ROWS], Lo[ROWS];   // input length and offset, source rate, output length (resample); L only otherwise
};

template <class Fn>
int for_row_chunks(int B, Fn fill_and_launch) {
    for (int r0 = 0; r0 < B; r0 += ROWS) {
        Rows R;
        std::memset(&R, 0, sizeof R);
        R.r0 = r0; R.n = B - r0 < ROWS ? B - r0 : ROWS;
        fill_and_launch(R);
        if (hipGetLastError() != hipSuccess) return DEX_ERR_HIP;
    }
    return DEX_OK;
}

// ---------------------------------------------------------------------------------------------------------------- trim
struct TrimGeo {
    double top_db;
    int frame, hop, K, pad, reflect;  // K = frame / hop blocks per frame
    int n_samples;                    // wav row stride
    int Fm;                           // frames of a row of n_samples samples: the stride of the optional mse output
    long RS;                          // block sums per row in the workspace
};

__device__ inline int reflect_index(int i, int L) {
    if (L == 1) return 0;
    const int P = 2 * (L - 1);
    int m = i % P;
    if (m < 0) m += P;
    return m >= L ? P - m : m;
}

// block k of row r: sum of x^2 over padded samples [k hop, (k + 1) hop); lane j takes j, j + 64, ... in order, then a butterfly
__global__ __launch_bounds__(256) void wav_trim_blocks_kernel(const float* __restrict__ wav, const TrimGeo g, const Rows R, double* blocks) {
    const int lane = threadIdx.x & 63, k = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int L = R.L[blockIdx.y], NB = L / g.hop + g.K;          // F + K - 1 blocks, F = 1 + L / hop
    if (k >= NB) return;
    const float* x = wav + (long)(R.r0 + blockIdx.y) * g.n_samples;
    const long p0 = (long)k * g.hop - g.pad;
    double s = 0.0;
    for (int q = lane; q < g.hop; q += 64) {
        long i = p0 + q;
        double v = 0.0;
        if (i >= 0 && i < L) v = (double)x[i];
        else if (g.reflect) v = (double)x[reflect_index((int)i, L)];
        s += v * v;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) blocks[(long)(R.r0 + blockIdx.y) * g.RS + k] = s;
}

__device__ inline double frame_mse(const double* b, int f, const TrimGeo& g) {
    double s = b[f];
    for (int j = 1; j < g.K; ++j) s += b[f + j];
    return s / g.frame;
}

// one workgroup per row over its F frames: (the frame mse, if asked for,) max mse, then the first and last frame above the threshold (max / min: exact in any order)
__global__ __launch_bounds__(256) void wav_trim_bounds_kernel(const TrimGeo g, const Rows R, const double* __restrict__ blocks, int* bounds,
                                                               double* mse_out) {
    __shared__ double red[256];
    __shared__ int lo[256], hi[256];
    const int r = R.r0 + blockIdx.x, L = R.L[blockIdx.x], F = 1 + L / g.hop;
    const double* b = blocks + (long)r * g.RS;
    double m = 0.0;
    for (int f = threadIdx.x; f < F; f += 256) m = fmax(m, frame_mse(b, f, g));
    if (mse_out)
        for (int f = threadIdx.x; f < g.Fm; f += 256) mse_out[(long)r * g.Fm + f] = f < F ? frame_mse(b, f, g) : 0.0;
    red[threadIdx.x] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    const double ref_db = 10.0 * log10(fmax(1e-10, red[0]));
    int first = INT_MAX, last = -1;
    for (int f = threadIdx.x; f < F; f += 256) {
        const double db = 10.0 * log10(fmax(1e-10, frame_mse(b, f, g))) - ref_db;
        if (db > -g.top_db) { first = min(first, f); last = max(last, f); }
    }
    lo[threadIdx.x] = first; hi[threadIdx.x] = last;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) { lo[threadIdx.x] = min(lo[threadIdx.x], lo[threadIdx.x + w]); hi[threadIdx.x] = max(hi[threadIdx.x], hi[threadIdx.x + w]); }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool any = hi[0] >= 0;
        bounds[2 * r] = any ? lo[0] * g.hop : 0;
        bounds[2 * r + 1] = any ? min(L, (hi[0] + 1) * g.hop) : 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------- resample
struct RsOpts {
    int num_zeros, precision;
    double beta, rolloff;
};

struct RsGeo {
    int num_table, nwin;            // 2^precision, N + 1
    int sr_new, in_stride, out_stride;
};

// I0 by its power series sum (x^2 / 4)^k / (k!)^2, summed in k order until a term no longer moves the sum
__device__ inline double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, s = 1.0;
    for (int k = 1; k < 1000; ++k) {
        term = term * q / ((double)k * (double)k);
        const double t = s + term;
        if (t == s) break;
        s = t;
    }
    return s;
}

// tab[j] = (win[j], win[j + 1]), tab[N] = (win[N], win[N]): one 16-byte load gives a tap's win and its delta (0 at N), scaled or not
__global__ __launch_bounds__(256) void wav_window_kernel(const RsOpts o, int N, double2* tab) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j > N) return;
    const double u = o.rolloff * ((double)j * ((double)o.num_zeros / (double)N));
    const double y = M_PI * (u == 0.0 ? 1.0e-20 : u);
    const double sinc_win = o.rolloff * (sin(y) / y);
    const double a = (double)j / (double)N;
    const double taper = bessel_i0(o.beta * sqrt(1.0 - a * a)) / bessel_i0(o.beta);
    const double w = taper * sinc_win;
    tab[j].x = w;
    if (j > 0) tab[j - 1].y = w;
    if (j == N) tab[j].y = w;
}

struct RowRate {
    double ratio, inv, scale;
    int step;
    bool scaled;
};

__host__ __device__ inline RowRate row_rate(int sr_orig, int sr_new, int num_table) {
    RowRate q;
    q.ratio = (double)sr_new / (double)sr_orig;
    q.inv = 1.0 / q.ratio;
    q.scale = q.ratio < 1.0 ? q.ratio : 1.0;
    q.step = (int)(q.scale * num_table);
    q.scaled = q.ratio < 1.0;
    return q;
}

// one wing of resampy's loop: taps x[base + dir * i], i = 0 .. min(count, (nwin - offset) / step) - 1, added to acc in that order
template <class T>
__device__ inline double rs_wing(const double2* __restrict__ tab, const RowRate& q, const RsGeo& g, double frac, int count, const T* x,
                                 int base, int dir, double acc) {
    const double index_frac = frac * g.num_table;
    const int offset = (int)index_frac;
    const double eta = index_frac - offset;
    const int lim = (g.nwin - offset) / q.step;
    const int cnt = count < lim ? count : lim;
    for (int i = 0; i < cnt; ++i) {
        const double2 p = tab[offset + i * q.step];
        double w0 = p.x, w1 = p.y;
        if (q.scaled) { w0 = q.ratio * w0; w1 = q.ratio * w1; }      // resampy scales the table, then differences it
        const double weight = w0 + eta * (w1 - w0);
        acc = acc + weight * (double)x[base + dir * i];
    }
    return acc;
}

// grid (output tiles, rows): tile outputs [t0, t0 + TILE) of one row; zeros past the row's output length up to out_stride.
// The tile's outputs are sorted by their table offset (a bitonic sort of (offset, index) keys in LDS) and thread j computes sorted
// output j: the 64 lanes of a wave then gather from a quarter of the offset range of the table per tap.  Each output's arithmetic
// is unchanged by the order.  (1024 outputs per workgroup, 4 per thread, narrow that to a sixteenth but were slower: 693 vs 494 us
// at B = 32, 118 vs 36 us at B = 1, fewer workgroups and a longer sort.)
template <bool LDS>
__global__ __launch_bounds__(RS_THREADS) void wav_resample_kernel(const float* __restrict__ wav, const RsGeo g, const Rows R,
                                                                   const double2* __restrict__ tab, double* out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int key[TILE];
    double* xs_lds = (double*)smem;
    const int row = R.r0 + blockIdx.y, L = R.L[blockIdx.y], Lo = R.Lo[blockIdx.y];
    const float* x = wav + (long)row * g.in_stride + R.off[blockIdx.y];
    double* y = out + (long)row * g.out_stride;
    const int t0 = blockIdx.x * TILE, t_end = min(t0 + TILE, g.out_stride);
    if (t0 >= Lo) {
        for (int t = t0 + threadIdx.x; t < t_end; t += RS_THREADS) y[t] = 0.0;
        return;
    }
    if (R.sr[blockIdx.y] == g.sr_new) {                 // already at the target rate: copied (synthesize.py resamples only if fs != 22050)
        for (int t = t0 + threadIdx.x; t < t_end; t += RS_THREADS) y[t] = t < Lo ? (double)x[t] : 0.0;
        return;
    }
    const RowRate q = row_rate(R.sr[blockIdx.y], g.sr_new, g.num_table);
    const int reach = g.nwin / q.step;                  // taps per wing are at most this
    const int t1 = min(t0 + TILE, Lo) - 1;
    const int n_first = (int)((double)t0 * q.inv), n_last = (int)((double)t1 * q.inv);
    const int lo = max(0, n_first - reach + 1), hi = min(L - 1, n_last + reach);
    if (LDS)
        for (int i = lo + (int)threadIdx.x; i <= hi; i += RS_THREADS) xs_lds[i - lo] = (double)x[i];
    for (int j = threadIdx.x; j < TILE; j += RS_THREADS) {
        const int t = t0 + j;
        int k = INT_MAX;
        if (t < Lo) {
            const double time = (double)t * q.inv;
            k = ((int)(q.scale * (time - (int)time) * g.num_table) << 10) | j;
        } else if (t < g.out_stride) {
            y[t] = 0.0;
        }
        key[j] = k;
    }
    __syncthreads();
    for (int kk = 2; kk <= TILE; kk <<= 1)
        for (int jj = kk >> 1; jj > 0; jj >>= 1) {
            for (int i = threadIdx.x; i < TILE; i += RS_THREADS) {
                const int ij = i ^ jj;
                if (ij > i) {
                    const int a = key[i], b = key[ij];
                    if ((a > b) == ((i & kk) == 0)) { key[i] = b; key[ij] = a; }
                }
            }
            __syncthreads();
        }
    for (int j = threadIdx.x; j < TILE; j += RS_THREADS) {
        const int kj = key[j];
        if (kj == INT_MAX) break;                       // the rest of this thread's keys are past the row's end too
        const int to = t0 + (kj & (TILE - 1));
        const double time = (double)to * q.inv;
        const int n = (int)time;
        const double frac = q.scale * (time - n);
        double acc;
        if (LDS) {
            acc = rs_wing(tab, q, g, frac, n + 1, xs_lds, n - lo, -1, 0.0);
            acc = rs_wing(tab, q, g, q.scale - frac, L - n - 1, xs_lds, n + 1 - lo, 1, acc);
        } else {
            acc = rs_wing(tab, q, g, frac, n + 1, x, n, -1, 0.0);
            acc = rs_wing(tab, q, g, q.scale - frac, L - n - 1, x, n + 1, 1, acc);
        }
        y[to] = acc;
    }
}

// ---------------------------------------------------------------------------------------------------------------- peak
__global__ __launch_bounds__(256) void wav_peak_tiles_kernel(const double* __restrict__ x, const Rows R, int n_samples, int NT, double* part) {
    __shared__ double red[256];
    const int r = R.r0 + blockIdx.y, L = R.L[blockIdx.y];
    const double* xr = x + (long)r * n_samples;
    const int i0 = blockIdx.x * PEAK_TILE, i1 = min(L, i0 + PEAK_TILE);
    double m = 0.0;
    for (int i = i0 + threadIdx.x; i < i1; i += 256) m = fmax(m, fabs(xr[i]));
    red[threadIdx.x] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(long)r * NT + blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void wav_peak_apply_kernel(const double* __restrict__ x, const Rows R, int n_samples, int NT,
                                                             const double* __restrict__ part, float* out) {
    __shared__ double red[256];
    const int r = R.r0 + blockIdx.y, L = R.L[blockIdx.y];
    const double* p = part + (long)r * NT;
    const int nt = (L + PEAK_TILE - 1) / PEAK_TILE;
    double m = 0.0;
    for (int k = threadIdx.x; k < nt; k += 256) m = fmax(m, p[k]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    const double pk = red[0];
    const double* xr = x + (long)r * n_samples;
    float* o = out + (long)r * n_samples;
    const int i0 = blockIdx.x * PEAK_TILE, i1 = min(n_samples, i0 + PEAK_TILE);
    for (int i = i0 + threadIdx.x; i < i1; i += 256) o[i] = (i < L && pk > 0.0) ? (float)(xr[i] / pk) : 0.0f;
}

// ---------------------------------------------------------------------------------------------------------------- host side
bool trim_geo(const DexWavTrimOpts* p, TrimGeo& g) {
    std::memset(&g, 0, sizeof g);
    g.top_db = p ? p->top_db : 30.0;
    g.frame = p ? p->frame_length : 2048;
    g.hop = p ? p->hop_length : 512;
    const int mode = p ? p->pad_mode : DEX_WAV_PAD_CONSTANT;
    if (!std::isfinite(g.top_db) || g.hop < 1 || g.frame < g.hop || g.frame % g.hop != 0 || g.frame > (1 << 24)) return false;
    if (mode != DEX_WAV_PAD_CONSTANT && mode != DEX_WAV_PAD_REFLECT) return false;
    g.reflect = mode == DEX_WAV_PAD_REFLECT;
    g.K = g.frame / g.hop;
    g.pad = g.frame / 2;
    return true;
}

bool lengths_ok(const int* lengths, int B, int n_samples) {
    if (!lengths || B < 1 || n_samples < 1) return false;
    for (int b = 0; b < B; ++b)
        if (lengths[b] < 1 || lengths[b] > n_samples) return false;
    return true;
}

int max_of(const int* v, int B) {
    int m = 0;
    for (int b = 0; b < B; ++b) m = v[b] > m ? v[b] : m;
    return m;
}

bool rs_opts(const DexWavResampleOpts* p, RsOpts& o) {
    if (!p) { o = RsOpts{64, 9, 14.769656459379492, 0.9475937167399596}; return true; }
    o = RsOpts{p->num_zeros, p->precision, p->beta, p->rolloff};
    if (o.precision < 1 || o.precision > 16 || o.num_zeros < 1) return false;
    if ((long)o.num_zeros << o.precision > TABLE_MAX) return false;
    return std::isfinite(o.beta) && o.beta >= 0.0 && o.beta <= 100.0 && o.rolloff > 0.0 && o.rolloff <= 1.0;
}

long resampled_length(long L, long sr_orig, long sr_new) { return L * sr_new / sr_orig; }

}  // namespace

extern "C" {

size_t dex_wav_trim_workspace_bytes(int B, const int* lengths_host, const DexWavTrimOpts* opts) {
    TrimGeo g;
    if (B < 1 || !lengths_host || !trim_geo(opts, g)) return 0;
    for (int b = 0; b < B; ++b)
        if (lengths_host[b] < 1) return 0;
    return (size_t)B * (max_of(lengths_host, B) / g.hop + g.K) * sizeof(double);
}

int dex_wav_trim(const float* wav_dev, const int* lengths_host, int B, int n_samples, const DexWavTrimOpts* opts, int32_t* bounds_dev,
                 double* frame_mse_dev, void* ws, size_t ws_bytes, dex_stream_t s) {
    TrimGeo g;
    if (!wav_dev || !bounds_dev || !ws || !trim_geo(opts, g) || !lengths_ok(lengths_host, B, n_samples)) return DEX_ERR_ARG;
    if (ws_bytes < dex_wav_trim_workspace_bytes(B, lengths_host, opts)) return DEX_ERR_WORKSPACE;
    g.n_samples = n_samples;
    g.Fm = 1 + n_samples / g.hop;
    g.RS = max_of(lengths_host, B) / g.hop + g.K;
    hipStream_t st = (hipStream_t)s;
    double* blocks = (double*)ws;
    return for_row_chunks(B, [&](Rows& R) {
        for (int k = 0; k < R.n; ++k) R.L[k] = lengths_host[R.r0 + k];
        wav_trim_blocks_kernel<<<dim3((unsigned)((g.RS + 3) / 4), R.n), 256, 0, st>>>(wav_dev, g, R, blocks);
        wav_trim_bounds_kernel<<<R.n, 256, 0, st>>>(g, R, blocks, bounds_dev, frame_mse_dev);
    });
}

int dex_wav_resampled_length(int n_samples, int sr_orig, int sr_new) {
    if (n_samples < 1 || sr_orig <= 0 || sr_new <= 0) return DEX_ERR_ARG;
    const long n = resampled_length(n_samples, sr_orig, sr_new);
    return n < 1 || n > INT_MAX ? DEX_ERR_ARG : (int)n;
}

size_t dex_wav_resample_table_bytes(const DexWavResampleOpts* opts) {
    RsOpts o;
    if (!rs_opts(opts, o)) return 0;
    return (size_t)(((long)o.num_zeros << o.precision) + 1) * 2 * sizeof(double);
}

int dex_wav_resample_table(const DexWavResampleOpts* opts, void* table_dev, size_t table_bytes, dex_stream_t s) {
    RsOpts o;
    if (!table_dev || ((uintptr_t)table_dev & 15) != 0 || !rs_opts(opts, o)) return DEX_ERR_ARG;
    if (table_bytes < dex_wav_resample_table_bytes(opts)) return DEX_ERR_WORKSPACE;
    const int N = o.num_zeros << o.precision;
    wav_window_kernel<<<(N + 1 + 255) / 256, 256, 0, (hipStream_t)s>>>(o, N, (double2*)table_dev);
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

int dex_wav_resample(const float* wav_dev, int in_stride, const int* offsets_host, const int* lengths_host, const int* sr_orig_host, int B,
                     int sr_new, const DexWavResampleOpts* opts, double* out_dev, int out_stride, const void* table_dev, size_t table_bytes,
                     dex_stream_t s) {
    RsOpts o;
    if (!wav_dev || !out_dev || !table_dev || ((uintptr_t)table_dev & 15) != 0 || !offsets_host || !lengths_host || !sr_orig_host || B < 1 ||
        in_stride < 1 || out_stride < 1 || sr_new <= 0 || !rs_opts(opts, o))
        return DEX_ERR_ARG;
    RsGeo g;
    g.num_table = 1 << o.precision;
    g.nwin = (o.num_zeros << o.precision) + 1;
    g.sr_new = sr_new; g.in_stride = in_stride; g.out_stride = out_stride;
    int span = 0;
    for (int b = 0; b < B; ++b) {
        const int off = offsets_host[b], L = lengths_host[b], sr = sr_orig_host[b];
        if (L < 1 || off < 0 || off > in_stride - L || sr <= 0) return DEX_ERR_ARG;
        const int Lo = sr == sr_new ? L : dex_wav_resampled_length(L, sr, sr_new);
        if (Lo < 1 || Lo > out_stride) return DEX_ERR_ARG;
        if (sr == sr_new) continue;
        const RowRate q = row_rate(sr, sr_new, g.num_table);
        if (q.step < 1) return DEX_ERR_ARG;
        if ((int)((double)(Lo - 1) * q.inv) > L - 1) return DEX_ERR_ARG;    // the last output's n lies inside the row
        const int reach = g.nwin / q.step;
        const long sp = (long)((double)(TILE - 1) * q.inv) + 4 + 2L * reach;
        span = (int)std::min<long>(std::max<long>(span, sp), INT_MAX / 2);
    }
    if (table_bytes < dex_wav_resample_table_bytes(opts)) return DEX_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)s;
    const double2* tab = (const double2*)table_dev;
    const bool lds = span <= LDS_SPAN;                  // static sort keys (1 KB) + at most 63 KB of staged input: within 64 KB
    const size_t lds_bytes = lds ? (size_t)span * sizeof(double) : 0;
    const unsigned tiles = (unsigned)((out_stride + TILE - 1) / TILE);
    return for_row_chunks(B, [&](Rows& R) {
        for (int k = 0; k < R.n; ++k) {
            const int b = R.r0 + k;
            R.L[k] = lengths_host[b]; R.off[k] = offsets_host[b]; R.sr[k] = sr_orig_host[b];
            R.Lo[k] = R.sr[k] == sr_new ? R.L[k] : dex_wav_resampled_length(R.L[k], R.sr[k], sr_new);
        }
        if (lds) wav_resample_kernel<true><<<dim3(tiles, R.n), RS_THREADS, lds_bytes, st>>>(wav_dev, g, R, tab, out_dev);
        else wav_resample_kernel<false><<<dim3(tiles, R.n), RS_THREADS, 0, st>>>(wav_dev, g, R, tab, out_dev);
    });
}

size_t dex_wav_peak_workspace_bytes(int B, int n_samples) {
    if (B < 1 || n_samples < 1) return 0;
    return (size_t)B * ((n_samples + PEAK_TILE - 1) / PEAK_TILE) * sizeof(double);
}

int dex_wav_peak_normalize_f64(const double* x_dev, const int* lengths_host, int B, int n_samples, float* out_dev, void* ws,
                               size_t ws_bytes, dex_stream_t s) {
    if (!x_dev || !out_dev || !ws || !lengths_ok(lengths_host, B, n_samples)) return DEX_ERR_ARG;
    if (ws_bytes < dex_wav_peak_workspace_bytes(B, n_samples)) return DEX_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)s;
    const int NT = (n_samples + PEAK_TILE - 1) / PEAK_TILE;
    double* part = (double*)ws;
    return for_row_chunks(B, [&](Rows& R) {
        for (int k = 0; k < R.n; ++k) R.L[k] = lengths_host[R.r0 + k];
        wav_peak_tiles_kernel<<<dim3((unsigned)NT, R.n), 256, 0, st>>>(x_dev, R, n_samples, NT, part);
        wav_peak_apply_kernel<<<dim3((unsigned)NT, R.n), 256, 0, st>>>(x_dev, R, n_samples, NT, part, out_dev);
    });
}

}  // extern "C"
