// mas.hip — Glow-TTS monotonic alignment search on the device: the log-prior of DEX-TTS/GeDEX-TTS compute_loss (tts.py:100-106)
// and model.monotonic_align.maximum_path with the reference's fp32 semantics, for a ragged batch.  The contract is the docstring of
// tests/mas_restatement.py.
//
// log-prior:  per (row, 64 x 64 tile) mu and y staged in LDS; the three contractions over n_feats in fp64, one rounding to fp32.
// MAS:        one wave per utterance.  Lane l holds rows [l R, l R + R) of the running column in registers (R = 64-row chunks
//             rounded up to a power of two); a column costs one __shfl_up (the value of the row above the lane's first row) and R
//             independent max + add.  The decision the backtrack needs at (x, y) is one bit, V[x, y] < V[x - 1, y]; it is formed
//             while the next column is computed and packed by row, 32 frames per word, into LDS — or into the workspace when the
//             matrix is larger than one workgroup may allocate.  Lane 0 then walks the bits from (t_x - 1, t_y - 1) and writes the
//             per-token durations.  No reassociation, no contraction: every cell is the reference's max(a, b) + v in fp32.
// Reductions: per row fixed-order partial sums of the duration and prior losses, then one combine on the device.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>

#include "../../include/dex_amd.h"

#pragma clang fp contract(off)

namespace {

constexpr int ROWS = 64;                   // utterances per launch (their lengths travel as kernel arguments)
constexpr float NEG = -1e9f;               // the reference's max_neg_val
constexpr int LDS_BITS_BYTES = 160 * 1024; // what one workgroup may allocate on gfx950
constexpr int LP_T = 64;                   // log-prior tile (x and y)
constexpr int LP_MAX_F = 128;

struct Rows {
    int r0, n;
    int tx[ROWS], ty[ROWS];
};

// ---------------------------------------------------------------------------------------------------------------- log-prior
// out[b, y, x] = -0.5 sum_f y^2 + sum_f mu y - 0.5 sum_f mu^2 - 0.5 log(2 pi) F  (x < Tx, y < Ty; every cell, masked or not)
__global__ __launch_bounds__(256) void mas_log_prior_kernel(const float* __restrict__ mu, const float* __restrict__ yv, int F, int Tx, int Ty,
                                                            double cst, float* __restrict__ out) {
    __shared__ float smu[LP_MAX_F][LP_T];
    __shared__ float sy[LP_MAX_F][LP_T];
    __shared__ double sysq[LP_T];
    const int b = blockIdx.z, x0 = blockIdx.x * LP_T, y0 = blockIdx.y * LP_T, t = threadIdx.x;
    const float* M = mu + (long)b * F * Tx;
    const float* Y = yv + (long)b * F * Ty;
    for (int i = t; i < F * LP_T; i += 256) {
        const int f = i / LP_T, j = i % LP_T;
        smu[f][j] = x0 + j < Tx ? M[(long)f * Tx + x0 + j] : 0.f;
        sy[f][j] = y0 + j < Ty ? Y[(long)f * Ty + y0 + j] : 0.f;
    }
    __syncthreads();
    if (t < LP_T) {
        double s = 0.0;
        for (int f = 0; f < F; ++f) s += (double)sy[f][t] * (double)sy[f][t];
        sysq[t] = -0.5 * s;
    }
    const int xl = t & 63, yg = t >> 6;    // 4 groups of 16 y per x
    double msq = 0.0, acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.0;
    for (int f = 0; f < F; ++f) {
        const double m = (double)smu[f][xl];
        msq += m * m;
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] += m * (double)sy[f][yg * 16 + k];
    }
    __syncthreads();
    const int x = x0 + xl;
    if (x >= Tx) return;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int y = y0 + yg * 16 + k;
        if (y < Ty) out[((long)b * Ty + y) * Tx + x] = (float)(sysq[yg * 16 + k] + acc[k] - 0.5 * msq + cst);
    }
}

// ---------------------------------------------------------------------------------------------------------------- MAS
struct MasGeo {
    long sb, sx, sy;                       // element strides of value (and of mask) per utterance, row x, frame y
    int Tx;                                // dur row stride
    int W;                                 // bit-matrix words per row (ceil(max t_y / 32)), LDS or workspace
    long bits_stride;                      // workspace words per utterance (global-memory bits)
};

// the reference's Cython max(a, b) on two C floats: b if b > a else a (it differs from fmaxf only in the sign of a zero, which no
// comparison of the backtrack can see)
__device__ inline float ref_max(float a, float b) { return b > a ? b : a; }

template <int R> struct Prefetch { static constexpr int P = R <= 4 ? 16 : (R == 8 ? 8 : 4); };

template <int R, bool LDS>
__global__ __launch_bounds__(64) void mas_kernel(const float* __restrict__ value, const float* __restrict__ mask, const MasGeo g, const Rows Rw,
                                                 int32_t* __restrict__ dur, uint32_t* __restrict__ gbits) {
    extern __shared__ uint32_t sbits[];
    constexpr int P = Prefetch<R>::P;
    const int lane = threadIdx.x;
    const int b = Rw.r0 + blockIdx.x, tx = Rw.tx[blockIdx.x], ty = Rw.ty[blockIdx.x];
    uint32_t* bits = LDS ? sbits : gbits + (long)b * g.bits_stride;
    const float* V = value + (long)b * g.sb;
    const float* Mk = mask ? mask + (long)b * g.sb : nullptr;
    const int x0 = lane * R;

    auto load = [&](int y, float (&c)[R]) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int x = x0 + r;
            float v = 0.f;
            if (x < tx && y < ty) {
                const long o = (long)x * g.sx + (long)y * g.sy;
                v = V[o];
                if (Mk) v = v * Mk[o];
            }
            c[r] = v;
        }
    };

    float v[R], pf[P][R];
    uint32_t word[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { v[r] = 0.f; word[r] = 0u; }
#pragma unroll
    for (int j = 0; j < P; ++j) load(j, pf[j]);

    for (int y0 = 0; y0 < ty; y0 += P) {
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int y = y0 + j;
            if (y < ty) {
                float c[R], old[R];
#pragma unroll
                for (int r = 0; r < R; ++r) { c[r] = pf[j][r]; old[r] = v[r]; }
                load(y + P, pf[j]);
                const float up = __shfl_up(old[R - 1], 1);           // column y - 1 of the row above this lane's first
                const int lo = tx + y - ty > 0 ? tx + y - ty : 0, hi = tx < y + 1 ? tx : y + 1;
                const int bit = (y - 1) & 31;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int x = x0 + r;
                    const float above = r ? old[r - 1] : up;
                    if (x >= lo && x < hi) {
                        const float vcur = x == y ? NEG : old[r];
                        const float vprev = x == 0 ? (y == 0 ? 0.f : NEG) : above;
                        v[r] = ref_max(vcur, vprev) + c[r];
                    }
                    word[r] |= (uint32_t)(old[r] < above) << bit;   // decision of column y - 1 (y = 0: shifted out below)
                }
                if (y >= 1 && bit == 31) {
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if (x0 + r < tx) bits[(long)(x0 + r) * g.W + ((y - 1) >> 5)] = word[r];
                        word[r] = 0u;
                    }
                } else if (y == 0) {
#pragma unroll
                    for (int r = 0; r < R; ++r) word[r] = 0u;
                }
            }
        }
    }
    if (ty >= 2 && ((ty - 2) & 31) != 31) {                           // the last, partial word (columns up to t_y - 2 are read)
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (x0 + r < tx) bits[(long)(x0 + r) * g.W + ((ty - 2) >> 5)] = word[r];
    }
    int32_t* D = dur + (long)b * g.Tx;
    for (int x = tx + lane; x < g.Tx; x += 64) D[x] = 0;              // past t_x, which the lanes' rows need not cover
    __syncthreads();
    if (lane != 0) return;
    int index = tx - 1, cnt = 0, crow = -1, cw = -1;
    uint32_t w = 0u;
    for (int y = ty - 1; y >= 0; --y) {
        ++cnt;
        bool step = false;
        if (index != 0) {
            if (index == y) {
                step = true;
            } else {                                                   // index < y here, so y - 1 >= index >= 1
                const int k = (y - 1) >> 5;
                if (index != crow || k != cw) { w = bits[(long)index * g.W + k]; crow = index; cw = k; }
                step = (w >> ((y - 1) & 31)) & 1u;
            }
        }
        if (step) { D[index] = cnt; cnt = 0; --index; }
    }
    D[index] = cnt;
}

// path[b, x, y] = 1 on [start_x, start_x + dur_x), start_x = sum of the durations before x; 0 elsewhere
__global__ __launch_bounds__(256) void mas_path_kernel(const int32_t* __restrict__ dur, int Tx, int Ty, float* __restrict__ path) {
    __shared__ int part[4];
    const int x = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int32_t* D = dur + (long)b * Tx;
    int s = 0;
    for (int i = t; i < x; i += 256) s += D[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((t & 63) == 0) part[t >> 6] = s;
    __syncthreads();
    const int start = part[0] + part[1] + part[2] + part[3], end = start + D[x];
    float* out = path + ((long)b * Tx + x) * Ty;
    for (int y = t; y < Ty; y += 256) out[y] = (y >= start && y < end) ? 1.f : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------- losses
// per utterance b (fixed order, fp64 accumulation of the reference's fp32 terms):
//   part[b, 0] = sum_x (logw - log(1e-8 + dur) * x_mask)^2       (utils.py:42-44 numerator)
//   part[b, 1] = sum_{f, y} 0.5 ((y - mu_y)^2 + log 2 pi) * y_mask  (tts.py:148)
__global__ __launch_bounds__(256) void mas_loss_rows_kernel(const float* __restrict__ logw, const int32_t* __restrict__ dur, int Tx,
                                                            const float* __restrict__ yv, const float* __restrict__ mu_y, int F, int Ty,
                                                            const Rows Rw, double* __restrict__ part) {
    __shared__ double red[2][256];
    const int i = blockIdx.x, b = Rw.r0 + i, t = threadIdx.x;
    const int tx = Rw.tx[i], ty = Rw.ty[i];
    const float l2pi = 1.8378770664093453f;   // (float)log(2 pi)
    double sd = 0.0, sp = 0.0;
    for (int x = t; x < Tx; x += 256) {
        const float m = x < tx ? 1.f : 0.f;
        const float lw = logf(1e-8f + (float)dur[(long)b * Tx + x]) * m;
        const float d = logw[(long)b * Tx + x] - lw;
        sd += (double)(d * d);
    }
    const long n = (long)F * Ty;
    for (long k = t; k < n; k += 256) {
        const int yy = (int)(k % Ty);
        const float m = yy < ty ? 1.f : 0.f;
        const float d = yv[(long)b * n + k] - mu_y[(long)b * n + k];
        sp += (double)(0.5f * (d * d + l2pi) * m);
    }
    red[0][t] = sd; red[1][t] = sp;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) { red[0][t] += red[0][t + o]; red[1][t] += red[1][t + o]; }
        __syncthreads();
    }
    if (t == 0) { part[2 * b] = red[0][0]; part[2 * b + 1] = red[1][0]; }
}

// out[0] = dur_loss, out[1] = prior_loss: the per-utterance sums in utterance order over the host-known denominators
__global__ void mas_loss_combine_kernel(const double* __restrict__ part, int B, double dur_den, double prior_den, float* __restrict__ out) {
    if (threadIdx.x != 0) return;
    double d = 0.0, p = 0.0;
    for (int b = 0; b < B; ++b) { d += part[2 * b]; p += part[2 * b + 1]; }
    out[0] = (float)(d / dur_den);
    out[1] = (float)(p / prior_den);
}

bool lengths_ok(const int* xl, const int* yl, int B, int Tx, int Ty) {
    if (!xl || !yl) return false;
    for (int b = 0; b < B; ++b)
        if (xl[b] < 1 || xl[b] > Tx || yl[b] < xl[b] || yl[b] > Ty) return false;
    return true;
}

bool dims_ok(int B, int Tx, int Ty) { return B >= 1 && Tx >= 1 && Ty >= 1 && Tx <= DEX_MAS_MAX_TX && Ty <= DEX_MAS_MAX_TY; }

int words(int Ty) { return (Ty + 31) / 32; }

bool bits_fit_lds(int Tx, int Ty) { return (long)Tx * words(Ty) * 4 <= LDS_BITS_BYTES; }

template <class Fn>
int for_row_chunks(int B, const int* xl, const int* yl, Fn launch) {
    for (int r0 = 0; r0 < B; r0 += ROWS) {
        Rows R;
        std::memset(&R, 0, sizeof R);
        R.r0 = r0; R.n = B - r0 < ROWS ? B - r0 : ROWS;
        for (int i = 0; i < R.n; ++i) { R.tx[i] = xl[r0 + i]; R.ty[i] = yl[r0 + i]; }
        launch(R);
        if (hipGetLastError() != hipSuccess) return DEX_ERR_HIP;
    }
    return DEX_OK;
}

template <int R, bool LDS>
void launch_mas(const float* value, const float* mask, const MasGeo& g, const Rows& Rw, int32_t* dur, uint32_t* gbits, hipStream_t st) {
    const size_t lds = LDS ? (size_t)g.W * 4 * (size_t)(R * 64 < g.Tx ? R * 64 : g.Tx) : 0;
    if (LDS) {
        static bool attr = false;
        if (!attr) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&mas_kernel<R, LDS>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BITS_BYTES);
            attr = true;
        }
    }
    mas_kernel<R, LDS><<<Rw.n, 64, lds, st>>>(value, mask, g, Rw, dur, gbits);
}

template <bool LDS>
void dispatch_mas(int Rn, const float* value, const float* mask, const MasGeo& g, const Rows& Rw, int32_t* dur, uint32_t* gbits, hipStream_t st) {
    switch (Rn) {
        case 1: launch_mas<1, LDS>(value, mask, g, Rw, dur, gbits, st); break;
        case 2: launch_mas<2, LDS>(value, mask, g, Rw, dur, gbits, st); break;
        case 4: launch_mas<4, LDS>(value, mask, g, Rw, dur, gbits, st); break;
        case 8: launch_mas<8, LDS>(value, mask, g, Rw, dur, gbits, st); break;
        case 16: launch_mas<16, LDS>(value, mask, g, Rw, dur, gbits, st); break;
        default: launch_mas<32, LDS>(value, mask, g, Rw, dur, gbits, st); break;
    }
}

}  // namespace

extern "C" {

int dex_mas_log_prior(const float* mu_x_dev, const float* y_dev, int B, int n_feats, int Tx, int Ty, float* log_prior_dev, dex_stream_t s) {
    if (!mu_x_dev || !y_dev || !log_prior_dev || !dims_ok(B, Tx, Ty) || n_feats < 1 || n_feats > LP_MAX_F) return DEX_ERR_ARG;
    const double cst = -0.5 * 1.8378770664093453 * (double)n_feats;   // -0.5 log(2 pi) n_feats
    dim3 grid((unsigned)((Tx + LP_T - 1) / LP_T), (unsigned)((Ty + LP_T - 1) / LP_T), (unsigned)B);
    mas_log_prior_kernel<<<grid, 256, 0, (hipStream_t)s>>>(mu_x_dev, y_dev, n_feats, Tx, Ty, cst, log_prior_dev);
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

size_t dex_mas_workspace_bytes(int B, int Tx, int Ty) {
    if (!dims_ok(B, Tx, Ty)) return 0;
    if (bits_fit_lds(Tx, Ty)) return 256;    // the bit matrices stay in LDS; a token workspace keeps the calling convention uniform
    return (size_t)B * Tx * words(Ty) * 4;
}

int dex_mas_durations(const float* value_dev, const float* mask_dev, int B, int Tx, int Ty, int64_t stride_b, int64_t stride_x,
                      int64_t stride_y, const int* x_lengths_host, const int* y_lengths_host, int32_t* dur_dev, float* path_dev,
                      void* workspace_dev, size_t workspace_bytes, dex_stream_t s) {
    if (!value_dev || !dur_dev || !workspace_dev || !dims_ok(B, Tx, Ty) || !lengths_ok(x_lengths_host, y_lengths_host, B, Tx, Ty))
        return DEX_ERR_ARG;
    if (stride_b < 1 || stride_x < 1 || stride_y < 1) return DEX_ERR_ARG;
    if (workspace_bytes < dex_mas_workspace_bytes(B, Tx, Ty)) return DEX_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)s;
    int mx = 1;
    for (int b = 0; b < B; ++b) mx = x_lengths_host[b] > mx ? x_lengths_host[b] : mx;
    int Rn = 1;
    while (Rn * 64 < mx) Rn *= 2;
    MasGeo g;
    g.sb = stride_b; g.sx = stride_x; g.sy = stride_y; g.Tx = Tx; g.W = words(Ty);
    g.bits_stride = (long)Tx * g.W;
    const bool lds = bits_fit_lds(Tx, Ty);
    int rc = for_row_chunks(B, x_lengths_host, y_lengths_host, [&](const Rows& R) {
        if (lds) dispatch_mas<true>(Rn, value_dev, mask_dev, g, R, dur_dev, nullptr, st);
        else dispatch_mas<false>(Rn, value_dev, mask_dev, g, R, dur_dev, (uint32_t*)workspace_dev, st);
    });
    if (rc != DEX_OK || !path_dev) return rc;
    mas_path_kernel<<<dim3((unsigned)Tx, (unsigned)B), 256, 0, st>>>(dur_dev, Tx, Ty, path_dev);
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

size_t dex_mas_loss_workspace_bytes(int B) { return B >= 1 ? (size_t)B * 2 * sizeof(double) : 0; }

int dex_mas_losses(const float* logw_dev, const int32_t* dur_dev, const int* x_lengths_host, int B, int Tx, const float* y_dev,
                   const float* mu_y_dev, const int* y_lengths_host, int n_feats, int Ty, float* out_dev, void* workspace_dev,
                   size_t workspace_bytes, dex_stream_t s) {
    if (!logw_dev || !dur_dev || !y_dev || !mu_y_dev || !out_dev || !workspace_dev || B < 1 || Tx < 1 || Ty < 1 || n_feats < 1)
        return DEX_ERR_ARG;
    if (!x_lengths_host || !y_lengths_host) return DEX_ERR_ARG;
    double xsum = 0.0, ysum = 0.0;
    for (int b = 0; b < B; ++b) {
        if (x_lengths_host[b] < 1 || x_lengths_host[b] > Tx || y_lengths_host[b] < 1 || y_lengths_host[b] > Ty) return DEX_ERR_ARG;
        xsum += x_lengths_host[b]; ysum += y_lengths_host[b];
    }
    if (workspace_bytes < dex_mas_loss_workspace_bytes(B)) return DEX_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)s;
    double* part = (double*)workspace_dev;
    int rc = for_row_chunks(B, x_lengths_host, y_lengths_host, [&](const Rows& R) {
        mas_loss_rows_kernel<<<R.n, 256, 0, st>>>(logw_dev, dur_dev, Tx, y_dev, mu_y_dev, n_feats, Ty, R, part);
    });
    if (rc != DEX_OK) return rc;
    mas_loss_combine_kernel<<<1, 64, 0, st>>>(part, B, xsum, ysum * n_feats, out_dev);
    return hipGetLastError() == hipSuccess ? DEX_OK : DEX_ERR_HIP;
}

}  // extern "C"
