// loss.hip — the two pieces of the reference's validation compute_loss (DEX-TTS/model/tts.py:86-153, GeDEX :57-121) that sit
// between the alignment search (mas.hip) and the decoder's EDM loss:
//
// VQ commitment loss (ref_encoder.py:226, VQEmbeddingEMA.forward in eval mode), run by dex_style_encode_loss right after the
//             codebook lookup:  commit_w * sum (x m - e[idx] m)^2 / (sum m * D).  One wave per [B*Ts] row forms the row's partial
//             in fp64 (each lane adds its columns lane, lane + 64, ... in order; then a fixed xor-shuffle tree) into a workspace
//             slot; one workgroup then adds the partials and the mask in a fixed order and divides, multiplies and rounds once.
//             No atomics: the value is the same bits on every run.
// Segment expand + cut (dex_loss_segment; tts.py:115-144): y_cut[b, :, t] = y[b, :, off_b + t] and mu_y_cut[b, :, t] = mu_x[b, :, k]
//             with k the token whose cumulative-duration span holds frame off_b + t, for t < cut_b = min(S, y_len_b); 0 past cut_b.
//             The [B, Tx, Ty] 0/1 path the reference multiplies by is never formed: a row's inclusive duration prefix sums go to
//             LDS (Tx <= DEX_MAS_MAX_TX), each lane owns one frame and binary-searches it, stores are contiguous along t.  The
//             reference's product has exactly one 1 per covered frame, so a copy of that column is its exact value.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/dex_amd.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace dex {

__global__ __launch_bounds__(256) void vq_loss_rows_kernel(const float* __restrict__ X, const float* __restrict__ Q,
                                                           const float* __restrict__ mask, long rows, int D, double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float m = mask[row];
    double s = 0.0;
    for (int c = lane; c < D; c += 64) {
        const float d = X[row * D + c] * m - Q[row * D + c];   // Q = e[idx] * m already (vq_lookup_kernel)
        s += (double)(d * d);
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) part[row] = s;
}

__global__ __launch_bounds__(256) void vq_loss_combine_kernel(const double* __restrict__ part, const float* __restrict__ mask, long rows,
                                                              int D, float commit_w, float* __restrict__ out) {
    __shared__ double rs[256], rm[256];
    const int t = threadIdx.x;
    double s = 0.0, m = 0.0;
    for (long r = t; r < rows; r += 256) { s += part[r]; m += (double)mask[r]; }
    rs[t] = s; rm[t] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) { rs[t] += rs[t + o]; rm[t] += rm[t + o]; }
        __syncthreads();
    }
    if (t == 0) out[0] = (float)((double)commit_w * (rs[0] / (rm[0] * (double)D)));
}

void launch_vq_loss(const float* X, const float* Q, const float* mask, long rows, int D, double* part, float commit_w, float* out,
                    hipStream_t st) {
    hipLaunchKernelGGL(vq_loss_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, X, Q, mask, rows, D, part);
    hipLaunchKernelGGL(vq_loss_combine_kernel, dim3(1), dim3(256), 0, st, part, mask, rows, D, commit_w, out);
}

}  // namespace dex

namespace {

constexpr int SEG_ROWS = 64;     // utterances per launch (their cut lengths and offsets travel as kernel arguments)
constexpr int SEG_T = 256;       // frames per workgroup

struct SegRows {
    int r0, n;
    int cut[SEG_ROWS], off[SEG_ROWS];
};

__global__ __launch_bounds__(SEG_T) void loss_segment_kernel(const float* __restrict__ mu, const int32_t* __restrict__ dur,
                                                             const float* __restrict__ yv, int F, int Tx, int Ty, int S, const SegRows R,
                                                             float* __restrict__ ycut, float* __restrict__ mucut, float* __restrict__ mcut) {
    __shared__ int cum[DEX_MAS_MAX_TX];
    __shared__ int part[SEG_T];
    const int i = blockIdx.y, b = R.r0 + i, tid = threadIdx.x;
    // inclusive prefix sums of the row's durations: a sequential run per lane, then a scan of the 256 run totals
    const int per = (Tx + SEG_T - 1) / SEG_T, base = tid * per;
    const int32_t* Dr = dur + (long)b * Tx;
    int s = 0;
    for (int k = 0; k < per; ++k) {
        const int x = base + k;
        if (x < Tx) { s += Dr[x]; cum[x] = s; }
    }
    part[tid] = s;
    __syncthreads();
    for (int o = 1; o < SEG_T; o <<= 1) {
        const int v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    const int excl = tid ? part[tid - 1] : 0;
    for (int k = 0; k < per; ++k) {
        const int x = base + k;
        if (x < Tx) cum[x] += excl;
    }
    __syncthreads();
    const int t = blockIdx.x * SEG_T + tid;
    if (t >= S) return;
    const int cut = R.cut[i], off = R.off[i];
    const bool in = t < cut;
    int tok = Tx;
    if (in) {                                  // the first token whose inclusive end exceeds the frame (zero-length tokens skip)
        const int f = off + t;
        int lo = 0, hi = Tx;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cum[mid] > f) hi = mid; else lo = mid + 1;
        }
        tok = lo;
    }
    const bool has = in && tok < Tx;
    for (int fe = 0; fe < F; ++fe) {
        const long ro = (long)b * F + fe;
        ycut[ro * S + t] = in ? yv[ro * Ty + off + t] : 0.f;
        mucut[ro * S + t] = has ? mu[ro * Tx + tok] : 0.f;
    }
    mcut[(long)b * S + t] = in ? 1.f : 0.f;
}

}  // namespace

extern "C" {

int dex_loss_segment(const float* mu_x_dev, const int32_t* dur_dev, const float* y_dev, int B, int n_feats, int Tx, int Ty,
                     const int* y_lengths_host, const int* offsets_host, int S, float* y_cut_dev, float* mu_y_cut_dev,
                     float* y_cut_mask_dev, dex_stream_t s) {
    if (!mu_x_dev || !dur_dev || !y_dev || !y_cut_dev || !mu_y_cut_dev || !y_cut_mask_dev || !y_lengths_host) return DEX_ERR_ARG;
    if (B < 1 || n_feats < 1 || Tx < 1 || Tx > DEX_MAS_MAX_TX || Ty < 1 || Ty > DEX_MAS_MAX_TY || S < 1 || S > Ty) return DEX_ERR_ARG;
    for (int b = 0; b < B; ++b) {
        const int yl = y_lengths_host[b], off = offsets_host ? offsets_host[b] : 0;
        const int cut = yl < S ? yl : S;
        if (yl < 1 || yl > Ty || off < 0 || off > yl - cut) return DEX_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)s;
    for (int r0 = 0; r0 < B; r0 += SEG_ROWS) {
        SegRows R;
        std::memset(&R, 0, sizeof R);
        R.r0 = r0; R.n = B - r0 < SEG_ROWS ? B - r0 : SEG_ROWS;
        for (int i = 0; i < R.n; ++i) {
            const int yl = y_lengths_host[r0 + i];
            R.cut[i] = yl < S ? yl : S;
            R.off[i] = offsets_host ? offsets_host[r0 + i] : 0;
        }
        dim3 grid((unsigned)((S + SEG_T - 1) / SEG_T), (unsigned)R.n);
        loss_segment_kernel<<<grid, SEG_T, 0, st>>>(mu_x_dev, dur_dev, y_dev, n_feats, Tx, Ty, S, R, y_cut_dev, mu_y_cut_dev, y_cut_mask_dev);
        if (hipGetLastError() != hipSuccess) return DEX_ERR_HIP;
    }
    return DEX_OK;
}

}  // extern "C"
