// wav_gated_attn.h — what the WavLM networks share (wavlm.hip: the base family with the x-vector head; ecapa.hip: the large family
// with the ECAPA-TDNN head): the gated relative-position bias and its attention, and the incremental layer mix.
//
//   wavlm_gate_kernel      gate[b][h][t] = a (b const[h] - 1) + 2 with (a, b) = sigmoid of the two grouped sums of
//                          gru_rel_pos_linear(x[t][64 h .. 64 h + 64]); x is what the attention reads (the layer's input in the
//                          post-norm order, its LayerNorm in the stable-layer-norm order), one thread per (frame, head).
//   wavlm_rel_kernel       rel[h][d + N - 1] = rel_attn_embed[bucket(d)][h], d = -(N - 1) .. N - 1, once per call from the bucket table
//                          the host computed at finalize (bucket_of).
//   wavlm_attn_kernel      softmax((q / 8) k^T + gate[b][h][i] rel[h][j - i]) v on v_mfma_f32_32x32x2_f32 in the transposed flash
//                          formulation of attention.hip's generic kernel; the bias is formed in registers from the two tables - no
//                          [B H][N][N] tensor exists.
//   wavlm_mix_kernel       the softmax(layer weights)-weighted sum of the hidden states, accumulated as the layers finish (one buffer).
//   wavlm_softmax_kernel   those weights' softmax in fp64, once at finalize.
// Includes wav_trunk.h; everything has internal linkage.
#pragma once
#include <cmath>

#include "wav_trunk.h"

namespace dex {
namespace wavenc {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int MAXF = 4096;               // encoder frames one call takes (DEX_WAVLM_MAX_FRAMES, DEX_ECAPA_MAX_FRAMES)

// one thread per (frame, head): gw [8][64], gb [8], gc [heads] -> gate [B][heads][T]
__global__ __launch_bounds__(256) void wavlm_gate_kernel(const float* X, const float* gw, const float* gb, const float* gc, float* gate, int B, int T,
                                                        int heads) {
    __shared__ float w[8 * 64 + 8];
    for (int i = threadIdx.x; i < 8 * 64 + 8; i += 256) w[i] = i < 512 ? gw[i] : gb[i - 512];
    __syncthreads();
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * T * heads) return;
    const int hd = (int)(idx % heads);
    const long row = idx / heads;
    const int b = (int)(row / T), t = (int)(row - (long)b * T);
    const float4* x = reinterpret_cast<const float4*>(X + row * heads * 64 + hd * 64);
    float acc[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) acc[o] = w[512 + o];
#pragma unroll
    for (int k4 = 0; k4 < 16; ++k4) {
        const float4 v = x[k4];
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            const float* wo = w + o * 64 + k4 * 4;
            acc[o] = fmaf(v.w, wo[3], fmaf(v.z, wo[2], fmaf(v.y, wo[1], fmaf(v.x, wo[0], acc[o]))));
        }
    }
    const float ga = 1.f / (1.f + expf(-((acc[0] + acc[1]) + (acc[2] + acc[3]))));
    const float gbv = 1.f / (1.f + expf(-((acc[4] + acc[5]) + (acc[6] + acc[7]))));
    gate[((long)b * heads + hd) * T + t] = ga * (gbv * gc[hd] - 1.f) + 2.f;
}

// rel [heads][2 N - 1]: entry d + N - 1 = embed[bucket(d)][h]; buckets holds d = -(MAXF - 1) .. MAXF - 1
__global__ __launch_bounds__(256) void wavlm_rel_kernel(const float* embed, const int* buckets, float* rel, int N, int heads) {
    const int j = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y;
    if (j >= 2 * N - 1) return;
    rel[(long)h * (2 * N - 1) + j] = embed[(long)buckets[j - (N - 1) + (MAXF - 1)] * heads + h];
}

// ---- attention with the gated relative-position bias.  The transposed flash formulation of attention.hip's generic kernel at
// head_dim 64: S^T = K Q^T (A = the K^T tile in wave-private LDS, B = the pre-scaled Q tile), O^T = V^T P^T with P^T the S^T
// accumulator registers themselves.  C-layout of a 32 x 32 tile: col = lane & 31 (query), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
// (key) - so a lane's 16 scores belong to ONE query: its gate is one register, and rel is read at 16 distances key - query.
constexpr int AT_NW = 4;                   // waves per workgroup: wave w takes key tiles w, w + 4, ...
constexpr int AT_KT_LD = 33;               // K^T tile [64 d][32 keys + 1]
constexpr int AT_V_LD = 64 + 8;            // V tile [32 keys][64 d + 8]; also the merged O tile [32 queries][64 d + 8]
constexpr int AT_WAVE_LDS = 32 * AT_V_LD;  // 2304 floats >= 64 * 33
constexpr int AT_Q_LD = 65;
struct AttnBiasP { const float* qkv; int ld; long bstride; float* O; int ldo; long ob; int N; const int* kv_len; int heads;
                   const float* rel; const float* gate; };

__global__ __launch_bounds__(AT_NW * 64) void wavlm_attn_kernel(const AttnBiasP p) {
    __shared__ __attribute__((aligned(16))) float smem[AT_NW * AT_WAVE_LDS + AT_NW * 64 + 32 * AT_Q_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, hh = lane >> 5;
    const int q0 = blockIdx.x * 32, h = blockIdx.y, b = blockIdx.z;
    float* wt = smem + wave * AT_WAVE_LDS;                  // wave-private tile
    float* stat = smem + AT_NW * AT_WAVE_LDS;               // [NW][2][32]
    float* qS = stat + AT_NW * 64;                          // [32 queries][AT_Q_LD] pre-scaled Q
    const int Nk = max(1, min(p.N, p.kv_len[b]));
    const int H = p.heads * 64;
    const float* Qb = p.qkv + (long)b * p.bstride + h * 64;
    const float* Kb = Qb + H;
    const float* Vb = Qb + 2 * H;
    for (int it = tid; it < 32 * 16; it += AT_NW * 64) {
        const int qi = it >> 4, d4 = (it & 15) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q0 + qi < p.N) v = *reinterpret_cast<const float4*>(Qb + (long)(q0 + qi) * p.ld + d4);
        float* d = qS + qi * AT_Q_LD + d4;
        d[0] = v.x * 0.125f; d[1] = v.y * 0.125f; d[2] = v.z * 0.125f; d[3] = v.w * 0.125f;
    }
    // this lane's query (clamped at the tail of the last tile: its result is not stored), its gate and its row of the distance table
    const int qi = min(q0 + i, p.N - 1);
    const float gq = p.gate[((long)b * p.heads + h) * p.N + qi];
    const float* relq = p.rel + (long)h * (2 * p.N - 1) + (p.N - 1) - qi;      // relq[key], key in [0, N): index in [0, 2 N - 2]
    f32x16 o[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const int ntiles = (Nk + 31) / 32;
    __syncthreads();
    for (int kt = wave; kt < ntiles; kt += AT_NW) {
        const int k0 = kt * 32;
        float rb[16];                                       // the 16 table entries, in flight under the S^T MFMAs
#pragma unroll
        for (int r = 0; r < 16; ++r) rb[r] = relq[min(k0 + (r & 3) + 8 * (r >> 2) + 4 * hh, Nk - 1)];
        f32x16 sT;
#pragma unroll
        for (int r = 0; r < 16; ++r) sT[r] = 0.f;
        // K tile [32 keys][64 d] -> K^T[d][key] (16 lanes per key row)
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int key = it * 4 + (lane >> 4), dd = (lane & 15) * 4;
            const float4 v = *reinterpret_cast<const float4*>(Kb + (long)min(k0 + key, Nk - 1) * p.ld + dd);
            float* d = wt + dd * AT_KT_LD + key;
            d[0] = v.x; d[AT_KT_LD] = v.y; d[2 * AT_KT_LD] = v.z; d[3 * AT_KT_LD] = v.w;
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);                 // lgkmcnt(0): this wave's LDS writes landed (wave-private tile)
        __builtin_amdgcn_wave_barrier();
        {
            const float* ka = wt + (hh * 32) * AT_KT_LD + i;
            const float* qa = qS + i * AT_Q_LD + hh * 32;
#pragma unroll
            for (int kk = 0; kk < 32; ++kk) sT = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[kk * AT_KT_LD], qa[kk], sT, 0, 0, 0);
        }
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
            sT[r] = key >= Nk ? -INFINITY : fmaf(gq, rb[r], sT[r]);
            mx = fmaxf(mx, sT[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        if (__builtin_amdgcn_ballot_w64(mx > m_run + 8.f) != 0) {         // lazy rescale, as in attention.hip
            const float m_new = fmaxf(m_run, mx);
            const float alpha = __expf(m_run - m_new);
            l_run *= alpha;
            m_run = m_new;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[t][r] *= alpha;
        }
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { sT[r] = __expf(sT[r] - m_run); psum += sT[r]; }
        l_run += psum;
        // V tile [32 keys][64 d] over the K^T image
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int key = it * 4 + (lane >> 4), dd = (lane & 15) * 4;
            *reinterpret_cast<float4*>(wt + key * AT_V_LD + dd) = *reinterpret_cast<const float4*>(Vb + (long)min(k0 + key, Nk - 1) * p.ld + dd);
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const float* vp = wt + ((s & 3) + 8 * (s >> 2) + 4 * hh) * AT_V_LD + i;
#pragma unroll
            for (int t = 0; t < 2; ++t) o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[t * 32], sT[s], o[t], 0, 0, 0);
        }
    }
    l_run += __shfl_xor(l_run, 32);
    if (hh == 0) { stat[(wave * 2 + 0) * 32 + i] = m_run; stat[(wave * 2 + 1) * 32 + i] = l_run; }
    __syncthreads();                                        // every wave done with its tile
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq)
            *reinterpret_cast<float4*>(wt + i * AT_V_LD + t * 32 + 8 * rq + 4 * hh) =
                make_float4(o[t][rq * 4 + 0], o[t][rq * 4 + 1], o[t][rq * 4 + 2], o[t][rq * 4 + 3]);
    __syncthreads();
    const int d4 = (tid & 15) * 4;
    for (int q = tid >> 4; q < 32; q += AT_NW * 4) {
        if (q0 + q >= p.N) continue;
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < AT_NW; ++w) M = fmaxf(M, stat[(w * 2) * 32 + q]);
        float L = 0.f;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int w = 0; w < AT_NW; ++w) {
            const float mw = stat[(w * 2) * 32 + q];
            const float f = (mw == -INFINITY) ? 0.f : __expf(mw - M);
            L += f * stat[(w * 2 + 1) * 32 + q];
            const float4 v = *reinterpret_cast<const float4*>(smem + w * AT_WAVE_LDS + q * AT_V_LD + d4);
            acc.x = fmaf(f, v.x, acc.x); acc.y = fmaf(f, v.y, acc.y); acc.z = fmaf(f, v.z, acc.z); acc.w = fmaf(f, v.w, acc.w);
        }
        const float inv = 1.f / L;
        float* op = p.O + (long)b * p.ob + (long)(q0 + q) * p.ldo + h * 64 + d4;
        *reinterpret_cast<float4*>(op) = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
    }
}

// dst = (first ? 0 : acc) + lw[l] h (lw null: weight 1); mask given (the last step): rows whose mask is 0 are stored as 0.  dst may be acc.
__global__ __launch_bounds__(256) void wavlm_mix_kernel(const float4* h, const float4* acc, float4* dst, const float* lw, int l, int first,
                                                       const float* mask, long n4, int H4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const float w = lw ? lw[l] : 1.f;
    const float4 v = h[i];
    float4 a = first ? make_float4(0.f, 0.f, 0.f, 0.f) : acc[i];
    a.x += w * v.x; a.y += w * v.y; a.z += w * v.z; a.w += w * v.w;
    if (mask && mask[i / H4] == 0.f) a = make_float4(0.f, 0.f, 0.f, 0.f);
    dst[i] = a;
}

// lw = softmax(w [n]) in fp64, one thread
__global__ void wavlm_softmax_kernel(const float* w, float* lw, int n) {
    if (threadIdx.x || blockIdx.x) return;
    double m = w[0], s = 0.0;
    for (int i = 1; i < n; ++i) m = fmax(m, (double)w[i]);
    for (int i = 0; i < n; ++i) s += exp((double)w[i] - m);
    for (int i = 0; i < n; ++i) lw[i] = (float)(exp((double)w[i] - m) / s);
}

// _relative_positions_bucket of the distance d = key - query, in fp64
int bucket_of(int num_buckets, int max_bucket_distance, long d) {
    const int nb = num_buckets / 2, max_exact = nb / 2;
    const int side = d > 0 ? nb : 0;
    const long a = d < 0 ? -d : d;
    if (a < max_exact) return side + (int)a;
    const double v = std::log((double)a / max_exact) / std::log((double)max_bucket_distance / max_exact) * (nb - max_exact);
    const long big = max_exact + (long)v;
    return side + (int)(big < nb - 1 ? big : nb - 1);
}

// the gate of one layer and the biased attention over the packed q | k | v: x [B][T][heads 64] is what the attention reads
struct GateW { const float *gw, *gb, *gc; };
void enqueue_gated_attention(const float* x, const GateW& g, const float* qkv, float* out, float* gate, const float* rel, const int* kv_len, int B, int T,
                             int heads, hipStream_t st) {
    const int H = heads * 64;
    const long rows = (long)B * T;
    hipLaunchKernelGGL(wavlm_gate_kernel, dim3((unsigned)((rows * heads + 255) / 256)), dim3(256), 0, st, x, g.gw, g.gb, g.gc, gate, B, T, heads);
    const AttnBiasP a{qkv, 3 * H, (long)T * 3 * H, out, H, (long)T * H, T, kv_len, heads, rel, gate};
    hipLaunchKernelGGL(wavlm_attn_kernel, dim3((T + 31) / 32, heads, B), dim3(AT_NW * 64), 0, st, a);
}

}  // namespace
}  // namespace wavenc
}  // namespace dex
