// griffin_lim.hip — the reference's vocoder-free mel inversion (audio/tools.py:18-34 inv_mel_spec -> audio/audio_processing.py:66-82
// griffin_lim -> audio/stft.py:52-121 STFT.transform / STFT.inverse, window_sumsquare audio_processing.py:7-63) on the device, for a
// ragged batch.  Only the reference configuration: filter_length 1024, hop 256, win_length 1024, periodic Hann, 80 Slaney mels.
//
// The reference runs the STFT as a dense conv1d / conv_transpose1d with a 1026 x 1024 basis.  Here every frame is a 1024-point real
// FFT in LDS: a 512-point complex FFT (three radix-8 Stockham passes, one wave per frame, 8 points per lane) of z[m] = x[2m] + i x[2m+1]
// plus the real-split pass.  The reference's inverse basis pinv(4 F).T is exactly irfft / 4 (weight 1/N on DC and Nyquist, 2/N
// elsewhere; the imaginary parts of DC and Nyquist are ignored), so the inverse frame is the inverse real FFT of the recombined
// spectrum, scaled by 1/4096 and windowed.
//
// Kernels (all per-row arithmetic is independent of the batch: a row's result is bitwise the same row run alone):
//   gl_frame_kernel<MODE>  one frame per 64-thread workgroup, frames of a launch's rows numbered through per-row offsets:
//     ANALYSIS  gather the reflect-padded row around the frame, window, rFFT -> magnitude, atan2 phase          (STFT.transform)
//     SYNTH     magnitude, phase -> mag (cos, sin) -> irFFT, window -> frame buffer                             (STFT.inverse)
//               (the first Griffin-Lim step also copies the magnitudes frame-major into the workspace)
//     ITER      gather the current signal, window, rFFT, unit phasor (1, 0 at |X| = 0: atan2(0, 0) = 0) x magnitude, irFFT,
//               window -> frame buffer                                    (one Griffin-Lim iteration: transform + inverse fused)
//   gl_ola_kernel          one output sample per thread: the frames covering it added in ascending order (a gather, no atomics),
//                          divided by window_sumsquare where it is > tiny(float32), times 4, cropped by 512 at each end.
//   mel_to_linear_kernel   exp(mel), x Slaney basis (ascending over the filters that touch the bin), x 1000    (tools.py:19-26)
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dex_amd.h"
#include "kernels.h"

namespace {

constexpr int NFFT = 1024, HOP = 256, NB = 513, PAD = 512, NMEL = 80;
constexpr int ROWS = 64;             // rows per launch (their frame counts travel as kernel arguments)
constexpr int MIN_FRAMES_GL = 4;     // the reflect pad of the transform needs 256 (F - 1) > 512 samples
constexpr int MIN_FRAMES_INV = 2;

enum { ANALYSIS = 0, SYNTH = 1, ITER = 2 };

struct GlRows {
    int r0, n;                       // first row of this launch, rows in it
    int F[ROWS];                     // frames of each row
    int off[ROWS];                   // first frame of each row in the launch's frame numbering (prefix sum of F)
    int L[ROWS];                     // samples of each row (transform input / inverse output)
};

struct FrameP {
    const float2* tw;                // [1024] e^{-2 pi i k / 1024}
    const float* win;                // [1024] the reference's fp32 window
    const float* sig; long sig_ld;   // ANALYSIS / ITER input rows
    const float* mag; const float* phase; long spec_ld;   // [B][513][spec_ld]: ANALYSIS outputs (mag_out / phase_out), SYNTH inputs
    float* mag_out; float* phase_out;
    float* st;                       // [frame][513] magnitudes, frame-major (written by the first Griffin-Lim step, read by ITER)
    float* frames;                   // [frame][1024] windowed inverse frames
};

// LDS swizzle of a 512-entry fp32 array: the low five bits (the ds_read_b32 / ds_write_b32 bank) are XORed with bits 5-7 and 6-7,
// which makes every access pattern of the three passes (lane stride 1, 8, and the 64-strided groups of eight) and of the
// real-split pass conflict-free per 32-lane half.
__device__ __forceinline__ int sw(int a) { return a ^ ((a >> 5) & 7) ^ (((a >> 6) & 3) << 3); }

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 conjf2(float2 a) { return make_float2(a.x, -a.y); }

// 8-point DFT in registers, sign -1 (forward) or +1 (INV): one radix-2 decimation-in-frequency step, then two 4-point DFTs
template <bool INV>
__device__ __forceinline__ void dft8(float2 (&v)[8]) {
    constexpr float h = 0.70710678118654752f;
    float2 a[4], b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { a[k] = cadd(v[k], v[k + 4]); b[k] = csub(v[k], v[k + 4]); }
    // b[k] *= w8^k, w8 = e^{-+ i pi / 4}
    b[1] = INV ? make_float2(h * (b[1].x - b[1].y), h * (b[1].x + b[1].y)) : make_float2(h * (b[1].x + b[1].y), h * (b[1].y - b[1].x));
    b[2] = INV ? make_float2(-b[2].y, b[2].x) : make_float2(b[2].y, -b[2].x);
    b[3] = INV ? make_float2(-h * (b[3].x + b[3].y), h * (b[3].x - b[3].y)) : make_float2(h * (b[3].y - b[3].x), -h * (b[3].x + b[3].y));
    auto dft4 = [](const float2 (&u)[4], float2& y0, float2& y1, float2& y2, float2& y3) {
        const float2 c0 = cadd(u[0], u[2]), c1 = cadd(u[1], u[3]), d0 = csub(u[0], u[2]), e = csub(u[1], u[3]);
        const float2 d1 = INV ? make_float2(-e.y, e.x) : make_float2(e.y, -e.x);          // x (-+ i)
        y0 = cadd(c0, c1); y2 = csub(c0, c1); y1 = cadd(d0, d1); y3 = csub(d0, d1);
    };
    dft4(a, v[0], v[2], v[4], v[6]);
    dft4(b, v[1], v[3], v[5], v[7]);
}

// one radix-8 Stockham pass of the 512-point FFT: lane j reads in[j + 64 r], twiddles by e^{-+2 pi i (j % NS) r / (8 NS)},
// transforms, writes out[(j / NS) 8 NS + j % NS + r NS]
template <int NS, bool INV>
__device__ __forceinline__ void stockham_pass(const float* ire, const float* iim, float* ore, float* oim, const float2* tw, int j) {
    float2 v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) { const int a = sw(j + 64 * r); v[r] = make_float2(ire[a], iim[a]); }
    const int k = j % NS;
    if (NS > 1) {
#pragma unroll
        for (int r = 1; r < 8; ++r) {
            float2 t = tw[2 * k * r * (64 / NS)];
            if (INV) t.y = -t.y;
            v[r] = cmul(v[r], t);
        }
    }
    dft8<INV>(v);
    const int d = (j / NS) * NS * 8 + k;
#pragma unroll
    for (int r = 0; r < 8; ++r) { const int a = sw(d + r * NS); ore[a] = v[r].x; oim[a] = v[r].y; }
}

// 512-point FFT of buffer 0 into buffer 1 (buffer 0 is scratch); the caller has synchronised after filling buffer 0
template <bool INV>
__device__ __forceinline__ void fft512(float (&re)[2][512], float (&im)[2][512], const float2* tw, int lane) {
    stockham_pass<1, INV>(re[0], im[0], re[1], im[1], tw, lane);
    __syncthreads();
    stockham_pass<8, INV>(re[1], im[1], re[0], im[0], tw, lane);
    __syncthreads();
    stockham_pass<64, INV>(re[0], im[0], re[1], im[1], tw, lane);
    __syncthreads();
}

__device__ __forceinline__ int reflect(int j, int L) { return j < 0 ? -j : (j >= L ? 2 * (L - 1) - j : j); }

// unit phasor of x: (re, im) / |x|, (1, 0) at |x| = 0 (the reference's cos / sin of atan2(0, 0) = 0)
__device__ __forceinline__ float2 phasor(float2 x) {
    const float m = fmaxf(fabsf(x.x), fabsf(x.y));
    if (m == 0.f) return make_float2(1.f, 0.f);
    const float a = __fdiv_rn(x.x, m), b = __fdiv_rn(x.y, m);
    const float r = __fsqrt_rn(a * a + b * b);
    return make_float2(__fdiv_rn(a, r), __fdiv_rn(b, r));
}

template <int MODE>
__global__ __launch_bounds__(64) void gl_frame_kernel(const FrameP p, const GlRows R) {
    __shared__ float re[2][512], im[2][512];
    const int g = blockIdx.x, lane = threadIdx.x;
    int lo = 0, hi = R.n - 1;                                   // the row of frame g: the last with off <= g
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (R.off[mid] <= g) lo = mid; else hi = mid - 1; }
    const int r = lo, f = g - R.off[r], b = R.r0 + r;

    float2 Za[5], Zb[5];                                        // X[k], X[512 - k] of this lane's pairs k = lane + 64 i <= 256
    if (MODE != SYNTH) {
        const float* s = p.sig + (long)b * p.sig_ld;
        const int L = R.L[r], base = f * HOP - PAD;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int m = lane + 64 * i;
            re[0][sw(m)] = s[reflect(base + 2 * m, L)] * p.win[2 * m];
            im[0][sw(m)] = s[reflect(base + 2 * m + 1, L)] * p.win[2 * m + 1];
        }
        __syncthreads();
        fft512<false>(re, im, p.tw, lane);
        // real split: E = (Z[k] + conj Z[512-k]) / 2, O = (Z[k] - conj Z[512-k]) / 2i; X[k] = E + W^k O, X[512-k] = conj(E - W^k O)
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int k = lane + 64 * i;
            if (k > 256) break;
            const int kb = (512 - k) & 511;
            const float2 za = make_float2(re[1][sw(k)], im[1][sw(k)]), zb = make_float2(re[1][sw(kb)], im[1][sw(kb)]);
            const float2 E = make_float2(0.5f * (za.x + zb.x), 0.5f * (za.y - zb.y));
            const float2 O = make_float2(0.5f * (za.y + zb.y), -0.5f * (za.x - zb.x));
            const float2 wO = cmul(p.tw[k], O);
            Za[i] = cadd(E, wO);
            Zb[i] = conjf2(csub(E, wO));
            if (k == 0) { Za[i].y = 0.f; Zb[i].y = 0.f; }          // DC and Nyquist are real
        }
        if (MODE == ANALYSIS) {
            float* mo = p.mag_out + (long)b * NB * p.spec_ld + f;
            float* po = p.phase_out + (long)b * NB * p.spec_ld + f;
            auto put = [&](int k, float2 x) {
                mo[(long)k * p.spec_ld] = __fsqrt_rn(x.x * x.x + x.y * x.y);
                po[(long)k * p.spec_ld] = atan2f(x.y, x.x);
            };
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const int k = lane + 64 * i;
                if (k > 256) break;
                put(k, Za[i]);
                if (k < 256) put(512 - k, Zb[i]);
            }
            return;
        }
        // ITER: X <- S x phasor(X)
        const float* S = p.st + (long)(R.off[r] + f) * NB;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int k = lane + 64 * i;
            if (k > 256) break;
            const float2 ua = phasor(Za[i]), ub = phasor(Zb[i]);
            const float sa = S[k], sb = S[512 - k];
            Za[i] = make_float2(sa * ua.x, sa * ua.y);
            Zb[i] = make_float2(sb * ub.x, sb * ub.y);
        }
    } else {
        const float* mg = p.mag + (long)b * NB * p.spec_ld + f;
        const float* ph = p.phase + (long)b * NB * p.spec_ld + f;
        float* S = p.st ? p.st + (long)(R.off[r] + f) * NB : nullptr;
        auto get = [&](int k) {
            const float m = mg[(long)k * p.spec_ld];
            const double a = (double)ph[(long)k * p.spec_ld];
            if (S) S[k] = m;
            return make_float2(m * (float)cos(a), m * (float)sin(a));
        };
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int k = lane + 64 * i;
            if (k > 256) break;
            Za[i] = get(k);
            Zb[i] = k < 256 ? get(512 - k) : Za[i];
        }
    }
    // inverse real split (the imaginary parts of DC and Nyquist do not enter, as in irfft / the reference's pinv basis):
    // P = X[k] + conj X[512-k], Q = i conj(W^k) (X[k] - conj X[512-k]);  Z[k] = P + Q, Z[512-k] = conj(P - Q)
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int k = lane + 64 * i;
        if (k > 256) break;
        float2 xa = Za[i], xb = Zb[i];
        if (k == 0) { xa.y = 0.f; xb.y = 0.f; }
        const float2 P = cadd(xa, conjf2(xb)), M = csub(xa, conjf2(xb));
        const float2 cw = conjf2(p.tw[k]);
        const float2 t = cmul(cw, M);
        const float2 Q = make_float2(-t.y, t.x);
        const float2 z0 = cadd(P, Q);
        re[0][sw(k)] = z0.x; im[0][sw(k)] = z0.y;
        if (k > 0 && k < 256) { const float2 z1 = conjf2(csub(P, Q)); re[0][sw(512 - k)] = z1.x; im[0][sw(512 - k)] = z1.y; }
    }
    __syncthreads();
    fft512<true>(re, im, p.tw, lane);
    // frame = window x irfft / 4 (the reference's pinv(4 F)): z / 4096
    float2* fr = reinterpret_cast<float2*>(p.frames + (long)(R.off[r] + f) * NFFT);
    const float2* w2 = reinterpret_cast<const float2*>(p.win);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int m = lane + 64 * i;
        const float2 w = w2[m];
        fr[m] = make_float2(w.x * (re[1][sw(m)] * (1.f / 4096.f)), w.y * (im[1][sw(m)] * (1.f / 4096.f)));
    }
}

struct OlaP { const float* frames; const double* wsq; float* out; long out_ld; };

// output sample j of row b (padded position q = j + 512): frames i with 0 <= q - 256 i < 1024, ascending.  The envelope repeats
// window_sumsquare exactly: a float32 accumulator, each frame's float64 squared window added in double and rounded to float.
__global__ __launch_bounds__(256) void gl_ola_kernel(const OlaP p, const GlRows R) {
    const int r = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= p.out_ld) return;
    float* o = p.out + (long)(R.r0 + r) * p.out_ld;
    const int F = R.F[r];
    if (j >= (F - 1) * HOP) { o[j] = 0.f; return; }
    const int q = j + PAD;
    const int i_lo = q >= NFFT ? (q - NFFT) / HOP + 1 : 0, i_hi = min(F - 1, q / HOP);
    const float* fr = p.frames + (long)R.off[r] * NFFT;
    float acc = 0.f, ws = 0.f;
    for (int i = i_lo; i <= i_hi; ++i) {
        const int n = q - i * HOP;
        acc = __fadd_rn(acc, fr[(long)i * NFFT + n]);
        ws = (float)__dadd_rn((double)ws, p.wsq[n]);
    }
    o[j] = __fmul_rn(ws > FLT_MIN ? __fdiv_rn(acc, ws) : acc, 4.f);
}

// spec[b][k][f] = 1000 sum_j exp(mel[b][j][f]) basis[j][k] for f < T_b - 1 (the last mel frame is dropped), 0 past it
struct M2LP { const float* mel; const float* filt; const int2* range; float* spec; int T; };
__global__ __launch_bounds__(256) void mel_to_linear_kernel(const M2LP p, const GlRows R) {
    const int f = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y, r = blockIdx.z, b = R.r0 + r;
    const int Fo = p.T - 1;
    if (f >= Fo) return;
    float* o = p.spec + ((long)b * NB + k) * Fo + f;
    if (f >= R.F[r]) { *o = 0.f; return; }
    const float* m = p.mel + (long)b * NMEL * p.T + f;
    const int2 rg = p.range[k];
    float acc = 0.f;
    for (int j = rg.x; j < rg.y; ++j) acc = fmaf((float)exp((double)m[(long)j * p.T]), p.filt[j * NB + k], acc);
    *o = __fmul_rn(acc, 1000.f);
}

// the reference's window: scipy.signal.get_window('hann', 1024, fftbins=True) = general_cosine over np.linspace(-pi, pi, 1025)[:1024],
// 0.5 + 0.5 cos(n step - pi) evaluated as numpy does (one rounding per operation), so its squares are bitwise window_sumsquare's
void reference_window(std::vector<double>& w) {
#pragma clang fp contract(off)
    const double step = (M_PI - (-M_PI)) / NFFT;
    w.resize(NFFT);
    for (int n = 0; n < NFFT; ++n) {
        const double fac = (double)n * step + (-M_PI);
        w[n] = 0.5 + 0.5 * cos(fac);
    }
}

bool rows_ok(const int* v, int B, int lo, int hi) {
    if (!v || B < 1) return false;
    for (int b = 0; b < B; ++b)
        if (v[b] < lo || v[b] > hi) return false;
    return true;
}

// rows in launches of ROWS; F(b) frames and L(b) samples of row b; each launch's frames are numbered from its own first row
template <class Fn>
int for_rows(int B, const int* frames_of, const int* samples_of, Fn launch) {
    long base = 0;                                                 // first frame of the launch in the batch's numbering
    for (int r0 = 0; r0 < B; r0 += ROWS) {
        GlRows R;
        std::memset(&R, 0, sizeof R);
        R.r0 = r0; R.n = B - r0 < ROWS ? B - r0 : ROWS;
        int total = 0;
        for (int k = 0; k < R.n; ++k) { R.F[k] = frames_of[k]; R.L[k] = samples_of[k]; R.off[k] = total; total += R.F[k]; }
        frames_of += R.n; samples_of += R.n;
        launch(R, base, total);
        if (hipGetLastError() != hipSuccess) return DEX_ERR_HIP;
        base += total;
    }
    return DEX_OK;
}

}  // namespace

struct DexGl {
    void* mem = nullptr;                       // one allocation: tables below
    float2* tw = nullptr; float* win = nullptr; double* wsq = nullptr; float* filt = nullptr; int2* range = nullptr;
    std::string err;
    int fail(int rc, const char* msg) { err = msg; return rc; }
};

namespace {

constexpr size_t TW_OFF = 0, WIN_OFF = TW_OFF + NFFT * sizeof(float2), WSQ_OFF = WIN_OFF + NFFT * sizeof(float),
                 FILT_OFF = WSQ_OFF + NFFT * sizeof(double), RANGE_OFF = FILT_OFF + ((NMEL * NB * sizeof(float) + 255) & ~size_t(255)),
                 TABLES_BYTES = RANGE_OFF + NB * sizeof(int2);

struct Ws { float* frames; float* st; };
Ws carve(void* ws, long total_frames) {
    float* f = (float*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    return {f, f + total_frames * NFFT};
}

FrameP frame_params(const DexGl* gl) {
    FrameP p{};
    p.tw = gl->tw; p.win = gl->win;
    return p;
}

int check_spec_args(DexGl* gl, const void* a, const void* b, const int* frames_host, int B, int max_frames, int min_frames, const void* out,
                    void* ws, size_t ws_bytes) {
    if (!a || !b || !out || !ws || !frames_host) return gl->fail(DEX_ERR_ARG, "null pointer argument");
    if (B < 1) return gl->fail(DEX_ERR_ARG, "B must be >= 1");
    if (max_frames < min_frames)
        return gl->fail(DEX_ERR_ARG, min_frames == MIN_FRAMES_GL ? "a spectrogram needs at least 4 frames (the reflect pad of the transform)"
                                                                 : "a spectrogram needs at least 2 frames");
    if (!rows_ok(frames_host, B, min_frames, max_frames))
        return gl->fail(DEX_ERR_ARG, min_frames == MIN_FRAMES_GL ? "row frame counts must lie in [4, max_frames]"
                                                                 : "row frame counts must lie in [2, max_frames]");
    if (ws_bytes < dex_gl_workspace_bytes(B, max_frames)) return gl->fail(DEX_ERR_WORKSPACE, "workspace too small (dex_gl_workspace_bytes)");
    return DEX_OK;
}

// inverse frames (SYNTH, optionally copying the magnitudes frame-major) + overlap-add into out [B][256 (max_frames - 1)]
int enqueue_inverse(DexGl* gl, const float* mag, const float* phase, const int* frames_host, int B, int max_frames, float* out,
                    const Ws& w, bool keep_mag, hipStream_t st) {
    std::vector<int> L(B);
    for (int b = 0; b < B; ++b) L[b] = (frames_host[b] - 1) * HOP;
    const long out_ld = (long)(max_frames - 1) * HOP;
    return for_rows(B, frames_host, L.data(), [&](const GlRows& R, long base, int total) {
        FrameP p = frame_params(gl);
        p.mag = mag; p.phase = phase; p.spec_ld = max_frames;
        p.st = keep_mag ? w.st + base * NB : nullptr;
        p.frames = w.frames + base * NFFT;
        hipLaunchKernelGGL(gl_frame_kernel<SYNTH>, dim3(total), dim3(64), 0, st, p, R);
        OlaP o{p.frames, gl->wsq, out, out_ld};
        hipLaunchKernelGGL(gl_ola_kernel, dim3((unsigned)((out_ld + 255) / 256), R.n), dim3(256), 0, st, o, R);
    });
}

}  // namespace

extern "C" {

int dex_gl_create(DexGl** out) {
    if (!out) return DEX_ERR_ARG;
    *out = nullptr;
    std::vector<unsigned char> host(TABLES_BYTES, 0);
    float2* tw = (float2*)(host.data() + TW_OFF);
    float* win = (float*)(host.data() + WIN_OFF);
    double* wsq = (double*)(host.data() + WSQ_OFF);
    float* filt = (float*)(host.data() + FILT_OFF);
    int2* range = (int2*)(host.data() + RANGE_OFF);
    for (int k = 0; k < NFFT; ++k) {                              // e^{-2 pi i k / 1024} in fp64, rounded to fp32
        const double a = M_PI * (double)k / 512.0;
        tw[k] = make_float2((float)cos(a), (float)-sin(a));
    }
    std::vector<double> w;
    reference_window(w);
    for (int n = 0; n < NFFT; ++n) { win[n] = (float)w[n]; wsq[n] = w[n] * w[n]; }
    dex::slaney_mel_filterbank(filt);                             // the table dex_mel_* uses (librosa.filters.mel(22050, 1024, 80, 0, 8000))
    for (int k = 0; k < NB; ++k) {                                // the filters that touch bin k (the Slaney triangles: at most two)
        int j0 = NMEL, j1 = 0;
        for (int j = 0; j < NMEL; ++j)
            if (filt[j * NB + k] != 0.f) { j0 = j < j0 ? j : j0; j1 = j + 1; }
        range[k] = j0 < j1 ? make_int2(j0, j1) : make_int2(0, 0);
    }
    DexGl* gl = new DexGl();
    if (hipMalloc(&gl->mem, TABLES_BYTES) != hipSuccess || hipMemcpy(gl->mem, host.data(), TABLES_BYTES, hipMemcpyHostToDevice) != hipSuccess) {
        if (gl->mem) (void)hipFree(gl->mem);
        delete gl;
        return DEX_ERR_HIP;
    }
    unsigned char* d = (unsigned char*)gl->mem;
    gl->tw = (float2*)(d + TW_OFF); gl->win = (float*)(d + WIN_OFF); gl->wsq = (double*)(d + WSQ_OFF);
    gl->filt = (float*)(d + FILT_OFF); gl->range = (int2*)(d + RANGE_OFF);
    *out = gl;
    return DEX_OK;
}

void dex_gl_destroy(DexGl* gl) {
    if (!gl) return;
    if (gl->mem) (void)hipFree(gl->mem);
    delete gl;
}

const char* dex_gl_last_error(const DexGl* gl) { return gl ? gl->err.c_str() : "null Griffin-Lim context"; }

size_t dex_gl_workspace_bytes(int B, int max_frames) {
    if (B < 1 || max_frames < 1) return 0;
    return (size_t)B * max_frames * (NFFT + NB) * sizeof(float) + 256;
}

int dex_stft_transform(DexGl* gl, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, float* mag_dev, float* phase_dev,
                       dex_stream_t stream) {
    if (!gl) return DEX_ERR_ARG;
    if (!wav_dev || !mag_dev || !phase_dev || !lengths_host) return gl->fail(DEX_ERR_ARG, "null pointer argument");
    if (B < 1) return gl->fail(DEX_ERR_ARG, "B must be >= 1");
    if (n_samples <= PAD) return gl->fail(DEX_ERR_ARG, "the reflect pad needs more than 512 samples per row");
    if (!rows_ok(lengths_host, B, PAD + 1, n_samples)) return gl->fail(DEX_ERR_ARG, "row lengths must lie in [513, n_samples]");
    std::vector<int> F(B);
    for (int b = 0; b < B; ++b) F[b] = lengths_host[b] / HOP + 1;
    const long Fmax = n_samples / HOP + 1;
    const int rc = for_rows(B, F.data(), lengths_host, [&](const GlRows& R, long, int total) {
        FrameP p = frame_params(gl);
        p.sig = wav_dev; p.sig_ld = n_samples;
        p.mag_out = mag_dev; p.phase_out = phase_dev; p.spec_ld = Fmax;
        hipLaunchKernelGGL(gl_frame_kernel<ANALYSIS>, dim3(total), dim3(64), 0, (hipStream_t)stream, p, R);
    });
    return rc ? gl->fail(rc, "kernel launch failed") : DEX_OK;
}

int dex_stft_inverse(DexGl* gl, const float* mag_dev, const float* phase_dev, const int32_t* frames_host, int B, int max_frames, float* wav_dev,
                     void* workspace_dev, size_t workspace_bytes, dex_stream_t stream) {
    if (!gl) return DEX_ERR_ARG;
    if (int rc = check_spec_args(gl, mag_dev, phase_dev, frames_host, B, max_frames, MIN_FRAMES_INV, wav_dev, workspace_dev, workspace_bytes)) return rc;
    long total = 0;
    for (int b = 0; b < B; ++b) total += frames_host[b];
    const int rc = enqueue_inverse(gl, mag_dev, phase_dev, frames_host, B, max_frames, wav_dev, carve(workspace_dev, total), false,
                                   (hipStream_t)stream);
    return rc ? gl->fail(rc, "kernel launch failed") : DEX_OK;
}

int dex_griffin_lim(DexGl* gl, const float* mag_dev, const float* angles_dev, const int32_t* frames_host, int B, int max_frames, int n_iters,
                    float* wav_dev, void* workspace_dev, size_t workspace_bytes, dex_stream_t stream) {
    if (!gl) return DEX_ERR_ARG;
    if (n_iters < 0) return gl->fail(DEX_ERR_ARG, "n_iters must be >= 0");
    if (int rc = check_spec_args(gl, mag_dev, angles_dev, frames_host, B, max_frames, MIN_FRAMES_GL, wav_dev, workspace_dev, workspace_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    long total = 0;
    for (int b = 0; b < B; ++b) total += frames_host[b];
    const Ws w = carve(workspace_dev, total);
    // signal = inverse(S, angles)
    int rc = enqueue_inverse(gl, mag_dev, angles_dev, frames_host, B, max_frames, wav_dev, w, true, st);
    std::vector<int> L(B);
    for (int b = 0; b < B; ++b) L[b] = (frames_host[b] - 1) * HOP;
    const long out_ld = (long)(max_frames - 1) * HOP;
    // n_iters x: signal = inverse(S, phase(transform(signal)))
    for (int it = 0; it < n_iters && rc == DEX_OK; ++it)
        rc = for_rows(B, frames_host, L.data(), [&](const GlRows& R, long base, int count) {
            FrameP p = frame_params(gl);
            p.sig = wav_dev; p.sig_ld = out_ld;
            p.st = w.st + base * NB;
            p.frames = w.frames + base * NFFT;
            hipLaunchKernelGGL(gl_frame_kernel<ITER>, dim3(count), dim3(64), 0, st, p, R);
            OlaP o{p.frames, gl->wsq, wav_dev, out_ld};
            hipLaunchKernelGGL(gl_ola_kernel, dim3((unsigned)((out_ld + 255) / 256), R.n), dim3(256), 0, st, o, R);
        });
    return rc ? gl->fail(rc, "kernel launch failed") : DEX_OK;
}

int dex_mel_to_linear(DexGl* gl, const float* mel_dev, const int32_t* mel_frames_host, int B, int T, float* spec_dev, dex_stream_t stream) {
    if (!gl) return DEX_ERR_ARG;
    if (!mel_dev || !spec_dev || !mel_frames_host) return gl->fail(DEX_ERR_ARG, "null pointer argument");
    if (B < 1) return gl->fail(DEX_ERR_ARG, "B must be >= 1");
    if (T < 2) return gl->fail(DEX_ERR_ARG, "a mel needs at least 2 frames (the last one is dropped)");
    if (!rows_ok(mel_frames_host, B, 2, T)) return gl->fail(DEX_ERR_ARG, "row mel frame counts must lie in [2, T]");
    std::vector<int> F(B), none(B, 0);
    for (int b = 0; b < B; ++b) F[b] = mel_frames_host[b] - 1;
    const int rc = for_rows(B, F.data(), none.data(), [&](const GlRows& R, long, int) {
        M2LP p{mel_dev, gl->filt, gl->range, spec_dev, T};
        hipLaunchKernelGGL(mel_to_linear_kernel, dim3((T - 1 + 255) / 256, NB, R.n), dim3(256), 0, (hipStream_t)stream, p, R);
    });
    return rc ? gl->fail(rc, "kernel launch failed") : DEX_OK;
}

}  // extern "C"
