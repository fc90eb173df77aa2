// dit_ends_stamps: the two launches at the ends of the DiT bottleneck at the GeDEX-LJ B = 1, T = 512 shape (650 tokens; bf16 operands):
// PatchEmbed2D as one launch (patch_embed.hip) at 8 / 4 / 2 tokens per workgroup and the unchanged 8-token body on the 4- / 2-token grids,
// and the FinalLayer + unpatchify GEMM (igemm_bf16.hip) as the column walker at DEX_NWALK_SPLIT = 8 / 16 / 32 and as the small-grid
// form.  Event time per launch (back to back) and the
// -DDEX_TIMING phase stamps of thread 0 of every workgroup (mean over workgroups, counter ticks).  Timing only: the operands are
// synthetic and the weight twins are not each other's images - the bitwise checks are tests/test_gpu_dit_ends_small.py.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -DDEX_TIMING -DDEX_LP_NS_OVERRIDE=dest -I dex_tts_amd/csrc \
//         tools/dit_ends_stamps.hip dex_tts_amd/csrc/patch_embed.hip dex_tts_amd/csrc/igemm_bf16.hip -o tools/dit_ends_stamps
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "kernels.h"
#include "kernels_lp.h"

namespace dex {
int knob(const char* name) { const char* v = getenv(name); return (v && *v) ? atoi(v) : KNOB_UNSET; }
thread_local const char* g_last_symbol = nullptr;
namespace dest { void pe_set_dbg(long long*); void pe_set_cut(int); void nw_set_dbg(long long*); }
}
using namespace dex;

static unsigned short to_bf16(float f) { unsigned u; memcpy(&u, &f, 4); return (unsigned short)((u + 0x7fff + ((u >> 16) & 1)) >> 16); }
template <class T> static T* upload(const std::vector<T>& h) { T* d; hipMalloc(&d, h.size() * sizeof(T)); hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice); return d; }
static float val(size_t i, float s) { return s * ((float)((i * 2654435761u) % 1000) / 1000.f - 0.5f); }
static std::vector<float> fvec(size_t n, size_t salt, float s) { std::vector<float> v(n); for (size_t i = 0; i < n; ++i) v[i] = val(i * 3 + salt, s); return v; }
static std::vector<unsigned short> hvec(size_t n, size_t salt, float s) { std::vector<unsigned short> v(n); for (size_t i = 0; i < n; ++i) v[i] = to_bf16(val(i * 7 + salt, s)); return v; }

template <class F> static void measure(const char* name, int wgs, long long* dbg, void (*set_dbg)(long long*), const char* const* phase, int nphase, F launch) {
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    for (int i = 0; i < 5; ++i) launch();
    hipDeviceSynchronize();
    hipEventRecord(a, 0);
    for (int i = 0; i < 200; ++i) launch();
    hipEventRecord(b, 0); hipEventSynchronize(b);
    float ms; hipEventElapsedTime(&ms, a, b);
    printf("  %-34s %4d wgs  %7.2f us/launch (back to back)\n", name, wgs, ms * 5.f);
    hipMemset(dbg, 0, (size_t)wgs * 64);
    set_dbg(dbg); launch(); hipDeviceSynchronize(); set_dbg(nullptr);
    std::vector<long long> d((size_t)wgs * 8); hipMemcpy(d.data(), dbg, d.size() * 8, hipMemcpyDeviceToHost);
    double m[8] = {0};
    for (int w = 0; w < wgs; ++w) for (int j = 0; j < 8; ++j) m[j] += (double)d[(size_t)w * 8 + j] / wgs;
    printf("     stamps (mean over workgroups, ticks):");
    for (int j = 0; j < nphase; ++j) printf(" %s=%.0f", phase[j], m[j]);
    printf(" | total=%.0f\n", m[7]);
}

int main() {
    const int Hm = 40, Wm = 256, C = 128, hid = 256, KS = 7, S = 4, Hf = 10, Wt = 65, ntok = Hf * Wt, T = 512;
    long long* dbg; hipMalloc(&dbg, 4096 * 64);
    std::vector<float> ones(T, 1.f);
    const float* mask = upload(ones);
    {   // ---- PatchEmbed2D
        DwConvP p{};
        p.X = upload(fvec((size_t)Hm * Wm * C, 1, 2.f)); p.ldx = C; p.xb = (long)Hm * Wm * C; p.Hi = Hm; p.Wi = Wm; p.C = C;
        p.k = KS; p.s = S; p.pad = KS / 2; p.Wd = upload(fvec((size_t)KS * KS * C, 5, 0.3f)); p.bd = upload(fvec(C, 9, 0.1f));
        p.mask = mask; p.mask_ws = 2; p.mask_bstride = T; p.Y = nullptr; p.Hf = Hf; p.Wt = Wt; p.B = 1;
        const unsigned short* wb = upload(hvec((size_t)hid * C, 3, 0.25f));
        const float* bias = upload(fvec(hid, 13, 0.1f));
        float* emb; hipMalloc(&emb, (size_t)ntok * hid * 4);
        const char* phase[6] = {"requests issued", "LDS barrier", "depthwise done", "barrier", "MFMA chains", "stores issued"};
        printf("== patch embedding, %d tokens (7 x 7 / stride 4, C = %d -> %d)\n", ntok, C, hid);
        for (int tok : {8, 4, 2}) {
            char v[8]; snprintf(v, sizeof v, "%d", tok); setenv("DEX_PE_TOK", v, 1);
            char name[48]; snprintf(name, sizeof name, "%d tokens per workgroup", tok);
            measure(name, (ntok + tok - 1) / tok, dbg, dest::pe_set_dbg, phase, 6, [&] { dest::launch_patch_embed_fused(p, wb, bias, emb, hid, 0); });
        }
        // the premise's cut-grid measurement: the UNCHANGED 8-token body with 4 / 2 live tokens per workgroup on the 4- / 2-token grid (its
        // 49 mask and 49 weight requests per item kept) - the grid effect without the small tiles' changes; outputs of dead rows are not stored
        setenv("DEX_PE_TOK", "8", 1);
        for (int cut : {4, 2}) {
            dest::pe_set_cut(cut);
            char name[48]; snprintf(name, sizeof name, "8-token body cut to %d live tokens", cut);
            measure(name, (ntok + cut - 1) / cut, dbg, dest::pe_set_dbg, phase, 6, [&] { dest::launch_patch_embed_fused(p, wb, bias, emb, hid, 0); });
        }
        dest::pe_set_cut(0);
        unsetenv("DEX_PE_TOK");
    }
    {   // ---- FinalLayer + unpatchify
        const int N = S * S * C, ldc = 2 * C;
        IGemmP g{};
        g.A = upload(fvec((size_t)ntok * hid, 21, 2.f)); g.lda = hid; g.a_bstride = (long)ntok * hid; g.Hi = Hf; g.Wi = Wt; g.Cin = hid;
        g.KH = 1; g.KW = 1; g.sh = 1; g.sw = 1; g.step_h = 1; g.step_w = 1; g.Ho = Hf; g.Wo = Wt;
        g.Wbf = upload(hvec((size_t)N * hid, 23, 0.25f)); g.Wfrag = upload(hvec((size_t)N * hid, 29, 0.25f));
        g.N = N; g.K = hid; g.ksplit = 1; g.groups = 1; g.bias = upload(fvec(N, 31, 0.1f));
        unsigned short* out; hipMalloc(&out, (size_t)Hm * Wm * ldc * 2);
        g.C = reinterpret_cast<float*>(out); g.ldc = ldc; g.c_bstride = (long)Hm * Wm * ldc; g.c_coff = C; g.c_lp = 1;
        g.OHf = Hm; g.OWf = Wm; g.osh = 1; g.osw = 1; g.inmask_ws = 1; g.outmask = mask; g.outmask_ws = 2; g.mask_bstride = T;
        g.gate_nstride = 1; g.unpatch_s = S; g.unpatch_C = C; g.B = 1;
        const float* mod = upload(fvec(2 * hid, 37, 0.2f));
        g.ln_shift = mod; g.ln_scale = mod + hid; g.ln_step_stride = 2L * hid;
        const char* phase[5] = {"requests issued", "rows staged", "barrier", "MFMA chains", "scatter issued"};
        printf("== FinalLayer + unpatchify, %d x %d x %d, 16-bit output\n", ntok, hid, N);
        setenv("DEX_NWALK_SMALL", "0", 1);
        for (int ns : {8, 16, 32}) {
            char v[8]; snprintf(v, sizeof v, "%d", ns); setenv("DEX_NWALK_SPLIT", v, 1);
            char name[48]; snprintf(name, sizeof name, "walker, DEX_NWALK_SPLIT=%d", ns);
            measure(name, (ntok + 63) / 64 * ns, dbg, dest::nw_set_dbg, phase, 5, [&] { dest::launch_igemm_lp(g, 0); });
        }
        unsetenv("DEX_NWALK_SPLIT"); setenv("DEX_NWALK_SMALL", "1", 1);
        measure("small-grid form (32 rows x 256)", (ntok + 31) / 32 * (N / 256), dbg, dest::nw_set_dbg, phase, 5, [&] { dest::launch_igemm_lp(g, 0); });
    }
    return 0;
}
