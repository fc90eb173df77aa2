// kvctx_stamps: the linear-attention context pass (linattn_fused.hip) at the three B = 1 shapes of GeDEX-LJ, both forms (4-wave /
// head-parallel), with the PRO prologue of the preceding ResnetBlock: event time per launch, the -DDEX_TIMING phase stamps of thread 0
// of every workgroup (mean over workgroups, in counter ticks), an nsub sweep, and a bitwise check of the forms (partials + Xout).  The
// head-parallel form runs with both deals of its prologue rows: lane = pixel, and the items in memory order (LinKvCtxP::rows).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -DDEX_TIMING -DDEX_LP_NS_OVERRIDE=kvst -I dex_tts_amd/csrc \
//         tools/kvctx_stamps.hip dex_tts_amd/csrc/linattn_fused.hip -o tools/kvctx_stamps
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>
#include <cmath>
#include "kernels.h"
#include "kernels_lp.h"

namespace dex {
int knob(const char* name) { const char* v = getenv(name); return (v && *v) ? atoi(v) : KNOB_UNSET; }
thread_local const char* g_last_symbol = nullptr;
}
using namespace dex;

static unsigned short to_bf16(float f) { unsigned u; memcpy(&u, &f, 4); return (unsigned short)((u + 0x7fff + ((u >> 16) & 1)) >> 16); }
template <class T> static T* upload(const std::vector<T>& h) { T* d; hipMalloc(&d, h.size() * sizeof(T)); hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice); return d; }
static float val(size_t i, float s) { return s * ((float)((i * 2654435761u) % 1000) / 1000.f - 0.5f); }

struct Shape { const char* name; int H, W, C, nsub, fl; };

int main() {
    int bad = 0;
    const Shape shapes[] = {{"80x512 C=64 (FL 13)", 80, 512, 64, 2, 13}, {"40x256 C=128 (FL 9)", 40, 256, 128, 1, 9}, {"40x256 C=64 (FL 9)", 40, 256, 64, 1, 9}, {"40x256 C=128 (FL 13)", 40, 256, 128, 1, 13}};
    const char* phase[7] = {"loads issued", "GN reduce", "prologue", "x-image barrier", "head chain(s)", "merge staging", "merge + stores"};
    for (const Shape& s : shapes) {
        const int npix = s.H * s.W, C = s.C;
        std::vector<unsigned short> h2(npix * C), wkv(256 * C);
        for (size_t i = 0; i < h2.size(); ++i) h2[i] = to_bf16(val(i, 2.f));
        for (size_t i = 0; i < wkv.size(); ++i) wkv[i] = to_bf16(val(i * 7 + 3, 0.25f));
        std::vector<float> res(npix * C), gam(C), bet(C), mask(s.W, 1.f);
        for (size_t i = 0; i < res.size(); ++i) res[i] = val(i * 3 + 1, 1.f);
        for (int c = 0; c < C; ++c) { gam[c] = 1.f + val(c, 0.2f); bet[c] = val(c + 11, 0.2f); }
        std::vector<long long> gn(8 * GN_SLOTS * 2, 0);
        for (int g = 0; g < 8; ++g) { gn[(g * GN_SLOTS) * 2] = 0; gn[(g * GN_SLOTS) * 2 + 1] = 1LL << 36; }   // mean 0, var 1 (2^-36 fixed point)
        const int maxblk = (npix + 127) / 128;
        float *pm, *ps, *pc; void* xo; long long* dbg;
        hipMalloc(&pm, 4 * maxblk * 32 * 4); hipMalloc(&ps, 4 * maxblk * 32 * 4); hipMalloc(&pc, (size_t)4 * maxblk * 1024 * 4);
        hipMalloc(&xo, (size_t)npix * C * 4); hipMalloc(&dbg, (size_t)maxblk * 64);
        LinKvCtxP k{};
        k.npix = npix; k.C = C; k.Wkv = upload(wkv); k.part_m = pm; k.part_s = ps; k.part_c = pc; k.B = 1;
        k.H2 = reinterpret_cast<const float*>(upload(h2)); k.gn_stats = upload(gn); k.gamma = upload(gam); k.beta = upload(bet);
        k.res = upload(res); k.ldres = C; k.resb = (long)npix * C; k.res_under_mask = (s.fl & 8) ? 1 : 0;
        k.mask = upload(mask); k.mask_ws = 1; k.mask_bstride = s.W; k.W = s.W; k.Xout = reinterpret_cast<float*>(xo);
        k.h2_bf16 = (s.fl & 1) ? 1 : 0; k.res_lp = 0; k.xout_lp = (s.fl & 4) ? 1 : 0;
        printf("== %s\n", s.name);
        std::vector<float> ref[3];
        for (int nsub : {1, 2, 4}) {
            k.nsub = nsub; k.nblk = (npix + 128 * nsub - 1) / (128 * nsub);
            for (int form : {0, 1, 2}) {                   // 4-wave, head-parallel lane = pixel, head-parallel rows in memory order
                const int hw = form > 0;
                k.headwaves = hw; k.rows = form == 2; k.dbg = nullptr;
                hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
                for (int i = 0; i < 5; ++i) kvst::launch_linattn_kvctx(k, 0);
                hipDeviceSynchronize();
                hipEventRecord(a, 0);
                for (int i = 0; i < 100; ++i) kvst::launch_linattn_kvctx(k, 0);
                hipEventRecord(b, 0); hipEventSynchronize(b);
                float ms; hipEventElapsedTime(&ms, a, b);
                printf("  nsub=%d %-14s %4d wgs  %7.2f us/launch (back to back)\n", nsub, form == 2 ? "head-par. rows" : hw ? "head-parallel" : "4-wave", k.nblk, ms * 10.f);
                if (nsub != s.nsub) continue;
                hipMemset(dbg, 0, (size_t)maxblk * 64);
                k.dbg = dbg; kvst::launch_linattn_kvctx(k, 0); hipDeviceSynchronize(); k.dbg = nullptr;
                std::vector<long long> d(k.nblk * 8); hipMemcpy(d.data(), dbg, d.size() * 8, hipMemcpyDeviceToHost);
                double m[8] = {0};
                for (int w = 0; w < k.nblk; ++w) for (int j = 0; j < 8; ++j) m[j] += (double)d[w * 8 + j] / k.nblk;
                printf("     stamps (mean over workgroups, ticks):");
                for (int j = 0; j < 7; ++j) printf(" %s=%.0f", phase[j], m[j]);
                printf(" | total=%.0f\n", m[7]);
                // bitwise: partials and Xout of this form
                const size_t nc = (size_t)4 * k.nblk * 1024, nm = (size_t)4 * k.nblk * 32, nx = (size_t)npix * C;
                std::vector<float> out(nc + 2 * nm + nx);
                hipMemcpy(out.data(), pc, nc * 4, hipMemcpyDeviceToHost);
                hipMemcpy(out.data() + nc, pm, nm * 4, hipMemcpyDeviceToHost);
                hipMemcpy(out.data() + nc + nm, ps, nm * 4, hipMemcpyDeviceToHost);
                hipMemcpy(out.data() + nc + 2 * nm, xo, nx * (k.xout_lp ? 2 : 4), hipMemcpyDeviceToHost);
                ref[form] = out;
            }
        }
        for (int form : {1, 2}) {
            const bool same = ref[0].size() == ref[form].size() && memcmp(ref[0].data(), ref[form].data(), ref[0].size() * 4) == 0;
            printf("  bitwise partials + Xout, %s vs 4-wave at nsub=%d: %s\n", form == 2 ? "head-parallel rows" : "head-parallel", s.nsub, same ? "IDENTICAL" : "DIFFERENT");
            if (same) continue;
            const int nblk = (npix + 128 * s.nsub - 1) / (128 * s.nsub);
            const size_t nc = (size_t)4 * nblk * 1024, nm = (size_t)4 * nblk * 32;
            const size_t cut[5] = {0, nc, nc + nm, nc + 2 * nm, ref[0].size()};
            const char* part[4] = {"part_c", "part_m", "part_s", "Xout"};
            for (int q = 0; q < 4; ++q) {
                size_t n = 0, first = 0; double mx = 0;
                for (size_t j = cut[q]; j < cut[q + 1]; ++j)
                    if (memcmp(&ref[0][j], &ref[form][j], 4)) { if (!n++) first = j - cut[q]; mx = std::max(mx, (double)fabsf(ref[0][j] - ref[form][j])); }
                printf("    %s: %zu of %zu differ, first %zu, max |d| %.3e\n", part[q], n, cut[q + 1] - cut[q], first, mx);
            }
            bad = 1;
        }
    }
    return bad;
}
