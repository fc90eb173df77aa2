// out2_stamps: the linear-attention tail (linattn_fused.hip) at the three B = 1 shapes of GeDEX-LJ, fp32 x and y (the latency regime's
// operands): the direct form, the wave-split form (one 32-pixel slot per 4-wave workgroup; lane = pixel, and x / y as whole pixel rows:
// LinOut2P::rows) and at 80x512 the throughput form.  Event
// time per launch (back to back), the -DDEX_TIMING phase stamps of thread 0 of every workgroup (mean over workgroups, counter ticks: thread 0 = the wave of he tile 0 / co tile 0), and a bitwise check against the direct form.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -DDEX_TIMING -DDEX_LP_NS_OVERRIDE=o2st -I dex_tts_amd/csrc \
//         tools/out2_stamps.hip dex_tts_amd/csrc/linattn_fused.hip -o tools/out2_stamps
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
}
using namespace dex;

static unsigned short to_bf16(float f) { unsigned u; memcpy(&u, &f, 4); return (unsigned short)((u + 0x7fff + ((u >> 16) & 1)) >> 16); }
template <class T> static T* upload(const std::vector<T>& h) { T* d; hipMalloc(&d, h.size() * sizeof(T)); hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice); return d; }
static float val(size_t i, float s) { return s * ((float)((i * 2654435761u) % 1000) / 1000.f - 0.5f); }

struct Shape { const char* name; int H, W, C; };
struct Form { const char* name; int hw, out2_min, rows; };

int main() {
    int bad = 0;
    const Shape shapes[] = {{"40x256 C=128", 40, 256, 128}, {"40x256 C=64", 40, 256, 64}, {"80x512 C=64", 80, 512, 64}};
    const Form forms[] = {{"direct", 0, 1 << 30, 0}, {"wave-split", 1, 1 << 30, 0}, {"wave-split rows", 1, 1 << 30, 1}, {"throughput", 0, 0, 0}};
    const char* phase[6] = {"loads issued", "x exchange", "GEMM1", "q exchange", "GEMM2", "epilogue"};
    for (const Shape& s : shapes) {
        const int npix = s.H * s.W, C = s.C, CT = C / 32;
        std::vector<float> x((size_t)npix * C), bias(C);
        std::vector<unsigned short> wq(128 * C), w2(CT * 8 * 64 * 8);
        for (size_t i = 0; i < x.size(); ++i) x[i] = val(i, 2.f);
        for (size_t i = 0; i < wq.size(); ++i) wq[i] = to_bf16(val(i * 7 + 3, 0.25f));
        for (size_t i = 0; i < w2.size(); ++i) w2[i] = to_bf16(val(i * 5 + 1, 0.25f));
        for (int c = 0; c < C; ++c) bias[c] = val(c + 11, 0.2f);
        float* y; long long* dbg;
        hipMalloc(&y, (size_t)npix * C * 4); hipMalloc(&dbg, (size_t)((npix + 31) / 32) * 64);
        LinOut2P o{};
        o.X = upload(x); o.ldx = C; o.xb = (long)npix * C; o.npix = npix; o.C = C; o.Wq = upload(wq); o.W2 = upload(w2); o.bias = upload(bias);
        o.Y = y; o.ldy = C; o.yb = (long)npix * C; o.B = 1;
        printf("== %s (B = 1, fp32 x and y)\n", s.name);
        std::vector<float> ref;
        for (const Form& f : forms) {
            if (f.out2_min == 0 && s.H != 80) continue;
            char mn[32]; snprintf(mn, sizeof mn, "%d", f.out2_min); setenv("DEX_OUT2_MIN", mn, 1);
            o.hw = f.hw; o.rows = f.rows; o.dbg = nullptr;
            const int wgs = f.hw ? (npix + 31) / 32 : (npix + 127) / 128;
            hipMemset(y, 0, (size_t)npix * C * 4);
            hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
            for (int i = 0; i < 5; ++i) o2st::launch_linattn_out2(o, 0);
            hipDeviceSynchronize();
            hipEventRecord(a, 0);
            for (int i = 0; i < 200; ++i) o2st::launch_linattn_out2(o, 0);
            hipEventRecord(b, 0); hipEventSynchronize(b);
            float ms; hipEventElapsedTime(&ms, a, b);
            printf("  %-22s %5d wgs  %7.2f us/launch (back to back)\n", f.name, wgs, ms * 5.f);
            hipMemset(dbg, 0, (size_t)wgs * 64);
            o.dbg = dbg; o2st::launch_linattn_out2(o, 0); hipDeviceSynchronize(); o.dbg = nullptr;
            std::vector<long long> d((size_t)wgs * 8); hipMemcpy(d.data(), dbg, d.size() * 8, hipMemcpyDeviceToHost);
            if (f.out2_min != 0) {
                double m[8] = {0};
                for (int w = 0; w < wgs; ++w) for (int j = 0; j < 8; ++j) m[j] += (double)d[(size_t)w * 8 + j] / wgs;
                printf("     stamps (mean over workgroups, ticks):");
                for (int j = 0; j < 6; ++j) printf(" %s=%.0f", phase[j], m[j]);
                printf(" | total=%.0f\n", m[7]);
            }
            std::vector<float> out((size_t)npix * C);
            hipMemcpy(out.data(), y, out.size() * 4, hipMemcpyDeviceToHost);
            if (ref.empty()) { ref = out; continue; }
            size_t n = 0;
            for (size_t j = 0; j < out.size(); ++j) n += memcmp(&out[j], &ref[j], 4) != 0;
            printf("     bitwise y vs the direct form: %s (%zu of %zu differ)\n", n ? "DIFFERENT" : "IDENTICAL", n, out.size());
            if (n && f.out2_min != 0) bad = 1;       // (the throughput form's line is listed, not checked)
        }
    }
    return bad;
}
