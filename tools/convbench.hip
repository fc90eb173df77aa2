// tools/convbench.hip — the 64->64 convolution kernels alone at batch size: timing + (with -DDEX_TIMING) the phase
// cycle counters of the strip-streaming kernel.  `convbench b1`: the B = 1 patch-conv launches of the headline in their current
// one-round and resident-weights forms (bitwise comparison, timing, the current grid cut to one round), and with -DDEX_TIMING each
// workgroup's phase counters next to the CU it ran on.  Build: see tools/convbench.sh
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <tuple>
#include <vector>
#include "../dex_tts_amd/csrc/kernels.h"
#include "../dex_tts_amd/csrc/kernels_lp.h"      // reduced-precision launchers, bf16 build (namespace dex::bf16)
#include "../dex_tts_amd/csrc/conv3x3_bf16.hip"  // (the launcher's templates: single forms and cut grids)
using namespace dex;
using namespace dex::bf16;
namespace dex {
thread_local const char* g_last_symbol = nullptr;                         // defined in lp_dispatch.hip in the library build
int knob(const char* name) { const char* e = getenv(name); return e ? atoi(e) : KNOB_UNSET; }   // (dex_api.hip in the library build)
}
static float* dalloc(size_t n, int fill = 0) { float* p; hipMalloc(&p, n * 4); hipMemset(p, fill, n * 4); return p; }
int main_b1();
int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "b1")) return main_b1();
    const int B = argc > 1 ? atoi(argv[1]) : 32, H = 80, W = 512, C = 64;
    const long npix = (long)H * W;
    float* x = dalloc(B * npix * C); float* y = dalloc(B * npix * C); float* res = dalloc(B * npix * C); float* xout = dalloc(B * npix * C);
    unsigned short* wb; hipMalloc(&wb, 9L * C * C * 2); hipMemset(wb, 0, 9L * C * C * 2);
    float* bias = dalloc(C); float* mask = dalloc((size_t)B * W, 0x3f); gnfix_t* st = (gnfix_t*)dalloc(8 * 64 * 2 * 2 * B); gnfix_t* st2 = (gnfix_t*)dalloc(8 * 64 * 2 * 2 * B);
    float* gam = dalloc(C); float* bet = dalloc(C);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    for (int variant = 0; variant < 6; ++variant) {
        Conv3P p{}; p.X = x; p.ldx = C; p.H = H; p.W = W; p.Cin = C; p.Cout = C; p.Wbf = wb; p.bias = bias; p.Y = y;
        p.mask = mask; p.mask_ws = 1; p.mask_bstride = W; p.gn_stats = st; p.B = B;
        const char* nm = "plain fp32->fp32";
        if (variant >= 1) { p.pro_stats = st2; p.pro_gamma = gam; p.pro_beta = bet; nm = "PRO fp32->fp32"; }
        if (variant == 2) { p.x_bf16 = 1; p.y_bf16 = 1; nm = "PRO bf16->bf16"; }
        if (variant == 3) { p.pro_res = res; p.pro_xout = xout; nm = "PRO2 fp32->fp32"; }
        if (variant == 4) { p.pro_res = res; p.pro_xout = xout; p.x_bf16 = 1; p.y_bf16 = 1; nm = "PRO2 bf16->bf16"; }
        if (variant == 5) { p.y_bf16 = 1; nm = "plain fp32->bf16"; }
        for (int mode = 0; mode < 3; ++mode) {
            setenv("DEX_CONV_STREAM", mode ? "1" : "0", 1);
            setenv("DEX_CONV_PP", mode == 2 ? "1" : "0", 1);
            for (int it = 0; it < 3; ++it) launch_conv3x3_lp(p, 0);
            hipEventRecord(e0, 0);
            for (int it = 0; it < 20; ++it) launch_conv3x3_lp(p, 0);
            hipEventRecord(e1, 0); hipEventSynchronize(e1);
            float ms; hipEventElapsedTime(&ms, e0, e1);
            printf("%-18s %s: %8.2f us\n", nm, mode == 2 ? "pingpong" : mode ? "stream  " : "tile    ", ms * 1000 / 20);
        }
#ifdef DEX_TIMING
        {   // ping-pong form: per group (two per workgroup) cycles by role
            setenv("DEX_CONV_PP", "1", 1); setenv("DEX_CONV_STREAM", "1", 1);
            const int nb = 2 * 1024;
            long long* dbg; hipMalloc(&dbg, (size_t)nb * 64); hipMemset(dbg, 0, (size_t)nb * 64);
            p.dbg = dbg; launch_conv3x3_lp(p, 0); hipDeviceSynchronize(); p.dbg = nullptr;
            std::vector<long long> h((size_t)nb * 8); hipMemcpy(h.data(), dbg, (size_t)nb * 64, hipMemcpyDeviceToHost);
            double a[8] = {0}; int n = 0; for (int bl = 0; bl < nb; ++bl) if (h[(size_t)bl * 8 + 7]) { ++n; for (int k = 0; k < 8; ++k) a[k] += h[(size_t)bl * 8 + k]; }
            if (n) printf("   ping-pong, avg cycles per group (%d groups): mfma role %.0f | emit %.0f | convert %.0f | barrier wait %.0f | loop total %.0f\n",
                   n, a[1] / n, a[2] / n, a[3] / n, a[4] / n, a[7] / n);
            hipFree(dbg);
        }
#endif
        setenv("DEX_CONV_PP", "0", 1);
#ifdef DEX_TIMING
        if (!conv3x3_stream_tiles(p)) {                    // small grid: the tile kernel's phase counters
            const int nb = (W / 32) * (H / 4) * B;
            long long* dbg; hipMalloc(&dbg, (size_t)nb * 64); hipMemset(dbg, 0, (size_t)nb * 64);
            p.dbg = dbg; launch_conv3x3_lp(p, 0); hipDeviceSynchronize(); p.dbg = nullptr;
            std::vector<long long> h((size_t)nb * 8); hipMemcpy(h.data(), dbg, (size_t)nb * 64, hipMemcpyDeviceToHost);
            double a[8] = {0}; for (int bl = 0; bl < nb; ++bl) for (int k = 0; k < 8; ++k) a[k] += h[(size_t)bl * 8 + k];
            printf("   tile kernel, avg cycles/wg (%d wgs): issue loads %.0f | GN coeffs + barrier %.0f | convert + LDS %.0f | nine taps %.0f | epilogue %.0f | total %.0f\n",
                   nb, a[0] / nb, a[1] / nb, a[2] / nb, a[3] / nb, a[4] / nb, a[7] / nb);
            hipFree(dbg);
        } else {
            const int tpw = conv3x3_stream_tiles(p);
            const int nb = (W / 32) * ((H / 8 + tpw - 1) / tpw) * B;
            long long* dbg; hipMalloc(&dbg, (size_t)nb * 64); hipMemset(dbg, 0, (size_t)nb * 64);
            p.dbg = dbg; launch_conv3x3_lp(p, 0); hipDeviceSynchronize(); p.dbg = nullptr;
            std::vector<long long> h((size_t)nb * 8); hipMemcpy(h.data(), dbg, (size_t)nb * 64, hipMemcpyDeviceToHost);
            double a[8] = {0}; for (int bl = 0; bl < nb; ++bl) for (int k = 0; k < 8; ++k) a[k] += h[(size_t)bl * 8 + k];
            printf("   avg cycles/wg (tpw=%d, %d wgs): setup %.0f | per wg total: load-issue %.0f mfma %.0f epilogue %.0f barrier1 %.0f convert+lds %.0f barrier2 %.0f | total %.0f\n",
                   tpw, nb, a[0] / nb, a[1] / nb, a[2] / nb, a[3] / nb, a[4] / nb, a[5] / nb, a[6] / nb, a[7] / nb);
            hipFree(dbg);
        }
#endif
    }
    return 0;
}

// ---- B = 1 ----------------------------------------------------------------------------------------------------------------------
static unsigned g_rng = 12345u;
static float frand() { g_rng = g_rng * 1664525u + 1013904223u; return ((g_rng >> 8) & 0xffff) / 32768.f - 1.f; }
static void* upload(const std::vector<float>& h) { void* d; hipMalloc(&d, h.size() * 4); hipMemcpy(d, h.data(), h.size() * 4, hipMemcpyHostToDevice); return d; }
static void* upload16(size_t n, float scale) {                 // random bf16 values
    std::vector<unsigned short> h(n);
    for (auto& v : h) { const float f = frand() * scale; unsigned u; memcpy(&u, &f, 4); v = (unsigned short)(u >> 16); }
    void* d; hipMalloc(&d, n * 2); hipMemcpy(d, h.data(), n * 2, hipMemcpyHostToDevice); return d;
}
static std::vector<float> rnd(size_t n, float scale, float off = 0.f) { std::vector<float> h(n); for (auto& v : h) v = off + scale * frand(); return h; }

typedef void (*LaunchFn)(const Conv3P&, hipStream_t);
// the current form at its full grid or cut to `cut` row tiles (timing only: the cut launch leaves rows uncomputed)
template <int CC, int COUT, int NSL, int TH, bool PRO2, bool RES, bool XB, int NW>
static void launch_cut(const Conv3P& p, int rows_cut) {
    constexpr int LDP = CC + 8;
    const size_t lds = ((size_t)(TH + 2) * 34 * LDP + (2 + (RES ? 1 : 0)) * NSL * LDP) * sizeof(unsigned short);
    hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_lp_kernel<CC, COUT, NSL, TH, PRO2, RES, XB, NW>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    dim3 grid((p.W + 31) / 32, rows_cut, p.B * (COUT / NSL));
    hipLaunchKernelGGL((conv3x3_lp_kernel<CC, COUT, NSL, TH, PRO2, RES, XB, NW>), grid, dim3(64 * NW), lds, 0, p);
}

struct B1Bufs { float *y, *ry, *xo; gnfix_t* st; size_t ny, nst; };
static void clear(const B1Bufs& b) { hipMemset(b.y, 0, b.ny * 4); hipMemset(b.ry, 0, b.ny * 4); hipMemset(b.xo, 0, b.ny * 4); hipMemset(b.st, 0, b.nst * 8); }
// y, shortcut output, block output, and the GroupNorm sums per (group, moment): the slot a workgroup adds into follows its grid
// position, so only the sums over the slots (what gn_slots_reduce computes) are the same between two grids
static std::vector<char> snap(const B1Bufs& b) {
    std::vector<char> h(b.ny * 12 + 16 * 8);
    std::vector<gnfix_t> st(b.nst);
    hipDeviceSynchronize();
    hipMemcpy(h.data(), b.y, b.ny * 4, hipMemcpyDeviceToHost); hipMemcpy(h.data() + b.ny * 4, b.ry, b.ny * 4, hipMemcpyDeviceToHost);
    hipMemcpy(h.data() + b.ny * 8, b.xo, b.ny * 4, hipMemcpyDeviceToHost); hipMemcpy(st.data(), b.st, b.nst * 8, hipMemcpyDeviceToHost);
    gnfix_t sums[16] = {};
    for (int g = 0; g < 8; ++g)
        for (int s = 0; s < GN_SLOTS; ++s) { sums[2 * g] += st[(g * GN_SLOTS + s) * 2]; sums[2 * g + 1] += st[(g * GN_SLOTS + s) * 2 + 1]; }
    memcpy(h.data() + b.ny * 12, sums, sizeof sums);
    return h;
}
static const char* diff_part(const std::vector<char>& a, const std::vector<char>& b, size_t ny) {
    const char* nm[4] = {"y", "shortcut y", "block output", "GN sums"};
    for (int k = 0; k < 4; ++k) {
        const size_t o = k * ny * 4, n = k < 3 ? ny * 4 : 16 * 8;
        if (memcmp(a.data() + o, b.data() + o, n)) return nm[k];
    }
    return "equal";
}
template <class F>
static float time_us(F f, int n = 50) {
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    for (int i = 0; i < 5; ++i) f();
    hipEventRecord(e0, 0);
    for (int i = 0; i < n; ++i) f();
    hipEventRecord(e1, 0); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1); hipEventDestroy(e0); hipEventDestroy(e1);
    return ms * 1000.f / n;
}
#ifdef DEX_TIMING
// per-workgroup phase cycles of one launch, split by whether the workgroup shared its CU with another of the launch
static void stamps(const char* nm, const std::function<void(const Conv3P&)>& f, Conv3P p, int nwg, const B1Bufs& bb) {
    long long* dbg; hipMalloc(&dbg, (size_t)nwg * 64); hipMemset(dbg, 0, (size_t)nwg * 64);
    clear(bb); p.dbg = dbg; f(p); hipDeviceSynchronize();
    std::vector<long long> h((size_t)nwg * 8); hipMemcpy(h.data(), dbg, (size_t)nwg * 64, hipMemcpyDeviceToHost); hipFree(dbg);
    std::map<std::tuple<int, int, int, int>, int> per_cu;
    auto key = [&](int w) { const unsigned hw = (unsigned)h[(size_t)w * 8 + 5];
        return std::make_tuple((int)h[(size_t)w * 8 + 6], (int)((hw >> 13) & 7), (int)((hw >> 12) & 1), (int)((hw >> 8) & 15)); };
    for (int w = 0; w < nwg; ++w) per_cu[key(w)]++;
    double a[2][8] = {}; int n[2] = {0, 0};
    for (int w = 0; w < nwg; ++w) { const int s = per_cu[key(w)] > 1; ++n[s]; for (int k = 0; k < 8; ++k) a[s][k] += h[(size_t)w * 8 + k]; }
    printf("   %-34s %zu CUs used; cycles per wg: issue loads | GN + barrier | convert + LDS | taps | epilogue | total\n", nm, per_cu.size());
    for (int s = 0; s < 2; ++s) if (n[s])
        printf("      %-9s (%3d wgs): %6.0f | %6.0f | %6.0f | %6.0f | %6.0f | %6.0f\n", s ? "CU shared" : "CU alone", n[s],
               a[s][0] / n[s], a[s][1] / n[s], a[s][2] / n[s], a[s][3] / n[s], a[s][4] / n[s], a[s][7] / n[s]);
}
#endif

int main_b1() {
    int ncu = 0; hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0);
    printf("B = 1 patch convolutions, %d CUs; times: mean of 50 back-to-back launches (device events)\n", ncu);
    const size_t NPIX = 80 * 512, CMAX = 128;
    void* x32 = upload(rnd(NPIX * CMAX, 1.f));
    void* x16 = upload16(NPIX * CMAX, 1.f);
    void* res = upload(rnd(NPIX * CMAX, 1.f));
    void* wb = upload16(9 * CMAX * CMAX, 0.05f);
    void* rw = upload16(CMAX * CMAX, 0.1f);
    void* bias = upload(rnd(CMAX, 0.1f)); void* rb = upload(rnd(CMAX, 0.1f));
    void* gam = upload(rnd(CMAX, 0.2f, 1.f)); void* bet = upload(rnd(CMAX, 0.2f));
    void* tadd = upload(rnd(CMAX, 0.2f));
    std::vector<float> mh(512, 1.f); for (int i = 480; i < 512; ++i) mh[i] = 0.f;   // a masked tail, as in a padded utterance
    void* mask = upload(mh);
    const size_t nst = 8 * GN_SLOTS * 2;
    B1Bufs bb{dalloc(NPIX * CMAX), dalloc(NPIX * CMAX), dalloc(NPIX * CMAX), (gnfix_t*)dalloc(nst * 2), NPIX * CMAX, nst};
    gnfix_t* pst[2] = {(gnfix_t*)dalloc(nst * 2), (gnfix_t*)dalloc(nst * 2)};   // producer statistics for the prologue forms (C = 64 / 128)
    for (int c = 0; c < 2; ++c) {
        const int C = c ? 128 : 64, H = c ? 40 : 80, W = c ? 256 : 512;
        Conv3P q{}; q.X = (const float*)x32; q.ldx = C; q.H = H; q.W = W; q.Cin = C; q.Cout = C; q.Wbf = wb; q.bias = (const float*)bias;
        q.Y = bb.y; q.mask = (const float*)mask; q.mask_ws = c ? 2 : 1; q.gn_stats = pst[c]; q.B = 1;
        launch_conv3x3_lp(q, 0);
    }
    hipDeviceSynchronize();
    struct Case { const char* nm; int C, Co, H, W; int pro, pro2, xb, res; };
    const Case cases[] = {
        {"80x512 64->64 PRO bf16 in", 64, 64, 80, 512, 1, 0, 1, 0},
        {"80x512 64->64 PRO2 bf16 in", 64, 64, 80, 512, 1, 1, 1, 0},
        {"80x512 64->64 plain fp32 in", 64, 64, 80, 512, 0, 0, 0, 0},
        {"40x256 64->128 +1x1 shortcut", 64, 128, 40, 256, 0, 0, 0, 1},
        {"40x256 128->128 PRO bf16 in", 128, 128, 40, 256, 1, 0, 1, 0},
        {"40x256 128->128 PRO2 bf16 in", 128, 128, 40, 256, 1, 1, 1, 0},
        {"40x256 64->64 PRO bf16 in", 64, 64, 40, 256, 1, 0, 1, 0},
        {"40x256 64->64 PRO2 bf16 in", 64, 64, 40, 256, 1, 1, 1, 0},
        {"40x256 64->64 plain fp32 in", 64, 64, 40, 256, 0, 0, 0, 0},
    };
    int bad = 0;
    for (const Case& c : cases) {
        Conv3P p{}; p.X = (const float*)(c.xb ? x16 : x32); p.ldx = c.C; p.H = c.H; p.W = c.W; p.Cin = c.C; p.Cout = c.Co; p.Wbf = wb;
        p.bias = (const float*)bias; p.Y = bb.y; p.mask = (const float*)mask; p.mask_ws = c.H == 80 ? 1 : 2; p.gn_stats = bb.st; p.B = 1;
        p.step = 0; p.x_bf16 = c.xb; p.y_bf16 = c.xb;
        if (c.pro) { p.pro_stats = pst[c.C == 128]; p.pro_gamma = (const float*)gam; p.pro_beta = (const float*)bet; p.pro_tadd = (const float*)tadd; }
        if (c.pro2) { p.pro_res = (const float*)res; p.pro_xout = bb.xo; }
        if (c.res) { p.res_w = rw; p.res_b = (const float*)rb; p.res_y = bb.ry; }
        // the current form, its grid cut to 256 workgroups, and the one-round forms
        std::vector<std::pair<const char*, std::function<void(const Conv3P&)>>> forms;
        int rows_old = 0, nwg_old = 0, nwg_new = 256;
        bool has_cut = true;
        if (c.C == 64 && c.Co == 64 && c.H == 40) {          // 160 workgroups of the 2-row form: streamed vs resident weights
            nwg_old = nwg_new = 160; has_cut = false;
            if (c.pro2) {
                forms.push_back({"current <64,64,64,2,PRO2,XB,4>", [](const Conv3P& q) { launch_c3<64, 64, 64, 2, true, false, true, 4>(q, 0); }});
                forms.push_back({"resident", [](const Conv3P& q) { launch_c3<64, 64, 64, 2, true, false, true, 4, true>(q, 0); }});
            } else if (c.xb) {
                forms.push_back({"current <64,64,64,2,PRO,XB,4>", [](const Conv3P& q) { launch_c3<64, 64, 64, 2, false, false, true, 4>(q, 0); }});
                forms.push_back({"resident", [](const Conv3P& q) { launch_c3<64, 64, 64, 2, false, false, true, 4, true>(q, 0); }});
            } else {
                forms.push_back({"current <64,64,64,2,plain,4>", [](const Conv3P& q) { launch_c3<64, 64, 64, 2, false, false, false, 4>(q, 0); }});
                forms.push_back({"resident", [](const Conv3P& q) { launch_c3<64, 64, 64, 2, false, false, false, 4, true>(q, 0); }});
            }
        } else if (c.C == 64 && c.Co == 64) {
            rows_old = 20; nwg_old = 320;
            if (c.pro2) {
                forms.push_back({"current <64,64,64,4,PRO2,XB,4>", [](const Conv3P& q) { launch_c3<64, 64, 64, 4, true, false, true, 4>(q, 0); }});
                forms.push_back({"current cut to 16 x 16", [](const Conv3P& q) { launch_cut<64, 64, 64, 4, true, false, true, 4>(q, 16); }});
                forms.push_back({"one round, 10 waves", [](const Conv3P& q) { launch_c3<64, 64, 64, 5, true, false, true, 10>(q, 0); }});
                forms.push_back({"one round, 5 waves", [](const Conv3P& q) { launch_c3<64, 64, 64, 5, true, false, true, 5>(q, 0); }});
                forms.push_back({"one round, 10 waves, resident", [](const Conv3P& q) { launch_c3<64, 64, 64, 5, true, false, true, 10, true>(q, 0); }});
            } else if (c.xb) {
                forms.push_back({"current <64,64,64,4,PRO,XB,4>", [](const Conv3P& q) { launch_c3<64, 64, 64, 4, false, false, true, 4>(q, 0); }});
                forms.push_back({"current cut to 16 x 16", [](const Conv3P& q) { launch_cut<64, 64, 64, 4, false, false, true, 4>(q, 16); }});
                forms.push_back({"one round, 10 waves", [](const Conv3P& q) { launch_c3<64, 64, 64, 5, false, false, true, 10>(q, 0); }});
                forms.push_back({"one round, 5 waves", [](const Conv3P& q) { launch_c3<64, 64, 64, 5, false, false, true, 5>(q, 0); }});
                forms.push_back({"one round, 10 waves, resident", [](const Conv3P& q) { launch_c3<64, 64, 64, 5, false, false, true, 10, true>(q, 0); }});
            } else {
                forms.push_back({"current <64,64,64,4,plain,4>", [](const Conv3P& q) { launch_c3<64, 64, 64, 4, false, false, false, 4>(q, 0); }});
                forms.push_back({"current cut to 16 x 16", [](const Conv3P& q) { launch_cut<64, 64, 64, 4, false, false, false, 4>(q, 16); }});
                forms.push_back({"one round, 10 waves", [](const Conv3P& q) { launch_c3<64, 64, 64, 5, false, false, false, 10>(q, 0); }});
                forms.push_back({"one round, 5 waves", [](const Conv3P& q) { launch_c3<64, 64, 64, 5, false, false, false, 5>(q, 0); }});
                forms.push_back({"one round, 10 waves, resident", [](const Conv3P& q) { launch_c3<64, 64, 64, 5, false, false, false, 10, true>(q, 0); }});
            }
        } else if (c.res) {
            rows_old = 20; nwg_old = 320;
            forms.push_back({"current <64,128,64,2,RES,4>", [](const Conv3P& q) { launch_c3<64, 128, 64, 2, false, true, false, 4>(q, 0); }});
            forms.push_back({"current cut to 8 x 16 x 2", [](const Conv3P& q) { launch_cut<64, 128, 64, 2, false, true, false, 4>(q, 16); }});
            forms.push_back({"one round <64,128,32,5,RES,5>", [](const Conv3P& q) { launch_c3<64, 128, 32, 5, false, true, false, 5>(q, 0); }});
            forms.push_back({"one round <64,128,32,5,RES,5>, resident", [](const Conv3P& q) { launch_c3<64, 128, 32, 5, false, true, false, 5, true>(q, 0); }});
        } else {
            rows_old = 20; nwg_old = 320;
            if (c.pro2) {
                forms.push_back({"current <128,128,64,2,PRO2,XB,4>", [](const Conv3P& q) { launch_c3<128, 128, 64, 2, true, false, true, 4>(q, 0); }});
                forms.push_back({"current cut to 8 x 16 x 2", [](const Conv3P& q) { launch_cut<128, 128, 64, 2, true, false, true, 4>(q, 16); }});
                forms.push_back({"one round <128,128,32,5,..,5>", [](const Conv3P& q) { launch_c3<128, 128, 32, 5, true, false, true, 5>(q, 0); }});
            } else {
                forms.push_back({"current <128,128,64,2,PRO,XB,4>", [](const Conv3P& q) { launch_c3<128, 128, 64, 2, false, false, true, 4>(q, 0); }});
                forms.push_back({"current cut to 8 x 16 x 2", [](const Conv3P& q) { launch_cut<128, 128, 64, 2, false, false, true, 4>(q, 16); }});
                forms.push_back({"one round <128,128,32,5,..,5>", [](const Conv3P& q) { launch_c3<128, 128, 32, 5, false, false, true, 5>(q, 0); }});
            }
        }
        (void)rows_old;
        printf("%s\n", c.nm);
        std::vector<char> ref;
        for (size_t k = 0; k < forms.size(); ++k) {
            const bool cut = has_cut && k == 1;
            if (!cut) {                                            // bitwise: every output of the full-grid forms, statistics included
                clear(bb); forms[k].second(p); const std::vector<char> h = snap(bb);
                if (k == 0) ref = h;
                else { const bool same = h == ref; bad += !same; printf("   %-40s bitwise %s%s\n", forms[k].first, same ? "equal" : "DIFFERENT: ", same ? "" : diff_part(h, ref, bb.ny)); }
            }
            const float us = time_us([&] { forms[k].second(p); });
            printf("   %-40s %7.2f us\n", forms[k].first, us);
        }
#ifdef DEX_TIMING
        stamps(forms[0].first, forms[0].second, p, nwg_old, bb);
        for (size_t k = has_cut ? 2 : 1; k < forms.size(); ++k) stamps(forms[k].first, forms[k].second, p, nwg_new, bb);
#endif
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { printf("HIP error %s\n", hipGetErrorString(e)); return 2; }
    }
    printf("%s\n", bad ? "MISMATCH" : "all one-round and resident forms bitwise equal to the current ones");
    return bad ? 1 : 0;
}
