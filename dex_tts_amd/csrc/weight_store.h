// weight_store.h — the weight plumbing every context of the C ABI shares (DexCtx, DexText, DexStyle, DexVoc derive from WeightStore):
// the inventory of reference state-dict keys and shapes, the raw fp32 copies the caller uploads under those keys, the device buffers
// finalize packs from them, the handle that carries a packed weight's 16-bit twins (PackedW), and the context's last error.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../include/dex_amd.h"
#include "kernels.h"

// a failed HIP call returns DEX_ERR_HIP from the enclosing function, with the call, the runtime's message and the place in obj's error
#define DEX_HIPCHK(obj, call)                                                                          \
    do { hipError_t e_ = (call); if (e_ != hipSuccess)                                                 \
        return (obj)->fail(DEX_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

namespace dex {

// A packed weight as the launch code holds it.  The reduced-precision modes read 16-bit twins of the fp32 pack, one set per mode: [0] bf16,
// [1] fp16, [2] fp16 hi + lo (the split-weight mode: fp16 of the weight, and in the same layout fp16 of what that rounding lost).  All sets
// are packed at finalize - the precision mode may change afterwards - and the context picks the index in ONE place (lpi()).  A twin that
// was not packed is a null view: the forms that need it test the handle.  Matrices packed together as a group (the Upsample's parity
// matrices, the grouped pos-conv) are one handle each, in order; handle 0 also serves a kernel that walks the whole group by stride.
struct LpView { const void* p = nullptr; long lo_off = 0; };      // 16-bit operand; lo_off: elements from a hi element to its lo element (0: no lo pack)
struct PackedW {
    PackedW(const float* f = nullptr) : f32(f) {}      // (an fp32-only operand, e.g. one built at run time, is a handle without twins)
    const float* f32;                 // the fp32 pack ([K][N]) every mode can read
    LpView nk[3], frag[3];            // [N][K] twin / MFMA-fragment-order twin per set
    explicit operator bool() const { return f32 != nullptr; }
};

struct RawW { float* p = nullptr; std::vector<int64_t> shape; long numel = 0; bool loaded = false; };

struct WeightStore {
    // noun: how error messages name this context's weights ("" for the score network, "text-encoder ", "style ", "vocoder ")
    explicit WeightStore(const char* noun) : noun(noun) {}
    const char* noun;
    std::string err;
    std::vector<std::string> keys;              // inventory, in registration order
    std::map<std::string, RawW> raw;
    std::vector<void*> owned;                   // hipMalloc'ed packs of the last finalize
    bool finalized = false;
    int alloc_rc = DEX_OK;                      // DEX_ERR_HIP once an alloc of the current finalize has failed

    int fail(int code, const char* fmt, ...) {
        char buf[512];
        va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
        err = buf;
        return code;
    }
    void add(const std::string& k, std::vector<int64_t> shape) {
        keys.push_back(k);
        RawW r; r.shape = std::move(shape); r.numel = 1;
        for (auto d : r.shape) r.numel *= d;
        raw[k] = r;
    }
    const float* R(const std::string& k) const { return raw.at(k).p; }
    int info(int i, const char** key, int64_t shape[4], int* ndim) const {
        if (i < 0 || i >= (int)keys.size()) return DEX_ERR_ARG;
        const RawW& r = raw.at(keys[i]);
        if (key) *key = keys[i].c_str();
        if (ndim) *ndim = (int)r.shape.size();
        if (shape) for (size_t k = 0; k < r.shape.size(); ++k) shape[k] = r.shape[k];
        return DEX_OK;
    }
    // copy the caller's device tensor into the raw weight `key`: stream-ordered on `st`, or (sync) finished before returning
    int load(const char* key, const float* w_dev, const int64_t* shape, int ndim, hipStream_t st, bool sync) {
        if (!key || !w_dev) return DEX_ERR_ARG;
        auto it = raw.find(key);
        if (it == raw.end()) return fail(DEX_ERR_ARG, "unknown %sweight key '%s'", noun, key);
        RawW& r = it->second;
        if ((int)r.shape.size() != ndim) return fail(DEX_ERR_ARG, "weight '%s': expected %d dims, got %d", key, (int)r.shape.size(), ndim);
        for (int k = 0; k < ndim; ++k)
            if (r.shape[k] != shape[k]) return fail(DEX_ERR_ARG, "weight '%s': dim %d is %lld, expected %lld", key, k, (long long)shape[k], (long long)r.shape[k]);
        if (!r.p) DEX_HIPCHK(this, hipMalloc((void**)&r.p, r.numel * sizeof(float)));
        if (sync) {
            DEX_HIPCHK(this, hipMemcpy(r.p, w_dev, r.numel * sizeof(float), hipMemcpyDeviceToDevice));
            DEX_HIPCHK(this, hipStreamSynchronize(nullptr));       // a device-to-device hipMemcpy may return before it has run
        } else {
            DEX_HIPCHK(this, hipMemcpyAsync(r.p, w_dev, r.numel * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
        r.loaded = true;
        finalized = false;
        return DEX_OK;
    }
    // the opening of every *_finalize: every key loaded, the previous packs freed
    int begin_finalize() {
        for (const auto& k : keys)
            if (!raw.at(k).loaded) return fail(DEX_ERR_STATE, "%sweight '%s' was never loaded", noun, k.c_str());
        for (void* p : owned) hipFree(p);
        owned.clear();
        alloc_rc = DEX_OK;
        return DEX_OK;
    }
    // n floats owned by the context until the next finalize; null (and alloc_rc set) if hipMalloc fails
    float* alloc(long n) {
        float* p = nullptr;
        if (hipMalloc((void**)&p, n * sizeof(float)) != hipSuccess) { alloc_rc = fail(DEX_ERR_HIP, "hipMalloc of %ld floats failed", n); return nullptr; }
        owned.push_back(p);
        return p;
    }
    void release() {
        for (auto& kv : raw) if (kv.second.p) hipFree(kv.second.p);
        for (void* p : owned) hipFree(p);
    }
};

// Conv1d weight [cout][cin][k] -> implicit-GEMM operand [(tap*cin_pad + ci)][cout], zero rows for padded input channels
inline float* conv1d_operand(WeightStore& s, const float* src, int cin, int cout, int k, int cin_pad, hipStream_t st) {
    float* t = s.alloc((long)k * cin * cout);
    if (t) launch_permute4(src, t, cout, cin, k, 1, 2, 1, 0, 3, st);
    if (cin_pad == cin) return t;
    float* d = s.alloc((long)k * cin_pad * cout);
    if (t && d) {
        hipMemsetAsync(d, 0, (size_t)k * cin_pad * cout * sizeof(float), st);
        hipMemcpy2DAsync(d, (size_t)cin_pad * cout * 4, t, (size_t)cin * cout * 4, (size_t)cin * cout * 4, k, hipMemcpyDeviceToDevice, st);
    }
    return d;
}

struct PackedConv { const float* w = nullptr; const float* b = nullptr; int cin, cout, k; };      // packed [k*cin][cout], bias or null

inline PackedConv pack_conv1d(WeightStore& s, const std::string& wkey, const char* bkey, int cin, int cout, int k, int cin_pad, hipStream_t st) {
    PackedConv o{}; o.cin = cin_pad; o.cout = cout; o.k = k;
    o.w = conv1d_operand(s, s.R(wkey), cin, cout, k, cin_pad, st);
    o.b = bkey ? s.R(bkey) : nullptr;
    return o;
}

}  // namespace dex
