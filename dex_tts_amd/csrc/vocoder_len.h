// vocoder_len.h — the per-utterance end of a layer in a ragged vocoder batch (dex_vocode_ragged; kernels.h).
#pragma once
#include <hip/hip_runtime.h>

namespace dex {

// Valid samples of utterance b in a layer of L = T R samples: len[b] mel frames, clamped to [0, T], times the layer's rate R.
// No lengths: the whole layer.
__device__ __forceinline__ int voc_valid_len(const int* len, int b, int R, int L) {
    return len ? min(max(len[b], 0), L / R) * R : L;
}

}  // namespace dex
