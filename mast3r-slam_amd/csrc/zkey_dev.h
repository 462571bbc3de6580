// The z-buffer of 64-bit keys (bits of the camera depth << 32 | index) that the point renderer (render.hip) and the
// triangle rasteriser (raster.hip) share: the empty key, the clear kernel and the commuting minimum.
#pragma once
#include "common.h"

namespace {

constexpr unsigned long long kNoKey = ~0ull;  // no source: a depth with these bits is a NaN and never a candidate
constexpr int kKeyThreads = 256;

// Key buffer to all ones, 16-byte stores.
__global__ void __launch_bounds__(kKeyThreads) k_render_clear(unsigned long long *__restrict__ keys, int64_t P) {
    const int64_t i = ((int64_t)blockIdx.x * kKeyThreads + threadIdx.x) * 2;
    if (i + 2 <= P) *(ulonglong2 *)(keys + i) = ulonglong2{kNoKey, kNoKey};
    else if (i < P) keys[i] = kNoKey;
}

inline void launch_key_clear(unsigned long long *keys, int64_t P, hipStream_t st) {
    hipLaunchKernelGGL(k_render_clear, dim3(m3_cdiv(P, 2 * kKeyThreads)), dim3(kKeyThreads), 0, st, keys, P);
}

// A plain load of the current key, and the atomic minimum only when the new key is smaller (keys only ever decrease,
// so a stale value read here costs an atomic and never a result).
__device__ __forceinline__ void key_min(unsigned long long *slot, unsigned long long key) {
    if (key < __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        __hip_atomic_fetch_min(slot, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace
