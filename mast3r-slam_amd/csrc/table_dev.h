// What the mesh and cloud passes share (mesh_components, mesh_normals, mesh_simplify, mesh_smooth, cloud_index and the
// voxel stage of map_export): the workspace checks, the one meaning of a grid, the fill kernels,
// the uint64 key table, the face loader and the counts -> row starts sequence.  Integer code only - the files that
// include this are compiled with different floating-point contraction, and nothing here depends on it.
//
// The key table: S slots, a power of two, kEmptyKey when free; a key lives at the first free slot at or after
// mix64(key) & (S - 1), going round.  The callers size it so that it is never more than half full (table_slots), so a
// probe ends.  Claiming is a compare-and-swap on the empty value and nobody waits; which slot a key lands in depends on
// the arrival order, and nothing that is output may read it.
#pragma once
#include "common.h"
#include "compact_dev.h"     // kThreads, launch_scan

namespace {

constexpr unsigned long long kEmptyKey = ~0ull;      // a packed cell or edge key uses 63 bits at most
constexpr uint32_t kNoSlot = ~0u;                     // no slot: S <= 2^31
constexpr int kCellBias = 1 << 20, kCellMask = (1 << 21) - 1;     // 21 bits per axis after the offset

// ---- host -------------------------------------------------------------------------------------------------------------
inline int64_t pad16(int64_t b) { return (b + 15) / 16 * 16; }
inline bool ws_ok(const void *ws) { return ws && ((uintptr_t)ws & 15) == 0; }
inline bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// The power of two >= max(floor, n).  n = twice the keys at most: never more than half full.
inline int64_t table_slots(int64_t n, int64_t floor = 1024) {
    int64_t s = floor;
    while (s < n) s *= 2;
    return s;
}

// Rows to workgroups of kThreads, at least one: the one workgroup of an empty pass does the work of its thread 0.
inline dim3 grid_of(int64_t rows) { return dim3((unsigned)(rows > 0 ? (rows + kThreads - 1) / kThreads : 1)); }

// ---- device -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t row_of() { return (int64_t)blockIdx.x * kThreads + threadIdx.x; }

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// Biased cell coordinates, each in [1, 2^21 - 1], as one key, and back.
__device__ __forceinline__ unsigned long long cell_key(int bx, int by, int bz) {
    return ((unsigned long long)bx << 42) | ((unsigned long long)by << 21) | (unsigned long long)bz;
}

__device__ __forceinline__ void cell_unkey(unsigned long long key, int &bx, int &by, int &bz) {
    bx = (int)(key >> 42) & kCellMask, by = (int)(key >> 21) & kCellMask, bz = (int)key & kCellMask;
}

// Tables and headers are set by a kernel, 16 bytes per thread: a captured memset left its words uncleared on replay
// (DESIGN.md section 7l).  int4 [0, a) = w0 .., [a, n) = w1 ..
__global__ void __launch_bounds__(kThreads) k_fill2(int4 *__restrict__ p, int64_t a, int64_t n, int w0, int w1) {
    const int64_t i = row_of();
    if (i >= n) return;
    const int w = i < a ? w0 : w1;
    p[i] = int4{w, w, w, w};
}

// int4 [0, a) = w0 .., [a, b) = w1 .., [b, n) = w2 ..; and head_n int4 of 0 at head, a block that does not adjoin p
// (head_n <= n; 0: none).
__global__ void __launch_bounds__(kThreads) k_fill3(int4 *__restrict__ p, int64_t a, int64_t b, int64_t n, int w0, int w1, int w2,
                                                     int4 *__restrict__ head, int head_n) {
    const int64_t i = row_of();
    if (i < head_n) head[i] = int4{0, 0, 0, 0};
    if (i >= n) return;
    const int w = i < a ? w0 : i < b ? w1 : w2;
    p[i] = int4{w, w, w, w};
}

inline void launch_fill(hipStream_t st, void *p, int64_t a, int64_t n, int w0, int w1) {
    hipLaunchKernelGGL(k_fill2, grid_of(n), dim3(kThreads), 0, st, (int4 *)p, a, n, w0, w1);
}

// The slot of key, claimed when no thread had it: claimed is true for the one thread whose compare-and-swap installed
// the key.  kNoSlot: every slot holds another key - never, in a table that is at most half full.
__device__ __forceinline__ uint32_t key_claim(unsigned long long *__restrict__ keys, int64_t S, unsigned long long key,
                                              bool &claimed) {
    const unsigned long long mask = (unsigned long long)(S - 1);
    unsigned long long s = mix64(key) & mask;
    uint32_t at = kNoSlot;
    claimed = false;
    for (int64_t probe = 0; probe < S; ++probe) {
        unsigned long long cur = __hip_atomic_load(keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kEmptyKey) {
            cur = atomicCAS(keys + s, kEmptyKey, key);
            claimed = cur == kEmptyKey;
        }
        if (claimed || cur == key) {
            at = (uint32_t)s;
            break;
        }
        s = (s + 1) & mask;
    }
    return at;
}

__device__ __forceinline__ unsigned long long key_home(unsigned long long key, int64_t S) {
    return mix64(key) & (unsigned long long)(S - 1);
}

// The slot of key in a table that no longer changes, or kNoSlot.  from: the first slot to look at - key_home(key, S),
// or a slot already known to hold the key.
__device__ __forceinline__ uint32_t key_find(const unsigned long long *__restrict__ keys, int64_t S, unsigned long long key,
                                             unsigned long long from) {
    const unsigned long long mask = (unsigned long long)(S - 1);
    unsigned long long s = from;
    uint32_t at = kNoSlot;
    for (int64_t probe = 0; probe < S; ++probe) {
        const unsigned long long cur = keys[s];
        if (cur == key) {
            at = (uint32_t)s;
            break;
        }
        if (cur == kEmptyKey) break;
        s = (s + 1) & mask;
    }
    return at;
}

// The rows of face f; true when all three are in [0, V): nothing may be indexed with them otherwise.
__device__ __forceinline__ bool load_face(const int32_t *__restrict__ faces, int64_t f, int64_t V, int32_t (&r)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i] = faces[3 * f + i];
    return r[0] >= 0 && r[0] < V && r[1] >= 0 && r[1] < V && r[2] >= 0 && r[2] < V;
}

// Faces that exist (in) and are not valid (ok), counted with one ballot and one atomic per wave.  F < 2^31: no overflow.
__device__ __forceinline__ void count_invalid(bool in, bool ok, int32_t *__restrict__ hdr_word) {
    const unsigned long long bad = __ballot(in && !ok);
    if (bad && (threadIdx.x & 63) == 0) atomicAdd(hdr_word, (int)__popcll(bad));
}

// Exclusive prefix of x over the workgroup in thread order, and the workgroup's total.
__device__ __forceinline__ int block_exclusive(int x, int &total) {
    __shared__ int wtot[kThreads / M3_WAVE];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int incl = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wtot[w] = incl;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < kThreads / M3_WAVE; ++i) {
        base += i < w ? wtot[i] : 0;
        total += wtot[i];
    }
    return base + incl - x;
}

// The counts of a tile of 256 rows, added up.  cnt has n entries; the last is 0 and becomes the total.
__global__ void __launch_bounds__(kThreads) k_tile_sums(const int32_t *__restrict__ cnt, int64_t n, int32_t *__restrict__ tile) {
    const int64_t i = row_of();
    int total;
    block_exclusive(i < n ? cnt[i] : 0, total);
    if (threadIdx.x == 0) tile[blockIdx.x] = total;
}

// Counts to row starts, in place: the tile's offset + the rank inside the tile.  Row i is [cnt[i], cnt[i + 1]).
__global__ void __launch_bounds__(kThreads) k_row_starts(int32_t *__restrict__ cnt, int64_t n, const int32_t *__restrict__ tile) {
    const int64_t i = row_of();
    int total;
    const int start = tile[blockIdx.x] + block_exclusive(i < n ? cnt[i] : 0, total);
    if (i < n) cnt[i] = start;
}

// Three launches: sums per tile, the scan of the ntile = grid_of(n) tiles (its total to *total_word), starts in place.
inline void launch_row_starts(hipStream_t st, int32_t *counts, int64_t n, int32_t *tile, int64_t ntile, int32_t *total_word) {
    const dim3 tiles((unsigned)ntile), block(kThreads);
    hipLaunchKernelGGL(k_tile_sums, tiles, block, 0, st, counts, n, tile);
    launch_scan(st, total_word, ScanJob{tile, ntile});
    hipLaunchKernelGGL(k_row_starts, tiles, block, 0, st, counts, n, tile);
}

}  // namespace
