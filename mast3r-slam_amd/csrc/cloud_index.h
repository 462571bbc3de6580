// The uniform-grid index of a point cloud, shared by the passes that search it: cloud.hip (fixed-radius neighbourhoods,
// k nearest) and icp.hip (the nearest target point of a moved source point).  The workspace layout, the cell of a point,
// the six launches that build the index and the key that orders candidates live here; what a pass does with the index
// stays in its own file.  DESIGN.md sections 7o and 7p describe the index; cloud.hip has the proof that 27 cells suffice.
//
// ws: int32 [16] header | tile int32 [ceil((S + 1) / 256)] | start int32 [S + 1] | keys uint64 [S] | slot uint32 [M] |
// rank int32 [M] | sslot uint32 [M] | sorted 16 bytes [M]; S = the power of two >= max(1024, 2 M).
//
// A file that includes this is compiled with -ffp-contract=off: the cell quotient and d2 are rounded per operation.
#pragma once
#include "common.h"
#include "compact_dev.h"
#pragma clang fp contract(off)

namespace {

constexpr int kIndexLaunches = 6;
constexpr int kClHdrWords = 16;
constexpr int kOutOfRange = 0, kInCells = 1, kKept = 2;
constexpr int64_t kMaxM = 1ll << 30;                  // S <= 2^31: slots fit uint32, list positions int32
constexpr unsigned long long kEmptyKey = ~0ull;       // a packed cell key uses 63 bits
constexpr uint32_t kNoSlot = ~0u;
constexpr double kCellLim = 1048576.0;                // 2^20: 21 bits per axis after the offset
constexpr int kCellBias = 1 << 20, kCellMask = (1 << 21) - 1;

struct ClWs {
    int64_t S, ntile;
    int64_t tile, start, keys, slot, rank, sslot, sorted, bytes;                // byte offsets into ws
};

inline int64_t pad16(int64_t b) { return (b + 15) / 16 * 16; }

inline bool cl_layout(int64_t M, ClWs &m) {
    if (M < 0 || M > kMaxM) return false;
    m.S = 1024;
    while (m.S < 2 * M) m.S *= 2;                        // at most M cells: never more than half full
    m.ntile = (m.S + 1 + kThreads - 1) / kThreads;
    m.tile = kClHdrWords * 4;
    m.start = m.tile + pad16(4 * m.ntile);
    m.keys = m.start + pad16(4 * (m.S + 1));             // the clear kernel fills [0, keys) with 0 and [keys, slot) with ff
    m.slot = m.keys + 8 * m.S;
    m.rank = m.slot + pad16(4 * M);
    m.sslot = m.rank + pad16(4 * M);
    m.sorted = m.sslot + pad16(4 * M);
    m.bytes = m.sorted + 16 * M;
    return true;
}

struct alignas(16) Ent {                      // an entry of the cell-sorted list
    float x, y, z;
    int32_t i;                                // the point's row
};

struct ClPtr {
    int32_t *hdr, *tile, *start, *rank;
    unsigned long long *keys;
    uint32_t *slot, *sslot;
    Ent *sorted;
};

inline ClPtr cl_ptr(void *ws, const ClWs &m) {
    char *p = (char *)ws;
    ClPtr q;
    q.hdr = (int32_t *)p;
    q.tile = (int32_t *)(p + m.tile);
    q.start = (int32_t *)(p + m.start);
    q.keys = (unsigned long long *)(p + m.keys);
    q.slot = (uint32_t *)(p + m.slot);
    q.rank = (int32_t *)(p + m.rank);
    q.sslot = (uint32_t *)(p + m.sslot);
    q.sorted = (Ent *)(p + m.sorted);
    return q;
}

inline dim3 grid_of(int64_t rows) { return dim3((unsigned)(rows ? (rows + kThreads - 1) / kThreads : 1)); }

__device__ __forceinline__ int64_t row_of() { return (int64_t)blockIdx.x * kThreads + threadIdx.x; }

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// Biased cell coordinates, each in [1, 2^21 - 1], packed as k_voxel_insert packs its voxels.
__device__ __forceinline__ unsigned long long cell_key(int bx, int by, int bz) {
    return ((unsigned long long)bx << 42) | ((unsigned long long)by << 21) | (unsigned long long)bz;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// Biased cell coordinates of a finite point or query; false when one of them reaches +-2^20: out of range.
__device__ __forceinline__ bool cell_of(float x, float y, float z, double h, int &bx, int &by, int &bz) {
    const double cx = floor((double)x / h), cy = floor((double)y / h), cz = floor((double)z / h);
    if (!(fabs(cx) < kCellLim && fabs(cy) < kCellLim && fabs(cz) < kCellLim)) return false;
    bx = (int)cx + kCellBias;
    by = (int)cy + kCellBias;
    bz = (int)cz + kCellBias;
    return true;
}

// Header, tiles, cell counts and keys are cleared by a kernel, 16 bytes per thread: a captured memset left its words
// uncleared on replay.  int4 [0, a) = 0, [a, n) = ff ..
__global__ void __launch_bounds__(kThreads) k_cl_clear(int4 *__restrict__ ws, int64_t a, int64_t n) {
    const int64_t i = row_of();
    if (i >= n) return;
    const int w = i < a ? 0 : -1;
    ws[i] = int4{w, w, w, w};
}

// One point per thread: claim or find the slot of its cell and take the next rank in it.  A point that is not finite
// or out of range gets no slot and its outputs - zeros - here, since the query pass never sees it.
__global__ void __launch_bounds__(kThreads) k_cl_insert(const float *__restrict__ points, int64_t M, double h,
                                                         unsigned long long *__restrict__ keys, int32_t *__restrict__ cnt,
                                                         int64_t S, uint32_t *__restrict__ slot, int32_t *__restrict__ rank,
                                                         int32_t *__restrict__ count, int64_t *__restrict__ moments,
                                                         int32_t *__restrict__ hdr) {
    const int64_t i = row_of();
    bool far = false;
    if (i < M) {
        const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
        uint32_t mine = kNoSlot;
        int32_t r = 0;
        if (finite3(x, y, z)) {
            int bx, by, bz;
            far = !cell_of(x, y, z, h, bx, by, bz);
            if (!far) {
                const unsigned long long key = cell_key(bx, by, bz);
                const unsigned long long mask = (unsigned long long)(S - 1);
                unsigned long long s = mix64(key) & mask;
                for (int64_t probe = 0; probe < S; ++probe) {                   // the table is at most half full: this ends
                    unsigned long long cur = __hip_atomic_load(keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (cur == kEmptyKey) {
                        cur = atomicCAS(keys + s, kEmptyKey, key);
                        if (cur == kEmptyKey) cur = key;
                    }
                    if (cur == key) {
                        mine = (uint32_t)s;
                        r = atomicAdd(cnt + s, 1);
                        break;
                    }
                    s = (s + 1) & mask;
                }
            }
        }
        slot[i] = mine;
        rank[i] = r;
        if (mine == kNoSlot) {
            if (count) count[i] = 0;                                            // NULL: the index alone is built (k-NN)
            if (moments) {
#pragma unroll
                for (int k = 0; k < 9; ++k) moments[9 * i + k] = 0;
            }
        }
    }
    const unsigned long long b = __ballot(far);
    if (b && (threadIdx.x & 63) == 0) atomicAdd(hdr + kOutOfRange, (int)__popcll(b));      // M <= 2^30: no overflow
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

// The cell counts of a tile of 256 slots, added up.  cnt has n = S + 1 entries; the last is 0 and becomes the total.
__global__ void __launch_bounds__(kThreads) k_cl_tile_counts(const int32_t *__restrict__ cnt, int64_t n,
                                                              int32_t *__restrict__ tile) {
    const int64_t i = row_of();
    int total;
    block_exclusive(i < n ? cnt[i] : 0, total);
    if (threadIdx.x == 0) tile[blockIdx.x] = total;
}

// Counts to cell starts, in place: the tile's offset + the rank inside the tile.  Cell s is [start[s], start[s + 1]).
__global__ void __launch_bounds__(kThreads) k_cl_starts(int32_t *__restrict__ cnt, int64_t n, const int32_t *__restrict__ tile) {
    const int64_t i = row_of();
    int total;
    const int start = tile[blockIdx.x] + block_exclusive(i < n ? cnt[i] : 0, total);
    if (i < n) cnt[i] = start;
}

// One point per thread again: its entry goes to its cell's start + its rank.
__global__ void __launch_bounds__(kThreads) k_cl_fill(const float *__restrict__ points, int64_t M,
                                                       const uint32_t *__restrict__ slot, const int32_t *__restrict__ rank,
                                                       const int32_t *__restrict__ start, int64_t S, Ent *__restrict__ sorted,
                                                       uint32_t *__restrict__ sslot) {
    const int64_t i = row_of();
    if (i >= M) return;
    const uint32_t s = slot[i];
    if (s == kNoSlot || (int64_t)s >= S) return;
    const int64_t at = (int64_t)start[s] + rank[i];
    if (at < 0 || at >= M) return;                                              // never, for a ws from the same points
    sorted[at] = Ent{points[3 * i], points[3 * i + 1], points[3 * i + 2], (int32_t)i};
    sslot[at] = s;
}

// The key that orders the candidates of a query: squared distance to 22 mantissa bits, then the row.
constexpr unsigned long long kRowMask = (1ull << 30) - 1;                       // the low 30 bits of a key: the row

__device__ __forceinline__ unsigned long long knn_key(double d2, int32_t j) {
    return ((unsigned long long)__double_as_longlong(d2) & ~kRowMask) | ((unsigned long long)(uint32_t)j & kRowMask);
}

inline bool ws_ok(const void *ws) { return ws && ((uintptr_t)ws & 15) == 0; }
inline bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool radius_ok(float radius) { return radius > 0.f && radius < INFINITY; }                    // NaN fails
inline double cell_edge(float radius) { return (double)radius * (1.0 + 0x1p-10); }

// The six launches that build the index: the same for the counting query, the k-NN query and the registration.
// count / moments: where a point without a cell gets its zeros, or NULL.
inline void launch_index(hipStream_t st, const float *points, int64_t M, float radius, void *ws, const ClWs &m, int32_t *count,
                         int64_t *moments) {
    const ClPtr p = cl_ptr(ws, m);
    const dim3 block(kThreads);
    const dim3 tiles((unsigned)m.ntile);
    hipLaunchKernelGGL(k_cl_clear, grid_of(m.slot / 16), block, 0, st, (int4 *)ws, m.keys / 16, m.slot / 16);
    // M = 0: no thread has a row.  The launches are kept so that their number is fixed.
    hipLaunchKernelGGL(k_cl_insert, grid_of(M), block, 0, st, points, M, cell_edge(radius), p.keys, p.start, m.S, p.slot, p.rank,
                       count, moments, p.hdr);
    hipLaunchKernelGGL(k_cl_tile_counts, tiles, block, 0, st, p.start, m.S + 1, p.tile);
    launch_scan(st, p.hdr + kInCells, ScanJob{p.tile, m.ntile});
    hipLaunchKernelGGL(k_cl_starts, tiles, block, 0, st, p.start, m.S + 1, p.tile);
    hipLaunchKernelGGL(k_cl_fill, grid_of(M), block, 0, st, points, M, p.slot, p.rank, p.start, m.S, p.sorted, p.sslot);
}

}  // namespace
