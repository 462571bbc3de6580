// The uniform-grid index of a point cloud, shared by the passes that search it: cloud.hip (fixed-radius neighbourhoods,
// k nearest) and icp.hip (the nearest target point of a moved source point).  The workspace layout, the cell of a point,
// the six launches that build the index and the key that orders candidates live here; what a pass does with the index -
// its walk over the 27 cells around a query included - stays in its own file.  The key table and the counts -> starts sequence: table_dev.h.
// DESIGN.md sections 7o and 7p describe the index; cloud.hip has the proof that 27 cells suffice.
//
// ws: int32 [16] header | tile int32 [ceil((S + 1) / 256)] | start int32 [S + 1] | keys uint64 [S] | slot uint32 [M] |
// rank int32 [M] | sslot uint32 [M] | sorted 16 bytes [M]; S = the power of two >= max(1024, 2 M).
//
// A file that includes this is compiled with -ffp-contract=off: the cell quotient and d2 are rounded per operation.
#pragma once
#include "table_dev.h"
#pragma clang fp contract(off)

namespace {

constexpr int kIndexLaunches = 6;
constexpr int kClHdrWords = 16;
constexpr int kOutOfRange = 0, kInCells = 1, kKept = 2;
constexpr int64_t kMaxM = 1ll << 30;                  // S <= 2^31: slots fit uint32, list positions int32
constexpr double kCellLim = 1048576.0;                // 2^20: 21 bits per axis after the offset (kCellBias)

struct ClWs {
    int64_t S, ntile;
    int64_t tile, start, keys, slot, rank, sslot, sorted, bytes;                // byte offsets into ws
};

inline bool cl_layout(int64_t M, ClWs &m) {
    if (M < 0 || M > kMaxM) return false;
    m.S = table_slots(2 * M);                            // at most M cells
    m.ntile = (m.S + 1 + kThreads - 1) / kThreads;
    m.tile = kClHdrWords * 4;
    m.start = m.tile + pad16(4 * m.ntile);
    m.keys = m.start + pad16(4 * (m.S + 1));             // the fill: [0, keys) 0 and [keys, slot) ff
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
                bool claimed;
                mine = key_claim(keys, S, cell_key(bx, by, bz), claimed);
                if (mine != kNoSlot) r = atomicAdd(cnt + mine, 1);
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

inline bool radius_ok(float radius) { return radius > 0.f && radius < INFINITY; }                    // NaN fails
inline double cell_edge(float radius) { return (double)radius * (1.0 + 0x1p-10); }

// The six launches that build the index: the same for the counting query, the k-NN query and the registration.
// count / moments: where a point without a cell gets its zeros, or NULL.
inline void launch_index(hipStream_t st, const float *points, int64_t M, float radius, void *ws, const ClWs &m, int32_t *count,
                         int64_t *moments) {
    const ClPtr p = cl_ptr(ws, m);
    const dim3 block(kThreads);
    launch_fill(st, ws, m.keys / 16, m.slot / 16, 0, -1);
    // M = 0: no thread has a row.  The launches are kept so that their number is fixed.
    hipLaunchKernelGGL(k_cl_insert, grid_of(M), block, 0, st, points, M, cell_edge(radius), p.keys, p.start, m.S, p.slot, p.rank,
                       count, moments, p.hdr);
    launch_row_starts(st, p.start, m.S + 1, p.tile, m.ntile, p.hdr + kInCells);   // cell s is [start[s], start[s + 1])
    hipLaunchKernelGGL(k_cl_fill, grid_of(M), block, 0, st, points, M, p.slot, p.rank, p.start, m.S, p.sorted, p.sslot);
}

}  // namespace
