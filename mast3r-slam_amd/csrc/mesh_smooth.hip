// Edge topology of a triangle mesh and Laplacian / Taubin smoothing on it (mast3r_slam/smooth.py).
// The rule is stated once, in include/m3slam.h; tests/smooth_twin.py restates it in numpy.
//
// build:  clear -> one thread per face (claim the slot of each of its three pairs, add to the slot's face count; the
//         claimer adds to the degrees of both ends) -> degrees per tile of 256 rows -> scan of the tiles -> row starts =
//         tile offset + rank -> one thread per face again (the corners that claimed a slot write each end into the
//         other's row at a cursor, with the boundary bit; the header counts) -> sort every row and set its vertex's
//         boundary flag.
// Seven launches whatever the mesh holds.  The edges live in the key table of table_dev.h, which also has the fill and the
// degrees -> row starts sequence.  The only atomics are integer ones whose results commute: the table's claim, add for
// the counts, the degrees and the cursors.  Where in its row a neighbour first lands depends on the arrival order; the
// sort removes that.  No thread waits for another.
//
// The cursor of a row is its start itself: the degrees are counted into off[1 + v], the scan turns them into row
// starts, and the fill's atomicAdd on off[1 + v] hands out the positions and leaves the row's END there - the start of
// row v + 1.  With off[0] = 0 the same array is then the CSR's off [V + 1], and no second array or load is needed.
// The fill runs in face order, not in slot order: the face pass leaves, per corner, the slot it claimed (or none), so
// that the cursors and rows touched by neighbouring threads are those of neighbouring vertices and not hash-random.
//
// Rows are filled into `raw` and sorted into `nbr`, out of place, by rank: the neighbours of a row are distinct (a slot
// per unique edge), so the rank of an entry is the number of smaller ones.  Bit 31 of a raw entry says that its edge is
// a boundary edge; the sort strips it and ors it into the row's flag, so the flags need neither atomics nor a clear.  A
// thread sorts a row of up to kShortRow entries; the lanes of a wave then sort its longer rows together, one row after
// the other, 64 entries against 64 entries held in registers.
//
// edges:  neighbours > v per tile of 256 rows -> scan -> scatter at tile offset + rank (lexicographic (lo, hi) order),
//         faces_of looked up in the table.  Three launches, only when asked for.
// pass:   one launch per pass, one thread per vertex (the hot path).  Between passes the positions live in ws as
//         16 bytes per vertex - x, y, z and a word of flags (finite, pinned) - so a neighbour is one 16-byte load.  The
//         first pass reads the caller's [V,3] array and the last writes the caller's [V,3] output.
//
// ws: int32 [16] header | tile int32 [ceil((V + 1) / 256)] | off int32 [V + 2] | cnt int32 [S] | keys uint64 [S] |
// bnd uint8 [V] | fslot uint32 [3 F] | raw int32 [6 F] | nbr int32 [6 F] | two position buffers of 16 bytes [V]; S = the power of two >=
// max(1024, 6 F).  Header words: [0] 2 E (the total of the degree scan), [1] boundary edges, [2] non-manifold edges,
// [3] invalid faces, [8] E (the total of the edge-list scan); the others are 0.
//
// Compiled with -ffp-contract=off: every float64 operation of the rule is rounded on its own.
#include "table_dev.h"
#pragma clang fp contract(off)

namespace {

constexpr int kBuildLaunches = 7;
constexpr int kSmHdrWords = 16;
constexpr int kTwoE = 0, kBoundary = 1, kNonManifold = 2, kInvalid = 3, kEdges = 8;
constexpr int64_t kMaxV = 0x7fffffff;
constexpr int64_t kMaxF = 0x7fffffff / 6;     // the CSR holds at most 6 F entries, indexed in int32
constexpr int kShortRow = 32;                 // rows up to this length are sorted by their own thread
constexpr int32_t kRowMask = 0x7fffffff;      // a raw entry: the neighbour, and bit 31 = on a boundary edge
constexpr unsigned kFinite = 1u, kPinned = 2u;

struct SmWs {
    int64_t ntile, S, cap;                                                               // cap = 6 F: entries of raw and nbr
    int64_t tile, off, cnt, keys, bnd, fslot, raw, nbr, posA, posB, bytes;                     // byte offsets into ws
};

inline bool sm_layout(int64_t V, int64_t F, SmWs &m) {
    if (V < 0 || F < 0 || V > kMaxV || F > kMaxF) return false;
    m.ntile = (V + 1 + kThreads - 1) / kThreads;         // tiles of the V + 1 row starts: at least one
    m.cap = 6 * F;
    m.S = table_slots(m.cap);                            // 3 F edges at most
    m.tile = kSmHdrWords * 4;
    m.off = m.tile + pad16(4 * m.ntile);
    m.cnt = m.off + pad16(4 * (V + 2));
    m.keys = m.cnt + 4 * m.S;                            // the fill: [0, keys) 0 and [keys, bnd) ff
    m.bnd = m.keys + 8 * m.S;
    m.fslot = m.bnd + pad16(V);
    m.raw = m.fslot + pad16(12 * F);
    m.nbr = m.raw + pad16(4 * m.cap);
    m.posA = m.nbr + pad16(4 * m.cap);
    m.posB = m.posA + 16 * V;
    m.bytes = m.posB + 16 * V;
    return true;
}

struct alignas(16) Pos {                      // a vertex between two passes
    float x, y, z;
    uint32_t flags;                           // kFinite | kPinned
};

struct SmPtr {
    int32_t *hdr, *tile, *off, *cnt, *raw, *nbr;
    uint8_t *bnd;
    uint32_t *fslot;
    unsigned long long *keys;
    Pos *pos[2];
};

inline SmPtr sm_ptr(void *ws, const SmWs &m) {
    char *p = (char *)ws;
    SmPtr q;
    q.hdr = (int32_t *)p;
    q.tile = (int32_t *)(p + m.tile);
    q.off = (int32_t *)(p + m.off);
    q.cnt = (int32_t *)(p + m.cnt);
    q.keys = (unsigned long long *)(p + m.keys);
    q.bnd = (uint8_t *)(p + m.bnd);
    q.fslot = (uint32_t *)(p + m.fslot);
    q.raw = (int32_t *)(p + m.raw);
    q.nbr = (int32_t *)(p + m.nbr);
    q.pos[0] = (Pos *)(p + m.posA);
    q.pos[1] = (Pos *)(p + m.posB);
    return q;
}

__device__ __forceinline__ unsigned long long edge_key(int32_t a, int32_t b) {
    const int32_t lo = a < b ? a : b, hi = a < b ? b : a;                        // 62 bits
    return ((unsigned long long)(uint32_t)lo << 31) | (unsigned long long)(uint32_t)hi;
}

// One face per thread: each of its three pairs claims or finds the slot of its key and adds 1 to the slot's count; the
// thread whose compare-and-swap claimed the slot, and only that one, adds 1 to the degrees of both ends and leaves the
// slot in fslot for the fill.
__global__ void __launch_bounds__(kThreads) k_sm_faces(const int32_t *__restrict__ faces, int64_t V, int64_t F,
                                                        unsigned long long *__restrict__ keys, int32_t *__restrict__ cnt,
                                                        int64_t S, int32_t *__restrict__ deg, uint32_t *__restrict__ fslot,
                                                        int32_t *__restrict__ hdr) {
    const int64_t f = row_of();
    int32_t r[3] = {0, 0, 0};
    const bool in = f < F, ok = in && load_face(faces, f, V, r);
    count_invalid(in, ok, hdr + kInvalid);
    if (!in) return;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int32_t a = r[i], b = r[i == 2 ? 0 : i + 1];
        fslot[3 * f + i] = kNoSlot;
        if (!ok || a == b) continue;                                            // no edge
        bool claimed;
        const uint32_t s = key_claim(keys, S, edge_key(a, b), claimed);
        if (s == kNoSlot) continue;                                             // never: 3 F pairs, at least 6 F slots
        atomicAdd(cnt + s, 1);
        if (claimed) {
            atomicAdd(deg + a, 1);
            atomicAdd(deg + b, 1);
            fslot[3 * f + i] = s;
        }
    }
}

__device__ __forceinline__ int wave_sum(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// One face per thread again: a corner that claimed its edge's slot writes each end into the other's row, with bit 31
// set when one face corner contributed the edge, and the edge is counted in the header.  cursor[v] starts as the start
// of row v and ends as its end.  A slot in fslot means a face with valid rows.
__global__ void __launch_bounds__(kThreads) k_sm_fill(const int32_t *__restrict__ faces, int64_t V, int64_t F,
                                                       const uint32_t *__restrict__ fslot, const int32_t *__restrict__ cnt,
                                                       int64_t S, int32_t *__restrict__ cursor, int32_t *__restrict__ raw,
                                                       int64_t cap, int32_t *__restrict__ hdr) {
    const int64_t f = row_of();
    int n1 = 0, n3 = 0;
    if (f < F) {
        int32_t r[3];
        uint32_t s[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            r[i] = faces[3 * f + i];
            s[i] = fslot[3 * f + i];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (s[i] == kNoSlot || (int64_t)s[i] >= S) continue;
            const int32_t a = r[i], b = r[i == 2 ? 0 : i + 1];
            if (a < 0 || a >= V || b < 0 || b >= V) continue;                   // never, for the faces the slots came from
            const int32_t c = cnt[s[i]];
            const int64_t at_a = atomicAdd(cursor + a, 1), at_b = atomicAdd(cursor + b, 1);
            const int32_t bit = c == 1 ? ~kRowMask : 0;
            if (at_a >= 0 && at_a < cap) raw[at_a] = b | bit;
            if (at_b >= 0 && at_b < cap) raw[at_b] = a | bit;
            n1 += c == 1 ? 1 : 0;
            n3 += c > 2 ? 1 : 0;
        }
    }
    n1 = wave_sum(n1);
    n3 = wave_sum(n3);
    if ((threadIdx.x & 63) == 0) {
        if (n1) atomicAdd(hdr + kBoundary, n1);                                 // E <= 3 F < 2^31: no overflow
        if (n3) atomicAdd(hdr + kNonManifold, n3);
    }
}

// The row [b, e) of vertex v, clamped to the arrays: a ws from this build never needs the clamp.
__device__ __forceinline__ void row_range(const int32_t *__restrict__ off, int64_t v, int64_t cap, int64_t &b, int64_t &e) {
    b = off[v];
    e = off[v + 1];
    if (b < 0 || e < b || e > cap) b = e = 0;
}

// One row per thread, sorted ascending by rank: nbr[b + rank] = the entry, rank = the entries of the row below it.
// Rows longer than kShortRow are left to the whole wave, one after the other: every lane holds one of 64 entries to
// rank and one of 64 entries to compare against, which go round by readlane.  bnd[v] = some entry had bit 31.
__global__ void __launch_bounds__(kThreads) k_sm_sort(const int32_t *__restrict__ off, int64_t V, int64_t cap,
                                                       const int32_t *__restrict__ raw, int32_t *__restrict__ nbr,
                                                       uint8_t *__restrict__ bnd) {
    const int64_t v = row_of();
    const int lane = threadIdx.x & 63;
    int64_t b = 0, e = 0;
    if (v < V) row_range(off, v, cap, b, e);
    const int d = (int)(e - b);
    bool flag = false;
    if (d <= kShortRow) {
        for (int i = 0; i < d; ++i) {
            const int32_t xr = raw[b + i], x = xr & kRowMask;
            flag = flag || xr < 0;
            int rank = 0;
            for (int j = 0; j < d; ++j) rank += (raw[b + j] & kRowMask) < x ? 1 : 0;
            nbr[b + rank] = x;
        }
    }
    unsigned long long longs = __ballot(d > kShortRow);
    while (longs) {                                                             // wave-uniform
        const int l = __ffsll((long long)longs) - 1;
        longs &= longs - 1;
        const int64_t bl = __shfl(b, l, 64);
        const int dl = __shfl(d, l, 64);
        bool any = false;
        for (int i0 = 0; i0 < dl; i0 += 64) {
            const bool mine = i0 + lane < dl;
            const int32_t xr = mine ? raw[bl + i0 + lane] : 0, x = xr & kRowMask;
            any = any || __ballot(xr < 0) != 0ull;
            int rank = 0;
            for (int j0 = 0; j0 < dl; j0 += 64) {
                const int32_t y = j0 + lane < dl ? raw[bl + j0 + lane] & kRowMask : kRowMask;   // padding is below nothing
#pragma unroll
                for (int t = 0; t < 64; ++t) rank += __builtin_amdgcn_readlane(y, t) < x ? 1 : 0;
            }
            if (mine) nbr[bl + rank] = x;
        }
        if (lane == l) flag = any;
    }
    if (v < V) bnd[v] = flag ? 1 : 0;
}

// degree and boundary of every vertex, for the host.
__global__ void __launch_bounds__(kThreads) k_sm_read(const int32_t *__restrict__ off, const uint8_t *__restrict__ bnd,
                                                       int64_t V, int32_t *__restrict__ degree_out,
                                                       uint8_t *__restrict__ boundary_out) {
    const int64_t v = row_of();
    if (v >= V) return;
    degree_out[v] = off[v + 1] - off[v];
    boundary_out[v] = bnd[v];
}

// The entries of v's sorted row that are above v: the edges whose lower end is v.  first = the index of the first.
__device__ __forceinline__ int upper_part(const int32_t *__restrict__ nbr, int64_t b, int64_t e, int64_t v, int64_t &first) {
    first = e;
    for (int64_t k = b; k < e; ++k) {
        if (nbr[k] > v) { first = k; break; }
    }
    return (int)(e - first);
}

__global__ void __launch_bounds__(kThreads) k_sm_count_edges(const int32_t *__restrict__ off, const int32_t *__restrict__ nbr,
                                                              int64_t V, int64_t cap, int32_t *__restrict__ cntE) {
    const int64_t v = row_of();
    int64_t b = 0, e = 0, first;
    if (v < V) row_range(off, v, cap, b, e);
    int total;
    block_exclusive(upper_part(nbr, b, e, v, first), total);
    if (threadIdx.x == 0) cntE[blockIdx.x] = total;
}

// Edges to rows tile offset + rank: lexicographic (lo, hi) order, since rows are ascending.  faces_of from the table.
__global__ void __launch_bounds__(kThreads) k_sm_scatter_edges(const int32_t *__restrict__ off, const int32_t *__restrict__ nbr,
                                                                int64_t V, int64_t cap, const int32_t *__restrict__ tile,
                                                                const unsigned long long *__restrict__ keys,
                                                                const int32_t *__restrict__ cnt, int64_t S, int64_t E,
                                                                int32_t *__restrict__ edges_out,
                                                                int32_t *__restrict__ edge_faces_out) {
    const int64_t v = row_of();
    int64_t b = 0, e = 0, first;
    if (v < V) row_range(off, v, cap, b, e);
    const int n = upper_part(nbr, b, e, v, first);
    int total;
    int64_t o = (int64_t)tile[blockIdx.x] + block_exclusive(n, total);
    for (int64_t k = first; k < e; ++k, ++o) {
        if (o >= E) return;                                                     // never, for a ws from the same faces
        const int32_t hi = nbr[k];
        const unsigned long long key = edge_key((int32_t)v, hi);
        const uint32_t s = key_find(keys, S, key, key_home(key, S));
        edges_out[2 * o] = (int32_t)v;
        edges_out[2 * o + 1] = hi;
        edge_faces_out[o] = s == kNoSlot ? 0 : cnt[s];
    }
}

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// Vertex j before the pass: from the caller's [V,3] array (the first pass) or from a position buffer.
template <bool PACKED>
__device__ __forceinline__ Pos load_pos(const float *__restrict__ src3, const Pos *__restrict__ src, int64_t j) {
    if (PACKED) return src[j];
    Pos p;
    p.x = src3[3 * j];
    p.y = src3[3 * j + 1];
    p.z = src3[3 * j + 2];
    p.flags = finite3(p.x, p.y, p.z) ? kFinite : 0u;
    return p;
}

// One pass, one vertex per thread.  SRC_PACKED / DST_PACKED: positions as 16-byte Pos, or the caller's float [V,3].
// The neighbours are fetched four at a time - four independent 16-byte loads in flight - and added one after the other
// in ascending order, each float64 add rounded on its own.
template <bool SRC_PACKED, bool DST_PACKED>
__global__ void __launch_bounds__(kThreads) k_sm_pass(const float *__restrict__ src3, const Pos *__restrict__ src,
                                                       int64_t V, int64_t cap, const int32_t *__restrict__ off,
                                                       const int32_t *__restrict__ nbr, const uint8_t *__restrict__ bnd,
                                                       const uint8_t *__restrict__ pinned, int fix_boundary, float w_f,
                                                       float *__restrict__ dst3, Pos *__restrict__ dst) {
    const int64_t v = row_of();
    if (v >= V) return;
    Pos p = load_pos<SRC_PACKED>(src3, src, v);
    if (!SRC_PACKED) {
        const bool pin = (fix_boundary && bnd[v]) || (pinned && pinned[v]);
        p.flags |= pin ? kPinned : 0u;
    }
    float out[3] = {p.x, p.y, p.z};
    if (p.flags == kFinite) {                                                   // finite and not pinned
        int64_t b, e;
        row_range(off, v, cap, b, e);
        double s[3] = {0.0, 0.0, 0.0};
        int n = 0;
        for (int64_t k = b; k < e; k += 4) {
            int32_t j[4];
            Pos q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                j[u] = k + u < e ? nbr[k + u] : -1;
                if (j[u] >= V) j[u] = -1;                                       // never, for a ws from the same mesh
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (j[u] >= 0) q[u] = load_pos<SRC_PACKED>(src3, src, j[u]);
                else q[u] = Pos{0.f, 0.f, 0.f, 0u};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (q[u].flags & kFinite) {
                    s[0] += (double)q[u].x;
                    s[1] += (double)q[u].y;
                    s[2] += (double)q[u].z;
                    ++n;
                }
            }
        }
        if (n) {
            const double w = (double)w_f, dn = (double)n;
            const double pv[3] = {(double)p.x, (double)p.y, (double)p.z};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double m = s[a] / dn;
                out[a] = (float)(pv[a] + w * (m - pv[a]));
            }
        }
    }
    if (DST_PACKED) {
        const uint32_t fl = (p.flags & kPinned) | (finite3(out[0], out[1], out[2]) ? kFinite : 0u);
        dst[v] = Pos{out[0], out[1], out[2], fl};
    } else {
        dst3[3 * v] = out[0];
        dst3[3 * v + 1] = out[1];
        dst3[3 * v + 2] = out[2];
    }
}

// iterations = 0: the output is the input.
__global__ void __launch_bounds__(kThreads) k_sm_copy(const float *__restrict__ src, int64_t n, float *__restrict__ dst) {
    const int64_t i = row_of();
    if (i < n) dst[i] = src[i];
}

}  // namespace

extern "C" {

int64_t m3_mesh_smooth_ws_bytes(int64_t V, int64_t F) {
    SmWs m;
    return sm_layout(V, F, m) ? m.bytes : 0;
}

int m3_mesh_smooth_launches(void) { return kBuildLaunches; }

int m3_mesh_topology_build(const int32_t *faces, int64_t V, int64_t F, void *ws, int64_t ws_bytes, void *stream) {
    SmWs m;
    M3_REQUIRE(sm_layout(V, F, m) && ws_ok(ws) && ws_bytes >= m.bytes);
    M3_REQUIRE((faces || F == 0) && aligned(faces, 4));
    hipStream_t st = (hipStream_t)stream;
    const SmPtr p = sm_ptr(ws, m);
    const dim3 block(kThreads);
    int32_t *deg = p.off + 1;                                                   // degree, then start, then end of row v
    launch_fill(st, ws, m.keys / 16, m.bnd / 16, 0, -1);
    // V = 0 or F = 0: no thread has a row.  The launches are kept so that their number is fixed.
    hipLaunchKernelGGL(k_sm_faces, grid_of(F), block, 0, st, faces, V, F, p.keys, p.cnt, m.S, deg, p.fslot, p.hdr);
    launch_row_starts(st, deg, V + 1, p.tile, m.ntile, p.hdr + kTwoE);          // deg[V] is 0 and becomes 2 E, as word 0
    hipLaunchKernelGGL(k_sm_fill, grid_of(F), block, 0, st, faces, V, F, p.fslot, p.cnt, m.S, deg, p.raw, m.cap, p.hdr);
    hipLaunchKernelGGL(k_sm_sort, grid_of(V), block, 0, st, p.off, V, m.cap, p.raw, p.nbr, p.bnd);
    M3_CHECK_LAUNCH("m3_mesh_topology_build");
    return M3_OK;
}

int m3_mesh_topology_read(const void *ws, int64_t V, int64_t F, int32_t *degree_out, uint8_t *boundary_out, void *stream) {
    SmWs m;
    M3_REQUIRE(sm_layout(V, F, m) && ws_ok(ws));
    M3_REQUIRE(((degree_out && boundary_out) || V == 0) && aligned(degree_out, 4));
    const SmPtr p = sm_ptr((void *)ws, m);
    hipLaunchKernelGGL(k_sm_read, grid_of(V), dim3(kThreads), 0, (hipStream_t)stream, p.off, p.bnd, V, degree_out, boundary_out);
    M3_CHECK_LAUNCH("m3_mesh_topology_read");
    return M3_OK;
}

int m3_mesh_topology_edges(void *ws, int64_t V, int64_t F, int64_t E, int32_t *edges_out, int32_t *edge_faces_out,
                           void *stream) {
    SmWs m;
    M3_REQUIRE(sm_layout(V, F, m) && ws_ok(ws));
    M3_REQUIRE(E >= 0 && E <= 3 * F && ((edges_out && edge_faces_out) || E == 0) && aligned(edges_out, 4) &&
               aligned(edge_faces_out, 4));
    hipStream_t st = (hipStream_t)stream;
    const SmPtr p = sm_ptr(ws, m);
    const dim3 block(kThreads);
    hipLaunchKernelGGL(k_sm_count_edges, grid_of(V), block, 0, st, p.off, p.nbr, V, m.cap, p.tile);
    launch_scan(st, p.hdr + kEdges, ScanJob{p.tile, (int64_t)grid_of(V).x});
    hipLaunchKernelGGL(k_sm_scatter_edges, grid_of(V), block, 0, st, p.off, p.nbr, V, m.cap, p.tile, p.keys, p.cnt, m.S, E,
                       edges_out, edge_faces_out);
    M3_CHECK_LAUNCH("m3_mesh_topology_edges");
    return M3_OK;
}

int m3_mesh_smooth_passes(const float *vertices, int64_t V, int64_t F, void *ws, int64_t ws_bytes, const uint8_t *pinned,
                          int fix_boundary, int method, int iterations, float lam, float mu, float *out, void *stream) {
    SmWs m;
    M3_REQUIRE(sm_layout(V, F, m) && ws_ok(ws) && ws_bytes >= m.bytes);
    M3_REQUIRE(((vertices && out) || V == 0) && aligned(vertices, 4) && aligned(out, 4) && vertices != out);
    M3_REQUIRE((fix_boundary == 0 || fix_boundary == 1) && (method == 0 || method == 1) && iterations >= 0);
    M3_REQUIRE(lam > 0.f && lam <= 1.f && mu > -INFINITY && mu < INFINITY);                          // NaN fails
    hipStream_t st = (hipStream_t)stream;
    const SmPtr p = sm_ptr(ws, m);
    const dim3 grid = grid_of(V), block(kThreads);
    const int64_t passes = (int64_t)iterations * (method == 1 ? 2 : 1);
    if (passes == 0) {
        hipLaunchKernelGGL(k_sm_copy, grid_of(3 * V), block, 0, st, vertices, 3 * V, out);
        M3_CHECK_LAUNCH("m3_mesh_smooth_passes");
        return M3_OK;
    }
    for (int64_t i = 0; i < passes; ++i) {
        const float w = method == 1 && (i & 1) ? mu : lam;
        const Pos *src = p.pos[(i + 1) & 1];                                    // pass i writes buffer i & 1
        Pos *dst = p.pos[i & 1];
        const bool first = i == 0, last = i == passes - 1;
#define M3_SM_PASS(S, D) hipLaunchKernelGGL((k_sm_pass<S, D>), grid, block, 0, st, vertices, src, V, m.cap, p.off, p.nbr, p.bnd, \
                                            pinned, fix_boundary, w, out, dst)
        if (first && last) M3_SM_PASS(false, false);
        else if (first) M3_SM_PASS(false, true);
        else if (last) M3_SM_PASS(true, false);
        else M3_SM_PASS(true, true);
#undef M3_SM_PASS
    }
    M3_CHECK_LAUNCH("m3_mesh_smooth_passes");
    return M3_OK;
}

}  // extern "C"
