// Mesh simplification by vertex clustering (mast3r_slam/simplify.py): one output vertex per
// occupied voxel, faces rewritten, collapsed and repeated faces removed.  The rule is stated once, in include/m3slam.h;
// tests/simplify_twin.py restates it in numpy.
//
// count:   clear -> one thread per vertex (claim the cell's slot, lower its leader, add the sums) -> one thread per vertex
//          (its leader; leaders per tile) -> one thread per face (leaders of its rows, the drops, claim or lower the
//          key's slot) -> winners per tile -> one scan of both counts.
// scatter: leaders write their cluster (and their output row into ws) -> winning faces, and cluster_of.
// Eight launches whatever the mesh holds.  The cells live in the key table of table_dev.h.  The only atomics are integer
// ones whose results commute: the claim of a slot, min for the leader row and for the face row, add for the sums.  Which
// slot a face key lands in depends on the arrival order, as for a cell; nothing that is output does.  Output rows are
// tile offset + rank (compact_dev.h), never a counter.
//
// A face key is the triple of its clusters' LEADER rows, rotated so the smallest comes first: clusters are output in the
// order of their leaders, so this is the rotation of the output rows, and the face pass does not have to wait for the
// scan.  The face table holds a face row per slot, never the 93-bit key: a thread that finds a slot occupied rebuilds
// the occupant's key from `faces` and the leaders.  An occupant is only ever replaced by a smaller row WITH THE SAME KEY
// (atomicMin after an equal comparison), so a comparison against an occupant that is being lowered stays valid and
// nobody waits.
//
// ws: int32 [16] header | offV int32 [max(1, ceil(V / 256))] | offF int32 [likewise, F] | vslot uint32 [V] | vlead int32 [V] |
// vrow int32 [V] | fslot uint32 [F] | keys uint64 [SV] | lead int32 [SV] | ftab int32 [SF] | cnt int32 [SV] |
// sums uint64 [6][SV] (q.x, q.y, q.z, red, green, blue: a plane each); SV, SF = the power of two >= max(1024, 2 V), 2 F.
// Header words: [0] V2, [1] F2 (the totals of the scan), [2] out-of-range vertices, [3] invalid faces, [4] the bits of
// voxel_size, which the scatter reads back; the others are 0.
//
// Compiled with -ffp-contract=off: every float64 operation of the rule is rounded on its own.
#include "table_dev.h"
#pragma clang fp contract(off)

namespace {

constexpr int kCountLaunches = 6, kScatterLaunches = 2;
constexpr int kSvHdrWords = 16;               // the fill zeroes them: kSvHdrWords / 4 int4 at the head of ws
constexpr int kOutOfRange = 2, kInvalid = 3, kVoxel = 4;
constexpr int64_t kMaxRows = 0x7fffffff;      // V and F stay below 2^31
constexpr int32_t kNoRow = 0x7fffffff;        // an empty leader / face slot: above every row
constexpr double kCellLim = 1048576.0;        // 2^20: 21 bits per axis after the offset (kCellBias)
constexpr double kQ = 16777216.0;             // 2^24

struct SvWs {
    int64_t ntileV, ntileF, SV, SF;
    int64_t offV, offF, vslot, vlead, vrow, fslot, keys, lead, ftab, cnt, sums, bytes;      // byte offsets into ws
};

inline bool sv_layout(int64_t V, int64_t F, SvWs &m) {
    if (V < 0 || F < 0 || V > kMaxRows || F > kMaxRows) return false;
    m.ntileV = V ? (V + kThreads - 1) / kThreads : 1;    // at least one tile: the one workgroup of an empty grid
    m.ntileF = F ? (F + kThreads - 1) / kThreads : 1;    // writes its count, 0
    m.SV = table_slots(2 * V);
    m.SF = table_slots(2 * F);
    m.offV = kSvHdrWords * 4;
    m.offF = m.offV + pad16(4 * m.ntileV);
    m.vslot = m.offF + pad16(4 * m.ntileF);
    m.vlead = m.vslot + pad16(4 * V);
    m.vrow = m.vlead + pad16(4 * V);
    m.fslot = m.vrow + pad16(4 * V);
    m.keys = m.fslot + pad16(4 * F);          // from here on the fill: ff .. | 7fffffff .. | 0 ..
    m.lead = m.keys + 8 * m.SV;
    m.ftab = m.lead + 4 * m.SV;
    m.cnt = m.ftab + 4 * m.SF;
    m.sums = m.cnt + 4 * m.SV;
    m.bytes = m.sums + 48 * m.SV;
    return true;
}

struct SvPtr {
    int32_t *hdr, *offV, *offF, *vlead, *vrow, *lead, *ftab, *cnt;
    uint32_t *vslot, *fslot;
    unsigned long long *keys, *sums;
};

inline SvPtr sv_ptr(void *ws, const SvWs &m) {
    char *p = (char *)ws;
    SvPtr q;
    q.hdr = (int32_t *)p;
    q.offV = (int32_t *)(p + m.offV);
    q.offF = (int32_t *)(p + m.offF);
    q.vslot = (uint32_t *)(p + m.vslot);
    q.vlead = (int32_t *)(p + m.vlead);
    q.vrow = (int32_t *)(p + m.vrow);
    q.fslot = (uint32_t *)(p + m.fslot);
    q.keys = (unsigned long long *)(p + m.keys);
    q.lead = (int32_t *)(p + m.lead);
    q.ftab = (int32_t *)(p + m.ftab);
    q.cnt = (int32_t *)(p + m.cnt);
    q.sums = (unsigned long long *)(p + m.sums);
    return q;
}

// Cell and quantised offset of one coordinate; false when it is out of range (NaN and infinities fail the test).
__device__ __forceinline__ bool cell_of(float x, double voxel, int &cell, long long &q) {
    const double t = (double)x / voxel;
    const double c = floor(t);
    if (!(fabs(c) < kCellLim)) return false;
    cell = (int)c;
    q = llrint((t - c) * kQ);
    return true;
}

// One vertex per thread: claim the slot of its cell, lower the slot's leader to this row, add to the slot's sums.  Thread 0
// leaves the bits of voxel_size in the header, which the fill has just zeroed.
// Keyframe meshes arrive in pixel order, so neighbouring lanes usually share a cell.  A run of adjacent lanes with the
// same cell adds up inside the wave first (a segmented shuffle sum: q < 2^24 + 1 and a colour < 2^8 over 64 lanes fit 32
// bits), and its first lane - the run's smallest row - probes, claims and adds once for all of them: eight atomics per run
// in place of eight per vertex (profiles/simplify_bench.md).  The sums are integers, so the bytes do not change.
__global__ void __launch_bounds__(kThreads) k_sv_insert(const float *__restrict__ vertices, const uint8_t *__restrict__ colors,
                                                         int64_t V, float voxel_f, unsigned long long *__restrict__ keys,
                                                         int32_t *__restrict__ lead, int32_t *__restrict__ cnt,
                                                         unsigned long long *__restrict__ sums, int64_t SV,
                                                         uint32_t *__restrict__ vslot, int32_t *__restrict__ vlead,
                                                         int32_t *__restrict__ hdr) {
    const int64_t v = row_of();
    const int lane = threadIdx.x & 63;
    const double voxel = (double)voxel_f;
    int cell[3] = {0, 0, 0};
    long long q[3] = {0, 0, 0};
    bool in = v < V;
    if (in) {
#pragma unroll
        for (int k = 0; k < 3; ++k) in = cell_of(vertices[3 * v + k], voxel, cell[k], q[k]) && in;
    }
    if (v == 0) hdr[kVoxel] = __float_as_int(voxel_f);
    const unsigned long long out = __ballot(v < V && !in);
    if (out && lane == 0) atomicAdd(hdr + kOutOfRange, (int)__popcll(out));      // V < 2^31: no overflow
    if (!__ballot(in)) {                                                        // wave-uniform: nothing to insert
        if (v < V) { vslot[v] = 0u; vlead[v] = -1; }
        return;
    }
    // every lane of the wave stays to the last shuffle
    const unsigned long long key = !in ? kEmptyKey : cell_key(cell[0] + kCellBias, cell[1] + kCellBias, cell[2] + kCellBias);
    unsigned x[5] = {(unsigned)q[0], (unsigned)q[1], (unsigned)q[2], 0u, 0u};    // q.x, q.y, q.z, red | green << 16, blue
    if (in) {
        x[3] = (unsigned)colors[3 * v] | ((unsigned)colors[3 * v + 1] << 16);
        x[4] = (unsigned)colors[3 * v + 2];
    }
    const unsigned long long prev = __shfl_up(key, 1, 64);
    const bool head = !in || lane == 0 || prev != key;                          // a lane with nothing to insert is a run of its own
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    const int after = above ? __ffsll((long long)above) - 1 : 63 - lane;         // lanes of my run behind me
    if (heads != ~0ull) {                                                       // wave-uniform: some run has two lanes
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const unsigned o = __shfl_down(x[k], off, 64);
                if (off <= after) x[k] += o;                                    // lane + off holds the sum of its next `off` lanes of the run
            }
        }
    }
    unsigned s32 = 0u;
    bool claimed;
    const uint32_t s = in && head ? key_claim(keys, SV, key, claimed) : kNoSlot;
    if (s != kNoSlot) {                                                         // always, for a lane that looked
        atomicMin(lead + s, (int32_t)v);                                        // the run's smallest row
        atomicAdd(cnt + s, after + 1);
        const unsigned c[3] = {x[3] & 0xffffu, x[3] >> 16, x[4]};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            atomicAdd(sums + (int64_t)k * SV + s, (unsigned long long)x[k]);
            atomicAdd(sums + (int64_t)(3 + k) * SV + s, (unsigned long long)c[k]);
        }
        s32 = s;
    }
    const unsigned long long upto = heads & (~0ull >> (63 - lane));             // heads at or below my lane: never empty (lane 0)
    s32 = __shfl(s32, 63 - __clzll((long long)upto), 64);                        // the slot my run's first lane found
    if (v >= V) return;
    vslot[v] = in ? s32 : 0u;
    vlead[v] = in ? 0 : -1;                                                     // in range: k_sv_leaders writes the leader
}

// vlead[v] = the leader of v's cluster (-1: out of range), and the leaders per tile.
__global__ void __launch_bounds__(kThreads) k_sv_leaders(int64_t V, const uint32_t *__restrict__ vslot,
                                                          const int32_t *__restrict__ lead, int32_t *__restrict__ vlead,
                                                          int32_t *__restrict__ cntV) {
    const int64_t v = row_of();
    bool leader = false;
    if (v < V && vlead[v] >= 0) {
        const int32_t l = lead[vslot[v]];
        vlead[v] = l;
        leader = l == (int32_t)v;
    }
    int total;
    block_prefix(leader ? 1u : 0u, total);
    if (threadIdx.x == 0) cntV[blockIdx.x] = total;
}

// The key of a face with valid rows r: the leaders of its clusters, rotated so the smallest comes first.  false when
// the face is dropped: a row out of range, or two rows in one cluster.
__device__ __forceinline__ bool face_key(const int32_t (&r)[3], const int32_t *__restrict__ vlead, int32_t (&k)[3]) {
    const int32_t a = vlead[r[0]], b = vlead[r[1]], c = vlead[r[2]];
    if (a < 0 || b < 0 || c < 0 || a == b || b == c || a == c) return false;
    if (a < b && a < c) { k[0] = a; k[1] = b; k[2] = c; }
    else if (b < c) { k[0] = b; k[1] = c; k[2] = a; }
    else { k[0] = c; k[1] = a; k[2] = b; }
    return true;
}

// One face per thread: the drops, then claim the slot of its key or lower the slot's face row to this one.
__global__ void __launch_bounds__(kThreads) k_sv_faces(const int32_t *__restrict__ faces, int64_t V, int64_t F,
                                                        const int32_t *__restrict__ vlead, int32_t *__restrict__ ftab,
                                                        int64_t SF, uint32_t *__restrict__ fslot, int32_t *__restrict__ hdr) {
    const int64_t f = row_of();
    int32_t r[3], k[3];
    const bool in = f < F, ok = in && load_face(faces, f, V, r);
    count_invalid(in, ok, hdr + kInvalid);
    if (!in) return;
    if (!ok || !face_key(r, vlead, k)) {
        fslot[f] = 0u;                                                          // no slot ever holds a dropped face's row
        return;
    }
    const unsigned long long mask = (unsigned long long)(SF - 1);
    unsigned long long s = mix64(mix64(((unsigned long long)(uint32_t)k[0] << 32) | (uint32_t)k[1]) ^ (uint32_t)k[2]) & mask;
    for (int64_t probe = 0; probe < SF; ++probe) {                              // the table is at most half full: this ends
        int32_t cur = __hip_atomic_load(ftab + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kNoRow) cur = atomicCAS(ftab + s, kNoRow, (int32_t)f);
        if (cur == kNoRow) break;                                               // claimed
        int32_t r2[3], k2[3];
        load_face(faces, cur, V, r2);                                           // an occupant is a face that has a key
        face_key(r2, vlead, k2);
        if (k2[0] == k[0] && k2[1] == k[1] && k2[2] == k[2]) {
            atomicMin(ftab + s, (int32_t)f);
            break;
        }
        s = (s + 1) & mask;
    }
    fslot[f] = (uint32_t)s;
}

__device__ __forceinline__ bool face_won(int64_t f, int64_t F, const uint32_t *__restrict__ fslot,
                                         const int32_t *__restrict__ ftab) {
    return f < F && ftab[fslot[f]] == (int32_t)f;
}

__global__ void __launch_bounds__(kThreads) k_sv_count_faces(int64_t F, const uint32_t *__restrict__ fslot,
                                                              const int32_t *__restrict__ ftab, int32_t *__restrict__ cntF) {
    int total;
    block_prefix(face_won(row_of(), F, fslot, ftab) ? 1u : 0u, total);
    if (threadIdx.x == 0) cntF[blockIdx.x] = total;
}

// Leaders to rows offV[tile] + rank: the vertex itself for a cluster of one, the float64 finish of the integer sums
// otherwise.  vrow[leader] = its row.
__global__ void __launch_bounds__(kThreads) k_sv_vertices(const float *__restrict__ vertices, const uint8_t *__restrict__ colors,
                                                           int64_t V, const int32_t *__restrict__ hdr,
                                                           const uint32_t *__restrict__ vslot, const int32_t *__restrict__ vlead,
                                                           const unsigned long long *__restrict__ keys,
                                                           const int32_t *__restrict__ cnt,
                                                           const unsigned long long *__restrict__ sums, int64_t SV,
                                                           const int32_t *__restrict__ offs, int64_t V2,
                                                           int32_t *__restrict__ vrow, float *__restrict__ vertices_out,
                                                           uint8_t *__restrict__ colors_out) {
    const int64_t v = row_of();
    const bool on = v < V && vlead[v] == (int32_t)v;
    int total;
    const int64_t o = (int64_t)offs[blockIdx.x] + block_prefix(on ? 1u : 0u, total);
    if (!on || o >= V2) return;                                                 // o < V2 always holds for a ws from the same inputs
    vrow[v] = (int32_t)o;
    const uint32_t s = vslot[v];
    const int32_t n = cnt[s];
    if (n == 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            vertices_out[3 * o + k] = vertices[3 * v + k];
            colors_out[3 * o + k] = colors[3 * v + k];
        }
        return;
    }
    const double voxel = (double)__int_as_float(hdr[kVoxel]);
    int b[3];
    cell_unkey(keys[s], b[0], b[1], b[2]);
    const double den = (double)n * kQ;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int cell = b[k] - kCellBias;
        const double mean = (double)(long long)sums[(int64_t)k * SV + s] / den;
        vertices_out[3 * o + k] = (float)(((double)cell + mean) * voxel);
        const unsigned long long C = sums[(int64_t)(3 + k) * SV + s];
        colors_out[3 * o + k] = (uint8_t)((2ull * C + (unsigned long long)n) / (2ull * (unsigned long long)n));
    }
}

// Winning faces to rows offF[tile] + rank, written as their key in output rows; and cluster_of for every input vertex.
__global__ void __launch_bounds__(kThreads) k_sv_scatter_faces(const int32_t *__restrict__ faces, int64_t V, int64_t F,
                                                                const int32_t *__restrict__ vlead,
                                                                const int32_t *__restrict__ vrow,
                                                                const uint32_t *__restrict__ fslot,
                                                                const int32_t *__restrict__ ftab,
                                                                const int32_t *__restrict__ offs, int64_t ntileF, int64_t F2,
                                                                int32_t *__restrict__ faces_out,
                                                                int64_t *__restrict__ face_rows_out,
                                                                int64_t *__restrict__ cluster_of_out) {
    const int64_t f = row_of();
    if (cluster_of_out && f < V) {
        const int32_t l = vlead[f];
        cluster_of_out[f] = l < 0 ? -1 : (int64_t)vrow[l];
    }
    if ((int64_t)blockIdx.x >= ntileF) return;                                  // workgroup-uniform: a tile of vertices only
    const bool on = face_won(f, F, fslot, ftab);
    int total;
    const int64_t o = (int64_t)offs[blockIdx.x] + block_prefix(on ? 1u : 0u, total);
    if (!on || o >= F2) return;                                                 // o < F2 always holds for a ws from the same inputs
    int32_t r[3], k[3];
    load_face(faces, f, V, r);
    face_key(r, vlead, k);
#pragma unroll
    for (int i = 0; i < 3; ++i) faces_out[3 * o + i] = vrow[k[i]];
    if (face_rows_out) face_rows_out[o] = f;
}

}  // namespace

extern "C" {

int64_t m3_mesh_simplify_ws_bytes(int64_t V, int64_t F) {
    SvWs m;
    return sv_layout(V, F, m) ? m.bytes : 0;
}

int m3_mesh_simplify_launches(void) { return kCountLaunches + kScatterLaunches; }

int m3_mesh_simplify_count(const float *vertices, const uint8_t *colors, const int32_t *faces, int64_t V, int64_t F,
                           float voxel_size, void *ws, int64_t ws_bytes, void *stream) {
    SvWs m;
    M3_REQUIRE(sv_layout(V, F, m) && ws_ok(ws) && ws_bytes >= m.bytes);
    M3_REQUIRE(((vertices && colors) || V == 0) && (faces || F == 0) && aligned(vertices, 4) && aligned(faces, 4));
    M3_REQUIRE(voxel_size > 0.f && voxel_size < INFINITY);                                           // NaN fails
    hipStream_t st = (hipStream_t)stream;
    const SvPtr p = sv_ptr(ws, m);
    const dim3 gv = grid_of(V), gf = grid_of(F), block(kThreads);
    const int64_t a = (m.lead - m.keys) / 16, b = (m.cnt - m.keys) / 16, n = (m.bytes - m.keys) / 16;
    hipLaunchKernelGGL(k_fill3, grid_of(n), block, 0, st, (int4 *)p.keys, a, b, n, -1, kNoRow, 0, (int4 *)p.hdr,
                       kSvHdrWords / 4);
    // V = 0 or F = 0: no thread has a row.  The launches are kept so that their number is fixed.
    hipLaunchKernelGGL(k_sv_insert, gv, block, 0, st, vertices, colors, V, voxel_size, p.keys, p.lead, p.cnt, p.sums, m.SV,
                       p.vslot, p.vlead, p.hdr);
    hipLaunchKernelGGL(k_sv_leaders, gv, block, 0, st, V, p.vslot, p.lead, p.vlead, p.offV);
    hipLaunchKernelGGL(k_sv_faces, gf, block, 0, st, faces, V, F, p.vlead, p.ftab, m.SF, p.fslot, p.hdr);
    hipLaunchKernelGGL(k_sv_count_faces, gf, block, 0, st, F, p.fslot, p.ftab, p.offF);
    launch_scan(st, p.hdr, ScanJob{p.offV, m.ntileV}, ScanJob{p.offF, m.ntileF});                     // V2 to word 0, F2 to word 1
    M3_CHECK_LAUNCH("m3_mesh_simplify_count");
    return M3_OK;
}

int m3_mesh_simplify_scatter(const float *vertices, const uint8_t *colors, const int32_t *faces, int64_t V, int64_t F,
                             void *ws, int64_t ws_bytes, int64_t V2, int64_t F2, float *vertices_out, uint8_t *colors_out,
                             int32_t *faces_out, int64_t *cluster_of_out, int64_t *face_rows_out, void *stream) {
    SvWs m;
    M3_REQUIRE(sv_layout(V, F, m) && ws_ok(ws) && ws_bytes >= m.bytes);
    M3_REQUIRE(((vertices && colors) || V == 0) && (faces || F == 0) && V2 >= 0 && V2 <= V && F2 >= 0 && F2 <= F);
    M3_REQUIRE(((vertices_out && colors_out) || V2 == 0) && (faces_out || F2 == 0));
    M3_REQUIRE(aligned(vertices, 4) && aligned(faces, 4) && aligned(vertices_out, 4) && aligned(faces_out, 4) &&
               aligned(cluster_of_out, 8) && aligned(face_rows_out, 8));
    hipStream_t st = (hipStream_t)stream;
    const SvPtr p = sv_ptr(ws, m);
    const dim3 block(kThreads);
    hipLaunchKernelGGL(k_sv_vertices, grid_of(V), block, 0, st, vertices, colors, V, p.hdr, p.vslot, p.vlead, p.keys,
                       p.cnt, p.sums, m.SV, p.offV, V2, p.vrow, vertices_out, colors_out);
    const int64_t rows = cluster_of_out && V > F ? V : F;                       // cluster_of takes a thread per vertex
    hipLaunchKernelGGL(k_sv_scatter_faces, grid_of(rows), block, 0, st, faces, V, F, p.vlead, p.vrow, p.fslot, p.ftab, p.offF,
                       m.ntileF, F2, faces_out, face_rows_out, cluster_of_out);
    M3_CHECK_LAUNCH("m3_mesh_simplify_scatter");
    return M3_OK;
}

}  // extern "C"
