// Connected components of a triangle mesh and the filter that drops small fragments (mast3r_slam/components.py,
// DESIGN.md section 7k).  The rule is stated once, in include/m3slam.h; tests/components_twin.py restates it in numpy.
//
// Labelling is a lock-free union-find over parent[V]: parent[v] = v, every valid face hooks the roots of its two edges
// (a, b) and (b, c), the larger root under the smaller, with atomicCAS(&parent[big], big, small).  A node is hooked at
// most once and only ever under a smaller row, so the hooks form a forest whose roots are the smallest rows of their
// trees; every value ever stored in parent[x] - by a hook or by path halving - is an ancestor of x in that forest.
//   * Nobody waits.  A walk to a root follows strictly decreasing rows, so it ends after fewer than V loads whatever
//     those loads return.  A unite() retries only after a failed CAS on `big`; it continues from the value the CAS
//     returned, which is smaller than big, and walks only downwards from there, so one thread fails at most once per
//     hooked node and at most V - 1 nodes are ever hooked.
//   * A stale load is harmless.  An old parent[x] is an ancestor of x (or x itself); an old "x is a root" only makes the
//     CAS, which is decided in L2, fail and hand back the current parent.
// Everything after the hooks runs in later launches and reads a forest that no longer changes.  The counts are int32
// atomicAdd and one 64-bit atomicMax: integer and commutative, so the result does not depend on the execution order.
// Output positions come from the ordered compaction of compact_dev.h: two calls give identical bytes.
//
// ws: int32 [16] header | offV int32 [ceil(V / 256)] | offF int32 [ceil(F / 256)] | parent int32 [V] | label int32 [V] |
// count int32 [V] (faces of the component, at its root's row) | remap int32 [V]; every array padded to 16 bytes.
// Header words: [0] V2, [1] F2 (the totals of the scan), [4] components with a face, [5] largest, [6] winner (-1: no
// valid face), [7] invalid faces, [8..9] the uint64 winner key, [10..12] the filter of the last m3_mesh_components_count
// (min_faces, the bits of min_fraction, largest_only), which the scatter reads back; the others are unused.
#include "table_dev.h"

namespace {

constexpr int kLabelLaunches = 6;             // init, hook, flatten, face count, winner, finish
constexpr int kCountLaunches = 3;             // kept vertices per tile, kept faces per tile, scan
constexpr int kScatterLaunches = 2;           // vertices (writes remap), faces (reads it)
constexpr int kCcHdrWords = 16;
constexpr int kComponents = 4, kLargest = 5, kWinner = 6, kInvalid = 7, kKey = 8, kMinFaces = 10, kFraction = 11, kOnly = 12;
constexpr int64_t kMaxRows = 0x7fffffff;      // V and F stay below 2^31

struct CcWs {
    int64_t ntileV, ntileF;                   // 256-row tiles
    int64_t offV, offF, parent, label, count, remap, bytes;      // byte offsets into ws
};

inline bool cc_layout(int64_t V, int64_t F, CcWs &m) {
    if (V < 0 || F < 0 || V > kMaxRows || F > kMaxRows) return false;
    m.ntileV = (V + kThreads - 1) / kThreads;
    m.ntileF = (F + kThreads - 1) / kThreads;
    m.offV = kCcHdrWords * 4;
    m.offF = m.offV + pad16(4 * m.ntileV);
    m.parent = m.offF + pad16(4 * m.ntileF);
    m.label = m.parent + pad16(4 * V);
    m.count = m.label + pad16(4 * V);
    m.remap = m.count + pad16(4 * V);
    m.bytes = m.remap + pad16(4 * V);
    return true;
}

__device__ __forceinline__ int32_t load_parent(const int32_t *parent, int32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root above x, halving the path on the way: parent[x] = parent[parent[x]] is a store of an ancestor of x.
__device__ __forceinline__ int32_t find_halving(int32_t *parent, int32_t x) {
    int32_t p = load_parent(parent, x);
    while (p != x) {
        const int32_t g = load_parent(parent, p);
        if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = g;
    }
    return x;
}

// The root above x in a forest that no longer changes.
__device__ __forceinline__ int32_t find_root(const int32_t *__restrict__ parent, int32_t x) {
    int32_t p = parent[x];
    while (p != x) {
        x = p;
        p = parent[x];
    }
    return x;
}

__device__ __forceinline__ void unite(int32_t *parent, int32_t a, int32_t b) {
    for (;;) {
        a = find_halving(parent, a);
        b = find_halving(parent, b);
        if (a == b) return;
        const int32_t big = a > b ? a : b, small = a > b ? b : a;
        const int32_t old = atomicCAS(parent + big, big, small);
        if (old == big) return;                                                 // hooked
        a = old;                                                                // somebody hooked big first: old < big
        b = small;
    }
}

__global__ void __launch_bounds__(kThreads) k_cc_init(int64_t V, int32_t *__restrict__ parent, int32_t *__restrict__ count,
                                                       int32_t *__restrict__ hdr) {
    const int64_t v = row_of();
    if (v < kCcHdrWords) hdr[v] = 0;
    if (v >= V) return;
    parent[v] = (int32_t)v;
    count[v] = 0;
}

__global__ void __launch_bounds__(kThreads) k_cc_hook(const int32_t *__restrict__ faces, int64_t V, int64_t F, int32_t *parent,
                                                       int32_t *__restrict__ hdr) {
    const int64_t f = row_of();
    int32_t r[3];
    const bool in = f < F, ok = in && load_face(faces, f, V, r);
    count_invalid(in, ok, hdr + kInvalid);
    if (!ok) return;
    if (r[0] != r[1]) unite(parent, r[0], r[1]);
    if (r[1] != r[2]) unite(parent, r[1], r[2]);
}

__global__ void __launch_bounds__(kThreads) k_cc_flatten(int64_t V, const int32_t *__restrict__ parent,
                                                          int32_t *__restrict__ label, int32_t *__restrict__ labels_out) {
    const int64_t v = row_of();
    if (v >= V) return;
    const int32_t root = find_root(parent, (int32_t)v);
    label[v] = root;
    if (labels_out) labels_out[v] = root;
}

// Valid faces at the root of their first row.  The lanes of a wave that share the first such root add once, together.
__global__ void __launch_bounds__(kThreads) k_cc_count_faces(const int32_t *__restrict__ faces, int64_t V, int64_t F,
                                                              const int32_t *__restrict__ label, int32_t *__restrict__ count) {
    const int64_t f = row_of();
    int32_t r[3];
    const bool ok = f < F && load_face(faces, f, V, r);
    const unsigned long long any = __ballot(ok);
    if (!any) return;                                                           // wave-uniform
    const int32_t root = ok ? label[r[0]] : -1;
    const int lead = __ffsll((long long)any) - 1;
    const int32_t first = __shfl(root, lead, 64);
    const unsigned long long same = __ballot(ok && root == first);
    if ((int)(threadIdx.x & 63) == lead) atomicAdd(count + first, (int)__popcll(same));
    else if (ok && root != first) atomicAdd(count + root, 1);
}

// Components with a face, and the winner: the largest (count << 32 | ~label), so a tie goes to the smaller label.
__global__ void __launch_bounds__(kThreads) k_cc_winner(int64_t V, const int32_t *__restrict__ label,
                                                         const int32_t *__restrict__ count, int32_t *__restrict__ hdr) {
    const int64_t v = row_of();
    const int32_t n = v < V && label[v] == (int32_t)v ? count[v] : 0;
    unsigned long long key = n > 0 ? ((unsigned long long)(uint32_t)n << 32) | (uint32_t)~(uint32_t)v : 0ull;
    const unsigned long long roots = __ballot(n > 0);
    if (!roots) return;                                                         // wave-uniform
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(key, off, 64);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(hdr + kComponents, (int)__popcll(roots));
        atomicMax((unsigned long long *)(hdr + kKey), key);
    }
}

__global__ void __launch_bounds__(kThreads) k_cc_finish(int64_t V, const int32_t *__restrict__ label,
                                                         const int32_t *__restrict__ count, int32_t *__restrict__ hdr,
                                                         int32_t *__restrict__ faces_of_out) {
    const int64_t v = row_of();
    if (v == 0) {
        const unsigned long long key = *(const unsigned long long *)(hdr + kKey);
        hdr[kLargest] = (int32_t)(key >> 32);
        hdr[kWinner] = key ? (int32_t)~(uint32_t)key : -1;
    }
    if (v < V && faces_of_out) faces_of_out[v] = count[label[v]];
}

struct Filter {
    int min_faces, largest_only;
    float min_fraction;
};

// Is component c kept?  largest and winner are read from the header: the host never passes them.
__device__ __forceinline__ bool component_kept(int32_t c, const int32_t *__restrict__ count, const int32_t *__restrict__ hdr,
                                               const Filter &fl) {
    const int32_t n = count[c];
    if (n < (fl.min_faces > 1 ? fl.min_faces : 1)) return false;
    if (fl.min_fraction != 0.f && !((double)n >= (double)fl.min_fraction * (double)hdr[kLargest])) return false;
    return !fl.largest_only || c == hdr[kWinner];
}

__device__ __forceinline__ Filter stored_filter(const int32_t *__restrict__ hdr) {
    return Filter{hdr[kMinFaces], hdr[kOnly], __int_as_float(hdr[kFraction])};
}

__device__ __forceinline__ bool vertex_kept(int64_t v, int64_t V, const int32_t *__restrict__ label,
                                            const int32_t *__restrict__ count, const int32_t *__restrict__ hdr, const Filter &fl) {
    return v < V && component_kept(label[v], count, hdr, fl);
}

__device__ __forceinline__ bool face_kept(const int32_t *__restrict__ faces, int64_t f, int64_t V, int64_t F,
                                          const int32_t *__restrict__ label, const int32_t *__restrict__ count,
                                          const int32_t *__restrict__ hdr, const Filter &fl, int32_t (&r)[3]) {
    return f < F && load_face(faces, f, V, r) && component_kept(label[r[0]], count, hdr, fl);
}

// Kept vertices per tile.  The scatter has no filter arguments: it reads the filter this kernel leaves in the header (the
// words 10 ... 12 are read by no thread of the two count kernels).
__global__ void __launch_bounds__(kThreads) k_cc_count_vertices(int64_t V, const int32_t *__restrict__ label,
                                                                 const int32_t *__restrict__ count, int32_t *hdr, Filter fl,
                                                                 int32_t *__restrict__ cntV) {
    const int64_t v = row_of();
    if (v == 0) {
        hdr[kMinFaces] = fl.min_faces;
        hdr[kFraction] = __float_as_int(fl.min_fraction);
        hdr[kOnly] = fl.largest_only;
    }
    int total;
    block_prefix(vertex_kept(v, V, label, count, hdr, fl) ? 1u : 0u, total);
    if (threadIdx.x == 0) cntV[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kThreads) k_cc_count_kept_faces(const int32_t *__restrict__ faces, int64_t V, int64_t F,
                                                                   const int32_t *__restrict__ label,
                                                                   const int32_t *__restrict__ count,
                                                                   const int32_t *__restrict__ hdr, Filter fl,
                                                                   int32_t *__restrict__ cntF) {
    int32_t r[3];
    int total;
    block_prefix(face_kept(faces, row_of(), V, F, label, count, hdr, fl, r) ? 1u : 0u, total);
    if (threadIdx.x == 0) cntF[blockIdx.x] = total;
}

// Kept vertices to rows offV[tile] + rank, with their colours as passed; remap[v] = its row.
__global__ void __launch_bounds__(kThreads) k_cc_vertices(const float *__restrict__ vertices, const uint8_t *__restrict__ colors,
                                                           int64_t V, const int32_t *__restrict__ label,
                                                           const int32_t *__restrict__ count, const int32_t *__restrict__ hdr,
                                                           const int32_t *__restrict__ offs, int64_t V2,
                                                           int32_t *__restrict__ remap, float *__restrict__ vertices_out,
                                                           uint8_t *__restrict__ colors_out, int64_t *__restrict__ rows_out) {
    const int64_t v = row_of();
    const bool on = vertex_kept(v, V, label, count, hdr, stored_filter(hdr));
    int total;
    const int64_t o = (int64_t)offs[blockIdx.x] + block_prefix(on ? 1u : 0u, total);
    if (!on || o >= V2) return;                                                 // o < V2 always holds for a ws from the same inputs
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        vertices_out[3 * o + i] = vertices[3 * v + i];
        colors_out[3 * o + i] = colors[3 * v + i];
    }
    if (rows_out) rows_out[o] = v;
    remap[v] = (int32_t)o;
}

// Kept faces to rows offF[tile] + rank, rewritten to the new vertex rows.
__global__ void __launch_bounds__(kThreads) k_cc_faces(const int32_t *__restrict__ faces, int64_t V, int64_t F,
                                                        const int32_t *__restrict__ label, const int32_t *__restrict__ count,
                                                        const int32_t *__restrict__ hdr, const int32_t *__restrict__ offs,
                                                        const int32_t *__restrict__ remap, int64_t F2,
                                                        int32_t *__restrict__ faces_out, int64_t *__restrict__ rows_out) {
    const int64_t f = row_of();
    int32_t r[3];
    const bool on = face_kept(faces, f, V, F, label, count, hdr, stored_filter(hdr), r);
    int total;
    const int64_t o = (int64_t)offs[blockIdx.x] + block_prefix(on ? 1u : 0u, total);
    if (!on || o >= F2) return;                                                 // o < F2 always holds for a ws from the same inputs
#pragma unroll
    for (int i = 0; i < 3; ++i) faces_out[3 * o + i] = remap[r[i]];
    if (rows_out) rows_out[o] = f;
}

}  // namespace

extern "C" {

int64_t m3_mesh_components_ws_bytes(int64_t V, int64_t F) {
    CcWs m;
    return cc_layout(V, F, m) ? m.bytes : 0;
}

int m3_mesh_components_launches(void) { return kLabelLaunches + kCountLaunches + kScatterLaunches; }

int m3_mesh_components_label(const int32_t *faces, int64_t V, int64_t F, void *ws, int64_t ws_bytes, int32_t *labels_out,
                             int32_t *faces_of_out, void *stream) {
    CcWs m;
    M3_REQUIRE(cc_layout(V, F, m) && ws_ok(ws) && ws_bytes >= m.bytes && (faces || F == 0));
    M3_REQUIRE(((uintptr_t)faces & 3) == 0 && ((uintptr_t)labels_out & 3) == 0 && ((uintptr_t)faces_of_out & 3) == 0);
    hipStream_t st = (hipStream_t)stream;
    char *p = (char *)ws;
    int32_t *hdr = (int32_t *)ws, *parent = (int32_t *)(p + m.parent), *label = (int32_t *)(p + m.label);
    int32_t *count = (int32_t *)(p + m.count);
    const dim3 gv = grid_of(V), gf = grid_of(F), block(kThreads);     // one workgroup for V = 0: thread 0 clears the header
    hipLaunchKernelGGL(k_cc_init, gv, block, 0, st, V, parent, count, hdr);
    if (F > 0) hipLaunchKernelGGL(k_cc_hook, gf, block, 0, st, faces, V, F, parent, hdr);
    hipLaunchKernelGGL(k_cc_flatten, gv, block, 0, st, V, parent, label, labels_out);
    if (F > 0) hipLaunchKernelGGL(k_cc_count_faces, gf, block, 0, st, faces, V, F, label, count);
    hipLaunchKernelGGL(k_cc_winner, gv, block, 0, st, V, label, count, hdr);
    hipLaunchKernelGGL(k_cc_finish, gv, block, 0, st, V, label, count, hdr, faces_of_out);
    M3_CHECK_LAUNCH("m3_mesh_components_label");
    return M3_OK;
}

int m3_mesh_components_count(void *ws, int64_t V, int64_t F, const int32_t *faces, int min_faces, float min_fraction,
                             int largest_only, void *stream) {
    CcWs m;
    M3_REQUIRE(cc_layout(V, F, m) && ws_ok(ws) && (faces || F == 0) && ((uintptr_t)faces & 3) == 0);
    M3_REQUIRE(min_fraction >= 0.f && min_fraction <= 1.f && (largest_only == 0 || largest_only == 1));     // NaN fails
    hipStream_t st = (hipStream_t)stream;
    char *p = (char *)ws;
    int32_t *hdr = (int32_t *)ws;
    if (V == 0 || F == 0) {                                                     // no face: nothing is kept
        M3_CHECK_HIP(hipMemsetAsync(ws, 0, 8, st), "m3_mesh_components_count/memset");
        return M3_OK;
    }
    const int32_t *label = (const int32_t *)(p + m.label), *count = (const int32_t *)(p + m.count);
    int32_t *cntV = (int32_t *)(p + m.offV), *cntF = (int32_t *)(p + m.offF);
    const Filter fl{min_faces, largest_only, min_fraction};
    const dim3 block(kThreads);
    hipLaunchKernelGGL(k_cc_count_vertices, grid_of(V), block, 0, st, V, label, count, hdr, fl, cntV);
    hipLaunchKernelGGL(k_cc_count_kept_faces, grid_of(F), block, 0, st, faces, V, F, label, count, hdr, fl, cntF);
    launch_scan(st, hdr, ScanJob{cntV, m.ntileV}, ScanJob{cntF, m.ntileF});                         // V2 to word 0, F2 to word 1
    M3_CHECK_LAUNCH("m3_mesh_components_count");
    return M3_OK;
}

int m3_mesh_components_scatter(const float *vertices, const uint8_t *colors, const int32_t *faces, int64_t V, int64_t F,
                               void *ws, int64_t V2, int64_t F2, float *vertices_out, uint8_t *colors_out, int32_t *faces_out,
                               int64_t *vertex_rows_out, int64_t *face_rows_out, void *stream) {
    CcWs m;
    M3_REQUIRE(cc_layout(V, F, m) && ws_ok(ws) && vertices && colors && faces && vertices_out && colors_out && faces_out);
    M3_REQUIRE(V2 >= 1 && V2 <= V && F2 >= 1 && F2 <= F);
    M3_REQUIRE(((uintptr_t)vertices & 3) == 0 && ((uintptr_t)faces & 3) == 0 && ((uintptr_t)vertices_out & 3) == 0 &&
               ((uintptr_t)faces_out & 3) == 0 && ((uintptr_t)vertex_rows_out & 7) == 0 && ((uintptr_t)face_rows_out & 7) == 0);
    hipStream_t st = (hipStream_t)stream;
    char *p = (char *)ws;
    const int32_t *hdr = (const int32_t *)ws, *label = (const int32_t *)(p + m.label), *count = (const int32_t *)(p + m.count);
    const int32_t *offV = (const int32_t *)(p + m.offV), *offF = (const int32_t *)(p + m.offF);
    int32_t *remap = (int32_t *)(p + m.remap);
    const dim3 block(kThreads);
    hipLaunchKernelGGL(k_cc_vertices, grid_of(V), block, 0, st, vertices, colors, V, label, count, hdr, offV, V2, remap,
                       vertices_out, colors_out, vertex_rows_out);
    hipLaunchKernelGGL(k_cc_faces, grid_of(F), block, 0, st, faces, V, F, label, count, hdr, offF, remap, F2, faces_out,
                       face_rows_out);
    M3_CHECK_LAUNCH("m3_mesh_components_scatter");
    return M3_OK;
}

}  // extern "C"
