// Triangle mesh export (mast3r_slam/export.py collect_mesh): every keyframe's pointmap is an organised H x W grid, so
// neighbouring pixels are the natural triangles; triangles that bridge a depth discontinuity are refused.
//
// Inputs, as for m3_map_export_*: device tables X[k] -> float [N,3] (points in the keyframe's own camera frame),
// C[k] -> float [N], img[k]; poses [K,8], Nk [K], layout M3_MAP_IMG_*; N = H * W in row-major order, H and W given.
// Parameters: stride s >= 1; edge_ratio > 0 (fp32); the export's use_thresh / thresh.
//
// Grid.  Vertices sit at pixels (gy * s, gx * s), with gy < Hg = ceil(H / s) and gx < Wg = ceil(W / s).  The source
// index of a vertex is k * N + (gy * s) * W + gx * s.  Cells are (gy, gx) with gy < Hg - 1 and gx < Wg - 1.  A cell has
// corners a = (gy, gx), b = (gy, gx + 1), c = (gy + 1, gx), d = (gy + 1, gx + 1).
//
// Candidate triangles per cell.  t = 0 is (a, c, b) and t = 1 is (b, c, d), with vertices in exactly this order.  The
// diagonal is always b - c.  With image x to the right, y down and z forward, both triangles are counter-clockwise seen
// from the keyframe's camera.  Their normal (v1 - v0) x (v2 - v0) points back at the camera.
//
// Vertex validity.  This is exactly the export rule: C[k][n] / (float)Nk[k] > thresh (IEEE fp32 divide, strict, NaN
// fails; use_thresh = 0 skips it); and the world point s R X + t is finite, as map_points.h computes it.
//
// Edge test.  It works on the camera-frame points X, so it does not depend on the pose or the Sim(3) scale.  It is fp32
// with every operation separately rounded, so this file is compiled with -ffp-contract=off.  For an edge (p, q):
// dx = p.x - q.x and likewise for y and z, then l2 = (dx*dx + dy*dy) + dz*dz.  For a vertex: r2 = (x*x + y*y) + z*z.
// t2 = edge_ratio * edge_ratio.  The edge passes iff l2 <= t2 * fminf(r2_p, r2_q).  The comparison is <=, and a NaN on
// either side fails.  No square root is taken anywhere.
//
// Keeping.  A triangle is kept iff its three vertices are valid and its three edges pass.  A vertex is emitted iff at
// least one kept triangle references it.
//
// Outputs.  vertices float32 [V,3]: world points, the same bytes collect_map writes for that source index.  colors
// uint8 [V,3]: the export's colour rule.  index int64 [V] (optional): source index.  Vertices are in ascending source
// index.  faces int32 [F,3] holds rows of the vertex arrays, in ascending (k, gy, gx, t).
//
// Passes.  The float rule is evaluated ONCE, by k_mesh_cells, which stages the vertex rows of a
// 8 x 256-cell tile in LDS (an invalid vertex is staged as NaN, so every edge that touches it fails) and leaves two
// bits per cell in ws.  Everything after it is integer work on those bits: a vertex is used when one of its up to six
// incident triangles is kept (a gather over four cell bytes, no flags are scattered); used vertices are counted per
// 1024-point tile (the export's grid: source order) and kept triangles per row segment of 256 cells (segments in
// (k, gy, segment) order are in output order), both are scanned, and the two scatter kernels place vertices and faces
// at offset + rank inside the tile or segment (ballots).  There is no atomic of any kind, so two calls give identical
// bytes, and a keyframe's rows depend on the others only through the scanned offsets.
#include "common.h"
#pragma clang fp contract(fast)                 // the world point is the exporter's: map_points.h as map_export.hip compiles it
#include "sim3_dev.h"
#include "map_points.h"
#pragma clang fp contract(off)
#include "compact_dev.h"

namespace {

constexpr int kSeg = 256;                     // grid columns per row segment (one wave, four rounds of 64)
constexpr int kTileRows = 8;                  // cell rows per k_mesh_cells workgroup: two per wave
constexpr int kPitch = kSeg + 8;              // staged floats per vertex row: 257 columns, a lead of <= 3 and a tail of <= 3
constexpr int kGroups = kPitch / kPts;        // 4-point load groups per staged row
constexpr int kLaunches = 5;                  // cells, used-vertex count, scan | vertex scatter, face scatter

struct Grid {
    int H, W, s, Hg, Wg, Hc, Wc;              // image, stride, vertex grid, cell grid
    int segF;                                 // row segments per cell row
};

struct MeshWs {
    Grid g;
    int64_t ntileV, nsegF, verts, cells;      // over all K keyframes: 1024-point tiles, cell-row segments
    int64_t offV, offF, remap, flags, bytes;  // byte offsets into ws
};

inline bool mesh_layout(int K, int H, int W, int stride, MeshWs &m) {
    if (K < 0 || H < 1 || W < 1 || stride < 1) return false;
    if ((int64_t)H * W > 0x7fffffff || (int64_t)K * H * W > 0x7fffffff) return false;
    Grid &g = m.g;
    g.H = H; g.W = W; g.s = stride;
    g.Hg = (int)(((int64_t)H + stride - 1) / stride);
    g.Wg = (int)(((int64_t)W + stride - 1) / stride);
    g.Hc = g.Hg - 1; g.Wc = g.Wg - 1;
    g.segF = m3_cdiv(g.Wc, kSeg);
    m.cells = (int64_t)K * g.Hc * g.Wc;
    if (2 * m.cells > 0x7fffffff) return false;
    if (K == 0 || g.Hc < 1 || g.Wc < 1) m.cells = 0;          // nothing to triangulate: the header alone
    m.verts = m.cells ? (int64_t)K * g.Hg * g.Wg : 0;
    m.ntileV = m.cells ? (int64_t)K * m3_cdiv((int64_t)H * W, kTile) : 0;
    m.nsegF = m.cells ? (int64_t)K * g.Hc * g.segF : 0;
    m.offV = kHdrWords * 4;
    m.offF = m.offV + (m.ntileV + 3) / 4 * 16;
    m.remap = m.offF + (m.nsegF + 3) / 4 * 16;
    m.flags = m.remap + (m.verts + 3) / 4 * 16;
    m.bytes = m.flags + (m.cells + 15) / 16 * 16;
    return true;
}

struct P3 { float x, y, z; };

__device__ __forceinline__ float norm2(const P3 &p) { return (p.x * p.x + p.y * p.y) + p.z * p.z; }

__device__ __forceinline__ bool edge_ok(const P3 &p, const P3 &q, float rp, float rq, float t2) {
    const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
    const float l2 = (dx * dx + dy * dy) + dz * dz;
    return l2 <= t2 * fminf(rp, rq);
}

// Validity of the <= 4 points t.n0 ... below nlim by the export rule, and their camera-frame coordinates into
// sx / sy / sz[at ...]; an invalid point is staged as NaN.
__device__ __forceinline__ void stage_points(const Tile &t, int nlim, const Pose<float> &T, float nk, int use_thresh,
                                             float thresh, float *__restrict__ sx, float *__restrict__ sy,
                                             float *__restrict__ sz, int at) {
    float avg[kPts];
    unsigned keep = conf_pass(t, nlim, nk, use_thresh, thresh, avg);
    float x[3 * kPts] = {};
    V3<float> p[kPts];
    if (keep) keep = world_points(t, T, keep, p, x);
#pragma unroll
    for (int j = 0; j < kPts; ++j) {
        if (t.n0 + j >= nlim) continue;
        const bool on = (keep >> j) & 1u;
        sx[at + j] = on ? x[3 * j] : __builtin_nanf("");
        sy[at + j] = on ? x[3 * j + 1] : 0.f;
        sz[at + j] = on ? x[3 * j + 2] : 0.f;
    }
}

// One workgroup per (keyframe, 8 cell rows, 256 cell columns): stage the 9 x 257 vertices, then two bits per cell
// (bit t = triangle t kept) to flags and the kept triangles of every cell-row segment to cntF.  DENSE (stride 1): a
// vertex row is a run of consecutive points, loaded in 4-point groups from the last multiple of 4 at or below its
// start (16-byte loads when N % 4 == 0 and the keyframe's arrays are 16-byte aligned); lead = the run's offset in
// its first group.  Otherwise one scalar load group of a single point per vertex.
template <bool DENSE>
__global__ void __launch_bounds__(kThreads) k_mesh_cells(const float *const *__restrict__ X,
                                                          const float *const *__restrict__ C,
                                                          const float *__restrict__ poses, const int32_t *__restrict__ Nk,
                                                          Grid g, int tilesY, int use_thresh, float thresh, float t2,
                                                          unsigned char *__restrict__ flags, int32_t *__restrict__ cntF) {
    __shared__ float sx[(kTileRows + 1) * kPitch], sy[(kTileRows + 1) * kPitch], sz[(kTileRows + 1) * kPitch];
    const int N = g.H * g.W;
    const int tx = blockIdx.x % g.segF, ty = (blockIdx.x / g.segF) % tilesY, k = blockIdx.x / (g.segF * tilesY);
    const int cy0 = ty * kTileRows, cx0 = tx * kSeg;
    const float *Xk = X[k], *Ck = C[k];
    const Pose<float> T = load_pose<float>(poses + 8 * k);
    const float nk = (float)Nk[k];
    if constexpr (DENSE) {
        for (int it = threadIdx.x; it < (kTileRows + 1) * kGroups; it += kThreads) {
            const int r = it / kGroups, y = cy0 + r;
            if (y >= g.H) break;
            const int row = y * g.W + cx0, end = y * g.W + min(cx0 + kSeg + 1, g.W);
            const int n0 = (row & ~3) + (it - r * kGroups) * kPts;
            if (n0 >= end) continue;
            stage_points(tile_at(k, n0, N, Xk, Ck), N, T, nk, use_thresh, thresh, sx, sy, sz,
                         r * kPitch + (n0 - (row & ~3)));
        }
    } else {
        for (int it = threadIdx.x; it < (kTileRows + 1) * (kSeg + 1); it += kThreads) {
            const int r = it / (kSeg + 1), c = it - r * (kSeg + 1);
            const int gy = cy0 + r, gx = cx0 + c;
            if (gy >= g.Hg) break;
            if (gx >= g.Wg) continue;
            const int n0 = gy * g.s * g.W + gx * g.s, nlim = n0 + 1;           // a group of one point: the scalar path
            stage_points(tile_at(k, n0, nlim, Xk, Ck), nlim, T, nk, use_thresh, thresh, sx, sy, sz, r * kPitch + c);
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int rr = 0; rr < kTileRows / 4; ++rr) {
        const int r = w * (kTileRows / 4) + rr, gy = cy0 + r;
        if (gy >= g.Hc) break;                                                  // wave-uniform
        const int lead0 = DENSE ? ((gy * g.W + cx0) & 3) : 0, lead1 = DENSE ? (((gy + 1) * g.W + cx0) & 3) : 0;
        int total = 0;
#pragma unroll
        for (int c0 = 0; c0 < kSeg; c0 += 64) {
            const int c = c0 + lane, gx = cx0 + c;
            unsigned f = 0;
            if (gx < g.Wc) {
                const int ia = r * kPitch + lead0 + c, ic = (r + 1) * kPitch + lead1 + c;
                const P3 a{sx[ia], sy[ia], sz[ia]}, b{sx[ia + 1], sy[ia + 1], sz[ia + 1]};
                const P3 cc{sx[ic], sy[ic], sz[ic]}, d{sx[ic + 1], sy[ic + 1], sz[ic + 1]};
                const float ra = norm2(a), rb = norm2(b), rc = norm2(cc), rd = norm2(d);
                const bool bc = edge_ok(b, cc, rb, rc, t2);
                if (bc && edge_ok(a, cc, ra, rc, t2) && edge_ok(b, a, rb, ra, t2)) f |= 1u;
                if (bc && edge_ok(cc, d, rc, rd, t2) && edge_ok(d, b, rd, rb, t2)) f |= 2u;
                flags[((size_t)k * g.Hc + gy) * g.Wc + gx] = (unsigned char)f;
            }
            total += __popcll(__ballot(f & 1u)) + __popcll(__ballot(f & 2u));
        }
        if (lane == 0) cntF[((size_t)k * g.Hc + gy) * g.segF + tx] = total;
    }
}

// Is vertex (gy, gx) of keyframe k referenced by a kept triangle?  Its up to six incident triangles: t = 1 of the cell
// up-left (corner d), both of the cell above (c), both of the cell to the left (b), t = 0 of its own cell (a).
__device__ __forceinline__ bool vertex_used(const unsigned char *__restrict__ flags, const Grid &g, int k, int gy, int gx) {
    const unsigned char *F = flags + (size_t)k * g.Hc * g.Wc;
    unsigned u = 0;
    if (gy > 0) {
        const unsigned char *row = F + (size_t)(gy - 1) * g.Wc;
        if (gx > 0) u |= row[gx - 1] & 2u;
        if (gx < g.Wc) u |= row[gx];
    }
    if (gy < g.Hc) {
        const unsigned char *row = F + (size_t)gy * g.Wc;
        if (gx > 0) u |= row[gx - 1];
        if (gx < g.Wc) u |= row[gx] & 1u;
    }
    return u != 0;
}

// Bits of the thread's four consecutive points that are grid vertices referenced by a kept triangle.
__device__ __forceinline__ unsigned used_bits(const unsigned char *__restrict__ flags, const Grid &g, const Tile &t) {
    const int N = g.H * g.W;
    unsigned keep = 0;
#pragma unroll
    for (int j = 0; j < kPts; ++j) {
        const int n = t.n0 + j;
        if (n >= N) continue;
        const int y = n / g.W, x = n - y * g.W;
        if (y % g.s || x % g.s) continue;
        if (vertex_used(flags, g, t.k, y / g.s, x / g.s)) keep |= 1u << j;
    }
    return keep;
}

// Used vertices per 1024-point tile: the export's grid, so that vertices come out in ascending source index.
__global__ void __launch_bounds__(kThreads) k_mesh_count_vertices(const unsigned char *__restrict__ flags, Grid g, int tiles,
                                                                   int32_t *__restrict__ cntV) {
    const Tile t = tile_of(tiles);
    int total;
    block_prefix(used_bits(flags, g, t), total);
    if (threadIdx.x == 0) cntV[blockIdx.x] = total;
}

// The wave's cell-row segment: seg -> (k, gy, first column); false beyond the last segment.
__device__ __forceinline__ bool segment_of(int64_t nseg, int rows, int segs, int64_t &seg, int &k, int &gy, int &gx0) {
    seg = (int64_t)blockIdx.x * (kThreads / M3_WAVE) + (threadIdx.x >> 6);
    if (seg >= nseg) return false;
    const int64_t row = seg / segs;
    gx0 = (int)(seg - row * segs) * kSeg;
    k = (int)(row / rows);
    gy = (int)(row - (int64_t)k * rows);
    return true;
}

// Used vertices to rows offV[tile] + rank inside the tile; remap[grid vertex] = its row.  The shape of k_export_scatter
// - a thread owns four consecutive points and takes their world points from one world_points call - so that the
// compiler sees the exporter's arithmetic in the exporter's context and the bytes are the exporter's.  Stride 1 takes
// 16-byte loads of X when the keyframe allows them; a larger stride reads only the points on the grid.  LAYOUT as there.
template <int LAYOUT>
__global__ void __launch_bounds__(kThreads) k_mesh_vertices(const float *const *__restrict__ X,
                                                             const void *const *__restrict__ img,
                                                             const float *__restrict__ poses, Grid g, int tiles,
                                                             const unsigned char *__restrict__ flags,
                                                             const int32_t *__restrict__ offs, int64_t V,
                                                             int32_t *__restrict__ remap, float *__restrict__ points,
                                                             unsigned char *__restrict__ colors, int64_t *__restrict__ index) {
    const int N = g.H * g.W;
    Tile t = tile_of(tiles);
    t.X = X[t.k];
    const void *Ik = img[t.k];
    t.vec = g.s == 1 && vec_ok(t.n0, N, t.X, t.X);                              // C is not read here
    // Validity was decided once, by k_mesh_cells; the count pass counted exactly these bits, so every one of them is
    // written and the finiteness result of this call is not consulted.
    const unsigned keep = used_bits(flags, g, t);
    V3<float> p[kPts];
    if (keep) world_points(t, load_pose<float>(poses + 8 * t.k), keep, p);
    int total;
    int64_t o = (int64_t)offs[blockIdx.x] + block_prefix(keep, total);
    if (!keep) return;
    unsigned char rgb[kPts][3];
    fetch_rgb<LAYOUT>(Ik, t, N, keep, rgb);
#pragma unroll
    for (int j = 0; j < kPts; ++j) {
        if (!((keep >> j) & 1u) || o >= V) continue;                            // o < V always holds for a ws from the same inputs
        store_row(o, p[j], rgb[j], (int64_t)t.k * N + t.n0 + j, points, colors, index);
        const int y = (t.n0 + j) / g.W, x = t.n0 + j - y * g.W;
        remap[((size_t)t.k * g.Hg + y / g.s) * g.Wg + x / g.s] = (int32_t)o;
        ++o;
    }
}

// Kept triangles of a cell-row segment to rows offF[seg] + rank in (gx, t) order, vertices through remap.
__global__ void __launch_bounds__(kThreads) k_mesh_faces(const unsigned char *__restrict__ flags, Grid g, int64_t nsegF,
                                                          const int32_t *__restrict__ offF, const int32_t *__restrict__ remap,
                                                          int64_t F, int32_t *__restrict__ faces) {
    int64_t seg;
    int k, gy, gx0;
    if (!segment_of(nsegF, g.Hc, g.segF, seg, k, gy, gx0)) return;
    int64_t base = offF[seg];
#pragma unroll 1
    for (int c0 = 0; c0 < kSeg; c0 += 64) {
        const int gx = gx0 + c0 + (threadIdx.x & 63);
        const unsigned f = gx < g.Wc ? flags[((size_t)k * g.Hc + gy) * g.Wc + gx] : 0u;
        const unsigned long long b0 = __ballot(f & 1u), b1 = __ballot(f & 2u);
        int64_t o = base + lanes_before(b0) + lanes_before(b1);
        base += __popcll(b0) + __popcll(b1);
        if (!f) continue;
        const int32_t *ra = remap + ((size_t)k * g.Hg + gy) * g.Wg + gx, *rc = ra + g.Wg;
        const int32_t a = ra[0], b = ra[1], c = rc[0], d = rc[1];              // d is read but unused when only t = 0 is kept
        if ((f & 1u) && o < F) {                                                // o < F always holds for a ws from the same inputs
            faces[3 * o] = a; faces[3 * o + 1] = c; faces[3 * o + 2] = b;
            ++o;
        }
        if ((f & 2u) && o < F) {
            faces[3 * o] = b; faces[3 * o + 1] = c; faces[3 * o + 2] = d;
        }
    }
}

inline bool mesh_args_ok(int K, int H, int W, int stride, int use_thresh, float edge_ratio, const void *ws,
                         int64_t ws_bytes, MeshWs &m) {
    return mesh_layout(K, H, W, stride, m) && (use_thresh == 0 || use_thresh == 1) && edge_ratio > 0.f && ws &&
           ((uintptr_t)ws & 15) == 0 && ws_bytes >= m.bytes;
}

}  // namespace

extern "C" {

int64_t m3_mesh_ws_bytes(int K, int H, int W, int stride) {
    MeshWs m;
    return mesh_layout(K, H, W, stride, m) ? m.bytes : 0;
}

int m3_mesh_launches(void) { return kLaunches; }

int m3_mesh_count(const float *const *X, const float *const *C, const float *poses, const int32_t *Nk, int K, int H, int W,
                  int stride, int use_thresh, float thresh, float edge_ratio, void *ws, int64_t ws_bytes, void *stream) {
    MeshWs m;
    M3_REQUIRE(mesh_args_ok(K, H, W, stride, use_thresh, edge_ratio, ws, ws_bytes, m));
    hipStream_t st = (hipStream_t)stream;
    char *p = (char *)ws;
    if (!m.cells) {
        M3_CHECK_HIP(hipMemsetAsync(ws, 0, kHdrWords * 4, st), "m3_mesh_count/memset");
        return M3_OK;
    }
    M3_REQUIRE(X && C && poses && Nk);
    const Grid &g = m.g;
    const int tilesY = m3_cdiv(g.Hc, kTileRows), blocks = K * tilesY * g.segF;
    const float t2 = edge_ratio * edge_ratio;
    unsigned char *flags = (unsigned char *)(p + m.flags);
    int32_t *cntV = (int32_t *)(p + m.offV), *cntF = (int32_t *)(p + m.offF);
    if (stride == 1)
        hipLaunchKernelGGL(k_mesh_cells<true>, dim3(blocks), dim3(kThreads), 0, st, X, C, poses, Nk, g, tilesY, use_thresh,
                           thresh, t2, flags, cntF);
    else
        hipLaunchKernelGGL(k_mesh_cells<false>, dim3(blocks), dim3(kThreads), 0, st, X, C, poses, Nk, g, tilesY, use_thresh,
                           thresh, t2, flags, cntF);
    const int tiles = m3_cdiv(g.H * g.W, kTile);
    hipLaunchKernelGGL(k_mesh_count_vertices, dim3(K * tiles), dim3(kThreads), 0, st, flags, g, tiles, cntV);
    launch_scan(st, (int32_t *)ws, ScanJob{cntV, m.ntileV}, ScanJob{cntF, m.nsegF});              // V to word 0, F to word 1
    M3_CHECK_LAUNCH("m3_mesh_count");
    return M3_OK;
}

int m3_mesh_scatter(const float *const *X, const float *const *C, const void *const *img, const float *poses,
                    const int32_t *Nk, int K, int H, int W, int stride, int use_thresh, float thresh, float edge_ratio,
                    int layout, void *ws, int64_t ws_bytes, int64_t V, int64_t F, float *vertices, uint8_t *colors,
                    int32_t *faces, int64_t *index, void *stream) {
    MeshWs m;
    M3_REQUIRE(mesh_args_ok(K, H, W, stride, use_thresh, edge_ratio, ws, ws_bytes, m));
    M3_REQUIRE(X && C && img && poses && Nk && vertices && colors && faces && m.cells);
    M3_REQUIRE(V >= 1 && V <= m.verts && F >= 1 && F <= 2 * m.cells);
    M3_REQUIRE(layout == M3_MAP_IMG_F32_CHW || layout == M3_MAP_IMG_U8_HWC);
    hipStream_t st = (hipStream_t)stream;
    char *p = (char *)ws;
    const Grid &g = m.g;
    const unsigned char *flags = (const unsigned char *)(p + m.flags);
    const int32_t *offV = (const int32_t *)(p + m.offV), *offF = (const int32_t *)(p + m.offF);
    int32_t *remap = (int32_t *)(p + m.remap);
    const int tiles = m3_cdiv(g.H * g.W, kTile);
    if (layout == M3_MAP_IMG_F32_CHW)
        hipLaunchKernelGGL(k_mesh_vertices<0>, dim3(K * tiles), dim3(kThreads), 0, st, X, img, poses, g, tiles, flags, offV, V,
                           remap, vertices, colors, index);
    else
        hipLaunchKernelGGL(k_mesh_vertices<1>, dim3(K * tiles), dim3(kThreads), 0, st, X, img, poses, g, tiles, flags, offV, V,
                           remap, vertices, colors, index);
    hipLaunchKernelGGL(k_mesh_faces, dim3(m3_cdiv(m.nsegF, kThreads / M3_WAVE)), dim3(kThreads), 0, st, flags, g, m.nsegF,
                       offF, remap, F, faces);
    M3_CHECK_LAUNCH("m3_mesh_scatter");
    return M3_OK;
}

}  // extern "C"
