// Volumetric fusion of the keyframe map (mast3r_slam/fusion.py): the keyframes' pointmaps are
// averaged into one truncated signed distance field on a dense voxel grid, and one connected surface mesh is extracted
// from it by naive surface nets.  No atomics and no floating-point reductions across threads: a voxel is owned by one
// thread, output rows come from an ordered compaction (compact_dev.h), so two calls give identical bytes.  Nothing here
// allocates; the integration reads the poses from device memory, waits for nothing and can be captured into a graph.
//
// Compiled with -ffp-contract=off: every fp32 operation below is separately rounded and the divides are IEEE
// (tests/tsdf_twin.py restates them in numpy float32 and expects the device's bits).  map_points.h is included with
// contraction on, as consistency.hip includes it; nothing of it that is used here has an operation to contract.
//
// ---- integration rule ------------------------------------------------------------------------------------------------
// Inputs: the keyframe tables (X float32 [K,N,3] in each keyframe's own camera frame, C float32 [K,N], img, poses
// float32 [K,8], N_k), the common grid H x W (N = H * W), a pinhole (fx, fy, cx, cy) of that grid, thr (or none), z_min,
// and a volume: origin fp32 [3], voxel size vs > 0, trunc > 0 and dims Dx, Dy, Dz, each in 2 ... 1024 with
// Dx * Dy * Dz <= 2^30.
//   observation plane   D[j][m] = X_j[m].z when point (j, m) passes the exporter's confidence test (C / N_j > thr: fp32
//                       divide, strict, NaN fails; thr none: no test), that z is finite and z > z_min; otherwise NaN.
//                       This is exactly step 1 of the consistency rule.
//   voxel (iz, iy, ix)  centre p.x = origin.x + ((float)ix + 0.5f) * vs, likewise y and z.  It holds sum = 0.f, n = 0
//                       and the colour sums r = g = b = 0, cn = 0 as uint32.
//   for j = 0 .. K-1    in ascending order, every keyframe:
//                       c = view_point(view_inverse(T_j), p) as in view_dev.h.  Skip unless c.z > z_min (strict, NaN
//                       fails).
//                       px = floorf((fx * (c.x / c.z) + cx) + 0.5f), py likewise.  Skip unless 0 <= px < W and
//                       0 <= py < H, compared as floats before converting to int.
//                       d = D[j][py * W + px].  Skip if d is NaN.
//                       sdf = (d - c.z) * s_j, s_j the pose's scale in fp32 (camera units to world units).  Skip unless
//                       sdf >= -trunc: the voxel is occluded in j.
//                       t = fminf(sdf / trunc, 1.f); sum += t; n += 1.  A voxel far in front of the surface counts as
//                       free space with t = 1: this carves away floating outliers.
//                       If sdf <= trunc: add the colour of pixel (py, px) of keyframe j (the export's colour rule:
//                       uint8 passed through, float (uint8)floorf(min(max(v, 0), 1) * 255.0f)) to r, g, b; cn += 1.
//   outputs             tsdf float32 [Dz,Dy,Dx] = sum / (float)n, or 1.f when n == 0; weight int32 [Dz,Dy,Dx] = n;
//                       color uint8 [Dz,Dy,Dx,3] = (2 * r + cn) / (2 * cn) in integer division per channel, or 0 when
//                       cn == 0; colored uint8 [Dz,Dy,Dx] = (cn > 0), the bit the extraction's colour rule needs.
// Every fp32 operation is separately rounded, and the divides are IEEE.
//
// ---- extraction rule (naive surface nets) ----------------------------------------------------------------------------
// Inputs: tsdf, weight, color, colored, origin, vs and min_weight >= 1.
//   valid voxel         weight >= min_weight.       inside voxel: tsdf < 0 (strict: a value of 0 is outside).
//   cell (z, y, x)      for z < Dz-1, y < Dy-1, x < Dx-1, with the 8 corner voxels (z+dz, y+dy, x+dx).  Active iff all 8
//                       corners are valid and are neither all inside nor all outside.
//   vertex              one per active cell, in ascending (z, y, x).  Walk the 12 cell edges - the 4 x-edges by
//                       (dz,dy) = (0,0),(0,1),(1,0),(1,1); then the 4 y-edges by (dz,dx); then the 4 z-edges by (dy,dx)
//                       - and add the crossing point of every edge whose ends differ in "inside" to acc = 0 (per
//                       component, in that order).  An edge from corner a to b = a + e_d has tt = Fa / (Fa - Fb); its
//                       crossing point is a's 0/1 offsets as floats, with tt along d.  local = acc / (float)count;
//                       world.x = origin.x + (((float)x + 0.5f) + local.x) * vs, likewise y and z.  Colour per channel:
//                       the rounded integer mean over the corners with colored set, (2 * sum + m) / (2 * m), or 0 when
//                       there is none.
//   faces               visit every grid edge from voxel (z, y, x) along d, d in the order x, y, z.  It yields faces when
//                       its ends differ in "inside" and its four surrounding cells all exist and are active: cells
//                       (z-1..z, y-1..y, x) for d = x, (z-1..z, y, x-1..x) for d = y, (z, y-1..y, x-1..x) for d = z.
//                       With (u, v, d) right-handed - d=x: (y,z), d=y: (z,x), d=z: (x,y) - the cells at (du,dv) =
//                       (-1,-1),(0,-1),(0,0),(-1,0) are q0..q3.  First end inside: (q0,q1,q2),(q0,q2,q3); otherwise
//                       (q3,q2,q1),(q3,q1,q0).  Face normals then point to the free-space side.  Faces come in
//                       ascending (z, y, x, d, triangle).
//   outputs             vertices float32 [V,3], colors uint8 [V,3], faces int32 [F,3] (rows of the vertex arrays).
//
// Passes.  A thread owns the voxel with the linear index i = (iz * Dy + iy) * Dx + ix (x fastest: loads and stores of a
// wave are consecutive), a workgroup 256 consecutive voxels; ascending i IS the output order of vertices (the cell whose
// lowest corner is i) and of faces (the edges that start at i), so the ordered compaction of compact_dev.h applies as it
// does to the exporter's tiles.  k_tsdf_cells leaves one byte per voxel (active cell, inside, valid) and the active
// cells per workgroup; everything after it that decides anything is integer work on those bytes.
#include "common.h"
#pragma clang fp contract(fast)
#include "sim3_dev.h"
#include "map_points.h"
#pragma clang fp contract(off)
#include "view_dev.h"
#include "cons_planes.h"
#include "compact_dev.h"

namespace {

constexpr int kIntegrateLaunches = 3;         // inverse poses, observation planes, voxels
constexpr int kExtractLaunches = 5;           // cells, edge count, scan | vertex scatter, face scatter
constexpr int kMaxDim = 1024;
constexpr int64_t kMaxVoxels = (int64_t)1 << 30;
constexpr unsigned kActive = 1u, kInside = 2u, kValid = 4u;     // the flag byte of a voxel

struct Vol {
    int Dx, Dy, Dz, total;                    // total = Dx * Dy * Dz <= 2^30
    float ox, oy, oz, vs;
};

inline bool finite_f(float v) { return v - v == 0.f; }

inline bool dims_ok(int Dx, int Dy, int Dz) {
    return Dx >= 2 && Dy >= 2 && Dz >= 2 && Dx <= kMaxDim && Dy <= kMaxDim && Dz <= kMaxDim &&
           (int64_t)Dx * Dy * Dz <= kMaxVoxels;
}

inline bool vol_ok(float ox, float oy, float oz, float vs, int Dx, int Dy, int Dz, Vol &v) {
    if (!dims_ok(Dx, Dy, Dz) || !finite_f(ox) || !finite_f(oy) || !finite_f(oz) || !(vs > 0.f) || !finite_f(vs)) return false;
    v = Vol{Dx, Dy, Dz, Dx * Dy * Dz, ox, oy, oz, vs};
    return true;
}

// The thread's voxel: false beyond the volume.
__device__ __forceinline__ bool voxel_of(const Vol &v, int &i, int &iz, int &iy, int &ix) {
    i = blockIdx.x * kThreads + threadIdx.x;                                     // < 2^30 + 256
    if (i >= v.total) return false;
    const int row = i / v.Dx;
    ix = i - row * v.Dx;
    iz = row / v.Dy;
    iy = row - iz * v.Dy;
    return true;
}

// One thread per voxel.  The keyframe loop is outermost; the inverse pose, the scale and the image pointer depend on j
// alone, so they come through wave-uniform (scalar) loads.  Per used pair: the transform, one divide pair, one 4-byte
// gather from D, one divide by trunc and one colour gather.  The lookup is k_cons_count's, written out in both and not
// shared as one observe(): see the comment there.
template <int LAYOUT>
__global__ void __launch_bounds__(kThreads) k_tsdf_voxels(const void *const *__restrict__ img, const float *__restrict__ poses,
                                                           int K, int N, int H, int W, float fx, float fy, float cx, float cy,
                                                           float z_min, Vol vol, float trunc, const float *__restrict__ inv,
                                                           const float *__restrict__ D, float *__restrict__ tsdf,
                                                           int32_t *__restrict__ weight, uint8_t *__restrict__ color,
                                                           uint8_t *__restrict__ colored) {
    int i, iz, iy, ix;
    if (!voxel_of(vol, i, iz, iy, ix)) return;
    const V3<float> p{vol.ox + ((float)ix + 0.5f) * vol.vs, vol.oy + ((float)iy + 0.5f) * vol.vs,
                      vol.oz + ((float)iz + 0.5f) * vol.vs};
    const Pinhole pin{fx, fy, cx, cy};
    const float fW = (float)W, fH = (float)H, lo = -trunc;
    float sum = 0.f;
    unsigned n = 0u, r = 0u, g = 0u, b = 0u, cn = 0u;
    for (int j = 0; j < K; ++j) {
        const float *sv = inv + (size_t)kInvStride * j;
        const V3<float> c = view_point(sv, p);
        if (!(c.z > z_min)) continue;                                            // NaN fails
        const float fu = nearest_pixel(image_u(pin, c)), fv = nearest_pixel(image_v(pin, c));
        if (!(fu >= 0.f && fu < fW && fv >= 0.f && fv < fH)) continue;           // as floats: u may be huge or NaN
        const int m = (int)fv * W + (int)fu;
        const float d = D[(size_t)j * N + m];
        if (!(d == d)) continue;                                                 // j has no observation there
        const float sdf = (d - c.z) * poses[8 * j + 7];
        if (!(sdf >= lo)) continue;                                              // occluded in j (NaN fails)
        sum += fminf(sdf / trunc, 1.f);
        ++n;
        if (sdf <= trunc) {
            unsigned char rgb[3];
            fetch_rgb<LAYOUT>(img[j], N, (size_t)m, rgb);
            r += rgb[0]; g += rgb[1]; b += rgb[2];
            ++cn;
        }
    }
    tsdf[i] = n ? sum / (float)n : 1.f;
    weight[i] = (int32_t)n;
    uint8_t *o = color + (size_t)3 * i;
    o[0] = cn ? (uint8_t)((2u * r + cn) / (2u * cn)) : 0;
    o[1] = cn ? (uint8_t)((2u * g + cn) / (2u * cn)) : 0;
    o[2] = cn ? (uint8_t)((2u * b + cn) / (2u * cn)) : 0;
    if (colored) colored[i] = cn ? 1 : 0;
}

// ---- extraction ------------------------------------------------------------------------------------------------------
struct ExtractWs {
    int64_t nblk, offV, offF, remap, flags, bytes;     // workgroups; byte offsets into ws
};

// Face-yielding edges are counted in int32: at most 3 per voxel.
inline bool extract_layout(int Dx, int Dy, int Dz, ExtractWs &m) {
    if (!dims_ok(Dx, Dy, Dz)) return false;
    const int64_t total = (int64_t)Dx * Dy * Dz;
    if (3 * total > 0x7fffffff) return false;
    m.nblk = (total + kThreads - 1) / kThreads;
    m.offV = kHdrWords * 4;
    m.offF = m.offV + (m.nblk + 3) / 4 * 16;
    m.remap = m.offF + (m.nblk + 3) / 4 * 16;
    m.flags = m.remap + (total + 3) / 4 * 16;
    m.bytes = m.flags + (total + 15) / 16 * 16;
    return true;
}

// The flag byte of every voxel - valid, inside, and whether the cell whose lowest corner it is is active - and the
// active cells of every workgroup.  The 8 corners are read from global memory: a wave's corner loads are 64
// consecutive floats of 4 rows, the x + 1 neighbour shares its cache lines and the y + 1 / z + 1 rows are the next
// workgroups' own rows (why no LDS tile).
__global__ void __launch_bounds__(kThreads) k_tsdf_cells(const float *__restrict__ tsdf, const int32_t *__restrict__ weight,
                                                          Vol vol, int min_weight, unsigned char *__restrict__ flags,
                                                          int32_t *__restrict__ cntV) {
    int i, iz, iy, ix;
    unsigned f = 0u;
    if (voxel_of(vol, i, iz, iy, ix)) {
        const int sy = vol.Dx, sz = vol.Dx * vol.Dy;
        if (weight[i] >= min_weight) f |= kValid;
        if (tsdf[i] < 0.f) f |= kInside;
        if (ix + 1 < vol.Dx && iy + 1 < vol.Dy && iz + 1 < vol.Dz) {
            // eight independent loads, no short-circuit between them; tsdf is read only where all corners are valid
            int lowest = weight[i];
#pragma unroll
            for (int c = 1; c < 8; ++c) lowest = min(lowest, weight[i + (c & 1) + ((c >> 1) & 1) * sy + (c >> 2) * sz]);
            if (lowest >= min_weight) {
                int in = 0;
#pragma unroll
                for (int c = 0; c < 8; ++c) in += tsdf[i + (c & 1) + ((c >> 1) & 1) * sy + (c >> 2) * sz] < 0.f ? 1 : 0;
                if (in > 0 && in < 8) f |= kActive;
            }
        }
        flags[i] = (unsigned char)f;
    }
    int total;
    block_prefix(f & kActive, total);
    if (threadIdx.x == 0) cntV[blockIdx.x] = total;
}

// Bits d = 0, 1, 2 (x, y, z): the grid edge from voxel i along d yields faces.  A cell beyond the upper faces of the
// volume has no active bit, so only the lower neighbours need a bounds test.
__device__ __forceinline__ unsigned edge_bits(const unsigned char *__restrict__ flags, const Vol &vol, int i, int iz, int iy,
                                              int ix) {
    const int sy = vol.Dx, sz = vol.Dx * vol.Dy;
    const unsigned self = flags[i];
    if (!(self & kActive)) return 0u;                                            // cell (z, y, x) surrounds all three edges
    unsigned e = 0u;
    if (iz >= 1 && iy >= 1 && ((self ^ flags[i + 1]) & kInside) &&              // an active cell has x + 1 < Dx
        (flags[i - sy] & flags[i - sz] & flags[i - sz - sy] & kActive)) e |= 1u;
    if (iz >= 1 && ix >= 1 && ((self ^ flags[i + sy]) & kInside) &&
        (flags[i - 1] & flags[i - sz] & flags[i - sz - 1] & kActive)) e |= 2u;
    if (iy >= 1 && ix >= 1 && ((self ^ flags[i + sz]) & kInside) &&
        (flags[i - 1] & flags[i - sy] & flags[i - sy - 1] & kActive)) e |= 4u;
    return e;
}

__global__ void __launch_bounds__(kThreads) k_tsdf_count_edges(const unsigned char *__restrict__ flags, Vol vol,
                                                                int32_t *__restrict__ cntF) {
    int i, iz, iy, ix;
    const unsigned e = voxel_of(vol, i, iz, iy, ix) ? edge_bits(flags, vol, i, iz, iy, ix) : 0u;
    int total;
    block_prefix(e, total);
    if (threadIdx.x == 0) cntF[blockIdx.x] = total;
}

// Active cells to rows offV[workgroup] + rank; remap[cell] = its row.
__global__ void __launch_bounds__(kThreads) k_tsdf_vertices(const float *__restrict__ tsdf, const uint8_t *__restrict__ color,
                                                             const uint8_t *__restrict__ colored, Vol vol,
                                                             const unsigned char *__restrict__ flags,
                                                             const int32_t *__restrict__ offs, int64_t V,
                                                             int32_t *__restrict__ remap, float *__restrict__ vertices,
                                                             uint8_t *__restrict__ colors) {
    int i, iz, iy, ix;
    const bool on = voxel_of(vol, i, iz, iy, ix) && (flags[i] & kActive);
    int total;
    const int64_t o = (int64_t)offs[blockIdx.x] + block_prefix(on ? 1u : 0u, total);
    if (!on || o >= V) return;                                                   // o < V always holds for a ws from the same inputs
    const int sy = vol.Dx, sz = vol.Dx * vol.Dy;
    float F[8];
    unsigned cs[3] = {0u, 0u, 0u}, m = 0u;
#pragma unroll
    for (int c = 0; c < 8; ++c) {                                                // corner c = dz * 4 + dy * 2 + dx
        const int q = i + (c & 1) + ((c >> 1) & 1) * sy + (c >> 2) * sz;
        F[c] = tsdf[q];
        if (!colored || colored[q]) {
            cs[0] += color[(size_t)3 * q]; cs[1] += color[(size_t)3 * q + 1]; cs[2] += color[(size_t)3 * q + 2];
            ++m;
        }
    }
    float ax = 0.f, ay = 0.f, az = 0.f;
    int count = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        const int d = e >> 2, s = (e >> 1) & 1, t = e & 1;                       // direction; the two fixed offsets in (z, y, x) order
        const int dz = d == 2 ? 0 : s, dy = d == 1 ? 0 : (d == 2 ? s : t), dx = d == 0 ? 0 : t;
        const int a = dz * 4 + dy * 2 + dx, b = a + (d == 0 ? 1 : d == 1 ? 2 : 4);
        const float Fa = F[a], Fb = F[b];
        if ((Fa < 0.f) == (Fb < 0.f)) continue;
        const float tt = Fa / (Fa - Fb);
        ax += d == 0 ? tt : (float)dx;
        ay += d == 1 ? tt : (float)dy;
        az += d == 2 ? tt : (float)dz;
        ++count;
    }
    const float cnt = (float)count;
    vertices[3 * o] = vol.ox + (((float)ix + 0.5f) + ax / cnt) * vol.vs;
    vertices[3 * o + 1] = vol.oy + (((float)iy + 0.5f) + ay / cnt) * vol.vs;
    vertices[3 * o + 2] = vol.oz + (((float)iz + 0.5f) + az / cnt) * vol.vs;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) colors[3 * o + ch] = m ? (uint8_t)((2u * cs[ch] + m) / (2u * m)) : 0;
    remap[i] = (int32_t)o;
}

// Face-yielding edges to rows 2 * (offF[workgroup] + rank) and the row after it, vertices through remap.
__global__ void __launch_bounds__(kThreads) k_tsdf_faces(Vol vol, const unsigned char *__restrict__ flags,
                                                          const int32_t *__restrict__ offs, const int32_t *__restrict__ remap,
                                                          int64_t F, int32_t *__restrict__ faces) {
    int i, iz, iy, ix;
    const unsigned e = voxel_of(vol, i, iz, iy, ix) ? edge_bits(flags, vol, i, iz, iy, ix) : 0u;
    int total;
    int64_t o = 2 * ((int64_t)offs[blockIdx.x] + block_prefix(e, total));
    if (!e) return;
    const int sy = vol.Dx, sz = vol.Dx * vol.Dy;
    const bool first_in = flags[i] & kInside;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        if (!((e >> d) & 1u) || o + 2 > F) continue;                             // o + 2 <= F always holds for a ws from the same inputs
        const int su = d == 0 ? sy : d == 1 ? sz : 1, sv = d == 0 ? sz : d == 1 ? 1 : sy;   // (u, v, d) right-handed
        const int32_t q0 = remap[i - su - sv], q1 = remap[i - sv], q2 = remap[i], q3 = remap[i - su];
        int32_t *f = faces + 3 * o;
        if (first_in) {
            f[0] = q0; f[1] = q1; f[2] = q2; f[3] = q0; f[4] = q2; f[5] = q3;
        } else {
            f[0] = q3; f[1] = q2; f[2] = q1; f[3] = q3; f[4] = q1; f[5] = q0;
        }
        o += 2;
    }
}

}  // namespace

extern "C" {

int64_t m3_tsdf_integrate_ws_bytes(int K, int N) { return planes_ws_bytes(K, N); }

int m3_tsdf_integrate_launches(void) { return kIntegrateLaunches; }

int m3_tsdf_integrate(const float *const *X, const float *const *C, const void *const *img, const float *poses,
                      const int32_t *Nk, int K, int H, int W, int use_thresh, float thresh, int layout, float fx, float fy,
                      float cx, float cy, float z_min, float ox, float oy, float oz, float voxel_size, float trunc, int Dx,
                      int Dy, int Dz, void *ws, int64_t ws_bytes, float *tsdf, int32_t *weight, uint8_t *color,
                      uint8_t *colored, void *stream) {
    Vol vol;
    const Pinhole pin{fx, fy, cx, cy};
    M3_REQUIRE(grid_ok(H, W) && map_or_empty_ok(K, H * W));                      // an empty map writes the unobserved volume
    M3_REQUIRE((use_thresh == 0 || use_thresh == 1) && (layout == M3_MAP_IMG_F32_CHW || layout == M3_MAP_IMG_U8_HWC));
    M3_REQUIRE(pinhole_ok(pin, true));
    M3_REQUIRE(z_min >= 0.f && z_min < INFINITY && trunc > 0.f && trunc < INFINITY);
    M3_REQUIRE(vol_ok(ox, oy, oz, voxel_size, Dx, Dy, Dz, vol));
    M3_REQUIRE(tsdf && weight && color && ((uintptr_t)tsdf & 3) == 0 && ((uintptr_t)weight & 3) == 0);
    const int N = H * W;
    if (K > 0) {
        M3_REQUIRE(X && C && img && poses && Nk && ws);
        M3_REQUIRE(((uintptr_t)ws & 15) == 0 && ws_bytes >= planes_ws_bytes(K, N));
    }
    hipStream_t st = (hipStream_t)stream;
    const Planes w = K > 0 ? split_planes(ws, K) : Planes{nullptr, nullptr};     // an empty map: ws may be null
    const dim3 block(kThreads), vgrid(m3_cdiv(vol.total, kThreads));
    if (K > 0) launch_planes(X, C, poses, Nk, K, N, use_thresh, thresh, z_min, w, st);
    if (layout == M3_MAP_IMG_F32_CHW)
        hipLaunchKernelGGL(k_tsdf_voxels<0>, vgrid, block, 0, st, img, poses, K, N, H, W, fx, fy, cx, cy, z_min, vol, trunc, w.inv,
                           w.D, tsdf, weight, color, colored);
    else
        hipLaunchKernelGGL(k_tsdf_voxels<1>, vgrid, block, 0, st, img, poses, K, N, H, W, fx, fy, cx, cy, z_min, vol, trunc, w.inv,
                           w.D, tsdf, weight, color, colored);
    M3_CHECK_LAUNCH("m3_tsdf_integrate");
    return M3_OK;
}

int64_t m3_tsdf_extract_ws_bytes(int Dx, int Dy, int Dz) {
    ExtractWs m;
    return extract_layout(Dx, Dy, Dz, m) ? m.bytes : 0;
}

int m3_tsdf_extract_launches(void) { return kExtractLaunches; }

int m3_tsdf_extract_count(const float *tsdf, const int32_t *weight, int Dx, int Dy, int Dz, int min_weight, void *ws,
                          int64_t ws_bytes, void *stream) {
    ExtractWs m;
    Vol vol;
    M3_REQUIRE(extract_layout(Dx, Dy, Dz, m) && vol_ok(0.f, 0.f, 0.f, 1.f, Dx, Dy, Dz, vol) && min_weight >= 1);
    M3_REQUIRE(tsdf && weight && ws && ((uintptr_t)tsdf & 3) == 0 && ((uintptr_t)weight & 3) == 0);
    M3_REQUIRE(((uintptr_t)ws & 15) == 0 && ws_bytes >= m.bytes);
    hipStream_t st = (hipStream_t)stream;
    char *p = (char *)ws;
    unsigned char *flags = (unsigned char *)(p + m.flags);
    int32_t *cntV = (int32_t *)(p + m.offV), *cntF = (int32_t *)(p + m.offF);
    const dim3 grid((unsigned)m.nblk), block(kThreads);
    hipLaunchKernelGGL(k_tsdf_cells, grid, block, 0, st, tsdf, weight, vol, min_weight, flags, cntV);
    hipLaunchKernelGGL(k_tsdf_count_edges, grid, block, 0, st, flags, vol, cntF);
    launch_scan(st, (int32_t *)ws, ScanJob{cntV, m.nblk}, ScanJob{cntF, m.nblk});                 // V to word 0, F / 2 to word 1
    M3_CHECK_LAUNCH("m3_tsdf_extract_count");
    return M3_OK;
}

int m3_tsdf_extract_scatter(const float *tsdf, const int32_t *weight, const uint8_t *color, const uint8_t *colored, float ox,
                            float oy, float oz, float voxel_size, int Dx, int Dy, int Dz, int min_weight, void *ws,
                            int64_t ws_bytes, int64_t V, int64_t F, float *vertices, uint8_t *colors, int32_t *faces,
                            void *stream) {
    ExtractWs m;
    Vol vol;
    M3_REQUIRE(extract_layout(Dx, Dy, Dz, m) && vol_ok(ox, oy, oz, voxel_size, Dx, Dy, Dz, vol) && min_weight >= 1);
    M3_REQUIRE(tsdf && weight && color && ws && vertices && colors && faces);
    M3_REQUIRE(((uintptr_t)tsdf & 3) == 0 && ((uintptr_t)vertices & 3) == 0 && ((uintptr_t)faces & 3) == 0);
    M3_REQUIRE(((uintptr_t)ws & 15) == 0 && ws_bytes >= m.bytes);
    M3_REQUIRE(V >= 1 && V <= vol.total && F >= 2 && F % 2 == 0 && F <= 6 * (int64_t)vol.total);
    hipStream_t st = (hipStream_t)stream;
    char *p = (char *)ws;
    const unsigned char *flags = (const unsigned char *)(p + m.flags);
    const int32_t *offV = (const int32_t *)(p + m.offV), *offF = (const int32_t *)(p + m.offF);
    int32_t *remap = (int32_t *)(p + m.remap);
    const dim3 grid((unsigned)m.nblk), block(kThreads);
    hipLaunchKernelGGL(k_tsdf_vertices, grid, block, 0, st, tsdf, color, colored, vol, flags, offV, V, remap, vertices, colors);
    hipLaunchKernelGGL(k_tsdf_faces, grid, block, 0, st, vol, flags, offF, remap, F, faces);
    M3_CHECK_LAUNCH("m3_tsdf_extract_scatter");
    return M3_OK;
}

}  // extern "C"
