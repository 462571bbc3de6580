// Multi-view consistency filter of the keyframe map (mast3r_slam/consistency.py): every exporter
// candidate (k, n) is projected into the keyframes of its neighbour row and counted as supported (the neighbour saw the
// same depth there), in conflict (the neighbour saw through it) or neither.  inverse poses -> observation planes ->
// count; no atomics and no floating-point reductions, so two calls give identical bytes.  Nothing here waits for the
// host or allocates: poses are read from device memory and the call can be captured into a graph.
//
// Compiled with -ffp-contract=off: the camera transform, the projection and the depth test are separately rounded fp32
// operations (tests/consistency_twin.py restates them).  The world point is the exporter's: map_points.h is included
// with contraction on, as map_export.hip compiles it.
#include "common.h"
#pragma clang fp contract(fast)
#include "sim3_dev.h"
#include "map_points.h"
#pragma clang fp contract(off)
#include "view_dev.h"
#include "cons_planes.h"                        // k_cons_inverse, k_cons_plane: shared with tsdf.hip

namespace {

// An empty map is accepted (and nothing is launched for it).
inline bool shape_ok(int K, int N) { return (K == 0 && N >= 1) || map_shape_ok(K, N); }

// Grid as k_export_count: a workgroup belongs to one keyframe, a thread owns 4 consecutive points.  The neighbour loop is
// outermost; the neighbour index and its inverse pose depend on the workgroup and the slot alone, so they are read
// through scalar loads (readfirstlane keeps the addresses in SGPRs).  Per pair: the transform, one divide pair, one
// 4-byte gather from D.
__global__ void __launch_bounds__(kThreads) k_cons_count(const float *const *__restrict__ X, const float *const *__restrict__ C,
                                                          const float *__restrict__ poses, const int32_t *__restrict__ Nk,
                                                          int K, int N, int H, int W, int tiles, int use_thresh, float thresh,
                                                          float fx, float fy, float cx, float cy,
                                                          const int32_t *__restrict__ nbr, int V, float z_min, float rtol,
                                                          int min_views, int max_conflicts, const float *__restrict__ inv,
                                                          const float *__restrict__ D, uint8_t *__restrict__ support,
                                                          uint8_t *__restrict__ conflict, float *__restrict__ conf) {
    const Tile t = tile_of(N, tiles, X, C);
    if (t.n0 >= N) return;
    float avg[kPts];
    unsigned keep = conf_pass(t, N, (float)Nk[t.k], use_thresh, thresh, avg);
    V3<float> p[kPts];
    if (keep) keep = world_points(t, load_pose<float>(poses + 8 * t.k), keep, p);
    unsigned sup[kPts] = {0u, 0u, 0u, 0u}, con[kPts] = {0u, 0u, 0u, 0u};
    if (keep) {
        const float fW = (float)W, fH = (float)H;
        const int32_t *row = nbr + (size_t)t.k * V;
        for (int v = 0; v < V; ++v) {
            const int j = __builtin_amdgcn_readfirstlane(row[v]);
            if (j < 0 || j >= K || j == t.k) continue;
            const float *sv = inv + (size_t)kInvStride * j;
            const float *Dj = D + (size_t)j * N;
#pragma unroll
            for (int i = 0; i < kPts; ++i) {
                if (!((keep >> i) & 1u)) continue;
                const V3<float> c = view_point(sv, p[i]);
                if (!(c.z > z_min)) continue;                                    // NaN fails
                const float fu = floorf((fx * (c.x / c.z) + cx) + 0.5f), fv = floorf((fy * (c.y / c.z) + cy) + 0.5f);
                if (!(fu >= 0.f && fu < fW && fv >= 0.f && fv < fH)) continue;   // as floats: u may be huge or NaN
                const float d = Dj[(int)fv * W + (int)fu];
                if (!(d == d)) continue;                                         // j has no observation there
                if (fabsf(c.z - d) <= rtol * d) ++sup[i];
                else if (c.z < d) ++con[i];
            }
        }
    }
    float c[kPts];
    load_conf(t.C, t, N, c);                                                     // raw: the masked confidence is not averaged
    unsigned ws = 0u, wc = 0u;
#pragma unroll
    for (int i = 0; i < kPts; ++i) {
        const bool kept = ((keep >> i) & 1u) && (int)sup[i] >= min_views && (max_conflicts < 0 || (int)con[i] <= max_conflicts);
        if (!kept) c[i] = -INFINITY;
        ws |= sup[i] << (8 * i);
        wc |= con[i] << (8 * i);
    }
    const size_t o = (size_t)t.k * N + t.n0;
    if (t.vec) {                                                                 // N % 4 == 0: o is a multiple of 4
        *(unsigned *)(support + o) = ws;
        *(unsigned *)(conflict + o) = wc;
        *(float4 *)(conf + o) = float4{c[0], c[1], c[2], c[3]};
    } else {
#pragma unroll
        for (int i = 0; i < kPts; ++i) {
            if (t.n0 + i >= N) continue;
            support[o + i] = (uint8_t)sup[i];
            conflict[o + i] = (uint8_t)con[i];
            conf[o + i] = c[i];
        }
    }
}

}  // namespace

extern "C" {

int64_t m3_consistency_ws_bytes(int K, int N) {
    return shape_ok(K, N) ? inv_bytes(K) + (int64_t)K * N * 4 : 0;
}

int m3_consistency_launches(void) { return 3; }

int m3_consistency(const float *const *X, const float *const *C, const float *poses, const int32_t *Nk, int K, int H, int W,
                   int use_thresh, float thresh, float fx, float fy, float cx, float cy, const int32_t *nbr, int V,
                   float z_min, float depth_rtol, int min_views, int max_conflicts, void *ws, int64_t ws_bytes,
                   uint8_t *support, uint8_t *conflict, float *conf, void *stream) {
    M3_REQUIRE(H >= 1 && W >= 1 && H <= (1 << 24) && W <= (1 << 24) && (int64_t)H * W <= 0x7fffffff && shape_ok(K, H * W));
    M3_REQUIRE((use_thresh == 0 || use_thresh == 1) && V >= 0 && V <= 255 && (V == 0 || nbr || K == 0));
    M3_REQUIRE(fx > 0.f && fy > 0.f && fx < INFINITY && fy < INFINITY && cx - cx == 0.f && cy - cy == 0.f);
    M3_REQUIRE(z_min >= 0.f && z_min < INFINITY && depth_rtol > 0.f && depth_rtol < 1.f && min_views >= 0 && max_conflicts >= -1);
    if (K == 0) return M3_OK;
    const int N = H * W;
    M3_REQUIRE(X && C && poses && Nk && ws && support && conflict && conf);
    M3_REQUIRE(((uintptr_t)ws & 15) == 0 && ws_bytes >= m3_consistency_ws_bytes(K, N));
    M3_REQUIRE(((uintptr_t)support & 3) == 0 && ((uintptr_t)conflict & 3) == 0 && ((uintptr_t)conf & 15) == 0);
    hipStream_t st = (hipStream_t)stream;
    float *inv = (float *)ws;
    float *D = (float *)((char *)ws + inv_bytes(K));
    const int tiles = m3_cdiv(N, kTile);
    const dim3 grid(K * tiles), block(kThreads);
    hipLaunchKernelGGL(k_cons_inverse, dim3(m3_cdiv(K, kThreads)), block, 0, st, poses, K, inv);
    hipLaunchKernelGGL(k_cons_plane, grid, block, 0, st, X, C, Nk, N, tiles, use_thresh, thresh, z_min, D);
    hipLaunchKernelGGL(k_cons_count, grid, block, 0, st, X, C, poses, Nk, K, N, H, W, tiles, use_thresh, thresh, fx, fy, cx, cy,
                       nbr, V, z_min, depth_rtol, min_views, max_conflicts, inv, D, support, conflict, conf);
    M3_CHECK_LAUNCH("m3_consistency");
    return M3_OK;
}

}  // extern "C"
