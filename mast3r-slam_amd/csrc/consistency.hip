// Multi-view consistency filter of the keyframe map (mast3r_slam/consistency.py): every exporter
// candidate (k, n) is projected into the keyframes of its neighbour row and counted as supported (the neighbour saw the
// same depth there), in conflict (the neighbour saw through it) or neither.  inverse poses -> observation planes ->
// count; no atomics and no floating-point reductions, so two calls give identical bytes.  Nothing here waits for the
// host or allocates: poses are read from device memory and the call can be captured into a graph.
//
// Compiled with -ffp-contract=off: the camera transform, the projection (view_dev.h) and the depth test are separately
// rounded fp32 operations (tests/consistency_twin.py restates them); planes and workspace are cons_planes.h's (DESIGN.md
// section 7s).  The world point is the exporter's: map_points.h is included with contraction on, as map_export.hip
// compiles it.
#include "common.h"
#pragma clang fp contract(fast)
#include "sim3_dev.h"
#include "map_points.h"
#pragma clang fp contract(off)
#include "view_dev.h"
#include "cons_planes.h"                        // k_cons_inverse, k_cons_plane: shared with tsdf.hip

namespace {

// Grid as k_export_count: a workgroup belongs to one keyframe, a thread owns 4 consecutive points.  The neighbour loop is
// outermost; the neighbour index and its inverse pose depend on the workgroup and the slot alone, so they are read
// through scalar loads (readfirstlane keeps the addresses in SGPRs).  Per pair: the transform, one divide pair, one
// 4-byte gather from D.  The lookup (z_min gate, bounds test, gather, NaN test) is written out here and in k_tsdf_voxels
// and not shared as one observe(): every shape of such a function changed this loop's instructions.
__global__ void __launch_bounds__(kThreads) k_cons_count(const float *const *__restrict__ X, const float *const *__restrict__ C,
                                                          const float *__restrict__ poses, const int32_t *__restrict__ Nk,
                                                          int K, int N, int H, int W, int tiles, int use_thresh, float thresh,
                                                          float fx, float fy, float cx, float cy,
                                                          const int32_t *__restrict__ nbr, int V, float z_min, float rtol,
                                                          int min_views, int max_conflicts, const float *__restrict__ inv,
                                                          const float *__restrict__ D, uint8_t *__restrict__ support,
                                                          uint8_t *__restrict__ conflict, float *__restrict__ conf) {
    const Pinhole pin{fx, fy, cx, cy};
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
                const float fu = nearest_pixel(image_u(pin, c)), fv = nearest_pixel(image_v(pin, c));
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

int64_t m3_consistency_ws_bytes(int K, int N) { return planes_ws_bytes(K, N); }

int m3_consistency_launches(void) { return 3; }

int m3_consistency(const float *const *X, const float *const *C, const float *poses, const int32_t *Nk, int K, int H, int W,
                   int use_thresh, float thresh, float fx, float fy, float cx, float cy, const int32_t *nbr, int V,
                   float z_min, float depth_rtol, int min_views, int max_conflicts, void *ws, int64_t ws_bytes,
                   uint8_t *support, uint8_t *conflict, float *conf, void *stream) {
    const Pinhole pin{fx, fy, cx, cy};
    M3_REQUIRE(grid_ok(H, W) && map_or_empty_ok(K, H * W));                      // an empty map launches nothing
    M3_REQUIRE((use_thresh == 0 || use_thresh == 1) && V >= 0 && V <= 255 && (V == 0 || nbr || K == 0));
    M3_REQUIRE(pinhole_ok(pin, true));
    M3_REQUIRE(z_min >= 0.f && z_min < INFINITY && depth_rtol > 0.f && depth_rtol < 1.f && min_views >= 0 && max_conflicts >= -1);
    if (K == 0) return M3_OK;
    const int N = H * W;
    M3_REQUIRE(X && C && poses && Nk && ws && support && conflict && conf);
    M3_REQUIRE(((uintptr_t)ws & 15) == 0 && ws_bytes >= planes_ws_bytes(K, N));
    M3_REQUIRE(((uintptr_t)support & 3) == 0 && ((uintptr_t)conflict & 3) == 0 && ((uintptr_t)conf & 15) == 0);
    hipStream_t st = (hipStream_t)stream;
    const Planes w = split_planes(ws, K);
    launch_planes(X, C, poses, Nk, K, N, use_thresh, thresh, z_min, w, st);
    const int tiles = m3_cdiv(N, kTile);
    hipLaunchKernelGGL(k_cons_count, dim3(K * tiles), dim3(kThreads), 0, st, X, C, poses, Nk, K, N, H, W, tiles, use_thresh,
                       thresh, fx, fy, cx, cy, nbr, V, z_min, depth_rtol, min_views, max_conflicts, w.inv, w.D, support, conflict, conf);
    M3_CHECK_LAUNCH("m3_consistency");
    return M3_OK;
}

}  // extern "C"
