// Inverse-pose table and observation planes of the keyframe map, shared by the multi-view consistency filter
// (consistency.hip) and the volumetric fusion (tsdf.hip): step 1 of the consistency rule, with
// the workspace that holds them and the launches that fill it (section 7s).
//
// Include it as consistency.hip does: map_points.h with contraction on (the exporter's context), then
// `#pragma clang fp contract(off)` and view_dev.h, in a file compiled with -ffp-contract=off.
#pragma once
#include "map_points.h"
#include "view_dev.h"

namespace {

constexpr int kInvStride = 16;                // floats per keyframe in the inverse-pose table: kViewWords, padded to 64 bytes

inline int64_t inv_bytes(int K) { return (int64_t)K * kInvStride * 4; }

// One thread per keyframe: the view_inverse of its pose.
__global__ void __launch_bounds__(kThreads) k_cons_inverse(const float *__restrict__ poses, int K, float *__restrict__ inv) {
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= K) return;
    float o[kInvStride];
    view_inverse(poses + 8 * k, o);
#pragma unroll
    for (int i = kViewWords; i < kInvStride; ++i) o[i] = 0.f;
#pragma unroll
    for (int i = 0; i < kInvStride; i += 4) *(float4 *)(inv + (size_t)kInvStride * k + i) = float4{o[i], o[i + 1], o[i + 2], o[i + 3]};
}

// Grid as k_export_count.  D[k][n] = X[k][n].z where the point passes the confidence test and z is finite and > z_min,
// else NaN.
__global__ void __launch_bounds__(kThreads) k_cons_plane(const float *const *__restrict__ X, const float *const *__restrict__ C,
                                                          const int32_t *__restrict__ Nk, int N, int tiles, int use_thresh,
                                                          float thresh, float z_min, float *__restrict__ D) {
    const Tile t = tile_of(N, tiles, X, C);
    if (t.n0 >= N) return;
    float avg[kPts];
    const unsigned pass = conf_pass(t, N, (float)Nk[t.k], use_thresh, thresh, avg);
    float x[3 * kPts];
    load_points(t.X, t, pass, x);                                                // only z is used
    float d[kPts];
#pragma unroll
    for (int j = 0; j < kPts; ++j) {
        const float z = x[3 * j + 2];
        d[j] = (((pass >> j) & 1u) && isfinite(z) && z > z_min) ? z : __builtin_nanf("");
    }
    float *Dk = D + (size_t)t.k * N + t.n0;
    if (t.vec) {
        *(float4 *)Dk = float4{d[0], d[1], d[2], d[3]};                          // D is 16-byte aligned and N % 4 == 0
    } else {
#pragma unroll
        for (int j = 0; j < kPts; ++j)
            if (t.n0 + j < N) Dk[j] = d[j];
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------
// An empty map is accepted by both passes: K == 0 with any grid.
inline bool map_or_empty_ok(int K, int N) { return (K == 0 && N >= 1) || map_shape_ok(K, N); }

// Workspace: the inverse-pose table, then the planes (both 16-byte aligned when ws is).  0 for a map that is not
// accepted, and for the empty one.
inline int64_t planes_ws_bytes(int K, int N) { return map_or_empty_ok(K, N) ? inv_bytes(K) + (int64_t)K * N * 4 : 0; }

struct Planes { float *inv, *D; };

inline Planes split_planes(void *ws, int K) { return Planes{(float *)ws, (float *)((char *)ws + inv_bytes(K))}; }

// The two launches that fill a Planes for K >= 1 keyframes of N points.
inline void launch_planes(const float *const *X, const float *const *C, const float *poses, const int32_t *Nk, int K, int N,
                          int use_thresh, float thresh, float z_min, const Planes &w, hipStream_t st) {
    const int tiles = m3_cdiv(N, kTile);
    hipLaunchKernelGGL(k_cons_inverse, dim3(m3_cdiv(K, kThreads)), dim3(kThreads), 0, st, poses, K, w.inv);
    hipLaunchKernelGGL(k_cons_plane, dim3(K * tiles), dim3(kThreads), 0, st, X, C, Nk, N, tiles, use_thresh, thresh, z_min, w.D);
}

}  // namespace
