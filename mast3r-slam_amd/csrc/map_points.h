// The source-point rule shared by the map export (map_export.hip) and the headless renderer (render.hip): which points
// (k, n) of the keyframe tables are candidates, their world points and their colours.  A thread owns kPts consecutive
// points of one keyframe; a workgroup owns a kTile-point tile.
#pragma once
#include "common.h"
#include "sim3_dev.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPts = 4;                       // consecutive points per thread: one 16-byte load of C, three of X
constexpr int kTile = kThreads * kPts;        // points per workgroup

__device__ __forceinline__ bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

struct Tile {
    int k, n0;            // keyframe, first point of this thread
    bool vec;             // 16-byte path: all four points exist and the keyframe's arrays are 16-byte aligned
};

__device__ __forceinline__ Tile tile_of(int N, int tiles) {
    Tile t;
    t.k = blockIdx.x / tiles;
    t.n0 = (blockIdx.x - t.k * tiles) * kTile + threadIdx.x * kPts;
    t.vec = false;
    return t;
}

// Average confidence of the thread's points (C / N_k, IEEE divide) and the bits of those that pass the strict test.
__device__ __forceinline__ unsigned conf_pass(const float *__restrict__ Ck, const Tile &t, int N, float nk, int use_thresh,
                                              float thresh, float (&avg)[kPts]) {
    float c[kPts];
    if (t.vec) {
        const float4 v = *(const float4 *)(Ck + t.n0);
        c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < kPts; ++j) c[j] = t.n0 + j < N ? Ck[t.n0 + j] : 0.f;
    }
    unsigned pass = 0;
#pragma unroll
    for (int j = 0; j < kPts; ++j) {
        avg[j] = c[j] / nk;
        if (t.n0 + j < N && (!use_thresh || avg[j] > thresh)) pass |= 1u << j;
    }
    return pass;
}

// World points of the thread's points whose bit is set in `want`; returns the bits whose world point is finite.
__device__ __forceinline__ unsigned world_points(const float *__restrict__ Xk, const Tile &t, const Pose<float> &T,
                                                 unsigned want, V3<float> (&p)[kPts]) {
    float x[3 * kPts];
    if (t.vec) {
        const float4 *src = (const float4 *)(Xk + (size_t)3 * t.n0);
        const float4 a = src[0], b = src[1], c = src[2];
        x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
        x[8] = c.x; x[9] = c.y; x[10] = c.z; x[11] = c.w;
    } else {
#pragma unroll
        for (int j = 0; j < kPts; ++j) {
            const bool on = (want >> j) & 1u;
#pragma unroll
            for (int d = 0; d < 3; ++d) x[3 * j + d] = on ? Xk[(size_t)3 * (t.n0 + j) + d] : 0.f;
        }
    }
    unsigned keep = 0;
#pragma unroll
    for (int j = 0; j < kPts; ++j) {
        p[j] = act(T, V3<float>{x[3 * j], x[3 * j + 1], x[3 * j + 2]});
        if (((want >> j) & 1u) && isfinite(p[j].x) && isfinite(p[j].y) && isfinite(p[j].z)) keep |= 1u << j;
    }
    return keep;
}

__device__ __forceinline__ unsigned char to_u8(float v) {
    return (unsigned char)floorf(fminf(fmaxf(v, 0.f), 1.f) * 255.0f);        // fmaxf(NaN, 0) = 0
}

}  // namespace
