// The source-point rule shared by every consumer of the keyframe map (map_export.hip, render.hip, mesh.hip,
// consistency.hip, intrinsics.hip): which points (k, n) of the keyframe tables are candidates, how a thread loads them,
// their world points, their colours and the output row of one.  A thread owns kPts consecutive points of one keyframe;
// a workgroup owns a kTile-point tile.
#pragma once
#include "common.h"
#include "sim3_dev.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPts = 4;                       // consecutive points per thread: one 16-byte load of C, three of X
constexpr int kTile = kThreads * kPts;        // points per workgroup

// K keyframes of N points fit one launch (int32 source indices, grid size).  K == 0 is the caller's to allow.
inline bool map_shape_ok(int K, int N) {
    return K >= 1 && N >= 1 && (int64_t)K * N <= 0x7fffffff && (int64_t)K * m3_cdiv(N, kTile) <= (1 << 30);
}

__device__ __forceinline__ bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// The 16-byte path: all four points from n0 on exist and the keyframe's arrays are 16-byte aligned.
__device__ __forceinline__ bool vec_ok(int n0, int N, const float *Xk, const float *Ck) {
    return n0 + kPts <= N && N % 4 == 0 && aligned16(Xk) && aligned16(Ck);
}

struct Tile {
    int k, n0;            // keyframe, first point of this thread
    const float *X, *C;   // the keyframe's arrays
    bool vec;             // vec_ok
};

// The four points from n0 on of a keyframe of N points.  A caller that has to restrict the 16-byte path clears vec.
__device__ __forceinline__ Tile tile_at(int k, int n0, int N, const float *Xk, const float *Ck) {
    return Tile{k, n0, Xk, Ck, vec_ok(n0, N, Xk, Ck)};
}

// The thread's place in a grid of K * tiles workgroups, keyframe-major ...
__device__ __forceinline__ Tile tile_of(int tiles) {
    Tile t;
    t.k = blockIdx.x / tiles;
    t.n0 = (blockIdx.x - t.k * tiles) * kTile + threadIdx.x * kPts;
    t.X = t.C = nullptr;
    t.vec = false;
    return t;
}

// ... and with the keyframe's arrays.
__device__ __forceinline__ Tile tile_of(int N, int tiles, const float *const *__restrict__ X,
                                        const float *const *__restrict__ C) {
    const Tile t = tile_of(tiles);
    return tile_at(t.k, t.n0, N, X[t.k], C[t.k]);
}

// The thread's four confidences; a point at or beyond N reads as 0.  Ck is t.C (and Xk below t.X): a parameter of its
// own, so that it is __restrict__ here as the tables are in the kernels.
__device__ __forceinline__ void load_conf(const float *__restrict__ Ck, const Tile &t, int N, float (&c)[kPts]) {
    if (t.vec) {
        const float4 v = *(const float4 *)(Ck + t.n0);
        c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < kPts; ++j) c[j] = t.n0 + j < N ? Ck[t.n0 + j] : 0.f;
    }
}

// The thread's twelve camera-frame coordinates.  The scalar path reads only the points whose bit is set in `want`
// (they must exist); the others are 0.
__device__ __forceinline__ void load_points(const float *__restrict__ Xk, const Tile &t, unsigned want,
                                            float (&x)[3 * kPts]) {
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
}

// Average confidence of the thread's points (C / N_k, IEEE divide) and the bits of those that pass the strict test.
__device__ __forceinline__ unsigned conf_pass(const Tile &t, int N, float nk, int use_thresh, float thresh,
                                              float (&avg)[kPts]) {
    float c[kPts];
    load_conf(t.C, t, N, c);
    unsigned pass = 0;
#pragma unroll
    for (int j = 0; j < kPts; ++j) {
        avg[j] = c[j] / nk;
        if (t.n0 + j < N && (!use_thresh || avg[j] > thresh)) pass |= 1u << j;
    }
    return pass;
}

// World points of the thread's points whose bit is set in `want`; returns the bits whose world point is finite.  x: the
// camera-frame coordinates they were computed from (load_points).
__device__ __forceinline__ unsigned world_points(const Tile &t, const Pose<float> &T, unsigned want, V3<float> (&p)[kPts],
                                                 float (&x)[3 * kPts]) {
    load_points(t.X, t, want, x);
    unsigned keep = 0;
#pragma unroll
    for (int j = 0; j < kPts; ++j) {
        p[j] = act(T, V3<float>{x[3 * j], x[3 * j + 1], x[3 * j + 2]});
        if (((want >> j) & 1u) && isfinite(p[j].x) && isfinite(p[j].y) && isfinite(p[j].z)) keep |= 1u << j;
    }
    return keep;
}

__device__ __forceinline__ unsigned world_points(const Tile &t, const Pose<float> &T, unsigned want,
                                                 V3<float> (&p)[kPts]) {
    float x[3 * kPts];
    return world_points(t, T, want, p, x);
}

__device__ __forceinline__ unsigned char to_u8(float v) {
    return (unsigned char)floorf(fminf(fmaxf(v, 0.f), 1.f) * 255.0f);        // fmaxf(NaN, 0) = 0
}

// Colour of point n of an image of N pixels.  LAYOUT 0: float32 [3,H,W] planes in [0,1]; 1: uint8 [H,W,3].
template <int LAYOUT>
__device__ __forceinline__ void fetch_rgb(const void *Ik, int N, size_t n, unsigned char (&rgb)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if constexpr (LAYOUT == 0) rgb[c] = to_u8(((const float *)Ik)[(size_t)c * N + n]);
        else rgb[c] = ((const unsigned char *)Ik)[3 * n + c];
    }
}

// Colours of the thread's points whose bit is set in `keep` (the others are 0 or the image's, nobody reads them): 16-byte
// or 12-byte loads on the thread's vector path when the image's address allows them, else point by point.
template <int LAYOUT>
__device__ __forceinline__ void fetch_rgb(const void *Ik, const Tile &t, int N, unsigned keep,
                                          unsigned char (&rgb)[kPts][3]) {
    if (LAYOUT == 0 && t.vec && aligned16(Ik)) {
        const float *I = (const float *)Ik;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float4 v = *(const float4 *)(I + (size_t)c * N + t.n0);
            rgb[0][c] = to_u8(v.x); rgb[1][c] = to_u8(v.y); rgb[2][c] = to_u8(v.z); rgb[3][c] = to_u8(v.w);
        }
    } else if (LAYOUT == 1 && t.vec && ((uintptr_t)Ik & 3) == 0) {             // 12 bytes from a 4-byte aligned address
        const unsigned *src = (const unsigned *)((const unsigned char *)Ik + (size_t)3 * t.n0);
        const unsigned w[3] = {src[0], src[1], src[2]};
#pragma unroll
        for (int b = 0; b < 12; ++b) rgb[b / 3][b % 3] = (unsigned char)(w[b / 4] >> (8 * (b % 4)));
    } else {
#pragma unroll
        for (int j = 0; j < kPts; ++j) {
            if ((keep >> j) & 1u) fetch_rgb<LAYOUT>(Ik, N, t.n0 + j, rgb[j]);
            else rgb[j][0] = rgb[j][1] = rgb[j][2] = 0;
        }
    }
}

// Output row o of a compacted cloud: world point, colour and (optional) source index.
__device__ __forceinline__ void store_row(int64_t o, const V3<float> &p, const unsigned char (&rgb)[3], int64_t source,
                                          float *__restrict__ points, unsigned char *__restrict__ colors,
                                          int64_t *__restrict__ index) {
    points[3 * o] = p.x; points[3 * o + 1] = p.y; points[3 * o + 2] = p.z;
    colors[3 * o] = rgb[0]; colors[3 * o + 1] = rgb[1]; colors[3 * o + 2] = rgb[2];
    if (index) index[o] = source;
}

}  // namespace
