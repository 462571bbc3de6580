// The streaming loop of a Gauss-Newton accumulation kernel: every lane walks its points, adds each point's sums in fp32 and
// folds them into float64 accumulators.  Only loads, control flow and the fold live here; the per-point arithmetic stays
// with its kernel.  k_gn_blocks<MODE> (gn_rays.hip) runs on all of it; k_track_accum<Model> (tracking.hip) keeps the same
// loop written out (see there) and takes only kSums from here.
#pragma once
#include "sim3_dev.h"

constexpr int kSums = 36;              // 28 (H upper) + 7 (g) + 1 (cost or count): the row m3_block_reduce36 reduces

// May four consecutive points come in as 16-byte accesses (one dword for their four validity bytes)?
template <class... P>
__device__ __forceinline__ bool vec16_ok(int count, const uint8_t *valid, const P *...streams) {
    return (count % 4 == 0) && ((... | reinterpret_cast<size_t>(streams)) % 16 == 0) && (reinterpret_cast<size_t>(valid) % 4 == 0);
}

// Four packed xyz points (three dwordx4) and the validity byte of point k within the group's dword.
__device__ __forceinline__ void unpack4(const float4 &a, const float4 &b, const float4 &c, V3<float> (&p)[4]) {
    p[0] = {a.x, a.y, a.z}; p[1] = {a.w, b.x, b.y}; p[2] = {b.z, b.w, c.x}; p[3] = {c.y, c.z, c.w};
}
__device__ __forceinline__ bool valid4(unsigned v, int k) { return v & (0xffu << (8 * k)); }

template <int S> __device__ __forceinline__ void fold_sums(const float (&h)[S], double (&acc)[S]) {
#pragma unroll
    for (int i = 0; i < S; ++i) acc[i] += (double)h[i];
}

// Groups first, first + stride, ... < groups, four consecutive points each.  load(g, G&) fetches group g's registers (a
// plain struct G); body(g, const G&, h) adds the <= 4 points' sums into the zeroed fp32 h.  The next group's loads are
// issued before this group's arithmetic; one float64 fold per group (36 conversions + adds per FOUR points).
template <int S, class G, class Load, class Body>
__device__ __forceinline__ void walk_groups(int groups, int first, int stride, double (&acc)[S], Load load, Body body) {
    G next;
    int gi = first;
    if (gi < groups) load(gi, next);
    while (gi < groups) {
        const G cur = next;
        const int nx = gi + stride;
        if (nx < groups) load(nx, next);                      // in flight under the arithmetic below
        float h[S];
#pragma unroll
        for (int i = 0; i < S; ++i) h[i] = 0.f;
        body(gi, cur, h);
        fold_sums(h, acc);
        gi = nx;
    }
}

// The one-point loop for sizes and pointers that do not allow 16-byte accesses: body(n, h) adds point n's sums.
template <int S, class Body>
__device__ __forceinline__ void walk_points(int N, int first, int stride, double (&acc)[S], Body body) {
    for (int n = first; n < N; n += stride) {
        float h[S];
#pragma unroll
        for (int i = 0; i < S; ++i) h[i] = 0.f;
        body(n, h);
        fold_sums(h, acc);
    }
}
