// Triangle rasteriser (mast3r_slam/render.py render_mesh): a mesh (vertices, colours, faces as
// collect_mesh and extract_surface return them) drawn into an image from any pinhole camera, over the point renderer's
// z-buffer of 64-bit keys (zkey_dev.h; here bits of the interpolated depth << 32 | face index).
// clear -> project -> raster -> resolve, whatever V and F are.  Coverage is decided in int64 on a grid of 256 steps per
// pixel with a top-left rule, so faces that share an edge neither overlap nor leave a crack; the only atomics are 64-bit
// integer minima, which commute, so two calls give identical bytes.  Nothing here waits for the host: the view pose is
// read from device memory and the call can be captured into a graph.
//
// Compiled with -ffp-contract=off: the depth and the colour are separately rounded fp32 operations (tests/raster_twin.py
// restates them); the vertex stage projects through view_dev.h.
#include "common.h"
#pragma clang fp contract(off)
#include "view_dev.h"
#include "zkey_dev.h"

// Largest screen-clipped bounding box, in pixels, that a face's own lane walks; larger boxes are walked by the wave.
// Measured at 16, 64 and 256 (profiles/raster_bench.md, tools/bench_raster.py builds the other two with -D).
#ifndef M3_RASTER_WALK
#define M3_RASTER_WALK 64
#endif

namespace {

constexpr int kThreads = 256;
constexpr int kSub = 256;                     // sub-pixel steps per pixel
constexpr float kGuard = 16384.f;             // |u|, |v| beyond this many pixels: the vertex (and its faces) is dropped
constexpr int64_t kWalk = M3_RASTER_WALK;

// One per vertex: snapped screen position, camera depth, 1 = near < z < far and inside the guard band.
struct alignas(16) Rec { int sx, sy; float z; unsigned ok; };

__global__ void __launch_bounds__(kThreads) k_raster_project(const float *__restrict__ vertices, int64_t V,
                                                              const float *__restrict__ view, float fx, float fy, float cx,
                                                              float cy, float near, float far, Rec *__restrict__ recs) {
    const Pinhole pin{fx, fy, cx, cy};
    __shared__ float sv[kViewWords];
    if (threadIdx.x == 0) view_inverse(view, sv);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= V) return;
    const V3<float> c = view_point(sv, V3<float>{vertices[3 * i], vertices[3 * i + 1], vertices[3 * i + 2]});
    const float z = c.z;
    Rec r{0, 0, z, 0u};
    if (in_depth(z, near, far)) {
        const float u = image_u(pin, c), v = image_v(pin, c);
        if (fabsf(u) <= kGuard && fabsf(v) <= kGuard) {                         // NaN fails
            r.sx = (int)floorf(u * (float)kSub + 0.5f);
            r.sy = (int)floorf(v * (float)kSub + 0.5f);
            r.ok = 1u;
        }
    }
    *(int4 *)(recs + i) = int4{r.sx, r.sy, __float_as_int(r.z), (int)r.ok};
}

// A drawn face, oriented so that its doubled area A is positive (b and c swapped when it was not).
struct Face {
    int x[3], y[3];
    float z[3];
    int v[3];                                 // rows of the vertex arrays, in the oriented order
};

// Loads face f: false when an index lies outside [0, V) (nothing is dereferenced then), a vertex is not ok, the area
// is zero, or cull = 1 and the face is clockwise on the screen (A > 0 before orientation, y down).
__device__ __forceinline__ bool load_face(const int32_t *__restrict__ faces, const Rec *__restrict__ recs, int64_t V,
                                          int64_t f, int cull, Face &t, int64_t &A) {
    const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) return false;
    const int4 a = *(const int4 *)(recs + i0), b = *(const int4 *)(recs + i1), c = *(const int4 *)(recs + i2);
    if (!(a.w & b.w & c.w)) return false;
    A = (int64_t)(b.x - a.x) * (c.y - a.y) - (int64_t)(b.y - a.y) * (c.x - a.x);
    if (A == 0 || (cull && A > 0)) return false;
    const bool flip = A < 0;
    const int4 p = flip ? c : b, q = flip ? b : c;
    A = flip ? -A : A;
    t.x[0] = a.x; t.y[0] = a.y; t.z[0] = __int_as_float(a.z); t.v[0] = i0;
    t.x[1] = p.x; t.y[1] = p.y; t.z[1] = __int_as_float(p.z); t.v[1] = flip ? i2 : i1;
    t.x[2] = q.x; t.y[2] = q.y; t.z[2] = __int_as_float(q.z); t.v[2] = flip ? i1 : i2;
    return true;
}

// The three edge functions of an oriented face.  Edge i runs from vertex i+1 to vertex i+2: E_i = dx (Y - py) -
// dy (X - px) at the pixel centre (X, Y) = (256 x, 256 y), exact in int64 (|coordinates| <= 2^22 + 1).  A pixel is
// covered iff E_i >= lo_i for every i, lo_i = 0 on a top-left edge (dy < 0, or dy == 0 and dx > 0) and 1 elsewhere.
struct Edges {
    int64_t e[3], stepx[3], stepy[3];         // value at pixel (x0, y0); change per pixel in x and in y
    int lo[3];
};

__device__ __forceinline__ Edges edges_at(const int *x, const int *y, int x0, int y0) {
    Edges g;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int p = (i + 1) % 3, q = (i + 2) % 3;
        const int dx = x[q] - x[p], dy = y[q] - y[p];
        g.e[i] = (int64_t)dx * ((int64_t)kSub * y0 - y[p]) - (int64_t)dy * ((int64_t)kSub * x0 - x[p]);
        g.stepx[i] = -(int64_t)dy * kSub;
        g.stepy[i] = (int64_t)dx * kSub;
        g.lo[i] = (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1;
    }
    return g;
}

// Perspective-correct depth from the edge values of a covered pixel; l_i are the barycentric weights.
__device__ __forceinline__ float pixel_depth(const int64_t *e, float area, const float *iz, float *l) {
    l[0] = (float)e[0] / area; l[1] = (float)e[1] / area; l[2] = (float)e[2] / area;
    const float w = (l[0] * iz[0] + l[1] * iz[1]) + l[2] * iz[2];
    return 1.0f / w;
}

// Enters a pixel whose edge values are e into the key buffer when the face covers it.
__device__ __forceinline__ void draw_pixel(const int64_t *e, const int *lo, int64_t pix, float area, const float *iz,
                                           unsigned f, unsigned long long *keys) {
    if (e[0] < lo[0] || e[1] < lo[1] || e[2] < lo[2]) return;
    float l[3];
    const float z = pixel_depth(e, area, iz, l);
    key_min(keys + pix, ((unsigned long long)__float_as_uint(z) << 32) | f);
}

__device__ __forceinline__ int bcast(int v, int src) { return __builtin_amdgcn_readlane(v, src); }

// A lane per face; blockIdx.y is one of gridDim.y slices.  A face whose screen-clipped bounding box holds at most
// kWalk pixels is walked by its own lane, in slice 0.  The others are taken one after another by the whole wave, which
// walks the box in 8 x 8 blocks, a pixel per lane, and every slice takes its share of the rows of blocks: one
// screen-filling triangle must not serialise a million pixels on one lane, nor on one wave when the mesh is too small
// to fill the chip (the host picks the slices).  No lane leaves before the wave loop.
__global__ void __launch_bounds__(kThreads) k_raster_faces(const int32_t *__restrict__ faces, int64_t F,
                                                            const Rec *__restrict__ recs, int64_t V, int cull, int Hv,
                                                            int Wv, unsigned long long *keys) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    Face t{};
    int64_t A = 0;
    bool draw = f < F && load_face(faces, recs, V, f, cull, t, A);
    int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
    if (draw) {
        // pixel centres inside the box of the snapped vertices, clipped to the image: ceil(min / 256) ... floor(max / 256)
        x0 = max(0, (min(t.x[0], min(t.x[1], t.x[2])) + kSub - 1) >> 8);
        x1 = min(Wv - 1, max(t.x[0], max(t.x[1], t.x[2])) >> 8);
        y0 = max(0, (min(t.y[0], min(t.y[1], t.y[2])) + kSub - 1) >> 8);
        y1 = min(Hv - 1, max(t.y[0], max(t.y[1], t.y[2])) >> 8);
        draw = x1 >= x0 && y1 >= y0;
    }
    const int64_t box = draw ? (int64_t)(x1 - x0 + 1) * (y1 - y0 + 1) : 0;
    if (draw && box <= kWalk && blockIdx.y == 0) {
        const Edges g = edges_at(t.x, t.y, x0, y0);
        const float area = (float)A, iz[3] = {1.0f / t.z[0], 1.0f / t.z[1], 1.0f / t.z[2]};
        int64_t row[3] = {g.e[0], g.e[1], g.e[2]};
        for (int y = y0; y <= y1; ++y) {
            int64_t e[3] = {row[0], row[1], row[2]};
            for (int x = x0; x <= x1; ++x) {
                draw_pixel(e, g.lo, (int64_t)y * Wv + x, area, iz, (unsigned)f, keys);
#pragma unroll
                for (int i = 0; i < 3; ++i) e[i] += g.stepx[i];
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) row[i] += g.stepy[i];
        }
    }
    unsigned long long todo = __ballot(draw && box > kWalk);
    const int lane = threadIdx.x & 63, lx = lane & 7, ly = lane >> 3;
    while (todo) {
        const int src = __ffsll(todo) - 1;
        todo &= todo - 1;
        int bx[3], by[3];
        float bz[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            bx[i] = bcast(t.x[i], src);
            by[i] = bcast(t.y[i], src);
            bz[i] = __int_as_float(bcast(__float_as_int(t.z[i]), src));
        }
        const int X0 = bcast(x0, src), X1 = bcast(x1, src), Y0 = bcast(y0, src), Y1 = bcast(y1, src);
        const unsigned face = (unsigned)(f - lane + src);
        const int64_t area2 = (int64_t)(bx[1] - bx[0]) * (by[2] - by[0]) - (int64_t)(by[1] - by[0]) * (bx[2] - bx[0]);
        const float area = (float)area2, iz[3] = {1.0f / bz[0], 1.0f / bz[1], 1.0f / bz[2]};
        const Edges g = edges_at(bx, by, X0, Y0);
        // this lane's pixel of the first block; the most an edge value grows from a block's first pixel to a corner
        int64_t mine[3], reach[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            mine[i] = g.e[i] + g.stepx[i] * lx + g.stepy[i] * ly;
            reach[i] = 7 * (max(g.stepx[i], (int64_t)0) + max(g.stepy[i], (int64_t)0));
        }
        for (int oy = 8 * (int)blockIdx.y; Y0 + oy <= Y1; oy += 8 * (int)gridDim.y) {
            for (int ox = 0; X0 + ox <= X1; ox += 8) {
                int64_t off[3], e[3];         // wave-uniform: the block's offset from the first block
                bool out = false;             // an edge function negative at all four corners: no pixel of the block is covered
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    off[i] = g.stepx[i] * ox + g.stepy[i] * oy;
                    out = out || g.e[i] + off[i] + reach[i] < 0;
                    e[i] = mine[i] + off[i];
                }
                if (out) continue;
                const int x = X0 + ox + lx, y = Y0 + oy + ly;
                if (x <= X1 && y <= Y1) draw_pixel(e, g.lo, (int64_t)y * Wv + x, area, iz, face, keys);
            }
        }
    }
}

// As k_render_resolve, and for the same reason not a shared frame.  A thread owns 4 consecutive output pixels.  The winning face is loaded again and its edge functions recomputed at
// the pixel, exactly; the colour is the perspective-correct blend of its vertex colours.
__global__ void __launch_bounds__(kThreads) k_raster_resolve(const unsigned long long *__restrict__ keys,
                                                              const int32_t *__restrict__ faces,
                                                              const Rec *__restrict__ recs, int64_t V,
                                                              const unsigned char *__restrict__ colors, int Wv, int64_t P,
                                                              unsigned bg, unsigned char *__restrict__ rgb,
                                                              float *__restrict__ depth, int64_t *__restrict__ index) {
    const int64_t i0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
    if (i0 >= P) return;
    const bool vec = i0 + 4 <= P && ((uintptr_t)rgb & 3) == 0 && ((uintptr_t)depth & 15) == 0 && ((uintptr_t)index & 15) == 0;
    unsigned long long key[4];
    if (vec) {
        const ulonglong2 a = *(const ulonglong2 *)(keys + i0), b = *(const ulonglong2 *)(keys + i0 + 2);
        key[0] = a.x; key[1] = a.y; key[2] = b.x; key[3] = b.y;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) key[j] = i0 + j < P ? keys[i0 + j] : kNoKey;
    }
    unsigned char c[4][3];
    float z[4];
    int64_t src[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j][0] = (unsigned char)bg; c[j][1] = (unsigned char)(bg >> 8); c[j][2] = (unsigned char)(bg >> 16);
        z[j] = INFINITY;
        src[j] = -1;
        Face t{};
        int64_t A = 0;
        if (key[j] == kNoKey || !load_face(faces, recs, V, (int64_t)(unsigned)key[j], 0, t, A)) continue;
        const int64_t i = i0 + j;
        const Edges g = edges_at(t.x, t.y, (int)(i % Wv), (int)(i / Wv));
        const float iz[3] = {1.0f / t.z[0], 1.0f / t.z[1], 1.0f / t.z[2]};
        float l[3];
        z[j] = pixel_depth(g.e, (float)A, iz, l);
        src[j] = (int64_t)(unsigned)key[j];
        const float m0 = l[0] * iz[0] * z[j], m1 = l[1] * iz[1] * z[j], m2 = l[2] * iz[2] * z[j];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float c0 = (float)colors[3 * (int64_t)t.v[0] + ch], c1 = (float)colors[3 * (int64_t)t.v[1] + ch],
                        c2 = (float)colors[3 * (int64_t)t.v[2] + ch];
            const float s = floorf(((m0 * c0 + m1 * c1) + m2 * c2) + 0.5f);
            c[j][ch] = (unsigned char)fminf(fmaxf(s, 0.f), 255.f);
        }
    }
    if (vec) {
        unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
        for (int b = 0; b < 12; ++b) w[b / 4] |= (unsigned)c[b / 3][b % 3] << (8 * (b % 4));
        unsigned *dst = (unsigned *)(rgb + 3 * i0);
        dst[0] = w[0]; dst[1] = w[1]; dst[2] = w[2];
        *(float4 *)(depth + i0) = float4{z[0], z[1], z[2], z[3]};
        if (index) {
            *(longlong2 *)(index + i0) = longlong2{src[0], src[1]};
            *(longlong2 *)(index + i0 + 2) = longlong2{src[2], src[3]};
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i0 + j >= P) continue;
            rgb[3 * (i0 + j)] = c[j][0]; rgb[3 * (i0 + j) + 1] = c[j][1]; rgb[3 * (i0 + j) + 2] = c[j][2];
            depth[i0 + j] = z[j];
            if (index) index[i0 + j] = src[j];
        }
    }
}

constexpr int kFillGroups = 1024;             // workgroups of k_raster_faces that keep 256 CUs busy
constexpr int64_t kMaxRows = 2147483647;      // V and F: the index type of faces, and the low half of a key

}  // namespace

extern "C" {

int64_t m3_raster_ws_bytes(int64_t V, int Hv, int Wv) {
    if (m3_render_ws_bytes(Hv, Wv) == 0 || V < 0 || V > kMaxRows) return 0;
    return (V * 16 + (int64_t)Hv * Wv * 8 + 15) & ~(int64_t)15;
}

int m3_raster_launches(int64_t F) { return F > 0 ? 4 : 2; }

int m3_raster_mesh(const float *vertices, const uint8_t *colors, const int32_t *faces, int64_t V, int64_t F,
                   const float *view_pose, float fx, float fy, float cx, float cy, int Hv, int Wv, float near, float far,
                   int cull, int bg_r, int bg_g, int bg_b, void *ws, int64_t ws_bytes, uint8_t *rgb, float *depth,
                   int64_t *index, void *stream) {
    const int64_t need = m3_raster_ws_bytes(V, Hv, Wv);
    M3_REQUIRE(need > 0 && F >= 0 && F <= kMaxRows && ws && rgb && depth);
    M3_REQUIRE((V == 0 || (vertices && colors)) && (F == 0 || (faces && view_pose)));        // an empty mesh is drawn
    M3_REQUIRE(((uintptr_t)ws & 15) == 0 && ws_bytes >= need && (cull == 0 || cull == 1));
    const Pinhole pin{fx, fy, cx, cy};
    M3_REQUIRE(pinhole_ok(pin, false) && depth_range_ok(near, far));           // an infinite cx draws the background
    M3_REQUIRE(background_ok(bg_r, bg_g, bg_b));
    hipStream_t st = (hipStream_t)stream;
    Rec *recs = (Rec *)ws;                                                      // V records, then the keys: both 16-byte aligned
    unsigned long long *keys = (unsigned long long *)(recs + V);
    const int64_t P = (int64_t)Hv * Wv;
    launch_key_clear(keys, P, st);
    if (F > 0) {
        // V = 0: no index is valid; the two launches are kept so that the count depends on F alone
        hipLaunchKernelGGL(k_raster_project, dim3(V ? m3_cdiv(V, kThreads) : 1), dim3(kThreads), 0, st, vertices, V, view_pose,
                           fx, fy, cx, cy, near, far, recs);
        // a mesh too small to fill the chip shares the rows of its large faces among up to 64 slices of workgroups
        const int groups = m3_cdiv(F, kThreads), slices = groups >= kFillGroups ? 1 : min(64, kFillGroups / groups);
        hipLaunchKernelGGL(k_raster_faces, dim3(groups, slices), dim3(kThreads), 0, st, faces, F, recs, V, cull, Hv, Wv, keys);
    }
    const unsigned bg = pack_background(bg_r, bg_g, bg_b);
    hipLaunchKernelGGL(k_raster_resolve, dim3(m3_cdiv(P, 4 * kThreads)), dim3(kThreads), 0, st, keys, faces, recs, V, colors,
                       Wv, P, bg, rgb, depth, index);
    M3_CHECK_LAUNCH("m3_raster_mesh");
    return M3_OK;
}

}  // extern "C"
