// Per-vertex normals of a triangle mesh and vertex colours lit with them (mast3r_slam/normals.py).
// The rule is stated once, in include/m3slam.h; tests/normals_twin.py restates it in numpy.
//
// fill -> faces -> vertices, whatever V and F are.  A face adds its unit normal, scaled by 2^24 and rounded to an
// integer, to three int64 sums of each of its three vertices.  The only atomics are 64-bit integer adds, which commute:
// the sums depend neither on the order of the faces nor on the order of the threads, so two calls give identical bytes
// (a float atomic sum would not: DESIGN.md section 7k).  The vertex pass divides by the length in float64.
//
// ws: int64 [3][V], a plane per component.  collect_mesh and extract_surface emit faces in vertex order, so the rows one
// wave instruction adds to are mostly neighbours, and in a plane their words are contiguous (three sums side by side per
// vertex took 1.4 to 1.8 times as long in the face pass: profiles/normals_bench.md).  When at least half of a wave's
// lanes add to the same row (a fan around one hub) the wave sums them in registers and one lane adds.
//
// Compiled with -ffp-contract=off: every fp32 and float64 operation of the rule is rounded on its own.
#include "table_dev.h"
#pragma clang fp contract(off)

namespace {

constexpr int64_t kMaxRows = 0x7fffffff;      // V and F stay below 2^31
constexpr float kMinLen2 = 0x1p-80f;          // faces with a smaller squared length of e1 x e2 contribute nothing
constexpr float kScale = 16777216.0f;         // 2^24
constexpr int kShared = M3_WAVE / 2;          // lanes on one row from which the wave adds them up first

// Sum k of a vertex row: three planes of V sums, so that the adds of one wave instruction to neighbouring rows are
// contiguous.
__device__ __forceinline__ int64_t slot(int64_t row, int k, int64_t V) { return (int64_t)k * V + row; }

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// q of face f: false when the face contributes nothing (an index outside [0, V): nothing is dereferenced).
__device__ __forceinline__ bool face_normal(const float *__restrict__ vertices, const int32_t *__restrict__ faces, int64_t V,
                                            int64_t f, int32_t (&r)[3], long long (&q)[3]) {
    if (!load_face(faces, f, V, r)) return false;
    float p[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) p[i][k] = vertices[3 * (int64_t)r[i] + k];
    const float ax = p[1][0] - p[0][0], ay = p[1][1] - p[0][1], az = p[1][2] - p[0][2];
    const float bx = p[2][0] - p[0][0], by = p[2][1] - p[0][1], bz = p[2][2] - p[0][2];
    const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const float len2 = (nx * nx + ny * ny) + nz * nz;
    if (!(len2 >= kMinLen2) || len2 == INFINITY) return false;                   // NaN fails the first test
    const float len = sqrtf(len2);
    q[0] = (long long)rintf((nx / len) * kScale);
    q[1] = (long long)rintf((ny / len) * kScale);
    q[2] = (long long)rintf((nz / len) * kScale);
    return true;
}

// Adds q to the sums of row (on = this lane has something to add).  The lanes that share the row of the first such
// lane add together when they are at least kShared; every other lane adds on its own.
__device__ __forceinline__ void add_to_row(unsigned long long *__restrict__ sums, int64_t V, bool on, int32_t row,
                                           const long long (&q)[3]) {
    const unsigned long long any = __ballot(on);
    if (!any) return;                                                           // wave-uniform
    const int lead = __ffsll((long long)any) - 1;
    const int32_t first = __shfl(row, lead, 64);
    const unsigned long long same = __ballot(on && row == first);
    const bool together = __popcll(same) >= kShared;                            // wave-uniform
    if (together) {
        const bool mine = on && row == first;
        long long t[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = wave_sum(mine ? q[k] : 0ll);        // the total arrives in lane 0
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) atomicAdd(sums + slot(first, k, V), (unsigned long long)t[k]);
        }
        on = on && row != first;
    }
    if (on) {
#pragma unroll
        for (int k = 0; k < 3; ++k) atomicAdd(sums + slot(row, k, V), (unsigned long long)q[k]);
    }
}

__global__ void __launch_bounds__(kThreads) k_normals_faces(const float *__restrict__ vertices, const int32_t *__restrict__ faces,
                                                             int64_t V, int64_t F, unsigned long long *__restrict__ sums) {
    const int64_t f = row_of();
    int32_t r[3] = {0, 0, 0};
    long long q[3] = {0, 0, 0};
    const bool on = f < F && face_normal(vertices, faces, V, f, r, q);
    if (!__ballot(on)) return;                                                  // wave-uniform
#pragma unroll
    for (int i = 0; i < 3; ++i) add_to_row(sums, V, on, r[i], q);
}

__global__ void __launch_bounds__(kThreads) k_normals_vertices(const long long *__restrict__ sums, int64_t V,
                                                                float *__restrict__ normals) {
    const int64_t v = row_of();
    if (v >= V) return;
    const long long sx = sums[slot(v, 0, V)], sy = sums[slot(v, 1, V)], sz = sums[slot(v, 2, V)];
    float n[3] = {0.f, 0.f, 0.f};
    if (sx | sy | sz) {
        const double x = (double)sx, y = (double)sy, z = (double)sz;
        const double L = sqrt((x * x + y * y) + z * z);
        n[0] = (float)(x / L); n[1] = (float)(y / L); n[2] = (float)(z / L);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) normals[3 * v + k] = n[k];
}

__device__ __forceinline__ unsigned char to_level(float x) { return (unsigned char)fminf(fmaxf(x, 0.f), 255.f); }

struct Shade {
    int light, two_sided, mode;
    float lx, ly, lz, ambient;
    unsigned albedo;                           // r | g << 8 | b << 16
};

__global__ void __launch_bounds__(kThreads) k_mesh_shade(const float *__restrict__ vertices, const float *__restrict__ normals,
                                                          const uint8_t *__restrict__ colors, int64_t V,
                                                          const float *__restrict__ view_pose, Shade s,
                                                          uint8_t *__restrict__ out) {
    const int64_t v = row_of();
    if (v >= V) return;
    const float nx = normals[3 * v], ny = normals[3 * v + 1], nz = normals[3 * v + 2];
    if (s.mode == 1) {
        out[3 * v] = to_level(floorf((nx * 0.5f + 0.5f) * 255.f + 0.5f));
        out[3 * v + 1] = to_level(floorf((ny * 0.5f + 0.5f) * 255.f + 0.5f));
        out[3 * v + 2] = to_level(floorf((nz * 0.5f + 0.5f) * 255.f + 0.5f));
        return;
    }
    float lx = s.lx, ly = s.ly, lz = s.lz;
    if (s.light == 0) {
        lx = view_pose[0] - vertices[3 * v];
        ly = view_pose[1] - vertices[3 * v + 1];
        lz = view_pose[2] - vertices[3 * v + 2];
    }
    float d = ((nx * lx + ny * ly) + nz * lz) / sqrtf((lx * lx + ly * ly) + lz * lz);
    if (s.two_sided) d = fabsf(d);
    d = d > 0.f ? fminf(d, 1.f) : 0.f;                                           // NaN -> 0
    const float I = s.ambient + (1.f - s.ambient) * d;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float c = colors ? (float)colors[3 * v + k] : (float)((s.albedo >> (8 * k)) & 255u);
        out[3 * v + k] = to_level(floorf(c * I + 0.5f));
    }
}

inline bool aligned4(const void *p) { return ((uintptr_t)p & 3) == 0; }
inline bool finite(float x) { return x - x == 0.f; }

}  // namespace

extern "C" {

int64_t m3_mesh_normals_ws_bytes(int64_t V) {
    if (V < 0 || V > kMaxRows) return 0;
    return V ? pad16(24 * V) : 16;
}

int m3_mesh_normals_launches(void) { return 3; }

int m3_mesh_normals(const float *vertices, const int32_t *faces, int64_t V, int64_t F, void *ws, int64_t ws_bytes,
                    float *normals, void *stream) {
    const int64_t need = m3_mesh_normals_ws_bytes(V);
    M3_REQUIRE(need > 0 && F >= 0 && F <= kMaxRows && ws_ok(ws) && ws_bytes >= need);
    M3_REQUIRE((V == 0 || (vertices && normals)) && (F == 0 || faces));
    M3_REQUIRE(aligned4(vertices) && aligned4(faces) && aligned4(normals));
    hipStream_t st = (hipStream_t)stream;
    launch_fill(st, ws, need / 16, need / 16, 0, 0);                            // the workspace is a multiple of 16 bytes long
    // V = 0: no index is valid; F = 0: no thread has a face.  The launches are kept so that their number is fixed.
    hipLaunchKernelGGL(k_normals_faces, grid_of(F), dim3(kThreads), 0, st, vertices, faces, V, F, (unsigned long long *)ws);
    hipLaunchKernelGGL(k_normals_vertices, grid_of(V), dim3(kThreads), 0, st, (const long long *)ws, V, normals);
    M3_CHECK_LAUNCH("m3_mesh_normals");
    return M3_OK;
}

int m3_mesh_shade(const float *vertices, const float *normals, const uint8_t *colors, int64_t V, const float *view_pose,
                  int light, float lx, float ly, float lz, float ambient, int two_sided, int mode, int albedo_r,
                  int albedo_g, int albedo_b, uint8_t *out, void *stream) {
    M3_REQUIRE(V >= 0 && V <= kMaxRows && (V == 0 || (vertices && normals && out)));
    M3_REQUIRE(aligned4(vertices) && aligned4(normals) && aligned4(view_pose));
    M3_REQUIRE((mode == 0 || mode == 1) && (light == 0 || light == 1) && (two_sided == 0 || two_sided == 1));
    M3_REQUIRE(ambient >= 0.f && ambient <= 1.f && ((albedo_r | albedo_g | albedo_b) & ~255) == 0);       // NaN fails
    if (mode == 0 && light == 0) M3_REQUIRE(view_pose != nullptr);
    if (mode == 0 && light == 1) M3_REQUIRE(finite(lx) && finite(ly) && finite(lz) && (lx != 0.f || ly != 0.f || lz != 0.f));
    const Shade s{light, two_sided, mode, lx, ly, lz, ambient,
                  (unsigned)albedo_r | ((unsigned)albedo_g << 8) | ((unsigned)albedo_b << 16)};
    hipLaunchKernelGGL(k_mesh_shade, grid_of(V), dim3(kThreads), 0, (hipStream_t)stream, vertices, normals, colors, V, view_pose,
                       s, out);
    M3_CHECK_LAUNCH("m3_mesh_shade");
    return M3_OK;
}

}  // extern "C"
