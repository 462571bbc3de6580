// A pinhole view of the world, shared by the view passes (render.hip, raster.hip, consistency.hip, tsdf.hip; DESIGN.md
// section 7s): world point -> camera frame of a Sim(3) view -> image position -> nearest pixel, and the host's checks
// of a camera's arguments.  tests/render_twin.py (view_inverse, sources) restates the arithmetic.
//
// Include it with floating-point contraction OFF (after `#pragma clang fp contract(off)` in a file compiled with
// -ffp-contract=off): the float64 inverse, the fp32 transform, and the divide, multiply, add and floor of the projection
// are separately rounded operations.  That holds for every device function below.
#pragma once
#include "sim3_dev.h"

namespace {

constexpr int kViewWords = 13;                // rows of R_v^T (9), t_v (3), 1 / s_v

// Inverse of the view pose (t, q xyzw, s), formed in float64 and rounded to fp32.  The rotation is the quaternion
// formula of liegroups/so3.py without normalisation, as export.save_trajectory writes it.
__device__ __forceinline__ void view_inverse(const float *__restrict__ T, float *__restrict__ o) {
    const double x = T[3], y = T[4], z = T[5], w = T[6];
    o[0] = (float)(1.0 - 2.0 * (y * y + z * z)); o[1] = (float)(2.0 * (x * y + w * z)); o[2] = (float)(2.0 * (x * z - w * y));
    o[3] = (float)(2.0 * (x * y - w * z)); o[4] = (float)(1.0 - 2.0 * (x * x + z * z)); o[5] = (float)(2.0 * (y * z + w * x));
    o[6] = (float)(2.0 * (x * z + w * y)); o[7] = (float)(2.0 * (y * z - w * x)); o[8] = (float)(1.0 - 2.0 * (x * x + y * y));
    o[9] = T[0]; o[10] = T[1]; o[11] = T[2];
    o[12] = (float)(1.0 / (double)T[7]);
}

// c = (R_v^T (p - t_v)) * (1 / s_v) from the kViewWords of view_inverse.
__device__ __forceinline__ V3<float> view_point(const float *__restrict__ sv, const V3<float> &p) {
    const float inv_s = sv[12];
    const float dx = p.x - sv[9], dy = p.y - sv[10], dz = p.z - sv[11];
    return V3<float>{((sv[0] * dx + sv[1] * dy) + sv[2] * dz) * inv_s, ((sv[3] * dx + sv[4] * dy) + sv[5] * dz) * inv_s,
                     ((sv[6] * dx + sv[7] * dy) + sv[8] * dz) * inv_s};
}

// A pinhole camera.  Kernels take the four values as scalar arguments and form it in their first line.
struct Pinhole { float fx, fy, cx, cy; };

// Image position of a camera point: fx * (x / z) + cx in this grouping.  Integers are pixel centres.
__device__ __forceinline__ float image_u(const Pinhole &k, const V3<float> &c) { return k.fx * (c.x / c.z) + k.cx; }
__device__ __forceinline__ float image_v(const Pinhole &k, const V3<float> &c) { return k.fy * (c.y / c.z) + k.cy; }

// The nearest pixel, still a float: it may be huge or NaN.
__device__ __forceinline__ float nearest_pixel(float u) { return floorf(u + 0.5f); }

// near < z < far, strict; NaN fails.  near >= 0, so a z that passes is positive.
__device__ __forceinline__ bool in_depth(float z, float near, float far) { return z > near && z < far; }

// ---- host checks of a camera's arguments ----------------------------------------------------------------------------
// Focal lengths positive and finite.  The principal point must be finite for the passes that read keyframe images
// through it (finite_centre), and only not NaN for the renderers, which draw the background for an infinite one.
inline bool pinhole_ok(const Pinhole &k, bool finite_centre) {
    if (!(k.fx > 0.f && k.fy > 0.f && k.fx < INFINITY && k.fy < INFINITY)) return false;
    return finite_centre ? (k.cx - k.cx == 0.f && k.cy - k.cy == 0.f) : (k.cx == k.cx && k.cy == k.cy);
}

inline bool depth_range_ok(float near, float far) { return near >= 0.f && near < far; }

inline bool background_ok(int r, int g, int b) { return ((r | g | b) & ~255) == 0; }
inline unsigned pack_background(int r, int g, int b) { return (unsigned)r | ((unsigned)g << 8) | ((unsigned)b << 16); }

// A keyframe grid: a pixel coordinate is exact as a float and a pixel index fits an int.
inline bool grid_ok(int H, int W) {
    return H >= 1 && W >= 1 && H <= (1 << 24) && W <= (1 << 24) && (int64_t)H * W <= 0x7fffffff;
}

}  // namespace
