// World point -> camera frame of a Sim(3) view, shared by the renderer (render.hip) and the multi-view consistency
// filter (consistency.hip).  DESIGN.md section 7d; tests/render_twin.py (view_inverse, sources) restates it.
//
// Include it with floating-point contraction OFF (after `#pragma clang fp contract(off)` in a file compiled with
// -ffp-contract=off): the float64 inverse and the fp32 transform are separately rounded operations.
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

}  // namespace
