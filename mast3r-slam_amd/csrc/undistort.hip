// Lens undistortion (mast3r_slam/camera.py): bilinear remap of an interleaved 8-bit RGB image through a host-built
// table of source coordinates in 1/256 pixel, in front of k_resize_crop.  Integer arithmetic only (the rule is in
// include/m3slam.h and restated by tests/undistort_twin.py).  One launch: a workgroup owns 256 columns x 4 rows of the
// output, a thread four neighbouring pixels of one row; the taps come from global memory (neighbouring pixels share
// lines, the vector L1 and the L2 serve them).  Every tap index is clamped into the source before it becomes an
// address and the border value is selected afterwards, so no table can make a load leave the source.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kQuadsX = 64;                   // threads along a row: 256 output columns per workgroup
constexpr int kRows = kThreads / kQuadsX;     // output rows per workgroup

struct RemapParams {
    const uint8_t *src;
    const int32_t *table;
    uint8_t *dst;
    int Hs, Ws, Ho, Wo, border, tiles_x;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One output pixel: -> its three bytes in bits 0..23.  img = the frame's first byte.
__device__ __forceinline__ unsigned remap_pixel(const RemapParams &p, const uint8_t *__restrict__ img, int qx, int qy) {
    const int ix = qx >> 8, iy = qy >> 8, a = qx & 255, b = qy & 255;
    const int x0 = clampi(ix, 0, p.Ws - 1), x1 = clampi(ix + 1, 0, p.Ws - 1);
    const int y0 = clampi(iy, 0, p.Hs - 1), y1 = clampi(iy + 1, 0, p.Hs - 1);
    const bool inx0 = (unsigned)ix < (unsigned)p.Ws, inx1 = (unsigned)(ix + 1) < (unsigned)p.Ws;
    const bool iny0 = (unsigned)iy < (unsigned)p.Hs, iny1 = (unsigned)(iy + 1) < (unsigned)p.Hs;
    const uint8_t *r0 = img + (int64_t)y0 * p.Ws * 3, *r1 = img + (int64_t)y1 * p.Ws * 3;
    const uint8_t *t00 = r0 + x0 * 3, *t01 = r0 + x1 * 3, *t10 = r1 + x0 * 3, *t11 = r1 + x1 * 3;
    const int w00 = __mul24(256 - a, 256 - b), w01 = __mul24(a, 256 - b), w10 = __mul24(256 - a, b), w11 = __mul24(a, b);
    const bool in00 = inx0 && iny0, in01 = inx1 && iny0, in10 = inx0 && iny1, in11 = inx1 && iny1;
    unsigned out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int p00 = in00 ? (int)t00[c] : p.border, p01 = in01 ? (int)t01[c] : p.border;
        const int p10 = in10 ? (int)t10[c] : p.border, p11 = in11 ? (int)t11[c] : p.border;
        // weights <= 2^16 and bytes: the full-rate 24-bit multiply is exact; the sum is <= 255 * 2^16 + 2^15
        const int acc = __mul24(p00, w00) + __mul24(p01, w01) + __mul24(p10, w10) + __mul24(p11, w11) + (1 << 15);
        out |= (unsigned)(acc >> 16) << (8 * c);
    }
    return out;
}

__global__ void __launch_bounds__(kThreads) k_remap_bilinear(const RemapParams p) {
    const int tile_y = blockIdx.x / p.tiles_x, tile_x = blockIdx.x - tile_y * p.tiles_x;
    const int u = (tile_x * kQuadsX + (threadIdx.x & (kQuadsX - 1))) * 4;
    const int v = tile_y * kRows + (threadIdx.x / kQuadsX);
    if (u >= p.Wo || v >= p.Ho) return;
    const uint8_t *img = p.src + (int64_t)blockIdx.y * p.Hs * p.Ws * 3;
    const int64_t e = (int64_t)v * p.Wo + u;                                  // first table entry of this thread
    const int64_t d = (((int64_t)blockIdx.y * p.Ho + v) * p.Wo + u) * 3;      // first output byte
    if (u + 4 <= p.Wo && (e & 1) == 0 && (d & 3) == 0) {
        const int4 ta = *(const int4 *)(p.table + 2 * e), tb = *(const int4 *)(p.table + 2 * e + 4);
        const unsigned o0 = remap_pixel(p, img, ta.x, ta.y), o1 = remap_pixel(p, img, ta.z, ta.w);
        const unsigned o2 = remap_pixel(p, img, tb.x, tb.y), o3 = remap_pixel(p, img, tb.z, tb.w);
        unsigned *q = (unsigned *)(p.dst + d);
        q[0] = o0 | (o1 << 24);
        q[1] = (o1 >> 8) | (o2 << 16);
        q[2] = (o2 >> 16) | (o3 << 8);
    } else {
        const int n = min(4, p.Wo - u);
        for (int i = 0; i < n; ++i) {
            const unsigned o = remap_pixel(p, img, p.table[2 * (e + i)], p.table[2 * (e + i) + 1]);
            p.dst[d + 3 * i] = (uint8_t)o;
            p.dst[d + 3 * i + 1] = (uint8_t)(o >> 8);
            p.dst[d + 3 * i + 2] = (uint8_t)(o >> 16);
        }
    }
}

}  // namespace

extern "C" {

int m3_remap_bilinear_u8(const uint8_t *src, const int32_t *table, uint8_t *dst, int B, int Hs, int Ws, int Ho, int Wo,
                         int border, void *stream) {
    M3_REQUIRE(src && table && dst && B >= 1 && B <= 65535 && Hs >= 1 && Ws >= 1 && Ho >= 1 && Wo >= 1);
    M3_REQUIRE(Hs <= (1 << 20) && Ws <= (1 << 20) && Ho <= (1 << 20) && Wo <= (1 << 20) && border >= 0 && border <= 255);
    M3_REQUIRE(((uintptr_t)src & 15) == 0 && ((uintptr_t)table & 15) == 0 && ((uintptr_t)dst & 15) == 0);
    RemapParams p;
    p.src = src; p.table = table; p.dst = dst;
    p.Hs = Hs; p.Ws = Ws; p.Ho = Ho; p.Wo = Wo; p.border = border;
    p.tiles_x = m3_cdiv(Wo, kQuadsX * 4);
    const int64_t tiles = (int64_t)p.tiles_x * m3_cdiv(Ho, kRows);
    if (tiles * kThreads >= ((int64_t)1 << 32)) return M3_ERR_UNSUPPORTED;      // the launch limit on gridDim.x * blockDim.x
    hipLaunchKernelGGL(k_remap_bilinear, dim3((unsigned)tiles, B), dim3(kThreads), 0, (hipStream_t)stream, p);
    M3_CHECK_LAUNCH("m3_remap_bilinear_u8");
    return M3_OK;
}

}  // extern "C"
