// EXPERIMENT, not part of the library: the staged variant of k_remap_bilinear (mast3r-slam_amd/csrc/undistort.hip).
// Same rule, same bytes (include/m3slam.h, tests/undistort_twin.py); only the way the taps reach the lanes differs.
// tools/experiments/undistort_staged.py builds it into a shared object of its own, builds the per-tile boxes on the
// host and calls it; tests/test_gpu_undistort_staged.py compares every byte with the twin; tools/bench_undistort.py
// times it against the library's kernel in alternation.  Outcome: profiles/undistort_bench.md and DESIGN.md section 7e.
//
// A workgroup (one wave) owns a tile of 64 x 4 output pixels, a lane four neighbouring pixels of one row, as in the
// library's kernel.  Before any tap is read the wave copies the bounding box of the tile's source taps into LDS:
// per source row the 16-byte-aligned span that holds the box's bytes, with 16-byte loads.  Source rows are Ws * 3
// bytes, so the span's first useful byte sits at (row start & 15) in its LDS row; that offset is recomputed per tap.
// The box (x0, y0, w, h in source pixels) comes from the host, one int4 per tile, built from the table.  It is never
// trusted: the kernel stages only a box that lies inside the source and fits the LDS budget, and a pixel reads LDS
// only where its four taps lie inside the staged box.  Every other pixel (a sentinel, a tap outside the source, a tile
// whose box is too large or marked empty by the host) takes the global path, which is the library's, clamps included.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kTileW = 64, kTileH = 4;        // output pixels per workgroup
constexpr int kThreads = 64;                  // one wave: 16 lanes along a row x 4 rows, four pixels per lane
constexpr int kQuadsX = kTileW / 4;
constexpr int kLdsBytes = 8192;               // 20 workgroups per CU; a 64 x 4 tile of a 1.3x map needs about 2.3 KiB

struct StagedParams {
    const uint8_t *src;
    const int32_t *table;
    const int4 *boxes;
    uint8_t *dst;
    int Hs, Ws, Ho, Wo, border, tiles_x;
};

struct Stage {
    const uint8_t *lds;
    int x0, y0, w, h, pitch;
    unsigned frame_mod;                       // the frame's first byte, modulo 16
    bool on;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ unsigned blend(int p00, int p01, int p10, int p11, int w00, int w01, int w10, int w11) {
    return (unsigned)((__mul24(p00, w00) + __mul24(p01, w01) + __mul24(p10, w10) + __mul24(p11, w11) + (1 << 15)) >> 16);
}

// One output pixel: -> its three bytes in bits 0..23.  img = the frame's first byte.
__device__ __forceinline__ unsigned remap_pixel(const StagedParams &p, const Stage &s, const uint8_t *__restrict__ img,
                                                int qx, int qy) {
    const int ix = qx >> 8, iy = qy >> 8, a = qx & 255, b = qy & 255;
    const int w00 = __mul24(256 - a, 256 - b), w01 = __mul24(a, 256 - b), w10 = __mul24(256 - a, b), w11 = __mul24(a, b);
    unsigned out = 0;
    if (s.on && ix >= s.x0 && ix - s.x0 <= s.w - 2 && iy >= s.y0 && iy - s.y0 <= s.h - 2) {
        const int r = iy - s.y0;
        // the row's first box byte, modulo 16 (unsigned wrap keeps the low bits)
        const unsigned off0 = (s.frame_mod + ((unsigned)iy * (unsigned)p.Ws + (unsigned)s.x0) * 3u) & 15u;
        const unsigned off1 = (off0 + (unsigned)p.Ws * 3u) & 15u;
        const uint8_t *l0 = s.lds + r * s.pitch + off0 + (ix - s.x0) * 3;
        const uint8_t *l1 = s.lds + (r + 1) * s.pitch + off1 + (ix - s.x0) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) out |= blend(l0[c], l0[3 + c], l1[c], l1[3 + c], w00, w01, w10, w11) << (8 * c);
        return out;
    }
    const int x0 = clampi(ix, 0, p.Ws - 1), x1 = clampi(ix + 1, 0, p.Ws - 1);
    const int y0 = clampi(iy, 0, p.Hs - 1), y1 = clampi(iy + 1, 0, p.Hs - 1);
    const bool inx0 = (unsigned)ix < (unsigned)p.Ws, inx1 = (unsigned)(ix + 1) < (unsigned)p.Ws;
    const bool iny0 = (unsigned)iy < (unsigned)p.Hs, iny1 = (unsigned)(iy + 1) < (unsigned)p.Hs;
    const uint8_t *r0 = img + (int64_t)y0 * p.Ws * 3, *r1 = img + (int64_t)y1 * p.Ws * 3;
    const uint8_t *t00 = r0 + x0 * 3, *t01 = r0 + x1 * 3, *t10 = r1 + x0 * 3, *t11 = r1 + x1 * 3;
    const bool in00 = inx0 && iny0, in01 = inx1 && iny0, in10 = inx0 && iny1, in11 = inx1 && iny1;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        out |= blend(in00 ? (int)t00[c] : p.border, in01 ? (int)t01[c] : p.border, in10 ? (int)t10[c] : p.border,
                     in11 ? (int)t11[c] : p.border, w00, w01, w10, w11) << (8 * c);
    return out;
}

__global__ void __launch_bounds__(kThreads) k_remap_staged(const StagedParams p) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsBytes];
    const int tile_y = blockIdx.x / p.tiles_x, tile_x = blockIdx.x - tile_y * p.tiles_x;
    const int64_t frame = (int64_t)blockIdx.y * p.Hs * p.Ws * 3;          // first byte of this frame
    const int64_t total = (int64_t)gridDim.y * p.Hs * p.Ws * 3;           // bytes in src
    const int4 box = p.boxes[blockIdx.x];
    Stage s;
    s.lds = lds; s.x0 = box.x; s.y0 = box.y; s.w = box.z; s.h = box.w;
    s.frame_mod = (unsigned)(frame & 15);
    // a usable box lies inside the source (so w * 3 < 2^22) and fits the budget; anything else is not staged
    s.on = box.x >= 0 && box.y >= 0 && box.z >= 2 && box.w >= 2 && box.z <= p.Ws - box.x && box.w <= p.Hs - box.y;
    s.pitch = s.on ? ((box.z * 3 + 30) >> 4) << 4 : 0;                    // 15 bytes of lead at most, rounded up to 16
    s.on = s.on && (int64_t)s.pitch * box.w <= kLdsBytes;                 // uniform over the workgroup
    if (s.on) {
        const int chunks = s.pitch >> 4, n = chunks * s.h;
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const int r = i / chunks, c = i - r * chunks;
            const int64_t g0 = frame + ((int64_t)(s.y0 + r) * p.Ws + s.x0) * 3;      // < total: the box is inside
            const int64_t ga = (g0 & ~(int64_t)15) + 16 * c;                          // >= 0, 16-byte aligned
            uint4 v = make_uint4(0, 0, 0, 0);
            if (ga + 16 <= total) {
                v = *(const uint4 *)(p.src + ga);
            } else {                                                                  // the last bytes of the buffer
                unsigned w4[4] = {0, 0, 0, 0};
                for (int k = 0; k < 16; ++k)
                    if (ga + k < total) w4[k >> 2] |= (unsigned)p.src[ga + k] << (8 * (k & 3));
                v = make_uint4(w4[0], w4[1], w4[2], w4[3]);
            }
            *(uint4 *)(lds + r * s.pitch + 16 * c) = v;
        }
        __syncthreads();
    }
    const int u = (tile_x * kQuadsX + (threadIdx.x & (kQuadsX - 1))) * 4;
    const int v = tile_y * kTileH + (threadIdx.x / kQuadsX);
    if (u >= p.Wo || v >= p.Ho) return;
    const uint8_t *img = p.src + frame;
    const int64_t e = (int64_t)v * p.Wo + u;
    const int64_t d = (((int64_t)blockIdx.y * p.Ho + v) * p.Wo + u) * 3;
    if (u + 4 <= p.Wo && (e & 1) == 0 && (d & 3) == 0) {
        const int4 ta = *(const int4 *)(p.table + 2 * e), tb = *(const int4 *)(p.table + 2 * e + 4);
        const unsigned o0 = remap_pixel(p, s, img, ta.x, ta.y), o1 = remap_pixel(p, s, img, ta.z, ta.w);
        const unsigned o2 = remap_pixel(p, s, img, tb.x, tb.y), o3 = remap_pixel(p, s, img, tb.z, tb.w);
        unsigned *q = (unsigned *)(p.dst + d);
        q[0] = o0 | (o1 << 24);
        q[1] = (o1 >> 8) | (o2 << 16);
        q[2] = (o2 >> 16) | (o3 << 8);
    } else {
        const int n = min(4, p.Wo - u);
        for (int i = 0; i < n; ++i) {
            const unsigned o = remap_pixel(p, s, img, p.table[2 * (e + i)], p.table[2 * (e + i) + 1]);
            p.dst[d + 3 * i] = (uint8_t)o;
            p.dst[d + 3 * i + 1] = (uint8_t)(o >> 8);
            p.dst[d + 3 * i + 2] = (uint8_t)(o >> 16);
        }
    }
}

}  // namespace

// 0 = launched, -1 = bad argument (nothing touched), -2 = the launch failed.  boxes: int32 [tiles_y * tiles_x, 4].
extern "C" int exp_remap_staged_u8(const uint8_t *src, const int32_t *table, const int32_t *boxes, uint8_t *dst, int B,
                                   int Hs, int Ws, int Ho, int Wo, int border, void *stream) {
    if (!(src && table && boxes && dst && B >= 1 && B <= 65535 && Hs >= 1 && Ws >= 1 && Ho >= 1 && Wo >= 1)) return -1;
    if (!(Hs <= (1 << 20) && Ws <= (1 << 20) && Ho <= (1 << 20) && Wo <= (1 << 20) && border >= 0 && border <= 255)) return -1;
    if (((uintptr_t)src & 15) || ((uintptr_t)table & 15) || ((uintptr_t)boxes & 15) || ((uintptr_t)dst & 15)) return -1;
    StagedParams p;
    p.src = src; p.table = table; p.boxes = (const int4 *)boxes; p.dst = dst;
    p.Hs = Hs; p.Ws = Ws; p.Ho = Ho; p.Wo = Wo; p.border = border;
    p.tiles_x = (Wo + kTileW - 1) / kTileW;
    const int64_t tiles = (int64_t)p.tiles_x * ((Ho + kTileH - 1) / kTileH);
    if (tiles * kThreads >= ((int64_t)1 << 32)) return -1;
    hipLaunchKernelGGL(k_remap_staged, dim3((unsigned)tiles, B), dim3(kThreads), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
