// Headless map renderer (mast3r_slam/render.py): the keyframe map drawn into an image from any pinhole camera, with a
// z-buffer of 64-bit keys (bits of the camera depth << 32 | source index).  clear -> splat -> resolve; the splat's only
// atomics are 64-bit integer minima, which commute, so two calls give identical bytes.  Nothing here waits for the
// host: the view pose is read from device memory and the call can be captured into a graph.
//
// Compiled with -ffp-contract=off for view_dev.h, which holds the camera transform, the projection and the checks of
// the camera arguments.  The world point is the exporter's:
// map_points.h is included with contraction on, as map_export.hip compiles it.
#include "common.h"
#pragma clang fp contract(fast)
#include "sim3_dev.h"
#include "map_points.h"
#pragma clang fp contract(off)
#include "view_dev.h"
#include "zkey_dev.h"

namespace {

// Grid as k_export_count.  A thread owns 4 consecutive points; X is only read when one of them passed the confidence
// test.  Per footprint pixel: key_min (zkey_dev.h).
template <int PS>
__global__ void __launch_bounds__(kThreads) k_render_splat(const float *const *__restrict__ X,
                                                            const float *const *__restrict__ C,
                                                            const float *__restrict__ poses, const int32_t *__restrict__ Nk,
                                                            int N, int tiles, int use_thresh, float thresh,
                                                            const float *__restrict__ view, float fx, float fy, float cx,
                                                            float cy, int Hv, int Wv, float near, float far,
                                                            unsigned long long *keys) {
    const Pinhole pin{fx, fy, cx, cy};
    __shared__ float sv[kViewWords];
    if (threadIdx.x == 0) view_inverse(view, sv);
    const Tile t = tile_of(N, tiles, X, C);
    float avg[kPts];
    unsigned keep = conf_pass(t, N, (float)Nk[t.k], use_thresh, thresh, avg);
    __syncthreads();
    if (!keep) return;
    V3<float> p[kPts];
    keep = world_points(t, load_pose<float>(poses + 8 * t.k), keep, p);
    constexpr int R = PS / 2;
#pragma unroll
    for (int j = 0; j < kPts; ++j) {
        if (!((keep >> j) & 1u)) continue;
        const V3<float> c = view_point(sv, p[j]);
        if (!in_depth(c.z, near, far)) continue;
        const float fu = nearest_pixel(image_u(pin, c)), fv = nearest_pixel(image_v(pin, c));
        if (!(fu >= (float)-R && fu < (float)(Wv + R) && fv >= (float)-R && fv < (float)(Hv + R))) continue;
        const int px = (int)fu, py = (int)fv;
        const unsigned long long key = ((unsigned long long)__float_as_uint(c.z) << 32) | (unsigned)(t.k * N + t.n0 + j);
#pragma unroll
        for (int oy = -R; oy <= R; ++oy) {
            const int yy = py + oy;
            if (yy < 0 || yy >= Hv) continue;
#pragma unroll
            for (int ox = -R; ox <= R; ++ox) {
                const int xx = px + ox;
                if (xx < 0 || xx >= Wv) continue;
                key_min(keys + ((int64_t)yy * Wv + xx), key);
            }
        }
    }
}

// Shares its frame with k_raster_resolve by copy, not through one template (load, per-key functor, store): that template
// compiled both kernels to other instructions and measured above the copies' range.
// A thread owns 4 consecutive output pixels.  LAYOUT as fetch_rgb takes it.
template <int LAYOUT>
__global__ void __launch_bounds__(kThreads) k_render_resolve(const unsigned long long *__restrict__ keys,
                                                              const void *const *__restrict__ img, int N, int64_t P,
                                                              unsigned bg, unsigned char *__restrict__ rgb,
                                                              float *__restrict__ depth, int64_t *__restrict__ index) {
    const int64_t i0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
    if (i0 >= P) return;
    const bool vec = i0 + 4 <= P && ((uintptr_t)rgb & 3) == 0 && aligned16(depth) && aligned16(index);
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
        if (key[j] == kNoKey) {
            c[j][0] = (unsigned char)bg; c[j][1] = (unsigned char)(bg >> 8); c[j][2] = (unsigned char)(bg >> 16);
            z[j] = INFINITY;
            src[j] = -1;
            continue;
        }
        const unsigned s = (unsigned)key[j];
        const unsigned k = s / (unsigned)N, n = s - k * (unsigned)N;
        z[j] = __uint_as_float((unsigned)(key[j] >> 32));
        src[j] = (int64_t)s;
        fetch_rgb<LAYOUT>(img[k], N, n, c[j]);
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

inline bool view_ok(int Hv, int Wv) { return Hv >= 1 && Wv >= 1 && Hv <= 16384 && Wv <= 16384; }

}  // namespace

extern "C" {

int64_t m3_render_ws_bytes(int Hv, int Wv) { return view_ok(Hv, Wv) ? (int64_t)Hv * Wv * 8 : 0; }

int m3_render_launches(int K) { return K > 0 ? 3 : 2; }

int m3_render_map(const float *const *X, const float *const *C, const void *const *img, const float *poses,
                  const int32_t *Nk, int K, int N, int use_thresh, float thresh, int layout, const float *view_pose,
                  float fx, float fy, float cx, float cy, int Hv, int Wv, float near, float far, int point_size, int bg_r,
                  int bg_g, int bg_b, void *ws, int64_t ws_bytes, uint8_t *rgb, float *depth, int64_t *index,
                  void *stream) {
    M3_REQUIRE(view_ok(Hv, Wv) && (K == 0 || map_shape_ok(K, N)) && ws && rgb && depth);     // an empty map is drawn
    M3_REQUIRE(K == 0 || (X && C && img && poses && Nk && view_pose));
    M3_REQUIRE((use_thresh == 0 || use_thresh == 1) && ((uintptr_t)ws & 15) == 0 && ws_bytes >= m3_render_ws_bytes(Hv, Wv));
    M3_REQUIRE(layout == M3_MAP_IMG_F32_CHW || layout == M3_MAP_IMG_U8_HWC);
    M3_REQUIRE(point_size == 1 || point_size == 3 || point_size == 5 || point_size == 7);
    const Pinhole pin{fx, fy, cx, cy};
    M3_REQUIRE(pinhole_ok(pin, false) && depth_range_ok(near, far));           // an infinite cx draws the background
    M3_REQUIRE(background_ok(bg_r, bg_g, bg_b));
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *keys = (unsigned long long *)ws;
    const int64_t P = (int64_t)Hv * Wv;
    launch_key_clear(keys, P, st);
    if (K > 0) {
        const int tiles = m3_cdiv(N, kTile);
        const dim3 grid(K * tiles), block(kThreads);
#define M3_SPLAT(PS)                                                                                                    \
    hipLaunchKernelGGL(k_render_splat<PS>, grid, block, 0, st, X, C, poses, Nk, N, tiles, use_thresh, thresh, view_pose, \
                       fx, fy, cx, cy, Hv, Wv, near, far, keys)
        if (point_size == 1) M3_SPLAT(1);
        else if (point_size == 3) M3_SPLAT(3);
        else if (point_size == 5) M3_SPLAT(5);
        else M3_SPLAT(7);
#undef M3_SPLAT
    }
    const unsigned bg = pack_background(bg_r, bg_g, bg_b);
    const dim3 rgrid(m3_cdiv(P, 4 * kThreads));
    if (layout == M3_MAP_IMG_F32_CHW)
        hipLaunchKernelGGL(k_render_resolve<0>, rgrid, dim3(kThreads), 0, st, keys, img, K > 0 ? N : 1, P, bg, rgb, depth, index);
    else
        hipLaunchKernelGGL(k_render_resolve<1>, rgrid, dim3(kThreads), 0, st, keys, img, K > 0 ? N : 1, P, bg, rgb, depth, index);
    M3_CHECK_LAUNCH("m3_render_map");
    return M3_OK;
}

}  // extern "C"
