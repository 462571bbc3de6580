// Dense map export (mast3r_slam/export.py): world points and colours of K keyframes, filtered by average confidence,
// compacted in source order and optionally thinned to one point per voxel.  Stage A is count -> scan -> scatter over
// 1024-point workgroup tiles; stage B claims voxels in the key table of table_dev.h and then reuses the same
// count -> scan -> scatter.  Output positions come from an exclusive scan, never from an atomic counter, and the
// only atomics are integer CAS / max, so the bytes of every output are the same on every call.
#include "common.h"
#include "sim3_dev.h"
#include "map_points.h"
#include "compact_dev.h"
#include "table_dev.h"

namespace {

// Kept points per workgroup.  X is only read by threads with a point that passed the confidence test.
__global__ void __launch_bounds__(kThreads) k_export_count(const float *const *__restrict__ X,
                                                            const float *const *__restrict__ C,
                                                            const float *__restrict__ poses, const int32_t *__restrict__ Nk,
                                                            int N, int tiles, int use_thresh, float thresh,
                                                            int32_t *__restrict__ cnt) {
    const Tile t = tile_of(N, tiles, X, C);
    float avg[kPts];
    unsigned keep = conf_pass(t, N, (float)Nk[t.k], use_thresh, thresh, avg);
    if (keep) {
        V3<float> p[kPts];
        keep = world_points(t, load_pose<float>(poses + 8 * t.k), keep, p);
    }
    int total;
    block_prefix(keep, total);
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

// LAYOUT as fetch_rgb takes it.
template <int LAYOUT>
__global__ void __launch_bounds__(kThreads) k_export_scatter(const float *const *__restrict__ X,
                                                              const float *const *__restrict__ C,
                                                              const void *const *__restrict__ img,
                                                              const float *__restrict__ poses, const int32_t *__restrict__ Nk,
                                                              int N, int tiles, int use_thresh, float thresh,
                                                              const int32_t *__restrict__ offs, int64_t M,
                                                              float *__restrict__ points, unsigned char *__restrict__ colors,
                                                              int64_t *__restrict__ index, float *__restrict__ conf) {
    const Tile t = tile_of(N, tiles, X, C);
    const void *Ik = img[t.k];
    float avg[kPts];
    unsigned keep = conf_pass(t, N, (float)Nk[t.k], use_thresh, thresh, avg);
    V3<float> p[kPts];
    if (keep) keep = world_points(t, load_pose<float>(poses + 8 * t.k), keep, p);
    int total;
    int64_t o = (int64_t)offs[blockIdx.x] + block_prefix(keep, total);
    if (!keep) return;
    unsigned char rgb[kPts][3];
    fetch_rgb<LAYOUT>(Ik, t, N, keep, rgb);
#pragma unroll
    for (int j = 0; j < kPts; ++j) {
        if (!((keep >> j) & 1u) || o >= M) continue;                            // o < M always holds for a ws from the same inputs
        store_row(o, p[j], rgb[j], (int64_t)t.k * N + t.n0 + j, points, colors, index);
        if (conf) conf[o] = avg[j];
        ++o;
    }
}

// ---- stage B -----------------------------------------------------------------------------------------------------
struct VoxelWs {
    int32_t *hdr, *offs;
    uint32_t *slot;                  // [M] table slot of each point, kNoSlot = dropped
    unsigned long long *keys, *vals; // [slots]
    int64_t slots, blocks, bytes;
};

inline VoxelWs voxel_ws(void *ws, int64_t M) {
    VoxelWs v;
    v.blocks = (M + kTile - 1) / kTile;
    v.slots = table_slots(2 * M);
    char *p = (char *)ws;
    v.hdr = (int32_t *)p;
    v.offs = v.hdr + kHdrWords;
    int64_t off = (kHdrWords + (v.blocks + 3) / 4 * 4) * 4;
    v.slot = (uint32_t *)(p + off);
    off += (M + 3) / 4 * 4 * 4;
    v.keys = (unsigned long long *)(p + off);
    off += v.slots * 8;
    v.vals = (unsigned long long *)(p + off);
    v.bytes = off + v.slots * 8;
    return v;
}

// Order-preserving unsigned key of a float (-0 = +0; NaN ranks below every number).
__device__ __forceinline__ unsigned conf_key(float c) {
    if (c != c) return 0u;
    const unsigned u = __float_as_uint(c + 0.f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// One point per thread: claim the voxel's slot (CAS on the key) and raise its value to (confidence key, ~i): the
// largest confidence wins, equal confidences go to the smaller i.  Both atomics commute, so the winner does not depend
// on the order in which points arrive (the slot a voxel lands in does; nothing that is output depends on it).
__global__ void __launch_bounds__(kThreads) k_voxel_insert(const float *__restrict__ points, const float *__restrict__ conf,
                                                            int64_t M, float voxel, unsigned long long *__restrict__ keys,
                                                            unsigned long long *__restrict__ vals, int64_t slots,
                                                            uint32_t *__restrict__ slot, int32_t *__restrict__ hdr) {
    const int64_t i = row_of();
    if (i >= M) return;
    const float vx = floorf(points[3 * i] / voxel), vy = floorf(points[3 * i + 1] / voxel),
                vz = floorf(points[3 * i + 2] / voxel);
    constexpr float kLim = 1048576.f;                                           // 2^20: 21 bits per axis after the offset
    if (!(fabsf(vx) < kLim && fabsf(vy) < kLim && fabsf(vz) < kLim)) {
        slot[i] = kNoSlot;
        atomicAdd(&hdr[1], 1);
        return;
    }
    const unsigned long long val = ((unsigned long long)conf_key(conf[i]) << 32) | (unsigned)~(unsigned)i;
    bool claimed;
    const uint32_t s = key_claim(keys, slots, cell_key((int)vx + kCellBias, (int)vy + kCellBias, (int)vz + kCellBias), claimed);
    slot[i] = s;
    if (s != kNoSlot) atomicMax(&vals[s], val);
    else atomicAdd(&hdr[1], 1);                                                 // unreachable: slots >= 2 M
}

// Bits of the thread's four consecutive points that won their voxel.
__device__ __forceinline__ unsigned voxel_winners(const uint32_t *__restrict__ slot,
                                                  const unsigned long long *__restrict__ vals, int64_t i0, int64_t M) {
    unsigned keep = 0;
#pragma unroll
    for (int j = 0; j < kPts; ++j) {
        const int64_t i = i0 + j;
        if (i >= M) continue;
        const uint32_t s = slot[i];
        if (s != kNoSlot && (unsigned)vals[s] == (unsigned)~(unsigned)i) keep |= 1u << j;
    }
    return keep;
}

__global__ void __launch_bounds__(kThreads) k_voxel_count(const uint32_t *__restrict__ slot,
                                                           const unsigned long long *__restrict__ vals, int64_t M,
                                                           int32_t *__restrict__ cnt) {
    const unsigned keep = voxel_winners(slot, vals, (int64_t)blockIdx.x * kTile + threadIdx.x * kPts, M);
    int total;
    block_prefix(keep, total);
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kThreads) k_voxel_scatter(const float *__restrict__ points,
                                                             const unsigned char *__restrict__ colors,
                                                             const int64_t *__restrict__ index,
                                                             const uint32_t *__restrict__ slot,
                                                             const unsigned long long *__restrict__ vals, int64_t M,
                                                             const int32_t *__restrict__ offs, int64_t M2,
                                                             float *__restrict__ points_out,
                                                             unsigned char *__restrict__ colors_out,
                                                             int64_t *__restrict__ index_out) {
    const int64_t i0 = (int64_t)blockIdx.x * kTile + threadIdx.x * kPts;
    const unsigned keep = voxel_winners(slot, vals, i0, M);
    int total;
    int64_t o = (int64_t)offs[blockIdx.x] + block_prefix(keep, total);
#pragma unroll
    for (int j = 0; j < kPts; ++j) {
        if (!((keep >> j) & 1u) || o >= M2) continue;
        const int64_t i = i0 + j;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            points_out[3 * o + d] = points[3 * i + d];
            colors_out[3 * o + d] = colors[3 * i + d];
        }
        if (index_out) index_out[o] = index ? index[i] : i;
        ++o;
    }
}

}  // namespace

extern "C" {

int64_t m3_map_export_ws_bytes(int K, int N) {
    if (!map_shape_ok(K, N)) return 0;
    const int64_t blocks = (int64_t)K * m3_cdiv(N, kTile);
    return (kHdrWords + (blocks + 3) / 4 * 4) * 4;
}

int m3_map_export_count(const float *const *X, const float *const *C, const float *poses, const int32_t *Nk, int K, int N,
                        int use_thresh, float thresh, void *ws, int64_t ws_bytes, void *stream) {
    M3_REQUIRE(X && C && poses && Nk && ws && map_shape_ok(K, N));
    M3_REQUIRE((use_thresh == 0 || use_thresh == 1) && ((uintptr_t)ws & 15) == 0 && ws_bytes >= m3_map_export_ws_bytes(K, N));
    hipStream_t st = (hipStream_t)stream;
    const int tiles = m3_cdiv(N, kTile), blocks = K * tiles;
    int32_t *hdr = (int32_t *)ws;
    hipLaunchKernelGGL(k_export_count, dim3(blocks), dim3(kThreads), 0, st, X, C, poses, Nk, N, tiles, use_thresh, thresh,
                       hdr + kHdrWords);
    launch_scan(st, hdr, ScanJob{hdr + kHdrWords, blocks});
    M3_CHECK_LAUNCH("m3_map_export_count");
    return M3_OK;
}

int m3_map_export_scatter(const float *const *X, const float *const *C, const void *const *img, const float *poses,
                          const int32_t *Nk, int K, int N, int use_thresh, float thresh, int layout, const void *ws,
                          int64_t ws_bytes, int64_t M, float *points, uint8_t *colors, int64_t *index, float *conf,
                          void *stream) {
    M3_REQUIRE(X && C && img && poses && Nk && ws && points && colors && map_shape_ok(K, N));
    M3_REQUIRE((use_thresh == 0 || use_thresh == 1) && ((uintptr_t)ws & 15) == 0 && ws_bytes >= m3_map_export_ws_bytes(K, N));
    M3_REQUIRE(M >= 1 && M <= (int64_t)K * N);
    M3_REQUIRE(layout == M3_MAP_IMG_F32_CHW || layout == M3_MAP_IMG_U8_HWC);
    hipStream_t st = (hipStream_t)stream;
    const int tiles = m3_cdiv(N, kTile), blocks = K * tiles;
    const int32_t *offs = (const int32_t *)ws + kHdrWords;
    if (layout == M3_MAP_IMG_F32_CHW)
        hipLaunchKernelGGL(k_export_scatter<0>, dim3(blocks), dim3(kThreads), 0, st, X, C, img, poses, Nk, N, tiles,
                           use_thresh, thresh, offs, M, points, colors, index, conf);
    else
        hipLaunchKernelGGL(k_export_scatter<1>, dim3(blocks), dim3(kThreads), 0, st, X, C, img, poses, Nk, N, tiles,
                           use_thresh, thresh, offs, M, points, colors, index, conf);
    M3_CHECK_LAUNCH("m3_map_export_scatter");
    return M3_OK;
}

int64_t m3_map_voxel_table_slots(int64_t M) {
    return M >= 1 && M <= 0x7fffffff ? table_slots(2 * M) : 0;
}

int64_t m3_map_voxel_ws_bytes(int64_t M) {
    return M >= 1 && M <= 0x7fffffff ? voxel_ws(nullptr, M).bytes : 0;
}

int m3_map_voxel_count(const float *points, const float *conf, int64_t M, float voxel_size, void *ws, int64_t ws_bytes,
                       void *stream) {
    M3_REQUIRE(points && conf && ws && M >= 1 && M <= 0x7fffffff && voxel_size > 0.f && voxel_size < INFINITY);
    M3_REQUIRE(((uintptr_t)ws & 15) == 0 && ws_bytes >= m3_map_voxel_ws_bytes(M));
    hipStream_t st = (hipStream_t)stream;
    const VoxelWs v = voxel_ws(ws, M);
    M3_CHECK_HIP(hipMemsetAsync(v.hdr, 0, kHdrWords * 4, st), "m3_map_voxel_count/memset");
    M3_CHECK_HIP(hipMemsetAsync(v.keys, 0xff, v.slots * 8, st), "m3_map_voxel_count/memset");
    M3_CHECK_HIP(hipMemsetAsync(v.vals, 0, v.slots * 8, st), "m3_map_voxel_count/memset");
    hipLaunchKernelGGL(k_voxel_insert, dim3(m3_cdiv(M, kThreads)), dim3(kThreads), 0, st, points, conf, M, voxel_size,
                       v.keys, v.vals, v.slots, v.slot, v.hdr);
    hipLaunchKernelGGL(k_voxel_count, dim3((int)v.blocks), dim3(kThreads), 0, st, v.slot, v.vals, M, v.offs);
    launch_scan(st, v.hdr, ScanJob{v.offs, v.blocks});
    M3_CHECK_LAUNCH("m3_map_voxel_count");
    return M3_OK;
}

int m3_map_voxel_scatter(const float *points, const uint8_t *colors, const int64_t *index, int64_t M, const void *ws,
                         int64_t ws_bytes, int64_t M2, float *points_out, uint8_t *colors_out, int64_t *index_out,
                         void *stream) {
    M3_REQUIRE(points && colors && ws && points_out && colors_out && M >= 1 && M <= 0x7fffffff && M2 >= 1 && M2 <= M);
    M3_REQUIRE(((uintptr_t)ws & 15) == 0 && ws_bytes >= m3_map_voxel_ws_bytes(M));
    const VoxelWs v = voxel_ws(const_cast<void *>(ws), M);
    hipLaunchKernelGGL(k_voxel_scatter, dim3((int)v.blocks), dim3(kThreads), 0, (hipStream_t)stream, points, colors, index,
                       v.slot, v.vals, M, v.offs, M2, points_out, colors_out, index_out);
    M3_CHECK_LAUNCH("m3_map_voxel_scatter");
    return M3_OK;
}

}  // extern "C"
