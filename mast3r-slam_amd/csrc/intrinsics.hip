// Focal length of every keyframe from its own pointmap (mast3r_slam/intrinsics.py): the f that
// minimises sum |(u, v) - f (x / z, y / z)| over the valid pixels, by Weiszfeld re-weighting from the least-squares
// start.  One launch per pass over the pixels plus one that finishes the mean residual; a workgroup reduces a fixed
// tile of one keyframe in a fixed order (thread, wave shuffle tree, LDS) and stores its partial sums, and every
// workgroup of the next pass re-adds its keyframe's partials in ascending tile order to get the focal it works with.
// No floating-point atomics, no counters: the bytes of the result are the same on every call and a keyframe's row does
// not depend on its neighbours in the call.
//
// Compiled with -ffp-contract=off: the per-pixel terms are separately rounded float64 operations
// (tests/focal_twin.py restates them).
#include "common.h"
#include "map_points.h"     // kThreads, kPts, kTile, aligned16; no world point is formed here

namespace {

constexpr int kChunk = kTile;                 // pixels a workgroup reads per round
constexpr int kMinRounds = 4;                 // 4096-pixel tiles ...
constexpr int kMaxTiles = 256;                // ... until a keyframe would have more tiles than this: then the tile grows
constexpr int kPart = 3;                      // partial sums per tile: numerator, denominator (0 in the residual pass), count

enum { LSQ = 0, WEISZFELD = 1, RESIDUAL = 2 };

struct Plan {
    int rounds, tiles;                        // rounds of kChunk pixels per workgroup, workgroups per keyframe
};

inline Plan plan_of(int N) {
    const int chunks = m3_cdiv(N, kChunk);
    Plan p;
    p.rounds = chunks > kMinRounds * kMaxTiles ? m3_cdiv(chunks, kMaxTiles) : kMinRounds;
    p.tiles = m3_cdiv(chunks, p.rounds);
    return p;
}

inline bool focal_shape_ok(int K, int N) {
    return K >= 1 && N >= 1 && (int64_t)K * N <= 0x7fffffff && (int64_t)K * plan_of(N).tiles <= (1 << 22);
}

// The kPart sums of one keyframe's tile partials, each added in ascending tile order; every thread gets them.
__device__ __forceinline__ void keyframe_sums(const double *__restrict__ part, int tiles, double (&s)[kPart]) {
    __shared__ double sp[kMaxTiles * kPart];
    __shared__ double tot[kPart];
    for (int i = threadIdx.x; i < tiles * kPart; i += kThreads) sp[i] = part[i];
    __syncthreads();
    if (threadIdx.x < kPart) {
        double a = 0.0;
        for (int t = 0; t < tiles; ++t) a += sp[t * kPart + threadIdx.x];
        tot[threadIdx.x] = a;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kPart; ++i) s[i] = tot[i];
}

// Grid: K * tiles workgroups, keyframe-major.  prev: the partials of the pass before (unused by LSQ), next: this pass's.
// The workgroup of tile 0 also writes what the sums of `prev` settle: f_0 and the count (first = 1: the pass after LSQ)
// and f_iters (RESIDUAL).
template <int MODE>
__global__ void __launch_bounds__(kThreads) k_focal_pass(const float *const *__restrict__ X,
                                                          const float *const *__restrict__ C,
                                                          const int32_t *__restrict__ Nk, int N, int W, int tiles,
                                                          int rounds, int use_thresh, float thresh, double cx, double cy,
                                                          float z_min, int first, const double *__restrict__ prev,
                                                          double *__restrict__ next, double *__restrict__ out) {
    const int k = blockIdx.x / tiles, tile = blockIdx.x - k * tiles;
    double f = 0.0;
    if constexpr (MODE != LSQ) {
        double s[kPart];
        keyframe_sums(prev + (size_t)k * tiles * kPart, tiles, s);
        f = s[0] / s[1];
        if (tile == 0 && threadIdx.x == 0) {
            if (first) { out[4 * k + 1] = f; out[4 * k + 2] = s[2]; }
            if (MODE == RESIDUAL) out[4 * k] = f;
        }
    }
    const float *Xk = X[k], *Ck = C[k];
    // The loads stay written out here, with the predicate hoisted out of the round loop: with load_conf / load_points
    // of map_points.h inside the loop the pass measured 2.7 % slower at one keyframe (profiles/map_family_refactor.md).
    const bool vec = N % 4 == 0 && aligned16(Xk) && aligned16(Ck);
    const float nk = (float)Nk[k];
    double acc[kPart] = {0.0, 0.0, 0.0};
    for (int r = 0; r < rounds; ++r) {
        const int64_t first_px = ((int64_t)tile * rounds + r) * kChunk + threadIdx.x * kPts;
        if (first_px >= N) break;
        const int n0 = (int)first_px, rem = N - n0;                             // rem >= 1 pixels exist from n0 on
        float c[kPts], x[3 * kPts];
        if (vec) {                                                              // N % 4 == 0: rem >= 4
            const float4 cv = *(const float4 *)(Ck + n0);
            const float4 *src = (const float4 *)(Xk + (size_t)3 * n0);
            const float4 a = src[0], b = src[1], d = src[2];
            c[0] = cv.x; c[1] = cv.y; c[2] = cv.z; c[3] = cv.w;
            x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
            x[8] = d.x; x[9] = d.y; x[10] = d.z; x[11] = d.w;
        } else {
#pragma unroll
            for (int j = 0; j < kPts; ++j) {
                const bool in = j < rem;
                c[j] = in ? Ck[n0 + j] : 0.f;
#pragma unroll
                for (int d = 0; d < 3; ++d) x[3 * j + d] = in ? Xk[(size_t)3 * (n0 + j) + d] : 0.f;
            }
        }
        int row = n0 / W, col = n0 - row * W;
#pragma unroll
        for (int j = 0; j < kPts; ++j) {
            const float px = x[3 * j], py = x[3 * j + 1], pz = x[3 * j + 2];
            const float avg = c[j] / nk;
            const bool ok = j < rem && (!use_thresh || avg > thresh) && isfinite(px) && isfinite(py) && isfinite(pz) &&
                            pz > z_min;
            const double u = (double)col - cx, v = (double)row - cy;
            const double a = (double)px / (double)pz, b = (double)py / (double)pz;
            const double pq = a * u + b * v, qq = a * a + b * b;
            double t0 = pq, t1 = qq;
            if constexpr (MODE != LSQ) {
                const double du = u - f * a, dv = v - f * b;
                const double d = sqrt(du * du + dv * dv);
                if constexpr (MODE == WEISZFELD) {
                    const double w = 1.0 / (d > 1e-8 ? d : 1e-8);
                    t0 = w * pq;
                    t1 = w * qq;
                } else {
                    t0 = d;
                    t1 = 0.0;
                }
            }
            acc[0] += ok ? t0 : 0.0;
            acc[1] += ok ? t1 : 0.0;
            acc[2] += ok ? 1.0 : 0.0;
            if (++col == W) { col = 0; ++row; }
        }
    }
    __shared__ double red[kThreads / M3_WAVE][kPart];
#pragma unroll
    for (int i = 0; i < kPart; ++i) {
        const double w = m3_wave_sum(acc[i]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][i] = w;
    }
    __syncthreads();
    if (threadIdx.x < kPart) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kThreads / M3_WAVE; ++w) s += red[w][threadIdx.x];
        next[(size_t)blockIdx.x * kPart + threadIdx.x] = s;
    }
}

// One workgroup per keyframe: the mean residual from the partials of the RESIDUAL pass.
__global__ void __launch_bounds__(kThreads) k_focal_finish(const double *__restrict__ part, int tiles,
                                                            double *__restrict__ out) {
    double s[kPart];
    keyframe_sums(part + (size_t)blockIdx.x * tiles * kPart, tiles, s);
    if (threadIdx.x == 0) out[4 * blockIdx.x + 3] = s[0] / s[2];
}

}  // namespace

extern "C" {

int64_t m3_focal_ws_bytes(int K, int N) {
    if (!focal_shape_ok(K, N)) return 0;
    return 2 * (int64_t)K * plan_of(N).tiles * kPart * (int64_t)sizeof(double);
}

int m3_focal_launches(int iters) { return iters >= 0 && iters <= 64 ? iters + 3 : 0; }

int m3_focal_estimate(const float *const *X, const float *const *C, const int32_t *Nk, int K, int N, int H, int W,
                      int use_thresh, float thresh, double cx, double cy, float z_min, int iters, void *ws,
                      int64_t ws_bytes, double *out, void *stream) {
    M3_REQUIRE(K >= 0 && N >= 1 && H >= 1 && W >= 1 && (int64_t)H * W == N && iters >= 0 && iters <= 64);
    M3_REQUIRE((use_thresh == 0 || use_thresh == 1) && z_min >= 0.f && cx - cx == 0.0 && cy - cy == 0.0);   // finite
    if (K == 0) return M3_OK;
    M3_REQUIRE(X && C && Nk && ws && out && focal_shape_ok(K, N));
    M3_REQUIRE(((uintptr_t)ws & 15) == 0 && ws_bytes >= m3_focal_ws_bytes(K, N));
    hipStream_t st = (hipStream_t)stream;
    const Plan p = plan_of(N);
    const dim3 grid(K * p.tiles), block(kThreads);
    double *buf[2] = {(double *)ws, (double *)ws + (size_t)K * p.tiles * kPart};
#define M3_FOCAL_PASS(MODE, pass)                                                                                        \
    hipLaunchKernelGGL(k_focal_pass<MODE>, grid, block, 0, st, X, C, Nk, N, W, p.tiles, p.rounds, use_thresh, thresh, cx, \
                       cy, z_min, (pass) == 1, buf[((pass) + 1) & 1], buf[(pass) & 1], out)
    M3_FOCAL_PASS(LSQ, 0);
    for (int i = 1; i <= iters; ++i) M3_FOCAL_PASS(WEISZFELD, i);
    M3_FOCAL_PASS(RESIDUAL, iters + 1);
#undef M3_FOCAL_PASS
    hipLaunchKernelGGL(k_focal_finish, dim3(K), block, 0, st, buf[(iters + 1) & 1], p.tiles, out);
    M3_CHECK_LAUNCH("m3_focal_estimate");
    return M3_OK;
}

}  // extern "C"
