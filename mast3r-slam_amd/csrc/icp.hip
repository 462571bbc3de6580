// Registration of one cloud onto another on the device: point-to-point and point-to-plane ICP over Sim(3)
// (mast3r_slam/register.py).  The rule is stated once, in include/m3slam.h; tests/icp_twin.py
// restates it in numpy and every result here equals the twin's byte for byte.
//
// The target gets the uniform-grid index of cloud_index.h once (six launches).  An iteration is two launches:
//   k_icp_accumulate<MODE>  one source row per thread: move it by the pose in the workspace, find its nearest target point
//                           (the k = 1 cross-mode rule of k_knn_query, the best key in a register), form the 36 terms of
//                           the normal equations in float64 and reduce the tile of 256 rows in the stated pairwise tree -
//                           shuffles inside a wave, one LDS exchange across the four waves;
//   k_icp_step              one workgroup: adds the tile partials (thread j takes tiles j, j + 256, ...), runs the same
//                           tree, and thread 0 solves by LDL^T, retracts with Cayley's map, sets the flags and writes
//                           the history row.
// Nothing comes back to the host between iterations: once `done` or a failure status is in the state block, the kernels
// of the remaining iterations return at once - a uniform branch, the same number of launches.  Two more launches
// evaluate the final pose.  No float atomics: the bytes do not depend on scheduling.
//
// ws: the target's index (m3_cloud_ws_bytes(Nt), padded to 16) | state double [24] | history double [iterations][5],
// padded to 16 | tile partials 8 bytes [ntile][40] (36 sums, then int64 pairs, finite rows, rows out of range, 0),
// ntile = max(1, ceil(Ns / 256)).
//
// Compiled with -ffp-contract=off: every float64 operation of the rule is rounded on its own.  No sqrt, no division
// other than the rule's.
#include "cloud_index.h"
#include "accum_dev.h"                         // kSums = 36: 28 (H upper) + 7 (g) + 1 (cost)
#pragma clang fp contract(off)

namespace {

constexpr int kPartWords = 40, kStateWords = 24, kHistWords = 5, kMaxIter = 1000;
constexpr int kWaves = kThreads / M3_WAVE;
enum { sR = 0, sT = 9, sS = 12, sIters = 13, sDone = 14, sStatus = 15, sPairs = 16, sCost = 17, sFinite = 18, sFar = 19,
       sEvalPairs = 20, sEvalCost = 21 };
enum { kStatusOk = 0, kStatusFew = 1, kStatusSingular = 2 };

struct IcpPose {
    double R[9], t[3], s;
};

struct IcpWs {
    ClWs cl;
    int64_t ntile, state, hist, part, bytes;
};

inline bool icp_layout(int64_t Ns, int64_t Nt, int iterations, IcpWs &w) {
    if (Ns < 0 || Ns > kMaxM || iterations < 0 || iterations > kMaxIter || !cl_layout(Nt, w.cl)) return false;
    w.ntile = Ns ? (Ns + kThreads - 1) / kThreads : 1;
    w.state = pad16(w.cl.bytes);
    w.hist = w.state + 8 * kStateWords;
    w.part = w.hist + pad16(8 * kHistWords * (int64_t)iterations);
    w.bytes = w.part + 8 * kPartWords * w.ntile;
    return true;
}

// Sums that are the same for every contributing row of a point-to-point tile: 1 (H00, H11, H22) or 0.  Their tree sum is
// the pair count or +0 exactly, so the wave stage takes them from the ballot instead of six shuffle levels.
__device__ __forceinline__ constexpr bool p2p_one(int i) { return i == 0 || i == 7 || i == 13; }
__device__ __forceinline__ constexpr bool p2p_zero(int i) {
    return i == 1 || i == 2 || i == 3 || i == 8 || i == 10 || i == 16 || i == 21 || i == 24 || i == 26;
}

// The stated tree over the workgroup's 256 slots: x = x[0::2] + x[1::2] eight times.  Six levels by xor shuffles (lane 0
// of a wave ends with the tree of its 64 slots; addition commutes, so every lane does), two through LDS.  Thread u < 36
// returns sum u.  FOLD: the constant sums of a point-to-point tile come from `ones`, the wave's contributing rows.
template <bool FOLD>
__device__ __forceinline__ double tree36(double (&v)[kSums], int ones, double (*lds)[kSums]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < kSums; ++i) {
        if (FOLD && p2p_one(i)) {
            v[i] = (double)ones;
        } else if (FOLD && p2p_zero(i)) {
            v[i] = 0.0;
        } else {
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) v[i] += __shfl_xor(v[i], o, 64);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < kSums; ++i) lds[w][i] = v[i];
    }
    __syncthreads();
    const int u = threadIdx.x < kSums ? threadIdx.x : 0;
    return (lds[0][u] + lds[1][u]) + (lds[2][u] + lds[3][u]);
}

// MODE 0: point to point; 1: point to plane.  first: the pose is `init`, the state block is not read.  always: the
// evaluation launch, which ignores the flags.
template <int MODE>
__global__ void __launch_bounds__(kThreads) k_icp_accumulate(const float *__restrict__ source, int64_t Ns,
                                                              const float *__restrict__ target,
                                                              const float *__restrict__ normals, int64_t Nt,
                                                              const Ent *__restrict__ sorted, const int32_t *__restrict__ start,
                                                              const unsigned long long *__restrict__ keys, int64_t S,
                                                              const int32_t *__restrict__ hdr, double h, double r2,
                                                              const double *__restrict__ state, IcpPose init, int first, int always,
                                                              double *__restrict__ part, int32_t *__restrict__ pairs_out) {
    __shared__ double lds[kWaves][kSums];
    __shared__ int cnt[kWaves][3];
    if (!first && !always && (state[sDone] != 0.0 || state[sStatus] != 0.0)) return;       // uniform
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = first ? init.R[k] : state[sR + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = first ? init.t[k] : state[sT + k];
    const double s = first ? init.s : state[sS];

    const int64_t i = row_of();
    const int64_t n_in = hdr[kInCells] < Nt ? hdr[kInCells] : Nt;
    const unsigned long long mask = (unsigned long long)(S - 1);
    bool fin = false, far = false, active = false, has = false, adds = false;
    double px = 0.0, py = 0.0, pz = 0.0;
    int bx = 0, by = 0, bz = 0;
    int64_t j = -1;
    if (i < Ns) {
        const double x = (double)source[3 * i], y = (double)source[3 * i + 1], z = (double)source[3 * i + 2];
        px = s * ((R[0] * x + R[1] * y) + R[2] * z) + t[0];
        py = s * ((R[3] * x + R[4] * y) + R[5] * z) + t[1];
        pz = s * ((R[6] * x + R[7] * y) + R[8] * z) + t[2];
        const float qx = (float)px, qy = (float)py, qz = (float)pz;
        fin = finite3(qx, qy, qz);
        if (fin) {
            active = cell_of(qx, qy, qz, h, bx, by, bz);
            far = !active;
        }
        if (active) {
            const double ux = (double)qx, uy = (double)qy, uz = (double)qz;
            unsigned long long best = ~0ull;
#pragma unroll 1
            for (int c = 0; c < 27; ++c) {
                const int ox = c % 3 - 1, oy = (c / 3) % 3 - 1, oz = c / 9 - 1;
                const int nx = bx + ox, ny = by + oy, nz = bz + oz;
                if (nx < 1 || nx > kCellMask || ny < 1 || ny > kCellMask || nz < 1 || nz > kCellMask) continue;
                int64_t b = 0, e = 0;
                const unsigned long long want = cell_key(nx, ny, nz);
                unsigned long long sl = mix64(want) & mask;
                for (int64_t probe = 0; probe < S; ++probe) {
                    const unsigned long long cur = keys[sl];
                    if (cur == want) {
                        b = start[sl];
                        e = start[sl + 1];
                        break;
                    }
                    if (cur == kEmptyKey) break;
                    sl = (sl + 1) & mask;
                }
                if (b < 0 || e < b || e > n_in) b = e = 0;                      // never, for a ws from the same target
                for (int64_t kk = b; kk < e; ++kk) {
                    const Ent q = sorted[kk];
                    const double dx = (double)q.x - ux, dy = (double)q.y - uy, dz = (double)q.z - uz;
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    if (!(d2 <= r2)) continue;
                    const unsigned long long key = knn_key(d2, q.i);
                    if (!has || key < best) best = key, has = true;
                }
            }
            if (has) {
                j = (int64_t)(best & kRowMask);
                if (j >= Nt) has = false, j = -1;                               // never, for a ws from the same target
            }
        }
        if (pairs_out) pairs_out[i] = (int32_t)j;
    }

    double v[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) v[k] = 0.0;
    if (has) {
        const double e0 = px - (double)target[3 * j], e1 = py - (double)target[3 * j + 1], e2 = pz - (double)target[3 * j + 2];
        if (MODE == 0) {
            adds = true;
            v[0] = 1.0;  v[4] = pz;   v[5] = -py;  v[6] = px;
            v[7] = 1.0;  v[9] = -pz;  v[11] = px;  v[12] = py;
            v[13] = 1.0; v[14] = py;  v[15] = -px; v[17] = pz;
            v[18] = py * py + pz * pz; v[19] = -(px * py); v[20] = -(px * pz);
            v[22] = px * px + pz * pz; v[23] = -(py * pz);
            v[25] = px * px + py * py;
            v[27] = (px * px + py * py) + pz * pz;
            v[28] = e0; v[29] = e1; v[30] = e2;
            v[31] = py * e2 - pz * e1;
            v[32] = pz * e0 - px * e2;
            v[33] = px * e1 - py * e0;
            v[34] = (px * e0 + py * e1) + pz * e2;
            v[35] = (e0 * e0 + e1 * e1) + e2 * e2;
        } else {
            const float f0 = normals[3 * j], f1 = normals[3 * j + 1], f2 = normals[3 * j + 2];
            adds = finite3(f0, f1, f2) && !(f0 == 0.f && f1 == 0.f && f2 == 0.f);
            if (adds) {
                const double n0 = (double)f0, n1 = (double)f1, n2 = (double)f2;
                double J[7];
                J[0] = n0; J[1] = n1; J[2] = n2;
                J[3] = py * n2 - pz * n1;
                J[4] = pz * n0 - px * n2;
                J[5] = px * n1 - py * n0;
                J[6] = (n0 * px + n1 * py) + n2 * pz;
                const double rho = (n0 * e0 + n1 * e1) + n2 * e2;
                int at = 0;
#pragma unroll
                for (int a = 0; a < 7; ++a) {
#pragma unroll
                    for (int b = a; b < 7; ++b) v[at++] = J[a] * J[b];
                }
#pragma unroll
                for (int a = 0; a < 7; ++a) v[28 + a] = J[a] * rho;
                v[35] = rho * rho;
            }
        }
    }
    const unsigned long long ba = __ballot(adds), bf = __ballot(fin), bo = __ballot(far);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        cnt[w][0] = (int)__popcll(ba);
        cnt[w][1] = (int)__popcll(bf);
        cnt[w][2] = (int)__popcll(bo);
    }
    const double sum = tree36<MODE == 0>(v, (int)__popcll(ba), lds);           // its barrier covers cnt
    double *row = part + (int64_t)blockIdx.x * kPartWords;
    if (threadIdx.x < kSums) {
        row[threadIdx.x] = sum;
    } else if (threadIdx.x < kSums + 3) {
        const int c = threadIdx.x - kSums;
        ((int64_t *)row)[threadIdx.x] = (int64_t)((cnt[0][c] + cnt[1][c]) + (cnt[2][c] + cnt[3][c]));
    } else if (threadIdx.x == kSums + 3) {
        ((int64_t *)row)[threadIdx.x] = 0;
    }
}

// H delta = -g by LDL^T without pivoting on the leading N x N block; sums: the 36 reduced sums.  False: a pivot with
// d <= 1e-12 H_jj, or one that is not finite.
template <int N>
__device__ __forceinline__ bool ldl_solve(const double *sums, double (&delta)[7]) {
    double H[N][N], L[N][N], d[N], y[N];
    {
        int at = 0;
#pragma unroll
        for (int a = 0; a < 7; ++a) {
#pragma unroll
            for (int b = a; b < 7; ++b) {
                if (a < N && b < N) H[a][b] = sums[at];
                ++at;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double wk[N];
        double p = H[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) {
            wk[k] = L[j][k] * d[k];
            p = p - L[j][k] * wk[k];
        }
        d[j] = p;
        if (p <= 1e-12 * H[j][j] || !isfinite(p)) return false;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double a = H[j][i];
#pragma unroll
            for (int k = 0; k < j; ++k) a = a - L[i][k] * wk[k];
            L[i][j] = a / p;
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double a = -sums[28 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) a = a - L[i][k] * y[k];
        y[i] = a;
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double a = y[i] / d[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) a = a - L[k][i] * delta[k];
        delta[i] = a;
    }
#pragma unroll
    for (int i = N; i < 7; ++i) delta[i] = 0.0;
    return true;
}

// eval: reduce only - the evaluation launch and m3_icp_sums; sums_out / count_out may be NULL.
__global__ void __launch_bounds__(kThreads) k_icp_step(const double *__restrict__ part, int64_t ntile, double *__restrict__ state,
                                                        double *__restrict__ hist, int iterations, IcpPose init, int first, int eval,
                                                        int with_scale, int64_t min_pairs, double tol, double radius,
                                                        double *__restrict__ sums_out, int64_t *__restrict__ count_out) {
    __shared__ double lds[kWaves][kSums];
    __shared__ double tot[kSums];
    __shared__ unsigned long long cnt[3];
    if (!first && !eval && (state[sDone] != 0.0 || state[sStatus] != 0.0)) return;         // uniform
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0ull;
    __syncthreads();
    double v[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) v[k] = 0.0;
    unsigned long long n0 = 0, n1 = 0, n2 = 0;
    for (int64_t tl = threadIdx.x; tl < ntile; tl += kThreads) {
        const double *row = part + tl * kPartWords;
#pragma unroll
        for (int k = 0; k < kSums; ++k) v[k] += row[k];
        const unsigned long long *ir = (const unsigned long long *)row;
        n0 += ir[kSums], n1 += ir[kSums + 1], n2 += ir[kSums + 2];
    }
    if (n0) atomicAdd(cnt + 0, n0);                                             // integers: the order does not matter
    if (n1) atomicAdd(cnt + 1, n1);
    if (n2) atomicAdd(cnt + 2, n2);
    const double sum = tree36<false>(v, 0, lds);
    if (threadIdx.x < kSums) tot[threadIdx.x] = sum;
    __syncthreads();
    const int64_t pairs = (int64_t)cnt[0];
    if (eval) {
        if (sums_out && threadIdx.x < kSums) sums_out[threadIdx.x] = sum;
        if (count_out && threadIdx.x < 3) count_out[threadIdx.x] = (int64_t)cnt[threadIdx.x];
    }
    if (threadIdx.x != 0) return;
    if (first) {
#pragma unroll
        for (int k = 0; k < 9; ++k) state[sR + k] = init.R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) state[sT + k] = init.t[k];
        state[sS] = init.s;
#pragma unroll
        for (int k = sIters; k < kStateWords; ++k) state[k] = 0.0;
    }
    state[sFinite] = (double)cnt[1];
    state[sFar] = (double)cnt[2];
    if (eval) {
        state[sEvalPairs] = (double)pairs;
        state[sEvalCost] = tot[35];
        return;
    }
    const double itd = first ? 0.0 : state[sIters];
    state[sPairs] = (double)pairs;
    state[sCost] = tot[35];
    state[sIters] = itd + 1.0;
    double delta[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int status = kStatusOk;
    if (pairs < min_pairs) status = kStatusFew;
    else if (!(with_scale ? ldl_solve<7>(tot, delta) : ldl_solve<6>(tot, delta))) status = kStatusSingular;
    double tt = 0.0, ww = 0.0, sg = 0.0;
    if (status == kStatusOk) {
        const double a0 = delta[3] * 0.5, a1 = delta[4] * 0.5, a2 = delta[5] * 0.5;
        const double c = 2.0 / (1.0 + ((a0 * a0 + a1 * a1) + a2 * a2));
        double D[9];
        D[0] = 1.0 + c * -(a1 * a1 + a2 * a2);
        D[1] = c * (a0 * a1 - a2);
        D[2] = c * (a0 * a2 + a1);
        D[3] = c * (a0 * a1 + a2);
        D[4] = 1.0 + c * -(a0 * a0 + a2 * a2);
        D[5] = c * (a1 * a2 - a0);
        D[6] = c * (a0 * a2 - a1);
        D[7] = c * (a1 * a2 + a0);
        D[8] = 1.0 + c * -(a0 * a0 + a1 * a1);
        sg = delta[6];
        const double k = 1.0 + sg;
        double R[9], t[3];
#pragma unroll
        for (int q = 0; q < 9; ++q) R[q] = state[sR + q];
#pragma unroll
        for (int q = 0; q < 3; ++q) t[q] = state[sT + q];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = 0; b < 3; ++b) state[sR + 3 * a + b] = (D[3 * a] * R[b] + D[3 * a + 1] * R[3 + b]) + D[3 * a + 2] * R[6 + b];
            state[sT + a] = k * ((D[3 * a] * t[0] + D[3 * a + 1] * t[1]) + D[3 * a + 2] * t[2]) + delta[a];
        }
        state[sS] = k * state[sS];
        tt = (delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2];
        ww = (delta[3] * delta[3] + delta[4] * delta[4]) + delta[5] * delta[5];
        const double tr = tol * radius;
        if (tt <= tr * tr && ww <= tol * tol && sg * sg <= tol * tol) state[sDone] = 1.0;
    } else {
        state[sStatus] = (double)status;
    }
    if (itd >= 0.0 && itd < (double)iterations) {                               // always, for a state of this call
        double *hr = hist + (int64_t)itd * kHistWords;
        hr[0] = (double)pairs;
        hr[1] = tot[35];
        hr[2] = tt;
        hr[3] = ww;
        hr[4] = sg;
    }
}

struct IcpArgs {
    const float *source, *target, *normals;
    int64_t Ns, Nt;
    float radius;
    int mode;
    const double *pose;
    void *ws;
    int64_t ws_bytes;
};

inline bool icp_args_ok(const IcpArgs &a, int iterations, IcpWs &w) {
    return icp_layout(a.Ns, a.Nt, iterations, w) && ws_ok(a.ws) && a.ws_bytes >= w.bytes && radius_ok(a.radius) &&
           (a.mode == 0 || a.mode == 1) && (a.mode == 0 || a.normals || a.Nt == 0) && a.pose && (a.source || a.Ns == 0) &&
           (a.target || a.Nt == 0) && aligned(a.source, 4) && aligned(a.target, 4) && aligned(a.normals, 4) && aligned(a.pose, 8);
}

inline IcpPose pose_of(const double *p) {
    IcpPose q;
    for (int k = 0; k < 9; ++k) q.R[k] = p[k];
    for (int k = 0; k < 3; ++k) q.t[k] = p[9 + k];
    q.s = p[12];
    return q;
}

void launch_accumulate(hipStream_t st, const IcpArgs &a, const IcpWs &w, int mode, const IcpPose &init, int first, int always,
                       int32_t *pairs) {
    const ClPtr p = cl_ptr(a.ws, w.cl);
    const double r = (double)a.radius;
    const double *state = (const double *)((char *)a.ws + w.state);
    double *part = (double *)((char *)a.ws + w.part);
    if (mode == 0)
        hipLaunchKernelGGL(k_icp_accumulate<0>, dim3((unsigned)w.ntile), dim3(kThreads), 0, st, a.source, a.Ns, a.target, a.normals,
                           a.Nt, p.sorted, p.start, p.keys, w.cl.S, p.hdr, cell_edge(a.radius), r * r, state, init, first, always,
                           part, pairs);
    else
        hipLaunchKernelGGL(k_icp_accumulate<1>, dim3((unsigned)w.ntile), dim3(kThreads), 0, st, a.source, a.Ns, a.target, a.normals,
                           a.Nt, p.sorted, p.start, p.keys, w.cl.S, p.hdr, cell_edge(a.radius), r * r, state, init, first, always,
                           part, pairs);
}

void launch_step(hipStream_t st, const IcpArgs &a, const IcpWs &w, int iterations, const IcpPose &init, int first, int eval,
                 int with_scale, int64_t min_pairs, double tol, double *sums, int64_t *count) {
    char *ws = (char *)a.ws;
    hipLaunchKernelGGL(k_icp_step, dim3(1), dim3(kThreads), 0, st, (const double *)(ws + w.part), w.ntile, (double *)(ws + w.state),
                       (double *)(ws + w.hist), iterations, init, first, eval, with_scale, min_pairs, tol, (double)a.radius, sums,
                       count);
}

}  // namespace

extern "C" {

int64_t m3_icp_ws_bytes(int64_t Ns, int64_t Nt, int iterations) {
    IcpWs w;
    return icp_layout(Ns, Nt, iterations, w) ? w.bytes : 0;
}

int m3_icp_launches(int iterations) {
    return iterations >= 0 && iterations <= kMaxIter ? kIndexLaunches + 2 * iterations + 2 : 0;
}

int m3_icp_sums(const float *source, int64_t Ns, const float *target, const float *target_normals, int64_t Nt, float radius,
                int mode, const double *pose, int64_t *count, double *sums, int32_t *pairs, void *ws, int64_t ws_bytes,
                void *stream) {
    IcpWs w;
    const IcpArgs a{source, target, target_normals, Ns, Nt, radius, mode, pose, ws, ws_bytes};
    M3_REQUIRE(icp_args_ok(a, 0, w) && count && sums && aligned(count, 8) && aligned(sums, 8) && aligned(pairs, 4));
    hipStream_t st = (hipStream_t)stream;
    const IcpPose init = pose_of(pose);
    launch_index(st, target, Nt, radius, ws, w.cl, nullptr, nullptr);
    launch_accumulate(st, a, w, mode, init, 1, 1, pairs);
    launch_step(st, a, w, 0, init, 1, 1, 0, 1, 0.0, sums, count);
    M3_CHECK_LAUNCH("m3_icp_sums");
    return M3_OK;
}

int m3_icp_register(const float *source, int64_t Ns, const float *target, const float *target_normals, int64_t Nt,
                    float radius, int mode, const double *pose, int with_scale, int iterations, double tol, int64_t min_pairs,
                    int32_t *pairs, void *ws, int64_t ws_bytes, void *stream) {
    IcpWs w;
    const IcpArgs a{source, target, target_normals, Ns, Nt, radius, mode, pose, ws, ws_bytes};
    M3_REQUIRE(iterations >= 0 && iterations <= kMaxIter && icp_args_ok(a, iterations, w) && aligned(pairs, 4));
    M3_REQUIRE(min_pairs >= 1 && tol >= 0.0 && tol < (double)INFINITY && (with_scale == 0 || with_scale == 1));
    hipStream_t st = (hipStream_t)stream;
    const IcpPose init = pose_of(pose);
    launch_index(st, target, Nt, radius, ws, w.cl, nullptr, nullptr);
    for (int it = 0; it < iterations; ++it) {
        launch_accumulate(st, a, w, mode, init, it == 0, 0, nullptr);
        launch_step(st, a, w, iterations, init, it == 0, 0, with_scale, min_pairs, tol, nullptr, nullptr);
    }
    launch_accumulate(st, a, w, 0, init, iterations == 0, 1, pairs);
    launch_step(st, a, w, iterations, init, iterations == 0, 1, with_scale, min_pairs, tol, nullptr, nullptr);
    M3_CHECK_LAUNCH("m3_icp_register");
    return M3_OK;
}

}  // extern "C"
