// Fixed-radius neighbourhoods of a point cloud on a uniform grid, and the two passes on top of them: normals from the
// neighbourhood moments and the radius outlier filter (mast3r_slam/cloud.py).
// The rule is stated once, in include/m3slam.h; tests/cloud_twin.py restates it in numpy.
//
// index:  clear -> one thread per point (claim the slot of its cell's key, take a rank in the cell; a point without a
//         cell writes its zero outputs here) -> cell counts per tile of 256 slots -> scan of the tiles -> cell starts =
//         tile offset + rank -> one thread per point writes (x, y, z, i) at its cell's start + its rank -> one thread
//         per entry of that list walks the 27 cells around its own (the hot path).
// Seven launches whatever the cloud holds.  The only atomics are integer ones whose results commute: CAS to claim a
// slot, add for the rank and the header.  Which slot a cell lands in and where in its cell a point lands depend on the
// arrival order; count and moments are integer sums over a set, so nothing that is output does.  No thread waits for
// another.
//
// Why 27 cells are enough.  The cell of p is floor(fl(p / h)) per axis, h = r (1 + 2^-10): r has 24 significant bits
// and 1 + 2^-10 eleven, so h is exact in float64.  Let j be a neighbour of i: d2 <= r r, where r r is exact and d2 is
// rounded three times, each operand a non-negative float64.  So dx dx <= r r (1 + 2^-52)^3 and |dx| <= r (1 + 2^-51)
// for the rounded difference dx, and |p_j - p_i| <= r (1 + 2^-50) for the exact one.  The exact quotients then differ by
// at most (1 + 2^-50) / (1 + 2^-10) < 1 - 2^-11.  A point with a cell has |fl(p / h)| < 2^20 + 1, so the division
// moves each quotient by at most 2^-32: the computed quotients differ by less than 1 - 2^-11 + 2^-31 < 1, and their
// floors by at most 1 - on every axis, near a power of two or not.  A float32 floorf(p / r) has no such margin: two
// points exactly r apart can land two cells apart.
//
// The queries run in the order of the cell-sorted list: the lanes of a wave that share a cell walk the same 27 ranges,
// so their 16-byte loads are one address per wave, and the range of a cell is contiguous.  The cells themselves lie in
// table order, which is hash order: neighbouring cells are not neighbours in memory (DESIGN.md 7o has what that costs).
//
// ws: int32 [16] header | tile int32 [ceil((S + 1) / 256)] | start int32 [S + 1] | keys uint64 [S] | slot uint32 [M] |
// rank int32 [M] | sslot uint32 [M] | sorted 16 bytes [M]; S = the power of two >= max(1024, 2 M).  Header words:
// [0] points out of range, [1] points that have a cell (the total of the scan), [2] rows a filter keeps, [3] k-NN
// queries out of range, [4] complete rows of the statistical filter, bytes 24 ... 47 its three 64-bit sums; the others
// are 0.  The filters keep their tile offsets in the tile array.
//
// On the same index: the k nearest within the radius - the six build launches and one query
// kernel of its own - and on top of them the statistical outlier filter and the moments over the k nearest.
//
// Compiled with -ffp-contract=off: every float64 operation of the rule is rounded on its own.
#include "cloud_index.h"                       // the index itself: layout, cell_of, the six build launches, the key
#pragma clang fp contract(off)

namespace {

constexpr int kBuildLaunches = 7;
constexpr int kSweeps = 10;                           // cyclic Jacobi on 3 x 3: converged after five or six

// One entry of the cell-sorted list per thread: the 27 cells around its own, each looked up in the table and walked
// from start to end, one 16-byte load per candidate.  n_in = hdr[kInCells] entries exist.
template <bool MOMENTS>
__global__ void __launch_bounds__(kThreads) k_cl_query(const Ent *__restrict__ sorted, const uint32_t *__restrict__ sslot,
                                                        const int32_t *__restrict__ start,
                                                        const unsigned long long *__restrict__ keys, int64_t S, int64_t M,
                                                        const int32_t *__restrict__ hdr, double r2, double scale,
                                                        int32_t *__restrict__ count, int64_t *__restrict__ moments) {
    const int64_t t = row_of();
    const int64_t n_in = hdr[kInCells] < M ? hdr[kInCells] : M;
    if (t >= n_in) return;
    const Ent me = sorted[t];
    const uint32_t s0 = sslot[t];
    if ((int64_t)s0 >= S || me.i < 0 || me.i >= M) return;                      // never, for a ws from the same points
    const unsigned long long key = keys[s0], mask = (unsigned long long)(S - 1);
    const int bx = (int)(key >> 42) & kCellMask, by = (int)(key >> 21) & kCellMask, bz = (int)key & kCellMask;
    const double px = (double)me.x, py = (double)me.y, pz = (double)me.z;
    int n = 0;
    int64_t a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0, a6 = 0, a7 = 0, a8 = 0;
#pragma unroll 1
    for (int c = 0; c < 27; ++c) {
        const int ox = c % 3 - 1, oy = (c / 3) % 3 - 1, oz = c / 9 - 1;
        const int nx = bx + ox, ny = by + oy, nz = bz + oz;
        if (nx < 1 || nx > kCellMask || ny < 1 || ny > kCellMask || nz < 1 || nz > kCellMask) continue;   // holds no point
        int64_t b = 0, e = 0;
        const unsigned long long want = cell_key(nx, ny, nz);
        unsigned long long s = c == 13 ? (unsigned long long)s0 : mix64(want) & mask;
        for (int64_t probe = 0; probe < S; ++probe) {
            const unsigned long long cur = keys[s];
            if (cur == want) {
                b = start[s];
                e = start[s + 1];
                break;
            }
            if (cur == kEmptyKey) break;
            s = (s + 1) & mask;
        }
        if (b < 0 || e < b || e > n_in) b = e = 0;                              // never, for a ws from the same points
        for (int64_t k = b; k < e; ++k) {
            const Ent q = sorted[k];
            const double dx = (double)q.x - px, dy = (double)q.y - py, dz = (double)q.z - pz;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            const bool in = d2 <= r2;
            n += in ? 1 : 0;
            if (MOMENTS) {
                // |q| <= 2^21 + 1 by the entry point's test of scale * r: the products are 32 x 32 -> 64 bits
                const int qx = (int)rint(in ? dx * scale : 0.0), qy = (int)rint(in ? dy * scale : 0.0),
                          qz = (int)rint(in ? dz * scale : 0.0);
                a0 += qx;
                a1 += qy;
                a2 += qz;
                a3 += (int64_t)qx * qx;
                a4 += (int64_t)qx * qy;
                a5 += (int64_t)qx * qz;
                a6 += (int64_t)qy * qy;
                a7 += (int64_t)qy * qz;
                a8 += (int64_t)qz * qz;
            }
        }
    }
    count[me.i] = n;
    if (MOMENTS) {
        int64_t *row = moments + 9 * (int64_t)me.i;
        row[0] = a0; row[1] = a1; row[2] = a2; row[3] = a3; row[4] = a4; row[5] = a5; row[6] = a6; row[7] = a7; row[8] = a8;
    }
}

// ---- normals ---------------------------------------------------------------------------------------------------------
// |v| < 2^127, rounded twice at most: the high and the low word of |v| are converted and added.
__device__ __forceinline__ double to_double(__int128 v) {
    const bool neg = v < 0;
    const unsigned __int128 a = neg ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
    const double d = (double)(unsigned long long)(a >> 64) * 18446744073709551616.0 + (double)(unsigned long long)a;
    return neg ? -d : d;
}

// One Jacobi rotation in the (P, Q) plane of the symmetric A, accumulated into the columns of V; R is the third axis.
template <int P, int Q, int R>
__device__ __forceinline__ void rotate(double (&A)[3][3], double (&V)[3][3]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));     // theta^2 = inf: t = 0
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[P][P] -= t * apq;
    A[Q][Q] += t * apq;
    A[P][Q] = A[Q][P] = 0.0;
    const double arp = A[R][P], arq = A[R][Q];
    A[R][P] = A[P][R] = c * arp - s * arq;
    A[R][Q] = A[Q][R] = s * arp + c * arq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vp = V[k][P], vq = V[k][Q];
        V[k][P] = c * vp - s * vq;
        V[k][Q] = s * vp + c * vq;
    }
}

// One point per thread: n S2 - S1 S1^T exactly, its eigenvector of the smallest eigenvalue, the orientation.
__global__ void __launch_bounds__(kThreads) k_cl_normals(const float *__restrict__ points, int64_t M,
                                                          const int32_t *__restrict__ count, const int64_t *__restrict__ moments,
                                                          const float *__restrict__ toward, int toward_stride, int min_points,
                                                          float *__restrict__ normals, float *__restrict__ variation) {
    const int64_t i = row_of();
    if (i >= M) return;
    float out[3] = {0.f, 0.f, 0.f}, var = 0.f;
    const int n = count[i];
    const float px = points[3 * i], py = points[3 * i + 1], pz = points[3 * i + 2];
    if (n >= min_points && n >= 1 && finite3(px, py, pz)) {
        int64_t m[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = moments[9 * i + k];
        const __int128 nn = n;
        const __int128 d00 = nn * m[3] - (__int128)m[0] * m[0], d01 = nn * m[4] - (__int128)m[0] * m[1],
                       d02 = nn * m[5] - (__int128)m[0] * m[2], d11 = nn * m[6] - (__int128)m[1] * m[1],
                       d12 = nn * m[7] - (__int128)m[1] * m[2], d22 = nn * m[8] - (__int128)m[2] * m[2];
        if (d00 + d11 + d22 != 0) {
            double A[3][3] = {{to_double(d00), to_double(d01), to_double(d02)},
                              {to_double(d01), to_double(d11), to_double(d12)},
                              {to_double(d02), to_double(d12), to_double(d22)}};
            double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll 1
            for (int sweep = 0; sweep < kSweeps; ++sweep) {
                rotate<0, 1, 2>(A, V);
                rotate<0, 2, 1>(A, V);
                rotate<1, 2, 0>(A, V);
            }
            const double l[3] = {A[0][0], A[1][1], A[2][2]};
            const int k = l[1] < l[0] ? (l[2] < l[1] ? 2 : 1) : (l[2] < l[0] ? 2 : 0);    // the smallest; a tie: the lower
            double u[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) u[a] = k == 0 ? V[a][0] : k == 1 ? V[a][1] : V[a][2];
            const double len = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
            const double l0 = k == 0 ? l[0] : k == 1 ? l[1] : l[2], sum = (l[0] + l[1]) + l[2];
            if (len > 0.0 && sum > 0.0) {
#pragma unroll
                for (int a = 0; a < 3; ++a) out[a] = (float)(u[a] / len);
                var = (float)((l0 > 0.0 ? l0 : 0.0) / sum);
                bool flip;
                if (toward) {
                    const float *c = toward + (int64_t)toward_stride * i;
                    const double dot = ((double)out[0] * ((double)c[0] - (double)px) + (double)out[1] * ((double)c[1] - (double)py)) +
                                       (double)out[2] * ((double)c[2] - (double)pz);
                    flip = dot < 0.0;
                } else {
                    const float ax = fabsf(out[0]), ay = fabsf(out[1]), az = fabsf(out[2]);
                    const float lead = ax >= ay && ax >= az ? out[0] : ay >= az ? out[1] : out[2];
                    flip = lead < 0.f;
                }
                if (flip) {
#pragma unroll
                    for (int a = 0; a < 3; ++a) out[a] = -out[a];
                }
            }
        }
    }
    normals[3 * i] = out[0];
    normals[3 * i + 1] = out[1];
    normals[3 * i + 2] = out[2];
    if (variation) variation[i] = var;
}

// ---- the filters' ordered compaction ---------------------------------------------------------------------------------
// Bits of the thread's four consecutive rows whose value v has lo < v <= hi.  The radius filter: v = count, lo =
// min_neighbors (the point itself and min_neighbors others at least), hi = INT32_MAX.  The statistical filter: v = q,
// lo = -1 (a complete row), hi = floor(T).
__device__ __forceinline__ unsigned kept_rows(const int32_t *__restrict__ v, int64_t i0, int64_t M, int lo, int hi) {
    unsigned keep = 0;
#pragma unroll
    for (int j = 0; j < kPts; ++j) {
        if (i0 + j < M && v[i0 + j] > lo && v[i0 + j] <= hi) keep |= 1u << j;
    }
    return keep;
}

__global__ void __launch_bounds__(kThreads) k_cl_keep_count(const int32_t *__restrict__ count, int64_t M, int lo, int hi,
                                                             int32_t *__restrict__ cnt) {
    const unsigned keep = kept_rows(count, (int64_t)blockIdx.x * kTile + threadIdx.x * kPts, M, lo, hi);
    int total;
    block_prefix(keep, total);
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kThreads) k_cl_keep_scatter(const float *__restrict__ points,
                                                               const unsigned char *__restrict__ colors,
                                                               const int64_t *__restrict__ index,
                                                               const int32_t *__restrict__ count, int64_t M, int lo, int hi,
                                                               const int32_t *__restrict__ offs, int64_t M2,
                                                               float *__restrict__ points_out,
                                                               unsigned char *__restrict__ colors_out,
                                                               int64_t *__restrict__ index_out, int64_t *__restrict__ rows_out) {
    const int64_t i0 = (int64_t)blockIdx.x * kTile + threadIdx.x * kPts;
    const unsigned keep = kept_rows(count, i0, M, lo, hi);
    int total;
    int64_t o = (int64_t)offs[blockIdx.x] + block_prefix(keep, total);
#pragma unroll
    for (int j = 0; j < kPts; ++j) {
        if (!((keep >> j) & 1u) || o < 0 || o >= M2) continue;                  // o < M2 always holds for a ws from the same count
        const int64_t i = i0 + j;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            points_out[3 * o + d] = points[3 * i + d];
            if (colors_out) colors_out[3 * o + d] = colors[3 * i + d];
        }
        if (index_out) index_out[o] = index ? index[i] : i;
        if (rows_out) rows_out[o] = i;
        ++o;
    }
}

// ---- k nearest within the radius -------------------------------------------------------------------------------------
// One query per thread.  Self mode (CROSS false): thread t takes entry t of the cell-sorted list, as k_cl_query does,
// so the lanes that share a cell walk the same ranges; as row t it also writes the empty outputs of a point without a
// cell, which is in no list.  Cross mode: thread t takes query row t, and its lanes diverge over the cells.
//
// The k best keys live in LDS, column layout [k][THREADS] of 64-bit words: entry e of lane l is word e * THREADS + l,
// so a wave's access to one entry is 512 contiguous bytes and no lane ever touches another's column - no barrier.  The
// worst key of the list and its position stay in registers: a candidate costs d2, the radius test and one 64-bit
// compare; only one that enters pays the scan of k words for the new worst.  The list is sorted once at the end
// (insertion sort in LDS) and written out with d2 recomputed from the stored rows.
// THREADS falls as k grows - 256 up to k = 16, 128 up to 32, 64 up to 64 - so that a workgroup never holds more than
// 8 k THREADS <= 32 KB of the CU's 160 KB and five workgroups fit whatever k is (the launch passes exactly 8 k THREADS).
constexpr int kKnnMaxK = 64;
constexpr int kQueriesFar = 3, kComplete = 4;                                   // header words (int32)
constexpr int kSumQ = 3, kSumQQLo = 4, kSumQQHi = 5;                            // header words (uint64): bytes 24 ... 47

__device__ __forceinline__ void knn_empty(int64_t row, int k, int32_t *__restrict__ index, float *__restrict__ dist2,
                                          int32_t *__restrict__ found, int from = 0) {
    for (int e = from; e < k; ++e) {
        index[row * k + e] = -1;
        dist2[row * k + e] = INFINITY;
    }
    if (from == 0) found[row] = 0;
}

template <int THREADS, bool CROSS>
__global__ void __launch_bounds__(THREADS) k_knn_query(const float *__restrict__ points, const float *__restrict__ queries,
                                                        int64_t Q, const Ent *__restrict__ sorted,
                                                        const uint32_t *__restrict__ sslot, const uint32_t *__restrict__ slot,
                                                        const int32_t *__restrict__ start,
                                                        const unsigned long long *__restrict__ keys, int64_t S, int64_t M,
                                                        int32_t *__restrict__ hdr, double h, double r2, int k,
                                                        int32_t *__restrict__ index, float *__restrict__ dist2,
                                                        int32_t *__restrict__ found) {
    extern __shared__ unsigned long long knn_lds[];
    unsigned long long *mine = knn_lds + threadIdx.x;                           // entry e: mine[e * THREADS]
    const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const int64_t n_in = hdr[kInCells] < M ? hdr[kInCells] : M;
    const unsigned long long mask = (unsigned long long)(S - 1);
    bool active = false, far = false;
    int64_t row = 0;
    int32_t self = -1;
    uint32_t s0 = kNoSlot;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    int bx = 0, by = 0, bz = 0;
    if (CROSS) {
        if (t < Q) {
            row = t;
            qx = queries[3 * t], qy = queries[3 * t + 1], qz = queries[3 * t + 2];
            if (finite3(qx, qy, qz)) {
                active = cell_of(qx, qy, qz, h, bx, by, bz);
                far = !active;
            }
            if (!active) knn_empty(row, k, index, dist2, found);
        }
        const unsigned long long b = __ballot(far);
        if (b && (threadIdx.x & 63) == 0) atomicAdd(hdr + kQueriesFar, (int)__popcll(b));
    } else {
        if (t < M && slot[t] == kNoSlot) knn_empty(t, k, index, dist2, found);
        if (t < n_in) {
            const Ent me = sorted[t];
            s0 = sslot[t];
            if ((int64_t)s0 < S && me.i >= 0 && me.i < M) {                     // always, for a ws from the same points
                active = true;
                row = self = me.i;
                qx = me.x, qy = me.y, qz = me.z;
                const unsigned long long key = keys[s0];
                bx = (int)(key >> 42) & kCellMask, by = (int)(key >> 21) & kCellMask, bz = (int)key & kCellMask;
            }
        }
    }
    if (!active) return;
    const double px = (double)qx, py = (double)qy, pz = (double)qz;
    int cnt = 0, wpos = 0;
    unsigned long long worst = 0;
#pragma unroll 1
    for (int c = 0; c < 27; ++c) {
        const int ox = c % 3 - 1, oy = (c / 3) % 3 - 1, oz = c / 9 - 1;
        const int nx = bx + ox, ny = by + oy, nz = bz + oz;
        if (nx < 1 || nx > kCellMask || ny < 1 || ny > kCellMask || nz < 1 || nz > kCellMask) continue;   // holds no point
        int64_t b = 0, e = 0;
        const unsigned long long want = cell_key(nx, ny, nz);
        unsigned long long s = !CROSS && c == 13 ? (unsigned long long)s0 : mix64(want) & mask;
        for (int64_t probe = 0; probe < S; ++probe) {
            const unsigned long long cur = keys[s];
            if (cur == want) {
                b = start[s];
                e = start[s + 1];
                break;
            }
            if (cur == kEmptyKey) break;
            s = (s + 1) & mask;
        }
        if (b < 0 || e < b || e > n_in) b = e = 0;                              // never, for a ws from the same points
        for (int64_t kk = b; kk < e; ++kk) {
            const Ent q = sorted[kk];
            const double dx = (double)q.x - px, dy = (double)q.y - py, dz = (double)q.z - pz;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (!(d2 <= r2) || (!CROSS && q.i == self)) continue;
            const unsigned long long key = knn_key(d2, q.i);
            if (cnt < k) {
                mine[cnt * THREADS] = key;
                if (cnt == 0 || key > worst) worst = key, wpos = cnt;
                ++cnt;
            } else if (key < worst) {
                mine[wpos * THREADS] = key;
                worst = mine[0], wpos = 0;
                for (int a = 1; a < k; ++a) {
                    const unsigned long long v = mine[a * THREADS];
                    if (v > worst) worst = v, wpos = a;
                }
            }
        }
    }
    for (int a = 1; a < cnt; ++a) {
        const unsigned long long v = mine[a * THREADS];
        int at = a;
        while (at > 0 && mine[(at - 1) * THREADS] > v) {
            mine[at * THREADS] = mine[(at - 1) * THREADS];
            --at;
        }
        mine[at * THREADS] = v;
    }
    for (int a = 0; a < cnt; ++a) {
        const int64_t j = (int64_t)(mine[a * THREADS] & kRowMask);
        double d2 = (double)INFINITY;
        if (j < M) {                                                            // always, for a ws from the same points
            const double dx = (double)points[3 * j] - px, dy = (double)points[3 * j + 1] - py, dz = (double)points[3 * j + 2] - pz;
            d2 = (dx * dx + dy * dy) + dz * dz;
        }
        index[row * k + a] = (int32_t)j;
        dist2[row * k + a] = (float)d2;
    }
    knn_empty(row, k, index, dist2, found, cnt);
    found[row] = cnt;
}

// count = found + 1 and the nine moments of a point and its k nearest others, with the quantisation of k_cl_query; a
// point without a cell gets zeros, as k_cl_insert gives it.  The point's own offset is 0 and adds nothing.
__global__ void __launch_bounds__(kThreads) k_knn_moments(const float *__restrict__ points, int64_t M, double h, double scale,
                                                           const int32_t *__restrict__ index, const int32_t *__restrict__ found,
                                                           int k, int32_t *__restrict__ count, int64_t *__restrict__ moments) {
    const int64_t i = row_of();
    if (i >= M) return;
    const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
    int bx, by, bz;
    const bool has = finite3(x, y, z) && cell_of(x, y, z, h, bx, by, bz);
    const int n = has ? min(max(found[i], 0), k) : 0;
    const double px = (double)x, py = (double)y, pz = (double)z;
    int64_t a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int e = 0; e < n; ++e) {
        const int64_t j = index[i * k + e];
        if (j < 0 || j >= M) continue;                                          // never, for an index of the same points
        const int qx = (int)rint(((double)points[3 * j] - px) * scale), qy = (int)rint(((double)points[3 * j + 1] - py) * scale),
                  qz = (int)rint(((double)points[3 * j + 2] - pz) * scale);
        a[0] += qx;
        a[1] += qy;
        a[2] += qz;
        a[3] += (int64_t)qx * qx;
        a[4] += (int64_t)qx * qy;
        a[5] += (int64_t)qx * qz;
        a[6] += (int64_t)qy * qy;
        a[7] += (int64_t)qy * qz;
        a[8] += (int64_t)qz * qz;
    }
    count[i] = has ? n + 1 : 0;
#pragma unroll
    for (int m = 0; m < 9; ++m) moments[9 * i + m] = a[m];
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// q of the statistical filter: the sum over a complete row's k neighbours of floor(sqrt(rint(d2 factor))), factor =
// 2^32 / r^2; -1 for a row that is not complete.  n, sum q and sum q^2 - the latter as the sums of its low and its high
// 32 bits, each below 2^62 - go to the header by integer atomics of per-wave sums: they commute.
__global__ void __launch_bounds__(kThreads) k_knn_mean_distance(const float *__restrict__ points, int64_t M, double factor,
                                                                 const int32_t *__restrict__ index,
                                                                 const int32_t *__restrict__ found, int k,
                                                                 int32_t *__restrict__ q, int32_t *__restrict__ hdr) {
    const int64_t i = row_of();
    int64_t sum = -1;
    if (i < M && found[i] == k) {
        const double px = (double)points[3 * i], py = (double)points[3 * i + 1], pz = (double)points[3 * i + 2];
        sum = 0;
        for (int e = 0; e < k; ++e) {
            const int64_t j = index[i * k + e];
            if (j < 0 || j >= M) continue;                                      // never, for an index of the same points
            const double dx = (double)points[3 * j] - px, dy = (double)points[3 * j + 1] - py, dz = (double)points[3 * j + 2] - pz;
            const double D = rint(((dx * dx + dy * dy) + dz * dz) * factor);
            // D <= 2^32 + 1 for d2 <= r r; anything else (a stale index) is clamped, so that the sum stays an int32
            const int64_t Di = D >= 0.0 && D <= 4294967297.0 ? (int64_t)D : 0;
            int64_t s = (int64_t)sqrt((double)Di);
            while (s * s > Di) --s;
            while ((s + 1) * (s + 1) <= Di) ++s;
            sum += s;
        }
        q[i] = (int32_t)sum;
    } else if (i < M) {
        q[i] = -1;
    }
    const bool complete = sum >= 0;
    const unsigned long long b = __ballot(complete);
    if (!b) return;
    const unsigned long long v = complete ? (unsigned long long)sum : 0ull, vv = v * v;
    const unsigned long long s1 = wave_sum(v), lo = wave_sum(vv & 0xffffffffull), hi = wave_sum(vv >> 32);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *h64 = (unsigned long long *)hdr;
        atomicAdd(hdr + kComplete, (int)__popcll(b));
        atomicAdd(h64 + kSumQ, s1);
        atomicAdd(h64 + kSumQQLo, lo);
        atomicAdd(h64 + kSumQQHi, hi);
    }
}

inline int64_t keep_tiles(int64_t M) { return M ? (M + kTile - 1) / kTile : 1; }

template <int THREADS>
void launch_knn(hipStream_t st, const float *points, int64_t M, const float *queries, int64_t Q, const ClPtr &p, const ClWs &m,
                float radius, int k, int32_t *index, float *dist2, int32_t *found) {
    const double r = (double)radius;
    const dim3 grid((unsigned)(Q ? (Q + THREADS - 1) / THREADS : 1));
    const size_t lds = sizeof(unsigned long long) * (size_t)k * THREADS;
    if (queries)
        hipLaunchKernelGGL((k_knn_query<THREADS, true>), grid, dim3(THREADS), lds, st, points, queries, Q, p.sorted, p.sslot, p.slot,
                           p.start, p.keys, m.S, M, p.hdr, cell_edge(radius), r * r, k, index, dist2, found);
    else
        hipLaunchKernelGGL((k_knn_query<THREADS, false>), grid, dim3(THREADS), lds, st, points, queries, Q, p.sorted, p.sslot, p.slot,
                           p.start, p.keys, m.S, M, p.hdr, cell_edge(radius), r * r, k, index, dist2, found);
}

// The two launches that count the rows a filter keeps, and the one that moves them.
void launch_keep_count(hipStream_t st, const int32_t *v, int64_t M, int lo, int hi, const ClPtr &p) {
    const int64_t tiles = keep_tiles(M);                                        // <= ntile: the offsets fit the tile array
    hipLaunchKernelGGL(k_cl_keep_count, dim3((unsigned)tiles), dim3(kThreads), 0, st, v, M, lo, hi, p.tile);
    launch_scan(st, p.hdr + kKept, ScanJob{p.tile, tiles});
}

struct KeepArgs {
    const float *points;
    const uint8_t *colors;
    const int64_t *index;
    const int32_t *v;
    int64_t M, M2;
    const void *ws;
    int64_t ws_bytes;
    float *points_out;
    uint8_t *colors_out;
    int64_t *index_out, *rows_out;
};

inline bool keep_args_ok(const KeepArgs &a, ClWs &m) {
    return cl_layout(a.M, m) && ws_ok(a.ws) && a.ws_bytes >= m.bytes && a.M2 >= 0 && a.M2 <= a.M &&
           ((a.points && a.v) || a.M == 0) && (a.points_out || a.M2 == 0) && (a.colors != nullptr) == (a.colors_out != nullptr) &&
           (!a.index || a.index_out) && aligned(a.points, 4) && aligned(a.v, 4) && aligned(a.points_out, 4) &&
           aligned(a.index, 8) && aligned(a.index_out, 8) && aligned(a.rows_out, 8);
}

void launch_keep_scatter(hipStream_t st, const KeepArgs &a, const ClWs &m, int lo, int hi) {
    const ClPtr p = cl_ptr(const_cast<void *>(a.ws), m);
    hipLaunchKernelGGL(k_cl_keep_scatter, dim3((unsigned)keep_tiles(a.M)), dim3(kThreads), 0, st, a.points, a.colors, a.index, a.v,
                       a.M, lo, hi, p.tile, a.M2, a.points_out, a.colors_out, a.index_out, a.rows_out);
}

}  // namespace

extern "C" {

int64_t m3_cloud_ws_bytes(int64_t M) {
    ClWs m;
    return cl_layout(M, m) ? m.bytes : 0;
}

int m3_cloud_launches(void) { return kBuildLaunches; }

int m3_cloud_neighbors(const float *points, int64_t M, float radius, double scale, int32_t *count, int64_t *moments,
                       void *ws, int64_t ws_bytes, void *stream) {
    ClWs m;
    M3_REQUIRE(cl_layout(M, m) && ws_ok(ws) && ws_bytes >= m.bytes);
    M3_REQUIRE(((points && count) || M == 0) && aligned(points, 4) && aligned(count, 4) && aligned(moments, 8));
    M3_REQUIRE(radius > 0.f && radius < INFINITY);                                                   // NaN fails
    M3_REQUIRE(scale > 0.0 && scale < (double)INFINITY && scale * (double)radius <= 2097152.0);
    hipStream_t st = (hipStream_t)stream;
    const ClPtr p = cl_ptr(ws, m);
    const dim3 block(kThreads);
    const double r = (double)radius;
    launch_index(st, points, M, radius, ws, m, count, moments);
    if (moments)
        hipLaunchKernelGGL(k_cl_query<true>, grid_of(M), block, 0, st, p.sorted, p.sslot, p.start, p.keys, m.S, M, p.hdr,
                           r * r, scale, count, moments);
    else
        hipLaunchKernelGGL(k_cl_query<false>, grid_of(M), block, 0, st, p.sorted, p.sslot, p.start, p.keys, m.S, M, p.hdr,
                           r * r, scale, count, moments);
    M3_CHECK_LAUNCH("m3_cloud_neighbors");
    return M3_OK;
}

int m3_cloud_normals(const float *points, int64_t M, const int32_t *count, const int64_t *moments, const float *toward,
                     int toward_stride, int min_points, float *normals, float *variation, void *stream) {
    M3_REQUIRE(M >= 0 && M <= kMaxM && ((points && count && moments && normals) || M == 0));
    M3_REQUIRE(aligned(points, 4) && aligned(count, 4) && aligned(moments, 8) && aligned(toward, 4) && aligned(normals, 4) &&
               aligned(variation, 4));
    M3_REQUIRE((toward_stride == 0 || toward_stride == 3) && min_points >= 1);
    hipLaunchKernelGGL(k_cl_normals, grid_of(M), dim3(kThreads), 0, (hipStream_t)stream, points, M, count, moments, toward,
                       toward_stride, min_points, normals, variation);
    M3_CHECK_LAUNCH("m3_cloud_normals");
    return M3_OK;
}

int m3_cloud_radius_count(const int32_t *count, int64_t M, int min_neighbors, void *ws, int64_t ws_bytes, void *stream) {
    ClWs m;
    M3_REQUIRE(cl_layout(M, m) && ws_ok(ws) && ws_bytes >= m.bytes);
    M3_REQUIRE((count || M == 0) && aligned(count, 4) && min_neighbors >= 0);
    launch_keep_count((hipStream_t)stream, count, M, min_neighbors, INT32_MAX, cl_ptr(ws, m));
    M3_CHECK_LAUNCH("m3_cloud_radius_count");
    return M3_OK;
}

int m3_cloud_radius_scatter(const float *points, const uint8_t *colors, const int64_t *index, const int32_t *count,
                            int64_t M, int min_neighbors, const void *ws, int64_t ws_bytes, int64_t M2, float *points_out,
                            uint8_t *colors_out, int64_t *index_out, int64_t *rows_out, void *stream) {
    ClWs m;
    const KeepArgs a{points, colors, index, count, M, M2, ws, ws_bytes, points_out, colors_out, index_out, rows_out};
    M3_REQUIRE(keep_args_ok(a, m) && min_neighbors >= 0);
    launch_keep_scatter((hipStream_t)stream, a, m, min_neighbors, INT32_MAX);
    M3_CHECK_LAUNCH("m3_cloud_radius_scatter");
    return M3_OK;
}

int m3_knn_launches(void) { return kBuildLaunches; }

int m3_knn_query(const float *points, int64_t M, float radius, const float *queries, int64_t Q, int k, int32_t *index,
                 float *dist2, int32_t *found, void *ws, int64_t ws_bytes, void *stream) {
    ClWs m;
    M3_REQUIRE(cl_layout(M, m) && ws_ok(ws) && ws_bytes >= m.bytes && radius_ok(radius) && k >= 1 && k <= kKnnMaxK);
    M3_REQUIRE(Q >= 0 && Q <= kMaxM && (queries || Q == M) && (points || M == 0) && ((index && dist2 && found) || Q == 0));
    M3_REQUIRE(aligned(points, 4) && aligned(queries, 4) && aligned(index, 4) && aligned(dist2, 4) && aligned(found, 4));
    hipStream_t st = (hipStream_t)stream;
    const ClPtr p = cl_ptr(ws, m);
    launch_index(st, points, M, radius, ws, m, nullptr, nullptr);
    if (k <= 16) launch_knn<256>(st, points, M, queries, Q, p, m, radius, k, index, dist2, found);
    else if (k <= 32) launch_knn<128>(st, points, M, queries, Q, p, m, radius, k, index, dist2, found);
    else launch_knn<64>(st, points, M, queries, Q, p, m, radius, k, index, dist2, found);
    M3_CHECK_LAUNCH("m3_knn_query");
    return M3_OK;
}

int m3_knn_moments(const float *points, int64_t M, float radius, double scale, const int32_t *index, const int32_t *found,
                   int k, int32_t *count, int64_t *moments, void *stream) {
    M3_REQUIRE(M >= 0 && M <= kMaxM && ((points && index && found && count && moments) || M == 0) && k >= 1 && k <= kKnnMaxK);
    M3_REQUIRE(aligned(points, 4) && aligned(index, 4) && aligned(found, 4) && aligned(count, 4) && aligned(moments, 8));
    M3_REQUIRE(radius_ok(radius) && scale > 0.0 && scale < (double)INFINITY && scale * (double)radius <= 2097152.0);
    hipLaunchKernelGGL(k_knn_moments, grid_of(M), dim3(kThreads), 0, (hipStream_t)stream, points, M, cell_edge(radius), scale,
                       index, found, k, count, moments);
    M3_CHECK_LAUNCH("m3_knn_moments");
    return M3_OK;
}

int m3_knn_mean_distance(const float *points, int64_t M, double factor, const int32_t *index, const int32_t *found, int k,
                         int32_t *q, void *ws, int64_t ws_bytes, void *stream) {
    ClWs m;
    M3_REQUIRE(cl_layout(M, m) && ws_ok(ws) && ws_bytes >= m.bytes && k >= 1 && k <= kKnnMaxK);
    M3_REQUIRE(((points && index && found && q) || M == 0) && factor > 0.0 && factor < (double)INFINITY);
    M3_REQUIRE(aligned(points, 4) && aligned(index, 4) && aligned(found, 4) && aligned(q, 4));
    hipLaunchKernelGGL(k_knn_mean_distance, grid_of(M), dim3(kThreads), 0, (hipStream_t)stream, points, M, factor, index, found,
                       k, q, cl_ptr(ws, m).hdr);
    M3_CHECK_LAUNCH("m3_knn_mean_distance");
    return M3_OK;
}

int m3_knn_stat_count(const int32_t *q, int64_t M, int threshold, void *ws, int64_t ws_bytes, void *stream) {
    ClWs m;
    M3_REQUIRE(cl_layout(M, m) && ws_ok(ws) && ws_bytes >= m.bytes);
    M3_REQUIRE((q || M == 0) && aligned(q, 4) && threshold >= 0);
    launch_keep_count((hipStream_t)stream, q, M, -1, threshold, cl_ptr(ws, m));
    M3_CHECK_LAUNCH("m3_knn_stat_count");
    return M3_OK;
}

int m3_knn_stat_scatter(const float *points, const uint8_t *colors, const int64_t *index, const int32_t *q, int64_t M,
                        int threshold, const void *ws, int64_t ws_bytes, int64_t M2, float *points_out, uint8_t *colors_out,
                        int64_t *index_out, int64_t *rows_out, void *stream) {
    ClWs m;
    const KeepArgs a{points, colors, index, q, M, M2, ws, ws_bytes, points_out, colors_out, index_out, rows_out};
    M3_REQUIRE(keep_args_ok(a, m) && threshold >= 0);
    launch_keep_scatter((hipStream_t)stream, a, m, -1, threshold);
    M3_CHECK_LAUNCH("m3_knn_stat_scatter");
    return M3_OK;
}

}  // extern "C"

