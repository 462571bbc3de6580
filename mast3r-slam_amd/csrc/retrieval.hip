// Keyframe retrieval database ("simple retrieval" of mast3r_utils.py:696-715, :717-795): global signatures of encoder
// tokens and the top-k similarity query against the stored signatures.  Both are stream-ordered, allocate nothing and
// never synchronise; every sum has a fixed order, so a row's bits depend on its own inputs only.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSigRows = 32;          // token rows per signature slice: T = 1024 -> 32 workgroups per 1024-column frame
constexpr int kSigVecs = 256;         // 8-column vectors per signature workgroup (2048 columns)
constexpr int kTopkMaxRows = 512;     // database rows per top-k workgroup (upper bound; 8 candidates per lane)
constexpr int kTopkLanes = 16;        // lanes per database row in the score loop (4 rows per wave)
constexpr int kTopkMaxQ = 8;          // queries per top-k workgroup
constexpr int kTopkQBytes = 32768;    // LDS for the query tile
constexpr int kMaxK = 64;

// ---- signature ---------------------------------------------------------------------------------------------------
// 8 consecutive values of a row as fp32; p is 16-byte aligned (8 x 16-bit = one dwordx4, 8 x fp32 = two).
template <int DT>
__device__ __forceinline__ void load8(const void *p, float (&x)[8]) {
    if constexpr (DT == M3_RETRIEVAL_F32) {
        const float4 a = ((const float4 *)p)[0], b = ((const float4 *)p)[1];
        x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
    } else {
        const uint4 v = *(const uint4 *)p;
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (DT == M3_RETRIEVAL_BF16) {
                x[2 * j] = __uint_as_float(w[j] << 16);
                x[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
            } else {
                typedef _Float16 h2 __attribute__((ext_vector_type(2)));
                const h2 h = __builtin_bit_cast(h2, w[j]);
                x[2 * j] = (float)h[0];
                x[2 * j + 1] = (float)h[1];
            }
        }
    }
}

// Column sums of one slice of kSigRows token rows.  Grid (slices, column chunks, B).  Thread (r, v) adds rows
// t0 + r, t0 + r + R, ... of 8-column vector v in row order; the R row phases are then added in phase order.  R and
// the lane map depend on C only, so the partial of (b, slice) has the same bits for every B.
template <int DT>
__global__ void __launch_bounds__(kThreads) k_sig_partial(const void *__restrict__ feat, float *__restrict__ part, int T,
                                                           int C) {
    __shared__ float red[kThreads][9];                 // 9: odd stride, the phase sums read distinct banks
    const int b = blockIdx.z, slice = blockIdx.x, S = gridDim.x;
    const int cv = C / 8, v0 = blockIdx.y * kSigVecs;
    const int W = min(cv - v0, kSigVecs), R = kThreads / W;
    const int r = threadIdx.x / W, v = threadIdx.x - r * W;
    const int t0 = slice * kSigRows, t1 = min(t0 + kSigRows, T);
    const size_t esz = DT == M3_RETRIEVAL_F32 ? 4 : 2;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (r < R) {
        const char *base = (const char *)feat + ((size_t)b * T * C + (size_t)(v0 + v) * 8) * esz;
        int t = t0 + r;
        for (; t + 3 * R < t1; t += 4 * R) {           // four loads in flight, added in row order
            float x0[8], x1[8], x2[8], x3[8];
            load8<DT>(base + (size_t)t * C * esz, x0);
            load8<DT>(base + (size_t)(t + R) * C * esz, x1);
            load8<DT>(base + (size_t)(t + 2 * R) * C * esz, x2);
            load8<DT>(base + (size_t)(t + 3 * R) * C * esz, x3);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = (((acc[j] + x0[j]) + x1[j]) + x2[j]) + x3[j];
        }
        for (; t < t1; t += R) {
            float x[8];
            load8<DT>(base + (size_t)t * C * esz, x);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += x[j];
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) red[threadIdx.x][j] = acc[j];
    __syncthreads();
    float *out = part + ((size_t)b * S + slice) * C + (size_t)v0 * 8;
    for (int i = threadIdx.x; i < W * 8; i += kThreads) {
        const int vv = i >> 3, j = i & 7;
        float s = 0.f;
        for (int rr = 0; rr < R; ++rr) s += red[rr * W + vv][j];
        out[i] = s;
    }
}

// One workgroup per batch item: m = (sum of the slice partials in slice order) / T, then m / sqrt(sum m^2 + 1e-8).
__global__ void __launch_bounds__(kThreads) k_sig_finish(const float *__restrict__ part, float *__restrict__ sig,
                                                          int64_t sig_stride, int S, int T, int C) {
    __shared__ float wsum[kThreads / M3_WAVE];
    const int b = blockIdx.x;
    const float *p = part + (size_t)b * S * C;
    float *o = sig + (size_t)b * sig_stride;
    float ss = 0.f;
    for (int c = threadIdx.x; c < C; c += kThreads) {
        float s = 0.f;
        int sl = 0;
        for (; sl + 8 <= S; sl += 8) {                 // eight loads in flight, added in slice order
            float x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = p[(size_t)(sl + j) * C + c];
#pragma unroll
            for (int j = 0; j < 8; ++j) s += x[j];
        }
        for (; sl < S; ++sl) s += p[(size_t)sl * C + c];
        const float m = s / (float)T;
        o[c] = m;
        ss = fmaf(m, m, ss);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = ss;
    __syncthreads();
    const float tot = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    const float nrm = sqrtf(tot + 1e-8f);
    for (int c = threadIdx.x; c < C; c += kThreads) o[c] = o[c] / nrm;
}

// ---- top-k -------------------------------------------------------------------------------------------------------
// Candidate order: higher score first, equal scores to the larger database index (reverse of a stable ascending
// argsort); idx < 0 marks "no candidate" and loses to every real one.
__device__ __forceinline__ bool better(float s1, int i1, float s2, int i2) {
    return i1 >= 0 && (i2 < 0 || s1 > s2 || (s1 == s2 && i1 > i2));
}

__device__ __forceinline__ void wave_best(float &s, int &i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float so = __shfl_xor(s, off, 64);
        const int io = __shfl_xor(i, off, 64);
        if (better(so, io, s, i)) { s = so; i = io; }
    }
}

struct TopkGeom {
    int nmax, rows, nblk;
};

// Rows per workgroup: about 512 workgroups over the database (a 4096-row database still spreads over the chip), at least
// one pass of the 16 row groups, at most kTopkMaxRows (8 candidates per lane in the selection).
inline TopkGeom topk_geom(int N, int Q, int causal) {
    TopkGeom g;
    g.nmax = N + (causal ? Q - 1 : 0);
    int rows = (g.nmax + 511) / 512;
    rows = (rows + 15) / 16 * 16;
    g.rows = rows < 16 ? 16 : rows > kTopkMaxRows ? kTopkMaxRows : rows;
    g.nblk = g.nmax > 0 ? (g.nmax + g.rows - 1) / g.rows : 1;
    return g;
}

// Grid (row blocks, query tiles).  Scores: 16 lanes per database row, lane l takes the float4 chunks l, l + 16, ... in
// order (one fma chain), then a fixed xor tree over the 16 lanes: the bits of score(q, n) depend on C only.  Every
// wave then selects the block's k best of one query by k wave-wide arg-max rounds.
__global__ void __launch_bounds__(kThreads) k_topk_partial(const float *__restrict__ qsig, int64_t ldq,
                                                            const float *__restrict__ db, int64_t ldd, int N, int Q, int C,
                                                            int k, int causal, int rows, int qt, int2 *__restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *qs = (float *)smem;                         // [qt][C]
    float *sc = qs + (size_t)qt * C;                   // [qt][rows]
    const int q0 = blockIdx.y * qt, nq = min(qt, Q - q0);
    const int nblk = gridDim.x, blk = blockIdx.x;
    const int r0 = blk * rows;
    const int nmax = N + (causal ? Q - 1 : 0);
    const int rend = min(r0 + rows, nmax);
    const int c4 = C / 4;
    for (int i = threadIdx.x; i < nq * c4; i += kThreads) {
        const int qi = i / c4, j = i - qi * c4;
        ((float4 *)qs)[(size_t)qi * c4 + j] = ((const float4 *)(qsig + (size_t)(q0 + qi) * ldq))[j];
    }
    __syncthreads();
    const int g = threadIdx.x / kTopkLanes, l = threadIdx.x % kTopkLanes;
    for (int n = r0 + g; n < rend; n += kThreads / kTopkLanes) {
        const float4 *row = (const float4 *)(db + (size_t)n * ldd);
        float acc[kTopkMaxQ];
#pragma unroll
        for (int qi = 0; qi < kTopkMaxQ; ++qi) acc[qi] = 0.f;
        for (int j = l; j < c4; j += kTopkLanes) {
            const float4 d = row[j];
#pragma unroll
            for (int qi = 0; qi < kTopkMaxQ; ++qi) {
                if (qi < nq) {
                    const float4 q = ((const float4 *)qs)[(size_t)qi * c4 + j];
                    acc[qi] = fmaf(d.w, q.w, fmaf(d.z, q.z, fmaf(d.y, q.y, fmaf(d.x, q.x, acc[qi]))));
                }
            }
        }
#pragma unroll
        for (int qi = 0; qi < kTopkMaxQ; ++qi) {
#pragma unroll
            for (int off = kTopkLanes / 2; off > 0; off >>= 1) acc[qi] += __shfl_xor(acc[qi], off, kTopkLanes);
            if (qi < nq && l == 0) sc[(size_t)qi * rows + (n - r0)] = acc[qi];
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int qi = threadIdx.x >> 6; qi < nq; qi += kThreads / M3_WAVE) {
        const int q = q0 + qi;
        const int lim = min(rend, causal ? N + q : N);              // rows [r0, lim) exist for this query
        float s[kTopkMaxRows / M3_WAVE];
        int id[kTopkMaxRows / M3_WAVE];
#pragma unroll
        for (int m = 0; m < kTopkMaxRows / M3_WAVE; ++m) {
            const int n = r0 + lane + m * M3_WAVE;
            const bool ok = n < lim;
            s[m] = ok ? sc[(size_t)qi * rows + (n - r0)] : 0.f;
            id[m] = ok ? n : -1;
        }
        int2 *out = ws + ((size_t)q * nblk + blk) * k;
        for (int j = 0; j < k; ++j) {
            float bs = 0.f;
            int bi = -1;
#pragma unroll
            for (int m = 0; m < kTopkMaxRows / M3_WAVE; ++m)
                if (better(s[m], id[m], bs, bi)) { bs = s[m]; bi = id[m]; }
            wave_best(bs, bi);
#pragma unroll
            for (int m = 0; m < kTopkMaxRows / M3_WAVE; ++m)
                if (id[m] == bi) id[m] = -1;                          // taken (bi < 0 matches nothing valid)
            if (lane == 0) out[j] = make_int2(__float_as_int(bs), bi);
        }
    }
}

// One workgroup per query: k block-wide arg-max rounds over the nblk * k block candidates, then the threshold.
__global__ void __launch_bounds__(kThreads) k_topk_merge(int2 *__restrict__ ws, int nblk, int k, int use_thresh,
                                                          float min_thresh, int32_t *__restrict__ count,
                                                          int32_t *__restrict__ idx, float *__restrict__ score) {
    __shared__ float bsw[2][kThreads / M3_WAVE];
    __shared__ int biw[2][kThreads / M3_WAVE];
    const int q = blockIdx.x, M = nblk * k;
    int2 *cand = ws + (size_t)q * M;
    int kept = 0;
    bool open = true;
    for (int j = 0; j < k; ++j) {
        float bs = 0.f;
        int bi = -1, bp = -1;
        if (open) {
            for (int p = threadIdx.x; p < M; p += kThreads) {
                const int2 c = cand[p];
                const float cs = __int_as_float(c.x);
                if (better(cs, c.y, bs, bi)) { bs = cs; bi = c.y; bp = p; }
            }
        }
        const int mine = bi;
        wave_best(bs, bi);
        const int w = threadIdx.x >> 6, par = j & 1;
        if ((threadIdx.x & 63) == 0) { bsw[par][w] = bs; biw[par][w] = bi; }
        __syncthreads();
        bs = bsw[par][0];
        bi = biw[par][0];
#pragma unroll
        for (int ww = 1; ww < kThreads / M3_WAVE; ++ww)
            if (better(bsw[par][ww], biw[par][ww], bs, bi)) { bs = bsw[par][ww]; bi = biw[par][ww]; }
        if (open && bi >= 0 && mine == bi) cand[bp] = make_int2(0, -1);   // only its owner reads it
        open = open && bi >= 0 && (!use_thresh || bs > min_thresh);
        if (threadIdx.x == 0) {
            idx[(size_t)q * k + j] = open ? bi : -1;
            score[(size_t)q * k + j] = open ? bs : 0.f;
        }
        kept += open ? 1 : 0;
    }
    if (threadIdx.x == 0) count[q] = kept;
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int64_t m3_retrieval_signature_ws_bytes(int B, int T, int C) {
    if (B < 1 || T < 1 || C < 8 || C % 8) return 0;
    return (int64_t)B * m3_cdiv(T, kSigRows) * C * 4;
}

int m3_retrieval_signature(const void *feat, float *sig, int64_t sig_stride, float *ws, int64_t ws_bytes, int B, int T,
                           int C, int dtype, void *stream) {
    M3_REQUIRE(feat && sig && ws && B >= 1 && T >= 1 && C >= 8 && C % 8 == 0 && sig_stride >= C);
    M3_REQUIRE(dtype == M3_RETRIEVAL_BF16 || dtype == M3_RETRIEVAL_F16 || dtype == M3_RETRIEVAL_F32);
    M3_REQUIRE(aligned16(feat) && ws_bytes >= m3_retrieval_signature_ws_bytes(B, T, C));
    M3_REQUIRE(B <= 65535 && (int64_t)B * T * C < ((int64_t)1 << 40));
    hipStream_t st = (hipStream_t)stream;
    const int S = m3_cdiv(T, kSigRows);
    const dim3 grid(S, m3_cdiv(C / 8, kSigVecs), B);
    if (dtype == M3_RETRIEVAL_BF16)
        hipLaunchKernelGGL(k_sig_partial<M3_RETRIEVAL_BF16>, grid, dim3(kThreads), 0, st, feat, ws, T, C);
    else if (dtype == M3_RETRIEVAL_F16)
        hipLaunchKernelGGL(k_sig_partial<M3_RETRIEVAL_F16>, grid, dim3(kThreads), 0, st, feat, ws, T, C);
    else
        hipLaunchKernelGGL(k_sig_partial<M3_RETRIEVAL_F32>, grid, dim3(kThreads), 0, st, feat, ws, T, C);
    hipLaunchKernelGGL(k_sig_finish, dim3(B), dim3(kThreads), 0, st, (const float *)ws, sig, sig_stride, S, T, C);
    M3_CHECK_LAUNCH("m3_retrieval_signature");
    return M3_OK;
}

int64_t m3_retrieval_ws_bytes(int N, int Q, int k, int causal) {
    if (N < 0 || Q < 1 || k < 1 || k > kMaxK || (causal != 0 && causal != 1)) return 0;
    const TopkGeom g = topk_geom(N, Q, causal);
    return (int64_t)Q * g.nblk * k * 8;
}

int m3_retrieval_topk(const float *qsig, int64_t ldq, const float *db, int64_t ldd, int N, int Q, int C, int k,
                      int use_thresh, float min_thresh, int causal, int32_t *count, int32_t *idx, float *score, void *ws,
                      int64_t ws_bytes, void *stream) {
    M3_REQUIRE(qsig && db && count && idx && score && ws);
    M3_REQUIRE(N >= 0 && Q >= 1 && C >= 8 && C % 8 == 0 && k >= 1 && k <= kMaxK && ldq >= C && ldd >= C);
    M3_REQUIRE(ldq % 4 == 0 && ldd % 4 == 0 && aligned16(qsig) && aligned16(db) && aligned16(ws));
    M3_REQUIRE((use_thresh == 0 || use_thresh == 1) && (causal == 0 || causal == 1));
    M3_REQUIRE(Q <= 65535 * kTopkMaxQ && (int64_t)N + Q < ((int64_t)1 << 30));
    M3_REQUIRE(ws_bytes >= m3_retrieval_ws_bytes(N, Q, k, causal));
    if (4 * C > kTopkQBytes) return M3_ERR_UNSUPPORTED;               // one query row must fit the LDS tile (C <= 8192)
    const TopkGeom g = topk_geom(N, Q, causal);
    const int qt = kTopkQBytes / (4 * C) < kTopkMaxQ ? kTopkQBytes / (4 * C) : kTopkMaxQ;
    if (m3_cdiv(Q, qt) > 65535) return M3_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = ((size_t)qt * C + (size_t)qt * g.rows) * 4;
    hipLaunchKernelGGL(k_topk_partial, dim3(g.nblk, m3_cdiv(Q, qt)), dim3(kThreads), lds, st, qsig, ldq, db, ldd, N, Q,
                       C, k, causal, g.rows, qt, (int2 *)ws);
    hipLaunchKernelGGL(k_topk_merge, dim3(Q), dim3(kThreads), 0, st, (int2 *)ws, g.nblk, k, use_thresh, min_thresh,
                       count, idx, score);
    M3_CHECK_LAUNCH("m3_retrieval_topk");
    return M3_OK;
}

}  // extern "C"
