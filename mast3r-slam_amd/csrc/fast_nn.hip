// Nearest neighbour in descriptor space (maximum dot product) - the search primitive of "fast reciprocal NN" matching
// (MASt3R, Leroy et al. 2024, section 3.3; mast3r/fast_nn.py of the public implementation).  Three forms, same result:
// an fp32 FMA-chain kernel (k_nn_search), the brute-force search on the matrix cores (k_nn_mfma) and an
// exact search that bounds most of the database away first (k_frnn_blockstats / _seed_lb / _survivors / _eval, further
// down) with k_nn_mfma as its device-side fallback.  BASELINE.json's north_star names this matcher; the reference tree has no implementation
// of it, so the semantics below are this repo's and are pinned by its own oracle:
//
//   score(s, n) = E + O,  E = fma chain over even k (ascending), O = fma chain over odd k (ascending), fp32
//   idx[s] = argmax_n score(s, n), ties -> the LOWEST n; score_out[s] = that maximum.
// (two interleaved chains = one v_pk_fma_f32 per pair of dimensions: twice the plain-FMA rate)
//
// Work layout: a lane owns one query (its D floats live in registers); database entries are wave-uniform,
// so they are fetched with scalar loads and feed the FMAs as SGPR operands - no LDS, no cross-lane
// reduction.  The database is split over blockIdx.y (so that a 4096-query search still fills the chip); the
// per-split winners are merged with ONE 64-bit atomicMax per query on a key = (order-preserving score bits,
// inverted index), which also implements the lowest-index tie-break deterministically.
//
// Device side, each written once: the key codec (make_key / key_index / key_score), Queries (which packed row is query q
// of pair b), score_tile (the MFMA sequence that defines a score), merge_lane_groups, block_origin / pixel_or_origin.
// Host side (below the kernels): PackedMap / BlockStats / PruneWs define each buffer layout once - pointers and size -,
// plan_search the database split, launch_nn_mfma / launch_pack the two template dispatches, and frnn_round is the one
// round body behind m3_frnn_round, m3_frnn_round_active and m3_frnn_round_pruned.
#include "common.h"
#include "../../include/m3slam.h"

namespace {

constexpr int kThreads = 256;

// ---- the 64-bit merge key: (order-preserving score bits) << 32 | (0xffffffff - n) ----
// atomicMax on it keeps the larger score and, among equal scores, the lower index.  Key 0 means "nothing found": every
// real key is larger (the score bits of -inf are 0x007fffff), and it decodes to index -1, which a reader clamps or ignores.
__device__ __forceinline__ unsigned ordered_bits(float f) {      // monotone float -> uint map
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_ordered(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ unsigned long long make_key(float score, int n) {
    return ((unsigned long long)ordered_bits(score) << 32) | (unsigned long long)(0xffffffffu - (unsigned)n);
}
__device__ __forceinline__ int32_t key_index(unsigned long long key) { return (int32_t)(0xffffffffu - (unsigned)(key & 0xffffffffull)); }
__device__ __forceinline__ float key_score(unsigned long long key) { return from_ordered((unsigned)(key >> 32)); }

constexpr int kQPL = 2;                                       // queries per lane: halves the scalar row traffic per FMA

template <int D>
__global__ void __launch_bounds__(kThreads)
k_nn_search(const float *__restrict__ Q, const float *__restrict__ DB, unsigned long long *__restrict__ keys,
            int S, int N, int per_split) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const int b = blockIdx.z;
    f32x2 q[kQPL][D / 2];
    int sidx[kQPL];
#pragma unroll
    for (int u = 0; u < kQPL; ++u) {
        sidx[u] = (blockIdx.x * kQPL + u) * kThreads + threadIdx.x;
        const int sq = sidx[u] < S ? sidx[u] : S - 1;        // idle lanes shadow the last query (no divergence)
        const float *qp = Q + ((size_t)b * S + sq) * D;
#pragma unroll
        for (int k = 0; k < D; k += 4) {
            const float4 v = *reinterpret_cast<const float4 *>(qp + k);
            q[u][k / 2] = f32x2{v.x, v.y}; q[u][k / 2 + 1] = f32x2{v.z, v.w};
        }
    }
    const int n0 = blockIdx.y * per_split;
    const int n1 = n0 + per_split < N ? n0 + per_split : N;
    const float *db = DB + (size_t)b * N * D;
    float best[kQPL];
    int best_n[kQPL];
#pragma unroll
    for (int u = 0; u < kQPL; ++u) { best[u] = -INFINITY; best_n[u] = n0; }
#pragma unroll 2
    for (int n = n0; n < n1; ++n) {                          // n is wave-uniform: the row loads are scalar loads
        const f32x2 *r = reinterpret_cast<const f32x2 *>(db + (size_t)n * D);
#pragma unroll
        for (int u = 0; u < kQPL; ++u) {
            f32x2 acc2 = {0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < D / 2; ++k) acc2 = __builtin_elementwise_fma(q[u][k], r[k], acc2);
            const float acc = acc2.x + acc2.y;
            if (acc > best[u]) { best[u] = acc; best_n[u] = n; }   // strict: the first (lowest) n wins inside a split
        }
    }
    if (n0 < n1) {
#pragma unroll
        for (int u = 0; u < kQPL; ++u) {
            if (sidx[u] >= S) continue;
            atomicMax(keys + (size_t)b * S + sidx[u], make_key(best[u], best_n[u]));
        }
    }
}

__global__ void __launch_bounds__(kThreads)
k_nn_unpack(const unsigned long long *__restrict__ keys, int32_t *__restrict__ idx, float *__restrict__ score,
            long long total) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    idx[i] = key_index(keys[i]);
    if (score) score[i] = key_score(keys[i]);
}

// ------------------------------------------------------------------------------------------------------------
// The same search on the matrix cores.  scores = Q . DB^T is a [S x D] x [D x N] GEMM with a tiny K (D <= 32 = ONE
// v_mfma_f32_16x16x32_f16 k-step) and an arg-max epilogue; the fp32 kernel above runs at the plain-FMA rate
// (66-72 TFLOP/s).  Operands are packed once per call to [rows][32] fp16 (K zero-padded):
//   fp16 descriptors (BASELINE configs[4] "fp16 features")  -> 1 MFMA per 16 x 16 scores, exact products, fp32 sums
//   fp32 descriptors -> hi = fp16(x), lo = fp16(x - hi); score = hi.hi + hi.lo + lo.hi (3 MFMAs), dropped lo.lo term
//                       <= 2^-24 for unit vectors: the result is as close to the float64 oracle as the fp32 FMA chain
// Workgroup = 4 waves x 128 queries (8 query tiles in registers per wave); 128 database rows per step are staged once
// in LDS (LDS-DMA, double-buffered, swizzled so the ds_read_b128 fragment reads are conflict-free) and shared by the
// four waves.  Arg-max: two v_max3 per tile find whether ANY lane improved; only then (O(log N) times per query) the
// exact sequential update runs - rows ascend, strict '>': the lowest index wins ties as in the fp32 kernel.
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

template <bool F16IN, int D>
__global__ void __launch_bounds__(kThreads)
k_nn_pack(const void *__restrict__ X, unsigned short *__restrict__ hi, unsigned short *__restrict__ lo, long long rows) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;      // one thread per (row, 8-element chunk)
    if (i >= rows * 4) return;
    const long long r = i >> 2;
    const int c = (int)(i & 3) * 8;
    union { unsigned short h[8]; uint4 q; } H, L;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float x = 0.f;
        if (c + k < D) x = F16IN ? (float)reinterpret_cast<const _Float16 *>(X)[r * D + c + k] : reinterpret_cast<const float *>(X)[r * D + c + k];
        const _Float16 h = (_Float16)x;
        H.h[k] = __builtin_bit_cast(unsigned short, h);
        const _Float16 l = (_Float16)(x - (float)h);
        L.h[k] = __builtin_bit_cast(unsigned short, l);
    }
    reinterpret_cast<uint4 *>(hi)[i] = H.q;
    if (lo) reinterpret_cast<uint4 *>(lo)[i] = L.q;
}

// ---- exact search with block bounds: shared definitions (kernels further down) ----
constexpr float kSlack = 1.52587890625e-05f;   // 2^-16: covers the fp32 rounding of the bound and of the scores it is compared with
// more than a quarter of all (query tile, block) pairs survived: the brute-force kernel is the faster one
__device__ __forceinline__ bool prune_overflow(int total, int S, int NB) {
    return (long long)total * 4 > (long long)((S + 15) / 16) * NB;
}

constexpr int kQT = 8;                      // query tiles (16 queries each) per wave
constexpr int kQPW = kQT * 16;              // queries per wave
constexpr int kQPB = kQPW * (kThreads / 64);   // queries per workgroup: 512
constexpr int kRows = 128;                  // database rows per LDS step (two workgroup barriers per step; 64 rows: 1564 us per round, 128: 1509)

// Which packed row is query q of pair b.  A search has S_all seed slots per pair; keys, mlb and qnorm are indexed by the
// slot.  qidx [P][S_all] (null: row = slot, NQ = S_all) names the packed row a slot currently sits on, so a descriptor map
// is packed once per matcher call and serves as database of one search direction and query source of the other.  Active-set
// form (rounds >= 2 of the reciprocal matcher): only the first qcount[b] entries of qlist[b] are queries - the slots that
// have not converged yet, in the caller's order.  Built on the host (frnn_search / m3_nn_search_mfma), passed by value.
struct Queries {
    const unsigned short *hi, *lo;          // packed rows [P][NQ][32]; lo only for fp32 descriptors
    const int32_t *qidx, *qlist, *qcount;
    int S_all, NQ;
    __device__ __forceinline__ int count(int b) const { return qcount ? qcount[b] : S_all; }
    // position q in the list of pair b (S = count(b)) -> seed slot; positions past the end shadow the last query
    __device__ __forceinline__ int slot(int b, int q, int S) const {
        q = q < S ? q : S - 1;
        return qlist ? qlist[(size_t)b * S_all + q] : q;
    }
    __device__ __forceinline__ size_t row(int b, int slot) const {           // seed slot -> packed row, pair offset included
        int qr = qidx ? qidx[(size_t)b * S_all + slot] : slot;
        qr = qr < 0 ? 0 : (qr >= NQ ? NQ - 1 : qr);
        return (size_t)b * NQ + qr;
    }
    // MFMA fragment of a packed row: k = 8 g .. 8 g + 7
    __device__ __forceinline__ f16x8 frag(const unsigned short *plane, size_t row, int g) const {
        return *reinterpret_cast<const f16x8 *>(plane + row * 32 + g * 8);
    }
};

// THE score of 16 database rows (A operand) x 16 queries (B operand): hi.hi, then hi.lo, then lo.hi into one accumulator
// (LO: fp32 descriptors), hi.hi alone otherwise.  The brute-force search (nn_step) and the block-bound search (k_frnn_eval)
// both score through it, so their scores are the same bits by construction.
template <bool LO>
__device__ __forceinline__ f32x4 score_tile(f16x8 a_hi, f16x8 a_lo, f16x8 q_hi, f16x8 q_lo) {
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, q_hi, c, 0, 0, 0);
    if (LO) {
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, q_lo, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_lo, q_hi, c, 0, 0, 0);
    }
    return c;
}

// the 4 lane groups of a wave hold disjoint row subsets of the same query: keep the larger score, ties -> lower index
__device__ __forceinline__ void merge_lane_groups(float &best, int &n) {
#pragma unroll
    for (int sh = 16; sh <= 32; sh <<= 1) {
        const float os = __shfl_xor(best, sh, 64);
        const int on = __shfl_xor(n, sh, 64);
        if (os > best || (os == best && on < n)) { best = os; n = on; }
    }
}

// One LDS step of the brute-force search.  The file is built with -amdgpu-mfma-vgpr-form (results land in VGPRs; through
// AGPRs every MFMA waited out the matrix core's latency behind 4 v_accvgpr_read); the 2 x 4 score_tiles of two row tiles x
// four query tiles are issued back to back into eight accumulators and only then reduced (max over a lane's 8 scores of a
// query: 3 x v_max3 + v_max, one compare + wave vote per PAIR of tiles); the ragged tail is a separate instantiation
// (RAGGED) taken for the last step of a split only.  One MFMA at a time ran at 358 TFLOP/s = 0.14 of the peak.
template <bool LO, bool RAGGED>
__device__ __forceinline__ void nn_step(const unsigned char *__restrict__ hi_s, const unsigned char *__restrict__ lo_s,
                                        const f16x8 (&qh)[kQT], const f16x8 (&ql)[LO ? kQT : 1],
                                        float (&best)[kQT], int (&bestn)[kQT], int nbase, int n1, int col, int g) {
#pragma unroll
    for (int rp = 0; rp < kRows / 32; ++rp) {                                 // pairs of 16-row tiles
        f16x8 ah[2], al[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = (2 * rp + h) * 16 + col;                          // A operand: lane -> row (lane & 15), k chunk g
            const int off = row * 64 + ((g ^ ((0 - (row >> 2)) & 3)) << 4);
            ah[h] = *reinterpret_cast<const f16x8 *>(hi_s + off);
            al[h] = ah[h];
            if (LO) al[h] = *reinterpret_cast<const f16x8 *>(lo_s + off);
        }
        const int nrow = nbase + rp * 32 + g * 4;                             // first of this lane's 2 x 4 output rows
#pragma unroll
        for (int t0 = 0; t0 < kQT; t0 += 4) {
            f32x4 acc[4][2];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int h = 0; h < 2; ++h) acc[tt][h] = score_tile<LO>(ah[h], al[h], qh[t0 + tt], ql[LO ? t0 + tt : 0]);
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                const int t = t0 + tt;
                f32x4 &a0 = acc[tt][0], &a1 = acc[tt][1];
                if (RAGGED) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (nrow + j >= n1) a0[j] = -INFINITY;
                        if (nrow + 16 + j >= n1) a1[j] = -INFINITY;
                    }
                }
                float mx = __builtin_fmaxf(__builtin_fmaxf(a0[0], a0[1]), a0[2]);
                mx = __builtin_fmaxf(__builtin_fmaxf(mx, a0[3]), a1[0]);
                mx = __builtin_fmaxf(__builtin_fmaxf(mx, a1[1]), a1[2]);
                mx = __builtin_fmaxf(mx, a1[3]);
                // the running maximum is updated on the straight-line path (one v_max); only the INDEX lives in the rare
                // branch - with both updated there, every loop-carried best[] register became a phi and was copied
                // around the branch on every tile (PMC: 8.4 VALU instructions per MFMA, most of them v_mov)
                const bool imp = mx > best[t];
                best[t] = __builtin_fmaxf(best[t], mx);
                if (__any(imp)) {                                             // rare after the first few steps
                    int bn = bestn[t];
#pragma unroll
                    for (int j = 3; j >= 0; --j) bn = (imp && a1[j] == best[t]) ? nrow + 16 + j : bn;   // descending: the lowest row
#pragma unroll
                    for (int j = 3; j >= 0; --j) bn = (imp && a0[j] == best[t]) ? nrow + j : bn;        // that holds the maximum wins
                    bestn[t] = bn;
                }
            }
        }
    }
}

template <bool LO>
__global__ void __launch_bounds__(kThreads, LO ? 2 : 4)                 // fp16 descriptors: 4 waves per SIMD (<= 128 registers)
k_nn_mfma(const Queries Q, const unsigned short *__restrict__ Dhi, const unsigned short *__restrict__ Dlo,
          unsigned long long *__restrict__ keys, int N, int per_split, const int32_t *__restrict__ gate_total, int gate_nb) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2][2][kRows * 64];   // [stage][hi|lo][64 rows x 64 B]
    const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = Q.count(b);
    // fallback of the block-bound search (k_frnn_eval below): runs only when the bounds pruned too little
    if (gate_total && !prune_overflow(gate_total[b], S, gate_nb)) return;
    const int col = lane & 15, g = lane >> 4;
    const size_t db = (size_t)b * N, kb = (size_t)b * Q.S_all;
    int bx = blockIdx.x, by = blockIdx.y;
    if (Q.qcount) {
        // Active-set form.  The grid was sized for S_all queries (gridDim.x query blocks x gridDim.y database splits = one
        // round of the chip).  With only nb = ceil(S / 512) query blocks left, the same workgroups are re-dealt as nb query
        // blocks x (slots / nb) database splits: every CU still works, each on a shorter database range - the round's time
        // shrinks with the active set instead of staying one full-length workgroup long.  (The per-split winners merge by
        // atomicMax whatever the number of splits; a workgroup past the end leaves in front of every barrier.)
        if (S <= 0) return;
        const int nb = (S + kQPB - 1) / kQPB, slots = (int)(gridDim.x * gridDim.y);
        const int w = by * (int)gridDim.x + bx, nsplit = slots / nb;
        bx = w % nb; by = w / nb;
        if (by >= nsplit) return;
        per_split = (((N + nsplit - 1) / nsplit) + kRows - 1) / kRows * kRows;
    }
    // query fragments (MFMA B operand): lane -> query col, k = 8 g .. 8 g + 7
    f16x8 qh[kQT], ql[LO ? kQT : 1];
    const int q0 = bx * kQPB + wave * kQPW;
#pragma unroll
    for (int t = 0; t < kQT; ++t) {
        const size_t qr = Q.row(b, Q.slot(b, q0 + t * 16 + col, S));
        qh[t] = Q.frag(Q.hi, qr, g);
        if (LO) ql[t] = Q.frag(Q.lo, qr, g);
    }
    const int n0 = by * per_split, n1 = min(n0 + per_split, N);
    float best[kQT];
    int bestn[kQT];
#pragma unroll
    for (int t = 0; t < kQT; ++t) { best[t] = -INFINITY; bestn[t] = n0; }
    // staging: thread -> (row = tid / 4, chunk' = tid % 4); source chunk = chunk' ^ ((-(row >> 2)) & 3)
    const int srow = tid >> 2, sc = (tid & 3) ^ ((0 - (srow >> 2)) & 3);
    auto stage = [&](int blk, int buf) {
#pragma unroll
        for (int i = 0; i < kRows / 64; ++i) {
            int n = n0 + blk * kRows + i * 64 + srow;
            n = n < N ? n : N - 1;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) unsigned *)(Dhi + (db + n) * 32 + sc * 8),
                                             (__attribute__((address_space(3))) unsigned *)(&lds[buf][0][i * 4096 + wave * 1024]), 16, 0, 0);
            if (LO)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) unsigned *)(Dlo + (db + n) * 32 + sc * 8),
                                                 (__attribute__((address_space(3))) unsigned *)(&lds[buf][1][i * 4096 + wave * 1024]), 16, 0, 0);
        }
    };
    const int nblk = (n1 - n0 + kRows - 1) / kRows;
    if (nblk > 0) stage(0, 0);
    for (int blk = 0; blk < nblk; ++blk) {
        const int buf = blk & 1;
        if (blk + 1 < nblk) {
            stage(blk + 1, buf ^ 1);
            static_assert(kRows == 128, "the counted waits below assume two 64-row issues per plane and stage");
            if (LO) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        const int nbase = n0 + blk * kRows;
        if (nbase + kRows > n1) nn_step<LO, true>(lds[buf][0], lds[buf][1], qh, ql, best, bestn, nbase, n1, col, g);   // last step of a split only
        else nn_step<LO, false>(lds[buf][0], lds[buf][1], qh, ql, best, bestn, nbase, n1, col, g);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                                         // reads of `buf` done before it is restaged
        __builtin_amdgcn_sched_barrier(0);
    }
    if (n0 >= n1) return;
#pragma unroll
    for (int t = 0; t < kQT; ++t) {
        merge_lane_groups(best[t], bestn[t]);
        const int q = q0 + t * 16 + col;
        if (g == 0 && q < S) atomicMax(keys + kb + Q.slot(b, q, S), make_key(best[t], bestn[t]));
    }
}

// ------------------------------------------------------------------------------------------------------------
// The SAME arg-max with most of the database never touched.  The brute-force search above scores every seed
// against every pixel of the other view (4096 x 262 144 x 2 directions per pair and round); a descriptor map is smooth,
// so whole patches of pixels can be excluded by a bound.  Per map, once per matcher call (k_frnn_blockstats): for every
// block = 8 x 8 pixel tile (64 consecutive pixels of an image row have radius 0.63 on the synthetic scene's unit
// descriptors and a quarter of all blocks survive; a square tile is four times more compact) a reference point
// c (the centroid, rounded to fp16 so that it is an exact MFMA operand), the radius r = max ||x - c|| and ||c|| + r.
// Blocks are numbered by * ceil(W / 8) + bx; block-local row 8 ry + rx is pixel (8 by + ry, 8 bx + rx); the packed map
// itself stays in raster order (a packed row is 64 bytes: the tile's rows are gathered by address).
// For a query q and ANY row x of the block (Cauchy-Schwarz)
//        <q, x> = <q, c> + <q, x - c>  <=  <q, c> + ||q|| r.
// Per search:
//   1. k_nn_mfma on the CENTROIDS (N / 64 rows) picks a promising block per query; k_frnn_seed_lb scores its 64 rows ->
//      a lower bound m(q) of the final maximum (minus a slack for the rounding differences to the MFMA scores);
//   2. k_frnn_survivors: <q, c> for all (query, block) pairs on the matrix core (1/64 of the full search), one bit per
//      (16-query tile, block): set unless  <q, c> + ||q|| (r + slack)  <  m(q)  for all 16 queries;
//   3. k_frnn_eval scores the surviving blocks through score_tile, as nn_step does (bit-identical scores), and keeps
//      (score, lowest PIXEL index) - tiles are not visited in raster order, so ties compare indices explicitly - then the
//      same 64-bit key merge; a block that holds the maximum, or a tie with it, always survives (its bound is >= its
//      best score >= m), so index AND score equal the brute-force result bit for bit;
//   4. if more than a quarter of the pairs survived (descriptors without spatial coherence, e.g. a random-weight
//      network), k_frnn_eval stands down and k_nn_mfma runs instead (both test the same device counter).
// Finite descriptors are assumed (this file is built with -fno-honor-nans, as the brute-force kernel always was).
constexpr float kRoundUp = 1.000244140625f;    // (1 + 2^-12): makes an fp32 norm or distance an upper bound of the exact one

struct Block { int y0, x0; };                  // top left pixel of a block
__device__ __forceinline__ Block block_origin(int blk, int W) {
    const int BW = (W + 7) >> 3, by = blk / BW;
    return {by * 8, (blk - by * BW) * 8};
}
// row of pixel (y, x) in its map; a pixel of the block that lies outside the map reads the block's origin instead
__device__ __forceinline__ size_t pixel_or_origin(bool inside, int y, int x, Block o, int W) {
    return inside ? (size_t)y * W + x : (size_t)o.y0 * W + o.x0;
}

__device__ __forceinline__ void load_row32(const unsigned short *__restrict__ hi, const unsigned short *__restrict__ lo, size_t row,
                                           float (&x)[32]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        union { uint4 q; _Float16 h[8]; } H, L;
        H.q = reinterpret_cast<const uint4 *>(hi + row * 32)[c];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[c * 8 + k] = (float)H.h[k];
        if (lo) {
            L.q = reinterpret_cast<const uint4 *>(lo + row * 32)[c];
#pragma unroll
            for (int k = 0; k < 8; ++k) x[c * 8 + k] += (float)L.h[k];
        }
    }
}

// cen [P][NBp][32] fp16, rad / bn [P][NBp] fp32; NBp = blocks rounded up to a multiple of 64 (padding: rad = -inf).
// One wave per tile: lane = (tile row ry = lane >> 3, dimension quad dq = lane & 7) owns the 8 pixels of its row x 4
// dimensions (8-byte loads; the 8 lanes of a row cover the pixels' 64-byte packed rows), so the centroid needs 3 shuffle
// steps per dimension quad and the squared distances 3 per pixel (lane = pixel with 32 wave reductions: 78 us per 8 maps,
// more than the searches it serves).
__global__ void __launch_bounds__(kThreads)
k_frnn_blockstats(const unsigned short *__restrict__ hi, const unsigned short *__restrict__ lo, unsigned short *__restrict__ cen,
                  float *__restrict__ rad, float *__restrict__ bn, int H, int W, int NB, int NBp) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, blk = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (blk >= NBp) return;
    const size_t sb = (size_t)b * NBp + blk;
    if (blk >= NB) {
        if (lane < 4) reinterpret_cast<uint4 *>(cen + sb * 32)[lane] = make_uint4(0u, 0u, 0u, 0u);
        if (lane == 0) { rad[sb] = -INFINITY; bn[sb] = 0.f; }
        return;
    }
    const Block o = block_origin(blk, W);
    const int ry = lane >> 3, dq = lane & 7;
    const int y = o.y0 + ry, ch = H - o.y0 < 8 ? H - o.y0 : 8, cw = W - o.x0 < 8 ? W - o.x0 : 8;
    const bool rowok = y < H;
    float v[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const bool ok = rowok && i < cw;
        const size_t row = (size_t)b * H * W + pixel_or_origin(ok, y, o.x0 + i, o, W);
        union { uint2 q; _Float16 h[4]; } A;
        A.q = *reinterpret_cast<const uint2 *>(hi + row * 32 + dq * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[i][k] = (float)A.h[k];
        if (lo) {
            A.q = *reinterpret_cast<const uint2 *>(lo + row * 32 + dq * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[i][k] += (float)A.h[k];
        }
        if (!ok) { v[i][0] = v[i][1] = v[i][2] = v[i][3] = 0.f; }
    }
    const float inv = 1.0f / (float)(ch * cw);
    float cf[4], c2 = 0.f;
    union { unsigned short h[4]; uint2 q; } C;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float sum = ((v[0][k] + v[1][k]) + (v[2][k] + v[3][k])) + ((v[4][k] + v[5][k]) + (v[6][k] + v[7][k]));
#pragma unroll
        for (int sh = 8; sh <= 32; sh <<= 1) sum += __shfl_xor(sum, sh, 64);        // over the 8 tile rows
        const _Float16 c16 = (_Float16)(sum * inv);
        C.h[k] = __builtin_bit_cast(unsigned short, c16);
        cf[k] = (float)c16;
        c2 = fmaf(cf[k], cf[k], c2);
    }
    float dmax = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float d2 = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const float e = v[i][k] - cf[k]; d2 = fmaf(e, e, d2); }
#pragma unroll
        for (int sh = 1; sh <= 4; sh <<= 1) d2 += __shfl_xor(d2, sh, 64);           // over the 8 dimension quads
        dmax = (rowok && i < cw) ? fmaxf(dmax, d2) : dmax;
    }
#pragma unroll
    for (int sh = 1; sh <= 4; sh <<= 1) c2 += __shfl_xor(c2, sh, 64);
#pragma unroll
    for (int sh = 8; sh <= 32; sh <<= 1) dmax = fmaxf(dmax, __shfl_xor(dmax, sh, 64));
    if (ry == 0) reinterpret_cast<uint2 *>(cen + sb * 32)[dq] = C.q;
    if (lane == 0) {
        const float r = sqrtf(dmax) * kRoundUp;
        rad[sb] = r;
        bn[sb] = sqrtf(c2) * kRoundUp + r;                                      // >= ||x|| for every row of the block
    }
}

// one wave per query: the exact-enough maximum over the rows of the block the centroid search chose -> mlb, ||q||
template <bool LO>
__global__ void __launch_bounds__(kThreads)
k_frnn_seed_lb(const Queries Q, const unsigned short *__restrict__ Dhi, const unsigned short *__restrict__ Dlo,
               const float *__restrict__ bn, unsigned long long *__restrict__ keysC, float *__restrict__ mlb,
               float *__restrict__ qnorm, int H, int W, int NB, int NBp) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = Q.count(b);
    const int q = blockIdx.x * (kThreads / 64) + wave;
    if (q >= S) return;
    const size_t kb = (size_t)b * Q.S_all;
    const int slot = Q.slot(b, q, S);
    int bs = key_index(keysC[kb + slot]);                                        // key 0 -> -1 -> block 0
    bs = bs < 0 ? 0 : (bs >= NB ? NB - 1 : bs);
    float qv[32], x[32];
    load_row32(Q.hi, LO ? Q.lo : nullptr, Q.row(b, slot), qv);
    const Block o = block_origin(bs, W);
    const int py = o.y0 + (lane >> 3), px = o.x0 + (lane & 7);
    const bool ok = py < H && px < W;
    load_row32(Dhi, LO ? Dlo : nullptr, (size_t)b * H * W + pixel_or_origin(ok, py, px, o, W), x);
    float sc = 0.f, q2 = 0.f;
#pragma unroll
    for (int d = 0; d < 32; ++d) { sc = fmaf(qv[d], x[d], sc); q2 = fmaf(qv[d], qv[d], q2); }
    sc = ok ? sc : -INFINITY;
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) sc = fmaxf(sc, __shfl_xor(sc, sh, 64));
    if (lane == 0) {
        const float qn = sqrtf(q2) * kRoundUp;
        mlb[kb + slot] = sc - kSlack * qn * bn[(size_t)b * NBp + bs];
        qnorm[kb + slot] = qn;
        keysC[kb + slot] = 0ull;                                                 // the scratch keys are left zero
    }
}

// surv [P][nqt_all][NBp / 64] words: bit i of word w = block 64 w + i may hold the maximum of one of the tile's 16 queries.
// This kernel computes a BOUND, not a score: <q, c> from two MFMAs (hi.hi + lo.hi of the queries, the centroid has no lo
// plane) with the QUERIES as the A operand, so it does not go through score_tile.  A lane then holds one block (column
// lane & 15) against four queries (rows 4 g + j), ORs its four tests, two shuffles OR the four lane groups and ONE ballot
// yields the tile's 16 block bits.  (With the blocks as rows every (block, lane group) bit had to be cut out of four
// ballots on the scalar unit - 120 instructions per MFMA, 82 us per search: more than the scoring of the survivors.)
constexpr int kQG = 4;                      // query tiles per wave in k_frnn_survivors
constexpr int kEvalY = 4;                   // workgroups per query tile in k_frnn_eval (1 / 2 / 4 / 8: 1292 / 1148 / 1065 / 1084 us per matcher call)
template <bool LO>
__global__ void __launch_bounds__(kThreads)
k_frnn_survivors(const Queries Q, const unsigned short *__restrict__ cen, const float *__restrict__ rad,
                 const float *__restrict__ bn, const float *__restrict__ mlb, const float *__restrict__ qnorm,
                 unsigned long long *__restrict__ surv, int32_t *__restrict__ total, int NBp, int nqt_all, int wpw) {
    const int b = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int S = Q.count(b);
    const int qt0 = (blockIdx.x * (kThreads / 64) + wave) * kQG;                 // kQG consecutive query tiles share every centroid fragment
    if (qt0 * 16 >= S) return;
    const int nt = (S - qt0 * 16 + 15) / 16 < kQG ? (S - qt0 * 16 + 15) / 16 : kQG;   // wave-uniform
    const size_t kb = (size_t)b * Q.S_all, sbase = (size_t)b * NBp;
    f16x8 qh[kQG], ql[LO ? kQG : 1];
    float mq[kQG][4], nq[kQG][4];                                                // the four queries per tile this lane gets scores of
#pragma unroll
    for (int u = 0; u < kQG; ++u) {
        const size_t qr = Q.row(b, Q.slot(b, (qt0 + u) * 16 + col, S));
        qh[u] = Q.frag(Q.hi, qr, g);                                             // A: row = query col, k chunk g
        if (LO) ql[u] = Q.frag(Q.lo, qr, g);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int sj = Q.slot(b, (qt0 + u) * 16 + 4 * g + j, S);
            mq[u][j] = mlb[kb + sj];
            nq[u][j] = qnorm[kb + sj];
        }
    }
    const int NBW = NBp / 64;
    const int w0 = blockIdx.y * wpw, w1 = w0 + wpw < NBW ? w0 + wpw : NBW;
    int cnt = 0;
    for (int w = w0; w < w1; ++w) {
        f16x8 c[4];
        float e[4], r[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {                                            // B: column = block col, k chunk g
            const size_t blk = sbase + w * 64 + t * 16 + col;
            c[t] = *reinterpret_cast<const f16x8 *>(cen + blk * 32 + g * 8);
            r[t] = rad[blk];
            e[t] = r[t] + kSlack * bn[blk];
        }
#pragma unroll
        for (int u = 0; u < kQG; ++u) {
            if (u >= nt) break;
            unsigned long long bits = 0ull;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(qh[u], c[t], acc, 0, 0, 0);
                if (LO) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ql[u], c[t], acc, 0, 0, 0);
                bool keep = false;
#pragma unroll
                for (int j = 0; j < 4; ++j) keep = keep || !(acc[j] + nq[u][j] * e[t] < mq[u][j]);
                int k = (keep && !(r[t] < 0.f)) ? 1 : 0;                          // padding blocks have r = -inf
                k |= __shfl_xor(k, 16, 64);
                k |= __shfl_xor(k, 32, 64);
                bits |= (__ballot(k != 0) & 0xffffull) << (16 * t);
            }
            if (lane == 0) surv[((size_t)b * nqt_all + qt0 + u) * NBW + w] = bits;
            cnt += __popcll(bits);
        }
    }
    if (lane == 0 && cnt) atomicAdd(total + b, cnt);
}

// grid (query tiles, kEvalY, P): ONE 16-query tile per workgroup, whose 4 x kEvalY waves take the words of the tile's
// survivor row round-robin (interleaved by 64-block word so that a cluster of survivors spreads).  (Four tiles per
// workgroup sharing every gathered block: 135 instead of 55 us per search - the kernel is bound by the serial work of a
// wave, not by the gathers the tiles would share.)  The rows of the NEXT surviving block are requested before the current
// block is scored (two register sets, alternating: with one set and a copy the wait for the copy exposed every round trip).
template <bool LO>
__global__ void __launch_bounds__(kThreads)
k_frnn_eval(const Queries Q, const unsigned short *__restrict__ Dhi, const unsigned short *__restrict__ Dlo,
            const unsigned long long *__restrict__ surv, const int32_t *__restrict__ total, unsigned long long *__restrict__ keys,
            int H, int W, int NB, int NBp, int nqt_all) {
    const int b = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const int S = Q.count(b), qt = blockIdx.x;
    if (qt * 16 >= S || prune_overflow(total[b], S, NB)) return;
    const size_t kb = (size_t)b * Q.S_all, db = (size_t)b * H * W;
    const int slot = Q.slot(b, qt * 16 + col, S);
    const size_t qr = Q.row(b, slot);
    const f16x8 qh = Q.frag(Q.hi, qr, g), ql = LO ? Q.frag(Q.lo, qr, g) : qh;
    float best = -INFINITY;
    int bestn = 0;
    const int NBW = NBp / 64;
    const unsigned long long *srow = surv + ((size_t)b * nqt_all + qt) * NBW;
    constexpr int NA = LO ? 8 : 4;
    const int stride = (kThreads / 64) * (int)gridDim.y, first = wave + (kThreads / 64) * (int)blockIdx.y;
    for (int wbase = first; wbase < NBW; wbase += 64 * stride) {                // 64 words of this wave at a time (one per lane)
        const int wmine = wbase + lane * stride;
        const unsigned long long mine = wmine < NBW ? srow[wmine] : 0ull;
        int k = -1;
        unsigned long long bits = 0ull;
        auto next_block = [&]() -> int {                                         // wave-uniform; -1 = no more
            while (bits == 0ull) {
                if (++k >= 64 || wbase + k * stride >= NBW) return -1;
                const unsigned lo32 = __builtin_amdgcn_readlane((unsigned)mine, k), hi32 = __builtin_amdgcn_readlane((unsigned)(mine >> 32), k);
                bits = ((unsigned long long)hi32 << 32) | lo32;
            }
            const int i = __builtin_ctzll(bits);
            bits &= bits - 1ull;
            return (wbase + k * stride) * 64 + i;
        };
        auto load_rows = [&](int blk, f16x8 (&a)[NA]) {                          // A rows 16 h + col = pixel (y0 + 2 h + (col >> 3), x0 + (col & 7))
            const Block o = block_origin(blk, W);
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                int py = o.y0 + 2 * h + (col >> 3), px = o.x0 + (col & 7);      // outside the map: the nearest pixel, masked in score
                py = py < H ? py : H - 1;
                px = px < W ? px : W - 1;
                const size_t row = db + (size_t)py * W + px;
                a[h] = *reinterpret_cast<const f16x8 *>(Dhi + row * 32 + g * 8);
                if (LO) a[4 + h] = *reinterpret_cast<const f16x8 *>(Dlo + row * 32 + g * 8);
            }
        };
        auto score = [&](int blk, const f16x8 (&a)[NA]) {
            const Block o = block_origin(blk, W);
            const int y0 = o.y0, x0 = o.x0;
            // this lane's outputs: tile h, j -> block row 16 h + 4 g + j = pixel (y0 + 2 h + (g >> 1), x0 + 4 (g & 1) + j)
            const int ox = x0 + 4 * (g & 1);
            const bool edge = y0 + 8 > H || x0 + 8 > W;                         // tiles on the bottom / right edge
            f32x4 acc[4];
#pragma unroll
            for (int h = 0; h < 4; ++h) acc[h] = score_tile<LO>(a[h], a[LO ? 4 + h : h], qh, ql);   // nn_step's scores: same bits
            if (edge) {
#pragma unroll
                for (int h = 0; h < 4; ++h)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (y0 + 2 * h + (g >> 1) >= H || ox + j >= W) acc[h][j] = -INFINITY;
            }
            float mx = acc[0][0];
#pragma unroll
            for (int h = 0; h < 4; ++h)
#pragma unroll
                for (int j = 0; j < 4; ++j) mx = __builtin_fmaxf(mx, acc[h][j]);
            const bool ge = mx >= best && mx > -INFINITY;                       // ties included: the LOWEST pixel index must win
            if (__any(ge)) {                                                    // rare after the first few blocks
                int nn = 0x7fffffff;                                            // lowest pixel index of this lane that holds mx
#pragma unroll
                for (int h = 3; h >= 0; --h)
#pragma unroll
                    for (int j = 3; j >= 0; --j) nn = (acc[h][j] == mx) ? (y0 + 2 * h + (g >> 1)) * W + ox + j : nn;
                if (ge && (mx > best || nn < bestn)) { best = mx; bestn = nn; }
            }
        };
        f16x8 ra[NA], rb[NA];
        int ba = next_block();
        if (ba >= 0) load_rows(ba, ra);
        while (ba >= 0) {
            const int bb = next_block();
            if (bb >= 0) load_rows(bb, rb);
            score(ba, ra);
            if (bb < 0) break;
            ba = next_block();
            if (ba >= 0) load_rows(ba, ra);
            score(bb, rb);
        }
    }
    merge_lane_groups(best, bestn);                                             // a lane that scored nothing holds (-inf, 0)
    if (g == 0 && qt * 16 + col < S) atomicMax(keys + kb + slot, make_key(best, bestn));
}

// ---- one round of fast reciprocal NN on the device (matching.fast_reciprocal_nn_device), batched over P pairs -----------
// mid: keys of the forward search -> xy2 (the view-2 pixel each seed landed on), keys cleared for the backward search
__global__ void __launch_bounds__(kThreads)
k_frnn_mid(unsigned long long *__restrict__ keys, int32_t *__restrict__ xy2, long long total) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    xy2[i] = key_index(keys[i]);                                              // (inactive slots: key 0 -> -1, which nobody reads)
    keys[i] = 0ull;
}
// Ordered compaction, one step of 256 entries: the rank of a flagged thread among the workgroup's flagged threads in thread
// order (one ballot per wave, the wave counts through LDS) and their number.  wsum: [2][kThreads / 64], the halves taken
// in turn (step & 1), so that ONE barrier per step separates the writes of a step from the reads of the step before.
__device__ __forceinline__ int ballot_rank(bool flag, int (*wsum)[kThreads / 64], int step, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    int *ws = wsum[step & 1];
    if (lane == 0) ws[wave] = __popcll(m);
    __syncthreads();
    int off = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) { off += w < wave ? ws[w] : 0; total += ws[w]; }
    return off + __popcll(m & ((1ull << lane) - 1ull));
}
// compact: the still-active seed slots of every pair, ascending, + their number - the query list of the next round's
// searches.  One workgroup per pair walks its S flags in order: deterministic.
__global__ void __launch_bounds__(kThreads)
k_frnn_compact(const uint8_t *__restrict__ active, const int32_t *__restrict__ order, int32_t *__restrict__ list,
               int32_t *__restrict__ count, int S) {
    __shared__ int wsum[2][kThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    int base = 0;
    for (int s0 = 0, step = 0; s0 < S; s0 += kThreads, ++step) {
        const int pos = s0 + tid;
        const int sl = (order && pos < S) ? order[pos] : pos;                   // walk the slots in the caller's order (NULL: ascending)
        const bool a = pos < S && sl >= 0 && sl < S && active[(size_t)b * S + sl] != 0;
        int n;
        const int r = ballot_rank(a, wsum, step, n);
        if (a) list[(size_t)b * S + base + r] = sl;
        base += n;
    }
    if (tid == 0) count[b] = base;
}
// collect: every reciprocal pair of every round (got1 / got2 [rounds][P][S], -1 = none) into dense maps - map1[pair][p1]
// = p2 (int32, -1 = none) and, for the tracker, idx2[pair][p2] = p1 / valid2[pair][p2] = 1.  A reciprocal pair is mutual,
// so p1 <-> p2 is one-to-one per image pair and seeds that found the same pair write the same values.
__global__ void __launch_bounds__(kThreads)
k_frnn_scatter(const int32_t *__restrict__ got1, const int32_t *__restrict__ got2, int32_t *__restrict__ map1,
               long long *__restrict__ idx2, uint8_t *__restrict__ valid2, int P, int S, int N1, int N2, long long total) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int p1 = got1[i], p2 = got2[i];
    if (p1 < 0 || p1 >= N1 || p2 < 0 || p2 >= N2) return;
    const int b = (int)((i / S) % P);
    map1[(size_t)b * N1 + p1] = p2;
    if (idx2) { idx2[(size_t)b * N2 + p2] = p1; valid2[(size_t)b * N2 + p2] = 1; }
}
// the distinct pairs as a list sorted by (pair, p1): ordered compaction of map1 in two launches (per-chunk counts, then
// offsets = sum of the counts in front + the rank inside the chunk) - what torch.unique (a sort and a host synchronisation) did
constexpr int kChunk = kThreads * 16;
// the steps of chunk c of a map1 row m: f(step, i, kept) for this thread's entry i of every step, kept = a pixel with a partner
template <class F>
__device__ __forceinline__ void chunk_keep(const int32_t *__restrict__ m, int c, int N1, F &&f) {
    for (int k = 0; k < kChunk / kThreads; ++k) {
        const int i = c * kChunk + k * kThreads + (int)threadIdx.x;
        f(k, i, i < N1 && m[i] >= 0);
    }
}
__global__ void __launch_bounds__(kThreads)
k_frnn_count(const int32_t *__restrict__ map1, int32_t *__restrict__ chunk_cnt, int N1, int nchunk) {
    __shared__ int wsum[kThreads / 64];
    const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
    int n = 0;                                                                   // wave-uniform
    chunk_keep(map1 + (size_t)b * N1, c, N1, [&](int, int, bool kept) { n += __popcll(__ballot(kept)); });
    if ((tid & 63) == 0) wsum[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) { int t = 0; for (int w = 0; w < kThreads / 64; ++w) t += wsum[w]; chunk_cnt[b * nchunk + c] = t; }
}
__global__ void __launch_bounds__(kThreads)
k_frnn_emit(const int32_t *__restrict__ map1, const int32_t *__restrict__ chunk_cnt, int32_t *__restrict__ pairs,
            int32_t *__restrict__ count, int N1, int nchunk, int cap) {
    __shared__ int wsum[2][kThreads / 64];
    const int b = blockIdx.y, c = blockIdx.x;
    const int32_t *m = map1 + (size_t)b * N1;
    int o = 0, tot = 0;                                                          // pairs of this map in front of chunk c / in all chunks
    for (int k = 0; k < nchunk; ++k) { const int v = chunk_cnt[b * nchunk + k]; o += k < c ? v : 0; tot += v; }
    if (c == 0 && threadIdx.x == 0) count[b] = tot < cap ? tot : cap;
    chunk_keep(m, c, N1, [&](int step, int i, bool kept) {
        int n;
        const int at = o + ballot_rank(kept, wsum, step, n);
        if (kept && at < cap) { pairs[((size_t)b * cap + at) * 2] = i; pairs[((size_t)b * cap + at) * 2 + 1] = m[i]; }
        o += n;
    });
}
// end: keys of the backward search -> back; a seed that returned to where it started is a reciprocal pair (recorded in
// row `round` of got1 / got2, -1 elsewhere) and leaves the active set, the others continue from where they landed
__global__ void __launch_bounds__(kThreads)
k_frnn_end(unsigned long long *__restrict__ keys, const int32_t *__restrict__ xy2, int32_t *__restrict__ cur,
           uint8_t *__restrict__ active, int32_t *__restrict__ got1, int32_t *__restrict__ got2, long long total) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int32_t back = key_index(keys[i]);
    keys[i] = 0ull;
    const int32_t c = cur[i];
    const bool act = active[i] != 0, conv = act && back == c;
    got1[i] = conv ? c : -1;
    got2[i] = conv ? xy2[i] : -1;
    active[i] = (uint8_t)(act && !conv);
    if (act && !conv) cur[i] = back;
}

// ---- host side: buffer views, the split plan and the launches every entry point shares ----------------------------------
// Each scratch layout is written down once, in the view that hands out its pointers.  A view on a NULL base has null
// pointers and still knows its size: that is what the m3_*_bytes entry points return.
inline char *at(const void *base, int64_t off) { return base ? (char *)base + off : nullptr; }

struct PackedMap {      // a descriptor map packed by k_nn_pack: hi fp16 [P][N][32] (K zero-padded), then lo for fp32 descriptors
    unsigned short *hi, *lo;
    int P, N;
    int64_t bytes;
    PackedMap(const void *p, int P, int N, int in_f16)
        : hi((unsigned short *)at(p, 0)), lo(in_f16 ? nullptr : (unsigned short *)at(p, (int64_t)P * N * 64)), P(P), N(N),
          bytes((int64_t)P * N * 64 * (in_f16 ? 1 : 2)) {}
};

struct BlockStats {     // k_frnn_blockstats of an H x W map: NB 8 x 8 pixel blocks per pair, stored with the pair stride NBp
    int H, W, NB, NBp;  // (NB rounded up to 64): centroids fp16 [P][NBp][32], then rad fp32 [P][NBp], then bn fp32 [P][NBp]
    unsigned short *cen;
    float *rad, *bn;
    int64_t bytes;
    BlockStats(const void *p, int P, int H, int W)
        : H(H), W(W), NB(m3_cdiv(H, 8) * m3_cdiv(W, 8)), NBp(m3_cdiv(NB, 64) * 64), cen((unsigned short *)at(p, 0)),
          rad((float *)at(p, (int64_t)P * NBp * 64)), bn((float *)at(p, (int64_t)P * NBp * 68)), bytes((int64_t)P * NBp * 72) {}
};

struct PruneWs {        // scratch of one block-bound search for S seeds and a database of nbp (padded) blocks
    int64_t head_bytes;                  // centroid-search keys [P][S] + survivor totals [P], padded to 16 bytes: zeroed per search
    unsigned long long *keysC;
    int32_t *total;
    float *mlb, *qn;                     // [P][S] each
    unsigned long long *surv;            // survivor bits [P][cdiv(S, 16)][nbp / 64]
    int64_t bytes;
    PruneWs(const void *p, int P, int S, int nbp)
        : head_bytes(((int64_t)P * S * 8 + (int64_t)P * 4 + 15) / 16 * 16), keysC((unsigned long long *)at(p, 0)),
          total((int32_t *)at(p, (int64_t)P * S * 8)), mlb((float *)at(p, head_bytes)), qn((float *)at(p, head_bytes + (int64_t)P * S * 4)),
          surv((unsigned long long *)at(p, head_bytes + (int64_t)P * S * 8)),
          bytes(head_bytes + (int64_t)P * S * 8 + (int64_t)P * m3_cdiv(S, 16) * (nbp / 64) * 8) {}
};

// The database is split over blockIdx.y so that about `target` workgroups run: at most max_splits, every split but the
// last a whole number of `step` rows.
struct SearchPlan { dim3 grid; int per_split; };
SearchPlan plan_search(int qblocks, int N, int P, int target, int max_splits, int step) {
    int splits = m3_cdiv(target, qblocks * P);
    if (splits < 1) splits = 1;
    if (splits > max_splits) splits = max_splits;
    if (splits > m3_cdiv(N, step)) splits = m3_cdiv(N, step);
    const int per_split = m3_cdiv(m3_cdiv(N, splits), step) * step;
    return {dim3(qblocks, m3_cdiv(N, per_split), P), per_split};
}
// ~4 workgroups per CU over the whole call, whole LDS steps except in the last split
SearchPlan plan_mfma_search(int S, int N, int P) { return plan_search(m3_cdiv(S, kQPB), N, P, 1024, 1024, kRows); }

// The queries of a search: S seed slots per pair whose rows (qidx; null: row s) lie in the packed map q
Queries queries(const PackedMap &q, const int32_t *qidx, int S, const int32_t *qlist = nullptr, const int32_t *qcount = nullptr) {
    return {q.hi, q.lo, qidx, qlist, qcount, S, q.N};
}

// The brute-force MFMA search of the queries in d: one pass for lo-less maps, three otherwise.
// gate_total / gate_nb: the fallback form of the block-bound search.
void launch_nn_mfma(const Queries &q, const PackedMap &d, unsigned long long *keys, const SearchPlan &pl, hipStream_t st,
                    const int32_t *gate_total = nullptr, int gate_nb = 0) {
    hipLaunchKernelGGL(d.lo ? k_nn_mfma<true> : k_nn_mfma<false>, pl.grid, dim3(kThreads), 0, st, q, d.hi, d.lo, keys, d.N,
                       pl.per_split, gate_total, gate_nb);
}

// X [m.P * m.N][D], IEEE fp16 for a lo-less map and fp32 otherwise, to the K-padded planes of m
void launch_pack(const void *X, const PackedMap &m, int D, hipStream_t st) {
    const long long rows = (long long)m.P * m.N;
    const auto k = m.lo ? (D == 24 ? k_nn_pack<false, 24> : D == 16 ? k_nn_pack<false, 16> : k_nn_pack<false, 32>)
                        : (D == 24 ? k_nn_pack<true, 24> : D == 16 ? k_nn_pack<true, 16> : k_nn_pack<true, 32>);
    hipLaunchKernelGGL(k, dim3((unsigned)m3_cdiv(rows * 4, (long long)kThreads)), dim3(kThreads), 0, st, X, m.hi, m.lo, rows);
}

void launch_unpack(const unsigned long long *keys, int32_t *idx_out, float *score_out, long long total, hipStream_t st) {
    hipLaunchKernelGGL(k_nn_unpack, dim3((unsigned)m3_cdiv(total, (long long)kThreads)), dim3(kThreads), 0, st, keys, idx_out,
                       score_out, total);
}

// One search of a round: the queries against d, merged into keys - the brute-force kernel.  With ds, the statistics of d,
// the block bounds run first (prune_ws: PruneWs scratch) and gate it.
int frnn_search(const Queries &q, const PackedMap &d, const BlockStats *ds, unsigned long long *keys, hipStream_t st,
                void *prune_ws) {
    const int P = d.P, S = q.S_all;
    const int32_t *gate_total = nullptr;
    if (ds) {
        const int H = ds->H, W = ds->W, NB = ds->NB, NBp = ds->NBp, NBW = NBp / 64, nqt = m3_cdiv(S, 16);
        const PruneWs ws(prune_ws, P, S, NBp);
        M3_CHECK_HIP(hipMemsetAsync(ws.keysC, 0, (size_t)ws.head_bytes, st), "m3_frnn_round_pruned/memset");
        // 1. the most promising block per query: the brute-force kernel on the centroids (hi plane of the queries).  The
        // centroid table is [P][NBp][32] and the search runs over NBp rows, so that pair b's rows start at b * NBp as
        // k_frnn_blockstats laid them out; the padding rows are zero vectors and k_frnn_seed_lb clamps the chosen block
        // to < NB
        launch_nn_mfma(q, PackedMap(ds->cen, P, NBp, 1), ws.keysC, plan_mfma_search(S, NBp, P), st);
        const dim3 blk(kThreads), gl(m3_cdiv(S, kThreads / 64), P);
        const int ngrp = m3_cdiv(nqt, kQG);
        int ysplit = m3_cdiv(8192, ngrp * P);
        ysplit = ysplit < 1 ? 1 : (ysplit > NBW ? NBW : ysplit);
        const int wpw = m3_cdiv(NBW, ysplit);
        const dim3 gs(m3_cdiv(ngrp, kThreads / 64), m3_cdiv(NBW, wpw), P), ge(nqt, kEvalY, P);
        // 2. - 3. lower bound per query, surviving blocks per query tile, exact scores of the survivors
        hipLaunchKernelGGL(d.lo ? k_frnn_seed_lb<true> : k_frnn_seed_lb<false>, gl, blk, 0, st, q, d.hi, d.lo, ds->bn, ws.keysC,
                           ws.mlb, ws.qn, H, W, NB, NBp);
        hipLaunchKernelGGL(d.lo ? k_frnn_survivors<true> : k_frnn_survivors<false>, gs, blk, 0, st, q, ds->cen, ds->rad, ds->bn,
                           ws.mlb, ws.qn, ws.surv, ws.total, NBp, nqt, wpw);
        hipLaunchKernelGGL(d.lo ? k_frnn_eval<true> : k_frnn_eval<false>, ge, blk, 0, st, q, d.hi, d.lo, ws.surv, ws.total, keys,
                           H, W, NB, NBp, nqt);
        gate_total = ws.total;      // 4. gated on the survivor count, the workgroups below leave at once when the bounds worked
    }
    launch_nn_mfma(q, d, keys, plan_mfma_search(S, d.N, P), st, gate_total, ds ? ds->NB : 0);
    return M3_OK;
}

// One round for P pairs: the optional compaction of the active seeds into act_ws (list [P][S], then count [P]), view 1 ->
// view 2, k_frnn_mid, and back, k_frnn_end.  s1 / s2: statistics of m1 / m2, or null for the brute-force search;
// where: the caller's name for the launch check.
int frnn_round(const PackedMap &m1, const PackedMap &m2, const BlockStats *s1, const BlockStats *s2, int32_t *cur, uint8_t *active,
               int32_t *got1, int32_t *got2, int32_t *xy2_ws, uint64_t *keys_ws, int32_t *act_ws, const int32_t *seed_order,
               void *prune_ws, int S, hipStream_t st, const char *where) {
    const int P = m1.P;
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(keys_ws);
    int32_t *list = act_ws, *count = act_ws ? act_ws + (size_t)P * S : nullptr;
    const long long total = (long long)P * S;
    const dim3 eb(kThreads), eg((unsigned)m3_cdiv(total, (long long)kThreads));
    if (act_ws) hipLaunchKernelGGL(k_frnn_compact, dim3(P), eb, 0, st, active, seed_order, list, count, S);
    int rc = frnn_search(queries(m1, cur, S, list, count), m2, s2, keys, st, prune_ws);           // view 1 -> view 2
    if (rc != M3_OK) return rc;
    hipLaunchKernelGGL(k_frnn_mid, eg, eb, 0, st, keys, xy2_ws, total);
    rc = frnn_search(queries(m2, xy2_ws, S, list, count), m1, s1, keys, st, prune_ws);            // and back
    if (rc != M3_OK) return rc;
    hipLaunchKernelGGL(k_frnn_end, eg, eb, 0, st, keys, xy2_ws, cur, active, got1, got2, total);
    M3_CHECK_LAUNCH(where);
    return M3_OK;
}

}  // namespace

extern "C" {

int m3_nn_search(const float *Q, const float *DB, int32_t *idx_out, float *score_out, uint64_t *keys_ws,
                 int B, int S, int N, int D, void *stream) {
    M3_REQUIRE(Q && DB && idx_out && keys_ws && B > 0 && S > 0 && N > 0 && B <= 65535);
    M3_REQUIRE(D == 16 || D == 24 || D == 32);
    M3_REQUIRE(((reinterpret_cast<size_t>(Q) | reinterpret_cast<size_t>(DB)) & 15) == 0);
    hipStream_t st = (hipStream_t)stream;
    M3_CHECK_HIP(hipMemsetAsync(keys_ws, 0, (size_t)B * S * 8, st), "m3_nn_search/memset");
    const SearchPlan pl = plan_search(m3_cdiv(S, kThreads * kQPL), N, B, 2048, 1024, 1);   // ~8 workgroups per CU over the whole call
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(keys_ws);
    hipLaunchKernelGGL(D == 24 ? k_nn_search<24> : D == 16 ? k_nn_search<16> : k_nn_search<32>, pl.grid, dim3(kThreads), 0, st, Q, DB,
                       keys, S, N, pl.per_split);
    M3_CHECK_LAUNCH("m3_nn_search");
    launch_unpack(keys, idx_out, score_out, (long long)B * S, st);
    M3_CHECK_LAUNCH("m3_nn_search/unpack");
    return M3_OK;
}

// MFMA search.  Q [B,S,D], DB [B,N,D] in fp32 (in_f16 = 0) or IEEE fp16 (in_f16 = 1), D <= 32 and D % 4 == 0.
// pack_ws: m3_nn_pack_bytes(B, S, N, in_f16) bytes of scratch: the packed queries, then the packed database.
int64_t m3_nn_pack_bytes(int B, int S, int N, int in_f16) {
    if (B <= 0 || S <= 0 || N <= 0) return 0;
    return PackedMap(nullptr, B, S, in_f16).bytes + PackedMap(nullptr, B, N, in_f16).bytes;
}

int m3_nn_search_mfma(const void *Q, const void *DB, int32_t *idx_out, float *score_out, uint64_t *keys_ws,
                      void *pack_ws, int B, int S, int N, int D, int in_f16, void *stream) {
    M3_REQUIRE(Q && DB && idx_out && keys_ws && pack_ws && B > 0 && S > 0 && N > 0 && B <= 65535);
    M3_REQUIRE((D == 16 || D == 24 || D == 32) && (reinterpret_cast<size_t>(pack_ws) & 15) == 0);
    hipStream_t st = (hipStream_t)stream;
    const PackedMap q(pack_ws, B, S, in_f16), d(at(pack_ws, q.bytes), B, N, in_f16);
    launch_pack(Q, q, D, st);
    launch_pack(DB, d, D, st);
    M3_CHECK_LAUNCH("m3_nn_search_mfma/pack");
    M3_CHECK_HIP(hipMemsetAsync(keys_ws, 0, (size_t)B * S * 8, st), "m3_nn_search_mfma/memset");
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(keys_ws);
    launch_nn_mfma(queries(q, nullptr, S), d, keys, plan_mfma_search(S, N, B), st);
    M3_CHECK_LAUNCH("m3_nn_search_mfma");
    launch_unpack(keys, idx_out, score_out, (long long)B * S, st);
    M3_CHECK_LAUNCH("m3_nn_search_mfma/unpack");
    return M3_OK;
}


// ---- batched fast reciprocal NN: pack each descriptor map ONCE, then rounds of (forward search, backward search) ------
int64_t m3_frnn_pack_bytes(int P, int N, int in_f16) {
    if (P <= 0 || N <= 0) return 0;
    return PackedMap(nullptr, P, N, in_f16).bytes;
}
int m3_frnn_pack(const void *Dmap, void *packed, int P, int N, int D, int in_f16, void *stream) {
    M3_REQUIRE(Dmap && packed && P > 0 && N > 0 && (D == 16 || D == 24 || D == 32));
    M3_REQUIRE((reinterpret_cast<size_t>(packed) & 15) == 0);
    launch_pack(Dmap, PackedMap(packed, P, N, in_f16), D, (hipStream_t)stream);
    M3_CHECK_LAUNCH("m3_frnn_pack");
    return M3_OK;
}

// One round for P pairs at once (no reference counterpart: SURVEY 8a row K8).  packed1 / packed2: the two views'
// packed maps (m3_frnn_pack; N1 / N2 rows per pair).  cur int32 [P,S]: the view-1 pixel every seed currently sits on
// (in / out), active uint8 [P,S] (in / out), got1 / got2 int32 [P,S]: this round's reciprocal pairs (-1 = none),
// xy2_ws int32 [P,S] and keys_ws uint64 [P,S] scratch; keys_ws must be ZERO on entry (it is left zero).
int m3_frnn_round(const void *packed1, const void *packed2, int32_t *cur, uint8_t *active, int32_t *got1, int32_t *got2,
                  int32_t *xy2_ws, uint64_t *keys_ws, int P, int S, int N1, int N2, int in_f16, void *stream) {
    M3_REQUIRE(packed1 && packed2 && cur && active && got1 && got2 && xy2_ws && keys_ws);
    M3_REQUIRE(P > 0 && P <= 65535 && S > 0 && N1 > 0 && N2 > 0);
    return frnn_round(PackedMap(packed1, P, N1, in_f16), PackedMap(packed2, P, N2, in_f16), nullptr, nullptr, cur, active, got1,
                      got2, xy2_ws, keys_ws, nullptr, nullptr, nullptr, S, (hipStream_t)stream, "m3_frnn_round");
}

// m3_frnn_round restricted to the seeds that are still active: act_ws int32 [P * (S + 1)] scratch receives the ascending
// list of active seed slots of every pair ([P][S]) and their count ([P]); the two searches then run on those queries only
// (workgroups past a pair's count exit at once).  After the first round most seeds of a well-textured pair have found
// their mutual nearest neighbour, so rounds >= 2 cost a fraction of a full round.  Same results as m3_frnn_round.
int m3_frnn_round_active(const void *packed1, const void *packed2, int32_t *cur, uint8_t *active, int32_t *got1,
                         int32_t *got2, int32_t *xy2_ws, uint64_t *keys_ws, int32_t *act_ws, int P, int S, int N1, int N2,
                         int in_f16, void *stream) {
    M3_REQUIRE(packed1 && packed2 && cur && active && got1 && got2 && xy2_ws && keys_ws && act_ws);
    M3_REQUIRE(P > 0 && P <= 65535 && S > 0 && N1 > 0 && N2 > 0);
    return frnn_round(PackedMap(packed1, P, N1, in_f16), PackedMap(packed2, P, N2, in_f16), nullptr, nullptr, cur, active, got1,
                      got2, xy2_ws, keys_ws, act_ws, nullptr, nullptr, S, (hipStream_t)stream, "m3_frnn_round_active");
}

// ---- block-bound search: statistics of a packed map, scratch, and the round built on it ---------------------------------
int64_t m3_frnn_stats_bytes(int P, int H, int W) {
    if (P <= 0 || H <= 0 || W <= 0) return 0;
    return BlockStats(nullptr, P, H, W).bytes;
}
int m3_frnn_blockstats(const void *packed, void *stats, int P, int H, int W, int in_f16, void *stream) {
    M3_REQUIRE(packed && stats && P > 0 && P <= 65535 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31));
    M3_REQUIRE((reinterpret_cast<size_t>(stats) & 15) == 0);
    const PackedMap m(packed, P, H * W, in_f16);
    const BlockStats s(stats, P, H, W);
    hipLaunchKernelGGL(k_frnn_blockstats, dim3(m3_cdiv(s.NBp, kThreads / 64), P), dim3(kThreads), 0, (hipStream_t)stream, m.hi, m.lo,
                       s.cen, s.rad, s.bn, H, W, s.NB, s.NBp);
    M3_CHECK_LAUNCH("m3_frnn_blockstats");
    return M3_OK;
}
// scratch of m3_frnn_round_pruned for S seeds: one PruneWs, sized for the map with more blocks
int64_t m3_frnn_prune_ws_bytes(int P, int S, int H1, int W1, int H2, int W2) {
    if (P <= 0 || S <= 0 || H1 <= 0 || W1 <= 0 || H2 <= 0 || W2 <= 0) return 0;
    const int nbp1 = BlockStats(nullptr, P, H1, W1).NBp, nbp2 = BlockStats(nullptr, P, H2, W2).NBp;
    return PruneWs(nullptr, P, S, nbp1 > nbp2 ? nbp1 : nbp2).bytes;
}

// m3_frnn_round / m3_frnn_round_active with the block-bound search: the maps are H1 x W1 / H2 x W2 pixels in raster order,
// stats1 / stats2 = m3_frnn_blockstats of packed1 / packed2, prune_ws = m3_frnn_prune_ws_bytes(...) bytes of scratch
// (16-byte aligned), act_ws as in m3_frnn_round_active or NULL (round on every seed slot).  seed_order int32 [S] (or NULL):
// the order in which the active slots are listed - the searches work on groups of 16 / 64 CONSECUTIVE list entries, and
// the fewer blocks the queries of a group need between them, the less is scored: an order that walks the seed grid in
// 4 x 4 patches (matching.py) halves the surviving work of a row-major one.  It changes no result (requires act_ws).
// Same cur / active / got1 / got2 as the brute-force rounds, bit for bit; the time follows how well the descriptor maps
// cluster.
int m3_frnn_round_pruned(const void *packed1, const void *packed2, const void *stats1, const void *stats2, int32_t *cur,
                         uint8_t *active, int32_t *got1, int32_t *got2, int32_t *xy2_ws, uint64_t *keys_ws, int32_t *act_ws,
                         const int32_t *seed_order, void *prune_ws, int P, int S, int H1, int W1, int H2, int W2, int in_f16,
                         void *stream) {
    M3_REQUIRE(packed1 && packed2 && stats1 && stats2 && cur && active && got1 && got2 && xy2_ws && keys_ws && prune_ws);
    M3_REQUIRE(P > 0 && P <= 65535 && S > 0 && H1 > 0 && W1 > 0 && H2 > 0 && W2 > 0 && (reinterpret_cast<size_t>(prune_ws) & 15) == 0);
    M3_REQUIRE((int64_t)H1 * W1 < (1ll << 31) && (int64_t)H2 * W2 < (1ll << 31) && (!seed_order || act_ws));
    const BlockStats s1(stats1, P, H1, W1), s2(stats2, P, H2, W2);
    return frnn_round(PackedMap(packed1, P, H1 * W1, in_f16), PackedMap(packed2, P, H2 * W2, in_f16), &s1, &s2, cur, active, got1,
                      got2, xy2_ws, keys_ws, act_ws, seed_order, prune_ws, S, (hipStream_t)stream, "m3_frnn_round_pruned");
}

// The reciprocal pairs of `rounds` rounds (got1 / got2 int32 [rounds,P,S]) as FIXED-SHAPE device outputs - no sort, no
// host synchronisation, so the whole matcher can be captured into a hipGraph:
//   map1  int32 [P,N1]   view-1 pixel -> its reciprocal partner in view 2, -1 = none            (always written)
//   idx2  int64 [P,N2], valid2 uint8 [P,N2]   the tracker's maps: view-2 pixel -> view-1 pixel  (optional: both or none)
//   pairs int32 [P,S,2], count int32 [P]   the distinct (p1, p2) of every image pair sorted by p1, rows >= count[pair] = -1
//                                          (a seed converges at most once: S bounds the number of pairs)
//   chunk_ws int32 [P * m3_frnn_chunks(N1)] scratch.
int m3_frnn_chunks(int N1) { return N1 > 0 ? (N1 + kChunk - 1) / kChunk : 0; }
int m3_frnn_collect(const int32_t *got1, const int32_t *got2, int rounds, int P, int S, int N1, int N2, int32_t *map1,
                    int64_t *idx2, uint8_t *valid2, int32_t *pairs, int32_t *count, int32_t *chunk_ws, void *stream) {
    M3_REQUIRE(got1 && got2 && map1 && pairs && count && chunk_ws && rounds > 0 && P > 0 && P <= 65535 && S > 0 && N1 > 0 && N2 > 0);
    M3_REQUIRE((idx2 == nullptr) == (valid2 == nullptr));
    hipStream_t st = (hipStream_t)stream;
    M3_CHECK_HIP(hipMemsetAsync(map1, 0xff, (size_t)P * N1 * 4, st), "m3_frnn_collect/memset");
    M3_CHECK_HIP(hipMemsetAsync(pairs, 0xff, (size_t)P * S * 8, st), "m3_frnn_collect/memset");
    if (idx2) {
        M3_CHECK_HIP(hipMemsetAsync(idx2, 0, (size_t)P * N2 * 8, st), "m3_frnn_collect/memset");
        M3_CHECK_HIP(hipMemsetAsync(valid2, 0, (size_t)P * N2, st), "m3_frnn_collect/memset");
    }
    const long long total = (long long)rounds * P * S;
    hipLaunchKernelGGL(k_frnn_scatter, dim3((unsigned)m3_cdiv(total, (long long)kThreads)), dim3(kThreads), 0, st, got1, got2, map1,
                       (long long *)idx2, valid2, P, S, N1, N2, total);
    const int nchunk = m3_frnn_chunks(N1);
    hipLaunchKernelGGL(k_frnn_count, dim3(nchunk, P), dim3(kThreads), 0, st, (const int32_t *)map1, chunk_ws, N1, nchunk);
    hipLaunchKernelGGL(k_frnn_emit, dim3(nchunk, P), dim3(kThreads), 0, st, (const int32_t *)map1, (const int32_t *)chunk_ws, pairs,
                       count, N1, nchunk, S);
    M3_CHECK_LAUNCH("m3_frnn_collect");
    return M3_OK;
}

}  // extern "C"
