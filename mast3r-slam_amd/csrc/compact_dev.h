// Ordered stream compaction for the map kernels (map_export.hip, mesh.hip): count kept items per workgroup -> exclusive
// scan of the counts -> scatter at offset + rank.  Output positions come from the scan, never from an atomic counter,
// so the order is the source order and the bytes are the same on every call.
#pragma once
#include "map_points.h"     // kThreads, kPts; a file that wants the exporter's contraction includes it first, its own way

namespace {

constexpr int kScanThreads = 1024;
constexpr int kHdrWords = 4;                  // ws words in front of the counts: [0], [1] the totals of scan jobs 0, 1 (the
                                              // voxel pass: [1] points dropped by the voxel key), [2..3] unused

// Lanes of this wave below the caller's whose bit is set in the ballot b.
__device__ __forceinline__ int lanes_before(unsigned long long b) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
}

// Position of this thread's first kept point among the workgroup's kept points (source order: thread, then bit), and the
// workgroup's total.  keep: bit j = point j of this thread is kept.
__device__ __forceinline__ int block_prefix(unsigned keep, int &total) {
    __shared__ int wsum[kThreads / M3_WAVE];
    int before = 0, wtot = 0;
#pragma unroll
    for (int j = 0; j < kPts; ++j) {
        const unsigned long long b = __ballot((keep >> j) & 1u);
        before += lanes_before(b);
        wtot += __popcll(b);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) wsum[w] = wtot;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < kThreads / M3_WAVE; ++i) {
        base += i < w ? wsum[i] : 0;
        total += wsum[i];
    }
    return base + before;
}

struct ScanJob {
    int32_t *cnt;                             // counts in, exclusive prefix sums out
    int64_t n;
};

// Exclusive scan in place, one workgroup per job, in rounds of kScanThreads * 4 counts (shuffle scan per wave, wave
// totals through LDS): workgroup i scans job i and writes its total to hdr[i].
__global__ void __launch_bounds__(kScanThreads) k_scan_counts(ScanJob job0, ScanJob job1, int32_t *__restrict__ hdr) {
    __shared__ int wsum[kScanThreads / M3_WAVE];
    int32_t *cnt = blockIdx.x ? job1.cnt : job0.cnt;
    const int64_t B = blockIdx.x ? job1.n : job0.n;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int carry = 0;
    for (int64_t i0 = 0; i0 < B; i0 += kScanThreads * 4) {
        const int64_t i = i0 + threadIdx.x * 4;
        int v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = i + j < B ? cnt[i + j] : 0;
        const int mine = (v[0] + v[1]) + (v[2] + v[3]);
        int incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        int base = carry, all = 0;
#pragma unroll
        for (int ww = 0; ww < kScanThreads / M3_WAVE; ++ww) {
            base += ww < w ? wsum[ww] : 0;
            all += wsum[ww];
        }
        int run = base + incl - mine;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i + j < B) cnt[i + j] = run;
            run += v[j];
        }
        carry += all;
        __syncthreads();                               // wsum is rewritten by the next round
    }
    if (threadIdx.x == 0) hdr[blockIdx.x] = carry;
}

// One launch: a scans into hdr[0] and, when given, b into hdr[1].
inline void launch_scan(hipStream_t st, int32_t *hdr, ScanJob a, ScanJob b = ScanJob{nullptr, 0}) {
    hipLaunchKernelGGL(k_scan_counts, dim3(b.cnt ? 2 : 1), dim3(kScanThreads), 0, st, a, b, hdr);
}

}  // namespace
