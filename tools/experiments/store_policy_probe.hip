// Probe: what does a kernel's closing burst of output stores cost at the boundary to the next, dependent kernel - and does a
// write-through (sc1) store, which leaves no dirty line in the XCD's L2, return any of it?  (profiles/store_policy.md)
//
// A hipGraph of 16 dependent launches, 256 workgroups of 512 threads.  Each launch reads 8 KB per workgroup of what its
// predecessor wrote (another workgroup's slab), spins ~40 us on the wall clock as a one-round GEMM's K loop would, then writes
// B bytes in one burst: 16 (or 8) bytes per lane, consecutive lanes consecutive addresses, i.e. full 128-byte lines.
// Store forms: 0 plain 16 B, 1 sc1 16 B (buffer store, aux 16), 2 sc1 8 B, 3 plain 8 B (the control for 2), 4 the buffer store
// of form 1 without sc1 (the control for 1: same instruction and addressing, only the cache policy differs).
// Prints us per launch (median and spread of the repeats) per form and B; B = 0 is the launch without the burst.
//
// hipcc -O3 --offload-arch=gfx950 tools/experiments/store_policy_probe.hip -o tools/experiments/_build/store_policy_probe
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int kWgs = 256, kThreads = 512, kLaunches = 16, kForms = 5;

// prev / out: buffers of `bytes` (a multiple of kWgs * kThreads * 16); workgroup w owns the slab [w * bytes / kWgs, + bytes / kWgs)
template <int FORM>
__global__ __launch_bounds__(kThreads) void k_burst(const uint4 *prev, unsigned char *out, unsigned slab_bytes, unsigned read_slab_bytes,
                                                    long long spin_ticks) {
    const int tid = threadIdx.x, wg = blockIdx.x;
    // 8 KB of the predecessor's output, from the slab of a workgroup elsewhere on the chip (read_slab_bytes >= 8 KB, host check)
    const int src = (wg * 37 + 11) % kWgs;
    const uint4 in = prev[((size_t)src * read_slab_bytes >> 4) + tid];
    unsigned seed = in.x ^ in.y ^ in.z ^ in.w;
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < spin_ticks) seed = seed * 1664525u + 1013904223u;
    asm volatile("" ::: "memory");
    unsigned char *slab = out + (size_t)wg * slab_bytes;
    if (FORM == 0) {
        for (unsigned o = tid * 16u; o < slab_bytes; o += kThreads * 16u)
            *reinterpret_cast<u32x4 *>(slab + o) = u32x4{seed, o, seed ^ o, (unsigned)wg};   // (as uint4 hipcc split it into dwords)
    } else if (FORM == 1) {
        const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(slab, 0, 0x7ffffff0, 0x00020000);
        for (unsigned o = tid * 16u; o < slab_bytes; o += kThreads * 16u)
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{seed, o, seed ^ o, (unsigned)wg}, r, o, 0, /*aux: sc1*/ 16);
    } else if (FORM == 2) {
        const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(slab, 0, 0x7ffffff0, 0x00020000);
        for (unsigned o = tid * 8u; o < slab_bytes; o += kThreads * 8u)
            __builtin_amdgcn_raw_buffer_store_b64(u32x2{seed, o}, r, o, 0, /*aux: sc1*/ 16);
    } else if (FORM == 3) {
        for (unsigned o = tid * 8u; o < slab_bytes; o += kThreads * 8u)
            *reinterpret_cast<u32x2 *>(slab + o) = u32x2{seed, o};
    } else {
        const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(slab, 0, 0x7ffffff0, 0x00020000);
        for (unsigned o = tid * 16u; o < slab_bytes; o += kThreads * 16u)
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{seed, o, seed ^ o, (unsigned)wg}, r, o, 0, 0);
    }
}

typedef void (*kern_t)(const uint4 *, unsigned char *, unsigned, unsigned, long long);

int main(int argc, char **argv) {
    const int repeats = argc > 1 ? atoi(argv[1]) : 7, replays = 5;
    const long long spin_ticks = argc > 2 ? atoll(argv[2]) : 4000;          // wall clock: 100 MHz -> 40 us
    const size_t MB = 1u << 20, sizes[] = {0, 8 * MB, 32 * MB, 64 * MB, 128 * MB};
    const size_t cap = 128 * MB;
    const kern_t kern[kForms] = {k_burst<0>, k_burst<1>, k_burst<2>, k_burst<3>, k_burst<4>};
    const char *names[kForms] = {"plain 16 B", "sc1 16 B", "sc1 8 B", "plain 8 B", "plain 16 B, buffer store"};
    unsigned char *buf[2];
    CK(hipMalloc(&buf[0], cap)); CK(hipMalloc(&buf[1], cap));
    CK(hipMemset(buf[0], 0, cap)); CK(hipMemset(buf[1], 0, cap));
    hipStream_t s; CK(hipStreamCreate(&s));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    printf("| B | form | us per launch, median | spread (max - min) | repeats |\n|---|---|---|---|---|\n");
    for (size_t bytes : sizes) {
        const unsigned slab = (unsigned)(bytes / kWgs);                      // 0 .. 512 KB: a multiple of kThreads * 16 or zero
        if (slab % (kThreads * 16) != 0) { fprintf(stderr, "slab %u is not a whole number of store rounds\n", slab); return 1; }
        const unsigned read_slab = (unsigned)((bytes ? bytes : 8 * MB) / kWgs);   // B = 0: read inside the first 8 MB (zeros or stale)
        if (read_slab < kThreads * 16 || (size_t)read_slab * kWgs > cap) { fprintf(stderr, "bad read slab\n"); return 1; }
        hipGraphExec_t exec[kForms];
        for (int f = 0; f < kForms; ++f) {
            hipGraph_t g;
            CK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            for (int l = 0; l < kLaunches; ++l)
                hipLaunchKernelGGL(kern[f], dim3(kWgs), dim3(kThreads), 0, s, reinterpret_cast<const uint4 *>(buf[(l + 1) & 1]), buf[l & 1],
                                   slab, read_slab, spin_ticks);
            CK(hipStreamEndCapture(s, &g));
            CK(hipGraphInstantiate(&exec[f], g, nullptr, nullptr, 0));
            CK(hipGraphDestroy(g));
            CK(hipGraphLaunch(exec[f], s)); CK(hipStreamSynchronize(s));    // warm
        }
        std::vector<float> us[kForms];
        for (int rep = 0; rep < repeats; ++rep)
            for (int f = 0; f < kForms; ++f) {                                    // forms interleaved inside a repeat
                CK(hipEventRecord(e0, s));
                for (int i = 0; i < replays; ++i) CK(hipGraphLaunch(exec[f], s));
                CK(hipEventRecord(e1, s)); CK(hipEventSynchronize(e1));
                float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                us[f].push_back(ms * 1e3f / (replays * kLaunches));
            }
        for (int f = 0; f < kForms; ++f) {
            std::sort(us[f].begin(), us[f].end());
            printf("| %zu MB | %s | %.2f | %.2f |", bytes / MB, names[f], us[f][us[f].size() / 2], us[f].back() - us[f].front());
            for (float v : us[f]) printf(" %.2f", v);
            printf(" |\n");
            CK(hipGraphExecDestroy(exec[f]));
        }
        fflush(stdout);
    }
    // the last graph (16 B, 128 MB) left (seed, o, seed ^ o, wg) in slab 0, o the byte offset: bytes 16..31 hold offset 16 and wg 0
    unsigned h[4]; CK(hipMemcpy(h, buf[1] + 16, 16, hipMemcpyDeviceToHost));
    printf("check: read back offset %u, workgroup %u (expected 16 0)\n", h[1], h[3]);
    CK(hipFree(buf[0])); CK(hipFree(buf[1]));
    return 0;
}
