// Frame preprocessing (mast3r_slam/preprocess.py): 8-bit separable resample of an interleaved RGB image followed by a
// crop, bit for bit the arithmetic of Pillow's Image.resize on host-built fixed-point coefficient tables.  One launch:
// a workgroup owns 64 columns x TH rows of the cropped output, stages the source rows its vertical taps need through
// LDS with 16-byte loads, writes their horizontally filtered uint8 rows to LDS and runs the vertical pass out of LDS.
// Every table entry that becomes an address is clamped first, so tables that do not belong to the sizes cannot make a
// load or store leave its buffer (the result is then meaningless, not unsafe).
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / M3_WAVE;
constexpr int kTW = 64;                       // output columns per workgroup: one per lane in the horizontal pass
constexpr int kInterPitch = kTW * 3;          // bytes per intermediate row (192 = 48 dwords)
constexpr int kBits = 22;                     // fixed-point position of the coefficients (Pillow's PRECISION_BITS)
constexpr int kLdsBudget = 64 * 1024;         // dynamic LDS available without a per-device opt-in
constexpr int kCoefLdsMax = 16 * 1024;        // horizontal coefficients of a tile are kept in LDS up to this size

struct ResizeParams {
    const uint8_t *src;
    const int32_t *bounds_h, *coef_h, *bounds_v, *coef_v;   // bounds NULL = no pass on that axis
    uint8_t *dst;
    float *img;
    int64_t src_bytes;
    int Hs, Ws, Wr, ksize_h, ksize_v;
    int cx0, cy0, Hc, Wc;
    int TH, rows_cap, span_cap, pitch;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ unsigned clip8(int acc) { return (unsigned)clampi(acc >> kBits, 0, 255); }

// R: source rows per wave in one staging round (4 R rows per round); KLDS: the tile's horizontal coefficients are
// copied to LDS once (tap-major, [ksize_h][64]) instead of being read from the global table at every tap.
template <int R, bool KLDS>
__global__ void __launch_bounds__(kThreads) k_resize_crop(const ResizeParams p) {
    extern __shared__ __align__(16) unsigned char lds[];
    unsigned char *inter = lds;                                          // [rows_cap][192]
    unsigned char *stage = lds + (size_t)p.rows_cap * kInterPitch;       // [4 R][pitch]
    int32_t *kl = (int32_t *)(stage + (size_t)kWaves * R * p.pitch);     // [ksize_h][64] when KLDS

    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.z, tx0 = blockIdx.x * kTW, ty0 = blockIdx.y * p.TH;
    const int ncols = min(kTW, p.Wc - tx0), nout = min(p.TH, p.Hc - ty0);
    const bool has_h = p.bounds_h != nullptr, has_v = p.bounds_v != nullptr;

    // source rows [y_lo, y_lo + nrows) feed this tile's output rows (the tables are monotone)
    int y_lo, nrows;
    if (has_v) {
        const int first = p.cy0 + ty0, last = first + nout - 1;
        y_lo = clampi(p.bounds_v[2 * first], 0, p.Hs);
        const int y_l = clampi(p.bounds_v[2 * last], 0, p.Hs);
        nrows = min(y_l + clampi(p.bounds_v[2 * last + 1], 0, p.ksize_v), p.Hs) - y_lo;
    } else {
        y_lo = p.cy0 + ty0;
        nrows = nout;
    }
    nrows = clampi(nrows, 0, min(p.rows_cap, p.Hs - y_lo));

    // this lane's column of the resized image and its taps; lanes past the tile repeat its last column
    const int col = p.cx0 + tx0 + min(lane, ncols - 1);
    int xmin = col, n = 1;
    if (has_h) {
        xmin = clampi(p.bounds_h[2 * col], 0, p.Ws);
        n = clampi(p.bounds_h[2 * col + 1], 0, min(p.ksize_h, p.Ws - xmin));
    }
    const int xs = __shfl(xmin, 0, 64);
    const int span = clampi(__shfl(xmin + n, ncols - 1, 64) - xs, 0, min(p.span_cap, p.Ws - xs));
    const int off = clampi(xmin - xs, 0, span);
    n = min(n, span - off);

    if (KLDS && has_h) {
        const int c0 = p.cx0 + tx0;
        for (int i = threadIdx.x; i < p.ksize_h * kTW; i += kThreads) {
            const int c = min(c0 + (i & 63), p.Wr - 1);
            kl[i] = p.coef_h[(size_t)(i >> 6) * p.Wr + c];
        }
    }

    // ---- horizontal pass: 4 R source rows per round, staged with 16-byte loads -------------------------------------
    for (int r0 = 0; r0 < nrows; r0 += kWaves * R) {
        __syncthreads();                                                 // the previous round's readers are done
        int shift[R];
#pragma unroll
        for (int rr = 0; rr < R; ++rr) {
            const int i = wv * R + rr, row = r0 + i;
            const int64_t g = (((int64_t)b * p.Hs + y_lo + min(row, nrows - 1)) * p.Ws + xs) * 3;
            shift[rr] = (int)(g & 15);
            if (row >= nrows) continue;
            const int64_t a0 = g - shift[rr];
            const int nvec = (shift[rr] + span * 3 + 15) >> 4;           // <= pitch / 16
            for (int v = lane; v < nvec; v += 64) {
                const int64_t o = a0 + 16 * (int64_t)v;
                uint4 val;
                if (o + 16 <= p.src_bytes) {
                    val = *(const uint4 *)(p.src + o);
                } else {                                                 // the vector that crosses the end of the source
                    unsigned w[4] = {0u, 0u, 0u, 0u};
                    for (int j = 0; j < 16; ++j)
                        if (o + j < p.src_bytes) w[j >> 2] |= (unsigned)p.src[o + j] << (8 * (j & 3));
                    val = make_uint4(w[0], w[1], w[2], w[3]);
                }
                *(uint4 *)(stage + (size_t)i * p.pitch + 16 * v) = val;
            }
        }
        __syncthreads();
        int acc[R][3];
        const unsigned char *sp[R];
#pragma unroll
        for (int rr = 0; rr < R; ++rr) {
            acc[rr][0] = acc[rr][1] = acc[rr][2] = 1 << (kBits - 1);
            sp[rr] = stage + (size_t)(wv * R + rr) * p.pitch + shift[rr] + off * 3;
        }
        for (int x = 0; x < n; ++x) {
            int kx = 1 << kBits;
            if (has_h) kx = KLDS ? kl[x * kTW + lane] : p.coef_h[(size_t)x * p.Wr + col];
#pragma unroll
            for (int rr = 0; rr < R; ++rr) {
                acc[rr][0] += __mul24(kx, (int)sp[rr][3 * x]);       // |k| < 2^23: the full-rate 24-bit multiply-add is exact
                acc[rr][1] += __mul24(kx, (int)sp[rr][3 * x + 1]);
                acc[rr][2] += __mul24(kx, (int)sp[rr][3 * x + 2]);
            }
        }
#pragma unroll
        for (int rr = 0; rr < R; ++rr) {
            const int row = r0 + wv * R + rr;
            if (row < nrows && lane < ncols) {
                unsigned char *q = inter + (size_t)row * kInterPitch + lane * 3;
                q[0] = (unsigned char)clip8(acc[rr][0]);
                q[1] = (unsigned char)clip8(acc[rr][1]);
                q[2] = (unsigned char)clip8(acc[rr][2]);
            }
        }
    }
    __syncthreads();

    // ---- vertical pass: a wave owns an output row (wave-uniform coefficients), a lane four bytes of it ------------
    const int nbytes = ncols * 3;
    for (int r = wv; r < nout; r += kWaves) {
        const int orow = p.cy0 + ty0 + r;
        int yoff = r, ny = 1;
        if (has_v) {
            yoff = clampi(clampi(p.bounds_v[2 * orow], 0, p.Hs) - y_lo, 0, nrows);
            ny = min(clampi(p.bounds_v[2 * orow + 1], 0, p.ksize_v), nrows - yoff);
        } else if (r >= nrows) {
            ny = 0;
        }
        const int bc = lane * 4;
        if (bc >= nbytes) continue;
        int acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = 1 << (kBits - 1);
        const int32_t *kv = has_v ? p.coef_v + (size_t)orow * p.ksize_v : nullptr;
        for (int y = 0; y < ny; ++y) {
            const int ky = has_v ? kv[y] : 1 << kBits;
            const unsigned wd = *(const unsigned *)(inter + (size_t)(yoff + y) * kInterPitch + bc);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += __mul24(ky, (int)((wd >> (8 * j)) & 255u));
        }
        unsigned o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = clip8(acc[j]);
        const int64_t d = (((int64_t)b * p.Hc + ty0 + r) * p.Wc + tx0) * 3 + bc;
        const bool wide = bc + 4 <= nbytes && (d & 3) == 0;
        if (wide) {
            *(unsigned *)(p.dst + d) = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (bc + j < nbytes) p.dst[d + j] = (unsigned char)o[j];
        }
        if (p.img) {
            float f[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) f[j] = ((float)o[j] / 255.0f - 0.5f) / 0.5f;      // three roundings, as numpy
            if (wide) {
                *(float4 *)(p.img + d) = make_float4(f[0], f[1], f[2], f[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (bc + j < nbytes) p.img[d + j] = f[j];
            }
        }
    }
}

struct ResizePlan {
    int TH, rows_cap, span_cap, pitch, R, klds;
    size_t lds;
};

// Rows per tile, staging depth and LDS bytes for one problem; false = no tiling fits the LDS budget.
inline bool resize_plan(int Hs, int Ws, int Hr, int Wr, int ksize_h, int ksize_v, int Hc, int Wc, int B, ResizePlan &pl) {
    const bool has_h = Wr != Ws, has_v = Hr != Hs;
    // source pixels under 64 neighbouring columns: < 63 * scale + 2 * support + 1 <= 63 * scale + ksize
    int64_t span = has_h ? (63 * (int64_t)Ws + Wr - 1) / Wr + ksize_h + 1 : kTW;
    if (span > Ws) span = Ws;
    pl.span_cap = (int)span;
    pl.pitch = (int)((span * 3 + 15 + 15) / 16 * 16);
    pl.klds = has_h && (int64_t)ksize_h * kTW * 4 <= kCoefLdsMax;
    const size_t coef = pl.klds ? (size_t)ksize_h * kTW * 4 : 0;
    const int tiles_x = m3_cdiv(Wc, kTW);
    for (int th = 16; th >= 1; th /= 2) {
        int64_t rows = has_v ? ((int64_t)(th - 1) * Hs + Hr - 1) / Hr + ksize_v + 1 : th;
        if (rows > Hs) rows = Hs;
        const size_t inter = (size_t)rows * kInterPitch;
        // halve the tile while the launch would leave most of the chip idle (256 CUs), down to 4 rows
        if (th > 4 && (int64_t)tiles_x * m3_cdiv(Hc, th) * B < 512) continue;
        for (int r = 4; r >= 1; r /= 2) {
            const size_t need = inter + (size_t)kWaves * r * pl.pitch + coef;
            if (need <= (size_t)kLdsBudget && (inter <= (size_t)kLdsBudget / 2 || th == 1)) {
                pl.TH = th; pl.rows_cap = (int)rows; pl.R = r; pl.lds = need;
                return true;
            }
        }
    }
    return false;
}

}  // namespace

extern "C" {

int m3_resize_crop_u8(const uint8_t *src, const int32_t *bounds_h, const int32_t *coef_h, int ksize_h,
                      const int32_t *bounds_v, const int32_t *coef_v, int ksize_v, uint8_t *dst, float *img, int B, int Hs,
                      int Ws, int Hr, int Wr, int crop_x0, int crop_y0, int Hc, int Wc, void *stream) {
    M3_REQUIRE(src && dst && B >= 1 && B <= 65535 && Hs >= 1 && Ws >= 1 && Hr >= 1 && Wr >= 1);
    M3_REQUIRE(Hs <= 65536 && Ws <= 65536 && Hr <= 65536 && Wr <= 65536);
    M3_REQUIRE(crop_x0 >= 0 && crop_y0 >= 0 && Wc >= 1 && Hc >= 1 && crop_x0 + (int64_t)Wc <= Wr && crop_y0 + (int64_t)Hc <= Hr);
    M3_REQUIRE(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0 && ((uintptr_t)img & 15) == 0);
    const bool has_h = Wr != Ws, has_v = Hr != Hs;
    M3_REQUIRE(!has_h || (bounds_h && coef_h && ksize_h >= 1 && ksize_h <= 65536));
    M3_REQUIRE(!has_v || (bounds_v && coef_v && ksize_v >= 1 && ksize_v <= 65536));
    ResizePlan pl;
    if (!resize_plan(Hs, Ws, Hr, Wr, has_h ? ksize_h : 1, has_v ? ksize_v : 1, Hc, Wc, B, pl)) return M3_ERR_UNSUPPORTED;
    const int tiles_y = m3_cdiv(Hc, pl.TH);
    if (tiles_y > 65535) return M3_ERR_UNSUPPORTED;
    ResizeParams p;
    p.src = src;
    p.bounds_h = has_h ? bounds_h : nullptr; p.coef_h = has_h ? coef_h : nullptr;
    p.bounds_v = has_v ? bounds_v : nullptr; p.coef_v = has_v ? coef_v : nullptr;
    p.dst = dst; p.img = img;
    p.src_bytes = (int64_t)B * Hs * Ws * 3;
    p.Hs = Hs; p.Ws = Ws; p.Wr = Wr; p.ksize_h = has_h ? ksize_h : 1; p.ksize_v = has_v ? ksize_v : 1;
    p.cx0 = crop_x0; p.cy0 = crop_y0; p.Hc = Hc; p.Wc = Wc;
    p.TH = pl.TH; p.rows_cap = pl.rows_cap; p.span_cap = pl.span_cap; p.pitch = pl.pitch;
    const dim3 grid(m3_cdiv(Wc, kTW), tiles_y, B), block(kThreads);
    hipStream_t st = (hipStream_t)stream;
#define M3_RC_LAUNCH(R_, K_) hipLaunchKernelGGL((k_resize_crop<R_, K_>), grid, block, pl.lds, st, p)
    if (pl.klds) {
        if (pl.R == 4) M3_RC_LAUNCH(4, true); else if (pl.R == 2) M3_RC_LAUNCH(2, true); else M3_RC_LAUNCH(1, true);
    } else {
        if (pl.R == 4) M3_RC_LAUNCH(4, false); else if (pl.R == 2) M3_RC_LAUNCH(2, false); else M3_RC_LAUNCH(1, false);
    }
#undef M3_RC_LAUNCH
    M3_CHECK_LAUNCH("m3_resize_crop_u8");
    return M3_OK;
}

}  // extern "C"
