// scale.hip -- libisxscale.so (include/isx_scale.h): the integer cubic resize of uint8 RGB images through a virtual noise-padded source, the
// device half of pre_process_dataset.py and of the second scale of train.classif_regions.
//
// One launch, isxs_resize_cubic_u8: grid (column tiles, row tiles, B), 256 threads; a workgroup produces one tile of kTileH x kTileW = 8 x 128
// pixels of dst for one image, in four steps:
//
//   tables   threads 0..127 derive the taps and coefficients of the tile's columns, threads 128..135 those of its rows: the int64 arithmetic
//            of the header, four floor divisions per axis index -- per column and per row of a tile, never per pixel -- into LDS.  A floor
//            division is one fp64 division whose quotient is then made exact on the integers.
//   stage    taps grow monotonically along an axis, so the tile reads the source rectangle [tap 0 of its first row/column, tap 3 of its
//            last]: the FOOTPRINT.  Where it has at most kFootPixels pixels (an 8 x 128 tile at 2:1 needs 19 x 260 = 4 940, at 2.41:1
//            23 x 312 = 7 176) it is staged in LDS as one dword R | G << 8 | B << 16 per pixel.  A footprint row that lies in the image is
//            contiguous in src: a lane takes a group of four pixels -- 12 bytes at any alignment -- as the four aligned dwords that hold
//            them (one global_load_dwordx4, consecutive lanes 12 bytes apart, four groups in flight per lane), shifts the bytes into place
//            and writes the four pixel dwords with one ds_write_b128.  Rows that touch the padding are filled pixel by pixel: their noise
//            bytes are computed here, once per footprint pixel.  A larger footprint (a reduction beyond about 3.5:1; 100:1 works the same)
//            is not staged: the taps then read the source -- or compute the noise -- directly, and neighbouring pixels share cache lines.
//            The LDS budget does not depend on the scale ratio.
//   cubic    a thread owns one column and four rows of the tile (its column's taps and coefficients stay in registers): per pixel 16 taps,
//            one aligned ds_read_b32 each, 60 multiply-adds with 24-bit factors (v_mad_i32_i24: the 32-bit multiply runs at a quarter of
//            its rate) into 32-bit sums, then round, shift and clip, and 3 bytes into the LDS image of the tile.
//   store    dst rows are 3 Wd bytes at any alignment.  A tile row is laid out in LDS at the offset its global address has inside a 16-byte
//            line, so piece p of a row is 16-byte aligned in both memories: one ds_read_b128 and one 16-byte global store per lane,
//            consecutive lanes consecutive pieces; the pieces that hang over the ends of the row segment (at most two per row) are
//            written byte by byte.  Nothing outside the segment is read or written.
//
// Exactness: every term is an integer, |sum of coefficients| <= 2818 per axis, so any partial sum is below 255 x 2818^2 + 2^21 < 2^31.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/isx_scale.h"

#define ISXS_API extern "C" __attribute__((visibility("default")))

static thread_local char g_err[256] = "";

static int fail(int rc, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return rc;
}

ISXS_API const char* isxs_last_error(void) { return g_err; }
ISXS_API int isxs_version(void) { return 100; }

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 128, kTileH = 8;         // pixels of dst per workgroup
constexpr int kRowsPerThread = kTileH / (kThreads / kTileW);
constexpr int kFootPixels = 7680;                // staged footprint, 4 bytes per pixel: 30 KiB of LDS, four workgroups per CU
constexpr int kOutStride = 3 * kTileW + 16;     // bytes per tile row of the output image in LDS: the row plus its offset in a 16-byte line
constexpr int kPieces = kOutStride / 16;        // 16-byte pieces per tile row

struct Geometry {
    int Hs, Ws, top, left, Hp, Wp, Hd, Wd;
};

// floor(a / b) for b > 0 and a quotient below 2^31 in size: the quotient comes from one fp64 division (off by at most one: a has 53 exact bits
// of at most 63, the quotient 31) and is made exact on the integers.  An int64 division proper is a few hundred quarter-rate instructions.
__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b) {
    int64_t q = (int64_t)floor((double)a / (double)b);
    const int64_t rem = a - q * b;
    if (rem < 0) --q;
    else if (rem >= b) ++q;
    return q;
}

// Taps and coefficients of output index j on an axis of source length S and output length T (header).  D = 2 T <= 2^15 and r, D - r < D, so
// squares fit 32 bits and cubes 45: the products are 32 x 32 -> 64 bit multiplies, not 64 x 64.
__device__ void axis_taps(int j, int S, int T, int* tap, int* coef) {
    const uint32_t D = 2u * (uint32_t)T;
    const int64_t num = (2 * (int64_t)j + 1) * S - T;                        // |num| < 2^31
    const int64_t s = floor_div(num, (int64_t)D);
    const uint32_t r = (uint32_t)(num - s * (int64_t)D), q = D - r;
    const uint64_t D3 = (uint64_t)(D * D) * D;
    const uint32_t rr = r * r, qq = q * q;
    const int64_t n0 = -1536 * (int64_t)((uint64_t)qq * r);
    const int64_t n1 = (int64_t)(2560 * ((uint64_t)rr * r) + 2048 * D3) - (int64_t)(4608 * ((uint64_t)rr * D));
    const int64_t n2 = (int64_t)(2560 * ((uint64_t)qq * q) + 2048 * D3) - (int64_t)(4608 * ((uint64_t)qq * D));
    const int c0 = (int)floor_div(2 * n0 + (int64_t)D3, 2 * (int64_t)D3);
    const int c1 = (int)floor_div(2 * n1 + (int64_t)D3, 2 * (int64_t)D3);
    const int c2 = (int)floor_div(2 * n2 + (int64_t)D3, 2 * (int64_t)D3);
    coef[0] = c0; coef[1] = c1; coef[2] = c2; coef[3] = 2048 - c0 - c1 - c2;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t i = s - 1 + k;
        tap[k] = (int)(i < 0 ? 0 : i > S - 1 ? S - 1 : i);
    }
}

__device__ __forceinline__ uint32_t noise_byte(uint64_t seed, uint64_t counter) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * counter;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (uint32_t)(z >> 56);
}

// Pixel (y, x) of the padded image, 0 <= y < Hp, 0 <= x < Wp, as R | G << 8 | B << 16.  img: this image's (Hs, Ws, 3) bytes.
__device__ __forceinline__ uint32_t padded_pixel(const uint8_t* __restrict__ img, const Geometry& g, uint64_t seed, uint64_t noise_base, int y, int x) {
    const int ys = y - g.top, xs = x - g.left;
    if ((unsigned)ys < (unsigned)g.Hs && (unsigned)xs < (unsigned)g.Ws) {
        const uint8_t* p = img + ((int64_t)ys * g.Ws + xs) * 3;
        return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    }
    const uint64_t counter = noise_base + 3ull * (uint64_t)((int64_t)y * g.Wp + x);
    return noise_byte(seed, counter) | noise_byte(seed, counter + 1) << 8 | noise_byte(seed, counter + 2) << 16;
}

struct __attribute__((aligned(4))) Dwords4 {     // 16 bytes at a 4-byte boundary: one global_load_dwordx4
    uint32_t v[4];
};

// Bytes sh .. sh + 3 of the 8 bytes lo, hi (little endian), sh = 0..3.
__device__ __forceinline__ uint32_t shifted(uint32_t lo, uint32_t hi, int sh) { return (uint32_t)(((uint64_t)hi << 32 | lo) >> (8 * sh)); }

// Both factors fit 24 signed bits (coefficients, bytes, row sums): the full-rate 24-bit multiply; a 32-bit one runs at a quarter of the rate.
__device__ __forceinline__ int mul24(int a, int b) { return __mul24(a, b); }

__device__ __forceinline__ uint32_t round_clip(int acc) {
    const int v = (acc + (1 << 21)) >> 22;
    return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

__global__ __launch_bounds__(kThreads) void resize_cubic_kernel(const uint8_t* __restrict__ src, Geometry g, uint64_t seed,
                                                                const int64_t* __restrict__ noise_ids, uint8_t* __restrict__ dst) {
    __shared__ int s_tx[kTileW][4], s_cx[kTileW][4], s_ty[kTileH][4], s_cy[kTileH][4], s_line[kTileH][4];
    __shared__ __attribute__((aligned(16))) uint32_t s_foot[kFootPixels];
    __shared__ __attribute__((aligned(16))) uint8_t s_out[kTileH * kOutStride];

    const int t = threadIdx.x;
    const int x0 = (int)blockIdx.x * kTileW, y0 = (int)blockIdx.y * kTileH;
    const int64_t b = blockIdx.z;
    const int ncol = g.Wd - x0 < kTileW ? g.Wd - x0 : kTileW;               // >= 1 by the grid
    const int nrow = g.Hd - y0 < kTileH ? g.Hd - y0 : kTileH;
    const uint8_t* img = src + b * (3 * (int64_t)g.Hs * g.Ws);
    uint8_t* out = dst + b * (3 * (int64_t)g.Hd * g.Wd);
    const uint64_t noise_base = noise_ids ? (uint64_t)noise_ids[b] * (3ull * (uint64_t)g.Hp * (uint64_t)g.Wp) : 0;   // null: nothing is padded

    // ---- tables: a dead column or row of the last tile repeats the last live one, so every tap in LDS is in range ----
    if (t < kTileW) {
        axis_taps(x0 + (t < ncol ? t : ncol - 1), g.Wp, g.Wd, s_tx[t], s_cx[t]);
    } else if (t < kTileW + kTileH) {
        const int r = t - kTileW;
        axis_taps(y0 + (r < nrow ? r : nrow - 1), g.Hp, g.Hd, s_ty[r], s_cy[r]);
    }
    __syncthreads();
    const int x_lo = s_tx[0][0], y_lo = s_ty[0][0];
    const int fw = s_tx[ncol - 1][3] - x_lo + 1, fh = s_ty[nrow - 1][3] - y_lo + 1;
    const int fwp = (fw + 3) & ~3;                                           // pixels per staged row: whole groups of four
    const bool staged = (int64_t)fwp * fh <= kFootPixels;                    // the same in every thread
    // A footprint row that lies in the image (not in the padding) is 3 fw contiguous bytes of src: a PLAIN row.
    const bool cols_inside = x_lo >= g.left && x_lo + fw <= g.left + g.Ws;
    auto plain_row = [&](int y) { return cols_inside && y >= g.top && y < g.top + g.Hs; };

    // ---- stage ----
    if (staged) {
        if (t < 4 * kTileH) s_line[t >> 2][t & 3] = (s_ty[t >> 2][t & 3] - y_lo) * fwp;      // where tap row i of tile row r starts
        const int gpr = fwp / 4, total = fh * gpr;                           // groups of 4 pixels = 12 source bytes = one 16-byte LDS store
        const uint8_t* const all_lo = src;
        const uint8_t* const all_hi = src + (int64_t)gridDim.z * (3 * (int64_t)g.Hs * g.Ws);
        for (int i0 = t; i0 < total; i0 += 4 * kThreads) {
            uint4 v[4];
            int at[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {                                    // four independent 16-byte loads in flight per lane
                const int i = i0 + u * kThreads;
                v[u] = make_uint4(0u, 0u, 0u, 0u);
                at[u] = -1;
                if (i < total) {
                    const int r = i / gpr, q = i - r * gpr, y = y_lo + r;
                    if (plain_row(y)) {
                        at[u] = r * fwp + 4 * q;
                        const uint8_t* a = img + ((int64_t)(y - g.top) * g.Ws + (x_lo - g.left + 4 * q)) * 3;     // the group's 12 bytes
                        const int sh = (int)((uintptr_t)a & 3);
                        const uint8_t* w = a - sh;                           // the four aligned dwords that hold them
                        if (w >= all_lo && w + 16 <= all_hi) {               // inside src (a last group runs on into the next row or image)
                            const Dwords4 d = *reinterpret_cast<const Dwords4*>(w);
                            const uint32_t b0 = shifted(d.v[0], d.v[1], sh), b1 = shifted(d.v[1], d.v[2], sh), b2 = shifted(d.v[2], d.v[3], sh);
                            v[u] = make_uint4(b0 & 0xFFFFFFu, b0 >> 24 | (b1 & 0xFFFFu) << 8, b1 >> 16 | (b2 & 0xFFu) << 16, b2 >> 8);
                        } else {                                             // the first or last dwords of the whole batch: pixel by pixel
                            uint32_t px[4] = {0u, 0u, 0u, 0u};
                            for (int k = 0; k < 4; ++k)
                                if (4 * q + k < fw) px[k] = padded_pixel(img, g, seed, noise_base, y, x_lo + 4 * q + k);
                            v[u] = make_uint4(px[0], px[1], px[2], px[3]);
                        }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (at[u] >= 0) *reinterpret_cast<uint4*>(s_foot + at[u]) = v[u];
        }
        for (int r = t >> 6; r < fh; r += kThreads / 64) {                   // rows that touch the padding: pixel by pixel, the noise computed here
            const int y = y_lo + r;
            if (plain_row(y)) continue;
            for (int x = t & 63; x < fw; x += 64) s_foot[r * fwp + x] = padded_pixel(img, g, seed, noise_base, y, x_lo + x);
        }
        __syncthreads();
    }

    // ---- cubic ----
    const int col = t & (kTileW - 1), row0 = t / kTileW;
    if (col < ncol) {
        int tx[4], cx[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            tx[k] = s_tx[col][k];
            cx[k] = s_cx[col][k];
        }
#pragma unroll
        for (int m = 0; m < kRowsPerThread; ++m) {
            const int r = row0 + m * (kThreads / kTileW);
            if (r >= nrow) break;
            int acc[3] = {0, 0, 0};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int y = s_ty[r][i], cy = s_cy[r][i];
                int h[3] = {0, 0, 0};
                const int line = staged ? s_line[r][i] - x_lo : 0;          // line + tap = (y - y_lo) fwp + (tap - x_lo) < fh fwp
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t px = staged ? s_foot[line + tx[k]] : padded_pixel(img, g, seed, noise_base, y, tx[k]);
                    h[0] += mul24(cx[k], (int)(px & 255u));
                    h[1] += mul24(cx[k], (int)((px >> 8) & 255u));
                    h[2] += mul24(cx[k], (int)((px >> 16) & 255u));
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] += mul24(cy, h[c]);              // |h| <= 255 x 2818 < 2^23
            }
            const int mis = (int)((uintptr_t)(out + ((int64_t)(y0 + r) * g.Wd + x0) * 3) & 15);
            uint8_t* o = s_out + r * kOutStride + mis + 3 * col;            // mis + 3 col + 2 <= 15 + 383 < kOutStride
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = (uint8_t)round_clip(acc[c]);
        }
    }
    __syncthreads();

    // ---- store: one 16-byte piece per thread ----
    if (t < kTileH * kPieces) {
        const int r = t / kPieces, p = t - r * kPieces;
        if (r < nrow) {
            uint8_t* row = out + ((int64_t)(y0 + r) * g.Wd + x0) * 3;       // the row segment: 3 ncol bytes
            const int mis = (int)((uintptr_t)row & 15);
            const int len = 3 * ncol;
            const int at = 16 * p - mis;                                    // the piece covers bytes [at, at + 16) of the segment
            const uint8_t* from = s_out + r * kOutStride + 16 * p;
            if (at >= 0 && at + 16 <= len) {
                *reinterpret_cast<uint4*>(row + at) = *reinterpret_cast<const uint4*>(from);
            } else {
                const int lo = at < 0 ? 0 : at, hi = at + 16 < len ? at + 16 : len;
                for (int i = lo; i < hi; ++i) row[i] = from[i - at];
            }
        }
    }
}

}  // namespace

ISXS_API int isxs_resize_cubic_u8(const uint8_t* src, int64_t B, int Hs, int Ws, int top, int left, int Hp, int Wp, uint64_t seed,
                                  const int64_t* noise_ids, uint8_t* dst, int Hd, int Wd, isxs_stream_t stream) {
    if (Hs < 1 || Ws < 1 || Hp < 1 || Wp < 1 || Hd < 1 || Wd < 1 || B < 0 || B > 65535 || top < 0 || left < 0 || (int64_t)top + Hs > Hp ||
        (int64_t)left + Ws > Wp)
        return fail(ISXS_ERR_ARG, "isxs_resize_cubic_u8: bad shape B=%lld src=%dx%d at (%d,%d) of %dx%d -> %dx%d (sides >= 1, 0 <= B <= 65535, "
                    "top + Hs <= Hp, left + Ws <= Wp)", (long long)B, Hs, Ws, top, left, Hp, Wp, Hd, Wd);
    if (Hd > 16384 || Wd > 16384 || Hp > 32768 || Wp > 32768 || 3 * (int64_t)Hp * Wp >= (1ll << 31) || 3 * (int64_t)Hd * Wd >= (1ll << 31))
        return fail(ISXS_ERR_ARG, "isxs_resize_cubic_u8: image too large: %dx%d -> %dx%d, needs Hd, Wd <= 16384, Hp, Wp <= 32768, 3 Hp Wp < 2^31 "
                    "and 3 Hd Wd < 2^31", Hp, Wp, Hd, Wd);
    if (B == 0) return ISXS_OK;
    const bool padded = top != 0 || left != 0 || Hp != Hs || Wp != Ws;
    if (!src || !dst || (padded && !noise_ids)) return fail(ISXS_ERR_ARG, "isxs_resize_cubic_u8: null pointer (src, dst, noise_ids when padded)");
    if ((uintptr_t)noise_ids % 8) return fail(ISXS_ERR_ARG, "isxs_resize_cubic_u8: noise_ids must be 8-B aligned");
    const Geometry g = {Hs, Ws, top, left, Hp, Wp, Hd, Wd};
    const dim3 grid((unsigned)((Wd + kTileW - 1) / kTileW), (unsigned)((Hd + kTileH - 1) / kTileH), (unsigned)B);
    hipLaunchKernelGGL(resize_cubic_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, src, g, seed, padded ? noise_ids : nullptr, dst);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ISXS_ERR_HIP, "isxs_resize_cubic_u8: launch failed: %s", hipGetErrorString(e));
    return ISXS_OK;
}
