// conv3x3_tile.hpp -- the implicit-GEMM main loop of the 3x3 convolution (shared by conv.hip and expand.hip).
#pragma once
#include "gemm_tile.hpp"

namespace isx {

// ---- 3x3 convolution (padding 1, stride 1 or 2) on NHWC activations as an IMPLICIT GEMM ----------------------
// Same tile machinery as cosine_gemm_kernel: M = B*Ho*Wo output pixels, N = Cout, K = 9*Cin ordered (kh, kw, ci),
// weights pre-arranged (Cout, 3, 3, Cin).  A k-tile lies inside one filter tap (Cin % BK == 0), so the A rows of a
// k-tile are the input pixels shifted by that tap: one base pixel per staged row, kept in registers, plus a
// bounds test per tap (padding rows load zeros -- fma(0, w, acc) leaves acc unchanged, as skipping the tap would; the position-major
// row order below does skip them).
// Epilogue: bias (+ residual) + ReLU fused, wave-uniform row pointers.  Replaces conv2 of the torchvision
// Bottleneck / both convolutions of BasicBlock inside the `features` trunk.
struct Conv3x3Geom { int H, W, Cin, Ho, Wo, stride, raster; };     // raster: position-major tiles in raster order (A/B, tests; read by POSMAJ kernels only)

// ---- position-major row order (inference, small maps: isx_conv3x3_nhwc picks it, conv.hip) -------------------------------------------
// In the pixel-major order a 128-row tile of a 7x7 map is 2.6 whole images: every tap is padding for SOME of its rows, so the padding
// MFMAs cannot be skipped -- 18.1 % of the (pixel, tap) pairs at 7x7 stride 1, 9.3 % at 14x14.  Here the output rows are numbered
//     v = ((grp * P + p) * 128 + i)        P = Ho * Wo, p = ho * Wo + wo, image b = 128 grp + i
// so a 128-row tile (and each 64-row tail tile) is ONE output position p of up to 128 images.  Tap validity is then one scalar per tile,
// and the k loop visits the valid taps only: a skipped tap costs no loads, no LDS stores, no barriers and no MFMAs.  The visited taps keep
// the (kh, kw, ci) order.  The image group is outermost: neighbouring tiles are neighbouring positions of the same images, which share taps
// in their XCD's L2.
// Same bits as the pixel-major order: Cin % kConvChunk == 0 is required, so a tap is a whole number of chunks of the two-level sum.  A
// padding chunk's chain is fma(0, w, +0) = +0 for every FINITE w, and tot -- which starts at +0 and can therefore never be -0 -- is
// unchanged by tot + (+0).  A NON-FINITE weight under a padding tap gives NaN in the pixel-major order (0 * inf) and is skipped here: the
// two orders agree on finite weights only (the oracle's tests use no others).
// Rows of a tile are H W Cin floats apart in x and P Cout floats apart in y: isx_conv3x3_nhwc admits the order only where 128 such rows
// stay inside the 32-bit offsets of a buffer descriptor.  Rows with b >= B load image B - 1 again and are not stored.
// LONGEST TILES FIRST: tiles are no longer equal -- an interior position runs nine taps, an edge six, a corner four -- and a launch that walks the
// positions in raster order ends on whatever comes last.  Within an image group, tile rank r (the p of the formula above) therefore maps to the
// position of rank r in descending order of visited taps: the interior positions, then the edges, then the corners, raster order inside each class
// (pos_major_position: closed form, no table).  Per axis index 0 always loses the tap before it; the last index loses the tap behind it where that tap
// lies outside the input (stride 1; stride 2 on an odd extent).  n x n outputs at stride 1: (n-2)^2, 4 (n-2), 4 positions; stride 2 on an even
// input: (n-1)^2, 2 (n-1), 1.  The launch's last tiles -- those the tail split cuts into 64-row tiles -- are then the cheapest positions of the last
// group.  Only WHICH workgroup computes a tile changes: no bit does.  g.raster (isx_debug_set_conv_cfg(10)) keeps the raster order.
__device__ __forceinline__ int pos_major_position(const Conv3x3Geom& g, int r) {
    if (g.raster) return r;
    const int sh = 1 + (g.Ho > 1 && (g.Ho - 1) * g.stride + 1 > g.H - 1), sw = 1 + (g.Wo > 1 && (g.Wo - 1) * g.stride + 1 > g.W - 1);      // short indices per axis: 0 (and the last)
    const int fh = g.Ho - sh, fw = g.Wo - sw;           // indices with all three taps: 1 .. fh, 1 .. fw
    int ho, wo;
    if (r < fh * fw) {                                  // interior
        ho = r / fw; wo = r - ho * fw;
        ++ho; ++wo;
    } else if ((r -= fh * fw) < sh * fw + fh * sw) {    // edges in raster order: row 0, the two (or one) ends of every full row, the last row
        if (r < fw) { ho = 0; wo = 1 + r; }
        else if ((r -= fw) < fh * sw) { ho = 1 + (r >> (sw - 1)); wo = (r & (sw - 1)) ? g.Wo - 1 : 0; }
        else { ho = g.Ho - 1; wo = 1 + r - fh * sw; }
    } else {                                            // corners
        r -= sh * fw + fh * sw;
        ho = (r >> (sw - 1)) ? g.Ho - 1 : 0; wo = (r & (sw - 1)) ? g.Wo - 1 : 0;
    }
    return ho * g.Wo + wo;
}
struct PosMajorTile { int B, b0, p, hi0, wi0, kh_lo, kh_n, kw_lo, kw_n; };
__device__ __forceinline__ PosMajorTile pos_major_tile(const Conv3x3Geom& g, int64_t M, int64_t m0) {
    PosMajorTile t;
    const int P = g.Ho * g.Wo, q = (int)(m0 >> 7), grp = q / P;
    t.B = (int)(M / P);
    // (readfirstlane: behind the branches of the mapping hipcc no longer takes p for wave-uniform and wraps the A loads of the k loop, whose SGPR
    // offset descends from it, into readfirstlane loops)
    t.p = __builtin_amdgcn_readfirstlane(pos_major_position(g, q - grp * P));
    t.b0 = grp * 128 + (int)(m0 & 127);
    const int ho = t.p / g.Wo, wo = t.p - ho * g.Wo;
    t.hi0 = ho * g.stride - 1;
    t.wi0 = wo * g.stride - 1;
    const int kh_hi = g.H - 1 - t.hi0 < 2 ? g.H - 1 - t.hi0 : 2, kw_hi = g.W - 1 - t.wi0 < 2 ? g.W - 1 - t.wi0 : 2;
    t.kh_lo = t.hi0 < 0 ? 1 : 0;
    t.kw_lo = t.wi0 < 0 ? 1 : 0;
    t.kh_n = kh_hi - t.kh_lo + 1;
    t.kw_n = kw_hi - t.kw_lo + 1;
    return t;
}

// accumulators of one (64 TM) x (64 TN) output tile at rows m0.., columns n0.. (every wave has left the LDS when this returns);
// lds: BK * (64 TM + 64 TN + 2 pads) floats
// AHEAD2 (64x64 tiles only): operands requested two k-tiles ahead instead of one (16 more VGPRs: the fused expand kernel has them, the plain
// 64x64 kernel at six workgroups per CU does not).
// CHUNK: terms per first-level chain of the two-level sum (gemm_tile.hpp; the inference trunk), 0 = one chain over all 9 Cin terms (gradients)
// POSMAJ: position-major row order (see the block above PosMajorTile); m0 is then a VIRTUAL row, M stays the real row count B * Ho * Wo
template <int TM, int TN, int BK, bool AHEAD2 = false, int CHUNK = kConvChunk, bool POSMAJ = false>
__device__ __forceinline__ void conv3x3_mainloop(float* __restrict__ lds, const float* __restrict__ x, int64_t M, const float* __restrict__ Wt, int64_t N,
                                                 const Conv3x3Geom& g, int64_t m0, int64_t n0, f32x16 (&acc)[TM][TN]) {
    constexpr int BM = 64 * TM, BN = 64 * TN, LDA = BM + lds_pad(BK), LDB = BN + lds_pad(BK);
    constexpr int CH = BK / 4, NA = BM * CH / 256;
    float* As = lds;
    float* Bs = lds + BK * LDA;
    const int D = 9 * g.Cin;
    static_assert(!POSMAJ || (!AHEAD2 && CHUNK != 0), "position-major rows: the plain staged loop of the inference kernels only");

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave / 2, wn = wave % 2;
    const int l31 = lane & 31, half = lane >> 5;

#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    f32x16 tot[CHUNK ? TM : 1][CHUNK ? TN : 1];
    zero_tiles(tot);

    // staged A rows of this thread: top-left input pixel of the 3x3 window (may be -1: padding)
    int pbase[NA], hw0[NA];                       // pixel index of (hi0, wi0); (hi0 + 1) << 16 | (wi0 + 1)
    const PosMajorTile pt = POSMAJ ? pos_major_tile(g, M, m0) : PosMajorTile{};
    const int kh_lo = POSMAJ ? pt.kh_lo : 0, kh_n = POSMAJ ? pt.kh_n : 3, kw_lo = POSMAJ ? pt.kw_lo : 0, kw_n = POSMAJ ? pt.kw_n : 3;    // taps the k loop visits
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const int idx = j * 256 + threadIdx.x;
        if constexpr (POSMAJ) {                   // one output position, image b0 + row (images past the batch repeat the last one: never stored)
            const int b = pt.b0 + idx / CH < pt.B ? pt.b0 + idx / CH : pt.B - 1;
            pbase[j] = (b * g.H + pt.hi0) * g.W + pt.wi0;
            hw0[j] = 0;
        } else {
            int64_t m = m0 + idx / CH;
            m = m < M ? m : M - 1;
            const int hw = g.Ho * g.Wo;
            const int b = (int)(m / hw), rem = (int)(m - (int64_t)b * hw);
            const int ho = rem / g.Wo, wo = rem - ho * g.Wo;
            const int hi0 = ho * g.stride - 1, wi0 = wo * g.stride - 1;
            pbase[j] = (b * g.H + hi0) * g.W + wi0;
            hw0[j] = ((hi0 + 1) << 16) | (wi0 + 1);
        }
    }
    const int c4 = (threadIdx.x % CH) << 2;
    int kh = kh_lo, kw = kw_lo, ci0 = 0;          // tap / channel offset of the NEXT k-tile to load (uniform)
    float4 ra[NA], rb[BN * BK / 1024];
    // A rows come through BUFFER loads: a wave-uniform descriptor that starts at the first input pixel this tile can touch, one 32-bit
    // byte offset per staged row (recomputed once per filter tap), the channel offset inside the tap as the SGPR offset.  A padding
    // tap gets an offset outside the descriptor and loads zeros: no per-k-tile address arithmetic, no select on the loaded values.
    int64_t mf = m0 < M ? m0 : M - 1;
    const int hw_ = g.Ho * g.Wo;
    const int bf = (int)(mf / hw_), remf = (int)(mf - (int64_t)bf * hw_);
    const int hof = remf / g.Wo, wof = remf - hof * g.Wo;
    int64_t base_pix = ((int64_t)bf * g.H + (hof * g.stride - 1)) * g.W + (wof * g.stride - 1);      // top-left tap of the tile's first row
    if constexpr (POSMAJ) {                       // the first visited tap of the tile's first image: no visited tap of any row lies below it
        const int bl = pt.b0 < pt.B ? pt.b0 : pt.B - 1;
        base_pix = ((int64_t)bl * g.H + pt.hi0 + kh_lo) * g.W + pt.wi0 + kw_lo;
    }
    base_pix = base_pix > 0 ? base_pix : 0;
    const int64_t left = ((int64_t)(M / hw_) * g.H * g.W - base_pix) * g.Cin * 4;                     // bytes up to the end of the input
    const auto xr = uniform_rsrc(x + base_pix * g.Cin, left);
    unsigned voff[NA];                            // byte offset of the current tap's pixel of each staged row (0xFFFFFFFF: padding)
    if constexpr (POSMAJ) {                       // every visited tap is valid for every row: the row offsets are loop invariant, the tap moves in the SGPR offset
#pragma unroll
        for (int j = 0; j < NA; ++j) voff[j] = (unsigned)(((int64_t)pbase[j] + kh_lo * g.W + kw_lo - base_pix) * g.Cin + c4) * 4u;
    }
    auto load_a = [&]() {
        if (!POSMAJ && ci0 == 0) {                // new tap (uniform branch, once per Cin / BK k-tiles)
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                const int hi = (hw0[j] >> 16) - 1 + kh, wi = (hw0[j] & 0xFFFF) - 1 + kw;
                const bool ok = (unsigned)hi < (unsigned)g.H && (unsigned)wi < (unsigned)g.W;
                voff[j] = ok ? (unsigned)(((int64_t)pbase[j] + kh * g.W + kw - base_pix) * g.Cin + c4) * 4u : 0xFFFFFFFFu;
            }
        }
        const unsigned soff = (unsigned)((POSMAJ ? ((kh - kh_lo) * g.W + (kw - kw_lo)) * g.Cin : 0) + ci0) * 4u;
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            // (bit_cast of the whole vector: indexing the builtin's result through `auto` gave element 0 four times with hipcc 7.2)
            ra[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(xr, voff[j], soff, 0));
        }
        ci0 += BK;
        if (ci0 == g.Cin) { ci0 = 0; if (++kw == kw_lo + kw_n) { kw = kw_lo; ++kh; } }
    };
    // POSMAJ: k offset of the NEXT k-tile in the weight rows -- the visited taps keep their (kh, kw, ci) place in the 9 Cin terms
    auto next_k0 = [&]() { return (kh * 3 + kw) * g.Cin + ci0; };
    const int nk = POSMAJ ? kh_n * kw_n * (g.Cin / BK) : D / BK;
    const float* a_base = As + half * LDA + wm * (32 * TM) + l31;
    const float* b_base = Bs + half * LDB + wn * (32 * TN) + l31;
    if (AHEAD2 && TM * TN == 1 && !(nk & 1)) {
        // 64x64 tiles: a k-tile is 16 MFMAs per wave -- 1024 matrix-pipe cycles, ~4000 when four waves share the SIMD -- while a loaded HBM / L2
        // round trip can take longer (scratch/lab/expand_lab.hip: 6200 -> 5800 cycles per k-tile, fused kernel 2.98 -> 2.95 ms): the operands are
        // requested TWO k-tiles ahead, in two staging register sets (+16 VGPRs; the LDS stays single-staged).  An even k-tile count only (Cin a
        // multiple of 64); one trip of the loop = two k-tiles = ONE chunk of the two-level sum.
        static_assert(!AHEAD2 || CHUNK % (2 * BK) == 0, "a chunk is a whole number of trips of the two-ahead loop");
        float4 ra1[NA], ra2[NA], rb2[BN * BK / 1024];
        auto stage = [&](float4 (&qa)[NA], float4 (&qb)[BN * BK / 1024], int kt) {
            load_a();
#pragma unroll
            for (int j = 0; j < NA; ++j) qa[j] = ra[j];
            load_tile<true, BN, BK>(Wt, N, D, n0, kt * BK, qb);
        };
        load_a();
        load_tile<true, BN, BK>(Wt, N, D, n0, 0, rb);
        store_tile<BM, BK>(As, ra);
        store_tile<BN, BK>(Bs, rb);
        __syncthreads();
        stage(ra1, rb, 1);
        // steady state, two k-tiles per trip: tile kt is in the LDS, tile kt + 1 on its way to (ra1, rb), tile kt + 2 is requested into (ra2, rb2).
        // The requests inside the loop are UNCONDITIONAL (hipcc's wait-count pass falls back to vmcnt(0) behind a conditional load, which would
        // undo the prefetch); those of the last trip point past the last tap / weight column -- range-checked buffer loads, values never used.
        for (int kt = 0; kt < nk; kt += 2) {
            stage(ra2, rb2, kt + 2);
            if (CHUNK != 0 && (kt * BK) % (CHUNK ? CHUNK : 1) == 0)      // chunk start: C = 0
                mfma_ktile<TM, TN, BK, LDA, LDB, CHUNK != 0>(a_base, b_base, acc);
            else mfma_ktile<TM, TN, BK, LDA, LDB>(a_base, b_base, acc);
            __syncthreads();
            store_tile<BM, BK>(As, ra1);
            store_tile<BN, BK>(Bs, rb);
            __syncthreads();
            stage(ra1, rb, kt + 3);
            mfma_ktile<TM, TN, BK, LDA, LDB>(a_base, b_base, acc);
            __syncthreads();
            if (kt + 2 < nk) {
                store_tile<BM, BK>(As, ra2);
                store_tile<BN, BK>(Bs, rb2);
                __syncthreads();
            }
            if constexpr (CHUNK == 2 * BK) add_chunk<TM, TN>(tot, acc);
            else if constexpr (CHUNK != 0) { if (((kt + 2) * BK) % CHUNK == 0 || kt + 2 >= nk) add_chunk<TM, TN>(tot, acc); }
        }
        if constexpr (CHUNK != 0) acc[0][0] = tot[0][0];       // the tile's value: the sum of the chunk sums
        return;
    }
    load_a();
    load_tile<true, BN, BK>(Wt, N, D, n0, POSMAJ ? (kh_lo * 3 + kw_lo) * g.Cin : 0, rb);       // (the first visited tap)
    store_tile<BM, BK>(As, ra);
    store_tile<BN, BK>(Bs, rb);
    __syncthreads();

    staged_kloop<TM, TN, BK, CHUNK>(a_base, b_base, nk, acc, tot,
        [&](int kt) {
            const int k0 = POSMAJ ? next_k0() : 0;           // (before load_a moves on)
            load_a();
            load_tile<true, BN, BK>(Wt, N, D, n0, POSMAJ ? k0 : kt * BK, rb);
        },
        [&]() {
            store_tile<BM, BK>(As, ra);
            store_tile<BN, BK>(Bs, rb);
        });
}

}  // namespace isx
