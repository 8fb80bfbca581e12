// gemm_tile.hpp -- device helpers shared by the fp32-MFMA GEMM (gemm.hip) and the implicit-GEMM 3x3 convolution
// (conv.hip): XCD-aware tile mapping, the K-major LDS staging of operand tiles, the staged k loop with the two-level sum (staged_kloop) and the
// block numbering of the 128x128 + 64x64 tail launches (tail_tile_of_block).
#pragma once
#include <type_traits>

#include "isx_internal.hpp"

namespace isx {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int GROUP_N = 16;                     // n-tiles per scheduling group

// b / nwg: block index and block count of the tile range (defaults: the whole grid); GROUP: n-tiles per scheduling group
template <int GROUP = GROUP_N>
__device__ __forceinline__ void tile_of_block(const TileMap tm, int& tile_m, int& tile_n, int b, int nwg) {
    const int wg = xcd_remap(b, nwg);
    // grouped order: GROUP n-tiles wide, all m-tiles tall, n fastest inside a group row
    const int per_group = GROUP * tm.tiles_m;
    const int gid = wg / per_group;
    const int first_n = gid * GROUP;
    const int gsz = min(GROUP, tm.tiles_n - first_n);
    const int within = wg - gid * per_group;
    tile_m = within / gsz;
    tile_n = first_n + within % gsz;
}

template <int GROUP = GROUP_N>
__device__ __forceinline__ void tile_of_block(const TileMap tm, int& tile_m, int& tile_n) {
    tile_of_block<GROUP>(tm, tile_m, tile_n, (int)blockIdx.x, tm.tiles_m * tm.tiles_n);
}

// Tile-shape dispatch of the launchers: calls f(TM, TN, BK) -- std::integral_constants -- for shape `cfg` of pick_tile_cfg (0 = 128x128,
// 1 = 64x128, 2 = 128x64, anything else = 64x64).  The ONE place that says which BK a shape runs with (BK = 16 for 128x128: gemm.hip's header).
// MASK: the shapes the caller's kernel family is instantiated for (pick_tile_cfg's mask; the convolutions have no 64x128 instance).
template <unsigned MASK = 0xF, class F>
static inline void with_tile_shape(int cfg, F&& f) {
    using std::integral_constant;
    if (cfg == 0) return f(integral_constant<int, 2>(), integral_constant<int, 2>(), integral_constant<int, 16>());
    if (cfg == 2) return f(integral_constant<int, 2>(), integral_constant<int, 1>(), integral_constant<int, 32>());
    if constexpr ((MASK & 2u) != 0) {
        if (cfg == 1) return f(integral_constant<int, 1>(), integral_constant<int, 2>(), integral_constant<int, 32>());
    }
    f(integral_constant<int, 1>(), integral_constant<int, 1>(), integral_constant<int, 32>());
}

// ROWS x BK k = ROWS*CH float4; thread t takes idx = j*256 + t: row = idx/CH, chunk = idx%CH.
// ALIGNED: 16-B aligned rows AND D a multiple of BK (unconditional 16-B loads); otherwise scalar loads with a zero-filled k tail.
// AUX: cache-policy bits of the buffer loads of the ALIGNED path (0 = default, 2 = nt: a stream that no later access of this CU re-reads)
template <bool ALIGNED, int ROWS, int BK, int AUX = 0>
__device__ __forceinline__ void load_tile(const float* __restrict__ P, int64_t rows, int D, int64_t row0, int k0,
                                          float4 (&reg)[ROWS * BK / 1024]) {
    constexpr int CH = BK / 4;               // 16-B chunks per staged row
    if (ALIGNED) {
        // ALIGNED: D % BK == 0, 16-B aligned rows.  Buffer loads: a wave-uniform descriptor of the tile's rows (loop invariant), one
        // constant 32-bit offset per staged chunk, the k offset as SGPR: no address arithmetic inside the k loop.  Rows past the edge
        // fall outside the descriptor and load zeros (they are never stored).
        const int64_t left = rows - row0;
        const auto rs = uniform_rsrc(P + row0 * D, (left < ROWS ? left : ROWS) * (int64_t)D * 4);
#pragma unroll
        for (int j = 0; j < ROWS * CH / 256; ++j) {
            const int idx = j * 256 + threadIdx.x;
            const unsigned vo = (unsigned)(idx / CH) * (unsigned)D * 4u + (unsigned)((idx % CH) << 4);
            reg[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, (unsigned)k0 * 4u, AUX));
        }
        return;
    }
    if ((D & 3) == 0 && ((uintptr_t)P & 15) == 0) {
        // D a multiple of 4 but not of BK (class-score descriptors: D = 464) on 16-B aligned rows: the same buffer loads; in the last
        // k-tile the chunks past D -- they would read the next row -- are sent outside the descriptor and load zeros (fma(0, 0, acc) = acc)
        const int64_t left = rows - row0;
        const auto rs = uniform_rsrc(P + row0 * D, (left < ROWS ? left : ROWS) * (int64_t)D * 4);
#pragma unroll
        for (int j = 0; j < ROWS * CH / 256; ++j) {
            const int idx = j * 256 + threadIdx.x;
            const unsigned vo = k0 + ((idx % CH) << 2) < D ? (unsigned)(idx / CH) * (unsigned)D * 4u + (unsigned)((idx % CH) << 4) : 0x80000000u;
            reg[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, (unsigned)k0 * 4u, 0));
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < ROWS * CH / 256; ++j) {
        const int idx = j * 256 + threadIdx.x;
        int64_t r = row0 + (idx / CH);
        r = r < rows ? r : rows - 1;                       // clamp: rows past the edge are never stored
        const int k = k0 + ((idx % CH) << 2);
        const float* src = P + r * D + k;
        reg[j].x = (k + 0 < D) ? src[0] : 0.f;
        reg[j].y = (k + 1 < D) ? src[1] : 0.f;
        reg[j].z = (k + 2 < D) ? src[2] : 0.f;
        reg[j].w = (k + 3 < D) ? src[3] : 0.f;
    }
}

// K-major LDS image [k][row] with row stride ROWS + pad.  A staging lane (chunk c = idx % CH, row r = idx / CH) writes
// element (4c + i, r): bank = ((4c + i) * stride + r) mod 32.  BK = 32 (CH = 8, 4 rows per 32-lane group): stride = 1 mod 32 gives
// 4c + r, all distinct.  BK = 16 (CH = 4, 8 rows per group): stride = 1 would give 4c + r with 4-way collisions (measured:
// SQ_LDS_BANK_CONFLICT = 25 % of the LDS cycles of the 128x128 kernel); stride = 2 mod 32 gives 8c + r, all distinct.  Operand
// reads are 32 consecutive floats per half-wave for either stride.
__host__ __device__ constexpr int lds_pad(int BK) { return BK == 16 ? 2 : 1; }

template <int ROWS, int BK>
__device__ __forceinline__ void store_tile(float* __restrict__ T, const float4 (&reg)[ROWS * BK / 1024]) {
    constexpr int CH = BK / 4;
    constexpr int LD = ROWS + lds_pad(BK);                  // K-major stride chosen for conflict-free transposed writes
#pragma unroll
    for (int j = 0; j < ROWS * CH / 256; ++j) {
        const int idx = j * 256 + threadIdx.x;
        const int r = idx / CH, k = (idx % CH) << 2;
        T[(k + 0) * LD + r] = reg[j].x;
        T[(k + 1) * LD + r] = reg[j].y;
        T[(k + 2) * LD + r] = reg[j].z;
        T[(k + 3) * LD + r] = reg[j].w;
    }
}

// Buffer descriptor of the rows [m0, min(m0 + BM, M)) of a row-major (M, ldc) fp32 matrix: wave-uniform by construction (kernel
// arguments and the tile index), so hipcc keeps it in SGPRs (no waterfall loop around the buffer instructions).
__device__ __forceinline__ auto conv_tile_rsrc(const float* base, int64_t m0, int64_t M, int64_t ldc, int BM) {
    const int64_t rows = (M - m0) < BM ? (M - m0) : BM;
    return uniform_rsrc(base + m0 * ldc, rows * ldc * 4);
}
// byte offset of (tile row `row`, column ncol) inside that descriptor; a column past N is sent outside it
__device__ __forceinline__ unsigned conv_lane_off(int64_t ncol, int64_t N, int row, int64_t ldc) {
    return ncol < N ? (unsigned)((row * ldc + ncol) * 4) : 0x80000000u;
}


// lane offset and SGPR row offsets of the 16 C elements a lane holds of one 32x32 MFMA tile
__device__ __forceinline__ constexpr int mfma_row_of(int e) { return (e & 3) + 8 * (e >> 2); }

// Residual (or mask) values of ALL of a wave's TM x TN accumulator tiles, requested back to back: ONE round trip to memory for the whole
// epilogue.  (Round 6: the per-tile form -- 16 loads, s_waitcnt vmcnt(0), 16 stores, next tile -- serialised TM x TN round trips, and on gfx9
// vmcnt counts stores too, so each wait also drained the previous tile's stores: four load + store latencies per 128x128 tile, as long as the
// matrix work of a K = 128 tile.)  The caller issues this ahead of its last k-tile's MFMAs where the registers allow.
template <int TM, int TN>
__device__ __forceinline__ void epilogue_fetch(float (&rv)[TM][TN][16], const float* __restrict__ src, int64_t m0, int64_t M, int64_t n0, int64_t N, int64_t ldc,
                                               int BM, int row0, int col0, int l31, int half) {
    const auto rr = conv_tile_rsrc(src, m0, M, ldc, BM);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int ncol = (int)n0 + col0 + j * 32 + l31;
            const unsigned lo = conv_lane_off(ncol, N, row0 + i * 32 + 4 * half, ldc);
#pragma unroll
            for (int e = 0; e < 16; ++e)
                rv[i][j][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rr, lo, (unsigned)(mfma_row_of(e) * ldc * 4), 0));
        }
}

// Convolution epilogue of one wave's TM x TN accumulator tiles through BUFFER instructions: y = act(acc + bias[n] (+ residual)).
// rc / rr: descriptors of the block tile's rows of C / the residual; row0 = the wave's first tile row (wave-uniform).
// AHEAD: how many of the TM x TN tiles have their residual (or mask) values requested before the first of them is stored -- 16 VGPRs each.
// TM x TN (default): one round trip for the whole epilogue; kernels at their register bound pass fewer (the fused expand kernel at 106 of 128
// VGPRs: 2; the gradient kernels, which read a mask: 1, and with residual AND mask the per-tile form).  The bias values are always read first: a
// bias load issued between two tiles' stores waits for those stores (vmcnt counts both on gfx9).
template <int TM, int TN, int AHEAD = TM * TN>
__device__ __forceinline__ void conv_epilogue_buffers(const f32x16 (&acc)[TM][TN], float* __restrict__ C, const float* __restrict__ res,
                                                      const float* __restrict__ bias, int relu, int64_t m0, int64_t M, int64_t n0, int64_t N,
                                                      int64_t ldc, int BM, int row0, int col0, int l31, int half, const float* __restrict__ mask = nullptr) {
    // bias == nullptr: no bias;  mask (same layout as C): y = mask > 0 ? y : 0 (backward of the ReLU whose OUTPUT is `mask`, backward.hip)
    const auto rc = conv_tile_rsrc(C, m0, M, ldc, BM);
    float bias_pre[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int ncol = (int)n0 + col0 + j * 32 + l31;
        bias_pre[j] = (bias && ncol < N) ? bias[ncol] : 0.0f;
    }
    if (!(res && mask)) {
        // one operand stream besides the accumulators (residual OR mask, or none): fetch AHEAD tiles' worth, then add / select / store them
        constexpr int NT = TM * TN, STEP = AHEAD < 1 ? 1 : (AHEAD > NT ? NT : AHEAD);
        const float* src = res ? res : mask;
        const auto rr = conv_tile_rsrc(src ? src : C, m0, M, ldc, BM);
#pragma unroll
        for (int t0 = 0; t0 < NT; t0 += STEP) {
            float rv[STEP][16];
            if (src) {
#pragma unroll
                for (int t = t0; t < t0 + STEP && t < NT; ++t) {
                    const int i = t / TN, j = t % TN;
                    const unsigned lo = conv_lane_off((int)n0 + col0 + j * 32 + l31, N, row0 + i * 32 + 4 * half, ldc);
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        rv[t - t0][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rr, lo, (unsigned)(mfma_row_of(e) * ldc * 4), 0));
                }
                __builtin_amdgcn_sched_barrier(0);           // keep the batch's loads above its first store
            }
#pragma unroll
            for (int t = t0; t < t0 + STEP && t < NT; ++t) {
                const int i = t / TN, j = t % TN;
                const unsigned lo = conv_lane_off((int)n0 + col0 + j * 32 + l31, N, row0 + i * 32 + 4 * half, ldc);
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float v = src ? rv[t - t0][e] : 0.0f;
                    float y = acc[i][j][e] + bias_pre[j];
                    if (res) y += v;
                    if (relu) y = fmaxf(y, 0.0f);
                    if (mask) y = v > 0.0f ? y : 0.0f;
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y), rc, lo, (unsigned)(mfma_row_of(e) * ldc * 4), 0);
                }
            }
        }
        return;
    }
    const auto rr = conv_tile_rsrc(res ? res : C, m0, M, ldc, BM);
    const auto rm = conv_tile_rsrc(mask ? mask : C, m0, M, ldc, BM);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int ncol = (int)n0 + col0 + j * 32 + l31;
            const float bias_v = bias_pre[j];
            const unsigned lo = conv_lane_off(ncol, N, row0 + i * 32 + 4 * half, ldc);
            float rv[16], mv[16];
            if (res) {
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    rv[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rr, lo, (unsigned)(((e & 3) + 8 * (e >> 2)) * ldc * 4), 0));
            }
            if (mask) {
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    mv[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rm, lo, (unsigned)(((e & 3) + 8 * (e >> 2)) * ldc * 4), 0));
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                float y = acc[i][j][e] + bias_v;
                if (res) y += rv[e];
                if (relu) y = fmaxf(y, 0.0f);
                if (mask) y = mv[e] > 0.0f ? y : 0.0f;
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y), rc, lo, (unsigned)(((e & 3) + 8 * (e >> 2)) * ldc * 4), 0);
            }
        }
    }
}

// ---- two-level accumulation of the trunk convolutions (round 5) -----------------------------------------------------------------
// A convolution output is NOT one fp32 chain over the whole reduction any more: the flattened reduction (kh, kw, ci) is cut into chunks of
// ISX_CONV_CHUNK terms; inside a chunk the k-ordered fma chain of the matrix core starts from +0, and the chunk sums are added, in order, into
// a second accumulator:   tot = 0;  for each chunk c: tot = tot + chain_c;   y = act(tot + bias (+ residual)).
// Why: a chain over K terms drifts from the exact sum like eps . K, chunks of c terms like eps . sqrt(K c + K^2 / c); measured end to end
// (scratch/chunk_study.py, ResNet-50 / ResNet-152 descriptors against a float64 evaluation): one chain is 1.2x further from float64 than torch's
// CPU fp32 path, chunks of 64 land at 0.7x.  K <= 64 (one chunk): tot = 0 + chain, the bits of rounds 1-4.  Restated by oracle/isx_oracle.c.
constexpr int kConvChunk = ISX_CONV_CHUNK;
constexpr int kWgPerCu128 = 2;      // resident workgroups per CU of the 128x128 convolution tiles: two accumulator sets = 128 VGPRs + ~55 -> two waves per SIMD
constexpr int kTailLdsFloats = 32 * (64 + 64 + 2);      // BK = 32 stage of a 64x64 tail tile of the 128x128 convolution launches (lds_pad(32) = 1 per operand)
static_assert(kConvChunk % 32 == 0, "a chunk is a whole number of k-tiles");

// ---- 128x128 tiles with a 64x64 tail in one grid (conv1x1_tail_kernel, conv3x3_tail_kernel, conv1x1_dual_tail_kernel; host side: gemm_tail_grid) ----
// LDS of such a kernel: the larger of the BK = 16 stage of a 128x128 tile and the BK = 32 stage of a 64x64 tile
constexpr int kBigLdsFloats = 16 * (128 + 128 + 2 * lds_pad(16));
constexpr int kTailKernelLdsFloats = kBigLdsFloats > kTailLdsFloats ? kBigLdsFloats : kTailLdsFloats;
// The tile of this block: the first tm_big.tiles_m * tm_big.tiles_n blocks are the 128x128 tiles of the rows below m_split, the rest are the 64x64
// tiles of the rows from m_split on.  (The number of big tiles is a multiple of 8: a block's XCD is the same in both numberings.)
// tile(T, BK, m0, n0) runs the (64 T) x (64 T) tile at row m0, column n0; T and BK are std::integral_constants (2, 16 or 1, 32).
template <class Tile>
__device__ __forceinline__ void tail_tile_of_block(const TileMap tm_big, const TileMap tm_small, int64_t m_split, Tile&& tile) {
    const int nbig = tm_big.tiles_m * tm_big.tiles_n;
    int tile_m, tile_n;
    if ((int)blockIdx.x < nbig) {
        tile_of_block(tm_big, tile_m, tile_n, (int)blockIdx.x, nbig);
        tile(std::integral_constant<int, 2>(), std::integral_constant<int, 16>(), (int64_t)tile_m * 128, (int64_t)tile_n * 128);
    } else {
        tile_of_block(tm_small, tile_m, tile_n, (int)blockIdx.x - nbig, tm_small.tiles_m * tm_small.tiles_n);
        tile(std::integral_constant<int, 1>(), std::integral_constant<int, 32>(), m_split + (int64_t)tile_m * 64, (int64_t)tile_n * 64);
    }
}

// tot += acc (the chain of the chunk that just ended; acc itself is overwritten by the first MFMAs of the next chunk, which take C = 0)
template <int TM, int TN>
__device__ __forceinline__ void add_chunk(f32x16 (&tot)[TM][TN], const f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) tot[i][j] = tot[i][j] + acc[i][j];
}

// a += t on the 16 registers of one MFMA tile IN PLACE (tied asm operands: the sum stays in a's registers, hipcc cannot rename it into fresh ones)
__device__ __forceinline__ void add_tile_inplace(f32x16& a, const f32x16& t) {
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        f32x2_t x = {a[2 * p], a[2 * p + 1]};
        const f32x2_t y = {t[2 * p], t[2 * p + 1]};
        asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(x) : "v"(y));
        a[2 * p] = x[0];
        a[2 * p + 1] = x[1];
    }
}

// MFMAs of one staged k-tile.  Small tiles (TM * TN <= 2) have too few MFMAs per k-step to hide an LDS round trip
// behind: the operand reads of HALF a k-tile are issued back to back, then the MFMAs (counted lgkmcnt(n) waits instead
// of a drain per step; +4 % on the trunk's 1x1 convolutions).  a_base / b_base: this lane's first operand element.
// ZERO_C: the first k-step starts new chains (C = 0 as an inline constant; the old contents of acc are dead): chunk start of the two-level sum.
template <int TM, int TN, int BK, int LDA, int LDB, bool ZERO_C = false>
__device__ __forceinline__ void mfma_ktile(const float* __restrict__ a_base, const float* __restrict__ b_base, f32x16 (&acc)[TM][TN]) {
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (TM * TN <= 2) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float af[BK / 4][TM], bf[BK / 4][TN];
#pragma unroll
            for (int kk = 0; kk < BK / 4; ++kk) {
#pragma unroll
                for (int i = 0; i < TM; ++i) af[kk][i] = a_base[(2 * (h * (BK / 4) + kk)) * LDA + 32 * i];
#pragma unroll
                for (int j = 0; j < TN; ++j) bf[kk][j] = b_base[(2 * (h * (BK / 4) + kk)) * LDB + 32 * j];
            }
#pragma unroll
            for (int kk = 0; kk < BK / 4; ++kk)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk][i], bf[kk][j], (ZERO_C && h == 0 && kk == 0) ? zero : acc[i][j], 0, 0, 0);
        }
    } else {
        // register prefetch one k-step ahead: the operand reads of step kk + 1 are issued BEFORE the MFMAs of step kk, so a wave
        // that finds itself alone on its SIMD (siblings parked at a barrier) does not expose an LDS round trip per step (+0.7-1.5 % on the big GEMMs
        // against the plain per-step loop)
        float a[2][TM], b[2][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) a[0][i] = a_base[32 * i];
#pragma unroll
        for (int j = 0; j < TN; ++j) b[0][j] = b_base[32 * j];
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            if (kk + 1 < BK / 2) {
#pragma unroll
                for (int i = 0; i < TM; ++i) a[(kk + 1) & 1][i] = a_base[(2 * kk + 2) * LDA + 32 * i];
#pragma unroll
                for (int j = 0; j < TN; ++j) b[(kk + 1) & 1][j] = b_base[(2 * kk + 2) * LDB + 32 * j];
            }
            __builtin_amdgcn_sched_barrier(0);             // keep the reads above the MFMAs
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk & 1][i], b[kk & 1][j], (ZERO_C && kk == 0) ? zero : acc[i][j], 0, 0, 0);
        }
    }
}

// Operand addresses of the k-steps of a staged k-tile, PINNED in registers.  The K-major images put k-step kk at 2 kk LDA floats = more than the
// 1020 B a ds_read2_b32 offset reaches, so every k-step needs a base register of its own.  In the plain loops hipcc computes these 2 x BK / 2
// addresses once; with the chunk fold in the loop it re-derived them with a v_add_u32 in front of every ds_read2 instead (15 VALU instructions
// among the 32 MFMAs of a k-tile; the two-level kernels ran 10 % below the one-chain ones at ANY chunk length).  The empty asm makes each
// address an opaque 32-bit LDS pointer that cannot be rematerialised.
using lds_cfp = const __attribute__((address_space(3))) float*;
template <int BK>
struct KtilePtrs { lds_cfp a[BK / 2], b[BK / 2]; };
template <int BK, int LDA, int LDB>
__device__ __forceinline__ KtilePtrs<BK> pin_ktile_ptrs(const float* a_base, const float* b_base) {
    KtilePtrs<BK> p;
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) {
        p.a[kk] = (lds_cfp)(a_base + 2 * kk * LDA);
        p.b[kk] = (lds_cfp)(b_base + 2 * kk * LDB);
        asm volatile("" : "+v"(p.a[kk]));
        asm volatile("" : "+v"(p.b[kk]));
    }
    return p;
}
// the k loop of mfma_ktile's prefetch variant on pinned addresses
// tot (ZERO_C only): the chain that ended with the previous k-tile is added to tot tile by tile right in front of the MFMA that
// restarts that tile from C = 0 -- the adds of tile n + 1 issue while the MFMA of tile n runs.  (The MFMAs that produced acc are at least one
// barrier old: no MFMA -> VALU wait states needed.)
template <int TM, int TN, int BK, bool ZERO_C = false>
__device__ __forceinline__ void mfma_ktile_pinned(const KtilePtrs<BK>& p, f32x16 (&acc)[TM][TN], f32x16 (*tot)[TN] = nullptr) {
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float a[2][TM], b[2][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) a[0][i] = p.a[0][32 * i];
#pragma unroll
    for (int j = 0; j < TN; ++j) b[0][j] = p.b[0][32 * j];
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) {
        if (kk + 1 < BK / 2) {
#pragma unroll
            for (int i = 0; i < TM; ++i) a[(kk + 1) & 1][i] = p.a[kk + 1][32 * i];
#pragma unroll
            for (int j = 0; j < TN; ++j) b[(kk + 1) & 1][j] = p.b[kk + 1][32 * j];
        }
        __builtin_amdgcn_sched_barrier(0);             // keep the reads above the MFMAs
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                if (ZERO_C && kk == 0 && tot) add_tile_inplace(tot[i][j], acc[i][j]);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk & 1][i], b[kk & 1][j], (ZERO_C && kk == 0) ? zero : acc[i][j], 0, 0, 0);
            }
    }
}

template <int TM, int TN>
__device__ __forceinline__ void zero_tiles(f32x16 (&t)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) t[i][j][e] = 0.0f;
}

// tot += acc;  acc = 0: the fold of the weight-gradient kernels (wgrad_kernel.hpp), whose k loops have a shape of their own
template <int TM, int TN>
__device__ __forceinline__ void fold_chunk(f32x16 (&tot)[TM][TN], f32x16 (&acc)[TM][TN]) {
    add_chunk<TM, TN>(tot, acc);
    zero_tiles(acc);
}
// PINNED (the 128x128 shape): the k-tile adds the previous chunk's chain to tot itself; otherwise staged_kloop folds with add_chunk behind the chunk
template <int TM, int TN, int BK, int LDA, int LDB, bool PINNED, bool ZERO_C = false>
__device__ __forceinline__ void mfma_ktile_sel(const float* __restrict__ a_base, const float* __restrict__ b_base, const KtilePtrs<BK>& pins, f32x16 (&acc)[TM][TN],
                                               f32x16 (*tot)[TN] = nullptr) {
    if constexpr (PINNED) mfma_ktile_pinned<TM, TN, BK, ZERO_C>(pins, acc, tot);
    else mfma_ktile<TM, TN, BK, LDA, LDB, ZERO_C>(a_base, b_base, acc);
}

// ---- THE staged k loop of the fp32 tile kernels (cosine_gemm_tile, conv1x1_dual_tile, the plain path of conv3x3_mainloop) -----------------------
// Per k-tile kt: request k-tile kt + 1 into the caller's staging registers (load_next(kt + 1)), run the MFMAs of k-tile kt out of the LDS,
// barrier, write the staged registers to the LDS (store_staged()), barrier.  The caller has k-tile 0 in the LDS (the K-major images of a
// (64 TM) x BK and a (64 TN) x BK operand tile, store_tile) behind a barrier, and acc zeroed; every wave has left the LDS on return.
// a_base / b_base: this lane's first operand element in the two images (mfma_ktile).  They come from the caller, next to the lane arithmetic of
// its epilogue: derived here a second time, hipcc shared less of that arithmetic and several instances moved by registers and scratch (round 8).
// CHUNK != 0: the two-level sum -- terms per first-level chain; tot (zeroed by the caller) collects the chains and acc returns their sum.
// CHUNK == 0: one chain over all nk k-tiles in acc (scores, gradients); tot is a dummy.
// The shape of the chunked loop is what round 5 paid for (A/B on the 3x3 / dual families, ms per lab pass; one chain: 9.89 / 6.61):
//  * NESTED: an outer loop over the chunks, the inner loop over the CHUNK / BK k-tiles of a chunk is the plain staged loop of rounds 1-4.  A
//    conditional fold INSIDE one k loop cost 10-15 % at any chunk length: behind the MFMAs it needs 16 wait states and keeps hipcc from hoisting
//    the loop's first barrier in between the last MFMAs (11.13 / 7.56; with the addresses pinned 10.85 / 7.29); in front of the MFMAs hipcc
//    duplicates the loop body and serialises the staging loads (11.37 / 7.61).
//  * C = 0: the FIRST k-tile of a chunk is a second copy of the body whose first MFMAs take C = 0 as an inline constant -- no zeroing pass
//    (fold between the inner loops 10.63 / 7.15, with the C = 0 start 10.41 / 6.97).
//  * PINNED operand addresses for the 128x128 shape (pin_ktile_ptrs: without them hipcc re-derived every address with a v_add_u32 per ds_read2),
//    whose C = 0 k-tile also adds the PREVIOUS chunk's chain to tot in place, tile by tile in front of the MFMA that restarts the tile
//    (add_tile_inplace: 3x3 10.49 -> 10.22, dual 7.04 -> 6.96; it loses on the smaller tiles, which fold with add_chunk behind the chunk).
//  * the LAST chunk's add_chunk of the pinned shape stands outside the loop: there is no next C = 0 k-tile to carry it.
template <int TM, int TN, int BK, int CHUNK, class LoadNext, class StoreStaged>
__device__ __forceinline__ void staged_kloop(const float* a_base, const float* b_base, int nk, f32x16 (&acc)[TM][TN],
                                             f32x16 (&tot)[CHUNK ? TM : 1][CHUNK ? TN : 1], LoadNext&& load_next, StoreStaged&& store_staged) {
    constexpr int LDA = 64 * TM + lds_pad(BK), LDB = 64 * TN + lds_pad(BK);
    constexpr bool PINNED = CHUNK != 0 && TM * TN == 4;
    KtilePtrs<BK> pins;
    if constexpr (PINNED) pins = pin_ktile_ptrs<BK, LDA, LDB>(a_base, b_base);
    f32x16 (*totp)[TN] = nullptr;
    if constexpr (CHUNK != 0) totp = tot;
    auto body = [&](int kt, auto zero_c) {
        const bool more = (kt + 1 < nk);
        if (more) load_next(kt + 1);
        mfma_ktile_sel<TM, TN, BK, LDA, LDB, PINNED, decltype(zero_c)::value>(a_base, b_base, pins, acc, totp);
        __syncthreads();
        if (more) {
            store_staged();
            __syncthreads();
        }
    };
    if constexpr (CHUNK == 0) {
        for (int kt = 0; kt < nk; ++kt) body(kt, std::false_type());
    } else {
        for (int kt = 0; kt < nk;) {
            const int kend = kt + CHUNK / BK < nk ? kt + CHUNK / BK : nk;
            body(kt++, std::true_type());                      // (PINNED: adds the PREVIOUS chunk's chain in front of its C = 0 MFMAs)
            for (; kt < kend; ++kt) body(kt, std::false_type());
            if (!PINNED) add_chunk<TM, TN>(tot, acc);
        }
        if (PINNED) add_chunk<TM, TN>(tot, acc);       // the last chunk
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = tot[i][j];       // the tile's value: the sum of the chunk sums (the epilogues read acc)
    }
}
}  // namespace isx
