// expand_kernel.hpp -- the fused conv2 + conv3 kernel of expand.hip (a header so that scratch/lab/expand_lab.hip can instantiate it with phase stamps).
#pragma once
#include <utility>

#include "conv3x3_tile.hpp"

namespace isx {

// ---- 3x3 convolution to 64 channels + the 1x1 expansion behind it, as ONE kernel ------------------------------
//   y = act3( W3 . relu(conv3x3(x, W2) + b2) + b3 (+ residual) )        (conv2 + conv3 of a torchvision Bottleneck with 64 mid channels)
// A 64-pixel tile of the 3x3 convolution holds ALL 64 mid channels of its pixels = a complete A tile of the 1x1 expansion: the wave
// accumulators get bias + ReLU, go to the LDS (K-major, in place of the operand stages) and feed a second MFMA loop against W3 (given
// TRANSPOSED, (64, Cout): the B operands are coalesced buffer loads that hit the L2, offsets as SGPRs).  The mid activation (0.8 GB at
// 56x56, B = 1024) is neither written nor read back, and the HBM-bound expansion (7.4 GB for 105 GFLOP) runs inside an MFMA-bound kernel.
// Same arithmetic per element as isx_conv3x3_nhwc followed by isx_conv1x1_nhwc: the mid values are the fp32 numbers that path stores.
// DUAL: the first block of the stage, whose shortcut is a 1x1 projection of the block input x2 (64 channels, same pixels: stride 1):
//   y = act( [W3 | Wd] . [relu(conv3x3(x, W2) + b2) ; x2] + b ),  W3t = the concatenated weight transposed, (128, Cout);
// the x2 rows of the tile are fetched at kernel start, wait in registers during the 3x3 loop and go to a second LDS tile.
// Two-level sum (gemm_tile.hpp): the 3x3 loop folds its chain every 64 terms (conv3x3_mainloop); the expansion is ONE chunk (64 mid channels), with
// DUAL two -- the chain over the mid channels, then the chain over the x2 channels, added: that kernel holds two accumulator sets (2 x 64 VGPRs)
// and runs two workgroups per CU (one launch per trunk: the first block of stage 1).
template <int TN2, bool DUAL, bool STAMPS = false>
__global__ __launch_bounds__(256, DUAL ? 2 : 4) void conv3x3_expand_kernel(const float* __restrict__ x, int64_t M, const float* __restrict__ W2, Conv3x3Geom g,
                                                                const float* __restrict__ b2, const float* __restrict__ W3t, const float* __restrict__ b3,
                                                                const float* __restrict__ res, int relu, float* __restrict__ y,
                                                                unsigned long long* __restrict__ stamps = nullptr) {
    constexpr int COUT = 64 * TN2, LDY = 64 + 1, TILE_F = 32 * (64 + 64 + 2 * lds_pad(32));
    __shared__ float lds[(DUAL ? 2 : 1) * TILE_F];                          // 4160 floats: the 3x3 operand stages, then the 64 x 65 mid tile (+ the x2 tile)
    static_assert(TILE_F >= 64 * LDY, "mid tile must fit the operand stages");
    // XCD-aware order: XCD x gets a contiguous range of pixel tiles (neighbouring tiles share their halo rows in its L2)
    const int nwg = (int)gridDim.x, b = (int)blockIdx.x;
    const int64_t m0 = (int64_t)xcd_remap(b, nwg) * 64;

    // STAMPS (scratch/lab/expand_lab.hip only): shader-clock stamps of wave 0 at the phase boundaries, 8 per workgroup
    auto stamp = [&](int i) { if (STAMPS && threadIdx.x == 0) stamps[(int64_t)blockIdx.x * 8 + i] = __builtin_amdgcn_s_memtime(); };
    stamp(0);
    float4 x2r[4];
    if (DUAL) {                                                             // rows m0 .. m0 + 63 of x2 (= res): 16 chunks of 16 B each; rows past M read zeros
        const int64_t left = M - m0;
        const auto xr2 = uniform_rsrc(res + m0 * 64, (left < 64 ? left : 64) * 256);
#pragma unroll
        for (int j = 0; j < 4; ++j) x2r[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(xr2, (unsigned)((j * 256 + (int)threadIdx.x) * 16), 0, 0));
    }
    f32x16 acc[1][1];
    conv3x3_mainloop<1, 1, 32, true>(lds, x, M, W2, 64, g, m0, 0, acc);
    stamp(1);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, half = lane >> 5;
    if (DUAL) {                                                             // x2 tile -> second LDS tile, K-major X[k][pixel]
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx = j * 256 + (int)threadIdx.x, row = idx >> 4, k = (idx & 15) << 2;
            float* d = lds + TILE_F + k * LDY + row;
            d[0] = x2r[j].x; d[LDY] = x2r[j].y; d[2 * LDY] = x2r[j].z; d[3 * LDY] = x2r[j].w;
        }
    }
    {   // mid tile -> LDS, K-major: Y[k = mid channel][pixel]; lanes of a half-wave write consecutive k (stride 65: conflict-free)
        const float bv = b2[wn * 32 + l31];
#pragma unroll
        for (int e = 0; e < 16; ++e)
            lds[(wn * 32 + l31) * LDY + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * half] = fmaxf(acc[0][0][e] + bv, 0.0f);
    }
    __syncthreads();
    stamp(2);

    // expansion: wave w = all 64 pixels x output channels 16 TN2 w .. (TN2 / 2 column blocks): per k-step (mid channels 2s, 2s + 1) two A reads
    // from the LDS, TN2 / 2 coalesced B loads from the L2 and TN2 MFMAs; the four waves read disjoint quarters of W3
    constexpr int NJ = TN2 / 2;
    f32x16 acc2[2][NJ];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc2[i][j][e] = 0.0f;
    const float* a_base = lds + half * LDY + l31;
    const auto wr = uniform_rsrc(W3t, (int64_t)(DUAL ? 128 : 64) * COUT * 4);
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const unsigned wvo = (unsigned)((half * COUT + l31) * 4);
    const unsigned wso = (unsigned)(wave_u * 32 * NJ * 4);
    f32x16 acc3[DUAL ? 2 : 1][DUAL ? NJ : 1];                                   // DUAL: chain over the x2 channels (second chunk)
    if (DUAL) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc3[i][j][e] = 0.0f;
    }
#pragma unroll
    for (int s = 0; s < (DUAL ? 64 : 32); ++s) {
        const int ao = s < 32 ? 2 * s * LDY : TILE_F + 2 * (s - 32) * LDY;      // mid channels, then the x2 channels
        const float a0 = a_base[ao], a1 = a_base[ao + 32];
        float bq[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            bq[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wr, wvo, wso + (unsigned)((2 * s * COUT + 32 * j) * 4), 0));
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (DUAL && s >= 32) {
                acc3[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bq[j], acc3[0][j], 0, 0, 0);
                acc3[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bq[j], acc3[1][j], 0, 0, 0);
            } else {
                acc2[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bq[j], acc2[0][j], 0, 0, 0);
                acc2[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bq[j], acc2[1][j], 0, 0, 0);
            }
        }
    }
    if (DUAL) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc2[i][j] = acc2[i][j] + acc3[i][j];       // tot = (0 + chain_0) + chain_1
    }
    stamp(3);
    conv_epilogue_buffers<2, NJ, 2>(acc2, y, DUAL ? nullptr : res, b3, relu, m0, M, 0, COUT, COUT, 64, 0, wave_u * (32 * NJ), l31, half);
    if (STAMPS) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stamp(4); }
}

// ---- 3x3 convolution to 128 channels + the 1x1 expansion behind it, as ONE kernel (conv2 + conv3 of an identity Bottleneck with 128 mid channels) ----
//   y = act( W3 . relu(conv3x3(x, W2) + b2) + b3 (+ residual) )        stride 1, Cin % 64 == 0, Cout % 128 == 0
// With 128 output channels the 3x3 convolution has ONE n-tile: the 128 x 128 accumulator tile a workgroup holds when its k loop ends is the complete
// mid activation of its 128 rows = the A operand the stand-alone expansion fetches again for each of its Cout / 128 n-tiles.  Here it gets bias +
// ReLU, goes to the LDS K-major (Y[mid channel][row], row stride 64 TM + 1: the transposed writes of a half-wave fall into 32 different banks, as with
// LDY = 64 + 1 above) in place of the operand stages, and after ONE barrier feeds the expansion, n-tile by n-tile of 128 output channels:
//  * wave (wm, wn) owns the sub-tile it would own in the stand-alone GEMM; its A operands are LDS reads of the read-only mid tile, its W3 operands
//    (W3 TRANSPOSED, (128, Cout)) coalesced buffer loads that hit the L2, requested kW3Ahead k-steps ahead;
//  * NO barrier: the waves drift apart, and one wave's residual wait and store issue sit under the other waves' MFMAs;
//  * two-level sum of a K = 128 reduction (gemm_tile.hpp): chain over the mid channels 0-63 from +0, chain over 64-127 from +0, tot = (0 + chain_0) + chain_1;
//  * the STORES of n-tile j are issued four per k-step under the MFMAs of n-tile j + 1 (the finished values wait in the registers of the second chain), and
//    the residual of an n-tile is requested in its second half: no burst of 64 stores, no wait for a store or for a residual round trip (see the pipeline below).
// Same bits as isx_conv3x3_nhwc followed by isx_conv1x1_nhwc: the mid values are the fp32 numbers that path stores.
// TM = 2 (BK = 16): a 128-row tile; TM = 1 (BK = 32): a 64-row tail tile (64 x 128 mid tile).  POSMAJ: position-major rows (conv3x3_tile.hpp) -- the
// tile is output position p of the images b0 .., whose rows of y and of the residual are P Cout floats apart.
// f(integral_constant<int, 0>()), ..., f(integral_constant<int, N - 1>()): a loop that is unrolled by construction
template <int... I, class F>
__device__ __forceinline__ void static_for_seq(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>()), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_seq(std::make_integer_sequence<int, N>(), f); }

constexpr int kW3Ahead = 8;                                                  // k-steps (of 4 TM MFMAs per wave) between a W3 request and its use
constexpr int kExpand128LdsFloats = 128 * (128 + 1);                        // the 128 x 129 mid tile (66 KB; the operand stages need 16.6 KB of it)
template <int TM, int BK, bool POSMAJ>
__device__ __forceinline__ void conv3x3_expand128_tile(float* __restrict__ lds, const float* __restrict__ x, int64_t M, const float* __restrict__ W2, const Conv3x3Geom& g,
                                                       const float* __restrict__ b2, const float* __restrict__ W3t, int Cout, const float* __restrict__ b3,
                                                       const float* __restrict__ res, int relu, float* __restrict__ y, int64_t m0) {
    constexpr int BM = 64 * TM, LDY = BM + 1;
    static_assert(BK * (BM + 128 + 2 * lds_pad(BK)) <= 128 * LDY && 128 * LDY <= kExpand128LdsFloats, "operand stages and mid tile share the LDS");
    int64_t em0 = m0, eM = M, ldc = Cout;                                   // the epilogue's row numbering: rows em0 .. of eM, ldc floats apart
    if constexpr (POSMAJ) {
        const PosMajorTile pt = pos_major_tile(g, M, m0);
        if (pt.b0 >= pt.B) return;                                          // a tail tile of the last image group without a live row (block-uniform)
        const int64_t off = (int64_t)pt.p * Cout;
        y += off;
        if (res) res += off;
        em0 = pt.b0; eM = pt.B; ldc = (int64_t)g.Ho * g.Wo * Cout;
    }
    f32x16 acc[TM][2];
    conv3x3_mainloop<TM, 2, BK, false, kConvChunk, POSMAJ>(lds, x, M, W2, 128, g, m0, 0, acc);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, half = lane >> 5;
    const int wm_u = __builtin_amdgcn_readfirstlane(wm), wn_u = __builtin_amdgcn_readfirstlane(wn);
    const int row0 = wm_u * (32 * TM), col0 = wn_u * 64;
    {   // mid tile -> LDS, K-major: Y[k = mid channel][row]; lanes of a half-wave write consecutive k (stride 64 TM + 1: conflict-free)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = wn * 64 + j * 32 + l31;
            const float b2v = b2[k];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    lds[k * LDY + wm * (32 * TM) + i * 32 + mfma_row_of(e) + 4 * half] = fmaxf(acc[i][j][e] + b2v, 0.0f);
        }
    }
    __syncthreads();

    const float* a_base = lds + half * LDY + wm * (32 * TM) + l31;
    const auto wr = uniform_rsrc(W3t, (int64_t)128 * Cout * 4);
    const unsigned wvo = (unsigned)((half * Cout + l31) * 4);
    const auto rc = conv_tile_rsrc(y, em0, eM, ldc, BM);
    const auto rr = conv_tile_rsrc(res ? res : y, em0, res ? eM : em0, ldc, BM);        // no residual: a descriptor of zero rows (the requests load zeros that nothing reads)
    const auto br = uniform_rsrc(b3, (int64_t)Cout * 4);
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto load_b = [&](int n0, int s, int j) {       // W3t[2 s + half][n0 + col0 + 32 j + l31]: k-step s of the n-tile at column n0 (behind the last n-tile: in range or zeros, never used)
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wr, wvo, (unsigned)((n0 + col0) * 4) + (unsigned)(2 * s) * (unsigned)Cout * 4u + (unsigned)(j * 128), 0));
    };
    // y / residual addresses as in conv_epilogue_buffers: the lane's row and column in the VGPR offset (one per i; j is 128 B of immediate offset), the
    // MFMA row mfma_row_of(e) and the n-tile's column base in the SGPR offset
    const unsigned ldc4 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(ldc * 4));       // row stride in bytes (32-bit: 128 rows stay below 2^31, expand.hip)
    unsigned lo[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) lo[i] = (unsigned)(((int64_t)(row0 + i * 32 + 4 * half) * ldc + col0 + l31) * 4);
    // The expansion is ONE software pipeline over all n-tiles.  Per k-step (4 TM MFMAs): the A operands of step s + 1 (LDS) and the W3 operands of step
    // s + kW3Ahead (L2, a register ring that runs on into the next n-tile) are requested; steps 8-23 also issue the 32 TM STORES of the PREVIOUS n-tile, four
    // per step (its finished values wait in the registers of chain 1, which are free until step 32), and steps 36-51 request this n-tile's residual.  vmcnt
    // counts loads and stores in order: a store is first waited for by the W3 operand requested behind it, kW3Ahead k-steps later, and no wait count
    // comes near the 63 the instruction can encode.  All of it is unconditional: what does not exist lies outside its descriptor.
    constexpr int NV = TM * 2 * 16, PER = NV / 16;      // values of a wave per n-tile; stores / residual requests per k-step
    float bq[kW3Ahead][2];
#pragma unroll
    for (int s = 0; s < kW3Ahead; ++s) {
#pragma unroll
        for (int j = 0; j < 2; ++j) bq[s][j] = load_b(0, s, j);
    }
    unsigned wso = (unsigned)(col0 * 4) + (unsigned)(2 * kW3Ahead) * (unsigned)Cout * 4u;       // SGPR offset of the next W3 request
    __builtin_amdgcn_sched_barrier(0);
    f32x16 acc1[TM][2];                             // chain over the mid channels 64-127 (acc: 0-63), then the finished values of the n-tile
    zero_tiles(acc1);
    float rv[TM][2][16], bv[2];
    for (int n0 = 0; n0 < Cout; n0 += 128) {
        unsigned lo_st[TM];                           // the previous n-tile's stores (n0 == 0: none -- outside the descriptor)
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            lo_st[i] = n0 > 0 ? lo[i] : 0x80000000u;
            asm volatile("" : "+v"(lo_st[i]));
        }
        const unsigned so_st = n0 > 0 ? (unsigned)((n0 - 128) * 4) : 0u, so_ld = (unsigned)(n0 * 4);
        float a[2][TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) a[0][i] = a_base[32 * i];
        static_for<64>([&](auto S) {                  // (not "#pragma unroll": a body of this size is past the threshold up to which hipcc honours it)
            constexpr int s = S();
            if (s + 1 < 64) {
#pragma unroll
                for (int i = 0; i < TM; ++i) a[(s + 1) & 1][i] = a_base[2 * (s + 1) * LDY + 32 * i];
            }
            const float b[2] = {bq[s % kW3Ahead][0], bq[s % kW3Ahead][1]};
#pragma unroll
            for (int j = 0; j < 2; ++j)             // k-step s + kW3Ahead (past 63: of the next n-tile)
                bq[s % kW3Ahead][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wr, wvo + (unsigned)(j * 128), wso, 0));
            wso = s + kW3Ahead + 1 == 64 ? (unsigned)((n0 + 128 + col0) * 4) : wso + 2u * (unsigned)Cout * 4u;
            asm volatile("" : "+s"(wso));           // ONE running scalar offset (left to itself hipcc keeps 64 multiples of Cout in SGPRs, runs out of them and moves the sums to VGPRs)
            if (s >= 8 && s < 24) {                 // stores of the previous n-tile (n0 == 0: none)
#pragma unroll
                for (int q = 0; q < PER; ++q) {
                    const int t = (s - 8) * PER + q, i = t / 32, j = (t / 16) % 2, e = t % 16;
                    const float v = acc1[i][j][e];  // (a copy: __builtin_bit_cast of the vector ELEMENT itself gave element 0 sixteen times with hipcc 7.2)
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rc, lo_st[i] + (unsigned)(j * 128), (unsigned)mfma_row_of(e) * ldc4 + so_st, 0);
                }
            }
            if (s >= 36 && s < 52) {                // residual (and, with its first request, the bias) of this n-tile
                if (s == 36) {
#pragma unroll
                    for (int j = 0; j < 2; ++j) bv[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(br, (unsigned)((n0 + col0 + j * 32 + l31) * 4), 0, 0));
                }
#pragma unroll
                for (int q = 0; q < PER; ++q) {
                    const int t = (s - 36) * PER + q, i = t / 32, j = (t / 16) % 2, e = t % 16;
                    rv[i][j][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rr, lo[i] + (unsigned)(j * 128), (unsigned)mfma_row_of(e) * ldc4 + so_ld, 0));
                }
            }
            __builtin_amdgcn_sched_barrier(0);      // keep the requests above the MFMAs (hipcc otherwise sinks each load to its use: one L2 round trip per k-step)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (s < 32) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s & 1][i], b[j], s == 0 ? zero : acc[i][j], 0, 0, 0);
                    else acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s & 1][i], b[j], s == 32 ? zero : acc1[i][j], 0, 0, 0);
                }
        });
        // the n-tile's values, in the registers of chain 1: y = act(((0 + chain_0) + chain_1) + bias (+ residual))
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    float v = ((0.0f + acc[i][j][e]) + acc1[i][j][e]) + bv[j];
                    if (res) v += rv[i][j][e];
                    if (relu) v = fmaxf(v, 0.0f);
                    acc1[i][j][e] = v;
                }
    }
    // the last n-tile's stores (nothing waits for them); the row stride through an SGPR constraint: hipcc otherwise carries the sixteen row offsets
    // out of the loop in VGPRs and wraps every store into a readfirstlane loop
    unsigned ldc4e = ldc4;
    asm volatile("" : "+s"(ldc4e));
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float v = acc1[i][j][e];
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rc, lo[i] + (unsigned)(j * 128), (unsigned)mfma_row_of(e) * ldc4e + (unsigned)((Cout - 128) * 4), 0);
            }
}

// 128-row tiles, with the rows past the last whole round of resident workgroups as 64-row tiles in the same grid (tail_tile_of_block; a launch without
// a tail has no small tiles).  Two workgroups per CU: two accumulator sets + the residual + the W3 ring: all 256 VGPRs, no scratch; 66 KB of LDS.
template <bool POSMAJ>
__global__ __launch_bounds__(256, 2) void conv3x3_expand128_kernel(const float* __restrict__ x, int64_t M, const float* __restrict__ W2, Conv3x3Geom g,
                                                                   const float* __restrict__ b2, const float* __restrict__ W3t, int Cout, const float* __restrict__ b3,
                                                                   const float* __restrict__ res, int relu, float* __restrict__ y, TileMap tm_big, TileMap tm_small,
                                                                   int64_t m_split) {
    __shared__ float lds[kExpand128LdsFloats];
    tail_tile_of_block(tm_big, tm_small, m_split, [&](auto T, auto BK, int64_t m0, int64_t) {
        conv3x3_expand128_tile<T(), BK(), POSMAJ>(lds, x, M, W2, g, b2, W3t, Cout, b3, res, relu, y, m0);
    });
}

}  // namespace isx
