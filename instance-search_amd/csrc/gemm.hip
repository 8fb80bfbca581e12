// gemm.hip -- the fp32-MFMA GEMM C = Q . G^T of libisx and its four epilogues (EpiArgs, isx_internal.hpp): the query x gallery
// scores (isx_cosine_sim), the fused top-k filter (run_topk_chunks, cosine.hip), the 1x1 convolutions of the inference trunk
// (isx_conv1x1_nhwc, conv.hip) and the masked input gradient of a 1x1 convolution (backward.hip).
//
// Numerics: v_mfma_f32_32x32x2_f32 is bit-for-bit a k-ordered fp32 fma chain, so every
// score equals  acc = fmaf(q[k], g[k], acc), k = 0..D-1  exactly -- the oracle's
// definition.  K is never split across waves or blocks, so the order is preserved.
//
// Tiling (gfx950): 128x128 output tile per 256-thread workgroup (4 waves as 2x2, each
// wave 64x64 = 2x2 MFMA tiles of 32x32, 64 accumulator VGPRs), BK = 16 (124 VGPRs, 16.5 KB LDS:
// 4 workgroups per CU; measured 133 TFLOP/s vs 130 at BK = 32 and 122 at BK = 8); smaller tiles
// (64x128, 128x64, 64x64, BK = 32) are picked for mid-size problems.  Q and G tiles
// are staged K-major in LDS ([k][row], row stride 129 floats): the staging loads are
// 16 B/lane with 8 lanes covering one 128-B row segment (coalesced), the transposed
// ds_write_b32 are bank-conflict-free by the odd stride, and the MFMA operand reads are
// 32 consecutive floats per half-wave (conflict-free ds_read_b32).  Global loads of
// tile t+1 are issued before the MFMAs of tile t (register prefetch).  Workgroups are
// remapped XCD-aware: each XCD walks a contiguous range of tiles, ordered so that
// concurrently resident tiles share Q / G panels in that XCD's L2.
#include <stdlib.h>

#include <tuple>

#include "gemm_tile.hpp"

namespace isx {

#ifndef ISX_STAMPS
#define ISX_STAMPS 0            // lab builds only (tools/build_variant.sh stamps -DISX_STAMPS=1, tools/conv_phase_lab.py): wave 0 of every workgroup of the
#endif                          // convolution GEMM records the shader clock at its phase boundaries into the buffer set by isx_debug_set_stamps
#if ISX_STAMPS
__device__ unsigned long long* g_stamps = nullptr;
#define ISX_STAMP(i) do { if (g_stamps && threadIdx.x == 0) g_stamps[(int64_t)blockIdx.x * 8 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#define ISX_STAMP_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#else
#define ISX_STAMP(i) do { } while (0)
#define ISX_STAMP_DRAIN() do { } while (0)
#endif

// The kernels and cosine_gemm_tile take the fields of EpiArgs<EPI> (isx_internal.hpp) as separate __restrict__ parameters p0, p1, n in
// field order (unused ones null / 0), and the tile rebuilds the struct.  Passed as a struct, a kernel argument arrives by reference in the
// kernarg segment and its pointers lose the noalias of __restrict__: the GEMM instances then compile to different code (more SGPRs, loads
// hoisted to the kernel entry), and so they do when only the tile takes the struct.
template <int EPI> using EpiP1 = std::conditional_t<EPI == kEpiFilter, uint8_t*, const float*>;
template <int EPI> __device__ __forceinline__ EpiArgs<EPI> epi_args(const float* p0, EpiP1<EPI> p1, int n) {
    if constexpr (EPI == kEpiFilter || EPI == kEpiConv) return {p0, p1, n};
    else if constexpr (EPI == kEpiMaskedGrad) return {p0, p1};
    else return {};
}
static std::tuple<const float*, const float*, int> kernel_args(const ScoresArgs&) { return {nullptr, nullptr, 0}; }
static std::tuple<const float*, uint8_t*, int> kernel_args(const FilterArgs& a) { return {a.thr, a.gflag, a.ngrp}; }
static std::tuple<const float*, const float*, int> kernel_args(const ConvArgs& a) { return {a.bias, a.residual, a.relu}; }
static std::tuple<const float*, const float*, int> kernel_args(const MaskedGradArgs& a) { return {a.mask, a.add, 0}; }

// Block tile (64*TM) x (64*TN): 4 waves as 2x2, each wave TM x TN MFMA tiles of 32x32.
// EPI: the epilogue mode (kEpiScores, kEpiFilter, kEpiConv, kEpiMaskedGrad), p0 / p1 / n: its arguments (above).
// CHUNK (convolution mode only): terms per first-level chain of the two-level sum (gemm_tile.hpp), 0 = one chain over all of D (scores, gradients)
template <bool ALIGNED, int TM, int TN, int EPI, int BK, int CHUNK = (EPI == kEpiConv ? kConvChunk : 0)>
__device__ __forceinline__ void cosine_gemm_tile(float* __restrict__ lds, const float* __restrict__ Q, int64_t M,
                                                 const float* __restrict__ G, int64_t N, int D,
                                                 float* __restrict__ C, int64_t ldc, int64_t m0, int64_t n0,
                                                 const float* __restrict__ p0, EpiP1<EPI> __restrict__ p1, int n) {
    const EpiArgs<EPI> ea = epi_args<EPI>(p0, p1, n);
    constexpr int BM = 64 * TM, BN = 64 * TN, LDA = BM + lds_pad(BK), LDB = BN + lds_pad(BK);
    float* As = lds;
    float* Bs = lds + BK * LDA;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, half = lane >> 5;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    f32x16 tot[CHUNK ? TM : 1][CHUNK ? TN : 1];
    zero_tiles(tot);

    // convolution epilogue on 64x64 tiles (short K loops, residual layers): fetch the residual values before
    // the main loop so that their latency overlaps the operand loads and the MFMAs
    constexpr bool PRE_RES = (EPI == kEpiConv && TM * TN == 1);
    float pre_res[PRE_RES ? 16 : 1];
    const float* res = nullptr;                 // convolution mode: the residual (layout of C) or null
    if constexpr (EPI == kEpiConv) res = ea.residual;
    // epilogue addressing of the convolution mode: wave-uniform row pointers (SGPRs) + one 32-bit lane offset
    const int wm_u = __builtin_amdgcn_readfirstlane(wm), wn_u = __builtin_amdgcn_readfirstlane(wn);
    if (PRE_RES) {
        if (res) {
            const auto rr = conv_tile_rsrc(res, m0, M, ldc, BM);
            const unsigned lo = conv_lane_off(n0 + wn_u * 32 + l31, N, wm_u * 32 + 4 * half, ldc);
#pragma unroll
            for (int e = 0; e < 16; ++e)
                pre_res[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rr, lo, (unsigned)(((e & 3) + 8 * (e >> 2)) * ldc * 4), 0));
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) pre_res[e] = 0.0f;
        }
    }

    // larger convolution tiles: the residual of the WHOLE tile is requested in one go right behind the main loop, into the registers the first-level
    // chains leave free, and consumed tile by tile as it arrives -- one round trip instead of TM x TN serialised ones (gemm_tile.hpp, epilogue_fetch).
    // (Requested one k-tile earlier, under the last MFMAs, the 64 values of a 128x128 tile push the kernel past 256 VGPRs: 204 B of scratch.)
    constexpr bool LATE_RES = (EPI == kEpiConv && TM * TN == 4);       // (128x64 tiles at their 128-register bound: 24-112 B of scratch with it)
    float late_res[LATE_RES ? TM : 1][LATE_RES ? TN : 1][16];

    float4 ra[BM * BK / 1024], rb[BN * BK / 1024];
    const int nk = (D + BK - 1) / BK;
    if (EPI == kEpiConv) ISX_STAMP(0);
    load_tile<ALIGNED, BM, BK>(Q, M, D, m0, 0, ra);
    load_tile<ALIGNED, BN, BK>(G, N, D, n0, 0, rb);
    store_tile<BM, BK>(As, ra);
    store_tile<BN, BK>(Bs, rb);
    __syncthreads();
    if (EPI == kEpiConv) ISX_STAMP(1);

    const float* a_base = As + half * LDA + wm * (32 * TM) + l31;
    const float* b_base = Bs + half * LDB + wn * (32 * TN) + l31;
    staged_kloop<TM, TN, BK, CHUNK>(a_base, b_base, nk, acc, tot,
        [&](int kt) {
            load_tile<ALIGNED, BM, BK>(Q, M, D, m0, kt * BK, ra);
            load_tile<ALIGNED, BN, BK>(G, N, D, n0, kt * BK, rb);
        },
        [&]() {
            store_tile<BM, BK>(As, ra);
            store_tile<BN, BK>(Bs, rb);
        });
    if (EPI == kEpiConv) ISX_STAMP(2);
    // the TN bias values of this lane's columns BEFORE everything else of the epilogue: a bias load behind the residual requests would make the first
    // add wait for all of them, and one between two tiles' stores would wait for those stores (vmcnt counts both on gfx9)
    float bias_pre[TN];
    if constexpr (EPI == kEpiConv) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int ncol = (int)(n0 + wn_u * (32 * TN) + j * 32) + l31;
            bias_pre[j] = ncol < N ? ea.bias[ncol] : 0.0f;
        }
    }
    if constexpr (LATE_RES) {
        if (res) {
            epilogue_fetch<TM, TN>(late_res, res, m0, M, n0, N, ldc, BM, wm_u * (32 * TM), wn_u * (32 * TN), l31, half);
            __builtin_amdgcn_sched_barrier(0);               // every load above the first store
            if (ISX_STAMPS) { ISX_STAMP_DRAIN(); ISX_STAMP(3); }
        }
    }

    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)
    if constexpr (EPI == kEpiMaskedGrad) {
        // backward.hip: C = (acc (+ add)) . [mask > 0]
        conv_epilogue_buffers<TM, TN, 1>(acc, C, ea.add, nullptr, 0, m0, M, n0, N, ldc, BM, wm_u * (32 * TM), wn_u * (32 * TN), l31, half, ea.mask);
        return;
    }
    if constexpr (EPI == kEpiConv) {
        // Convolution epilogue through BUFFER instructions: a wave-uniform descriptor of the tile's rows (clipped at row M by the
        // hardware), one 32-bit lane offset per 32x32 MFMA tile (a column >= N gets an offset outside the descriptor: its loads return
        // 0, its stores are dropped) and the row offset (e & 3) + 8 (e >> 2) as an SGPR: ~4 instructions per output element and no
        // branch, where per-element 64-bit addresses and edge tests cost ~20 (a fifth of a K = 256 tile's time).
        const auto rc = conv_tile_rsrc(C, m0, M, ldc, BM);
        const auto rr = conv_tile_rsrc(res ? res : C, m0, M, ldc, BM);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int ncol = (int)(n0 + wn_u * (32 * TN) + j * 32) + l31;
                const float bias_v = bias_pre[j];
                const unsigned lo = conv_lane_off(ncol, N, wm_u * (32 * TM) + i * 32 + 4 * half, ldc);
                float rv[16];
                if (!PRE_RES && !LATE_RES && res) {
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        rv[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rr, lo, (unsigned)(((e & 3) + 8 * (e >> 2)) * ldc * 4), 0));
                }
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    float y = acc[i][j][e] + bias_v;
                    if (PRE_RES) { if (res) y += pre_res[e]; }
                    else if (LATE_RES) { if (res) y += late_res[LATE_RES ? i : 0][LATE_RES ? j : 0][e]; }
                    else if (res) y += rv[e];
                    if (ea.relu) y = fmaxf(y, 0.0f);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y), rc, lo, (unsigned)(((e & 3) + 8 * (e >> 2)) * ldc * 4), 0);
                }
            }
        }
        if (ISX_STAMPS) { ISX_STAMP(4); ISX_STAMP_DRAIN(); ISX_STAMP(5); }
        return;
    }
    if (EPI == kEpiScores && (int64_t)BM * ldc * 4 < (1ll << 32)) {
        // plain score store through BUFFER instructions (round 4; the convolution epilogue has used them since round 2): a wave-uniform
        // descriptor of the tile's rows clipped at row M, one 32-bit lane offset per MFMA tile (a column >= N is sent outside the
        // descriptor and its store dropped), the row offset as an SGPR -- no per-element 64-bit address, no edge branch.  Short-K
        // problems (D = 464: 29 k-tiles per 128 x 128 tile) spent a tenth of their time in the old epilogue.
        const auto rc = conv_tile_rsrc(C, m0, M, ldc, BM);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int ncol = (int)(n0 + wn_u * (32 * TN) + j * 32) + l31;
                const unsigned lo = conv_lane_off(ncol, N, wm_u * (32 * TM) + i * 32 + 4 * half, ldc);
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float v = acc[i][j][e];             // (a scalar copy first: bit_cast applied to the vector element itself stored element 0 sixteen times, hipcc 7.2)
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rc, lo, (unsigned)(((e & 3) + 8 * (e >> 2)) * ldc * 4), 0);
                }
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            // wave-uniform row pointers + 32-bit lane offsets (64-bit per-element addresses cost ~35 VGPRs and a wave per SIMD)
            const int64_t ng = n0 + wn_u * (32 * TN) + j * 32;      // first column of this 32-column group (uniform)
            const int ncol = (int)ng + l31;
            const bool n_ok = ncol < N;
            const int lane_off = 4 * half * (int)ldc + ncol;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int64_t mu = m0 + wm_u * (32 * TM) + i * 32 + (e & 3) + 8 * (e >> 2);     // uniform; this lane's row = mu + 4 * half
                const bool row_ok = (mu + 4 * half < M);
                const float v = acc[i][j][e];
                if constexpr (EPI == kEpiFilter) {
                    // fused top-k filter: a 32-column group of row m is stored only if one of its scores
                    // can still enter the row's top-k (score >= thr[m], a lower bound of the final k-th
                    // score); one flag byte per (row, group) tells the select kernel which groups exist.
                    // The test is a compare + wave ballot (no cross-lane data movement).
                    const float t = row_ok ? (ea.thr + mu)[4 * half] : INFINITY;
                    const unsigned long long qm = __ballot(n_ok && v >= t);
                    const bool q = ((half ? (qm >> 32) : qm) & 0xFFFFFFFFull) != 0ull;
                    if (row_ok && ng < N) {
                        if (l31 == 0) (ea.gflag + mu * ea.ngrp + (ng >> 5))[4 * half * ea.ngrp] = q ? 1 : 0;
                        if (q && n_ok) (C + mu * ldc)[lane_off] = v;
                    }
                } else {
                    if (row_ok && n_ok) (C + mu * ldc)[lane_off] = v;
                }
            }
        }
    }
}

// (convolution mode: two accumulator sets.  128x128 tiles: two workgroups per CU -- without the bound hipcc takes 296 registers and one fits;
// the smaller tiles serve the HBM-bound layers and keep four -- unbounded, the 128x64 shape took 164 registers and lost a fifth on 256 -> 64 at 56x56)
template <bool ALIGNED, int TM, int TN, int EPI, int BK>
__global__ __launch_bounds__(256, EPI != kEpiConv ? 1 : TM * TN == 4 ? kWgPerCu128 : 4) void cosine_gemm_kernel(const float* __restrict__ Q, int64_t M,
                                                          const float* __restrict__ G, int64_t N, int D,
                                                          float* __restrict__ C, int64_t ldc, TileMap tm,
                                                          const float* __restrict__ p0, EpiP1<EPI> __restrict__ p1, int n) {
    __shared__ float lds[BK * (64 * TM + 64 * TN + 2 * lds_pad(BK))];
    int tile_m, tile_n;
    tile_of_block(tm, tile_m, tile_n);
    const int64_t m0 = (int64_t)tile_m * (64 * TM), n0 = (int64_t)tile_n * (64 * TN);
    if (tm.m_active && m0 >= *tm.m_active) return;          // uniform: whole tile beyond the live rows
    cosine_gemm_tile<ALIGNED, TM, TN, EPI, BK>(lds, Q, M, G, N, D, C, ldc, m0, n0, p0, p1, n);
}

// 1x1-convolution GEMM (kEpiConv) as 128x128 tiles with a 64x64 TAIL: the rows past the last whole round of 1024 resident workgroups run
// as 64x64 tiles in the same grid (see conv3x3_tail_kernel in conv.hip: a few 128x128 tiles alone on their CUs at the end of a launch of
// three to twelve rounds cost 3-10 % of it).  Same arithmetic per output element.
template <bool ALIGNED>
__global__ __launch_bounds__(256, kWgPerCu128) void conv1x1_tail_kernel(const float* __restrict__ Q, int64_t M, const float* __restrict__ G, int64_t N, int D,
                                                              float* __restrict__ C, int64_t ldc, TileMap tm_big, TileMap tm_small, int64_t m_split,
                                                              const float* __restrict__ bias, const float* __restrict__ residual, int relu) {
    __shared__ float lds[kTailKernelLdsFloats];
    tail_tile_of_block(tm_big, tm_small, m_split, [&](auto T, auto BK, int64_t m0, int64_t n0) {
        cosine_gemm_tile<ALIGNED, T(), T(), kEpiConv, BK()>(lds, Q, M, G, N, D, C, ldc, m0, n0, bias, residual, relu);
    });
}

// rows covered by whole rounds of 128x128 tiles when the rest of the grid is a partial round (0: no split)
std::atomic<int> g_tail_split{1};
int64_t gemm_tail_split_rows(int64_t M, int64_t N, int64_t slots) {
    const int64_t tn = (N + 127) / 128, tiles = ((M + 127) / 128) * tn;
    if (!g_tail_split || tn > slots || slots % tn != 0) return 0;
    const int64_t rounds = tiles / slots, rem = tiles - rounds * slots;
    if (rounds < 1 || rem == 0 || rem > slots * 4 / 5) return 0;
    return rounds * (slots / tn) * 128;
}
TailGrid gemm_tail_grid(int64_t rows, int64_t N, int64_t split) {
    TailGrid t;
    t.big.m_active = t.small.m_active = nullptr;
    t.big.tiles_m = (int)(split / 128);
    t.big.tiles_n = (int)((N + 127) / 128);
    t.small.tiles_m = (int)((rows - split + 63) / 64);          // (virtual rows: exact, isx_internal.hpp)
    t.small.tiles_n = (int)((N + 63) / 64);
    t.blocks = (unsigned)(t.big.tiles_m * t.big.tiles_n + t.small.tiles_m * t.small.tiles_n);
    return t;
}

// ---- tile-shape selection ------------------------------------------------------------------
// Candidate block tiles with their measured steady-state efficiency (fraction of the fp32-MFMA
// peak on a large problem) and resident workgroups per CU.  The launcher picks the shape with the
// smallest estimated time  rounds(T tiles over S slots) * tile_work / efficiency  -- large
// problems get 128x128, mid-size ones (bench: 512 x 10k) avoid a half-empty last round.
struct TileCfg { int tm, tn, wg_per_cu; float eff; };
static const TileCfg kCfgs[] = { {2, 2, 4, 0.92f}, {1, 2, 4, 0.87f}, {2, 1, 4, 0.89f}, {1, 1, 6, 0.84f} };     // 10 000 x 32 768 x 2048: 145 / 137 / 140 / 132 TFLOP/s
// The tile shape (index into kCfgs: 0 = 128x128, 1 = 64x128, 2 = 128x64, 3 = 64x64) with the smallest estimated time among those in
// `mask`; eff[c]: steady-state efficiency of shape c for the calling kernel family; split > 0: shape 0 runs with a 64x64 tail.
int pick_tile_cfg(int64_t M, int64_t N, int64_t split, const float* eff, unsigned mask, int wg_per_cu_128) {
    int best = -1;
    double best_t = 1e300;
    for (int c = 0; c < 4; ++c) {
        if (!((mask >> c) & 1u)) continue;
        TileCfg k = kCfgs[c];
        if (c == 0) k.wg_per_cu = wg_per_cu_128;
        const double tiles = (double)((M + 64 * k.tm - 1) / (64 * k.tm)) * (double)((N + 64 * k.tn - 1) / (64 * k.tn));
        const double slots = 256.0 * k.wg_per_cu;
        // time in units of "one full round" (= wg_per_cu tiles on every CU).  Workgroups finish unevenly,
        // so a launch costs its tile count plus a tail that is ~0.2 round for launches below one round and
        // fades quadratically for longer ones (fitted on MI355X, 256 ... 10k query rows x 10k ... 100k)
        const double x = tiles / slots;
        const double t0 = (c == 0 ? 0.22 : c == 3 ? 0.15 : 0.25);
        double rounds = x + (x <= 0.7 ? t0 : t0 * (0.7 / x) * (0.7 / x));
        // a CU works its tiles off at the rate of its matrix pipe however many of them are resident: the launch cannot end before the
        // CU with one tile more than the average is done (50 176 x 512 x 2048: 1568 tiles of 128x128 = 6.1 per CU took 7 tile times)
        const double per_cu = (double)((int64_t)((tiles + 255.0) / 256.0)) / k.wg_per_cu;
        rounds = rounds > per_cu ? rounds : per_cu;
        if (c == 0 && split > 0) rounds = x + 0.05;                          // the tail runs as small tiles: no round quantisation
        const double t = rounds * k.wg_per_cu * (k.tm * k.tn) / eff[c];
        if (t < best_t) { best_t = t; best = c; }
    }
    return best;
}

static std::atomic<int> g_force_cfg{[] { const char* e = getenv("ISX_DEBUG_GEMM_CFG"); return e ? atoi(e) : -1; }()};            // debug / A-B hook
void set_gemm_cfg(int c) { g_force_cfg = c; }

template <int EPI, int TM, int TN, int BK>
static void launch_cfg(bool aligned, const float* Q, int64_t M, const float* G, int64_t N, int D, float* C, int64_t ldc,
                       const EpiArgs<EPI>& ea, hipStream_t st, const int* m_active) {
    TileMap tm;
    tm.m_active = m_active;
    tm.tiles_m = (int)((M + 64 * TM - 1) / (64 * TM));
    tm.tiles_n = (int)((N + 64 * TN - 1) / (64 * TN));
    const dim3 grid((unsigned)(tm.tiles_m * tm.tiles_n)), block(256);
    const auto [p0, p1, n] = kernel_args(ea);
    if (aligned) hipLaunchKernelGGL((cosine_gemm_kernel<true, TM, TN, EPI, BK>), grid, block, 0, st, Q, M, G, N, D, C, ldc, tm, p0, p1, n);
    else hipLaunchKernelGGL((cosine_gemm_kernel<false, TM, TN, EPI, BK>), grid, block, 0, st, Q, M, G, N, D, C, ldc, tm, p0, p1, n);
}

template <int EPI>
static int launch_gemm_any(const float* Q, int64_t M, const float* G, int64_t N, int D, float* C, int64_t ldc, const EpiArgs<EPI>& ea,
                           hipStream_t st, const int* m_active = nullptr) {
    if (M == 0 || N == 0) return ISX_OK;
    if (((M + 63) / 64) * ((N + 63) / 64) >= (1ll << 31)) { isx_set_error("cosine gemm: too many tiles for one grid"); return ISX_ERR_ARG; }
    const bool aligned = (D % 32 == 0) && (((uintptr_t)Q | (uintptr_t)G) % 16 == 0);     // no k tail for BK = 16 or 32
    const bool aligned16 = aligned || ((D % 16 == 0) && (((uintptr_t)Q | (uintptr_t)G) % 16 == 0));   // enough for the BK = 16 (128x128) tiles: D = 464
    // convolutions: 128x128 tiles (two workgroups per CU: the two-level sum) + 64x64 tail in one grid
    const int64_t split = (EPI == kEpiConv) ? gemm_tail_split_rows(M, N, 256 * kWgPerCu128) : 0;
    static const float eff_gemm[4] = {kCfgs[0].eff, kCfgs[1].eff, kCfgs[2].eff, kCfgs[3].eff};
    int best = pick_tile_cfg(M, N, split, eff_gemm, 0xF, EPI == kEpiConv ? kWgPerCu128 : 4);
    // (Round 1 forced 64x64 tiles on residual layers and 128x64 on the others: the per-element epilogue was a visible share of a tile.
    // With the buffer-instruction epilogue the same round / tail model as for the score GEMM picks the convolution tiles: 128x128
    // wherever the grid fills the chip -- 256->1024 + residual 0.90 -> 0.87 ms, 512->2048 + residual 0.85 -> 0.81, 512->256 1.64 -> 1.58 --
    // and 128x64 for Cout = 64.)
    if (g_force_cfg >= 0 && g_force_cfg < 4) best = g_force_cfg;
    if (EPI == kEpiScores && best == 0 && g_force_cfg < 0 && g_tail_split && !m_active) {
        // Score matrix of FEW query rows against a long gallery (configs[1] / [2] retrieval: 1 000 x 100 000): 8 x 782 tiles of 128x128 are
        // 6.1 rounds of the 1024 resident workgroups and cost 7 -- the last 112 tiles run alone.  The gallery columns covered by whole rounds
        // go out as 128x128 tiles, the remaining columns as a second launch of 64x64 tiles (a quarter of the work each, 1536 resident).
        // Every score is the same k-ordered chain in either tile shape.
        const int64_t tm_ = (M + 127) / 128, tn_ = (N + 127) / 128, slots = 1024;
        const int64_t rounds = tm_ * tn_ / slots, rem = tm_ * tn_ - rounds * slots;
        const int64_t n_big = rounds * slots / tm_ * 128;                  // columns of the whole rounds
        if (rounds >= 1 && rem > 0 && rem <= slots * 3 / 5 && n_big > 0 && n_big < N && (n_big * D * 4) % 16 == 0) {
            launch_cfg<EPI, 2, 2, 16>(aligned16, Q, M, G, n_big, D, C, ldc, ea, st, m_active);
            launch_cfg<EPI, 1, 1, 32>(aligned, Q, M, G + n_big * D, N - n_big, D, C + n_big, ldc, ea, st, m_active);
            ISX_CHECK_LAUNCH("cosine_gemm");
            return ISX_OK;
        }
    }
    if constexpr (EPI == kEpiConv) {
        if (best == 0 && split > 0) {
            const TailGrid tg = gemm_tail_grid(M, N, split);
            const dim3 grid(tg.blocks), block(256);
            if (aligned) hipLaunchKernelGGL((conv1x1_tail_kernel<true>), grid, block, 0, st, Q, M, G, N, D, C, ldc, tg.big, tg.small, split, ea.bias, ea.residual, ea.relu);
            else hipLaunchKernelGGL((conv1x1_tail_kernel<false>), grid, block, 0, st, Q, M, G, N, D, C, ldc, tg.big, tg.small, split, ea.bias, ea.residual, ea.relu);
            ISX_CHECK_LAUNCH("conv1x1_tail");
            return ISX_OK;
        }
    }
    with_tile_shape(best, [&](auto TM, auto TN, auto BK) {          // (D % 16 == 0 is enough for the BK = 16 shape)
        launch_cfg<EPI, TM(), TN(), BK()>(BK() == 16 ? aligned16 : aligned, Q, M, G, N, D, C, ldc, ea, st, m_active);
    });
    ISX_CHECK_LAUNCH("cosine_gemm");
    return ISX_OK;
}

int launch_cosine_gemm(const float* Q, int64_t M, const float* G, int64_t N, int D, float* C, int64_t ldc, hipStream_t st,
                       const int* m_active) {
    return launch_gemm_any(Q, M, G, N, D, C, ldc, ScoresArgs{}, st, m_active);
}

int launch_cosine_gemm_filter(const float* Q, int64_t M, const float* G, int64_t N, int D, float* C, int64_t ldc,
                              const float* thr, uint8_t* gflag, hipStream_t st, const int* m_active) {
    return launch_gemm_any(Q, M, G, N, D, C, ldc, FilterArgs{thr, gflag, (int)((N + 31) / 32)}, st, m_active);
}

// 1x1 convolution = the same GEMM with the bias / residual / ReLU epilogue (conv.hip)
int launch_conv1x1_gemm(const float* x, int64_t M, const float* w, int64_t N, int D, float* y, const float* bias, const float* residual, int relu,
                        hipStream_t st) {
    return launch_gemm_any(x, M, w, N, D, y, N, ConvArgs{bias, residual, relu}, st);
}

// gradient of a 1x1 convolution wrt its input (backward.hip)
int launch_gemm_masked(const float* A, int64_t M, const float* Bt, int64_t N, int D, float* C, const float* mask, const float* add, hipStream_t st) {
    return launch_gemm_any(A, M, Bt, N, D, C, N, MaskedGradArgs{mask, add}, st);
}
}  // namespace isx

using namespace isx;

// Test hook (include/isx.h): force a tile shape (0..3), -1 = automatic.
ISX_API void isx_debug_set_gemm_cfg(int c) { set_gemm_cfg(c); }

#if ISX_STAMPS
// lab builds only: where the convolution GEMM's workgroups record their phase stamps (8 x u64 per workgroup); nullptr = off
extern "C" __attribute__((visibility("default"))) int isx_debug_set_stamps(unsigned long long* buf) {
    return hipMemcpyToSymbol(HIP_SYMBOL(isx::g_stamps), &buf, sizeof(buf)) == hipSuccess ? 0 : -1;
}
#endif
