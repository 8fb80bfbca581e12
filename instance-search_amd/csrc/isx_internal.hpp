// isx_internal.hpp -- launchers shared between translation units of libisx.
#pragma once
#include <atomic>

#include "isx_common.hpp"

namespace isx {

// Zero `bytes` (a multiple of 4) at a 4-byte aligned device pointer with a KERNEL on `st` (cosine.hip); 0 or ISX_ERR_HIP (error string set, prefixed
// with `who`).  Every entry zeroes through this and none through hipMemsetAsync: captured into a hipGraph, the memset node zeroes on the first
// replay only and fills with stale bits on every later one (ROCm 7.0; found by tests/test_gpu_graph_capture.py, docs/rounds/r16.md).
int zero_words_async(void* p, size_t bytes, hipStream_t st, const char* who);

// ---- the fp32 GEMM of gemm.hip ----------------------------------------------------------------------------------------------------
// Epilogue modes (the EPI template argument of cosine_gemm_kernel) and the arguments of each mode.
constexpr int kEpiScores = 0, kEpiFilter = 1, kEpiConv = 2, kEpiMaskedGrad = 3;
template <int EPI> struct EpiArgs {};                                                     // kEpiScores: store every score
// kEpiFilter: a 32-column group of row m is stored only if one of its scores reaches thr[m]; gflag (M x ngrp, ngrp = ceil(N/32)) flags them
template <> struct EpiArgs<kEpiFilter> { const float* thr; uint8_t* gflag; int ngrp; };
// kEpiConv: y = acc + bias[n] (+ residual, layout of C, or null), then max(y, 0) if relu
template <> struct EpiArgs<kEpiConv> { const float* bias; const float* residual; int relu; };
// kEpiMaskedGrad: C = (acc (+ add)) . [mask > 0]; mask and add have the layout of C, either may be null
template <> struct EpiArgs<kEpiMaskedGrad> { const float* mask; const float* add; };
using ScoresArgs = EpiArgs<kEpiScores>;
using FilterArgs = EpiArgs<kEpiFilter>;
using ConvArgs = EpiArgs<kEpiConv>;
using MaskedGradArgs = EpiArgs<kEpiMaskedGrad>;

// C[m][n] = sum_k Q[m][k] * G[n][k]  (k-ordered fp32 fma chain), C row stride ldc.
// m_active (optional, device scalar): tiles whose first row is >= *m_active exit immediately.
int launch_cosine_gemm(const float* Q, int64_t M, const float* G, int64_t N, int D, float* C, int64_t ldc,
                       hipStream_t st, const int* m_active = nullptr);

// Same GEMM with the filtering epilogue: the scores of a (row, 32-column group) are stored to C only
// when one of them reaches thr[row] (a lower bound of the row's final k-th best score); gflag
// (M, ngrp = ceil(N/32)) bytes say which groups were stored.
int launch_cosine_gemm_filter(const float* Q, int64_t M, const float* G, int64_t N, int D, float* C, int64_t ldc,
                              const float* thr, uint8_t* gflag, hipStream_t st, const int* m_active = nullptr);

// 1x1 convolution over channels-last pixels: the same GEMM, epilogue y = act(. + bias[n] (+ residual)) (used by conv.hip)
int launch_conv1x1_gemm(const float* x, int64_t M, const float* w, int64_t N, int D, float* y, const float* bias, const float* residual, int relu,
                        hipStream_t st);

// Gradient of a 1x1 convolution wrt its input (backward.hip): C = (A . Bt^T (+ add)) . [mask > 0], C row stride N
int launch_gemm_masked(const float* A, int64_t M, const float* Bt, int64_t N, int D, float* C, const float* mask, const float* add, hipStream_t st);

// Tail of a convolution launch in 128x128 tiles: rows covered by whole rounds of 1024 resident workgroups when the rest of the grid is a
// partial round -- the caller runs the remaining rows as 64x64 tiles in the same grid; 0 = no split.  g_tail_split: debug / A-B switch.
extern std::atomic<int> g_tail_split;      // (the debug / A-B knobs are relaxed atomics: a test thread may flip them while another thread launches)
int64_t gemm_tail_split_rows(int64_t M, int64_t N, int64_t slots = 1024);       // slots: resident 128x128 workgroups of the calling kernel (256 CUs x workgroups per CU)
// Tile grid of a kernel: tiles_m x tiles_n tiles, numbered by tile_of_block (gemm_tile.hpp)
struct TileMap {
    int tiles_m, tiles_n;
    const int* m_active;       // optional device scalar: only rows < *m_active are live (fast.hip fallback)
};
// Grid of a launch with such a tail: `big` = the 128x128 tiles of the rows below `split` (> 0, from gemm_tail_split_rows: a multiple of 128),
// `small` = the 64x64 tiles of the rows from `split` on, blocks = the tiles of both.  rows: the REAL row count M, whose last tail tile may be
// partial -- the count rounds up -- or the VIRTUAL row count of a position-major 3x3 launch (conv3x3_tile.hpp), a multiple of 128: there the
// 64-row tail tiles divide the rest exactly, and the same rounding is exact.
struct TailGrid { TileMap big, small; unsigned blocks; };
TailGrid gemm_tail_grid(int64_t rows, int64_t N, int64_t split);
// Tile shape (0 = 128x128, 1 = 64x128, 2 = 128x64, 3 = 64x64) with the smallest estimated launch time among those in `mask` (rounds of resident
// workgroups + tail + per-CU quantisation, gemm.hip); eff[4]: steady-state efficiency per shape of the calling kernel family.
int pick_tile_cfg(int64_t M, int64_t N, int64_t split, const float* eff, unsigned mask, int wg_per_cu_128 = 4);

// Position-major row order of a 3x3 launch (conv3x3_tile.hpp; conv.hip holds the eligibility and its debug switch): the virtual row count, 0 = pixel-major
int64_t conv3x3_pos_major_rows(int64_t B, int H, int W, int Cin, int Ho, int Wo, int64_t Cout, int64_t tiles_n64);
int conv3x3_pos_major_raster();            // 1: the debug switch that keeps those tiles in raster order (Conv3x3Geom::raster) instead of longest first

// Streaming variant for the HBM-bound Cin = 64 layers (stream1x1.hip): persistent workgroups, weights in registers, pixel tiles by LDS-DMA.
bool conv1x1_stream_applicable(int64_t M, int Cin, int Cout, const float* x, const float* res);
int launch_conv1x1_stream(const float* x, int64_t M, const float* w, int Cin, int Cout, const float* bias, const float* res, int relu, float* y,
                          hipStream_t st);

// fp16-operand variant (fast.hip): approximate scores, fp32 accumulate; the kEpiFilter epilogue, gflag == nullptr -> plain GEMM.
int launch_gemm_f16(const _Float16* Q, int64_t M, const _Float16* G, int64_t N, int D, float* C, int64_t ldc, const float* thr,
                    uint8_t* gflag, hipStream_t st);

// Per-row running top-k over a score chunk.  sim: (M, Nc) with row stride ld; column j
// of the chunk is gallery row col_base + j.  carry: (M, k) u64 keys (canonical order,
// 0 = empty); read unless `first`, written unless `emit`.  With `emit` the final
// (score, idx_base + index) lists are written instead.
int launch_select(const float* sim, int64_t M, int64_t Nc, int64_t ld, int64_t col_base, int k, uint64_t* carry,
                  bool first, bool emit, int64_t idx_base, float* top_score, int64_t* top_idx, hipStream_t st,
                  float* thr_out = nullptr);

// Running top-k update from a FILTERED chunk: only the flagged 32-column groups are read from sim.  k <= kGroupSelectMaxK.  Updates carry and thr
// (thr[row] = score of the k-th key, -inf while fewer than k).
int launch_select_groups(const float* sim, const uint8_t* gflag, int64_t M, int64_t Nc, int64_t ld, int64_t col_base, int k,
                         uint64_t* carry, float* thr, int mode, int64_t idx_base, float* top_score, int64_t* top_idx,
                         hipStream_t st, const int* m_active = nullptr, const int* row_map = nullptr, const float* win = nullptr, int k_win = 0);
// mode 0: intermediate chunk (carry unsorted, k-th largest key in slot k-1), 1: last chunk, emit sorted lists, 2: last chunk, sorted carry.
// m_active / row_map (optional, device): only rows < *m_active are processed and row r emits to output row row_map[r].
// win / k_win (optional): the caller only needs candidates within win[row] of the final k_win-th best score (k_win < k); the threshold
// written for the next filter GEMM is then max(k-th best, current k_win-th best - win[row]).

constexpr int kGroupSelectMaxK = 256;

constexpr int kSelectMaxK = 1024;

// One chunked running-top-k search (cosine.hip).  fp32 operands (Q, G) or fp16 operands (Qh, Gh); with
// emit the final lists go to top_score / top_idx, otherwise the keys stay in the workspace (carry at
// ws + 0, thr after it).  Workspace layout: [carry M*k u64 | thr M f32 | flags | score chunk].
struct TopkJob {
    const char* who;
    const float* Q; const float* G;
    const _Float16* Qh; const _Float16* Gh;
    int64_t M, N; int D, k;
    int64_t idx_base; float* top_score; int64_t* top_idx; bool emit;
    void* ws; size_t ws_bytes; hipStream_t st;
    const int* m_active; const int* row_map;
    const float* win; int k_win;                  // optional window of interest below the k_win-th best score (see launch_select_groups)
};
int run_topk_chunks(const TopkJob& job);
size_t topk_fixed_bytes(int64_t M, int k);
size_t topk_chunk_bytes(int64_t M, int64_t nc);
int64_t topk_recommended_chunk(int64_t M, int64_t N);

}  // namespace isx
