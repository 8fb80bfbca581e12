// cosine.hip -- query x gallery cosine similarity on the fp32 matrix cores.
//
// Replaces  sim = torch.mm(test_emb, ref_emb.t())  (test/classif_finetune_test.py:82,
// classif_regions_test.py:73, siamese_descriptor_test.py:77, siamese_regions_test.py:76,
// utils/train_siamese.py:53,70) and, fused with select.hip, the sort/topk/max that the
// reference runs on that matrix (utils/metrics.py:10-13,33).
//
// The GEMM itself and its filtering epilogue live in gemm.hip; this file holds the chunked running-top-k driver (run_topk_chunks),
// which serves isx_cosine_topk and both phases of fast.hip, and the isx_cosine_* entry points.
#include "isx_internal.hpp"

namespace isx {

// Workspace layout of isx_cosine_topk:
//   [ carry keys: M*k u64 | thr: M f32 | group flags: M*ceil(Nc/32) u8 | score chunk: M*Nc f32 ]
// The first column chunk (<= kFirstChunk columns) is materialised and selected in full; it leaves a
// per-row lower bound thr of the final k-th score.  Every later chunk runs the FILTERING GEMM: only
// 32-column groups whose best score reaches thr are stored and read back, so for typical data the
// M x N matrix is never written -- just one float per 32 scores.  Exact for any data: in the worst
// case (every group qualifies) the chunk is simply materialised in full, as in round 0.
constexpr int64_t kFirstChunk = 8192;
constexpr size_t kChunkBudget = (size_t)1 << 30;          // score-chunk budget of topk_recommended_chunk: 1 GiB
static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// ---- zero fill (isx_internal.hpp: the library's replacement of hipMemsetAsync) --------------------
template <typename T> __global__ __launch_bounds__(256) void zero_fill_kernel(T* __restrict__ p, size_t n) {
    T z;
    __builtin_memset(&z, 0, sizeof(T));
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = z;
}

int zero_words_async(void* p, size_t bytes, hipStream_t st, const char* who) {
    if (bytes == 0) return ISX_OK;
    if (!p || bytes % 4 || (uintptr_t)p % 4) {
        isx_set_error("%s: zero fill of %zu bytes at a pointer that is null or off a 4-byte boundary", who, bytes);
        return ISX_ERR_ARG;
    }
    const bool wide = (uintptr_t)p % 16 == 0 && bytes % 16 == 0;              // 16-byte stores where the range allows them
    const size_t n = bytes / (wide ? 16 : 4), blocks = (n + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 4096 ? blocks : 4096);          // grid-stride beyond 1 Mi elements
    if (wide) hipLaunchKernelGGL(zero_fill_kernel<uint4>, dim3(grid), dim3(256), 0, st, (uint4*)p, n);
    else hipLaunchKernelGGL(zero_fill_kernel<uint32_t>, dim3(grid), dim3(256), 0, st, (uint32_t*)p, n);
    ISX_CHECK_LAUNCH(who);
    return ISX_OK;
}

// ---- chunked running top-k driver (shared by isx_cosine_topk and the fast path of fast.hip) ------
size_t topk_fixed_bytes(int64_t M, int k) { return align256((size_t)M * k * 8) + align256((size_t)M * 4); }
size_t topk_chunk_bytes(int64_t M, int64_t nc) { return align256((size_t)M * ((nc + 31) / 32)) + (size_t)M * nc * 4; }

int64_t topk_recommended_chunk(int64_t M, int64_t N) {
    // whole matrix if it is <= 1 GiB, else column chunks of ~1 GiB (multiple of 2048 columns)
    int64_t nc = N;
    if ((size_t)M * N * 4 > kChunkBudget) {
        nc = (int64_t)(kChunkBudget / ((size_t)M * 4));
        nc = nc / 2048 * 2048;
        if (nc < 2048) nc = 2048;
        if (nc > N) nc = N;
    }
    return nc;
}

int run_topk_chunks(const TopkJob& j) {
    const int64_t M = j.M, N = j.N;
    const int k = j.k, D = j.D;
    hipStream_t st = j.st;
    const size_t fixed_b = topk_fixed_bytes(M, k);
    const int64_t min_nc = N < 128 ? N : 128;
    if (!j.ws || ((uintptr_t)j.ws % 256) != 0 || j.ws_bytes < fixed_b + topk_chunk_bytes(M, min_nc)) {
        isx_set_error("%s: workspace of %zu bytes too small or misaligned (need >= %zu, 256-B aligned)", j.who, j.ws_bytes,
                      fixed_b + topk_chunk_bytes(M, min_nc));
        return ISX_ERR_WORKSPACE;
    }
    // largest chunk width (multiple of 128 unless it covers N) whose flags + scores fit
    int64_t nc = (int64_t)((j.ws_bytes - fixed_b) / ((size_t)M * 4));
    if (nc > N) nc = N;
    // (never below min_nc, which the check above has shown to fit: a workspace a few bytes above the minimum starts at nc = 128 + a few and
    // used to step down to chunks of those few columns)
    while (nc > min_nc && topk_chunk_bytes(M, nc) > j.ws_bytes - fixed_b) {
        nc -= (nc > 4096 ? 1024 : 128);
        if (nc < min_nc) nc = min_nc;
    }
    if (nc < N) nc = nc >= 128 ? nc / 128 * 128 : nc;
    if (nc < N && nc >= 4096) {
        // a chunk launch runs ceil(tiles / slots) lock-step rounds of tiles (fp32: 128x128, 512 resident at the
        // filter kernel's 2 workgroups per CU ... measured best with 512; fp16: 256x256, one per CU): trim the width
        // (by at most 16 tiles) so that the last round is >= 90 % full
        const int64_t tile = j.Qh ? 256 : 128, slots = j.Qh ? 256 : 512;
        const int64_t tm_ = (M + tile - 1) / tile;
        for (int64_t tn = nc / tile, tries = 0; tries < 16 && tn > 16; --tn, ++tries) {
            const int64_t rem = (tm_ * tn) % slots;
            if (rem == 0 || rem >= slots * 9 / 10) { nc = tn * tile; break; }
        }
    }
    uint64_t* carry = (uint64_t*)j.ws;
    float* thr = (float*)((char*)j.ws + align256((size_t)M * k * 8));
    uint8_t* gflag = (uint8_t*)((char*)j.ws + fixed_b);
    float* chunk = (float*)((char*)gflag + align256((size_t)M * ((nc + 31) / 32)));
    const bool filter = (k <= kGroupSelectMaxK);
    if (!filter && (j.Qh || !j.emit || j.m_active)) { isx_set_error("%s: k=%d unsupported on this path", j.who, k); return ISX_ERR_ARG; }
    auto gemm = [&](int64_t c0, int64_t w, const float* t, uint8_t* gf) -> int {
        if (j.Qh) return launch_gemm_f16(j.Qh, M, j.Gh + c0 * D, w, D, chunk, w, t, gf, st);
        if (gf) return launch_cosine_gemm_filter(j.Q, M, j.G + c0 * D, w, D, chunk, w, t, gf, st, j.m_active);
        return launch_cosine_gemm(j.Q, M, j.G + c0 * D, w, D, chunk, w, st, j.m_active);
    };
    int64_t c0 = 0;
    while (c0 < N) {
        const bool first = (c0 == 0);
        int64_t w = N - c0 < nc ? N - c0 : nc;
        if (first && filter && w > kFirstChunk && N >= 4 * kFirstChunk) w = kFirstChunk;   // short bootstrap chunk
        const bool last = (c0 + w >= N);
        const bool emit = last && j.emit;
        int rc;
        if (!filter) {
            rc = gemm(c0, w, nullptr, nullptr);
            if (rc) return rc;
            rc = launch_select(chunk, M, w, w, c0, k, carry, first, last, j.idx_base, j.top_score, j.top_idx, st, thr);
        } else if (first) {
            // bootstrap chunk: plain GEMM, every group present, empty carry (all-zero keys sort last)
            rc = gemm(c0, w, nullptr, nullptr);
            if (rc) return rc;
            rc = zero_words_async(carry, (size_t)M * k * 8, st, j.who);
            if (rc) return rc;
            rc = launch_select_groups(chunk, nullptr /* all groups present */, M, w, w, c0, k, carry, thr, emit ? 1 : (last ? 2 : 0), j.idx_base, j.top_score,
                                      j.top_idx, st, j.m_active, j.row_map, j.win, j.k_win);
        } else {
            rc = gemm(c0, w, thr, gflag);
            if (rc) return rc;
            rc = launch_select_groups(chunk, gflag, M, w, w, c0, k, carry, thr, emit ? 1 : (last ? 2 : 0), j.idx_base, j.top_score, j.top_idx, st, j.m_active,
                                      j.row_map, j.win, j.k_win);
        }
        if (rc) return rc;
        c0 += w;
    }
    return ISX_OK;
}

}  // namespace isx

using namespace isx;


ISX_API int isx_cosine_sim(const float* Q, int64_t M, const float* G, int64_t N, int D, float* sim, isx_stream_t stream) {
    ISX_REQUIRE(M >= 0 && N >= 0 && D > 0, "isx_cosine_sim: bad shape M=%lld N=%lld D=%d", (long long)M, (long long)N, D);
    ISX_REQUIRE((Q && G && sim) || M * N == 0, "isx_cosine_sim: null pointer");
    return launch_cosine_gemm(Q, M, G, N, D, sim, N, (hipStream_t)stream);
}

ISX_API size_t isx_cosine_topk_workspace(int64_t M, int64_t N, int D, int k) {
    (void)D;
    if (M <= 0 || N <= 0 || k <= 0) return 256;
    return topk_fixed_bytes(M, k) + topk_chunk_bytes(M, topk_recommended_chunk(M, N));
    // minimum accepted by isx_cosine_topk: the same formula with nc = min(N, 128)
}

ISX_API int isx_cosine_topk(const float* Q, int64_t M, const float* G, int64_t N, int D, int k, int64_t idx_base,
                            float* top_score, int64_t* top_idx, void* ws, size_t ws_bytes, isx_stream_t stream) {
    ISX_REQUIRE(M >= 0 && N >= 0 && D > 0, "isx_cosine_topk: bad shape M=%lld N=%lld D=%d", (long long)M, (long long)N, D);
    ISX_REQUIRE(k >= 1 && k <= kSelectMaxK, "isx_cosine_topk: k=%d outside [1,%d]", k, kSelectMaxK);
    ISX_REQUIRE(idx_base >= 0 && idx_base + N <= 0xFFFFFFFFll && N <= 0x7FFFFFFFll, "isx_cosine_topk: gallery indices must stay below 2^32");
    if (M == 0) return ISX_OK;
    ISX_REQUIRE(Q && top_score && top_idx && (G || N == 0), "isx_cosine_topk: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) return launch_select(nullptr, M, 0, 0, 0, k, nullptr, true, true, idx_base, top_score, top_idx, st);
    TopkJob j{};
    j.who = "isx_cosine_topk";
    j.Q = Q; j.G = G; j.M = M; j.N = N; j.D = D; j.k = k;
    j.idx_base = idx_base; j.top_score = top_score; j.top_idx = top_idx; j.emit = true;
    j.ws = ws; j.ws_bytes = ws_bytes; j.st = st;
    return run_topk_chunks(j);
}

