// prep.hip -- libisxprep.so (include/isx_prep.h): exact per-channel moments of uint8 RGB images, the device half of create_mean_std_file.py.
//
// One launch, isxp_channel_moments_u8: grid (chunks per image, B), 192 threads.  An image is 3 H W bytes at any alignment:
//
//   head   the bytes in front of the first 16-byte boundary (at most 15)            byte loads, workgroup 0 of the image
//   body   whole GROUPS of 48 bytes = lcm(3, 16) = 16 pixels = three 16-byte PIECES    one 16-byte load per piece, fully coalesced
//   tail   what is left behind the last group (at most 47 bytes)                     byte loads, workgroup 0 of the image
//
// A workgroup owns a contiguous run of groups and thread t reads pieces 3 g0 + t, + 192, + 384, ...: 192 = 3 x 64, so (piece index) mod 3 is
// t mod 3 for every piece of a thread, and byte j of a piece has channel (head + piece + j) mod 3 -- the thread sums by j mod 3 with constant
// byte masks (v_dot4_u32_u8: one for the sum, one for the sum of squares per dword and class) and renames the three classes to channels once,
// at the end.  Four independent loads are in flight per thread (64 B per lane; at the 5 waves per SIMD its 81 VGPRs allow, 80 KiB per CU: the kernel has
// no other way to hide HBM latency, it does ~2 VALU operations per byte).
//
// Exactness: a class holds at most 6 bytes of a piece, so a piece adds at most 6 x 255^2 = 390 150 to a 32-bit partial; the partials move to
// 64-bit accumulators every kFlush = 32 pieces (at most 1.25e7 < 2^32).  Everything after that -- wave butterfly, the three wave sums in LDS,
// one atomic add per workgroup and moment into the zeroed output -- is 64-bit integer addition, which has no order: the result does not depend
// on the grid, and the largest accepted image (sum of squares < 2^31 / 3 x 65 025 = 4.7e13) is far inside int64.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/isx_prep.h"

#define ISXP_API extern "C" __attribute__((visibility("default")))

static thread_local char g_err[256] = "";

static int fail(int rc, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return rc;
}

ISXP_API const char* isxp_last_error(void) { return g_err; }
ISXP_API int isxp_version(void) { return 100; }

namespace {

constexpr int kThreads = 192;                  // 3 waves: a thread's pieces keep their channel phase (header)
constexpr int kFlush = 32;                     // pieces per thread between two flushes of the 32-bit partials (header)
constexpr int kTargetBlocks = 4096;            // 16 workgroups per CU: small batches are cut into chunks until the grid has about this many ...
constexpr int kMinGroups = 256;                // ... but a chunk keeps at least 4 pieces per thread (12 KiB per workgroup)

// Bytes q of dword m of a piece whose index in the piece, 4 m + q, is k mod 3: 0xFF there (sel = 0xFF) or 0x01 there (sel = 0x01).
constexpr uint32_t class_bytes(int m, int k, uint32_t sel) {
    uint32_t v = 0;
    for (int q = 0; q < 4; ++q)
        if ((4 * m + q) % 3 == k) v |= sel << (8 * q);
    return v;
}

__device__ __forceinline__ void add_piece(const uint4& v, uint32_t (&a1)[3], uint32_t (&a2)[3]) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a1[k] = __builtin_amdgcn_udot4(w[m], class_bytes(m, k, 0x01), a1[k], false);
            a2[k] = __builtin_amdgcn_udot4(w[m] & class_bytes(m, k, 0xFF), w[m], a2[k], false);
        }
    }
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The output is zeroed by a kernel, not by hipMemsetAsync: captured into a hipGraph, the memset node zeroes on the first replay only and fills
// with stale bits on every later one (ROCm 7.0; tests/test_gpu_graph_capture.py::test_captured_and_replayed[prep_channel_moments_u8]).
__global__ __launch_bounds__(256) void zero_moments_kernel(unsigned long long* __restrict__ moments, int n) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i < n) moments[i] = 0;
}

__global__ __launch_bounds__(kThreads) void channel_moments_kernel(const uint8_t* __restrict__ img, int64_t N, int gpc,
                                                                   unsigned long long* __restrict__ moments) {
    __shared__ unsigned long long part[kThreads / 64][6];
    const int t = threadIdx.x;
    const uint8_t* p = img + (int64_t)blockIdx.y * N;
    const int64_t to_boundary = (int64_t)((16 - ((uintptr_t)p & 15)) & 15);
    const int head = (int)(to_boundary < N ? to_boundary : N);
    const int G = (int)((N - head) / 48);                     // whole groups of this image
    const int g0 = (int)blockIdx.x * gpc;
    const int g1 = g0 + gpc < G ? g0 + gpc : G;
    if (blockIdx.x != 0 && g0 >= g1) return;                  // nothing left for this chunk (the whole workgroup leaves)

    // ---- body: sums by byte class j mod 3 ----
    unsigned long long s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0};
    const uint4* body = reinterpret_cast<const uint4*>(p + head);
    const int end = 3 * g1;                                   // pieces [3 g0, 3 g1): byte offsets < 48 G <= N - head
    int i = 3 * g0 + t;
    while (i < end) {
        uint32_t a1[3] = {0, 0, 0}, a2[3] = {0, 0, 0};
        const int stop = end - i < kFlush * kThreads ? end : i + kFlush * kThreads;
        for (; i + 3 * kThreads < stop; i += 4 * kThreads) {
            const uint4 v0 = body[i], v1 = body[i + kThreads], v2 = body[i + 2 * kThreads], v3 = body[i + 3 * kThreads];
            add_piece(v0, a1, a2);
            add_piece(v1, a1, a2);
            add_piece(v2, a1, a2);
            add_piece(v3, a1, a2);
        }
        for (; i < stop; i += kThreads) add_piece(body[i], a1, a2);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s1[k] += a1[k];
            s2[k] += a2[k];
        }
    }
    // class k of this thread is channel (head + t + k) mod 3
    const int ph = (head + t) % 3;
    unsigned long long c[6];                                  // [channel][moment]
    c[0] = ph == 0 ? s1[0] : ph == 1 ? s1[2] : s1[1];
    c[1] = ph == 0 ? s2[0] : ph == 1 ? s2[2] : s2[1];
    c[2] = ph == 0 ? s1[1] : ph == 1 ? s1[0] : s1[2];
    c[3] = ph == 0 ? s2[1] : ph == 1 ? s2[0] : s2[2];
    c[4] = ph == 0 ? s1[2] : ph == 1 ? s1[1] : s1[0];
    c[5] = ph == 0 ? s2[2] : ph == 1 ? s2[1] : s2[0];

    // ---- head and tail bytes: workgroup 0, one byte per thread ----
    if (blockIdx.x == 0) {
        const int64_t tail_at = (int64_t)head + 48ll * G;
        const int tail = (int)(N - tail_at);                  // < 48
        int64_t at = -1;
        if (t < head) at = t;
        else if (t - head < tail) at = tail_at + (t - head);  // head + tail <= 62 threads
        if (at >= 0) {
            const unsigned long long v = p[at];
            const int ch = (int)(at % 3);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                c[2 * k] += ch == k ? v : 0;
                c[2 * k + 1] += ch == k ? v * v : 0;
            }
        }
    }

    // ---- workgroup sum, one atomic per moment ----
#pragma unroll
    for (int k = 0; k < 6; ++k) c[k] = wave_sum_u64(c[k]);
    if ((t & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) part[t >> 6][k] = c[k];
    }
    __syncthreads();
    if (t < 6) {
        unsigned long long v = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) v += part[w][t];
        atomicAdd(moments + (int64_t)blockIdx.y * 6 + t, v);
    }
}

}  // namespace

ISXP_API int isxp_channel_moments_u8(const uint8_t* img, int64_t B, int H, int W, int64_t* moments, isxp_stream_t stream) {
    if (H < 1 || W < 1 || B < 0 || B > 65535)
        return fail(ISXP_ERR_ARG, "isxp_channel_moments_u8: bad shape B=%lld H=%d W=%d (H, W >= 1, 0 <= B <= 65535)", (long long)B, H, W);
    const int64_t N = 3 * (int64_t)H * W;
    if (N >= (1ll << 31)) return fail(ISXP_ERR_ARG, "isxp_channel_moments_u8: image too large: 3 H W = %lld, needs < 2^31", (long long)N);
    if (B == 0) return ISXP_OK;
    if (!img || !moments) return fail(ISXP_ERR_ARG, "isxp_channel_moments_u8: null pointer (img, moments)");
    if ((uintptr_t)moments % 8) return fail(ISXP_ERR_ARG, "isxp_channel_moments_u8: moments must be 8-B aligned");
    hipStream_t st = (hipStream_t)stream;
    const int n_mom = (int)B * 6;                             // B <= 65535
    hipLaunchKernelGGL(zero_moments_kernel, dim3((unsigned)((n_mom + 255) / 256)), dim3(256), 0, st, reinterpret_cast<unsigned long long*>(moments), n_mom);
    const hipError_t ez = hipGetLastError();
    if (ez != hipSuccess) return fail(ISXP_ERR_HIP, "isxp_channel_moments_u8: zero fill failed: %s", hipGetErrorString(ez));
    const int64_t groups = N / 48;
    int64_t chunks = (kTargetBlocks + B - 1) / B;
    const int64_t most = (groups + kMinGroups - 1) / kMinGroups;
    if (chunks > most) chunks = most;
    if (chunks < 1) chunks = 1;
    int64_t gpc = (groups + chunks - 1) / chunks;             // groups per chunk: chunks x gpc >= groups
    if (gpc < 1) gpc = 1;
    hipLaunchKernelGGL(channel_moments_kernel, dim3((unsigned)chunks, (unsigned)B), dim3(kThreads), 0, st, img, N, (int)gpc,
                       reinterpret_cast<unsigned long long*>(moments));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ISXP_ERR_HIP, "isxp_channel_moments_u8: launch failed: %s", hipGetErrorString(e));
    return ISXP_OK;
}
