// classif.hip -- the classifier tail of the classification fine-tuning step (pipeline stage 1):
//   * softmax cross-entropy, forward + analytic backward (reference train/classif_finetune.py:154 nn.CrossEntropyLoss, called once per
//     micro-batch from utils/train_general.py:51-61), per row and for all micro-batches ("leaves") of a step in one launch
//   * backward of the whole-map average pool in front of the classifier (reference model/siamese.py:20-23 AvgPool2d(7))
//   * per-leaf weight gradient of the classifier Linear (reference model/siamese.py:28-32)
// Every row is computed by one wave exactly as it would be alone; per-leaf sums run over the leaf's rows in row order.
#include "isx_common.hpp"

namespace isx {

__device__ __forceinline__ float wave_fmax(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// One wave on one row z[0 .. C): m = max_j z_j; s = sum_j exp(z_j - m), summed in this FIXED order: lane i adds its columns
// i, i + 64, i + 128, ... in ascending order from +0, then the 64 lane sums meet in the butterfly of wave_sum (xor 32, 16, 8, 4, 2, 1).
// Every lane returns the same (m, s).  On finite logits s >= 1 (the maximum contributes exp(0)), so log s is finite whatever their spread;
// -inf columns add exp(-inf) = +0 exactly.  fmaxf skips a NaN, but the NaN column's own term is NaN; +inf gives inf - inf, a row of -inf only
// gives -inf + inf: in all three s is NaN, and so are the row's loss and every element of its gradient.
__device__ __forceinline__ void xent_row_stats(const float* __restrict__ z, int C, int lane, float& m, float& s) {
    float mx = -INFINITY;
    for (int j = lane; j < C; j += 64) mx = fmaxf(mx, z[j]);
    m = wave_fmax(mx);
    float t = 0.0f;
    for (int j = lane; j < C; j += 64) t += expf(z[j] - m);
    s = wave_sum(t);
}

// loss = (log s + m) - z_label, in this grouping.  A label outside [0, C) is the caller's error (train_classif checks its label list on the host); the kernel reads
// nothing out of bounds for it and reports NaN.
__device__ __forceinline__ float xent_row_loss(const float* __restrict__ z, int C, int label, float m, float s) {
    if ((unsigned)label >= (unsigned)C) return __uint_as_float(0x7FC00000u);
    return logf(s) + m - z[label];
}

// dz_j = (exp(z_j - m) / s - [j == label]) * scale; a label outside [0, C) matches no column: the row is (exp(z_j - m) / s) * scale
__device__ __forceinline__ void xent_row_grad(const float* __restrict__ z, int C, int label, int lane, float m, float s, float scale,
                                              float* __restrict__ dz) {
    for (int j = lane; j < C; j += 64) {
        const float p = expf(z[j] - m) / s;
        dz[j] = (p - (j == label ? 1.0f : 0.0f)) * scale;
    }
}

__global__ __launch_bounds__(256) void xent_fwd_kernel(const float* __restrict__ z, const int32_t* __restrict__ lab, int64_t B, int C,
                                                       float* __restrict__ loss_rows) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    float m, s;
    xent_row_stats(z + b * C, C, lane, m, s);
    if (lane == 0) loss_rows[b] = xent_row_loss(z + b * C, C, lab[b], m, s);
}

__global__ __launch_bounds__(256) void xent_bwd_kernel(const float* __restrict__ z, const int32_t* __restrict__ lab, int64_t B, int C, float scale,
                                                       const float* __restrict__ scale_dev, float* __restrict__ dz) {
    if (scale_dev) scale = scale * scale_dev[0];          // grad_output left on the device (as triplet_bwd_kernel)
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    float m, s;
    xent_row_stats(z + b * C, C, lane, m, s);
    xent_row_grad(z + b * C, C, lab[b], lane, m, s, scale, dz + b * C);
}

// All leaves of a step: one workgroup per leaf, one wave per row in turn (rows wave, wave + 4, ...); the row's loss and gradient exactly as
// the two kernels above form them (scale = scale_a * scale_b, the product the per-leaf path forms from 1 / k and autograd's grad_output);
// the leaf's loss = its rows' losses added in row order by one thread.
__global__ __launch_bounds__(256) void xent_leaves_kernel(const float* __restrict__ z, const int32_t* __restrict__ lab, int k, int C, float scale_a,
                                                          float scale_b, float* __restrict__ loss_leaf, float* __restrict__ dz) {
    extern __shared__ float rows[];                                   // k row losses
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * k;
    const float scale = scale_a * scale_b;
    for (int r = wave; r < k; r += 4) {
        const float* zr = z + (base + r) * C;
        const int label = lab[base + r];
        float m, s;
        xent_row_stats(zr, C, lane, m, s);
        if (lane == 0) rows[r] = xent_row_loss(zr, C, label, m, s);
        xent_row_grad(zr, C, label, lane, m, s, scale, dz + (base + r) * C);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.0f;
        for (int r = 0; r < k; ++r) t += rows[r];
        loss_leaf[blockIdx.x] = t;
    }
}

// dx[b][p][c] = g[b][c] / HW for every pixel p of image b (channels-last map, C % 4 == 0): the pool spreads its gradient evenly.
__global__ __launch_bounds__(256) void gap_bwd_nhwc_kernel(const float4* __restrict__ g, int64_t total4, int HW, int C4, float hw,
                                                           float4* __restrict__ dx) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t pix = i / C4;
        const int c = (int)(i - pix * C4);
        const float4 v = g[(pix / HW) * C4 + c];
        dx[i] = make_float4(v.x / hw, v.y / hw, v.z / hw, v.w / hw);
    }
}

// Backward of the stride-1 box pool (boxpool_s1_nhwc_kernel of pool.hip), channels-last: g (B,Ho,Wo,C) -> dx (B,H,W,C).  Same layout as the
// forward: one workgroup per (image, slice of CS channels), the slice of the whole gradient map staged in LDS with 16-B loads, a thread owns 4
// consecutive channels of an INPUT pixel and adds the windows that cover it -- rows p ascending outside, columns q ascending inside, fp32 from
// +0 -- then divides ONCE by kh * kw (the forward forms s / div the same way).  No atomics, no dependence on other images.
__global__ __launch_bounds__(256) void boxpool_s1_bwd_nhwc_kernel(const float* __restrict__ g, int C, int H, int W, int kh, int kw, int CS,
                                                                  float* __restrict__ dx) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int Ho = H - kh + 1, Wo = W - kw + 1, HWi = H * W, HWo = Ho * Wo;
    const int q4 = CS >> 2;                                      // float4 per pixel of the slice
    const int c0 = blockIdx.x * CS;
    const float* src = g + (int64_t)blockIdx.y * HWo * C + c0;
    float4* l4 = reinterpret_cast<float4*>(lds);
    for (int i = threadIdx.x; i < HWo * q4; i += 256) {
        const int p = i / q4, cq = i - p * q4;
        l4[i] = *reinterpret_cast<const float4*>(src + (int64_t)p * C + cq * 4);
    }
    __syncthreads();
    const float div = (float)(kh * kw);
    float* dst = dx + (int64_t)blockIdx.y * HWi * C + c0;
    for (int o = threadIdx.x; o < HWi * q4; o += 256) {
        const int pix = o / q4, cq = o - pix * q4, i = pix / W, j = pix - i * W;
        const int p0 = i - kh + 1 > 0 ? i - kh + 1 : 0, p1 = i < Ho - 1 ? i : Ho - 1;
        const int q0 = j - kw + 1 > 0 ? j - kw + 1 : 0, q1 = j < Wo - 1 ? j : Wo - 1;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int p = p0; p <= p1; ++p)
            for (int q = q0; q <= q1; ++q) {
                const float4 v = l4[(p * Wo + q) * q4 + cq];
                s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            }
        *reinterpret_cast<float4*>(dst + (int64_t)pix * C + cq * 4) = make_float4(s.x / div, s.y / div, s.z / div, s.w / div);
    }
}

// dw[l][n][k] = sum_r dy[l R + r][n] * x[l R + r][k]: ONE fp32 fma chain from +0 over the leaf's rows in row order, never split.
// A thread owns 4 consecutive k of 4 consecutive n (16 chains); a block covers 16 n x 256 k of one leaf.  R is 8..64: R / 2 flop per byte
// written, and gfx950's fp32 MFMA rate equals its vector rate, so the chains run on the vector ALU, where fmaf IS the canonical chain,
// instead of in matrix instructions.  Measured 11-21 us per call at 1-8 leaves of 464 x 2048: launch-latency sized.
__global__ __launch_bounds__(256) void linear_wgrad_leaves_kernel(const float* __restrict__ dy, const float* __restrict__ x, int R, int N, int K,
                                                                  float* __restrict__ dw) {
    const int l = blockIdx.z;
    const int k0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    const int n0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * 4;
    if (k0 >= K || n0 >= N) return;
    const float* dyl = dy + (int64_t)l * R * N;
    const float* xl = x + (int64_t)l * R * K;
    const int nn = N - n0 < 4 ? N - n0 : 4;                 // N need not be a multiple of 4 (464 is; 311 is not)
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0f;
    for (int r = 0; r < R; ++r) {
        const float4 xv = *reinterpret_cast<const float4*>(xl + (int64_t)r * K + k0);
        float d[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) d[a] = a < nn ? dyl[(int64_t)r * N + n0 + a] : 0.0f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            acc[a][0] = __builtin_fmaf(d[a], xv.x, acc[a][0]);
            acc[a][1] = __builtin_fmaf(d[a], xv.y, acc[a][1]);
            acc[a][2] = __builtin_fmaf(d[a], xv.z, acc[a][2]);
            acc[a][3] = __builtin_fmaf(d[a], xv.w, acc[a][3]);
        }
    }
    float* out = dw + ((int64_t)l * N + n0) * K + k0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
        if (a < nn) *reinterpret_cast<float4*>(out + (int64_t)a * K) = make_float4(acc[a][0], acc[a][1], acc[a][2], acc[a][3]);
}

// Test hook: the expf and logf the kernels above call, one element per thread and trip -- this translation unit, these flags.
__global__ __launch_bounds__(256) void debug_expf_logf_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ e, float* __restrict__ l) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = x[i];
        if (e) e[i] = expf(v);
        if (l) l[i] = logf(v);
    }
}

}  // namespace isx

using namespace isx;

ISX_API int isx_softmax_xent_fwd(const float* logits, const int32_t* labels, int64_t B, int C, float* loss_rows, isx_stream_t stream) {
    ISX_REQUIRE(B >= 0 && C > 0 && B < (1ll << 31), "isx_softmax_xent_fwd: bad shape B=%lld C=%d", (long long)B, C);
    if (B == 0) return ISX_OK;
    ISX_REQUIRE(logits && labels && loss_rows, "isx_softmax_xent_fwd: null pointer");
    hipLaunchKernelGGL(xent_fwd_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits, labels, B, C, loss_rows);
    ISX_CHECK_LAUNCH("isx_softmax_xent_fwd");
    return ISX_OK;
}

ISX_API int isx_softmax_xent_bwd(const float* logits, const int32_t* labels, int64_t B, int C, float scale, const float* scale_dev,
                                 float* dlogits, isx_stream_t stream) {
    ISX_REQUIRE(B >= 0 && C > 0 && B < (1ll << 31), "isx_softmax_xent_bwd: bad shape B=%lld C=%d", (long long)B, C);
    if (B == 0) return ISX_OK;
    ISX_REQUIRE(logits && labels && dlogits && dlogits != logits, "isx_softmax_xent_bwd: null pointer or dlogits aliases logits");
    hipLaunchKernelGGL(xent_bwd_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits, labels, B, C, scale, scale_dev, dlogits);
    ISX_CHECK_LAUNCH("isx_softmax_xent_bwd");
    return ISX_OK;
}

ISX_API int isx_softmax_xent_leaves(const float* logits, const int32_t* labels, int leaves, int k, int C, float scale_a, float scale_b,
                                    float* loss_leaf, float* dlogits, isx_stream_t stream) {
    ISX_REQUIRE(leaves >= 0 && k > 0 && k <= 8192 && C > 0, "isx_softmax_xent_leaves: bad shape leaves=%d k=%d C=%d (k <= 8192)", leaves, k, C);
    if (leaves == 0) return ISX_OK;
    ISX_REQUIRE(logits && labels && loss_leaf && dlogits && dlogits != logits, "isx_softmax_xent_leaves: null pointer or dlogits aliases logits");
    hipLaunchKernelGGL(xent_leaves_kernel, dim3((unsigned)leaves), dim3(256), (size_t)k * sizeof(float), (hipStream_t)stream, logits, labels, k, C,
                       scale_a, scale_b, loss_leaf, dlogits);
    ISX_CHECK_LAUNCH("isx_softmax_xent_leaves");
    return ISX_OK;
}

ISX_API int isx_gap_bwd_nhwc(const float* g, int64_t B, int H, int W, int C, float* dx, isx_stream_t stream) {
    ISX_REQUIRE(B >= 0 && H > 0 && W > 0 && C > 0 && (int64_t)H * W < (1 << 24), "isx_gap_bwd_nhwc: bad shape B=%lld H=%d W=%d C=%d", (long long)B, H, W, C);
    ISX_REQUIRE(C % 4 == 0, "isx_gap_bwd_nhwc: C=%d must be a multiple of 4", C);
    if (B == 0) return ISX_OK;
    ISX_REQUIRE(g && dx && ((uintptr_t)g % 16 == 0) && ((uintptr_t)dx % 16 == 0), "isx_gap_bwd_nhwc: null or misaligned pointer (16 bytes)");
    const int64_t total4 = B * H * W * (C / 4);
    const unsigned grid = (unsigned)((total4 + 255) / 256 < 8192 ? (total4 + 255) / 256 : 8192);
    hipLaunchKernelGGL(gap_bwd_nhwc_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float4*)g, total4, H * W, C / 4, (float)(H * W), (float4*)dx);
    ISX_CHECK_LAUNCH("isx_gap_bwd_nhwc");
    return ISX_OK;
}

ISX_API int isx_boxpool_s1_bwd_nhwc(const float* g, int64_t B, int C, int H, int W, int kh, int kw, float* dx, isx_stream_t stream) {
    ISX_REQUIRE(B >= 0 && B < 65536 && C > 0 && H > 0 && W > 0 && kh > 0 && kw > 0 && kh <= H && kw <= W && (int64_t)H * W < (1 << 24),
                "isx_boxpool_s1_bwd_nhwc: bad shape B=%lld C=%d H=%d W=%d k=%dx%d", (long long)B, C, H, W, kh, kw);
    ISX_REQUIRE(C % 4 == 0, "isx_boxpool_s1_bwd_nhwc: C=%d must be a multiple of 4", C);
    if (B == 0) return ISX_OK;
    ISX_REQUIRE(g && dx && g != dx, "isx_boxpool_s1_bwd_nhwc: null or aliased pointer");
    ISX_REQUIRE((((uintptr_t)g | (uintptr_t)dx) % 16) == 0, "isx_boxpool_s1_bwd_nhwc: misaligned pointer (16 bytes)");
    const size_t HWo = (size_t)(H - kh + 1) * (W - kw + 1);
    int CS = 64;                                                  // channels per workgroup: the slice of the gradient map must fit 64 KB of LDS
    while (CS > 4 && (C % CS != 0 || HWo * CS * 4 > 64 * 1024)) CS >>= 1;
    ISX_REQUIRE(C % CS == 0 && HWo * CS * 4 <= 64 * 1024, "isx_boxpool_s1_bwd_nhwc: a %dx%d map does not fit the LDS staging", H, W);
    hipLaunchKernelGGL(boxpool_s1_bwd_nhwc_kernel, dim3((unsigned)(C / CS), (unsigned)B), dim3(256), HWo * CS * 4, (hipStream_t)stream, g, C, H, W, kh, kw,
                       CS, dx);
    ISX_CHECK_LAUNCH("isx_boxpool_s1_bwd_nhwc");
    return ISX_OK;
}

ISX_API int isx_linear_wgrad_leaves(const float* dy, const float* x, int leaves, int R, int N, int K, float* dw, isx_stream_t stream) {
    ISX_REQUIRE(leaves >= 0 && leaves <= 65535 && R > 0 && N > 0 && K > 0, "isx_linear_wgrad_leaves: bad shape leaves=%d R=%d N=%d K=%d", leaves, R, N, K);
    ISX_REQUIRE(K % 4 == 0, "isx_linear_wgrad_leaves: K=%d must be a multiple of 4", K);
    if (leaves == 0) return ISX_OK;
    ISX_REQUIRE(dy && x && dw && ((uintptr_t)x % 16 == 0) && ((uintptr_t)dw % 16 == 0), "isx_linear_wgrad_leaves: null or misaligned pointer (16 bytes)");
    const unsigned gy = (unsigned)((N + 15) / 16);
    ISX_REQUIRE(gy <= 65535, "isx_linear_wgrad_leaves: N=%d too large", N);
    hipLaunchKernelGGL(linear_wgrad_leaves_kernel, dim3((unsigned)((K + 255) / 256), gy, (unsigned)leaves), dim3(256), 0, (hipStream_t)stream, dy, x, R, N, K, dw);
    ISX_CHECK_LAUNCH("isx_linear_wgrad_leaves");
    return ISX_OK;
}

ISX_API int isx_debug_expf_logf(const float* x, int64_t n, float* e, float* l, isx_stream_t stream) {
    ISX_REQUIRE(n >= 0, "isx_debug_expf_logf: bad shape n=%lld", (long long)n);
    if (n == 0) return ISX_OK;
    ISX_REQUIRE(x, "isx_debug_expf_logf: null pointer");
    const unsigned grid = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(debug_expf_logf_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, n, e, l);
    ISX_CHECK_LAUNCH("isx_debug_expf_logf");
    return ISX_OK;
}
