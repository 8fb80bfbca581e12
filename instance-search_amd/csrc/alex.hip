// alex.hip -- libisxalex.so (include/isx_alex.h): the convolutions and pools of an AlexNet-style `features` trunk that libisx has no kernel for.
//
//   isxa_conv2d_nhwc       square K x K convolution, any stride / padding / Cin, channels-last, as an implicit GEMM on the fp32 matrix cores:
//                          M = B Ho Wo output pixels, N = Cout, the reduction K K Cin in (kh, kw, ci) order.  The tile kernel is the staged k loop of
//                          gemm_tile.hpp (staged_kloop: the two-level sum in chunks of 64 terms, the K-major LDS images, the buffer-store epilogue) --
//                          the loop isx_conv3x3_nhwc runs -- behind an operand gather of its own:
//                            A   a staging lane owns rows (output pixels) and four consecutive k of every k-tile.  Its position in the flattened
//                                reduction, (tap = kh K + kw, ci), advances by a k-tile with one add and one compare (BK = q Cin + r, from the host);
//                                a table of the K K taps in LDS gives (kh, kw, offset in x).  A tap outside the image -- the padding -- loads nothing
//                                and stages 0: fma(0, w, acc).  Cin % 4 == 0: the four k are one pixel's 16 aligned bytes, one global_load_dwordx4;
//                                otherwise (Cin = 3, the first layer) four decodes and four dword loads.  All addresses are 64-bit.
//                            B   the weight matrix (Cout, K K Cin) row-major through load_tile: the k past K K Cin in the last k-tile load zeros.
//                          Terms past K K Cin have zero weight AND zero activation: fma(0, 0, acc) = acc -- the chain's value is untouched (a chain
//                          that is -0 becomes +0, which tot = tot + chain cannot tell apart).
//                          Tiles: 128x128 (BK 16) where Cout % 128 == 0 and the grid fills the chip, else 128x64 (BK 32), 64x64 (BK 32) for small
//                          launches -- by the launch's size alone; the sum of an output does not depend on the tile, nor on B.
//   isxa_maxpool3s2_nhwc   one lane per (output pixel, four channels): nine 16-byte loads, torch's CPU comparison, one 16-byte store.
//
// Reference call sites: torchvision's AlexNet `features` (utils/general.py:39-44 admits alexnet | resnet152) and the reference's clone of it,
// model/ModelDefinition.py:13-45, run from model/siamese.py:20,107,151.
#include <stdarg.h>

#include "gemm_tile.hpp"
#include "../../include/isx_alex.h"

#define ISXA_API extern "C" __attribute__((visibility("default")))

static_assert(ISXA_CONV_CHUNK == ISX_CONV_CHUNK, "one canonical convolution sum");

static thread_local char g_err[256] = "";

static int fail(int rc, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return rc;
}

ISXA_API const char* isxa_last_error(void) { return g_err; }
ISXA_API int isxa_version(void) { return 100; }

namespace {

using namespace isx;

constexpr int kMaxTaps = ISXA_MAX_K * ISXA_MAX_K;
constexpr int kDeadTap = 1 << 24;               // kh of the table entry past the last tap: outside any image (H <= 2^20)

struct ConvGeom {
    int H, W, Cin, Ho, Wo, K, stride, pad;
    int Kred;                                   // K K Cin
    int step_tap, step_ci;                      // BK = step_tap Cin + step_ci
    int64_t M;                                  // B Ho Wo
};

// Where a staging lane stands in the flattened reduction, and one k-tile further.
struct KPos {
    int tap, ci;
    __device__ __forceinline__ void advance(const ConvGeom& g) {
        tap += g.step_tap;
        ci += g.step_ci;
        if (ci >= g.Cin) {
            ci -= g.Cin;
            ++tap;
        }
    }
};

template <int TM, int TN, int BK, bool VEC4, bool WALIGNED>
__global__ __launch_bounds__(256, TM * TN == 4 ? 2 : TM * TN == 2 ? 3 : 4) void conv2d_nhwc_kernel(const float* __restrict__ x, const float* __restrict__ Wt, int N, ConvGeom g,
                                                                                 float* __restrict__ y, TileMap tm, const float* __restrict__ bias, int relu) {
    constexpr int BM = 64 * TM, BN = 64 * TN, LDA = BM + lds_pad(BK), LDB = BN + lds_pad(BK);
    constexpr int CH = BK / 4, NA = BM * CH / 256;
    __shared__ float lds[BK * (LDA + LDB)];
    __shared__ int s_kh[kMaxTaps + 1], s_kw[kMaxTaps + 1], s_off[kMaxTaps + 1];
    float* As = lds;
    float* Bs = lds + BK * LDA;

    int tile_m, tile_n;
    tile_of_block(tm, tile_m, tile_n);
    const int64_t m0 = (int64_t)tile_m * BM, n0 = (int64_t)tile_n * BN, M = g.M;

    // ---- the taps: (kh, kw) and the offset of x[.][kh][kw][0] from the window's first element; entry K K = no tap (k past the reduction) ----
    const int KK = g.K * g.K;
    for (int t = threadIdx.x; t <= KK; t += 256) {
        const int kh = t / g.K, kw = t - kh * g.K;
        s_kh[t] = t < KK ? kh : kDeadTap;
        s_kw[t] = t < KK ? kw : 0;
        s_off[t] = t < KK ? (kh * g.W + kw) * g.Cin : 0;           // < K (W + 1) Cin < 2^31 (host)
    }

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, half = lane >> 5;

    // ---- the rows of this staging lane: row = j (256 / CH) + threadIdx.x / CH; rows past M repeat the last one (never stored) ----
    int64_t rbase[NA];
    int hi0[NA], wi0[NA];
    const int64_t P = (int64_t)g.Ho * g.Wo;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        int64_t m = m0 + (j * 256 + (int)threadIdx.x) / CH;
        m = m < M ? m : M - 1;
        const int64_t b = m / P;
        const int rem = (int)(m - b * P);
        const int ho = rem / g.Wo, wo = rem - ho * g.Wo;
        hi0[j] = ho * g.stride - g.pad;
        wi0[j] = wo * g.stride - g.pad;
        rbase[j] = ((b * g.H + hi0[j]) * (int64_t)g.W + wi0[j]) * g.Cin;          // the window's first element; read only where the tap is inside
    }
    const int c4 = ((int)threadIdx.x % CH) << 2;                                    // this lane's four k of a k-tile: k0 + c4 ..
    KPos pos[VEC4 ? 1 : 4];
#pragma unroll
    for (int i = 0; i < (VEC4 ? 1 : 4); ++i) {
        pos[i].tap = (c4 + i) / g.Cin;
        pos[i].ci = (c4 + i) - pos[i].tap * g.Cin;
    }
    __syncthreads();                                                                // the tap table

    float4 ra[NA], rb[BN * BK / 1024];
    auto load_a = [&]() {                                                           // the k-tile the positions stand at; then one k-tile on
        if constexpr (VEC4) {
            const int tp = pos[0].tap < KK ? pos[0].tap : KK;
            const int kh = s_kh[tp], kw = s_kw[tp], off = s_off[tp] + pos[0].ci;
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                const bool ok = (unsigned)(hi0[j] + kh) < (unsigned)g.H && (unsigned)(wi0[j] + kw) < (unsigned)g.W;
                ra[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ok) ra[j] = *reinterpret_cast<const float4*>(x + (rbase[j] + off));
            }
            pos[0].advance(g);
        } else {
            float v[NA][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int tp = pos[i].tap < KK ? pos[i].tap : KK;
                const int kh = s_kh[tp], kw = s_kw[tp], off = s_off[tp] + pos[i].ci;
#pragma unroll
                for (int j = 0; j < NA; ++j) {
                    const bool ok = (unsigned)(hi0[j] + kh) < (unsigned)g.H && (unsigned)(wi0[j] + kw) < (unsigned)g.W;
                    v[j][i] = 0.f;
                    if (ok) v[j][i] = x[rbase[j] + off];
                }
                pos[i].advance(g);
            }
#pragma unroll
            for (int j = 0; j < NA; ++j) ra[j] = make_float4(v[j][0], v[j][1], v[j][2], v[j][3]);
        }
    };

    f32x16 acc[TM][TN], tot[TM][TN];
    zero_tiles(acc);
    zero_tiles(tot);
    const int nk = (g.Kred + BK - 1) / BK;
    load_a();
    load_tile<WALIGNED, BN, BK>(Wt, N, g.Kred, n0, 0, rb);
    store_tile<BM, BK>(As, ra);
    store_tile<BN, BK>(Bs, rb);
    __syncthreads();

    const float* a_base = As + half * LDA + wm * (32 * TM) + l31;
    const float* b_base = Bs + half * LDB + wn * (32 * TN) + l31;
    staged_kloop<TM, TN, BK, kConvChunk>(a_base, b_base, nk, acc, tot,
        [&](int kt) {
            load_a();
            load_tile<WALIGNED, BN, BK>(Wt, N, g.Kred, n0, kt * BK, rb);
        },
        [&]() {
            store_tile<BM, BK>(As, ra);
            store_tile<BN, BK>(Bs, rb);
        });

    const int wm_u = __builtin_amdgcn_readfirstlane(wm), wn_u = __builtin_amdgcn_readfirstlane(wn);
    conv_epilogue_buffers<TM, TN, TM * TN < 4 ? 1 : 2>(acc, y, nullptr, bias, relu, m0, M, n0, N, N, BM, wm_u * (32 * TM), wn_u * (32 * TN), l31, half);
}

template <int TM, int TN, int BK>
void launch_conv2d(const float* x, const float* w, int N, ConvGeom g, float* y, const float* bias, int relu, hipStream_t st) {
    TileMap tm;
    tm.m_active = nullptr;
    tm.tiles_m = (int)((g.M + 64 * TM - 1) / (64 * TM));
    tm.tiles_n = (N + 64 * TN - 1) / (64 * TN);
    g.step_tap = BK / g.Cin;
    g.step_ci = BK - g.step_tap * g.Cin;
    const dim3 grid((unsigned)(tm.tiles_m * tm.tiles_n));
    const bool vec4 = g.Cin % 4 == 0, waligned = g.Kred % BK == 0;
    if (vec4 && waligned) hipLaunchKernelGGL((conv2d_nhwc_kernel<TM, TN, BK, true, true>), grid, dim3(256), 0, st, x, w, N, g, y, tm, bias, relu);
    else if (vec4) hipLaunchKernelGGL((conv2d_nhwc_kernel<TM, TN, BK, true, false>), grid, dim3(256), 0, st, x, w, N, g, y, tm, bias, relu);
    else hipLaunchKernelGGL((conv2d_nhwc_kernel<TM, TN, BK, false, false>), grid, dim3(256), 0, st, x, w, N, g, y, tm, bias, relu);
}

// torch's CPU max-pool comparison (aten/src/ATen/native/cpu/MaxPoolKernel.cpp): a NaN replaces anything, a larger value replaces a smaller one
__device__ __forceinline__ void pool_take(float& m, float v) {
    if (v > m || v != v) m = v;
}

__global__ __launch_bounds__(256) void maxpool3s2_nhwc_kernel(const float4* __restrict__ x, int H, int W, int C4, int Ho, int Wo, int64_t total, float4* __restrict__ y) {
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
        const int64_t p = i / C4;
        const int c = (int)(i - p * C4);
        const int64_t q = p / Wo;
        const int wo = (int)(p - q * Wo);
        const int64_t b = q / Ho;
        const int ho = (int)(q - b * Ho);
        const float4* win = x + (((b * H + 2 * ho) * (int64_t)W + 2 * wo) * C4 + c);       // rows 2 ho .. 2 ho + 2 <= H - 1, columns likewise
        float4 v[9];
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) v[kh * 3 + kw] = win[((int64_t)kh * W + kw) * C4];
        float4 m = v[0];
#pragma unroll
        for (int t = 1; t < 9; ++t) {
            pool_take(m.x, v[t].x);
            pool_take(m.y, v[t].y);
            pool_take(m.z, v[t].z);
            pool_take(m.w, v[t].w);
        }
        y[i] = m;
    }
}

}  // namespace

ISXA_API int isxa_conv2d_nhwc(const float* x, int64_t B, int H, int W, int Cin, const float* w_ohwi, int Cout, int K, int stride, int pad,
                              const float* bias, int relu, float* y, isxa_stream_t stream) {
    const int lim = 1 << 20;
    if (B < 0 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || K < 1 || K > ISXA_MAX_K || stride < 1 || stride > 4 || pad < 0 || pad >= K || H > lim ||
        W > lim || Cin > lim || Cout > lim || Cout % 32 != 0)
        return fail(ISXA_ERR_ARG, "isxa_conv2d_nhwc: bad shape B=%lld H=%d W=%d Cin=%d Cout=%d K=%d stride=%d pad=%d (B >= 0; 1 <= H, W, Cin, Cout <= 2^20; "
                    "Cout %% 32 == 0; 1 <= K <= %d; 1 <= stride <= 4; 0 <= pad < K)", (long long)B, H, W, Cin, Cout, K, stride, pad, ISXA_MAX_K);
    if (H + 2 * pad < K || W + 2 * pad < K)
        return fail(ISXA_ERR_ARG, "isxa_conv2d_nhwc: bad shape: no output, H=%d W=%d pad=%d K=%d give Ho or Wo < 1", H, W, pad, K);
    ConvGeom g;
    g.H = H; g.W = W; g.Cin = Cin; g.K = K; g.stride = stride; g.pad = pad;
    g.Ho = (H + 2 * pad - K) / stride + 1;
    g.Wo = (W + 2 * pad - K) / stride + 1;
    g.step_tap = g.step_ci = 0;
    const int64_t kred = (int64_t)K * K * Cin;
    if (kred > (1ll << 22) || (int64_t)K * (W + 1) * Cin >= (1ll << 31))
        return fail(ISXA_ERR_ARG, "isxa_conv2d_nhwc: bad shape: K K Cin = %lld above 2^22 or K (W + 1) Cin = %lld not below 2^31 (32-bit offsets inside a window)",
                    (long long)kred, (long long)K * (W + 1) * Cin);
    g.Kred = (int)kred;
    const int64_t P = (int64_t)g.Ho * g.Wo;
    if (B > (int64_t)(1ll << 40) / P)
        return fail(ISXA_ERR_ARG, "isxa_conv2d_nhwc: bad shape: B Ho Wo = %lld x %lld above 2^40", (long long)B, (long long)P);
    g.M = B * P;
    const int64_t tiles_m64 = (g.M + 63) / 64, tiles_n64 = (Cout + 63) / 64;
    if (tiles_m64 >= (1ll << 26) || tiles_m64 * tiles_n64 >= (1ll << 31))
        return fail(ISXA_ERR_ARG, "isxa_conv2d_nhwc: bad shape: too many tiles (%lld x %lld of 64 x 64 outputs)", (long long)tiles_m64, (long long)tiles_n64);
    if (B == 0) return ISXA_OK;
    if (!x || !w_ohwi || !bias || !y) return fail(ISXA_ERR_ARG, "isxa_conv2d_nhwc: null pointer (x, w_ohwi, bias, y)");
    if (y == x) return fail(ISXA_ERR_ARG, "isxa_conv2d_nhwc: y must not alias x");
    if ((((uintptr_t)x | (uintptr_t)w_ohwi | (uintptr_t)y) % 16) != 0)
        return fail(ISXA_ERR_ARG, "isxa_conv2d_nhwc: x, w_ohwi and y must be 16-B aligned");
    hipStream_t st = (hipStream_t)stream;
    const int r = relu ? 1 : 0;
    // 128x128 tiles hold two accumulator sets: two workgroups per CU, 512 on the chip; 128x64 three per CU, 64x64 four
    const int64_t tiles_m128 = (g.M + 127) / 128;
    if (Cout % 128 == 0 && tiles_m128 * (Cout / 128) >= 512) launch_conv2d<2, 2, 16>(x, w_ohwi, Cout, g, y, bias, r, st);
    else if (tiles_m128 * tiles_n64 >= 1024) launch_conv2d<2, 1, 32>(x, w_ohwi, Cout, g, y, bias, r, st);
    else launch_conv2d<1, 1, 32>(x, w_ohwi, Cout, g, y, bias, r, st);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ISXA_ERR_HIP, "isxa_conv2d_nhwc: launch failed: %s", hipGetErrorString(e));
    return ISXA_OK;
}

ISXA_API int isxa_maxpool3s2_nhwc(const float* x, int64_t B, int H, int W, int C, float* y, isxa_stream_t stream) {
    if (B < 0 || H < 3 || W < 3 || C < 1 || C % 4 != 0)
        return fail(ISXA_ERR_ARG, "isxa_maxpool3s2_nhwc: bad shape B=%lld H=%d W=%d C=%d (B >= 0; H, W >= 3; C %% 4 == 0)", (long long)B, H, W, C);
    const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
    const int64_t per = (int64_t)H * W * (C / 4);
    if (B > (1ll << 58) / per) return fail(ISXA_ERR_ARG, "isxa_maxpool3s2_nhwc: bad shape: B H W C = %lld x %lld x 4 above 2^60", (long long)B, (long long)per);
    if (B == 0) return ISXA_OK;
    if (!x || !y) return fail(ISXA_ERR_ARG, "isxa_maxpool3s2_nhwc: null pointer (x, y)");
    if (y == x) return fail(ISXA_ERR_ARG, "isxa_maxpool3s2_nhwc: y must not alias x");
    if ((((uintptr_t)x | (uintptr_t)y) % 16) != 0) return fail(ISXA_ERR_ARG, "isxa_maxpool3s2_nhwc: x and y must be 16-B aligned");
    const int64_t total = B * Ho * Wo * (C / 4);
    const int64_t blocks = (total + 255) / 256;
    const unsigned grid = (unsigned)(blocks < (1ll << 22) ? blocks : (1ll << 22));          // beyond that a lane walks on by the grid's size
    hipLaunchKernelGGL(maxpool3s2_nhwc_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(x), H, W, C / 4, Ho, Wo, total,
                       reinterpret_cast<float4*>(y));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ISXA_ERR_HIP, "isxa_maxpool3s2_nhwc: launch failed: %s", hipGetErrorString(e));
    return ISXA_OK;
}
