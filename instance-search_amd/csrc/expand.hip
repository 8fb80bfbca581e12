// expand.hip -- conv2 + conv3 (+ projection) of the 64-channel bottlenecks as ONE kernel (isx_conv3x3_expand_nhwc, isx_conv3x3_expand_dual_nhwc), and
// conv2 + conv3 of the identity bottlenecks with 128 mid channels (isx_conv3x3_expand128_nhwc).
// A translation unit of its own: conv.hip and gemm.hip are compiled with the max-ILP scheduling strategy, which suits their plain tile loops
// (-0.3 ms each on the bench) and costs this kernel 4 % (Makefile).
// Reference call sites: the torchvision ResNet `features` trunk built by model/ModelDefinition.py, split by model/nn_utils.py:56-71 and run from
// model/siamese.py:20,107,151.
#include "expand_kernel.hpp"

using namespace isx;

// 3x3 convolution (padding 1, stride 1 or 2) to 64 channels + ReLU, then the 1x1 expansion to 256 channels + bias (+ residual) (+ ReLU), one kernel
// (see conv3x3_expand_kernel).  w2_ohwi: (64,3,3,Cin); w3t: (64, 256) = the expansion weight TRANSPOSED; y / residual: (B,Ho,Wo,256).
ISX_API int isx_conv3x3_expand_nhwc(const float* x, int64_t B, int H, int W, int Cin, const float* w2_ohwi, const float* b2, int stride,
                                    const float* w3t, int Cout, const float* b3, const float* residual, int relu, float* y, isx_stream_t stream) {
    ISX_REQUIRE(B >= 0 && H > 0 && W > 0 && Cin > 0 && (stride == 1 || stride == 2),
                "isx_conv3x3_expand_nhwc: bad shape B=%lld H=%d W=%d Cin=%d stride=%d", (long long)B, H, W, Cin, stride);
    ISX_REQUIRE(Cin % 32 == 0, "isx_conv3x3_expand_nhwc: Cin=%d must be a multiple of 32", Cin);
    ISX_REQUIRE(Cout == 256, "isx_conv3x3_expand_nhwc: Cout=%d (this kernel is built for 64 mid channels -> 256)", Cout);
    ISX_REQUIRE(H < 32767 && W < 32767 && B * H * W < (1ll << 31), "isx_conv3x3_expand_nhwc: input has too many pixels for 32-bit pixel indices");
    if (B == 0) return ISX_OK;
    ISX_REQUIRE(x && w2_ohwi && b2 && w3t && b3 && y, "isx_conv3x3_expand_nhwc: null pointer");
    ISX_REQUIRE((((uintptr_t)x | (uintptr_t)w2_ohwi | (uintptr_t)w3t) % 16) == 0, "isx_conv3x3_expand_nhwc: x, w2 and w3t must be 16-B aligned");
    ISX_REQUIRE(y != x && y != residual, "isx_conv3x3_expand_nhwc: y must not alias x or residual");
    Conv3x3Geom g;
    g.H = H; g.W = W; g.Cin = Cin; g.stride = stride; g.raster = 0;
    g.Ho = (H - 1) / stride + 1;
    g.Wo = (W - 1) / stride + 1;
    const int64_t M = B * g.Ho * g.Wo;
    ISX_REQUIRE((M + 63) / 64 < (1ll << 31), "isx_conv3x3_expand_nhwc: too many tiles");
    hipLaunchKernelGGL((conv3x3_expand_kernel<4, false>), dim3((unsigned)((M + 63) / 64)), dim3(256), 0, (hipStream_t)stream, x, M, w2_ohwi, g, b2, w3t, b3, residual,
                       relu ? 1 : 0, y);
    ISX_CHECK_LAUNCH("isx_conv3x3_expand_nhwc");
    return ISX_OK;
}

// The same with a 1x1 PROJECTION shortcut of the 64-channel block input x2 (first block of the stage; stride 1 only):
//   y = act( [W3 | Wd] . [relu(conv3x3(t, W2) + b2) ; x2] + bias ).  wcat_t: (128, 256) = [W3 | Wd] transposed; x2: (B,H,W,64).
ISX_API int isx_conv3x3_expand_dual_nhwc(const float* t, int64_t B, int H, int W, int Cin, const float* w2_ohwi, const float* b2, const float* x2,
                                         const float* wcat_t, int Cout, const float* bias, int relu, float* y, isx_stream_t stream) {
    ISX_REQUIRE(B >= 0 && H > 0 && W > 0 && Cin > 0, "isx_conv3x3_expand_dual_nhwc: bad shape B=%lld H=%d W=%d Cin=%d", (long long)B, H, W, Cin);
    ISX_REQUIRE(Cin % 32 == 0, "isx_conv3x3_expand_dual_nhwc: Cin=%d must be a multiple of 32", Cin);
    ISX_REQUIRE(Cout == 256, "isx_conv3x3_expand_dual_nhwc: Cout=%d (this kernel is built for 64 mid channels -> 256)", Cout);
    ISX_REQUIRE(H < 32767 && W < 32767 && B * H * W < (1ll << 31), "isx_conv3x3_expand_dual_nhwc: input has too many pixels for 32-bit pixel indices");
    if (B == 0) return ISX_OK;
    ISX_REQUIRE(t && w2_ohwi && b2 && x2 && wcat_t && bias && y, "isx_conv3x3_expand_dual_nhwc: null pointer");
    ISX_REQUIRE((((uintptr_t)t | (uintptr_t)w2_ohwi | (uintptr_t)wcat_t | (uintptr_t)x2) % 16) == 0, "isx_conv3x3_expand_dual_nhwc: t, x2, w2 and wcat_t must be 16-B aligned");
    ISX_REQUIRE(y != t && y != x2, "isx_conv3x3_expand_dual_nhwc: y must not alias an input");
    Conv3x3Geom g;
    g.H = H; g.W = W; g.Cin = Cin; g.stride = 1; g.Ho = H; g.Wo = W; g.raster = 0;
    const int64_t M = B * H * W;
    hipLaunchKernelGGL((conv3x3_expand_kernel<4, true>), dim3((unsigned)((M + 63) / 64)), dim3(256), 0, (hipStream_t)stream, t, M, w2_ohwi, g, b2, wcat_t, bias, x2,
                       relu ? 1 : 0, y);
    ISX_CHECK_LAUNCH("isx_conv3x3_expand_dual_nhwc");
    return ISX_OK;
}

// Tile grid of a conv3x3_expand128_kernel launch over `rows` (real or virtual) rows.  ONE n-tile everywhere: a 128-row tile and a 64-row tail tile
// both hold all 128 mid channels.  split > 0 (gemm_tail_split_rows, a multiple of 128): 128-row tiles below it, 64-row tiles from it on;
// split == 0: 128-row tiles only, the last one possibly partial.
static TailGrid expand128_grid(int64_t rows, int64_t split) {
    TailGrid t;
    t.big.m_active = t.small.m_active = nullptr;
    t.big.tiles_n = t.small.tiles_n = 1;
    t.big.tiles_m = (int)(split > 0 ? split / 128 : (rows + 127) / 128);
    t.small.tiles_m = (int)(split > 0 ? (rows - split + 63) / 64 : 0);
    t.blocks = (unsigned)(t.big.tiles_m + t.small.tiles_m);
    return t;
}

// conv2 + conv3 of an identity Bottleneck with 128 mid channels as ONE kernel (conv3x3_expand128_kernel): 3x3 convolution (padding 1, stride 1) to 128
// channels + ReLU, then the 1x1 expansion to Cout channels + bias (+ residual) (+ ReLU).  w2_ohwi: (128,3,3,Cin); w3t: (128, Cout) = the expansion
// weight TRANSPOSED; y / residual: (B,H,W,Cout).  Row order and tail as isx_conv3x3_nhwc's 128x128 launches: position-major under the same conditions
// (the output-side bound taken with Cout), rows past the last whole round of resident workgroups as 64-row tiles in the same grid.
ISX_API int isx_conv3x3_expand128_nhwc(const float* x, int64_t B, int H, int W, int Cin, const float* w2_ohwi, const float* b2, const float* w3t, int Cout,
                                       const float* b3, const float* residual, int relu, float* y, isx_stream_t stream) {
    ISX_REQUIRE(B >= 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "isx_conv3x3_expand128_nhwc: bad shape B=%lld H=%d W=%d Cin=%d Cout=%d", (long long)B, H, W, Cin, Cout);
    ISX_REQUIRE(Cin % kConvChunk == 0, "isx_conv3x3_expand128_nhwc: Cin=%d must be a multiple of %d", Cin, kConvChunk);
    ISX_REQUIRE(Cout % 128 == 0 && Cout <= (1 << 20), "isx_conv3x3_expand128_nhwc: Cout=%d must be a multiple of 128, at most 2^20", Cout);
    ISX_REQUIRE(H < 32767 && W < 32767 && B * H * W < (1ll << 31), "isx_conv3x3_expand128_nhwc: input has too many pixels for 32-bit pixel indices");
    if (B == 0) return ISX_OK;
    ISX_REQUIRE(x && w2_ohwi && b2 && w3t && b3 && y, "isx_conv3x3_expand128_nhwc: null pointer");
    ISX_REQUIRE((((uintptr_t)x | (uintptr_t)w2_ohwi | (uintptr_t)w3t) % 16) == 0, "isx_conv3x3_expand128_nhwc: x, w2 and w3t must be 16-B aligned");
    ISX_REQUIRE(y != x && y != residual, "isx_conv3x3_expand128_nhwc: y must not alias x or residual");
    Conv3x3Geom g;
    g.H = H; g.W = W; g.Cin = Cin; g.stride = 1; g.Ho = H; g.Wo = W; g.raster = conv3x3_pos_major_raster();
    const int64_t M = B * H * W;
    const int64_t Mv = conv3x3_pos_major_rows(B, H, W, Cin, H, W, Cout, 2);
    const int64_t rows = Mv > 0 ? Mv : M;
    const TailGrid tg = expand128_grid(rows, gemm_tail_split_rows(rows, 128, 256 * 2));
    const int64_t split = (int64_t)tg.big.tiles_m * 128;
    const dim3 grid(tg.blocks), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (Mv > 0) hipLaunchKernelGGL(conv3x3_expand128_kernel<true>, grid, block, 0, st, x, M, w2_ohwi, g, b2, w3t, Cout, b3, residual, relu ? 1 : 0, y, tg.big, tg.small, split);
    else hipLaunchKernelGGL(conv3x3_expand128_kernel<false>, grid, block, 0, st, x, M, w2_ohwi, g, b2, w3t, Cout, b3, residual, relu ? 1 : 0, y, tg.big, tg.small, split);
    ISX_CHECK_LAUNCH("isx_conv3x3_expand128_nhwc");
    return ISX_OK;
}
