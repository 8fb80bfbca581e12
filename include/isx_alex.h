/*
 * isx_alex.h -- C ABI of libisxalex.so: the convolutions and pools of an AlexNet-style `features` trunk on the MI355X (gfx950).
 *
 * What the ResNet trunks do not need and isx.h does not have: a square K x K convolution of any kernel size, stride and padding on
 * channels-last activations (the 11x11 / stride 4 and 5x5 layers of the reference's AlexNet and of its own clone, model/ModelDefinition.py:13-45)
 * and the un-padded MaxPool2d(3, stride 2) behind them.  The convolution's sum is the canonical trunk sum of isx.h, so a layer that both
 * libraries take (3x3, padding 1, Cin % 32 == 0) has the same bits from either.
 *
 * A library of its own, like libisxprep.so (include/isx_prep.h) and libisxscale.so (include/isx_scale.h): nothing links it into the other
 * three and it exports no isx_, isxp_ or isxs_ symbol.  Its conventions are those of isx_scale.h:
 *   - every pointer is a DEVICE pointer owned by the caller, densely packed
 *   - every call only ENQUEUES kernels on `stream` (a hipStream_t passed as void*) and returns:
 *     no allocation, no memset or memcpy node, no host wait, no other stream, no global state, no environment read --
 *     safe to capture in a hipGraph and to replay, and to call from several host threads on
 *     distinct streams.  It has no debug hooks and no calls outside this contract
 *   - return 0 = ISXA_OK, <0 = error; isxa_last_error() gives a thread-local message that
 *     starts with the name of the entry
 *   - every index is 64-bit: x and y may exceed 2^31 elements and 4 GiB
 */
#ifndef ISX_ALEX_H_
#define ISX_ALEX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISXA_OK 0
#define ISXA_ERR_ARG (-1) /* bad shape / pointer */
#define ISXA_ERR_HIP (-3) /* a HIP call failed */

#define ISXA_CONV_CHUNK 64 /* terms per first-level chain: ISX_CONV_CHUNK of isx.h */
#define ISXA_MAX_K 16      /* largest kernel side */

typedef void* isxa_stream_t; /* hipStream_t */

const char* isxa_last_error(void);
int isxa_version(void);

/* Square K x K convolution, groups 1, dilation 1, channels-last, as an implicit GEMM on the fp32 matrix cores (v_mfma_f32_32x32x2_f32).
 * x: (B,H,W,Cin); w_ohwi: (Cout,K,K,Cin); bias: (Cout); y: (B,Ho,Wo,Cout), Ho = (H + 2 pad - K) / stride + 1 (floor), Wo the same of W.
 *
 * Sum: the canonical convolution sum of isx.h.  The reduction is flattened in (kh, kw, ci) order and cut into chunks of ISXA_CONV_CHUNK = 64
 * terms (the last one short); a chunk is a k-ordered fp32 fma chain from +0; the chunk sums are added in order into a second fp32 accumulator
 * (tot = tot + chain_c, from +0); then y = tot + bias[co] (one rounded add), and max(y, 0) with relu (a NaN becomes 0, as in isx_conv3x3_nhwc).
 * A padding tap keeps its place in the flattened order and contributes fma(0, w, acc).  Where K K Cin is no multiple of the k-tile the chain
 * goes on over terms of zero weight and zero activation, which change no bit of it.  For K = 3, pad = 1, stride 1 | 2 and Cin % 32 == 0 the
 * result is bit-identical to isx_conv3x3_nhwc without a residual.  An output is a function of its own image alone: it does not depend on B.
 *
 * Refused before any launch (-1): B < 0, H, W, Cin or Cout < 1, K < 1 or K > ISXA_MAX_K, stride < 1 or > 4, pad < 0 or pad >= K, Ho or Wo < 1,
 * Cout % 32 != 0 or Cout > 2^20, H or W > 2^20, Cin > 2^20, K K Cin > 2^22, K (W + 1) Cin >= 2^31 (offsets inside a window are 32-bit), B Ho Wo > 2^40,
 * 2^26 or more rows of 64 x 64 output tiles or 2^31 or more such tiles ("bad shape"); a null x, w_ohwi, bias or y when
 * B > 0 ("null pointer"); y == x ("alias"); x, w_ohwi or y off a 16-byte boundary ("16-B aligned"; bias: any fp32 alignment; a pixel's
 * Cin floats need not be a multiple of 16 bytes).  B == 0 returns 0 and launches nothing. */
int isxa_conv2d_nhwc(const float* x, int64_t B, int H, int W, int Cin, const float* w_ohwi, int Cout, int K, int stride, int pad,
                     const float* bias, int relu, float* y, isxa_stream_t stream);

/* MaxPool2d(3, stride 2, padding 0, floor) on a channels-last map.  x: (B,H,W,C); y: (B,(H-3)/2+1,(W-3)/2+1,C).
 * The window is scanned in (kh, kw) order from its first element m with `if (v > m || v != v) m = v`: torch's CPU rule, so a NaN in the window
 * is the result (the last one met), +-inf compare as numbers, and of -0 and +0 the one met first stays.
 * Refused before any launch (-1): B < 0, H or W < 3, C < 1 or C % 4 != 0 ("bad shape"); a null x or y when B > 0 ("null pointer"); y == x
 * ("alias"); x or y off a 16-byte boundary ("16-B aligned").  B == 0 returns 0 and launches nothing. */
int isxa_maxpool3s2_nhwc(const float* x, int64_t B, int H, int W, int C, float* y, isxa_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* ISX_ALEX_H_ */
