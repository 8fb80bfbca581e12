/*
 * isx_scale.h -- C ABI of libisxscale.so: the cubic resize of 8-bit images on the MI355X (gfx950).
 *
 * The operation behind pre_process_dataset.py (the reference's script of that name: pad extreme
 * aspect ratios with random bytes, bring the shorter side to 448) and behind the second scale of
 * train.classif_regions (the reference's scale_cv(224) on the decoded image).  The pixels are
 * DEFINED HERE, entirely in integers (below); they follow the conventions of OpenCV's INTER_CUBIC
 * for 8-bit images but were never compared with an OpenCV binary.
 *
 * A library of its own, like libisxprep.so (include/isx_prep.h): nothing links it into the other
 * two and it exports no isx_ or isxp_ symbol.  Its conventions are those of isx_prep.h:
 *   - every pointer is a DEVICE pointer owned by the caller, densely packed
 *   - every call only ENQUEUES kernels on `stream` (a hipStream_t passed as void*) and returns:
 *     no allocation, no memset or memcpy node, no host wait, no other stream, no global state --
 *     safe to capture in a hipGraph and to replay, and to call from several host threads on
 *     distinct streams.  It has no debug hooks and no calls outside this contract
 *   - return 0 = ISXS_OK, <0 = error; isxs_last_error() gives a thread-local message that
 *     starts with the name of the entry
 */
#ifndef ISX_SCALE_H_
#define ISX_SCALE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISXS_OK 0
#define ISXS_ERR_ARG (-1) /* bad shape / pointer */
#define ISXS_ERR_HIP (-3) /* a HIP call failed */

typedef void* isxs_stream_t; /* hipStream_t */

const char* isxs_last_error(void);
int isxs_version(void);

/* Cubic resize of B images, each read through a VIRTUAL PADDED image P of (Hp, Wp, 3) bytes:
 *   P[y][x][c] = src[b][y - top][x - left][c]   where top <= y < top + Hs and left <= x < left + Ws
 *              = the top byte of mix64(seed + GOLDEN * (noise_ids[b] * 3 Hp Wp + 3 (y Wp + x) + c))   everywhere else
 * (splitmix64's output function and golden ratio, all modulo 2^64: the generator isx.h documents for isx_affine_noisy_u8).
 * src: (B, Hs, Ws, 3) uint8, dst: (B, Hd, Wd, 3) uint8, both at ANY byte alignment.  noise_ids: (B) int64, 8-byte aligned; may be null when
 * nothing is padded (top = left = 0, Hp = Hs, Wp = Ws), where no noise is read.
 *
 * Per axis, source length S (Hp or Wp), output length T, D = 2 T; output index j has
 *   num = (2 j + 1) S - T     s = floor(num / D)     r = num - s D  (0 <= r < D)     taps clip(s - 1 + k, 0, S - 1), k = 0..3
 *   c0 = floor((2 n0 + D^3) / (2 D^3)),  n0 = -1536 r (D - r)^2               the cubic with a = -3/4 at scale 2^11,
 *   c1 the same rounding of n1(r) = 2560 r^3 - 4608 r^2 D + 2048 D^3          rounded to nearest, ties toward +infinity,
 *   c2 the same rounding of n1(D - r)                                         floor division on signed 64-bit integers
 *   c3 = 2048 - c0 - c1 - c2
 * and dst[y'][x'][c] = clip((sum_i cy[y'][i] sum_j cx[x'][j] P[ty_i][tx_j][c] + 2^21) >> 22, 0, 255), the shift arithmetic.  Every term is
 * an integer and any partial sum stays below 2^31, so the sum has no order: the result does not depend on the launch geometry.
 *
 * Refused before any launch (-1): a side < 1, B < 0 or B > 65535, top < 0, left < 0, top + Hs > Hp or left + Ws > Wp ("bad shape");
 * Hd or Wd > 16384, Hp or Wp > 32768, 3 Hp Wp >= 2^31 or 3 Hd Wd >= 2^31 ("too large"); a null src or dst, or a null noise_ids with
 * padding, when B > 0 ("null pointer"); noise_ids off an 8-byte boundary ("8-B aligned").  B == 0 returns 0 and launches nothing. */
int isxs_resize_cubic_u8(const uint8_t* src, int64_t B, int Hs, int Ws, int top, int left, int Hp, int Wp, uint64_t seed,
                         const int64_t* noise_ids, uint8_t* dst, int Hd, int Wd, isxs_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* ISX_SCALE_H_ */
