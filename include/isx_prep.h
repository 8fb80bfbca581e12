/*
 * isx_prep.h -- C ABI of libisxprep.so: dataset preparation on the MI355X (gfx950).
 *
 * Pipeline stage 0: the per-channel moments from which create_mean_std_file.py writes the
 * mean/std file every entry point reads before it decodes its first image (the reference's
 * create_mean_std_file.py:25-46 holds the whole dataset as one fp32 tensor for this).
 *
 * This is an OFFLINE tool's library, separate from libisx.so (include/isx.h): it is not part
 * of the drop-in boundary of the retrieval and training path, nothing in libisx links it and
 * it exports no isx_ symbol.  Its conventions are those of isx.h:
 *   - every pointer is a DEVICE pointer owned by the caller, densely packed
 *   - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*) and returns:
 *     no allocation, no host wait, no other stream, no global state -- safe to capture in a
 *     hipGraph (kernels only: the output is zeroed by a kernel, a hipMemsetAsync node replays
 *     wrongly) and to call from several host threads on distinct streams;
 *     tests/test_gpu_graph_capture.py captures the entry and replays it into its own earlier
 *     result.  It has no debug hooks and no calls outside this contract
 *   - return 0 = ISXP_OK, <0 = error; isxp_last_error() gives a thread-local message that
 *     starts with the name of the entry
 *   - operands may exceed 2^31 elements and 4 GiB except where an entry states a limit;
 *     tests/test_gpu_large_tensors.py holds this (14 270 images of 224 x 224: 2.1 GB of bytes)
 */
#ifndef ISX_PREP_H_
#define ISX_PREP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISXP_OK 0
#define ISXP_ERR_ARG (-1) /* bad shape / pointer / alignment */
#define ISXP_ERR_HIP (-3) /* a HIP call failed */

typedef void* isxp_stream_t; /* hipStream_t */

const char* isxp_last_error(void);
int isxp_version(void);

/* Exact integer moments of every channel of every image.
 * img: (B, H, W, 3) uint8 RGB, densely packed, at ANY byte alignment.  moments: (B, 3, 2) int64, 8-byte aligned:
 *   moments[b][c][0] = sum over (y, x) of img[b][y][x][c]        moments[b][c][1] = the same sum of squares
 * The call OVERWRITES moments (it zeroes them on `stream` with a kernel, then every workgroup adds its part with 64-bit integer atomics: integer
 * addition has no order, so the result is independent of the launch geometry and of what moments held before).
 * Refused before any launch (-1): H < 1, W < 1, B < 0 or B > 65535 ("bad shape"); 3 H W >= 2^31 ("too large"); a null img or
 * moments with B > 0 ("null pointer"); moments off an 8-byte boundary ("8-B aligned").  B == 0 returns 0 and launches nothing. */
int isxp_channel_moments_u8(const uint8_t* img, int64_t B, int H, int W, int64_t* moments, isxp_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* ISX_PREP_H_ */
