/*
 * buzzdetect_rows.h — C ABI of stored embedding rows in libbuzzdetect_hip.so (gfx950): the record codec and slice
 * checksums of an on-disk embedding store (buzzdetect_amd/store.py), and the attached heads on rows that are already
 * resident (bd_score_rows), so that a new head, threshold or query costs a read of the rows and one head launch set, not a
 * pass through the CNN.
 *
 * Records.  A row is BD_EMBEDDING_SIZE float32; a stored row is one record, every record size a multiple of 16 bytes:
 *
 *   BD_ROWS_F32   4096 B        the row's own bits
 *   BD_ROWS_H     16 + 2048 B   int32 exponent e, 12 zero bytes, 1024 IEEE binary16 codes (little endian)
 *   BD_ROWS_B     16 + 1024 B   int32 exponent e, 12 zero bytes, 1024 uint8 codes
 *
 * Every scale is an exact power of two, so the host restatements and the kernels agree in every bit without a division.
 * With m = max_k |x_k| and m = f * 2^p, f in [0.5, 1) (frexp); m == 0 gives e = 0.
 *
 *   H   e = p - 15;  code_k = f16_rne(clamp(ldexpf(x_k, -e), -32752, 32752))      the maximum lands in [2^14, 2^15)
 *   B   e = p - 8;   code_k = min(255, rintf(ldexpf(x_k, -e)))                    the maximum lands in [128, 256)
 *   decode           ldexpf((float)code_k, e)
 *
 * Decisions at the edges:
 *   - 32752 = 2^15 - 16 is the largest binary16 below 2^15.  A scaled element above 32760 would round up to 2^15; it is
 *     clamped to 32752 instead, for every row alike.  So a code never reaches 2^15, and a row with m at FLT_MAX (p = 128,
 *     e = 113) decodes to at most 32752 * 2^113, a finite float, where 2^15 * 2^113 would be an infinity.  The clamp costs
 *     at most x * 2^-e - 32752 < 16 + 2^-9 scaled units on an element of at least 32760: inside the bound below.
 *   - B at FLT_MAX: e = 120, the largest decoded value 255 * 2^120 is finite.  The clamp to 255 is the only place where
 *     the error exceeds half a step.
 *   - B takes rows without negative elements (an embedding is a mean of ReLU6 outputs); -0.0f counts as zero.
 *   - A row with a non-finite element, or under B a negative one, is not representable: its record carries
 *     e = INT32_MIN and zero codes, it is counted in the flags word, and it decodes to a row of quiet NaN (0x7FC00000),
 *     so nothing downstream scores it silently.  A BD_ROWS_F32 record has no header: the row is stored as it is (it
 *     decodes to itself, non-finite elements included) and counted in the flags word all the same.
 *   - Decoding is exact whenever code * 2^e is a normal float: for every row with m >= 2^-100.  Below that the product is
 *     rounded once, to nearest even, on host and device alike.
 *
 * Error bounds (xh the decoded element; rows with m >= 2^-100):
 *   H   |xh - x| <= max(2^-11 |x|, 2^-39 m).   s = x * 2^-e is exact, |s| < 2^15.  For 2^-14 <= |s| <= 32760 binary16
 *       rounding is relative: at most 2^-11 |s|.  Below 2^-14 the code is subnormal, spacing 2^-24: at most 2^-25 scaled,
 *       i.e. 2^(e - 25) = 2^(p - 40) = 2^-39 * 2^(p - 1) <= 2^-39 m.  Above 32760 the clamp: s - 32752 <= 2^-11 s for
 *       every s <= 32752 / (1 - 2^-11) = 32768.0039..., and s < 2^15.
 *   B   |xh - x| <= 2^e <= m / 128, and half of that when the code is not clamped.  rintf moves s by at most 0.5; only
 *       s in [255.5, 256) is clamped, by less than 1.  2^e = 2^(p - 8) = 2^(p - 1) / 128 <= m / 128.
 *   For a Dense(1024 -> C) head in exact arithmetic a logit therefore moves under H by at most
 *   sum_k |w_ck| max(2^-11 |x_k|, 2^-39 m) <= 2^-11 sum_k |w_ck| |x_k| + 2^-39 m sum_k |w_ck|.
 *
 * Checksums.  A slice is BD_ROWS_SLICE consecutive records (the last one of a call may be shorter).  Over the slice's
 * 32-bit little-endian words w_i in file order, S1 = sum w_i and S2 = sum (i + 1) w_i, both mod 2^64: integer sums, a
 * function of the bytes alone whatever the grid and the order in which partial sums arrive (integer atomics).
 *
 * Conventions are those of buzzdetect_hip.h: device pointers 16-byte aligned, negative return = BD_E*, text in
 * bd_last_error(), a refused call names its argument and launches nothing.
 */
#ifndef BUZZDETECT_ROWS_H
#define BUZZDETECT_ROWS_H

#include <stdint.h>

#include "buzzdetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BD_ROWS_ABI_VERSION 1
#define BD_ROWS_F32 0
#define BD_ROWS_H 1
#define BD_ROWS_B 2
#define BD_ROWS_SLICE 256
#define BD_ROWS_HEADER_BYTES 16
#define BD_ROWS_MAX_WINDOWS (1 << 24)
#define BD_ROWS_H_MAX_CODE 32752.0f      /* the largest binary16 below 2^15 */

BD_API int bd_rows_abi_version(void);

/* Bytes of one record of `codec`; BD_EINVAL for another codec. */
BD_API int64_t bd_rows_record_bytes(int32_t codec);

/* rows_dev [windows][1024] float32 -> records_dev [windows][record bytes]; sums_dev [ceil(windows / BD_ROWS_SLICE)][2]
 * uint64 (S1, S2 per slice, 8-byte aligned) and flags_dev (one uint32: the number of rows that are not representable, see
 * above) are set by the call, not added to.  windows = 0 .. BD_ROWS_MAX_WINDOWS; asynchronous on `stream`. */
BD_API int bd_rows_encode(const float* rows_dev, int64_t windows, int32_t codec, void* records_dev, uint64_t* sums_dev,
                          uint32_t* flags_dev, void* stream);

/* records_dev -> rows_dev [windows][1024]; sums_dev as above, of the bytes the call read: the caller compares them with
 * the file's. */
BD_API int bd_rows_decode(const void* records_dev, int64_t windows, int32_t codec, float* rows_dev, uint64_t* sums_dev,
                          void* stream);

/* The same on host arrays, in plain C++ from the same element functions (csrc/rowcodec_device.h): bit for bit what the
 * kernels write.  They need no device. */
BD_API int bd_rows_encode_host(const float* rows, int64_t windows, int32_t codec, void* records, uint64_t* sums,
                               uint32_t* flags);
BD_API int bd_rows_decode_host(const void* records, int64_t windows, int32_t codec, float* rows, uint64_t* sums);

/* The heads of engine h on resident rows: rows_dev [windows][1024] float32 (contiguous) -> logits_dev
 * [windows][n_classes], by exactly the launches that follow the pool in a pass - the packaged head, a lone stack
 * (bd_head_attach), a set of heads (bd_headset_attach) or an ensemble over a set (bd_ensemble_attach) - in groups of at
 * most the engine's group size (bd_set_group_windows).  A window's logits are, bit for bit, those bd_predict* writes for
 * a window whose embedding is that row.  The scratch of the attached heads comes from workspace_dev (at least
 * bd_score_rows_workspace_bytes; it may be NULL where that is 0: the packaged head needs none).  windows == 0 launches
 * nothing.  An engine without a classifier is refused. */
BD_API int64_t bd_score_rows_workspace_bytes(bd_handle h, int64_t windows);
BD_API int bd_score_rows(bd_handle h, const float* rows_dev, int64_t windows, float* logits_dev, void* workspace_dev,
                         int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* BUZZDETECT_ROWS_H */
