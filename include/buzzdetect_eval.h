/*
 * buzzdetect_eval.h — C ABI of the threshold sweep in libbuzzdetect_hip.so (gfx950): score columns and labels become the integer
 * counts from which buzzdetect_amd/evaluate.py writes the rows of a model's tests/metrics.csv, where the logits lie.
 *
 *   bd_eval_accumulate     adds the windows of one call to the state      (bd_eval_accumulate_host: the same words on the host)
 *
 * The table (train.metrics_table) has one row per distinct value of the logits rounded to two decimals, and a window counts as
 * detected at threshold t when its logit >= t.  Both are functions of two integers per logit.  With z the float32 logit widened
 * to float64 and every operation below one correctly rounded float64 operation:
 *
 *     kr(z) = rint(z * 100.0)                       the row the logit creates (rint(z * 100) / 100 is NumPy's round(z, 2))
 *     kf(z) = max{k : k / 100.0 <= z}               the lowest row that still detects it
 *
 * kf is floor(z * 100.0), corrected by at most one step each way with the comparisons (k + 1) / 100.0 <= z and k / 100.0 > z.
 * A row exists for every k some logit rounds to; its `detected` is the number of logits with kf >= k, its `tp` the same over
 * the positives.
 *
 * Call-wide: W windows, C score columns, L label columns.  x, float32 scores, column c of window w at
 * x[w * row_stride + c * col_stride] (strides in elements, as bd_calls_events reads its matrix: [W][C] logits and column-major
 * matrices both serve).  labels, dense uint8 [W][L]: 0 negative, 1 positive, 2 skip; any other value is skip.  label_of[C],
 * int32 in [-1, L): the label column of score column c; several score columns (the same class of several models) may share
 * one; a column with label_of == -1 leaves its state untouched.
 *
 * State, owned by the caller, both uint32:
 *
 *     hist[C][BD_EVAL_PLANES][BD_EVAL_BINS]    planes: negatives by kf, positives by kf, all labelled rows by kr;
 *                                              bin b is k = b + BD_EVAL_K_MIN, so the bins cover logits in -81.92 .. 81.91
 *     tail[C][BD_EVAL_TAILS]                   rows skipped by label, non-finite rows, rows below the range, rows above it
 *
 * A row is in range iff both kf and kr are.  A labelled row that is non-finite or out of range counts in tail only, a skipped
 * row in tail[0] only, whatever its score.  bd_eval_accumulate ADDS to the state: zeroing it is the caller's memset, and more
 * than 2^32 - 1 rows per column of a state is the caller's error (the counters wrap).  Everything accumulated is an integer, so
 * the state is a function of the rows alone, whatever the order, the grid or the split into calls.
 *
 * Device side.  One workgroup per (column, slice of at most BD_EVAL_SLICE windows) holds the three planes in LDS as 16-bit
 * counters, two to a word (96 KiB; BD_EVAL_SLICE rows cannot carry one half into the other), adds its rows there and then adds
 * the non-zero counters to the global state with no-return atomics: at most min(rows, 3 * BD_EVAL_BINS) global adds a slice,
 * whatever the distribution of the logits.
 *
 * Limits (refused on the host with the argument named, nothing launched): 0 <= W <= BD_EVAL_MAX_WINDOWS,
 * 1 <= C <= BD_EVAL_MAX_COLUMNS, 1 <= L <= BD_EVAL_MAX_LABELS, non-zero strides, non-null pointers, 4-byte aligned where they
 * hold words, label_of within [-1, L).  bd_eval_accumulate reads label_of_dev back (C * 4 bytes, waiting for the stream) to
 * check it before it launches.  W == 0 launches nothing.
 *
 * Conventions are those of buzzdetect_hip.h: 0 on success, a negative BD_E* code on failure, bd_last_error() for the text; the
 * caller owns all device memory; `stream` is a hipStream_t.
 */
#ifndef BUZZDETECT_EVAL_H
#define BUZZDETECT_EVAL_H

#include <stdint.h>

#include "buzzdetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BD_EVAL_ABI_VERSION 1
#define BD_EVAL_BINS 16384                      /* rows k = BD_EVAL_K_MIN .. BD_EVAL_K_MIN + BD_EVAL_BINS - 1 */
#define BD_EVAL_K_MIN (-8192)
#define BD_EVAL_PLANES 3                        /* negatives by kf, positives by kf, labelled rows by kr */
#define BD_EVAL_TAILS 4                         /* skipped, non-finite, below the range, above it */
#define BD_EVAL_SLICE 32768                     /* windows a workgroup counts in 16-bit halves */
#define BD_EVAL_MAX_WINDOWS (1 << 24)           /* windows per call */
#define BD_EVAL_MAX_COLUMNS 2048
#define BD_EVAL_MAX_LABELS 2048

BD_API int bd_eval_abi_version(void);

/* bytes of hist plus tail for `columns` score columns; BD_EINVAL outside 1 .. BD_EVAL_MAX_COLUMNS */
BD_API int64_t bd_eval_state_bytes(int32_t columns);

BD_API int bd_eval_accumulate(const float* x_dev, int64_t windows, int32_t columns, int64_t row_stride, int64_t col_stride,
                              const uint8_t* labels_dev, int32_t n_labels, const int32_t* label_of_dev, uint32_t* hist_dev,
                              uint32_t* tail_dev, void* stream);
BD_API int bd_eval_accumulate_host(const float* x, int64_t windows, int32_t columns, int64_t row_stride, int64_t col_stride,
                                   const uint8_t* labels, int32_t n_labels, const int32_t* label_of, uint32_t* hist,
                                   uint32_t* tail);

#ifdef __cplusplus
}
#endif

#endif /* BUZZDETECT_EVAL_H */
