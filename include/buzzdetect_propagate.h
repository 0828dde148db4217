/*
 * buzzdetect_propagate.h — C ABI of label propagation in libbuzzdetect_hip.so (gfx950): a few labels spread along a
 * neighbour graph (buzzdetect_knn.h), for buzzdetect_amd/propagate.py.  Every result is reproducible bit for bit.
 *
 *   bd_propagate_weights    neighbour lists (ids, sims) -> the edges' (nbr, w)         (bd_propagate_weights_host: the same bits)
 *   bd_propagate_step       F_out = one step of F_in along the graph, and how far it moved  (bd_propagate_step_host: the same)
 *   bd_propagate_readout    per row: reach, label, confidence, margin                   (bd_propagate_readout_host: the same)
 *
 * Graph.  CSR over N rows: row_start int64 [N + 1] ascending from 0 to E, nbr int32 [E], w float32 [E].  A fixed-k list is the
 * CSR with row_start[i] = i k; a symmetrised graph has rows of any length.  Every step named below is one correctly rounded
 * float32 operation, and nothing is contracted into a fused multiply-add except where fmaf is named.
 *
 * Weights.  For slot s of row i of lists ids, sims [N][k]: x = fmaxf(sims, 0.0f) (a NaN gives 0), w = x^power by power - 1
 * rounded multiplications w = w * x from w = x, nbr = ids.  An empty slot (id < 0) gets w = 0.0f and nbr = i.
 *
 * Step.  F_in, F_out and Y are [N][C] float32, C <= BD_PROPAGATE_MAX_CLASSES; alpha is [N].  A wave per row, a lane per class,
 * over the row's edges in stored order, from acc = den = 0.0f:
 *   acc = fmaf(w_e, F_in[nbr_e][c], acc);  den = den + w_e
 *   mean = den > 0 ? acc / den : 0.0f
 *   F_out[i][c] = fmaf(alpha[i], mean, (1.0f - alpha[i]) * Y[i][c])
 * alpha 0 clamps a labelled row to its label, alpha 1 makes a row the weighted mean of its neighbours, a value between is a
 * soft clamp.  delta[slice] over slices of BD_PROPAGATE_SLICE rows is the largest |F_out - F_in| of the slice, a NaN counting
 * as +INFINITY (a maximum does not depend on order).  The device cannot look at the graph before it launches: a neighbour
 * outside 0 .. N - 1 is taken as the nearest end of the range and a row's edge range is brought inside 0 .. E, so that nothing
 * is read out of bounds; the host restatement refuses such a graph (BD_ERANGE).  F_in and F_out must not overlap.
 *
 * Read-out.  A wave per row; lanes c >= C hold 0.0f.  reach = the butterfly of bd_search_norms over the lanes' F[i][c]
 * (v += v[lane ^ m], m = 32 .. 1).  top = the largest class value, a NaN counting as -INFINITY, the lowest class on a tie;
 * second = the largest among the other classes (0.0f when C == 1).  Where reach is 0 or not finite: label -1, confidence and
 * margin 0.0f.  Otherwise label = the top's class, confidence = top / reach, margin = (top - second) / reach.
 *
 * Limits (refused on the host with the argument named, nothing launched and nothing written): 1 <= C <=
 * BD_PROPAGATE_MAX_CLASSES, 1 <= k <= BD_KNN_MAX_K, 1 <= power <= BD_PROPAGATE_MAX_POWER, 0 <= N <= BD_PROPAGATE_MAX_ROWS
 * (N = 0 does nothing), 0 <= E, non-null pointers (row_start 8-byte aligned, everything else 4-byte).
 *
 * Conventions are those of buzzdetect_hip.h: 0 on success, a negative BD_E* code on failure, bd_last_error() for the text; the
 * caller owns all device memory; `stream` is a hipStream_t.
 */
#ifndef BUZZDETECT_PROPAGATE_H
#define BUZZDETECT_PROPAGATE_H

#include <stdint.h>

#include "buzzdetect_hip.h"
#include "buzzdetect_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BD_PROPAGATE_ABI_VERSION 1
#define BD_PROPAGATE_MAX_CLASSES 64
#define BD_PROPAGATE_MAX_POWER 16
#define BD_PROPAGATE_MAX_ROWS (1 << 24)
#define BD_PROPAGATE_SLICE 256                  /* rows per element of delta */

BD_API int bd_propagate_abi_version(void);

/* ids, sims, nbr, w: [rows][k] */
BD_API int bd_propagate_weights(const int32_t* ids_dev, const float* sims_dev, int64_t rows, int32_t k, int32_t power,
                                int32_t* nbr_dev, float* w_dev, void* stream);
BD_API int bd_propagate_weights_host(const int32_t* ids, const float* sims, int64_t rows, int32_t k, int32_t power, int32_t* nbr,
                                     float* w);

/* delta: [(rows + BD_PROPAGATE_SLICE - 1) / BD_PROPAGATE_SLICE] */
BD_API int bd_propagate_step(const int64_t* row_start_dev, const int32_t* nbr_dev, const float* w_dev, int64_t rows, int64_t edges,
                             const float* f_in_dev, const float* y_dev, const float* alpha_dev, int32_t classes, float* f_out_dev,
                             float* delta_dev, void* stream);
BD_API int bd_propagate_step_host(const int64_t* row_start, const int32_t* nbr, const float* w, int64_t rows, int64_t edges,
                                  const float* f_in, const float* y, const float* alpha, int32_t classes, float* f_out,
                                  float* delta);

/* reach, confidence, margin float32 [rows]; label int32 [rows] */
BD_API int bd_propagate_readout(const float* f_dev, int64_t rows, int32_t classes, float* reach_dev, int32_t* label_dev,
                                float* confidence_dev, float* margin_dev, void* stream);
BD_API int bd_propagate_readout_host(const float* f, int64_t rows, int32_t classes, float* reach, int32_t* label,
                                     float* confidence, float* margin);

#ifdef __cplusplus
}
#endif

#endif /* BUZZDETECT_PROPAGATE_H */
