/*
 * buzzdetect_tsne.h — C ABI of the neighbour-preserving 2-D map (exact t-SNE) in libbuzzdetect_hip.so (gfx950), for
 * buzzdetect_amd/tsne.py: the perplexity calibration of the neighbour lists (buzzdetect_knn.h) and the layout iterations,
 * whose repulsion is the full sum over all pairs.  No floating-point number is added atomically and no result depends on the
 * grid.  Attraction, repulsion and update are reproducible bit for bit and every entry point has a host restatement
 * (bd_tsne_*_host) from the same arithmetic (csrc/tsne_device.h); the affinities and the divergence use expf and logf, which
 * the device and the host library round differently, so those two agree with their restatements closely, not in every bit.
 *
 * Every step named below is one correctly rounded float32 operation; nothing is contracted except where fmaf is named; a
 * quotient a / b is one correctly rounded division.  A *butterfly* over the 64 lanes of a wave is v += v[lane ^ m] for
 * m = 32, 16, .. 1 (bd_search_norms').  y, v, gain, attr and rep are [N][2] float32.
 *
 * Slice sums.  The sum of a column over N rows, used for Z, the mean and the divergence: over slices of BD_TSNE_SLICE rows,
 * lane l adds rows first + l + 64 u, u = 0 .. BD_TSNE_SLICE / 64 - 1 ascending, from 0.0f (a row past N counts as 0.0f); the
 * 64 sums meet in the butterfly; the slices' sums are added in ascending order from 0.0f.
 *
 * Affinities.  Lists ids int32 [N][k], sims float32 [N][k] (cosine), k <= BD_TSNE_MAX_K; a wave per row, a lane per slot.  A
 * slot is usable if id >= 0 and sim is finite; every other slot gets p = 0.  d = fmaxf(0, fmaf(-2, sim, 2)) minus the row's
 * smallest d.  m = the usable slots: m == 0 gives p = 0 and beta = 0; (float)m <= perplexity gives p = 1 / m on the usable
 * slots and beta = 0.  Otherwise BD_TSNE_BISECTIONS steps from beta = 1, lo = 0, no upper bound: e = expf(-(d * beta)),
 * S = butterfly(e), A = butterfly(d * e), H = logf(S) + (beta * A) / S; H > logf(perplexity): lo = beta and beta = beta * 2
 * while no upper bound is known, else 0.5f * (lo + hi); otherwise hi = beta, beta = 0.5f * (lo + hi).  Then p = e / S at the
 * beta the last step left.
 *
 * Graph.  CSR over N rows as in buzzdetect_propagate.h: row_start int64 [N + 1] ascending from 0 to E, nbr int32 [E],
 * P float32 [E].  The device cannot look at the graph before it launches: a neighbour outside 0 .. N - 1 is taken as the
 * nearest end of the range and a row's edge range is brought inside 0 .. E; the host restatements refuse such a graph
 * (BD_ERANGE).
 *
 * Pair.  For points i and j: dx = y[i][0] - y[j][0], dy = y[i][1] - y[j][1], q = 1 / fmaf(dy, dy, fmaf(dx, dx, 1.0f)).
 *
 * Attraction.  A wave per row.  Lane l takes edges l, l + 64, .. of the row in stored order, from ax = ay = 0.0f:
 * w = P_e * q, ax = fmaf(w, dx, ax), ay = fmaf(w, dy, ay); attr[i] = the butterflies of ax and ay.  Degree 0 gives 0.
 *
 * Repulsion.  For row i and slice s of BD_TSNE_SLICE candidates j, ascending j, from z = rx = ry = 0.0f:
 * z = z + q, q2 = q * q, rx = fmaf(q2, dx, rx), ry = fmaf(q2, dy, ry); for j == i, q is taken as 0.0f.  The slices' partials
 * are added in ascending slice order from 0.0f: rep[i] = (rx, ry), z[i] = z.  Coincident points have q = 1 and dx = dy = 0: no
 * force, but they count in z.  A q2 below the normal range is a subnormal and is multiplied as one; below the subnormal range
 * it is 0.0f.  Coordinates must be finite.
 *
 * Update.  Z = the slice sums of z.  Per coordinate: g = 4.0f * (exaggeration * attr - rep / Z);
 * gain = (g > 0) != (v > 0) ? gain + 0.2f : gain * 0.8f, then fmaxf(gain, min_gain) - a zero (of either sign) and a NaN count
 * as not positive, so g = 0 against v = 0 shrinks the gain; v = fmaf(momentum, v, -((rate * gain) * g)); y = y + v.  Then
 * mean = (the slice sums of the new y) / (float)N per coordinate, and y = y - mean.  Z stays on the device.
 *
 * Divergence.  Z as above from z (as the last repulsion left it).  A wave per row, lane l over edges l, l + 64, .. from 0.0f:
 * t = t + (P_e > 0 ? P_e * ((logf(P_e) - logf(q)) + logf(Z)) : 0.0f); the butterfly gives the row's term; kl = the slice sums
 * of the rows' terms.
 *
 * Limits (refused on the host with the argument named, nothing launched and nothing written): 0 <= N <= BD_TSNE_MAX_ROWS
 * (N = 0 does nothing), 1 <= k <= BD_TSNE_MAX_K, 0 <= E, perplexity >= 1 and finite, non-null pointers (row_start, y, v,
 * gain, attr and rep 8-byte aligned, the workspace 16-byte, everything else 4-byte), a workspace of at least
 * bd_tsne_workspace_bytes(N) bytes; the host restatements also refuse a row_start that does not ascend from 0 to E.
 *
 * Conventions are those of buzzdetect_hip.h: 0 on success, a negative BD_E* code on failure, bd_last_error() for the text; the
 * caller owns all device memory; `stream` is a hipStream_t.
 */
#ifndef BUZZDETECT_TSNE_H
#define BUZZDETECT_TSNE_H

#include <stdint.h>

#include "buzzdetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BD_TSNE_ABI_VERSION 1
#define BD_TSNE_MAX_ROWS (1 << 20)
#define BD_TSNE_MAX_K 64
#define BD_TSNE_SLICE 2048                      /* candidates staged at a time; rows per slice sum */
#define BD_TSNE_ROWS_PER_BLOCK 256              /* rows a workgroup of the repulsion owns */
#define BD_TSNE_BISECTIONS 64

BD_API int bd_tsne_abi_version(void);

/* bytes of workspace bd_tsne_repulse, bd_tsne_update and bd_tsne_kl take for `rows` rows (BD_EINVAL out of range) */
BD_API int64_t bd_tsne_workspace_bytes(int64_t rows);

/* ids, sims, p: [rows][k]; beta: [rows] */
BD_API int bd_tsne_affinities(const int32_t* ids_dev, const float* sims_dev, int64_t rows, int32_t k, float perplexity,
                              float* p_dev, float* beta_dev, void* stream);
BD_API int bd_tsne_affinities_host(const int32_t* ids, const float* sims, int64_t rows, int32_t k, float perplexity, float* p,
                                   float* beta);

BD_API int bd_tsne_attract(const int64_t* row_start_dev, const int32_t* nbr_dev, const float* p_dev, int64_t rows, int64_t edges,
                           const float* y_dev, float* attr_dev, void* stream);
BD_API int bd_tsne_attract_host(const int64_t* row_start, const int32_t* nbr, const float* p, int64_t rows, int64_t edges,
                                const float* y, float* attr);

/* rep: [rows][2], z: [rows] */
BD_API int bd_tsne_repulse(const float* y_dev, int64_t rows, float* rep_dev, float* z_dev, void* workspace_dev,
                           int64_t workspace_bytes, void* stream);
BD_API int bd_tsne_repulse_host(const float* y, int64_t rows, float* rep, float* z);

/* y, v, gain are updated in place; total_dev (may be null) takes Z */
BD_API int bd_tsne_update(float* y_dev, float* v_dev, float* gain_dev, const float* attr_dev, const float* rep_dev,
                          const float* z_dev, int64_t rows, float exaggeration, float momentum, float rate, float min_gain,
                          float* total_dev, void* workspace_dev, int64_t workspace_bytes, void* stream);
BD_API int bd_tsne_update_host(float* y, float* v, float* gain, const float* attr, const float* rep, const float* z, int64_t rows,
                               float exaggeration, float momentum, float rate, float min_gain, float* total);

/* kl: one float32 */
BD_API int bd_tsne_kl(const int64_t* row_start_dev, const int32_t* nbr_dev, const float* p_dev, int64_t rows, int64_t edges,
                      const float* y_dev, const float* z_dev, float* kl_dev, void* workspace_dev, int64_t workspace_bytes,
                      void* stream);
BD_API int bd_tsne_kl_host(const int64_t* row_start, const int32_t* nbr, const float* p, int64_t rows, int64_t edges, const float* y,
                           const float* z, float* kl);

#ifdef __cplusplus
}
#endif

#endif /* BUZZDETECT_TSNE_H */
