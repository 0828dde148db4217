/*
 * buzzdetect_knn.h — C ABI of the k-nearest-neighbour lists in libbuzzdetect_hip.so (gfx950): for every query row the k most
 * similar candidate rows, over [W][1024] embeddings where they lie, for buzzdetect_amd/propagate.py.  No [Wq][Wc] matrix is
 * written anywhere, and the lists are reproducible bit for bit.
 *
 *   bd_knn_workspace_bytes   host only: the scratch bd_knn_update takes for (Wq, Wc)
 *   bd_knn_update            keys[q] = the k best of (keys[q] + this call's candidates)   (bd_knn_update_host: the same bits)
 *   bd_knn_decode_host       keys -> (id, sim)
 *
 * Notation.  Q is [Wq][BD_KNN_DIM] float32, C is [Wc][BD_KNN_DIM] float32, both 16-byte aligned; they may be the same array.
 * n2 is bd_search_norms of the rows (buzzdetect_search.h).  Query row i has id q_base_id + i, candidate row j has id
 * c_base_id + j.  Every step named below is one correctly rounded float32 operation, and nothing is contracted into a fused
 * multiply-add except where fmaf is named.
 *
 * Scores.  dot(i, j) is the chain acc = fmaf(Q[i][c], C[j][c], acc) from 0.0f over the channels in the order of the walk of
 * the Dense heads (buzzdetect_head.h): within each group of eight channels 8 s .. 8 s + 7, s ascending, the order is
 * 0, 4, 1, 5, 2, 6, 3, 7.  It has exactly the bits bd_search_scores(..., BD_SEARCH_DOT) stores for row i against query row j,
 * and the products commute, so dot(i, j) and dot(j, i) are the same bits.
 *   BD_KNN_DOT      sim = dot
 *   BD_KNN_COSINE   sim = dot / (sqrtf(n2_q[i]) * sqrtf(n2_c[j])): two roots, one rounded product, one division; 0.0f where
 *                   either squared norm is below BD_SEARCH_NORM_FLOOR.  sim(i, j) and sim(j, i) are the same bits.
 * A NaN sim counts as -INFINITY and -0.0f as +0.0f, as in the search.
 *
 * State.  keys[Wq][k] uint64 in the key format of buzzdetect_search.h (the higher sim first, among equal sims the lower id),
 * best first, 0 for an empty slot, zero-filled by the caller before the first call.  After bd_knn_update every query row holds
 * the k best of (its old state + this call's candidates); with exclude_self the candidate whose id equals the query's id is
 * left out.  The result is a function of the candidate set alone (ids are distinct as long as the calls' candidate id ranges
 * do not overlap): one call over all candidates equals any split of them into calls, and a row's list depends neither on where
 * the row sits nor on which other queries there are.
 *
 * Kernel.  A workgroup owns 128 query rows and sweeps the candidates in panels of 128; both operands are staged through LDS
 * from the row-major rows, 16 channels at a time, and each of the four waves holds 64 x 64 sims in four accumulator tiles of
 * v_mfma_f32_32x32x2_f32.  After the walk a lane keys its sims and compares them with its rows' k-th best key, kept in LDS; the
 * survivors go to a pending list per row in LDS (an integer LDS counter: the order inside a list does not matter).  When a
 * list might not take the next round, and at the end, a wave merges the row's k keys and its pending keys by a bitonic network
 * in registers and lowers the threshold.  No floating-point number is added atomically, no workgroup waits for another, every
 * output element has one writer, inputs are only read, and all element offsets are 64-bit.  For BD_KNN_COSINE the workspace holds
 * the roots of the squared norms, written by a launch of its own in front.
 *
 * Limits (refused on the host with the argument named, nothing launched and nothing written): 1 <= k <= BD_KNN_MAX_K,
 * 0 <= Wq, Wc <= BD_KNN_MAX_ROWS per call (either being 0 does nothing), base ids >= 0 with base + rows <= 0xFFFFFFFF
 * (BD_ERANGE), a known metric, exclude_self 0 or 1, non-null pointers (the rows and the workspace 16-byte aligned, keys 8-byte,
 * the norms 4-byte; the norms are read for BD_KNN_COSINE only and may be null otherwise), and a workspace of at least
 * bd_knn_workspace_bytes(Wq, Wc) bytes (BD_EWORKSPACE).
 *
 * Conventions are those of buzzdetect_hip.h: 0 on success, a negative BD_E* code on failure, bd_last_error() for the text; the
 * caller owns all device memory; `stream` is a hipStream_t.
 */
#ifndef BUZZDETECT_KNN_H
#define BUZZDETECT_KNN_H

#include <stdint.h>

#include "buzzdetect_hip.h"
#include "buzzdetect_search.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BD_KNN_ABI_VERSION 1
#define BD_KNN_DIM 1024                         /* floats per row: BD_SEARCH_DIM */
#define BD_KNN_MAX_K 64
#define BD_KNN_MAX_ROWS (1 << 22)               /* query rows, and candidate rows, per call */
#define BD_KNN_DOT 0
#define BD_KNN_COSINE 1

BD_API int bd_knn_abi_version(void);

/* Host only.  Bytes of scratch for bd_knn_update (a negative code for arguments out of range). */
BD_API int64_t bd_knn_workspace_bytes(int64_t query_rows, int64_t candidate_rows);

BD_API int bd_knn_update(const float* queries_dev, int64_t query_rows, const float* n2_q_dev, int64_t q_base_id,
                         const float* candidates_dev, int64_t candidate_rows, const float* n2_c_dev, int64_t c_base_id,
                         int32_t metric, int32_t exclude_self, uint64_t* keys_dev, int32_t k, void* workspace_dev,
                         int64_t workspace_bytes, void* stream);
BD_API int bd_knn_update_host(const float* queries, int64_t query_rows, const float* n2_q, int64_t q_base_id,
                              const float* candidates, int64_t candidate_rows, const float* n2_c, int64_t c_base_id,
                              int32_t metric, int32_t exclude_self, uint64_t* keys, int32_t k);

/* Host only.  n keys -> ids[n], sims[n]; an empty slot gives (-1, 0.0f); an id past 2^31 - 1 is refused (BD_ERANGE).  Returns
 * the number of real keys. */
BD_API int64_t bd_knn_decode_host(const uint64_t* keys, int64_t n, int32_t* ids, float* sims);

#ifdef __cplusplus
}
#endif

#endif /* BUZZDETECT_KNN_H */
