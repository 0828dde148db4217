/*
 * buzzdetect_search.h — C ABI of search by example in libbuzzdetect_hip.so (gfx950): a score per (window, query) and a
 * running top-k per query, on the device, for buzzdetect_amd/search.py.
 *
 *   bd_search_packed_floats   host only: the floats bd_search_pack_queries writes for Q queries
 *   bd_search_pack_queries    host only: Q query rows -> the matrix instruction's fragment order (upload the result once)
 *   bd_search_norms           n2[w] = sum_c E[w][c]^2                      (bd_search_norms_host: the same bits on the host)
 *   bd_search_scores          S[w][q] = dot(E[w], query q), or that over sqrt(n2[w])
 *   bd_search_update          the k best (score, id) per query so far      (bd_search_update_host: the same bits on the host)
 *   bd_search_decode_host     keys -> (score, id)
 *
 * Row norms.  E is [W][BD_SEARCH_DIM] float32.  One wave per row: lane l adds E[w][l + 64 j]^2 for j = 0 .. 15 in ascending
 * order, one fused multiply-add each, from 0; the 64 partial sums meet in the butterfly v += v[lane ^ m], m = 32, 16, .. 1.
 * Every step is one correctly rounded float32 operation on both sides.
 *
 * Scores.  The queries are packed once by bd_search_pack_queries (K = BD_SEARCH_DIM, N = Q, zero-padded to tiles of 32) and
 * lie in device memory.  One wave owns a 32 x 32 tile of S and walks K alone in ascending steps with exact-float32 matrix
 * instructions - the walk of the Dense heads (buzzdetect_head.h) - so a score is a chain over its own row and its own query:
 * its bits depend neither on where the row sits in the call nor on which other queries there are.  BD_SEARCH_DOT stores the
 * sum; BD_SEARCH_COSINE stores S / sqrtf(n2[w]) - one correctly rounded root, one correctly rounded division - and 0.0f where
 * n2[w] < BD_SEARCH_NORM_FLOOR.  For a cosine the caller brings the query rows to unit length (in double, then float).
 * Score (w, q) is stored at scores[w * row_stride + q * col_stride] (strides in elements): row_stride = Q, col_stride = 1 is
 * the row-major [W][Q] matrix; buzzdetect_amd/search.py keeps the scores of a pass query-major (row_stride = 1,
 * col_stride = W), which is what bd_search_update then reads with consecutive lanes on consecutive addresses.
 *
 * Selection.  The state is keys[Q][k] uint64 in device memory, zero-filled by the caller before the first call; 0 is an
 * empty slot.  A candidate is (score, id), id = base_id + w.  A NaN score counts as -INFINITY and -0.0f as +0.0f.  The order is
 * total: the higher score first, among equal scores the lower id first.  Key = (m << 32) | (0xFFFFFFFF - id), where m is the
 * monotone map of the score's bits (a negative float's bits complemented, a non-negative one's with the sign bit set): a
 * larger key is a better hit and no real key is 0.  After the call the state holds the k best of (old state + this call's W
 * candidates), best first, empty slots last.  The result is a function of the candidate set alone (ids are distinct as long as
 * the calls' id ranges do not overlap).  One workgroup per query sorts in LDS; there are no atomics on global memory and nothing
 * depends on the grid.  The matrix is read by the same two strides, so logits serve as well as similarities.
 *
 * Limits (refused on the host with the argument named, nothing launched): 1 <= Q <= BD_SEARCH_MAX_QUERIES,
 * 1 <= k <= BD_SEARCH_MAX_K, 0 <= W <= BD_SEARCH_MAX_WINDOWS per call (W = 0 launches nothing), base_id >= 0 and
 * base_id + W <= 0xFFFFFFFF (BD_ERANGE), a known metric, non-zero strides, non-null pointers (E and the packed queries
 * 16-byte aligned).
 *
 * Conventions are those of buzzdetect_hip.h: 0 on success, a negative BD_E* code on failure, bd_last_error() for the text; the
 * caller owns all device memory; `stream` is a hipStream_t.
 */
#ifndef BUZZDETECT_SEARCH_H
#define BUZZDETECT_SEARCH_H

#include <stdint.h>

#include "buzzdetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BD_SEARCH_ABI_VERSION 1
#define BD_SEARCH_DIM 1024                      /* floats per row: BD_EMBEDDING_SIZE */
#define BD_SEARCH_MAX_QUERIES 1024
#define BD_SEARCH_MAX_K 1024
#define BD_SEARCH_MAX_WINDOWS (1 << 20)         /* rows per call */
#define BD_SEARCH_NORM_FLOOR 1e-30f             /* a row whose squared norm is below this has cosine 0 with everything */
#define BD_SEARCH_DOT 0
#define BD_SEARCH_COSINE 1

BD_API int bd_search_abi_version(void);

/* Host only.  Floats of the packed form of n_queries queries (a negative code outside 1..BD_SEARCH_MAX_QUERIES). */
BD_API int64_t bd_search_packed_floats(int32_t n_queries);

/* Host only.  queries [n_queries][BD_SEARCH_DIM] -> packed [bd_search_packed_floats(n_queries)], both in host memory. */
BD_API int bd_search_pack_queries(const float* queries, int32_t n_queries, float* packed);

BD_API int bd_search_norms(const float* e_dev, int64_t windows, float* n2_dev, void* stream);
BD_API int bd_search_norms_host(const float* e, int64_t windows, float* n2);

/* n2_dev: the rows' squared norms (bd_search_norms) for BD_SEARCH_COSINE; not read for BD_SEARCH_DOT (may be null). */
BD_API int bd_search_scores(const float* e_dev, int64_t windows, const float* packed_dev, int32_t n_queries, int32_t metric,
                            const float* n2_dev, float* scores_dev, int64_t row_stride, int64_t col_stride, void* stream);

BD_API int bd_search_update(const float* scores_dev, int64_t windows, int32_t n_queries, int64_t row_stride, int64_t col_stride,
                            int64_t base_id, uint64_t* keys_dev, int32_t k, void* stream);
BD_API int bd_search_update_host(const float* scores, int64_t windows, int32_t n_queries, int64_t row_stride, int64_t col_stride,
                                 int64_t base_id, uint64_t* keys, int32_t k);

/* Host only.  n keys -> scores[n], ids[n]; an empty slot gives (-INFINITY, 0xFFFFFFFF).  Returns the number of real keys. */
BD_API int64_t bd_search_decode_host(const uint64_t* keys, int64_t n, float* scores, uint32_t* ids);

#ifdef __cplusplus
}
#endif

#endif /* BUZZDETECT_SEARCH_H */
