/*
 * buzzdetect_cluster.h — C ABI of k-means clustering in libbuzzdetect_hip.so (gfx950): one Lloyd iteration over [W][1024]
 * embeddings where they lie, for buzzdetect_amd/cluster.py.  No [W][K] matrix is written, no row goes back to the host, and
 * a fit is reproducible bit for bit.
 *
 *   bd_cluster_workspace_bytes   host only: the scratch bd_cluster_order and bd_cluster_centroids take for (rows, n_clusters)
 *   bd_cluster_assign            labels[w] = the nearest centroid of row w, dist[w] = its distance
 *   bd_cluster_order             the row ids sorted by (label, row id), and where each cluster's segment starts
 *                                                                            (bd_cluster_order_host: the same on the host)
 *   bd_cluster_centroids         the next centroids from the ordered rows: row-major, packed for the next assign, and their
 *                                squared norms                               (bd_cluster_centroids_host: the same bits)
 *   bd_cluster_stats             per slice of 256 rows: the sum of dist and the number of rows whose label changed
 *                                                                            (bd_cluster_stats_host: the same bits)
 *
 * Notation.  E is [W][BD_CLUSTER_DIM] float32, 16-byte aligned.  K = n_clusters.  n2[w] is bd_search_norms of E
 * (buzzdetect_search.h), c2[j] the same chain and butterfly over centroid j.  metric is BD_CLUSTER_EUCLIDEAN or BD_CLUSTER_COSINE;
 * for a cosine the centroids have unit length (the caller brings the first ones there in double, then float; bd_cluster_centroids
 * keeps them there).  Every step named below is one correctly rounded float32 operation, and nothing is contracted into a fused
 * multiply-add except where fmaf is named.
 *
 * Assign.  The centroids lie in the fragment order bd_search_pack_queries writes (K columns, zero-padded to tiles of 32).  One
 * wave owns 32 rows and walks the column tiles one after another, each by the walk of the Dense heads over K = 1024: the score
 * s(w, j) = dot(E[w], C[j]) has exactly the bits bd_search_scores(..., BD_SEARCH_DOT) stores for the same rows and the same
 * packed matrix.  t = c2[j] - 2.0f * s (Euclidean; the product is exact) or t = -s (cosine; c2 is not read, may be null).  A NaN
 * t counts as +INFINITY.  labels[w] is the j of the smallest t, among equal t the lowest j, and 0 if every t is +INFINITY.  A
 * lane keeps the best (t, j) of its own columns in registers; the 32 lanes of a half meet in a butterfly on (t, j) pairs at the
 * end.  Padded columns j >= K hold (+INFINITY, j) and lose every tie against column 0.  With t_best the winner's t:
 *   Euclidean   dist[w] = fmaxf(n2[w] + t_best, 0.0f)                                        (the squared distance)
 *   cosine      dist[w] = 1.0f - (-t_best) / sqrtf(n2[w]), and 1.0f where n2[w] < BD_SEARCH_NORM_FLOOR
 * A label's and a distance's bits depend on the row and the centroid set alone, not on W or on where the row sits.
 *
 * Order.  A stable counting sort: order[offsets[j] .. offsets[j + 1]) are the rows with label j in ascending row id,
 * offsets[K] = W.  Slices of BD_CLUSTER_ORDER_SLICE rows are counted (integer additions in LDS, whose sum does not depend on
 * their order), one workgroup scans the counts over slices and clusters, and one wave per slice places its rows in ascending
 * order: a row's place is the slice's base for its label plus the number of earlier rows of the slice with that label.  Labels
 * must lie in 0 .. K - 1, as bd_cluster_assign writes them: the host restatement refuses others (BD_ERANGE); the device cannot
 * look before it launches and takes a label outside as the nearest end of the range, so that nothing is written out of bounds.
 *
 * Sums and centroids.  The members of cluster j in ascending row id are cut into chunks of BD_CLUSTER_CHUNK.  A chunk's partial
 * is, per channel c, the chain 0.0f + x_0 + x_1 + ... in that order, where x = E[r][c] (Euclidean) or E[r][c] * rinv[r]
 * (cosine: the product is rounded, then added; rinv[r] = 1.0f / sqrtf(n2[r]), and 0.0f where n2[r] < BD_SEARCH_NORM_FLOOR).
 * The cluster's sum is the chain over its chunks' partials in ascending order, starting from the first partial.  The centroid
 * is sum / (float)count (Euclidean) or sum / sqrtf(m2) (cosine), m2 being the norm chain and butterfly of buzzdetect_search.h
 * over the sum row.  A cluster with no members, and for a cosine one with m2 < BD_SEARCH_NORM_FLOOR, keeps the row of `prev` bit
 * for bit.  One workgroup per (cluster, chunk) reads whole 4 KB rows through `order`; one workgroup per cluster finishes and
 * writes three things, each element once: the centroids row-major, their packed form (bit-equal to bd_search_pack_queries of
 * those rows, padding included) and c2 (bit-equal to bd_search_norms_host of those rows).
 *
 * Statistics.  Rows are taken in slices of BD_CLUSTER_STAT_SLICE = 256.  partial[slice]: lane l adds dist of rows l, l + 64,
 * l + 128, l + 192 of the slice in that order, from 0.0f, rows past W as 0.0f; the 64 sums meet in the butterfly m = 32 .. 1.
 * changed[slice] is the number of rows of the slice with labels[r] != prev_labels[r].  There are (W + 255) / 256 slices; the
 * host adds the partials in float64 (the inertia) and the counts.
 *
 * No floating-point number is added atomically, no result depends on the grid, every output element has one writer, inputs
 * are only read, and all element offsets are 64-bit.
 *
 * Limits (refused on the host with the argument named, nothing launched): 1 <= K <= BD_CLUSTER_MAX_CLUSTERS,
 * 0 <= W <= BD_CLUSTER_MAX_ROWS per call (W = 0 launches nothing and writes nothing, on the host too; a count up to 2^24 is
 * exact in float32), a known metric, non-null
 * pointers (E, the packed centroids, the centroid rows and the workspace 16-byte aligned, everything else 4-byte aligned), and
 * a workspace of at least bd_cluster_workspace_bytes(W, K) bytes (BD_EWORKSPACE).
 *
 * Conventions are those of buzzdetect_hip.h: 0 on success, a negative BD_E* code on failure, bd_last_error() for the text; the
 * caller owns all device memory; `stream` is a hipStream_t.
 */
#ifndef BUZZDETECT_CLUSTER_H
#define BUZZDETECT_CLUSTER_H

#include <stdint.h>

#include "buzzdetect_hip.h"
#include "buzzdetect_search.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BD_CLUSTER_ABI_VERSION 1
#define BD_CLUSTER_DIM 1024                     /* floats per row: BD_SEARCH_DIM */
#define BD_CLUSTER_MAX_CLUSTERS 1024
#define BD_CLUSTER_MAX_ROWS (1 << 24)           /* rows per call */
#define BD_CLUSTER_CHUNK 256                    /* members per partial sum */
#define BD_CLUSTER_STAT_SLICE 256               /* rows per partial of the statistics */
#define BD_CLUSTER_ORDER_SLICE 1024             /* rows one wave places */
#define BD_CLUSTER_EUCLIDEAN 0
#define BD_CLUSTER_COSINE 1

BD_API int bd_cluster_abi_version(void);

/* Host only.  Bytes of scratch for bd_cluster_order and bd_cluster_centroids (a negative code for arguments out of range). */
BD_API int64_t bd_cluster_workspace_bytes(int64_t rows, int32_t n_clusters);

/* packed_dev: bd_search_pack_queries of the centroids; c2_dev: their squared norms (not read for BD_CLUSTER_COSINE). */
BD_API int bd_cluster_assign(const float* e_dev, int64_t rows, const float* n2_dev, const float* packed_dev, const float* c2_dev,
                             int32_t n_clusters, int32_t metric, int32_t* labels_dev, float* dist_dev, void* stream);

/* order [rows], offsets [n_clusters + 1] */
BD_API int bd_cluster_order(const int32_t* labels_dev, int64_t rows, int32_t n_clusters, int32_t* order_dev, int32_t* offsets_dev,
                            void* workspace_dev, int64_t workspace_bytes, void* stream);
BD_API int bd_cluster_order_host(const int32_t* labels, int64_t rows, int32_t n_clusters, int32_t* order, int32_t* offsets);

/* prev, centroids [n_clusters][BD_CLUSTER_DIM]; packed [bd_search_packed_floats(n_clusters)]; c2 [n_clusters].  n2 is read for
 * BD_CLUSTER_COSINE only (may be null otherwise). */
BD_API int bd_cluster_centroids(const float* e_dev, int64_t rows, const float* n2_dev, const int32_t* order_dev,
                                const int32_t* offsets_dev, int32_t n_clusters, int32_t metric, const float* prev_dev,
                                float* centroids_dev, float* packed_dev, float* c2_dev, void* workspace_dev,
                                int64_t workspace_bytes, void* stream);
BD_API int bd_cluster_centroids_host(const float* e, int64_t rows, const float* n2, const int32_t* order, const int32_t* offsets,
                                     int32_t n_clusters, int32_t metric, const float* prev, float* centroids, float* packed,
                                     float* c2);

/* partial, changed [(rows + 255) / 256] */
BD_API int bd_cluster_stats(const float* dist_dev, const int32_t* labels_dev, const int32_t* prev_labels_dev, int64_t rows,
                            float* partial_dev, int32_t* changed_dev, void* stream);
BD_API int bd_cluster_stats_host(const float* dist, const int32_t* labels, const int32_t* prev_labels, int64_t rows,
                                 float* partial, int32_t* changed);

#ifdef __cplusplus
}
#endif

#endif /* BUZZDETECT_CLUSTER_H */
