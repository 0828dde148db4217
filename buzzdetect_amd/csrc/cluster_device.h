// The arithmetic of k-means clustering (include/buzzdetect_cluster.h) that the kernels of cluster.hip and its host restatements
// (bd_cluster_order_host, bd_cluster_centroids_host, bd_cluster_stats_host) both compile from, as simsearch_device.h is for
// the search: a member's term and the step of a chunk's chain, the centroid's division, a lane's part of a slice's statistics,
// and where a centroid's element lies in the packed form.  The norm chain and the butterfly are simsearch_device.h's.
#ifndef BD_CLUSTER_DEVICE_H
#define BD_CLUSTER_DEVICE_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/buzzdetect_cluster.h"
#include "simsearch_device.h"

#pragma clang fp contract(off)

namespace bd {
namespace cluster {

constexpr int kDim = BD_CLUSTER_DIM;
constexpr int kSuper = BD_CLUSTER_DIM / 8;               // super-steps of the walk over a row
static_assert(BD_CLUSTER_DIM == BD_SEARCH_DIM, "the rows are the search's rows");
static_assert(BD_CLUSTER_STAT_SLICE == 4 * 64, "a lane takes four rows of a slice");

// one correctly rounded division on both sides
__host__ __device__ inline float div_rn(float a, float b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

// a label as the kernels index with it (the host restatement refuses what this would change)
__host__ __device__ inline int clamp_label(int label, int n_clusters) {
    return label < 0 ? 0 : (label >= n_clusters ? n_clusters - 1 : label);
}

// 1 / |row| for a cosine, 0 for a row below the norm floor
__host__ __device__ inline float row_rinv(float n2) { return n2 < BD_SEARCH_NORM_FLOOR ? 0.0f : div_rn(1.0f, sqrtf(n2)); }

// what a member adds to its chunk's partial: the element, or for a cosine the element of the row at unit length (rounded)
__host__ __device__ inline float member_term(float x, float rinv, int metric) { return metric == BD_CLUSTER_COSINE ? x * rinv : x; }

// one step of a chain of sums (a chunk's partial over its members, a cluster's sum over its partials)
__host__ __device__ inline float chain_add(float acc, float x) { return acc + x; }

// a cluster with no members, or whose cosine sum has no direction, keeps its centroid
__host__ __device__ inline bool keeps_previous(int count, float m2, int metric) {
    return count == 0 || (metric == BD_CLUSTER_COSINE && m2 < BD_SEARCH_NORM_FLOOR);
}

// what the sum row is divided by: the count, or for a cosine the length of the sum row
__host__ __device__ inline float centroid_denominator(int count, float m2, int metric) {
    return metric == BD_CLUSTER_COSINE ? sqrtf(m2) : (float)count;
}

__host__ __device__ inline float centroid_value(float sum, float denominator) { return div_rn(sum, denominator); }

// the distance bd_cluster_assign stores for a row with squared norm n2 whose best candidate has t_best
__host__ __device__ inline float assigned_distance(float n2, float t_best, int metric) {
    if (metric == BD_CLUSTER_COSINE) return n2 < BD_SEARCH_NORM_FLOOR ? 1.0f : 1.0f - div_rn(-t_best, sqrtf(n2));
    return fmaxf(n2 + t_best, 0.0f);
}

// lane l's part of a slice's inertia: dist of rows first + l + 64 u, u = 0 .. 3 in that order, from 0; rows past W count as 0
__host__ __device__ inline float stat_chain(const float* __restrict__ dist, int64_t first, int64_t rows, int lane) {
    float a = 0.0f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t r = first + lane + 64 * u;
        a = a + (r < rows ? dist[r] : 0.0f);
    }
    return a;
}

// lane l's part of a slice's count of rows whose label changed
__host__ __device__ inline int stat_changed(const int32_t* __restrict__ labels, const int32_t* __restrict__ prev, int64_t first,
                                            int64_t rows, int lane) {
    int n = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t r = first + lane + 64 * u;
        n += r < rows && labels[r] != prev[r] ? 1 : 0;
    }
    return n;
}

// where channels 4 q .. 4 q + 3 of centroid j lie in the packed form, in units of four floats (headmlp.hip: dense_pack_weights
// with k = 1024: super-step q / 2, half q & 1, lane (q & 1) * 32 + j % 32 of column tile j / 32)
__host__ __device__ inline size_t packed_quad(int j, int q) {
    return ((size_t)(j >> 5) * kSuper + (size_t)(q >> 1)) * 64 + (size_t)((q & 1) * 32 + (j & 31));
}

// chunks of a cluster with n members
__host__ __device__ inline int chunks_of(int n) { return (n + BD_CLUSTER_CHUNK - 1) / BD_CLUSTER_CHUNK; }

}  // namespace cluster
}  // namespace bd

#endif  // BD_CLUSTER_DEVICE_H
