// The arithmetic of the neighbour lists (include/buzzdetect_knn.h) that the kernels of knn.hip and its host restatement
// (bd_knn_update_host) both compile from, as cluster_device.h is for the clustering: the order of a dot's chain, the root a row
// enters a cosine with, the similarity, and the key of a candidate.  The key format and its order are simsearch_device.h's.
#ifndef BD_KNN_DEVICE_H
#define BD_KNN_DEVICE_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/buzzdetect_knn.h"
#include "cluster_device.h"
#include "simsearch_device.h"

#pragma clang fp contract(off)

namespace bd {
namespace knn {

static_assert(BD_KNN_DIM == BD_SEARCH_DIM && BD_KNN_DIM % 8 == 0, "the rows are the search's rows, whole groups of eight");

// the channel of step t of a dot's chain: groups of eight ascending, inside a group 0, 4, 1, 5, 2, 6, 3, 7 (dense_tile_walk:
// instruction j of a super-step takes channel j from the lower half of the wave, then channel 4 + j from the upper)
__host__ __device__ inline int chain_channel(int t) { return (t & ~7) + ((t & 7) >> 1) + 4 * (t & 1); }

__host__ __device__ inline float dot_step(float a, float b, float acc) { return fmaf(a, b, acc); }

// what a row enters a cosine with: the root of its squared norm, 0.0f for a row below the norm floor
__host__ __device__ inline float root(float n2) { return n2 < BD_SEARCH_NORM_FLOOR ? 0.0f : sqrtf(n2); }

__host__ __device__ inline float similarity(float dot, float root_q, float root_c, int metric) {
    if (metric != BD_KNN_COSINE) return dot;
    if (root_q == 0.0f || root_c == 0.0f) return 0.0f;
    return cluster::div_rn(dot, root_q * root_c);
}

}  // namespace knn
}  // namespace bd

#endif  // BD_KNN_DEVICE_H
