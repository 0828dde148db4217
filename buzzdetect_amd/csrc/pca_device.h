// The arithmetic of the streaming PCA (include/buzzdetect_pca.h) that the kernels of pca.hip and its host restatements
// (bd_pca_sums_host, bd_pca_gram_host, bd_pca_project_host) both compile from, as cluster_device.h is for the clustering: the
// term of a row, the steps of the chains, where a tile of the upper triangle lies in a partial, which element an accumulator
// register of the matrix instruction holds, and what the projection makes of a score.  The norm chain's butterfly is
// simsearch_device.h's.
#ifndef BD_PCA_DEVICE_H
#define BD_PCA_DEVICE_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/buzzdetect_pca.h"
#include "simsearch_device.h"

#pragma clang fp contract(off)

namespace bd {
namespace pca {

constexpr int kDim = BD_PCA_DIM;
constexpr int kTilesAcross = BD_PCA_DIM / 32;                        // 32 x 32 tiles along one side of the Gram matrix
constexpr int kTiles = kTilesAcross * (kTilesAcross + 1) / 2;        // ... and in its upper triangle, the diagonal included
constexpr int kTileFloats = 32 * 32;
static_assert(BD_PCA_DIM == BD_SEARCH_DIM, "the rows are the search's rows");
static_assert(kTiles == 528, "the header states the workspace in these tiles");
static_assert(BD_PCA_SLICE % 2 == 0, "a matrix instruction takes two rows of a slice");

// a row id as the kernels index with it (the host restatements refuse what this would change)
__host__ __device__ inline int64_t clamp_row(int64_t id, int64_t rows_total) {
    return id < 0 ? 0 : (id >= rows_total ? rows_total - 1 : id);
}

// a row whose squared norm is not finite is absent: it holds a NaN or an infinity, or its norm overflows
__host__ __device__ inline bool row_present(float n2) { return n2 - n2 == 0.0f; }

// t(r, c) of a present row: one rounded subtraction, or the element itself where there is no shift
__host__ __device__ inline float term(float x, float shift) { return x - shift; }

// one step of a chain of sums (a column's partial over its rows, a tile's total over its slices, q over the components)
__host__ __device__ inline float chain_add(float acc, float x) { return acc + x; }

// one step of a Gram partial's chain: what the matrix instruction does with one k (fmaf, spelt so that the host compiler may
// take a fused multiply-add instruction for it where the processor has one)
__host__ __device__ inline float gram_step(float a, float b, float acc) { return __builtin_fmaf(a, b, acc); }

// where tile (ti, tj), ti <= tj, lies among the kTiles tiles of a partial
__host__ __device__ inline int tile_index(int ti, int tj) { return ti * kTilesAcross - ti * (ti - 1) / 2 + (tj - ti); }

// the row (within its tile) of accumulator register r in lane l of v_mfma_f32_32x32x2_f32; the column is l & 31
__host__ __device__ inline int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// lane l's part of the squared norm of a centred row: (row[l + 64 j] - mean[l + 64 j])^2, j ascending, the difference rounded,
// then one fused multiply-add each, from 0 (simsearch_device.h's norm_chain over the centred row)
__host__ __device__ inline float centred_norm_chain(const float* __restrict__ row, const float* __restrict__ mean, int lane) {
    float a = 0.0f;
#pragma unroll
    for (int j = 0; j < search::kChainSteps; ++j) {
        const float x = row[lane + 64 * j] - mean[lane + 64 * j];
        a = fmaf(x, x, a);
    }
    return a;
}

// u = s - mv[j]
__host__ __device__ inline float centred_score(float s, float mv) { return s - mv; }

// y[w][j] of a present row
__host__ __device__ inline float coordinate(float u, float scale) { return u * scale; }

// one step of q's chain: the product is rounded, then added
__host__ __device__ inline float energy_step(float q, float u) {
    const float p = u * u;
    return q + p;
}

// resid[w] of a present row
__host__ __device__ inline float residual(float c2, float q) { return fmaxf(c2 - q, 0.0f); }

__host__ __device__ inline float quiet_nan() { return search::bits_float(0x7FC00000u); }

}  // namespace pca
}  // namespace bd

#endif  // BD_PCA_DEVICE_H
