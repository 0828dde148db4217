// Device code of the attached heads (headset.hip: a lone stack or many stacks behind one embedder pass): the walk of one wave
// over K for its 32 x 32 tile of C, the activation, and the order of a softmax row.  simsearch.hip and cluster.hip take the walk
// for their own products.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/buzzdetect_head.h"

namespace bd {

typedef float dense_v16f __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float head_act(float x, int act) {
    if (act == BD_HEAD_RELU) return fmaxf(x, 0.0f);
    if (act == BD_HEAD_SIGMOID) return 1.0f / (1.0f + expf(-x));
    if (act == BD_HEAD_TANH) return tanhf(x);
    return x;                                   // linear, and softmax (a row pass follows)
}

// One wave's 32 x 32 tile of A W: ap = the lane's row of A at k = 4 (lane >> 5), bp = the tile's packed fragments at this lane
// (headmlp.hip: operand map).  K is walked alone in ascending super-steps of 8, four super-steps (32 k) in flight ahead of the
// sixteen matrix instructions that use them; elements at k >= K are replaced by zero.  n_super is a multiple of 4.
// Accumulator r of lane l is C[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31] of the tile.
__device__ __forceinline__ dense_v16f dense_tile_walk(const float* __restrict__ ap, const float4* __restrict__ bp, int K,
                                                      int n_super, int half) {
    float4 a[4], b[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        a[q] = *reinterpret_cast<const float4*>(ap + 8 * q);
        b[q] = bp[(size_t)q * 64];
    }
    dense_v16f acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int s = 0; s < n_super; s += 4) {
        float4 an[4], bn[4];
        const bool more = s + 4 < n_super;
        if (more) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                an[q] = *reinterpret_cast<const float4*>(ap + 8 * (s + 4 + q));
                bn[q] = bp[(size_t)(s + 4 + q) * 64];
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k0 = 8 * (s + q) + 4 * half;
            const float ax = k0 + 0 < K ? a[q].x : 0.0f;
            const float ay = k0 + 1 < K ? a[q].y : 0.0f;
            const float az = k0 + 2 < K ? a[q].z : 0.0f;
            const float aw = k0 + 3 < K ? a[q].w : 0.0f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ax, b[q].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ay, b[q].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(az, b[q].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aw, b[q].w, acc, 0, 0, 0);
        }
        if (more) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a[q] = an[q];
                b[q] = bn[q];
            }
        }
    }
    return acc;
}

// The tile's epilogue: bias, activation, the rows below W and the columns below N of C (tile row tr, tile column tc)
__device__ __forceinline__ void dense_tile_store(const dense_v16f& acc, const float* __restrict__ bias, int act, int tr, int tc,
                                                 int W, int N, float* __restrict__ C, int ldc, int lane) {
    const int col = 32 * tc + (lane & 31);
    if (col >= N) return;
    const float bv = bias[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = 32 * tr + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < W) C[(size_t)row * ldc + col] = head_act(acc[r] + bv, act);
    }
}

// softmax of one row p[0..n) into q[0..n) by one wave: lane l takes columns l, l + 64, ... in ascending order, the 64 partial
// results meet in a butterfly - the same order for every row wherever it sits
__device__ __forceinline__ void softmax_row(const float* __restrict__ p, float* __restrict__ q, int n, int lane) {
    float m = -INFINITY;
    for (int c = lane; c < n; c += 64) m = fmaxf(m, p[c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float sum = 0.0f;
    for (int c = lane; c < n; c += 64) sum += expf(p[c] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    for (int c = lane; c < n; c += 64) q[c] = expf(p[c] - m) / sum;
}

}  // namespace bd
