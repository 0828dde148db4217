// The arithmetic of search by example (include/buzzdetect_search.h) that the kernels of simsearch.hip and its host restatements
// (bd_search_norms_host, bd_search_update_host) both compile from, as ensemble_device.h is for the ensemble: a lane's chain of
// a row's squared norm, the butterfly the 64 chains meet in, and the key of a (score, id) candidate with its inverse.
#ifndef BD_SIMSEARCH_DEVICE_H
#define BD_SIMSEARCH_DEVICE_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/buzzdetect_search.h"

namespace bd {
namespace search {

constexpr int kChainSteps = BD_SEARCH_DIM / 64;
static_assert(BD_SEARCH_DIM % 64 == 0, "a row is whole rounds of a wave");

// lane l's part of a row's squared norm: row[l + 64 j]^2, j ascending, one fused multiply-add each, from 0
__host__ __device__ inline float norm_chain(const float* __restrict__ row, int lane) {
    float a = 0.0f;
#pragma unroll
    for (int j = 0; j < kChainSteps; ++j) {
        const float x = row[lane + 64 * j];
        a = fmaf(x, x, a);
    }
    return a;
}

// one step of the butterfly: what a lane holds after v += v[lane ^ m] (a plain sum, nothing to contract)
__host__ __device__ inline float butterfly_add(float mine, float other) { return mine + other; }

// the butterfly over a wave, m = 32, 16, .. 1: every lane ends with the same sum
__device__ inline float butterfly_wave(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = butterfly_add(v, __shfl_xor(v, m, 64));
    return v;
}

// the same over 64 values on the host; the sum is v[0] (and every other element)
inline float butterfly_host(float* v) {
    for (int m = 32; m >= 1; m >>= 1) {
        float t[64];
        for (int lane = 0; lane < 64; ++lane) t[lane] = butterfly_add(v[lane], v[lane ^ m]);
        for (int lane = 0; lane < 64; ++lane) v[lane] = t[lane];
    }
    return v[0];
}

__host__ __device__ inline uint32_t float_bits(float x) {
#ifdef __HIP_DEVICE_COMPILE__
    return __float_as_uint(x);
#else
    uint32_t u;
    std::memcpy(&u, &x, 4);
    return u;
#endif
}

__host__ __device__ inline float bits_float(uint32_t u) {
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(u);
#else
    float x;
    std::memcpy(&x, &u, 4);
    return x;
#endif
}

// a NaN counts as -INFINITY, -0.0f as +0.0f
__host__ __device__ inline float canonical_score(float s) {
    if (s != s) return -INFINITY;
    if (s == 0.0f) return 0.0f;
    return s;
}

// the key of candidate (score, id): larger is better - the higher score, then the lower id; never 0 for id < 0xFFFFFFFF
__host__ __device__ inline uint64_t make_key(float score, uint32_t id) {
    const uint32_t b = float_bits(canonical_score(score));
    const uint32_t m = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)m << 32) | (uint64_t)(0xFFFFFFFFu - id);
}

__host__ __device__ inline float key_score(uint64_t key) {
    const uint32_t m = (uint32_t)(key >> 32);
    return bits_float((m & 0x80000000u) ? (m & 0x7FFFFFFFu) : ~m);
}

__host__ __device__ inline uint32_t key_id(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFu); }

}  // namespace search
}  // namespace bd

#endif  // BD_SIMSEARCH_DEVICE_H
