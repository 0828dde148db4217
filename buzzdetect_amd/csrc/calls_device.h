// The small pieces of detection calling (include/buzzdetect_calls.h) that the kernels of calls.hip and its host restatements
// (bd_calls_events_host, bd_calls_bins_host) must agree on bit for bit and therefore both compile from, as ensemble_device.h and
// cluster_device.h are for theirs: what a score does to the state under a rule, the peak comparison, a tick difference, the
// maximum's canonical zero, a lane's chain of a bin's sum and the butterfly the 64 chains meet in.
#ifndef BD_CALLS_DEVICE_H
#define BD_CALLS_DEVICE_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/buzzdetect_calls.h"

namespace bd {
namespace calls {

enum Verdict : int { kKeep = 0, kSwitchOn = 1, kSwitchOff = 2 };

// what score v does to the state: above high it switches on, not above low (a NaN included) it switches off, between it keeps
__host__ __device__ inline Verdict classify(float v, float high, float low) {
    if (v > high) return kSwitchOn;
    if (!(v > low)) return kSwitchOff;
    return kKeep;
}

// whether score v takes the peak from the score that holds it (a tie leaves it with the earlier window)
__host__ __device__ inline bool peak_beats(float v, float held) { return v > held; }

// ticks from window a to window b
__host__ __device__ inline int64_t ticks_between(int32_t t_a, int32_t t_b) { return (int64_t)t_b - (int64_t)t_a; }

// the running maximum of a bin after score v: a NaN is ignored, -0.0f counts as +0.0f
__host__ __device__ inline float max_take(float held, float v) {
    if (v != v) return held;
    if (v == 0.0f) v = 0.0f;
    return v > held ? v : held;
}

// lane l's part of a bin's sum: windows lo + l + 64 j below hi, j ascending, from 0.0f, one addition each
__host__ __device__ inline float sum_chain(const float* __restrict__ col, int64_t row_stride, int lo, int hi, int lane) {
    float a = 0.0f;
    for (int w = lo + lane; w < hi; w += 64) a = a + col[(int64_t)w * row_stride];
    return a;
}

// one step of the butterfly: what a lane holds after v += v[lane ^ m]
__host__ __device__ inline float butterfly_add(float mine, float other) { return mine + other; }

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

// a sum as it is stored: every NaN becomes the quiet NaN 0x7FC00000
__host__ __device__ inline float stored_sum(float s) {
    if (s == s) return s;
    const uint32_t u = 0x7FC00000u;
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(u);
#else
    float x;
    std::memcpy(&x, &u, 4);
    return x;
#endif
}

}  // namespace calls
}  // namespace bd

#endif  // BD_CALLS_DEVICE_H
