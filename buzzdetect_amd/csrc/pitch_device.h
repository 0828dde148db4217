// Everything of wingbeat pitch tracking (include/buzzdetect_pitch.h) that the kernel of pitch.hip and its host restatement
// (bd_pitch_windows_host) must agree on bit for bit and therefore both compile from, as calls_device.h and suggest_device.h are
// for theirs: the order of the mean, the chains of a lag's cross term and energy and how they meet, the division, the rules of
// the lobe, the run and the argmax, the interpolation, the median's order and the canonical NaN.  Where a fused operation is
// meant, fmaf is written out, and contraction is off for everything else, so that neither side fuses what the other does not.
// What differs between the two sides is only how the lags of a frame meet: butterflies over the wave on the device, a serial
// walk on the host - over minima and maxima of values that hold no NaN and no -0.0, which do not depend on the order.
#ifndef BD_PITCH_DEVICE_H
#define BD_PITCH_DEVICE_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/buzzdetect_pitch.h"

#pragma clang fp contract(off)

namespace bd {
namespace pitch {

constexpr int kNoLag = 1 << 30;                 // "no such lag" in a minimum over lags

// the f0 of a window without enough voiced frames
__host__ __device__ inline float quiet_nan() {
    const uint32_t u = 0x7FC00000u;
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(u);
#else
    float x;
    std::memcpy(&x, &u, 4);
    return x;
#endif
}

// neither an infinity nor a NaN
__host__ __device__ inline bool finite(float v) { return fabsf(v) <= 3.402823466e+38f; }

// lane l's part of a frame's sum: samples l + 64 i, i ascending, from 0.0f, one addition each
__host__ __device__ inline float mean_chain(const float* frame, int lane) {
    float a = 0.0f;
    for (int i = 0; i < BD_PITCH_FRAME / 64; ++i) a = a + frame[lane + 64 * i];
    return a;
}

// one step of the butterfly the 64 chains meet in: what a lane holds after v += v[lane ^ m], m = 32, 16, .. 1
__host__ __device__ inline float butterfly_add(float mine, float other) { return mine + other; }

// the same over 64 values on the host; the sum is v[0] (and every other element)
inline float butterfly_host(float* v) {
    for (int m = 32; m >= 1; m >>= 1) {
        float t[64];
        for (int lane = 0; lane < 64; ++lane) t[lane] = butterfly_add(v[lane], v[lane ^ m]);
        for (int lane = 0; lane < 64; ++lane) v[lane] = t[lane];
    }
    return v[0];
}

// the mean from the sum: an exact scaling
__host__ __device__ inline float mean_of(float total) { return total * (1.0f / (float)BD_PITCH_FRAME); }

struct Sums {
    float cross;                                // sum_{j<512} y[j] y[j+tau]
    float energy;                               // sum_{j<512} y[j+tau]^2
};

// The two sums of lag tau over y = frame - mu.  Four chains each: chain k takes j = 4 i + k, i ascending, from 0.0f, one fused
// multiply-add per product; they meet as (c0 + c1) + (c2 + c3).  The eight chains are independent, which hides the latency of
// a fused multiply-add; frame[j] is the same address in every lane, frame[j + tau] consecutive addresses in consecutive lanes.
// The energy of lag 0 is the other energy term of every lag.
__host__ __device__ inline Sums lag_sums(const float* frame, float mu, int tau) {
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f, e0 = 0.0f, e1 = 0.0f, e2 = 0.0f, e3 = 0.0f;
    const float* shifted = frame + tau;
    for (int j = 0; j < BD_PITCH_INTEGRATION; j += 4) {
        const float a0 = frame[j] - mu, a1 = frame[j + 1] - mu, a2 = frame[j + 2] - mu, a3 = frame[j + 3] - mu;
        const float b0 = shifted[j] - mu, b1 = shifted[j + 1] - mu, b2 = shifted[j + 2] - mu, b3 = shifted[j + 3] - mu;
        c0 = fmaf(a0, b0, c0);
        c1 = fmaf(a1, b1, c1);
        c2 = fmaf(a2, b2, c2);
        c3 = fmaf(a3, b3, c3);
        e0 = fmaf(b0, b0, e0);
        e1 = fmaf(b1, b1, e1);
        e2 = fmaf(b2, b2, e2);
        e3 = fmaf(b3, b3, e3);
    }
    Sums s;
    s.cross = (c0 + c1) + (c2 + c3);
    s.energy = (e0 + e1) + (e2 + e3);
    return s;
}

// n[tau] from the lag's sums and the energy of lag 0; *m is what must be finite.  -0.0f is stored as +0.0f: maxima over n do
// then not depend on their order.
__host__ __device__ inline float normalised(float cross, float energy0, float energy, float* m) {
    *m = energy0 + energy;
    float n = *m > 0.0f ? (2.0f * cross) / *m : 0.0f;
    if (n == 0.0f) n = 0.0f;
    return n;
}

// the lag-0 lobe ends at the first lag whose n is below zero
__host__ __device__ inline bool ends_lobe(float n) { return n < 0.0f; }

// a frame whose greatest n is not at least clarity_min is unvoiced (a NaN is not)
__host__ __device__ inline bool clear_enough(float nmax, float clarity_min) { return nmax >= clarity_min; }

__host__ __device__ inline float run_threshold(float pick_ratio, float nmax) { return pick_ratio * nmax; }

// whether a lag belongs to a run above the threshold
__host__ __device__ inline bool in_run(float n, float thr) { return n >= thr; }

// the frame's f0 from the picked lag i, n[i-1], n[i] and n[i+1]: the vertex of the parabola through the three, at most half a
// lag from i; a flat or convex triple keeps i
__host__ __device__ inline float refined_f0(int i, float before, float at, float after, float rate_hz) {
    const float den = (before - 2.0f * at) + after;
    float d = 0.0f;
    if (den < 0.0f) {
        d = (0.5f * (before - after)) / den;
        d = d < -0.5f ? -0.5f : (d > 0.5f ? 0.5f : d);
    }
    return rate_hz / ((float)i + d);
}

// the median's total order over voiced frames: by f0, then by frame index
__host__ __device__ inline bool ordered_before(float f0_a, int a, float f0_b, int b) { return f0_a < f0_b || (f0_a == f0_b && a < b); }

// the place of the lower median among `voiced` frames in that order
__host__ __device__ inline int median_rank(int voiced) { return (voiced - 1) / 2; }

}  // namespace pitch
}  // namespace bd

#endif  // BD_PITCH_DEVICE_H
