// The arithmetic of include/buzzdetect_suggest.h that the kernels of suggest.hip and its host restatements
// (bd_suggest_acquire_host, bd_suggest_pick_host) both compile from, as ensemble_device.h, simsearch_device.h and calls_device.h
// are for theirs.  What differs between the two sides of the acquisition is only how a row's terms meet (butterflies over the
// wave on the device, a serial sum on the host) and whose expf / logf is called; the pick has nothing that differs.
#ifndef BD_SUGGEST_DEVICE_H
#define BD_SUGGEST_DEVICE_H

#include "ensemble_device.h"
#include "simsearch_device.h"

#include "../../include/buzzdetect_suggest.h"

namespace bd {
namespace suggest {

// p log p from p and its logarithm, 0 at p = 0 (where log p may be -INFINITY); a NaN p stays NaN
__host__ __device__ inline float term(float p, float logp) { return p == 0.0f ? 0.0f : p * logp; }

// x log x, 0 at x = 0; a NaN stays NaN
__host__ __device__ inline float xlogx(float x) { return x == 0.0f ? 0.0f : x * logf(x); }

// into [0, 1]; a NaN stays NaN (fminf / fmaxf would drop it)
__host__ __device__ inline float unit(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }

// one member's (q, r) = (class t, not class t) and their logarithms
struct Binary {
    float q, r, logq, logr;
};

// softmax: d_t = z[t] - max, e_t = expf(d_t), s = sum of all e, s_other = sum of the e of the classes but t, ls = logf(s)
__host__ __device__ inline Binary binary_softmax(float d_t, float e_t, float s, float s_other, float ls) {
    Binary b;
    b.q = e_t / s;
    b.r = s_other / s;
    // near 1 a probability's logarithm is taken from the other one, which is small and carries its digits
    b.logq = b.r < 0.5f ? log1pf(-b.r) : d_t - ls;
    b.logr = b.q < 0.5f ? log1pf(-b.q) : logf(s_other) - ls;
    return b;
}

__host__ __device__ inline Binary binary_sigmoid(float z) {
    Binary b;
    b.logq = ens::log_sigmoid(z);
    b.logr = ens::log_sigmoid(-z);
    b.q = expf(b.logq);
    b.r = expf(b.logr);
    return b;
}

// The three scores from a = sum_c pbar[c] log pbar[c], b = sum_c sum_m p_m[c] log p_m[c] and gap = largest - second largest
// of pbar (|2 qbar - 1| with a target).  r_members = 1.0f / M, L = logf(C) or logf(2).  A NaN in a or b (a NaN logit) makes
// all three NaN.
__host__ __device__ inline void scores(float a, float b, float gap, int members, float r_members, float L, float* entropy,
                                       float* margin, float* bald) {
    if (a != a || b != b) {
        *entropy = *margin = *bald = a != a ? a : b;
        return;
    }
    const float h_bar = -a;
    const float h_members = -(b * r_members);
    *entropy = unit(h_bar / L);
    *margin = unit(1.0f - gap);
    *bald = members == 1 ? 0.0f : unit(fmaxf(h_bar - h_members, 0.0f) / L);
}

// a candidate's gain discounted by its distance to everything picked or labelled so far: ONE rounded product
__host__ __device__ inline float discounted(float gain, float d) { return gain * d; }

// a candidate's distance after `sim`, its similarity to the candidate just picked, is known
__host__ __device__ inline float closer(float d, float sim) { return fminf(d, fmaxf(1.0f - sim, 0.0f)); }

}  // namespace suggest
}  // namespace bd

#endif  // BD_SUGGEST_DEVICE_H
