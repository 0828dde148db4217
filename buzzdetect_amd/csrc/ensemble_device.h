// The arithmetic of the ensemble combine pass (include/buzzdetect_ensemble.h), one output column at a time: the text
// ensemble_combine_kernel and bd_ensemble_combine_host (ensemble.hip) both call, as mixaug.hip and headtrain_device.h keep theirs.
//
// z points at member 0's value of the column, the next member's lies `stride` floats on (the members of one output are
// contiguous in the wide row and share a width).  Everything is float32, walked in ascending member order by ONE thread, so a
// column has the same bits wherever it is computed - with one exception: the per-member log-sum-exp over a row that
// mean_probability_softmax takes in `lse` is reduced over the lanes of a wave on the device and serially on the host.
#ifndef BD_ENSEMBLE_DEVICE_H
#define BD_ENSEMBLE_DEVICE_H

#include "bd_internal.h"

#include <cfloat>
#include <cmath>

namespace bd {
namespace ens {

// (z[0] + z[1] + ... + z[K-1]) * r, r = 1.0f / K: a sum and a product, nothing to contract
__host__ __device__ inline float mean(const float* __restrict__ z, int stride, int k, float r) {
    float s = z[0];
    for (int m = 1; m < k; ++m) s += z[(size_t)m * stride];
    return s * r;
}

// log-sum-exp of a row from its maximum and sum_c exp(z[c] - max)
__host__ __device__ inline float lse_of(float mx, float sum) { return mx + logf(sum); }

// log softmax of member m's column, kept finite where z - lse overflows (a finite z against an lse of the other sign)
__host__ __device__ inline float log_softmax_at(float z, float lse) { return fmaxf(z - lse, -FLT_MAX); }

// log((1/K) sum_m softmax(z[m])[c]) from the members' log-sum-exps: max_m a + log(sum_m exp(a - max_m a)) - log K
__host__ __device__ inline float mean_probability_softmax(const float* __restrict__ z, int stride, const float* __restrict__ lse,
                                                          int k, float log_k) {
    float mx = log_softmax_at(z[0], lse[0]);
    for (int m = 1; m < k; ++m) mx = fmaxf(mx, log_softmax_at(z[(size_t)m * stride], lse[m]));
    float s = 0.0f;
    for (int m = 0; m < k; ++m) s += expf(log_softmax_at(z[(size_t)m * stride], lse[m]) - mx);
    return mx + logf(s) - log_k;
}

// log sigmoid(x) = min(x, 0) - log1p(exp(-|x|))
__host__ __device__ inline float log_sigmoid(float x) { return fminf(x, 0.0f) - log1pf(expf(-fabsf(x))); }

// logit((1/K) sum_m sigmoid(z[m])) = logsumexp_m logsigmoid(z[m]) - logsumexp_m logsigmoid(-z[m])
__host__ __device__ inline float mean_probability_sigmoid(const float* __restrict__ z, int stride, int k) {
    float mp = log_sigmoid(z[0]), mn = log_sigmoid(-z[0]);
    for (int m = 1; m < k; ++m) {
        const float v = z[(size_t)m * stride];
        mp = fmaxf(mp, log_sigmoid(v));
        mn = fmaxf(mn, log_sigmoid(-v));
    }
    float sp = 0.0f, sn = 0.0f;
    for (int m = 0; m < k; ++m) {
        const float v = z[(size_t)m * stride];
        sp += expf(log_sigmoid(v) - mp);
        sn += expf(log_sigmoid(-v) - mn);
    }
    return (mp + logf(sp)) - (mn + logf(sn));
}

}  // namespace ens
}  // namespace bd

#endif  // BD_ENSEMBLE_DEVICE_H
