// The arithmetic of label propagation (include/buzzdetect_propagate.h) that the kernels of propagate.hip and their host
// restatements both compile from, as cluster_device.h is for the clustering: an edge's weight, the pieces of a step, and the
// order and the quotients of the read-out.  The division and the butterfly are cluster_device.h's and simsearch_device.h's.
#ifndef BD_PROPAGATE_DEVICE_H
#define BD_PROPAGATE_DEVICE_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/buzzdetect_propagate.h"
#include "cluster_device.h"
#include "simsearch_device.h"

#pragma clang fp contract(off)

namespace bd {
namespace propagate {

// max(sim, 0)^power by power - 1 rounded multiplications; a NaN sim weighs nothing
__host__ __device__ inline float weight(float sim, int power) {
    const float x = sim > 0.0f ? sim : 0.0f;
    float w = x;
    for (int p = 1; p < power; ++p) w = w * x;
    return w;
}

// a neighbour as the kernels index with it (the host restatement refuses what this would change)
__host__ __device__ inline int64_t clamp_index(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

__host__ __device__ inline float edge_acc(float w, float f, float acc) { return fmaf(w, f, acc); }
__host__ __device__ inline float edge_den(float w, float den) { return den + w; }
__host__ __device__ inline float mean_of(float acc, float den) { return den > 0.0f ? cluster::div_rn(acc, den) : 0.0f; }
__host__ __device__ inline float step_out(float alpha, float mean, float y) { return fmaf(alpha, mean, (1.0f - alpha) * y); }

// how far an element moved; a NaN counts as +INFINITY
__host__ __device__ inline float moved(float out, float in) {
    const float d = fabsf(out - in);
    return d != d ? INFINITY : d;
}

// a class value as the read-out orders it: a NaN counts as -INFINITY
__host__ __device__ inline float ordered(float v) { return v != v ? -INFINITY : v; }

// whether (v1, class c1) comes before (v2, class c2): the higher value, among equal values the lower class
__host__ __device__ inline bool before(float v1, int c1, float v2, int c2) { return v1 > v2 || (v1 == v2 && c1 < c2); }

__host__ __device__ inline bool reached(float reach) { return reach != 0.0f && reach - reach == 0.0f; }      // not 0, finite

__host__ __device__ inline float confidence(float top, float reach) { return cluster::div_rn(top, reach); }
__host__ __device__ inline float margin(float top, float second, float reach) { return cluster::div_rn(top - second, reach); }

}  // namespace propagate
}  // namespace bd

#endif  // BD_PROPAGATE_DEVICE_H
