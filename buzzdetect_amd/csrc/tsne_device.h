// The arithmetic of the neighbour-preserving map (include/buzzdetect_tsne.h) that the kernels of tsne.hip and their host
// restatements both compile from, as knn_device.h and propagate_device.h are for the lists and the propagation.  The summation
// orders are part of the contract:
//
//   pair          q = 1 / fmaf(dy, dy, fmaf(dx, dx, 1)): the x term first, then the y term, one correctly rounded division.
//   repulsion     per (row i, slice of BD_TSNE_SLICE candidates): ONE chain over j ascending from 0.0f for each of z, rx, ry;
//                 j == i takes part with q = 0.0f (it adds 0.0f to z and fmaf(0, 0, r) to the force: nothing).  The slices'
//                 partials are added in ascending slice order from 0.0f.  A subnormal q * q stays a subnormal (no flush) and is
//                 multiplied as one; a q * q below the subnormal range is 0.0f and adds nothing.
//   attraction    lane l of the row's wave takes edges l, l + 64, .. in stored order from 0.0f; the 64 chains meet in the
//                 butterfly m = 32 .. 1 (simsearch_device.h).
//   slice sums    (Z, the mean, the divergence) lane l adds rows first + l + 64 u of a slice, u ascending, from 0.0f, a row past
//                 the end counting as 0.0f; the butterfly; the slices' sums in ascending order from 0.0f.
//   gains         the sign convention at zero: a value counts as positive only if it is > 0, so +0, -0 and a NaN are all "not
//                 positive"; g = 0 against v = 0 therefore have the same sign and the gain shrinks.
//
// The division is cluster_device.h's.
#ifndef BD_TSNE_DEVICE_H
#define BD_TSNE_DEVICE_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/buzzdetect_tsne.h"
#include "cluster_device.h"
#include "simsearch_device.h"

#pragma clang fp contract(off)

namespace bd {
namespace tsne {

constexpr int kSliceRounds = BD_TSNE_SLICE / 64;
static_assert(BD_TSNE_SLICE % 64 == 0, "a lane takes whole rounds of a slice");
static_assert(BD_TSNE_ROWS_PER_BLOCK % 64 == 0, "a lane takes whole rounds of a block's rows");
static_assert(BD_TSNE_MAX_K == 64, "a lane per slot");

__host__ __device__ inline int64_t slices_of(int64_t rows) { return (rows + BD_TSNE_SLICE - 1) / BD_TSNE_SLICE; }

// an index as the kernels use it (the host restatements refuse what this would change)
__host__ __device__ inline int64_t clamp_index(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---------------------------------------------------------------------------------------------------- pairs
__host__ __device__ inline float q_of(float dx, float dy) { return cluster::div_rn(1.0f, fmaf(dy, dy, fmaf(dx, dx, 1.0f))); }

struct Force {
    float x, y, z;
};

// one step of a (row, slice) chain of the repulsion
__host__ __device__ inline void repel(float xi, float yi, float xj, float yj, bool self, Force& f) {
    const float dx = xi - xj, dy = yi - yj;
    const float q = self ? 0.0f : q_of(dx, dy);
    f.z = f.z + q;
    const float q2 = q * q;
    f.x = fmaf(q2, dx, f.x);
    f.y = fmaf(q2, dy, f.y);
}

// one step of a lane's chain of the attraction
__host__ __device__ inline void attract(float p, float xi, float yi, float xj, float yj, float& ax, float& ay) {
    const float dx = xi - xj, dy = yi - yj;
    const float w = p * q_of(dx, dy);
    ax = fmaf(w, dx, ax);
    ay = fmaf(w, dy, ay);
}

// one step of a chain of sums (slices' partials, a lane's rows)
__host__ __device__ inline float chain_add(float acc, float x) { return acc + x; }

// lane l's part of a slice's sum of column `col` of src [rows][ncol]
__host__ __device__ inline float slice_chain(const float* __restrict__ src, int ncol, int col, int64_t first, int64_t rows, int lane) {
    float a = 0.0f;
    for (int u = 0; u < kSliceRounds; ++u) {
        const int64_t r = first + lane + 64 * u;
        a = chain_add(a, r < rows ? src[(size_t)r * ncol + col] : 0.0f);
    }
    return a;
}

// ---------------------------------------------------------------------------------------------------- update
__host__ __device__ inline float gradient(float exaggeration, float attr, float rep, float total) {
    return 4.0f * (exaggeration * attr - cluster::div_rn(rep, total));
}

__host__ __device__ inline float gain_next(float gain, float g, float v, float min_gain) {
    const bool differ = (g > 0.0f) != (v > 0.0f);
    return fmaxf(differ ? gain + 0.2f : gain * 0.8f, min_gain);
}

__host__ __device__ inline float velocity_next(float momentum, float v, float rate, float gain, float g) {
    return fmaf(momentum, v, -((rate * gain) * g));
}

__host__ __device__ inline float mean_of(float sum, int64_t rows) { return cluster::div_rn(sum, (float)rows); }

// ---------------------------------------------------------------------------------------------------- affinities
__host__ __device__ inline bool usable(int32_t id, float sim) { return id >= 0 && sim - sim == 0.0f; }
__host__ __device__ inline float distance(float sim) { return fmaxf(0.0f, fmaf(-2.0f, sim, 2.0f)); }
__host__ __device__ inline float kernel_term(bool ok, float d, float beta) { return ok ? expf(-(d * beta)) : 0.0f; }

struct Bisect {
    float beta, lo, hi;
    bool bounded;
};

__host__ __device__ inline Bisect bisect_start() { return Bisect{1.0f, 0.0f, 0.0f, false}; }

// s = sum e, a = sum d e at b.beta; target = logf(perplexity)
__host__ __device__ inline void bisect_step(Bisect& b, float s, float a, float target) {
    const float h = logf(s) + cluster::div_rn(b.beta * a, s);
    if (h > target) {
        b.lo = b.beta;
        b.beta = b.bounded ? 0.5f * (b.lo + b.hi) : b.beta * 2.0f;
    } else {
        b.hi = b.beta;
        b.bounded = true;
        b.beta = 0.5f * (b.lo + b.hi);
    }
}

// ---------------------------------------------------------------------------------------------------- divergence
__host__ __device__ inline float kl_term(float p, float xi, float yi, float xj, float yj, float log_total) {
    if (!(p > 0.0f)) return 0.0f;
    const float q = q_of(xi - xj, yi - yj);
    return p * ((logf(p) - logf(q)) + log_total);
}

}  // namespace tsne
}  // namespace bd

#endif  // BD_TSNE_DEVICE_H
