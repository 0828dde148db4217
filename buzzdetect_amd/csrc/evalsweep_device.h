// The one piece of the threshold sweep (include/buzzdetect_eval.h) that the kernel of evalsweep.hip and its host restatement
// (bd_eval_accumulate_host) must agree on bit for bit and therefore both compile from, as calls_device.h is for its kernels:
// what a float32 logit is to the table - non-finite, out of range, or the two rows kf and kr.
#ifndef BD_EVALSWEEP_DEVICE_H
#define BD_EVALSWEEP_DEVICE_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/buzzdetect_eval.h"

namespace bd {
namespace evalsweep {

enum Kind : int { kInRange = 0, kNonFinite = 1, kBelow = 2, kAbove = 3 };     // kNonFinite .. kAbove are the words of `tail`

constexpr int kMaxK = BD_EVAL_K_MIN + BD_EVAL_BINS - 1;

// The rows of logit v: kf = max{k : k / 100.0 <= z}, kr = rint(z * 100.0), z = (double)v.  Every operation is one float64
// operation whose result feeds a comparison, a conversion or a division - no product feeds a sum, so a compiler that contracts
// has nothing to contract and device and host give the same bits.  kf <= kr <= kf + 1.
__host__ __device__ inline Kind rows_of(float v, int* kf, int* kr) {
    if (!(fabsf(v) <= 3.402823466e+38f)) return kNonFinite;                  // an infinity or a NaN
    const double z = (double)v;
    const double s = z * 100.0;
    if (s < (double)(BD_EVAL_K_MIN - 8)) return kBelow;                       // (far outside: nothing below needs an int that large)
    if (s > (double)(kMaxK + 8)) return kAbove;
    int k = (int)floor(s);
    if ((double)(k + 1) / 100.0 <= z) k = k + 1;
    else if ((double)k / 100.0 > z) k = k - 1;
    const int r = (int)rint(s);
    if (k < BD_EVAL_K_MIN || r < BD_EVAL_K_MIN) return kBelow;
    if (k > kMaxK || r > kMaxK) return kAbove;
    *kf = k;
    *kr = r;
    return kInRange;
}

}  // namespace evalsweep
}  // namespace bd

#endif  // BD_EVALSWEEP_DEVICE_H
