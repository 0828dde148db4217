// Everything of recording health (include/buzzdetect_health.h) that the kernels of health.hip and their host restatements must
// agree on bit for bit and therefore both compile from, as pitch_device.h is for pitch tracking: how a sample enters, the three
// run predicates, the summary of a stretch of samples under a predicate and how two summaries meet, the recount of a span of
// samples with the runs that come in and go out, the order of the sums, and every butterfly, the bin scaling and the band walk
// of the spectrum.  Where a fused operation is meant, fmaf would be written out; none is, and contraction is off, so that
// neither side fuses what the other does not.
//
// Levels.  A segment of n <= 4096 frames is dealt to 256 chains: chain t takes the frames 16 t .. 16 t + 15 of the segment (those
// below n).  A chain adds its samples in ascending order from +0.0f, one addition each (sumsq: x * x is rounded, then added).
// Chains 64 w .. 64 w + 63 meet in a butterfly (v += v[lane ^ m], m = 32, 16, .. 1), the four results as (w0 + w1) + (w2 + w3).
// The longest addition chain is 16 + 6 + 2 = BD_HEALTH_SUM_DEPTH.  On the device chain t is thread t: a thread reads 16
// consecutive frames, which for every channel count and sample type is a whole number of 16-byte pieces of the interleaved data.
//
// Runs.  Under a predicate a stretch of samples is summarised by a Run {head, tail, first, last, flags}: the length of the run
// its first sample begins (0 when that sample is no member), of the run its last sample ends, the keys of its first and last
// sample, and whether the whole stretch is one run.  For high and low the key is 0 (two members always continue one another),
// for flat it is the sample's bits (and every sample is a member).  `meet(a, b)` is the summary of a followed by b; it is
// associative, lengths saturate at BD_HEALTH_MAX_RUN (saturating addition is associative too), and an EMPTY summary is its
// identity.  The same routine joins samples to a thread's span, spans to a segment and segments to a chunk.
//
// Spectrum.  Frame y = w x goes bit-reversed into re (im = 0); stage s = 0..9 has 512 butterflies j: half = 1 << s,
// pos = j & (half - 1), i0 = ((j >> s) << (s + 1)) + pos, i1 = i0 + half, twiddle pos << (9 - s).  Butterflies of one stage
// touch disjoint pairs, so their order does not matter.  A wave accumulates the band powers of the frames j, j + 4, .. of its
// segment in ascending order from +0.0f; the four sums meet as (s0 + s1) + (s2 + s3).
#ifndef BD_HEALTH_DEVICE_H
#define BD_HEALTH_DEVICE_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/buzzdetect_health.h"

#pragma clang fp contract(off)

namespace bd {
namespace health {

constexpr int kThreads = 256;                   // chains of a levels segment; threads of every kernel
constexpr int kSpan = BD_HEALTH_SEGMENT / kThreads;     // frames of a chain
constexpr int kCap = BD_HEALTH_MAX_RUN;         // run lengths saturate here
constexpr int kHigh = 0, kLow = 1, kFlat = 2, kPredicates = 3;
constexpr int kWhole = 1, kEmpty = 2;           // Run::flags
static_assert(kSpan == 16, "16 frames of any channel count and sample type are whole 16-byte pieces");

__host__ __device__ inline uint32_t bits_of(float v) {
#ifdef __HIP_DEVICE_COMPILE__
    return __float_as_uint(v);
#else
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
#endif
}

// neither an infinity nor a NaN
__host__ __device__ inline bool finite(float v) { return fabsf(v) <= 3.402823466e+38f; }

// sample `index` of x as it enters: an int16 scaled by 2^-15 (exact), a float32 as it is unless it is not finite - then +0.0f,
// and *nonfinite is counted up
__host__ __device__ inline float sample_at(const void* x, int dtype, long long index, int* nonfinite) {
    if (dtype == BD_HEALTH_S16) return (float)static_cast<const int16_t*>(x)[index] * (1.0f / 32768.0f);
    const float v = static_cast<const float*>(x)[index];
    if (finite(v)) return v;
    ++*nonfinite;
    return 0.0f;
}

__host__ __device__ inline bool is_high(float v, const bd_health_level_params& p) { return v >= p.clip_hi; }
__host__ __device__ inline bool is_low(float v, const bd_health_level_params& p) { return v <= p.clip_lo; }

// whether a sample can belong to a run of the predicate, and the key two neighbours must share to continue one another
__host__ __device__ inline bool member(int pred, float v, const bd_health_level_params& p) {
    return pred == kHigh ? is_high(v, p) : (pred == kLow ? is_low(v, p) : true);
}
__host__ __device__ inline uint32_t key(int pred, float v) { return pred == kFlat ? bits_of(v) : 0u; }

// the samples a run of the predicate needs to count
__host__ __device__ inline int threshold(int pred, const bd_health_level_params& p) { return pred == kFlat ? p.flat_run : p.clip_run; }

__host__ __device__ inline int sat_add(int a, int b) { return a + b < kCap ? a + b : kCap; }

struct Run {
    int32_t head;                               // length of the run the first sample begins (0: it is no member)
    int32_t tail;                               // length of the run the last sample ends
    uint32_t first;                             // key of the first sample
    uint32_t last;                              // key of the last
    int32_t flags;                              // kWhole: the stretch is one run; kEmpty: no samples
};

__host__ __device__ inline Run empty_run() { return Run{0, 0, 0u, 0u, kWhole | kEmpty}; }

__host__ __device__ inline Run sample_run(int pred, float v, const bd_health_level_params& p) {
    const int m = member(pred, v, p) ? 1 : 0;
    return Run{m, m, key(pred, v), key(pred, v), m ? kWhole : 0};
}

// the summary of a followed by b
__host__ __device__ inline Run meet(const Run& a, const Run& b) {
    if (a.flags & kEmpty) return b;
    if (b.flags & kEmpty) return a;
    const bool join = a.last == b.first;
    Run r;
    r.first = a.first;
    r.last = b.last;
    r.head = ((a.flags & kWhole) && join) ? sat_add(a.head, b.head) : a.head;
    r.tail = ((b.flags & kWhole) && join) ? sat_add(a.tail, b.tail) : b.tail;
    r.flags = ((a.flags & kWhole) && (b.flags & kWhole) && join) ? kWhole : 0;
    return r;
}

// The samples of a span v[0 .. m) (m <= 16) that lie in a run of at least threshold(pred) samples, and the runs among them that
// begin in the span; `before` / `after` summarise everything of the chunk in front of and behind the span.
__host__ __device__ inline void recount(int pred, const float* v, int m, const Run& before, const Run& after,
                                        const bd_health_level_params& p, int* counted, int* runs) {
    int fwd[kSpan];
    int k = (before.flags & kEmpty) ? 0 : before.tail;
    uint32_t near = before.last;
#pragma unroll
    for (int i = 0; i < kSpan; ++i) {
        fwd[i] = 0;
        if (i < m) {
            if (!member(pred, v[i], p)) {
                k = 0;
            } else {
                k = (k > 0 && near == key(pred, v[i])) ? sat_add(k, 1) : 1;
            }
            near = key(pred, v[i]);
            fwd[i] = k;
        }
    }
    k = (after.flags & kEmpty) ? 0 : after.head;
    near = after.first;
    const int need = threshold(pred, p);
    int c = 0, r = 0;
#pragma unroll
    for (int i = kSpan - 1; i >= 0; --i) {
        if (i < m) {
            if (!member(pred, v[i], p)) {
                k = 0;
            } else {
                k = (k > 0 && near == key(pred, v[i])) ? sat_add(k, 1) : 1;
            }
            near = key(pred, v[i]);
            if (fwd[i] > 0 && fwd[i] + k - 1 >= need) {
                ++c;
                if (fwd[i] == 1) ++r;
            }
        }
    }
    *counted = c;
    *runs = r;
}

// a chain's sums: its samples in ascending order from +0.0f
__host__ __device__ inline void chain_sums(const float* v, int m, float* sum, float* sumsq) {
    float s = 0.0f, q = 0.0f;
#pragma unroll
    for (int i = 0; i < kSpan; ++i) {
        if (i < m) {
            const float sq = v[i] * v[i];
            s = s + v[i];
            q = q + sq;
        }
    }
    *sum = s;
    *sumsq = q;
}

// one step of the butterfly 64 chains meet in, and how the four results meet
__host__ __device__ inline float butterfly_add(float mine, float other) { return mine + other; }
__host__ __device__ inline float four_add(float w0, float w1, float w2, float w3) { return (w0 + w1) + (w2 + w3); }

// the butterfly over 64 values on the host; the sum is v[0] (and every other element)
inline float butterfly_host(float* v) {
    for (int m = 32; m >= 1; m >>= 1) {
        float t[64];
        for (int lane = 0; lane < 64; ++lane) t[lane] = butterfly_add(v[lane], v[lane ^ m]);
        for (int lane = 0; lane < 64; ++lane) v[lane] = t[lane];
    }
    return v[0];
}

// ---------------------------------------------------------------------------------------------------- spectrum
constexpr int kStages = 10;
constexpr int kWindowAt = 0, kCosAt = BD_HEALTH_FRAME, kSinAt = BD_HEALTH_FRAME + BD_HEALTH_FRAME / 2;     // places in the tables
constexpr float kPowerScale = (float)(1.0 / (1024.0 * 384.0));     // 1 / (N sum w^2)
static_assert(BD_HEALTH_FRAME == 1 << kStages && kSinAt + BD_HEALTH_FRAME / 2 == BD_HEALTH_TABLE_FLOATS, "1024-point frames");

__host__ __device__ inline int bitrev10(int i) {
    int r = 0;
#pragma unroll
    for (int b = 0; b < kStages; ++b) r |= ((i >> b) & 1) << (kStages - 1 - b);
    return r;
}

__host__ __device__ inline float windowed(float w, float x) { return w * x; }

// butterfly j of stage s: the two places it reads and writes and its twiddle
__host__ __device__ inline void butterfly_places(int s, int j, int* i0, int* i1, int* tw) {
    const int half = 1 << s, pos = j & (half - 1);
    *i0 = ((j >> s) << (s + 1)) + pos;
    *i1 = *i0 + half;
    *tw = pos << (kStages - 1 - s);
}

// t = W b (four products, one subtraction, one addition); a' = a + t, b' = a - t
__host__ __device__ inline void butterfly(float* re, float* im, int i0, int i1, float wr, float wi) {
    const float ar = re[i0], ai = im[i0], br = re[i1], bi = im[i1];
    const float p0 = wr * br, p1 = wi * bi, p2 = wr * bi, p3 = wi * br;
    const float tr = p0 - p1, ti = p2 + p3;
    re[i0] = ar + tr;
    im[i0] = ai + ti;
    re[i1] = ar - tr;
    im[i1] = ai - ti;
}

// P[k] of the one-sided spectrum
__host__ __device__ inline float bin_power(float re, float im, int k) {
    const float c = (k == 0 || k == BD_HEALTH_FRAME / 2) ? 1.0f : 2.0f;
    const float r2 = re * re, i2 = im * im;
    return (c * (r2 + i2)) * kPowerScale;
}

// a band's power: its bins in ascending order from +0.0f
__host__ __device__ inline float band_walk(const float* power, int k0, int k1) {
    float a = 0.0f;
    for (int k = k0; k < k1; ++k) a = a + power[k];
    return a;
}

// a wave's running sum over its frames takes one more frame's band power
__host__ __device__ inline float frame_add(float acc, float band) { return acc + band; }

}  // namespace health
}  // namespace bd

#endif  // BD_HEALTH_DEVICE_H
