// Wingbeat pitch tracking for gfx950 (include/buzzdetect_pitch.h): the fundamental of selected windows of a chunk, by a
// normalised autocorrelation per frame and a median over a window's frames.
//
//   pitch_windows_kernel   ONE workgroup of eight waves per selected window.  The window's 15 360 samples are staged once into
//                          LDS (60 KB: two workgroups share a CU's 160 KB), zero where the chunk has ended.  Frames are dealt to
//                          the waves (frame f to wave f mod 8), lags to the lanes: lane l holds lags l, l + 64, .. in registers,
//                          one group of 64 lags after the other.  In the inner loop (pitch_device.h: lag_sums, the text the host
//                          calls too) y[j] is one LDS address for the whole wave, a broadcast, and y[j + tau] consecutive
//                          addresses in consecutive lanes: no bank conflict.  The lobe's end, the greatest n, the run and its
//                          argmax are xor butterflies over the wave, so every lane ends with the same values, and lane 0 leaves
//                          the frame's result in LDS.  After one barrier thread f < 29 ranks frame f among the voiced ones; the
//                          thread of the lower median stores the window's values.
//
// Nothing is added atomically, nothing depends on the grid, on S or on a window's place in sel, every output element has one
// writer and inputs are only read: a launch is idempotent.  The cost is the point of selecting: at lags 16..200 a window takes
// 29 frames x 202 lags x 512 products x 2 sums, about 6 M fused multiply-adds, some hundred times what its share of reading
// the chunk costs.
#include "bd_internal.h"
#include "bd_error.h"
#include "pitch_device.h"

#include "../../include/buzzdetect_pitch.h"

#include <string>
#include <vector>

#pragma clang fp contract(off)

namespace bd {
namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kGroups = (BD_PITCH_MAX_LAG + 2 + 63) / 64;     // groups of 64 lags that hold 0 .. lag_hi + 1
static_assert(kGroups == 9, "lags 0..512");
static_assert(BD_PITCH_WINDOW == BD_PITCH_INTEGRATION * (BD_PITCH_FRAMES + 1), "29 half-overlapping frames fill a window");
static_assert(BD_PITCH_INTEGRATION + BD_PITCH_MAX_LAG + 1 <= BD_PITCH_FRAME, "every product lies inside its frame");
static_assert(BD_PITCH_WINDOW * 4 + 3 * 32 * 4 <= 65536, "the window and the frame results fit a workgroup's LDS");

__device__ __forceinline__ float wave_add(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = pitch::butterfly_add(v, __shfl_xor(v, m, 64));
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m, 64));
    return v;
}

struct FrameResult {
    float f0;                                   // 0 for an unvoiced frame
    float clarity;
    int voiced;
};

// n of lag `at` (0 .. 64 G - 1), from the lane that holds it; `at` is the same in every lane
__device__ __forceinline__ float lag_value(const float (&n)[kGroups], int at) {
    float v = 0.0f;
#pragma unroll
    for (int g = 0; g < kGroups; ++g)
        if (g == (at >> 6)) v = n[g];
    return __shfl(v, at & 63, 64);
}

// One frame by one wave.  `frame`: its 1024 samples in LDS.  Every lane returns the same result.
__device__ FrameResult track_frame(const float* frame, const bd_pitch_params& p, int lane) {
    FrameResult r = {0.0f, 0.0f, 0};
    const float mu = pitch::mean_of(wave_add(pitch::mean_chain(frame, lane)));
    if (!pitch::finite(mu)) return r;           // (the same in every lane)
    const int last = p.lag_hi + 1;              // the last lag that is computed
    const int groups = (last + 64) >> 6;
    float n[kGroups];
    float energy0 = 0.0f;
    bool bad = false;
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
        n[g] = 0.0f;
        if (g < groups) {
            // a lane beyond the last lag repeats it: in bounds, and never looked at
            const pitch::Sums s = pitch::lag_sums(frame, mu, min(64 * g + lane, last));
            if (g == 0) energy0 = __shfl(s.energy, 0, 64);
            float m;
            n[g] = pitch::normalised(s.cross, energy0, s.energy, &m);
            bad = bad || !pitch::finite(m);
        }
    }
    if (__any(bad)) return r;
    int z = pitch::kNoLag;
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
        const int tau = 64 * g + lane;
        if (g < groups && tau >= 1 && tau <= p.lag_hi && pitch::ends_lobe(n[g])) z = min(z, tau);
    }
    z = wave_min(z);
    const int s = max(p.lag_lo, z);
    if (s > p.lag_hi) return r;                 // (no end of the lobe included)
    float nmax = -INFINITY;
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
        const int tau = 64 * g + lane;
        if (g < groups && tau >= s && tau <= p.lag_hi) nmax = fmaxf(nmax, n[g]);
    }
    nmax = wave_max(nmax);
    if (!pitch::clear_enough(nmax, p.clarity_min)) {
        r.clarity = nmax;
        return r;
    }
    const float thr = pitch::run_threshold(p.pick_ratio, nmax);
    int j = pitch::kNoLag;
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
        const int tau = 64 * g + lane;
        if (g < groups && tau >= s && tau <= p.lag_hi && pitch::in_run(n[g], thr)) j = min(j, tau);
    }
    j = wave_min(j);                            // (exists: nmax itself is not below thr)
    int stop = last;                            // the first lag behind j that is not in the run
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
        const int tau = 64 * g + lane;
        if (g < groups && tau > j && tau <= p.lag_hi && !pitch::in_run(n[g], thr)) stop = min(stop, tau);
    }
    stop = wave_min(stop);
    float best = -INFINITY;
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
        const int tau = 64 * g + lane;
        if (g < groups && tau >= j && tau < stop) best = fmaxf(best, n[g]);
    }
    best = wave_max(best);
    int i = pitch::kNoLag;
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
        const int tau = 64 * g + lane;
        if (g < groups && tau >= j && tau < stop && n[g] == best) i = min(i, tau);
    }
    i = wave_min(i);
    r.f0 = pitch::refined_f0(i, lag_value(n, i - 1), best, lag_value(n, i + 1), p.rate_hz);
    r.clarity = best;
    r.voiced = 1;
    return r;
}

__global__ __launch_bounds__(kThreads) void pitch_windows_kernel(const float* __restrict__ x, long long n_samples,
                                                                 const int* __restrict__ sel, int step, bd_pitch_params p,
                                                                 float* __restrict__ values, int* __restrict__ voiced,
                                                                 float* __restrict__ frames) {
    __shared__ float s_x[BD_PITCH_WINDOW];
    __shared__ float s_f0[32];
    __shared__ float s_clarity[32];
    __shared__ int s_voiced[32];
    const int w = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int k = sel[w];
    const long long base = (long long)k * (long long)step;
    for (int i = threadIdx.x; i < BD_PITCH_WINDOW; i += kThreads) {
        const long long at = base + i;
        s_x[i] = (k >= 0 && at < n_samples) ? x[at] : 0.0f;
    }
    __syncthreads();
    for (int f = wave; f < BD_PITCH_FRAMES; f += kWaves) {
        const FrameResult r = track_frame(s_x + BD_PITCH_INTEGRATION * f, p, lane);
        if (lane == 0) {
            s_f0[f] = r.f0;
            s_clarity[f] = r.clarity;
            s_voiced[f] = r.voiced;
        }
    }
    __syncthreads();
    const int f = threadIdx.x;
    if (f >= BD_PITCH_FRAMES) return;           // (no barrier below)
    const float mine = s_f0[f];
    int count = 0, rank = 0;
    for (int u = 0; u < BD_PITCH_FRAMES; ++u) {
        if (!s_voiced[u]) continue;
        ++count;
        if (pitch::ordered_before(s_f0[u], u, mine, f)) ++rank;
    }
    if (frames) {
        frames[((long long)w * BD_PITCH_FRAMES + f) * 2] = mine;
        frames[((long long)w * BD_PITCH_FRAMES + f) * 2 + 1] = s_clarity[f];
    }
    if (f == 0) voiced[w] = count;
    if (count >= p.min_voiced) {
        if (s_voiced[f] && rank == pitch::median_rank(count)) {
            values[2 * (long long)w] = mine;
            values[2 * (long long)w + 1] = s_clarity[f];
        }
    } else if (f == 0) {
        values[2 * (long long)w] = pitch::quiet_nan();
        values[2 * (long long)w + 1] = 0.0f;
    }
}

// one frame on the host: the same rules over n[0 .. lag_hi + 1], walked in order
FrameResult track_frame_host(const float* frame, const bd_pitch_params& p) {
    FrameResult r = {0.0f, 0.0f, 0};
    float part[64];
    for (int lane = 0; lane < 64; ++lane) part[lane] = pitch::mean_chain(frame, lane);
    const float mu = pitch::mean_of(pitch::butterfly_host(part));
    if (!pitch::finite(mu)) return r;
    const int last = p.lag_hi + 1;
    float n[BD_PITCH_MAX_LAG + 2];
    float energy0 = 0.0f;
    bool bad = false;
    for (int tau = 0; tau <= last; ++tau) {
        const pitch::Sums s = pitch::lag_sums(frame, mu, tau);
        if (tau == 0) energy0 = s.energy;
        float m;
        n[tau] = pitch::normalised(s.cross, energy0, s.energy, &m);
        bad = bad || !pitch::finite(m);
    }
    if (bad) return r;
    int z = pitch::kNoLag;
    for (int tau = p.lag_hi; tau >= 1; --tau)
        if (pitch::ends_lobe(n[tau])) z = tau;
    const int s = p.lag_lo > z ? p.lag_lo : z;
    if (s > p.lag_hi) return r;
    float nmax = -INFINITY;
    for (int tau = s; tau <= p.lag_hi; ++tau) nmax = fmaxf(nmax, n[tau]);
    if (!pitch::clear_enough(nmax, p.clarity_min)) {
        r.clarity = nmax;
        return r;
    }
    const float thr = pitch::run_threshold(p.pick_ratio, nmax);
    int j = s;
    while (!pitch::in_run(n[j], thr)) ++j;      // (ends: nmax itself is not below thr)
    int stop = j + 1;
    while (stop <= p.lag_hi && pitch::in_run(n[stop], thr)) ++stop;
    int i = j;
    for (int tau = j + 1; tau < stop; ++tau)
        if (n[tau] > n[i]) i = tau;
    r.f0 = pitch::refined_f0(i, n[i - 1], n[i], n[i + 1], p.rate_hz);
    r.clarity = n[i];
    r.voiced = 1;
    return r;
}

// what bd_pitch_windows and its host restatement refuse alike
int check(const std::string& fn, const float* x, int64_t n_samples, const int32_t* sel, int32_t n_sel, int32_t step,
          const bd_pitch_params* p, const float* values, const int32_t* voiced, const float* frames) {
    if (n_sel < 0 || n_sel > BD_PITCH_MAX_SELECTED)
        return fail(BD_EINVAL, fn + "n_sel = " + std::to_string(n_sel) + ", a call takes 0.." + std::to_string(BD_PITCH_MAX_SELECTED));
    if (n_samples < 0) return fail(BD_EINVAL, fn + "n_samples = " + std::to_string(n_samples) + " is negative");
    if (step < 1 || step > BD_PITCH_MAX_STEP)
        return fail(BD_EINVAL, fn + "step_samples = " + std::to_string(step) + ", allowed are 1.." + std::to_string(BD_PITCH_MAX_STEP));
    if (!p) return fail(BD_EINVAL, fn + "params is null");
    if (p->lag_lo < 1 || p->lag_lo > p->lag_hi)
        return fail(BD_EINVAL, fn + "lag_lo = " + std::to_string(p->lag_lo) + ", allowed are 1..lag_hi = " + std::to_string(p->lag_hi));
    if (p->lag_hi > BD_PITCH_MAX_LAG)
        return fail(BD_EINVAL, fn + "lag_hi = " + std::to_string(p->lag_hi) + " is above " + std::to_string(BD_PITCH_MAX_LAG));
    if (!(p->pick_ratio > 0.0f && p->pick_ratio <= 1.0f))
        return fail(BD_EINVAL, fn + "pick_ratio = " + std::to_string(p->pick_ratio) + " is not in (0, 1]");
    if (!(p->clarity_min > 0.0f && p->clarity_min <= 1.0f))
        return fail(BD_EINVAL, fn + "clarity_min = " + std::to_string(p->clarity_min) + " is not in (0, 1]");
    if (p->min_voiced < 1 || p->min_voiced > BD_PITCH_FRAMES)
        return fail(BD_EINVAL, fn + "min_voiced = " + std::to_string(p->min_voiced) + ", allowed are 1.." + std::to_string(BD_PITCH_FRAMES));
    if (!(p->rate_hz > 0.0f) || !pitch::finite(p->rate_hz))
        return fail(BD_EINVAL, fn + "rate_hz = " + std::to_string(p->rate_hz) + " is not a positive finite rate");
    if ((n_samples > 0 && !x) || (uintptr_t)x % 4) return fail(BD_EINVAL, fn + "x is null or misaligned");
    if ((n_sel > 0 && !sel) || (uintptr_t)sel % 4) return fail(BD_EINVAL, fn + "sel is null or misaligned");
    if ((n_sel > 0 && !values) || (uintptr_t)values % 4) return fail(BD_EINVAL, fn + "values is null or misaligned");
    if ((n_sel > 0 && !voiced) || (uintptr_t)voiced % 4) return fail(BD_EINVAL, fn + "voiced is null or misaligned");
    if ((uintptr_t)frames % 4) return fail(BD_EINVAL, fn + "frames is misaligned");
    return BD_OK;
}

}  // namespace
}  // namespace bd

extern "C" {

int bd_pitch_abi_version(void) { return BD_PITCH_ABI_VERSION; }

int bd_pitch_windows(const float* x_dev, int64_t n_samples, const int32_t* sel_dev, int32_t n_sel, int32_t step_samples,
                     const bd_pitch_params* params, float* values_dev, int32_t* voiced_dev, float* frames_dev_or_null, void* stream) {
    const std::string fn = "bd_pitch_windows: ";
    const int rc = bd::check(fn, x_dev, n_samples, sel_dev, n_sel, step_samples, params, values_dev, voiced_dev, frames_dev_or_null);
    if (rc != BD_OK) return rc;
    if (n_sel == 0) return BD_OK;
    hipLaunchKernelGGL(bd::pitch_windows_kernel, dim3((unsigned)n_sel), dim3(bd::kThreads), 0, static_cast<hipStream_t>(stream), x_dev,
                       (long long)n_samples, sel_dev, (int)step_samples, *params, values_dev, voiced_dev, frames_dev_or_null);
    return bd::hip_result(fn);
}

int bd_pitch_windows_host(const float* x, int64_t n_samples, const int32_t* sel, int32_t n_sel, int32_t step_samples,
                          const bd_pitch_params* params, float* values, int32_t* voiced, float* frames_or_null) {
    namespace pt = bd::pitch;
    const int rc = bd::check("bd_pitch_windows_host: ", x, n_samples, sel, n_sel, step_samples, params, values, voiced, frames_or_null);
    if (rc != BD_OK) return rc;
    std::vector<float> window((size_t)BD_PITCH_WINDOW);
    bd::FrameResult got[BD_PITCH_FRAMES];
    for (int32_t w = 0; w < n_sel; ++w) {
        const int32_t k = sel[w];
        const int64_t base = (int64_t)k * (int64_t)step_samples;
        for (int i = 0; i < BD_PITCH_WINDOW; ++i) window[(size_t)i] = (k >= 0 && base + i < n_samples) ? x[base + i] : 0.0f;
        int count = 0;
        for (int f = 0; f < BD_PITCH_FRAMES; ++f) {
            got[f] = bd::track_frame_host(window.data() + BD_PITCH_INTEGRATION * f, *params);
            count += got[f].voiced;
            if (frames_or_null) {
                frames_or_null[((int64_t)w * BD_PITCH_FRAMES + f) * 2] = got[f].f0;
                frames_or_null[((int64_t)w * BD_PITCH_FRAMES + f) * 2 + 1] = got[f].clarity;
            }
        }
        voiced[w] = count;
        values[2 * (int64_t)w] = pt::quiet_nan();
        values[2 * (int64_t)w + 1] = 0.0f;
        if (count < params->min_voiced) continue;
        for (int f = 0; f < BD_PITCH_FRAMES; ++f) {
            if (!got[f].voiced) continue;
            int rank = 0;
            for (int u = 0; u < BD_PITCH_FRAMES; ++u)
                if (got[u].voiced && pt::ordered_before(got[u].f0, u, got[f].f0, f)) ++rank;
            if (rank == pt::median_rank(count)) {
                values[2 * (int64_t)w] = got[f].f0;
                values[2 * (int64_t)w + 1] = got[f].clarity;
            }
        }
    }
    return BD_OK;
}

}  // extern "C"
