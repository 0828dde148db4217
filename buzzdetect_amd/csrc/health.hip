// Recording health for gfx950 (include/buzzdetect_health.h): per segment of a chunk what the recorder wrote - levels, clipped
// and stuck runs on the native samples - and what the model hears - band powers of the 16 kHz mono chunk.
//
//   levels_summary_kernel   ONE workgroup of 256 threads per segment.  Thread t is chain t of health_device.h: it reads the 16
//                           consecutive frames 16 t .. 16 t + 15 of the segment, channel by channel, and folds them into the
//                           chain's sums and, per predicate, a Run.  Sums meet in xor butterflies and over LDS, Runs in an
//                           ordered reduction (meet is not commutative).  Thread 0 writes the record's own fields (n, nonfinite,
//                           peak, sum, sumsq, n_full) and the segment's three Runs.
//   levels_scan_kernel      ONE workgroup per (channel, predicate, direction): it walks the segments in tiles of 256 with a
//                           carry, forwards for what comes in (the summary of everything in front of a segment), backwards for
//                           what goes out.  Inside a tile: shuffles up or down the wave, four wave totals in LDS.
//   levels_recount_kernel   the summary kernel's mapping again: the same spans, an exclusive scan of the threads' Runs in both
//                           directions seeded with the segment's two scans, then health::recount on every span and an integer
//                           reduction.  Thread 0 writes clipped, clip_runs, flat, flat_runs.
//   spectrum_kernel         ONE workgroup of four waves per segment of up to 64 frames; wave w takes the segment's frames w,
//                           w + 4, ..: the windowed frame goes bit-reversed into the wave's 8 KB of LDS, ten radix-2 stages of
//                           eight butterflies per lane, bin powers in place, then lane b walks band b.
//
// No workgroup waits for another, nothing is added atomically, every output word has one writer and inputs are only read: a
// launch is idempotent.  A thread's loads are element loads of a span that lies contiguous in memory; a wave covers 64 spans
// end to end, so every cache line it touches is used whole.
#include "bd_internal.h"
#include "bd_error.h"
#include "health_device.h"

#include "../../include/buzzdetect_health.h"

#include <string>
#include <vector>

#pragma clang fp contract(off)

namespace bd {
namespace {

namespace hl = health;

constexpr int kThreads = hl::kThreads;
constexpr int kWaves = kThreads / 64;
static_assert(sizeof(hl::Run) == 20 && sizeof(bd_health_record) == 40, "no padding");
static_assert(kWaves == 4, "four wave totals meet");

__device__ __forceinline__ hl::Run shfl_run(const hl::Run& v, int from) {
    hl::Run r;
    r.head = __shfl(v.head, from, 64);
    r.tail = __shfl(v.tail, from, 64);
    r.first = (uint32_t)__shfl((int)v.first, from, 64);
    r.last = (uint32_t)__shfl((int)v.last, from, 64);
    r.flags = __shfl(v.flags, from, 64);
    return r;
}

// What lies in front of this thread (exclusive, `seed` first) and behind it (exclusive, `seed_after` last) among the block's 256
// Runs in thread order.  s_tot: 2 * kWaves Runs of LDS; two barriers.  *total: all 256 in order (without the seeds).
__device__ void block_scan(const hl::Run& mine, const hl::Run& seed, const hl::Run& seed_after, hl::Run* s_tot, hl::Run* before,
                           hl::Run* after, hl::Run* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    hl::Run up = mine, down = mine;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const hl::Run a = shfl_run(up, (lane - m) & 63);
        const hl::Run b = shfl_run(down, (lane + m) & 63);
        if (lane >= m) up = hl::meet(a, up);
        if (lane + m < 64) down = hl::meet(down, b);
    }
    hl::Run ex_up = shfl_run(up, (lane - 1) & 63), ex_down = shfl_run(down, (lane + 1) & 63);
    if (lane == 0) ex_up = hl::empty_run();
    if (lane == 63) ex_down = hl::empty_run();
    __syncthreads();                            // (s_tot may still be read from the call before)
    if (lane == 63) s_tot[wave] = up;
    if (lane == 0) s_tot[kWaves + wave] = down;
    __syncthreads();
    hl::Run b = seed, a = seed_after, t = hl::empty_run();
    for (int w = 0; w < kWaves; ++w) {
        if (w < wave) b = hl::meet(b, s_tot[w]);
        t = hl::meet(t, s_tot[w]);
    }
    for (int w = kWaves - 1; w > wave; --w) a = hl::meet(s_tot[kWaves + w], a);
    *before = hl::meet(b, ex_up);
    *after = hl::meet(ex_down, a);
    *total = t;
}

__device__ __forceinline__ int block_add(int v, int* s_int) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_int[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s_int[0] + s_int[1]) + (s_int[2] + s_int[3]);
}

__device__ __forceinline__ float block_sum(float v, float* s_f) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = hl::butterfly_add(v, __shfl_xor(v, m, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_f[threadIdx.x >> 6] = v;
    __syncthreads();
    return hl::four_add(s_f[0], s_f[1], s_f[2], s_f[3]);
}

__device__ __forceinline__ float block_max(float v, float* s_f) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_f[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(s_f[0], s_f[1]), fmaxf(s_f[2], s_f[3]));
}

// the segment's frames [*e0, *e0 + *n): whatever the table holds, 0 <= n <= 4096 and inside 0..n_frames
__device__ __forceinline__ void segment_of(const long long* edges, long long s, long long n_frames, long long* e0, int* n) {
    long long a = edges[s], b = edges[s + 1];
    a = a < 0 ? 0 : (a > n_frames ? n_frames : a);
    b = b < a ? a : (b > n_frames ? n_frames : b);
    *e0 = a;
    *n = (int)(b - a > BD_HEALTH_SEGMENT ? BD_HEALTH_SEGMENT : b - a);
}

// this thread's span of channel c: v[0 .. m), and the non-finite samples among them
__device__ __forceinline__ int load_span(const void* x, int dtype, long long e0, int n, int channels, int c, float (&v)[hl::kSpan],
                                         int* nonfinite) {
    const int at = hl::kSpan * (int)threadIdx.x;
    const int m = n - at < 0 ? 0 : (n - at > hl::kSpan ? hl::kSpan : n - at);
    const long long base = (e0 + at) * (long long)channels + c;
#pragma unroll
    for (int i = 0; i < hl::kSpan; ++i) v[i] = i < m ? hl::sample_at(x, dtype, base + (long long)i * channels, nonfinite) : 0.0f;
    return m;
}

__device__ __forceinline__ hl::Run span_run(int pred, const float (&v)[hl::kSpan], int m, const bd_health_level_params& p) {
    hl::Run r = hl::empty_run();
#pragma unroll
    for (int i = 0; i < hl::kSpan; ++i)
        if (i < m) r = hl::meet(r, hl::sample_run(pred, v[i], p));
    return r;
}

__global__ __launch_bounds__(kThreads) void levels_summary_kernel(const void* __restrict__ x, int dtype, long long n_frames, int channels,
                                                                  const long long* __restrict__ edges, bd_health_level_params p,
                                                                  bd_health_record* __restrict__ records, hl::Run* __restrict__ summary) {
    __shared__ hl::Run s_tot[2 * kWaves];
    __shared__ int s_int[kWaves];
    __shared__ float s_f[kWaves];
    const long long s = blockIdx.x;
    long long e0;
    int n;
    segment_of(edges, s, n_frames, &e0, &n);
    for (int c = 0; c < channels; ++c) {
        float v[hl::kSpan];
        int nonfinite = 0;
        const int m = load_span(x, dtype, e0, n, channels, c, v, &nonfinite);
        float sum, sumsq, peak = 0.0f;
        hl::chain_sums(v, m, &sum, &sumsq);
        int full = 0;
#pragma unroll
        for (int i = 0; i < hl::kSpan; ++i) {
            if (i < m) {
                peak = fmaxf(peak, fabsf(v[i]));
                full += (hl::is_high(v[i], p) || hl::is_low(v[i], p)) ? 1 : 0;
            }
        }
        nonfinite = block_add(nonfinite, s_int);
        full = block_add(full, s_int);
        peak = block_max(peak, s_f);
        sum = block_sum(sum, s_f);
        sumsq = block_sum(sumsq, s_f);
        const long long at = s * channels + c;
        for (int pred = 0; pred < hl::kPredicates; ++pred) {
            hl::Run before, after, total;
            block_scan(span_run(pred, v, m, p), hl::empty_run(), hl::empty_run(), s_tot, &before, &after, &total);
            if (threadIdx.x == 0) summary[at * hl::kPredicates + pred] = total;
        }
        if (threadIdx.x == 0) {
            bd_health_record& r = records[at];
            r.n = n;
            r.nonfinite = nonfinite;
            r.peak = peak;
            r.sum = sum;
            r.sumsq = sumsq;
            r.n_full = full;
        }
    }
}

// grid (channels * 3, 2): y = 0 scans forwards into `before`, y = 1 backwards into `after`
__global__ __launch_bounds__(kThreads) void levels_scan_kernel(const hl::Run* __restrict__ summary, long long n_segments, int channels,
                                                               hl::Run* __restrict__ before_out, hl::Run* __restrict__ after_out) {
    __shared__ hl::Run s_tot[2 * kWaves];
    const int c = blockIdx.x / hl::kPredicates, pred = blockIdx.x % hl::kPredicates;
    const bool backwards = blockIdx.y != 0;
    hl::Run carry = hl::empty_run();
    for (long long done = 0; done < n_segments; done += kThreads) {
        // forwards the tile is done .. done + 255, backwards the 256 segments that end at n_segments - done
        const long long s = backwards ? n_segments - done - kThreads + threadIdx.x : done + threadIdx.x;
        const bool there = s >= 0 && s < n_segments;
        const long long at = (s * channels + c) * hl::kPredicates + pred;
        const hl::Run mine = there ? summary[at] : hl::empty_run();
        hl::Run before, after, total;
        block_scan(mine, backwards ? hl::empty_run() : carry, backwards ? carry : hl::empty_run(), s_tot, &before, &after, &total);
        if (there) {
            if (backwards) after_out[at] = after;
            else before_out[at] = before;
        }
        carry = backwards ? hl::meet(total, carry) : hl::meet(carry, total);
    }
}

__global__ __launch_bounds__(kThreads) void levels_recount_kernel(const void* __restrict__ x, int dtype, long long n_frames, int channels,
                                                                  const long long* __restrict__ edges, bd_health_level_params p,
                                                                  const hl::Run* __restrict__ before_in, const hl::Run* __restrict__ after_in,
                                                                  bd_health_record* __restrict__ records) {
    __shared__ hl::Run s_tot[2 * kWaves];
    __shared__ int s_int[kWaves];
    const long long s = blockIdx.x;
    long long e0;
    int n;
    segment_of(edges, s, n_frames, &e0, &n);
    for (int c = 0; c < channels; ++c) {
        float v[hl::kSpan];
        int nonfinite = 0;
        const int m = load_span(x, dtype, e0, n, channels, c, v, &nonfinite);
        const long long at = s * channels + c;
        int counted[hl::kPredicates], runs[hl::kPredicates];
        for (int pred = 0; pred < hl::kPredicates; ++pred) {
            hl::Run before, after, total;
            block_scan(span_run(pred, v, m, p), before_in[at * hl::kPredicates + pred], after_in[at * hl::kPredicates + pred], s_tot,
                       &before, &after, &total);
            int k, r;
            hl::recount(pred, v, m, before, after, p, &k, &r);
            counted[pred] = block_add(k, s_int);
            runs[pred] = block_add(r, s_int);
        }
        if (threadIdx.x == 0) {
            bd_health_record& r = records[at];
            r.clipped = counted[hl::kHigh] + counted[hl::kLow];
            r.clip_runs = runs[hl::kHigh] + runs[hl::kLow];
            r.flat = counted[hl::kFlat];
            r.flat_runs = runs[hl::kFlat];
        }
    }
}

// ---------------------------------------------------------------------------------------------------- spectrum
struct Bands {
    int n;
    int edge[BD_HEALTH_MAX_BANDS + 1];
};

constexpr int kFrame = BD_HEALTH_FRAME;

__global__ __launch_bounds__(kThreads) void spectrum_kernel(const float* __restrict__ x, long long frames, const long long* __restrict__ fedges,
                                                            Bands bands, const float* __restrict__ tables, float* __restrict__ power,
                                                            int* __restrict__ bad_frames) {
    __shared__ float s_re[kWaves][kFrame];
    __shared__ float s_im[kWaves][kFrame];
    __shared__ float s_acc[kWaves][64];
    __shared__ int s_bad[kWaves];
    __shared__ int s_edge[BD_HEALTH_MAX_BANDS + 1];
    const long long t = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x <= bands.n) s_edge[threadIdx.x] = min(max(bands.edge[threadIdx.x], 0), BD_HEALTH_BINS);
    long long f0 = fedges[t], f1 = fedges[t + 1];
    f0 = f0 < 0 ? 0 : (f0 > frames ? frames : f0);
    f1 = f1 < f0 ? f0 : (f1 > frames ? frames : f1);
    const int nf = (int)(f1 - f0 > BD_HEALTH_SEGMENT_FRAMES ? BD_HEALTH_SEGMENT_FRAMES : f1 - f0);
    float* re = s_re[wave];
    float* im = s_im[wave];
    float acc = 0.0f;
    int bad_count = 0;
    for (int slot = 0; slot < (nf + kWaves - 1) / kWaves; ++slot) {        // (the same trips in every wave: barriers inside)
        const int local = kWaves * slot + wave;
        const bool active = local < nf;
        bool bad = false;
        if (active) {
            const float* frame = x + BD_HEALTH_HOP * (f0 + local);
#pragma unroll
            for (int i = 0; i < kFrame / 64; ++i) {
                // a lane takes 16 consecutive samples: bit-reversed they lie 64 apart with the lane in the low bits, which
                // spreads a half-wave's stores over 16 banks (two-way, free for a 4-byte store) instead of two
                const int at = (kFrame / 64) * lane + i;
                const float v = frame[at];
                bad = bad || !hl::finite(v);
                const int to = hl::bitrev10(at);
                re[to] = hl::windowed(tables[hl::kWindowAt + at], v);
                im[to] = 0.0f;
            }
        }
        bad = __any(bad);                       // (per wave: a wave holds one frame)
        const bool go = active && !bad;
        __syncthreads();
        for (int stage = 0; stage < hl::kStages; ++stage) {
            if (go) {
#pragma unroll
                for (int i = 0; i < kFrame / 2 / 64; ++i) {
                    int i0, i1, tw;
                    hl::butterfly_places(stage, lane + 64 * i, &i0, &i1, &tw);
                    hl::butterfly(re, im, i0, i1, tables[hl::kCosAt + tw], tables[hl::kSinAt + tw]);
                }
            }
            __syncthreads();
        }
        if (go) {
            for (int k = lane; k < BD_HEALTH_BINS; k += 64) re[k] = hl::bin_power(re[k], im[k], k);
        }
        __syncthreads();
        if (go && lane < bands.n) acc = hl::frame_add(acc, hl::band_walk(re, s_edge[lane], s_edge[lane + 1]));
        if (active && bad) ++bad_count;
        __syncthreads();                        // (the next frame overwrites re)
    }
    s_acc[wave][lane] = acc;
    if (lane == 0) s_bad[wave] = bad_count;
    __syncthreads();
    if (threadIdx.x < bands.n)
        power[t * bands.n + threadIdx.x] = hl::four_add(s_acc[0][threadIdx.x], s_acc[1][threadIdx.x], s_acc[2][threadIdx.x], s_acc[3][threadIdx.x]);
    if (threadIdx.x == 0) bad_frames[t] = (s_bad[0] + s_bad[1]) + (s_bad[2] + s_bad[3]);
}

// ---------------------------------------------------------------------------------------------------- host side
int check_cover(const std::string& fn, const int64_t* edges, int64_t count, int64_t total, int64_t max_len, const std::string& what) {
    if (count < 0 || count > BD_HEALTH_MAX_SEGMENTS)
        return fail(BD_EINVAL, fn + "n_segments = " + std::to_string(count) + " (" + what + "), a call takes 0.." + std::to_string(BD_HEALTH_MAX_SEGMENTS));
    if (!edges) return fail(BD_EINVAL, fn + what + " is null");
    if (edges[0] != 0) return fail(BD_EINVAL, fn + what + "[0] = " + std::to_string(edges[0]) + " is not 0");
    for (int64_t s = 0; s < count; ++s) {
        const int64_t len = edges[s + 1] - edges[s];
        if (len < 1 || len > max_len)
            return fail(BD_EINVAL, fn + what + "[" + std::to_string(s) + "] = " + std::to_string(edges[s]) + " and its successor " +
                                       std::to_string(edges[s + 1]) + " are not a segment of 1.." + std::to_string(max_len));
    }
    if (edges[count] != total)
        return fail(BD_EINVAL, fn + what + "[" + std::to_string(count) + "] = " + std::to_string(edges[count]) + " is not the total " +
                                   std::to_string(total));
    return BD_OK;
}

// what bd_health_levels and its host restatement refuse alike
int check_levels(const std::string& fn, const void* x, int32_t dtype, int64_t n_frames, int32_t channels, const int64_t* edges,
                 int64_t n_segments, const bd_health_level_params* p, const bd_health_record* records) {
    if (dtype != BD_HEALTH_S16 && dtype != BD_HEALTH_F32)
        return fail(BD_EINVAL, fn + "dtype = " + std::to_string(dtype) + " is neither BD_HEALTH_S16 nor BD_HEALTH_F32");
    if (channels < 1 || channels > BD_HEALTH_MAX_CHANNELS)
        return fail(BD_EINVAL, fn + "channels = " + std::to_string(channels) + ", allowed are 1.." + std::to_string(BD_HEALTH_MAX_CHANNELS));
    if (n_segments < 0 || n_segments > BD_HEALTH_MAX_SEGMENTS)
        return fail(BD_EINVAL, fn + "n_segments = " + std::to_string(n_segments) + ", a call takes 0.." + std::to_string(BD_HEALTH_MAX_SEGMENTS));
    if (n_frames < n_segments || n_frames > n_segments * BD_HEALTH_SEGMENT)
        return fail(BD_EINVAL, fn + "n_frames = " + std::to_string(n_frames) + " cannot be covered by " + std::to_string(n_segments) +
                                   " segments of 1.." + std::to_string(BD_HEALTH_SEGMENT) + " frames");
    if (!p) return fail(BD_EINVAL, fn + "params is null");
    if (!hl::finite(p->clip_hi) || !hl::finite(p->clip_lo) || !(p->clip_lo < p->clip_hi))
        return fail(BD_EINVAL, fn + "clip_lo = " + std::to_string(p->clip_lo) + " must be finite and below clip_hi = " + std::to_string(p->clip_hi));
    if (p->clip_run < 1 || p->clip_run > BD_HEALTH_MAX_RUN)
        return fail(BD_EINVAL, fn + "clip_run = " + std::to_string(p->clip_run) + ", allowed are 1.." + std::to_string(BD_HEALTH_MAX_RUN));
    if (p->flat_run < 2 || p->flat_run > BD_HEALTH_MAX_RUN)
        return fail(BD_EINVAL, fn + "flat_run = " + std::to_string(p->flat_run) + ", allowed are 2.." + std::to_string(BD_HEALTH_MAX_RUN));
    const uintptr_t align = dtype == BD_HEALTH_S16 ? 2 : 4;
    if ((n_frames > 0 && !x) || (uintptr_t)x % align) return fail(BD_EINVAL, fn + "x is null or misaligned");
    if ((n_segments > 0 && !edges) || (uintptr_t)edges % 8) return fail(BD_EINVAL, fn + "edges is null or misaligned");
    if ((n_segments > 0 && !records) || (uintptr_t)records % 4) return fail(BD_EINVAL, fn + "records is null or misaligned");
    return BD_OK;
}

int check_spectrum(const std::string& fn, const float* x, int64_t n, const int64_t* fedges, int64_t n_segments, const int32_t* bedges,
                   int32_t n_bands, const float* tables, const float* power, const int32_t* bad_frames, int64_t* frames) {
    if (n < 0) return fail(BD_EINVAL, fn + "n = " + std::to_string(n) + " is negative");
    *frames = n >= BD_HEALTH_FRAME ? (n - BD_HEALTH_FRAME) / BD_HEALTH_HOP + 1 : 0;
    if (n_segments < 0 || n_segments > BD_HEALTH_MAX_SEGMENTS)
        return fail(BD_EINVAL, fn + "n_segments = " + std::to_string(n_segments) + ", a call takes 0.." + std::to_string(BD_HEALTH_MAX_SEGMENTS));
    if (*frames < n_segments || *frames > n_segments * BD_HEALTH_SEGMENT_FRAMES)
        return fail(BD_EINVAL, fn + "n_segments = " + std::to_string(n_segments) + " segments of 1.." + std::to_string(BD_HEALTH_SEGMENT_FRAMES) +
                                   " frames cannot cover the " + std::to_string(*frames) + " frames of n = " + std::to_string(n));
    if (n_bands < 1 || n_bands > BD_HEALTH_MAX_BANDS)
        return fail(BD_EINVAL, fn + "n_bands = " + std::to_string(n_bands) + ", allowed are 1.." + std::to_string(BD_HEALTH_MAX_BANDS));
    if (!bedges) return fail(BD_EINVAL, fn + "bedges is null");
    for (int b = 0; b <= n_bands; ++b)
        if (bedges[b] < 0 || bedges[b] > BD_HEALTH_BINS || (b > 0 && bedges[b] <= bedges[b - 1]))
            return fail(BD_EINVAL, fn + "bedges[" + std::to_string(b) + "] = " + std::to_string(bedges[b]) +
                                       " is not strictly ascending within 0.." + std::to_string(BD_HEALTH_BINS));
    if ((n > 0 && !x) || (uintptr_t)x % 4) return fail(BD_EINVAL, fn + "x16k is null or misaligned");
    if ((n_segments > 0 && !fedges) || (uintptr_t)fedges % 8) return fail(BD_EINVAL, fn + "fedges is null or misaligned");
    if (!tables || (uintptr_t)tables % 4) return fail(BD_EINVAL, fn + "tables is null or misaligned");
    if ((n_segments > 0 && !power) || (uintptr_t)power % 4) return fail(BD_EINVAL, fn + "power is null or misaligned");
    if ((n_segments > 0 && !bad_frames) || (uintptr_t)bad_frames % 4) return fail(BD_EINVAL, fn + "bad_frames is null or misaligned");
    return BD_OK;
}

// per sample of one channel the length of the run it ends (forwards) or begins (backwards), 0 for no member: a serial walk
void run_lengths(int pred, const std::vector<float>& v, const bd_health_level_params& p, bool backwards, std::vector<int32_t>& out) {
    const int64_t n = (int64_t)v.size();
    int k = 0;
    uint32_t near = 0;
    for (int64_t step = 0; step < n; ++step) {
        const int64_t i = backwards ? n - 1 - step : step;
        if (!hl::member(pred, v[(size_t)i], p)) k = 0;
        else k = (k > 0 && near == hl::key(pred, v[(size_t)i])) ? hl::sat_add(k, 1) : 1;
        near = hl::key(pred, v[(size_t)i]);
        out[(size_t)i] = k;
    }
}

}  // namespace
}  // namespace bd

extern "C" {

int bd_health_abi_version(void) { return BD_HEALTH_ABI_VERSION; }

int bd_health_check_cover(const int64_t* edges, int64_t count, int64_t total, int64_t max_len, const char* what) {
    return bd::check_cover("bd_health_check_cover: ", edges, count, total, max_len, what ? what : "edges");
}

int64_t bd_health_levels_workspace_bytes(int64_t n_segments, int32_t channels) {
    if (n_segments < 0 || n_segments > BD_HEALTH_MAX_SEGMENTS || channels < 1 || channels > BD_HEALTH_MAX_CHANNELS)
        return bd::fail(BD_EINVAL, "bd_health_levels_workspace_bytes: n_segments = " + std::to_string(n_segments) + ", channels = " +
                                       std::to_string(channels) + " are not 0.." + std::to_string(BD_HEALTH_MAX_SEGMENTS) + " and 1.." +
                                       std::to_string(BD_HEALTH_MAX_CHANNELS));
    return 3 * n_segments * channels * bd::hl::kPredicates * (int64_t)sizeof(bd::hl::Run);
}

int bd_health_levels(const void* x_dev, int32_t dtype, int64_t n_frames, int32_t channels, const int64_t* edges_dev, int64_t n_segments,
                     const bd_health_level_params* params, bd_health_record* records_dev, void* workspace_dev, int64_t workspace_bytes,
                     void* stream) {
    namespace hl = bd::hl;
    const std::string fn = "bd_health_levels: ";
    const int rc = bd::check_levels(fn, x_dev, dtype, n_frames, channels, edges_dev, n_segments, params, records_dev);
    if (rc != BD_OK) return rc;
    if (n_segments == 0) return BD_OK;
    const int64_t need = bd_health_levels_workspace_bytes(n_segments, channels);
    if (!workspace_dev || (uintptr_t)workspace_dev % 16 || workspace_bytes < need)
        return bd::fail(BD_EINVAL, fn + "workspace is null, not 16-byte aligned or workspace_bytes = " + std::to_string(workspace_bytes) +
                                       " is below the " + std::to_string(need) + " that bd_health_levels_workspace_bytes asks for");
    const int64_t each = n_segments * channels * hl::kPredicates;
    hl::Run* summary = static_cast<hl::Run*>(workspace_dev);
    hl::Run* before = summary + each;
    hl::Run* after = before + each;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long* edges = reinterpret_cast<const long long*>(edges_dev);
    hipLaunchKernelGGL(bd::levels_summary_kernel, dim3((unsigned)n_segments), dim3(bd::kThreads), 0, st, x_dev, (int)dtype, (long long)n_frames,
                       (int)channels, edges, *params, records_dev, summary);
    hipLaunchKernelGGL(bd::levels_scan_kernel, dim3((unsigned)(channels * hl::kPredicates), 2), dim3(bd::kThreads), 0, st, summary,
                       (long long)n_segments, (int)channels, before, after);
    hipLaunchKernelGGL(bd::levels_recount_kernel, dim3((unsigned)n_segments), dim3(bd::kThreads), 0, st, x_dev, (int)dtype, (long long)n_frames,
                       (int)channels, edges, *params, before, after, records_dev);
    return bd::hip_result(fn);
}

int bd_health_levels_host(const void* x, int32_t dtype, int64_t n_frames, int32_t channels, const int64_t* edges, int64_t n_segments,
                          const bd_health_level_params* params, bd_health_record* records) {
    namespace hl = bd::hl;
    const std::string fn = "bd_health_levels_host: ";
    int rc = bd::check_levels(fn, x, dtype, n_frames, channels, edges, n_segments, params, records);
    if (rc != BD_OK) return rc;
    if (n_segments == 0) return BD_OK;
    rc = bd::check_cover(fn, edges, n_segments, n_frames, BD_HEALTH_SEGMENT, "edges");
    if (rc != BD_OK) return rc;
    const bd_health_level_params& p = *params;
    std::vector<float> v((size_t)n_frames);
    std::vector<int32_t> bad((size_t)n_frames), fwd((size_t)n_frames), bwd((size_t)n_frames);
    for (int c = 0; c < channels; ++c) {
        for (int64_t i = 0; i < n_frames; ++i) {
            int nonfinite = 0;
            v[(size_t)i] = hl::sample_at(x, dtype, i * channels + c, &nonfinite);
            bad[(size_t)i] = nonfinite;
        }
        for (int64_t s = 0; s < n_segments; ++s) {
            bd_health_record& r = records[s * channels + c];
            const int64_t e0 = edges[s];
            const int n = (int)(edges[s + 1] - e0);
            float sums[hl::kThreads], squares[hl::kThreads];
            r.n = n;
            r.nonfinite = 0;
            r.peak = 0.0f;
            r.n_full = 0;
            for (int t = 0; t < hl::kThreads; ++t) {
                const int at = hl::kSpan * t;
                const int m = n - at < 0 ? 0 : (n - at > hl::kSpan ? hl::kSpan : n - at);
                hl::chain_sums(v.data() + e0 + (m ? at : 0), m, &sums[t], &squares[t]);
                for (int i = 0; i < m; ++i) {
                    const float a = v[(size_t)(e0 + at + i)];
                    r.nonfinite += bad[(size_t)(e0 + at + i)];
                    r.peak = fmaxf(r.peak, fabsf(a));
                    r.n_full += (hl::is_high(a, p) || hl::is_low(a, p)) ? 1 : 0;
                }
            }
            r.sum = hl::four_add(hl::butterfly_host(sums), hl::butterfly_host(sums + 64), hl::butterfly_host(sums + 128), hl::butterfly_host(sums + 192));
            r.sumsq = hl::four_add(hl::butterfly_host(squares), hl::butterfly_host(squares + 64), hl::butterfly_host(squares + 128),
                                   hl::butterfly_host(squares + 192));
            r.clipped = r.clip_runs = r.flat = r.flat_runs = 0;
        }
        for (int pred = 0; pred < hl::kPredicates; ++pred) {
            bd::run_lengths(pred, v, p, false, fwd);
            bd::run_lengths(pred, v, p, true, bwd);
            const int need = hl::threshold(pred, p);
            for (int64_t s = 0; s < n_segments; ++s) {
                bd_health_record& r = records[s * channels + c];
                for (int64_t i = edges[s]; i < edges[s + 1]; ++i) {
                    if (fwd[(size_t)i] == 0 || fwd[(size_t)i] + bwd[(size_t)i] - 1 < need) continue;
                    (pred == hl::kFlat ? r.flat : r.clipped) += 1;
                    if (fwd[(size_t)i] == 1) (pred == hl::kFlat ? r.flat_runs : r.clip_runs) += 1;
                }
            }
        }
    }
    return BD_OK;
}

int bd_health_tables(float* tables) {
    namespace hl = bd::hl;
    if (!tables || (uintptr_t)tables % 4) return bd::fail(BD_EINVAL, "bd_health_tables: tables is null or misaligned");
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < BD_HEALTH_FRAME; ++i) tables[hl::kWindowAt + i] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * (double)i / BD_HEALTH_FRAME));
    for (int k = 0; k < BD_HEALTH_FRAME / 2; ++k) {
        tables[hl::kCosAt + k] = (float)std::cos(2.0 * pi * (double)k / BD_HEALTH_FRAME);
        tables[hl::kSinAt + k] = (float)(-std::sin(2.0 * pi * (double)k / BD_HEALTH_FRAME));
    }
    return BD_OK;
}

int bd_health_spectrum(const float* x16k_dev, int64_t n, const int64_t* fedges_dev, int64_t n_segments, const int32_t* bedges, int32_t n_bands,
                       const float* tables_dev, float* power_dev, int32_t* bad_frames_dev, void* stream) {
    const std::string fn = "bd_health_spectrum: ";
    int64_t frames = 0;
    const int rc = bd::check_spectrum(fn, x16k_dev, n, fedges_dev, n_segments, bedges, n_bands, tables_dev, power_dev, bad_frames_dev, &frames);
    if (rc != BD_OK) return rc;
    if (n_segments == 0) return BD_OK;
    bd::Bands bands;
    bands.n = n_bands;
    for (int b = 0; b <= BD_HEALTH_MAX_BANDS; ++b) bands.edge[b] = b <= n_bands ? bedges[b] : 0;
    hipLaunchKernelGGL(bd::spectrum_kernel, dim3((unsigned)n_segments), dim3(bd::kThreads), 0, static_cast<hipStream_t>(stream), x16k_dev,
                       (long long)frames, reinterpret_cast<const long long*>(fedges_dev), bands, tables_dev, power_dev, bad_frames_dev);
    return bd::hip_result(fn);
}

int bd_health_spectrum_host(const float* x16k, int64_t n, const int64_t* fedges, int64_t n_segments, const int32_t* bedges, int32_t n_bands,
                            const float* tables, float* power, int32_t* bad_frames) {
    namespace hl = bd::hl;
    const std::string fn = "bd_health_spectrum_host: ";
    int64_t frames = 0;
    int rc = bd::check_spectrum(fn, x16k, n, fedges, n_segments, bedges, n_bands, tables, power, bad_frames, &frames);
    if (rc != BD_OK) return rc;
    if (n_segments == 0) return BD_OK;
    rc = bd::check_cover(fn, fedges, n_segments, frames, BD_HEALTH_SEGMENT_FRAMES, "fedges");
    if (rc != BD_OK) return rc;
    std::vector<float> re((size_t)BD_HEALTH_FRAME), im((size_t)BD_HEALTH_FRAME);
    for (int64_t t = 0; t < n_segments; ++t) {
        float acc[4][BD_HEALTH_MAX_BANDS] = {};
        int bad_count = 0;
        for (int64_t f = fedges[t]; f < fedges[t + 1]; ++f) {
            const float* frame = x16k + BD_HEALTH_HOP * f;
            bool bad = false;
            for (int i = 0; i < BD_HEALTH_FRAME; ++i) {
                bad = bad || !hl::finite(frame[i]);
                re[(size_t)hl::bitrev10(i)] = hl::windowed(tables[hl::kWindowAt + i], frame[i]);
                im[(size_t)hl::bitrev10(i)] = 0.0f;
            }
            if (bad) {
                ++bad_count;
                continue;
            }
            for (int stage = 0; stage < hl::kStages; ++stage) {
                for (int j = 0; j < BD_HEALTH_FRAME / 2; ++j) {
                    int i0, i1, tw;
                    hl::butterfly_places(stage, j, &i0, &i1, &tw);
                    hl::butterfly(re.data(), im.data(), i0, i1, tables[hl::kCosAt + tw], tables[hl::kSinAt + tw]);
                }
            }
            for (int k = 0; k < BD_HEALTH_BINS; ++k) re[(size_t)k] = hl::bin_power(re[(size_t)k], im[(size_t)k], k);
            float* mine = acc[(f - fedges[t]) % 4];
            for (int b = 0; b < n_bands; ++b) mine[b] = hl::frame_add(mine[b], hl::band_walk(re.data(), bedges[b], bedges[b + 1]));
        }
        for (int b = 0; b < n_bands; ++b) power[t * n_bands + b] = hl::four_add(acc[0][b], acc[1][b], acc[2][b], acc[3][b]);
        bad_frames[t] = bad_count;
    }
    return BD_OK;
}

}  // extern "C"
