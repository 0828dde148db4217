// Detection calling for gfx950 (include/buzzdetect_calls.h): events and per-bin statistics from score columns where they lie.
//
//   calls_scan_kernel     a workgroup of BD_CALLS_TILE lanes per column walks the sequence tile by tile, a window per lane.  Three
//                         rounds per tile, each a pair of ballots, a summary per wave in LDS and one barrier:
//                           1. the state.  A window decides the state when its score is above high (on), not above low (off) or,
//                              between the two, when it follows a hole (off).  A lane's state is that of the last deciding lane
//                              at or below it - the highest set bit of the two ballots under the lane's mask - else that of
//                              the last deciding wave before its own, else the tile's carry.
//                           2. the previous ON window and the number of ON windows before the lane, the same way from the
//                              ballot of the states.  An ON window begins an event iff there is no previous ON window or it lies
//                              more than `link` ticks back.
//                           3. the event's index: the firsts before the lane.
//                         A first writes its window and its ON rank into its own row and the previous ON window and the same
//                         rank into the row before: the last window of that event and the rank it ends at.  The walk's last
//                         event is closed from the carries.  Rows: first, last, rank at first, rank at end, -.
//   calls_finish_kernel   a wave per event, grid-stride over the n_events the scan left on the device: n_on from the two ranks,
//                         kept from the two ticks, then the lanes walk the event's span, raise the marks of a kept event and
//                         keep their best (score, window); the 64 candidates meet in a butterfly whose order is total (the
//                         better score, then the earlier window), so the peak is the earliest of the greatest.  Spans are
//                         disjoint: W reads per column.
//   calls_bins_kernel     a wave per (column, bin): the lane chains and butterfly of calls_device.h for the sum, integer sums for
//                         the counts, comparisons for the maximum.
//
// No atomics.  Every output element has one writer per launch, apart from a mark, which the finishing wave of the one event that
// spans it may raise; inputs are only read.  The tile's carries live in registers, identical in every lane.
#include "bd_error.h"
#include "calls_device.h"

#include "../../include/buzzdetect_calls.h"

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#pragma clang fp contract(off)

namespace bd {
namespace {

constexpr int kTile = BD_CALLS_TILE;
constexpr int kTileWaves = kTile / 64;
constexpr int kFields = BD_CALLS_EVENT_FIELDS;
constexpr int kWaveThreads = 256;                       // the finishing and bins kernels: four waves, each on its own
static_assert(kTile % 64 == 0 && kTile <= 1024, "a tile is whole waves of one workgroup");

__device__ __forceinline__ int top_bit(unsigned long long m) { return 63 - __clzll((long long)m); }      // m != 0

__global__ __launch_bounds__(kTile) void calls_scan_kernel(const float* __restrict__ x, int W, long long row_stride,
                                                           long long col_stride, const int32_t* __restrict__ t, int adjacent,
                                                           const bd_calls_rule* __restrict__ rules, uint8_t* __restrict__ marks,
                                                           int32_t* __restrict__ events, int32_t* __restrict__ n_events) {
    __shared__ int s_state[kTileWaves];                   // 0: no window of the wave decides, 1: the last one says off, 2: on
    __shared__ int s_last_on[kTileWaves];                 // the wave's last ON window, -1 if none
    __shared__ int s_on[kTileWaves];                      // its ON windows
    __shared__ int s_firsts[kTileWaves];                  // its event beginnings
    const int c = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const bd_calls_rule rule = rules[c];
    const float* __restrict__ col = x + (long long)c * col_stride;
    uint8_t* __restrict__ mark = marks + (size_t)c * W;
    int32_t* __restrict__ rows = events + (size_t)c * W * kFields;
    const unsigned long long below = (1ull << lane) - 1;  // the lanes before this one
    const unsigned long long upto = below | (1ull << lane);

    bool carry_on = false;                                // the state after the last window of the tiles so far
    int carry_last_on = -1;                               // their last ON window
    int carry_on_count = 0;                               // their ON windows
    int carry_events = 0;                                 // their events
    for (int tile = 0; tile < W; tile += kTile) {
        const int w = tile + (int)threadIdx.x;
        const bool valid = w < W;
        int32_t tw = 0;
        bool on_sets = false, off_sets = false;
        if (valid) {
            tw = t[w];
            const bool hole = w > 0 && calls::ticks_between(t[w - 1], tw) > adjacent;
            const calls::Verdict verdict = calls::classify(col[(long long)w * row_stride], rule.high, rule.low);
            on_sets = verdict == calls::kSwitchOn;
            off_sets = verdict == calls::kSwitchOff || (verdict == calls::kKeep && hole);
        }
        // round 1: the state
        const unsigned long long on_b = __ballot(on_sets), off_b = __ballot(off_sets);
        if (lane == 63) s_state[wave] = (on_b | off_b) ? 1 + (int)((on_b >> top_bit(on_b | off_b)) & 1) : 0;
        __syncthreads();
        bool before = carry_on;                           // the state this wave inherits
        for (int i = wave - 1; i >= 0; --i)
            if (s_state[i]) {
                before = s_state[i] == 2;
                break;
            }
        for (int i = kTileWaves - 1; i >= 0; --i)
            if (s_state[i]) {
                carry_on = s_state[i] == 2;
                break;
            }
        const unsigned long long decided = (on_b | off_b) & upto;
        const bool on = valid && (decided ? ((on_b >> top_bit(decided)) & 1) != 0 : before);
        // round 2: the previous ON window, the ON windows before this one
        const unsigned long long state_b = __ballot(on);
        if (lane == 63) {
            s_last_on[wave] = state_b ? tile + 64 * wave + top_bit(state_b) : -1;
            s_on[wave] = __popcll(state_b);
        }
        __syncthreads();
        int prev_on = carry_last_on, on_rank = carry_on_count;
        for (int i = 0; i < kTileWaves; ++i) {
            const int last = s_last_on[i], n = s_on[i];
            if (i < wave) {
                prev_on = last >= 0 ? last : prev_on;
                on_rank += n;
            }
            carry_last_on = last >= 0 ? last : carry_last_on;
            carry_on_count += n;
        }
        if (state_b & below) prev_on = tile + 64 * wave + top_bit(state_b & below);
        on_rank += __popcll(state_b & below);
        const bool first = on && (prev_on < 0 || calls::ticks_between(t[prev_on], tw) > rule.link);
        // round 3: the event's index
        const unsigned long long first_b = __ballot(first);
        if (lane == 63) s_firsts[wave] = __popcll(first_b);
        __syncthreads();
        int e = carry_events + __popcll(first_b & below);
        for (int i = 0; i < kTileWaves; ++i) {
            const int n = s_firsts[i];
            e += i < wave ? n : 0;
            carry_events += n;
        }
        if (valid) mark[w] = on ? 1 : 0;
        if (first) {                                      // e < W: there are no more firsts than windows
            rows[(size_t)e * kFields + 0] = w;
            rows[(size_t)e * kFields + 2] = on_rank;
            if (e > 0) {
                rows[(size_t)(e - 1) * kFields + 1] = prev_on;
                rows[(size_t)(e - 1) * kFields + 3] = on_rank;
            }
        }
        // (each round has its own LDS words: a wave rewrites a word only after a barrier every reader of it has passed)
    }
    if (threadIdx.x == 0) {
        n_events[c] = carry_events;
        if (carry_events > 0) {
            rows[(size_t)(carry_events - 1) * kFields + 1] = carry_last_on;
            rows[(size_t)(carry_events - 1) * kFields + 3] = carry_on_count;
        }
    }
}

__global__ __launch_bounds__(kWaveThreads) void calls_finish_kernel(const float* __restrict__ x, int W, long long row_stride,
                                                                    long long col_stride, const int32_t* __restrict__ t,
                                                                    const bd_calls_rule* __restrict__ rules,
                                                                    uint8_t* __restrict__ marks, int32_t* __restrict__ events,
                                                                    const int32_t* __restrict__ n_events) {
    const int c = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int n = min(n_events[c], W);
    const int min_extent = rules[c].min_extent;
    const float* __restrict__ col = x + (long long)c * col_stride;
    uint8_t* __restrict__ mark = marks + (size_t)c * W;
    const int waves = (int)gridDim.x * (kWaveThreads / 64);
    for (int e = (int)blockIdx.x * (kWaveThreads / 64) + (int)(threadIdx.x >> 6); e < n; e += waves) {      // (no barrier here)
        int32_t* __restrict__ row = events + ((size_t)c * W + e) * kFields;
        const int first = row[0], last = row[1], n_on = row[3] - row[2];
        if (first < 0 || last >= W || first > last) continue;                 // (cannot happen; nothing out of bounds if it did)
        const bool kept = calls::ticks_between(t[first], t[last]) >= min_extent;
        float best = 0.0f;
        int at = INT32_MAX;                               // no candidate yet
        for (int w = first + lane; w <= last; w += 64) {
            if (!mark[w]) continue;
            const float v = col[(long long)w * row_stride];
            if (at == INT32_MAX || calls::peak_beats(v, best)) {
                best = v;
                at = w;
            }
            if (kept) mark[w] = w == first ? 3 : 2;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float other = __shfl_xor(best, m, 64);
            const int other_at = __shfl_xor(at, m, 64);
            const bool mine = at != INT32_MAX && (other_at == INT32_MAX || calls::peak_beats(best, other)
                                                  || (!calls::peak_beats(other, best) && at < other_at));
            if (!mine) {
                best = other;
                at = other_at;
            }
        }
        if (lane == 0) {
            row[2] = n_on;
            row[3] = at;
            row[4] = kept ? 1 : 0;
        }
    }
}

__global__ __launch_bounds__(kWaveThreads) void calls_bins_kernel(const float* __restrict__ x, int W, long long row_stride,
                                                                  long long col_stride, const uint8_t* __restrict__ marks,
                                                                  const int32_t* __restrict__ seg, int B,
                                                                  int32_t* __restrict__ counts, float* __restrict__ values) {
    const int c = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int b = (int)blockIdx.x * (kWaveThreads / 64) + (int)(threadIdx.x >> 6);
    if (b >= B) return;                                   // (no barrier in this kernel)
    const int lo = min(max(seg[b], 0), W), hi = min(max(seg[b + 1], lo), W);
    const float* __restrict__ col = x + (long long)c * col_stride;
    const uint8_t* __restrict__ mark = marks + (size_t)c * W;
    const float sum = calls::butterfly_wave(calls::sum_chain(col, row_stride, lo, hi, lane));
    int detected = 0, firsts = 0;
    float top = -INFINITY;
    for (int w = lo + lane; w < hi; w += 64) {
        const int m = mark[w];
        detected += m >= 2;
        firsts += m == 3;
        top = calls::max_take(top, col[(long long)w * row_stride]);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        detected += __shfl_xor(detected, m, 64);
        firsts += __shfl_xor(firsts, m, 64);
        top = calls::max_take(top, __shfl_xor(top, m, 64));
    }
    if (lane == 0) {
        const size_t at = ((size_t)c * B + b) * 2;
        counts[at] = detected;
        counts[at + 1] = firsts;
        values[at] = calls::stored_sum(sum);
        values[at + 1] = top;
    }
}

// what the device entry points and their host restatements refuse alike
int check_matrix(const std::string& fn, const float* x, int64_t W, int32_t C, int64_t row_stride, int64_t col_stride) {
    if (W < 0 || W > BD_CALLS_MAX_WINDOWS)
        return fail(BD_EINVAL, fn + "windows = " + std::to_string(W) + ", a call takes 0.." + std::to_string(BD_CALLS_MAX_WINDOWS));
    if (C < 1 || C > BD_CALLS_MAX_COLUMNS)
        return fail(BD_EINVAL, fn + "columns = " + std::to_string(C) + ", allowed are 1.." + std::to_string(BD_CALLS_MAX_COLUMNS));
    if (row_stride == 0 || col_stride == 0) return fail(BD_EINVAL, fn + (row_stride == 0 ? "row_stride" : "col_stride") + " is 0");
    if (W > 0 && (!x || (uintptr_t)x % 4)) return fail(BD_EINVAL, fn + "x is null or misaligned");
    return BD_OK;
}

int check_rules(const std::string& fn, const bd_calls_rule* rules, int32_t C, int32_t adjacent) {
    for (int c = 0; c < C; ++c) {
        const bd_calls_rule& r = rules[c];
        const std::string at = fn + "rules[" + std::to_string(c) + "].";
        if (r.high != r.high || r.low != r.low) return fail(BD_EINVAL, at + (r.high != r.high ? "high" : "low") + " is a NaN");
        if (!(r.high >= r.low)) return fail(BD_EINVAL, at + "high is below low");
        if (r.link < adjacent)
            return fail(BD_EINVAL, at + "link = " + std::to_string(r.link) + " is below adjacent = " + std::to_string(adjacent));
        if (r.min_extent < 0) return fail(BD_EINVAL, at + "min_extent = " + std::to_string(r.min_extent) + " is negative");
    }
    return BD_OK;
}

int check_events(const std::string& fn, const float* x, int64_t W, int32_t C, int64_t row_stride, int64_t col_stride,
                 const int32_t* t, int32_t adjacent, const bd_calls_rule* rules, const uint8_t* marks, const int32_t* events,
                 const int32_t* n_events) {
    const int rc = check_matrix(fn, x, W, C, row_stride, col_stride);
    if (rc != BD_OK) return rc;
    if (adjacent < 1) return fail(BD_EINVAL, fn + "adjacent = " + std::to_string(adjacent) + ", at least 1 tick");
    if (!rules || (uintptr_t)rules % 4) return fail(BD_EINVAL, fn + "rules is null or misaligned");
    if (!n_events || (uintptr_t)n_events % 4) return fail(BD_EINVAL, fn + "n_events is null or misaligned");
    if (W > 0 && (!t || (uintptr_t)t % 4)) return fail(BD_EINVAL, fn + "t is null or misaligned");
    if (W > 0 && !marks) return fail(BD_EINVAL, fn + "marks is null");
    if (W > 0 && (!events || (uintptr_t)events % 4)) return fail(BD_EINVAL, fn + "events is null or misaligned");
    return BD_OK;
}

int check_bins(const std::string& fn, const float* x, int64_t W, int32_t C, int64_t row_stride, int64_t col_stride,
               const uint8_t* marks, const int32_t* seg, int32_t B, const int32_t* counts, const float* values) {
    const int rc = check_matrix(fn, x, W, C, row_stride, col_stride);
    if (rc != BD_OK) return rc;
    if (B < 0 || B > BD_CALLS_MAX_BINS)
        return fail(BD_EINVAL, fn + "bins = " + std::to_string(B) + ", allowed are 0.." + std::to_string(BD_CALLS_MAX_BINS));
    if (B == 0) return BD_OK;
    if (!seg || (uintptr_t)seg % 4) return fail(BD_EINVAL, fn + "seg is null or misaligned");
    if (!counts || (uintptr_t)counts % 4) return fail(BD_EINVAL, fn + "counts is null or misaligned");
    if (!values || (uintptr_t)values % 4) return fail(BD_EINVAL, fn + "values is null or misaligned");
    if (W > 0 && !marks) return fail(BD_EINVAL, fn + "marks is null");
    return BD_OK;
}

}  // namespace
}  // namespace bd

extern "C" {

int bd_calls_abi_version(void) { return BD_CALLS_ABI_VERSION; }

int bd_calls_events(const float* x_dev, int64_t windows, int32_t columns, int64_t row_stride, int64_t col_stride,
                    const int32_t* t_dev, int32_t adjacent, const bd_calls_rule* rules_dev, uint8_t* marks_dev,
                    int32_t* events_dev, int32_t* n_events_dev, void* stream) {
    const std::string fn = "bd_calls_events: ";
    int rc = bd::check_events(fn, x_dev, windows, columns, row_stride, col_stride, t_dev, adjacent, rules_dev, marks_dev, events_dev,
                              n_events_dev);
    if (rc != BD_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<bd_calls_rule> rules((size_t)columns);
    BD_HIP(hipMemcpyAsync(rules.data(), rules_dev, rules.size() * sizeof(bd_calls_rule), hipMemcpyDeviceToHost, s));
    BD_HIP(hipStreamSynchronize(s));
    if ((rc = bd::check_rules(fn, rules.data(), columns, adjacent)) != BD_OK) return rc;
    if (windows == 0) {
        BD_HIP(hipMemsetAsync(n_events_dev, 0, (size_t)columns * sizeof(int32_t), s));
        return BD_OK;
    }
    const int W = (int)windows;
    hipLaunchKernelGGL(bd::calls_scan_kernel, dim3((unsigned)columns), dim3(bd::kTile), 0, s, x_dev, W, (long long)row_stride,
                       (long long)col_stride, t_dev, (int)adjacent, rules_dev, marks_dev, events_dev, n_events_dev);
    // a wave per event, at most W events a column: enough workgroups for the short events of a day, a stride for the rest
    const unsigned blocks = (unsigned)std::min<int64_t>((windows + 63) / 64, 128);
    hipLaunchKernelGGL(bd::calls_finish_kernel, dim3(blocks, (unsigned)columns), dim3(bd::kWaveThreads), 0, s, x_dev, W,
                       (long long)row_stride, (long long)col_stride, t_dev, rules_dev, marks_dev, events_dev, n_events_dev);
    return bd::hip_result(fn);
}

int bd_calls_events_host(const float* x, int64_t windows, int32_t columns, int64_t row_stride, int64_t col_stride, const int32_t* t,
                         int32_t adjacent, const bd_calls_rule* rules, uint8_t* marks, int32_t* events, int32_t* n_events) {
    const std::string fn = "bd_calls_events_host: ";
    int rc = bd::check_events(fn, x, windows, columns, row_stride, col_stride, t, adjacent, rules, marks, events, n_events);
    if (rc != BD_OK) return rc;
    if ((rc = bd::check_rules(fn, rules, columns, adjacent)) != BD_OK) return rc;
    struct Event {
        int64_t first, last, n_on, peak;
    };
    for (int32_t c = 0; c < columns; ++c) {
        const bd_calls_rule& rule = rules[c];
        const float* col = x + (int64_t)c * col_stride;
        uint8_t* mark = marks + (size_t)c * windows;
        int32_t* rows = events + (size_t)c * windows * BD_CALLS_EVENT_FIELDS;
        int32_t n = 0;
        const auto close = [&](const Event& ev) {
            const bool kept = bd::calls::ticks_between(t[ev.first], t[ev.last]) >= rule.min_extent;
            int32_t* row = rows + (size_t)n++ * BD_CALLS_EVENT_FIELDS;
            row[0] = (int32_t)ev.first;
            row[1] = (int32_t)ev.last;
            row[2] = (int32_t)ev.n_on;
            row[3] = (int32_t)ev.peak;
            row[4] = kept ? 1 : 0;
            if (!kept) return;
            for (int64_t w = ev.first; w <= ev.last; ++w)
                if (mark[w]) mark[w] = 2;
            mark[ev.first] = 3;
        };
        bool on = false, open = false;
        Event cur{};
        for (int64_t w = 0; w < windows; ++w) {
            if (w > 0 && bd::calls::ticks_between(t[w - 1], t[w]) > adjacent) on = false;
            const float v = col[w * row_stride];
            const bd::calls::Verdict verdict = bd::calls::classify(v, rule.high, rule.low);
            if (verdict == bd::calls::kSwitchOn) on = true;
            else if (verdict == bd::calls::kSwitchOff) on = false;
            mark[w] = on ? 1 : 0;
            if (!on) continue;
            if (open && bd::calls::ticks_between(t[cur.last], t[w]) <= rule.link) {
                cur.last = w;
                ++cur.n_on;
                if (bd::calls::peak_beats(v, col[cur.peak * row_stride])) cur.peak = w;
            } else {
                if (open) close(cur);
                cur = Event{w, w, 1, w};
                open = true;
            }
        }
        if (open) close(cur);
        n_events[c] = n;
    }
    return BD_OK;
}

int bd_calls_bins(const float* x_dev, int64_t windows, int32_t columns, int64_t row_stride, int64_t col_stride,
                  const uint8_t* marks_dev, const int32_t* seg_dev, int32_t bins, int32_t* counts_dev, float* values_dev,
                  void* stream) {
    const std::string fn = "bd_calls_bins: ";
    const int rc = bd::check_bins(fn, x_dev, windows, columns, row_stride, col_stride, marks_dev, seg_dev, bins, counts_dev,
                                  values_dev);
    if (rc != BD_OK) return rc;
    if (bins == 0) return BD_OK;
    hipLaunchKernelGGL(bd::calls_bins_kernel, dim3((unsigned)((bins + 3) / 4), (unsigned)columns), dim3(bd::kWaveThreads), 0,
                       static_cast<hipStream_t>(stream), x_dev, (int)windows, (long long)row_stride, (long long)col_stride,
                       marks_dev, seg_dev, (int)bins, counts_dev, values_dev);
    return bd::hip_result(fn);
}

int bd_calls_bins_host(const float* x, int64_t windows, int32_t columns, int64_t row_stride, int64_t col_stride, const uint8_t* marks,
                       const int32_t* seg, int32_t bins, int32_t* counts, float* values) {
    const std::string fn = "bd_calls_bins_host: ";
    const int rc = bd::check_bins(fn, x, windows, columns, row_stride, col_stride, marks, seg, bins, counts, values);
    if (rc != BD_OK) return rc;
    for (int32_t b = 0; b < bins; ++b)
        if (seg[b] < 0 || seg[b + 1] < seg[b] || seg[b + 1] > windows)
            return bd::fail(BD_EINVAL, fn + "seg[" + std::to_string(b) + "] .. seg[" + std::to_string(b + 1) + "] = "
                                           + std::to_string(seg[b]) + " .. " + std::to_string(seg[b + 1]) + " is not a range of the "
                                           + std::to_string(windows) + " windows");
    for (int32_t c = 0; c < columns; ++c) {
        const float* col = x + (int64_t)c * col_stride;
        const uint8_t* mark = marks + (size_t)c * windows;
        for (int32_t b = 0; b < bins; ++b) {
            const int lo = seg[b], hi = seg[b + 1];
            float v[64];
            for (int lane = 0; lane < 64; ++lane) v[lane] = bd::calls::sum_chain(col, row_stride, lo, hi, lane);
            int32_t detected = 0, firsts = 0;
            float top = -INFINITY;
            for (int w = lo; w < hi; ++w) {
                detected += mark[w] >= 2;
                firsts += mark[w] == 3;
                top = bd::calls::max_take(top, col[(int64_t)w * row_stride]);
            }
            const size_t at = ((size_t)c * bins + b) * 2;
            counts[at] = detected;
            counts[at + 1] = firsts;
            values[at] = bd::calls::stored_sum(bd::calls::butterfly_host(v));
            values[at + 1] = top;
        }
    }
    return BD_OK;
}

}  // extern "C"
