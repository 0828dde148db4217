/*
 * buzzdetect_calls.h — C ABI of detection calling in libbuzzdetect_hip.so (gfx950): a model's score columns become events and
 * per-bin statistics where the logits lie, for buzzdetect_amd/calls.py.
 *
 *   bd_calls_events        marks per window and the events of every column   (bd_calls_events_host: the same bits on the host)
 *   bd_calls_bins          detected windows, events, sum and maximum per bin  (bd_calls_bins_host: the same bits on the host)
 *
 * A sequence is the windows of one recording in time order.  Call-wide: W windows; t[W], int32 ticks, strictly increasing (a
 * tick is a window's start in hundredths of a second); adjacent >= 1: two consecutive windows with t[w] - t[w-1] <= adjacent are
 * neighbours, a larger step is a hole in the recording; x, float32 scores, column c of window w at
 * x[w * row_stride + c * col_stride] (strides in elements, as bd_search_update reads its matrix: [W][C] logits and column-major
 * matrices both serve).  Differences of ticks are taken in 64 bits.
 *
 * A rule per column, bd_calls_rule {high, low, link, min_extent}: high >= low, neither NaN (an infinity is allowed),
 * link >= adjacent, min_extent >= 0.
 *
 * Per column, the sequential definition:
 *
 *     on = false; cur = none
 *     for w in 0 .. W-1:
 *         if w > 0 and t[w] - t[w-1] > adjacent: on = false          # a hole switches the state off
 *         v = x[w]
 *         if v > high: on = true
 *         elif not (v > low): on = false                              # a NaN fails both comparisons: off
 *         mark[w] = on ? 1 : 0
 *         if on:
 *             if cur and t[w] - t[cur.last] <= link:                  # the previous ON window is near enough: the same event
 *                 cur.last = w; cur.n_on += 1
 *                 if v > x[cur.peak]: cur.peak = w                    # a float comparison: the earliest window wins a tie
 *             else:
 *                 close cur (append it); cur = {first = w, last = w, n_on = 1, peak = w}
 *     close cur
 *     an event is kept iff t[last] - t[first] >= min_extent
 *     for every kept event: its ON windows get mark 2, its first window mark 3
 *
 * So high == low, link == adjacent, min_extent == 0 is the plain threshold (mark >= 2 iff x > high), events are listed in time
 * order, the dropped ones among them with kept = 0, and a column has at most W events (holes can make every ON window its own).
 *
 * Layouts.  marks [C][W] uint8.  events [C][W][BD_CALLS_EVENT_FIELDS] int32: first, last, n_on, peak, kept (window indices);
 * only the first n_events[c] rows of column c are written, not one word beyond.  n_events [C] int32.
 *
 * Bins.  seg[B+1] holds non-decreasing int32 window offsets, 0 <= seg[0], seg[B] <= W (the device clamps what it reads to that
 * range); bin b is windows seg[b] .. seg[b+1]-1.  Per (column, bin): counts [C][B][2] int32 = windows with mark >= 2 (detected),
 * windows with mark == 3 (events); values [C][B][2] float32 = sum, max.  max is the greatest score, NaN ignored, -0.0 counted as
 * +0.0; -INFINITY for an empty or all-NaN bin.  sum is a float32 sum in a fixed order: lane l of one wave adds windows
 * seg[b] + l + 64 j, j ascending, from 0.0f, each add one correctly rounded addition; the 64 partial sums meet in the butterfly
 * v += v[lane ^ m], m = 32, 16, .. 1 (the shape of bd_search_norms).  A sum that is a NaN is stored as the one quiet NaN
 * 0x7FC00000 (which NaN an addition yields is not the same on every machine).  An empty bin has sum 0.0f.
 *
 * Device side.  The scan walks a column in tiles of BD_CALLS_TILE windows, one workgroup per column, one window per lane: the
 * state of a window is that of the most recent window whose score is not between the thresholds (two 64-bit ballots and a count
 * of leading zeros, a summary per wave through LDS, a carry from tile to tile); the previous ON window, the ON rank and the event
 * rank come the same way.  A finishing pass, one wave per event, finds the peak, decides kept and raises the marks.  One wave
 * per (column, bin) fills the bins.  No atomics, no floating-point arithmetic apart from the bin sum, and no result depends on
 * the grid or on where a tile edge falls: every output is a function of the sequence and the rules alone.
 *
 * Limits (refused on the host with the argument named, nothing launched): 0 <= W <= BD_CALLS_MAX_WINDOWS,
 * 1 <= C <= BD_CALLS_MAX_COLUMNS, 0 <= B <= BD_CALLS_MAX_BINS, adjacent >= 1, non-zero strides, non-null 4-byte aligned
 * pointers, valid rules.  bd_calls_events reads rules_dev back (C * 16 bytes, waiting for the stream) to check them before it
 * launches.  W == 0: bd_calls_events launches no kernel and zeroes n_events (a memset on the stream); bd_calls_bins then finds
 * every bin empty.  B == 0 launches nothing.  t not strictly increasing is the caller's error (buzzdetect_amd/calls.py checks
 * it); the device stays in bounds all the same.
 *
 * Conventions are those of buzzdetect_hip.h: 0 on success, a negative BD_E* code on failure, bd_last_error() for the text; the
 * caller owns all device memory; `stream` is a hipStream_t.
 */
#ifndef BUZZDETECT_CALLS_H
#define BUZZDETECT_CALLS_H

#include <stdint.h>

#include "buzzdetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BD_CALLS_ABI_VERSION 1
#define BD_CALLS_TILE 1024                      /* windows a workgroup scans between two carries */
#define BD_CALLS_MAX_WINDOWS (1 << 20)          /* windows per call */
#define BD_CALLS_MAX_COLUMNS 64
#define BD_CALLS_MAX_BINS (1 << 20)
#define BD_CALLS_EVENT_FIELDS 5                 /* first, last, n_on, peak, kept */

typedef struct bd_calls_rule {
    float high;                                 /* a score above it switches the state on */
    float low;                                  /* a score not above it switches the state off */
    int32_t link;                               /* ON windows at most this many ticks apart belong to one event */
    int32_t min_extent;                         /* an event is kept iff t[last] - t[first] >= min_extent */
} bd_calls_rule;

BD_API int bd_calls_abi_version(void);

BD_API int bd_calls_events(const float* x_dev, int64_t windows, int32_t columns, int64_t row_stride, int64_t col_stride,
                           const int32_t* t_dev, int32_t adjacent, const bd_calls_rule* rules_dev, uint8_t* marks_dev,
                           int32_t* events_dev, int32_t* n_events_dev, void* stream);
BD_API int bd_calls_events_host(const float* x, int64_t windows, int32_t columns, int64_t row_stride, int64_t col_stride,
                                const int32_t* t, int32_t adjacent, const bd_calls_rule* rules, uint8_t* marks, int32_t* events,
                                int32_t* n_events);

BD_API int bd_calls_bins(const float* x_dev, int64_t windows, int32_t columns, int64_t row_stride, int64_t col_stride,
                         const uint8_t* marks_dev, const int32_t* seg_dev, int32_t bins, int32_t* counts_dev, float* values_dev,
                         void* stream);
BD_API int bd_calls_bins_host(const float* x, int64_t windows, int32_t columns, int64_t row_stride, int64_t col_stride,
                              const uint8_t* marks, const int32_t* seg, int32_t bins, int32_t* counts, float* values);

#ifdef __cplusplus
}
#endif

#endif /* BUZZDETECT_CALLS_H */
