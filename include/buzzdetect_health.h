/*
 * buzzdetect_health.h — C ABI of recording health in libbuzzdetect_hip.so (gfx950): what a recorder wrote (levels, clipping,
 * stuck or zero runs) and what the model hears (band powers of the 16 kHz mono chunk), taken from the samples where the engine
 * holds them, for buzzdetect_amd/health.py.
 *
 *   bd_health_levels      one bd_health_record per (segment, channel) of a chunk of native samples   (bd_health_levels_host)
 *   bd_health_spectrum    band powers and bad frames per segment of frames of a 16 kHz chunk         (bd_health_spectrum_host)
 *   bd_health_tables      the Hann window and the twiddles both sides of bd_health_spectrum read     (host only)
 *   bd_health_check_cover whether an edge table is a contiguous cover by segments of 1..max_len      (host only)
 *
 * Every *_host routine gives the same bits as its device routine: both compile from csrc/health_device.h, which spells out the
 * order of every floating-point sum.
 *
 * ---- bd_health_levels ------------------------------------------------------------------------------------------------------
 * Input.  x[n_frames][channels], interleaved, dtype BD_HEALTH_S16 (int16) or BD_HEALTH_F32 (float32), channels 1..8: the layout
 * HipEngine.read_audio(raw=True) returns.  An int16 sample enters as x * 2^-15 (exact); a non-finite float32 sample is counted
 * in `nonfinite` and enters everything else as +0.0f.  From there on there is one arithmetic path.  edges[S + 1], int64,
 * ascending: a contiguous cover of 0..n_frames (edges[0] = 0, edges[S] = n_frames) by segments of 1..BD_HEALTH_SEGMENT frames;
 * the caller cuts them so that none straddles a bin edge.  All index arithmetic is 64-bit: n_frames * channels may pass 2^31
 * (600 s at 768 kHz with 8 channels is 3.7e9 samples).
 *
 * Parameters bd_health_level_params {clip_hi, clip_lo, clip_run, flat_run}: clip_lo < clip_hi, both finite;
 * 1 <= clip_run <= BD_HEALTH_MAX_RUN; 2 <= flat_run <= BD_HEALTH_MAX_RUN.
 *
 * Output.  records[S][channels], one bd_health_record each, every word written:
 *     n          frames of the segment
 *     nonfinite  non-finite samples
 *     peak       the maximum of |x|
 *     sum, sumsq float32 sums of x and x * x: frame i of the segment belongs to chain i / 16 (256 chains of 16 consecutive
 *                frames, added in ascending order from +0.0f, x * x rounded before it is added), the chains of 64 consecutive
 *                chain numbers meet in a butterfly (v += v[lane ^ m], m = 32 .. 1) and the four results as (w0 + w1) + (w2 + w3).
 *                The order is a function of the segment's own samples alone; the longest addition chain is
 *                BD_HEALTH_SUM_DEPTH = 16 + 6 + 2 = 24 additions.
 *     n_full     samples with x >= clip_hi or x <= clip_lo
 *     clipped    samples that lie in a maximal run of at least clip_run consecutive samples that are all high (x >= clip_hi) or
 *                all low (x <= clip_lo); a high run and a low run that touch are two runs
 *     clip_runs  such runs, counted in the segment that holds the run's first sample
 *     flat       samples that lie in a maximal run of at least flat_run consecutive samples with identical bits (of the float32
 *                value the sample entered as: -0.0f and +0.0f differ)
 *     flat_runs  such runs, likewise
 * Runs are runs of the CHUNK, per channel: they do not end at a segment edge (a dead channel is one run through every segment),
 * each sample is counted in its own segment, and a run is cut at the chunk's two ends - nothing is carried from one call to the
 * next, so a run that crosses a chunk end counts as two, each judged by its own length.
 *
 * Device side, three launches on `stream`, none of which waits for another workgroup (no look-back, no flag, no floating-point
 * atomic): (1) per (segment, channel) the record's own fields and, per predicate (high, low, flat), a run summary - head run,
 * tail run, whether the segment is one run, first and last sample bits; (2) an exclusive scan of those summaries over the
 * segments of each channel, forwards and backwards, one workgroup per (channel, predicate, direction) that walks tiles of 256
 * segments with a carry; (3) the recount of every segment with the run lengths that come in and go out in hand.  Run lengths
 * saturate at BD_HEALTH_MAX_RUN, which no threshold exceeds, so they fit 32 bits whatever the chunk.  The workspace holds the
 * summaries and scans: bd_health_levels_workspace_bytes(S, channels) bytes, 16-byte aligned, contents unspecified before and
 * after.  Inputs are only read: a launch is idempotent.  S == 0 (then n_frames must be 0) launches nothing and writes nothing.
 *
 * edges lie in device memory, so the device routine cannot read them on the host: it refuses what it can see (counts, pointers,
 * parameters), and the kernels clamp every segment to 0..BD_HEALTH_SEGMENT frames inside 0..n_frames, so that a bad table
 * gives unspecified records but no access outside x.  bd_health_check_cover (and bd_health_levels_host, which calls it) names
 * what is wrong with a table.
 *
 * ---- bd_health_spectrum ----------------------------------------------------------------------------------------------------
 * Input.  x16k[n], float32: the 16 kHz mono chunk the embedder gets.  Frame f is the BD_HEALTH_FRAME = 1024 samples from
 * BD_HEALTH_HOP * f = 512 f, whole frames only: F = n >= 1024 ? (n - 1024) / 512 + 1 : 0.  fedges[T + 1], int64 (device memory
 * for the device routine): a contiguous cover of 0..F by segments of 1..BD_HEALTH_SEGMENT_FRAMES = 64 frames.  bedges[B + 1],
 * int32, HOST memory for both routines (they travel as kernel arguments): strictly ascending FFT-bin indices in 0..513,
 * 1 <= B <= BD_HEALTH_MAX_BANDS = 64; band b is the bins bedges[b] .. bedges[b + 1] - 1.  tables: BD_HEALTH_TABLE_FLOATS
 * float32 as bd_health_tables fills them (device memory for the device routine): the periodic Hann window
 * w[i] = 0.5 - 0.5 cos(2 pi i / 1024), then cos(2 pi k / 1024), k < 512, then -sin(2 pi k / 1024), each computed in double
 * and rounded once.  Neither side calls sin or cos.
 *
 * Per frame: y = w x; a 1024-point radix-2 decimation-in-time transform of (y, 0) (bit-reversed load, ten stages of 512
 * butterflies: t = W b as four products, one subtraction and one addition; a' = a + t, b' = a - t);
 * P[k] = (c_k (re^2 + im^2)) * (1 / (1024 * 384)), c_k = 2 for k = 1..511 and 1 for k = 0 and k = 512 (384 = sum w^2), so that the
 * one-sided sum over k is sum (w x)^2 / sum w^2; a band's power is the sum of its P[k] in ascending k from +0.0f.
 *
 * Output.  power[T][B] float32: per band the sum over the segment's good frames - the frames j, j + 4, j + 8, .. of the segment
 * (j = 0..3, counted from the segment's first frame) are added in ascending order from +0.0f, and the four sums meet as
 * (s0 + s1) + (s2 + s3).  bad_frames[T] int32: the frames that hold a non-finite sample; they are left out of power.
 *
 * Device side: one workgroup of four waves per segment, a wave per frame with the frame in LDS.  T == 0 launches nothing.
 *
 * Conventions are those of buzzdetect_hip.h: 0 on success, a negative BD_E* code on failure, bd_last_error() for the text; bad
 * arguments are refused on the host with the argument named and nothing launched; the caller owns all device memory; `stream`
 * is a hipStream_t.
 */
#ifndef BUZZDETECT_HEALTH_H
#define BUZZDETECT_HEALTH_H

#include <stdint.h>

#include "buzzdetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BD_HEALTH_ABI_VERSION 1
#define BD_HEALTH_S16 0                         /* dtype codes of bd_health_levels */
#define BD_HEALTH_F32 1
#define BD_HEALTH_MAX_CHANNELS 8
#define BD_HEALTH_SEGMENT 4096                  /* frames of a levels segment, at most */
#define BD_HEALTH_MAX_SEGMENTS (1 << 24)        /* segments per call, of either routine */
#define BD_HEALTH_MAX_RUN (1 << 24)             /* clip_run and flat_run, at most; run lengths saturate here */
#define BD_HEALTH_SUM_DEPTH 24                  /* the longest addition chain of sum and sumsq */
#define BD_HEALTH_FRAME 1024                    /* samples of a spectrum frame */
#define BD_HEALTH_HOP 512                       /* samples between frame starts */
#define BD_HEALTH_BINS 513                      /* one-sided FFT bins */
#define BD_HEALTH_SEGMENT_FRAMES 64             /* frames of a spectrum segment, at most */
#define BD_HEALTH_MAX_BANDS 64
#define BD_HEALTH_TABLE_FLOATS 2048             /* window[1024], cos[512], -sin[512] */

typedef struct bd_health_level_params {
    float clip_hi;                              /* x >= clip_hi is high */
    float clip_lo;                              /* x <= clip_lo is low */
    int32_t clip_run;                           /* samples a high or low run needs to count as clipped */
    int32_t flat_run;                           /* samples a run of identical bits needs to count as flat */
} bd_health_level_params;

typedef struct bd_health_record {               /* 40 bytes, no padding */
    int32_t n;
    int32_t nonfinite;
    float peak;
    float sum;
    float sumsq;
    int32_t n_full;
    int32_t clipped;
    int32_t clip_runs;
    int32_t flat;
    int32_t flat_runs;
} bd_health_record;

BD_API int bd_health_abi_version(void);

/* 0 if edges[count + 1] is a contiguous cover of 0..total by segments of 1..max_len, else BD_EINVAL with `what` and the place named */
BD_API int bd_health_check_cover(const int64_t* edges, int64_t count, int64_t total, int64_t max_len, const char* what);

BD_API int64_t bd_health_levels_workspace_bytes(int64_t n_segments, int32_t channels);
BD_API int bd_health_levels(const void* x_dev, int32_t dtype, int64_t n_frames, int32_t channels, const int64_t* edges_dev,
                            int64_t n_segments, const bd_health_level_params* params, bd_health_record* records_dev,
                            void* workspace_dev, int64_t workspace_bytes, void* stream);
BD_API int bd_health_levels_host(const void* x, int32_t dtype, int64_t n_frames, int32_t channels, const int64_t* edges,
                                 int64_t n_segments, const bd_health_level_params* params, bd_health_record* records);

BD_API int bd_health_tables(float* tables);
BD_API int bd_health_spectrum(const float* x16k_dev, int64_t n, const int64_t* fedges_dev, int64_t n_segments, const int32_t* bedges,
                              int32_t n_bands, const float* tables_dev, float* power_dev, int32_t* bad_frames_dev, void* stream);
BD_API int bd_health_spectrum_host(const float* x16k, int64_t n, const int64_t* fedges, int64_t n_segments, const int32_t* bedges,
                                   int32_t n_bands, const float* tables, float* power, int32_t* bad_frames);

#ifdef __cplusplus
}
#endif

#endif /* BUZZDETECT_HEALTH_H */
