/*
 * buzzdetect_pitch.h — C ABI of wingbeat pitch tracking in libbuzzdetect_hip.so (gfx950): the fundamental frequency of selected
 * windows of a chunk of audio, from the samples where the engine holds them, for buzzdetect_amd/pitch.py.
 *
 *   bd_pitch_windows        f0, clarity and voiced frames of S selected windows   (bd_pitch_windows_host: the same bits on the host)
 *
 * Input.  x[n_samples], float32: one chunk at rate_hz (16 000 in every caller of the package).  sel[S], int32 window indices.
 * step_samples: the distance between window starts.  Window k is the BD_PITCH_WINDOW = 15 360 samples from k * step_samples (a
 * 64-bit product); a sample at or beyond n_samples reads as 0.0f, as the front end pads.  A negative k reads as silence, as does
 * one whose window starts at or beyond n_samples.
 *
 * Parameters bd_pitch_params {lag_lo, lag_hi, pick_ratio, clarity_min, min_voiced, rate_hz}: 1 <= lag_lo <= lag_hi <=
 * BD_PITCH_MAX_LAG, 0 < pick_ratio <= 1, 0 < clarity_min <= 1, 1 <= min_voiced <= BD_PITCH_FRAMES, rate_hz finite and positive.
 * A fundamental between fmin and fmax is lag_lo = ceil(rate / fmax), lag_hi = floor(rate / fmin).
 *
 * A window has BD_PITCH_FRAMES = 29 frames of BD_PITCH_FRAME = 1024 samples at offsets 512 f.  Per frame, the sequential
 * definition (the order of every sum is spelled out in csrc/pitch_device.h, which the kernel and the host routine compile from):
 *
 *     mu   = mean of the frame's 1024 samples
 *     y[i] = x[i] - mu
 *     for tau in 0 .. lag_hi + 1:
 *         cross = sum_{j<512} y[j] * y[j+tau]
 *         m     = sum_{j<512} y[j]^2  +  sum_{j<512} y[j+tau]^2
 *         n[tau] = (m > 0) ? 2 * cross / m : 0            # normalised, in [-1, 1]; -0.0 stored as +0.0; n[0] = 1 unless silent
 *     a non-finite mu or m (any non-finite sample makes one)  -> the frame is unvoiced, clarity 0
 *     z = first tau in 1 .. lag_hi with n[tau] < 0           # the end of the lag-0 lobe; none -> unvoiced, clarity 0
 *     s = max(lag_lo, z);  s > lag_hi                        -> unvoiced, clarity 0
 *     nmax = max n[s .. lag_hi];  not (nmax >= clarity_min)  -> unvoiced, clarity nmax
 *     thr = pick_ratio * nmax
 *     j = first tau >= s with n[tau] >= thr;  e = last tau of that unbroken run of n >= thr (not beyond lag_hi)
 *     i = the tau in j .. e with the greatest n, the smallest such tau on a tie
 *     den = (n[i-1] - 2 n[i]) + n[i+1];  d = (den < 0) ? clamp((0.5 * (n[i-1] - n[i+1])) / den, -0.5, 0.5) : 0
 *     frame f0 = rate_hz / (i + d),  frame clarity = n[i]
 *
 * The pick is the greatest value of the FIRST run above pick_ratio * nmax behind the lag-0 lobe: the first local maximum above
 * the ratio reads sharp on a noisy tone (noise puts small maxima on the rising flank), and a run that may start inside the
 * lag-0 lobe picks the shortest lag for a low tone.
 *
 * Per window: voiced = the number of voiced frames.  If voiced >= min_voiced, f0 is the lower median of the voiced frames' f0
 * (ordered by value, then frame index: element (voiced - 1) / 2 of that total order) and clarity is that frame's clarity;
 * otherwise f0 is the quiet NaN 0x7FC00000 and clarity is 0.
 *
 * Layouts.  values [S][2] float32: f0, clarity.  voiced [S] int32.  frames [S][29][2] float32: (f0 or 0, clarity) of every
 * frame, written only when the pointer is non-null.
 *
 * Device side.  One workgroup per selected window: its 15 360 samples are staged once into LDS, frames are dealt to the waves
 * and lags to the lanes (y[j] is a broadcast read, y[j+tau] lies at consecutive addresses of consecutive lanes), butterflies
 * over the wave find z, nmax, the run and the argmax, and the 29 frame results meet in LDS for the median.  No atomics; no
 * result depends on the grid, on S or on a window's position in sel; inputs are only read, so a launch is idempotent.
 *
 * Limits (refused on the host with the argument named, nothing launched): 0 <= n_sel <= BD_PITCH_MAX_SELECTED,
 * 0 <= n_samples, 1 <= step_samples <= BD_PITCH_MAX_STEP, valid parameters, non-null 4-byte aligned pointers (x may be null
 * when n_samples is 0; frames may be null).  n_sel == 0 launches nothing and writes nothing.
 *
 * Conventions are those of buzzdetect_hip.h: 0 on success, a negative BD_E* code on failure, bd_last_error() for the text; the
 * caller owns all device memory; `stream` is a hipStream_t.
 */
#ifndef BUZZDETECT_PITCH_H
#define BUZZDETECT_PITCH_H

#include <stdint.h>

#include "buzzdetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BD_PITCH_ABI_VERSION 1
#define BD_PITCH_MAX_SELECTED (1 << 20)         /* windows per call */
#define BD_PITCH_MAX_STEP (1 << 24)             /* samples between window starts */
#define BD_PITCH_WINDOW 15360                   /* samples of a window */
#define BD_PITCH_FRAMES 29                      /* frames of a window, 512 samples apart */
#define BD_PITCH_FRAME 1024                     /* samples of a frame */
#define BD_PITCH_INTEGRATION 512                /* products of one lag */
#define BD_PITCH_MAX_LAG 511

typedef struct bd_pitch_params {
    int32_t lag_lo;                             /* the shortest lag picked */
    int32_t lag_hi;                             /* the longest */
    float pick_ratio;                           /* the first run of n >= pick_ratio * nmax holds the pick */
    float clarity_min;                          /* a frame whose nmax is below it is unvoiced */
    int32_t min_voiced;                         /* voiced frames a window needs for an f0 */
    float rate_hz;                              /* samples per second */
} bd_pitch_params;

BD_API int bd_pitch_abi_version(void);

BD_API int bd_pitch_windows(const float* x_dev, int64_t n_samples, const int32_t* sel_dev, int32_t n_sel, int32_t step_samples,
                            const bd_pitch_params* params, float* values_dev, int32_t* voiced_dev, float* frames_dev_or_null,
                            void* stream);
BD_API int bd_pitch_windows_host(const float* x, int64_t n_samples, const int32_t* sel, int32_t n_sel, int32_t step_samples,
                                 const bd_pitch_params* params, float* values, int32_t* voiced, float* frames_or_null);

#ifdef __cplusplus
}
#endif

#endif /* BUZZDETECT_PITCH_H */
