/*
 * buzzdetect_mix.h — C ABI of the SNR mixer in libbuzzdetect_hip.so (gfx950): annotated events overlaid on background
 * stretches at chosen signal-to-noise ratios, on the device, for buzzdetect_amd/dataset.py's augment().
 *
 *   bd_mix_workspace_bytes   host only: the workspace a call with these descriptors needs
 *   bd_mix                   mix every clip of the call with one pair of launches
 *   bd_mix_host              the same arithmetic restated on the host, in the same order (bit for bit)
 *
 * Definition.  Both sources are float32 16 kHz mono.  For clip j with descriptor (ev_off, nz_off, out_off, n, ev_gain, ratio):
 *
 *   Pe = mean square of ev[ev_off .. ev_off + n)        Pn = mean square of nz[nz_off .. nz_off + n)
 *   b  = ratio * sqrt(Pe / Pn) * ev_gain
 *   out[out_off + i] = ev_gain * ev[ev_off + i] + b * nz[nz_off + i],  0 <= i < n
 *
 * with ratio = 10^(-snr_db / 20) and ev_gain = 10^(gain_db / 20), both computed in double by the caller and passed as
 * float: the mixture has the requested SNR, and the gain moves event and background alike.
 *
 *   Pn < BD_MIX_POWER_FLOOR   b = 0 and BD_MIX_FLAG_SILENT_BACKGROUND is set in the clip's flag word: a silent background
 *                             cannot reach an SNR;
 *   ratio == 0                b = 0: the event alone;
 *   Pe == 0                   b = 0.
 *
 * Order of the arithmetic (a constant of the source, not of the grid; no atomics).  A clip is cut into slices of
 * BD_MIX_SLICE samples.  Within a slice 256 chains run side by side: chain t squares and adds samples t, t + 256, ... of
 * the slice in ascending order, one fused multiply-add each, from 0.  The chains of each group of 64 meet in a butterfly
 * (v += v[lane ^ m], m = 32, 16, .. 1), and the four groups add as (g0 + g1) + (g2 + g3).  A clip's slice sums are added
 * in ascending slice order from 0, the sum is divided by (float) n, and b and the output follow as written above: one
 * division, one square root, two products for b; per sample one product and one fused multiply-add.  Every step is a
 * single correctly rounded float32 operation on both sides, so bd_mix and bd_mix_host agree in every bit.
 *
 * Conventions are those of buzzdetect_hip.h: 0 on success, a negative BD_E* code on failure, bd_last_error() for the text.
 */
#ifndef BUZZDETECT_MIX_H
#define BUZZDETECT_MIX_H

#include <stdint.h>

#include "buzzdetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BD_MIX_ABI_VERSION 1
#define BD_MIX_SLICE 4096                       /* samples per slice of the power sums */
#define BD_MIX_POWER_FLOOR 1e-20f               /* mean square below which a background counts as silent (-200 dB) */
#define BD_MIX_FLAG_SILENT_BACKGROUND 1         /* flag word bit: Pn < BD_MIX_POWER_FLOOR, b = 0 */
#define BD_MIX_MAX_CLIPS 65536                  /* clips per call */

typedef struct { int64_t ev_off, nz_off, out_off; int32_t n; float ev_gain; float ratio; } bd_mix_clip;

BD_API int bd_mix_abi_version(void);

/* Host only.  Bytes of device workspace bd_mix needs for these descriptors (their lengths decide it; at least 256). */
BD_API int64_t bd_mix_workspace_bytes(const bd_mix_clip* clips, int32_t n_clips);

/* Mix `n_clips` clips on `stream`.  ev_dev [ev_len], nz_dev [nz_len]: the sources (they may be the same buffer);
 * out_dev [out_len]: the mixtures, written only inside [out_off, out_off + n) of each clip; power_dev [n_clips][2] float:
 * (Pe, Pn); flags_dev [n_clips] uint32.  Every descriptor is checked on the host against the three lengths first
 * (1 <= n, 0 <= offset, offset + n <= length, output ranges that do not overlap one another, finite ev_gain and ratio,
 * ratio >= 0): a failing one returns BD_EINVAL, names the clip and launches nothing.  n_clips == 0 launches nothing.
 * The output must not overlap the sources.  `clips` is read before the call returns. */
BD_API int bd_mix(const float* ev_dev, int64_t ev_len, const float* nz_dev, int64_t nz_len, const bd_mix_clip* clips,
                  int32_t n_clips, float* out_dev, int64_t out_len, float* power_dev, uint32_t* flags_dev, void* workspace,
                  int64_t workspace_bytes, void* stream);

/* The same on host arrays, in the same order of operations; the same checks and errors. */
BD_API int bd_mix_host(const float* ev, int64_t ev_len, const float* nz, int64_t nz_len, const bd_mix_clip* clips,
                       int32_t n_clips, float* out, int64_t out_len, float* power, uint32_t* flags);

#ifdef __cplusplus
}
#endif

#endif /* BUZZDETECT_MIX_H */
