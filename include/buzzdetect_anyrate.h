/*
 * buzzdetect_anyrate.h — C ABI of the any-ratio resampler in libbuzzdetect_hip.so (gfx950).
 *
 * The reference resamples whatever rate a recording has: np.mean(axis=1), then librosa.resample(y, orig_sr, 16000)
 * (src/stream/worker.py:116-128).  bd_resample (buzzdetect_hip.h) runs one-pass plans that exist only where the rate
 * ratio reduces to <= 4096 and, under the HQ filter, decimates by no more than about 43.  The entries below accept
 * every other pair as well:
 *
 *   bd_anyrate_supported    host only: would bd_resample_any accept this pair?
 *   bd_resample_any         float PCM; bd_resample's own code where bd_resample_supported is 1, anyrate_kernel elsewhere
 *   bd_resample_any_s16     the same from 16-bit PCM
 *   bd_resample_any_host    anyrate_kernel's arithmetic restated on the host, in the same order (bit for bit)
 *
 * Definition (oracle/resample_oracle.py, quality "hq"): mono = float32 channel mean; with up / down the reduced ratio and
 * h the Kaiser-windowed sinc of taps(up, down),  y[j] = sum_i mono[i] h[j down - i up + half],  ceil(n_in up / down)
 * outputs, zeros outside the chunk.  For an irreducible ratio h has millions of taps, so the kernel takes each
 * coefficient from the continuous prototype g(t) = h(up t), t = i - j down / up in input samples:
 *
 *   up <= 256   the `up` polyphase rows of h themselves, one row per output: no interpolation;
 *   otherwise   rows at 256 phases per input sample (and one before, two behind), 2 W + 1 taps each,
 *               W = half / up + 2; an output at phase (p + a) / 256 reads rows p - 1 .. p + 2, accumulates one dot
 *               product with each and combines the four with the cubic Lagrange weights of a.
 *
 * The rows are designed in double on the host, kept as float32 and cached per (ratio, quality) in the handle beside
 * bd_resample's filters (same upload and event discipline).  A wave owns an output, its lanes split the taps in a
 * fixed order and meet in a fixed butterfly; nothing is added atomically, so a result depends on its input alone.
 *
 * Accepted range (bd_anyrate_supported is 1 exactly for): every pair bd_resample_supported accepts, at its quality;
 * and at BD_RESAMPLE_HQ every 1 <= rate_in, rate_out < 2^27 whose table, rows x round_up(2 W + 1, 64) x 4 bytes with
 * rows = up (up <= 256) or 259, stays within BD_ANYRATE_MAX_TABLE_BYTES: decimation up to about 1370 : 1 where
 * up > 256 and about 1380 .. 355 000 : 1 for up = 256 .. 1; any interpolation.  That holds
 * every rate from 2 000 Hz to 4 096 000 Hz to or from 16 000 Hz, and 16 000 * 4099 Hz.  BD_RESAMPLE_SCIPY (the
 * resample_poly filter of rounds 1-3) has no any-ratio form: the query answers 0 where bd_resample_supported does.
 *
 * Conventions are those of buzzdetect_hip.h: 0 or a count on success, a negative BD_E* code on failure,
 * bd_last_error() for the text.
 */
#ifndef BUZZDETECT_ANYRATE_H
#define BUZZDETECT_ANYRATE_H

#include <stdint.h>

#include "buzzdetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BD_ANYRATE_ABI_VERSION 1
#define BD_ANYRATE_PHASES 256                      /* interpolated table: phases per input sample */
#define BD_ANYRATE_MAX_RATE (1 << 27)              /* rates below this */
#define BD_ANYRATE_MAX_TABLE_BYTES (256ll << 20)   /* coefficient table of one ratio */

BD_API int bd_anyrate_abi_version(void);

/* Host only (src/stream/worker.py:116-128: the reference accepts every rate).  1 when bd_resample_any accepts
 * rate_in -> rate_out at `quality` (BD_RESAMPLE_*), 0 when it refuses the pair with BD_EINVAL (outside the range
 * above), negative for a bad argument. */
BD_API int bd_anyrate_supported(int32_t rate_in, int32_t rate_out, int32_t quality);

/* Downmix + resample (src/stream/worker.py:116-128), arguments as bd_resample / bd_resample_s16, at the quality
 * bd_set_resample_quality chose.  Where bd_resample_supported is 1 this IS bd_resample, bit for bit; elsewhere it runs
 * anyrate_kernel.  bd_resample_length gives the output's length for every pair. */
BD_API int bd_resample_any(bd_handle h, const float* in_dev, int64_t n_in, int32_t channels, int32_t rate_in,
                           int32_t rate_out, float* out_dev, void* stream);
BD_API int bd_resample_any_s16(bd_handle h, const int16_t* in_dev, int64_t n_in, int32_t channels, int32_t rate_in,
                               int32_t rate_out, float* out_dev, void* stream);

/* Host restatement (src/stream/worker.py:116-128) of anyrate_kernel at BD_RESAMPLE_HQ: the same coefficient rows, the
 * same lane split and the same order of additions, for every pair of the any-ratio range (also one bd_resample_any
 * would hand to bd_resample).  `in`: n_in frames of `channels` interleaved int16 (is_s16 != 0) or float32; `out`:
 * bd_resample_length(n_in, rate_in, rate_out) floats. */
BD_API int bd_resample_any_host(const void* in, int32_t is_s16, int64_t n_in, int32_t channels, int32_t rate_in,
                                int32_t rate_out, float* out);

#ifdef __cplusplus
}
#endif

#endif /* BUZZDETECT_ANYRATE_H */
