/*
 * buzzdetect_flac.h — C ABI of the FLAC frame decoder in libbuzzdetect_hip.so (gfx950).
 *
 * The reference reads any format libsndfile knows (src/stream/audio.py:24-25); FLAC is the lossless format
 * archived field recordings are usually kept in.  Its frames are independent and integer-coded, so the
 * decoder runs on the device where the streamer already stages a chunk's bytes (bd_stager_read): the
 * compressed bytes of one chunk go up, PCM in the layout a WAV chunk has comes out.
 *
 *   bd_flac_crc8 / bd_flac_crc16      the two checksums of a frame (host)
 *   bd_flac_parse_frame_header        one frame header from a byte buffer (host; the locator of flacio.py)
 *   bd_flac_decode_host               the decoder over a byte range on the host (same parse/decode code as the device)
 *   bd_flac_workspace_bytes           device workspace bd_flac_decode needs
 *   bd_flac_decode                    the decoder over a byte range on the device (stream-ordered; writes a status)
 *
 * A byte range starts on a frame boundary.  Samples [first, first + n) (absolute sample indices of the stream)
 * come out interleaved: int16 for 16-bit streams (the bytes a 16-bit WAV holds), float32 value / 2^(bps - 1)
 * otherwise (libsndfile's float read).  Every sample is bit-exact.  A frame counts only if the previous frame's
 * decode ends exactly where it starts, its CRC-16 matches and its frame / sample number follows on; the first
 * frame that fails ends the readable audio, and the status says where and why.
 *
 * Conventions are those of buzzdetect_hip.h: 0 or a count on success, a negative BD_E* code on failure,
 * bd_last_error() for the text.  32-bit streams are refused (BD_EINVAL).
 */
#ifndef BUZZDETECT_FLAC_H
#define BUZZDETECT_FLAC_H

#include <stdint.h>

#include "buzzdetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BD_FLAC_ABI_VERSION 1
#define BD_FLAC_MAX_CHANNELS 8

/* why a decode stopped (bd_flac_status.reason) */
#define BD_FLAC_STOP_END 0           /* the range was decoded to its last byte */
#define BD_FLAC_STOP_CRC16 1         /* a frame's CRC-16 does not match its bytes */
#define BD_FLAC_STOP_BAD_SUBFRAME 2  /* a reserved subframe type, residual coding or partition layout */
#define BD_FLAC_STOP_LOST_SYNC 3     /* no valid, consecutive frame header where the previous frame ended */
#define BD_FLAC_STOP_TRUNCATED 4     /* a frame runs past the end of the range (a file cut short) */
#define BD_FLAC_STOP_OVERFLOW 5      /* more sync candidates than the workspace holds (not FLAC data) */

typedef struct bd_flac_streaminfo {
    int32_t min_blocksize;
    int32_t max_blocksize;
    int32_t sample_rate;
    int32_t channels;
    int32_t bits_per_sample;
    int32_t reserved;
    int64_t total_samples;          /* 0: unknown */
} bd_flac_streaminfo;

typedef struct bd_flac_frame_header {
    int64_t number;                 /* frame number (fixed blocking) or first sample (variable blocking) */
    int64_t first_sample;           /* the frame's first sample (fixed blocking: number * max_blocksize) */
    int32_t blocksize;
    int32_t sample_rate;            /* 0: "see STREAMINFO" */
    int32_t channel_assignment;     /* 0-7 independent (channels - 1), 8 left/side, 9 side/right, 10 mid/side */
    int32_t channels;
    int32_t bits_per_sample;        /* resolved against STREAMINFO */
    int32_t variable;               /* blocking strategy bit */
    int32_t header_bytes;           /* including the CRC-8 */
    int32_t reserved;
} bd_flac_frame_header;

typedef struct bd_flac_status {
    int64_t samples;                /* samples of [first, first + n) delivered (a prefix) */
    int64_t stop_offset;            /* byte offset in the range where decoding stopped */
    int64_t first_sample;           /* first sample of the range's first frame (-1: none) */
    int64_t end_sample;             /* the sample after the last good frame of the range */
    int32_t reason;                 /* BD_FLAC_STOP_* */
    int32_t frames;                 /* good frames in the range */
} bd_flac_status;

BD_API int bd_flac_abi_version(void);

/* CRC-8 (poly 0x07) / CRC-16 (poly 0x8005), initial value 0, of n bytes */
BD_API uint32_t bd_flac_crc8(const uint8_t* data, int64_t n);
BD_API uint32_t bd_flac_crc16(const uint8_t* data, int64_t n);

/* Frame header at data[0]: its size in bytes when it is a valid header (sync, reserved bits, CRC-8, and when
 * `si` is given the fields agree with STREAMINFO), 0 when it is not, a negative code on a bad argument. */
BD_API int bd_flac_parse_frame_header(const uint8_t* data, int64_t n, const bd_flac_streaminfo* si,
                                      bd_flac_frame_header* out);

/* Host decoder: `data` (n_bytes, starting on a frame boundary) -> samples [first, first + n) into `out`
 * (int16 or float32 interleaved, see above).  Returns 0 and fills `status`. */
BD_API int bd_flac_decode_host(const uint8_t* data, int64_t n_bytes, const bd_flac_streaminfo* si, int64_t first,
                               int64_t n, void* out, bd_flac_status* status);

/* Device workspace bytes for a range of n_bytes decoded into n samples. */
BD_API int64_t bd_flac_workspace_bytes(const bd_flac_streaminfo* si, int64_t n_bytes, int64_t n);

/* Device decoder, enqueued on `stream`: `data` is a device buffer of n_bytes rounded up to a multiple of 4
 * (n_bytes < 2^31), `out` a device buffer of n samples, `status` a device bd_flac_status.  No synchronisation. */
BD_API int bd_flac_decode(const void* data, int64_t n_bytes, const bd_flac_streaminfo* si, int64_t first, int64_t n,
                          void* out, void* workspace, int64_t workspace_bytes, void* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* BUZZDETECT_FLAC_H */
