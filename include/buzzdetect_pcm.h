/*
 * buzzdetect_pcm.h — C ABI of the table-free sample decoders in libbuzzdetect_hip.so (gfx950).
 *
 * The reference reads every format libsndfile knows (src/stream/audio.py:22-25).  Besides RIFF/WAVE PCM and FLAC
 * this library decodes the sample encodings of AIFF/AIFF-C, Sun AU, Sony Wave64 and the codec tags of WAVE that
 * are defined by a few lines of arithmetic: linear integers and floats in either byte order, G.711 mu-law and
 * A-law, IMA/DVI ADPCM and Microsoft ADPCM.  The container is parsed on the host (buzzdetect_amd/pcmio.py); a
 * chunk's bytes go to the device as they lie in the file and are decoded there into the chunk's pool slot.
 *
 *   bd_pcm_decode_host        the decoder over a byte range on the host (same routines as the device)
 *   bd_pcm_workspace_bytes    device workspace bd_pcm_decode needs
 *   bd_pcm_decode             the decoder over a byte range on the device (stream-ordered; writes a status)
 *
 * Every encoding is a sequence of blocks of `block_align` bytes holding `samples_per_block` frames (for the
 * sample layouts and G.711 a block is one frame).  A byte range starts on the block that holds frame `first`
 * (absolute frame index); frames [first, first + n) come out interleaved: int16 for 16-bit linear, G.711 and
 * ADPCM (the bytes a 16-bit WAV holds), float32 otherwise, value / 2^(bits - 1) ((x - 128) / 128 for unsigned
 * 8-bit), which is libsndfile's float read.  Frames outside [first, first + n) are not written.
 *
 * An ADPCM block whose header is invalid (IMA step index > 88, MS predictor index >= n_coefs) ends the readable
 * audio at that block; a final block cut short yields the frames whose codes are entirely present.  The status
 * says how many frames came out and why decoding stopped.
 *
 * Conventions are those of buzzdetect_hip.h: 0 or a count on success, a negative BD_E* code on failure,
 * bd_last_error() for the text.
 */
#ifndef BUZZDETECT_PCM_H
#define BUZZDETECT_PCM_H

#include <stdint.h>

#include "buzzdetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BD_PCM_ABI_VERSION 1
#define BD_PCM_MAX_CHANNELS 8
#define BD_PCM_MAX_COEFS 32

/* bd_pcm_format.codec */
#define BD_PCM_LINEAR 0              /* integers of 8, 16, 24 or 32 bits, signed or offset binary, either byte order */
#define BD_PCM_FLOAT 1               /* IEEE float of 32 or 64 bits, either byte order */
#define BD_PCM_ULAW 2                /* G.711 mu-law, one byte per sample */
#define BD_PCM_ALAW 3                /* G.711 A-law, one byte per sample */
#define BD_PCM_IMA_ADPCM 4           /* IMA/DVI ADPCM, WAVE block layout (format tag 0x11) */
#define BD_PCM_MS_ADPCM 5            /* Microsoft ADPCM (format tag 2) */

/* why a decode stopped (bd_pcm_status.reason) */
#define BD_PCM_STOP_END 0            /* the range was decoded to its end, or to frame first + n */
#define BD_PCM_STOP_BAD_HEADER 1     /* an ADPCM block header is invalid: the audio ends at block `bad_block` */
#define BD_PCM_STOP_TRUNCATED 2      /* the range ends inside a block (a file cut short) */

typedef struct bd_pcm_format {
    int32_t codec;                   /* BD_PCM_* */
    int32_t channels;                /* 1 .. BD_PCM_MAX_CHANNELS */
    int32_t bits;                    /* bits of one stored sample: 8/16/24/32 (LINEAR), 32/64 (FLOAT), 8 (G.711), 4 (ADPCM) */
    int32_t big_endian;              /* LINEAR / FLOAT: 1 when the most significant byte comes first */
    int32_t is_signed;               /* LINEAR: 0 for offset binary (unsigned) samples */
    int32_t block_align;             /* bytes of one block (one frame for LINEAR, FLOAT and G.711) */
    int32_t samples_per_block;       /* frames of one block (1 for LINEAR, FLOAT and G.711) */
    int32_t n_coefs;                 /* MS ADPCM: coefficient pairs in `coefs` (1 .. BD_PCM_MAX_COEFS) */
    int16_t coefs[2 * BD_PCM_MAX_COEFS];  /* MS ADPCM: pairs (c1, c2) as the fmt chunk lists them */
} bd_pcm_format;

typedef struct bd_pcm_status {
    int64_t samples;                 /* frames of [first, first + n) delivered (a prefix) */
    int64_t end_sample;              /* the frame after the last readable frame of the range */
    int64_t bad_block;               /* absolute index of the first invalid block, -1: none */
    int32_t reason;                  /* BD_PCM_STOP_* */
    int32_t reserved;
} bd_pcm_status;

BD_API int bd_pcm_abi_version(void);

/* Host decoder: `data` (n_bytes, starting at the block that holds frame `first`) -> frames [first, first + n)
 * into `out` (int16 or float32 interleaved, see above).  Returns 0 and fills `status`. */
BD_API int bd_pcm_decode_host(const uint8_t* data, int64_t n_bytes, const bd_pcm_format* fmt, int64_t first, int64_t n,
                              void* out, bd_pcm_status* status);

/* Device workspace bytes for a range of n_bytes decoded into n frames. */
BD_API int64_t bd_pcm_workspace_bytes(const bd_pcm_format* fmt, int64_t n_bytes, int64_t n);

/* Device decoder, enqueued on `stream`: `data` is a device buffer of n_bytes rounded up to a multiple of 4
 * (n_bytes < 2^31), `out` a device buffer of n frames, `status` a device bd_pcm_status.  No synchronisation. */
BD_API int bd_pcm_decode(const void* data, int64_t n_bytes, const bd_pcm_format* fmt, int64_t first, int64_t n, void* out,
                         void* workspace, int64_t workspace_bytes, void* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* BUZZDETECT_PCM_H */
