// Table-free sample decoders (include/buzzdetect_pcm.h): sample layouts, G.711 and the two WAVE ADPCMs on gfx950, and the
// same routines on the host.
//
// A byte range starts at the block that holds frame `first` (a block is one frame for the layouts and G.711).  It becomes
// interleaved int16 or float32 frames [first, first + n) in one launch for the layouts and G.711:
//   pcm_layout<W>      one thread per group of 8 (W <= 2) or 4 stored samples of W bytes: one range-checked vector load,
//                      byte order / sign / scale, one vector store (int16 out) or one or two (float32 out); the group that
//                      holds the range's end goes sample by sample; block 0 lane 0 writes the status
// and in two for ADPCM:
//   pcm_adpcm_check    one thread per block of the range that overlaps the window: header valid?  atomicMin of the first
//                      bad block into the workspace word (which the host set to INT_MAX)
//   pcm_adpcm_decode   one lane per (block, channel) before the first bad block: the block's codes in order, frames in
//                      [first, first + n) stored straight to the slot; block 0 lane 0 writes the status
// Blocks are independent (every ADPCM block restarts from its header), so there is no chain to resolve.
//
// Bytes are read through aligned 32-bit little-endian words (on the device: raw buffer loads over the range rounded up to
// 4 bytes, so nothing past the caller's buffer is touched and reads past the range see zeros; on the host: zeros past n).
// Every read a decode makes lies inside the bytes its block holds in the range; block_frames() says how far that is.
#include <climits>
#include <cstring>
#include <string>

#include "bd_internal.h"
#include "bd_error.h"
#include "../../include/buzzdetect_pcm.h"

namespace {

#define HD __host__ __device__ inline

constexpr int kLayoutThreads = 256;
constexpr int kAdpcmThreads = 64;

// ---------------------------------------------------------------- byte sources
struct HostSrc {
    const uint8_t* p;
    int64_t n;
    HD uint32_t word(int64_t a) const {          // bytes a .. a + 3, little-endian, zero past n (a is a multiple of 4)
        uint32_t v = 0;
        for (int k = 3; k >= 0; --k) v = (v << 8) | (a + k < n ? p[a + k] : 0u);
        return v;
    }
};

struct DevSrc {
    __amdgpu_buffer_rsrc_t rs;
    int64_t n;
    __device__ uint32_t word(int64_t a) const { return __builtin_amdgcn_raw_buffer_load_b32(rs, (int)a, 0, 0); }
};

template <class S>
HD uint32_t byte_at(const S& s, int64_t a) {
    return (s.word(a & ~3LL) >> (8 * (int)(a & 3))) & 0xFFu;
}

template <class S>
HD uint32_t u32le(const S& s, int64_t a) {      // bytes a .. a + 3, little-endian, any alignment
    const int sh = (int)(a & 3);
    const uint32_t lo = s.word(a - sh);
    if (sh == 0) return lo;
    return (lo >> (8 * sh)) | (s.word(a - sh + 4) << (32 - 8 * sh));
}

template <class S>
HD int32_t s16le(const S& s, int64_t a) {
    return (int16_t)(uint16_t)(byte_at(s, a) | (byte_at(s, a + 1) << 8));
}

// ---------------------------------------------------------------- formats
HD bool out_is_s16(const bd_pcm_format& f) {
    return (f.codec == BD_PCM_LINEAR && f.bits == 16) || f.codec == BD_PCM_ULAW || f.codec == BD_PCM_ALAW ||
           f.codec == BD_PCM_IMA_ADPCM || f.codec == BD_PCM_MS_ADPCM;
}

HD bool is_adpcm(const bd_pcm_format& f) { return f.codec == BD_PCM_IMA_ADPCM || f.codec == BD_PCM_MS_ADPCM; }

// Frames whose codes lie entirely inside the first `rem` bytes of a block (0 when its header is not complete), at most
// samples_per_block.  For the layouts and G.711 a block is one frame.
HD int64_t block_frames(const bd_pcm_format& f, int64_t rem) {
    const int ch = f.channels;
    int64_t k;
    if (f.codec == BD_PCM_IMA_ADPCM) {
        // header (4 bytes per channel) = frame 0; then groups of one 4-byte word per channel, 8 frames each, low nibble
        // first: frame 1 + 8g + j needs byte j / 2 of the last channel's word of group g
        if (rem < 4 * ch) return 0;
        const int64_t body = rem - 4 * ch, g = body / (4 * ch), r = body % (4 * ch) - 4 * (ch - 1);
        k = 1 + 8 * g + (r > 0 ? (r >= 4 ? 8 : 2 * r) : 0);
    } else if (f.codec == BD_PCM_MS_ADPCM) {
        // header (7 bytes per channel) = frames 0 and 1; then nibbles interleaved by channel, high nibble first:
        // frame 2 + i needs nibble (i + 1) * ch - 1
        if (rem < 7 * ch) return 0;
        k = 2 + 2 * (rem - 7 * ch) / ch;
    } else {
        k = rem >= f.block_align ? 1 : 0;
    }
    return k < f.samples_per_block ? k : f.samples_per_block;
}

template <class S>
HD bool header_ok(const S& s, const bd_pcm_format& f, int64_t blk) {
    if (f.codec == BD_PCM_IMA_ADPCM) {
        for (int c = 0; c < f.channels; ++c)
            if (byte_at(s, blk + 4 * c + 2) > 88u) return false;
    } else if (f.codec == BD_PCM_MS_ADPCM) {
        for (int c = 0; c < f.channels; ++c)
            if (byte_at(s, blk + c) >= (uint32_t)f.n_coefs) return false;
    }
    return true;
}

// ---------------------------------------------------------------- G.711 (ITU-T G.711, the expansion audioop implements)
HD int32_t ulaw_to_s16(uint32_t u) {
    u = ~u & 0xFFu;
    int32_t t = (int32_t)(((u & 0x0Fu) << 3) + 0x84u);
    t <<= (u & 0x70u) >> 4;
    return (u & 0x80u) ? (0x84 - t) : (t - 0x84);
}

HD int32_t alaw_to_s16(uint32_t a) {
    a ^= 0x55u;
    int32_t t = (int32_t)((a & 0x0Fu) << 4);
    const int seg = (int)((a & 0x70u) >> 4);
    if (seg == 0) t += 8;
    else if (seg == 1) t += 0x108;
    else t = (t + 0x108) << (seg - 1);
    return (a & 0x80u) ? t : -t;
}

// ---------------------------------------------------------------- one stored sample -> output
// `b` holds the sample's W bytes in file order in its low bytes (b0 in bits 0-7); W = bits / 8.
template <int W>
struct Sample {
    // -> int16 (16-bit linear, G.711) in `i` or float32 in `x`
    HD static void convert(const bd_pcm_format& f, uint64_t b, int32_t& i, float& x) {
        if (f.codec == BD_PCM_ULAW) { i = ulaw_to_s16((uint32_t)b); return; }
        if (f.codec == BD_PCM_ALAW) { i = alaw_to_s16((uint32_t)b); return; }
        uint64_t v = b;
        if (f.big_endian) {
            v = 0;
            for (int k = 0; k < W; ++k) v |= ((b >> (8 * k)) & 0xFFu) << (8 * (W - 1 - k));
        }
        if (f.codec == BD_PCM_FLOAT) {
            if (W == 8) {
                double d;
                memcpy(&d, &v, 8);
                x = (float)d;
            } else {
                const uint32_t u = (uint32_t)v;
                memcpy(&x, &u, 4);
            }
            return;
        }
        constexpr int bits = W >= 4 ? 32 : 8 * W;
        uint32_t u = (uint32_t)v;
        if (!f.is_signed) u ^= 1u << (bits - 1);                    // offset binary -> two's complement
        const int32_t s = (int32_t)(u << (32 - bits)) >> (32 - bits);
        if (W == 2) i = s;
        else x = (float)s * (1.0f / (float)(1u << (bits - 1)));     // exact: a power of two (int -> float rounds to nearest)
    }
};

// ---------------------------------------------------------------- ADPCM
HD int ima_step(int index) {
    // the 89 step sizes of the IMA ADPCM recommendation (tests/test_pcm_host.py pins them against audioop)
    constexpr int16_t kStep[89] = {
        7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118,
        130, 143, 157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060,
        1166, 1282, 1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132,
        7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};
    return kStep[index];
}

HD int ima_index_delta(uint32_t code) { return (code & 4u) ? 2 * (int)(code & 3u) + 2 : -1; }   // -1 -1 -1 -1 2 4 6 8

HD int ms_adapt(uint32_t code) {
    // Microsoft ADPCM's adaptation of the quantiser step by the code just read (16 entries, the format's definition)
    constexpr int16_t kAdapt[16] = {230, 230, 230, 230, 307, 409, 512, 614, 768, 614, 512, 409, 307, 230, 230, 230};
    return kAdapt[code & 15u];
}

HD int32_t clamp16(int64_t v) { return (int32_t)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }

// Channel c of the block at byte `blk`: frames [0, limit) of the block; frame k goes to out when first <= start + k.
template <class S>
HD void ima_channel(const S& s, const bd_pcm_format& f, int64_t blk, int c, int64_t limit, int64_t start, int64_t first,
                    int16_t* out) {
    if (limit <= 0) return;
    const int ch = f.channels;
    int32_t pred = s16le(s, blk + 4 * c);
    int index = (int)byte_at(s, blk + 4 * c + 2);
    if (start >= first) out[(start - first) * ch + c] = (int16_t)pred;
    // one code word (8 frames) at a time: the step index chain does not wait for the predictor, so the 8 table lookups of
    // a word are issued before the predictor walks through them
    for (int64_t k0 = 1; k0 < limit; k0 += 8) {
        const uint32_t w = u32le(s, blk + 4 * ch + (((k0 - 1) >> 3) * ch + c) * 4);
        int step[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            step[j] = ima_step(index);
            index += ima_index_delta((w >> (4 * j)) & 15u);
            index = index < 0 ? 0 : (index > 88 ? 88 : index);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t k = k0 + j;
            if (k >= limit) break;
            const uint32_t code = (w >> (4 * j)) & 15u;
            int32_t diff = step[j] >> 3;
            if (code & 4u) diff += step[j];
            if (code & 2u) diff += step[j] >> 1;
            if (code & 1u) diff += step[j] >> 2;
            pred = clamp16((int64_t)pred + ((code & 8u) ? -diff : diff));
            if (start + k >= first) out[(start + k - first) * ch + c] = (int16_t)pred;
        }
    }
}

template <class S>
HD void ms_channel(const S& s, const bd_pcm_format& f, int64_t blk, int c, int64_t limit, int64_t start, int64_t first,
                   int16_t* out) {
    if (limit <= 0) return;                  // (the header is not read: it may not be complete)
    const int ch = f.channels;
    const int p = (int)byte_at(s, blk + c);
    const int64_t c1 = f.coefs[2 * p], c2 = f.coefs[2 * p + 1];
    int64_t delta = s16le(s, blk + ch + 2 * c);
    int64_t s1 = s16le(s, blk + 3 * ch + 2 * c), s2 = s16le(s, blk + 5 * ch + 2 * c);
    if (start >= first) out[(start - first) * ch + c] = (int16_t)s2;
    if (limit > 1 && start + 1 >= first) out[(start + 1 - first) * ch + c] = (int16_t)s1;
    // the codes are interleaved by channel: one aligned 32-bit word serves the 8 / ch frames whose codes it holds
    int64_t wa = -1;
    uint32_t w = 0;
    for (int64_t k = 2; k < limit; ++k) {
        const int64_t i = (k - 2) * ch + c;
        const int64_t a = blk + 7 * ch + (i >> 1);
        if ((a & ~3LL) != wa) {
            wa = a & ~3LL;
            w = s.word(wa);
        }
        const uint32_t byte = (w >> (8 * (int)(a & 3))) & 0xFFu;
        const uint32_t code = (i & 1) ? (byte & 15u) : (byte >> 4);
        const int64_t predict = (s1 * c1 + s2 * c2) >> 8;
        const int64_t v = clamp16(predict + (int64_t)((int32_t)(code << 28) >> 28) * delta);
        s2 = s1;
        s1 = v;
        delta = (ms_adapt(code) * delta) >> 8;
        delta = delta < 16 ? 16 : (delta > INT32_MAX ? INT32_MAX : delta);   // (the bound only matters to corrupt data)
        if (start + k >= first) out[(start + k - first) * ch + c] = (int16_t)v;
    }
}

// ---------------------------------------------------------------- the range
struct Range {
    int64_t base;       // absolute index of the range's first block
    int64_t blocks;     // blocks of the range that overlap [first, first + n) and hold at least one byte
    int64_t full;       // of which are complete
};

HD Range range_of(const bd_pcm_format& f, int64_t n_bytes, int64_t first, int64_t n) {
    Range r;
    const int64_t spb = f.samples_per_block;
    r.base = first / spb;
    const int64_t need = n > 0 ? (first + n - 1) / spb - r.base + 1 : 0;
    const int64_t have = (n_bytes + f.block_align - 1) / f.block_align;
    r.blocks = need < have ? need : have;
    const int64_t full = n_bytes / f.block_align;
    r.full = full < r.blocks ? full : r.blocks;
    return r;
}

// The status once the first bad block (relative, >= r.blocks: none) is known.
HD void fill_status(const bd_pcm_format& f, const Range& r, int64_t n_bytes, int64_t first, int64_t n, int64_t bad,
                    bd_pcm_status* st) {
    const int64_t spb = f.samples_per_block;
    int64_t end;
    if (bad < r.blocks) end = (r.base + bad) * spb;
    else if (r.blocks > r.full) end = (r.base + r.full) * spb + block_frames(f, n_bytes - r.full * f.block_align);
    else end = (r.base + r.blocks) * spb;
    int64_t got = end - first;
    got = got < 0 ? 0 : (got > n ? n : got);
    st->samples = got;
    st->end_sample = end;
    st->bad_block = bad < r.blocks ? r.base + bad : -1;
    st->reason = bad < r.blocks ? BD_PCM_STOP_BAD_HEADER : (got < n ? BD_PCM_STOP_TRUNCATED : BD_PCM_STOP_END);
    st->reserved = 0;
}

// ---------------------------------------------------------------- device
__device__ DevSrc dev_src(const void* data, int nbytes) {
    DevSrc s;
    s.rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(data), 0, (nbytes + 3) & ~3, 0x00020000);
    s.n = nbytes;
    return s;
}

template <int W>
struct Group {
    static constexpr int G = W <= 2 ? 8 : 4;         // stored samples per thread
    static constexpr int Words = G * W / 4;          // 32-bit words they occupy (2, 4, 3, 4, 8)
};

// Items (samples of all channels) [0, items) of the range; item i is stored at bytes [i W, (i + 1) W) and goes to out[i].
template <int W, bool Vec>
__global__ __launch_bounds__(kLayoutThreads) void pcm_layout(const void* data, int nbytes, bd_pcm_format f, long long items,
                                                             void* out, bd_pcm_status st_val, bd_pcm_status* status) {
    constexpr int G = Group<W>::G, Words = Group<W>::Words;
    const long long t = (long long)blockIdx.x * kLayoutThreads + threadIdx.x;
    if (t == 0) *status = st_val;
    const long long i0 = t * G;
    if (i0 >= items) return;
    const DevSrc s = dev_src(data, nbytes);
    const bool s16 = out_is_s16(f);
    int32_t iv[G];
    float fv[G];
    if (i0 + G <= items) {
        uint32_t w[Words];
        const int at = (int)(i0 * W);
        if constexpr (Words % 4 == 0) {
            for (int k = 0; k < Words; k += 4) {
                const auto v = __builtin_amdgcn_raw_buffer_load_b128(s.rs, at + 4 * k, 0, 0);
                w[k] = v[0]; w[k + 1] = v[1]; w[k + 2] = v[2]; w[k + 3] = v[3];
            }
        } else if constexpr (Words == 2) {
            const auto v = __builtin_amdgcn_raw_buffer_load_b64(s.rs, at, 0, 0);
            w[0] = v[0]; w[1] = v[1];
        } else {
            for (int k = 0; k < Words; ++k) w[k] = __builtin_amdgcn_raw_buffer_load_b32(s.rs, at + 4 * k, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            uint64_t b = 0;
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const int q = g * W + k;
                b |= (uint64_t)((w[q >> 2] >> (8 * (q & 3))) & 0xFFu) << (8 * k);
            }
            Sample<W>::convert(f, b, iv[g], fv[g]);
        }
        if (s16) {
            int16_t* o = static_cast<int16_t*>(out) + i0;
            if constexpr (Vec && G == 8) {
                uint4 v;
                v.x = (uint16_t)iv[0] | ((uint32_t)(uint16_t)iv[1] << 16);
                v.y = (uint16_t)iv[2] | ((uint32_t)(uint16_t)iv[3] << 16);
                v.z = (uint16_t)iv[4] | ((uint32_t)(uint16_t)iv[5] << 16);
                v.w = (uint16_t)iv[6] | ((uint32_t)(uint16_t)iv[7] << 16);
                *reinterpret_cast<uint4*>(o) = v;
            } else {
                for (int g = 0; g < G; ++g) o[g] = (int16_t)iv[g];
            }
        } else {
            float* o = static_cast<float*>(out) + i0;
            if constexpr (Vec) {
                for (int g = 0; g < G; g += 4) *reinterpret_cast<float4*>(o + g) = make_float4(fv[g], fv[g + 1], fv[g + 2], fv[g + 3]);
            } else {
                for (int g = 0; g < G; ++g) o[g] = fv[g];
            }
        }
        return;
    }
    for (long long i = i0; i < items; ++i) {          // the group that holds the end of the range
        uint64_t b = 0;
        for (int k = 0; k < W; ++k) b |= (uint64_t)byte_at(s, i * W + k) << (8 * k);
        int32_t a;
        float x;
        Sample<W>::convert(f, b, a, x);
        if (s16) static_cast<int16_t*>(out)[i] = (int16_t)a;
        else static_cast<float*>(out)[i] = x;
    }
}

__global__ __launch_bounds__(kAdpcmThreads) void pcm_adpcm_check(const void* data, int nbytes, bd_pcm_format f, Range r,
                                                                  int* bad) {
    const long long j = (long long)blockIdx.x * kAdpcmThreads + threadIdx.x;
    if (j >= r.blocks) return;
    const DevSrc s = dev_src(data, nbytes);
    const int64_t blk = j * f.block_align;
    // a final block whose header is not complete yields nothing and is no bad header
    if (block_frames(f, nbytes - blk) > 0 && !header_ok(s, f, blk)) atomicMin(bad, (int)j);
}

__global__ __launch_bounds__(kAdpcmThreads) void pcm_adpcm_decode(const void* data, int nbytes, bd_pcm_format f, Range r,
                                                                   long long first, long long n, const int* bad_word,
                                                                   int16_t* out, bd_pcm_status* status) {
    const long long lane = (long long)blockIdx.x * kAdpcmThreads + threadIdx.x;
    const int64_t bad = *bad_word;
    if (lane == 0) fill_status(f, r, nbytes, first, n, bad, status);
    const int ch = f.channels;
    const long long j = lane / ch;
    const int c = (int)(lane - j * ch);
    if (j >= r.blocks || j >= bad) return;
    const DevSrc s = dev_src(data, nbytes);
    const int64_t blk = j * f.block_align, start = (r.base + j) * f.samples_per_block;
    const int64_t rem = nbytes - blk;
    int64_t limit = block_frames(f, rem < f.block_align ? rem : f.block_align);
    if (limit > first + n - start) limit = first + n - start;
    if (f.codec == BD_PCM_IMA_ADPCM) ima_channel(s, f, blk, c, limit, start, first, out);
    else ms_channel(s, f, blk, c, limit, start, first, out);
}

// ---------------------------------------------------------------- host
int check_fmt(const bd_pcm_format* f, const char* who) {
    std::string why;
    if (!f) why = "no format";
    else if (f->channels < 1 || f->channels > BD_PCM_MAX_CHANNELS) why = "channels must be 1-8";
    else if (f->codec == BD_PCM_LINEAR || f->codec == BD_PCM_FLOAT) {
        const bool ok = f->codec == BD_PCM_LINEAR ? (f->bits == 8 || f->bits == 16 || f->bits == 24 || f->bits == 32)
                                                  : (f->bits == 32 || f->bits == 64);
        if (!ok) why = "unsupported sample width";
        else if (f->block_align != f->channels * f->bits / 8 || f->samples_per_block != 1) why = "block_align must be one frame";
    } else if (f->codec == BD_PCM_ULAW || f->codec == BD_PCM_ALAW) {
        if (f->bits != 8 || f->block_align != f->channels || f->samples_per_block != 1) why = "G.711 is one byte per sample";
    } else if (is_adpcm(*f)) {
        const int hdr = (f->codec == BD_PCM_IMA_ADPCM ? 4 : 7) * f->channels;
        bd_pcm_format g = *f;
        g.samples_per_block = INT32_MAX;
        if (f->bits != 4 || f->block_align < hdr || f->block_align > (1 << 24)) why = "bad ADPCM block_align";
        else if (f->samples_per_block < (f->codec == BD_PCM_IMA_ADPCM ? 1 : 2) || f->samples_per_block > block_frames(g, f->block_align))
            why = "samples_per_block does not fit the block";
        else if (f->codec == BD_PCM_MS_ADPCM && (f->n_coefs < 1 || f->n_coefs > BD_PCM_MAX_COEFS)) why = "MS ADPCM needs 1-32 coefficient pairs";
    } else {
        why = "unknown codec";
    }
    if (!why.empty()) {
        bd::set_error(std::string(who) + ": " + why);
        return BD_EINVAL;
    }
    return BD_OK;
}

template <int W>
void host_layout(const HostSrc& s, const bd_pcm_format& f, int64_t items, void* out) {
    const bool s16 = out_is_s16(f);
    for (int64_t i = 0; i < items; ++i) {
        uint64_t b = 0;
        for (int k = 0; k < W; ++k) b |= (uint64_t)s.p[i * W + k] << (8 * k);
        int32_t a;
        float x;
        Sample<W>::convert(f, b, a, x);
        if (s16) static_cast<int16_t*>(out)[i] = (int16_t)a;
        else static_cast<float*>(out)[i] = x;
    }
}

template <int W>
hipError_t launch_layout(const void* data, int nb, const bd_pcm_format& f, long long items, void* out, const bd_pcm_status& sv,
                         bd_pcm_status* status, hipStream_t st) {
    constexpr int G = Group<W>::G;
    const long long threads = (items + G - 1) / G;
    const unsigned blocks = (unsigned)((threads + kLayoutThreads - 1) / kLayoutThreads);
    if (((uintptr_t)out & 15) == 0)
        hipLaunchKernelGGL((pcm_layout<W, true>), dim3(blocks ? blocks : 1), dim3(kLayoutThreads), 0, st, data, nb, f, items, out, sv, status);
    else
        hipLaunchKernelGGL((pcm_layout<W, false>), dim3(blocks ? blocks : 1), dim3(kLayoutThreads), 0, st, data, nb, f, items, out, sv, status);
    return hipGetLastError();
}

}  // namespace

extern "C" {

int bd_pcm_abi_version(void) { return BD_PCM_ABI_VERSION; }

int bd_pcm_decode_host(const uint8_t* data, int64_t n_bytes, const bd_pcm_format* fmt, int64_t first, int64_t n, void* out,
                       bd_pcm_status* status) {
    const int rc = check_fmt(fmt, "bd_pcm_decode_host");
    if (rc != BD_OK) return rc;
    if ((!data && n_bytes) || n_bytes < 0 || first < 0 || n < 0 || (!out && n) || !status) {
        bd::set_error("bd_pcm_decode_host: bad argument");
        return BD_EINVAL;
    }
    const bd_pcm_format& f = *fmt;
    const HostSrc s{data, n_bytes};
    const Range r = range_of(f, n_bytes, first, n);
    if (!is_adpcm(f)) {
        fill_status(f, r, n_bytes, first, n, INT64_MAX, status);
        const int64_t items = status->samples * f.channels;
        switch (f.bits) {
            case 8: host_layout<1>(s, f, items, out); break;
            case 16: host_layout<2>(s, f, items, out); break;
            case 24: host_layout<3>(s, f, items, out); break;
            case 32: host_layout<4>(s, f, items, out); break;
            default: host_layout<8>(s, f, items, out); break;
        }
        return BD_OK;
    }
    int64_t bad = INT64_MAX;
    for (int64_t j = 0; j < r.blocks; ++j) {
        const int64_t blk = j * f.block_align;
        if (block_frames(f, n_bytes - blk) > 0 && !header_ok(s, f, blk)) {
            bad = j;
            break;
        }
    }
    fill_status(f, r, n_bytes, first, n, bad, status);
    int16_t* o = static_cast<int16_t*>(out);
    for (int64_t j = 0; j < r.blocks && j < bad; ++j) {
        const int64_t blk = j * f.block_align, start = (r.base + j) * f.samples_per_block;
        const int64_t rem = n_bytes - blk;
        int64_t limit = block_frames(f, rem < f.block_align ? rem : f.block_align);
        if (limit > first + n - start) limit = first + n - start;
        for (int c = 0; c < f.channels; ++c) {
            if (f.codec == BD_PCM_IMA_ADPCM) ima_channel(s, f, blk, c, limit, start, first, o);
            else ms_channel(s, f, blk, c, limit, start, first, o);
        }
    }
    return BD_OK;
}

int64_t bd_pcm_workspace_bytes(const bd_pcm_format* fmt, int64_t n_bytes, int64_t n) {
    const int rc = check_fmt(fmt, "bd_pcm_workspace_bytes");
    if (rc != BD_OK) return rc;
    if (n_bytes < 0 || n_bytes >= (int64_t(1) << 31) || n < 0) {
        bd::set_error("bd_pcm_workspace_bytes: byte range must be below 2 GiB");
        return BD_EINVAL;
    }
    return is_adpcm(*fmt) ? 256 : 0;               // the first bad block (one word, padded)
}

int bd_pcm_decode(const void* data, int64_t n_bytes, const bd_pcm_format* fmt, int64_t first, int64_t n, void* out,
                  void* workspace, int64_t workspace_bytes, void* status, void* stream) {
    const int rc = check_fmt(fmt, "bd_pcm_decode");
    if (rc != BD_OK) return rc;
    if ((!data && n_bytes) || n_bytes < 0 || n_bytes >= (int64_t(1) << 31) || first < 0 || n < 0 || (!out && n) || !status) {
        bd::set_error("bd_pcm_decode: bad argument");
        return BD_EINVAL;
    }
    const bd_pcm_format& f = *fmt;
    const Range r = range_of(f, n_bytes, first, n);
    hipStream_t st = static_cast<hipStream_t>(stream);
    bd_pcm_status* sp = static_cast<bd_pcm_status*>(status);
    const int nb = (int)n_bytes;
    hipError_t e = hipSuccess;
    if (!is_adpcm(f)) {
        bd_pcm_status sv;
        fill_status(f, r, n_bytes, first, n, INT64_MAX, &sv);
        const long long items = sv.samples * f.channels;
        switch (f.bits) {
            case 8: e = launch_layout<1>(data, nb, f, items, out, sv, sp, st); break;
            case 16: e = launch_layout<2>(data, nb, f, items, out, sv, sp, st); break;
            case 24: e = launch_layout<3>(data, nb, f, items, out, sv, sp, st); break;
            case 32: e = launch_layout<4>(data, nb, f, items, out, sv, sp, st); break;
            default: e = launch_layout<8>(data, nb, f, items, out, sv, sp, st); break;
        }
    } else {
        if (!workspace || workspace_bytes < 4) {
            bd::set_error("bd_pcm_decode: ADPCM needs a workspace of " + std::to_string(bd_pcm_workspace_bytes(fmt, n_bytes, n)) +
                          " bytes");
            return BD_EWORKSPACE;
        }
        int* bad = static_cast<int*>(workspace);
        e = hipMemsetAsync(bad, 0x7F, 4, st);      // INT_MAX-ish: no bad block yet (any value >= r.blocks means none)
        if (e == hipSuccess) {
            const unsigned cb = (unsigned)((r.blocks + kAdpcmThreads - 1) / kAdpcmThreads);
            if (cb) hipLaunchKernelGGL(pcm_adpcm_check, dim3(cb), dim3(kAdpcmThreads), 0, st, data, nb, f, r, bad);
            const long long lanes = r.blocks * f.channels;
            const unsigned db = (unsigned)((lanes + kAdpcmThreads - 1) / kAdpcmThreads);
            hipLaunchKernelGGL(pcm_adpcm_decode, dim3(db ? db : 1), dim3(kAdpcmThreads), 0, st, data, nb, f, r, (long long)first,
                               (long long)n, bad, static_cast<int16_t*>(out), sp);
            e = hipGetLastError();
        }
    }
    if (e != hipSuccess) {
        bd::set_error(std::string("bd_pcm_decode: ") + hipGetErrorString(e));
        return BD_EHIP;
    }
    return BD_OK;
}

}  // extern "C"
