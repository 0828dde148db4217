// FLAC frame decoder (include/buzzdetect_flac.h): sync scan, chain resolution and frame decode on gfx950, and the
// same parse / decode routines on the host.
//
// A byte range of one stream, starting on a frame boundary, becomes PCM in six stream-ordered launches:
//   flac_scan<false>   every byte offset: sync code + frame header + CRC-8 + STREAMINFO agreement -> hits per tile
//   flac_scan_prefix   one workgroup: exclusive prefix of the tiles' hit counts, the candidate total
//   flac_scan<true>    the same test again, each hit written to its place in the candidate list (offset order)
//   flac_parse         one lane per candidate: parse the frame to its end (no stores), CRC-16 -> end offset + verdict
//   flac_chain         one workgroup: next pointer per candidate (the candidate at its end offset whose frame / sample
//                      number follows on), pointer jumping from candidate 0 -> the frames of the stream, status record
//   flac_decode        one lane per frame on the chain that overlaps the window: decode into an int32 scratch
//   flac_convert       one thread per output sample: int32 -> int16 (16-bit streams) or float32 value / 2^(bps - 1)
// A sync pattern with a good CRC-8 can occur inside frame data; such a candidate lies strictly inside a real frame, so
// the chain from candidate 0 (whose next pointers follow real frame ends) never reaches it.
//
// Bits are read through a 64-bit window refilled by aligned 32-bit loads (on the device: raw buffer loads over the
// range rounded up to 4 bytes, so nothing past the caller's buffer is touched; past the range the parse sees zeros and
// stops on its bit limit).
#include <cstring>
#include <string>
#include <vector>

#include "bd_internal.h"
#include "bd_error.h"
#include "../../include/buzzdetect_flac.h"

namespace {

#define HD __host__ __device__ inline

enum : int { kOk = 0 };

constexpr int kScanThreads = 256, kScanPer = 16, kScanTile = kScanThreads * kScanPer;
constexpr int kLaneThreads = 64;
constexpr int kChainThreads = 1024;
constexpr int kConvertThreads = 256;

// ---------------------------------------------------------------- byte sources
struct HostSrc {
    const uint8_t* p;
    int64_t n;
    HD uint32_t word(int64_t a) const {          // bytes a .. a + 3, big-endian, zero past n (a is a multiple of 4)
        uint32_t v = 0;
        for (int k = 0; k < 4; ++k) v = (v << 8) | (a + k < n ? p[a + k] : 0u);
        return v;
    }
};

struct DevSrc {
    __amdgpu_buffer_rsrc_t rs;
    int64_t n;
    __device__ uint32_t word(int64_t a) const {
        return __builtin_bswap32(__builtin_amdgcn_raw_buffer_load_b32(rs, (int)a, 0, 0));
    }
};

template <class S>
HD uint32_t byte_at(const S& s, int64_t a) {
    return (s.word(a & ~3LL) >> (24 - 8 * (int)(a & 3))) & 0xFFu;
}

// ---------------------------------------------------------------- bit reader
template <class S>
struct Bits {
    const S& s;
    uint64_t win;     // the next `nb` bits of the stream, MSB first; the bits below them are zero
    int nb;
    int64_t pos;      // next (aligned) byte address to load

    HD Bits(const S& src, int64_t off) : s(src) {
        const int64_t a = off & ~3LL;
        const int skip = (int)(off - a);
        win = (uint64_t)s.word(a) << (32 + 8 * skip);
        nb = 32 - 8 * skip;
        pos = a + 4;
    }
    HD void refill() {
        if (nb <= 32) {
            win |= (uint64_t)s.word(pos) << (32 - nb);
            nb += 32;
            pos += 4;
        }
    }
    HD uint32_t get(int n) {                      // 0 <= n <= 32
        if (n == 0) return 0;
        if (nb < n) refill();
        const uint32_t v = (uint32_t)(win >> (64 - n));
        win <<= n;
        nb -= n;
        return v;
    }
    HD int32_t get_signed(int n) {
        if (n == 0) return 0;
        const uint32_t v = get(n) << (32 - n);
        return (int32_t)v >> (32 - n);
    }
    HD int64_t bitpos() const { return pos * 8 - nb; }
    HD void align() {
        const int r = nb & 7;
        win <<= r;
        nb -= r;
    }
    // zeros before the next 1 (which is consumed); false once the position passes `limit` bits
    HD bool unary(uint32_t& q, int64_t limit) {
        q = 0;
        for (;;) {
            refill();
            if (win != 0) {
                const int z = __builtin_clzll(win);
                q += (uint32_t)z;
                win <<= z;
                win <<= 1;
                nb -= z + 1;
                return true;
            }
            q += (uint32_t)nb;
            win = 0;
            nb = 0;
            if (bitpos() > limit) return false;
        }
    }
};

// ---------------------------------------------------------------- checksums
HD uint32_t crc8_update(uint32_t crc, uint32_t byte) {
    crc ^= byte;
    for (int k = 0; k < 8; ++k) crc = (crc & 0x80u) ? ((crc << 1) ^ 0x07u) & 0xFFu : (crc << 1) & 0xFFu;
    return crc;
}

HD uint32_t crc16_entry(uint32_t i) {
    uint32_t c = i << 8;
    for (int k = 0; k < 8; ++k) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) & 0xFFFFu : (c << 1) & 0xFFFFu;
    return c;
}

// CRC-16 of bytes [a, b) through the 256-entry table `t`
template <class S>
HD uint32_t crc16_range(const S& s, int64_t a, int64_t b, const uint16_t* t) {
    uint32_t crc = 0;
    for (int64_t w = a & ~3LL; w < b; w += 4) {
        const uint32_t v = s.word(w);
        for (int k = 0; k < 4; ++k) {
            const int64_t at = w + k;
            if (at >= a && at < b) crc = ((crc << 8) ^ t[((crc >> 8) ^ (v >> (24 - 8 * k))) & 0xFFu]) & 0xFFFFu;
        }
    }
    return crc;
}

// ---------------------------------------------------------------- frame header
struct Hdr {
    int64_t number, first_sample;
    int bs, rate, assign, channels, bps, variable, bytes;
};

// The header at `off`: sync, reserved bits, field codes, CRC-8; with `si` the fields must agree with STREAMINFO.
template <class S>
HD bool parse_header(const S& s, int64_t off, const bd_flac_streaminfo* si, Hdr& h) {
    if (off + 6 > s.n) return false;
    Bits<S> b(s, off);
    const uint32_t sync = b.get(16);
    if ((sync & 0xFFFEu) != 0xFFF8u) return false;
    h.variable = (int)(sync & 1u);
    const int bs_code = (int)b.get(4), sr_code = (int)b.get(4), assign = (int)b.get(4), bps_code = (int)b.get(3);
    if (b.get(1) != 0 || bs_code == 0 || sr_code == 15 || assign > 10 || bps_code == 3) return false;
    // UTF-8-style coded frame number (fixed blocking, <= 31 bits) or sample number (variable, <= 36 bits)
    const uint32_t c0 = b.get(8);
    int extra;
    uint64_t v;
    if (c0 < 0x80u) { v = c0; extra = 0; }
    else if ((c0 & 0xE0u) == 0xC0u) { v = c0 & 0x1Fu; extra = 1; }
    else if ((c0 & 0xF0u) == 0xE0u) { v = c0 & 0x0Fu; extra = 2; }
    else if ((c0 & 0xF8u) == 0xF0u) { v = c0 & 0x07u; extra = 3; }
    else if ((c0 & 0xFCu) == 0xF8u) { v = c0 & 0x03u; extra = 4; }
    else if ((c0 & 0xFEu) == 0xFCu) { v = c0 & 0x01u; extra = 5; }
    else if (c0 == 0xFEu) { v = 0; extra = 6; }
    else return false;
    if (extra > (h.variable ? 6 : 5)) return false;
    for (int k = 0; k < extra; ++k) {
        const uint32_t c = b.get(8);
        if ((c & 0xC0u) != 0x80u) return false;
        v = (v << 6) | (c & 0x3Fu);
    }
    int bs;
    if (bs_code == 1) bs = 192;
    else if (bs_code <= 5) bs = 576 << (bs_code - 2);
    else if (bs_code == 6) bs = (int)b.get(8) + 1;
    else if (bs_code == 7) bs = (int)b.get(16) + 1;
    else bs = 256 << (bs_code - 8);
    int rate = 0;
    switch (sr_code) {
        case 1: rate = 88200; break;   case 2: rate = 176400; break;  case 3: rate = 192000; break;
        case 4: rate = 8000; break;    case 5: rate = 16000; break;   case 6: rate = 22050; break;
        case 7: rate = 24000; break;   case 8: rate = 32000; break;   case 9: rate = 44100; break;
        case 10: rate = 48000; break;  case 11: rate = 96000; break;
        case 12: rate = (int)b.get(8) * 1000; break;
        case 13: rate = (int)b.get(16); break;
        case 14: rate = (int)b.get(16) * 10; break;
        default: break;
    }
    const int64_t crc_at = b.bitpos() / 8;
    if (crc_at + 1 > s.n) return false;
    const uint32_t crc_stored = b.get(8);
    uint32_t crc = 0;
    for (int64_t a = off; a < crc_at; ++a) crc = crc8_update(crc, byte_at(s, a));
    if (crc != crc_stored) return false;
    h.bs = bs;
    h.rate = rate;
    h.assign = assign;
    h.channels = assign < 8 ? assign + 1 : 2;
    h.bps = bps_code == 0 ? 0 : bps_code == 1 ? 8 : bps_code == 2 ? 12 : bps_code == 4 ? 16 : bps_code == 5 ? 20 : bps_code == 6 ? 24 : 32;
    h.number = (int64_t)v;
    h.bytes = (int)(crc_at + 1 - off);
    h.first_sample = h.variable ? h.number : h.number * bs;
    if (si) {
        if (h.bps == 0) h.bps = si->bits_per_sample;
        if (h.bps != si->bits_per_sample || h.channels != si->channels || bs > si->max_blocksize) return false;
        if (rate != 0 && rate != si->sample_rate) return false;
        if (!h.variable) h.first_sample = h.number * (int64_t)si->max_blocksize;
    }
    return true;
}

// ---------------------------------------------------------------- subframes
template <class Acc>
HD Acc mac(Acc s, int32_t c, int32_t x) {
    if constexpr (sizeof(Acc) == 4) return (Acc)((uint32_t)s + (uint32_t)c * (uint32_t)x);
    else return s + (Acc)c * (Acc)x;
}

// Residual partitions (Rice / Rice2 / escaped) of one subframe, each residual added to the order-`order` prediction
// from the history `h` (h[0] the newest sample) and stored shifted left by `wasted`.  W false: the bits are consumed,
// nothing is computed or stored (the parse pass).
template <int P, class Acc, bool W, class S>
__host__ __device__ __forceinline__ int residual(Bits<S>& b, int bs, int order, const int32_t (&c)[P], int shift, int32_t (&h)[P],
                                                 int wasted, int32_t* x, int stride, int64_t limit) {
    const uint32_t method = b.get(2);
    if (method > 1) return BD_FLAC_STOP_BAD_SUBFRAME;
    const int pbits = method ? 5 : 4, esc = method ? 31 : 15;
    const int po = (int)b.get(4);
    const int per = bs >> po;
    if ((per << po) != bs || per < order) return BD_FLAC_STOP_BAD_SUBFRAME;
    int i = order;
    for (int p = 0; p < (1 << po); ++p) {
        const int k = (int)b.get(pbits);
        const int cnt = p == 0 ? per - order : per;
        const int w = k == esc ? (int)b.get(5) : 0;
        for (int j = 0; j < cnt; ++j, ++i) {
            int32_t r;
            if (k == esc) {
                r = b.get_signed(w);
            } else {
                uint32_t q;
                if (!b.unary(q, limit)) return BD_FLAC_STOP_TRUNCATED;
                const uint32_t u = (q << k) | b.get(k);
                r = (int32_t)(u >> 1) ^ -(int32_t)(u & 1u);
            }
            if constexpr (W) {
                Acc s = 0;
#pragma unroll
                for (int t = 0; t < P; ++t) s = mac<Acc>(s, c[t], h[t]);
                const int32_t v = (int32_t)((uint32_t)r + (uint32_t)(int32_t)(s >> shift));
#pragma unroll
                for (int t = P - 1; t > 0; --t) h[t] = h[t - 1];
                h[0] = v;
                x[(int64_t)i * stride] = (int32_t)((uint32_t)v << wasted);
            }
        }
        if (b.bitpos() > limit) return BD_FLAC_STOP_TRUNCATED;
    }
    return kOk;
}

// coefficient t of the fixed predictor of order 1-4: {1}, {2, -1}, {3, -3, 1}, {4, -6, 4, -1}
HD int32_t fixed_coef(int order, int t) {
    switch (order) {
        case 1: return t == 0 ? 1 : 0;
        case 2: return t == 0 ? 2 : t == 1 ? -1 : 0;
        case 3: return t == 0 ? 3 : t == 1 ? -3 : t == 2 ? 1 : 0;
        case 4: return t == 0 ? 4 : t == 1 ? -6 : t == 2 ? 4 : t == 3 ? -1 : 0;
        default: return 0;
    }
}

HD int ceil_log2(int v) {
    int r = 0;
    while ((1 << r) < v) ++r;
    return r;
}

// FIXED (lpc false) or LPC subframe of order `order` <= P
template <int P, bool W, class S>
HD int predictive(Bits<S>& b, int bs, int order, bool lpc, int eb, int wasted, int32_t* x, int stride, int64_t limit) {
    int32_t h[P], c[P];
#pragma unroll
    for (int t = 0; t < P; ++t) h[t] = c[t] = 0;
    if (order > bs) return BD_FLAC_STOP_BAD_SUBFRAME;
    if constexpr (W) {
#pragma unroll
        for (int t = 0; t < P; ++t) {
            if (t < order) {
                const int32_t v = b.get_signed(eb);
                x[(int64_t)t * stride] = (int32_t)((uint32_t)v << wasted);
#pragma unroll
                for (int u = P - 1; u > 0; --u) h[u] = h[u - 1];
                h[0] = v;
            }
        }
    } else {
        for (int t = 0; t < order; ++t) b.get(eb);
    }
    int shift = 0, prec = 0;
    if (lpc) {
        prec = (int)b.get(4) + 1;
        shift = b.get_signed(5);
        if (prec == 16 || shift < 0) return BD_FLAC_STOP_BAD_SUBFRAME;
        if constexpr (W) {
#pragma unroll
            for (int t = 0; t < P; ++t)
                if (t < order) c[t] = b.get_signed(prec);
        } else {
            for (int t = 0; t < order; ++t) b.get(prec);
        }
    } else if constexpr (W) {
        // x[i] = sum c[t] x[i - 1 - t]: the fixed predictors of orders 1-4
#pragma unroll
        for (int t = 0; t < P; ++t) c[t] = fixed_coef(order, t);
    }
    if (b.bitpos() > limit) return BD_FLAC_STOP_TRUNCATED;
    // 32-bit sums whenever they cannot overflow: |sum| < order * 2^(prec - 1) * 2^(eb - 1) (fixed: |sum| <= 16 * 2^(eb - 1))
    if (!W || !lpc || eb + prec + ceil_log2(order) <= 32)
        return residual<P, int32_t, W>(b, bs, order, c, shift, h, wasted, x, stride, limit);
    return residual<P, int64_t, W>(b, bs, order, c, shift, h, wasted, x, stride, limit);
}

template <bool W, class S>
HD int predictive_any(Bits<S>& b, int bs, int order, bool lpc, int eb, int wasted, int32_t* x, int stride, int64_t limit) {
    if constexpr (!W) return predictive<1, false>(b, bs, order, lpc, eb, wasted, x, stride, limit);
    else {
        if (order <= 1) return predictive<1, true>(b, bs, order, lpc, eb, wasted, x, stride, limit);
        if (order <= 2) return predictive<2, true>(b, bs, order, lpc, eb, wasted, x, stride, limit);
        if (order <= 4) return predictive<4, true>(b, bs, order, lpc, eb, wasted, x, stride, limit);
        if (order <= 8) return predictive<8, true>(b, bs, order, lpc, eb, wasted, x, stride, limit);
        if (order <= 12) return predictive<12, true>(b, bs, order, lpc, eb, wasted, x, stride, limit);
        if (order <= 16) return predictive<16, true>(b, bs, order, lpc, eb, wasted, x, stride, limit);
        return predictive<32, true>(b, bs, order, lpc, eb, wasted, x, stride, limit);
    }
}

// One subframe of `bs` samples at `sbps` bits into x[0], x[stride], ...
template <bool W, class S>
HD int subframe(Bits<S>& b, int bs, int sbps, int32_t* x, int stride, int64_t limit) {
    if (b.get(1) != 0) return BD_FLAC_STOP_BAD_SUBFRAME;
    const int type = (int)b.get(6);
    int wasted = 0;
    if (b.get(1)) {
        uint32_t q;
        if (!b.unary(q, limit)) return BD_FLAC_STOP_TRUNCATED;
        if (q + 1 > (uint32_t)sbps) return BD_FLAC_STOP_BAD_SUBFRAME;
        wasted = (int)q + 1;
    }
    const int eb = sbps - wasted;
    if (type == 0) {                                    // CONSTANT
        const int32_t v = (int32_t)((uint32_t)b.get_signed(eb) << wasted);
        if constexpr (W)
            for (int i = 0; i < bs; ++i) x[(int64_t)i * stride] = v;
    } else if (type == 1) {                             // VERBATIM
        for (int i = 0; i < bs; ++i) {
            const int32_t v = b.get_signed(eb);
            if constexpr (W) x[(int64_t)i * stride] = (int32_t)((uint32_t)v << wasted);
        }
    } else if (type >= 8 && type <= 12) {               // FIXED, orders 0-4
        return predictive_any<W>(b, bs, type - 8, false, eb, wasted, x, stride, limit);
    } else if (type >= 32) {                            // LPC, orders 1-32
        return predictive_any<W>(b, bs, type - 31, true, eb, wasted, x, stride, limit);
    } else {
        return BD_FLAC_STOP_BAD_SUBFRAME;
    }
    return b.bitpos() > limit ? BD_FLAC_STOP_TRUNCATED : kOk;
}

// The frame at `off` (header `h` already parsed) up to its CRC-16: its end offset and verdict.  W: the samples go to
// pcm[i * channels + c], decorrelated.  CRC false: the CRC-16 is not recomputed (a frame already checked).
template <bool W, bool CRC, class S>
HD int frame(const S& s, int64_t off, const Hdr& h, const uint16_t* crc_table, int32_t* pcm, int64_t* end) {
    Bits<S> b(s, off + h.bytes);
    const int64_t limit = (s.n - 2) * 8;                // the CRC-16 must still fit
    for (int c = 0; c < h.channels; ++c) {
        const bool side = (h.assign == 8 && c == 1) || (h.assign == 9 && c == 0) || (h.assign == 10 && c == 1);
        const int rc = subframe<W>(b, h.bs, h.bps + (side ? 1 : 0), pcm + c, h.channels, limit);
        if (rc != kOk) return rc;
    }
    b.align();
    const int64_t body = b.bitpos() / 8;
    if (body + 2 > s.n) return BD_FLAC_STOP_TRUNCATED;
    const uint32_t stored = b.get(16);
    *end = body + 2;
    if (CRC && crc16_range(s, off, body, crc_table) != stored) return BD_FLAC_STOP_CRC16;
    if constexpr (W) {
        if (h.assign >= 8) {
            for (int i = 0; i < h.bs; ++i) {
                int32_t* p = pcm + (int64_t)i * 2;
                const int32_t a = p[0], d = p[1];
                if (h.assign == 8) {                    // left / side
                    p[1] = (int32_t)((uint32_t)a - (uint32_t)d);
                } else if (h.assign == 9) {             // side / right
                    p[0] = (int32_t)((uint32_t)a + (uint32_t)d);
                } else {                                // mid / side
                    const int32_t m = (int32_t)(((uint32_t)a << 1) | ((uint32_t)d & 1u));
                    p[0] = (int32_t)((uint32_t)m + (uint32_t)d) >> 1;
                    p[1] = (int32_t)((uint32_t)m - (uint32_t)d) >> 1;
                }
            }
        }
    }
    return kOk;
}

HD bool follows(int var_a, int64_t num_a, int bs_a, int var_b, int64_t num_b) {
    return var_a == var_b && (var_a ? num_b == num_a + bs_a : num_b == num_a + 1);
}

HD void put_sample(void* out, int64_t i, int32_t v, int bps) {
    if (bps == 16) static_cast<int16_t*>(out)[i] = (int16_t)v;
    else static_cast<float*>(out)[i] = (float)v * __builtin_bit_cast(float, (uint32_t)(127 - (bps - 1)) << 23);
}

// ---------------------------------------------------------------- device workspace
struct Layout {
    int64_t cap, tiles, pcm_samples;
    int64_t total, tile_count, off, end, code, bs, var, num, first, next, p0, p1, reached, pcm, bytes;
};

Layout layout(const bd_flac_streaminfo& si, int64_t nbytes, int64_t n) {
    Layout L;
    L.cap = nbytes / 8 + 64;                    // a frame is at least 10 bytes; room for false syncs besides
    L.tiles = (nbytes + kScanTile - 1) / kScanTile;
    L.pcm_samples = n + 2 * (int64_t)si.max_blocksize;
    int64_t at = 0;
    auto take = [&](int64_t bytes) { const int64_t o = at; at += (bytes + 255) / 256 * 256; return o; };
    L.total = take(64);
    L.tile_count = take(4 * (L.tiles + 1));
    L.off = take(4 * L.cap);
    L.end = take(4 * L.cap);
    L.code = take(4 * L.cap);
    L.bs = take(4 * L.cap);
    L.var = take(4 * L.cap);
    L.num = take(8 * L.cap);
    L.first = take(8 * L.cap);
    L.next = take(4 * L.cap);
    L.p0 = take(4 * L.cap);
    L.p1 = take(4 * L.cap);
    L.reached = take(4 * L.cap);
    L.pcm = take(4 * L.pcm_samples * si.channels);
    L.bytes = at;
    return L;
}

struct Cands {
    int* total;
    int* off;
    int* end;
    int* code;
    int* bs;
    int* var;
    long long* num;
    long long* first;
    int* next;
    int* p0;
    int* p1;
    int* reached;
};

__device__ DevSrc dev_src(const void* data, int nbytes) {
    DevSrc s;
    s.rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(data), 0, (nbytes + 3) & ~3, 0x00020000);
    s.n = nbytes;
    return s;
}

__device__ void load_crc_table(uint16_t* t) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) t[i] = (uint16_t)crc16_entry((uint32_t)i);
    __syncthreads();
}

// Hits of each tile of kScanTile bytes; WRITE: each hit's offset at its place in the candidate list.
template <bool WRITE>
__global__ __launch_bounds__(kScanThreads) void flac_scan(const void* data, int nbytes, bd_flac_streaminfo si,
                                                          int* tile_count, int* cand_off, int cap) {
    const DevSrc s = dev_src(data, nbytes);
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanPer;
    uint32_t w[kScanPer / 4 + 1];
#pragma unroll
    for (int k = 0; k < kScanPer / 4 + 1; ++k) w[k] = s.word(base + 4 * k);
    unsigned hits = 0;                                   // bit k: a frame header at base + k
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        const uint32_t b0 = (w[k >> 2] >> (24 - 8 * (k & 3))) & 0xFFu;
        const uint32_t b1 = (w[(k + 1) >> 2] >> (24 - 8 * ((k + 1) & 3))) & 0xFFu;
        if (b0 == 0xFFu && (b1 & 0xFEu) == 0xF8u && base + k < nbytes) {
            Hdr h;
            if (parse_header(s, base + k, &si, h)) hits |= 1u << k;
        }
    }
    // exclusive prefix of the threads' hit counts (wave prefix by shuffles, then across the block's waves)
    __shared__ int wave_sum[kScanThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int mine = __popc(hits);
    int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int v = __shfl_up(incl, d, 64);
        if (lane >= d) incl += v;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int before = 0, block_total = 0;
    for (int q = 0; q < kScanThreads / 64; ++q) {
        if (q < wave) before += wave_sum[q];
        block_total += wave_sum[q];
    }
    if (!WRITE) {
        if (threadIdx.x == 0) tile_count[blockIdx.x] = block_total;
        return;
    }
    int at = tile_count[blockIdx.x] + before + incl - mine;
    while (hits) {
        const int k = __builtin_ctz(hits);
        hits &= hits - 1;
        if (at < cap) cand_off[at] = (int)(base + k);
        ++at;
    }
}

// tile_count[0 .. tiles) -> exclusive prefix, the total into *total
__global__ __launch_bounds__(kChainThreads) void flac_scan_prefix(int* tile_count, int tiles, int* total) {
    __shared__ int part[kChainThreads];
    const int per = (tiles + kChainThreads - 1) / kChainThreads;
    const int a = threadIdx.x * per, b = min(a + per, tiles);
    int sum = 0;
    for (int i = a; i < b; ++i) sum += tile_count[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < kChainThreads; d <<= 1) {
        const int v = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - sum;
    for (int i = a; i < b; ++i) {
        const int c = tile_count[i];
        tile_count[i] = run;
        run += c;
    }
    if (threadIdx.x == kChainThreads - 1) *total = part[kChainThreads - 1];
}

// One lane per candidate: header fields, the frame's end offset and verdict (no samples stored).
__global__ __launch_bounds__(kLaneThreads) void flac_parse(const void* data, int nbytes, bd_flac_streaminfo si, Cands c, int cap) {
    __shared__ uint16_t table[256];
    load_crc_table(table);
    const DevSrc s = dev_src(data, nbytes);
    const int count = min(*c.total, cap);
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const int off = c.off[k];
        Hdr h;
        parse_header(s, off, &si, h);                     // (a candidate: the scan found it valid)
        int64_t end = off;
        const int rc = frame<false, true>(s, off, h, table, nullptr, &end);
        c.end[k] = (int)end;
        c.code[k] = rc;
        c.bs[k] = h.bs;
        c.var[k] = h.variable;
        c.num[k] = h.number;
        c.first[k] = h.first_sample;
    }
}

// One workgroup: next pointers, the frames reachable from candidate 0 (pointer jumping), the status record.
__global__ __launch_bounds__(kChainThreads) void flac_chain(int nbytes, Cands c, int cap, long long first, long long n,
                                                            bd_flac_status* st) {
    __shared__ int s_last, s_reached;
    const int total = *c.total;
    const int count = min(total, cap);
    if (total > cap || count == 0 || c.off[0] != 0) {
        if (threadIdx.x == 0) {
            st->samples = 0;
            st->stop_offset = 0;
            st->first_sample = total > cap || count == 0 || c.off[0] != 0 ? -1 : c.first[0];
            st->end_sample = st->first_sample;
            st->reason = total > cap ? BD_FLAC_STOP_OVERFLOW : (nbytes == 0 ? BD_FLAC_STOP_END : BD_FLAC_STOP_LOST_SYNC);
            st->frames = 0;
        }
        return;
    }
    for (int k = threadIdx.x; k < count; k += kChainThreads) {
        int nx = -1;
        const int e = c.end[k];
        if (c.code[k] == kOk && e < nbytes) {
            int lo = k + 1, hi = count - 1;
            while (lo <= hi) {
                const int mid = (lo + hi) >> 1;
                const int o = c.off[mid];
                if (o == e) { lo = mid; break; }
                if (o < e) lo = mid + 1; else hi = mid - 1;
            }
            if (lo < count && c.off[lo] == e && follows(c.var[k], c.num[k], c.bs[k], c.var[lo], c.num[lo])) nx = lo;
        }
        c.next[k] = nx;
        c.p0[k] = nx;
        c.reached[k] = k == 0;
    }
    if (threadIdx.x == 0) { s_last = 0; s_reached = 0; }
    __syncthreads();
    // after round r every frame within 2^(r + 1) - 1 steps of candidate 0 is marked (a mark made within a round is
    // reachable too, so the race of marks inside a round only adds reachable frames)
    int* p = c.p0;
    int* q = c.p1;
    for (int span = 1; span < count; span <<= 1) {
        for (int k = threadIdx.x; k < count; k += kChainThreads)
            if (c.reached[k] && p[k] >= 0) c.reached[p[k]] = 1;
        __syncthreads();
        for (int k = threadIdx.x; k < count; k += kChainThreads) q[k] = p[k] >= 0 ? p[p[k]] : -1;
        __syncthreads();
        int* t = p; p = q; q = t;
    }
    int last = 0, marked = 0;
    for (int k = threadIdx.x; k < count; k += kChainThreads)
        if (c.reached[k]) { last = k; ++marked; }
    atomicMax(&s_last, last);
    atomicAdd(&s_reached, marked);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int t = s_last;
        const bool good = c.code[t] == kOk;
        const long long base = c.first[0];
        const long long end_sample = good ? c.first[t] + c.bs[t] : c.first[t];
        st->first_sample = base;
        st->end_sample = end_sample;
        st->frames = s_reached - (good ? 0 : 1);
        if (!good) { st->reason = c.code[t]; st->stop_offset = c.off[t]; }
        else if (c.end[t] == nbytes) { st->reason = BD_FLAC_STOP_END; st->stop_offset = nbytes; }
        else { st->reason = BD_FLAC_STOP_LOST_SYNC; st->stop_offset = c.end[t]; }
        long long got = base > first ? 0 : end_sample - first;
        st->samples = got < 0 ? 0 : (got > n ? n : got);
    }
}

// One lane per frame of the chain that overlaps [first, first + n): samples into pcm, whose row 0 is sample first - max_bs.
__global__ __launch_bounds__(kLaneThreads) void flac_decode(const void* data, int nbytes, bd_flac_streaminfo si, Cands c, int cap,
                                                             long long first, long long n, int32_t* pcm) {
    const DevSrc s = dev_src(data, nbytes);
    const int count = min(*c.total, cap);
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        if (!c.reached[k] || c.code[k] != kOk) continue;
        const long long fs = c.first[k];
        if (fs >= first + n || fs + c.bs[k] <= first) continue;
        const int off = c.off[k];
        Hdr h;
        parse_header(s, off, &si, h);
        int64_t end;
        frame<true, false>(s, off, h, nullptr, pcm + (fs - first + si.max_blocksize) * si.channels, &end);
    }
}

__global__ __launch_bounds__(kConvertThreads) void flac_convert(const int32_t* pcm, int channels, int max_bs, int bps,
                                                                const bd_flac_status* st, void* out, long long n) {
    const long long i = (long long)blockIdx.x * kConvertThreads + threadIdx.x;
    if (i >= st->samples * channels) return;
    put_sample(out, i, pcm[(long long)max_bs * channels + i], bps);
}

int check_si(const bd_flac_streaminfo* si, const char* who) {
    if (!si) { bd::set_error(std::string(who) + ": no STREAMINFO"); return BD_EINVAL; }
    if (si->bits_per_sample < 4 || si->bits_per_sample > 24) {
        bd::set_error(std::string(who) + ": " + std::to_string(si->bits_per_sample) + "-bit streams are not supported (4-24)");
        return BD_EINVAL;
    }
    if (si->channels < 1 || si->channels > BD_FLAC_MAX_CHANNELS || si->max_blocksize < 16 || si->max_blocksize > 65535 ||
        si->min_blocksize < 1 || si->min_blocksize > si->max_blocksize) {
        bd::set_error(std::string(who) + ": bad STREAMINFO");
        return BD_EINVAL;
    }
    return BD_OK;
}

const uint16_t* host_crc_table() {
    static const std::vector<uint16_t> t = [] {
        std::vector<uint16_t> v(256);
        for (int i = 0; i < 256; ++i) v[i] = (uint16_t)crc16_entry((uint32_t)i);
        return v;
    }();
    return t.data();
}

}  // namespace

extern "C" {

int bd_flac_abi_version(void) { return BD_FLAC_ABI_VERSION; }

uint32_t bd_flac_crc8(const uint8_t* data, int64_t n) {
    uint32_t crc = 0;
    for (int64_t i = 0; i < n; ++i) crc = crc8_update(crc, data[i]);
    return crc;
}

uint32_t bd_flac_crc16(const uint8_t* data, int64_t n) {
    const HostSrc s{data, n};
    return n > 0 ? crc16_range(s, 0, n, host_crc_table()) : 0;
}

int bd_flac_parse_frame_header(const uint8_t* data, int64_t n, const bd_flac_streaminfo* si, bd_flac_frame_header* out) {
    if (!data || n < 0 || !out) { bd::set_error("bd_flac_parse_frame_header: bad argument"); return BD_EINVAL; }
    const HostSrc s{data, n};
    Hdr h;
    if (!parse_header(s, 0, si, h)) return 0;
    out->number = h.number;
    out->first_sample = h.first_sample;
    out->blocksize = h.bs;
    out->sample_rate = h.rate;
    out->channel_assignment = h.assign;
    out->channels = h.channels;
    out->bits_per_sample = h.bps;
    out->variable = h.variable;
    out->header_bytes = h.bytes;
    out->reserved = 0;
    return h.bytes;
}

int bd_flac_decode_host(const uint8_t* data, int64_t n_bytes, const bd_flac_streaminfo* si, int64_t first, int64_t n,
                        void* out, bd_flac_status* status) {
    const int rc = check_si(si, "bd_flac_decode_host");
    if (rc != BD_OK) return rc;
    if ((!data && n_bytes) || n_bytes < 0 || first < 0 || n < 0 || (!out && n) || !status) {
        bd::set_error("bd_flac_decode_host: bad argument");
        return BD_EINVAL;
    }
    const HostSrc s{data, n_bytes};
    const uint16_t* table = host_crc_table();
    const int ch = si->channels;
    std::vector<int32_t> buf((size_t)si->max_blocksize * ch);
    int64_t off = 0, base = -1, end_sample = -1;
    int frames = 0, reason = BD_FLAC_STOP_END, pvar = 0, pbs = 0;
    int64_t pnum = 0;
    while (off < n_bytes) {
        Hdr h;
        if (!parse_header(s, off, si, h) || (frames > 0 && !follows(pvar, pnum, pbs, h.variable, h.number))) {
            reason = BD_FLAC_STOP_LOST_SYNC;
            break;
        }
        if (base < 0) base = end_sample = h.first_sample;
        const int64_t fs = h.first_sample;
        const bool want = fs < first + n && fs + h.bs > first;
        int64_t end = off;
        const int code = want ? frame<true, true>(s, off, h, table, buf.data(), &end)
                              : frame<false, true>(s, off, h, table, nullptr, &end);
        if (code != kOk) {
            reason = code;
            break;
        }
        if (want) {
            const int64_t a = fs > first ? fs : first;
            const int64_t b = fs + h.bs < first + n ? fs + h.bs : first + n;
            for (int64_t i = a; i < b; ++i)
                for (int c = 0; c < ch; ++c) put_sample(out, (i - first) * ch + c, buf[(size_t)(i - fs) * ch + c], si->bits_per_sample);
        }
        ++frames;
        end_sample = fs + h.bs;
        pvar = h.variable;
        pnum = h.number;
        pbs = h.bs;
        off = end;
    }
    int64_t got = (base < 0 || base > first) ? 0 : end_sample - first;
    status->samples = got < 0 ? 0 : (got > n ? n : got);
    status->stop_offset = off;
    status->first_sample = base;
    status->end_sample = end_sample;
    status->reason = reason;
    status->frames = frames;
    return BD_OK;
}

int64_t bd_flac_workspace_bytes(const bd_flac_streaminfo* si, int64_t n_bytes, int64_t n) {
    const int rc = check_si(si, "bd_flac_workspace_bytes");
    if (rc != BD_OK) return rc;
    if (n_bytes < 0 || n_bytes >= (int64_t(1) << 31) || n < 0) {
        bd::set_error("bd_flac_workspace_bytes: byte range must be below 2 GiB");
        return BD_EINVAL;
    }
    return layout(*si, n_bytes, n).bytes;
}

int bd_flac_decode(const void* data, int64_t n_bytes, const bd_flac_streaminfo* si, int64_t first, int64_t n, void* out,
                   void* workspace, int64_t workspace_bytes, void* status, void* stream) {
    const int rc = check_si(si, "bd_flac_decode");
    if (rc != BD_OK) return rc;
    if ((!data && n_bytes) || n_bytes < 0 || n_bytes >= (int64_t(1) << 31) || first < 0 || n < 0 || (!out && n) || !status ||
        !workspace) {
        bd::set_error("bd_flac_decode: bad argument");
        return BD_EINVAL;
    }
    const Layout L = layout(*si, n_bytes, n);
    if (workspace_bytes < L.bytes) {
        bd::set_error("bd_flac_decode: workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(L.bytes) +
                      " needed");
        return BD_EWORKSPACE;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    Cands c{reinterpret_cast<int*>(ws + L.total), reinterpret_cast<int*>(ws + L.off), reinterpret_cast<int*>(ws + L.end),
            reinterpret_cast<int*>(ws + L.code), reinterpret_cast<int*>(ws + L.bs), reinterpret_cast<int*>(ws + L.var),
            reinterpret_cast<long long*>(ws + L.num), reinterpret_cast<long long*>(ws + L.first),
            reinterpret_cast<int*>(ws + L.next), reinterpret_cast<int*>(ws + L.p0), reinterpret_cast<int*>(ws + L.p1),
            reinterpret_cast<int*>(ws + L.reached)};
    int* tile_count = reinterpret_cast<int*>(ws + L.tile_count);
    const int nb = (int)n_bytes, cap = (int)L.cap, tiles = (int)L.tiles;
    hipError_t e = hipMemsetAsync(c.total, 0, 4, st);
    if (e == hipSuccess && tiles > 0) {
        hipLaunchKernelGGL(flac_scan<false>, dim3(tiles), dim3(kScanThreads), 0, st, data, nb, *si, tile_count, c.off, cap);
        hipLaunchKernelGGL(flac_scan_prefix, dim3(1), dim3(kChainThreads), 0, st, tile_count, tiles, c.total);
        hipLaunchKernelGGL(flac_scan<true>, dim3(tiles), dim3(kScanThreads), 0, st, data, nb, *si, tile_count, c.off, cap);
        // lanes for the frames a range can hold (grid-stride beyond)
        const int64_t frames = (L.pcm_samples + si->min_blocksize - 1) / si->min_blocksize + 64;
        const int64_t lanes = frames < L.cap ? frames : L.cap;
        int blocks = (int)((lanes + kLaneThreads - 1) / kLaneThreads);
        if (blocks > 16 * bd::cu_count()) blocks = 16 * bd::cu_count();
        hipLaunchKernelGGL(flac_parse, dim3(blocks), dim3(kLaneThreads), 0, st, data, nb, *si, c, cap);
        hipLaunchKernelGGL(flac_chain, dim3(1), dim3(kChainThreads), 0, st, nb, c, cap, (long long)first, (long long)n,
                           static_cast<bd_flac_status*>(status));
        hipLaunchKernelGGL(flac_decode, dim3(blocks), dim3(kLaneThreads), 0, st, data, nb, *si, c, cap, (long long)first,
                           (long long)n, reinterpret_cast<int32_t*>(ws + L.pcm));
    } else if (e == hipSuccess) {
        hipLaunchKernelGGL(flac_chain, dim3(1), dim3(kChainThreads), 0, st, nb, c, cap, (long long)first, (long long)n,
                           static_cast<bd_flac_status*>(status));
    }
    if (e == hipSuccess && n > 0) {
        const int64_t items = n * si->channels;
        hipLaunchKernelGGL(flac_convert, dim3((unsigned)((items + kConvertThreads - 1) / kConvertThreads)), dim3(kConvertThreads), 0,
                           st, reinterpret_cast<const int32_t*>(ws + L.pcm), si->channels, si->max_blocksize, si->bits_per_sample,
                           static_cast<const bd_flac_status*>(status), out, (long long)n);
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) {
        bd::set_error(std::string("bd_flac_decode: ") + hipGetErrorString(e));
        return BD_EHIP;
    }
    return BD_OK;
}

}  // extern "C"
