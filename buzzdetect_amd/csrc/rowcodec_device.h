// What the kernels of rowcodec.hip and their host restatements (bd_rows_encode_host / bd_rows_decode_host) must agree on bit
// for bit and therefore both compile from, as evalsweep_device.h is for its kernel: a row's exponent, an element's code and
// its decoded value (include/buzzdetect_rows.h states the rules and derives the bounds).  Every operation is exact or one
// correctly rounded conversion: frexpf, ldexpf by an integer, one float32 -> binary16 conversion to nearest even, rintf.
#ifndef BD_ROWCODEC_DEVICE_H
#define BD_ROWCODEC_DEVICE_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/buzzdetect_rows.h"

namespace bd {
namespace rowcodec {

constexpr int kDim = BD_EMBEDDING_SIZE;
constexpr int32_t kBadExponent = INT32_MIN;               // the record of a row that is not representable
constexpr uint32_t kQuietNaN = 0x7FC00000u;               // what such a record decodes to
constexpr int kHeaderWords = BD_ROWS_HEADER_BYTES / 4;

__host__ __device__ constexpr int record_bytes(int codec) {
    return codec == BD_ROWS_F32 ? kDim * 4 : codec == BD_ROWS_H ? BD_ROWS_HEADER_BYTES + kDim * 2 : BD_ROWS_HEADER_BYTES + kDim;
}

// an infinity or a NaN; under B also a negative element (-0.0f is zero)
__host__ __device__ inline bool bad_element(float x, int codec) {
    return !(fabsf(x) <= 3.402823466e+38f) || (codec == BD_ROWS_B && x < 0.0f);
}

// e of a row whose largest magnitude is m (finite, >= 0): m = f 2^p, f in [0.5, 1)
__host__ __device__ inline int32_t exponent(float m, int codec) {
    if (!(m > 0.0f)) return 0;
    int p = 0;
    (void)frexpf(m, &p);
    return p - (codec == BD_ROWS_H ? 15 : 8);
}

__host__ __device__ inline uint16_t code_h(float x, int32_t e) {
    float s = ldexpf(x, -e);
    s = s > BD_ROWS_H_MAX_CODE ? BD_ROWS_H_MAX_CODE : (s < -BD_ROWS_H_MAX_CODE ? -BD_ROWS_H_MAX_CODE : s);
    const _Float16 h = (_Float16)s;                       // round to nearest even
    uint16_t bits;
    memcpy(&bits, &h, sizeof(bits));
    return bits;
}

__host__ __device__ inline float value_h(uint16_t bits, int32_t e) {
    _Float16 h;
    memcpy(&h, &bits, sizeof(h));
    return ldexpf((float)h, e);
}

__host__ __device__ inline uint8_t code_b(float x, int32_t e) {
    const float r = rintf(ldexpf(x, -e));                 // x >= 0 here, r in 0 .. 256
    return (uint8_t)(r > 255.0f ? 255 : (int)r);
}

__host__ __device__ inline float value_b(uint8_t code, int32_t e) { return ldexpf((float)code, e); }

}  // namespace rowcodec
}  // namespace bd

#endif  // BD_ROWCODEC_DEVICE_H
