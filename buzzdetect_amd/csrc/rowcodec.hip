// The record codec and slice checksums of stored embedding rows for gfx950 (include/buzzdetect_rows.h).
//
//   rows_encode_kernel<CODEC>   a wave per row, four rows per workgroup.  A lane loads its 16 floats as four float4, the row's
//                               largest magnitude goes round the wave by a butterfly, every lane encodes its own elements with
//                               the row's exponent and stores them 16 bytes at a time; lane 0 also stores the 16-byte header.
//                               Which elements a lane owns follows the record, so that its stores are whole 16-byte pieces:
//                                 F32  float4 k 64 + lane, k = 0..3                       -> the same float4 of the record
//                                 H    elements 8 c .. 8 c + 7, c = k 64 + lane, k = 0, 1  -> code bytes 16 c .. 16 c + 15
//                                 B    elements 16 lane .. 16 lane + 15                   -> code bytes 16 lane .. + 15
//   rows_decode_kernel<CODEC>   the walk backwards, laid out by its stores: lane and k take float4 k 64 + lane of the row (16-byte
//                               stores, a KB in a row per wave) and load the 16 / 8 / 4 record bytes that hold it.
//
// Both sum the 32-bit words they store (encode) or load (decode) into S1 and S2 in 64-bit integer registers, weight i + 1 by the
// word's place in its slice; a butterfly brings a wave's sums to every lane, four waves meet in 64 bytes of LDS, and one thread a
// workgroup adds the pair to the slice's words with two integer atomics (256 rows a slice: 64 pairs land on a slice's words).
// BD_ROWS_SLICE is a multiple of the rows of a workgroup, so a workgroup's rows lie in one slice.  Integer sums mod 2^64: the
// result is a function of the bytes alone.  The kernels are bound by HBM: 4096 B in and 4096 / 2064 / 1040 B out per row.
#include "bd_error.h"
#include "rowcodec_device.h"

#include "../../include/buzzdetect_rows.h"

#include <cstdint>
#include <cstring>
#include <string>

namespace bd {
namespace {

using namespace rowcodec;

constexpr int kWaves = 4;                                 // rows per workgroup
static_assert(BD_ROWS_SLICE % kWaves == 0, "a workgroup's rows lie in one slice");
static_assert(kDim == 64 * 16, "a lane owns 16 elements of a row");
static_assert(record_bytes(BD_ROWS_F32) % 16 == 0 && record_bytes(BD_ROWS_H) % 16 == 0 && record_bytes(BD_ROWS_B) % 16 == 0,
              "records keep 16-byte alignment");

typedef unsigned long long u64;

struct Sums {
    u64 s1 = 0, s2 = 0;
    u64 base = 0;                                         // words of the slice in front of this record
    __device__ __host__ void add(unsigned word_of_record, uint32_t w) {
        s1 += w;
        s2 += (base + word_of_record + 1) * (u64)w;
    }
    __device__ __host__ void add4(unsigned first_word, const uint4& v) {
        add(first_word, v.x);
        add(first_word + 1, v.y);
        add(first_word + 2, v.z);
        add(first_word + 3, v.w);
    }
};

// A workgroup's sums onto its slice: butterfly inside each wave, the four waves through LDS, two atomics by thread 0.  Every
// thread of the workgroup comes here (a wave without a row brings zeros).
__device__ __forceinline__ void flush_sums(Sums s, u64* __restrict__ sums, long long first_row) {
    __shared__ u64 s_part[kWaves][2];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s.s1 += __shfl_xor(s.s1, o, 64);
        s.s2 += __shfl_xor(s.s2, o, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_part[wave][0] = s.s1;
        s_part[wave][1] = s.s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 a = 0, b = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            a += s_part[w][0];
            b += s_part[w][1];
        }
        u64* mine = sums + 2 * (first_row / BD_ROWS_SLICE);
        atomicAdd(&mine[0], a);
        atomicAdd(&mine[1], b);
    }
}

__device__ __forceinline__ uint32_t bits_of(float x) { return __float_as_uint(x); }

template <int CODEC>
__global__ __launch_bounds__(64 * kWaves) void rows_encode_kernel(const float* __restrict__ rows, long long W,
                                                                  unsigned char* __restrict__ records, u64* __restrict__ sums,
                                                                  unsigned* __restrict__ flags) {
    constexpr int kRecord = record_bytes(CODEC);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long first_row = (long long)blockIdx.x * kWaves;
    const long long row = first_row + wave;
    Sums sum;
    if (row < W) {                                        // (wave-uniform)
        sum.base = (u64)(row % BD_ROWS_SLICE) * (kRecord / 4);
        const float4* __restrict__ src = reinterpret_cast<const float4*>(rows + (size_t)row * kDim);
        unsigned char* __restrict__ rec = records + (size_t)row * kRecord;
        float4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int at = CODEC == BD_ROWS_F32 ? k * 64 + lane : CODEC == BD_ROWS_H ? 2 * ((k >> 1) * 64 + lane) + (k & 1) : 4 * lane + k;
            v[k] = src[at];
        }
        float m = 0.0f;
        bool bad = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float x[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                bad |= bad_element(x[j], CODEC);
                m = fmaxf(m, fabsf(x[j]));
            }
        }
        bad = __ballot(bad) != 0;
        if (bad && lane == 0) atomicAdd(flags, 1u);
        if constexpr (CODEC == BD_ROWS_F32) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint4 w = make_uint4(bits_of(v[k].x), bits_of(v[k].y), bits_of(v[k].z), bits_of(v[k].w));
                reinterpret_cast<uint4*>(rec)[k * 64 + lane] = w;
                sum.add4(4 * (k * 64 + lane), w);
            }
        } else {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
            const int32_t e = bad ? kBadExponent : exponent(m, CODEC);
            if (lane == 0) {
                const uint4 head = make_uint4((uint32_t)e, 0u, 0u, 0u);
                reinterpret_cast<uint4*>(rec)[0] = head;
                sum.add4(0, head);
            }
            uint4* __restrict__ codes = reinterpret_cast<uint4*>(rec + BD_ROWS_HEADER_BYTES);
            if constexpr (CODEC == BD_ROWS_H) {
#pragma unroll
                for (int c = 0; c < 2; ++c) {             // elements 8 (c 64 + lane) ..: v[2 c], v[2 c + 1]
                    const float4 a = v[2 * c], b = v[2 * c + 1];
                    uint4 w = make_uint4(0u, 0u, 0u, 0u);
                    if (!bad) {
                        w.x = code_h(a.x, e) | ((uint32_t)code_h(a.y, e) << 16);
                        w.y = code_h(a.z, e) | ((uint32_t)code_h(a.w, e) << 16);
                        w.z = code_h(b.x, e) | ((uint32_t)code_h(b.y, e) << 16);
                        w.w = code_h(b.z, e) | ((uint32_t)code_h(b.w, e) << 16);
                    }
                    codes[c * 64 + lane] = w;
                    sum.add4(kHeaderWords + 4 * (c * 64 + lane), w);
                }
            } else {
                uint32_t w[4] = {0u, 0u, 0u, 0u};
                if (!bad) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        w[k] = code_b(v[k].x, e) | ((uint32_t)code_b(v[k].y, e) << 8) | ((uint32_t)code_b(v[k].z, e) << 16) |
                               ((uint32_t)code_b(v[k].w, e) << 24);
                }
                const uint4 out = make_uint4(w[0], w[1], w[2], w[3]);
                codes[lane] = out;
                sum.add4(kHeaderWords + 4 * lane, out);
            }
        }
    }
    flush_sums(sum, sums, first_row);
}

template <int CODEC>
__global__ __launch_bounds__(64 * kWaves) void rows_decode_kernel(const unsigned char* __restrict__ records, long long W,
                                                                  float* __restrict__ rows, u64* __restrict__ sums) {
    constexpr int kRecord = record_bytes(CODEC);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long first_row = (long long)blockIdx.x * kWaves;
    const long long row = first_row + wave;
    Sums sum;
    if (row < W) {                                        // (wave-uniform)
        sum.base = (u64)(row % BD_ROWS_SLICE) * (kRecord / 4);
        const unsigned char* __restrict__ rec = records + (size_t)row * kRecord;
        float4* __restrict__ dst = reinterpret_cast<float4*>(rows + (size_t)row * kDim);
        if constexpr (CODEC == BD_ROWS_F32) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint4 w = reinterpret_cast<const uint4*>(rec)[k * 64 + lane];
                sum.add4(4 * (k * 64 + lane), w);
                dst[k * 64 + lane] = make_float4(__uint_as_float(w.x), __uint_as_float(w.y), __uint_as_float(w.z), __uint_as_float(w.w));
            }
        } else {
            const uint4 head = reinterpret_cast<const uint4*>(rec)[0];        // every lane: one line, and each needs e
            if (lane == 0) sum.add4(0, head);
            const int32_t e = (int32_t)head.x;
            const bool bad = e == kBadExponent;
            const float nan = __uint_as_float(kQuietNaN);
            // The floats are four times (twice) the codes: the stores decide.  Lane and k take float4 k 64 + lane, a wave's store
            // one KB in a row, and load the 8 (4) code bytes that belong to it (16-byte code loads would leave every store's
            // lanes 32 (64) bytes apart: measured at 0.34 of the HBM peak for b where encode reaches 0.57)
            if constexpr (CODEC == BD_ROWS_H) {
                const uint2* __restrict__ codes = reinterpret_cast<const uint2*>(rec + BD_ROWS_HEADER_BYTES);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint2 w = codes[k * 64 + lane];
                    sum.add(kHeaderWords + 2 * (k * 64 + lane), w.x);
                    sum.add(kHeaderWords + 2 * (k * 64 + lane) + 1, w.y);
                    dst[k * 64 + lane] = bad ? make_float4(nan, nan, nan, nan)
                                             : make_float4(value_h((uint16_t)(w.x & 0xFFFFu), e), value_h((uint16_t)(w.x >> 16), e),
                                                           value_h((uint16_t)(w.y & 0xFFFFu), e), value_h((uint16_t)(w.y >> 16), e));
                }
            } else {
                const uint32_t* __restrict__ codes = reinterpret_cast<const uint32_t*>(rec + BD_ROWS_HEADER_BYTES);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t w = codes[k * 64 + lane];
                    sum.add(kHeaderWords + k * 64 + lane, w);
                    dst[k * 64 + lane] = bad ? make_float4(nan, nan, nan, nan)
                                             : make_float4(value_b((uint8_t)(w & 0xFFu), e), value_b((uint8_t)((w >> 8) & 0xFFu), e),
                                                           value_b((uint8_t)((w >> 16) & 0xFFu), e), value_b((uint8_t)(w >> 24), e));
                }
            }
        }
    }
    flush_sums(sum, sums, first_row);
}

int64_t slices_of(int64_t windows) { return (windows + BD_ROWS_SLICE - 1) / BD_ROWS_SLICE; }

// what the device entry points and their host restatements refuse alike
int check_call(const std::string& fn, const void* rows, int64_t windows, int32_t codec, const void* records, const void* sums,
               int row_align, int record_align) {
    if (codec != BD_ROWS_F32 && codec != BD_ROWS_H && codec != BD_ROWS_B)
        return fail(BD_EINVAL, fn + "codec = " + std::to_string(codec) + ", allowed are 0 (f32), 1 (h), 2 (b)");
    if (windows < 0 || windows > BD_ROWS_MAX_WINDOWS)
        return fail(BD_EINVAL, fn + "windows = " + std::to_string(windows) + ", a call takes 0.." + std::to_string(BD_ROWS_MAX_WINDOWS));
    if (windows > 0 && (!rows || (uintptr_t)rows % row_align)) return fail(BD_EINVAL, fn + "rows is null or misaligned");
    if (windows > 0 && (!records || (uintptr_t)records % record_align)) return fail(BD_EINVAL, fn + "records is null or misaligned");
    if (windows > 0 && (!sums || (uintptr_t)sums % 8)) return fail(BD_EINVAL, fn + "sums is null or misaligned");
    return BD_OK;
}

// the slice sums of finished records on the host: the words in file order
void sums_host(const unsigned char* records, int64_t windows, int record, uint64_t* sums) {
    for (int64_t s = 0; s < slices_of(windows); ++s) {
        const int64_t first = s * BD_ROWS_SLICE;
        const int64_t n = windows - first < BD_ROWS_SLICE ? windows - first : BD_ROWS_SLICE;
        uint64_t s1 = 0, s2 = 0;
        const unsigned char* p = records + (size_t)first * record;
        for (int64_t i = 0; i < n * (record / 4); ++i) {
            uint32_t w;
            memcpy(&w, p + 4 * i, 4);
            s1 += w;
            s2 += (uint64_t)(i + 1) * w;
        }
        sums[2 * s] = s1;
        sums[2 * s + 1] = s2;
    }
}

}  // namespace
}  // namespace bd

extern "C" {

int bd_rows_abi_version(void) { return BD_ROWS_ABI_VERSION; }

int64_t bd_rows_record_bytes(int32_t codec) {
    if (codec != BD_ROWS_F32 && codec != BD_ROWS_H && codec != BD_ROWS_B)
        return bd::fail(BD_EINVAL, "bd_rows_record_bytes: codec = " + std::to_string(codec) + ", allowed are 0 (f32), 1 (h), 2 (b)");
    return bd::rowcodec::record_bytes(codec);
}

int bd_rows_encode(const float* rows_dev, int64_t windows, int32_t codec, void* records_dev, uint64_t* sums_dev,
                   uint32_t* flags_dev, void* stream) {
    const std::string fn = "bd_rows_encode: ";
    const int rc = bd::check_call(fn, rows_dev, windows, codec, records_dev, sums_dev, 16, 16);
    if (rc != BD_OK) return rc;
    if (!flags_dev || (uintptr_t)flags_dev % 4) return bd::fail(BD_EINVAL, fn + "flags is null or misaligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    BD_HIP(hipMemsetAsync(flags_dev, 0, sizeof(uint32_t), s));
    if (windows == 0) return BD_OK;
    BD_HIP(hipMemsetAsync(sums_dev, 0, (size_t)bd::slices_of(windows) * 2 * sizeof(uint64_t), s));
    const dim3 grid((unsigned)((windows + bd::kWaves - 1) / bd::kWaves)), block(64 * bd::kWaves);
    unsigned char* rec = static_cast<unsigned char*>(records_dev);
    bd::u64* sums = reinterpret_cast<bd::u64*>(sums_dev);
    if (codec == BD_ROWS_F32)
        hipLaunchKernelGGL(bd::rows_encode_kernel<BD_ROWS_F32>, grid, block, 0, s, rows_dev, (long long)windows, rec, sums, flags_dev);
    else if (codec == BD_ROWS_H)
        hipLaunchKernelGGL(bd::rows_encode_kernel<BD_ROWS_H>, grid, block, 0, s, rows_dev, (long long)windows, rec, sums, flags_dev);
    else
        hipLaunchKernelGGL(bd::rows_encode_kernel<BD_ROWS_B>, grid, block, 0, s, rows_dev, (long long)windows, rec, sums, flags_dev);
    return bd::hip_result(fn);
}

int bd_rows_decode(const void* records_dev, int64_t windows, int32_t codec, float* rows_dev, uint64_t* sums_dev, void* stream) {
    const std::string fn = "bd_rows_decode: ";
    const int rc = bd::check_call(fn, rows_dev, windows, codec, records_dev, sums_dev, 16, 16);
    if (rc != BD_OK) return rc;
    if (windows == 0) return BD_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    BD_HIP(hipMemsetAsync(sums_dev, 0, (size_t)bd::slices_of(windows) * 2 * sizeof(uint64_t), s));
    const dim3 grid((unsigned)((windows + bd::kWaves - 1) / bd::kWaves)), block(64 * bd::kWaves);
    const unsigned char* rec = static_cast<const unsigned char*>(records_dev);
    bd::u64* sums = reinterpret_cast<bd::u64*>(sums_dev);
    if (codec == BD_ROWS_F32)
        hipLaunchKernelGGL(bd::rows_decode_kernel<BD_ROWS_F32>, grid, block, 0, s, rec, (long long)windows, rows_dev, sums);
    else if (codec == BD_ROWS_H)
        hipLaunchKernelGGL(bd::rows_decode_kernel<BD_ROWS_H>, grid, block, 0, s, rec, (long long)windows, rows_dev, sums);
    else
        hipLaunchKernelGGL(bd::rows_decode_kernel<BD_ROWS_B>, grid, block, 0, s, rec, (long long)windows, rows_dev, sums);
    return bd::hip_result(fn);
}

int bd_rows_encode_host(const float* rows, int64_t windows, int32_t codec, void* records, uint64_t* sums, uint32_t* flags) {
    using namespace bd::rowcodec;
    const std::string fn = "bd_rows_encode_host: ";
    const int rc = bd::check_call(fn, rows, windows, codec, records, sums, 4, 1);
    if (rc != BD_OK) return rc;
    if (!flags) return bd::fail(BD_EINVAL, fn + "flags is null or misaligned");
    *flags = 0;
    const int record = record_bytes(codec);
    unsigned char* out = static_cast<unsigned char*>(records);
    for (int64_t r = 0; r < windows; ++r) {
        const float* x = rows + (size_t)r * kDim;
        unsigned char* rec = out + (size_t)r * record;
        float m = 0.0f;
        bool bad = false;
        for (int k = 0; k < kDim; ++k) {
            bad |= bad_element(x[k], codec);
            m = fmaxf(m, fabsf(x[k]));
        }
        if (bad) ++*flags;
        if (codec == BD_ROWS_F32) {
            memcpy(rec, x, (size_t)record);
            continue;
        }
        memset(rec, 0, (size_t)record);
        const int32_t e = bad ? kBadExponent : exponent(m, codec);
        memcpy(rec, &e, 4);
        if (bad) continue;
        for (int k = 0; k < kDim; ++k) {
            if (codec == BD_ROWS_H) {
                const uint16_t c = code_h(x[k], e);
                memcpy(rec + BD_ROWS_HEADER_BYTES + 2 * k, &c, 2);
            } else {
                rec[BD_ROWS_HEADER_BYTES + k] = code_b(x[k], e);
            }
        }
    }
    bd::sums_host(out, windows, record, sums);
    return BD_OK;
}

int bd_rows_decode_host(const void* records, int64_t windows, int32_t codec, float* rows, uint64_t* sums) {
    using namespace bd::rowcodec;
    const std::string fn = "bd_rows_decode_host: ";
    const int rc = bd::check_call(fn, rows, windows, codec, records, sums, 4, 1);
    if (rc != BD_OK) return rc;
    const int record = record_bytes(codec);
    const unsigned char* in = static_cast<const unsigned char*>(records);
    for (int64_t r = 0; r < windows; ++r) {
        const unsigned char* rec = in + (size_t)r * record;
        float* x = rows + (size_t)r * kDim;
        if (codec == BD_ROWS_F32) {
            memcpy(x, rec, (size_t)record);
            continue;
        }
        int32_t e;
        memcpy(&e, rec, 4);
        for (int k = 0; k < kDim; ++k) {
            if (e == kBadExponent) {
                const uint32_t nan = kQuietNaN;
                memcpy(&x[k], &nan, 4);
            } else if (codec == BD_ROWS_H) {
                uint16_t c;
                memcpy(&c, rec + BD_ROWS_HEADER_BYTES + 2 * k, 2);
                x[k] = value_h(c, e);
            } else {
                x[k] = value_b(rec[BD_ROWS_HEADER_BYTES + k], e);
            }
        }
    }
    bd::sums_host(in, windows, record, sums);
    return BD_OK;
}

}  // extern "C"
