// What the kernel files share: vector types, the f16 range guard, the split into f16 halves, the LDS swizzle, counted LDS
// operations, the XCD-aware tile order, and the two host helpers every launcher with dynamic LDS needs.  Included by the kernel
// .hip files (never by the host files: engine.hip and the files engine_state.h lists); every file is its own translation unit, so everything sits in an anonymous namespace.
#pragma once

#include "bd_internal.h"

#include <mutex>
#include <type_traits>
#ifdef BD_KERNEL_TRACE
#include <cstdio>
#include <cstdlib>
#endif

namespace bd {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// Range guard of the f16 arithmetic modes.  Every activation is split as hi = f16(a), lo = f16(a - hi): beyond the f16
// range (65 504) hi is +inf and the result is garbage that the following ReLU can even hide (max(NaN, 0) = 0).  The
// kernels keep a running max |a| of what they convert (two v_max3 per four values) and raise the engine's sticky flag
// when it is out of range; the host reads the flag with the results and repeats the chunk in exact-f32 mode.
constexpr float kF16Max = 65504.0f;
__device__ __forceinline__ float range_of(float m, float4 v) {
    return fmaxf(fmaxf(m, fabsf(v.x)), fmaxf(fmaxf(fabsf(v.y), fabsf(v.z)), fabsf(v.w)));
}
__device__ __forceinline__ float range_of(float m, v4f v) {
    return fmaxf(fmaxf(m, fabsf(v.x)), fmaxf(fmaxf(fabsf(v.y), fabsf(v.z)), fabsf(v.w)));
}
__device__ __forceinline__ void range_report(float m, unsigned* __restrict__ flag) {
    if (flag && !(m <= kF16Max)) *flag = 1u;  // also true for NaN (flag == nullptr: the handle-less debug entry points)
}

// Split-f16 LDS tiles are [rows][32 f16] = 64-byte rows with no padding; the 16-byte slot index is XORed with
// (row >> 2) & 3 so that the 16 rows a ds_read_b128 lane group touches land on 16 different slots of
// the 256-byte bank row.
__device__ __forceinline__ int swz64(int row, int slot) { return row * 64 + ((slot ^ ((row >> 2) & 3)) << 4); }

// a = hi + lo with hi = f16(a) and lo = f16(a - hi), four values at a time.  The difference and its rounding are ONE
// v_fma_mixlo/mixhi_f16 per value (fma(hi as f16, -1, a as f32), rounded to f16 into one half of the result): six
// instructions per four values where the convert / subtract / convert form took eleven.  a - hi is exact in f32, so the
// bits are those of (_Float16)(a - (float)hi).
__device__ __forceinline__ void split_f16(float x, float y, float z, float w, f16x4& hi, f16x4& lo) {
    const f16x2 h0 = {(_Float16)x, (_Float16)y}, h1 = {(_Float16)z, (_Float16)w};
    f16x2 l0, l1;
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(l0) : "v"(h0), "v"(x));
    asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(l0) : "v"(h0), "v"(y));
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(l1) : "v"(h1), "v"(z));
    asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(l1) : "v"(h1), "v"(w));
    hi[0] = h0[0]; hi[1] = h0[1]; hi[2] = h1[0]; hi[3] = h1[1];
    lo[0] = l0[0]; lo[1] = l0[1]; lo[2] = l1[0]; lo[3] = l1[1];
}
__device__ __forceinline__ void split_f16(v4f a, f16x4& hi, f16x4& lo) { split_f16(a.x, a.y, a.z, a.w, hi, lo); }

// Channel-major hand-off image (round 10): a stage tile a layer publishes from its ACCUMULATORS (lane = channel, registers =
// positions) and the next product reads as its A operand (lane = position).  Two halves (hi, lo) of [32 k][96 positions] f16:
// a k-row is 192 bytes = 24 chunks of 8 bytes (four consecutive tile rows), no padding, and chunk t of k-row c sits at chunk
// t ^ ((c >> 1) & 7) of its row (the key touches the low three bits only: a chunk stays in its group of eight).  A lane writes
// four of its own positions per ds_write_b64; the reader takes it back transposed with ds_read_b64_tr_b16 - lane 4 q + p of a
// 16-lane group gives the address of k-row q of the block, positions 4 p .. 4 p + 3, and receives position (lane & 15) of the
// four k-rows.  Why neither side meets a bank twice (checked below for every lane group):
//   write  16 contiguous lanes = k-rows 16 a .. + 15 at one chunk t, bank (byte / 4) % 32.  A row is 48 dwords: odd rows start
//          16 banks further, and the key gives the eight row pairs eight different chunks of the 16-dword group: 32 banks.
//   read   a 32-lane half = 4 k-rows x 8 chunks (one group of eight), bank (byte / 4) % 64.  The four rows start at banks 0,
//          48, 32, 16 and each covers the 16 dwords of its group: 64 banks.
constexpr int kTrRowBytes = 192, kTrHalfBytes = 32 * kTrRowBytes, kTrSlotBytes = 2 * kTrHalfBytes;
__host__ __device__ constexpr int tr_image_off(int half, int k, int chunk) {
    return half * kTrHalfBytes + k * kTrRowBytes + ((chunk ^ ((k >> 1) & 7)) << 3);
}
// the reader's k-row and chunk: 16-lane group g = 2 h + gp (h: the k half of the MFMA lane, gp: rows 0-15 / 16-31 of the row
// tile), lane 4 q + p of it, sub-read r (elements 0-3 / 4-7 of the fragment), k16 step s of the stage, row tile i
__host__ __device__ constexpr int tr_read_k(int s, int h, int r, int q) { return 16 * s + 8 * h + 4 * r + q; }
__host__ __device__ constexpr int tr_read_chunk(int i, int gp, int p) { return 8 * i + 4 * gp + p; }
constexpr bool tr_image_is_bijection() {
    bool seen[kTrSlotBytes / 8] = {};
    for (int half = 0; half < 2; ++half)
        for (int k = 0; k < 32; ++k)
            for (int t = 0; t < 24; ++t) {
                const int o = tr_image_off(half, k, t);
                if (o < 0 || o >= kTrSlotBytes || o % 8 || seen[o / 8]) return false;
                seen[o / 8] = true;
            }
    return true;
}
constexpr bool tr_image_writes_conflict_free() {       // ds_write_b64: 16 contiguous lanes, two dwords each, 32 banks
    for (int half = 0; half < 2; ++half)
        for (int a = 0; a < 2; ++a)
            for (int t = 0; t < 24; ++t) {
                unsigned banks = 0;
                for (int l = 0; l < 16; ++l)
                    for (int d = 0; d < 2; ++d) {
                        const unsigned b = 1u << ((tr_image_off(half, 16 * a + l, t) / 4 + d) % 32);
                        if (banks & b) return false;
                        banks |= b;
                    }
            }
    return true;
}
constexpr bool tr_image_reads_conflict_free() {        // ds_read_b64_tr_b16: 32-lane halves, two dwords each, 64 banks
    for (int half = 0; half < 2; ++half)
        for (int i = 0; i < 3; ++i)
            for (int s = 0; s < 2; ++s)
                for (int h = 0; h < 2; ++h)
                    for (int r = 0; r < 2; ++r) {
                        unsigned long long banks = 0;
                        for (int gp = 0; gp < 2; ++gp)
                            for (int q = 0; q < 4; ++q)
                                for (int p = 0; p < 4; ++p)
                                    for (int d = 0; d < 2; ++d) {
                                        const unsigned long long b =
                                            1ull << ((tr_image_off(half, tr_read_k(s, h, r, q), tr_read_chunk(i, gp, p)) / 4 + d) % 64);
                                        if (banks & b) return false;
                                        banks |= b;
                                    }
                    }
    return true;
}
static_assert(tr_image_is_bijection(), "every (half, k, chunk) has its own 8 bytes of the slot, and they fill it");
static_assert(tr_image_writes_conflict_free(), "a lane group of the publication meets no bank twice");
static_assert(tr_image_reads_conflict_free(), "a lane half of the transposed read meets no bank twice");
// Per-lane byte offset of sub-read r = 0 of (k16 step 0, row tile 0) in a half; sub-read 1 is tr_read_next() of it, k16 step 1
// + 16 k-rows and row tile i + 64 i bytes (immediates).  k-row 8 h + 4 r + q has key (4 h + 2 r + (q >> 1)) & 7 whatever the
// k16 step, so r = 1 is four rows further with bit 1 of the key = bit 4 of the byte offset flipped (rows are multiples of 64).
__device__ __forceinline__ int tr_read_lane_off(int lane) {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    return tr_image_off(0, tr_read_k(0, g >> 1, 0, q), tr_read_chunk(0, g & 1, p));
}
__host__ __device__ constexpr int tr_read_next(int off) { return (off ^ 16) + 4 * kTrRowBytes; }
constexpr bool tr_read_next_holds() {
    for (int lane = 0; lane < 64; ++lane) {
        const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
        if (tr_read_next(tr_image_off(0, tr_read_k(0, g >> 1, 0, q), tr_read_chunk(0, g & 1, p))) !=
            tr_image_off(0, tr_read_k(0, g >> 1, 1, q), tr_read_chunk(0, g & 1, p)))
            return false;
        for (int s = 0; s < 2; ++s)
            for (int i = 0; i < 3; ++i)
                for (int r = 0; r < 2; ++r)
                    if (tr_image_off(0, tr_read_k(s, g >> 1, r, q), tr_read_chunk(i, g & 1, p)) !=
                        tr_image_off(0, tr_read_k(0, g >> 1, r, q), tr_read_chunk(0, g & 1, p)) + 16 * s * kTrRowBytes + 64 * i)
                        return false;
    }
    return true;
}
static_assert(tr_read_next_holds(), "the reader's immediates");
// one A fragment (8 k of a lane's row) of the channel-major image: elements 0-3 from `p0`, 4-7 from `p1`.  EXEC must be all ones.
__device__ __forceinline__ f16x8 tr_read_frag(const char* p0, const char* p1) {
    typedef short s16x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) s16x4* lds4;
    const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)p0), b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)p1);
    return __builtin_bit_cast(f16x8, __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}

// LDS operations the compiler must not reorder or wait for on its own: pw_res_kernel and l4_window_kernel count them (lgkmcnt).
__device__ __forceinline__ unsigned pw_lds_addr(const void* p) {
    return (unsigned)(unsigned long long)(__attribute__((address_space(3))) const void*)p;
}
template <int OFFSET>
__device__ __forceinline__ f16x8 pw_lds_frag(unsigned addr) {
    f16x8 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFFSET) : "memory");
    return v;
}
__device__ __forceinline__ void pw_lds_store64(unsigned addr, f16x4 v) {
    asm volatile("ds_write_b64 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
__device__ __forceinline__ f16x8 pw_landed(f16x8 v) {       // after the wait that covers the read: later uses stay behind it
    asm volatile("" : "+v"(v));
    return v;
}
template <int N>
__device__ __forceinline__ void pw_lds_wait() {
    asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
}
template <int I, int E, typename F>
__device__ __forceinline__ void static_for_pw(F&& f) {
    if constexpr (I < E) {
        f(std::integral_constant<int, I>{});
        static_for_pw<I + 1, E>(f);
    }
}
// Issue order of a tile's LDS operations in pw_res_kernel (and of l4_window_kernel's matrix waves, with V = 0): fragments of
// steps 0 and 1 (R reads each: hi, lo), then per step q the fragments of step q + 2 and, at V evenly spaced steps, the R stores
// of one split item; pending(q) is how many of them may still be in flight when the fragments of step q are needed.
template <int K16, int V, int R>
struct PwResSchedule {
    static constexpr int split_at(int q) {                      // item index whose stores follow the reads of step q, or -1
        for (int j = 0; j < V; ++j)
            if (q == j * K16 / (V > 0 ? V : 1) + 1) return j;
        return -1;
    }
    static constexpr int issued_at_step(int u) { return (u + 2 < K16 ? R : 0) + (split_at(u) >= 0 ? R : 0); }
    static constexpr int pending(int q) {
        int upto_wait = 2 * R;
        for (int u = 0; u <= q; ++u) upto_wait += issued_at_step(u);
        int through_read = q < 2 ? R * (q + 1) : 2 * R;
        if (q >= 2) {
            for (int u = 0; u < q - 2; ++u) through_read += issued_at_step(u);
            through_read += R;
        }
        return upto_wait - through_read;
    }
};

// hipFuncSetAttribute(max dynamic LDS) once per kernel instantiation and device; safe when several analyzer threads
// (one engine each, src/inference/worker.py:21) make their first launch at the same time.
constexpr int kMaxDevices = 64;
template <auto Kernel>
void allow_dynamic_lds(int bytes) {
    static std::once_flag once[kMaxDevices];
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::call_once(once[dev & (kMaxDevices - 1)], [&] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    });
}

#ifdef BD_KERNEL_TRACE
// Developer builds only: the launch of a kernel's TRACE instantiation when BD_WS_TRACE begins with `key`.  launch(stamps)
// enqueues it on `stream` with a zeroed buffer of kTraceStamps shader-clock stamps (the kernel's own form of it, `kernel`, is
// allowed `lds_bytes` of dynamic LDS first); the call waits for it, and the 8th call of a launch site prints, for the two stamp
// groups [0, per_group) and [per_group, 2 per_group), the cycles between consecutive stamps behind `legend` - a printf format
// whose first %d is the group's wave or workgroup (0 / id1), followed by args.  Returns a pointer to the stamps on the host
// (null: not selected, the caller launches as usual); *printed says whether this call was the one that printed.
constexpr int kTraceStamps = 128;
template <typename Kernel, typename Launch, typename... Args>
const unsigned long long* traced_launch(char key, Kernel kernel, int lds_bytes, hipStream_t stream, int per_group, int id1,
                                        bool* printed, Launch&& launch, const char* legend, Args... args) {
    const char* tr = getenv("BD_WS_TRACE");
    if (!tr || tr[0] != key) return nullptr;
    static unsigned long long* dbg = nullptr;
    static unsigned long long h[kTraceStamps];
    static int shots = 0;
    if (!dbg) (void)hipMalloc(&dbg, sizeof(h));
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    (void)hipMemsetAsync(dbg, 0, sizeof(h), stream);
    launch(dbg);
    (void)hipStreamSynchronize(stream);
    (void)hipMemcpy(h, dbg, sizeof(h), hipMemcpyDeviceToHost);
    const bool print = ++shots == 8;
    if (printed) *printed = print;
    if (print)
        for (int w = 0; w < 2; ++w) {
            fprintf(stderr, "[trace] ");
            fprintf(stderr, legend, w ? id1 : 0, args...);
            for (int i = 1; i < per_group && h[w * per_group + i]; ++i) fprintf(stderr, " %llu", h[w * per_group + i] - h[w * per_group + i - 1]);
            fprintf(stderr, "\n");
        }
    return h;
}
#endif

}  // namespace

}  // namespace bd
