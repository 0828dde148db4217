// What the kernel files share: vector types, the f16 range guard, the split into f16 halves, the LDS swizzle, counted LDS
// operations, the XCD-aware tile order, and the two host helpers every launcher with dynamic LDS needs.  Included by the kernel
// .hip files (never by engine.hip); every file is its own translation unit, so everything sits in an anonymous namespace.
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
