// SNR mixing for gfx950 (include/buzzdetect_mix.h): annotated events overlaid on background stretches, every clip of a call
// by one pair of launches.
//
//   out[out_off + i] = ev_gain ev[ev_off + i] + b nz[nz_off + i],   b = ratio sqrt(Pe / Pn) ev_gain,
//
// Pe, Pn the mean squares of the clip's two sources.  b needs both sums before the first output, so a clip is walked twice:
//
//   mix_power_kernel   one workgroup per slice of BD_MIX_SLICE samples of one clip: 256 chains of fused multiply-adds over the
//                      slice, a butterfly per wave, the four waves as (w0 + w1) + (w2 + w3); the slice's two sums go to the
//                      workspace.
//   mix_apply_kernel   the same grid: the workgroup's first lane adds its clip's slice sums in ascending order, forms b, and the
//                      workgroup writes its slice of the mixture (the clip's first slice also writes (Pe, Pn) and the flags).
//
// The job is memory-bound: two sources read, one output written.  The second pass re-reads what the first pass read a few
// microseconds earlier; a call of 64 clips of ten windows reads 79 MB of sources, which stays in the 256 MiB Infinity Cache
// between the passes, so HBM delivers each source once.  (Holding a clip in LDS for both passes was the alternative; it caps
// the clip at ~19 000 samples per workgroup of a 160 KiB CU and leaves one workgroup per clip, 64 of 256 CUs busy.)
//
// Offsets and lengths are arbitrary, so loads and stores are one dword per lane, consecutive lanes on consecutive samples.  The
// order of every addition is fixed by (n, i) alone: the slice is a constant, the chains and trees are spelled out, nothing is
// added atomically.  Each step is one correctly rounded float32 operation (__fmaf_rn, __fmul_rn, __fadd_rn, __fdiv_rn, sqrtf)
// here and fmaf / sqrtf / IEEE arithmetic in bd_mix_host, which walks the same chains in the same order.  The root is sqrtf, not
// __fsqrt_rn: this toolchain's __fsqrt_rn is the native approximate root (__clang_hip_math.h without
// OCML_BASIC_ROUNDED_OPERATIONS), one unit off for some arguments, while sqrtf is correctly rounded under hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt.  Contraction is switched off for the whole file, so that no product spelled `*`
// (which is all __fmul_rn is in that header) can fuse with an addition on one side and not on the other.
#include "bd_internal.h"
#include "bd_error.h"

#include "../../include/buzzdetect_mix.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#pragma clang fp contract(off)

namespace bd {
namespace {

constexpr int kMixThreads = 256;
constexpr int kMixWaves = kMixThreads / 64;
static_assert(BD_MIX_SLICE % kMixThreads == 0, "a slice is whole rounds of the chains");

// a clip as the kernels see it: the caller's descriptor and the index of its first slice among the call's slices
struct MixItem {
    long long ev_off, nz_off, out_off;
    int n;
    float ev_gain, ratio;
    int slice0;
};

__host__ __device__ __forceinline__ int mix_slices(int n) { return (n + BD_MIX_SLICE - 1) / BD_MIX_SLICE; }

// the clip that owns slice `s` of the call: the last item whose slice0 <= s
__device__ __forceinline__ int mix_find(const MixItem* __restrict__ items, int n_clips, int s) {
    int lo = 0, hi = n_clips - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].slice0 <= s) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ float mix_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = __fadd_rn(v, __shfl_xor(v, m, 64));
    return v;
}

__global__ __launch_bounds__(kMixThreads) void mix_power_kernel(const float* __restrict__ ev, const float* __restrict__ nz,
                                                                const MixItem* __restrict__ items, int n_clips,
                                                                float2* __restrict__ partial) {
    __shared__ float s_w[2][kMixWaves];
    const int tid = threadIdx.x;
    const MixItem it = items[mix_find(items, n_clips, (int)blockIdx.x)];
    const int i0 = ((int)blockIdx.x - it.slice0) * BD_MIX_SLICE;
    const int len = it.n - i0 < BD_MIX_SLICE ? it.n - i0 : BD_MIX_SLICE;
    const float* __restrict__ e = ev + it.ev_off + i0;
    const float* __restrict__ z = nz + it.nz_off + i0;
    float ae = 0.0f, az = 0.0f;
#pragma unroll 4
    for (int i = tid; i < len; i += kMixThreads) {
        const float x = e[i], y = z[i];
        ae = __fmaf_rn(x, x, ae);
        az = __fmaf_rn(y, y, az);
    }
    ae = mix_wave_sum(ae);
    az = mix_wave_sum(az);
    if ((tid & 63) == 0) {
        s_w[0][tid >> 6] = ae;
        s_w[1][tid >> 6] = az;
    }
    __syncthreads();
    if (tid == 0)
        partial[blockIdx.x] = make_float2(__fadd_rn(__fadd_rn(s_w[0][0], s_w[0][1]), __fadd_rn(s_w[0][2], s_w[0][3])),
                                          __fadd_rn(__fadd_rn(s_w[1][0], s_w[1][1]), __fadd_rn(s_w[1][2], s_w[1][3])));
}

__global__ __launch_bounds__(kMixThreads) void mix_apply_kernel(const float* __restrict__ ev, const float* __restrict__ nz,
                                                                const MixItem* __restrict__ items, int n_clips,
                                                                const float2* __restrict__ partial, float* __restrict__ out,
                                                                float* __restrict__ power, unsigned* __restrict__ flags) {
    __shared__ float s_b;
    const int tid = threadIdx.x;
    const int c = mix_find(items, n_clips, (int)blockIdx.x);
    const MixItem it = items[c];
    const int slice = (int)blockIdx.x - it.slice0;
    if (tid == 0) {
        float se = 0.0f, sn = 0.0f;
        const int ns = mix_slices(it.n);
        for (int k = 0; k < ns; ++k) {
            const float2 p = partial[it.slice0 + k];
            se = __fadd_rn(se, p.x);
            sn = __fadd_rn(sn, p.y);
        }
        const float nf = (float)it.n;
        const float pe = __fdiv_rn(se, nf), pn = __fdiv_rn(sn, nf);
        const bool silent = pn < BD_MIX_POWER_FLOOR;
        float b = 0.0f;
        if (!silent && it.ratio != 0.0f && pe != 0.0f)
            b = __fmul_rn(__fmul_rn(it.ratio, sqrtf(__fdiv_rn(pe, pn))), it.ev_gain);
        s_b = b;
        if (slice == 0) {
            power[2 * c] = pe;
            power[2 * c + 1] = pn;
            flags[c] = silent ? BD_MIX_FLAG_SILENT_BACKGROUND : 0u;
        }
    }
    __syncthreads();
    const float b = s_b, g = it.ev_gain;
    const int i0 = slice * BD_MIX_SLICE;
    const int len = it.n - i0 < BD_MIX_SLICE ? it.n - i0 : BD_MIX_SLICE;
    const float* __restrict__ e = ev + it.ev_off + i0;
    const float* __restrict__ z = nz + it.nz_off + i0;
    float* __restrict__ o = out + it.out_off + i0;
#pragma unroll 4
    for (int i = tid; i < len; i += kMixThreads) o[i] = __fmaf_rn(b, z[i], __fmul_rn(g, e[i]));
}

// Every descriptor against the three lengths; on success the kernels' items and the call's slice count.
int mix_check(const char* who, const bd_mix_clip* clips, int32_t n_clips, int64_t ev_len, int64_t nz_len, int64_t out_len,
              bool lengths, std::vector<MixItem>* items, int64_t* slices) {
    if (n_clips < 0 || n_clips > BD_MIX_MAX_CLIPS || (!clips && n_clips) || (lengths && (ev_len < 0 || nz_len < 0 || out_len < 0))) {
        set_error(std::string(who) + ": bad argument (0.." + std::to_string(BD_MIX_MAX_CLIPS) + " clips, lengths >= 0)");
        return BD_EINVAL;
    }
    items->resize((size_t)n_clips);
    int64_t total = 0;
    for (int32_t j = 0; j < n_clips; ++j) {
        const bd_mix_clip& c = clips[j];
        const char* why = nullptr;
        if (c.n < 1) why = "n < 1";
        else if (c.ev_off < 0 || c.nz_off < 0 || c.out_off < 0) why = "negative offset";
        else if (!std::isfinite(c.ev_gain) || !std::isfinite(c.ratio) || c.ratio < 0.0f) why = "ev_gain and ratio must be finite, ratio >= 0";
        else if (lengths && c.ev_off > ev_len - c.n) why = "event range past the end of the event buffer";
        else if (lengths && c.nz_off > nz_len - c.n) why = "background range past the end of the background buffer";
        else if (lengths && c.out_off > out_len - c.n) why = "output range past the end of the output buffer";
        if (why) {
            set_error(std::string(who) + ": clip " + std::to_string(j) + ": " + why);
            return BD_EINVAL;
        }
        if (total > INT32_MAX - (int64_t)mix_slices(c.n)) {
            set_error(std::string(who) + ": the call has 2^31 slices or more; split it");
            return BD_EINVAL;
        }
        (*items)[j] = MixItem{c.ev_off, c.nz_off, c.out_off, c.n, c.ev_gain, c.ratio, (int)total};
        total += mix_slices(c.n);
    }
    if (lengths && n_clips > 1) {                 // two clips writing the same samples would race
        std::vector<int32_t> order((size_t)n_clips);
        for (int32_t j = 0; j < n_clips; ++j) order[j] = j;
        std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return clips[a].out_off < clips[b].out_off; });
        for (int32_t k = 1; k < n_clips; ++k) {
            const bd_mix_clip &p = clips[order[k - 1]], &q = clips[order[k]];
            if (p.out_off + p.n > q.out_off) {
                set_error(std::string(who) + ": clip " + std::to_string(order[k]) + ": output range overlaps clip " +
                          std::to_string(order[k - 1]) + "'s");
                return BD_EINVAL;
            }
        }
    }
    *slices = total;
    return BD_OK;
}

int64_t mix_items_bytes(int32_t n_clips) { return ((int64_t)n_clips * (int64_t)sizeof(MixItem) + 255) / 256 * 256; }

// mix_power_kernel's slice sum on the host: the same chains, butterflies and tree
void mix_slice_host(const float* x, int len, float* sum) {
    float v[kMixThreads];
    for (int t = 0; t < kMixThreads; ++t) {
        float a = 0.0f;
        for (int i = t; i < len; i += kMixThreads) a = fmaf(x[i], x[i], a);
        v[t] = a;
    }
    float w[kMixWaves];
    for (int g = 0; g < kMixWaves; ++g) {
        float* l = v + 64 * g;
        for (int m = 32; m >= 1; m >>= 1) {
            float t[64];
            for (int lane = 0; lane < 64; ++lane) t[lane] = l[lane] + l[lane ^ m];
            for (int lane = 0; lane < 64; ++lane) l[lane] = t[lane];
        }
        w[g] = l[0];
    }
    *sum = (w[0] + w[1]) + (w[2] + w[3]);
}

}  // namespace

}  // namespace bd

extern "C" {

int bd_mix_abi_version(void) { return BD_MIX_ABI_VERSION; }

int64_t bd_mix_workspace_bytes(const bd_mix_clip* clips, int32_t n_clips) {
    std::vector<bd::MixItem> items;
    int64_t slices = 0;
    const int rc = bd::mix_check("bd_mix_workspace_bytes", clips, n_clips, 0, 0, 0, false, &items, &slices);
    if (rc != BD_OK) return rc;
    const int64_t bytes = bd::mix_items_bytes(n_clips) + slices * (int64_t)sizeof(float2);
    return bytes < 256 ? 256 : bytes;
}

int bd_mix(const float* ev_dev, int64_t ev_len, const float* nz_dev, int64_t nz_len, const bd_mix_clip* clips, int32_t n_clips,
           float* out_dev, int64_t out_len, float* power_dev, uint32_t* flags_dev, void* workspace, int64_t workspace_bytes,
           void* stream) {
    // (thread-local: the table outlives the call, whatever the runtime does with a copy from pageable memory)
    static thread_local std::vector<bd::MixItem> items;
    int64_t slices = 0;
    const int rc = bd::mix_check("bd_mix", clips, n_clips, ev_len, nz_len, out_len, true, &items, &slices);
    if (rc != BD_OK) return rc;
    if (n_clips == 0) return BD_OK;
    if (!ev_dev || !nz_dev || !out_dev || !power_dev || !flags_dev || ((uintptr_t)ev_dev | (uintptr_t)nz_dev | (uintptr_t)out_dev |
                                                                        (uintptr_t)power_dev | (uintptr_t)flags_dev) % 4) {
        bd::set_error("bd_mix: null or misaligned buffer");
        return BD_EINVAL;
    }
    const int64_t items_bytes = bd::mix_items_bytes(n_clips);
    const int64_t need = items_bytes + slices * (int64_t)sizeof(float2);
    if (!workspace || workspace_bytes < need || (uintptr_t)workspace % 16) {
        bd::set_error("bd_mix: needs a 16-byte aligned workspace of " + std::to_string(need) + " bytes (bd_mix_workspace_bytes)");
        return BD_EWORKSPACE;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    bd::MixItem* d_items = static_cast<bd::MixItem*>(workspace);
    float2* d_partial = reinterpret_cast<float2*>(static_cast<char*>(workspace) + items_bytes);
    hipError_t e = hipMemcpyAsync(d_items, items.data(), (size_t)n_clips * sizeof(bd::MixItem), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(bd::mix_power_kernel, dim3((unsigned)slices), dim3(bd::kMixThreads), 0, st, ev_dev, nz_dev, d_items,
                           (int)n_clips, d_partial);
        hipLaunchKernelGGL(bd::mix_apply_kernel, dim3((unsigned)slices), dim3(bd::kMixThreads), 0, st, ev_dev, nz_dev, d_items,
                           (int)n_clips, d_partial, out_dev, power_dev, flags_dev);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        bd::set_error(std::string("bd_mix: ") + hipGetErrorString(e));
        return BD_EHIP;
    }
    return BD_OK;
}

int bd_mix_host(const float* ev, int64_t ev_len, const float* nz, int64_t nz_len, const bd_mix_clip* clips, int32_t n_clips,
                float* out, int64_t out_len, float* power, uint32_t* flags) {
    std::vector<bd::MixItem> items;
    int64_t slices = 0;
    const int rc = bd::mix_check("bd_mix_host", clips, n_clips, ev_len, nz_len, out_len, true, &items, &slices);
    if (rc != BD_OK) return rc;
    if (n_clips == 0) return BD_OK;
    if (!ev || !nz || !out || !power || !flags) {
        bd::set_error("bd_mix_host: null buffer");
        return BD_EINVAL;
    }
    for (int32_t j = 0; j < n_clips; ++j) {
        const bd::MixItem& it = items[j];
        const float* e = ev + it.ev_off;
        const float* z = nz + it.nz_off;
        float se = 0.0f, sn = 0.0f;
        for (int i0 = 0; i0 < it.n; i0 += BD_MIX_SLICE) {
            const int len = it.n - i0 < BD_MIX_SLICE ? it.n - i0 : BD_MIX_SLICE;
            float pe, pn;
            bd::mix_slice_host(e + i0, len, &pe);
            bd::mix_slice_host(z + i0, len, &pn);
            se = se + pe;
            sn = sn + pn;
        }
        const float nf = (float)it.n;
        const float pe = se / nf, pn = sn / nf;
        const bool silent = pn < BD_MIX_POWER_FLOOR;
        float b = 0.0f;
        if (!silent && it.ratio != 0.0f && pe != 0.0f) {
            const float q = pe / pn;
            const float r = it.ratio * sqrtf(q);
            b = r * it.ev_gain;
        }
        power[2 * j] = pe;
        power[2 * j + 1] = pn;
        flags[j] = silent ? BD_MIX_FLAG_SILENT_BACKGROUND : 0u;
        float* o = out + it.out_off;
        for (int i = 0; i < it.n; ++i) {
            const float a = it.ev_gain * e[i];
            o[i] = fmaf(b, z[i], a);
        }
    }
    return BD_OK;
}

}  // extern "C"
