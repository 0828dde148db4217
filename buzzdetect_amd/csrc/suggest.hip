// What to annotate next, for gfx950 (include/buzzdetect_suggest.h): an acquisition score per window from the members' logits
// where a set of heads left them, and the greedy choice of a diverse batch from a pool of candidates.
//
//   suggest_acquire_kernel   a wave per window, four windows a workgroup.  Lane c < C holds class c; the members are walked in a
//                            loop, their offsets in the wide row come by value in the kernel's arguments.  A row's maximum and
//                            sums are xor butterflies over the wave, so every lane ends with the same values and lane 0 stores
//                            the window's three scores (suggest_device.h: the text bd_suggest_acquire_host calls too).  With a
//                            target the wave still spans the classes for the softmax's sums; under sigmoid every lane reads the
//                            one column.  No barrier, no LDS.
//   suggest_pick_kernel      ONE workgroup of 1024 threads, thread i owns candidate i: its distance, its gain and whether it is
//                            chosen live in registers.  A step: key (gain * d, i) - 0 for a chosen or absent candidate, which no
//                            real key is - a butterfly maximum of the 64-bit keys per wave, sixteen wave maxima in LDS, one
//                            barrier, every thread takes the maximum of the sixteen; the winner's thread stores the step's three
//                            outputs, and every thread reads its element of the winner's row of sim: one coalesced row.  Step
//                            t writes slot t & 1 of LDS: a wave that is early for step t + 1 writes the other slot, and cannot
//                            be two steps early, because the barrier of step t + 1 needs the wave that still reads slot t & 1.
//
// Nothing is added atomically, nothing depends on the grid, every output element has one writer, inputs are only read: both
// launches are idempotent, and a window's scores do not depend on where it sits in the call.
#include "bd_internal.h"
#include "bd_error.h"
#include "suggest_device.h"

#include "../../include/buzzdetect_suggest.h"

#include <string>
#include <vector>

#pragma clang fp contract(off)

namespace bd {
namespace {

constexpr int kAcquireThreads = 256;
constexpr int kPickThreads = BD_SUGGEST_MAX_POOL;
constexpr int kPickWaves = kPickThreads / 64;
static_assert(BD_SUGGEST_MAX_WIDTH == 64, "a lane per class");
static_assert(BD_SUGGEST_MAX_POOL == BD_SEARCH_MAX_K && kPickThreads <= 1024, "a thread per candidate of the selector's state");

struct Members {
    int first[BD_SUGGEST_MAX_MEMBERS];       // 256 bytes of kernel arguments
};

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m, 64));
    return v;
}

__global__ __launch_bounds__(kAcquireThreads) void suggest_acquire_kernel(const float* __restrict__ wide, int ld_wide, int W,
                                                                          Members first, int M, int C, int link, int target,
                                                                          float r_members, float L, float* __restrict__ out,
                                                                          long long out_stride) {
    const int lane = threadIdx.x & 63;
    const int row = 4 * blockIdx.x + (threadIdx.x >> 6);
    if (row >= W) return;                                 // (no barrier in this kernel)
    const float* __restrict__ z0 = wide + (size_t)row * ld_wide;
    const bool active = lane < C;
    float a, b, gap;
    if (target < 0) {
        float pbar = 0.0f, hs = 0.0f;                     // this lane's class: sum_m p_m[c] and sum_m p_m[c] log p_m[c]
        for (int m = 0; m < M; ++m) {
            const float z = active ? z0[first.first[m] + lane] : -INFINITY;
            const float mx = wave_max(z);
            const float d = z - mx;
            const float e = active ? expf(d) : 0.0f;
            const float s = wave_sum(e);
            const float p = e / s;
            pbar += p;
            hs += suggest::term(p, d - logf(s));
        }
        pbar *= r_members;
        a = wave_sum(active ? suggest::xlogx(pbar) : 0.0f);
        b = wave_sum(active ? hs : 0.0f);
        const float top = wave_max(active ? pbar : -1.0f);
        const int at = wave_min(active && pbar == top ? lane : 64);           // the first class that holds the maximum
        gap = top - wave_max(active && lane != at ? pbar : -1.0f);
    } else {
        float qs = 0.0f, rs = 0.0f, hs = 0.0f;            // (the same in every lane)
        for (int m = 0; m < M; ++m) {
            suggest::Binary v;
            if (link == BD_LINK_SIGMOID) {
                v = suggest::binary_sigmoid(z0[first.first[m] + target]);
            } else {
                const float z = active ? z0[first.first[m] + lane] : -INFINITY;
                const float mx = wave_max(z);
                const float d = z - mx;
                const float e = active ? expf(d) : 0.0f;
                const float s = wave_sum(e);
                const float s_other = wave_sum(lane == target ? 0.0f : e);
                v = suggest::binary_softmax(__shfl(d, target, 64), __shfl(e, target, 64), s, s_other, logf(s));
            }
            qs += v.q;
            rs += v.r;
            hs += suggest::term(v.q, v.logq) + suggest::term(v.r, v.logr);
        }
        const float qbar = qs * r_members, rbar = rs * r_members;
        a = suggest::xlogx(qbar) + suggest::xlogx(rbar);
        b = hs;
        gap = fabsf(2.0f * qbar - 1.0f);
    }
    float entropy, margin, bald;
    suggest::scores(a, b, gap, M, r_members, L, &entropy, &margin, &bald);
    if (lane == 0) {
        out[(long long)BD_SUGGEST_ENTROPY * out_stride + row] = entropy;
        out[(long long)BD_SUGGEST_MARGIN * out_stride + row] = margin;
        out[(long long)BD_SUGGEST_BALD * out_stride + row] = bald;
    }
}

__global__ __launch_bounds__(kPickThreads) void suggest_pick_kernel(const float* __restrict__ sim, long long ld,
                                                                    const float* __restrict__ gain, const float* __restrict__ d0,
                                                                    int n, int k, int* __restrict__ picked, float* __restrict__ value,
                                                                    float* __restrict__ dist) {
    __shared__ uint64_t s_best[2][kPickWaves];
    const int i = threadIdx.x;
    const int lane = i & 63;
    const int wave = i >> 6;
    const bool live = i < n;
    const float my_gain = live ? gain[i] : 0.0f;
    float d = live ? (d0 ? d0[i] : 1.0f) : 0.0f;
    bool chosen = false;
    for (int t = 0; t < k; ++t) {                         // (k is uniform: every thread meets every barrier)
        const float g = suggest::discounted(my_gain, d);
        uint64_t best = live && !chosen ? search::make_key(g, (uint32_t)i) : 0;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const uint64_t other = __shfl_xor((unsigned long long)best, m, 64);
            best = other > best ? other : best;
        }
        if (lane == 0) s_best[t & 1][wave] = best;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kPickWaves; ++w) {
            const uint64_t other = s_best[t & 1][w];
            best = other > best ? other : best;
        }
        const int won = (int)search::key_id(best);        // k <= n: someone is not chosen yet, so best is a real key and won < n
        if (i == won) {
            chosen = true;
            picked[t] = won;
            value[t] = g;
            dist[t] = d;
        }
        if (live) d = suggest::closer(d, sim[(long long)won * ld + i]);
    }
}

// what bd_suggest_acquire and its host restatement refuse alike
int check_acquire(const std::string& fn, const float* wide, int64_t W, int32_t ld_wide, const int32_t* member_first, int32_t M,
                  int32_t C, int32_t link, int32_t target, const float* out, int64_t out_stride) {
    if (M < 1 || M > BD_SUGGEST_MAX_MEMBERS)
        return fail(BD_EINVAL, fn + "n_members = " + std::to_string(M) + ", allowed are 1.." + std::to_string(BD_SUGGEST_MAX_MEMBERS));
    if (link != BD_LINK_SOFTMAX && link != BD_LINK_SIGMOID)
        return fail(BD_EINVAL, fn + "link = " + std::to_string(link) + " is neither BD_LINK_SOFTMAX nor BD_LINK_SIGMOID");
    if (C < 1 || C > BD_SUGGEST_MAX_WIDTH)
        return fail(BD_EINVAL, fn + "width = " + std::to_string(C) + ", allowed are 1.." + std::to_string(BD_SUGGEST_MAX_WIDTH));
    if (C < 2 && link != BD_LINK_SIGMOID) return fail(BD_EINVAL, fn + "width = 1 under BD_LINK_SOFTMAX: a softmax needs 2 classes");
    if (target < -1 || target >= C)
        return fail(BD_EINVAL, fn + "target = " + std::to_string(target) + ", allowed are -1.." + std::to_string(C - 1));
    if (target < 0 && link == BD_LINK_SIGMOID)
        return fail(BD_EINVAL, fn + "target = -1 under BD_LINK_SIGMOID: independent columns have no joint distribution, name one");
    if (W < 0 || W > BD_SEARCH_MAX_WINDOWS)
        return fail(BD_EINVAL, fn + "windows = " + std::to_string(W) + ", a call takes 0.." + std::to_string(BD_SEARCH_MAX_WINDOWS));
    if (!member_first) return fail(BD_EINVAL, fn + "member_first is null");
    for (int m = 0; m < M; ++m)
        if (member_first[m] < 0 || (int64_t)member_first[m] + C > ld_wide)
            return fail(BD_EINVAL, fn + "member_first[" + std::to_string(m) + "] = " + std::to_string(member_first[m]) + ": columns " +
                                       std::to_string(member_first[m]) + ".." + std::to_string((int64_t)member_first[m] + C) +
                                       " do not lie in ld_wide = " + std::to_string(ld_wide));
    if (out_stride < W) return fail(BD_EINVAL, fn + "out_stride = " + std::to_string(out_stride) + " is below windows = " + std::to_string(W));
    if ((W > 0 && !wide) || (uintptr_t)wide % 4) return fail(BD_EINVAL, fn + "wide is null or misaligned");
    if ((W > 0 && !out) || (uintptr_t)out % 4) return fail(BD_EINVAL, fn + "out is null or misaligned");
    return BD_OK;
}

// what bd_suggest_pick and its host restatement refuse alike
int check_pick(const std::string& fn, const float* sim, int64_t ld, const float* gain, const float* d0, int32_t n, int32_t k,
               const int32_t* picked, const float* value, const float* dist) {
    if (n < 1 || n > BD_SUGGEST_MAX_POOL)
        return fail(BD_EINVAL, fn + "n = " + std::to_string(n) + ", allowed are 1.." + std::to_string(BD_SUGGEST_MAX_POOL));
    if (k < 1 || k > n) return fail(BD_EINVAL, fn + "k = " + std::to_string(k) + ", allowed are 1..n = " + std::to_string(n));
    if (ld < n) return fail(BD_EINVAL, fn + "ld = " + std::to_string(ld) + " is below n = " + std::to_string(n));
    if (!sim || (uintptr_t)sim % 4) return fail(BD_EINVAL, fn + "sim is null or misaligned");
    if (!gain || (uintptr_t)gain % 4) return fail(BD_EINVAL, fn + "gain is null or misaligned");
    if ((uintptr_t)d0 % 4) return fail(BD_EINVAL, fn + "d0 is misaligned");
    if (!picked || (uintptr_t)picked % 4) return fail(BD_EINVAL, fn + "picked is null or misaligned");
    if (!value || (uintptr_t)value % 4) return fail(BD_EINVAL, fn + "value is null or misaligned");
    if (!dist || (uintptr_t)dist % 4) return fail(BD_EINVAL, fn + "dist is null or misaligned");
    return BD_OK;
}

float scale_of(int32_t C, int32_t target) { return logf(target < 0 ? (float)C : 2.0f); }

}  // namespace
}  // namespace bd

extern "C" {

int bd_suggest_abi_version(void) { return BD_SUGGEST_ABI_VERSION; }

int bd_suggest_acquire(const float* wide_dev, int64_t windows, int32_t ld_wide, const int32_t* member_first, int32_t n_members,
                       int32_t width, int32_t link, int32_t target, float* out_dev, int64_t out_stride, void* stream) {
    const std::string fn = "bd_suggest_acquire: ";
    const int rc = bd::check_acquire(fn, wide_dev, windows, ld_wide, member_first, n_members, width, link, target, out_dev, out_stride);
    if (rc != BD_OK) return rc;
    if (windows == 0) return BD_OK;
    bd::Members first;
    for (int m = 0; m < BD_SUGGEST_MAX_MEMBERS; ++m) first.first[m] = m < n_members ? member_first[m] : 0;
    hipLaunchKernelGGL(bd::suggest_acquire_kernel, dim3((unsigned)((windows + 3) / 4)), dim3(bd::kAcquireThreads), 0,
                       static_cast<hipStream_t>(stream), wide_dev, (int)ld_wide, (int)windows, first, (int)n_members, (int)width,
                       (int)link, (int)target, 1.0f / (float)n_members, bd::scale_of(width, target), out_dev, (long long)out_stride);
    return bd::hip_result(fn);
}

int bd_suggest_acquire_host(const float* wide, int64_t windows, int32_t ld_wide, const int32_t* member_first, int32_t n_members,
                            int32_t width, int32_t link, int32_t target, float* out, int64_t out_stride) {
    namespace sg = bd::suggest;
    const int rc = bd::check_acquire("bd_suggest_acquire_host: ", wide, windows, ld_wide, member_first, n_members, width, link, target,
                                     out, out_stride);
    if (rc != BD_OK) return rc;
    const int M = n_members, C = width;
    const float r_members = 1.0f / (float)M, L = bd::scale_of(width, target);
    float e[BD_SUGGEST_MAX_WIDTH], pbar[BD_SUGGEST_MAX_WIDTH], hs[BD_SUGGEST_MAX_WIDTH];
    for (int64_t w = 0; w < windows; ++w) {
        const float* z0 = wide + (size_t)w * ld_wide;
        float a = 0.0f, b = 0.0f, gap;
        if (target < 0) {
            for (int c = 0; c < C; ++c) pbar[c] = hs[c] = 0.0f;
            for (int m = 0; m < M; ++m) {
                const float* z = z0 + member_first[m];
                float mx = -INFINITY, s = 0.0f;
                for (int c = 0; c < C; ++c) mx = fmaxf(mx, z[c]);
                for (int c = 0; c < C; ++c) s = s + (e[c] = expf(z[c] - mx));
                const float ls = logf(s);
                for (int c = 0; c < C; ++c) {
                    const float p = e[c] / s;
                    pbar[c] += p;
                    hs[c] += sg::term(p, (z[c] - mx) - ls);
                }
            }
            int at = 64;
            float top = -1.0f, second = -1.0f;
            for (int c = 0; c < C; ++c) {
                pbar[c] *= r_members;
                a = a + sg::xlogx(pbar[c]);
                b = b + hs[c];
                if (pbar[c] > top) { top = pbar[c]; at = c; }                  // (the first class that holds the maximum)
            }
            for (int c = 0; c < C; ++c)
                if (c != at) second = fmaxf(second, pbar[c]);
            gap = top - second;
        } else {
            float qs = 0.0f, rs = 0.0f;
            for (int m = 0; m < M; ++m) {
                const float* z = z0 + member_first[m];
                sg::Binary v;
                if (link == BD_LINK_SIGMOID) {
                    v = sg::binary_sigmoid(z[target]);
                } else {
                    float mx = -INFINITY, s = 0.0f, s_other = 0.0f;
                    for (int c = 0; c < C; ++c) mx = fmaxf(mx, z[c]);
                    for (int c = 0; c < C; ++c) {
                        e[c] = expf(z[c] - mx);
                        s = s + e[c];
                        if (c != target) s_other = s_other + e[c];
                    }
                    v = sg::binary_softmax(z[target] - mx, e[target], s, s_other, logf(s));
                }
                qs += v.q;
                rs += v.r;
                b += sg::term(v.q, v.logq) + sg::term(v.r, v.logr);
            }
            const float qbar = qs * r_members, rbar = rs * r_members;
            a = sg::xlogx(qbar) + sg::xlogx(rbar);
            gap = fabsf(2.0f * qbar - 1.0f);
        }
        sg::scores(a, b, gap, M, r_members, L, out + BD_SUGGEST_ENTROPY * out_stride + w, out + BD_SUGGEST_MARGIN * out_stride + w,
                   out + BD_SUGGEST_BALD * out_stride + w);
    }
    return BD_OK;
}

int bd_suggest_pick(const float* sim_dev, int64_t ld, const float* gain_dev, const float* d0_dev, int32_t n, int32_t k,
                    int32_t* picked_dev, float* value_dev, float* dist_dev, void* stream) {
    const std::string fn = "bd_suggest_pick: ";
    const int rc = bd::check_pick(fn, sim_dev, ld, gain_dev, d0_dev, n, k, picked_dev, value_dev, dist_dev);
    if (rc != BD_OK) return rc;
    hipLaunchKernelGGL(bd::suggest_pick_kernel, dim3(1), dim3(bd::kPickThreads), 0, static_cast<hipStream_t>(stream), sim_dev,
                       (long long)ld, gain_dev, d0_dev, (int)n, (int)k, picked_dev, value_dev, dist_dev);
    return bd::hip_result(fn);
}

int bd_suggest_pick_host(const float* sim, int64_t ld, const float* gain, const float* d0, int32_t n, int32_t k, int32_t* picked,
                         float* value, float* dist) {
    namespace sg = bd::suggest;
    const int rc = bd::check_pick("bd_suggest_pick_host: ", sim, ld, gain, d0, n, k, picked, value, dist);
    if (rc != BD_OK) return rc;
    std::vector<float> d((size_t)n);
    std::vector<char> chosen((size_t)n, 0);
    for (int i = 0; i < n; ++i) d[i] = d0 ? d0[i] : 1.0f;
    for (int t = 0; t < k; ++t) {
        uint64_t best = 0;
        for (int i = 0; i < n; ++i) {
            if (chosen[i]) continue;
            const uint64_t key = bd::search::make_key(sg::discounted(gain[i], d[i]), (uint32_t)i);
            best = key > best ? key : best;
        }
        const int won = (int)bd::search::key_id(best);
        chosen[won] = 1;
        picked[t] = won;
        value[t] = sg::discounted(gain[won], d[won]);
        dist[t] = d[won];
        for (int i = 0; i < n; ++i) d[i] = sg::closer(d[i], sim[(int64_t)won * ld + i]);
    }
    return BD_OK;
}

}  // extern "C"
