// Label propagation for gfx950 (include/buzzdetect_propagate.h): a few labels spread along a neighbour graph in CSR form.
//
//   propagate_weights_kernel   a thread per slot of the neighbour lists: the edge's weight and its neighbour.
//   propagate_step_kernel      a workgroup per slice of 256 rows, a wave per row, a lane per class: the row's edges in stored
//                              order, one fused multiply-add a class and an edge, the weighted mean, the clamp against Y; the
//                              lanes' largest movements meet in a butterfly of maxima, the four waves' in LDS.
//   propagate_readout_kernel   a wave per row: the butterfly of bd_search_norms over the classes for the reach, a butterfly on
//                              (value, class) pairs for the top class, one of maxima over the others for the second.
//
// No floating-point number is added atomically, no result depends on the grid, every output element has one writer, inputs are
// only read, element offsets are 64-bit, and every index read from memory (a neighbour, a row's edge range) is brought into
// range before it addresses anything.
#include "bd_internal.h"
#include "bd_error.h"
#include "propagate_device.h"
#include "simsearch_device.h"

#include "../../include/buzzdetect_propagate.h"

#include <algorithm>
#include <string>

#pragma clang fp contract(off)

namespace bd {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
static_assert(BD_PROPAGATE_SLICE % kWaves == 0, "a slice is whole rounds of the workgroup's waves");
static_assert(BD_PROPAGATE_MAX_CLASSES == 64, "a lane per class");

__global__ __launch_bounds__(kThreads) void propagate_weights_kernel(const int32_t* __restrict__ ids, const float* __restrict__ sims,
                                                                      int64_t rows, int k, int power, int32_t* __restrict__ nbr,
                                                                      float* __restrict__ w) {
    const int64_t at = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (at >= rows * k) return;
    const int32_t id = ids[at];
    nbr[at] = id < 0 ? (int32_t)(at / k) : id;
    w[at] = id < 0 ? 0.0f : propagate::weight(sims[at], power);
}

__global__ __launch_bounds__(kThreads) void propagate_step_kernel(const int64_t* __restrict__ row_start, const int32_t* __restrict__ nbr,
                                                                   const float* __restrict__ w, int64_t N, int64_t E,
                                                                   const float* __restrict__ f_in, const float* __restrict__ y,
                                                                   const float* __restrict__ alpha, int C, float* __restrict__ f_out,
                                                                   float* __restrict__ delta) {
    __shared__ float s_moved[kWaves];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t first = (int64_t)blockIdx.x * BD_PROPAGATE_SLICE;
    const int c = min(lane, C - 1);                       // lanes past the classes walk along with the last class and store nothing
    float far = 0.0f;
#pragma unroll 1
    for (int r = wave; r < BD_PROPAGATE_SLICE; r += kWaves) {
        const int64_t i = first + r;
        if (i >= N) break;                                // (uniform over the wave; the barrier lies behind the loop)
        const int64_t lo = propagate::clamp_index(row_start[i], 0, E);
        const int64_t hi = propagate::clamp_index(row_start[i + 1], lo, E);
        float acc = 0.0f, den = 0.0f;
#pragma unroll 4
        for (int64_t e = lo; e < hi; ++e) {
            const float we = w[e];
            const int64_t j = propagate::clamp_index(nbr[e], 0, N - 1);
            acc = propagate::edge_acc(we, f_in[(size_t)j * C + c], acc);
            den = propagate::edge_den(we, den);
        }
        const float out = propagate::step_out(alpha[i], propagate::mean_of(acc, den), y[(size_t)i * C + c]);
        if (lane < C) {
            f_out[(size_t)i * C + c] = out;
            far = fmaxf(far, propagate::moved(out, f_in[(size_t)i * C + c]));
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) far = fmaxf(far, __shfl_xor(far, m, 64));
    if (lane == 0) s_moved[wave] = far;
    __syncthreads();
    if (threadIdx.x == 0) {
        float v = s_moved[0];
#pragma unroll
        for (int u = 1; u < kWaves; ++u) v = fmaxf(v, s_moved[u]);
        delta[blockIdx.x] = v;
    }
}

__global__ __launch_bounds__(kThreads) void propagate_readout_kernel(const float* __restrict__ f, int64_t N, int C,
                                                                      float* __restrict__ reach, int32_t* __restrict__ label,
                                                                      float* __restrict__ confidence, float* __restrict__ margin) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (i >= N) return;                                   // (no barrier in this kernel)
    const float v = lane < C ? f[(size_t)i * C + lane] : 0.0f;
    const float total = search::butterfly_wave(v);
    float tv = lane < C ? propagate::ordered(v) : -INFINITY;
    const float mine = tv;
    int tc = lane;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(tv, m, 64);
        const int oc = __shfl_xor(tc, m, 64);
        if (propagate::before(ov, oc, tv, tc)) {
            tv = ov;
            tc = oc;
        }
    }
    float second = lane == tc ? -INFINITY : mine;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) second = fmaxf(second, __shfl_xor(second, m, 64));
    if (C == 1) second = 0.0f;
    if (lane != 0) return;
    const bool ok = propagate::reached(total);
    reach[i] = total;
    label[i] = ok ? tc : -1;
    confidence[i] = ok ? propagate::confidence(tv, total) : 0.0f;
    margin[i] = ok ? propagate::margin(tv, second, total) : 0.0f;
}

// ---------------------------------------------------------------------------------------------------- host side
int check_pointer(const std::string& fn, const char* name, const void* p, int align) {
    if (!p) return fail(BD_EINVAL, fn + name + " is null");
    if ((uintptr_t)p % (uintptr_t)align) return fail(BD_EINVAL, fn + name + " is not " + std::to_string(align) + "-byte aligned");
    return BD_OK;
}

int check_rows(const std::string& fn, int64_t N) {
    if (N < 0 || N > BD_PROPAGATE_MAX_ROWS)
        return fail(BD_EINVAL, fn + "rows = " + std::to_string(N) + ", a call takes 0.." + std::to_string(BD_PROPAGATE_MAX_ROWS));
    return BD_OK;
}

int check_classes(const std::string& fn, int32_t C) {
    if (C < 1 || C > BD_PROPAGATE_MAX_CLASSES)
        return fail(BD_EINVAL, fn + "classes = " + std::to_string(C) + ", allowed are 1.." + std::to_string(BD_PROPAGATE_MAX_CLASSES));
    return BD_OK;
}

int check_weights(const std::string& fn, const int32_t* ids, const float* sims, int64_t N, int32_t k, int32_t power, const int32_t* nbr,
                  const float* w) {
    if (k < 1 || k > BD_KNN_MAX_K) return fail(BD_EINVAL, fn + "k = " + std::to_string(k) + ", allowed are 1.." + std::to_string(BD_KNN_MAX_K));
    if (power < 1 || power > BD_PROPAGATE_MAX_POWER)
        return fail(BD_EINVAL, fn + "power = " + std::to_string(power) + ", allowed are 1.." + std::to_string(BD_PROPAGATE_MAX_POWER));
    int rc = check_rows(fn, N);
    if (rc != BD_OK || N == 0) return rc;
    if ((rc = check_pointer(fn, "ids", ids, 4)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "sims", sims, 4)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "nbr", nbr, 4)) != BD_OK) return rc;
    return check_pointer(fn, "w", w, 4);
}

int check_step(const std::string& fn, const int64_t* row_start, const int32_t* nbr, const float* w, int64_t N, int64_t E,
               const float* f_in, const float* y, const float* alpha, int32_t C, const float* f_out, const float* delta) {
    int rc = check_classes(fn, C);
    if (rc != BD_OK) return rc;
    if (E < 0) return fail(BD_EINVAL, fn + "edges = " + std::to_string(E) + " is negative");
    if ((rc = check_rows(fn, N)) != BD_OK || N == 0) return rc;
    if ((rc = check_pointer(fn, "row_start", row_start, 8)) != BD_OK) return rc;
    if (E > 0 && (rc = check_pointer(fn, "nbr", nbr, 4)) != BD_OK) return rc;
    if (E > 0 && (rc = check_pointer(fn, "w", w, 4)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "f_in", f_in, 4)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "y", y, 4)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "alpha", alpha, 4)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "f_out", f_out, 4)) != BD_OK) return rc;
    if (f_out == f_in) return fail(BD_EINVAL, fn + "f_out is f_in: a step reads its neighbours' rows while it writes");
    return check_pointer(fn, "delta", delta, 4);
}

int check_readout(const std::string& fn, const float* f, int64_t N, int32_t C, const float* reach, const int32_t* label,
                  const float* confidence, const float* margin) {
    int rc = check_classes(fn, C);
    if (rc != BD_OK) return rc;
    if ((rc = check_rows(fn, N)) != BD_OK || N == 0) return rc;
    if ((rc = check_pointer(fn, "f", f, 4)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "reach", reach, 4)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "label", label, 4)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "confidence", confidence, 4)) != BD_OK) return rc;
    return check_pointer(fn, "margin", margin, 4);
}

}  // namespace
}  // namespace bd

extern "C" {

int bd_propagate_abi_version(void) { return BD_PROPAGATE_ABI_VERSION; }

int bd_propagate_weights(const int32_t* ids_dev, const float* sims_dev, int64_t rows, int32_t k, int32_t power, int32_t* nbr_dev,
                         float* w_dev, void* stream) {
    const std::string fn = "bd_propagate_weights: ";
    const int rc = bd::check_weights(fn, ids_dev, sims_dev, rows, k, power, nbr_dev, w_dev);
    if (rc != BD_OK || rows == 0) return rc;
    hipLaunchKernelGGL(bd::propagate_weights_kernel, dim3((unsigned)((rows * k + bd::kThreads - 1) / bd::kThreads)), dim3(bd::kThreads),
                       0, static_cast<hipStream_t>(stream), ids_dev, sims_dev, rows, (int)k, (int)power, nbr_dev, w_dev);
    return bd::hip_result(fn);
}

int bd_propagate_weights_host(const int32_t* ids, const float* sims, int64_t rows, int32_t k, int32_t power, int32_t* nbr, float* w) {
    const int rc = bd::check_weights("bd_propagate_weights_host: ", ids, sims, rows, k, power, nbr, w);
    if (rc != BD_OK) return rc;
    for (int64_t at = 0; at < rows * k; ++at) {
        nbr[at] = ids[at] < 0 ? (int32_t)(at / k) : ids[at];
        w[at] = ids[at] < 0 ? 0.0f : bd::propagate::weight(sims[at], power);
    }
    return BD_OK;
}

int bd_propagate_step(const int64_t* row_start_dev, const int32_t* nbr_dev, const float* w_dev, int64_t rows, int64_t edges,
                      const float* f_in_dev, const float* y_dev, const float* alpha_dev, int32_t classes, float* f_out_dev,
                      float* delta_dev, void* stream) {
    const std::string fn = "bd_propagate_step: ";
    const int rc = bd::check_step(fn, row_start_dev, nbr_dev, w_dev, rows, edges, f_in_dev, y_dev, alpha_dev, classes, f_out_dev,
                                  delta_dev);
    if (rc != BD_OK || rows == 0) return rc;
    hipLaunchKernelGGL(bd::propagate_step_kernel, dim3((unsigned)((rows + BD_PROPAGATE_SLICE - 1) / BD_PROPAGATE_SLICE)),
                       dim3(bd::kThreads), 0, static_cast<hipStream_t>(stream), row_start_dev, nbr_dev, w_dev, rows, edges, f_in_dev,
                       y_dev, alpha_dev, (int)classes, f_out_dev, delta_dev);
    return bd::hip_result(fn);
}

int bd_propagate_step_host(const int64_t* row_start, const int32_t* nbr, const float* w, int64_t rows, int64_t edges, const float* f_in,
                           const float* y, const float* alpha, int32_t classes, float* f_out, float* delta) {
    namespace pr = bd::propagate;
    const std::string fn = "bd_propagate_step_host: ";
    const int rc = bd::check_step(fn, row_start, nbr, w, rows, edges, f_in, y, alpha, classes, f_out, delta);
    if (rc != BD_OK || rows == 0) return rc;
    if (row_start[0] < 0 || row_start[rows] > edges)
        return bd::fail(BD_ERANGE, fn + "row_start does not lie within 0.." + std::to_string(edges));
    for (int64_t i = 0; i < rows; ++i)
        if (row_start[i] > row_start[i + 1]) return bd::fail(BD_ERANGE, fn + "row_start[" + std::to_string(i) + "..] does not ascend");
    for (int64_t e = row_start[0]; e < row_start[rows]; ++e)
        if (nbr[e] < 0 || nbr[e] >= rows)
            return bd::fail(BD_ERANGE, fn + "nbr[" + std::to_string(e) + "] = " + std::to_string(nbr[e]) + " is no row");
    const int C = classes;
    for (int64_t first = 0; first < rows; first += BD_PROPAGATE_SLICE) {
        float far = 0.0f;
        for (int64_t i = first; i < std::min<int64_t>(first + BD_PROPAGATE_SLICE, rows); ++i)
            for (int c = 0; c < C; ++c) {
                float acc = 0.0f, den = 0.0f;
                for (int64_t e = row_start[i]; e < row_start[i + 1]; ++e) {
                    acc = pr::edge_acc(w[e], f_in[(size_t)nbr[e] * C + c], acc);
                    den = pr::edge_den(w[e], den);
                }
                const float out = pr::step_out(alpha[i], pr::mean_of(acc, den), y[(size_t)i * C + c]);
                f_out[(size_t)i * C + c] = out;
                far = fmaxf(far, pr::moved(out, f_in[(size_t)i * C + c]));
            }
        delta[first / BD_PROPAGATE_SLICE] = far;
    }
    return BD_OK;
}

int bd_propagate_readout(const float* f_dev, int64_t rows, int32_t classes, float* reach_dev, int32_t* label_dev,
                         float* confidence_dev, float* margin_dev, void* stream) {
    const std::string fn = "bd_propagate_readout: ";
    const int rc = bd::check_readout(fn, f_dev, rows, classes, reach_dev, label_dev, confidence_dev, margin_dev);
    if (rc != BD_OK || rows == 0) return rc;
    hipLaunchKernelGGL(bd::propagate_readout_kernel, dim3((unsigned)((rows + bd::kWaves - 1) / bd::kWaves)), dim3(bd::kThreads), 0,
                       static_cast<hipStream_t>(stream), f_dev, rows, (int)classes, reach_dev, label_dev, confidence_dev, margin_dev);
    return bd::hip_result(fn);
}

int bd_propagate_readout_host(const float* f, int64_t rows, int32_t classes, float* reach, int32_t* label, float* confidence,
                              float* margin) {
    namespace pr = bd::propagate;
    const int rc = bd::check_readout("bd_propagate_readout_host: ", f, rows, classes, reach, label, confidence, margin);
    if (rc != BD_OK) return rc;
    const int C = classes;
    for (int64_t i = 0; i < rows; ++i) {
        const float* row = f + (size_t)i * C;
        float v[64];
        for (int lane = 0; lane < 64; ++lane) v[lane] = lane < C ? row[lane] : 0.0f;
        const float total = bd::search::butterfly_host(v);
        float tv = pr::ordered(row[0]);
        int tc = 0;
        for (int c = 1; c < C; ++c)
            if (pr::before(pr::ordered(row[c]), c, tv, tc)) {
                tv = pr::ordered(row[c]);
                tc = c;
            }
        float second = C == 1 ? 0.0f : -INFINITY;
        for (int c = 0; c < C; ++c)
            if (c != tc) second = fmaxf(second, pr::ordered(row[c]));
        const bool ok = pr::reached(total);
        reach[i] = total;
        label[i] = ok ? tc : -1;
        confidence[i] = ok ? pr::confidence(tv, total) : 0.0f;
        margin[i] = ok ? pr::margin(tv, second, total) : 0.0f;
    }
    return BD_OK;
}

}  // extern "C"
