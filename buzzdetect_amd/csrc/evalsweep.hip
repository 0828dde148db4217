// The threshold sweep for gfx950 (include/buzzdetect_eval.h): the integer counts behind a model's metrics table, taken where
// the logits lie.
//
//   eval_sweep_kernel     a workgroup of kThreads lanes per (slice of BD_EVAL_SLICE windows, column).  The three planes live in
//                         LDS as 16-bit counters, two to a word: 3 * BD_EVAL_BINS / 2 words = 96 KiB, one workgroup a CU.  A lane
//                         takes the windows slice + lane + kThreads j: its label byte, its score, rows_of, then two LDS adds
//                         (kf in the label's plane, kr in the third) of 1 << 16 * (bin & 1) at word bin >> 1.  A slice has at
//                         most 32 768 windows, so a half reaches at most 0x8000 and never carries into its neighbour.  Rows that
//                         only count in `tail` go to four LDS words.  After a barrier every lane walks its share of the words
//                         and adds the non-zero halves to the global state: no-return integer atomics, at most
//                         min(windows, 3 * BD_EVAL_BINS) of them a slice whatever the distribution - real logits pile into a
//                         few hundred bins, which would serialise a million rows adding straight into global words.
//
// Everything added is an integer: the state is a function of the rows alone, whatever the slice size, the grid or the order in
// which the atomics land.  Inputs are only read.  Reads: a lane's windows are kThreads apart, so consecutive lanes read
// consecutive windows - coalesced for a column-major matrix (row_stride 1); for [W][C] logits the lanes of a wave are C floats
// apart and the C workgroups of a slice read the same lines.
#include "bd_error.h"
#include "evalsweep_device.h"

#include "../../include/buzzdetect_eval.h"

#include <cstdint>
#include <string>
#include <vector>

#pragma clang fp contract(off)

namespace bd {
namespace {

constexpr int kThreads = 1024;
constexpr int kBins = BD_EVAL_BINS;
constexpr int kPlaneWords = kBins / 2;                    // two 16-bit counters to a word
constexpr int kWords = BD_EVAL_PLANES * kPlaneWords;
static_assert(BD_EVAL_SLICE <= 0xFFFF, "a slice's windows fit a 16-bit counter");
static_assert(kWords % kThreads == 0 && kBins % 2 == 0, "every lane clears and flushes the same number of words");
static_assert(kWords * 4 + BD_EVAL_TAILS * 4 <= 160 * 1024, "the planes fit a CU's LDS");

__global__ __launch_bounds__(kThreads) void eval_sweep_kernel(const float* __restrict__ x, int W, long long row_stride,
                                                              long long col_stride, const uint8_t* __restrict__ labels, int L,
                                                              const int32_t* __restrict__ label_of, uint32_t* __restrict__ hist,
                                                              uint32_t* __restrict__ tail) {
    __shared__ uint32_t s_pair[kWords];
    __shared__ uint32_t s_tail[BD_EVAL_TAILS];
    const int c = blockIdx.y;
    const int l = label_of[c];
    if (l < 0) return;                                    // (the whole workgroup, before any barrier)
    for (int i = threadIdx.x; i < kWords; i += kThreads) s_pair[i] = 0u;
    if (threadIdx.x < BD_EVAL_TAILS) s_tail[threadIdx.x] = 0u;
    __syncthreads();
    const int first = (int)blockIdx.x * BD_EVAL_SLICE;
    const int end = min(W, first + BD_EVAL_SLICE);
    const float* __restrict__ col = x + (long long)c * col_stride;
    for (int w = first + (int)threadIdx.x; w < end; w += kThreads) {
        const uint8_t label = labels[(size_t)w * L + l];
        const float v = col[(long long)w * row_stride];
        if (label > 1) {
            atomicAdd(&s_tail[0], 1u);
            continue;                                     // (no barrier inside the loop)
        }
        int kf = 0, kr = 0;
        const evalsweep::Kind kind = evalsweep::rows_of(v, &kf, &kr);
        if (kind != evalsweep::kInRange) {
            atomicAdd(&s_tail[(int)kind], 1u);
            continue;
        }
        const int bf = kf - BD_EVAL_K_MIN, br = kr - BD_EVAL_K_MIN;           // 0 .. kBins - 1 (rows_of)
        atomicAdd(&s_pair[(int)label * kPlaneWords + (bf >> 1)], 1u << (16 * (bf & 1)));
        atomicAdd(&s_pair[2 * kPlaneWords + (br >> 1)], 1u << (16 * (br & 1)));
    }
    __syncthreads();
    uint32_t* __restrict__ mine = hist + (size_t)c * BD_EVAL_PLANES * kBins;
    for (int i = threadIdx.x; i < kWords; i += kThreads) {                    // word i: bins 2 i, 2 i + 1 of the planes laid end to end
        const uint32_t pair = s_pair[i];
        if (pair & 0xFFFFu) atomicAdd(&mine[2 * i], pair & 0xFFFFu);
        if (pair >> 16) atomicAdd(&mine[2 * i + 1], pair >> 16);
    }
    if (threadIdx.x < BD_EVAL_TAILS && s_tail[threadIdx.x]) atomicAdd(&tail[(size_t)c * BD_EVAL_TAILS + threadIdx.x], s_tail[threadIdx.x]);
}

// what the device entry point and its host restatement refuse alike
int check_call(const std::string& fn, const float* x, int64_t W, int32_t C, int64_t row_stride, int64_t col_stride,
               const uint8_t* labels, int32_t L, const int32_t* label_of, const uint32_t* hist, const uint32_t* tail) {
    if (W < 0 || W > BD_EVAL_MAX_WINDOWS)
        return fail(BD_EINVAL, fn + "windows = " + std::to_string(W) + ", a call takes 0.." + std::to_string(BD_EVAL_MAX_WINDOWS));
    if (C < 1 || C > BD_EVAL_MAX_COLUMNS)
        return fail(BD_EINVAL, fn + "columns = " + std::to_string(C) + ", allowed are 1.." + std::to_string(BD_EVAL_MAX_COLUMNS));
    if (L < 1 || L > BD_EVAL_MAX_LABELS)
        return fail(BD_EINVAL, fn + "n_labels = " + std::to_string(L) + ", allowed are 1.." + std::to_string(BD_EVAL_MAX_LABELS));
    if (row_stride == 0 || col_stride == 0) return fail(BD_EINVAL, fn + (row_stride == 0 ? "row_stride" : "col_stride") + " is 0");
    if (W > 0 && (!x || (uintptr_t)x % 4)) return fail(BD_EINVAL, fn + "x is null or misaligned");
    if (W > 0 && !labels) return fail(BD_EINVAL, fn + "labels is null");
    if (!label_of || (uintptr_t)label_of % 4) return fail(BD_EINVAL, fn + "label_of is null or misaligned");
    if (!hist || (uintptr_t)hist % 4) return fail(BD_EINVAL, fn + "hist is null or misaligned");
    if (!tail || (uintptr_t)tail % 4) return fail(BD_EINVAL, fn + "tail is null or misaligned");
    return BD_OK;
}

int check_label_of(const std::string& fn, const int32_t* label_of, int32_t C, int32_t L) {
    for (int c = 0; c < C; ++c)
        if (label_of[c] < -1 || label_of[c] >= L)
            return fail(BD_EINVAL, fn + "label_of[" + std::to_string(c) + "] = " + std::to_string(label_of[c]) + ", allowed are -1.."
                                       + std::to_string(L - 1));
    return BD_OK;
}

}  // namespace
}  // namespace bd

extern "C" {

int bd_eval_abi_version(void) { return BD_EVAL_ABI_VERSION; }

int64_t bd_eval_state_bytes(int32_t columns) {
    if (columns < 1 || columns > BD_EVAL_MAX_COLUMNS)
        return bd::fail(BD_EINVAL, "bd_eval_state_bytes: columns = " + std::to_string(columns) + ", allowed are 1.."
                                       + std::to_string(BD_EVAL_MAX_COLUMNS));
    return (int64_t)columns * (BD_EVAL_PLANES * BD_EVAL_BINS + BD_EVAL_TAILS) * (int64_t)sizeof(uint32_t);
}

int bd_eval_accumulate(const float* x_dev, int64_t windows, int32_t columns, int64_t row_stride, int64_t col_stride,
                       const uint8_t* labels_dev, int32_t n_labels, const int32_t* label_of_dev, uint32_t* hist_dev,
                       uint32_t* tail_dev, void* stream) {
    const std::string fn = "bd_eval_accumulate: ";
    int rc = bd::check_call(fn, x_dev, windows, columns, row_stride, col_stride, labels_dev, n_labels, label_of_dev, hist_dev,
                            tail_dev);
    if (rc != BD_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<int32_t> label_of((size_t)columns);
    BD_HIP(hipMemcpyAsync(label_of.data(), label_of_dev, label_of.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    BD_HIP(hipStreamSynchronize(s));
    if ((rc = bd::check_label_of(fn, label_of.data(), columns, n_labels)) != BD_OK) return rc;
    if (windows == 0) return BD_OK;
    const unsigned slices = (unsigned)((windows + BD_EVAL_SLICE - 1) / BD_EVAL_SLICE);
    hipLaunchKernelGGL(bd::eval_sweep_kernel, dim3(slices, (unsigned)columns), dim3(bd::kThreads), 0, s, x_dev, (int)windows,
                       (long long)row_stride, (long long)col_stride, labels_dev, (int)n_labels, label_of_dev, hist_dev, tail_dev);
    return bd::hip_result(fn);
}

int bd_eval_accumulate_host(const float* x, int64_t windows, int32_t columns, int64_t row_stride, int64_t col_stride,
                            const uint8_t* labels, int32_t n_labels, const int32_t* label_of, uint32_t* hist, uint32_t* tail) {
    const std::string fn = "bd_eval_accumulate_host: ";
    int rc = bd::check_call(fn, x, windows, columns, row_stride, col_stride, labels, n_labels, label_of, hist, tail);
    if (rc != BD_OK) return rc;
    if ((rc = bd::check_label_of(fn, label_of, columns, n_labels)) != BD_OK) return rc;
    for (int32_t c = 0; c < columns; ++c) {
        if (label_of[c] < 0) continue;
        uint32_t* planes = hist + (size_t)c * BD_EVAL_PLANES * BD_EVAL_BINS;
        uint32_t* tails = tail + (size_t)c * BD_EVAL_TAILS;
        for (int64_t w = 0; w < windows; ++w) {
            const uint8_t label = labels[(size_t)w * n_labels + label_of[c]];
            if (label > 1) {
                ++tails[0];
                continue;
            }
            int kf = 0, kr = 0;
            const bd::evalsweep::Kind kind = bd::evalsweep::rows_of(x[w * row_stride + (int64_t)c * col_stride], &kf, &kr);
            if (kind != bd::evalsweep::kInRange) {
                ++tails[(int)kind];
                continue;
            }
            ++planes[(size_t)label * BD_EVAL_BINS + (kf - BD_EVAL_K_MIN)];
            ++planes[(size_t)2 * BD_EVAL_BINS + (kr - BD_EVAL_K_MIN)];
        }
    }
    return BD_OK;
}

}  // extern "C"
