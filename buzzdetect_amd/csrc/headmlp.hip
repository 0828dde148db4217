// The dense-stack classifier head (include/buzzdetect_head.h): one launch per Dense layer, C[W][N] = act(A[W][K] W + b), in
// exact float32 on v_mfma_f32_32x32x2_f32, whatever arithmetic the CNN runs in; a softmax is a row pass behind the last layer
// (from the workspace into the logits).
//
// A wave owns one 32 x 32 tile of C and walks K alone, in ascending super-steps of 8 k: nothing is split over waves or
// workgroups and nothing is added atomically, and the instruction is a chain of fused multiply-adds per output element, so an
// output depends on its row of A, its column of W and this file's k order only - not on where the row sits in the launch.
// That is what lets a window give the same bits alone, inside a full pass and inside a ragged last pass.
//
// Operand map (cnn.hip, pointwise_kernel): lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]; lane-half h
// takes k = 8 s + 4 h + j for the j-th instruction of super-step s, so one 16-byte load per operand feeds four instructions.
//   A  straight from global memory: row min(row, W - 1) (always in bounds, never stored), 16 bytes at k = 8 s + 4 h.  Rows are
//      lda >= round_up(K, 32) floats apart, so the load stays inside its row; elements at k >= K (never written: the layer
//      before stores its N columns only) are replaced by zero.
//   B  the host packs W into fragment order at attach time, zero-padded to 32-column tiles and 32-k groups:
//      [N / 32 tiles][K / 8 super-steps][64 lanes][4]: lane l holds W[8 s + 4 (l >> 5) + j][32 t + (l & 31)], j = 0..3.
//      A wave's load of a super-step is 1 KB, contiguous.
// Four super-steps (32 k) are in flight ahead of the sixteen matrix instructions that use them; one accumulator per wave is
// enough, the instruction's issue interval and its dependent latency both being 64 cycles.  A workgroup is 2 x 2 waves = a
// 64 x 64 tile, so 1024 windows x 1024 columns are 256 workgroups, one per compute unit.  There is no LDS and no barrier.
#include "engine_state.h"
#include "dense_device.h"

#include <cstring>

#include "../../include/buzzdetect_head.h"

namespace bd {
namespace {

__global__ __launch_bounds__(256) void dense_kernel(const float* __restrict__ A, int lda, int W, int K, int n_super,
                                                     const float4* __restrict__ Wf, const float* __restrict__ bias, int N,
                                                     int act, float* __restrict__ C, int ldc) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int tr = 2 * blockIdx.x + (wave & 1);         // 32-row tile of C
    const int tc = 2 * blockIdx.y + (wave >> 1);        // 32-column tile
    if (32 * tr >= W || 32 * tc >= N) return;           // (no barrier in this kernel)
    const int half = lane >> 5;
    const int arow = min(32 * tr + (lane & 31), W - 1);
    const float* ap = A + (size_t)arow * lda + 4 * half;
    const float4* bp = Wf + (size_t)tc * n_super * 64 + lane;

    const dense_v16f acc = dense_tile_walk(ap, bp, K, n_super, half);     // (dense_device.h: shared with headset.hip)
    dense_tile_store(acc, bias, act, tr, tc, W, N, C, ldc, lane);
}

// softmax over each row of x = [W][ldx] (columns < n) into y = [W][n], out of place (a launch repeated on the same operands gives
// the same result): one wave per row, lane l takes columns l, l + 64, ... in ascending order, the 64 partial results meet in a
// butterfly - the same order for every row wherever it sits
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y, int W,
                                                            int n) {
    const int lane = threadIdx.x & 63;
    const int row = 4 * blockIdx.x + (threadIdx.x >> 6);
    if (row >= W) return;
    const float* p = x + (size_t)row * ldx;
    float* q = y + (size_t)row * n;
    softmax_row(p, q, n, lane);
}

}  // namespace

size_t dense_packed_floats(int k, int n) { return (size_t)((k + 31) / 32 * 32) * ((n + 31) / 32 * 32); }

void dense_pack_weights(const float* kernel, int k, int n, float* dst) {
    const int n_super = (k + 31) / 32 * 4, tiles = (n + 31) / 32;
    for (int t = 0; t < tiles; ++t)
        for (int s = 0; s < n_super; ++s)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 4; ++j) {
                    const int kk = 8 * s + 4 * (l >> 5) + j, nn = 32 * t + (l & 31);
                    dst[(((size_t)t * n_super + s) * 64 + l) * 4 + j] = kk < k && nn < n ? kernel[(size_t)kk * n + nn] : 0.0f;
                }
}

void launch_dense(const float* A, int lda, int windows, const DenseLayer& L, float* C, int ldc, hipStream_t stream) {
    if (windows <= 0) return;
    const int n_super = (L.k + 31) / 32 * 4;
    hipLaunchKernelGGL(dense_kernel, dim3((windows + 63) / 64, (L.n + 63) / 64), dim3(256), 0, stream, A, lda, windows, L.k,
                       n_super, reinterpret_cast<const float4*>(L.wfrag), L.bias, L.n, L.act, C, ldc);
}

void launch_softmax_rows(const float* x, int ldx, float* y, int windows, int n, hipStream_t stream) {
    if (windows <= 0) return;
    hipLaunchKernelGGL(softmax_rows_kernel, dim3((windows + 3) / 4), dim3(256), 0, stream, x, ldx, y, windows, n);
}

}  // namespace bd

extern "C" {

int bd_head_abi_version(void) { return BD_HEAD_ABI_VERSION; }

int bd_head_outputs(bd_handle h) {
    if (!h) return fail(BD_EINVAL, "bd_head_outputs: null handle");
    return h->stack.empty() ? 0 : h->stack.back().n;
}

int bd_head_attach(bd_handle h, const bd_head_layer* layers, int32_t n_layers) {
    if (!h || !layers) return fail(BD_EINVAL, "bd_head_attach: null argument");
    if (h->n_classes != 0 || !h->stack.empty())
        return fail(BD_EINVAL, "bd_head_attach: the engine already has a head (create it with n_classes == 0)");
    if (n_layers < 1 || n_layers > BD_HEAD_MAX_LAYERS)
        return fail(BD_EINVAL, "bd_head_attach: a stack has 1.." + std::to_string(BD_HEAD_MAX_LAYERS) + " layers, not " +
                                   std::to_string(n_layers));
    int width = BD_EMBEDDING_SIZE;
    size_t floats = 0;
    for (int i = 0; i < n_layers; ++i) {
        const bd_head_layer& L = layers[i];
        const std::string who = "bd_head_attach: layer " + std::to_string(i);
        if (!L.kernel) return fail(BD_EINVAL, who + " has no kernel");
        if (L.n_out < 1 || L.n_out > BD_HEAD_MAX_WIDTH)
            return fail(BD_EINVAL, who + ": width " + std::to_string(L.n_out) + " outside 1.." + std::to_string(BD_HEAD_MAX_WIDTH));
        if (L.n_in != width)
            return fail(BD_EINVAL, who + " takes " + std::to_string(L.n_in) + " inputs, the layer before it gives " +
                                       std::to_string(width));
        if (L.activation < BD_HEAD_LINEAR || L.activation > BD_HEAD_SOFTMAX)
            return fail(BD_EINVAL, who + ": unknown activation " + std::to_string(L.activation));
        if (L.activation == BD_HEAD_SOFTMAX && i + 1 != n_layers) return fail(BD_EINVAL, who + ": softmax on a hidden layer");
        floats += bd::dense_packed_floats(L.n_in, L.n_out) + (size_t)align_up(L.n_out, 4);
        width = L.n_out;
    }
    std::vector<float> host(floats, 0.0f);
    std::vector<bd::DenseLayer> stack;
    std::vector<size_t> at;
    size_t off = 0;
    for (int i = 0; i < n_layers; ++i) {
        const bd_head_layer& L = layers[i];
        at.push_back(off);
        bd::dense_pack_weights(L.kernel, L.n_in, L.n_out, host.data() + off);
        off += bd::dense_packed_floats(L.n_in, L.n_out);
        if (L.bias) std::memcpy(host.data() + off, L.bias, (size_t)L.n_out * sizeof(float));
        off += (size_t)align_up(L.n_out, 4);
    }
    BD_HIP(hipSetDevice(h->device));
    float* dev = nullptr;
    BD_HIP(hipMalloc(&dev, floats * sizeof(float)));
    if (hipMemcpy(dev, host.data(), floats * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(dev);
        return fail(BD_EHIP, "bd_head_attach: upload failed");
    }
    for (int i = 0; i < n_layers; ++i) {
        const bd_head_layer& L = layers[i];
        stack.push_back(bd::DenseLayer{L.n_in, L.n_out, L.activation, dev + at[i],
                                       dev + at[i] + bd::dense_packed_floats(L.n_in, L.n_out)});
    }
    h->d_stack = dev;
    h->stack = std::move(stack);
    h->n_classes = width;
    return BD_OK;
}

}  // extern "C"
