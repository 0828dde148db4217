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
#include "bd_internal.h"

#include "../../include/buzzdetect_head.h"

namespace bd {
namespace {

typedef float v16f __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float head_act(float x, int act) {
    if (act == BD_HEAD_RELU) return fmaxf(x, 0.0f);
    if (act == BD_HEAD_SIGMOID) return 1.0f / (1.0f + expf(-x));
    if (act == BD_HEAD_TANH) return tanhf(x);
    return x;                                   // linear, and softmax (a row pass follows)
}

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

    float4 a[4], b[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        a[q] = *reinterpret_cast<const float4*>(ap + 8 * q);
        b[q] = bp[(size_t)q * 64];
    }
    v16f acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int s = 0; s < n_super; s += 4) {              // n_super is a multiple of 4
        float4 an[4], bn[4];
        const bool more = s + 4 < n_super;
        if (more) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                an[q] = *reinterpret_cast<const float4*>(ap + 8 * (s + 4 + q));
                bn[q] = bp[(size_t)(s + 4 + q) * 64];
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k0 = 8 * (s + q) + 4 * half;
            const float ax = k0 + 0 < K ? a[q].x : 0.0f;
            const float ay = k0 + 1 < K ? a[q].y : 0.0f;
            const float az = k0 + 2 < K ? a[q].z : 0.0f;
            const float aw = k0 + 3 < K ? a[q].w : 0.0f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ax, b[q].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ay, b[q].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(az, b[q].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aw, b[q].w, acc, 0, 0, 0);
        }
        if (more) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a[q] = an[q];
                b[q] = bn[q];
            }
        }
    }
    // accumulator r of lane l is C[32 tr + (r & 3) + 8 (r >> 2) + 4 (l >> 5)][32 tc + (l & 31)]
    const int col = 32 * tc + (lane & 31);
    if (col >= N) return;
    const float bv = bias[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = 32 * tr + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (row < W) C[(size_t)row * ldc + col] = head_act(acc[r] + bv, act);
    }
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
    float m = -INFINITY;
    for (int c = lane; c < n; c += 64) m = fmaxf(m, p[c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float sum = 0.0f;
    for (int c = lane; c < n; c += 64) sum += expf(p[c] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    for (int c = lane; c < n; c += 64) q[c] = expf(p[c] - m) / sum;
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
