// Device routines of the classifier-head trainer, shared by headtrain.hip (one stack: include/buzzdetect_train.h),
// headbank.hip (a bank of one-layer heads: include/buzzdetect_bank.h) and stackbank.hip (a bank of Dense stacks:
// include/buzzdetect_stackbank.h).  The three files call these and nothing else for a product, a row's loss, a partial's sum
// or an update, so a member of a bank and a trainer on its own run the same instructions in the same order: the bit identity
// the banks promise rests on this file being the only copy.  (headtrain_host.h is its counterpart for the host side, and
// headtrain_stack.h holds the layer-by-layer kernels that headtrain.hip and stackbank.hip both launch.)
//
// Every product is one routine, mma_chain: a wave owns a 32 x 32 output tile and walks the reduced index alone in ascending
// super-steps of 8, in headmlp.hip's operand map (lane l supplies A[i = l & 31][k] and B[k][j = l & 31], lane-half h takes
// k = 8 s + 4 h + j for the j-th instruction of super-step s), four super-steps in flight ahead of the sixteen instructions
// that use them.  An output element is one chain of fused multiply-adds in ascending k whatever its neighbours in the tile hold.
// Elements outside a matrix are zeros chosen by a compare, never loaded; no address outside a row that exists is formed.
#ifndef BD_HEADTRAIN_DEVICE_H
#define BD_HEADTRAIN_DEVICE_H

#include "bd_internal.h"

#include <cmath>

#include "../../include/buzzdetect_train.h"

namespace bd {
namespace train {

constexpr int kSliceRows = BD_TRAIN_SLICE_ROWS;
static_assert(kSliceRows % 32 == 0, "a slice is whole 32-row steps of the matrix instruction");

typedef float v16f __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float act_fwd(float x, int act) {       // dense_device.h's head_act
    if (act == BD_HEAD_RELU) return fmaxf(x, 0.0f);
    if (act == BD_HEAD_SIGMOID) return 1.0f / (1.0f + expf(-x));
    if (act == BD_HEAD_TANH) return tanhf(x);
    return x;
}

__device__ __forceinline__ float act_grad(float y, int act) {      // from the stored activation y
    if (act == BD_HEAD_RELU) return y > 0.0f ? 1.0f : 0.0f;
    if (act == BD_HEAD_SIGMOID) return y * (1.0f - y);
    if (act == BD_HEAD_TANH) return 1.0f - y * y;
    return 1.0f;
}

// acc[32][32] = sum over super-steps s < n_super (a multiple of 4) of fa(s) x fb(s): fa(s) / fb(s) give this lane's four
// operand elements k = 8 s + 4 (lane >> 5) + 0..3
template <class FA, class FB>
__device__ __forceinline__ v16f mma_chain(int n_super, FA fa, FB fb) {
    float4 a[4], b[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        a[q] = fa(q);
        b[q] = fb(q);
    }
    v16f acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int s = 0; s < n_super; s += 4) {
        float4 an[4], bn[4];
        const bool more = s + 4 < n_super;
        if (more) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                an[q] = fa(s + 4 + q);
                bn[q] = fb(s + 4 + q);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].x, b[q].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].y, b[q].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].z, b[q].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].w, b[q].w, acc, 0, 0, 0);
        }
        if (more) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a[q] = an[q];
                b[q] = bn[q];
            }
        }
    }
    return acc;
}

// accumulator r of lane l is element [(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31] of the tile
__device__ __forceinline__ int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// Y[32 tr ..][32 tc ..] = act(A W + b).  A is [.][lda] with lda >= round_up(K, 32) (X: ldx >= 1024 = K), rows < B; `rows`
// (layer 0 only) names the row of A that batch row r reads.  P = W [K][N] then b [N].
__device__ __forceinline__ void forward_tile(const float* __restrict__ A, int64_t lda, const int* __restrict__ rows, int B, int K,
                                             const float* __restrict__ P, int N, int act, float* Y, int ldy, int tr,
                                             int tc, int lane) {
    const int half = lane >> 5, li = lane & 31;
    const int br = min(32 * tr + li, B - 1);
    const int64_t src = rows ? rows[br] : br;
    const float* ap = A + src * lda + 4 * half;
    const int col = 32 * tc + li;
    const bool col_ok = col < N;
    const float* wp = P + (col_ok ? col : 0);
    const v16f acc = mma_chain((K + 31) / 32 * 4,
        [&](int s) {
            float4 v = *reinterpret_cast<const float4*>(ap + 8 * s);
            const int k0 = 8 * s + 4 * half;
            v.x = k0 + 0 < K ? v.x : 0.0f;
            v.y = k0 + 1 < K ? v.y : 0.0f;
            v.z = k0 + 2 < K ? v.z : 0.0f;
            v.w = k0 + 3 < K ? v.w : 0.0f;
            return v;
        },
        [&](int s) {
            const int k0 = 8 * s + 4 * half;
            float4 v;
            v.x = col_ok && k0 + 0 < K ? wp[(size_t)(k0 + 0) * N] : 0.0f;
            v.y = col_ok && k0 + 1 < K ? wp[(size_t)(k0 + 1) * N] : 0.0f;
            v.z = col_ok && k0 + 2 < K ? wp[(size_t)(k0 + 2) * N] : 0.0f;
            v.w = col_ok && k0 + 3 < K ? wp[(size_t)(k0 + 3) * N] : 0.0f;
            return v;
        });
    if (!col_ok) return;
    const float bv = P[(size_t)K * N + col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = 32 * tr + acc_row(r, half);
        if (row < B) Y[(size_t)row * ldy + col] = act_fwd(acc[r] + bv, act);
    }
}

// Gp[32 tr ..][32 tc ..] = (G W^T) * act'(Yp): G [B][ldg] (columns < N), W [K][N], Yp / Gp [B][ldp] (columns < K)
__device__ __forceinline__ void input_grad_tile(const float* __restrict__ G, int ldg, int B, int K, const float* __restrict__ W,
                                                int N, const float* __restrict__ Yp, int act_p, float* __restrict__ Gp, int ldp,
                                                int tr, int tc, int lane) {
    const int half = lane >> 5, li = lane & 31;
    const float* gp = G + (size_t)min(32 * tr + li, B - 1) * ldg + 4 * half;
    const int col = 32 * tc + li;                        // an input of the layer: a row of W
    const bool col_ok = col < K;
    const float* wp = W + (size_t)(col_ok ? col : 0) * N;
    const v16f acc = mma_chain((N + 31) / 32 * 4,
        [&](int s) {
            float4 v = *reinterpret_cast<const float4*>(gp + 8 * s);
            const int n0 = 8 * s + 4 * half;
            v.x = n0 + 0 < N ? v.x : 0.0f;
            v.y = n0 + 1 < N ? v.y : 0.0f;
            v.z = n0 + 2 < N ? v.z : 0.0f;
            v.w = n0 + 3 < N ? v.w : 0.0f;
            return v;
        },
        [&](int s) {
            const int n0 = 8 * s + 4 * half;
            float4 v;
            v.x = col_ok && n0 + 0 < N ? wp[n0 + 0] : 0.0f;
            v.y = col_ok && n0 + 1 < N ? wp[n0 + 1] : 0.0f;
            v.z = col_ok && n0 + 2 < N ? wp[n0 + 2] : 0.0f;
            v.w = col_ok && n0 + 3 < N ? wp[n0 + 3] : 0.0f;
            return v;
        });
    if (!col_ok) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = 32 * tr + acc_row(r, half);
        if (row < B) {
            const size_t at = (size_t)row * ldp + col;
            Gp[at] = acc[r] * act_grad(Yp[at], act_p);
        }
    }
}

// part[32 tk ..][32 tn ..] = sum over batch rows r0 <= r < r1 of A[r][.]^T G[r][.]: part is the slice's [K][N]
__device__ __forceinline__ void weight_grad_tile(const float* __restrict__ A, int64_t lda, const int* __restrict__ rows, int r0,
                                                 int r1, int K, const float* G, int ldg, int N,
                                                 float* __restrict__ part, int tk, int tn, int lane) {
    const int half = lane >> 5, li = lane & 31;
    const int kk = 32 * tk + li, col = 32 * tn + li;
    const bool kk_ok = kk < K, col_ok = col < N;
    const v16f acc = mma_chain((r1 - r0 + 31) / 32 * 4,
        [&](int s) {
            const int r = r0 + 8 * s + 4 * half;
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = 0.0f;
                if (kk_ok && r + j < r1) {
                    const int64_t src = rows ? rows[r + j] : r + j;
                    v[j] = A[src * lda + kk];
                }
            }
            return make_float4(v[0], v[1], v[2], v[3]);
        },
        [&](int s) {
            const int r = r0 + 8 * s + 4 * half;
            float4 v;
            v.x = col_ok && r + 0 < r1 ? G[(size_t)(r + 0) * ldg + col] : 0.0f;
            v.y = col_ok && r + 1 < r1 ? G[(size_t)(r + 1) * ldg + col] : 0.0f;
            v.z = col_ok && r + 2 < r1 ? G[(size_t)(r + 2) * ldg + col] : 0.0f;
            v.w = col_ok && r + 3 < r1 ? G[(size_t)(r + 3) * ldg + col] : 0.0f;
            return v;
        });
    if (!col_ok) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = 32 * tk + acc_row(r, half);
        if (row < K) part[(size_t)row * N + col] = acc[r];
    }
}

// the slice's db partial for columns 32 tn ..: lane-half h adds rows r0 + h, r0 + h + 2, ... in ascending order, then h = 0 + h = 1
__device__ __forceinline__ void bias_grad_tile(const float* G, int ldg, int r0, int r1, int N, float* __restrict__ part_b,
                                               int tn, int lane) {
    const int half = lane >> 5, col = 32 * tn + (lane & 31);
    float sum = 0.0f;
    if (col < N)
        for (int r = r0 + half; r < r1; r += 2) sum += G[(size_t)r * ldg + col];
    const float other = __shfl_xor(sum, 32, 64);
    if (half == 0 && col < N) part_b[col] = sum + other;
}

// One row of the last layer: its loss and the delta of its logits.  One wave; lane l takes columns l, l + 64, ... in ascending
// order and the 64 partial results meet in a butterfly, the same order for every row wherever it sits.
// kWeighted: the row counts w_r = row_w[row] times: scale_r = inv * w_r (one product) takes inv's place in the delta and the
// row's loss is stored as w_r * loss_r (one product).  Without it row_w is not read.
template <bool kWeighted>
__device__ __forceinline__ void loss_row(const float* z, float* g, int C, int loss,
                                         const void* __restrict__ targets, const float* __restrict__ row_w, int row, float inv,
                                         float* __restrict__ row_loss, int lane) {
    float w = 1.0f;
    if (kWeighted) {
        w = row_w[row];
        inv = inv * w;
    }
    if (loss == BD_TRAIN_CATEGORICAL) {
        const int label = reinterpret_cast<const int*>(targets)[row];
        float m = -INFINITY;
        for (int c = lane; c < C; c += 64) m = fmaxf(m, z[c]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        float sum = 0.0f;
        for (int c = lane; c < C; c += 64) sum += expf(z[c] - m);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        for (int c = lane; c < C; c += 64) g[c] = (expf(z[c] - m) / sum - (c == label ? 1.0f : 0.0f)) * inv;
        if (lane == 0) {
            const float l = (m + logf(sum)) - z[min(max(label, 0), C - 1)];
            row_loss[row] = kWeighted ? w * l : l;
        }
    } else {
        const float* t = reinterpret_cast<const float*>(targets) + (size_t)row * C;
        float sum = 0.0f;
        for (int c = lane; c < C; c += 64) {
            const float x = z[c], y = t[c];
            const float e = expf(-fabsf(x));
            sum += (fmaxf(x, 0.0f) - x * y) + log1pf(e);
            const float sig = x >= 0.0f ? 1.0f / (1.0f + e) : e / (1.0f + e);
            g[c] = (sig - y) * inv;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if (lane == 0) row_loss[row] = kWeighted ? w * sum : sum;
    }
}

// The sum of a batch's row losses, one workgroup of 256 threads: thread t adds rows t, t + 256, ... in ascending order (in
// double: the sum is not what limits the loss), then a fixed tree over part[256] (shared memory).  out[0] = the batch's mean
// loss; acc[0] += mean * B, acc[1] += B (the running sum of bd_trainer_mean_loss).  Every thread of the workgroup calls it.
__device__ __forceinline__ void loss_sum_block(const float* __restrict__ row_loss, int B, double scale, float* __restrict__ out,
                                               double* __restrict__ acc, double* part) {
    double sum = 0.0;
    for (int r = threadIdx.x; r < B; r += 256) sum += (double)row_loss[r];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double mean = part[0] * scale;
        if (out) out[0] = (float)mean;
        if (acc) {
            acc[0] += mean * B;
            acc[1] += B;
        }
    }
}

struct Update {
    int kind;
    float lr, b1, b2, eps;
    float lr_t;                     // Adam: lr sqrt(1 - b2^t) / (1 - b1^t) of this step
    float decay;                    // lr * weight_decay of this step, one float32 product; 0 = none
    int decay_n;                    // the leading elements it applies to: the layer's kernel, not the bias behind it
};

// p - decay * p in two roundings (no fused multiply-add: the host restates it as a product and a difference)
__device__ __forceinline__ float decayed(float p, float decay) {
#pragma clang fp contract(off)
    const float d = decay * p;
    return p - d;
}

// the slices' partials of one element in ascending order: ws points at slice 0's, the next slice's lies `stride` floats on
__device__ __forceinline__ float sum_partials(const float* __restrict__ ws, int slices, size_t stride) {
    float g = ws[0];
    for (int s = 1; s < slices; ++s) g += ws[(size_t)s * stride];
    return g;
}

// One element of a layer's [W | b], at index `at` of grad / P / m / v: its gradient g goes to grad, then the decay (`decays`: a
// kernel element, not a bias), then the optimizer's update.
__device__ __forceinline__ void apply_element(float g, size_t at, bool decays, float* __restrict__ grad, float* __restrict__ P,
                                              float* __restrict__ m, float* __restrict__ v, const Update& u) {
    grad[at] = g;
    float p = P[at];
    if (u.decay != 0.0f && decays) p = decayed(p, u.decay);
    if (u.kind == BD_TRAIN_ADAM) {
        const float mi = u.b1 * m[at] + (1.0f - u.b1) * g;
        const float vi = u.b2 * v[at] + (1.0f - u.b2) * (g * g);
        m[at] = mi;
        v[at] = vi;
        P[at] = p - u.lr_t * mi / (sqrtf(vi) + u.eps);
    } else {
        P[at] = __builtin_fmaf(-u.lr, g, p);             // p - lr g in one rounding, as it has always been compiled: spelled out so that
                                                         // the code around it cannot change the bits
    }
}

}  // namespace train
}  // namespace bd

#endif  // BD_HEADTRAIN_DEVICE_H
