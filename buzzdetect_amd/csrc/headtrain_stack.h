// The layer-by-layer training route of Dense stacks, written once: its six kernels and the launches built on them.
// headtrain.hip runs it with one member (bd_trainer_*: the lone trainer is a stack bank of one) and stackbank.hip with M
// (bd_stackbank_*); both include this file behind headtrain_device.h and headtrain_host.h.  Every product, row loss, partial
// sum and update is a call into headtrain_device.h, and there is one copy of every launch, so a member of a bank and the
// lone trainer do not merely run the same instructions: they run the same code.
//
// A run (StackRun) is members of one shape whose blocks lie `stride` floats apart; inside a block the pieces of the stack lie
// at the StackLayout's offsets.  The slices' dW / db partials of the layer at work go to ws [member][slice][k n + n], members
// `ws_stride` apart; the rows' losses to row_loss [member][max_batch], members `row_loss_stride` apart.  A launch gets the
// pointers of its first member from the host (StackRun::from); its kernels add (the grid's member coordinate) x stride in
// 64 bits.
//
// Grids: the member is blockIdx.x of the forward, weight-gradient and input-gradient kernels - the coordinate that varies
// fastest - so the workgroups that read the same rows of X (layer 0: every member reads the same gathered rows) are
// scheduled next to each other: the rows come from HBM once per step and from cache after that.
//
// A member's rate, bias-corrected rate, decay and frozen flag travel by value in the launch (Members), kMembersPerLaunch at
// a time: nothing a later bd_*_set_* could overwrite before the step has run.  The workgroups of a frozen member return at
// once in the three backward kernels - the first statement, the same for every thread of the workgroup.
//
// Every kernel is a template of Members' capacity: 64 for a bank's launches, 1 for a launch of exactly one member (the lone
// trainer, a bank of one, the last launch of 65 members).  A launch of one member carries what a kernel written for one stack
// would: no strides and no frozen flags (Stride<1> and Frozen<1> are empty types: the products fold to nothing, and the host
// does not make the backward launches of a frozen member, nor hand its running sum to the loss sum); only the update takes
// the member's rates.
#ifndef BD_HEADTRAIN_STACK_H
#define BD_HEADTRAIN_STACK_H

#include "headtrain_device.h"
#include "headtrain_host.h"

#include <type_traits>

namespace bd {
namespace {

// ---- between the members of a launch: the strides of their pieces and who is frozen; nothing for a launch of one member ----

template <int kCapacity>
struct Stride {
    int64_t floats;
    explicit Stride(int64_t f) : floats(f) {}
    __device__ int64_t operator*(int64_t member) const { return floats * member; }
};
template <>
struct Stride<1> {
    explicit Stride(int64_t) {}
    __device__ int64_t operator*(int64_t) const { return 0; }
};

template <int kCapacity>
struct Frozen {
    int flag[kCapacity];
    explicit Frozen(const Members<kCapacity>& a) { std::memcpy(flag, a.frozen, sizeof flag); }
    __device__ bool operator[](int j) const { return flag[j] != 0; }
};
template <>
struct Frozen<1> {                  // (the host asks frozen_alone and leaves the launch out)
    explicit Frozen(const Members<1>&) {}
    __device__ bool operator[](int) const { return false; }
};

// ---- kernels: member = the grid's member coordinate; A, P, Y, ... are those of the launch's first member ----

// grid (members, ceil(N / 64), ceil(B / 64)): four waves, a 32 x 32 tile each.  a_stride = 0: every member reads the same A (X).
template <int kCapacity>
__global__ __launch_bounds__(256) void stack_forward_kernel(const float* __restrict__ A, int64_t lda, const int* __restrict__ rows,
                                                             int B, int K, const float* __restrict__ P, int N, int act,
                                                             float* __restrict__ Y, int ldy, Stride<kCapacity> a_stride,
                                                             Stride<kCapacity> p_stride, Stride<kCapacity> y_stride) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t member = blockIdx.x;
    const int tr = 2 * blockIdx.z + (wave & 1), tc = 2 * blockIdx.y + (wave >> 1);
    if (32 * tr >= B || 32 * tc >= N) return;           // (no barrier in this kernel)
    forward_tile(A + a_stride * member, lda, rows, B, K, P + p_stride * member, N, act, Y + y_stride * member, ldy, tr, tc, lane);
}

// grid (ceil(B / 4), members): a wave per (row, member)
template <bool kWeighted, int kCapacity>
__global__ __launch_bounds__(256) void stack_loss_rows_kernel(const float* __restrict__ Z, float* __restrict__ G, int ld, int B, int C,
                                                               int loss, const void* __restrict__ targets,
                                                               const float* __restrict__ row_w, float inv,
                                                               float* __restrict__ row_loss, Stride<kCapacity> stride,
                                                               Stride<kCapacity> ldw, Stride<kCapacity> row_loss_stride) {
    const int row = 4 * blockIdx.x + (threadIdx.x >> 6);
    const int64_t member = blockIdx.y;
    if (row >= B) return;
    const int64_t at = stride * member + (int64_t)row * ld;
    loss_row<kWeighted>(Z + at, G + at, C, loss, targets, kWeighted ? row_w + ldw * member : nullptr, row, inv,
                        row_loss + row_loss_stride * member, threadIdx.x & 63);
}

// grid (1, members): member's batch loss to out[member]; its running sum moves unless the member is frozen
template <int kCapacity>
__global__ __launch_bounds__(256) void stack_loss_sum_kernel(const float* __restrict__ row_loss, int B, double scale,
                                                              float* __restrict__ out, double* __restrict__ acc,
                                                              Stride<kCapacity> stride, Frozen<kCapacity> frozen) {
    __shared__ double part[256];
    const int64_t member = blockIdx.y;
    loss_sum_block(row_loss + stride * member, B, scale, out ? out + member : nullptr,
                   acc && !frozen[blockIdx.y] ? acc + 2 * member : nullptr, part);
}

// grid (members, ceil(tiles / 4), slices): a wave per 32 x 32 tile of a slice's partial; the waves of the first row of tiles add db
template <int kCapacity>
__global__ __launch_bounds__(256) void stack_weight_grad_kernel(const float* __restrict__ A, int64_t lda, const int* __restrict__ rows,
                                                                 int B, int K, const float* __restrict__ G, int ldg, int N,
                                                                 float* __restrict__ ws, Stride<kCapacity> a_stride,
                                                                 Stride<kCapacity> g_stride, Stride<kCapacity> ws_stride,
                                                                 Frozen<kCapacity> frozen) {
    if (frozen[blockIdx.x]) return;                      // the whole workgroup; no barrier in this kernel
    const int lane = threadIdx.x & 63;
    const int64_t member = blockIdx.x;
    const int tiles_n = (N + 31) / 32, tiles = (K + 31) / 32 * tiles_n;
    const int t = 4 * blockIdx.y + (threadIdx.x >> 6);
    if (t >= tiles) return;
    const int slice = blockIdx.z, r0 = slice * kSliceRows, r1 = min(B, r0 + kSliceRows);
    float* part = ws + ws_stride * member + (size_t)slice * ((size_t)K * N + N);
    const int tk = t / tiles_n, tn = t % tiles_n;
    G += g_stride * member;
    weight_grad_tile(A + a_stride * member, lda, rows, r0, r1, K, G, ldg, N, part, tk, tn, lane);
    if (tk == 0) bias_grad_tile(G, ldg, r0, r1, N, part + (size_t)K * N, tn, lane);
}

// grid (members, ceil(K / 64), ceil(B / 64)); G, W, Yp and Gp lie in the members' blocks, `stride` apart
template <int kCapacity>
__global__ __launch_bounds__(256) void stack_input_grad_kernel(const float* __restrict__ G, int ldg, int B, int K,
                                                                const float* __restrict__ W, int N, const float* __restrict__ Yp,
                                                                int act_p, float* __restrict__ Gp, int ldp,
                                                                Stride<kCapacity> stride, Frozen<kCapacity> frozen) {
    if (frozen[blockIdx.x]) return;                      // the whole workgroup; no barrier in this kernel
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t off = stride * (int64_t)blockIdx.x;
    const int tr = 2 * blockIdx.z + (wave & 1), tc = 2 * blockIdx.y + (wave >> 1);
    if (32 * tr >= B || 32 * tc >= K) return;
    input_grad_tile(G + off, ldg, B, K, W + off, N, Yp + off, act_p, Gp + off, ldp, tr, tc, lane);
}

// grid (ceil(n / 256), members): element i of the layer's [W | b] of member blockIdx.y: the slices' partials in
// ascending order, then the decay (kernel elements only), then the optimizer
template <int kCapacity>
__global__ __launch_bounds__(256) void stack_apply_kernel(const float* __restrict__ ws, int slices, int n, int decay_n,
                                                           float* __restrict__ grad, float* __restrict__ P, float* __restrict__ m,
                                                           float* __restrict__ v, int kind, float b1, float b2, float eps,
                                                           Stride<kCapacity> ws_stride, Stride<kCapacity> stride,
                                                           Members<kCapacity> a) {
    const int j = blockIdx.y;
    if (a.frozen[j]) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t off = stride * (int64_t)j;
    const Update u{kind, a.lr[j], b1, b2, eps, a.lr_t[j], a.decay[j], decay_n};
    apply_element(sum_partials(ws + ws_stride * (int64_t)j + i, slices, (size_t)n), (size_t)i, i < decay_n, grad + off, P + off,
                  m ? m + off : nullptr, v ? v + off : nullptr, u);
}

// ---- where a run's pieces lie ----

struct StackRun {
    float* block;                   // member 0's block: the layout's offsets count from here
    int64_t stride;                 // from a member's block to the next member's
    const StackLayout* s;
    float* ws;                      // member 0's [slice][k n + n] of the layer at work
    int64_t ws_stride;
    float* row_loss;                // member 0's [max_batch]
    int64_t row_loss_stride;
    double* acc;                    // [members][2]
    int loss;

    // the run whose member 0 is this run's `member`
    StackRun from(int member) const {
        return {block + member * stride, stride, s, ws + member * ws_stride, ws_stride, row_loss + member * row_loss_stride,
                row_loss_stride, acc + 2 * member, loss};
    }
};

// a launch of exactly one member whose member is frozen: its backward launches are not made, its running sum not handed on
template <int kCapacity>
bool frozen_alone(const Members<kCapacity>& a) { return kCapacity == 1 && a.frozen[0]; }

// f(first, capacity) for every launch of M members, kMembersPerLaunch at a time; capacity is a std::integral_constant: 1 for a
// launch of exactly one member, kMembersPerLaunch otherwise
template <class F>
void for_each_launch(int M, F f) {
    for (int first = 0; first < M; first += kMembersPerLaunch) {
        if (M - first == 1)
            f(first, std::integral_constant<int, 1>());
        else
            f(first, std::integral_constant<int, kMembersPerLaunch>());
    }
}

// ---- the launches, of the members `a` names ----

// the forward pass: the last layer's output goes to Y (member 0's, members y_stride apart, rows ldy apart) where given, else
// to the layer's own logits
template <int kCapacity>
void stack_forward(const StackRun& run, const float* X, int64_t ldx, const int* rows, int B, const Members<kCapacity>& a, float* Y,
                   int64_t y_stride, int ldy, hipStream_t stream) {
    const StackRun r = run.from(a.first);
    const float* src = X;
    int64_t lda = ldx, a_stride = 0;
    for (int l = 0; l < r.s->n_layers; ++l) {
        const StackLayer& L = r.s->layers[l];
        const bool last = l + 1 == r.s->n_layers;
        const bool outside = last && Y;
        hipLaunchKernelGGL(stack_forward_kernel<kCapacity>, dim3(a.count, (L.n + 63) / 64, (B + 63) / 64), dim3(256), 0, stream, src,
                           lda, l == 0 ? rows : nullptr, B, L.k, r.block + L.p, L.n, last ? BD_HEAD_LINEAR : L.act,
                           outside ? Y + a.first * y_stride : r.block + L.y, outside ? ldy : L.ld,
                           Stride<kCapacity>(a_stride), Stride<kCapacity>(r.stride), Stride<kCapacity>(outside ? y_stride : r.stride));
        src = r.block + L.y;
        lda = L.ld;
        a_stride = r.stride;
    }
}

// the rows' losses and the deltas of the logits; row_w: nullptr or the members' rows of weights, ldw apart
template <int kCapacity>
void stack_loss_rows(const StackRun& run, const void* targets, const float* row_w, int64_t ldw, int B, const Members<kCapacity>& a,
                     hipStream_t stream) {
    const StackRun r = run.from(a.first);
    const StackLayer& L = r.s->last();
    const float inv = loss_inv(r.loss, B, L.n);
    const Stride<kCapacity> stride(r.stride), w_stride(ldw), l_stride(r.row_loss_stride);
    if (row_w)
        hipLaunchKernelGGL((stack_loss_rows_kernel<true, kCapacity>), dim3((B + 3) / 4, a.count), dim3(256), 0, stream, r.block + L.y,
                           r.block + L.g, L.ld, B, L.n, r.loss, targets, row_w + a.first * ldw, inv, r.row_loss, stride, w_stride,
                           l_stride);
    else
        hipLaunchKernelGGL((stack_loss_rows_kernel<false, kCapacity>), dim3((B + 3) / 4, a.count), dim3(256), 0, stream, r.block + L.y,
                           r.block + L.g, L.ld, B, L.n, r.loss, targets, row_w, inv, r.row_loss, stride, w_stride, l_stride);
}

// the sum of the rows' losses, wherever they came from (stack_loss_rows, or the trainer's fused kernel): the batch loss to
// loss_dev[member] where given, and into the running sums if `accumulate`
template <int kCapacity>
void stack_loss_sum(const StackRun& run, int B, const Members<kCapacity>& a, float* loss_dev, bool accumulate, hipStream_t stream) {
    const StackRun r = run.from(a.first);
    hipLaunchKernelGGL(stack_loss_sum_kernel<kCapacity>, dim3(1, a.count), dim3(256), 0, stream, r.row_loss, B,
                       loss_scale(r.loss, B, r.s->last().n), loss_dev ? loss_dev + a.first : nullptr,
                       accumulate && !frozen_alone(a) ? r.acc : nullptr, Stride<kCapacity>(r.row_loss_stride), Frozen<kCapacity>(a));
}

// layer l's update from the partials in ws
template <int kCapacity>
void stack_apply(const StackRun& run, const bd_train_optimizer& opt, int l, int slices, const Members<kCapacity>& a, hipStream_t stream) {
    const StackRun r = run.from(a.first);
    const StackLayer& L = r.s->layers[l];
    const int n = L.k * L.n + L.n;
    hipLaunchKernelGGL(stack_apply_kernel<kCapacity>, dim3((n + 255) / 256, a.count), dim3(256), 0, stream, r.ws, slices, n, L.k * L.n,
                       r.block + L.grad, r.block + L.p, slot(r.block, L.m), slot(r.block, L.v), opt.kind, opt.beta_1, opt.beta_2,
                       opt.epsilon, Stride<kCapacity>(r.ws_stride), Stride<kCapacity>(r.stride), a);
}

// from the deltas of the logits back to layer 0: a layer's partials, the deltas of the layer before it, its update
template <int kCapacity>
void stack_backward(const StackRun& run, const bd_train_optimizer& opt, const float* X, int64_t ldx, const int* rows, int B,
                    const Members<kCapacity>& a, hipStream_t stream) {
    if (frozen_alone(a)) return;
    const StackRun r = run.from(a.first);
    const Stride<kCapacity> stride(r.stride);
    const Frozen<kCapacity> frozen(a);
    const int slices = slices_of(B);
    float* pool = r.block;
    for (int l = r.s->n_layers - 1; l >= 0; --l) {
        const StackLayer& L = r.s->layers[l];
        const int tiles = (L.k + 31) / 32 * ((L.n + 31) / 32);
        hipLaunchKernelGGL(stack_weight_grad_kernel<kCapacity>, dim3(a.count, (tiles + 3) / 4, slices), dim3(256), 0, stream,
                           l == 0 ? X : pool + r.s->layers[l - 1].y, l == 0 ? ldx : (int64_t)r.s->layers[l - 1].ld,
                           l == 0 ? rows : nullptr, B, L.k, pool + L.g, L.ld, L.n, r.ws, Stride<kCapacity>(l == 0 ? 0 : r.stride),
                           stride, Stride<kCapacity>(r.ws_stride), frozen);
        if (l > 0) {                                     // with this layer's weights as the forward pass saw them
            const StackLayer& Lp = r.s->layers[l - 1];
            hipLaunchKernelGGL(stack_input_grad_kernel<kCapacity>, dim3(a.count, (L.k + 63) / 64, (B + 63) / 64), dim3(256), 0, stream,
                               pool + L.g, L.ld, B, L.k, pool + L.p, L.n, pool + Lp.y, Lp.act, pool + Lp.g, Lp.ld, stride, frozen);
        }
        stack_apply(run, opt, l, slices, a, stream);
    }
}

// one step of the members `a` names: forward, loss (into the running sums), backward, update
template <int kCapacity>
void stack_step(const StackRun& r, const bd_train_optimizer& opt, const float* X, int64_t ldx, const int* rows, const void* targets,
                const float* row_w, int64_t ldw, int B, const Members<kCapacity>& a, hipStream_t stream) {
    stack_forward(r, X, ldx, rows, B, a, nullptr, 0, 0, stream);
    stack_loss_rows(r, targets, row_w, ldw, B, a, stream);
    stack_loss_sum(r, B, a, nullptr, true, stream);
    stack_backward(r, opt, X, ldx, rows, B, a, stream);
}

// the batch loss of the members `a` names to loss_dev[member]: nothing but the activations, deltas and rows' losses moves
template <int kCapacity>
void stack_batch_loss(const StackRun& r, const float* X, int64_t ldx, const int* rows, const void* targets, const float* row_w,
                      int64_t ldw, int B, const Members<kCapacity>& a, float* loss_dev, hipStream_t stream) {
    stack_forward(r, X, ldx, rows, B, a, nullptr, 0, 0, stream);
    stack_loss_rows(r, targets, row_w, ldw, B, a, stream);
    stack_loss_sum(r, B, a, loss_dev, false, stream);
}

}  // namespace
}  // namespace bd

#endif  // BD_HEADTRAIN_STACK_H
