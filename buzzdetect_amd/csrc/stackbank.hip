// A bank of Dense stacks (include/buzzdetect_stackbank.h): M members of one shape - 1024 -> widths... -> C, the stacks
// bd_trainer_create takes - that share each step's rows of X, targets and batch order and differ in parameters, row weights,
// rate, decay and stopping.  Every kernel is headtrain.hip's layer-by-layer kernel with a member coordinate in the grid, and
// every product, row loss, partial sum and update is a call into headtrain_device.h: a member's element is the same chain of
// instructions as the lone trainer's, so its bits are the trainer's.
//
// Layout: member m's block lies at m x `stride` floats of one pool (stride a multiple of 64: the 16-byte row loads of
// forward_tile / input_grad_tile stay aligned); inside it, at offsets every member shares,
//   per layer   P, grad, (m, v,) snap   [k n + n] each: W then b, as the trainer keeps them
//   per layer   y, g                    [max_batch][round_up(n, 32)]: activations (the last: logits) and deltas
//   row_loss                            [max_batch]
// The slices' dW / db partials go to a workspace [member][slice][k n + n] of the layer at work, members `ws_stride` apart.
// A kernel gets member 0's pointers and adds member x stride in 64 bits.
//
// Grids: the member is blockIdx.x of the forward, weight-gradient and input-gradient kernels - the coordinate that varies
// fastest - so the workgroups that read the same rows of X (layer 0: every member reads the same gathered rows) are
// scheduled next to each other: the rows come from HBM once per step and from cache after that.
//
// A member's rate, bias-corrected rate, decay and frozen flag travel by value in the launch (Members), kMembersPerLaunch at
// a time: nothing a later bd_stackbank_set_* could overwrite before the step has run.  The workgroups of a frozen member
// return at once in the three backward kernels - the first statement, the same for every thread of the workgroup.
//
// This file: the stack bank's kernels, the members' blocks in its pool and the launches of its entry points.  The checks, the
// offsets of a stack's pieces inside a block (StackLayout: the lone trainer's too), Members and the members' state on the host
// (MemberState), the running losses and the workspace's test hooks are headtrain_host.h's, shared with headtrain.hip and
// headbank.hip.
#include "headtrain_device.h"
#include "headtrain_host.h"

#include "../../include/buzzdetect_stackbank.h"

namespace bd {
namespace {

// ---- kernels: member = first + the grid's member coordinate; A, P, Y, ... are member 0's ----

// grid (members, ceil(N / 64), ceil(B / 64)): four waves, a 32 x 32 tile each.  a_stride = 0: every member reads the same A (X).
__global__ __launch_bounds__(256) void stack_forward_kernel(const float* __restrict__ A, int64_t lda, int64_t a_stride,
                                                             const int* __restrict__ rows, int B, int K,
                                                             const float* __restrict__ P, int64_t p_stride, int N, int act,
                                                             float* __restrict__ Y, int64_t y_stride, int ldy, int first) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t member = first + (int)blockIdx.x;
    const int tr = 2 * blockIdx.z + (wave & 1), tc = 2 * blockIdx.y + (wave >> 1);
    if (32 * tr >= B || 32 * tc >= N) return;           // (no barrier in this kernel)
    forward_tile(A + member * a_stride, lda, rows, B, K, P + member * p_stride, N, act, Y + member * y_stride, ldy, tr, tc, lane);
}

// grid (ceil(B / 4), members): a wave per (row, member)
template <bool kWeighted>
__global__ __launch_bounds__(256) void stack_loss_rows_kernel(const float* __restrict__ Z, float* __restrict__ G, int64_t stride,
                                                               int ld, int B, int C, int loss, const void* __restrict__ targets,
                                                               const float* __restrict__ row_w, int64_t ldw, float inv,
                                                               float* __restrict__ row_loss, int first) {
    const int row = 4 * blockIdx.x + (threadIdx.x >> 6);
    const int64_t member = first + (int)blockIdx.y;
    if (row >= B) return;
    const int64_t at = member * stride + (int64_t)row * ld;
    loss_row<kWeighted>(Z + at, G + at, C, loss, targets, kWeighted ? row_w + member * ldw : nullptr, row, inv,
                        row_loss + member * stride, threadIdx.x & 63);
}

// grid (1, members): member's batch loss to out[member]; its running sum moves unless the member is frozen
__global__ __launch_bounds__(256) void stack_loss_sum_kernel(const float* __restrict__ row_loss, int64_t stride, int B, double scale,
                                                              float* __restrict__ out, double* __restrict__ acc, Members a) {
    __shared__ double part[256];
    const int64_t member = a.first + (int)blockIdx.y;
    loss_sum_block(row_loss + member * stride, B, scale, out ? out + member : nullptr,
                   acc && !a.frozen[blockIdx.y] ? acc + 2 * member : nullptr, part);
}

// grid (members, ceil(tiles / 4), slices): a wave per 32 x 32 tile of a slice's partial; the waves of the first row of tiles add db
__global__ __launch_bounds__(256) void stack_weight_grad_kernel(const float* __restrict__ A, int64_t lda, int64_t a_stride,
                                                                 const int* __restrict__ rows, int B, int K,
                                                                 const float* __restrict__ G, int64_t g_stride, int ldg, int N,
                                                                 float* __restrict__ ws, int64_t ws_stride, Members a) {
    if (a.frozen[blockIdx.x]) return;                    // the whole workgroup; no barrier in this kernel
    const int lane = threadIdx.x & 63;
    const int64_t member = a.first + (int)blockIdx.x;
    const int tiles_n = (N + 31) / 32, tiles = (K + 31) / 32 * tiles_n;
    const int t = 4 * blockIdx.y + (threadIdx.x >> 6);
    if (t >= tiles) return;
    const int slice = blockIdx.z, r0 = slice * kSliceRows, r1 = min(B, r0 + kSliceRows);
    float* part = ws + member * ws_stride + (size_t)slice * ((size_t)K * N + N);
    const int tk = t / tiles_n, tn = t % tiles_n;
    G += member * g_stride;
    weight_grad_tile(A + member * a_stride, lda, rows, r0, r1, K, G, ldg, N, part, tk, tn, lane);
    if (tk == 0) bias_grad_tile(G, ldg, r0, r1, N, part + (size_t)K * N, tn, lane);
}

// grid (members, ceil(K / 64), ceil(B / 64)); G, W, Yp and Gp lie in the members' blocks, `stride` apart
__global__ __launch_bounds__(256) void stack_input_grad_kernel(const float* __restrict__ G, int ldg, int B, int K,
                                                                const float* __restrict__ W, int N, const float* __restrict__ Yp,
                                                                int act_p, float* __restrict__ Gp, int ldp, int64_t stride, Members a) {
    if (a.frozen[blockIdx.x]) return;                    // the whole workgroup; no barrier in this kernel
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t off = (a.first + (int)blockIdx.x) * stride;
    const int tr = 2 * blockIdx.z + (wave & 1), tc = 2 * blockIdx.y + (wave >> 1);
    if (32 * tr >= B || 32 * tc >= K) return;
    input_grad_tile(G + off, ldg, B, K, W + off, N, Yp + off, act_p, Gp + off, ldp, tr, tc, lane);
}

// grid (ceil(n / 256), members): element i of the layer's [W | b] of member a.first + blockIdx.y
__global__ __launch_bounds__(256) void stack_apply_kernel(const float* __restrict__ ws, int64_t ws_stride, int slices, int n, int decay_n,
                                                           float* __restrict__ grad, float* __restrict__ P, float* __restrict__ m,
                                                           float* __restrict__ v, int64_t stride, int kind, float b1, float b2, float eps,
                                                           Members a) {
    const int j = blockIdx.y;
    if (a.frozen[j]) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t off = (a.first + j) * stride;
    const Update u{kind, a.lr[j], b1, b2, eps, a.lr_t[j], a.decay[j], decay_n};
    apply_element(sum_partials(ws + (a.first + j) * ws_stride + i, slices, (size_t)n), (size_t)i, i < decay_n, grad + off, P + off,
                  m ? m + off : nullptr, v ? v + off : nullptr, u);
}

}  // namespace
}  // namespace bd

struct bd_stackbank_s : bd::TrainHandle {
    int M = 0;
    bd::StackLayout s;              // offsets inside a member's block
    int64_t stride = 0;             // a member's block
    int64_t off_row_loss = 0;       // [max_batch] inside the block
    int64_t ws_stride = 0;          // ws: [M][ws_stride], [slice][k n + n] of the layer at work
};

namespace bd {
namespace {

// the forward pass of members a.first ..: the last layer's output goes to Y (member 0's, members y_stride apart, rows ldy
// apart) where given, else to the layer's own logits
void enqueue_forward(bd_stackbank_s* b, const float* X, int64_t ldx, const int* rows, int B, const Members& a, float* Y, int64_t y_stride,
                     int ldy, hipStream_t stream) {
    const float* src = X;
    int64_t lda = ldx, a_stride = 0;
    for (int l = 0; l < b->s.n_layers; ++l) {
        const StackLayer& L = b->s.layers[l];
        const bool last = l + 1 == b->s.n_layers;
        const bool outside = last && Y;
        hipLaunchKernelGGL(stack_forward_kernel, dim3(a.count, (L.n + 63) / 64, (B + 63) / 64), dim3(256), 0, stream, src, lda, a_stride,
                           l == 0 ? rows : nullptr, B, L.k, b->pool + L.p, b->stride, L.n, last ? BD_HEAD_LINEAR : L.act,
                           outside ? Y : b->pool + L.y, outside ? y_stride : b->stride, outside ? ldy : L.ld, a.first);
        src = b->pool + L.y;
        lda = L.ld;
        a_stride = b->stride;
    }
}

void enqueue_loss(bd_stackbank_s* b, const void* targets, const float* row_w, int64_t ldw, int B, float* loss_dev, bool accumulate,
                  const Members& a, hipStream_t stream) {
    const StackLayer& L = b->s.last();
    const float inv = loss_inv(b->loss, B, L.n);
    float* row_loss = b->pool + b->off_row_loss;
    if (row_w)
        hipLaunchKernelGGL(stack_loss_rows_kernel<true>, dim3((B + 3) / 4, a.count), dim3(256), 0, stream, b->pool + L.y, b->pool + L.g,
                           b->stride, L.ld, B, L.n, b->loss, targets, row_w, ldw, inv, row_loss, a.first);
    else
        hipLaunchKernelGGL(stack_loss_rows_kernel<false>, dim3((B + 3) / 4, a.count), dim3(256), 0, stream, b->pool + L.y, b->pool + L.g,
                           b->stride, L.ld, B, L.n, b->loss, targets, row_w, ldw, inv, row_loss, a.first);
    hipLaunchKernelGGL(stack_loss_sum_kernel, dim3(1, a.count), dim3(256), 0, stream, row_loss, b->stride, B, loss_scale(b->loss, B, L.n),
                       loss_dev, accumulate ? b->acc : nullptr, a);
}

// every layer of the member's parameters -> its snapshot (to_snapshot) or back, on the caller's stream
int copy_member(bd_stackbank_s* b, int32_t member, bool to_snapshot, void* stream_) {
    hipStream_t stream;
    const int rc = enter(b, stream_, &stream);
    return rc < 0 ? rc : copy_stack(b->pool + member * b->stride, b->s, to_snapshot, stream);
}

}  // namespace
}  // namespace bd

using bd::fail;

extern "C" {

int bd_stackbank_abi_version(void) { return BD_STACKBANK_ABI_VERSION; }

int bd_stackbank_create(int device, const bd_head_layer* layers, int32_t n_members, int32_t n_layers, int32_t loss,
                        const bd_train_optimizer* opt, int32_t max_batch, bd_stackbank* out) {
    const std::string who = "bd_stackbank_create";
    if (!out || !layers || !opt) return fail(BD_EINVAL, who + ": null argument");
    *out = nullptr;
    if (n_members < 1 || n_members > BD_BANK_MAX_MEMBERS) return fail(BD_EINVAL, who + ": the members must number 1..4096");
    if (n_layers < 1 || n_layers > BD_HEAD_MAX_LAYERS) return fail(BD_EINVAL, who + ": n_layers must be in 1..8");
    int rc = bd::check_training_setup(who, loss, opt, max_batch);
    for (int mb = 0; mb < n_members && rc == BD_OK; ++mb)
        rc = bd::check_stack(who + ": member " + std::to_string(mb) + ", layer ", layers + (size_t)mb * n_layers, n_layers, layers);
    if (rc < 0) return rc;
    std::unique_ptr<bd_stackbank_s> b(new bd_stackbank_s);
    // a member's block: its stack's pieces, then its rows' losses
    b->s = bd::stack_layout(layers, n_layers, opt->kind == BD_TRAIN_ADAM, max_batch);
    b->off_row_loss = b->s.floats;
    b->stride = b->off_row_loss + bd::up64(max_batch);
    b->ws_stride = bd::slices_of(max_batch) * bd::up64(b->s.params_max);
    b->ws_floats = b->ws_stride * n_members;
    const int64_t acc_floats = bd::up64(4 * (int64_t)n_members);
    const int64_t pool_floats = (b->stride + b->ws_stride) * n_members + acc_floats;
    if (pool_floats * (int64_t)sizeof(float) > BD_STACKBANK_MAX_WORKSPACE_BYTES) {
        std::string widths;
        for (int l = 0; l < n_layers; ++l) widths += (l ? ", " : "") + std::to_string(b->s.layers[l].n);
        return fail(BD_EWORKSPACE, who + ": " + std::to_string(n_members) + " members of widths " + widths + " at max_batch " +
                                       std::to_string(max_batch) + " need " + std::to_string(pool_floats * (int64_t)sizeof(float)) +
                                       " bytes, more than BD_STACKBANK_MAX_WORKSPACE_BYTES; use fewer members or a smaller max_batch");
    }
    if ((rc = bd::select_device(who, device)) < 0) return rc;

    b->device = device;
    b->loss = loss;
    b->M = n_members;
    b->max_batch = max_batch;
    b->opt = *opt;
    b->members.assign(n_members, opt->learning_rate);
    BD_HIP(hipMalloc(&b->pool, (size_t)pool_floats * sizeof(float)));
    b->ws = b->pool + b->stride * n_members;
    b->acc = reinterpret_cast<double*>(b->ws + b->ws_floats);
    hipError_t err = hipMemset(b->pool, 0, (size_t)pool_floats * sizeof(float));
    for (int mb = 0; mb < n_members && err == hipSuccess; ++mb)
        err = bd::upload_stack(b->pool + mb * b->stride, b->s, layers + (size_t)mb * n_layers);
    if (err != hipSuccess) {
        (void)hipFree(b->pool);
        return fail(BD_EHIP, who + ": " + hipGetErrorString(err));
    }
    *out = b.release();
    return BD_OK;
}

int bd_stackbank_destroy(bd_stackbank b) { return bd::destroy(b); }

int bd_stackbank_step(bd_stackbank b, const float* X, int64_t ldx, const int32_t* rows, const void* targets, const float* row_w,
                      int64_t ldw, int32_t B, void* stream_) {
    const char* who = "bd_stackbank_step";
    if (!b || !X || !targets) return fail(BD_EINVAL, std::string(who) + ": null argument");
    int rc = bd::check_batch(who, b->max_batch, X, ldx, B);
    if (rc == BD_OK) rc = bd::check_row_weights(who, row_w, ldw, B);
    if (rc < 0) return rc;
    hipStream_t stream;
    if ((rc = bd::enter(b, stream_, &stream)) < 0) return rc;
    const int slices = bd::slices_of(B);
    b->members.advance();
    float* pool = b->pool;
    for (int first = 0; first < b->M; first += bd::kMembersPerLaunch) {
        const bd::Members a = b->members.launch_args(b->opt, first);
        bd::enqueue_forward(b, X, ldx, rows, B, a, nullptr, 0, 0, stream);
        bd::enqueue_loss(b, targets, row_w, ldw, B, nullptr, true, a, stream);
        for (int l = b->s.n_layers - 1; l >= 0; --l) {
            const bd::StackLayer& L = b->s.layers[l];
            const int n = L.k * L.n + L.n;
            const int tiles = (L.k + 31) / 32 * ((L.n + 31) / 32);
            hipLaunchKernelGGL(bd::stack_weight_grad_kernel, dim3(a.count, (tiles + 3) / 4, slices), dim3(256), 0, stream,
                               l == 0 ? X : pool + b->s.layers[l - 1].y, l == 0 ? ldx : (int64_t)b->s.layers[l - 1].ld,
                               l == 0 ? (int64_t)0 : b->stride, l == 0 ? rows : nullptr, B, L.k, pool + L.g, b->stride, L.ld, L.n, b->ws,
                               b->ws_stride, a);
            if (l > 0) {                                 // with this layer's weights as the forward pass saw them
                const bd::StackLayer& Lp = b->s.layers[l - 1];
                hipLaunchKernelGGL(bd::stack_input_grad_kernel, dim3(a.count, (L.k + 63) / 64, (B + 63) / 64), dim3(256), 0, stream,
                                   pool + L.g, L.ld, B, L.k, pool + L.p, L.n, pool + Lp.y, Lp.act, pool + Lp.g, Lp.ld, b->stride, a);
            }
            hipLaunchKernelGGL(bd::stack_apply_kernel, dim3((n + 255) / 256, a.count), dim3(256), 0, stream, b->ws, b->ws_stride, slices, n,
                               L.k * L.n, pool + L.grad, pool + L.p, bd::slot(pool, L.m), bd::slot(pool, L.v), b->stride, b->opt.kind,
                               b->opt.beta_1, b->opt.beta_2, b->opt.epsilon, a);
        }
    }
    BD_HIP(hipGetLastError());
    return BD_OK;
}

int bd_stackbank_loss(bd_stackbank b, const float* X, int64_t ldx, const int32_t* rows, const void* targets, const float* row_w,
                      int64_t ldw, int32_t B, float* loss_dev, void* stream_) {
    const char* who = "bd_stackbank_loss";
    if (!b || !X || !targets || !loss_dev) return fail(BD_EINVAL, std::string(who) + ": null argument");
    int rc = bd::check_batch(who, b->max_batch, X, ldx, B);
    if (rc == BD_OK) rc = bd::check_row_weights(who, row_w, ldw, B);
    if (rc < 0) return rc;
    hipStream_t stream;
    if ((rc = bd::enter(b, stream_, &stream)) < 0) return rc;
    for (int first = 0; first < b->M; first += bd::kMembersPerLaunch) {
        const bd::Members a = bd::members_from(b->M, first);
        bd::enqueue_forward(b, X, ldx, rows, B, a, nullptr, 0, 0, stream);
        bd::enqueue_loss(b, targets, row_w, ldw, B, loss_dev, false, a, stream);
    }
    BD_HIP(hipGetLastError());
    return BD_OK;
}

int bd_stackbank_forward(bd_stackbank b, const float* X, int64_t ldx, const int32_t* rows, int32_t B, float* logits_dev, int64_t ldl,
                         void* stream_) {
    const char* who = "bd_stackbank_forward";
    if (!b || !X || !logits_dev) return fail(BD_EINVAL, std::string(who) + ": null argument");
    int rc = bd::check_batch(who, b->max_batch, X, ldx, B);
    if (rc < 0) return rc;
    const int C = b->s.last().n;
    if (ldl < (int64_t)b->M * C || ldl > INT32_MAX || (reinterpret_cast<uintptr_t>(logits_dev) & 3u))
        return fail(BD_EINVAL, std::string(who) + ": logits_dev must be float-aligned with ldl >= M C");
    hipStream_t stream;
    if ((rc = bd::enter(b, stream_, &stream)) < 0) return rc;
    for (int first = 0; first < b->M; first += bd::kMembersPerLaunch)
        bd::enqueue_forward(b, X, ldx, rows, B, bd::members_from(b->M, first), logits_dev, C, (int)ldl, stream);
    BD_HIP(hipGetLastError());
    return BD_OK;
}

int bd_stackbank_set_learning_rate(bd_stackbank b, int32_t member, float learning_rate) {
    return bd::set_learning_rate(b, member, learning_rate, "bd_stackbank_set_learning_rate");
}

int bd_stackbank_set_weight_decay(bd_stackbank b, int32_t member, float weight_decay) {
    return bd::set_weight_decay(b, member, weight_decay, "bd_stackbank_set_weight_decay");
}

int bd_stackbank_set_frozen(bd_stackbank b, int32_t member, int32_t frozen) {
    return bd::set_frozen(b, member, frozen, "bd_stackbank_set_frozen");
}

int bd_stackbank_snapshot(bd_stackbank b, int32_t member, void* stream) {
    return bd::snapshot_member(b, member, stream, "bd_stackbank_snapshot", bd::copy_member);
}

int bd_stackbank_restore(bd_stackbank b, int32_t member, void* stream) {
    return bd::restore_member(b, member, stream, "bd_stackbank_restore", "bd_stackbank_snapshot", bd::copy_member);
}

static int read_pair(bd_stackbank b, int32_t member, int32_t layer, bool grad, float* w_host, float* b_host, const char* who) {
    const int rc = bd::check_member(b, member, who);
    if (rc < 0) return rc;
    if (layer < 0 || layer >= b->s.n_layers) return fail(BD_EINVAL, std::string(who) + ": no such layer");
    return bd::read_stack_pair(b, b->pool + member * b->stride, b->s.layers[layer], grad, w_host, b_host);
}

int bd_stackbank_read(bd_stackbank b, int32_t member, int32_t layer, float* kernel_host, float* bias_host) {
    return read_pair(b, member, layer, false, kernel_host, bias_host, "bd_stackbank_read");
}

int bd_stackbank_gradients(bd_stackbank b, int32_t member, int32_t layer, float* dW_host, float* db_host) {
    return read_pair(b, member, layer, true, dW_host, db_host, "bd_stackbank_gradients");
}

int bd_stackbank_mean_loss(bd_stackbank b, int32_t reset, float* mean_host) {
    return bd::mean_losses(b, reset, mean_host, "bd_stackbank_mean_loss");
}

int64_t bd_stackbank_workspace_floats(bd_stackbank b) { return bd::workspace_floats(b, "bd_stackbank_workspace_floats"); }

int bd_stackbank_workspace_fill(bd_stackbank b, uint32_t pattern) { return bd::workspace_fill(b, pattern, "bd_stackbank_workspace_fill"); }

int bd_stackbank_workspace_read(bd_stackbank b, float* host, int64_t floats) {
    return bd::workspace_read(b, host, floats, "bd_stackbank_workspace_read");
}

}  // extern "C"
