// A bank of Dense stacks (include/buzzdetect_stackbank.h): M members of one shape - 1024 -> widths... -> C, the stacks
// bd_trainer_create takes - that share each step's rows of X, targets and batch order and differ in parameters, row weights,
// rate, decay and stopping.  Its kernels and their launches are headtrain_stack.h's, the one layer-by-layer training route:
// bd_trainer_* runs it with one member, this file with M, so a member's bits are the lone trainer's.
//
// Layout: member m's block lies at m x `stride` floats of one pool (stride a multiple of 64: the 16-byte row loads of
// forward_tile / input_grad_tile stay aligned); inside it, at offsets every member shares,
//   per layer   P, grad, (m, v,) snap   [k n + n] each: W then b, as the trainer keeps them
//   per layer   y, g                    [max_batch][round_up(n, 32)]: activations (the last: logits) and deltas
//   row_loss                            [max_batch]
// The slices' dW / db partials go to a workspace [member][slice][k n + n] of the layer at work, members `ws_stride` apart.
//
// The members run kMembersPerLaunch at a time; a launch of exactly one member (a bank of one, the 65th of 65) takes the
// route's one-member argument block, as the lone trainer does.
//
// This file: the stack bank's handle, the members' blocks in its pool (run_of: what the shared route needs to know of them)
// and its entry points.  The checks, the offsets of a stack's pieces inside a block (StackLayout: the lone trainer's too),
// Members and the members' state on the host (MemberState), the running losses and the workspace's test hooks are
// headtrain_host.h's, shared with headtrain.hip and headbank.hip.
#include "headtrain_device.h"
#include "headtrain_host.h"
#include "headtrain_stack.h"

#include "../../include/buzzdetect_stackbank.h"

struct bd_stackbank_s : bd::TrainHandle {
    int M = 0;
    bd::StackLayout s;              // offsets inside a member's block
    int64_t stride = 0;             // a member's block
    int64_t off_row_loss = 0;       // [max_batch] inside the block
    int64_t ws_stride = 0;          // ws: [M][ws_stride], [slice][k n + n] of the layer at work
};

namespace bd {
namespace {

StackRun run_of(const bd_stackbank_s* b) {
    return {b->pool, b->stride, &b->s, b->ws, b->ws_stride, b->pool + b->off_row_loss, b->stride, b->acc, b->loss};
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
    b->members.advance();
    const bd::StackRun r = bd::run_of(b);
    bd::for_each_launch(b->M, [&](int first, auto capacity) {
        constexpr int kCapacity = decltype(capacity)::value;
        bd::stack_step(r, b->opt, X, ldx, rows, targets, row_w, ldw, B, b->members.launch_args<kCapacity>(b->opt, first), stream);
    });
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
    const bd::StackRun r = bd::run_of(b);
    bd::for_each_launch(b->M, [&](int first, auto capacity) {
        constexpr int kCapacity = decltype(capacity)::value;
        bd::stack_batch_loss(r, X, ldx, rows, targets, row_w, ldw, B, bd::members_from<kCapacity>(b->M, first), loss_dev, stream);
    });
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
    const bd::StackRun r = bd::run_of(b);
    bd::for_each_launch(b->M, [&](int first, auto capacity) {
        constexpr int kCapacity = decltype(capacity)::value;
        bd::stack_forward(r, X, ldx, rows, B, bd::members_from<kCapacity>(b->M, first), logits_dev, C, (int)ldl, stream);
    });
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
