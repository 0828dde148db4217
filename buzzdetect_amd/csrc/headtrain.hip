// The classifier-head trainer (include/buzzdetect_train.h): forward, loss, backward and update of a Dense stack on
// embeddings, in exact float32 on v_mfma_f32_32x32x2_f32.
//
// This file: the trainer's handle, its pool (a Dense stack's pieces as headtrain_host.h lays them out, then the workspace, the
// rows' losses and the running loss), its entry points and the one kernel that is the trainer's alone, fused_step_kernel.
// The layer-by-layer route - forward, rows' losses and their sum, weight gradient, input gradient, update: six kernels and
// their launches - is headtrain_stack.h's, shared with stackbank.hip: the trainer hands it its pool as a run of one member
// (run_of), so the lone trainer is a stack bank of one.  The device routines - mma_chain and the tiles built on it, loss_row,
// the partials' sum and the update - live in headtrain_device.h, and the host side the three training families share - the
// checks, the trainer's rate, decay, snapshot flag and step count (a MemberState of one member), the bias-corrected Adam
// rate, the stack's layout, the running loss and the workspace's test hooks - in headtrain_host.h; headbank.hip and
// stackbank.hip include both too.  The three matrix products differ in where a lane finds its operands:
//   forward  Y = act(A W + b)      reduce over n_in    A: 16 bytes of a row (row rows[r] of X for layer 0)   B: W[k][col]
//   dA       G' = (G W^T) * act'   reduce over n_out   A: 16 bytes of a row of G                             B: W[col][k]
//   dW       P_s = A^T G           reduce over the rows of slice s   A: A[row][col]                          B: G[row][col]
// The parameters stay row-major [n_in][n_out] + [n_out] (the update writes them every step; no fragment copy to keep in step).
//
// Order of sums (the determinism contract): an output element is one chain of fused multiply-adds in ascending k.  dW reduces
// over the batch: slice s is rows [256 s, 256 s + 256) - kSliceRows, a constant - its partial goes to workspace
// [slice][n_in n_out + n_out], and stack_apply_kernel adds the partials in ascending s before the optimizer's update.  Row losses go
// to a buffer and one workgroup adds them in a fixed tree.  Nothing depends on the grid or the number of compute units.
//
// fused_step_kernel (one layer, n_out <= 64): a workgroup of eight waves owns a slice and calls the route's three routines -
// logits of its 256 rows, their deltas, the slice's dW partial - so the partial's second walk over the slice's rows of X finds
// them in the cache the first walk filled: X comes from HBM once per step.
//
// Row weights (bd_trainer_step_weighted): loss_row<true> reads w_r beside the row's target and uses scale_r = inv * w_r where
// the plain pass uses inv, and stores w_r * loss_r; loss_row<false> is the plain pass, instruction for instruction.  The
// weight is a kernel argument, the same for every lane: no lane leaves or branches apart in front of the fused kernel's
// barriers.  Decoupled weight decay is stack_apply_kernel's: p = p - (lr wd) p on a layer's kernel elements (never its bias), two
// roundings, before the optimizer's update is subtracted from p.
#include "headtrain_device.h"
#include "headtrain_host.h"
#include "headtrain_stack.h"

namespace bd {
namespace {

// One layer of at most 64 outputs; grid = slices, eight waves.  Z / G [B][64].  Every wave reaches both barriers: the loops
// around them end on their bounds, and row_w changes what a row's pass computes, not which waves run it.
template <bool kWeighted>
__global__ __launch_bounds__(512) void fused_step_kernel(const float* __restrict__ X, int64_t ldx, const int* __restrict__ rows,
                                                           int B, int K, const float* __restrict__ P, int N, float* Z,
                                                           float* G, int ld, int loss,
                                                           const void* __restrict__ targets, const float* __restrict__ row_w,
                                                           float inv, float* __restrict__ row_loss, float* __restrict__ ws) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slice = blockIdx.x, r0 = slice * kSliceRows, r1 = min(B, r0 + kSliceRows);
    const int tiles_n = (N + 31) / 32;
    for (int t = wave; t < 8 * tiles_n; t += 8) {
        const int tr = r0 / 32 + (t & 7), tc = t >> 3;
        if (32 * tr < r1) forward_tile(X, ldx, rows, B, K, P, N, BD_HEAD_LINEAR, Z, ld, tr, tc, lane);
    }
    __syncthreads();                                     // the slice's logits, written above by this workgroup
    for (int row = r0 + wave; row < r1; row += 8)
        loss_row<kWeighted>(Z + (size_t)row * ld, G + (size_t)row * ld, N, loss, targets, row_w, row, inv, row_loss, lane);
    __syncthreads();                                     // the slice's deltas
    float* part = ws + (size_t)slice * ((size_t)K * N + N);
    const int tiles = (K + 31) / 32 * tiles_n;
    for (int t = wave; t < tiles; t += 8) {
        const int tk = t / tiles_n, tn = t % tiles_n;
        weight_grad_tile(X, ldx, rows, r0, r1, K, G, ld, N, part, tk, tn, lane);
        if (tk == 0) bias_grad_tile(G, ld, r0, r1, N, part + (size_t)K * N, tn, lane);
    }
}

}  // namespace
}  // namespace bd

struct bd_trainer_s : bd::TrainHandle {     // members: the one of this trainer (its rate, decay, snapshot flag and step count)
    bd::StackLayout s;              // offsets into pool
    bool fused = true;
    float* row_loss = nullptr;      // [max_batch]
    // ws: [slices][k n + n] of the layer at work
};

namespace bd {
namespace {

bool fusable(const bd_trainer_s* t) { return t->s.n_layers == 1 && t->s.layers[0].n <= BD_TRAIN_FUSED_MAX_WIDTH; }

// what every step and loss call checks, in this order
int check_call(const bd_trainer_s* t, const float* X, int64_t ldx, const void* targets, const float* row_w, int32_t B, const char* who) {
    if (!t || !X || !targets) return fail(BD_EINVAL, std::string(who) + ": null argument");
    const int rc = check_batch(who, t->max_batch, X, ldx, B);
    return rc < 0 ? rc : check_row_weights(who, row_w, B, B);
}

// the trainer's pool as a run of one member: no stride is ever multiplied by a member other than 0 (row weights likewise: one
// row of them, so the calls below give B for ldw)
StackRun run_of(const bd_trainer_s* t) { return {t->pool, 0, &t->s, t->ws, 0, t->row_loss, 0, t->acc, t->loss}; }

}  // namespace
}  // namespace bd

using bd::fail;

extern "C" {

int bd_train_abi_version(void) { return BD_TRAIN_ABI_VERSION; }

int bd_trainer_create(int device, const bd_head_layer* layers, int32_t n_layers, int32_t loss, const bd_train_optimizer* opt,
                      int32_t max_batch, bd_trainer* out) {
    const std::string who = "bd_trainer_create";
    if (!out || !layers || !opt) return fail(BD_EINVAL, who + ": null argument");
    *out = nullptr;
    if (n_layers < 1 || n_layers > BD_HEAD_MAX_LAYERS) return fail(BD_EINVAL, who + ": n_layers must be in 1..8");
    int rc = bd::check_training_setup(who, loss, opt, max_batch);
    if (rc == BD_OK) rc = bd::check_stack(who + ": layer ", layers, n_layers);
    if (rc == BD_OK) rc = bd::select_device(who, device);
    if (rc < 0) return rc;

    std::unique_ptr<bd_trainer_s> t(new bd_trainer_s);
    t->device = device;
    t->loss = loss;
    t->max_batch = max_batch;
    t->opt = *opt;
    t->members.assign(1, opt->learning_rate);
    t->s = bd::stack_layout(layers, n_layers, opt->kind == BD_TRAIN_ADAM, max_batch);
    // behind the layers: the workspace, the rows' losses, the running loss
    t->ws_floats = bd::slices_of(max_batch) * t->s.params_max;
    const int64_t off_ws = t->s.floats, off_rl = off_ws + bd::up64(t->ws_floats), off_acc = off_rl + bd::up64(max_batch);
    const int64_t total = off_acc + 64;
    BD_HIP(hipMalloc(&t->pool, (size_t)total * sizeof(float)));
    hipError_t err = hipMemset(t->pool, 0, (size_t)total * sizeof(float));
    if (err == hipSuccess) err = bd::upload_stack(t->pool, t->s, layers);
    if (err != hipSuccess) {
        (void)hipFree(t->pool);
        return fail(BD_EHIP, who + ": " + hipGetErrorString(err));
    }
    t->ws = t->pool + off_ws;
    t->row_loss = t->pool + off_rl;
    t->acc = reinterpret_cast<double*>(t->pool + off_acc);
    *out = t.release();
    return BD_OK;
}

int bd_trainer_destroy(bd_trainer t) { return bd::destroy(t); }

int bd_trainer_set_fusion(bd_trainer t, int32_t fused) {
    if (!t) return fail(BD_EINVAL, "bd_trainer_set_fusion: null handle");
    t->fused = fused != 0;
    return BD_OK;
}

// bd_trainer_step (row_w == nullptr: the plain kernels) and bd_trainer_step_weighted
static int do_step(bd_trainer t, const float* X, int64_t ldx, const int32_t* rows, const void* targets, const float* row_w, int32_t B,
                   void* stream_, const char* who) {
    int rc = bd::check_call(t, X, ldx, targets, row_w, B, who);
    if (rc < 0) return rc;
    hipStream_t stream;
    if ((rc = bd::enter(t, stream_, &stream)) < 0) return rc;
    t->members.advance();
    const bd::Members<1> a = t->members.launch_args<1>(t->opt, 0);
    const bd::StackRun r = bd::run_of(t);
    if (t->fused && bd::fusable(t)) {
        const bd::StackLayer& L = t->s.layers[0];
        const int slices = bd::slices_of(B);
        const float inv = bd::loss_inv(t->loss, B, L.n);
        float* pool = t->pool;
        if (row_w)
            hipLaunchKernelGGL(bd::fused_step_kernel<true>, dim3(slices), dim3(512), 0, stream, X, ldx, rows, B, L.k, pool + L.p, L.n,
                               pool + L.y, pool + L.g, L.ld, t->loss, targets, row_w, inv, t->row_loss, t->ws);
        else
            hipLaunchKernelGGL(bd::fused_step_kernel<false>, dim3(slices), dim3(512), 0, stream, X, ldx, rows, B, L.k, pool + L.p, L.n,
                               pool + L.y, pool + L.g, L.ld, t->loss, targets, row_w, inv, t->row_loss, t->ws);
        bd::stack_loss_sum(r, B, a, nullptr, true, stream);         // the rows' losses and the partials are the kernel's
        bd::stack_apply(r, t->opt, 0, slices, a, stream);
    } else {
        bd::stack_step(r, t->opt, X, ldx, rows, targets, row_w, B, B, a, stream);
    }
    BD_HIP(hipGetLastError());
    return BD_OK;
}

int bd_trainer_step(bd_trainer t, const float* X, int64_t ldx, const int32_t* rows, const void* targets, int32_t B, void* stream) {
    return do_step(t, X, ldx, rows, targets, nullptr, B, stream, "bd_trainer_step");
}

int bd_trainer_step_weighted(bd_trainer t, const float* X, int64_t ldx, const int32_t* rows, const void* targets,
                             const float* row_weights, int32_t B, void* stream) {
    return do_step(t, X, ldx, rows, targets, row_weights, B, stream, "bd_trainer_step_weighted");
}

static int do_loss(bd_trainer t, const float* X, int64_t ldx, const int32_t* rows, const void* targets, const float* row_w, int32_t B,
                   float* loss_dev, void* stream_, const char* who) {
    int rc = bd::check_call(t, X, ldx, targets, row_w, B, who);
    if (rc < 0) return rc;
    if (!loss_dev) return fail(BD_EINVAL, std::string(who) + ": null loss_dev");
    hipStream_t stream;
    if ((rc = bd::enter(t, stream_, &stream)) < 0) return rc;
    bd::stack_batch_loss(bd::run_of(t), X, ldx, rows, targets, row_w, B, B, bd::members_from<1>(1, 0), loss_dev, stream);
    BD_HIP(hipGetLastError());
    return BD_OK;
}

int bd_trainer_loss(bd_trainer t, const float* X, int64_t ldx, const int32_t* rows, const void* targets, int32_t B, float* loss_dev,
                    void* stream) {
    return do_loss(t, X, ldx, rows, targets, nullptr, B, loss_dev, stream, "bd_trainer_loss");
}

int bd_trainer_loss_weighted(bd_trainer t, const float* X, int64_t ldx, const int32_t* rows, const void* targets,
                             const float* row_weights, int32_t B, float* loss_dev, void* stream) {
    return do_loss(t, X, ldx, rows, targets, row_weights, B, loss_dev, stream, "bd_trainer_loss_weighted");
}

int bd_trainer_set_weight_decay(bd_trainer t, float weight_decay) {
    return bd::set_weight_decay(t, 0, weight_decay, "bd_trainer_set_weight_decay");
}

int bd_trainer_set_learning_rate(bd_trainer t, float learning_rate) {
    return bd::set_learning_rate(t, 0, learning_rate, "bd_trainer_set_learning_rate");
}

// parameters -> snapshot (to_snapshot) or back, on the caller's stream
static int copy_parameters(bd_trainer t, bool to_snapshot, void* stream_) {
    hipStream_t stream;
    const int rc = bd::enter(t, stream_, &stream);
    return rc < 0 ? rc : bd::copy_stack(t->pool, t->s, to_snapshot, stream);
}

int bd_trainer_snapshot(bd_trainer t, void* stream) {
    if (!t) return fail(BD_EINVAL, "bd_trainer_snapshot: null handle");
    const int rc = copy_parameters(t, true, stream);
    if (rc == BD_OK) t->members.has_snapshot[0] = 1;
    return rc;
}

int bd_trainer_restore(bd_trainer t, void* stream) {
    if (!t) return fail(BD_EINVAL, "bd_trainer_restore: null handle");
    if (!t->members.has_snapshot[0]) return fail(BD_EINVAL, "bd_trainer_restore: no snapshot was taken (bd_trainer_snapshot)");
    return copy_parameters(t, false, stream);
}

static int read_pair(bd_trainer t, int32_t layer, bool grad, float* w_host, float* b_host, const char* who) {
    if (!t || layer < 0 || layer >= t->s.n_layers) return fail(BD_EINVAL, std::string(who) + ": no such layer");
    return bd::read_stack_pair(t, t->pool, t->s.layers[layer], grad, w_host, b_host);
}

int bd_trainer_gradients(bd_trainer t, int32_t layer, float* dW_host, float* db_host) {
    return read_pair(t, layer, true, dW_host, db_host, "bd_trainer_gradients");
}

int bd_trainer_read(bd_trainer t, int32_t layer, float* kernel_host, float* bias_host) {
    return read_pair(t, layer, false, kernel_host, bias_host, "bd_trainer_read");
}

int bd_trainer_logits(bd_trainer t, int32_t B, float* logits_host) {
    if (!t || !logits_host || B < 1 || B > t->max_batch) return fail(BD_EINVAL, "bd_trainer_logits: bad argument");
    const int rc = bd::enter_and_wait(t);
    if (rc < 0) return rc;
    const bd::StackLayer& L = t->s.last();
    BD_HIP(hipMemcpy2D(logits_host, (size_t)L.n * sizeof(float), t->pool + L.y, (size_t)L.ld * sizeof(float),
                        (size_t)L.n * sizeof(float), B, hipMemcpyDeviceToHost));
    return BD_OK;
}

int bd_trainer_mean_loss(bd_trainer t, int32_t reset, float* mean_host) {
    return bd::mean_losses(t, reset, mean_host, "bd_trainer_mean_loss");
}

int64_t bd_trainer_workspace_floats(bd_trainer t) { return bd::workspace_floats(t, "bd_trainer_workspace_floats"); }

int bd_trainer_workspace_fill(bd_trainer t, uint32_t pattern) { return bd::workspace_fill(t, pattern, "bd_trainer_workspace_fill"); }

int bd_trainer_workspace_read(bd_trainer t, float* host, int64_t floats) {
    return bd::workspace_read(t, host, floats, "bd_trainer_workspace_read");
}

}  // extern "C"
