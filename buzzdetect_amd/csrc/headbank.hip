// A bank of one-layer classifier heads (include/buzzdetect_bank.h): M members 1024 -> C that share each step's rows of X,
// targets and batch order and differ in row weights, rate, decay and stopping - the folds of a cross-validation, the entries of
// a sweep.  Every product, row loss, partial sum and update is a call into headtrain_device.h, the routines headtrain.hip's
// kernels call: a member's element is the same chain of instructions as the lone trainer's, so its bits are the trainer's.
//
// Layout: members are packed into groups of kGroupCols = 64 columns, mpg = 64 / C whole members per group; group g holds
// members g mpg .. and is ng = (members in it) x C columns wide - the last group may be narrower, and columns past ng do not
// exist for any routine (they are the `col < N` compares of the tiles).  Per group, at a fixed stride of kGroupFloats:
//   P, grad, m, v, snap   row-major [1025][ng]: W then the bias as row 1024, member j of the group in columns j C .. j C + C
//   Z, G                  [max_batch][64]: the group's logits and deltas
//   ws                    [slice][group][1025][ng]: the slices' dW / db partials
//
// bank_step_kernel, grid (slices, groups), is fused_step_kernel per group: forward tiles of the slice's rows over the group's
// columns, loss_row per (row, member of the group) on that member's C columns with that member's weight, then the slice's dW
// and db partial.  The groups of a slice read the same rows of X: they come from HBM once per step for the whole bank.
// bank_apply_kernel adds an element's partials in ascending slice order and applies its member's decay and update; a frozen
// member's workgroups return at once.  A member's rate, bias-corrected rate, decay and frozen flag travel by value in the
// launch (Members), kMembersPerLaunch at a time: nothing a later bd_bank_set_* could overwrite before the step has run.
//
// This file: the bank's kernels, Shape and the group layout of its pool, and the launches of its entry points.  The checks,
// Members and the members' state on the host (MemberState: the validated setters, the step counts, the launch arguments with
// the bias-corrected Adam rate), the running losses and the workspace's test hooks are headtrain_host.h's, shared with
// headtrain.hip and stackbank.hip.
#include "headtrain_device.h"
#include "headtrain_host.h"

#include "../../include/buzzdetect_bank.h"

namespace bd {
namespace {

constexpr int kGroupCols = BD_BANK_GROUP_COLUMNS;
constexpr int kIn = BD_EMBEDDING_SIZE;
constexpr int64_t kGroupFloats = (int64_t)(kIn + 1) * kGroupCols;      // stride of a group's [1025][ng] block
static_assert(kGroupCols == BD_TRAIN_FUSED_MAX_WIDTH && kGroupCols % 32 == 0, "a group is the fused kernel's two column tiles");

struct Shape {
    int M, C, mpg, groups;          // mpg: members per group
    int max_batch;
};

__device__ __forceinline__ int group_width(const Shape& s, int group) { return min(s.mpg, s.M - group * s.mpg) * s.C; }

// grid (ceil(B / 64), groups): four waves, a 32 x 32 tile each.  Y + group y_stride is the group's [B][ldy] output.
__global__ __launch_bounds__(256) void bank_forward_kernel(const float* __restrict__ X, int64_t ldx, const int* __restrict__ rows,
                                                            int B, const float* __restrict__ P, Shape s, float* __restrict__ Y,
                                                            int64_t y_stride, int ldy) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int group = blockIdx.y, ng = group_width(s, group);
    const int tr = 2 * blockIdx.x + (wave & 1), tc = wave >> 1;
    if (32 * tr >= B || 32 * tc >= ng) return;          // (no barrier in this kernel)
    forward_tile(X, ldx, rows, B, kIn, P + group * kGroupFloats, ng, BD_HEAD_LINEAR, Y + group * y_stride, ldy, tr, tc, lane);
}

// grid (ceil(B / 4), M): a wave per (row, member)
template <bool kWeighted>
__global__ __launch_bounds__(256) void bank_loss_rows_kernel(const float* __restrict__ Z, float* __restrict__ G, int B, Shape s,
                                                              int loss, const void* __restrict__ targets,
                                                              const float* __restrict__ row_w, int64_t ldw, float inv,
                                                              float* __restrict__ row_loss) {
    const int row = 4 * blockIdx.x + (threadIdx.x >> 6), member = blockIdx.y;
    if (row >= B) return;
    const size_t at = ((size_t)(member / s.mpg) * s.max_batch + row) * kGroupCols + (member % s.mpg) * s.C;
    loss_row<kWeighted>(Z + at, G + at, s.C, loss, targets, kWeighted ? row_w + (size_t)member * ldw : nullptr, row, inv,
                        row_loss + (size_t)member * s.max_batch, threadIdx.x & 63);
}

// grid (slices, groups), eight waves: fused_step_kernel on the group's columns.  Every wave reaches both barriers: the loops
// around them end on their bounds.
template <bool kWeighted>
__global__ __launch_bounds__(512) void bank_step_kernel(const float* __restrict__ X, int64_t ldx, const int* __restrict__ rows, int B,
                                                          const float* __restrict__ P, Shape s, float* Z, float* G, int loss,
                                                          const void* __restrict__ targets, const float* __restrict__ row_w,
                                                          int64_t ldw, float inv, float* __restrict__ row_loss,
                                                          float* __restrict__ ws) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slice = blockIdx.x, r0 = slice * kSliceRows, r1 = min(B, r0 + kSliceRows);
    const int group = blockIdx.y, first = group * s.mpg, nm = min(s.mpg, s.M - first), ng = nm * s.C;
    const int tiles_n = (ng + 31) / 32;
    P += group * kGroupFloats;
    Z += (size_t)group * s.max_batch * kGroupCols;
    G += (size_t)group * s.max_batch * kGroupCols;
    for (int t = wave; t < 8 * tiles_n; t += 8) {
        const int tr = r0 / 32 + (t & 7), tc = t >> 3;
        if (32 * tr < r1) forward_tile(X, ldx, rows, B, kIn, P, ng, BD_HEAD_LINEAR, Z, kGroupCols, tr, tc, lane);
    }
    __syncthreads();                                     // the slice's logits, written above by this workgroup
    for (int row = r0 + wave; row < r1; row += 8)
        for (int j = 0; j < nm; ++j) {
            const size_t at = (size_t)row * kGroupCols + j * s.C;
            loss_row<kWeighted>(Z + at, G + at, s.C, loss, targets, kWeighted ? row_w + (size_t)(first + j) * ldw : nullptr, row, inv,
                                row_loss + (size_t)(first + j) * s.max_batch, lane);
        }
    __syncthreads();                                     // the slice's deltas
    float* part = ws + ((size_t)slice * s.groups + group) * kGroupFloats;
    const int tiles = kIn / 32 * tiles_n;
    for (int t = wave; t < tiles; t += 8) {
        const int tk = t / tiles_n, tn = t % tiles_n;
        weight_grad_tile(X, ldx, rows, r0, r1, kIn, G, kGroupCols, ng, part, tk, tn, lane);
        if (tk == 0) bias_grad_tile(G, kGroupCols, r0, r1, ng, part + (size_t)kIn * ng, tn, lane);
    }
}

// grid (a.count): member a.first + blockIdx.x's batch loss to out[member]; its running sum moves unless the member is frozen
__global__ __launch_bounds__(256) void bank_loss_sum_kernel(const float* __restrict__ row_loss, int B, int max_batch, double scale,
                                                             float* __restrict__ out, double* __restrict__ acc,
                                                             Members<kMembersPerLaunch> a) {
    __shared__ double part[256];
    const int member = a.first + blockIdx.x;
    loss_sum_block(row_loss + (size_t)member * max_batch, B, scale, out ? out + member : nullptr,
                   acc && !a.frozen[blockIdx.x] ? acc + 2 * (size_t)member : nullptr, part);
}

// grid (ceil((1024 C + C) / 256), a.count): element i = k C + c of member a.first + blockIdx.y's [W | b]
__global__ __launch_bounds__(256) void bank_apply_kernel(const float* __restrict__ ws, int slices, Shape s, float* __restrict__ grad,
                                                          float* __restrict__ P, float* __restrict__ m, float* __restrict__ v,
                                                          int kind, float b1, float b2, float eps, Members<kMembersPerLaunch> a) {
    const int j = blockIdx.y, member = a.first + j;
    if (a.frozen[j]) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (kIn + 1) * s.C) return;
    const int k = i / s.C, c = i - k * s.C;
    const int group = member / s.mpg, ng = group_width(s, group);
    const size_t at = (size_t)group * kGroupFloats + (size_t)k * ng + (member % s.mpg) * s.C + c;
    const Update u{kind, a.lr[j], b1, b2, eps, a.lr_t[j], a.decay[j], 0};
    apply_element(sum_partials(ws + at, slices, (size_t)s.groups * kGroupFloats), at, k < kIn, grad, P, m, v, u);
}

// a member's [1025][C] columns of one group block to the same place of another (snapshot and back)
__global__ __launch_bounds__(256) void bank_copy_member_kernel(float* __restrict__ dst, const float* __restrict__ src, int C, int ng,
                                                                int col0) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (kIn + 1) * C) return;
    const int k = i / C, c = i - k * C;
    const size_t at = (size_t)k * ng + col0 + c;
    dst[at] = src[at];
}

}  // namespace
}  // namespace bd

struct bd_bank_s : bd::TrainHandle {
    bd::Shape s{};
    float *p = nullptr, *grad = nullptr, *m = nullptr, *v = nullptr, *snap = nullptr;      // [groups][kGroupFloats]
    float *z = nullptr, *g = nullptr;                                                      // [groups][max_batch][64]
    float* row_loss = nullptr;      // [M][max_batch]
    // ws: [slices of max_batch][groups][kGroupFloats]
};

namespace bd {
namespace {

// where member's columns begin in its group's block, and how many columns that block has (the host's group_width)
struct Columns {
    int64_t block;                  // the group's block in p, grad, m, v, snap
    int ng, col0;
};

Columns columns_of(const Shape& s, int member) {
    const int group = member / s.mpg;
    return {group * kGroupFloats, (s.mpg < s.M - group * s.mpg ? s.mpg : s.M - group * s.mpg) * s.C, (member % s.mpg) * s.C};
}

// member's columns of the parameters -> its columns of the snapshot (to_snapshot) or back, on the caller's stream
int copy_member(bd_bank_s* b, int32_t member, bool to_snapshot, void* stream_) {
    hipStream_t stream;
    const int rc = enter(b, stream_, &stream);
    if (rc < 0) return rc;
    const Columns c = columns_of(b->s, member);
    float *p = b->p + c.block, *snap = b->snap + c.block;
    hipLaunchKernelGGL(bank_copy_member_kernel, dim3(((kIn + 1) * b->s.C + 255) / 256), dim3(256), 0, stream, to_snapshot ? snap : p,
                       to_snapshot ? p : snap, b->s.C, c.ng, c.col0);
    BD_HIP(hipGetLastError());
    return BD_OK;
}

}  // namespace
}  // namespace bd

using bd::fail;

extern "C" {

int bd_bank_abi_version(void) { return BD_BANK_ABI_VERSION; }

int bd_bank_create(int device, const bd_head_layer* layers, int32_t n_members, int32_t loss, const bd_train_optimizer* opt,
                   int32_t max_batch, bd_bank* out) {
    const std::string who = "bd_bank_create";
    if (!out || !layers || !opt) return fail(BD_EINVAL, who + ": null argument");
    *out = nullptr;
    if (n_members < 1 || n_members > BD_BANK_MAX_MEMBERS) return fail(BD_EINVAL, who + ": the members must number 1..4096");
    int rc = bd::check_training_setup(who, loss, opt, max_batch);
    if (rc < 0) return rc;
    const int C = layers[0].n_out;
    if (C < 1 || C > BD_TRAIN_FUSED_MAX_WIDTH) return fail(BD_EINVAL, who + ": n_out must be in 1..64 (a bank holds one-layer heads of the fused width)");
    for (int mb = 0; mb < n_members; ++mb) {
        const std::string where = who + ": member " + std::to_string(mb);
        if (!layers[mb].kernel) return fail(BD_EINVAL, where + " has no kernel");
        if (layers[mb].n_in != BD_EMBEDDING_SIZE) return fail(BD_EINVAL, where + ": n_in must be 1024");
        if (layers[mb].n_out != C) return fail(BD_EINVAL, where + ": every member has the first member's n_out");
    }
    const bool adam = opt->kind == BD_TRAIN_ADAM;
    bd::Shape s{n_members, C, bd::kGroupCols / C, 0, max_batch};
    s.groups = (n_members + s.mpg - 1) / s.mpg;
    const int64_t block = s.groups * bd::kGroupFloats, zg = (int64_t)s.groups * max_batch * bd::kGroupCols;
    const int64_t ws_floats = bd::slices_of(max_batch) * block, rl = bd::up64((int64_t)n_members * max_batch),
                  acc_floats = bd::up64(4 * (int64_t)n_members);
    const int64_t total = block * (adam ? 5 : 3) + 2 * zg + ws_floats + rl + acc_floats;
    if (total * (int64_t)sizeof(float) > BD_BANK_MAX_WORKSPACE_BYTES)
        return fail(BD_EWORKSPACE, who + ": " + std::to_string(n_members) + " members of " + std::to_string(C) + " outputs at max_batch " +
                                       std::to_string(max_batch) + " need " + std::to_string(total * (int64_t)sizeof(float)) +
                                       " bytes, more than BD_BANK_MAX_WORKSPACE_BYTES; use fewer members or a smaller max_batch");
    if ((rc = bd::select_device(who, device)) < 0) return rc;

    std::unique_ptr<bd_bank_s> b(new bd_bank_s);
    b->device = device;
    b->loss = loss;
    b->max_batch = max_batch;
    b->s = s;
    b->opt = *opt;
    b->members.assign(n_members, opt->learning_rate);
    BD_HIP(hipMalloc(&b->pool, (size_t)total * sizeof(float)));
    float* at = b->pool;
    auto take = [&at](int64_t n) {
        float* p = at;
        at += n;
        return p;
    };
    b->p = take(block);
    b->grad = take(block);
    if (adam) {
        b->m = take(block);
        b->v = take(block);
    }
    b->snap = take(block);
    b->z = take(zg);
    b->g = take(zg);
    b->ws = take(ws_floats);
    b->ws_floats = ws_floats;
    b->row_loss = take(rl);
    b->acc = reinterpret_cast<double*>(take(acc_floats));
    hipError_t err = hipMemset(b->pool, 0, (size_t)total * sizeof(float));
    for (int mb = 0; mb < n_members && err == hipSuccess; ++mb) {
        const bd::Columns c = bd::columns_of(s, mb);
        float* dst = b->p + c.block + c.col0;
        err = hipMemcpy2D(dst, (size_t)c.ng * sizeof(float), layers[mb].kernel, (size_t)C * sizeof(float), (size_t)C * sizeof(float),
                          bd::kIn, hipMemcpyHostToDevice);
        if (err == hipSuccess && layers[mb].bias)
            err = hipMemcpy(dst + (size_t)bd::kIn * c.ng, layers[mb].bias, (size_t)C * sizeof(float), hipMemcpyHostToDevice);
    }
    if (err != hipSuccess) {
        (void)hipFree(b->pool);
        return fail(BD_EHIP, who + ": " + hipGetErrorString(err));
    }
    *out = b.release();
    return BD_OK;
}

int bd_bank_destroy(bd_bank b) { return bd::destroy(b); }

int bd_bank_step(bd_bank b, const float* X, int64_t ldx, const int32_t* rows, const void* targets, const float* row_w, int64_t ldw,
                 int32_t B, void* stream_) {
    const char* who = "bd_bank_step";
    if (!b || !X || !targets) return fail(BD_EINVAL, std::string(who) + ": null argument");
    int rc = bd::check_batch(who, b->max_batch, X, ldx, B);
    if (rc == BD_OK) rc = bd::check_row_weights(who, row_w, ldw, B);
    if (rc < 0) return rc;
    hipStream_t stream;
    if ((rc = bd::enter(b, stream_, &stream)) < 0) return rc;
    const bd::Shape& s = b->s;
    const int slices = bd::slices_of(B);
    const float inv = bd::loss_inv(b->loss, B, s.C);
    b->members.advance();
    if (row_w)
        hipLaunchKernelGGL(bd::bank_step_kernel<true>, dim3(slices, s.groups), dim3(512), 0, stream, X, ldx, rows, B, b->p, s, b->z, b->g,
                           b->loss, targets, row_w, ldw, inv, b->row_loss, b->ws);
    else
        hipLaunchKernelGGL(bd::bank_step_kernel<false>, dim3(slices, s.groups), dim3(512), 0, stream, X, ldx, rows, B, b->p, s, b->z, b->g,
                           b->loss, targets, row_w, ldw, inv, b->row_loss, b->ws);
    const int n = (bd::kIn + 1) * s.C;
    for (int first = 0; first < s.M; first += bd::kMembersPerLaunch) {
        const bd::Members<bd::kMembersPerLaunch> a = b->members.launch_args(b->opt, first);
        hipLaunchKernelGGL(bd::bank_loss_sum_kernel, dim3(a.count), dim3(256), 0, stream, b->row_loss, B, s.max_batch,
                           bd::loss_scale(b->loss, B, s.C), (float*)nullptr, b->acc, a);
        hipLaunchKernelGGL(bd::bank_apply_kernel, dim3((n + 255) / 256, a.count), dim3(256), 0, stream, b->ws, slices, s, b->grad, b->p,
                           b->m, b->v, b->opt.kind, b->opt.beta_1, b->opt.beta_2, b->opt.epsilon, a);
    }
    BD_HIP(hipGetLastError());
    return BD_OK;
}

int bd_bank_loss(bd_bank b, const float* X, int64_t ldx, const int32_t* rows, const void* targets, const float* row_w, int64_t ldw,
                 int32_t B, float* loss_dev, void* stream_) {
    const char* who = "bd_bank_loss";
    if (!b || !X || !targets || !loss_dev) return fail(BD_EINVAL, std::string(who) + ": null argument");
    int rc = bd::check_batch(who, b->max_batch, X, ldx, B);
    if (rc == BD_OK) rc = bd::check_row_weights(who, row_w, ldw, B);
    if (rc < 0) return rc;
    hipStream_t stream;
    if ((rc = bd::enter(b, stream_, &stream)) < 0) return rc;
    const bd::Shape& s = b->s;
    const float inv = bd::loss_inv(b->loss, B, s.C);
    hipLaunchKernelGGL(bd::bank_forward_kernel, dim3((B + 63) / 64, s.groups), dim3(256), 0, stream, X, ldx, rows, B, b->p, s, b->z,
                       (int64_t)s.max_batch * bd::kGroupCols, bd::kGroupCols);
    if (row_w)
        hipLaunchKernelGGL(bd::bank_loss_rows_kernel<true>, dim3((B + 3) / 4, s.M), dim3(256), 0, stream, b->z, b->g, B, s, b->loss, targets,
                           row_w, ldw, inv, b->row_loss);
    else
        hipLaunchKernelGGL(bd::bank_loss_rows_kernel<false>, dim3((B + 3) / 4, s.M), dim3(256), 0, stream, b->z, b->g, B, s, b->loss,
                           targets, row_w, ldw, inv, b->row_loss);
    for (int first = 0; first < s.M; first += bd::kMembersPerLaunch) {
        const bd::Members<bd::kMembersPerLaunch> a = bd::members_from(s.M, first);
        hipLaunchKernelGGL(bd::bank_loss_sum_kernel, dim3(a.count), dim3(256), 0, stream, b->row_loss, B, s.max_batch,
                           bd::loss_scale(b->loss, B, s.C), loss_dev, (double*)nullptr, a);
    }
    BD_HIP(hipGetLastError());
    return BD_OK;
}

int bd_bank_forward(bd_bank b, const float* X, int64_t ldx, const int32_t* rows, int32_t B, float* logits_dev, int64_t ldl,
                    void* stream_) {
    const char* who = "bd_bank_forward";
    if (!b || !X || !logits_dev) return fail(BD_EINVAL, std::string(who) + ": null argument");
    int rc = bd::check_batch(who, b->max_batch, X, ldx, B);
    if (rc < 0) return rc;
    const bd::Shape& s = b->s;
    if (ldl < (int64_t)s.M * s.C || ldl > INT32_MAX || (reinterpret_cast<uintptr_t>(logits_dev) & 3u))
        return fail(BD_EINVAL, std::string(who) + ": logits_dev must be float-aligned with ldl >= M C");
    hipStream_t stream;
    if ((rc = bd::enter(b, stream_, &stream)) < 0) return rc;
    // group g's columns are members g mpg ..: columns g mpg C .. of a row of the caller's matrix, side by side as in the group
    hipLaunchKernelGGL(bd::bank_forward_kernel, dim3((B + 63) / 64, s.groups), dim3(256), 0, stream, X, ldx, rows, B, b->p, s, logits_dev,
                       (int64_t)s.mpg * s.C, (int)ldl);
    BD_HIP(hipGetLastError());
    return BD_OK;
}

int bd_bank_set_learning_rate(bd_bank b, int32_t member, float learning_rate) {
    return bd::set_learning_rate(b, member, learning_rate, "bd_bank_set_learning_rate");
}

int bd_bank_set_weight_decay(bd_bank b, int32_t member, float weight_decay) {
    return bd::set_weight_decay(b, member, weight_decay, "bd_bank_set_weight_decay");
}

int bd_bank_set_frozen(bd_bank b, int32_t member, int32_t frozen) { return bd::set_frozen(b, member, frozen, "bd_bank_set_frozen"); }

int bd_bank_snapshot(bd_bank b, int32_t member, void* stream) {
    return bd::snapshot_member(b, member, stream, "bd_bank_snapshot", bd::copy_member);
}

int bd_bank_restore(bd_bank b, int32_t member, void* stream) {
    return bd::restore_member(b, member, stream, "bd_bank_restore", "bd_bank_snapshot", bd::copy_member);
}

static int read_pair(bd_bank b, int32_t member, bool grad, float* w_host, float* b_host, const char* who) {
    int rc = bd::check_member(b, member, who);
    if (rc == BD_OK) rc = bd::enter_and_wait(b);
    if (rc < 0) return rc;
    const bd::Shape& s = b->s;
    const bd::Columns c = bd::columns_of(s, member);
    const float* src = (grad ? b->grad : b->p) + c.block + c.col0;
    if (w_host)
        BD_HIP(hipMemcpy2D(w_host, (size_t)s.C * sizeof(float), src, (size_t)c.ng * sizeof(float), (size_t)s.C * sizeof(float),
                                 bd::kIn, hipMemcpyDeviceToHost));
    if (b_host) BD_HIP(hipMemcpy(b_host, src + (size_t)bd::kIn * c.ng, (size_t)s.C * sizeof(float), hipMemcpyDeviceToHost));
    return BD_OK;
}

int bd_bank_read(bd_bank b, int32_t member, float* kernel_host, float* bias_host) {
    return read_pair(b, member, false, kernel_host, bias_host, "bd_bank_read");
}

int bd_bank_gradients(bd_bank b, int32_t member, float* dW_host, float* db_host) {
    return read_pair(b, member, true, dW_host, db_host, "bd_bank_gradients");
}

int bd_bank_mean_loss(bd_bank b, int32_t reset, float* mean_host) { return bd::mean_losses(b, reset, mean_host, "bd_bank_mean_loss"); }

int64_t bd_bank_workspace_floats(bd_bank b) { return bd::workspace_floats(b, "bd_bank_workspace_floats"); }

int bd_bank_workspace_fill(bd_bank b, uint32_t pattern) { return bd::workspace_fill(b, pattern, "bd_bank_workspace_fill"); }

int bd_bank_workspace_read(bd_bank b, float* host, int64_t floats) {
    return bd::workspace_read(b, host, floats, "bd_bank_workspace_read");
}

}  // extern "C"
