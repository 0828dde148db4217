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
#include "headtrain_device.h"

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/buzzdetect_stackbank.h"

namespace bd {

void set_error(const std::string& msg);     // engine.hip: the text bd_last_error() returns on this thread

namespace {

using namespace train;

constexpr int kMembersPerLaunch = 64;

struct Members {                    // the members first .. first + count of a launch, by value
    int first, count;
    float lr[kMembersPerLaunch], lr_t[kMembersPerLaunch], decay[kMembersPerLaunch];
    int frozen[kMembersPerLaunch];
};

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

int fail(int code, const std::string& msg) {
    set_error(msg);
    return code;
}

#define BDS_HIP(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(BD_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct Layer {                      // offsets in floats inside a member's block
    int k, n, act, ld;              // ld = round_up(n, 32): row stride of y and g
    int64_t p, grad, m, v, snap;    // [k n + n] each: W then b (m, v: Adam only, else -1)
    int64_t y, g;                   // [max_batch][ld]
};

}  // namespace
}  // namespace bd

struct bd_stackbank_s {
    int device = 0, loss = 0, M = 0, n_layers = 0, max_batch = 0;
    bd_train_optimizer opt{};       // kind, betas, epsilon; learning_rate: the members' first
    bd::Layer layers[BD_HEAD_MAX_LAYERS]{};
    std::vector<float> lr, wd;
    std::vector<int> frozen, has_snapshot;
    std::vector<int64_t> step;
    float* pool = nullptr;          // one allocation behind every pointer below
    int64_t stride = 0;             // a member's block
    int64_t off_row_loss = 0;       // [max_batch] inside the block
    float* ws = nullptr;            // [M][ws_stride]: [slice][k n + n] of the layer at work
    int64_t ws_stride = 0, ws_floats = 0;
    double* acc = nullptr;          // [M][2]: running loss sum, rows
    hipStream_t last = nullptr;
};

namespace bd {
namespace {

int check_member(const bd_stackbank_s* b, int32_t member, const char* who) {
    if (!b) return fail(BD_EINVAL, std::string(who) + ": null handle");
    if (member < 0 || member >= b->M) return fail(BD_EINVAL, std::string(who) + ": no such member");
    return BD_OK;
}

int check_batch(const bd_stackbank_s* b, const float* X, int64_t ldx, int32_t B, const char* who) {
    if (B < 1 || B > b->max_batch) return fail(BD_EINVAL, std::string(who) + ": B must be in 1..max_batch");
    if (ldx < BD_EMBEDDING_SIZE || ldx % 4 || (reinterpret_cast<uintptr_t>(X) & 15u))
        return fail(BD_EINVAL, std::string(who) + ": X needs 16-byte alignment and ldx >= 1024, a multiple of 4");
    return BD_OK;
}

int check_weights(const float* row_w, int64_t ldw, int32_t B, const char* who) {
    if (!row_w) return BD_OK;
    if (reinterpret_cast<uintptr_t>(row_w) & 3u) return fail(BD_EINVAL, std::string(who) + ": row_weights is not aligned to a float");
    if (ldw < B) return fail(BD_EINVAL, std::string(who) + ": ldw must be at least B");
    return BD_OK;
}

// the launch arguments of members first .. first + count as the host has them now (step counts already advanced)
Members members_of(const bd_stackbank_s* b, int first, int count) {
    Members a{};
    a.first = first;
    a.count = count;
    for (int j = 0; j < count; ++j) {
        const int mb = first + j;
        const float lr = b->lr[mb];
        a.lr[j] = lr;
        a.decay[j] = b->wd[mb] != 0.0f ? lr * b->wd[mb] : 0.0f;
        a.frozen[j] = b->frozen[mb];
        if (b->opt.kind == BD_TRAIN_ADAM && b->step[mb] > 0)
            a.lr_t[j] = (float)((double)lr * std::sqrt(1.0 - std::pow((double)b->opt.beta_2, (double)b->step[mb])) /
                                (1.0 - std::pow((double)b->opt.beta_1, (double)b->step[mb])));
    }
    return a;
}

int width_of(const bd_stackbank_s* b) { return b->layers[b->n_layers - 1].n; }
float inv_of(const bd_stackbank_s* b, int B) { return 1.0f / (b->loss == BD_TRAIN_BINARY ? (float)B * (float)width_of(b) : (float)B); }
double scale_of(const bd_stackbank_s* b, int B) { return 1.0 / (b->loss == BD_TRAIN_BINARY ? (double)B * width_of(b) : (double)B); }

// the forward pass of members a.first ..: the last layer's output goes to Y (member 0's, members y_stride apart, rows ldy
// apart) where given, else to the layer's own logits
void enqueue_forward(bd_stackbank_s* b, const float* X, int64_t ldx, const int* rows, int B, const Members& a, float* Y, int64_t y_stride,
                     int ldy, hipStream_t stream) {
    const float* src = X;
    int64_t lda = ldx, a_stride = 0;
    for (int l = 0; l < b->n_layers; ++l) {
        const Layer& L = b->layers[l];
        const bool last = l + 1 == b->n_layers;
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
    const Layer& L = b->layers[b->n_layers - 1];
    const float inv = inv_of(b, B);
    float* row_loss = b->pool + b->off_row_loss;
    if (row_w)
        hipLaunchKernelGGL(stack_loss_rows_kernel<true>, dim3((B + 3) / 4, a.count), dim3(256), 0, stream, b->pool + L.y, b->pool + L.g,
                           b->stride, L.ld, B, L.n, b->loss, targets, row_w, ldw, inv, row_loss, a.first);
    else
        hipLaunchKernelGGL(stack_loss_rows_kernel<false>, dim3((B + 3) / 4, a.count), dim3(256), 0, stream, b->pool + L.y, b->pool + L.g,
                           b->stride, L.ld, B, L.n, b->loss, targets, row_w, ldw, inv, row_loss, a.first);
    hipLaunchKernelGGL(stack_loss_sum_kernel, dim3(1, a.count), dim3(256), 0, stream, row_loss, b->stride, B, scale_of(b, B), loss_dev,
                       accumulate ? b->acc : nullptr, a);
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
    if (loss != BD_TRAIN_CATEGORICAL && loss != BD_TRAIN_BINARY) return fail(BD_EINVAL, who + ": unknown loss");
    if (opt->kind != BD_TRAIN_SGD && opt->kind != BD_TRAIN_ADAM) return fail(BD_EINVAL, who + ": unknown optimizer");
    if (!(opt->learning_rate > 0.0f) || !std::isfinite(opt->learning_rate))
        return fail(BD_EINVAL, who + ": learning_rate must be positive and finite");
    if (opt->kind == BD_TRAIN_ADAM && !(opt->beta_1 >= 0.0f && opt->beta_1 < 1.0f && opt->beta_2 >= 0.0f && opt->beta_2 < 1.0f &&
                                        opt->epsilon > 0.0f))
        return fail(BD_EINVAL, who + ": Adam needs 0 <= beta < 1 and epsilon > 0");
    if (max_batch < 1 || max_batch > BD_TRAIN_MAX_BATCH) return fail(BD_EINVAL, who + ": max_batch must be in 1..65536");
    for (int mb = 0; mb < n_members; ++mb)
        for (int l = 0; l < n_layers; ++l) {
            const bd_head_layer& L = layers[(size_t)mb * n_layers + l];
            const bd_head_layer& L0 = layers[l];
            const std::string where = who + ": member " + std::to_string(mb) + ", layer " + std::to_string(l);
            if (!L.kernel) return fail(BD_EINVAL, where + " has no kernel");
            if (L.n_in != (l == 0 ? BD_EMBEDDING_SIZE : layers[(size_t)mb * n_layers + l - 1].n_out))
                return fail(BD_EINVAL, where + ": n_in must be 1024 for the first layer, the width before it for the others");
            if (L.n_out < 1 || L.n_out > BD_HEAD_MAX_WIDTH) return fail(BD_EINVAL, where + ": n_out must be in 1..2048");
            if (L.activation < BD_HEAD_LINEAR || L.activation > BD_HEAD_SOFTMAX || (L.activation == BD_HEAD_SOFTMAX && l + 1 < n_layers))
                return fail(BD_EINVAL, where + ": hidden activations are linear, relu, sigmoid or tanh");
            if (L.n_out != L0.n_out || (l + 1 < n_layers && L.activation != L0.activation))
                return fail(BD_EINVAL, where + ": every member has the first member's widths and hidden activations");
        }
    const bool adam = opt->kind == BD_TRAIN_ADAM;
    std::unique_ptr<bd_stackbank_s> b(new bd_stackbank_s);
    const int64_t slices = (max_batch + bd::kSliceRows - 1) / bd::kSliceRows;
    auto up64 = [](int64_t v) { return (v + 63) / 64 * 64; };
    // a member's block in floats, every piece on a 64-float boundary
    int64_t total = 0, params_max = 0;
    std::string widths;
    for (int l = 0; l < n_layers; ++l) {
        bd::Layer& L = b->layers[l];
        L.k = layers[l].n_in;
        L.n = layers[l].n_out;
        L.act = layers[l].activation;
        L.ld = (L.n + 31) / 32 * 32;
        widths += (l ? ", " : "") + std::to_string(L.n);
        const int64_t np = up64((int64_t)L.k * L.n + L.n);
        params_max = np > params_max ? np : params_max;
        L.p = total;
        L.grad = L.p + np;
        L.m = adam ? L.p + 2 * np : -1;
        L.v = adam ? L.p + 3 * np : -1;
        L.snap = L.p + (adam ? 4 : 2) * np;
        total += np * (adam ? 5 : 3);
        L.y = total;
        L.g = L.y + up64((int64_t)max_batch * L.ld);
        total += up64((int64_t)max_batch * L.ld) * 2;
    }
    b->off_row_loss = total;
    total += up64(max_batch);
    b->stride = total;
    b->ws_stride = slices * params_max;                   // params_max is a multiple of 64
    b->ws_floats = b->ws_stride * n_members;
    const int64_t acc_floats = up64(4 * (int64_t)n_members);
    const int64_t pool_floats = (b->stride + b->ws_stride) * n_members + acc_floats;
    if (pool_floats * (int64_t)sizeof(float) > BD_STACKBANK_MAX_WORKSPACE_BYTES)
        return fail(BD_EWORKSPACE, who + ": " + std::to_string(n_members) + " members of widths " + widths + " at max_batch " +
                                       std::to_string(max_batch) + " need " + std::to_string(pool_floats * (int64_t)sizeof(float)) +
                                       " bytes, more than BD_STACKBANK_MAX_WORKSPACE_BYTES; use fewer members or a smaller max_batch");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(BD_ENODEVICE, who + ": no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= count) return fail(BD_ENODEVICE, who + ": device index out of range");
    hipDeviceProp_t prop;
    BDS_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(BD_ENODEVICE, who + ": kernels are built for gfx950 only, device is " + prop.gcnArchName);
    BDS_HIP(hipSetDevice(device));

    b->device = device;
    b->loss = loss;
    b->M = n_members;
    b->n_layers = n_layers;
    b->max_batch = max_batch;
    b->opt = *opt;
    b->lr.assign(n_members, opt->learning_rate);
    b->wd.assign(n_members, 0.0f);
    b->frozen.assign(n_members, 0);
    b->has_snapshot.assign(n_members, 0);
    b->step.assign(n_members, 0);
    BDS_HIP(hipMalloc(&b->pool, (size_t)pool_floats * sizeof(float)));
    b->ws = b->pool + b->stride * n_members;
    b->acc = reinterpret_cast<double*>(b->ws + b->ws_floats);
    hipError_t err = hipMemset(b->pool, 0, (size_t)pool_floats * sizeof(float));
    for (int mb = 0; mb < n_members && err == hipSuccess; ++mb)
        for (int l = 0; l < n_layers && err == hipSuccess; ++l) {
            const bd_head_layer& src = layers[(size_t)mb * n_layers + l];
            const bd::Layer& L = b->layers[l];
            float* dst = b->pool + mb * b->stride + L.p;
            err = hipMemcpy(dst, src.kernel, (size_t)L.k * L.n * sizeof(float), hipMemcpyHostToDevice);
            if (err == hipSuccess && src.bias)
                err = hipMemcpy(dst + (size_t)L.k * L.n, src.bias, (size_t)L.n * sizeof(float), hipMemcpyHostToDevice);
        }
    if (err != hipSuccess) {
        (void)hipFree(b->pool);
        return fail(BD_EHIP, who + ": " + hipGetErrorString(err));
    }
    *out = b.release();
    return BD_OK;
}

int bd_stackbank_destroy(bd_stackbank b) {
    if (!b) return BD_OK;
    (void)hipSetDevice(b->device);
    (void)hipStreamSynchronize(b->last);
    if (b->pool) (void)hipFree(b->pool);
    delete b;
    return BD_OK;
}

int bd_stackbank_step(bd_stackbank b, const float* X, int64_t ldx, const int32_t* rows, const void* targets, const float* row_w,
                      int64_t ldw, int32_t B, void* stream_) {
    const char* who = "bd_stackbank_step";
    if (!b || !X || !targets) return fail(BD_EINVAL, std::string(who) + ": null argument");
    int rc = bd::check_batch(b, X, ldx, B, who);
    if (rc == BD_OK) rc = bd::check_weights(row_w, ldw, B, who);
    if (rc < 0) return rc;
    BDS_HIP(hipSetDevice(b->device));
    hipStream_t stream = (hipStream_t)stream_;
    b->last = stream;
    const int slices = (B + bd::kSliceRows - 1) / bd::kSliceRows;
    for (int mb = 0; mb < b->M; ++mb)
        if (!b->frozen[mb]) b->step[mb] += 1;
    const bool adam = b->opt.kind == BD_TRAIN_ADAM;
    for (int first = 0; first < b->M; first += bd::kMembersPerLaunch) {
        const bd::Members a = bd::members_of(b, first, b->M - first < bd::kMembersPerLaunch ? b->M - first : bd::kMembersPerLaunch);
        bd::enqueue_forward(b, X, ldx, rows, B, a, nullptr, 0, 0, stream);
        bd::enqueue_loss(b, targets, row_w, ldw, B, nullptr, true, a, stream);
        for (int l = b->n_layers - 1; l >= 0; --l) {
            const bd::Layer& L = b->layers[l];
            const int n = L.k * L.n + L.n;
            const int tiles = (L.k + 31) / 32 * ((L.n + 31) / 32);
            hipLaunchKernelGGL(bd::stack_weight_grad_kernel, dim3(a.count, (tiles + 3) / 4, slices), dim3(256), 0, stream,
                               l == 0 ? X : b->pool + b->layers[l - 1].y, l == 0 ? ldx : (int64_t)b->layers[l - 1].ld,
                               l == 0 ? (int64_t)0 : b->stride, l == 0 ? rows : nullptr, B, L.k, b->pool + L.g, b->stride, L.ld, L.n, b->ws,
                               b->ws_stride, a);
            if (l > 0) {                                 // with this layer's weights as the forward pass saw them
                const bd::Layer& Lp = b->layers[l - 1];
                hipLaunchKernelGGL(bd::stack_input_grad_kernel, dim3(a.count, (L.k + 63) / 64, (B + 63) / 64), dim3(256), 0, stream,
                                   b->pool + L.g, L.ld, B, L.k, b->pool + L.p, L.n, b->pool + Lp.y, Lp.act, b->pool + Lp.g, Lp.ld,
                                   b->stride, a);
            }
            hipLaunchKernelGGL(bd::stack_apply_kernel, dim3((n + 255) / 256, a.count), dim3(256), 0, stream, b->ws, b->ws_stride, slices, n,
                               L.k * L.n, b->pool + L.grad, b->pool + L.p, adam ? b->pool + L.m : nullptr,
                               adam ? b->pool + L.v : nullptr, b->stride, b->opt.kind, b->opt.beta_1, b->opt.beta_2, b->opt.epsilon, a);
        }
    }
    BDS_HIP(hipGetLastError());
    return BD_OK;
}

int bd_stackbank_loss(bd_stackbank b, const float* X, int64_t ldx, const int32_t* rows, const void* targets, const float* row_w,
                      int64_t ldw, int32_t B, float* loss_dev, void* stream_) {
    const char* who = "bd_stackbank_loss";
    if (!b || !X || !targets || !loss_dev) return fail(BD_EINVAL, std::string(who) + ": null argument");
    int rc = bd::check_batch(b, X, ldx, B, who);
    if (rc == BD_OK) rc = bd::check_weights(row_w, ldw, B, who);
    if (rc < 0) return rc;
    BDS_HIP(hipSetDevice(b->device));
    hipStream_t stream = (hipStream_t)stream_;
    b->last = stream;
    for (int first = 0; first < b->M; first += bd::kMembersPerLaunch) {
        bd::Members a{};
        a.first = first;
        a.count = b->M - first < bd::kMembersPerLaunch ? b->M - first : bd::kMembersPerLaunch;
        bd::enqueue_forward(b, X, ldx, rows, B, a, nullptr, 0, 0, stream);
        bd::enqueue_loss(b, targets, row_w, ldw, B, loss_dev, false, a, stream);
    }
    BDS_HIP(hipGetLastError());
    return BD_OK;
}

int bd_stackbank_forward(bd_stackbank b, const float* X, int64_t ldx, const int32_t* rows, int32_t B, float* logits_dev, int64_t ldl,
                         void* stream_) {
    const char* who = "bd_stackbank_forward";
    if (!b || !X || !logits_dev) return fail(BD_EINVAL, std::string(who) + ": null argument");
    const int rc = bd::check_batch(b, X, ldx, B, who);
    if (rc < 0) return rc;
    const int C = bd::width_of(b);
    if (ldl < (int64_t)b->M * C || ldl > INT32_MAX || (reinterpret_cast<uintptr_t>(logits_dev) & 3u))
        return fail(BD_EINVAL, std::string(who) + ": logits_dev must be float-aligned with ldl >= M C");
    BDS_HIP(hipSetDevice(b->device));
    hipStream_t stream = (hipStream_t)stream_;
    b->last = stream;
    for (int first = 0; first < b->M; first += bd::kMembersPerLaunch) {
        bd::Members a{};
        a.first = first;
        a.count = b->M - first < bd::kMembersPerLaunch ? b->M - first : bd::kMembersPerLaunch;
        bd::enqueue_forward(b, X, ldx, rows, B, a, logits_dev, C, (int)ldl, stream);
    }
    BDS_HIP(hipGetLastError());
    return BD_OK;
}

int bd_stackbank_set_learning_rate(bd_stackbank b, int32_t member, float learning_rate) {
    const int rc = bd::check_member(b, member, "bd_stackbank_set_learning_rate");
    if (rc < 0) return rc;
    if (!(learning_rate > 0.0f) || !std::isfinite(learning_rate))
        return fail(BD_EINVAL, "bd_stackbank_set_learning_rate: learning_rate must be positive and finite");
    b->lr[member] = learning_rate;
    return BD_OK;
}

int bd_stackbank_set_weight_decay(bd_stackbank b, int32_t member, float weight_decay) {
    const int rc = bd::check_member(b, member, "bd_stackbank_set_weight_decay");
    if (rc < 0) return rc;
    if (!(weight_decay >= 0.0f) || !std::isfinite(weight_decay))
        return fail(BD_EINVAL, "bd_stackbank_set_weight_decay: weight_decay must be finite and not negative");
    b->wd[member] = weight_decay;
    return BD_OK;
}

int bd_stackbank_set_frozen(bd_stackbank b, int32_t member, int32_t frozen) {
    const int rc = bd::check_member(b, member, "bd_stackbank_set_frozen");
    if (rc < 0) return rc;
    if (frozen != 0 && frozen != 1) return fail(BD_EINVAL, "bd_stackbank_set_frozen: frozen must be 0 or 1");
    b->frozen[member] = frozen;
    return BD_OK;
}

// every layer of the member's parameters -> its snapshot (to_snapshot) or back, on the caller's stream
static int copy_member(bd_stackbank b, int32_t member, bool to_snapshot, void* stream_) {
    BDS_HIP(hipSetDevice(b->device));
    hipStream_t stream = (hipStream_t)stream_;
    b->last = stream;
    float* block = b->pool + member * b->stride;
    for (int l = 0; l < b->n_layers; ++l) {
        const bd::Layer& L = b->layers[l];
        const size_t bytes = ((size_t)L.k * L.n + L.n) * sizeof(float);
        float *p = block + L.p, *snap = block + L.snap;
        BDS_HIP(hipMemcpyAsync(to_snapshot ? snap : p, to_snapshot ? p : snap, bytes, hipMemcpyDeviceToDevice, stream));
    }
    return BD_OK;
}

int bd_stackbank_snapshot(bd_stackbank b, int32_t member, void* stream) {
    int rc = bd::check_member(b, member, "bd_stackbank_snapshot");
    if (rc < 0) return rc;
    rc = copy_member(b, member, true, stream);
    if (rc == BD_OK) b->has_snapshot[member] = 1;
    return rc;
}

int bd_stackbank_restore(bd_stackbank b, int32_t member, void* stream) {
    const int rc = bd::check_member(b, member, "bd_stackbank_restore");
    if (rc < 0) return rc;
    if (!b->has_snapshot[member])
        return fail(BD_EINVAL, "bd_stackbank_restore: no snapshot of member " + std::to_string(member) + " was taken (bd_stackbank_snapshot)");
    return copy_member(b, member, false, stream);
}

static int read_pair(bd_stackbank b, int32_t member, int32_t layer, bool grad, float* w_host, float* b_host, const char* who) {
    const int rc = bd::check_member(b, member, who);
    if (rc < 0) return rc;
    if (layer < 0 || layer >= b->n_layers) return fail(BD_EINVAL, std::string(who) + ": no such layer");
    BDS_HIP(hipSetDevice(b->device));
    BDS_HIP(hipStreamSynchronize(b->last));
    const bd::Layer& L = b->layers[layer];
    const float* src = b->pool + member * b->stride + (grad ? L.grad : L.p);
    if (w_host) BDS_HIP(hipMemcpy(w_host, src, (size_t)L.k * L.n * sizeof(float), hipMemcpyDeviceToHost));
    if (b_host) BDS_HIP(hipMemcpy(b_host, src + (size_t)L.k * L.n, (size_t)L.n * sizeof(float), hipMemcpyDeviceToHost));
    return BD_OK;
}

int bd_stackbank_read(bd_stackbank b, int32_t member, int32_t layer, float* kernel_host, float* bias_host) {
    return read_pair(b, member, layer, false, kernel_host, bias_host, "bd_stackbank_read");
}

int bd_stackbank_gradients(bd_stackbank b, int32_t member, int32_t layer, float* dW_host, float* db_host) {
    return read_pair(b, member, layer, true, dW_host, db_host, "bd_stackbank_gradients");
}

int bd_stackbank_mean_loss(bd_stackbank b, int32_t reset, float* mean_host) {
    if (!b || !mean_host) return fail(BD_EINVAL, "bd_stackbank_mean_loss: null argument");
    BDS_HIP(hipSetDevice(b->device));
    BDS_HIP(hipStreamSynchronize(b->last));
    std::vector<double> acc(2 * (size_t)b->M, 0.0);
    BDS_HIP(hipMemcpy(acc.data(), b->acc, acc.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int mb = 0; mb < b->M; ++mb) mean_host[mb] = acc[2 * mb + 1] > 0.0 ? (float)(acc[2 * mb] / acc[2 * mb + 1]) : 0.0f;
    if (reset) BDS_HIP(hipMemset(b->acc, 0, acc.size() * sizeof(double)));
    return BD_OK;
}

int64_t bd_stackbank_workspace_floats(bd_stackbank b) {
    if (!b) return fail(BD_EINVAL, "bd_stackbank_workspace_floats: null handle");
    return b->ws_floats;
}

int bd_stackbank_workspace_fill(bd_stackbank b, uint32_t pattern) {
    if (!b) return fail(BD_EINVAL, "bd_stackbank_workspace_fill: null handle");
    BDS_HIP(hipSetDevice(b->device));
    BDS_HIP(hipStreamSynchronize(b->last));
    BDS_HIP(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(b->ws), (int)pattern, (size_t)b->ws_floats));
    BDS_HIP(hipDeviceSynchronize());
    return BD_OK;
}

int bd_stackbank_workspace_read(bd_stackbank b, float* host, int64_t floats) {
    if (!b || !host || floats < 0 || floats > b->ws_floats) return fail(BD_EINVAL, "bd_stackbank_workspace_read: bad argument");
    BDS_HIP(hipSetDevice(b->device));
    BDS_HIP(hipStreamSynchronize(b->last));
    BDS_HIP(hipMemcpy(host, b->ws, (size_t)floats * sizeof(float), hipMemcpyDeviceToHost));
    return BD_OK;
}

}  // extern "C"
