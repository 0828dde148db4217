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
#include "headtrain_device.h"

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/buzzdetect_bank.h"

namespace bd {

void set_error(const std::string& msg);     // engine.hip: the text bd_last_error() returns on this thread

namespace {

using namespace train;

constexpr int kGroupCols = BD_BANK_GROUP_COLUMNS;
constexpr int kIn = BD_EMBEDDING_SIZE;
constexpr int64_t kGroupFloats = (int64_t)(kIn + 1) * kGroupCols;      // stride of a group's [1025][ng] block
constexpr int kMembersPerLaunch = 64;
static_assert(kGroupCols == BD_TRAIN_FUSED_MAX_WIDTH && kGroupCols % 32 == 0, "a group is the fused kernel's two column tiles");

struct Members {                    // the members first .. first + count of a launch, by value
    int first, count;
    float lr[kMembersPerLaunch], lr_t[kMembersPerLaunch], decay[kMembersPerLaunch];
    int frozen[kMembersPerLaunch];
};

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
                                                             float* __restrict__ out, double* __restrict__ acc, Members a) {
    __shared__ double part[256];
    const int member = a.first + blockIdx.x;
    loss_sum_block(row_loss + (size_t)member * max_batch, B, scale, out ? out + member : nullptr,
                   acc && !a.frozen[blockIdx.x] ? acc + 2 * (size_t)member : nullptr, part);
}

// grid (ceil((1024 C + C) / 256), a.count): element i = k C + c of member a.first + blockIdx.y's [W | b]
__global__ __launch_bounds__(256) void bank_apply_kernel(const float* __restrict__ ws, int slices, Shape s, float* __restrict__ grad,
                                                          float* __restrict__ P, float* __restrict__ m, float* __restrict__ v,
                                                          int kind, float b1, float b2, float eps, Members a) {
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

int fail(int code, const std::string& msg) {
    set_error(msg);
    return code;
}

#define BDB_HIP(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(BD_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

}  // namespace
}  // namespace bd

struct bd_bank_s {
    int device = 0, loss = 0;
    bd::Shape s{};
    bd_train_optimizer opt{};       // kind, betas, epsilon; learning_rate: the members' first
    std::vector<float> lr, wd;
    std::vector<int> frozen, has_snapshot;
    std::vector<int64_t> step;
    float* pool = nullptr;          // one allocation behind every pointer below
    float *p = nullptr, *grad = nullptr, *m = nullptr, *v = nullptr, *snap = nullptr;      // [groups][kGroupFloats]
    float *z = nullptr, *g = nullptr;                                                      // [groups][max_batch][64]
    float* ws = nullptr;            // [slices of max_batch][groups][kGroupFloats]
    int64_t ws_floats = 0;
    float* row_loss = nullptr;      // [M][max_batch]
    double* acc = nullptr;          // [M][2]: running loss sum, rows
    hipStream_t last = nullptr;
};

namespace bd {
namespace {

int check_member(const bd_bank_s* b, int32_t member, const char* who) {
    if (!b) return fail(BD_EINVAL, std::string(who) + ": null handle");
    if (member < 0 || member >= b->s.M) return fail(BD_EINVAL, std::string(who) + ": no such member");
    return BD_OK;
}

int check_batch(const bd_bank_s* b, const float* X, int64_t ldx, int32_t B, const char* who) {
    if (B < 1 || B > b->s.max_batch) return fail(BD_EINVAL, std::string(who) + ": B must be in 1..max_batch");
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
Members members_of(const bd_bank_s* b, int first, int count) {
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

float inv_of(const bd_bank_s* b, int B) { return 1.0f / (b->loss == BD_TRAIN_BINARY ? (float)B * (float)b->s.C : (float)B); }
double scale_of(const bd_bank_s* b, int B) { return 1.0 / (b->loss == BD_TRAIN_BINARY ? (double)B * b->s.C : (double)B); }

}  // namespace
}  // namespace bd

using bd::fail;

extern "C" {

int bd_bank_abi_version(void) { return BD_BANK_ABI_VERSION; }

int bd_bank_create(int device, const bd_head_layer* layers, int32_t n_members, int32_t loss, const bd_train_optimizer* opt,
                   int32_t max_batch, bd_bank* out) {
    if (!out || !layers || !opt) return fail(BD_EINVAL, "bd_bank_create: null argument");
    *out = nullptr;
    if (n_members < 1 || n_members > BD_BANK_MAX_MEMBERS) return fail(BD_EINVAL, "bd_bank_create: the members must number 1..4096");
    if (loss != BD_TRAIN_CATEGORICAL && loss != BD_TRAIN_BINARY) return fail(BD_EINVAL, "bd_bank_create: unknown loss");
    if (opt->kind != BD_TRAIN_SGD && opt->kind != BD_TRAIN_ADAM) return fail(BD_EINVAL, "bd_bank_create: unknown optimizer");
    if (!(opt->learning_rate > 0.0f) || !std::isfinite(opt->learning_rate))
        return fail(BD_EINVAL, "bd_bank_create: learning_rate must be positive and finite");
    if (opt->kind == BD_TRAIN_ADAM && !(opt->beta_1 >= 0.0f && opt->beta_1 < 1.0f && opt->beta_2 >= 0.0f && opt->beta_2 < 1.0f &&
                                        opt->epsilon > 0.0f))
        return fail(BD_EINVAL, "bd_bank_create: Adam needs 0 <= beta < 1 and epsilon > 0");
    if (max_batch < 1 || max_batch > BD_TRAIN_MAX_BATCH) return fail(BD_EINVAL, "bd_bank_create: max_batch must be in 1..65536");
    const int C = layers[0].n_out;
    if (C < 1 || C > BD_TRAIN_FUSED_MAX_WIDTH) return fail(BD_EINVAL, "bd_bank_create: n_out must be in 1..64 (a bank holds one-layer heads of the fused width)");
    for (int mb = 0; mb < n_members; ++mb) {
        const std::string where = "bd_bank_create: member " + std::to_string(mb);
        if (!layers[mb].kernel) return fail(BD_EINVAL, where + " has no kernel");
        if (layers[mb].n_in != BD_EMBEDDING_SIZE) return fail(BD_EINVAL, where + ": n_in must be 1024");
        if (layers[mb].n_out != C) return fail(BD_EINVAL, where + ": every member has the first member's n_out");
    }
    const bool adam = opt->kind == BD_TRAIN_ADAM;
    bd::Shape s{n_members, C, bd::kGroupCols / C, 0, max_batch};
    s.groups = (n_members + s.mpg - 1) / s.mpg;
    const int64_t slices = (max_batch + bd::kSliceRows - 1) / bd::kSliceRows;
    auto up64 = [](int64_t v) { return (v + 63) / 64 * 64; };
    const int64_t block = s.groups * bd::kGroupFloats, zg = (int64_t)s.groups * max_batch * bd::kGroupCols;
    const int64_t ws_floats = slices * block, rl = up64((int64_t)n_members * max_batch), acc_floats = up64(4 * (int64_t)n_members);
    const int64_t total = block * (adam ? 5 : 3) + 2 * zg + ws_floats + rl + acc_floats;
    if (total * (int64_t)sizeof(float) > BD_BANK_MAX_WORKSPACE_BYTES)
        return fail(BD_EWORKSPACE, "bd_bank_create: " + std::to_string(n_members) + " members of " + std::to_string(C) + " outputs at max_batch " +
                                       std::to_string(max_batch) + " need " + std::to_string(total * (int64_t)sizeof(float)) +
                                       " bytes, more than BD_BANK_MAX_WORKSPACE_BYTES; use fewer members or a smaller max_batch");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(BD_ENODEVICE, "bd_bank_create: no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= count) return fail(BD_ENODEVICE, "bd_bank_create: device index out of range");
    hipDeviceProp_t prop;
    BDB_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(BD_ENODEVICE, std::string("bd_bank_create: kernels are built for gfx950 only, device is ") + prop.gcnArchName);
    BDB_HIP(hipSetDevice(device));

    std::unique_ptr<bd_bank_s> b(new bd_bank_s);
    b->device = device;
    b->loss = loss;
    b->s = s;
    b->opt = *opt;
    b->lr.assign(n_members, opt->learning_rate);
    b->wd.assign(n_members, 0.0f);
    b->frozen.assign(n_members, 0);
    b->has_snapshot.assign(n_members, 0);
    b->step.assign(n_members, 0);
    BDB_HIP(hipMalloc(&b->pool, (size_t)total * sizeof(float)));
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
        const int group = mb / s.mpg, ng = (s.mpg < n_members - group * s.mpg ? s.mpg : n_members - group * s.mpg) * C;
        float* dst = b->p + group * bd::kGroupFloats + (mb % s.mpg) * C;
        err = hipMemcpy2D(dst, (size_t)ng * sizeof(float), layers[mb].kernel, (size_t)C * sizeof(float), (size_t)C * sizeof(float),
                          bd::kIn, hipMemcpyHostToDevice);
        if (err == hipSuccess && layers[mb].bias)
            err = hipMemcpy(dst + (size_t)bd::kIn * ng, layers[mb].bias, (size_t)C * sizeof(float), hipMemcpyHostToDevice);
    }
    if (err != hipSuccess) {
        (void)hipFree(b->pool);
        return fail(BD_EHIP, std::string("bd_bank_create: ") + hipGetErrorString(err));
    }
    *out = b.release();
    return BD_OK;
}

int bd_bank_destroy(bd_bank b) {
    if (!b) return BD_OK;
    (void)hipSetDevice(b->device);
    (void)hipStreamSynchronize(b->last);
    if (b->pool) (void)hipFree(b->pool);
    delete b;
    return BD_OK;
}

int bd_bank_step(bd_bank b, const float* X, int64_t ldx, const int32_t* rows, const void* targets, const float* row_w, int64_t ldw,
                 int32_t B, void* stream_) {
    const char* who = "bd_bank_step";
    if (!b || !X || !targets) return fail(BD_EINVAL, std::string(who) + ": null argument");
    int rc = bd::check_batch(b, X, ldx, B, who);
    if (rc == BD_OK) rc = bd::check_weights(row_w, ldw, B, who);
    if (rc < 0) return rc;
    BDB_HIP(hipSetDevice(b->device));
    hipStream_t stream = (hipStream_t)stream_;
    b->last = stream;
    const bd::Shape& s = b->s;
    const int slices = (B + bd::kSliceRows - 1) / bd::kSliceRows;
    const float inv = bd::inv_of(b, B);
    for (int mb = 0; mb < s.M; ++mb)
        if (!b->frozen[mb]) b->step[mb] += 1;
    if (row_w)
        hipLaunchKernelGGL(bd::bank_step_kernel<true>, dim3(slices, s.groups), dim3(512), 0, stream, X, ldx, rows, B, b->p, s, b->z, b->g,
                           b->loss, targets, row_w, ldw, inv, b->row_loss, b->ws);
    else
        hipLaunchKernelGGL(bd::bank_step_kernel<false>, dim3(slices, s.groups), dim3(512), 0, stream, X, ldx, rows, B, b->p, s, b->z, b->g,
                           b->loss, targets, row_w, ldw, inv, b->row_loss, b->ws);
    const int n = (bd::kIn + 1) * s.C;
    for (int first = 0; first < s.M; first += bd::kMembersPerLaunch) {
        const bd::Members a = bd::members_of(b, first, s.M - first < bd::kMembersPerLaunch ? s.M - first : bd::kMembersPerLaunch);
        hipLaunchKernelGGL(bd::bank_loss_sum_kernel, dim3(a.count), dim3(256), 0, stream, b->row_loss, B, s.max_batch, bd::scale_of(b, B),
                           (float*)nullptr, b->acc, a);
        hipLaunchKernelGGL(bd::bank_apply_kernel, dim3((n + 255) / 256, a.count), dim3(256), 0, stream, b->ws, slices, s, b->grad, b->p,
                           b->m, b->v, b->opt.kind, b->opt.beta_1, b->opt.beta_2, b->opt.epsilon, a);
    }
    BDB_HIP(hipGetLastError());
    return BD_OK;
}

int bd_bank_loss(bd_bank b, const float* X, int64_t ldx, const int32_t* rows, const void* targets, const float* row_w, int64_t ldw,
                 int32_t B, float* loss_dev, void* stream_) {
    const char* who = "bd_bank_loss";
    if (!b || !X || !targets || !loss_dev) return fail(BD_EINVAL, std::string(who) + ": null argument");
    int rc = bd::check_batch(b, X, ldx, B, who);
    if (rc == BD_OK) rc = bd::check_weights(row_w, ldw, B, who);
    if (rc < 0) return rc;
    BDB_HIP(hipSetDevice(b->device));
    hipStream_t stream = (hipStream_t)stream_;
    b->last = stream;
    const bd::Shape& s = b->s;
    const float inv = bd::inv_of(b, B);
    hipLaunchKernelGGL(bd::bank_forward_kernel, dim3((B + 63) / 64, s.groups), dim3(256), 0, stream, X, ldx, rows, B, b->p, s, b->z,
                       (int64_t)s.max_batch * bd::kGroupCols, bd::kGroupCols);
    if (row_w)
        hipLaunchKernelGGL(bd::bank_loss_rows_kernel<true>, dim3((B + 3) / 4, s.M), dim3(256), 0, stream, b->z, b->g, B, s, b->loss, targets,
                           row_w, ldw, inv, b->row_loss);
    else
        hipLaunchKernelGGL(bd::bank_loss_rows_kernel<false>, dim3((B + 3) / 4, s.M), dim3(256), 0, stream, b->z, b->g, B, s, b->loss,
                           targets, row_w, ldw, inv, b->row_loss);
    for (int first = 0; first < s.M; first += bd::kMembersPerLaunch) {
        bd::Members a{};
        a.first = first;
        a.count = s.M - first < bd::kMembersPerLaunch ? s.M - first : bd::kMembersPerLaunch;
        hipLaunchKernelGGL(bd::bank_loss_sum_kernel, dim3(a.count), dim3(256), 0, stream, b->row_loss, B, s.max_batch, bd::scale_of(b, B),
                           loss_dev, (double*)nullptr, a);
    }
    BDB_HIP(hipGetLastError());
    return BD_OK;
}

int bd_bank_forward(bd_bank b, const float* X, int64_t ldx, const int32_t* rows, int32_t B, float* logits_dev, int64_t ldl,
                    void* stream_) {
    const char* who = "bd_bank_forward";
    if (!b || !X || !logits_dev) return fail(BD_EINVAL, std::string(who) + ": null argument");
    const int rc = bd::check_batch(b, X, ldx, B, who);
    if (rc < 0) return rc;
    const bd::Shape& s = b->s;
    if (ldl < (int64_t)s.M * s.C || ldl > INT32_MAX || (reinterpret_cast<uintptr_t>(logits_dev) & 3u))
        return fail(BD_EINVAL, std::string(who) + ": logits_dev must be float-aligned with ldl >= M C");
    BDB_HIP(hipSetDevice(b->device));
    hipStream_t stream = (hipStream_t)stream_;
    b->last = stream;
    // group g's columns are members g mpg ..: columns g mpg C .. of a row of the caller's matrix, side by side as in the group
    hipLaunchKernelGGL(bd::bank_forward_kernel, dim3((B + 63) / 64, s.groups), dim3(256), 0, stream, X, ldx, rows, B, b->p, s, logits_dev,
                       (int64_t)s.mpg * s.C, (int)ldl);
    BDB_HIP(hipGetLastError());
    return BD_OK;
}

int bd_bank_set_learning_rate(bd_bank b, int32_t member, float learning_rate) {
    const int rc = bd::check_member(b, member, "bd_bank_set_learning_rate");
    if (rc < 0) return rc;
    if (!(learning_rate > 0.0f) || !std::isfinite(learning_rate))
        return fail(BD_EINVAL, "bd_bank_set_learning_rate: learning_rate must be positive and finite");
    b->lr[member] = learning_rate;
    return BD_OK;
}

int bd_bank_set_weight_decay(bd_bank b, int32_t member, float weight_decay) {
    const int rc = bd::check_member(b, member, "bd_bank_set_weight_decay");
    if (rc < 0) return rc;
    if (!(weight_decay >= 0.0f) || !std::isfinite(weight_decay))
        return fail(BD_EINVAL, "bd_bank_set_weight_decay: weight_decay must be finite and not negative");
    b->wd[member] = weight_decay;
    return BD_OK;
}

int bd_bank_set_frozen(bd_bank b, int32_t member, int32_t frozen) {
    const int rc = bd::check_member(b, member, "bd_bank_set_frozen");
    if (rc < 0) return rc;
    if (frozen != 0 && frozen != 1) return fail(BD_EINVAL, "bd_bank_set_frozen: frozen must be 0 or 1");
    b->frozen[member] = frozen;
    return BD_OK;
}

// member's columns of the parameters -> its columns of the snapshot (to_snapshot) or back, on the caller's stream
static int copy_member(bd_bank b, int32_t member, bool to_snapshot, void* stream_) {
    BDB_HIP(hipSetDevice(b->device));
    hipStream_t stream = (hipStream_t)stream_;
    b->last = stream;
    const bd::Shape& s = b->s;
    const int group = member / s.mpg, nm = s.mpg < s.M - group * s.mpg ? s.mpg : s.M - group * s.mpg;
    float *p = b->p + group * bd::kGroupFloats, *snap = b->snap + group * bd::kGroupFloats;
    hipLaunchKernelGGL(bd::bank_copy_member_kernel, dim3(((bd::kIn + 1) * s.C + 255) / 256), dim3(256), 0, stream, to_snapshot ? snap : p,
                       to_snapshot ? p : snap, s.C, nm * s.C, (member % s.mpg) * s.C);
    BDB_HIP(hipGetLastError());
    return BD_OK;
}

int bd_bank_snapshot(bd_bank b, int32_t member, void* stream) {
    int rc = bd::check_member(b, member, "bd_bank_snapshot");
    if (rc < 0) return rc;
    rc = copy_member(b, member, true, stream);
    if (rc == BD_OK) b->has_snapshot[member] = 1;
    return rc;
}

int bd_bank_restore(bd_bank b, int32_t member, void* stream) {
    const int rc = bd::check_member(b, member, "bd_bank_restore");
    if (rc < 0) return rc;
    if (!b->has_snapshot[member])
        return fail(BD_EINVAL, "bd_bank_restore: no snapshot of member " + std::to_string(member) + " was taken (bd_bank_snapshot)");
    return copy_member(b, member, false, stream);
}

static int read_pair(bd_bank b, int32_t member, bool grad, float* w_host, float* b_host, const char* who) {
    const int rc = bd::check_member(b, member, who);
    if (rc < 0) return rc;
    BDB_HIP(hipSetDevice(b->device));
    BDB_HIP(hipStreamSynchronize(b->last));
    const bd::Shape& s = b->s;
    const int group = member / s.mpg, ng = (s.mpg < s.M - group * s.mpg ? s.mpg : s.M - group * s.mpg) * s.C;
    const float* src = (grad ? b->grad : b->p) + group * bd::kGroupFloats + (member % s.mpg) * s.C;
    if (w_host)
        BDB_HIP(hipMemcpy2D(w_host, (size_t)s.C * sizeof(float), src, (size_t)ng * sizeof(float), (size_t)s.C * sizeof(float), bd::kIn,
                            hipMemcpyDeviceToHost));
    if (b_host) BDB_HIP(hipMemcpy(b_host, src + (size_t)bd::kIn * ng, (size_t)s.C * sizeof(float), hipMemcpyDeviceToHost));
    return BD_OK;
}

int bd_bank_read(bd_bank b, int32_t member, float* kernel_host, float* bias_host) {
    return read_pair(b, member, false, kernel_host, bias_host, "bd_bank_read");
}

int bd_bank_gradients(bd_bank b, int32_t member, float* dW_host, float* db_host) {
    return read_pair(b, member, true, dW_host, db_host, "bd_bank_gradients");
}

int bd_bank_mean_loss(bd_bank b, int32_t reset, float* mean_host) {
    if (!b || !mean_host) return fail(BD_EINVAL, "bd_bank_mean_loss: null argument");
    BDB_HIP(hipSetDevice(b->device));
    BDB_HIP(hipStreamSynchronize(b->last));
    std::vector<double> acc(2 * (size_t)b->s.M, 0.0);
    BDB_HIP(hipMemcpy(acc.data(), b->acc, acc.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int mb = 0; mb < b->s.M; ++mb) mean_host[mb] = acc[2 * mb + 1] > 0.0 ? (float)(acc[2 * mb] / acc[2 * mb + 1]) : 0.0f;
    if (reset) BDB_HIP(hipMemset(b->acc, 0, acc.size() * sizeof(double)));
    return BD_OK;
}

int64_t bd_bank_workspace_floats(bd_bank b) {
    if (!b) return fail(BD_EINVAL, "bd_bank_workspace_floats: null handle");
    return b->ws_floats;
}

int bd_bank_workspace_fill(bd_bank b, uint32_t pattern) {
    if (!b) return fail(BD_EINVAL, "bd_bank_workspace_fill: null handle");
    BDB_HIP(hipSetDevice(b->device));
    BDB_HIP(hipStreamSynchronize(b->last));
    BDB_HIP(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(b->ws), (int)pattern, (size_t)b->ws_floats));
    BDB_HIP(hipDeviceSynchronize());
    return BD_OK;
}

int bd_bank_workspace_read(bd_bank b, float* host, int64_t floats) {
    if (!b || !host || floats < 0 || floats > b->ws_floats) return fail(BD_EINVAL, "bd_bank_workspace_read: bad argument");
    BDB_HIP(hipSetDevice(b->device));
    BDB_HIP(hipStreamSynchronize(b->last));
    BDB_HIP(hipMemcpy(host, b->ws, (size_t)floats * sizeof(float), hipMemcpyDeviceToHost));
    return BD_OK;
}

}  // extern "C"
