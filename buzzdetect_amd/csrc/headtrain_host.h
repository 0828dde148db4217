// Host side of the classifier-head trainers, shared by headtrain.hip (one stack: include/buzzdetect_train.h), headbank.hip (a
// bank of one-layer heads: include/buzzdetect_bank.h) and stackbank.hip (a bank of Dense stacks:
// include/buzzdetect_stackbank.h), as headtrain_device.h is the one copy of their device routines.  Host code only: no kernel
// and no device routine lives here (the layer-by-layer route of Dense stacks, kernels and launches, is headtrain_stack.h's).
// What the three files keep is what differs between the products - the kernels that are theirs alone, the layout of their
// pools and their entry points; what they check, how a member's rate, decay, frozen flag, snapshot flag and step count are
// kept and become launch arguments, where the pieces of a Dense stack lie, and how the running losses and the workspace are
// read is written here once.
//
// The bias-corrected Adam rate (adam_rate) is part of the bit contract between a trainer and a member of a bank: it is a
// double expression rounded to float once, and this is its only copy.
#ifndef BD_HEADTRAIN_HOST_H
#define BD_HEADTRAIN_HOST_H

#include "headtrain_device.h"
#include "bd_error.h"

#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace bd {
namespace {

using namespace train;

// ---- a launch's members ----

constexpr int kMembersPerLaunch = 64;

// The members first .. first + count of a launch, by value.  kCapacity: kMembersPerLaunch for a bank's launches, 1 for a
// launch of exactly one member (the lone trainer, a stack bank's last member alone), a block of 24 bytes instead of 1 KiB.
template <int kCapacity>
struct Members {
    int first, count;
    float lr[kCapacity], lr_t[kCapacity], decay[kCapacity];
    int frozen[kCapacity];
};

// the launch that starts at member `first` of M: its range, nothing else set
template <int kCapacity = kMembersPerLaunch>
Members<kCapacity> members_from(int M, int first) {
    Members<kCapacity> a{};
    a.first = first;
    a.count = M - first < kCapacity ? M - first : kCapacity;
    return a;
}

// lr sqrt(1 - beta_2^t) / (1 - beta_1^t) of step t >= 1, in double, rounded to float once
float adam_rate(float lr, float beta_1, float beta_2, int64_t step) {
    return (float)((double)lr * std::sqrt(1.0 - std::pow((double)beta_2, (double)step)) / (1.0 - std::pow((double)beta_1, (double)step)));
}

// What the host keeps per member (the lone trainer: of its one member) between the calls.
struct MemberState {
    std::vector<float> lr, wd;
    std::vector<int> frozen, has_snapshot;
    std::vector<int64_t> step;

    void assign(int M, float learning_rate) {
        lr.assign(M, learning_rate);
        wd.assign(M, 0.0f);
        frozen.assign(M, 0);
        has_snapshot.assign(M, 0);
        step.assign(M, 0);
    }
    int size() const { return (int)lr.size(); }

    void advance() {                // a step begins: the members that are not frozen count it
        for (size_t mb = 0; mb < step.size(); ++mb)
            if (!frozen[mb]) step[mb] += 1;
    }

    // member mb's update as the host has it now (step counts already advanced); decay_n is the caller's
    Update update_of(const bd_train_optimizer& opt, int mb) const {
        Update u{opt.kind, lr[mb], opt.beta_1, opt.beta_2, opt.epsilon, 0.0f, wd[mb] != 0.0f ? lr[mb] * wd[mb] : 0.0f, 0};
        if (opt.kind == BD_TRAIN_ADAM && step[mb] > 0) u.lr_t = adam_rate(u.lr, u.b1, u.b2, step[mb]);
        return u;
    }

    // the launch arguments of the members from `first` on
    template <int kCapacity = kMembersPerLaunch>
    Members<kCapacity> launch_args(const bd_train_optimizer& opt, int first) const {
        Members<kCapacity> a = members_from<kCapacity>(size(), first);
        for (int j = 0; j < a.count; ++j) {
            const Update u = update_of(opt, first + j);
            a.lr[j] = u.lr;
            a.lr_t[j] = u.lr_t;
            a.decay[j] = u.decay;
            a.frozen[j] = frozen[first + j];
        }
        return a;
    }
};

// ---- what the three handles share ----

struct TrainHandle {
    int device = 0, loss = 0, max_batch = 0;
    bd_train_optimizer opt{};       // kind, betas, epsilon; learning_rate: the members' first
    MemberState members;
    float* pool = nullptr;          // the one allocation behind every pointer and offset of the handle
    float* ws = nullptr;            // the slices' dW / db partials
    int64_t ws_floats = 0;
    double* acc = nullptr;          // [members][2]: running loss sum, rows
    hipStream_t last = nullptr;     // the stream of the last call that enqueued
};

// the prologue of a call that enqueues: the handle's device, the caller's stream, remembered for the calls that wait
int enter(TrainHandle* h, void* stream_, hipStream_t* stream) {
    BD_HIP(hipSetDevice(h->device));
    *stream = (hipStream_t)stream_;
    h->last = *stream;
    return BD_OK;
}

// the prologue of a call that reads: the handle's device, everything enqueued so far done
int enter_and_wait(const TrainHandle* h) {
    BD_HIP(hipSetDevice(h->device));
    BD_HIP(hipStreamSynchronize(h->last));
    return BD_OK;
}

// ---- checks of *_create, in the order the headers document: before a device is looked for ----

int check_training_setup(const std::string& who, int32_t loss, const bd_train_optimizer* opt, int32_t max_batch) {
    if (loss != BD_TRAIN_CATEGORICAL && loss != BD_TRAIN_BINARY) return fail(BD_EINVAL, who + ": unknown loss");
    if (opt->kind != BD_TRAIN_SGD && opt->kind != BD_TRAIN_ADAM) return fail(BD_EINVAL, who + ": unknown optimizer");
    if (!(opt->learning_rate > 0.0f) || !std::isfinite(opt->learning_rate))
        return fail(BD_EINVAL, who + ": learning_rate must be positive and finite");
    if (opt->kind == BD_TRAIN_ADAM && !(opt->beta_1 >= 0.0f && opt->beta_1 < 1.0f && opt->beta_2 >= 0.0f && opt->beta_2 < 1.0f &&
                                        opt->epsilon > 0.0f))
        return fail(BD_EINVAL, who + ": Adam needs 0 <= beta < 1 and epsilon > 0");
    if (max_batch < 1 || max_batch > BD_TRAIN_MAX_BATCH) return fail(BD_EINVAL, who + ": max_batch must be in 1..65536");
    return BD_OK;
}

// One Dense stack 1024 -> ... ; a message starts with `where` and the layer's number.  `like`: the stack whose widths and
// hidden activations this one must have (a bank's first member), compared layer by layer behind the layer's own checks.
int check_stack(const std::string& where, const bd_head_layer* layers, int n_layers, const bd_head_layer* like = nullptr) {
    for (int l = 0; l < n_layers; ++l) {
        const bd_head_layer& L = layers[l];
        const std::string at = where + std::to_string(l);
        if (!L.kernel) return fail(BD_EINVAL, at + " has no kernel");
        if (L.n_in != (l == 0 ? BD_EMBEDDING_SIZE : layers[l - 1].n_out))
            return fail(BD_EINVAL, at + ": n_in must be 1024 for the first layer, the width before it for the others");
        if (L.n_out < 1 || L.n_out > BD_HEAD_MAX_WIDTH) return fail(BD_EINVAL, at + ": n_out must be in 1..2048");
        if (L.activation < BD_HEAD_LINEAR || L.activation > BD_HEAD_SOFTMAX || (L.activation == BD_HEAD_SOFTMAX && l + 1 < n_layers))
            return fail(BD_EINVAL, at + ": hidden activations are linear, relu, sigmoid or tanh");
        if (like && (L.n_out != like[l].n_out || (l + 1 < n_layers && L.activation != like[l].activation)))
            return fail(BD_EINVAL, at + ": every member has the first member's widths and hidden activations");
    }
    return BD_OK;
}

// the device of a handle to be: it exists, it is a gfx950, and it is the current one from here on
int select_device(const std::string& who, int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(BD_ENODEVICE, who + ": no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= count) return fail(BD_ENODEVICE, who + ": device index out of range");
    hipDeviceProp_t prop;
    BD_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(BD_ENODEVICE, who + ": kernels are built for gfx950 only, device is " + prop.gcnArchName);
    BD_HIP(hipSetDevice(device));
    return BD_OK;
}

// ---- checks of the calls on a live handle ----

int check_member(const TrainHandle* h, int32_t member, const char* who) {
    if (!h) return fail(BD_EINVAL, std::string(who) + ": null handle");
    if (member < 0 || member >= h->members.size()) return fail(BD_EINVAL, std::string(who) + ": no such member");
    return BD_OK;
}

int check_batch(const char* who, int max_batch, const float* X, int64_t ldx, int32_t B) {
    if (B < 1 || B > max_batch) return fail(BD_EINVAL, std::string(who) + ": B must be in 1..max_batch");
    if (ldx < BD_EMBEDDING_SIZE || ldx % 4 || (reinterpret_cast<uintptr_t>(X) & 15u))
        return fail(BD_EINVAL, std::string(who) + ": X needs 16-byte alignment and ldx >= 1024, a multiple of 4");
    return BD_OK;
}

// row_w: nullptr (the unweighted kernels) or the members' rows of weights, ldw apart (the lone trainer: one row, ldw = B)
int check_row_weights(const char* who, const float* row_w, int64_t ldw, int32_t B) {
    if (!row_w) return BD_OK;
    if (reinterpret_cast<uintptr_t>(row_w) & 3u) return fail(BD_EINVAL, std::string(who) + ": row_weights is not aligned to a float");
    if (ldw < B) return fail(BD_EINVAL, std::string(who) + ": ldw must be at least B");
    return BD_OK;
}

// ---- per-member settings: the lone trainer's is member 0 ----

int set_learning_rate(TrainHandle* h, int32_t member, float learning_rate, const char* who) {
    const int rc = check_member(h, member, who);
    if (rc < 0) return rc;
    if (!(learning_rate > 0.0f) || !std::isfinite(learning_rate))
        return fail(BD_EINVAL, std::string(who) + ": learning_rate must be positive and finite");
    h->members.lr[member] = learning_rate;
    return BD_OK;
}

int set_weight_decay(TrainHandle* h, int32_t member, float weight_decay, const char* who) {
    const int rc = check_member(h, member, who);
    if (rc < 0) return rc;
    if (!(weight_decay >= 0.0f) || !std::isfinite(weight_decay))
        return fail(BD_EINVAL, std::string(who) + ": weight_decay must be finite and not negative");
    h->members.wd[member] = weight_decay;
    return BD_OK;
}

int set_frozen(TrainHandle* h, int32_t member, int32_t frozen, const char* who) {
    const int rc = check_member(h, member, who);
    if (rc < 0) return rc;
    if (frozen != 0 && frozen != 1) return fail(BD_EINVAL, std::string(who) + ": frozen must be 0 or 1");
    h->members.frozen[member] = frozen;
    return BD_OK;
}

// bd_*_snapshot / bd_*_restore of a bank's member around the product's copy(member, to_snapshot, stream)
template <class H, class Copy>
int snapshot_member(H* h, int32_t member, void* stream, const char* who, Copy copy) {
    int rc = check_member(h, member, who);
    if (rc < 0) return rc;
    rc = copy(h, member, true, stream);
    if (rc == BD_OK) h->members.has_snapshot[member] = 1;
    return rc;
}

template <class H, class Copy>
int restore_member(H* h, int32_t member, void* stream, const char* who, const char* snapshot_call, Copy copy) {
    const int rc = check_member(h, member, who);
    if (rc < 0) return rc;
    if (!h->members.has_snapshot[member])
        return fail(BD_EINVAL, std::string(who) + ": no snapshot of member " + std::to_string(member) + " was taken (" + snapshot_call + ")");
    return copy(h, member, false, stream);
}

// ---- the loss's two divisors: B rows, or B rows x C outputs for the binary loss ----

float loss_inv(int loss, int B, int C) { return 1.0f / (loss == BD_TRAIN_BINARY ? (float)B * (float)C : (float)B); }
double loss_scale(int loss, int B, int C) { return 1.0 / (loss == BD_TRAIN_BINARY ? (double)B * C : (double)B); }

int slices_of(int B) { return (B + kSliceRows - 1) / kSliceRows; }

// ---- where the pieces of a Dense stack lie: offsets in floats, every piece on a 64-float boundary ----

int64_t up64(int64_t v) { return (v + 63) / 64 * 64; }

struct StackLayer {
    int k, n, act, ld;              // ld = round_up(n, 32): row stride of y and g
    int64_t p, grad, m, v, snap;    // [k n + n] each: W then b (m, v: Adam only, else -1)
    int64_t y, g;                   // [max_batch][ld]: activations (the last layer's: logits) and d loss / d pre-activation
    int64_t params() const { return (int64_t)k * n + n; }
};

struct StackLayout {
    int n_layers = 0;
    StackLayer layers[BD_HEAD_MAX_LAYERS]{};
    int64_t floats = 0;             // the end of the last layer's pieces
    int64_t params_max = 0;         // the largest layer's k n + n (not rounded)
    const StackLayer& last() const { return layers[n_layers - 1]; }
};

StackLayout stack_layout(const bd_head_layer* layers, int n_layers, bool adam, int max_batch) {
    StackLayout s;
    s.n_layers = n_layers;
    for (int l = 0; l < n_layers; ++l) {
        StackLayer& L = s.layers[l];
        L.k = layers[l].n_in;
        L.n = layers[l].n_out;
        L.act = layers[l].activation;
        L.ld = (L.n + 31) / 32 * 32;
        s.params_max = L.params() > s.params_max ? L.params() : s.params_max;
        const int64_t np = up64(L.params()), rows = up64((int64_t)max_batch * L.ld);
        L.p = s.floats;
        L.grad = L.p + np;
        L.m = adam ? L.p + 2 * np : -1;
        L.v = adam ? L.p + 3 * np : -1;
        L.snap = L.p + (adam ? 4 : 2) * np;
        L.y = L.p + (adam ? 5 : 3) * np;
        L.g = L.y + rows;
        s.floats = L.g + rows;
    }
    return s;
}

float* slot(float* block, int64_t off) { return off < 0 ? nullptr : block + off; }      // m, v: nullptr without Adam

// the initial values of one stack (a missing bias: the zeros the pool was cleared to) into its block
hipError_t upload_stack(float* block, const StackLayout& s, const bd_head_layer* layers) {
    hipError_t err = hipSuccess;
    for (int l = 0; l < s.n_layers && err == hipSuccess; ++l) {
        const StackLayer& L = s.layers[l];
        err = hipMemcpy(block + L.p, layers[l].kernel, (size_t)L.k * L.n * sizeof(float), hipMemcpyHostToDevice);
        if (err == hipSuccess && layers[l].bias)
            err = hipMemcpy(block + L.p + (size_t)L.k * L.n, layers[l].bias, (size_t)L.n * sizeof(float), hipMemcpyHostToDevice);
    }
    return err;
}

// a stack's parameters -> its snapshot (to_snapshot) or back, layer by layer, on the stream
int copy_stack(float* block, const StackLayout& s, bool to_snapshot, hipStream_t stream) {
    for (int l = 0; l < s.n_layers; ++l) {
        const StackLayer& L = s.layers[l];
        float *p = block + L.p, *snap = block + L.snap;
        BD_HIP(hipMemcpyAsync(to_snapshot ? snap : p, to_snapshot ? p : snap, (size_t)L.params() * sizeof(float),
                                    hipMemcpyDeviceToDevice, stream));
    }
    return BD_OK;
}

// a layer's (kernel, bias) or (dW, db) of the stack in `block` to the host; either pointer may be null
int read_stack_pair(const TrainHandle* h, const float* block, const StackLayer& L, bool grad, float* w_host, float* b_host) {
    const int rc = enter_and_wait(h);
    if (rc < 0) return rc;
    const float* src = block + (grad ? L.grad : L.p);
    if (w_host) BD_HIP(hipMemcpy(w_host, src, (size_t)L.k * L.n * sizeof(float), hipMemcpyDeviceToHost));
    if (b_host) BD_HIP(hipMemcpy(b_host, src + (size_t)L.k * L.n, (size_t)L.n * sizeof(float), hipMemcpyDeviceToHost));
    return BD_OK;
}

// ---- the ends of the three families: running losses, the workspace's test hooks, destroy ----

int mean_losses(const TrainHandle* h, int32_t reset, float* mean_host, const char* who) {
    if (!h || !mean_host) return fail(BD_EINVAL, std::string(who) + ": null argument");
    const int rc = enter_and_wait(h);
    if (rc < 0) return rc;
    const int M = h->members.size();
    std::vector<double> acc(2 * (size_t)M, 0.0);
    BD_HIP(hipMemcpy(acc.data(), h->acc, acc.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int mb = 0; mb < M; ++mb) mean_host[mb] = acc[2 * mb + 1] > 0.0 ? (float)(acc[2 * mb] / acc[2 * mb + 1]) : 0.0f;
    if (reset) BD_HIP(hipMemset(h->acc, 0, acc.size() * sizeof(double)));
    return BD_OK;
}

int64_t workspace_floats(const TrainHandle* h, const char* who) {
    if (!h) return fail(BD_EINVAL, std::string(who) + ": null handle");
    return h->ws_floats;
}

int workspace_fill(const TrainHandle* h, uint32_t pattern, const char* who) {
    if (!h) return fail(BD_EINVAL, std::string(who) + ": null handle");
    const int rc = enter_and_wait(h);
    if (rc < 0) return rc;
    BD_HIP(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(h->ws), (int)pattern, (size_t)h->ws_floats));
    BD_HIP(hipDeviceSynchronize());
    return BD_OK;
}

int workspace_read(const TrainHandle* h, float* host, int64_t floats, const char* who) {
    if (!h || !host || floats < 0 || floats > h->ws_floats) return fail(BD_EINVAL, std::string(who) + ": bad argument");
    const int rc = enter_and_wait(h);
    if (rc < 0) return rc;
    BD_HIP(hipMemcpy(host, h->ws, (size_t)floats * sizeof(float), hipMemcpyDeviceToHost));
    return BD_OK;
}

template <class H>
int destroy(H* h) {
    if (!h) return BD_OK;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->last);
    if (h->pool) (void)hipFree(h->pool);
    delete h;
    return BD_OK;
}

}  // namespace
}  // namespace bd

#endif  // BD_HEADTRAIN_HOST_H
