// The classifier-head trainer (include/buzzdetect_train.h): forward, loss, backward and update of a Dense stack on
// embeddings, in exact float32 on v_mfma_f32_32x32x2_f32.
//
//
// The device routines - mma_chain and the tiles built on it, loss_row, the partials' sum and the update - live in
// headtrain_device.h, which headbank.hip includes too.  What differs between the three products is where a lane finds its operands:
//   forward  Y = act(A W + b)      reduce over n_in    A: 16 bytes of a row (row rows[r] of X for layer 0)   B: W[k][col]
//   dA       G' = (G W^T) * act'   reduce over n_out   A: 16 bytes of a row of G                             B: W[col][k]
//   dW       P_s = A^T G           reduce over the rows of slice s   A: A[row][col]                          B: G[row][col]
// The parameters stay row-major [n_in][n_out] + [n_out] (the update writes them every step; no fragment copy to keep in step).
//
// Order of sums (the determinism contract): an output element is one chain of fused multiply-adds in ascending k.  dW reduces
// over the batch: slice s is rows [256 s, 256 s + 256) - kSliceRows, a constant - its partial goes to workspace
// [slice][n_in n_out + n_out], and apply_kernel adds the partials in ascending s before the optimizer's update.  Row losses go
// to a buffer and one workgroup adds them in a fixed tree.  Nothing depends on the grid or the number of compute units.
//
// fused_step_kernel (one layer, n_out <= 64): a workgroup of eight waves owns a slice and calls the same three routines -
// logits of its 256 rows, their deltas, the slice's dW partial - so the partial's second walk over the slice's rows of X finds
// them in the cache the first walk filled: X comes from HBM once per step.
//
// Row weights (bd_trainer_step_weighted): loss_row<true> reads w_r beside the row's target and uses scale_r = inv * w_r where
// the plain pass uses inv, and stores w_r * loss_r; loss_row<false> is the plain pass, instruction for instruction.  The
// weight is a kernel argument, the same for every lane: no lane leaves or branches apart in front of the fused kernel's
// barriers.  Decoupled weight decay is apply_kernel's: p = p - (lr wd) p on a layer's kernel elements (never its bias), two
// roundings, before the optimizer's update is subtracted from p.
#include "headtrain_device.h"

#include <cstring>
#include <memory>
#include <string>

namespace bd {

void set_error(const std::string& msg);     // engine.hip: the text bd_last_error() returns on this thread

namespace {

using namespace train;

// ---- kernels ----

__global__ __launch_bounds__(256) void forward_kernel(const float* __restrict__ A, int64_t lda, const int* __restrict__ rows, int B,
                                                       int K, const float* __restrict__ P, int N, int act, float* __restrict__ Y,
                                                       int ldy) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tr = 2 * blockIdx.x + (wave & 1), tc = 2 * blockIdx.y + (wave >> 1);
    if (32 * tr >= B || 32 * tc >= N) return;           // (no barrier in this kernel)
    forward_tile(A, lda, rows, B, K, P, N, act, Y, ldy, tr, tc, lane);
}

__global__ __launch_bounds__(256) void input_grad_kernel(const float* __restrict__ G, int ldg, int B, int K,
                                                          const float* __restrict__ W, int N, const float* __restrict__ Yp, int act_p,
                                                          float* __restrict__ Gp, int ldp) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tr = 2 * blockIdx.x + (wave & 1), tc = 2 * blockIdx.y + (wave >> 1);
    if (32 * tr >= B || 32 * tc >= K) return;
    input_grad_tile(G, ldg, B, K, W, N, Yp, act_p, Gp, ldp, tr, tc, lane);
}

// grid (ceil(tiles / 4), slices): a wave per 32 x 32 tile of a slice's partial; the waves of the first row of tiles add db
__global__ __launch_bounds__(256) void weight_grad_kernel(const float* __restrict__ A, int64_t lda, const int* __restrict__ rows,
                                                           int B, int K, const float* __restrict__ G, int ldg, int N,
                                                           float* __restrict__ ws) {
    const int lane = threadIdx.x & 63;
    const int tiles_n = (N + 31) / 32, tiles = (K + 31) / 32 * tiles_n;
    const int t = 4 * blockIdx.x + (threadIdx.x >> 6);
    if (t >= tiles) return;
    const int slice = blockIdx.y, r0 = slice * kSliceRows, r1 = min(B, r0 + kSliceRows);
    float* part = ws + (size_t)slice * ((size_t)K * N + N);
    const int tk = t / tiles_n, tn = t % tiles_n;
    weight_grad_tile(A, lda, rows, r0, r1, K, G, ldg, N, part, tk, tn, lane);
    if (tk == 0) bias_grad_tile(G, ldg, r0, r1, N, part + (size_t)K * N, tn, lane);
}

template <bool kWeighted>
__global__ __launch_bounds__(256) void loss_rows_kernel(const float* __restrict__ Z, float* __restrict__ G, int ld, int B, int C,
                                                         int loss, const void* __restrict__ targets,
                                                         const float* __restrict__ row_w, float inv,
                                                         float* __restrict__ row_loss) {
    const int row = 4 * blockIdx.x + (threadIdx.x >> 6);
    if (row >= B) return;
    loss_row<kWeighted>(Z + (size_t)row * ld, G + (size_t)row * ld, C, loss, targets, row_w, row, inv, row_loss, threadIdx.x & 63);
}

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

__global__ __launch_bounds__(256) void loss_sum_kernel(const float* __restrict__ row_loss, int B, double scale, float* __restrict__ out,
                                                        double* __restrict__ acc) {
    __shared__ double part[256];
    loss_sum_block(row_loss, B, scale, out, acc, part);
}

// element i of a layer's [W | b]: the slices' partials in ascending order, then the decay (kernel elements only), then the optimizer
__global__ __launch_bounds__(256) void apply_kernel(const float* __restrict__ ws, int slices, int n, float* __restrict__ grad,
                                                     float* __restrict__ P, float* __restrict__ m, float* __restrict__ v, Update u) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    apply_element(sum_partials(ws + i, slices, (size_t)n), (size_t)i, i < u.decay_n, grad, P, m, v, u);
}

__global__ void fill_kernel(uint32_t* p, size_t n, uint32_t pattern) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = pattern;
}

int fail(int code, const std::string& msg) {
    set_error(msg);
    return code;
}

#define BDT_HIP(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(BD_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct Layer {
    int k, n, act, ld;              // ld = round_up(n, 32): row stride of y and g
    float *p, *grad, *m, *v;        // [k n + n] each: W then b (m, v: Adam only)
    float* snap;                    // [k n + n]: the parameters as bd_trainer_snapshot found them
    float *y, *g;                   // [max_batch][ld]: activations (the last layer's: logits) and d loss / d pre-activation
};

}  // namespace
}  // namespace bd

struct bd_trainer_s {
    int device = 0, n_layers = 0, loss = 0, max_batch = 0;
    bd_train_optimizer opt{};
    int64_t step = 0;
    bool fused = true;
    float weight_decay = 0.0f;
    bool has_snapshot = false;
    bd::Layer layers[BD_HEAD_MAX_LAYERS]{};
    float* pool = nullptr;          // one allocation behind every pointer above and below
    float* ws = nullptr;            // [slices][k n + n] of the layer at work
    int64_t ws_floats = 0;
    float* row_loss = nullptr;      // [max_batch]
    double* acc = nullptr;          // running loss sum, rows
    hipStream_t last = nullptr;
};

namespace bd {
namespace {

bool fusable(const bd_trainer_s* t) { return t->n_layers == 1 && t->layers[0].n <= BD_TRAIN_FUSED_MAX_WIDTH; }

int check_batch(const bd_trainer_s* t, const float* X, int64_t ldx, const void* targets, int32_t B, const char* who) {
    if (!t || !X || !targets) return fail(BD_EINVAL, std::string(who) + ": null argument");
    if (B < 1 || B > t->max_batch) return fail(BD_EINVAL, std::string(who) + ": B must be in 1..max_batch");
    if (ldx < BD_EMBEDDING_SIZE || ldx % 4 || (reinterpret_cast<uintptr_t>(X) & 15u))
        return fail(BD_EINVAL, std::string(who) + ": X needs 16-byte alignment and ldx >= 1024, a multiple of 4");
    return BD_OK;
}

void enqueue_forward(bd_trainer_s* t, const float* X, int64_t ldx, const int* rows, int B, hipStream_t stream) {
    const float* a = X;
    int64_t lda = ldx;
    for (int l = 0; l < t->n_layers; ++l) {
        const Layer& L = t->layers[l];
        const int act = l + 1 < t->n_layers ? L.act : BD_HEAD_LINEAR;
        hipLaunchKernelGGL(forward_kernel, dim3((B + 63) / 64, (L.n + 63) / 64), dim3(256), 0, stream, a, lda, l == 0 ? rows : nullptr,
                           B, L.k, L.p, L.n, act, L.y, L.ld);
        a = L.y;
        lda = L.ld;
    }
}

void enqueue_loss(bd_trainer_s* t, const void* targets, const float* row_w, int B, float* loss_dev, bool accumulate, bool rows_done,
                  hipStream_t stream) {
    const Layer& L = t->layers[t->n_layers - 1];
    const bool binary = t->loss == BD_TRAIN_BINARY;
    if (!rows_done) {
        const float inv = 1.0f / (binary ? (float)B * (float)L.n : (float)B);
        if (row_w)
            hipLaunchKernelGGL(loss_rows_kernel<true>, dim3((B + 3) / 4), dim3(256), 0, stream, L.y, L.g, L.ld, B, L.n, t->loss,
                               targets, row_w, inv, t->row_loss);
        else
            hipLaunchKernelGGL(loss_rows_kernel<false>, dim3((B + 3) / 4), dim3(256), 0, stream, L.y, L.g, L.ld, B, L.n, t->loss,
                               targets, row_w, inv, t->row_loss);
    }
    hipLaunchKernelGGL(loss_sum_kernel, dim3(1), dim3(256), 0, stream, t->row_loss, B, 1.0 / (binary ? (double)B * L.n : (double)B),
                       loss_dev, accumulate ? t->acc : nullptr);
}

}  // namespace
}  // namespace bd

using bd::fail;

extern "C" {

int bd_train_abi_version(void) { return BD_TRAIN_ABI_VERSION; }

int bd_trainer_create(int device, const bd_head_layer* layers, int32_t n_layers, int32_t loss, const bd_train_optimizer* opt,
                      int32_t max_batch, bd_trainer* out) {
    if (!out || !layers || !opt) return fail(BD_EINVAL, "bd_trainer_create: null argument");
    *out = nullptr;
    if (n_layers < 1 || n_layers > BD_HEAD_MAX_LAYERS) return fail(BD_EINVAL, "bd_trainer_create: n_layers must be in 1..8");
    if (loss != BD_TRAIN_CATEGORICAL && loss != BD_TRAIN_BINARY) return fail(BD_EINVAL, "bd_trainer_create: unknown loss");
    if (opt->kind != BD_TRAIN_SGD && opt->kind != BD_TRAIN_ADAM) return fail(BD_EINVAL, "bd_trainer_create: unknown optimizer");
    if (!(opt->learning_rate > 0.0f) || !std::isfinite(opt->learning_rate))
        return fail(BD_EINVAL, "bd_trainer_create: learning_rate must be positive and finite");
    if (opt->kind == BD_TRAIN_ADAM && !(opt->beta_1 >= 0.0f && opt->beta_1 < 1.0f && opt->beta_2 >= 0.0f && opt->beta_2 < 1.0f &&
                                        opt->epsilon > 0.0f))
        return fail(BD_EINVAL, "bd_trainer_create: Adam needs 0 <= beta < 1 and epsilon > 0");
    if (max_batch < 1 || max_batch > BD_TRAIN_MAX_BATCH) return fail(BD_EINVAL, "bd_trainer_create: max_batch must be in 1..65536");
    for (int l = 0; l < n_layers; ++l) {
        const bd_head_layer& L = layers[l];
        const std::string where = "bd_trainer_create: layer " + std::to_string(l);
        if (!L.kernel) return fail(BD_EINVAL, where + " has no kernel");
        if (L.n_in != (l == 0 ? BD_EMBEDDING_SIZE : layers[l - 1].n_out))
            return fail(BD_EINVAL, where + ": n_in must be 1024 for the first layer, the width before it for the others");
        if (L.n_out < 1 || L.n_out > BD_HEAD_MAX_WIDTH) return fail(BD_EINVAL, where + ": n_out must be in 1..2048");
        if (L.activation < BD_HEAD_LINEAR || L.activation > BD_HEAD_SOFTMAX || (L.activation == BD_HEAD_SOFTMAX && l + 1 < n_layers))
            return fail(BD_EINVAL, where + ": hidden activations are linear, relu, sigmoid or tanh");
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(BD_ENODEVICE, "bd_trainer_create: no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= count) return fail(BD_ENODEVICE, "bd_trainer_create: device index out of range");
    hipDeviceProp_t prop;
    BDT_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(BD_ENODEVICE, std::string("bd_trainer_create: kernels are built for gfx950 only, device is ") + prop.gcnArchName);
    BDT_HIP(hipSetDevice(device));

    std::unique_ptr<bd_trainer_s> t(new bd_trainer_s);
    t->device = device;
    t->n_layers = n_layers;
    t->loss = loss;
    t->max_batch = max_batch;
    t->opt = *opt;
    const bool adam = opt->kind == BD_TRAIN_ADAM;
    const int64_t slices = (max_batch + bd::kSliceRows - 1) / bd::kSliceRows;
    // lay the pool out in floats, every piece on a 64-float boundary
    auto up64 = [](int64_t v) { return (v + 63) / 64 * 64; };
    int64_t total = 0, params_max = 0;
    int64_t off_p[BD_HEAD_MAX_LAYERS], off_y[BD_HEAD_MAX_LAYERS];
    for (int l = 0; l < n_layers; ++l) {
        bd::Layer& L = t->layers[l];
        L.k = layers[l].n_in;
        L.n = layers[l].n_out;
        L.act = layers[l].activation;
        L.ld = (L.n + 31) / 32 * 32;
        const int64_t np = (int64_t)L.k * L.n + L.n;
        params_max = np > params_max ? np : params_max;
        off_p[l] = total;
        total += up64(np) * (adam ? 5 : 3);
        off_y[l] = total;
        total += up64((int64_t)max_batch * L.ld) * 2;
    }
    const int64_t off_ws = total;
    t->ws_floats = slices * params_max;
    total += up64(t->ws_floats);
    const int64_t off_rl = total;
    total += up64(max_batch);
    const int64_t off_acc = total;
    total += 64;
    BDT_HIP(hipMalloc(&t->pool, (size_t)total * sizeof(float)));
    hipError_t err = hipMemset(t->pool, 0, (size_t)total * sizeof(float));
    for (int l = 0; l < n_layers && err == hipSuccess; ++l) {
        bd::Layer& L = t->layers[l];
        const int64_t np = (int64_t)L.k * L.n + L.n, step = up64(np);
        L.p = t->pool + off_p[l];
        L.grad = L.p + step;
        L.m = adam ? L.p + 2 * step : nullptr;
        L.v = adam ? L.p + 3 * step : nullptr;
        L.snap = L.p + (adam ? 4 : 2) * step;
        L.y = t->pool + off_y[l];
        L.g = L.y + up64((int64_t)max_batch * L.ld);
        err = hipMemcpy(L.p, layers[l].kernel, (size_t)L.k * L.n * sizeof(float), hipMemcpyHostToDevice);
        if (err == hipSuccess && layers[l].bias)
            err = hipMemcpy(L.p + (size_t)L.k * L.n, layers[l].bias, (size_t)L.n * sizeof(float), hipMemcpyHostToDevice);
    }
    if (err != hipSuccess) {
        (void)hipFree(t->pool);
        return fail(BD_EHIP, std::string("bd_trainer_create: ") + hipGetErrorString(err));
    }
    t->ws = t->pool + off_ws;
    t->row_loss = t->pool + off_rl;
    t->acc = reinterpret_cast<double*>(t->pool + off_acc);
    *out = t.release();
    return BD_OK;
}

int bd_trainer_destroy(bd_trainer t) {
    if (!t) return BD_OK;
    (void)hipSetDevice(t->device);
    (void)hipStreamSynchronize(t->last);
    if (t->pool) (void)hipFree(t->pool);
    delete t;
    return BD_OK;
}

int bd_trainer_set_fusion(bd_trainer t, int32_t fused) {
    if (!t) return fail(BD_EINVAL, "bd_trainer_set_fusion: null handle");
    t->fused = fused != 0;
    return BD_OK;
}

// bd_trainer_step (row_w == nullptr: the plain kernels) and bd_trainer_step_weighted
static int do_step(bd_trainer t, const float* X, int64_t ldx, const int32_t* rows, const void* targets, const float* row_w, int32_t B,
                   void* stream_, const char* who) {
    const int rc = bd::check_batch(t, X, ldx, targets, B, who);
    if (rc < 0) return rc;
    if (reinterpret_cast<uintptr_t>(row_w) & 3u) return fail(BD_EINVAL, std::string(who) + ": row_weights is not aligned to a float");
    BDT_HIP(hipSetDevice(t->device));
    hipStream_t stream = (hipStream_t)stream_;
    t->last = stream;
    const int slices = (B + bd::kSliceRows - 1) / bd::kSliceRows;
    const bool binary = t->loss == BD_TRAIN_BINARY;
    t->step += 1;
    bd::Update u{t->opt.kind, t->opt.learning_rate, t->opt.beta_1, t->opt.beta_2, t->opt.epsilon, 0.0f,
                 t->weight_decay != 0.0f ? t->opt.learning_rate * t->weight_decay : 0.0f, 0};
    if (u.kind == BD_TRAIN_ADAM)
        u.lr_t = (float)((double)u.lr * std::sqrt(1.0 - std::pow((double)u.b2, (double)t->step)) /
                         (1.0 - std::pow((double)u.b1, (double)t->step)));
    const bool fused = t->fused && bd::fusable(t);
    if (fused) {
        const bd::Layer& L = t->layers[0];
        const float inv = 1.0f / (binary ? (float)B * (float)L.n : (float)B);
        if (row_w)
            hipLaunchKernelGGL(bd::fused_step_kernel<true>, dim3(slices), dim3(512), 0, stream, X, ldx, rows, B, L.k, L.p, L.n, L.y,
                               L.g, L.ld, t->loss, targets, row_w, inv, t->row_loss, t->ws);
        else
            hipLaunchKernelGGL(bd::fused_step_kernel<false>, dim3(slices), dim3(512), 0, stream, X, ldx, rows, B, L.k, L.p, L.n, L.y,
                               L.g, L.ld, t->loss, targets, row_w, inv, t->row_loss, t->ws);
    } else {
        bd::enqueue_forward(t, X, ldx, rows, B, stream);
    }
    bd::enqueue_loss(t, targets, row_w, B, nullptr, true, fused, stream);
    for (int l = t->n_layers - 1; l >= 0; --l) {
        const bd::Layer& L = t->layers[l];
        const int n = L.k * L.n + L.n;
        if (!fused) {
            const float* a = l == 0 ? X : t->layers[l - 1].y;
            const int64_t lda = l == 0 ? ldx : t->layers[l - 1].ld;
            const int tiles = (L.k + 31) / 32 * ((L.n + 31) / 32);
            hipLaunchKernelGGL(bd::weight_grad_kernel, dim3((tiles + 3) / 4, slices), dim3(256), 0, stream, a, lda,
                               l == 0 ? rows : nullptr, B, L.k, L.g, L.ld, L.n, t->ws);
        }
        if (l > 0) {                                     // with this layer's weights as the forward pass saw them
            const bd::Layer& Lp = t->layers[l - 1];
            hipLaunchKernelGGL(bd::input_grad_kernel, dim3((B + 63) / 64, (L.k + 63) / 64), dim3(256), 0, stream, L.g, L.ld, B, L.k,
                               L.p, L.n, Lp.y, Lp.act, Lp.g, Lp.ld);
        }
        u.decay_n = L.k * L.n;
        hipLaunchKernelGGL(bd::apply_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, t->ws, slices, n, L.grad, L.p, L.m, L.v, u);
    }
    BDT_HIP(hipGetLastError());
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
    const int rc = bd::check_batch(t, X, ldx, targets, B, who);
    if (rc < 0) return rc;
    if (reinterpret_cast<uintptr_t>(row_w) & 3u) return fail(BD_EINVAL, std::string(who) + ": row_weights is not aligned to a float");
    if (!loss_dev) return fail(BD_EINVAL, std::string(who) + ": null loss_dev");
    BDT_HIP(hipSetDevice(t->device));
    hipStream_t stream = (hipStream_t)stream_;
    t->last = stream;
    bd::enqueue_forward(t, X, ldx, rows, B, stream);
    bd::enqueue_loss(t, targets, row_w, B, loss_dev, false, false, stream);
    BDT_HIP(hipGetLastError());
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
    if (!t) return fail(BD_EINVAL, "bd_trainer_set_weight_decay: null handle");
    if (!(weight_decay >= 0.0f) || !std::isfinite(weight_decay))
        return fail(BD_EINVAL, "bd_trainer_set_weight_decay: weight_decay must be finite and not negative");
    t->weight_decay = weight_decay;
    return BD_OK;
}

int bd_trainer_set_learning_rate(bd_trainer t, float learning_rate) {
    if (!t) return fail(BD_EINVAL, "bd_trainer_set_learning_rate: null handle");
    if (!(learning_rate > 0.0f) || !std::isfinite(learning_rate))
        return fail(BD_EINVAL, "bd_trainer_set_learning_rate: learning_rate must be positive and finite");
    t->opt.learning_rate = learning_rate;
    return BD_OK;
}

// parameters -> snapshot (to_snapshot) or back, layer by layer, on the caller's stream
static int copy_parameters(bd_trainer t, bool to_snapshot, void* stream_) {
    BDT_HIP(hipSetDevice(t->device));
    hipStream_t stream = (hipStream_t)stream_;
    t->last = stream;
    for (int l = 0; l < t->n_layers; ++l) {
        const bd::Layer& L = t->layers[l];
        const size_t bytes = ((size_t)L.k * L.n + L.n) * sizeof(float);
        BDT_HIP(hipMemcpyAsync(to_snapshot ? L.snap : L.p, to_snapshot ? L.p : L.snap, bytes, hipMemcpyDeviceToDevice, stream));
    }
    return BD_OK;
}

int bd_trainer_snapshot(bd_trainer t, void* stream) {
    if (!t) return fail(BD_EINVAL, "bd_trainer_snapshot: null handle");
    const int rc = copy_parameters(t, true, stream);
    if (rc == BD_OK) t->has_snapshot = true;
    return rc;
}

int bd_trainer_restore(bd_trainer t, void* stream) {
    if (!t) return fail(BD_EINVAL, "bd_trainer_restore: null handle");
    if (!t->has_snapshot) return fail(BD_EINVAL, "bd_trainer_restore: no snapshot was taken (bd_trainer_snapshot)");
    return copy_parameters(t, false, stream);
}

static int read_pair(bd_trainer t, int32_t layer, bool grad, float* w_host, float* b_host, const char* who) {
    if (!t || layer < 0 || layer >= t->n_layers) return fail(BD_EINVAL, std::string(who) + ": no such layer");
    BDT_HIP(hipSetDevice(t->device));
    BDT_HIP(hipStreamSynchronize(t->last));
    const bd::Layer& L = t->layers[layer];
    const float* src = grad ? L.grad : L.p;
    if (w_host) BDT_HIP(hipMemcpy(w_host, src, (size_t)L.k * L.n * sizeof(float), hipMemcpyDeviceToHost));
    if (b_host) BDT_HIP(hipMemcpy(b_host, src + (size_t)L.k * L.n, (size_t)L.n * sizeof(float), hipMemcpyDeviceToHost));
    return BD_OK;
}

int bd_trainer_gradients(bd_trainer t, int32_t layer, float* dW_host, float* db_host) {
    return read_pair(t, layer, true, dW_host, db_host, "bd_trainer_gradients");
}

int bd_trainer_read(bd_trainer t, int32_t layer, float* kernel_host, float* bias_host) {
    return read_pair(t, layer, false, kernel_host, bias_host, "bd_trainer_read");
}

int bd_trainer_logits(bd_trainer t, int32_t B, float* logits_host) {
    if (!t || !logits_host || B < 1 || B > t->max_batch) return fail(BD_EINVAL, "bd_trainer_logits: bad argument");
    BDT_HIP(hipSetDevice(t->device));
    BDT_HIP(hipStreamSynchronize(t->last));
    const bd::Layer& L = t->layers[t->n_layers - 1];
    BDT_HIP(hipMemcpy2D(logits_host, (size_t)L.n * sizeof(float), L.y, (size_t)L.ld * sizeof(float), (size_t)L.n * sizeof(float), B,
                        hipMemcpyDeviceToHost));
    return BD_OK;
}

int bd_trainer_mean_loss(bd_trainer t, int32_t reset, float* mean_host) {
    if (!t || !mean_host) return fail(BD_EINVAL, "bd_trainer_mean_loss: null argument");
    BDT_HIP(hipSetDevice(t->device));
    BDT_HIP(hipStreamSynchronize(t->last));
    double acc[2] = {0.0, 0.0};
    BDT_HIP(hipMemcpy(acc, t->acc, sizeof(acc), hipMemcpyDeviceToHost));
    *mean_host = acc[1] > 0.0 ? (float)(acc[0] / acc[1]) : 0.0f;
    if (reset) BDT_HIP(hipMemset(t->acc, 0, sizeof(acc)));
    return BD_OK;
}

int64_t bd_trainer_workspace_floats(bd_trainer t) {
    if (!t) return fail(BD_EINVAL, "bd_trainer_workspace_floats: null handle");
    return t->ws_floats;
}

int bd_trainer_workspace_fill(bd_trainer t, uint32_t pattern) {
    if (!t) return fail(BD_EINVAL, "bd_trainer_workspace_fill: null handle");
    BDT_HIP(hipSetDevice(t->device));
    BDT_HIP(hipStreamSynchronize(t->last));
    hipLaunchKernelGGL(bd::fill_kernel, dim3(256), dim3(256), 0, t->last, reinterpret_cast<uint32_t*>(t->ws), (size_t)t->ws_floats,
                       pattern);
    BDT_HIP(hipGetLastError());
    BDT_HIP(hipStreamSynchronize(t->last));
    return BD_OK;
}

int bd_trainer_workspace_read(bd_trainer t, float* host, int64_t floats) {
    if (!t || !host || floats < 0 || floats > t->ws_floats) return fail(BD_EINVAL, "bd_trainer_workspace_read: bad argument");
    BDT_HIP(hipSetDevice(t->device));
    BDT_HIP(hipStreamSynchronize(t->last));
    BDT_HIP(hipMemcpy(host, t->ws, (size_t)floats * sizeof(float), hipMemcpyDeviceToHost));
    return BD_OK;
}

}  // extern "C"
