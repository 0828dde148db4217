/*
 * buzzdetect_train.h — C ABI of the classifier-head trainer in libbuzzdetect_hip.so (gfx950).
 *
 * The engine runs whatever Dense stack lies in models/<name> (buzzdetect_head.h); this header fits one.  The data are
 * embeddings, not audio, so a trainer is a handle of its own and needs no bd_handle:
 *
 *   y_0 = a row of X,  y_k = act_k(y_{k-1} W_k + b_k),  k = 1 .. n_layers,  the last layer always raw logits
 *
 * on the stacks bd_head_attach accepts (at most BD_HEAD_MAX_LAYERS layers, widths 1..BD_HEAD_MAX_WIDTH, first n_in
 * BD_EMBEDDING_SIZE; hidden activations linear / ReLU / sigmoid / tanh).  The last layer's activation field is not used
 * while training: `loss` says how its logits are read.
 *
 *   BD_TRAIN_CATEGORICAL   softmax cross-entropy from logits, int32 labels [B], mean over the batch:
 *                          loss_r = max_c z + log(sum_c exp(z_c - max)) - z_label,  dz = (softmax(z) - onehot) / B
 *   BD_TRAIN_BINARY        sigmoid cross-entropy from logits, float multi-hot targets [B][C], mean over batch x classes:
 *                          loss_rc = max(z, 0) - z t + log1p(exp(-|z|)),            dz = (sigmoid(z) - t) / (B C)
 *
 * Row weights (bd_trainer_step_weighted / bd_trainer_loss_weighted; Keras's sample_weight with sum_over_batch_size: the sums
 * are divided by B, not by the sum of the weights).  Row r counts w_r times, w_r >= 0 a float in batch order:
 *   categorical   loss = (1/B) sum_r w_r loss_r,             dz_r  = w_r (softmax(z_r) - onehot_r) / B
 *   binary        loss = (1/(B C)) sum_r w_r sum_c loss_rc,  dz_rc = w_r (sigmoid(z_rc) - t_rc) / (B C)
 * in this float32 arithmetic: scale_r = inv * w_r (one product; inv = 1/B or 1/(B C)), the delta is (...) * scale_r, and the
 * row's loss is stored as w_r * loss_r (one product).  Class weights are row weights the caller builds: w_r = class_weight
 * [label_r].  Without weights (NULL) the plain kernels run, instruction for instruction; weights of 1.0f give their bits.
 *
 * Weight decay (bd_trainer_set_weight_decay) is decoupled, as AdamW's: decay = lr * weight_decay, one float32 product on the
 * host per step; an element p of a layer's kernel - never of its bias - becomes p - decay * p (a product, then a difference)
 * and the optimizer's update of the step is subtracted from that.  It is not a term of the loss: neither the loss nor the
 * gradients read back change.  0 (the default) is no decay at all: the branch is not taken.
 *
 * Order within a step: forward, row losses and deltas (weighted), backward, then per element the sum of the slices' partials,
 * the decay, the SGD or Adam update.  The learning rate of a step is the one set when it is enqueued
 * (bd_trainer_set_learning_rate: a schedule is the caller's loop).
 *
 * Snapshot (bd_trainer_snapshot / bd_trainer_restore): a device-to-device copy of every layer's parameters into a second
 * buffer of the trainer's and back, enqueued like a step.  Adam's slots and the step count are not part of it: it exists to
 * hand back the best weights seen, not to resume.
 *
 * Arithmetic: exact float32 on v_mfma_f32_32x32x2_f32 with f32 accumulate, the forward pass in headmlp.hip's operand map
 * and k order (a trained head gives the engine the logits the trainer saw).  Hidden derivatives come from the stored
 * activations.  Three products per layer: Y = act(A W + b), dA = (dY * act') W^T, dW = A^T (dY * act'), db its column sum.
 *
 * Determinism: nothing is added atomically.  The batch is cut into slices of BD_TRAIN_SLICE_ROWS rows - a constant, not a
 * function of the grid, the device or B; each slice's partial dW / db goes to workspace and a second pass adds the partials
 * in ascending slice order, so the same inputs give the same bits on every run and on any number of compute units.  A
 * one-layer stack of at most BD_TRAIN_FUSED_MAX_WIDTH outputs runs forward, loss, delta and the dW partial of a slice in one
 * kernel (bd_trainer_set_fusion(t, 0) takes the layer-by-layer route instead: same bits).
 *
 * Conventions are those of buzzdetect_hip.h: 0 or a negative BD_E* code, bd_last_error(), work enqueued on the caller's
 * stream with no hidden synchronisation (bd_trainer_create / _destroy and the calls marked synchronous excepted), X, rows,
 * targets and loss_dev owned by the caller, 16-byte aligned X with ldx a multiple of 4.  The trainer owns the parameters,
 * the optimizer's slots and its workspace.  A handle is not thread-safe.
 *
 * Out of scope: dropout, penalties added to the loss (L1 / L2), a per-class pos_weight for the binary loss, focal loss and
 * label smoothing, resuming from a snapshot, more than one device, and anything below the embedding.
 */
#ifndef BUZZDETECT_TRAIN_H
#define BUZZDETECT_TRAIN_H

#include <stdint.h>

#include "buzzdetect_head.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BD_TRAIN_ABI_VERSION 2
#define BD_TRAIN_SLICE_ROWS 256          /* rows of the batch per dW partial (fixed: part of the results' bits) */
#define BD_TRAIN_FUSED_MAX_WIDTH 64      /* widest one-layer stack that takes the fused kernel */
#define BD_TRAIN_MAX_BATCH 65536

/* loss */
#define BD_TRAIN_CATEGORICAL 0
#define BD_TRAIN_BINARY 1
/* bd_train_optimizer.kind */
#define BD_TRAIN_SGD 0
#define BD_TRAIN_ADAM 1

typedef struct bd_train_optimizer {
    int32_t kind;                    /* BD_TRAIN_SGD: w -= lr g.  BD_TRAIN_ADAM (Keras): m = b1 m + (1 - b1) g,
                                        v = b2 v + (1 - b2) g^2, w -= lr sqrt(1 - b2^t) / (1 - b1^t) m / (sqrt(v) + eps) */
    float learning_rate;
    float beta_1, beta_2, epsilon;   /* Adam only */
    int32_t reserved;                /* 0 */
} bd_train_optimizer;

typedef struct bd_trainer_s* bd_trainer;

BD_API int bd_train_abi_version(void);

/* Copies the layers' initial values to the device and allocates slots, activations and workspace for batches of up to
 * max_batch (1 .. BD_TRAIN_MAX_BATCH) rows.  Synchronous. */
BD_API int bd_trainer_create(int device, const bd_head_layer* layers, int32_t n_layers, int32_t loss,
                             const bd_train_optimizer* optimizer, int32_t max_batch, bd_trainer* trainer);
BD_API int bd_trainer_destroy(bd_trainer t);

/* One optimisation step on B <= max_batch rows: forward, loss and output delta, backward, update.
 *   X        device [N][ldx] float32, ldx >= BD_EMBEDDING_SIZE
 *   rows     device int32[B], row numbers into X (the caller vouches for 0 <= rows[i] < N), or NULL for rows 0 .. B-1; the
 *            rows are gathered inside the first layer's operand loads
 *   targets  device int32[B] (categorical, 0 .. C-1) or float[B][C] (binary), in batch order
 * The batch's loss is also added to the trainer's running sum (bd_trainer_mean_loss). */
BD_API int bd_trainer_step(bd_trainer t, const float* X, int64_t ldx, const int32_t* rows, const void* targets, int32_t B,
                           void* stream);

/* Forward pass and loss only: writes the batch's mean loss to loss_dev[0] (device float). */
BD_API int bd_trainer_loss(bd_trainer t, const float* X, int64_t ldx, const int32_t* rows, const void* targets, int32_t B,
                           float* loss_dev, void* stream);

/* The same two calls with a weight per row: row_weights is device float[B] in batch order, like targets (finite, >= 0: the
 * caller vouches for it); NULL is bd_trainer_step / bd_trainer_loss.  bd_trainer_mean_loss then reports the weighted loss
 * per row (the running sum still counts B rows a step). */
BD_API int bd_trainer_step_weighted(bd_trainer t, const float* X, int64_t ldx, const int32_t* rows, const void* targets,
                                    const float* row_weights, int32_t B, void* stream);
BD_API int bd_trainer_loss_weighted(bd_trainer t, const float* X, int64_t ldx, const int32_t* rows, const void* targets,
                                    const float* row_weights, int32_t B, float* loss_dev, void* stream);

/* Host-side settings of the steps enqueued from now on; nothing is enqueued.  weight_decay >= 0 and finite (0: none; it
 * applies to kernels only), learning_rate > 0 and finite (it replaces bd_train_optimizer.learning_rate). */
BD_API int bd_trainer_set_weight_decay(bd_trainer t, float weight_decay);
BD_API int bd_trainer_set_learning_rate(bd_trainer t, float learning_rate);

/* Copy every layer's parameters to the trainer's snapshot buffer / back from it, on `stream`, without synchronisation.
 * bd_trainer_restore before any bd_trainer_snapshot is BD_EINVAL. */
BD_API int bd_trainer_snapshot(bd_trainer t, void* stream);
BD_API int bd_trainer_restore(bd_trainer t, void* stream);

/* Synchronous reads (they wait for the stream of the trainer's last call).  Gradients are those of the last step;
 * kernel_host / dW_host [n_in][n_out], bias_host / db_host [n_out]; either may be NULL. */
BD_API int bd_trainer_gradients(bd_trainer t, int32_t layer, float* dW_host, float* db_host);
BD_API int bd_trainer_read(bd_trainer t, int32_t layer, float* kernel_host, float* bias_host);
/* The logits [B][n_out of the last layer] of the last bd_trainer_step / bd_trainer_loss (of a step: before its update). */
BD_API int bd_trainer_logits(bd_trainer t, int32_t B, float* logits_host);
/* Mean loss per row over the steps since the last reset (each step's batch mean weighted by its B), then reset if asked. */
BD_API int bd_trainer_mean_loss(bd_trainer t, int32_t reset, float* mean_host);

/* Test switches.  bd_trainer_set_fusion: 0 = layer by layer even where the fused kernel applies.  The workspace calls fill
 * the dW-partial workspace with a 32-bit pattern and read it back (floats = bd_trainer_workspace_floats). */
BD_API int bd_trainer_set_fusion(bd_trainer t, int32_t fused);
BD_API int64_t bd_trainer_workspace_floats(bd_trainer t);
BD_API int bd_trainer_workspace_fill(bd_trainer t, uint32_t pattern);
BD_API int bd_trainer_workspace_read(bd_trainer t, float* host, int64_t floats);

#ifdef __cplusplus
}
#endif

#endif /* BUZZDETECT_TRAIN_H */
