/*
 * buzzdetect_stackbank.h — C ABI of the bank of Dense stacks in libbuzzdetect_hip.so (gfx950).
 *
 * A bd_bank (buzzdetect_bank.h) steps M one-layer heads of at most 64 outputs together.  A bd_stackbank does the same for
 * whole stacks - the heads bd_trainer_create takes: 1 .. BD_HEAD_MAX_LAYERS Dense layers, widths 1 .. BD_HEAD_MAX_WIDTH, the
 * first reading BD_EMBEDDING_SIZE - so that a head with a hidden layer, or a one-layer head of more than 64 classes, can be
 * cross-validated and swept in one pass as well.
 *
 *   shared by the members    the shape (number of layers, widths, hidden activations), the loss (BD_TRAIN_CATEGORICAL /
 *                            BD_TRAIN_BINARY), the optimizer's kind, betas and epsilon, and per call X, rows, targets and B
 *   a member's own           parameters, gradients, Adam's slots and step count of every layer, its snapshot of every layer,
 *                            learning rate, weight decay, frozen flag, row weights and running loss sum
 *
 * The contract is the bank's, for stacks: after any sequence of calls, member m's parameters, Adam slots, last gradients of
 * every layer, logits, batch loss and running mean loss equal, bit for bit, those of a bd_trainer created from member m's
 * initial layers that received the same calls - bd_trainer_step_weighted with row m of the weights, or bd_trainer_step where
 * the bank got NULL.  It holds by construction: the bank's kernels and launches (csrc/headtrain_stack.h) are the ones the
 * lone trainer's layer-by-layer route runs with one member, and call csrc/headtrain_device.h for every product, row loss,
 * partial sum and update.
 * Slices are the same BD_TRAIN_SLICE_ROWS rows and a member's partials are added in ascending slice order; nothing is added
 * atomically; nothing depends on the grid, the number of compute units, M, or a member's place in the bank.
 *
 * Layout: one pool, member m's block at m x a fixed stride (a multiple of 64 floats, so the 16-byte row loads of the shared
 * tiles stay aligned): per layer [W | b], gradients, Adam's two slots and the snapshot, then per layer the activations and
 * deltas [max_batch][round_up(n, 32)], then the row losses.  The dW / db partials live in a workspace
 * [member][slice][k n + n] of the layer at work.  Every member offset is formed in 64 bits.
 *
 * Frozen members (bd_stackbank_set_frozen): a step leaves a frozen member's parameters, slots, step count, last gradients
 * and running loss sum as they are - the member is a trainer that did not get the call.  Its batch loss and logits are still
 * computed: bd_stackbank_loss and bd_stackbank_forward report every member.
 *
 * Conventions are those of buzzdetect_bank.h: 0 or a negative BD_E* code, bd_last_error() names the failing call, work is
 * enqueued on the caller's stream with no hidden synchronisation (bd_stackbank_create / _destroy and the calls marked
 * synchronous excepted), NULL handles or pointers give BD_EINVAL before anything is enqueued; X is 16-byte aligned with
 * ldx >= 1024 a multiple of 4.  The learning rate, decay and frozen flag of a step are those set when it is enqueued: they
 * travel by value in its launches.  A handle is not thread-safe.
 *
 * Out of scope: members that differ in shape, loss or optimizer kind; dropout; more than one device; splitting a bank that
 * exceeds BD_STACKBANK_MAX_WORKSPACE_BYTES into several; and everything buzzdetect_train.h lists as out of scope.
 */
#ifndef BUZZDETECT_STACKBANK_H
#define BUZZDETECT_STACKBANK_H

#include <stdint.h>

#include "buzzdetect_bank.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BD_STACKBANK_ABI_VERSION 1
#define BD_STACKBANK_MAX_WORKSPACE_BYTES 8589934592LL   /* bd_stackbank_create refuses shapes whose device memory exceeds this */

typedef struct bd_stackbank_s* bd_stackbank;

BD_API int bd_stackbank_abi_version(void);

/* layers[m n_layers + l] holds layer l of member m's initial values (member-major).  Every member has member 0's shape:
 * n_layers in 1 .. BD_HEAD_MAX_LAYERS, layer 0 with n_in = BD_EMBEDDING_SIZE and every later layer with the n_out before it,
 * n_out in 1 .. BD_HEAD_MAX_WIDTH, hidden activations linear / relu / sigmoid / tanh (the last layer's is not used: the loss
 * reads raw logits), bias NULL for zeros.  Every member starts with optimizer->learning_rate, no decay, not frozen.
 * max_batch in 1 .. BD_TRAIN_MAX_BATCH, n_members in 1 .. BD_BANK_MAX_MEMBERS.  Shapes and the device memory they need
 * (BD_EWORKSPACE past BD_STACKBANK_MAX_WORKSPACE_BYTES) are refused before a device is looked for.  Synchronous. */
BD_API int bd_stackbank_create(int device, const bd_head_layer* layers, int32_t n_members, int32_t n_layers, int32_t loss,
                               const bd_train_optimizer* optimizer, int32_t max_batch, bd_stackbank* bank);
BD_API int bd_stackbank_destroy(bd_stackbank b);

/* One optimisation step of every member that is not frozen; arguments as bd_bank_step defines them: row_weights is device
 * float[M][ldw] (ldw >= B), or NULL: every member runs the unweighted pass. */
BD_API int bd_stackbank_step(bd_stackbank b, const float* X, int64_t ldx, const int32_t* rows, const void* targets,
                             const float* row_weights, int64_t ldw, int32_t B, void* stream);

/* Forward pass and loss only: member m's (weighted) mean loss of the batch goes to loss_dev[m] (device float[M]). */
BD_API int bd_stackbank_loss(bd_stackbank b, const float* X, int64_t ldx, const int32_t* rows, const void* targets,
                             const float* row_weights, int64_t ldw, int32_t B, float* loss_dev, void* stream);

/* Logits only: logits_dev is device float [B][ldl], member m's C logits of batch row r at logits_dev[r ldl + m C ..]
 * (ldl >= M C, C the last layer's width).  No parameter, slot, gradient or loss sum of the bank changes. */
BD_API int bd_stackbank_forward(bd_stackbank b, const float* X, int64_t ldx, const int32_t* rows, int32_t B, float* logits_dev,
                                int64_t ldl, void* stream);

/* Host-side settings of a member for the steps enqueued from now on; nothing is enqueued.  learning_rate > 0 and finite,
 * weight_decay >= 0 and finite (decoupled, kernels only: buzzdetect_train.h), frozen 0 or 1. */
BD_API int bd_stackbank_set_learning_rate(bd_stackbank b, int32_t member, float learning_rate);
BD_API int bd_stackbank_set_weight_decay(bd_stackbank b, int32_t member, float weight_decay);
BD_API int bd_stackbank_set_frozen(bd_stackbank b, int32_t member, int32_t frozen);

/* Copy every layer of a member's parameters to its snapshot / back from it, on `stream`, without synchronisation (Adam's
 * slots and the step count are not part of it).  bd_stackbank_restore of a member before a bd_stackbank_snapshot of that
 * member is BD_EINVAL. */
BD_API int bd_stackbank_snapshot(bd_stackbank b, int32_t member, void* stream);
BD_API int bd_stackbank_restore(bd_stackbank b, int32_t member, void* stream);

/* Synchronous reads (they wait for the stream of the bank's last call).  kernel_host / dW_host [n_in][n_out] of the layer,
 * bias_host / db_host [n_out]; either may be NULL.  Gradients are those of the member's last step.
 * bd_stackbank_mean_loss: every member's mean loss per row over its steps since the last reset into mean_host[M], then reset
 * if asked. */
BD_API int bd_stackbank_read(bd_stackbank b, int32_t member, int32_t layer, float* kernel_host, float* bias_host);
BD_API int bd_stackbank_gradients(bd_stackbank b, int32_t member, int32_t layer, float* dW_host, float* db_host);
BD_API int bd_stackbank_mean_loss(bd_stackbank b, int32_t reset, float* mean_host);

/* Test switches: fill the dW-partial workspace with a 32-bit pattern and read it back (floats =
 * bd_stackbank_workspace_floats: [member][slices of max_batch x the largest layer's k n + n, rounded up to 64]). */
BD_API int64_t bd_stackbank_workspace_floats(bd_stackbank b);
BD_API int bd_stackbank_workspace_fill(bd_stackbank b, uint32_t pattern);
BD_API int bd_stackbank_workspace_read(bd_stackbank b, float* host, int64_t floats);

#ifdef __cplusplus
}
#endif

#endif /* BUZZDETECT_STACKBANK_H */
