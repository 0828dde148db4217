/*
 * buzzdetect_bank.h — C ABI of the bank of one-layer classifier heads in libbuzzdetect_hip.so (gfx950).
 *
 * A bd_trainer (buzzdetect_train.h) fits one head.  Cross-validation and a sweep over rates, decays and class weights fit many
 * heads that differ only in what weighs, scales and stops them, on the same rows in the same order.  A bank holds M such
 * members - each one Dense layer BD_EMBEDDING_SIZE -> C, 1 <= C <= BD_TRAIN_FUSED_MAX_WIDTH - and steps them together: the
 * batch's rows of X are gathered once per step for the whole bank, members sit side by side in the 64 columns a workgroup of
 * the one-head trainer owns, and the groups of columns run on compute units a single head leaves idle.
 *
 *   shared by the members    C, the loss (BD_TRAIN_CATEGORICAL / BD_TRAIN_BINARY, the definitions of buzzdetect_train.h), the
 *                            optimizer's kind, betas and epsilon, and per call X, rows, targets and B
 *   a member's own           parameters, Adam's slots and step count, learning rate, weight decay, row weights, running loss
 *                            sum, last gradients, snapshot, and the frozen flag
 *
 * The contract: after any sequence of calls, member m's parameters, Adam slots, last gradients, logits, batch loss and running
 * mean loss equal, bit for bit, those of a bd_trainer created from member m's initial values that received the same calls -
 * bd_trainer_step_weighted with row m of the weights, or bd_trainer_step where the bank got NULL.  Nothing is added
 * atomically; nothing depends on the grid, the number of compute units, M, or a member's position in the bank.  It holds
 * because both run the same device routines (csrc/headtrain_device.h): an output element is one chain of fused multiply-adds
 * in ascending k whatever its neighbours in the tile hold, the batch is cut into the same BD_TRAIN_SLICE_ROWS slices, and a
 * member's partials are added in the same ascending order.  A k-fold split is row weights: a row of weight 0 contributes
 * exactly nothing.
 *
 * Layout: members are packed into groups of BD_BANK_GROUP_COLUMNS columns, floor(64 / C) whole members per group, none
 * straddling two groups; a group's parameters are one row-major [1025][members in it x C] block (the bias is row 1024).  The
 * step runs on a grid of (slices, groups).  Columns past a group's last member do not exist: they are never loaded and
 * never stored.
 *
 * Frozen members (bd_bank_set_frozen): a step leaves a frozen member's parameters, slots, step count, last gradients and
 * running loss sum as they are - the member is a trainer that did not get the call.  Its batch loss and logits are still
 * computed: bd_bank_loss and bd_bank_forward report every member.
 *
 * Conventions are those of buzzdetect_train.h: 0 or a negative BD_E* code, bd_last_error() names the failing call, work is
 * enqueued on the caller's stream with no hidden synchronisation (bd_bank_create / _destroy and the calls marked synchronous
 * excepted), NULL handles or pointers give BD_EINVAL before anything is enqueued; X is 16-byte aligned with ldx >= 1024 a
 * multiple of 4.  The learning rate and decay of a step are those set when it is enqueued: they travel by value in its
 * launches.  A handle is not thread-safe.
 *
 * Out of scope: hidden layers and more than BD_TRAIN_FUSED_MAX_WIDTH outputs in this bank (buzzdetect_stackbank.h holds whole
 * stacks, with the same contract); members that differ in C, loss, optimizer kind or batch order; more than one device; and
 * everything buzzdetect_train.h lists as out of scope.
 */
#ifndef BUZZDETECT_BANK_H
#define BUZZDETECT_BANK_H

#include <stdint.h>

#include "buzzdetect_train.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BD_BANK_ABI_VERSION 1
#define BD_BANK_GROUP_COLUMNS 64         /* columns of a group: BD_TRAIN_FUSED_MAX_WIDTH, what one workgroup of a step owns */
#define BD_BANK_MAX_MEMBERS 4096
#define BD_BANK_MAX_WORKSPACE_BYTES 2147483648LL   /* bd_bank_create refuses M, C and max_batch whose device memory exceeds this */

typedef struct bd_bank_s* bd_bank;

BD_API int bd_bank_abi_version(void);

/* layers[m] holds member m's initial values: n_in = BD_EMBEDDING_SIZE, the same n_out = C for every member (1 ..
 * BD_TRAIN_FUSED_MAX_WIDTH), bias NULL for zeros, activation not used (the loss reads raw logits).  Every member starts with
 * optimizer->learning_rate, no decay, not frozen.  max_batch in 1 .. BD_TRAIN_MAX_BATCH, M in 1 .. BD_BANK_MAX_MEMBERS.
 * Synchronous. */
BD_API int bd_bank_create(int device, const bd_head_layer* layers, int32_t n_members, int32_t loss,
                          const bd_train_optimizer* optimizer, int32_t max_batch, bd_bank* bank);
BD_API int bd_bank_destroy(bd_bank b);

/* One optimisation step of every member that is not frozen.  X, ldx, rows, targets and B as bd_trainer_step defines them,
 * shared by the members.  row_weights: device float[M][ldw], member m's weights of the batch's rows at row_weights + m ldw in
 * batch order (ldw >= B; finite, >= 0: the caller vouches for it), or NULL: every member runs the unweighted pass. */
BD_API int bd_bank_step(bd_bank b, const float* X, int64_t ldx, const int32_t* rows, const void* targets,
                        const float* row_weights, int64_t ldw, int32_t B, void* stream);

/* Forward pass and loss only: member m's (weighted) mean loss of the batch goes to loss_dev[m] (device float[M]). */
BD_API int bd_bank_loss(bd_bank b, const float* X, int64_t ldx, const int32_t* rows, const void* targets,
                        const float* row_weights, int64_t ldw, int32_t B, float* loss_dev, void* stream);

/* Logits only: logits_dev is device float [B][ldl], member m's C logits of batch row r at logits_dev[r ldl + m C ..]
 * (ldl >= M C).  Nothing else of the bank changes. */
BD_API int bd_bank_forward(bd_bank b, const float* X, int64_t ldx, const int32_t* rows, int32_t B, float* logits_dev,
                           int64_t ldl, void* stream);

/* Host-side settings of a member for the steps enqueued from now on; nothing is enqueued.  learning_rate > 0 and finite,
 * weight_decay >= 0 and finite (decoupled, kernels only: buzzdetect_train.h), frozen 0 or 1. */
BD_API int bd_bank_set_learning_rate(bd_bank b, int32_t member, float learning_rate);
BD_API int bd_bank_set_weight_decay(bd_bank b, int32_t member, float weight_decay);
BD_API int bd_bank_set_frozen(bd_bank b, int32_t member, int32_t frozen);

/* Copy a member's parameters to its snapshot / back from it, on `stream`, without synchronisation (Adam's slots and the step
 * count are not part of it).  bd_bank_restore of a member before a bd_bank_snapshot of that member is BD_EINVAL. */
BD_API int bd_bank_snapshot(bd_bank b, int32_t member, void* stream);
BD_API int bd_bank_restore(bd_bank b, int32_t member, void* stream);

/* Synchronous reads (they wait for the stream of the bank's last call).  kernel_host / dW_host [1024][C], bias_host / db_host
 * [C]; either may be NULL.  Gradients are those of the member's last step.  bd_bank_mean_loss: every member's mean loss per
 * row over its steps since the last reset into mean_host[M], then reset if asked. */
BD_API int bd_bank_read(bd_bank b, int32_t member, float* kernel_host, float* bias_host);
BD_API int bd_bank_gradients(bd_bank b, int32_t member, float* dW_host, float* db_host);
BD_API int bd_bank_mean_loss(bd_bank b, int32_t reset, float* mean_host);

/* Test switches: fill the dW-partial workspace with a 32-bit pattern and read it back (floats = bd_bank_workspace_floats). */
BD_API int64_t bd_bank_workspace_floats(bd_bank b);
BD_API int bd_bank_workspace_fill(bd_bank b, uint32_t pattern);
BD_API int bd_bank_workspace_read(bd_bank b, float* host, int64_t floats);

#ifdef __cplusplus
}
#endif

#endif /* BUZZDETECT_BANK_H */
