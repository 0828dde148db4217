/*
 * buzzdetect_headset.h — C ABI of the set of classifier heads in libbuzzdetect_hip.so (gfx950).
 *
 * A lab that has swept or cross-validated heads (buzzdetect_bank.h, buzzdetect_stackbank.h) holds a handful of candidate
 * models over ONE embedder.  An engine carries one head (bd_create's fused Dense(1024 -> n <= BD_MAX_CLASSES), or one stack
 * attached with bd_head_attach), so listening to M candidates costs M embedder passes for about 2 % different arithmetic.
 * This header attaches a SET of heads instead: the embedder runs once per pass and every member's outputs land side by side
 * in the logits.
 *
 *   bd_headset_attach    give an engine created WITHOUT a head (bd_weights.n_classes == 0, no stack) 1 .. 64 members
 *   bd_headset_members   number of members (0: no set attached)
 *   bd_headset_outputs   sum of the members' last widths
 *   bd_headset_columns   the columns of one member
 *
 * Logits.  After bd_headset_attach the engine's logits are [windows][bd_headset_outputs()] wherever buzzdetect_hip.h says
 * [windows][n_classes]: member 0's columns first, then member 1's ..., each member's columns contiguous, no padding.
 * bd_head_outputs keeps returning 0 for such an engine.  bd_workspace_bytes does not change.
 *
 * Bits.  A member's columns are bit for bit those of an engine that carries this member alone - a member of one linear
 * layer of at most BD_MAX_CLASSES outputs as bd_create's fused head, every other member as a stack attached with
 * bd_head_attach - in all three arithmetic modes of the CNN, wherever the window sits in a pass.  The number of launches per
 * pass does not grow with the number of members: one per depth of the deepest stack, one softmax row pass, one for the
 * members of the fused kind.
 *
 * Limits (each refused with BD_EINVAL before anything is uploaded, the message naming the member, layer or depth):
 *   1 .. BD_HEADSET_MAX_MEMBERS members, every one a stack bd_head_attach accepts;
 *   bd_headset_outputs() <= BD_HEAD_MAX_WIDTH;
 *   for every depth d, the widths (each rounded up to 32) of the layers at depth d whose output is not the member's logits -
 *   hidden layers, and a last layer in front of a softmax - sum to at most BD_HEAD_MAX_WIDTH.
 * Conventions are those of buzzdetect_hip.h.
 */
#ifndef BUZZDETECT_HEADSET_H
#define BUZZDETECT_HEADSET_H

#include <stdint.h>

#include "buzzdetect_head.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BD_HEADSET_ABI_VERSION 1
#define BD_HEADSET_MAX_MEMBERS 64

typedef struct bd_headset_member {
    const bd_head_layer* layers;     /* host, as bd_head_attach takes them */
    int32_t n_layers;                /* 1 .. BD_HEAD_MAX_LAYERS */
    int32_t reserved;                /* 0 */
} bd_headset_member;

BD_API int bd_headset_abi_version(void);

/* Copies every member to the device (synchronous; the host arrays may be freed on return).  The engine must have been
 * created without a head, must have neither a stack nor a set yet, and nothing of it may be in flight. */
BD_API int bd_headset_attach(bd_handle h, const bd_headset_member* members, int32_t n_members);

/* Members of the attached set; 0 when the engine has none. */
BD_API int bd_headset_members(bd_handle h);

/* Outputs per window of the attached set (the sum of the members' last widths); 0 when the engine has none. */
BD_API int bd_headset_outputs(bd_handle h);

/* Member `member`'s columns of the logits: [*first, *first + *count). */
BD_API int bd_headset_columns(bd_handle h, int32_t member, int32_t* first, int32_t* count);

#ifdef __cplusplus
}
#endif

#endif /* BUZZDETECT_HEADSET_H */
