/*
 * buzzdetect_head.h — C ABI of the dense-stack classifier head in libbuzzdetect_hip.so (gfx950).
 *
 * The reference loads whatever classifier lies in models/<modelname> (src/inference/models.py:40-79); a lab that
 * trains its own on YAMNet embeddings gets a stack of Dense layers.  bd_create's own head is one
 * Dense(1024 -> n <= BD_MAX_CLASSES) fused behind the average pool.  This header attaches a stack instead:
 *
 *   y_0 = the 1024-wide embedding,  y_k = act_k(y_{k-1} W_k + b_k),  k = 1 .. n_layers <= BD_HEAD_MAX_LAYERS
 *
 * every width 1 .. BD_HEAD_MAX_WIDTH, act one of BD_HEAD_LINEAR / RELU / SIGMOID / TANH, BD_HEAD_SOFTMAX on the
 * last layer only.  Every layer is one launch in exact float32 (v_mfma_f32_32x32x2_f32, f32 accumulate) in all three
 * arithmetic modes of the CNN; a softmax is a row pass behind the last one.  A window's outputs depend on its
 * embedding only: k runs in one fixed order, nothing is split over workgroups and nothing is added atomically, so a
 * window gives the same bits alone, inside a full pass and inside a ragged last pass.
 *
 *   bd_head_attach     give an engine created WITHOUT a head (bd_weights.n_classes == 0) a stack
 *   bd_head_outputs    width of the attached stack's last layer (0: none attached)
 *
 * After bd_head_attach the engine's logits are [windows][bd_head_outputs()] wherever buzzdetect_hip.h says
 * [windows][n_classes]; the hidden activations live in the workspace the engine already asks for
 * (bd_workspace_bytes does not change).  Conventions are those of buzzdetect_hip.h.
 */
#ifndef BUZZDETECT_HEAD_H
#define BUZZDETECT_HEAD_H

#include <stdint.h>

#include "buzzdetect_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BD_HEAD_ABI_VERSION 1
#define BD_HEAD_MAX_LAYERS 8
#define BD_HEAD_MAX_WIDTH 2048

/* bd_head_layer.activation */
#define BD_HEAD_LINEAR 0
#define BD_HEAD_RELU 1
#define BD_HEAD_SIGMOID 2
#define BD_HEAD_TANH 3
#define BD_HEAD_SOFTMAX 4            /* last layer only */

typedef struct bd_head_layer {
    const float* kernel;             /* host, [n_in][n_out] row-major, as a Keras Dense keeps it */
    const float* bias;               /* host, [n_out]; NULL = zeros */
    int32_t n_in;                    /* layer 0: BD_EMBEDDING_SIZE; layer k: n_out of layer k - 1 */
    int32_t n_out;                   /* 1 .. BD_HEAD_MAX_WIDTH */
    int32_t activation;              /* BD_HEAD_* */
    int32_t reserved;                /* 0 */
} bd_head_layer;

BD_API int bd_head_abi_version(void);

/* Copies the layers to the device (synchronous; the host arrays may be freed on return).  The engine must have been
 * created without a head and must not have a stack yet; nothing of it may be in flight. */
BD_API int bd_head_attach(bd_handle h, const bd_head_layer* layers, int32_t n_layers);

/* Outputs per window of the attached stack; 0 when the engine has none. */
BD_API int bd_head_outputs(bd_handle h);

#ifdef __cplusplus
}
#endif

#endif /* BUZZDETECT_HEAD_H */
