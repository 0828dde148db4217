/*
 * buzzdetect_ensemble.h — C ABI of ensembles of heads in libbuzzdetect_hip.so (gfx950).
 *
 * A cross-validation leaves K fitted folds, a sweep its members: the standard ensemble.  buzzdetect_headset.h already runs 1 .. 64
 * members behind one embedder pass; this header reduces groups of those members to one output each, on the device, so that an
 * ensemble is a model like any other: one row of logits per window.
 *
 *   bd_ensemble_attach        group the members of an attached set into outputs (each a mean of its members, or one member as it is)
 *   bd_ensemble_count         number of outputs (0: no ensemble attached)
 *   bd_ensemble_outputs       columns per window of the logits: the sum of the outputs' widths
 *   bd_ensemble_columns       the columns of one output
 *   bd_ensemble_combine_host  the same arithmetic in plain C++, callable without a device
 *
 * Logits.  After bd_ensemble_attach the engine's logits are [windows][bd_ensemble_outputs()] wherever buzzdetect_hip.h says
 * [windows][n_classes]: output 0's columns first, then output 1's ..., no padding.  An output's width is its members' common last
 * width.  bd_headset_outputs keeps reporting the wide sum over the members, bd_workspace_bytes does not change.
 *
 * Placement.  The set's kernels write the members' columns into a row of the workspace a set already owns instead of the caller's
 * logits; ONE further launch per pass, whatever the number of members, writes every public column (pass-through columns are
 * copied).  An engine without bd_ensemble_attach runs exactly the launches it ran before.
 *
 * Combine kinds (z[m][c]: member m's column c of one window, m = 0 .. K-1 in the set's order; float32 throughout):
 *   BD_COMBINE_NONE              one member, copied bit for bit.
 *   BD_COMBINE_MEAN              y[c] = (z[0][c] + z[1][c] + ... + z[K-1][c]) * r: one chain of float32 additions in ascending member
 *                                order that starts from member 0's value, then one multiplication by r = 1.0f / K (rounded once, at
 *                                attach time).  No atomics, nothing split over threads: bit-reproducible, and bit-equal between the
 *                                device and bd_ensemble_combine_host.  Any common last activation.
 *   BD_COMBINE_MEAN_PROBABILITY  soft voting, returned in the domain thresholds are taken in; every member's last layer must be linear.
 *       BD_LINK_SOFTMAX          y[c] = log((1/K) sum_m softmax(z[m])[c]), in the log domain: lse[m] = logsumexp_c z[m][c], a[m][c] =
 *                                z[m][c] - lse[m], y[c] = max_m a[m][c] + log(sum_m exp(a[m][c] - max_m a[m][c])) - log K.
 *       BD_LINK_SIGMOID          y[c] = logit((1/K) sum_m sigmoid(z[m][c])) = logsumexp_m logsigmoid(z[m][c]) - logsumexp_m
 *                                logsigmoid(-z[m][c]) (the 1/K cancels).
 *                                Both are finite for every finite input.  The device reduces a row over the lanes of a wave, the host
 *                                serially: the two agree to rounding, not by bits.
 *
 * Refusals (each BD_EINVAL, the message naming the output or member; the engine stays as it was): no set attached; a second
 * attach; outputs that do not tile the set's members in order without gap or overlap; n_members < 1; members of one output with
 * different last widths or different last activations; MEAN_PROBABILITY over a last layer that is not linear, or without a link;
 * an unknown combine or link; NONE with more than one member.  Conventions are those of buzzdetect_hip.h.
 */
#ifndef BUZZDETECT_ENSEMBLE_H
#define BUZZDETECT_ENSEMBLE_H

#include <stdint.h>

#include "buzzdetect_headset.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BD_ENSEMBLE_ABI_VERSION 1

#define BD_COMBINE_NONE 0
#define BD_COMBINE_MEAN 1
#define BD_COMBINE_MEAN_PROBABILITY 2

#define BD_LINK_NONE 0
#define BD_LINK_SOFTMAX 1
#define BD_LINK_SIGMOID 2

typedef struct bd_ensemble_output {
    int32_t first_member;            /* index into the set's members */
    int32_t n_members;               /* 1 .. BD_HEADSET_MAX_MEMBERS */
    int32_t combine;                 /* BD_COMBINE_* */
    int32_t link;                    /* BD_LINK_*; BD_LINK_NONE unless combine is BD_COMBINE_MEAN_PROBABILITY */
} bd_ensemble_output;

BD_API int bd_ensemble_abi_version(void);

/* The engine must carry a set (bd_headset_attach) and no ensemble yet, and nothing of it may be in flight.  Synchronous; the
 * array may be freed on return. */
BD_API int bd_ensemble_attach(bd_handle h, const bd_ensemble_output* outputs, int32_t n_outputs);

/* Outputs of the attached ensemble; 0 when the engine has none. */
BD_API int bd_ensemble_count(bd_handle h);

/* Columns per window of the logits with the ensemble attached (the sum of the outputs' widths); 0 when the engine has none. */
BD_API int bd_ensemble_outputs(bd_handle h);

/* Output `output`'s columns of the logits: [*first, *first + *count). */
BD_API int bd_ensemble_columns(bd_handle h, int32_t output, int32_t* first, int32_t* count);

/* The combine pass on the host.  wide = [windows][ld_wide]: the members' columns as a set without an ensemble gives them;
 * member_first has one entry per member of the set PLUS ONE: member m's columns of `wide` are [member_first[m],
 * member_first[m + 1]).  out = [windows][ld_out]: output o's columns follow output o - 1's from column 0; columns at and beyond
 * the sum of the outputs' widths are not touched.  The outputs must tile the members and the members of one output must share a
 * width, as for bd_ensemble_attach (the activations are the caller's business here).  Needs no device. */
BD_API int bd_ensemble_combine_host(const float* wide, int64_t windows, int32_t ld_wide, const bd_ensemble_output* outputs,
                                    int32_t n_outputs, const int32_t* member_first, float* out, int32_t ld_out);

#ifdef __cplusplus
}
#endif

#endif /* BUZZDETECT_ENSEMBLE_H */
