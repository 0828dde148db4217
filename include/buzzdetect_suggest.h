/*
 * buzzdetect_suggest.h — C ABI of "what to annotate next" in libbuzzdetect_hip.so (gfx950): an acquisition score per window
 * from the logits of a set of heads where they lie, and the greedy choice of a diverse batch from a pool of candidates, for
 * buzzdetect_amd/suggest.py.
 *
 *   bd_suggest_acquire   out[s][w], s = entropy, margin, BALD, of window w        (bd_suggest_acquire_host: agrees to rounding)
 *   bd_suggest_pick      k of n candidates, each the best gain * distance so far  (bd_suggest_pick_host: the same bits)
 *
 * Acquisition.  wide is [W][ld_wide] float32: the columns a set of heads WITHOUT an ensemble writes (buzzdetect_headset.h).
 * Member m's C = width logits of a window start at column member_first[m]; member_first is a HOST array on both sides (the
 * device entry point hands it to the kernel by value).  The members' last layers are linear; link says how logits become
 * probabilities.  Everything is float32.
 *   target = -1   the whole distribution (BD_LINK_SOFTMAX, C >= 2): with mx = max_c z[c], e[c] = expf(z[c] - mx),
 *                 s = sum_c e[c]:  p_m[c] = e[c] / s  and  log p_m[c] = (z[c] - mx) - logf(s).  L = logf(C).
 *   target = t    the question "class t or not", a distribution (q, r) per member.  L = logf(2).
 *                 BD_LINK_SOFTMAX: q = e[t] / s and r = (sum_{c != t} e[c]) / s - the other classes are summed, 1 - q is never
 *                 formed by subtraction; log q = (z[t] - mx) - logf(s), and log1pf(-r) where r < 0.5; log r =
 *                 logf(sum_{c != t} e[c]) - logf(s), and log1pf(-q) where q < 0.5.
 *                 BD_LINK_SIGMOID: log q = logsigmoid(z[t]), log r = logsigmoid(-z[t]) (logsigmoid(x) = min(x, 0) -
 *                 log1pf(expf(-|x|))), q = expf(log q), r = expf(log r).  Only column t is read.
 * The committee mean pbar[c] = (p_0[c] + p_1[c] + ... + p_{M-1}[c]) * (1.0f / M): members added in ascending order from 0.0f, one
 * product at the end.  x log x is 0 at x = 0.  H(pbar) = -sum_c pbar[c] logf(pbar[c]); the members' mean entropy is
 * Hm = -(sum_c (sum_m p_m[c] log p_m[c])) * (1.0f / M), the inner sum over members in ascending order.
 *   BD_SUGGEST_ENTROPY (0)   H(pbar) / L
 *   BD_SUGGEST_MARGIN  (1)   1 - (largest - second largest of pbar); with a target 1 - |2 qbar - 1|
 *   BD_SUGGEST_BALD    (2)   max(H(pbar) - Hm, 0) / L: how much the members disagree.  For M = 1 this is identically zero and the
 *                            constant 0.0f is stored: the difference is not computed.
 * Every value is then brought into [0, 1] (below 0 -> 0, above 1 -> 1).  Score s of window w is stored at
 * out[s * out_stride + w]; all three rows are always written, so bd_search_update(out + s * out_stride, W, 1, 1, out_stride, ...)
 * ranks any of them.  Finite logits of any size (|z| = 1e4, say) give finite outputs.  A NaN among the logits that are read
 * makes the window's three outputs NaN (for M = 1 too), which the selector of buzzdetect_search.h ranks last.
 *
 * One wave per window: lane c < C holds class c, the members are walked in a loop, and sums and maxima over a row are
 * butterflies over the wave (v op= v[lane ^ m], m = 32, 16, .. 1).  bd_suggest_acquire_host adds a row's terms serially in
 * ascending c and calls the host's expf / logf, so the two sides AGREE TO ROUNDING, NOT BY BITS - as the soft vote of
 * buzzdetect_ensemble.h.  A window's three outputs depend on that window's logits alone: the device gives the same bits wherever the
 * window sits in a call and whatever W is.  No atomics, one writer per output element, 64-bit element offsets.
 *
 * Limits of acquire (refused on the host with the argument named, nothing launched): 1 <= n_members <= BD_SUGGEST_MAX_MEMBERS,
 * 1 <= width <= BD_SUGGEST_MAX_WIDTH, width >= 2 unless link is BD_LINK_SIGMOID, link BD_LINK_SOFTMAX or BD_LINK_SIGMOID,
 * -1 <= target < width, a target with BD_LINK_SIGMOID, 0 <= member_first[m] and member_first[m] + width <= ld_wide for every m,
 * 0 <= W <= BD_SEARCH_MAX_WINDOWS (W = 0 launches and writes nothing), out_stride >= W, non-null 4-byte aligned pointers.
 *
 * Pick.  n candidates with gains gain[n], a similarity matrix with sim[j * ld + i] = similarity of candidate i to candidate j
 * (what bd_search_scores(P, n, pack(unit rows of P), n, BD_SEARCH_COSINE, .., row_stride = 1, col_stride = ld) stores, so a
 * step reads ONE contiguous row), and optionally d0[n], the distance of every candidate to what is labelled already (null:
 * 1.0f everywhere).  State: d[i] = d0[i], nothing chosen.  Step t = 0 .. k - 1:
 *   g[i] = gain[i] * d[i] for every candidate not yet chosen                    (one rounded float32 product)
 *   i* = the candidate with the largest key (g[i], i) of buzzdetect_search.h: the higher g, among equal g the lower index; a NaN
 *        counts as -INFINITY and -0.0f as +0.0f
 *   picked[t] = i*, value[t] = g[i*] (the product as it is, not its key's score), dist[t] = d[i*]
 *   d[i] = fminf(d[i], fmaxf(1.0f - sim[i* * ld + i], 0.0f)) for every i        (each operation rounded once)
 * The first pick is the candidate with the highest gain; every later one the candidate whose gain, discounted by its closeness
 * to anything already picked, is highest.  ONE workgroup of BD_SUGGEST_MAX_POOL threads runs the k steps in one launch: thread
 * i owns candidate i (d, gain and the chosen flag in registers), a step is a butterfly maximum of 64-bit keys per wave, sixteen
 * wave maxima in LDS (two slots that alternate, so a step costs one barrier) and one coalesced read of row i* of sim.  There is
 * no grid-wide synchronisation and no atomic; maxima are exact and every other step is one correctly rounded operation, so
 * bd_suggest_pick_host - the plain sequential loop over the same expressions - gives the same picked, value and dist IN EVERY BIT.
 *
 * Limits of pick (refused alike): 1 <= n <= BD_SUGGEST_MAX_POOL, 1 <= k <= n, ld >= n, non-null 4-byte aligned sim, gain,
 * picked, value and dist (d0 may be null).
 *
 * Conventions are those of buzzdetect_hip.h: 0 on success, a negative BD_E* code on failure, bd_last_error() for the text; the
 * caller owns all device memory; `stream` is a hipStream_t.
 */
#ifndef BUZZDETECT_SUGGEST_H
#define BUZZDETECT_SUGGEST_H

#include <stdint.h>

#include "buzzdetect_hip.h"
#include "buzzdetect_ensemble.h"
#include "buzzdetect_search.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BD_SUGGEST_ABI_VERSION 1
#define BD_SUGGEST_MAX_MEMBERS 64               /* BD_HEADSET_MAX_MEMBERS */
#define BD_SUGGEST_MAX_WIDTH 64                 /* classes per member: a lane each */
#define BD_SUGGEST_MAX_POOL 1024                /* BD_SEARCH_MAX_K: the most the selector keeps */
#define BD_SUGGEST_STRATEGIES 3
#define BD_SUGGEST_ENTROPY 0
#define BD_SUGGEST_MARGIN 1
#define BD_SUGGEST_BALD 2

BD_API int bd_suggest_abi_version(void);

/* member_first [n_members] in HOST memory; out [BD_SUGGEST_STRATEGIES rows of out_stride floats]. */
BD_API int bd_suggest_acquire(const float* wide_dev, int64_t windows, int32_t ld_wide, const int32_t* member_first,
                              int32_t n_members, int32_t width, int32_t link, int32_t target, float* out_dev, int64_t out_stride,
                              void* stream);
BD_API int bd_suggest_acquire_host(const float* wide, int64_t windows, int32_t ld_wide, const int32_t* member_first,
                                   int32_t n_members, int32_t width, int32_t link, int32_t target, float* out, int64_t out_stride);

/* sim [n rows of ld floats]; gain, d0 [n] (d0 may be null); picked, value, dist [k]. */
BD_API int bd_suggest_pick(const float* sim_dev, int64_t ld, const float* gain_dev, const float* d0_dev, int32_t n, int32_t k,
                           int32_t* picked_dev, float* value_dev, float* dist_dev, void* stream);
BD_API int bd_suggest_pick_host(const float* sim, int64_t ld, const float* gain, const float* d0, int32_t n, int32_t k,
                                int32_t* picked, float* value, float* dist);

#ifdef __cplusplus
}
#endif

#endif /* BUZZDETECT_SUGGEST_H */
