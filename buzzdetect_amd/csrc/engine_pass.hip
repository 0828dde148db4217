// The pass: the launch plan of a batch of chunks through the front end, the CNN and the attached head, one launch set per
// arithmetic mode, the calibration passes that set the operand scales of the f16 modes, and the exports that run them.
#include <cmath>
#include <cstring>
#include <string>
#include <utility>

#include "engine_state.h"

#include "../../include/buzzdetect_head.h"
#include "../../include/buzzdetect_rows.h"

namespace {

// Geometry of a batch of chunks processed in one launch set (each chunk keeps its own zero padding).
struct BatchPlan {
    bd::WindowMap map;
    int64_t sample_base[bd::kMaxBatchChunks];
    int64_t frames[bd::kMaxBatchChunks];
    int64_t total_frames, total_windows;
};

int plan_batch(const int64_t* chunk_samples, int32_t n_chunks, int32_t hop, int32_t step, BatchPlan* p) {
    if (!chunk_samples || n_chunks <= 0 || n_chunks > bd::kMaxBatchChunks)
        return fail(BD_EINVAL, "batch must hold 1..64 chunks");
    if (step <= 0) return fail(BD_EINVAL, "patch_step must be > 0");
    p->map.n_chunks = n_chunks;
    int64_t samples = 0, frames = 0, windows = 0;
    for (int c = 0; c < n_chunks; ++c) {
        Geometry g;
        const int rc = geometry(chunk_samples[c], hop, step, &g);
        if (rc < 0) return rc;
        p->sample_base[c] = samples;
        p->frames[c] = g.n_frames;
        p->map.win_start[c] = (int)windows;
        p->map.frame_base[c] = (int)frames;
        samples += chunk_samples[c];
        frames += g.n_frames;
        windows += g.n_windows;
        if (frames > (1LL << 30)) return fail(BD_ERANGE, "batch too large");
    }
    p->map.win_start[n_chunks] = (int)windows;
    p->total_frames = frames;
    p->total_windows = windows;
    return BD_OK;
}

// The workspace of a call, in bytes from its start: the log-mel frames at 0, then the two activation buffers of one group of
// windows (the whole call where it has fewer), then 256 spare bytes.  What bd_workspace_bytes promises and what run_chunks
// carves are this one layout.
struct Workspace {
    int64_t buf_a, buf_b, total;
};

Workspace workspace_layout(const bd_engine* e, int64_t n_frames, int64_t n_windows) {
    const int64_t group = n_windows < e->group_windows ? n_windows : e->group_windows;
    Workspace ws;
    ws.buf_a = align_up(n_frames * BD_MEL_BANDS * 4, 256);
    ws.buf_b = ws.buf_a + align_up(group * kFloatsA * 4, 256);
    ws.total = ws.buf_b + align_up(group * kFloatsB * 4, 256) + 256;
    return ws;
}

int64_t batch_workspace(const bd_engine* e, const BatchPlan& p) {
    return workspace_layout(e, p.total_frames, p.total_windows).total;
}

// One group of windows on its way through the CNN.  Of the two activation buffers, `a` (98 304 floats per window) holds the
// latest conv / 1x1 output and `b` (49 152) the depthwise side; where a fused launch leaves them the other way round, the
// pass swaps them right behind it.
struct Group {
    bd_engine* e;
    const bd::SepLayer* sep;       // this call's view of the layers (sep[l] = layer l + 2)
    hipStream_t stream;
    const float* logmel;           // the batch's log-mel frames; map and step take windows to them
    const bd::WindowMap* map;
    int step;
    int w0, gw;                    // the group's first window and its number of windows
    float* a;
    float* b;
    float* emb;                    // the group's rows of the outputs, or null
    float* logits;
    template <class F>
    bool launch(int slot, F fn) { return ::launch(e, stream, slot, fn); }
};

// conv1 (layer 1): log-mel patches -> a
void conv1(Group& g) {
    g.launch(1, [&] { bd::launch_conv1(g.logmel, g.step, *g.map, g.w0, g.gw, g.e->conv1_w, g.e->conv1_b, g.a, g.stream); });
}

// Layers 1-3 as one kernel: log-mel patches -> the layer-3 output in a, timed in the slot of pointwise 3 (slots 1-4 stay empty)
void stem(Group& g, decltype(&bd::launch_stem4) fn) {
    g.launch(5, [&] { fn(g.logmel, g.step, *g.map, g.w0, g.gw, g.e->conv1_w, g.e->conv1_b, g.sep[0], g.sep[1], g.a, g.stream); });
}

// The 1x1 convolution of layer index l: b -> a
void pointwise(Group& g, int l) {
    const bd::SepLayer& L = g.sep[l];
    g.launch(3 + 2 * l, [&] { bd::launch_pointwise(g.b, g.a, (int64_t)g.gw * L.h_out * L.w_out, L, g.stream); });
}

static_assert(BD_EMBEDDING_SIZE + (bd::kHeadSetRegions + 1) * bd::kHeadSetRow <= kFloatsB,
              "pooled embeddings + the scratch of a set of heads + the members' columns under an ensemble fit either buffer");
static_assert(bd::kEnsembleRegion == bd::kHeadSetRegions && BD_HEAD_MAX_WIDTH <= bd::kHeadSetRow, "the wide row of an ensemble is the region behind the set's own");

// The attached heads (headset.hip: a lone stack or a set) on pooled = [gw][1024]: one launch per depth of the deepest stack, one
// softmax row pass, one launch for the members of the fused kind - whatever the number of members; scratch = kHeadSetRegions *
// kHeadSetRow floats per window, free at this point of the pass.  With an ensemble over the set (ensemble.hip) the members'
// columns go to a fourth region, rows of set.outputs floats packed as the logits would be, and one more launch writes the logits
// from it.  All in slot 28
int attached_head(Group& g, const float* pooled, float* scratch) {
    const bd::HeadSet& set = g.e->set;
    const bd::Ensemble& ens = g.e->ens;
    float* wide = ens.n_outputs ? scratch + bd::kEnsembleRegion * (size_t)g.gw * bd::kHeadSetRow : g.logits;
    for (size_t d = 0; d < set.depths.size(); ++d)
        g.launch(28, [&] { bd::launch_dense_set(set, (int)d, pooled, scratch, wide, g.gw, g.stream); });
    if (set.n_softmax) g.launch(28, [&] { bd::launch_softmax_set(set, scratch, wide, g.gw, g.stream); });
    if (set.n_fused) g.launch(28, [&] { bd::launch_head_set(set, pooled, wide, g.gw, g.stream); });
    if (ens.n_outputs) g.launch(28, [&] { bd::launch_ensemble_combine(ens, wide, set.outputs, g.logits, g.gw, g.stream); });
    return BD_OK;
}

// The dense head on the embeddings a tail kernel pooled (into the embeddings or b: a is free by now)
int head(Group& g, const float* pooled) {
    if (!g.logits) return BD_OK;
    if (g.e->set.dev) return attached_head(g, pooled, g.a);
    g.launch(28, [&] { bd::launch_head(pooled, g.gw, g.e->head_wt, g.e->head_b, g.e->n_classes, g.logits, g.stream); });
    return BD_OK;
}

// One kernel per op from layer index `from` (layer from + 2) on; dw_done: b already holds that layer's depthwise output.  In
// the f16 modes with separable != 0, a stride-1 layer followed by a stride-2 one runs with the next depthwise in its epilogue
// (launch_separable_fused_next_dw: a -> b) unless stop_stage lies between.  stop_stage >= 0: stop once that stage is in place
// (an even stage, a conv / 1x1 output, in a; an odd one, a depthwise output, in b); otherwise end the group with pool + head.
int walk_layers(Group& g, int from, bool dw_done, int stop_stage) {
    const bd::SepLayer* sep = g.sep;
    const bool fuse_next_dw = sep[0].pw_mode != 0 && g.e->separable != 0;
    for (int l = from; l < 13; ++l) {
        if (stop_stage == 2 * l) return BD_OK;
        const bd::SepLayer& L = sep[l];
        if (fuse_next_dw && !dw_done && l + 1 < 13 && (stop_stage < 0 || stop_stage >= 2 * l + 4) &&
            g.launch(3 + 2 * l, [&] { return bd::launch_separable_fused_next_dw(g.a, g.b, g.gw, L, sep[l + 1], g.stream); })) {
            dw_done = true;
            continue;
        }
        if (!dw_done) g.launch(2 + 2 * l, [&] { bd::launch_depthwise(g.a, g.b, g.gw, L, g.stream); });
        if (stop_stage == 2 * l + 1) return BD_OK;
        pointwise(g, l);
        dw_done = false;
    }
    if (stop_stage < 0 && g.e->set.dev && g.logits) {
        // pool alone (a -> the embeddings, or the front of b: the last 1x1 convolution has read b), then the attached heads
        // behind it
        float* const pooled = g.emb ? g.emb : g.b;
        g.launch(28, [&] { bd::launch_pool_head(g.a, g.gw, nullptr, nullptr, 0, pooled, nullptr, g.stream); });
        return attached_head(g, pooled, g.b + (size_t)g.gw * BD_EMBEDDING_SIZE);
    }
    if (stop_stage < 0)
        g.launch(28, [&] {
            bd::launch_pool_head(g.a, g.gw, g.e->head_wt, g.e->head_b, g.e->n_classes, g.emb, g.logits, g.stream);
        });
    return BD_OK;
}

// The split-f16 launch set (modes 1 and 2) of one group.  A fused launcher that declines (shape guard, window limit) hands
// the rest of the group to walk_layers.
int pass_f16(Group& g) {
    const bd_engine* e = g.e;
    const bd::SepLayer* sep = g.sep;
    if (e->stem == 3 && e->separable != 0 && bd::l4_window_planes_supported(sep[1], sep[2], sep[3])) {
        // layers 1-2 + depthwise 3 (stemreg.hip), then pointwise 3 + layer 4 + depthwise 5 (l4_window_kernel): a -> b through
        // the split-f16 A tiles of pointwise 3.  Decided before the stem runs: nothing else reads those planes
        stem(g, bd::launch_stem_reg_planes);
        if (!g.launch(7, [&] { return bd::launch_l4_window_planes(g.a, sep[1], sep[2], sep[3], g.b, g.gw, g.stream); }))
            return fail(BD_EHIP, "l4_window_kernel declined the planes of the stem");
    } else {
        if (e->stem != 0) {
            // the layer-2 tile handed to depthwise 3 in registers (stemreg.hip), or through LDS (stem3_kernel, stem 5)
            stem(g, e->stem == 3 ? bd::launch_stem_reg : bd::launch_stem4);
        } else {
            conv1(g);
            walk_layers(g, 0, false, 4);
        }
        if (e->separable == 0) return walk_layers(g, 2, false, -1);
        // layer 4 + depthwise 5, a window per workgroup (l4_window_kernel): a -> b
        if (!g.launch(7, [&] { return bd::launch_separable_fused_next_dw(g.a, g.b, g.gw, sep[2], sep[3], g.stream); }))
            return walk_layers(g, 2, false, -1);
    }
    const bool planes = bd::tail_supported(sep[11], sep[12]);
    if (e->separable == 1 && planes && bd::separable_mid_planes_supported(sep[3], sep[4], sep[5]) &&
        bd::separable_chip_pw7_supported(sep[5], &sep[6], 5, sep[11], g.gw)) {
        // pointwise 5 -> layer 6 -> depthwise 7 (sepmid.hip), then pointwise 7 -> layers 8-12 -> depthwise 13 (sepchip.hip): b -> a
        // -> b through the split-f16 depthwise-7 planes, the second launch's output the planes septail.hip reads.  Decided
        // before the middle run: nothing else reads those planes
        if (!g.launch(13, [&] { return bd::launch_separable_mid_planes(g.b, g.a, g.gw, sep[3], sep[4], sep[5], g.stream); }))
            return fail(BD_EHIP, "sep_mid_kernel declined the depthwise-7 planes");
        if (!g.launch(23, [&] { return bd::launch_separable_chip_pw7(g.a, g.b, g.gw, sep[5], &sep[6], 5, sep[11], g.stream); }))
            return fail(BD_EHIP, "sep_chip_kernel declined the planes of the middle run");
    } else {
        // pointwise 5 -> layer 6 -> depthwise 7 -> pointwise 7 as one on-chip launch (sepmid.hip): b -> a.  Separable 10, or the
        // launcher declined: pointwise 5, layer 6 + depthwise 7 (sep_ws_kernel<1, 0>: a -> b), pointwise 7
        if (!(e->separable == 1 &&
              g.launch(13, [&] { return bd::launch_separable_mid(g.b, g.a, g.gw, sep[3], sep[4], sep[5], g.stream); }))) {
            pointwise(g, 3);
            if (!g.launch(11, [&] { return bd::launch_separable_fused_next_dw(g.a, g.b, g.gw, sep[4], sep[5], g.stream); }))
                return walk_layers(g, 4, false, -1);
            pointwise(g, 5);
        }
        // layers 8-12 + depthwise 13 as one on-chip launch (sepchip.hip): a -> b, as the f16 hi / lo planes septail.hip reads
        // when its kernel can follow, else as f32 for one kernel per op
        if (!g.launch(23, [&] { return bd::launch_separable_run_next_dw(g.a, g.b, g.gw, &sep[6], 7, g.stream, planes); }))
            return walk_layers(g, 6, false, -1);
        if (!planes) return walk_layers(g, 11, true, -1);
    }
    // pointwise 13 + depthwise 14 (planes b -> planes a), pointwise 14 + average pool (-> [windows][1024]) on septail.hip
    float* const pooled = g.emb ? g.emb : g.b;
    if (!g.launch(25, [&] { return bd::launch_tail_pw13_dw14(g.b, g.a, g.gw, sep[11], sep[12], g.stream); }) ||
        !g.launch(27, [&] { return bd::launch_tail_pw14_pool(g.a, pooled, g.gw, sep[12], g.stream); }))
        return fail(BD_EHIP, "septail.hip declined the planes of the on-chip run");
    return head(g, pooled);
}

// The exact-f32 launch set (mode 0) of one group, behind the fused stem (stem != 0).  Every kernel is bit-identical to the
// ones it replaces.  A fused launcher that declines hands the rest of the group to walk_layers.
int pass_f32(Group& g) {
    const bd_engine* e = g.e;
    const bd::SepLayer* sep = g.sep;
    // layers 1-3 on v_mfma_f32_32x32x2_f32 with the layer-2 tile handed over in registers (stemregf32.hip; stem 5 too)
    stem(g, bd::launch_stem_reg_f32);
    if (e->separable == 0) return walk_layers(g, 2, false, -1);
    // layer 4 + depthwise 5, the layer-4 tile handed over in registers (l4regf32.hip): a -> b
    if (!g.launch(7, [&] { return bd::launch_l4_reg_f32(g.a, g.b, g.gw, sep[2], sep[3], g.stream); }))
        return walk_layers(g, 2, false, -1);
    // pointwise 5 -> layer 6 -> layer 7 as one launch (sepmidf32.hip): b -> a.  Separable 10, or the launcher declined: the 1x1
    // convolutions of layers 5, 6 and 7, each with the next depthwise in its epilogue (b -> a, then swapped: b holds it)
    bool dw8_done = false;
    if (!(e->separable == 1 &&
          g.launch(13, [&] { return bd::launch_separable_mid_f32(g.b, g.a, g.gw, sep[3], sep[4], sep[5], g.stream); }))) {
        for (int l = 3; l < 6; ++l) {
            if (!g.launch(3 + 2 * l, [&] { return bd::launch_pointwise_next_dw_f32(g.b, g.a, g.gw, sep[l], sep[l + 1], g.stream); }))
                return walk_layers(g, l, true, -1);
            std::swap(g.a, g.b);
        }
        dw8_done = true;
    }
    // layers 8-12 + depthwise 13 as one launch whose tiles stay on the CU (sepchipf32.hip): the layer-7 output in a (or the
    // depthwise-8 output in b) -> the depthwise-13 output in the other buffer
    if (!g.launch(23, [&] {
            return dw8_done ? bd::launch_separable_chip_f32(g.b, g.a, g.gw, &sep[6], 5, g.stream, &sep[11], true)
                            : bd::launch_separable_chip_f32(g.a, g.b, g.gw, &sep[6], 5, g.stream, &sep[11], false);
        }))
        return walk_layers(g, 6, dw8_done, -1);
    if (dw8_done) std::swap(g.a, g.b);
    // pointwise 13 + depthwise 14 (b -> a), pointwise 14 + average pool (-> [windows][1024]) on septail.hip
    if (!bd::tail_f32_supported(sep[11], sep[12])) return walk_layers(g, 11, true, -1);
    float* const pooled = g.emb ? g.emb : g.b;
    if (!g.launch(25, [&] { return bd::launch_tail_f32(g.b, g.a, pooled, g.gw, sep[11], sep[12], g.stream, 0); }) ||
        !g.launch(27, [&] { return bd::launch_tail_f32(g.b, g.a, pooled, g.gw, sep[11], sep[12], g.stream, 1); }))
        return fail(BD_EHIP, "septail.hip declined the exact-f32 tail");
    return head(g, pooled);
}

// Calibration, the stage taps and the exact-f32 mode with stem 0: one kernel per op from conv1 on.  An f16 tap at or behind
// stage 4 keeps the fused stem (stemreg.hip only when the tap is its output, stem3_kernel otherwise, even with stem 3) and
// the depthwise fusions of walk_layers.
int pass_per_op(Group& g, int stop_stage) {
    if (g.sep[0].pw_mode != 0 && g.e->stem != 0 && stop_stage >= 4) {
        stem(g, g.e->stem == 3 && stop_stage == 4 ? bd::launch_stem_reg : bd::launch_stem4);
        return walk_layers(g, 2, false, stop_stage);
    }
    conv1(g);
    return walk_layers(g, 0, false, stop_stage);
}

// The launch plan of one batch of chunks.  stop_stage < 0: run everything; otherwise stop after that CNN
// stage of the first group and copy it to tap_out.
// chunk_pcm[c]: device pointer of chunk c (4-byte aligned; the packed entry points pass pcm + the samples before it).
// mode: arithmetic of the 1x1 convolutions for THIS call (-1: the handle's).  range_word: the word this call's kernels
// raise instead of the engine's sticky one (device memory, or pinned host memory - the kernels then write across PCIe,
// which only ever happens when a chunk does leave the range), or null.  calibrating: the depthwise kernels report their
// largest output into e->d_amax (exact-f32, one kernel per op).
int run_chunks(bd_engine* e, const float* const* chunk_pcm, const int64_t* chunk_samples, int32_t n_chunks, int32_t hop,
               int32_t step, void* ws, int64_t ws_bytes, float* emb, float* logits, int stop_stage, int tap_windows,
               float* tap_out, int mode_arg, int32_t* range_word, bool calibrating, hipStream_t stream) {
    if (!e) return fail(BD_EINVAL, "null handle");
    if (misaligned(ws) || misaligned(emb) || misaligned(logits) || misaligned(tap_out))
        return fail(BD_EINVAL, "device pointers need 16-byte alignment");
    if (mode_arg < -1 || mode_arg > 2) return fail(BD_EINVAL, "mode must be -1 (the handle's), 0, 1 or 2");
    if (logits && e->n_classes == 0) return fail(BD_EINVAL, "engine was created without a head");
    if (!chunk_pcm) return fail(BD_EINVAL, "null chunk pointer table");
    BatchPlan plan;
    int rc = plan_batch(chunk_samples, n_chunks, hop, step, &plan);
    if (rc < 0) return rc;
    for (int c = 0; c < n_chunks; ++c) {
        if (!chunk_pcm[c] && chunk_samples[c] > 0) return fail(BD_EINVAL, "null pcm pointer");
        if (reinterpret_cast<uintptr_t>(chunk_pcm[c]) & 3u) return fail(BD_EINVAL, "pcm pointers need 4-byte alignment");
    }
    const int mode = calibrating ? 0 : (mode_arg < 0 ? e->pointwise_mode : mode_arg);
    BD_HIP(hipSetDevice(e->device));
    unsigned* flag = e->d_range_flag;
    if (range_word) {
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, range_word) != hipSuccess || !attr.devicePointer) {
            (void)hipGetLastError();
            return fail(BD_EINVAL, "range_word must be device memory or pinned (device-mapped) host memory");
        }
        flag = static_cast<unsigned*>(attr.devicePointer);
    }
    bd::SepLayer sep[13];                     // this call's view of the layers: its own mode, range word, calibration words
    for (int l = 0; l < 13; ++l) {
        sep[l] = e->sep[l];
        sep[l].pw_mode = mode;
        sep[l].range_flag = flag;
        sep[l].amax = calibrating ? e->d_amax + l : nullptr;
    }
    const int64_t n_windows = plan.total_windows;
    const Workspace layout = workspace_layout(e, plan.total_frames, n_windows);
    if (!ws || ws_bytes < layout.total) return fail(BD_EWORKSPACE, "workspace smaller than bd_workspace_bytes()");
    if (stop_stage >= 0 && (tap_windows <= 0 || tap_windows > n_windows || tap_windows > e->group_windows))
        return fail(BD_EINVAL, "bd_stage_tap: windows must be in 1..min(n_windows, group)");

    const int64_t group = n_windows < e->group_windows ? n_windows : e->group_windows;
    char* base = static_cast<char*>(ws);
    float* const logmel = reinterpret_cast<float*>(base);
    float* const buf_a = reinterpret_cast<float*>(base + layout.buf_a);
    float* const buf_b = reinterpret_cast<float*>(base + layout.buf_b);

    if (e->profiling) mark(e, stream, -1);
    for (int c = 0; c < n_chunks; ++c)        // one front-end launch per chunk: its padding is its own
        launch(e, stream, 0, [&] {
            bd::launch_logmel(chunk_pcm[c], chunk_samples[c], plan.frames[c],
                              logmel + (int64_t)plan.map.frame_base[c] * BD_MEL_BANDS, e->d_tables, stream);
        });
    for (int64_t w0 = 0; w0 < n_windows; w0 += group) {
        const int gw = stop_stage >= 0 ? tap_windows : (int)(n_windows - w0 < group ? n_windows - w0 : group);
        Group g{e, sep, stream, logmel, &plan.map, step, (int)w0, gw, buf_a, buf_b,
                emb ? emb + w0 * BD_EMBEDDING_SIZE : nullptr, logits ? logits + w0 * e->n_classes : nullptr};
        if (stop_stage >= 0 || calibrating || (mode == 0 && e->stem == 0)) rc = pass_per_op(g, stop_stage);
        else rc = mode != 0 ? pass_f16(g) : pass_f32(g);
        if (rc < 0) return rc;
        if (stop_stage >= 0) {
            // the tap: stage 0 is layer 2's input, stage 2 l + 1 / 2 l + 2 the depthwise / 1x1 output of layer index l
            const bool dw = stop_stage & 1;
            const bd::SepLayer& L = sep[stop_stage == 0 ? 0 : (stop_stage - 1) / 2];
            const int64_t floats = stop_stage == 0 ? (int64_t)gw * L.h_in * L.w_in * L.cin
                                                   : (int64_t)gw * L.h_out * L.w_out * (dw ? L.cin : L.cout);
            if (mode != 0 && dw) {
                // a depthwise output of the f16 modes carries its layer's power-of-two activation scale: hand out the true values
                bd::launch_scale_copy(g.b, tap_out, floats, std::ldexp(1.0f, -L.act_exp), stream);
            } else {
                BD_HIP(hipMemcpyAsync(tap_out, dw ? g.b : g.a, floats * sizeof(float), hipMemcpyDeviceToDevice, stream));
            }
            break;
        }
    }
    BD_HIP(hipGetLastError());
    return BD_OK;
}

// chunk pointers of the packed entry points: chunk c starts where chunk c - 1 ended
int run_packed(bd_engine* e, const float* pcm, const int64_t* chunk_samples, int32_t n_chunks, int32_t hop, int32_t step,
               void* ws, int64_t ws_bytes, float* emb, float* logits, int stop_stage, int tap_windows, float* tap_out,
               hipStream_t stream) {
    if (!chunk_samples || n_chunks <= 0 || n_chunks > bd::kMaxBatchChunks) return fail(BD_EINVAL, "batch must hold 1..64 chunks");
    if (misaligned(pcm)) return fail(BD_EINVAL, "device pointers need 16-byte alignment");
    const float* ptrs[bd::kMaxBatchChunks];
    int64_t at = 0;
    for (int c = 0; c < n_chunks; ++c) {
        if (chunk_samples[c] < 0) return fail(BD_EINVAL, "n_samples must be >= 0");
        if (!pcm && chunk_samples[c] > 0) return fail(BD_EINVAL, "null pcm pointer");
        ptrs[c] = pcm ? pcm + at : nullptr;
        at += chunk_samples[c];
    }
    return run_chunks(e, ptrs, chunk_samples, n_chunks, hop, step, ws, ws_bytes, emb, logits, stop_stage, tap_windows, tap_out,
                      -1, nullptr, false, stream);
}

// ---- operand scaling of the f16 modes (SepLayer in bd_internal.h) ----

// Exponent s with amax * 2^s in [2^8, 2^9): a factor 128 below the f16 overflow for inputs beyond the calibration set,
// and hi + lo both normal f16 numbers (22-bit operands) for every activation down to 2^-11 of the layer's largest.
int exponent_for(float amax) {
    if (!(amax > 0.0f) || !(amax <= 3.0e38f)) return 0;
    int ex = 0;
    (void)std::frexp(amax, &ex);
    const int s = 9 - ex;
    return s > 60 ? 60 : (s < -60 ? -60 : s);
}

}  // namespace

int bd::apply_scales(bd_engine* e) {
    BD_HIP(hipSetDevice(e->device));
    std::vector<float> buf;
    for (int l = 0; l < 13; ++l) {
        bd::SepLayer& L = e->sep[l];
        const int s = e->act_exp[l];
        buf.resize(e->h_dw[l].size());
        for (size_t i = 0; i < buf.size(); ++i) {
            buf[i] = std::ldexp(e->h_dw[l][i], s);
            if (!std::isfinite(buf[i])) return fail(BD_EWEIGHTS, "activation scale overflows a depthwise weight");
        }
        BD_HIP(hipMemcpy(e->d_pool + e->off_dw16[l], buf.data(), buf.size() * sizeof(float), hipMemcpyHostToDevice));
        buf.resize(L.cout);
        for (int n = 0; n < L.cout; ++n) buf[n] = std::ldexp(1.0f, -(s + e->row_exp[l][n]));
        BD_HIP(hipMemcpy(e->d_pool + e->off_pw_u[l], buf.data(), buf.size() * sizeof(float), hipMemcpyHostToDevice));
        L.act_exp = s;
    }
    return BD_OK;
}

namespace {

// One exact-f32 pass (one kernel per op) over the given chunks with the depthwise kernels reporting their largest
// output; the per-layer maxima only ever grow, the exponents follow them.  Waits for the stream.
int calibrate_on(bd_engine* e, const float* const* chunk_pcm, const int64_t* chunk_samples, int32_t n_chunks, int32_t hop,
                 int32_t step, void* ws, int64_t ws_bytes, hipStream_t stream) {
    BD_HIP(hipSetDevice(e->device));
    BD_HIP(hipMemsetAsync(e->d_amax, 0, 64, stream));
    const int rc = run_chunks(e, chunk_pcm, chunk_samples, n_chunks, hop, step, ws, ws_bytes, nullptr, nullptr, -1, 0, nullptr,
                              0, nullptr, true, stream);
    if (rc < 0) return rc;
    unsigned words[16] = {0};
    BD_HIP(hipMemcpyAsync(words, e->d_amax, 64, hipMemcpyDeviceToHost, stream));
    BD_HIP(hipStreamSynchronize(stream));
    for (int l = 0; l < 13; ++l) {
        float m;
        std::memcpy(&m, &words[l], sizeof(m));
        if (m > e->act_max[l] && m <= 3.0e38f) e->act_max[l] = m;
        e->act_exp[l] = exponent_for(e->act_max[l]);
    }
    return bd::apply_scales(e);
}

// The signal bd_create calibrates on: sixteen 0.96 s windows that span what 16 kHz PCM in [-1, 1] can do to the log-mel
// input (silence = the log(0.001) floor everywhere, full-scale noise = the ceiling everywhere, tones, clicks, a chirp,
// a buzz-like square wave).  The CNN's input is a LOG spectrum, so a recording can leave this envelope only by a small
// factor; the exponents keep a factor 128 in hand and the range word catches whatever goes beyond.
std::vector<float> calibration_signal() {
    const int seg = 15360, nseg = 16;
    std::vector<float> x((size_t)seg * nseg + 240, 0.0f);
    uint32_t lcg = 20260723u;
    auto uni = [&]() {                                     // uniform in [-1, 1)
        lcg = lcg * 1664525u + 1013904223u;
        return (float)((int32_t)lcg) * (1.0f / 2147483648.0f);
    };
    const double w = 2.0 * M_PI / 16000.0;
    for (int g = 0; g < nseg; ++g)
        for (int i = 0; i < seg; ++i) {
            const double t = i;
            double v = 0.0;
            switch (g) {
                case 0: v = 0.0; break;
                case 1: v = uni(); break;
                case 2: v = 0.1 * uni(); break;
                case 3: v = 0.01 * uni(); break;
                case 4: v = 0.001 * uni(); break;
                case 5: v = 0.9 * std::sin(w * 220.0 * t); break;
                case 6: v = 0.5 * std::sin(w * 1000.0 * t) + 0.05 * uni(); break;
                case 7: v = 0.9 * std::sin(w * 4000.0 * t); break;
                case 8: v = 0.7 * std::sin(w * (100.0 + 6900.0 * t / (2.0 * seg)) * t); break;
                case 9: v = i % 1000 == 0 ? 1.0 : 0.0; break;
                case 10: v = std::sin(w * 300.0 * t) >= 0.0 ? 1.0 : -1.0; break;
                case 11: v = 0.3 * uni() * (0.5 + 0.5 * std::sin(w * 200.0 * t)); break;
                case 12: v = 0.5 + 0.0001 * uni(); break;
                case 13: v = 0.8 * std::sin(w * 50.0 * t) + 0.2 * std::sin(w * 150.0 * t); break;
                case 14: v = uni() >= 0.0f ? 1.0 : -1.0; break;
                default: v = uni() * t / seg; break;
            }
            v = v > 1.0 ? 1.0 : (v < -1.0 ? -1.0 : v);
            x[(size_t)g * seg + i] = (float)v;
        }
    return x;
}

}  // namespace

int bd::calibrate_builtin(bd_engine* e) {
    const std::vector<float> sig = calibration_signal();
    const int64_t n = (int64_t)sig.size();
    const int32_t hop = 15360, step = 96;
    const int64_t ws_bytes = bd_workspace_bytes(e, n, hop, step);
    if (ws_bytes < 0) return (int)ws_bytes;
    float* d_pcm = nullptr;
    void* d_ws = nullptr;
    hipError_t err = hipMalloc(&d_pcm, sig.size() * sizeof(float));
    if (err == hipSuccess) err = hipMalloc(&d_ws, (size_t)ws_bytes);
    if (err == hipSuccess) err = hipMemcpy(d_pcm, sig.data(), sig.size() * sizeof(float), hipMemcpyHostToDevice);
    int rc = BD_OK;
    if (err != hipSuccess) {
        rc = fail(BD_EHIP, std::string("bd_create (calibration): ") + hipGetErrorString(err));
    } else {
        const float* ptr = d_pcm;
        rc = calibrate_on(e, &ptr, &n, 1, hop, step, d_ws, ws_bytes, nullptr);
    }
    if (d_pcm) (void)hipFree(d_pcm);
    if (d_ws) (void)hipFree(d_ws);
    return rc;
}

extern "C" {

int64_t bd_workspace_bytes(bd_handle h, int64_t n_samples, int32_t hop_samples, int32_t patch_step) {
    if (!h) return fail(BD_EINVAL, "bd_workspace_bytes: null handle");
    if (patch_step <= 0) return fail(BD_EINVAL, "patch_step must be > 0");
    Geometry g;
    const int rc = geometry(n_samples, hop_samples, patch_step, &g);
    if (rc < 0) return rc;
    return workspace_layout(h, g.n_frames, g.n_windows).total;
}

int bd_frontend(bd_handle h, const float* pcm_dev, int64_t n_samples, int32_t hop_samples, float* logmel_dev,
                void* stream) {
    if (!h || !logmel_dev || (!pcm_dev && n_samples > 0)) return fail(BD_EINVAL, "bd_frontend: null argument");
    if (misaligned(pcm_dev) || misaligned(logmel_dev)) return fail(BD_EINVAL, "bd_frontend: pointers need 16-byte alignment");
    Geometry g;
    const int rc = geometry(n_samples, hop_samples, 0, &g);
    if (rc < 0) return rc;
    BD_HIP(hipSetDevice(h->device));
    if (h->profiling) mark(h, (hipStream_t)stream, -1);
    launch(h, (hipStream_t)stream, 0,
           [&] { bd::launch_logmel(pcm_dev, n_samples, g.n_frames, logmel_dev, h->d_tables, (hipStream_t)stream); });
    BD_HIP(hipGetLastError());
    return BD_OK;
}

int bd_patches(bd_handle h, const float* logmel_dev, int64_t n_frames, int32_t patch_step, float* patches_dev,
               void* stream) {
    if (!h || !logmel_dev || !patches_dev) return fail(BD_EINVAL, "bd_patches: null argument");
    if (patch_step <= 0 || n_frames < 0) return fail(BD_EINVAL, "bd_patches: bad size");
    if (misaligned(logmel_dev) || misaligned(patches_dev)) return fail(BD_EINVAL, "bd_patches: pointers need 16-byte alignment");
    const int64_t w = n_frames >= BD_PATCH_FRAMES ? 1 + (n_frames - BD_PATCH_FRAMES) / patch_step : 0;
    BD_HIP(hipSetDevice(h->device));
    bd::launch_patches(logmel_dev, w, patch_step, patches_dev, (hipStream_t)stream);
    BD_HIP(hipGetLastError());
    return BD_OK;
}

int bd_embed(bd_handle h, const float* pcm_dev, int64_t n_samples, int32_t hop_samples, int32_t patch_step,
             void* workspace_dev, int64_t workspace_bytes, float* emb_dev, void* stream) {
    if (!emb_dev) return fail(BD_EINVAL, "bd_embed: null output");
    return run_packed(h, pcm_dev, &n_samples, 1, hop_samples, patch_step, workspace_dev, workspace_bytes, emb_dev,
                      nullptr, -1, 0, nullptr, (hipStream_t)stream);
}

int bd_predict(bd_handle h, const float* pcm_dev, int64_t n_samples, int32_t hop_samples, int32_t patch_step,
               void* workspace_dev, int64_t workspace_bytes, float* emb_dev, float* logits_dev, void* stream) {
    if (!logits_dev) return fail(BD_EINVAL, "bd_predict: null output");
    return run_packed(h, pcm_dev, &n_samples, 1, hop_samples, patch_step, workspace_dev, workspace_bytes, emb_dev,
                      logits_dev, -1, 0, nullptr, (hipStream_t)stream);
}

int64_t bd_batch_num_windows(const int64_t* chunk_samples, int32_t n_chunks, int32_t hop_samples, int32_t patch_step,
                             int64_t* per_chunk_windows) {
    BatchPlan plan;
    const int rc = plan_batch(chunk_samples, n_chunks, hop_samples, patch_step, &plan);
    if (rc < 0) return rc;
    if (per_chunk_windows)
        for (int c = 0; c < n_chunks; ++c) per_chunk_windows[c] = plan.map.win_start[c + 1] - plan.map.win_start[c];
    return plan.total_windows;
}

int64_t bd_batch_workspace_bytes(bd_handle h, const int64_t* chunk_samples, int32_t n_chunks, int32_t hop_samples,
                                 int32_t patch_step) {
    if (!h) return fail(BD_EINVAL, "bd_batch_workspace_bytes: null handle");
    BatchPlan plan;
    const int rc = plan_batch(chunk_samples, n_chunks, hop_samples, patch_step, &plan);
    if (rc < 0) return rc;
    return batch_workspace(h, plan);
}

int bd_predict_batch(bd_handle h, const float* pcm_dev, const int64_t* chunk_samples, int32_t n_chunks,
                     int32_t hop_samples, int32_t patch_step, void* workspace_dev, int64_t workspace_bytes,
                     float* emb_dev, float* logits_dev, void* stream) {
    if (!logits_dev && !emb_dev) return fail(BD_EINVAL, "bd_predict_batch: no output requested");
    return run_packed(h, pcm_dev, chunk_samples, n_chunks, hop_samples, patch_step, workspace_dev, workspace_bytes,
                      emb_dev, logits_dev, -1, 0, nullptr, (hipStream_t)stream);
}

int bd_predict_chunks(bd_handle h, const float* const* chunk_pcm_dev, const int64_t* chunk_samples, int32_t n_chunks,
                      int32_t hop_samples, int32_t patch_step, void* workspace_dev, int64_t workspace_bytes, float* emb_dev,
                      float* logits_dev, int32_t mode, int32_t* range_word, void* stream) {
    if (!logits_dev && !emb_dev) return fail(BD_EINVAL, "bd_predict_chunks: no output requested");
    if (!chunk_pcm_dev || !chunk_samples || n_chunks <= 0 || n_chunks > bd::kMaxBatchChunks)
        return fail(BD_EINVAL, "batch must hold 1..64 chunks");
    return run_chunks(h, chunk_pcm_dev, chunk_samples, n_chunks, hop_samples, patch_step, workspace_dev, workspace_bytes,
                      emb_dev, logits_dev, -1, 0, nullptr, mode, range_word, false, (hipStream_t)stream);
}

int bd_calibrate(bd_handle h, const float* pcm_dev, int64_t n_samples, int32_t hop_samples, int32_t patch_step,
                 void* workspace_dev, int64_t workspace_bytes, void* stream) {
    if (!h) return fail(BD_EINVAL, "bd_calibrate: null handle");
    if (!pcm_dev && n_samples > 0) return fail(BD_EINVAL, "bd_calibrate: null pcm pointer");
    if (misaligned(pcm_dev)) return fail(BD_EINVAL, "device pointers need 16-byte alignment");
    return calibrate_on(h, &pcm_dev, &n_samples, 1, hop_samples, patch_step, workspace_dev, workspace_bytes,
                        (hipStream_t)stream);
}

int bd_get_scales(bd_handle h, int32_t* act_exp, float* act_max) {
    if (!h) return fail(BD_EINVAL, "bd_get_scales: null handle");
    for (int l = 0; l < 13; ++l) {
        if (act_exp) act_exp[l] = h->act_exp[l];
        if (act_max) act_max[l] = h->act_max[l];
    }
    return 13;
}

int bd_set_activation_exponents(bd_handle h, const int32_t* act_exp) {
    if (!h || !act_exp) return fail(BD_EINVAL, "bd_set_activation_exponents: null argument");
    for (int l = 0; l < 13; ++l)
        if (act_exp[l] < -60 || act_exp[l] > 60) return fail(BD_EINVAL, "bd_set_activation_exponents: exponent outside -60..60");
    for (int l = 0; l < 13; ++l) h->act_exp[l] = act_exp[l];
    return bd::apply_scales(h);
}

int bd_stage_tap(bd_handle h, const float* pcm_dev, int64_t n_samples, int32_t hop_samples, int32_t patch_step,
                 void* workspace_dev, int64_t workspace_bytes, int32_t stage, int32_t windows, float* out_dev,
                 void* stream) {
    if (!out_dev) return fail(BD_EINVAL, "bd_stage_tap: null output");
    if (stage < 0 || stage >= BD_NUM_STAGES) return fail(BD_EINVAL, "bd_stage_tap: stage out of range");
    return run_packed(h, pcm_dev, &n_samples, 1, hop_samples, patch_step, workspace_dev, workspace_bytes, nullptr,
                      nullptr, stage, windows, out_dev, (hipStream_t)stream);
}

// The scratch of the attached heads for one group of bd_score_rows: the regions attached_head carves (a set's three, and the
// wide rows of an ensemble behind them); the packaged head needs none
static int64_t score_rows_scratch(const bd_engine* e, int64_t windows) {
    if (!e->set.dev) return 0;
    const int64_t group = windows < e->group_windows ? windows : e->group_windows;
    return group * (bd::kHeadSetRegions + 1) * bd::kHeadSetRow * (int64_t)sizeof(float);
}

int64_t bd_score_rows_workspace_bytes(bd_handle h, int64_t windows) {
    if (!h) return fail(BD_EINVAL, "bd_score_rows_workspace_bytes: null handle");
    if (windows < 0 || windows > BD_ROWS_MAX_WINDOWS)
        return fail(BD_EINVAL, "bd_score_rows_workspace_bytes: windows = " + std::to_string(windows) + ", a call takes 0.." +
                                   std::to_string(BD_ROWS_MAX_WINDOWS));
    if (h->n_classes == 0) return fail(BD_EINVAL, "bd_score_rows_workspace_bytes: engine was created without a head");
    return score_rows_scratch(h, windows);
}

int bd_score_rows(bd_handle h, const float* rows_dev, int64_t windows, float* logits_dev, void* workspace_dev,
                  int64_t workspace_bytes, void* stream) {
    if (!h) return fail(BD_EINVAL, "bd_score_rows: null handle");
    if (h->n_classes == 0) return fail(BD_EINVAL, "bd_score_rows: engine was created without a head");
    if (windows < 0 || windows > BD_ROWS_MAX_WINDOWS)
        return fail(BD_EINVAL, "bd_score_rows: windows = " + std::to_string(windows) + ", a call takes 0.." +
                                   std::to_string(BD_ROWS_MAX_WINDOWS));
    if (windows == 0) return BD_OK;
    if (!rows_dev || misaligned(rows_dev)) return fail(BD_EINVAL, "bd_score_rows: rows_dev is null or not 16-byte aligned");
    if (!logits_dev || misaligned(logits_dev)) return fail(BD_EINVAL, "bd_score_rows: logits_dev is null or not 16-byte aligned");
    const int64_t need = score_rows_scratch(h, windows);
    if (misaligned(workspace_dev)) return fail(BD_EINVAL, "bd_score_rows: workspace_dev is not 16-byte aligned");
    if (need > 0 && (!workspace_dev || workspace_bytes < need))
        return fail(BD_EWORKSPACE, "bd_score_rows: workspace smaller than bd_score_rows_workspace_bytes()");
    BD_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (h->profiling) mark(h, s, -1);
    for (int64_t w0 = 0; w0 < windows; w0 += h->group_windows) {
        const int gw = (int)(windows - w0 < h->group_windows ? windows - w0 : h->group_windows);
        Group g{h, nullptr, s, nullptr, nullptr, 0, (int)w0, gw, nullptr, nullptr, nullptr, logits_dev + w0 * h->n_classes};
        const float* pooled = rows_dev + w0 * BD_EMBEDDING_SIZE;
        const int rc = h->set.dev ? attached_head(g, pooled, static_cast<float*>(workspace_dev)) : head(g, pooled);
        if (rc < 0) return rc;
    }
    BD_HIP(hipGetLastError());
    return BD_OK;
}

int bd_debug_pointwise(const float* a_dev, const float* wt_dev, const float* bias_dev, float* c_dev, int64_t m,
                       int32_t n, int32_t k, int32_t variant, void* stream) {
    if (!a_dev || !wt_dev || !bias_dev || !c_dev || m < 0) return fail(BD_EINVAL, "bd_debug_pointwise: bad argument");
    if (bd::launch_pointwise_variant(a_dev, wt_dev, bias_dev, c_dev, m, n, k, variant, (hipStream_t)stream) != 0)
        return fail(BD_EINVAL, "bd_debug_pointwise: shape/variant not supported (K % 32, N % tile)");
    BD_HIP(hipGetLastError());
    return BD_OK;
}

int bd_debug_pointwise_f16x3(const float* a_dev, const void* whi_dev, const void* wlo_dev, const float* unscale_dev,
                             const float* bias_dev, float* c_dev, int64_t m, int32_t n, int32_t k, int32_t variant,
                             void* stream) {
    if (!a_dev || !whi_dev || !wlo_dev || !unscale_dev || !bias_dev || !c_dev || m < 0)
        return fail(BD_EINVAL, "bd_debug_pointwise_f16x3: bad argument");
    if (bd::launch_pointwise_f16x3_variant(a_dev, whi_dev, wlo_dev, unscale_dev, bias_dev, c_dev, m, n, k, variant,
                                           (hipStream_t)stream) != 0)
        return fail(BD_EINVAL, "bd_debug_pointwise_f16x3: shape/variant not supported");
    BD_HIP(hipGetLastError());
    return BD_OK;
}

}  // extern "C"
