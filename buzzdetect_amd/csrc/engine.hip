// C-ABI host layer of libbuzzdetect_hip.so (include/buzzdetect_hip.h): the error state, the framing exports, the life of an
// engine handle (bd_create / bd_destroy), its setters, the range flag and per-stage event timing.  The handle and the map of
// the other host files are in engine_state.h.
#include <cstring>
#include <string>

#include "engine_state.h"

namespace {

thread_local std::string g_error;

}  // namespace

namespace bd {
void set_error(const std::string& msg) { g_error = msg; }
}  // namespace bd

extern "C" {

int bd_abi_version(void) { return BD_ABI_VERSION; }

const char* bd_last_error(void) { return g_error.c_str(); }

int64_t bd_padded_length(int64_t n_samples, int32_t hop_samples) {
    Geometry g;
    const int rc = geometry(n_samples, hop_samples, 0, &g);
    return rc < 0 ? rc : g.n_padded;
}

int64_t bd_num_frames(int64_t n_samples, int32_t hop_samples) {
    Geometry g;
    const int rc = geometry(n_samples, hop_samples, 0, &g);
    return rc < 0 ? rc : g.n_frames;
}

int64_t bd_num_windows(int64_t n_samples, int32_t hop_samples, int32_t patch_step) {
    if (patch_step <= 0) return fail(BD_EINVAL, "patch_step must be > 0");
    Geometry g;
    const int rc = geometry(n_samples, hop_samples, patch_step, &g);
    return rc < 0 ? rc : g.n_windows;
}

int bd_stage_shape(int32_t stage, int32_t* h, int32_t* w, int32_t* c) {
    if (stage < 0 || stage >= BD_NUM_STAGES || !h || !w || !c) return fail(BD_EINVAL, "bad stage");
    int hh = 96, ww = 64, cc = 1;
    // stage 0 = conv1; stage 2k-1 = depthwise of layer k+1, stage 2k = its pointwise
    hh = 48, ww = 32, cc = 32;
    for (int s = 1; s <= stage; ++s) {
        const int layer = (s + 1) / 2;   // index into kLayerDefs (1..13)
        if (s & 1) {                     // depthwise
            if (kLayerDefs[layer][0] == 2) {
                hh /= 2;
                ww /= 2;
            }
        } else {
            cc = kLayerDefs[layer][1];
        }
    }
    *h = hh;
    *w = ww;
    *c = cc;
    return BD_OK;
}

int bd_create(bd_handle* out, int device, const bd_weights* w) {
    if (!out || !w) return fail(BD_EINVAL, "bd_create: null argument");
    *out = nullptr;
    if (!w->embedder_blob || !w->mel) return fail(BD_EINVAL, "bd_create: embedder_blob and mel are required");
    if (w->embedder_floats != BD_EMBEDDER_BLOB_FLOATS)
        return fail(BD_EWEIGHTS, "bd_create: embedder blob must hold exactly 3217344 floats "
                                 "(payload of variables.data-00000-of-00001)");
    if (w->n_classes < 0 || w->n_classes > BD_MAX_CLASSES) return fail(BD_EINVAL, "bd_create: n_classes out of range");
    if (w->n_classes > 0 && (!w->head_kernel || !w->head_bias))
        return fail(BD_EINVAL, "bd_create: head_kernel/head_bias missing");

    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(BD_ENODEVICE, "bd_create: no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= count) return fail(BD_ENODEVICE, "bd_create: device index out of range");
    hipDeviceProp_t prop;
    BD_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(BD_ENODEVICE, std::string("bd_create: kernels are built for gfx950 only, device is ") +
                                      prop.gcnArchName);
    BD_HIP(hipSetDevice(device));

    bd::FoldedWeights folded;                 // (weights_fold.hip; refuses bad weights before anything is allocated)
    int rc = bd::fold_weights(*w, &folded);
    if (rc < 0) return rc;
    std::vector<float>& host = folded.image;

    bd_engine* e = new bd_engine();
    e->device = device;
    e->n_classes = w->n_classes;
    hipError_t err = hipMalloc(&e->d_pool, host.size() * sizeof(float));
    if (err == hipSuccess) err = hipMalloc(&e->d_tables, sizeof(bd::FeTables));
    if (err == hipSuccess) err = hipMalloc(&e->d_range_flag, 256);
    if (err == hipSuccess) err = hipMemset(e->d_range_flag, 0, 256);
    if (err == hipSuccess) err = hipMalloc(&e->d_amax, 64);
    if (err == hipSuccess) err = hipMemset(e->d_amax, 0, 64);
    if (err == hipSuccess) err = hipMemcpy(e->d_pool, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(e->d_tables, &folded.tables, sizeof(folded.tables), hipMemcpyHostToDevice);
    if (err != hipSuccess) {
        if (e->d_pool) (void)hipFree(e->d_pool);
        if (e->d_tables) (void)hipFree(e->d_tables);
        if (e->d_range_flag) (void)hipFree(e->d_range_flag);
        if (e->d_amax) (void)hipFree(e->d_amax);
        delete e;
        return fail(BD_EHIP, std::string("bd_create: ") + hipGetErrorString(err));
    }
    e->conv1_w = e->d_pool + folded.conv1_w;
    e->conv1_b = e->d_pool + folded.conv1_b;
    int h = 48, wd = 32;
    int cin = kLayerDefs[0][1];
    for (int l = 0; l < 13; ++l) {
        const bd::LayerOffsets& o = folded.layer[l];
        bd::SepLayer& L = e->sep[l];
        L.cin = cin;
        L.cout = kLayerDefs[l + 1][1];
        L.stride = kLayerDefs[l + 1][0];
        L.h_in = h;
        L.w_in = wd;
        L.h_out = (h + L.stride - 1) / L.stride;
        L.w_out = (wd + L.stride - 1) / L.stride;
        L.dw_w = e->d_pool + o.dw_w;
        L.dw_b = e->d_pool + o.dw_b;
        L.pw_wt = e->d_pool + o.pw_w;
        L.pw_b = e->d_pool + o.pw_b;
        L.pw_variant = 0;
        L.pw_whi = e->d_pool + o.pw_hi;
        L.pw_wlo = e->d_pool + o.pw_lo;
        L.pw_fhi = e->d_pool + o.pw_fhi;
        L.pw_flo = e->d_pool + o.pw_flo;
        L.pw_ffrag = o.pw_ffrag ? e->d_pool + o.pw_ffrag : nullptr;
        L.pw_variant16 = 0;
        L.pw_mode = e->pointwise_mode;
        L.range_flag = e->d_range_flag;
        L.dw_w16 = e->d_pool + o.dw16;
        L.dw_b16 = L.dw_w16 + 9 * (size_t)cin;
        L.pw_u = e->d_pool + o.pw_u;
        L.act_exp = 0;
        L.amax = nullptr;
        e->off_dw16[l] = o.dw16;
        e->off_pw_u[l] = o.pw_u;
        e->row_exp[l] = o.row_exp;
        e->h_dw[l].assign(host.begin() + o.dw_w, host.begin() + o.dw_w + 9 * (size_t)cin);
        e->h_dw[l].insert(e->h_dw[l].end(), host.begin() + o.dw_b, host.begin() + o.dw_b + cin);
        h = L.h_out;
        wd = L.w_out;
        cin = L.cout;
    }
    if (w->n_classes > 0) {
        e->head_wt = e->d_pool + folded.head_w;
        e->head_b = e->d_pool + folded.head_b;
    }
    // activation scales of the f16 modes from a pass over the built-in calibration signal in exact-f32 arithmetic
    rc = bd::apply_scales(e);
    if (rc == BD_OK) rc = bd::calibrate_builtin(e);
    if (rc < 0) {
        const std::string msg = g_error;
        (void)bd_destroy(e);
        return fail(rc, msg);
    }
    *out = e;
    return BD_OK;
}

int bd_destroy(bd_handle h) {
    if (!h) return BD_OK;
    (void)hipSetDevice(h->device);
    for (auto& ev : h->pending) (void)hipEventDestroy(ev.ev);
    for (auto& ev : h->free_events) (void)hipEventDestroy(ev.ev);
    if (h->d_pool) (void)hipFree(h->d_pool);
    if (h->d_tables) (void)hipFree(h->d_tables);
    if (h->d_range_flag) (void)hipFree(h->d_range_flag);
    bd::resample_release(h);
    if (h->d_amax) (void)hipFree(h->d_amax);
    bd::headset_free(&h->set);
    bd::ensemble_free(&h->ens);
    delete h;
    return BD_OK;
}

int bd_set_group_windows(bd_handle h, int32_t windows) {
    if (!h || windows < 0 || windows > kMaxGroup) return fail(BD_EINVAL, "bd_set_group_windows: windows must be in 0..65536");
    h->group_windows = windows == 0 ? kDefaultGroup : windows;
    return BD_OK;
}

int bd_set_pointwise_variant(bd_handle h, int32_t layer, int32_t variant) {
    if (!h || layer < 2 || layer > 14) return fail(BD_EINVAL, "bd_set_pointwise_variant: layer must be 2..14");
    if (h->sep[layer - 2].pw_mode != 0) h->sep[layer - 2].pw_variant16 = variant;
    else h->sep[layer - 2].pw_variant = variant;
    return BD_OK;
}

int bd_set_fusion(bd_handle h, int32_t stem, int32_t separable) {
    if (!h) return fail(BD_EINVAL, "null handle");
    // (removed in round 6 and refused like any unknown code: stem 2 = layers 1-2 + depthwise 3 only, 4 = the walk of stemroll.hip;
    //  separable 2 = layer 4 as band tiles, 3 = one launch per layer for layers 8-11, 4 / 5 = layer 12 / 14 on the 8-wave kernel,
    //  6 = one exact-f32 kernel per separable layer, 7 = the round-3 run of layers 8-11 through global memory + layer 12 / 14 on the
    //  12-wave kernel, 8 = the on-chip run ending at layer 11, 9 / 12 = plain fused layers)
    if (stem != 0 && stem != 3 && stem != 5) return fail(BD_EINVAL, "bd_set_fusion: stem must be 0, 3 or 5");
    if (separable != 0 && separable != 1 && separable != 10)
        return fail(BD_EINVAL, "bd_set_fusion: separable must be 0, 1 or 10");
    h->stem = stem;
    h->separable = separable;
    return BD_OK;
}

int bd_set_pointwise_mode(bd_handle h, int32_t mode) {
    if (!h || mode < 0 || mode > 2)
        return fail(BD_EINVAL, "bd_set_pointwise_mode: mode must be 0 (f32), 1 (split f16) or 2 (plain f16)");
    h->pointwise_mode = mode;
    for (auto& L : h->sep) L.pw_mode = mode;
    return BD_OK;
}

int bd_range_flag(bd_handle h, int32_t* flag_host, int32_t reset, void* stream) {
    if (!h || !flag_host) return fail(BD_EINVAL, "bd_range_flag: null argument");
    BD_HIP(hipSetDevice(h->device));
    unsigned v = 0;
    BD_HIP(hipMemcpyAsync(&v, h->d_range_flag, sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)stream));
    BD_HIP(hipStreamSynchronize((hipStream_t)stream));
    if (reset && v) BD_HIP(hipMemsetAsync(h->d_range_flag, 0, sizeof(v), (hipStream_t)stream));
    *flag_host = (int32_t)v;
    return BD_OK;
}

int bd_range_flag_copy(bd_handle h, int32_t* dst, int32_t reset, void* stream) {
    if (!h || !dst) return fail(BD_EINVAL, "bd_range_flag_copy: null argument");
    BD_HIP(hipSetDevice(h->device));
    BD_HIP(hipMemcpyAsync(dst, h->d_range_flag, sizeof(int32_t), hipMemcpyDefault, (hipStream_t)stream));
    if (reset) BD_HIP(hipMemsetAsync(h->d_range_flag, 0, sizeof(int32_t), (hipStream_t)stream));
    return BD_OK;
}

int bd_profile_enable(bd_handle h, int32_t on) {
    if (!h) return fail(BD_EINVAL, "null handle");
    h->profiling = on != 0;
    return BD_OK;
}

int bd_profile_read(bd_handle h, double* ms, int64_t* launches, int32_t slots) {
    if (!h || !ms || !launches || slots < BD_PROFILE_SLOTS) return fail(BD_EINVAL, "bd_profile_read: bad argument");
    BD_HIP(hipSetDevice(h->device));
    for (size_t i = 0; i < h->pending.size(); ++i) {
        const bd::Event2& ev = h->pending[i];
        BD_HIP(hipEventSynchronize(ev.ev));
        if (ev.slot >= 0 && i > 0) {
            float t = 0.f;
            BD_HIP(hipEventElapsedTime(&t, h->pending[i - 1].ev, ev.ev));
            h->ms[ev.slot] += t;
            h->launches[ev.slot] += 1;
        }
    }
    for (auto& ev : h->pending) h->free_events.push_back(ev);
    h->pending.clear();
    for (int i = 0; i < BD_PROFILE_SLOTS; ++i) {
        ms[i] = h->ms[i];
        launches[i] = h->launches[i];
        h->ms[i] = 0;
        h->launches[i] = 0;
    }
    return BD_PROFILE_SLOTS;
}

}  // extern "C"
