// The engine handle (struct bd_engine) and what every host file that works on one shares: the layer table and buffer sizes,
// framing arithmetic, the profiling launch wrapper, and the functions the host files call across each other.  Host code only.
//   engine.hip          error state, framing exports, bd_create / bd_destroy, setters, range flag, profile
//   weights_fold.hip    BatchNorm folding and the layout of the weight pool (no HIP runtime call)
//   engine_pass.hip     the launch plan of a batch of chunks, calibration, workspace layout
//   resample_host.hip   filter design and the resampler's filter caches
//   headmlp.hip / headset.hip / ensemble.hip    attach and query exports of the three head kinds; a lone stack and a set run
//                       on headset.hip's kernels
#pragma once

#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "bd_internal.h"
#include "bd_error.h"

using bd::fail;

// (stride, filters): embedders/yamnet/yamnet.py:77-93
const int kLayerDefs[14][2] = {{2, 32},  {1, 64},  {2, 128}, {1, 128}, {2, 256}, {1, 256},  {2, 512},
                               {1, 512}, {1, 512}, {1, 512}, {1, 512}, {1, 512}, {2, 1024}, {1, 1024}};

constexpr int64_t kFloatsA = 98304;   // largest activation per window held in buffer A (layer 2 output 48x32x64)
constexpr int64_t kFloatsB = 49152;   // largest per window in buffer B (layer-2 depthwise output 48x32x32)
constexpr int kDefaultGroup = 1024;
// The largest pass bd_set_group_windows accepts: the size tests/test_pass_size.py runs every launch set at.  Its buffer A
// is 25.8 GB, so every activation tensor of a pass crosses 2^31 and 2^32 bytes below it.
constexpr int kMaxGroup = 65536;
// septail.hip's kernels take 32-bit byte offsets: up to 2^18 windows (split-f16 planes), 2^17 (exact f32)
static_assert(kMaxGroup <= 1 << 17, "the tail launchers of pass_f16 / pass_f32 cover the largest pass");
static_assert(bd::kDw7PlaneBytes <= kFloatsA * 4, "the depthwise-7 planes of the middle run fit buffer a");

namespace bd {

// One event is recorded after every launch; the time between consecutive events on the stream is
// charged to the later one's slot (slot < 0 = the marker at the head of a call).  Event pairs around
// each launch leave the gaps between pairs unattributed, and on this stack they under-read some
// kernels by tens of microseconds against rocprofv3.
struct Event2 {
    hipEvent_t ev;
    int slot;
};

// The filters of the resampler, kept on the device until bd_destroy (resample_host.hip).  An entry owns a device block, the
// host source of its asynchronous upload, the stream it was uploaded on and the event recorded behind that copy.  The first
// use uploads in the caller's stream order; a launch on any OTHER stream first waits for `uploaded`.  There are at most 64
// entries and they never move (uploads read from them); nothing is freed or re-uploaded on a rate change: hipFree would
// synchronise the device under the caller's streams.  Key is what tells the filters apart and what their launch needs.
template <class Key>
struct FilterCache {
    struct Entry : Key {
        float* dev = nullptr;
        std::vector<float> host;
        hipStream_t upload_stream = nullptr;
        hipEvent_t uploaded = nullptr;
    };
    std::vector<Entry> entries;

    bool full() const { return entries.size() >= 64; }
    // First use: allocates t's block, keeps t and uploads it in the order of `stream`.  *filt is the kept entry as soon as
    // there is one, whatever comes back; a failure before that leaves nothing behind.
    int upload(Entry&& t, void* stream, const char* who, Entry** filt);
    int order_behind_upload(const Entry* filt, void* stream) const;    // a later use: waits where the stream is another
    void release();                                                    // bd_destroy
};

struct TapsKey {
    int up, down, quality, half;
    // The block: the taps as float32 (the vector kernels), then, 16-byte aligned, the matrix-core plan's fragment-ordered
    // filter and its two index tables (bd::FirPlan points into it)
    bool has_plan;                    // the ratio fits fir_mfma_kernel (resample.hip)
    FirPlanHost fir;
};
// the coefficient rows of the ratios those plans do not cover (anyrate.hip)
struct AnyTapsKey {
    AnyratePlan plan;
    int quality;
};

// ---- weights_fold.hip ----
// Where one separable layer's tensors lie in the folded image, in floats (each a multiple of 64; the fields of SepLayer)
struct LayerOffsets {
    size_t dw_w, dw_b, pw_w, pw_b;    // folded f32: [9][cin], [cin], [cout][cin], [cout]
    size_t pw_hi, pw_lo;              // [cout][cin] f16 halves of the row-scaled pointwise kernel
    size_t dw16, pw_u;                // [10][cin] and [cout]: left zero, apply_scales fills them on the device
    size_t pw_fhi, pw_flo;            // the halves in MFMA fragment order
    size_t pw_ffrag;                  // the f32 kernel in fragment order; 0 = none (cin < 128)
    std::vector<int> row_exp;         // [cout]: power-of-two exponent the pointwise row was scaled by before its f16 split
};
struct FoldedWeights {
    std::vector<float> image;         // the weight pool as it is uploaded
    size_t conv1_w = 0, conv1_b = 0;  // [9][32], [32]
    LayerOffsets layer[13];
    size_t head_w = 0, head_b = 0;    // [n_classes][1024], [BD_MAX_CLASSES]; n_classes > 0 only
    FeTables tables;
};
// Folds BatchNorm into the embedder blob, lays every tensor out and builds the front end's tables.  BD_OK, or BD_EWEIGHTS
// with the error text set.  Host arithmetic only: nothing here touches the device.
int fold_weights(const bd_weights& w, FoldedWeights* out);

}  // namespace bd

struct bd_engine {
    int device = 0;
    int n_classes = 0;
    int group_windows = kDefaultGroup;
    int pointwise_mode = 1;           // 0 = exact f32 MFMA, 1 = split-f16 MFMA, 2 = plain f16 MFMA
    unsigned* d_range_flag = nullptr; // sticky: an activation exceeded the f16 range in mode 1 / 2 (bd_range_flag)
    int stem = 3, separable = 1;      // bd_set_fusion codes (pass_f16 / pass_f32 read them)
    float* d_pool = nullptr;          // one allocation for every folded tensor
    bd::FeTables* d_tables = nullptr;
    // operand scaling of the f16 modes (bd_internal.h, SepLayer): host copies of what the scaled tensors are made from
    std::vector<float> h_dw[13];      // [10][cin]: folded depthwise taps, then the shift (unscaled)
    std::vector<int> row_exp[13];     // [cout]: LayerOffsets::row_exp
    size_t off_dw16[13] = {0}, off_pw_u[13] = {0};   // float offsets of dw_w16 (dw_b16 follows at + 9 cin) / pw_u in d_pool
    float act_max[13] = {0};          // largest depthwise output seen by the calibration passes (exact-f32 arithmetic)
    int act_exp[13] = {0};
    unsigned* d_amax = nullptr;       // [16] calibration words
    const float* conv1_w = nullptr;   // [9][32]
    const float* conv1_b = nullptr;   // [32]
    bd::SepLayer sep[13];
    const float* head_wt = nullptr;   // [n_classes][1024]
    const float* head_b = nullptr;
    // heads attached in place of that head (headset.hip; set.dev != nullptr): a lone dense stack (bd_head_attach, set.lone) or
    // a set of heads (bd_headset_attach) - n_classes is then the sum of the members' last widths
    bd::HeadSet set;
    // and outputs over that set's members (bd_ensemble_attach, ensemble.hip): n_classes is then the sum of the outputs' widths
    bd::Ensemble ens;
    // resampler: the filters of every (up, down) pair used so far
    bd::FilterCache<bd::TapsKey> taps;
    bd::FilterCache<bd::AnyTapsKey> any_taps;
    int resample_quality = BD_RESAMPLE_HQ;
    // profiling
    bool profiling = false;
    std::vector<bd::Event2> pending;
    std::vector<bd::Event2> free_events;
    double ms[BD_PROFILE_SLOTS] = {0};
    int64_t launches[BD_PROFILE_SLOTS] = {0};
};

namespace bd {

// ---- engine_pass.hip ----
// Rebuilds the scaled depthwise copies and the epilogue factors from e->act_exp.  Blocking copies into the pool: only
// call it while no work that uses the handle is in flight (bd_create, bd_calibrate, bd_set_activation_exponents).
int apply_scales(bd_engine* e);
int calibrate_builtin(bd_engine* e);        // bd_create: the activation scales from the built-in signal

// ---- resample_host.hip ----
void resample_release(bd_engine* e);        // bd_destroy: both filter caches

}  // namespace bd

namespace {

inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

// Records the marker event of one launch (or, with slot < 0, the head marker of a call).
void mark(bd_engine* e, hipStream_t s, int slot) {
    bd::Event2 ev;
    if (!e->free_events.empty()) {
        ev = e->free_events.back();
        e->free_events.pop_back();
    } else if (hipEventCreate(&ev.ev) != hipSuccess) {
        return;
    }
    ev.slot = slot;
    (void)hipEventRecord(ev.ev, s);
    e->pending.push_back(ev);
}

// Developer build (-DBD_KERNEL_TRACE) only: BD_REPEAT_SLOT=<profile slot> BD_REPEAT_N=<n> launches that slot's kernel n times
// per pass (same operands: the kernels are idempotent), so that one kernel dominates a run - its sustained clock and the
// board power it draws alone can then be read from hwmon (tools/power_profile.py).  The shipped library reads no environment.
#ifdef BD_KERNEL_TRACE
static int repeat_of(int slot) {
    static const int want = getenv("BD_REPEAT_SLOT") ? atoi(getenv("BD_REPEAT_SLOT")) : -1;
    static const int n = getenv("BD_REPEAT_N") ? atoi(getenv("BD_REPEAT_N")) : 1;
    return slot == want ? n : 1;
}
#endif

// One launch timed in profile `slot`: fn() launches the kernel (a launcher that returns false or 0 declined: nothing ran,
// nothing is recorded and launch returns false), the developer build repeats it, and with profiling on the slot's marker
// event follows it.
template <class F>
bool launch(bd_engine* e, hipStream_t s, int slot, F fn) {
    if constexpr (std::is_void_v<decltype(fn())>) fn();
    else if (!fn()) return false;
#ifdef BD_KERNEL_TRACE
    for (int r = repeat_of(slot); r > 1; --r) (void)fn();
#endif
    if (e->profiling) mark(e, s, slot);
    return true;
}

// ---- index arithmetic: embedders/yamnet/features.py:82-108, :42-46, :65-76 ----
int64_t padded_length(int64_t n, int32_t hop) {
    const int64_t min_samples = BD_MIN_SAMPLES;
    int64_t pad = min_samples - n > 0 ? min_samples - n : 0;
    const int64_t num = n > min_samples ? n : min_samples;
    const int64_t after = num - min_samples;
    // tf.cast(tf.math.ceil(tf.cast(after, f32) / tf.cast(hop, f32)), int32): float32 on purpose
    const volatile float q = (float)after / (float)hop;
    const int64_t hops = (int64_t)ceilf(q);
    pad += (int64_t)hop * hops - after;
    return n + pad;
}

struct Geometry {
    int64_t n_padded, n_frames, n_windows;
};

int geometry(int64_t n, int32_t hop, int32_t step, Geometry* g) {
    if (n < 0) return fail(BD_EINVAL, "n_samples must be >= 0");
    if (hop <= 0) return fail(BD_EINVAL, "hop_samples must be > 0");
    if (n >= (1LL << 24))
        return fail(BD_ERANGE,
                    "chunk of 2^24 samples or more: the float32 ceil in pad_waveform (features.py:100-102) is "
                    "no longer exact; split the chunk");
    g->n_padded = padded_length(n, hop);
    if (g->n_padded < n) return fail(BD_ERANGE, "pad_waveform would need negative padding");
    g->n_frames = g->n_padded >= BD_STFT_WINDOW ? 1 + (g->n_padded - BD_STFT_WINDOW) / BD_STFT_HOP : 0;
    if (step > 0)
        g->n_windows = g->n_frames >= BD_PATCH_FRAMES ? 1 + (g->n_frames - BD_PATCH_FRAMES) / step : 0;
    else
        g->n_windows = 0;
    return BD_OK;
}

}  // namespace
