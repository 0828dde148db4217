// Weight preparation of bd_create as a host function: the embedder blob with BatchNorm folded in, every tensor in every form
// the kernels read it in, laid out in one image that is uploaded as it stands, and the front end's constant tables.
// Host arithmetic only: no HIP runtime call, so it runs (and can be checked) without a device.
#include <cmath>
#include <cstring>

#include "engine_state.h"

namespace bd {
namespace {

struct BnFold {
    std::vector<double> scale, shift;
};

BnFold fold_bn(const float* beta, const float* mean, const float* var, int c) {
    // keras BatchNormalization inference with scale=False: (x - mean) * rsqrt(var + eps) + beta
    BnFold f;
    f.scale.resize(c);
    f.shift.resize(c);
    for (int i = 0; i < c; ++i) {
        const double s = 1.0 / std::sqrt((double)var[i] + 1e-4);
        f.scale[i] = s;
        f.shift[i] = (double)beta[i] - (double)mean[i] * s;
    }
    return f;
}

int build_tables(const float* mel, FeTables* t) {
    std::memset(t, 0, sizeof(*t));
    // tf.signal.hann_window(400, periodic=True, dtype=float32): float32 arithmetic throughout
    for (int k = 0; k < BD_STFT_WINDOW; ++k) {
        const float arg = (float)(2.0 * M_PI) * (float)k / (float)BD_STFT_WINDOW;
        t->hann[k] = 0.5f - 0.5f * (float)std::cos((double)arg);
    }
    for (int k = 0; k < 256; ++k) {
        const double a = -2.0 * M_PI * k / 256.0;
        t->tw256[k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    for (int k = 0; k <= BD_SPECTRUM_BINS; ++k) {
        const double a = -2.0 * M_PI * k / 512.0;
        t->tw512[k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    for (int m = 0; m < BD_MEL_BANDS; ++m) {
        const int first = kMelStart[m], len = kMelLen[m];
        for (int k = 0; k < BD_SPECTRUM_BINS; ++k) {
            const float w = mel[k * BD_MEL_BANDS + m];
            if (!std::isfinite(w)) return fail(BD_EWEIGHTS, "mel matrix has a non-finite entry");
            if (w != 0.0f && (k < first || k >= first + len))
                return fail(BD_EWEIGHTS, "mel matrix has a non-zero outside the 64-band YAMNet filterbank pattern "
                                         "(linear_to_mel_weight_matrix(64, 257, 16000, 125, 7500)); not a YAMNet front end");
        }
        for (int j = 0; j < len; ++j) t->melw[mel_offset(m) + j] = mel[(first + j) * BD_MEL_BANDS + m];
    }
    return BD_OK;
}

bool all_finite(const float* v, size_t n) {
    bool finite = true;
    for (size_t i = 0; i < n; ++i) finite = finite && std::isfinite(v[i]);
    return finite;
}

// the pointwise kernel goes on into the row scaling of the f16 split: it has always been held below 3.0e38, not FLT_MAX
bool all_splittable(const float* v, size_t n) {
    bool ok = true;
    for (size_t i = 0; i < n; ++i) ok = ok && std::fabs(v[i]) <= 3.0e38f;
    return ok;
}

}  // namespace

int fold_weights(const bd_weights& w, FoldedWeights* out) {
    // ---- fold + lay out every tensor in one host staging buffer ----
    std::vector<float>& host = out->image;
    host.clear();
    host.reserve(BD_EMBEDDER_BLOB_FLOATS + 64 * 1024);
    auto reserve = [&](size_t n) {
        const size_t off = (host.size() + 63) / 64 * 64;
        host.resize(off + n, 0.0f);
        return off;
    };
    const float* p = w.embedder_blob;
    bool finite;
    {
        const int c = kLayerDefs[0][1];
        const float* kern = p;   // [3][3][1][32]
        const BnFold f = fold_bn(p + 9 * c, p + 10 * c, p + 11 * c, c);
        p += 12 * c;
        out->conv1_w = reserve(9 * c);
        out->conv1_b = reserve(c);
        for (int t = 0; t < 9; ++t)
            for (int i = 0; i < c; ++i) host[out->conv1_w + t * c + i] = (float)((double)kern[t * c + i] * f.scale[i]);
        for (int i = 0; i < c; ++i) host[out->conv1_b + i] = (float)f.shift[i];
        finite = all_finite(host.data() + out->conv1_w, 9 * c) && all_finite(host.data() + out->conv1_b, c);
    }
    int cin = kLayerDefs[0][1];
    for (int l = 0; l < 13; ++l) {
        LayerOffsets& o = out->layer[l];
        const int cout = kLayerDefs[l + 1][1];
        const float* dw = p;   // [3][3][cin][1]
        const BnFold fd = fold_bn(p + 9 * cin, p + 10 * cin, p + 11 * cin, cin);
        p += 12 * (size_t)cin;
        const float* pw = p;   // [1][1][cin][cout]
        p += (size_t)cin * cout;
        const BnFold fp = fold_bn(p, p + cout, p + 2 * cout, cout);
        p += 3 * (size_t)cout;
        const size_t nw = (size_t)cin * cout;
        o.dw_w = reserve(9 * (size_t)cin);
        o.dw_b = reserve(cin);
        o.pw_w = reserve(nw);
        o.pw_b = reserve(cout);
        for (int t = 0; t < 9; ++t)
            for (int i = 0; i < cin; ++i)
                host[o.dw_w + (size_t)t * cin + i] = (float)((double)dw[(size_t)t * cin + i] * fd.scale[i]);
        for (int i = 0; i < cin; ++i) host[o.dw_b + i] = (float)fd.shift[i];
        for (int n = 0; n < cout; ++n)
            for (int k = 0; k < cin; ++k)
                host[o.pw_w + (size_t)n * cin + k] = (float)((double)pw[(size_t)k * cout + n] * fp.scale[n]);
        for (int n = 0; n < cout; ++n) host[o.pw_b + n] = (float)fp.shift[n];
        // the one finite check, on the folded f32 tensors (conv1's with layer 2's): nothing below it runs on a value that is
        // not a number, and bd_create has allocated nothing on the device yet
        finite = finite && all_finite(host.data() + o.dw_w, 9 * (size_t)cin) && all_finite(host.data() + o.dw_b, cin) &&
                 all_splittable(host.data() + o.pw_w, nw) && all_finite(host.data() + o.pw_b, cout);
        if (!finite) return fail(BD_EWEIGHTS, "bd_create: non-finite value after BatchNorm folding");
        // split-f16 copy of the folded pointwise kernel.  Every output channel (row of W^T) is first multiplied by the
        // power of two that puts its largest magnitude into [2^12, 2^13): then hi = f16(w) and lo = f16(w - hi) are both
        // NORMAL f16 numbers for every weight within 2^-15 of the row's largest, i.e. w = hi + lo to 22 bits whatever the
        // scale BatchNorm folding left the row at (unscaled, lo is subnormal - absolute quantum 2^-24 - below |w| = 0.125).
        // The epilogue multiplies the accumulator by the inverse power of two (SepLayer::pw_u): nothing is rounded.
        o.pw_hi = reserve((nw + 1) / 2);
        o.pw_lo = reserve((nw + 1) / 2);
        o.row_exp.assign(cout, 0);
        {
            _Float16* hi = reinterpret_cast<_Float16*>(host.data() + o.pw_hi);
            _Float16* lo = reinterpret_cast<_Float16*>(host.data() + o.pw_lo);
            const float* wf = host.data() + o.pw_w;
            for (int n = 0; n < cout; ++n) {
                float wmax = 0.0f;
                for (int k = 0; k < cin; ++k) {
                    const float a = std::fabs(wf[(size_t)n * cin + k]);
                    wmax = a > wmax ? a : wmax;
                }
                int ex = 0;
                if (wmax > 0.0f) {
                    (void)std::frexp(wmax, &ex);                  // wmax = m 2^ex, 0.5 <= m < 1
                    ex = 13 - ex;
                    ex = ex > 60 ? 60 : (ex < -60 ? -60 : ex);
                }
                o.row_exp[n] = ex;
                for (int k = 0; k < cin; ++k) {
                    const float w = std::ldexp(wf[(size_t)n * cin + k], ex);
                    const _Float16 h = (_Float16)w;
                    hi[(size_t)n * cin + k] = h;
                    lo[(size_t)n * cin + k] = (_Float16)(w - (float)h);
                }
            }
        }
        o.dw16 = reserve(10 * (size_t)cin);
        o.pw_u = reserve(cout);
        // the same halves in MFMA fragment order (v_mfma_f32_32x32x16_f16 B operand): for a 32-channel tile t
        // and a 16-deep k step q, lane l holds W[32 t + l % 32][16 q + 8 (l / 32) .. + 8], so a wave's fragment
        // load is 1 KiB contiguous:  frag[((t * K/16 + q) * 64 + l) * 8 + e]
        o.pw_fhi = reserve((nw + 1) / 2);
        o.pw_flo = reserve((nw + 1) / 2);
        {
            const _Float16* hi = reinterpret_cast<const _Float16*>(host.data() + o.pw_hi);
            const _Float16* lo = reinterpret_cast<const _Float16*>(host.data() + o.pw_lo);
            _Float16* fhi = reinterpret_cast<_Float16*>(host.data() + o.pw_fhi);
            _Float16* flo = reinterpret_cast<_Float16*>(host.data() + o.pw_flo);
            const int kq = cin / 16;
            for (int n = 0; n < cout; ++n)
                for (int k = 0; k < cin; ++k) {
                    const int lane = (n & 31) + 32 * ((k & 15) >> 3);
                    const size_t dst = (((size_t)(n >> 5) * kq + (k >> 4)) * 64 + lane) * 8 + (k & 7);
                    fhi[dst] = hi[(size_t)n * cin + k];
                    flo[dst] = lo[(size_t)n * cin + k];
                }
        }
        // the f32 kernel in the fragment order of v_mfma_f32_32x32x2_f32 as the exact-f32 on-chip run reads it (sepchipf32.hip):
        // for a 32-channel tile t and a super-step S of 8 k, lane l holds W[32 t + l % 32][8 S + 4 (l / 32) .. + 4]
        o.pw_ffrag = 0;
        if (cin >= 128) {                                          // layers 5-14: what the exact-f32 on-chip runs and the tail kernel cover (12 MB)
            o.pw_ffrag = reserve(nw);
            const float* wf = host.data() + o.pw_w;
            float* ff = host.data() + o.pw_ffrag;
            const int ks = cin / 8;
            for (int n = 0; n < cout; ++n)
                for (int k = 0; k < cin; ++k) {
                    const int lane = (n & 31) + 32 * ((k & 7) >> 2);
                    ff[(((size_t)(n >> 5) * ks + (k >> 3)) * 64 + lane) * 4 + (k & 3)] = wf[(size_t)n * cin + k];
                }
        }
        cin = cout;
    }
    if (p - w.embedder_blob != BD_EMBEDDER_BLOB_FLOATS) return fail(BD_EWEIGHTS, "internal: blob walk mismatch");
    out->head_w = out->head_b = 0;
    if (w.n_classes > 0) {
        out->head_w = reserve((size_t)w.n_classes * BD_EMBEDDING_SIZE);
        out->head_b = reserve(BD_MAX_CLASSES);
        for (int c = 0; c < w.n_classes; ++c)
            for (int k = 0; k < BD_EMBEDDING_SIZE; ++k)
                host[out->head_w + (size_t)c * BD_EMBEDDING_SIZE + k] = w.head_kernel[(size_t)k * w.n_classes + c];
        for (int c = 0; c < w.n_classes; ++c) host[out->head_b + c] = w.head_bias[c];
    }
    return build_tables(w.mel, &out->tables);
}

}  // namespace bd
