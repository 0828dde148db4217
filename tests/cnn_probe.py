"""A second set of embedder weights with no channel dead or saturated, and per-channel error bookkeeping.

With the seeded stand-in weights (``weights.synthetic_embedder_blob``) 66-159 of the 1024 channels of CNN stages 23-26
never leave zero and most of the others never reach it ("Per-channel CNN parity on weights that leave no
channel dead"): a kernel that read the wrong weight row, bias or scale for such a channel writes the same zeros as a
right one.  ``live_blob`` re-centres every BatchNorm channel whose output is on for less than a quarter or more than three
quarters of the positions of one fixed signal, so that every channel of every stage crosses the ReLU edge about half the
time.  Plain helpers for tests/test_cnn_channels.py (CPU) and tests/test_cnn_channels_gpu.py; no fixtures, no GPU.
"""
import hashlib
import json
import os

import numpy as np

from oracle import yamnet_oracle as O

HOP, STEP = 15360, 96
N_STAGES = 27
LIVE_LO, LIVE_HI = 0.25, 0.75            # a channel whose fraction of positive pre-activations lies outside is re-centred
TOL_ABS = 1e-4                           # the suite's absolute gate on activations and logits (tests/test_gpu_parity.py)

_MANIFEST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "buzzdetect_amd", "data",
                         "embedder_manifest.json")
_cache = {}


def centring_signal():
    """The 8-window signal the BatchNorm shifts are centred on."""
    return O.synthetic_audio(HOP * 7 + 15600, seed=11)


def held_out_signal():
    """5 windows of the same kind of audio as the centring signal, from another seed."""
    return O.synthetic_audio(HOP * 4 + 15600, seed=78)


def noise_signal():
    """8 windows of white noise at 0.15: no tone bursts, a flat spectrum above the synthetic audio's noise floor."""
    rng = np.random.default_rng(1)
    return np.clip(0.15 * rng.standard_normal(HOP * 7 + 15600), -1.0, 1.0 - 2.0 ** -23).astype(np.float32)


def fused_signal(windows=65):
    """The first ``windows`` windows of one 65-window signal.  Window w reads samples [w*HOP, w*HOP + 15600) only, so the
    windows of a prefix are the first windows of the whole signal, bit for bit."""
    return O.synthetic_audio(HOP * 64 + 15600, seed=6500)[:HOP * (windows - 1) + 15600]


ONE_WINDOW_INPUTS = 5        # one 3x2 map cannot switch 1024 channels on: the one-window case is this many one-window inputs


def one_window_input(w):
    """Window ``w`` of the fused signal as an input of its own."""
    return fused_signal(65)[HOP * w:HOP * w + 15600]


def patches_of(x, mel, dtype=np.float64):
    return O.frame_patches(O.log_mel(O.pad_waveform(np.asarray(x, np.float32), HOP), mel, dtype), STEP)


def oracle_taps(x, blob, mel, dtype=np.float64):
    """(27 NHWC stage outputs, [W,1024] embeddings) of the CPU oracle in ``dtype``."""
    taps = []
    emb = O.yamnet_body(patches_of(x, mel, dtype), blob, dtype, taps)
    assert len(taps) == N_STAGES
    return taps, emb


def bn_of_stage(stage):
    """k of the BatchNorm ``layer_with_weights-k`` whose output is CNN stage ``stage`` (0..26)."""
    return 2 * stage + 1


def blob_views(blob):
    """name -> writable view into ``blob`` (the reference layout, buzzdetect_amd/data/embedder_manifest.json)."""
    with open(_MANIFEST) as f:
        tensors = json.load(f)["tensors"]
    out = {}
    for t in tensors:
        off, n = t["offset"] // 4, t["size"] // 4
        out[t["name"]] = blob[off:off + n].reshape(t["shape"])
    return out


def _recentre(pre, t, k):
    """BatchNorm ``k`` + ReLU in float64 on the pre-activations ``pre``; before that, the beta of every channel that would
    be on for a fraction of the positions outside [LIVE_LO, LIVE_HI] becomes minus the channel's median normalised
    pre-activation (rounded to float32, which is what the layers behind it are then fed with)."""
    p = f"layer_with_weights-{k}/"
    beta, mean, var = t[p + "beta"], t[p + "moving_mean"], t[p + "moving_variance"]
    c = pre.shape[-1]
    inv = np.float64(1.0) / np.sqrt(var.astype(np.float64) + np.float64(O.BN_EPS))       # the very expression of O._bn_relu,
    z = ((pre - mean.astype(np.float64)) * inv).reshape(-1, c)                            # so z + beta > 0 is its output > 0

    def outside(b):
        on = (z + b.astype(np.float64) > 0).mean(axis=0)
        return (on < LIVE_LO) | (on > LIVE_HI)

    off_centre = outside(beta)
    beta[off_centre] = (-np.median(z, axis=0)[off_centre]).astype(np.float32)
    # Many positions of a channel can share one pre-activation exactly (a depthwise window that saw only zeros): when the
    # median is such a value, the float32 rounding of beta switches all of them on or all of them off.  Those few channels
    # take the midpoint to the next distinct value below or above the median instead, whichever lands nearer to one half.
    for c in np.flatnonzero(outside(beta)):
        v = np.unique(z[:, c])
        m = np.median(z[:, c])
        below, above = v[v < m], v[v > m]
        cands = [np.float32(-(m + w[i]) / 2) for w, i in ((below, -1), (above, 0)) if w.size]
        beta[c] = min(cands, key=lambda b: abs((z[:, c] + np.float64(b) > 0).mean() - 0.5))
    assert not outside(beta).any(), f"BatchNorm {k}: a channel cannot be centred on this signal"
    return O._bn_relu(pre, beta, mean, var, np.float64)


def live_blob(base_blob, mel):
    """``base_blob`` with the BatchNorm ``beta`` of every nearly-dead or nearly-always-on channel re-centred on
    ``centring_signal()``: the layers are walked in float64 with the oracle's own operators, each fed by the layers
    already re-centred.  Kernels, means and variances are untouched.  Deterministic; cached per (blob, mel)."""
    base_blob = np.ascontiguousarray(base_blob, dtype=np.float32)
    key = (hashlib.sha256(base_blob.tobytes()).hexdigest(), hashlib.sha256(np.ascontiguousarray(mel).tobytes()).hexdigest())
    if key not in _cache:
        blob = base_blob.copy()
        t = blob_views(blob)
        x = patches_of(centring_signal(), mel)[..., None]
        x = _recentre(O.conv3x3_full(x, t["layer_with_weights-0/kernel"], O.LAYER_DEFS[0][0], np.float64), t, 1)
        k = 2
        for stride, _ in O.LAYER_DEFS[1:]:
            x = _recentre(O.depthwise3x3(x, t[f"layer_with_weights-{k}/depthwise_kernel"], stride, np.float64), t, k + 1)
            x = _recentre(O.pointwise(x, t[f"layer_with_weights-{k + 2}/kernel"], np.float64), t, k + 3)
            k += 4
        blob.setflags(write=False)
        _cache[key] = blob
    return _cache[key]


def channel_report(taps):
    """Per stage: (fraction of windows x positions at which each channel is nonzero, each channel's maximum)."""
    out = []
    for a in taps:
        a = np.asarray(a).reshape(-1, a.shape[-1])
        out.append(((a > 0).mean(axis=0), a.max(axis=0)))
    return out


def channel_errors(got, ref, where=None):
    """Per stage: (each channel's max |got - ref| over windows and positions, each channel's max |ref|).  ``where``: an
    optional [H, W] mask per stage (None = every position) that restricts both to some positions of the map."""
    out = []
    for s, (g, r) in enumerate(zip(got, ref)):
        g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
        assert g.shape == r.shape, (s, g.shape, r.shape)
        if where is not None and where[s] is not None:
            g, r = g[:, where[s]], r[:, where[s]]
        c = r.shape[-1]
        out.append((np.abs(g - r).reshape(-1, c).max(axis=0), np.abs(r).reshape(-1, c).max(axis=0)))
    return out


def border_mask(h, w):
    """True on the first and last row and column of an [h, w] map."""
    m = np.zeros((h, w), dtype=bool)
    m[0, :] = m[-1, :] = True
    m[:, 0] = m[:, -1] = True
    return m


# --------------------------------------------------------------------------- the per-channel rule
# err_gpu(c) <= min(TOL_ABS, max(K * err_f32oracle(c), F(stage) * max|ref_c|)), where err_f32oracle is the float32 CPU
# oracle's own distance from the float64 oracle for that channel.  K and F: DESIGN.md, same subsection.
K_ORACLE = 16.0                          # smallest power of two with 2x headroom over the worst measured ratio, 7.51
F_LAYER = 1.5e-6                         # the pointwise GEMM's per-output budget (test_pointwise_gemm_every_tile_variant)


def floor_factor(stage):
    """F of the rule: the pointwise test's 1.5e-6 per layer, times the number of layers up to and including ``stage``."""
    return F_LAYER * (stage + 1)


def channel_bound(stage, err_oracle, ref_max):
    return np.minimum(TOL_ABS, np.maximum(K_ORACLE * err_oracle, floor_factor(stage) * ref_max))


def worst_position(got, ref, channel, where=None):
    """(window, row, column, on_border) of the largest |got - ref| of one channel of one stage."""
    d = np.abs(np.asarray(got, np.float64)[..., channel] - np.asarray(ref, np.float64)[..., channel])
    if where is not None:
        d = np.where(where[None], d, -1.0)
    n, i, j = np.unravel_index(int(np.argmax(d)), d.shape)
    return int(n), int(i), int(j), bool(border_mask(*d.shape[1:])[i, j])


def check_channels(got, ref, ref32, what, where=None):
    """The rule on every channel of every stage.  Returns (per stage: the worst err_gpu / err_f32oracle over all channels
    and over the channels whose error is above the floor F * max|ref|; one line per stage that misses, naming stage, worst
    channel and worst position)."""
    e_gpu = channel_errors(got, ref, where)
    e_cpu = channel_errors(ref32, ref, where)
    ratios, misses = [], []
    for s, ((eg, rmax), (ec, _)) in enumerate(zip(e_gpu, e_cpu)):
        r = np.divide(eg, ec, out=np.zeros_like(eg), where=ec > 0)
        above = eg > floor_factor(s) * rmax
        ratios.append((float(r.max()), float(r[above].max()) if above.any() else 0.0))
        bound = channel_bound(s, ec, rmax)
        bad = np.flatnonzero(eg > bound)
        if bad.size:
            c = int(bad[np.argmax(eg[bad] / bound[bad])])
            n, i, j, edge = worst_position(got[s], ref[s], c, None if where is None else where[s])
            misses.append(f"{what}: stage {s} channel {c}: err {eg[c]:.3e} > bound {bound[c]:.3e} (f32 oracle err {ec[c]:.3e}, "
                          f"max|ref| {rmax[c]:.3e}); worst at window {n} row {i} column {j} of a "
                          f"{ref[s].shape[1]}x{ref[s].shape[2]} map, {'on the border' if edge else 'interior'}; "
                          f"{bad.size} of {eg.size} channels of the stage miss")
    return ratios, misses
