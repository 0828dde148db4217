"""HIP CNN against the float64 oracle channel by channel, on weights that leave no channel dead (run on the GPU box:
``pytest -m gpu``).

The engine is built on ``cnn_probe.live_blob``: the stock stand-in weights with every BatchNorm shift centred so that each
channel of each of the 27 stages crosses the ReLU edge about half the time (tests/test_cnn_channels.py checks that with
the oracle alone).  The rule, per stage and channel c, over windows and positions:

    err_gpu(c) <= min(1e-4, max(K * err_f32oracle(c), F(stage) * max|ref_c|))

``err_f32oracle`` is the float32 CPU oracle's distance from the float64 oracle for that channel; K = 16 and
F = 1.5e-6 x (stage + 1) (cnn_probe.K_ORACLE / floor_factor; DESIGN.md, "Per-channel CNN parity on weights that leave no
channel dead", has the measured ratios behind them).
"""
import functools

import numpy as np
import pytest

import cnn_probe as P
from buzzdetect_amd import weights as W
from oracle import yamnet_oracle as O

pytestmark = pytest.mark.gpu

HOP, STEP = P.HOP, P.STEP
SIGNALS = {"held-out": P.held_out_signal, "noise": P.noise_signal}
POOL_STAGE = 27                          # the pooled embedding counts as one more layer behind stage 26


@functools.lru_cache(maxsize=None)
def _weights():
    base, mel = W.synthetic_embedder_blob(), W.load_mel("yamnet_k2")
    return P.live_blob(base, mel), mel


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(float64 taps, float64 embeddings, float32 taps, float32 embeddings) of the CPU oracle, computed once per signal."""
    live, mel = _weights()
    x = SIGNALS[name]()
    taps, emb = P.oracle_taps(x, live, mel)
    taps32, emb32 = P.oracle_taps(x, live, mel, np.float32)
    for a in taps + taps32 + [emb, emb32]:
        a.setflags(write=False)
    return taps, emb, taps32, emb32


@pytest.fixture(scope="module")
def probe_engine():
    """One engine on the probe weights for this module."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible (there is no CPU fallback)")
    from buzzdetect_amd.engine import HipEngine
    eng = HipEngine(embeddername="yamnet_k2", modelname="model_general_v3", embedder_blob=_weights()[0])
    yield eng
    eng.close()


_gpu_taps = {}


def _unfused_taps(eng, mode, name):
    """All 27 stages of one signal on the one-kernel-per-op path, once per (mode, signal)."""
    if (mode, name) not in _gpu_taps:
        x = SIGNALS[name]()
        ref = _reference(name)[0]
        try:
            eng.set_pointwise_mode(mode)
            eng.set_fusion(False, False)
            got = [eng.stage_tap(x, HOP, STEP, s, ref[s].shape[0]).cpu().numpy() for s in range(P.N_STAGES)]
        finally:
            eng.set_pointwise_mode("f16x3")
            eng.set_fusion(True, True)
        for s in range(P.N_STAGES):
            assert got[s].shape == ref[s].shape, s
        _gpu_taps[(mode, name)] = got
    return _gpu_taps[(mode, name)]


def _show(what, ratios):
    print(f"\n[ratios] {what}: worst err_gpu / err_f32oracle per stage (all channels | channels above the floor)")
    print("[ratios]   all   " + " ".join(f"{a:.2f}" for a, _ in ratios))
    print("[ratios]   above " + " ".join(f"{b:.2f}" for _, b in ratios))


@pytest.mark.parametrize("name", list(SIGNALS))
@pytest.mark.parametrize("mode", ["f32", "f16x3"])
def test_every_channel_of_every_stage_against_oracle(probe_engine, mode, name):
    ref, _, ref32, _ = _reference(name)
    got = _unfused_taps(probe_engine, mode, name)
    ratios, misses = P.check_channels(got, ref, ref32, f"{mode} {name}")
    _show(f"{mode} {name}", ratios)
    assert not misses, "\n".join(misses)


@pytest.mark.parametrize("name", list(SIGNALS))
@pytest.mark.parametrize("mode", ["f32", "f16x3"])
def test_border_and_interior_positions_apart(probe_engine, mode, name):
    """The same rule over the first and last row and column (where SAME padding cuts the 3x3 window, asymmetrically for the
    stride-2 layers) and over the rest of the map, each with the float32 oracle's error over the same positions; for the
    stages whose map is at least 6x4 (0..22), where both sets exist."""
    ref, _, ref32, _ = _reference(name)
    got = _unfused_taps(probe_engine, mode, name)
    stages = [s for s in range(P.N_STAGES) if ref[s].shape[1] >= 6 and ref[s].shape[2] >= 4]
    assert stages == list(range(23))
    misses = []
    for part in ("border", "interior"):
        masks = [P.border_mask(*ref[s].shape[1:3]) for s in stages]
        where = masks if part == "border" else [~m for m in masks]
        assert all(w.any() for w in where)
        ratios, m = P.check_channels([got[s] for s in stages], [ref[s] for s in stages], [ref32[s] for s in stages],
                                     f"{mode} {name} {part}", where)
        _show(f"{mode} {name} {part}", ratios)
        misses += m
    assert not misses, "\n".join(misses)


FUSION_SETTINGS = ((True, True), (3, False), (5, True), (False, 10))
FUSED_STAGES = (2, 4, 6, 10, 12, 14, 22, 24, 26)


@pytest.mark.parametrize("windows", [1, 5, 17, 65])
def test_fused_paths_bit_identical_on_live_channels(probe_engine, windows):
    """The assertion of the bit-identity tests of tests/test_gpu_parity.py on a network with no channel at zero: logits,
    embeddings and nine stages under every fusion setting carry the bits of one kernel per op, in all three arithmetic
    modes; one window, one more than a 4-window workgroup, than a 16-window row tile, than 64.  The one-window case is
    five one-window inputs (one 3x2 map cannot switch every channel on; tests/test_cnn_channels.py)."""
    eng = probe_engine
    inputs = [P.one_window_input(w) for w in range(P.ONE_WINDOW_INPUTS)] if windows == 1 else [P.fused_signal(windows)]

    def outputs(x):
        out = {"logits": eng.predict(x, 0.96).numpy().copy(), "emb": eng.embed(x, 0.96).numpy().copy()}
        for st in FUSED_STAGES:
            out[st] = eng.stage_tap(x, HOP, STEP, st, windows).cpu().numpy()
        return out

    try:
        for mode in ("f16x3", "f16", "f32"):
            eng.set_pointwise_mode(mode)
            for i, x in enumerate(inputs):
                eng.set_fusion(False, False)
                plain = outputs(x)
                assert plain["logits"].shape == (windows, 13) and plain["emb"].shape == (windows, 1024)
                assert np.isfinite(plain["logits"]).all()
                assert all((plain[st] > 0).any() and (plain[st] == 0).any() for st in FUSED_STAGES)
                for setting in FUSION_SETTINGS:
                    eng.set_fusion(*setting)
                    for key, got in outputs(x).items():
                        assert np.array_equal(got, plain[key]), (mode, setting, key, i)
        assert eng.overflow_reruns == 0
        exps, maxima = eng.scales()
        scaled = np.ldexp(maxima, exps)
        assert np.all(maxima > 0) and np.all(scaled >= 256.0) and np.all(scaled < 512.0), (exps, maxima)
    finally:
        eng.set_pointwise_mode("f16x3")
        eng.set_fusion(True, True)


@pytest.mark.parametrize("name", list(SIGNALS))
@pytest.mark.parametrize("mode", ["f32", "f16x3"])
def test_embedding_per_channel_and_logits_against_oracle(probe_engine, mode, name):
    """The pooled tail on the default (fused) path: every embedding channel by the rule of the stages, the logits within
    the suite's 1e-4 x max(1, max|ref|) of ``O.predict`` on the probe weights."""
    eng = probe_engine
    live, mel = _weights()
    head = W.load_head()
    x = SIGNALS[name]()
    _, emb, _, emb32 = _reference(name)
    ref_logits = O.predict(x, live, mel, head.kernel, head.bias, HOP, STEP, np.float64)
    assert np.abs(ref_logits - O.dense_head(emb, head.kernel, head.bias, np.float64)).max() < 1e-12
    try:
        eng.set_pointwise_mode(mode)
        got_emb = eng.embed(x, 0.96).numpy().copy()
        got_logits = eng.predict(x, 0.96).numpy().copy()
    finally:
        eng.set_pointwise_mode("f16x3")
    assert got_emb.shape == emb.shape and got_logits.shape == ref_logits.shape
    err = np.abs(got_emb - emb).max(axis=0)
    err32 = np.abs(emb32 - emb).max(axis=0)
    ref_max = np.abs(emb).max(axis=0)
    bound = P.channel_bound(POOL_STAGE, err32, ref_max)
    ratio = np.divide(err, err32, out=np.zeros_like(err), where=err32 > 0)
    above = err > P.floor_factor(POOL_STAGE) * ref_max
    print(f"\n[ratios] {mode} {name} embedding: worst err_gpu / err_f32oracle {ratio.max():.2f} (all channels), "
          f"{ratio[above].max() if above.any() else 0.0:.2f} (above the floor); logits err "
          f"{np.abs(got_logits - ref_logits).max():.3e}, max|ref| {np.abs(ref_logits).max():.3e}")
    assert (ref_max > 0).all()                                       # no embedding channel is multiplied by zeros
    bad = np.flatnonzero(err > bound)
    assert bad.size == 0, (f"{mode} {name}: embedding channel {bad[np.argmax(err[bad] / bound[bad])]}: {bad.size} channels "
                           f"miss; worst err {err[bad].max():.3e}, bounds {bound[bad].min():.3e}..{bound[bad].max():.3e}")
    assert np.abs(got_logits - ref_logits).max() < P.TOL_ABS * max(1.0, float(np.abs(ref_logits).max()))
    assert eng.overflow_reruns == 0
