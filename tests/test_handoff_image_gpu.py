"""The hand-offs between the layers that sep_mid_kernel (A6) and sep_chip_kernel (layers 8-12) keep on the CU: published
channel-major with 8-byte LDS writes and read back transposed.  Only the route through LDS changed, so no
bit may move: logits and embeddings of the default launch set must be those of one kernel per op - the independent
reference: separable 10 runs the same on-chip kernel - and of separable 10, in both f16 modes, each run twice so that the
second call finds the first one's buffers.  On the probe weights no channel is dead, so a swapped chunk or k-row cannot
cancel; and the range guards of the two rewritten splits must still send a chunk to the exact-f32 path."""
import numpy as np
import pytest

import cnn_probe as P
from buzzdetect_amd import weights as W
from oracle import yamnet_oracle as O

HOP = 15360
# every partial 4-window tile of the on-chip run, an uneven run of the persistent middle workgroups, a second tile wave
WINDOWS = (1, 2, 3, 4, 5, 9, 257)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def audio():
    return O.synthetic_audio(HOP * (WINDOWS[-1] - 1) + 15600, seed=101)


def _outputs(engine, x, hop_s):
    return engine.predict(x, hop_s).numpy().copy(), engine.embed(x, hop_s).numpy().copy()


def _check(engine, x, hop_s, tag):
    refs = {}
    for fusion in ((0, 0), (3, 10)):
        engine.set_fusion(*fusion)
        refs[fusion] = _outputs(engine, x, hop_s)
    engine.set_fusion(3, 1)
    got = _outputs(engine, x, hop_s)
    again = _outputs(engine, x, hop_s)                  # the second call finds the first one's buffers
    for fusion, (logits, emb) in refs.items():
        assert np.array_equal(got[0], logits), (tag, fusion)
        assert np.array_equal(got[1], emb), (tag, fusion)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1]), tag
    return got


@pytest.mark.parametrize("pw_mode", ["f16x3", "f16"])
def test_window_counts_are_bit_identical(engine, audio, pw_mode):
    try:
        engine.set_pointwise_mode(pw_mode)
        for windows in WINDOWS:
            _check(engine, audio[: HOP * (windows - 1) + 15600], 0.96, (pw_mode, windows))
    finally:
        engine.set_pointwise_mode("f16x3")
        engine.set_fusion(True, True)


@pytest.mark.parametrize("pw_mode", ["f16x3", "f16"])
def test_small_passes_end_in_partial_tiles(engine, audio, pw_mode):
    """23 windows in passes of 5 and of 7: every pass ends in a partial tile of the on-chip run."""
    x = audio[: HOP * 22 + 15600]
    try:
        engine.set_pointwise_mode(pw_mode)
        for group in (5, 7):
            engine.set_group_windows(group)
            _check(engine, x, 0.96, (pw_mode, "group", group))
    finally:
        engine.set_group_windows(0)
        engine.set_pointwise_mode("f16x3")
        engine.set_fusion(True, True)


@pytest.mark.parametrize("pw_mode", ["f16x3", "f16"])
def test_half_hop_is_bit_identical(engine, audio, pw_mode):
    try:
        engine.set_pointwise_mode(pw_mode)
        _check(engine, audio[: HOP // 2 * 2 + 15600], 0.48, (pw_mode, "half hop", 3))
    finally:
        engine.set_pointwise_mode("f16x3")
        engine.set_fusion(True, True)


@pytest.fixture(scope="module")
def probe_engine():
    """One engine on the probe weights (no dead channel) for this module."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible (there is no CPU fallback)")
    from buzzdetect_amd.engine import HipEngine
    live = P.live_blob(W.synthetic_embedder_blob(), W.load_mel("yamnet_k2"))
    eng = HipEngine(embeddername="yamnet_k2", modelname="model_general_v3", embedder_blob=live)
    yield eng
    eng.close()


@pytest.mark.parametrize("windows", [5, 17])
def test_live_channels_are_bit_identical(probe_engine, windows):
    eng = probe_engine
    x = P.fused_signal(windows)
    try:
        for pw_mode in ("f16x3", "f16"):
            eng.set_pointwise_mode(pw_mode)
            logits, emb = _check(eng, x, 0.96, ("probe", pw_mode, windows))
            assert logits.shape == (windows, 13) and emb.shape == (windows, 1024)
            assert np.isfinite(logits).all()
        assert eng.overflow_reruns == 0
    finally:
        eng.set_pointwise_mode("f16x3")
        eng.set_fusion(True, True)


@pytest.mark.parametrize("layer", [6, 9, 12])
def test_split_out_of_range_is_recomputed_in_f32(layer):
    """The product input of layer 6 (the depthwise-6 output, split by the middle run's A6 publication) or of layers 9 and 12
    (split between the layers of the on-chip run) scaled 2^14 above its calibration leaves the f16 range: the rows must be
    flagged and recomputed with exact f32 products."""
    from buzzdetect_amd.engine import HipEngine
    x = O.synthetic_audio(HOP * 20 + 15600, seed=102)
    eng = HipEngine()
    try:
        exps, _ = eng.scales()
        bad = exps.copy()
        bad[layer - 2] += 14
        eng.set_pointwise_mode("f32")
        exact = eng.predict(x, 0.96).numpy().copy()
        assert exact.shape[0] == 21
        eng.set_activation_exponents(bad)
        for mode in ("f16x3", "f16"):
            eng.set_pointwise_mode(mode)
            before = eng.overflow_reruns
            assert np.array_equal(eng.predict(x, 0.96).numpy(), exact), (layer, mode)
            assert eng.overflow_reruns == before + 1, (layer, mode)
            assert not eng.range_exceeded()
    finally:
        eng.close()
