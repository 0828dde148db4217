"""The default f16 launch set hands layer 3 from the stem to the layer-4 kernel as the split-f16 A tiles of its 1x1
convolution (stem_reg_kernel ends at depthwise 3, l4_window_kernel opens with pointwise 3).  Logits and embeddings must be
the bits of one kernel per op and of the stem of rounds 2-4 (stem 5, which still writes the f32 layer-3 output)."""
import numpy as np
import pytest

from oracle import yamnet_oracle as O

HOP = 15360
WINDOWS = (1, 2, 13, 255, 256, 257, 1024, 1051)     # one / several / uneven windows per workgroup, a partial second pass

pytestmark = pytest.mark.gpu


def _outputs(engine, x, hop_s):
    return engine.predict(x, hop_s).numpy().copy(), engine.embed(x, hop_s).numpy().copy()


def _check(engine, x, hop_s, tag):
    refs = {}
    for fusion in ((0, 0), (5, 1)):
        engine.set_fusion(*fusion)
        refs[fusion] = _outputs(engine, x, hop_s)
    engine.set_fusion(3, 1)
    got = _outputs(engine, x, hop_s)
    again = _outputs(engine, x, hop_s)                  # the second call finds the first one's buffers
    for fusion, (logits, emb) in refs.items():
        assert np.array_equal(got[0], logits), (tag, fusion)
        assert np.array_equal(got[1], emb), (tag, fusion)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1]), tag


@pytest.mark.parametrize("pw_mode", ["f16x3", "f16"])
def test_stem_planes_are_bit_identical(engine, pw_mode):
    y = O.synthetic_audio(HOP * (WINDOWS[-1] - 1) + 15600, seed=71)
    try:
        engine.set_pointwise_mode(pw_mode)
        for windows in WINDOWS:
            _check(engine, y[: HOP * (windows - 1) + 15600], 0.96, (pw_mode, windows))
        for windows in (3, 257):                        # hop 0.48: overlapping windows share log-mel rows
            _check(engine, y[: HOP // 2 * (windows - 1) + 15600], 0.48, (pw_mode, "half hop", windows))
    finally:
        engine.set_pointwise_mode("f16x3")
        engine.set_fusion(True, True)


def test_depthwise3_out_of_range_is_recomputed_in_f32():
    """Layer 3's GEMM input scaled 2^14 above its calibration leaves the f16 range in the stem, which now ends there: the
    result must be flagged and recomputed with exact f32 products."""
    from buzzdetect_amd.engine import HipEngine
    x = O.synthetic_audio(HOP * 20 + 15600, seed=72)
    eng = HipEngine()
    try:
        exps, _ = eng.scales()
        bad = exps.copy()
        bad[3 - 2] += 14
        eng.set_pointwise_mode("f32")
        exact = eng.predict(x, 0.96).numpy().copy()
        eng.set_activation_exponents(bad)
        for mode in ("f16x3", "f16"):
            eng.set_pointwise_mode(mode)
            before = eng.overflow_reruns
            assert np.array_equal(eng.predict(x, 0.96).numpy(), exact), mode
            assert eng.overflow_reruns == before + 1, mode
            assert not eng.range_exceeded()
    finally:
        eng.close()
