"""The default f16 launch set hands layer 7 from the middle run to the on-chip run as the split-f16 A operand of its 1x1
convolution (sep_mid_kernel ends at depthwise 7, sep_chip_kernel opens with pointwise 7).  Logits and embeddings must be
the bits of one kernel per op and of separable 10 (layers 5-7 on four kernels, the on-chip run reading the f32 layer-7
output)."""
import numpy as np
import pytest

from oracle import yamnet_oracle as O

HOP = 15360
# one / several / uneven windows per middle-run workgroup, partial on-chip tiles (4 windows each), a second pass
WINDOWS = (1, 2, 3, 4, 5, 13, 255, 256, 257, 1024, 1051)

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("pw_mode", ["f16x3", "f16"])
def test_mid_planes_are_bit_identical(engine, pw_mode):
    y = O.synthetic_audio(HOP * (WINDOWS[-1] - 1) + 15600, seed=81)
    try:
        engine.set_pointwise_mode(pw_mode)
        for windows in WINDOWS:
            _check(engine, y[: HOP * (windows - 1) + 15600], 0.96, (pw_mode, windows))
        for windows in (3, 257):                        # hop 0.48: overlapping windows share log-mel rows
            _check(engine, y[: HOP // 2 * (windows - 1) + 15600], 0.48, (pw_mode, "half hop", windows))
    finally:
        engine.set_pointwise_mode("f16x3")
        engine.set_fusion(True, True)


def test_depthwise7_out_of_range_is_recomputed_in_f32():
    """Layer 7's GEMM input scaled 2^14 above its calibration leaves the f16 range in the middle run, which now ends there:
    the result must be flagged and recomputed with exact f32 products."""
    from buzzdetect_amd.engine import HipEngine
    x = O.synthetic_audio(HOP * 20 + 15600, seed=82)
    eng = HipEngine()
    try:
        exps, _ = eng.scales()
        bad = exps.copy()
        bad[7 - 2] += 14
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
