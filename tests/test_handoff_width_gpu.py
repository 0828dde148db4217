"""The hand-offs around the two on-chip kernels of the default f16 launch set: sep_mid_kernel reads its window (the f32
depthwise-5 output) with six 16-byte loads per lane and publishes four channels per LDS write; sep_chip_kernel's waves take
the ring-free barrier on either side of their depthwise and write the depthwise-13 planes the tail reads.  None of it may
change a bit: logits and embeddings of the default set must be those of one kernel per op and of separable 10, for every partial
on-chip tile (windows mod 4), every run length of the persistent middle workgroups, passes that all end in a partial tile
(a hi-plane row stored past the batch would land on lo rows that are read afterwards), and the range guards of the two
rewritten splits must still send a chunk to the exact-f32 path."""
import numpy as np
import pytest

from oracle import yamnet_oracle as O

HOP = 15360
# every partial on-chip tile (windows mod 4 = 1, 2, 3); empty, one-window and uneven runs of the persistent middle
# workgroups; a second pass
WINDOWS = (1, 2, 3, 4, 5, 6, 7, 9, 255, 256, 257, 1024, 1027)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def audio():
    return O.synthetic_audio(HOP * (WINDOWS[-1] - 1) + 15600, seed=91)


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
        for windows in (3, 257):                        # hop 0.48: overlapping windows share log-mel rows
            _check(engine, audio[: HOP // 2 * (windows - 1) + 15600], 0.48, (pw_mode, "half hop", windows))
    finally:
        engine.set_pointwise_mode("f16x3")
        engine.set_fusion(True, True)


@pytest.mark.parametrize("layer", [5, 13])
def test_split_out_of_range_is_recomputed_in_f32(layer):
    """The product input of layer 5 (the depthwise-5 output, split by the middle run's A5 publication) or of layer 13 (the
    depthwise-13 output, split in the on-chip run's epilogue) scaled 2^14 above its calibration leaves the f16 range: the
    rows must be flagged and recomputed with exact f32 products."""
    from buzzdetect_amd.engine import HipEngine
    x = O.synthetic_audio(HOP * 20 + 15600, seed=92)
    eng = HipEngine()
    try:
        exps, _ = eng.scales()
        bad = exps.copy()
        bad[layer - 2] += 14
        eng.set_pointwise_mode("f32")
        exact = eng.predict(x, 0.96).numpy().copy()
        eng.set_activation_exponents(bad)
        for mode in ("f16x3", "f16"):
            eng.set_pointwise_mode(mode)
            before = eng.overflow_reruns
            assert np.array_equal(eng.predict(x, 0.96).numpy(), exact), (layer, mode)
            assert eng.overflow_reruns == before + 1, (layer, mode)
            assert not eng.range_exceeded()
    finally:
        eng.close()
