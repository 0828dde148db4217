"""Memory hygiene of the inference hot path: bd_predict_chunks and bd_stage_tap on a workspace of exactly the bytes
the library asks for, between guard words, prefilled with zeros, NaNs and huge finite values; results written into guarded,
sentinel-prefilled tensors.  Held for every case: the same bits under the three patterns and on the session engine (whose
workspace is oversized and holds what earlier tests left), every result word written, no guard word changed, the call's range
word 0 and `overflow_reruns` where it was.  Every comparison is bit equality: there is no tolerance here."""
import numpy as np
import pytest

from buzzdetect_amd import modeldir as G, weights as W
from buzzdetect_amd.engine import LaunchVerdict
from tests.gpu_guards import HUGE, NAN, PATTERN_NAMES, PATTERNS, SENTINEL, ZERO, GuardedEngine
from oracle import yamnet_oracle as O

pytestmark = pytest.mark.gpu

HOP, STEP = 15360, 96
HALF = (7680, 48)
MODES = ("f16x3", "f16", "f32")
# launch sets (bd_set_fusion): the default, the stem of rounds 2-4 (f16 modes only), layers 5-7 on four kernels, a kernel per op
FUSIONS = ((True, True), (5, True), (True, 10), (False, False))
# the tile edges of 4 and 16 windows and one past each; (windows, hop, step)
SHAPES = [(w, HOP, STEP) for w in (1, 2, 3, 4, 5, 15, 16, 17, 33)] + [(w,) + HALF for w in (1, 5, 17)]
MAX_WINDOWS = 37


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} against {want.shape} {want.dtype}"
    differ = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert differ.size == 0, f"{what}: {differ.size} of {got.size} words differ, the first at flat index {int(differ[0])} " \
                             f"({bits(got).ravel()[differ[0]]:#010x} against {bits(want).ravel()[differ[0]]:#010x})"


@pytest.fixture(scope="module")
def audio(engine):
    """Audio for MAX_WINDOWS windows at whole hop, on the device once."""
    import torch
    return torch.from_numpy(O.synthetic_audio(HOP * (MAX_WINDOWS - 1) + 15600, seed=2201)).to(engine.device)


@pytest.fixture(scope="module")
def geng(engine, audio):
    """The packaged head on a GuardedEngine (the session engine is asked for first: it reports a missing GPU).  The session
    engine runs MAX_WINDOWS windows first, so that also when this file runs alone every case below finds it with a workspace
    larger than the case needs, holding another input's activations (the same audio, reversed)."""
    engine.launch([audio.flip(0)], HOP, STEP, True, True)
    eng = GuardedEngine(embeddername="yamnet_k2", modelname="model_general_v3")
    yield eng
    eng.close()


def guarded_run(eng, parts, hop, step, mode, want_embeddings):
    """One launch set per workspace pattern with guarded logits through `out=`; the embeddings (or None) and the logits of the
    first pattern after all three were found to hold the same bits.  Checks the guards, the range word and overflow_reruns."""
    import torch
    reruns = eng.overflow_reruns
    lengths = [int(p.numel()) for p in parts]
    total = sum(eng.num_windows(n, hop, step) for n in lengths)
    first = None
    for pattern in PATTERNS:
        eng.pattern = pattern
        out = eng.guards.empty((total, eng.n_classes), torch.float32, name="logits")
        verdict = LaunchVerdict(torch.cuda.current_stream(eng.device))
        emb, logits, counts = eng.launch(parts, hop, step, want_embeddings, True, out=out, mode=mode, verdict=verdict)
        assert sum(counts) == total and logits is out
        raised = verdict.wait()
        got = (emb.cpu().numpy() if want_embeddings else None, logits.cpu().numpy())
        eng.check_workspace()
        assert not raised, f"the range word was raised with the workspace prefilled with {PATTERN_NAMES[pattern]}"
        if first is None:
            first = got
        else:
            assert_same_bits(got[1], first[1], f"logits, workspace {PATTERN_NAMES[pattern]} against ZERO")
            if want_embeddings:
                assert_same_bits(got[0], first[0], f"embeddings, workspace {PATTERN_NAMES[pattern]} against ZERO")
    eng.pattern = ZERO
    assert eng.overflow_reruns == reruns
    return first


def plain_run(eng, parts, hop, step, mode, want_embeddings):
    emb, logits, _ = eng.launch(parts, hop, step, want_embeddings, True, mode=mode)
    return (emb.cpu().numpy() if want_embeddings else None, logits.cpu().numpy())


def hold_case(geng, engine, x, hop, step, mode):
    """Both result layouts of a pass: logits alone (the pooled rows then live in the workspace) and embeddings + logits."""
    for want_embeddings in (False, True):
        emb, logits = guarded_run(geng, [x], hop, step, mode, want_embeddings)
        ref_emb, ref_logits = plain_run(engine, [x], hop, step, mode, want_embeddings)
        assert_same_bits(logits, ref_logits, "logits against the session engine")
        if want_embeddings:
            assert_same_bits(emb, ref_emb, "embeddings against the session engine")
    return logits


LAUNCH_SETS = [(m, f) for m in MODES for f in FUSIONS if not (m == "f32" and f == (5, True))]      # stem 5: f16 modes only


@pytest.mark.parametrize("windows,hop,step", SHAPES)
@pytest.mark.parametrize("mode,fusion", LAUNCH_SETS, ids=[f"{m}-stem{int(f[0])}-sep{int(f[1])}" for m, f in LAUNCH_SETS])
def test_every_launch_set_is_blind_to_its_workspace_and_stays_inside_it(geng, engine, audio, mode, fusion, windows, hop, step):
    x = audio[: hop * (windows - 1) + 15600]
    assert geng.num_windows(x.numel(), hop, step) == windows
    try:
        for eng in (geng, engine):
            eng.set_fusion(*fusion)
        logits = hold_case(geng, engine, x, hop, step, mode)
        assert logits.shape == (windows, 13)
    finally:
        for eng in (geng, engine):
            eng.set_fusion(True, True)


@pytest.fixture(scope="module")
def default_pass_rows(geng, audio):
    """Embeddings and logits of MAX_WINDOWS windows at the default pass size, per mode, computed once."""
    geng.exact = False
    try:
        return {mode: plain_run(geng, [audio], HOP, STEP, mode, True) for mode in MODES}
    finally:
        geng.exact = True


@pytest.mark.parametrize("group", (4, 5, 16, 17))
@pytest.mark.parametrize("mode", MODES)
def test_a_partial_last_pass_at_a_small_pass_size(geng, engine, audio, default_pass_rows, mode, group):
    """The workspace is sized for `group` windows; the last pass has fewer, and finds the rows of the pass before it where its
    missing windows would be."""
    assert MAX_WINDOWS % group
    try:
        for eng in (geng, engine):
            eng.set_group_windows(group)
        emb, logits = guarded_run(geng, [audio], HOP, STEP, mode, True)
        ref_emb, ref_logits = plain_run(engine, [audio], HOP, STEP, mode, True)
    finally:
        for eng in (geng, engine):
            eng.set_group_windows(0)
    assert_same_bits(logits, ref_logits, "logits against the session engine")
    assert_same_bits(emb, ref_emb, "embeddings against the session engine")
    assert_same_bits(logits, default_pass_rows[mode][1], "logits against the default pass size")
    assert_same_bits(emb, default_pass_rows[mode][0], "embeddings against the default pass size")


# tests/test_gpu_parity.py's test_predict_batch_equals_per_chunk_calls lengths, the long chunks cut: 39 windows at whole hop, 37
# at half hop (an empty chunk is one window of padding); the 0-, 1- and 7-sample chunks kept
RAGGED = {1.0: [153_840, 15_600, 1, 0, 23_360, 100_001, 7, 138_479, 15_601, 64_000],
          0.5: [84_720, 15_600, 1, 0, 23_360, 53_999, 7, 69_359, 15_601, 32_000]}


def ragged_parts(guards, chunks, poison):
    """The chunks as views into one arena of `poison` words, chunk i at a float offset of i modulo 4, at least 4 poison words
    between two chunks and 4096 behind the last."""
    import torch
    at, starts = 0, []
    for i, c in enumerate(chunks):
        while at % 4 != i % 4:
            at += 1
        starts.append(at)
        at += len(c) + 4
    arena = guards.empty((at + 4096,), torch.float32, fill=poison, name="chunk arena")
    for s, c in zip(starts, chunks):
        if len(c):
            arena[s:s + len(c)].copy_(torch.from_numpy(c))
    return [arena[s:s + len(c)] for s, c in zip(starts, chunks)]


@pytest.fixture(scope="module")
def ragged_singles(geng):
    """Per hop: the chunks and the rows of one predict / embed per cloned chunk, computed once."""
    out = {}
    for hop_prop, lengths in RAGGED.items():
        chunks = [O.synthetic_audio(max(n, 1), seed=900 + i)[:n] for i, n in enumerate(lengths)]
        rows = [(geng.embed(c.copy(), 0.96 * hop_prop).numpy(), geng.predict(c.copy(), 0.96 * hop_prop).numpy()) for c in chunks]
        geng.check_workspace()
        out[hop_prop] = (chunks, rows)
    return out


@pytest.mark.parametrize("poison", (NAN, HUGE), ids=lambda p: PATTERN_NAMES[p])
@pytest.mark.parametrize("hop_prop", (1.0, 0.5))
def test_ragged_chunks_do_not_see_what_lies_between_and_behind_them(geng, ragged_singles, hop_prop, poison):
    chunks, singles = ragged_singles[hop_prop]
    hop, step = int(15360 * hop_prop), int(96 * hop_prop)
    total = sum(s[1].shape[0] for s in singles)
    assert 30 <= total <= 40
    want_emb = np.concatenate([s[0] for s in singles])
    want_logits = np.concatenate([s[1] for s in singles])
    parts = ragged_parts(geng.guards, chunks, poison)
    assert [p.data_ptr() % 16 // 4 for p in parts if p.numel()] == [i % 4 for i, p in enumerate(parts) if p.numel()]
    # launch: the views as they are
    emb, logits = guarded_run(geng, parts, hop, step, None, True)
    assert_same_bits(logits, want_logits, "launch: logits against one predict per cloned chunk")
    assert_same_bits(emb, want_emb, "launch: embeddings against one embed per cloned chunk")
    # predict_batch: the same views (it copies those that are not 16-byte aligned), results read through DeviceResult
    reruns = geng.overflow_reruns
    for pattern in PATTERNS:
        geng.pattern = pattern
        rows, embs = geng.predict_batch(parts, 0.96 * hop_prop, want_embeddings=True)
        for i, (r, e) in enumerate(zip(rows, embs)):
            assert_same_bits(r.numpy(), singles[i][1], f"predict_batch: logits of chunk {i}")
            assert_same_bits(e.numpy(), singles[i][0], f"predict_batch: embeddings of chunk {i}")
        geng.check_workspace()
    geng.pattern = ZERO
    assert geng.overflow_reruns == reruns


@pytest.mark.parametrize("windows", (1, 3))
@pytest.mark.parametrize("mode", ("f16x3", "f32"))
def test_stage_taps_are_fully_written_and_blind_to_the_workspace(geng, audio, mode, windows):
    """All 27 stages for the first 1 and 3 of 5 windows: tap_out guarded and fully written, the same bits under the three
    patterns."""
    from buzzdetect_amd import _lib
    x = audio[: HOP * 4 + 15600]
    geng.set_pointwise_mode(mode)
    try:
        for stage in range(_lib.NUM_STAGES):
            first = None
            for pattern in PATTERNS:
                geng.pattern = pattern
                got = geng.stage_tap(x, HOP, STEP, stage, windows).cpu().numpy()
                geng.check_workspace()
                assert got.shape[0] == windows
                if first is None:
                    first = got
                else:
                    assert_same_bits(got, first, f"stage {stage}, workspace {PATTERN_NAMES[pattern]} against ZERO")
    finally:
        geng.pattern = ZERO
        geng.set_pointwise_mode("f16x3")


# ---- heads that use the scratch behind the pooled embeddings

def head(widths, acts, seed):
    return W.HeadWeights(G.glorot_layers(widths, acts, seed=seed), [f"c{i}" for i in range(widths[-1])])


def head_engines():
    members = {"m0": head([33, 2], ["relu", "linear"], 41), "m1": head([33, 2], ["relu", "linear"], 42)}
    return {
        "stack": dict(head=head([48, 33, 5], ["relu", "tanh", "linear"], 31)),                 # two hidden layers deep
        "set": dict(heads={"fused": head([13], ["linear"], 32), "stacked": head([40, 7], ["relu", "softmax"], 33)}),
        "ensemble": dict(heads={"voted": W.EnsembleWeights(members, "mean", None, ["c0", "c1"]),
                                "lone": head([13], ["linear"], 34)}),
    }


@pytest.fixture(scope="module", params=sorted(head_engines()))
def head_engine(request, engine, audio):
    """A GuardedEngine with the head of the case, and the rows its plain side gives: computed with `exact` off, i.e. as a
    HipEngine computes them, after a pass of MAX_WINDOWS windows of other audio has grown its workspace and left its rows there."""
    eng = GuardedEngine(modelname=None, **head_engines()[request.param])
    eng.exact = False
    plain_run(eng, [audio.flip(0)], HOP, STEP, None, True)
    want = {(mode, w): plain_run(eng, [audio[: HOP * (w - 1) + 15600]], HOP, STEP, mode, True) for mode in MODES for w in (1, 5, 17)}
    eng.exact = True
    yield eng, want
    eng.close()


@pytest.mark.parametrize("windows", (1, 5, 17))
@pytest.mark.parametrize("mode", MODES)
def test_head_scratch_behind_the_embeddings(head_engine, audio, mode, windows):
    eng, want = head_engine
    x = audio[: HOP * (windows - 1) + 15600]
    for want_embeddings in (False, True):           # False: the pooled rows sit in the workspace, the scratch right behind them
        emb, logits = guarded_run(eng, [x], HOP, STEP, mode, want_embeddings)
        assert logits.shape == (windows, eng.n_classes)
        assert_same_bits(logits, want[(mode, windows)][1], "logits against the engine's plain side")
        if want_embeddings:
            assert_same_bits(emb, want[(mode, windows)][0], "embeddings against the engine's plain side")


# ---- negative controls: a guard helper that cannot fail proves nothing

def test_control_a_write_behind_the_workspace_is_reported(geng, audio):
    """The library is handed one 256-byte unit more than the helper guards.  If it writes there, `check` says so; it does not
    (bd_workspace_bytes ends in 256 bytes no kernel is given), so one guard word is changed from here instead.  Then the helper
    is made to guard 64 KiB less than the library was handed, where a kernel does write: `check` has to report the library's
    own stores."""
    import torch
    x = audio[:15600]
    geng.workspace_slack = 256
    try:
        geng.launch([x], HOP, STEP, True, True)
    finally:
        geng.workspace_slack = 0
    name, raw, nbytes, _, _ = next(a for a in geng.guards.whole if a[0].startswith("workspace"))
    kept = list(geng.guards.whole)
    try:
        geng.check_workspace()
        wrote = False
    except AssertionError as err:
        wrote = True
        assert "workspace" in str(err) and "behind the buffer" in str(err)
    if not wrote:
        from tests.gpu_guards import FRONT
        geng.guards.whole = kept
        word = FRONT // 4 + (nbytes + 3) // 4 + 5
        raw[word] = 0
        with pytest.raises(AssertionError, match=rf"workspace \(ZERO\): the guard word at byte offset {nbytes + 20} \(20 bytes behind"):
            geng.check_workspace()
        raw[word] = raw[word + 1]
        geng.guards.whole = kept
        raw[3] = 1                                   # ... and one in front
        with pytest.raises(AssertionError, match="in front of the buffer"):
            geng.check_workspace()
    # the same on the library's own writes: the helper guards all but the last 64 KiB of what the library asked for and was
    # handed.  A kernel per op: depthwise 2 fills buffer b, the workspace's last region, to its last float (48 x 32 x 32 per
    # window), so the last window's rows land in what the helper takes for guard words - memory of the same arena
    geng.workspace_short = 64 << 10
    try:
        geng.set_fusion(False, False)
        geng.launch([x], HOP, STEP, True, True, mode="f32")
    finally:
        geng.workspace_short = 0
        geng.set_fusion(True, True)
    with pytest.raises(AssertionError, match=r"workspace \(ZERO\): the guard word at byte offset \d+ \(\d+ bytes behind"):
        geng.check_workspace()
    # an output word nobody wrote is reported too
    geng.guards.empty((4, 13), torch.float32, name="never written")
    with pytest.raises(AssertionError, match="never written: the word at byte offset 0 was not written"):
        geng.guards.check()
    # and the clean run passes
    geng.launch([x], HOP, STEP, True, True)
    geng.check_workspace()


def test_control_b_a_poisoned_word_in_a_row_fails_the_bit_equality(geng, audio):
    import torch
    x = audio[: HOP * 2 + 15600]
    emb, logits, _ = geng.launch([x], HOP, STEP, True, True)
    clean = logits.cpu().numpy()
    geng.check_workspace()
    assert_same_bits(logits.cpu().numpy(), clean, "clean")
    for poison in (NAN, HUGE, SENTINEL):
        bad = logits.clone()
        bad.view(torch.int32)[1, 7] = poison - (1 << 32) if poison >= 1 << 31 else poison
        with pytest.raises(AssertionError, match="1 of 39 words differ, the first at flat index 20"):
            assert_same_bits(bad.cpu().numpy(), clean, "poisoned")
