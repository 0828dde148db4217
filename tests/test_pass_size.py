"""Passes through the CNN up to the largest supported size (``bd_set_group_windows``, 65 536 windows), on the GPU.

A pass needs 589 824 bytes of workspace per window: buffer A holds 393 216, buffer B 196 608, and the activation tensors in
them take 393 216, 196 608, 98 304 or 49 152 bytes per window.  Each kind crosses 2^31 and 2^32 bytes at some pass size
below the cap:

    bytes per window    2^31 at window    2^32 at window
    393 216                   5 462            10 923
    196 608                  10 923            21 846
     98 304                  21 846            43 691
     49 152                  43 691                 -

A kernel that builds a byte offset or a buffer resource in 32 bits goes wrong past one of these windows.  Every launch set
runs one batch of 31 half-hop chunks (about 67.7k windows, so the second pass is a partial one) at a pass of 1024 windows
and at passes just past each crossing and at the cap; logits and embeddings must agree bit for bit.  Spot checks against
the float64 oracle cover the windows on both sides of each crossing.

The module keeps its own engine: its workspace at the cap is 38.7 GB, which the session engine would hold on to.
"""
import time

import numpy as np
import pytest

from oracle import yamnet_oracle as O

pytestmark = pytest.mark.gpu

TOL_LOGITS = 1e-4
HOP, STEP = 7680, 48                 # half hop
CHUNK = (1 << 24) - 1                # the longest chunk plan_batch accepts
N_CHUNKS = 31
CAP = 65536
SIZES = (CAP, 43692, 21847, 10924, 5463)          # descending: the workspace is allocated once
NEED_BYTES = 45 * 10 ** 9

# (pointwise mode, bd_set_fusion stem, separable)
LAUNCH_SETS = [
    ("f16x3", True, True),
    ("f16", True, True),
    ("f32", True, True),
    ("f32", True, 10),
    ("f16x3", 5, True),
    ("f16x3", False, False),
    ("f32", False, False),
]


@pytest.fixture(scope="module")
def big():
    """The module's engine and its input: 31 chunks of 2^24 - 1 samples of seeded noise, drawn on the device."""
    import torch
    from buzzdetect_amd.engine import HipEngine
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible (there is no CPU fallback)")
    free, _ = torch.cuda.mem_get_info()
    if free < NEED_BYTES:
        pytest.fail(f"test_pass_size needs {NEED_BYTES / 1e9:.0f} GB of free device memory, the device has {free / 1e9:.1f} GB")
    eng = HipEngine(embeddername="yamnet_k2", modelname="model_general_v3")
    gen = torch.Generator(device=eng.device).manual_seed(20261016)
    # rows of 2^24 floats keep every chunk 16-byte aligned; the last sample of each row is not used
    pcm = torch.randn((N_CHUNKS, 1 << 24), generator=gen, device=eng.device).mul_(0.1).clamp_(-1.0, 1.0)
    parts = [pcm[c, :CHUNK] for c in range(N_CHUNKS)]
    per_chunk = O.num_windows(CHUNK, HOP, STEP)
    torch.cuda.reset_peak_memory_stats(eng.device)
    state = {"engine": eng, "pcm": pcm, "parts": parts, "per_chunk": per_chunk, "total": per_chunk * N_CHUNKS}
    yield state
    peak = torch.cuda.max_memory_allocated(eng.device)
    print(f"\n[pass_size] peak device memory allocated by torch: {peak / 1e9:.1f} GB")
    eng.close()
    eng._workspace = None
    state.clear()
    del pcm, parts, eng
    torch.cuda.empty_cache()


def _configure(eng, mode, stem, separable, group):
    eng.set_pointwise_mode(mode)
    eng.set_fusion(stem, separable)
    eng.set_group_windows(group)


def _run(big, mode):
    """One bd_predict_chunks over the whole batch; in the f16 modes the launch set's range word must stay clear."""
    import torch
    from buzzdetect_amd.engine import LaunchVerdict
    eng = big["engine"]
    stream = torch.cuda.current_stream(eng.device)
    verdict = LaunchVerdict(stream) if mode != "f32" else None
    emb, logits, per = eng.launch(big["parts"], HOP, STEP, True, True, verdict=verdict)
    assert per == [big["per_chunk"]] * N_CHUNKS
    if verdict is not None:
        assert not verdict.wait(), f"{mode}: an activation left the f16 range; the f16 result is not the one under test"
    torch.cuda.synchronize(eng.device)
    return emb, logits


def _first_difference(a, b):
    rows = (a != b).reshape(a.shape[0], -1).any(dim=1).nonzero()
    return int(rows[0]) if rows.numel() else None


@pytest.mark.parametrize("mode,stem,separable", LAUNCH_SETS)
def test_every_pass_size_gives_the_1024_window_bits(big, mode, stem, separable):
    import torch
    eng = big["engine"]
    assert big["total"] > CAP and big["total"] - CAP < big["per_chunk"]
    try:
        _configure(eng, mode, stem, separable, 1024)
        ref_emb, ref_logits = _run(big, mode)
        assert ref_logits.shape == (big["total"], 13) and bool(ref_logits.isfinite().all())
        for group in SIZES:
            eng.set_group_windows(group)
            t0 = time.perf_counter()
            emb, logits = _run(big, mode)
            dt = time.perf_counter() - t0
            print(f"\n[pass_size] {mode} ({stem}, {separable}) group {group}: {dt:.3f} s")
            for name, got, ref in (("logits", logits, ref_logits), ("embeddings", emb, ref_emb)):
                assert got.shape == ref.shape
                if not torch.equal(got, ref):
                    w = _first_difference(got, ref)
                    pytest.fail(f"{mode} ({stem}, {separable}) group {group}: {name} differ from the 1024-window pass, "
                                f"first at window {w} of {big['total']}")
            del emb, logits
    finally:
        _configure(eng, "f16x3", True, True, 0)


# windows either side of each crossing, the cap's last window, the first window of the second pass, and the last window of
# the batch (the zero-padded end of a chunk, in the partial pass)
SPOT_WINDOWS = (5461, 5462, 10922, 10923, 21845, 21846, 43690, 43691, CAP - 1, CAP)


@pytest.fixture(scope="module")
def oracle_rows(big, weights_bundle):
    """The float64 oracle's logits of single windows, each from that window's samples only (computed once per window)."""
    rows = {}

    def get(j):
        if j not in rows:
            c, k = divmod(j, big["per_chunk"])
            seg = big["parts"][c][k * HOP: k * HOP + 15600].cpu().numpy()
            b = weights_bundle
            ref = O.predict(seg, b["blob"], b["mel"], b["head_kernel"], b["head_bias"], HOP, STEP, np.float64)
            assert ref.shape == (1, 13)
            rows[j] = ref[0]
        return rows[j]
    return get


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
def test_largest_pass_against_the_oracle(big, oracle_rows, mode):
    eng = big["engine"]
    last = big["total"] - 1
    assert (last + 1) % big["per_chunk"] == 0
    try:
        _configure(eng, mode, True, True, CAP)
        _, logits = _run(big, mode)
        got = logits.cpu().numpy()
        for j in SPOT_WINDOWS + (last,):
            err = float(np.abs(got[j] - oracle_rows(j)).max())
            assert err < TOL_LOGITS, (mode, j, err)
    finally:
        _configure(eng, "f16x3", True, True, 0)


def test_pass_size_limit(big):
    import torch
    from buzzdetect_amd._lib import BuzzdetectHipError
    eng = big["engine"]
    parts = big["parts"][:2]
    lengths = [int(p.numel()) for p in parts]

    def workspace_bytes():
        import ctypes as C
        arr = (C.c_int64 * len(lengths))(*lengths)
        return eng._lib.bd_batch_workspace_bytes(eng._handle, arr, len(lengths), HOP, STEP)

    try:
        eng.set_group_windows(1024)
        ws_1024 = workspace_bytes()
        _, ref, _ = eng.launch(parts, HOP, STEP, False, True)
        with pytest.raises(BuzzdetectHipError, match="BD_EINVAL") as info:
            eng.set_group_windows(CAP + 1)
        assert info.value.code == -1
        with pytest.raises(BuzzdetectHipError, match="BD_EINVAL"):
            eng.set_group_windows(-1)
        assert workspace_bytes() == ws_1024                  # a refused size leaves the pass size alone
        eng.set_group_windows(CAP)
        assert workspace_bytes() > ws_1024                   # the 4368 windows are one pass
        eng.set_group_windows(0)
        assert workspace_bytes() == ws_1024                  # 0 is the default of 1024
        _, again, _ = eng.launch(parts, HOP, STEP, False, True)
        torch.cuda.synchronize(eng.device)
        assert torch.equal(again, ref)
    finally:
        eng.set_group_windows(0)
