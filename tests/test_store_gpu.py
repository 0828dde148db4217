"""The embedding store on the GPU (csrc/rowcodec.hip, bd_score_rows, buzzdetect_amd/store.py): the codec's kernels against their
host restatements in every bit, engine.score_rows against engine.predict in every bit for every kind of head, and every tool from
a store against the same tool from the audio - with an engine whose embedder cannot launch.  Outputs lie between guard words."""
import dataclasses
import os
import wave

import numpy as np
import pytest

from buzzdetect_amd import _lib, dataset as D, modeldir as G, store, weights as W
from oracle import yamnet_oracle as O
from tests.test_store_host import all_rows

pytestmark = pytest.mark.gpu

CODECS = ("f32", "h", "b")
HOP = 15360
CHUNK = 4.8                       # five windows per chunk


def guards():
    from tests.gpu_guards import Guarded
    return Guarded()


# ---------------------------------------------------------------------------------------------------- 1. device against host
@pytest.mark.parametrize("w", (1, 63, 64, 65, 255, 256, 257, 1025))
@pytest.mark.parametrize("codec", CODECS)
def test_device_codec_is_the_host_codec_in_every_bit(monkeypatch, codec, w):
    import torch
    rows = np.concatenate([all_rows(513), all_rows(513)[::-1]])[:w]          # (the edge rows of the host tests are among them)
    g = guards()
    monkeypatch.setattr(store, "_device_empty", lambda shape, dtype, device: g.empty(shape, dtype))
    dev = torch.from_numpy(rows).cuda()
    records, sums, flags = store.encode_device(dev, codec)
    got = (records.cpu().numpy(), sums.cpu().numpy().view(np.uint64), int(flags.cpu()[0]))
    g.check()
    want = store.encode_host(rows, codec)
    assert got[0].tobytes() == want[0].tobytes(), "records"
    assert got[1].tobytes() == want[1].tobytes(), "sums"
    assert got[2] == want[2] and (w < 10 or want[2] >= 2), "flags"
    back, read = store.decode_device(records, codec)
    got = (back.cpu().numpy(), read.cpu().numpy().view(np.uint64))
    g.check()
    want_back, want_read = store.decode_host(want[0], codec)
    assert got[0].tobytes() == want_back.tobytes(), "decoded rows"
    assert got[1].tobytes() == want_read.tobytes() == want[1].tobytes(), "sums of the bytes read"
    if codec == "f32":
        assert got[0].tobytes() == rows.tobytes()


def test_refusals_name_their_argument_and_launch_nothing():
    import torch
    lib = _lib.load()
    rows = torch.zeros((4, 1024), dtype=torch.float32, device="cuda")
    g = guards()
    rec, sums, flags = g.empty((4, 4096), torch.uint8), g.empty((1, 2), torch.int64), g.empty((1,), torch.int32)
    s = torch.cuda.current_stream().cuda_stream
    for args, word in (((rows.data_ptr(), 4, 7, rec.data_ptr(), sums.data_ptr(), flags.data_ptr(), s), "codec"),
                       ((rows.data_ptr(), -1, 0, rec.data_ptr(), sums.data_ptr(), flags.data_ptr(), s), "windows"),
                       ((rows.data_ptr() + 4, 4, 0, rec.data_ptr(), sums.data_ptr(), flags.data_ptr(), s), "rows"),
                       ((rows.data_ptr(), 4, 0, None, sums.data_ptr(), flags.data_ptr(), s), "records"),
                       ((rows.data_ptr(), 4, 0, rec.data_ptr(), sums.data_ptr() + 4, flags.data_ptr(), s), "sums"),
                       ((rows.data_ptr(), 4, 0, rec.data_ptr(), sums.data_ptr(), None, s), "flags")):
        assert lib.bd_rows_encode(*args) == -1 and word in lib.bd_last_error().decode()
    assert lib.bd_rows_decode(rec.data_ptr(), 4, 0, None, sums.data_ptr(), s) == -1 and "rows" in lib.bd_last_error().decode()
    g.check(written=False)
    assert lib.bd_rows_record_bytes(3) == -1 and [lib.bd_rows_record_bytes(c) for c in range(3)] == [4096, 2064, 1040]


# ---------------------------------------------------------------------------------------------------- 2. scoring equals predicting
def _head(widths, acts, seed):
    return W.HeadWeights(G.glorot_layers(widths, acts, seed=seed), [f"c{i}" for i in range(widths[-1])])


def _engine_kwargs(kind):
    if kind == "packaged":
        return dict(modelname="model_general_v3")
    if kind == "stack":
        return dict(modelname=None, head=_head([31, 13], ["relu", "linear"], 5))
    members = {"fused": _head([13], ["linear"], 6), "stack": _head([33, 2], ["relu", "linear"], 7),
               "soft": _head([64, 7], ["relu", "softmax"], 8), "lin65": _head([65], ["linear"], 9)}
    if kind == "set":                                        # members of both routes: the fused kernel and the stack kernels
        return dict(modelname=None, heads=members)
    trio = {f"m{i}": _head([33, 4], ["relu", "linear"], 20 + i) for i in range(3)}
    pair = {f"m{i}": _head([5], ["linear"], 30 + i) for i in range(2)}
    return dict(modelname=None, heads={"soft_vote": W.EnsembleWeights(trio, "mean_probability", "softmax", list(trio["m0"].classes)),
                                       "plain": members["stack"],
                                       "mean": W.EnsembleWeights(pair, "mean", None, list(pair["m0"].classes))})


@pytest.fixture(scope="module")
def audio():
    return O.synthetic_audio(HOP * 1025 + 240, seed=77)


@pytest.mark.parametrize("mode", ("f16x3", "f32"))
@pytest.mark.parametrize("kind", ("packaged", "stack", "set", "ensemble"))
def test_scoring_stored_rows_equals_predicting(audio, kind, mode):
    import torch
    from buzzdetect_amd.engine import HipEngine
    from tests.gpu_guards import NAN

    class ScoringEngine(HipEngine):
        guards = None

        def _empty(self, shape):
            return self.guards.empty(shape, torch.float32, name=f"result {tuple(shape)}") if self.guards else super()._empty(shape)

        def _score_ws(self, nbytes):                          # exactly bd_score_rows_workspace_bytes, poisoned
            if not nbytes or self.guards is None:
                return super()._score_ws(nbytes)
            return self.guards.empty((nbytes,), torch.uint8, fill=NAN, name="score workspace")

    eng = ScoringEngine(**_engine_kwargs(kind))
    try:
        eng.set_pointwise_mode(mode)
        for w in (1, 64, 65, 1025):
            x = audio[:HOP * w + 240]
            want = eng.predict(x, 0.96).numpy()
            rows = eng.embed(x, 0.96).device_tensor()
            assert want.shape == (w, eng.n_classes) and rows.shape == (w, 1024)
            need = eng._lib.bd_score_rows_workspace_bytes(eng._handle, w)
            assert need == (0 if kind == "packaged" else min(w, 1024) * 4 * 2048 * 4)
            eng.guards = guards()
            got = eng.score_rows(rows)
            host = got.cpu().numpy()
            eng.guards.check()
            eng.guards = None
            assert host.tobytes() == want.tobytes(), f"{kind}, {mode}, {w} windows"
        empty = eng.score_rows(rows[:0])
        assert tuple(empty.shape) == (0, eng.n_classes)
        lib, s = eng._lib, torch.cuda.current_stream().cuda_stream
        out = torch.zeros((2, eng.n_classes), dtype=torch.float32, device="cuda")
        ws = torch.zeros(2 * 4 * 2048 * 4, dtype=torch.uint8, device="cuda")
        for args, word in (((eng._handle, None, 2, out.data_ptr(), ws.data_ptr(), ws.numel(), s), "rows_dev"),
                           ((eng._handle, rows.data_ptr(), 2, out.data_ptr() + 4, ws.data_ptr(), ws.numel(), s), "logits_dev"),
                           ((eng._handle, rows.data_ptr(), -2, out.data_ptr(), ws.data_ptr(), ws.numel(), s), "windows")):
            assert lib.bd_score_rows(*args) == -1 and word in lib.bd_last_error().decode()
        if kind != "packaged":
            assert lib.bd_score_rows(eng._handle, rows.data_ptr(), 2, out.data_ptr(), ws.data_ptr(), ws.numel() - 1, s) == -4
            assert "workspace" in lib.bd_last_error().decode()
        torch.cuda.synchronize()
        assert not out.any()
    finally:
        eng.close()


def test_an_engine_without_a_classifier_is_refused():
    from buzzdetect_amd.engine import HipEngine
    import torch
    eng = HipEngine(modelname=None)
    try:
        with pytest.raises(RuntimeError, match="classifier"):
            eng.score_rows(torch.zeros((1, 1024), dtype=torch.float32, device="cuda"))
        assert eng._lib.bd_score_rows_workspace_bytes(eng._handle, 1) == -1
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------- 3. tools from a store
def write_wav(path, pcm16, rate):
    pcm16 = np.asarray(pcm16, "<i2")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if pcm16.ndim == 1 else pcm16.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm16.tobytes())


def to_s16(x):
    return (np.clip(x, -1, 1 - 2 ** -15) * 32768.0).round().astype(np.int16)


def tree(root):
    return {os.path.relpath(os.path.join(b, f), root): open(os.path.join(b, f), "rb").read()
            for b, _, files in os.walk(root) for f in files if f.endswith((".csv", ".json"))}


NOTES = {"a": [(0.96, 1.46, "ins_buzz"), (3 * 0.96, 3 * 0.96 + 0.5, "ins_buzz"), (5.0, 5.9, "ambient_rain")],
         "site/b": [(2.0, 4.1, "ins_buzz")], "nowhere": [(0.0, 1.0, "ins_buzz")]}


@pytest.fixture(scope="module")
def scene(tmp_path_factory, engine):
    """The folder of tests/test_search_gpu.py - three recordings of about ten windows: 16 kHz mono, 44.1 kHz stereo, 16 kHz mono -
    a second model, and the folder embedded once per codec."""
    root = tmp_path_factory.mktemp("store")
    audio = root / "audio"
    a = to_s16(O.synthetic_audio(10 * HOP + 3000, seed=11))
    left = O.synthetic_audio(int(44100 * 9.7), seed=12)
    b = to_s16(np.stack([left, 0.5 * np.roll(left, 441)], axis=1))
    c = to_s16(O.synthetic_audio(9 * HOP + 8000, seed=13))
    write_wav(str(audio / "a.wav"), a, 16000)
    write_wav(str(audio / "site" / "b.wav"), b, 44100)
    write_wav(str(audio / "c.wav"), c, 16000)
    G.write_model_dir(str(root / "models" / "b"), G.glorot_layers([16, 3], ["relu", "linear"], seed=3), classes=["x", "ins_buzz", "z"],
                      digits_results=3)
    mp = pytest.MonkeyPatch()
    mp.setenv("BUZZDETECT_MODELS_DIR", str(root / "models"))
    stores = {}
    for codec in CODECS:
        rep = store.embed_recordings(str(audio), str(root / f"emb_{codec}"), codec=codec, chunklength=CHUNK, engine=engine)
        assert rep.written == ["a", "c", "site/b"] and rep.kept == [] and 25 <= rep.windows <= 35 and rep.messages == []
        stores[codec] = str(root / f"emb_{codec}")
    yield root, str(audio), stores
    mp.undo()


def same(a, b, where="result"):
    """Every value and message of two results: dataclasses field by field, arrays and tensors byte by byte."""
    import torch
    if isinstance(a, torch.Tensor):
        a, b = a.cpu().numpy(), b.cpu().numpy()
    if isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where
    elif dataclasses.is_dataclass(a) and not isinstance(a, type):
        assert type(a) is type(b), where
        for f in dataclasses.fields(a):
            same(getattr(a, f.name), getattr(b, f.name), f"{where}.{f.name}")
    elif isinstance(a, dict):
        assert list(a) == list(b), where
        for k in a:
            same(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{where}[{i}]")
    elif isinstance(a, float):
        assert isinstance(b, float) and (a == b or (a != a and b != b)), f"{where}: {a} != {b}"
    elif hasattr(a, "__dict__") and not callable(a):
        assert type(a) is type(b), where
        same(vars(a), vars(b), where)
    else:
        assert a == b, f"{where}: {a!r} != {b!r}"


@pytest.fixture()
def no_embedder(engine, monkeypatch):
    """The engine with an embedder that cannot launch and its launch counters running: what the store route may use is
    ``score_rows``."""
    def launch(*args, **kwargs):
        raise AssertionError("an embedder launch on the store route")
    reads = []

    def on():
        monkeypatch.setattr(engine, "launch", launch)
        engine.profile_enable(True)
        engine.profile_read()

    def off():
        monkeypatch.undo()
        _, counts = engine.profile_read()
        engine.profile_enable(False)
        reads.append(counts)
        assert not counts[:28].any(), f"launches in the CNN's slots: {counts}"
        return int(counts[28])
    yield on, off
    engine.profile_enable(False)


def test_score_store_writes_the_trees_analyze_writes(scene, engine, no_embedder):
    from buzzdetect_amd.analyze import analyze
    root, audio, stores = scene
    on, off = no_embedder
    for name, kw in (("act", {}), ("det", {"precision": 0.9}), ("buzz", {"classes_out": ["ins_buzz"]})):
        want = analyze("model_general_v3", chunklength=CHUNK, dir_audio=audio, dir_out=str(root / f"an_{name}"), engine=engine, **kw)
        on()
        got = store.score_store(stores["f32"], "model_general_v3", str(root / f"st_{name}"), engine=engine, **kw)
        assert off() > 0
        assert tree(root / f"st_{name}") == tree(root / f"an_{name}") and len(tree(root / f"st_{name}")) == 4
        assert (got.files_done, got.windows) == (want.files_done, want.windows) and got.files_done == 3 and 25 <= got.windows <= 35
    again = store.score_store(stores["f32"], "model_general_v3", str(root / "st_act"), engine=engine)
    assert (again.files_done, again.files_skipped, again.windows) == (0, 3, 0)
    with pytest.raises(RuntimeError, match="different settings"):
        store.score_store(stores["f32"], "model_general_v3", str(root / "st_act"), engine=engine, precision=0.9)
    names = ["model_general_v3", "b"]
    analyze(names, chunklength=CHUNK, dir_audio=audio, dir_out=str(root / "an_set"), analyzers_gpu=1)
    store.score_store(stores["f32"], names, str(root / "st_set"))
    want = tree(root / "an_set")
    assert tree(root / "st_set") == want and len(want) == 8 and sorted({os.path.dirname(p).split(os.sep)[0] for p in want}) == ["b", "model_general_v3"]
    assert tree(root / "st_set" / "model_general_v3") == tree(root / "an_act")


def test_tools_from_a_store_return_what_they_return_from_audio(scene, engine, no_embedder):
    from buzzdetect_amd import calls, cluster, evaluate, search
    root, audio, stores = scene
    on, off = no_embedder
    emb = stores["f32"]
    queries = search.queries_from_annotations(audio, NOTES, "ins_buzz", engine=engine, chunklength=CHUNK)
    assert queries.shape[0] >= 2 and queries.shape[1] == 1024
    rule = calls.Rule(-1.0, -2.0, 0.0, 0.0)
    tools = {
        "queries_from_annotations": lambda d: search.queries_from_annotations(d, NOTES, "ins_buzz", engine=engine, chunklength=CHUNK),
        "search_recordings": lambda d: search.search_recordings(d, queries[:2], k=7, engine=engine, chunklength=CHUNK),
        "top_windows": lambda d: search.top_windows(d, classes=["ins_buzz", "ambient_rain"], k=7, engine=engine, chunklength=CHUNK),
        "call_recordings": lambda d: calls.call_recordings(d, classes=["ins_buzz"], thresholds={"ins_buzz": -1.0}, low=-2.0, bin_s=5.0,
                                                           engine=engine, chunklength=CHUNK),
        "evaluate_recordings": lambda d: evaluate.evaluate_recordings(d, NOTES, classes=["ins_buzz"], rules={"ins_buzz": rule},
                                                                       only_annotated=False, engine=engine, chunklength=CHUNK),
        "cluster_recordings": lambda d: cluster.cluster_recordings(d, 3, engine=engine, chunklength=CHUNK, seed=4),
        "embed_annotated": lambda d: D.embed_annotated(d, NOTES, ["ambient_rain", "ins_buzz"], background="ambient_rain", engine=engine,
                                                       chunklength=CHUNK),
    }
    heads = {"top_windows", "call_recordings", "evaluate_recordings"}
    for name, tool in tools.items():
        want = tool(audio)
        on()
        got = tool(emb)
        launches = off()
        assert (launches > 0) == (name in heads), f"{name}: {launches} head launches"
        same(got, want, name)
    found = tools["cluster_recordings"](audio)
    centres = cluster.ClusterModel(found.centroids, found.metric, found.counts)
    want = cluster.assign_recordings(audio, centres, engine=engine, chunklength=CHUNK)
    on()
    got = cluster.assign_recordings(store.Store(emb), centres, engine=engine, chunklength=CHUNK)      # (a Store is taken as it is)
    assert off() == 0
    same(got, want, "assign_recordings")
    assert any("nowhere" in m for m in tools["evaluate_recordings"](emb).messages)


def test_refusals_and_resume(scene, engine):
    from buzzdetect_amd import search
    from buzzdetect_amd.engine import HipEngine
    root, audio, stores = scene
    emb = stores["f32"]
    with pytest.raises(ValueError, match=r"framehop_prop=1\.0, chunklength=4\.8; asked for framehop_prop=0\.5, chunklength=4\.8"):
        search.top_windows(emb, k=3, engine=engine, framehop_prop=0.5, chunklength=CHUNK)
    with pytest.raises(ValueError, match=r"chunklength=4\.8; asked for framehop_prop=1\.0, chunklength=199\.68"):
        search.search_recordings(emb, np.ones((1, 1024), np.float32), engine=engine)
    with pytest.raises(ValueError, match="embedding store"):
        D.augment(emb, NOTES, ["ambient_rain", "ins_buzz"], background="ambient_rain", engine=engine)
    blob = np.array(W.synthetic_embedder_blob(), np.float32)
    blob[1000] += 1.0
    other = HipEngine(embedder_blob=blob)
    try:
        assert other.weights_sha256 != engine.weights_sha256 and len(engine.weights_sha256) == 64
        with pytest.raises(ValueError, match="other embedder weights"):
            search.top_windows(emb, k=3, engine=other, chunklength=CHUNK)
    finally:
        other.close()
    with pytest.raises(ValueError, match="codec='f32'.*codec='h'"):
        store.embed_recordings(audio, emb, codec="h", chunklength=CHUNK, engine=engine)
    # resume: a second run writes nothing; a touched source and a stale .part are written again
    before = {p: os.stat(p).st_mtime_ns for p in (os.path.join(b, f) for b, _, fs in os.walk(emb) for f in fs if f.endswith(store.SUFFIX))}
    rep = store.embed_recordings(audio, emb, chunklength=CHUNK, engine=engine)
    assert rep.written == [] and rep.kept == ["a", "c", "site/b"] and rep.windows == 0
    assert before == {p: os.stat(p).st_mtime_ns for p in before} and len(before) == 3
    assert store.Store(emb).verify() == sum(r.windows for r in store.Store(emb).recordings)
    whole = open(os.path.join(emb, "c" + store.SUFFIX), "rb").read()
    os.utime(os.path.join(audio, "c.wav"), ns=(1, 1))
    open(os.path.join(emb, "c" + store.SUFFIX + ".part"), "wb").write(b"stale")
    rep = store.embed_recordings(audio, emb, chunklength=CHUNK, engine=engine)
    assert rep.written == ["c"] and rep.kept == ["a", "site/b"] and not os.path.exists(os.path.join(emb, "c" + store.SUFFIX + ".part"))
    now = open(os.path.join(emb, "c" + store.SUFFIX), "rb").read()
    assert len(now) == len(whole) and now[-4096:] == whole[-4096:] and now != whole       # the same rows under a new header
    # a damaged record is found when the rows are read on the device, and its slice named
    bad = root / "emb_bad"
    import shutil
    shutil.copytree(emb, bad)
    rec = store.Store(str(bad)).recordings[0]
    with open(rec.path, "r+b") as f:
        f.seek(rec.layout.records + 3 * 4096 + 40)
        f.write(b"\x01\x02\x03\x04")
    with pytest.raises(store.StoreError, match=r"a\.bdemb: slice 0 "):
        search.top_windows(str(bad), k=3, engine=engine, chunklength=CHUNK)


# ---------------------------------------------------------------------------------------------------- 4. lossy codecs
@pytest.mark.parametrize("codec", ("h", "b"))
def test_lossy_stores_stay_within_the_codec_bounds(scene, engine, codec, no_embedder):
    """The tools run from an h and a b store and the decoded rows lie within the codec's bounds of the f32 store's rows.  The
    largest logit deviation is printed, not gated; on an MI355X with the stand-in weights: 3.1e-3 under h, 7.0e-2 under b
    (DESIGN §27)."""
    from buzzdetect_amd import search
    root, audio, stores = scene
    exact, lossy = store.Store(stores["f32"]), store.Store(stores[codec])
    assert lossy.idents == exact.idents and lossy.parameters["codec"] == codec
    on, off = no_embedder
    on()
    worst = 0.0
    for ident in exact.idents:
        x = exact.rows(engine, ident)
        xh = lossy.rows(engine, ident)
        want, got = engine.score_rows(x).cpu().numpy(), engine.score_rows(xh).cpu().numpy()
        worst = max(worst, float(np.abs(got.astype(np.float64) - want).max()))
        x, xh = x.cpu().numpy().astype(np.float64), xh.cpu().numpy().astype(np.float64)
        assert x.shape == xh.shape and x.min() >= 0
        m = x.max(axis=1, keepdims=True)
        if codec == "h":
            assert (np.abs(xh - x) <= np.maximum(2.0 ** -11 * x, 2.0 ** -39 * m)).all()
        else:
            assert (np.abs(xh - x) <= m / 128).all()
        assert xh.astype(np.float32).tobytes() == lossy.recordings[lossy.idents.index(ident)].rows_host().tobytes()
    found = search.top_windows(stores[codec], classes=["ins_buzz"], k=5, engine=engine, chunklength=CHUNK)
    assert off() > 0 and len(found.hits[0]) == 5 and found.messages == []
    print(f"codec {codec}: largest logit deviation from the f32 store {worst:.3g}")
    assert np.isfinite(worst)
