"""analyze(modelname=[...]) on the GPU: every recording is embedded once and every model's result tree is, byte for byte, the
tree a run with that model alone writes - activations and detections, a classes_out list, resume per member, the stop event."""
import os
import threading
import wave

import numpy as np
import pytest

from buzzdetect_amd import modeldir as G
from oracle import yamnet_oracle as O

pytestmark = pytest.mark.gpu

NAMES = ["model_general_v3", "b", "c"]                  # the packaged head, a one-layer 2-class head, a 1024 -> 16 -> 3 stack
RECORDINGS = ("one", os.path.join("site", "two"))       # three chunks each at chunklength 9.6 s
CHUNK = 9.6


def write_wav(path, x, rate=16000):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes((np.clip(x, -1, 1 - 2 ** -15) * 32768.0).round().astype("<i2").tobytes())


def tree(root):
    """{relative path: bytes} of every result file under root."""
    out = {}
    for base, _, files in os.walk(root):
        for f in files:
            if f.endswith(".csv"):
                p = os.path.join(base, f)
                out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def mtimes(root):
    return {os.path.relpath(os.path.join(b, f), root): os.stat(os.path.join(b, f)).st_mtime_ns
            for b, _, files in os.walk(root) for f in files if f.endswith((".csv", ".json"))}


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """Audio, models and the three lone runs every test compares against (computed once, never changed)."""
    from buzzdetect_amd.analyze import analyze
    root = tmp_path_factory.mktemp("headset_analyze")
    models = root / "models"
    G.write_model_dir(str(models / "b"), G.glorot_layers([2], ["linear"], seed=2), classes=["ins_buzz", "other"], digits_results=3)
    G.write_model_dir(str(models / "c"), G.glorot_layers([16, 3], ["relu", "linear"], seed=3), classes=["x", "ins_buzz", "z"])
    G.write_model_dir(str(models / "d"), G.glorot_layers([2], ["linear"], seed=4), classes=["p", "q"])       # no ins_buzz
    for k, rel in enumerate(RECORDINGS):
        write_wav(str(root / "audio" / (rel + ".wav")), O.synthetic_audio(16000 * 25, seed=40 + k))
    mp = pytest.MonkeyPatch()
    mp.setenv("BUZZDETECT_MODELS_DIR", str(models))     # the packaged model stays reachable beside the generated ones
    lone = {}
    for mode, kw in (("act", {}), ("det", {"precision": 0.9}), ("buzz", {"classes_out": ["ins_buzz"]})):
        for name in NAMES:
            out = root / f"lone_{mode}" / name
            rep = analyze(name, chunklength=CHUNK, dir_audio=str(root / "audio"), dir_out=str(out), analyzers_gpu=1, **kw)
            assert rep.files_done == 2 and rep.chunks == 6
            lone[mode, name] = (rep, tree(out), open(out / "buzzdetect_manifest.json").read())
    yield root, lone
    mp.undo()


def run_set(root, out, names=NAMES, **kw):
    from buzzdetect_amd.analyze import analyze
    return analyze(names, chunklength=CHUNK, dir_audio=str(root / "audio"), dir_out=str(out), analyzers_gpu=1, **kw)


def rows_of(lone, rel, name="c"):
    return len(lone["act", name][1][rel + "_buzzdetect.csv"].splitlines()) - 1


def assert_trees_equal(out, lone, mode, names=NAMES):
    for name in names:
        _, files, manifest = lone[mode, name]
        assert sorted(files) == sorted(r + "_buzzdetect.csv" for r in RECORDINGS)
        assert tree(out / name) == files, f"{name}: the set's tree differs from the lone run's"
        assert open(out / name / "buzzdetect_manifest.json").read() == manifest


def test_one_pass_writes_every_models_tree(scene):
    from buzzdetect_amd.analyze import analyze
    root, lone = scene
    out = root / "set_act"
    rep = run_set(root, out)
    assert_trees_equal(out, lone, "act")
    one = lone["act", "b"][0]
    assert (rep.windows, rep.chunks) == (one.windows, one.chunks) == (rows_of(lone, "one") + rows_of(lone, RECORDINGS[1]), 6)
    assert rep.audio_seconds == pytest.approx(one.audio_seconds) == pytest.approx(50.0)      # once, not three times
    assert rep.files_done == 2 and rep.files_total == 2 and rep.end_reason == "completed"
    # the digits are each model's own: b writes three decimals
    assert lone["act", "b"][1]["one_buzzdetect.csv"] != lone["act", "c"][1]["one_buzzdetect.csv"]
    # a lone run on a member's folder accepts the manifest and finds nothing to do
    before = mtimes(out)
    again = analyze("b", chunklength=CHUNK, dir_audio=str(root / "audio"), dir_out=str(out / "b"), analyzers_gpu=1)
    assert again.files_done == 0 and again.chunks == 0 and again.files_skipped == 2
    assert mtimes(out) == before and tree(out / "b") == lone["act", "b"][1]
    # ... and the other way round: the set over the lone runs' folders has nothing left to do either
    rerun = run_set(root, out)
    assert rerun.chunks == 0 and rerun.files_skipped == 2 and mtimes(out) == before


def test_detections_use_every_models_own_threshold(scene):
    root, lone = scene
    out = root / "set_det"
    run_set(root, out, precision=0.9)
    assert_trees_equal(out, lone, "det")
    assert lone["det", "c"][1]["one_buzzdetect.csv"].startswith(b"start,detections_ins_buzz\n")


def test_a_classes_out_list_applies_to_every_model(scene):
    root, lone = scene
    out = root / "set_buzz"
    run_set(root, out, classes_out=["ins_buzz"])
    assert_trees_equal(out, lone, "buzz")
    bad = root / "set_bad"
    with pytest.raises(ValueError, match="model 'd' has no class 'ins_buzz'"):
        run_set(root, bad, names=["b", "d"], classes_out=["ins_buzz"])
    assert not bad.exists() or not tree(bad)


def test_resume_is_per_member(scene):
    root, lone = scene
    out = root / "set_resume"
    run_set(root, out)
    # member b lost one complete file: only that file comes back
    victim = out / "b" / "one_buzzdetect.csv"
    victim.unlink()
    before = mtimes(out)
    rep = run_set(root, out)
    assert rep.chunks == 3 and rep.windows == rows_of(lone, "one") and rep.files_done == 1 and rep.files_skipped == 1
    after = mtimes(out)
    assert set(after) == set(before) | {os.path.join("b", "one_buzzdetect.csv")}
    assert all(after[k] == v for k, v in before.items())
    assert_trees_equal(out, lone, "act")
    # member c's file becomes a partial file with chunk 0's rows only, cut from the lone run
    rel = os.path.join("site", "two")
    whole = lone["act", "c"][1][rel + "_buzzdetect.csv"].splitlines(keepends=True)
    assert whole[10].startswith(b"8.64,") and whole[11].startswith(b"9.6,")      # chunk 0 is ten windows
    (out / "c" / (rel + "_buzzdetect.csv")).unlink()
    (out / "c" / (rel + "_buzzpart.csv")).write_bytes(b"".join(whole[:1 + 10]))
    rep = run_set(root, out)
    assert rep.chunks == 2 and rep.windows == len(whole) - 11 and rep.files_done == 1
    assert_trees_equal(out, lone, "act")


def test_the_stop_event_leaves_every_member_resumable(scene, monkeypatch):
    """The event is set by the first append of the first chunk; the reader holds every later chunk until the pipeline has seen
    it, so exactly one chunk is written - for every member."""
    from buzzdetect_amd import pipeline as P
    from buzzdetect_amd import results as R
    root, lone = scene
    out = root / "set_stop"
    stop = threading.Event()
    seen = {"pipe": None, "reads": 0, "appends": 0}
    real_append, real_read, real_run = R.ResultFile.append_text, P.ReaderStage.read, P.Pipeline.run

    def append(self, head, body):
        real_append(self, head, body)
        seen["appends"] += 1
        stop.set()

    def read(self, fd, off, n, dev):
        seen["reads"] += 1
        if seen["reads"] > 1:
            assert seen["pipe"].aborted.wait(60), "the stop event never reached the pipeline"
        return real_read(self, fd, off, n, dev)

    def run(self, jobs):
        seen["pipe"] = self
        return real_run(self, jobs)

    monkeypatch.setattr(R.ResultFile, "append_text", append)
    monkeypatch.setattr(P.ReaderStage, "read", read)
    monkeypatch.setattr(P.Pipeline, "run", run)
    rep = run_set(root, out, n_streamers=1, stream_buffer_depth=1, event_stopanalysis=stop)
    assert rep.end_reason == "interrupted" and rep.files_done == 0
    assert seen["appends"] == 3                          # one chunk, three members
    parts = sorted(os.path.relpath(p, out) for p in map(str, out.rglob("*_buzzpart.csv")))
    assert len(parts) == 3 and not list(out.rglob("*_buzzdetect.csv"))
    monkeypatch.undo()
    again = run_set(root, out)
    assert again.end_reason == "completed" and again.chunks == 5 and again.files_done == 2
    assert_trees_equal(out, lone, "act")
    assert not list(out.rglob("*_buzzpart.csv"))
