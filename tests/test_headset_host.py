"""The set of heads without a device (include/buzzdetect_headset.h): header, binding and exports agree; every refusal of
HipEngine(modelname=[...]) / analyze(modelname=[...]) is a ValueError raised before any device work; the planner groups the
members of a set by the chunks their own result files still lack; every model's folder takes that model's own manifest."""
import ctypes as C
import json
import os
import re
import wave

import numpy as np
import pytest

from buzzdetect_amd import _lib, build, modeldir as G, pipeline as P, results as R, weights as W

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def declared(header):
    text = open(os.path.join(INCLUDE, header)).read()
    return sorted(set(re.findall(r"^BD_API[^;(]*?\b(bd_[a-z_0-9]+)\s*\(", text, flags=re.M)))


# ---------------------------------------------------------------------------------------------------- the ABI
def test_header_binding_and_library_list_the_same_functions():
    build.build(verbose=False)
    lib = _lib.load()
    names = declared("buzzdetect_headset.h")
    assert names == sorted(_lib.HEADSET_PROTOTYPES) and len(names) == 5
    raw = C.CDLL(_lib.library_path())
    for name in names:
        assert hasattr(raw, name), f"{name} not exported"
    assert lib.bd_headset_abi_version() == _lib.HEADSET_ABI_VERSION == 1
    text = open(os.path.join(INCLUDE, "buzzdetect_headset.h")).read()
    assert re.search(r"#define\s+BD_HEADSET_ABI_VERSION\s+1\b", text)
    assert int(re.search(r"#define\s+BD_HEADSET_MAX_MEMBERS\s+(\d+)", text).group(1)) == _lib.HEADSET_MAX_MEMBERS == W.HEADSET_MAX_MEMBERS
    assert _lib.HEADSET_ROW == W.HEADSET_ROW == _lib.HEAD_MAX_WIDTH
    # nothing went into the main header
    assert lib.bd_abi_version() == 5 and len(declared("buzzdetect_hip.h")) == 44 == len(_lib.PROTOTYPES)
    assert C.sizeof(_lib.bd_headset_member) == 16


# ---------------------------------------------------------------------------------------------------- the engine's refusals
def head(widths, acts, seed=1, embedder="yamnet_k2", classes=None):
    layers = G.glorot_layers(widths, acts, seed=seed)
    return W.HeadWeights(layers, classes or [f"c{i}" for i in range(widths[-1])], embeddername=embedder)


@pytest.fixture()
def no_device(monkeypatch):
    """Anything that would touch the library or a device fails the test."""
    import torch
    from buzzdetect_amd import engine as E

    def touched(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    monkeypatch.setattr(E._lib, "load", touched)
    monkeypatch.setattr(torch.cuda, "is_available", touched)
    monkeypatch.setattr(W, "load_embedder_blob", touched)
    return E.HipEngine


def test_an_empty_list_is_refused(no_device):
    with pytest.raises(ValueError, match="empty"):
        no_device(modelname=[])
    with pytest.raises(ValueError, match="at least one"):
        no_device(heads={})


def test_a_name_given_twice_is_refused(no_device, tmp_path):
    G.write_model_dir(str(tmp_path / "a"), G.glorot_layers([3], ["linear"], seed=1))
    with pytest.raises(ValueError, match="given twice: a"):
        no_device(modelname=["a", "b", "a"], models_dir=str(tmp_path))


def test_members_on_different_embedders_are_refused_naming_both(no_device):
    heads = {"mine": head([3], ["linear"]), "theirs": head([3], ["linear"], embedder="yamnet")}
    with pytest.raises(ValueError, match=r"'mine' is on 'yamnet_k2', 'theirs' on 'yamnet'"):
        no_device(heads=heads)


def hidden(n, width=128):
    return {f"m{i:02d}": head([width, 2], ["relu", "linear"], seed=i) for i in range(n)}


def test_the_hidden_widths_of_one_depth_may_sum_to_2048():
    assert list(W.check_head_set(hidden(16)).values())[-1] == slice(30, 32)          # 16 x 128 = 2048: accepted
    heads = hidden(16)
    heads["one_more"] = head([1, 2], ["relu", "linear"])                             # + 32 (1 rounded up) = 2080
    with pytest.raises(ValueError, match=r"depth 0: .* sum to 2080, more than 2048"):
        W.check_head_set(heads)
    with pytest.raises(ValueError, match=r"depth 0: .* sum to 2176, more than 2048"):
        W.check_head_set(hidden(17))
    # a last layer in front of a softmax counts at its depth; one linear layer of at most 64 outputs (the fused route) does not
    soft = {f"s{i:02d}": head([33], ["softmax"], seed=i) for i in range(32)}           # 32 x 64 (33 rounded up) = 2048
    soft["fused"] = head([64], ["linear"])
    assert W.check_head_set(soft)["fused"] == slice(32 * 33, 32 * 33 + 64)
    with pytest.raises(ValueError, match=r"depth 0: .* sum to 2080, more than 2048"):
        W.check_head_set({**soft, "one_more": head([1], ["softmax"])})


def test_the_engine_refuses_the_sums_before_any_device_work(no_device):
    with pytest.raises(ValueError, match="sum to 2176"):
        no_device(heads=hidden(17))
    wide = {"a": head([1024], ["sigmoid"]), "b": head([1024], ["sigmoid"], seed=2)}
    assert W.check_head_set(wide)["b"] == slice(1024, 2048)                          # 2048 outputs: accepted
    wide["c"] = head([1], ["linear"])
    with pytest.raises(ValueError, match="outputs sum to 2049, more than 2048"):
        no_device(heads=wide)
    with pytest.raises(ValueError, match="at most 64"):
        no_device(heads={f"m{i}": head([1], ["linear"]) for i in range(65)})
    with pytest.raises(ValueError, match="not both"):
        no_device(head=head([1], ["linear"]), heads={"a": head([1], ["linear"])})


# ---------------------------------------------------------------------------------------------------- analyze()'s refusals
@pytest.fixture()
def models(tmp_path):
    root = tmp_path / "models"
    G.write_model_dir(str(root / "a"), G.glorot_layers([13], ["linear"], seed=1))                     # has ins_buzz
    G.write_model_dir(str(root / "b"), G.glorot_layers([2], ["linear"], seed=2), classes=["ins_buzz", "other"], digits_results=3)
    G.write_model_dir(str(root / "c"), G.glorot_layers([16, 3], ["relu", "linear"], seed=3), classes=["x", "y", "z"])
    return str(root)


def test_analyze_refuses_before_any_device_work(models, tmp_path, monkeypatch):
    from buzzdetect_amd import analyze as A
    from buzzdetect_amd import engine as E

    def touched(*a, **k):
        raise AssertionError("an engine was built before the arguments were checked")
    monkeypatch.setattr(E, "HipEngine", touched)
    out = tmp_path / "out"
    common = dict(dir_audio=str(tmp_path), dir_out=str(out), dir_models=models)
    with pytest.raises(ValueError, match=r"model 'c' has no class 'ins_buzz'"):
        A.analyze(["a", "b", "c"], classes_out=["ins_buzz"], **common)
    with pytest.raises(ValueError, match="gather_logits"):
        A.analyze(["a", "b"], gather_logits=True, **common)
    with pytest.raises(ValueError, match="empty"):
        A.analyze([], **common)
    with pytest.raises(ValueError, match="given twice"):
        A.analyze(["a", "a"], **common)
    assert not out.exists()                                # nothing was written, not even a manifest

    class Carries:
        def __init__(self, members):
            self.members, self.head = members, None
    heads = W.load_head_set(["a", "b"], models)
    with pytest.raises(ValueError, match="must carry the models"):
        A.analyze(["a", "b"], engine=Carries(dict(reversed(list(heads.items())))), **common)
    with pytest.raises(ValueError, match="must carry the models"):
        A.analyze(["a", "b"], engines=[Carries(heads), Carries(None)], **common)
    with pytest.raises(ValueError, match="name the same models as a list"):
        A.analyze("a", engine=Carries(heads), **common)    # one name, but the engine carries a set
    assert not out.exists()


# ---------------------------------------------------------------------------------------------------- folders and manifests
def test_every_model_writes_to_its_own_folder(tmp_path):
    from buzzdetect_amd.analyze import member_dirs
    assert member_dirs(["a", "b"], None) == {"a": os.path.join("models", "a", "output"), "b": os.path.join("models", "b", "output")}
    assert member_dirs(["a", "b"], str(tmp_path)) == {"a": str(tmp_path / "a"), "b": str(tmp_path / "b")}


def test_a_members_folder_is_accepted_under_its_lone_manifest(models, tmp_path):
    from buzzdetect_amd.analyze import member_dirs, set_members
    heads = W.load_head_set(["a", "b"], models)
    members = set_members(heads, "all", None)
    assert [(m.name, m.columns, m.digits_results, m.threshold) for m in members] == [("a", slice(0, 13), 2, None),
                                                                                     ("b", slice(13, 15), 3, None)]
    assert members[1].classes == ["ins_buzz", "other"] == members[1].classes_out
    dirs = member_dirs(["a", "b"], str(tmp_path / "out"))
    for m in members:                                      # what _analyze_set writes ...
        assert R.check_or_write_manifest(dirs[m.name], R.build_manifest(m.name, 1, None, m.classes_out)) == (True, None)
    # ... is what a run with the model alone builds (analyze(): classes_out "all" -> the model's classes), and the other way round
    lone = R.build_manifest("a", 1, None, list(heads["a"].classes))
    assert R.check_or_write_manifest(dirs["a"], lone) == (True, None)
    assert json.load(open(os.path.join(dirs["a"], R.MANIFEST_NAME))) == lone
    ok, msg = R.check_or_write_manifest(dirs["a"], R.build_manifest("b", 1, None, ["ins_buzz", "other"]))
    assert not ok and "modelname" in msg
    # detection mode: every member's threshold from its own metrics
    det = set_members(heads, "all", 0.9)
    assert all(m.threshold == R.threshold_for_precision(m.name, 0.9, metrics_path=heads[m.name].metrics_path) for m in det)
    assert np.isfinite(det[0].threshold)


# ---------------------------------------------------------------------------------------------------- the planner
DURATION = 25.0


@pytest.fixture()
def planner(tmp_path):
    with wave.open(str(tmp_path / "rec.wav"), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.zeros(int(16000 * DURATION), "<i2").tobytes())
    members = [P.Member(n, slice(i, i + 1), ["k"], ["k"], 2, None) for i, n in enumerate("abc")]
    pipe = P.Pipeline(make_engine=None, classes=["a/k", "b/k", "c/k"], framehop_s=0.96, hop=15360, step=96, chunklength=9.6,
                      framelength_s=0.96, digits_time=2, digits_results=2, classes_out="all", threshold=None, readers=1,
                      analyzers=1, pin_memory=False, members=members)

    def job():
        from buzzdetect_amd.analyze import set_jobs
        return set_jobs([(str(tmp_path / "rec.wav"), "rec")], members, {n: str(tmp_path / "out" / n) for n in "abc"})[0]

    def write(name, suffix, starts):
        path = tmp_path / "out" / name / ("rec" + suffix)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text("start,activation_k\n" + "".join(f"{s:.2f},0.5\n" for s in starts))
    return pipe, job, write


ALL = [(0.0, 9.6), (9.6, 19.2), (19.2, 25.0)]
EVERY_START = [round(0.96 * i, 2) for i in range(26)]


def planned(pipe, job):
    out = pipe.plan(job)
    for j, _ in out:
        j.track.close()
    return [([pipe.members[mf.member].name for mf in j.outputs], [(round(a, 2), round(b, 2)) for a, b in chunks]) for j, chunks in out]


def test_fresh_members_share_one_job(planner):
    pipe, job, _ = planner
    j = job()
    assert planned(pipe, j) == [(["a", "b", "c"], ALL)]
    assert all(mf.fresh for mf in j.outputs) and j.rf is j.outputs[0].rf and j.siblings == [1, 0]


def test_a_finished_member_is_left_out(planner):
    pipe, job, write = planner
    write("b", R.SUFFIX_COMPLETE, EVERY_START)
    assert planned(pipe, job()) == [(["a", "c"], ALL)]


def test_a_member_with_a_partial_file_gets_a_job_of_its_own(planner):
    pipe, job, write = planner
    write("c", R.SUFFIX_PARTIAL, EVERY_START[:10])         # chunk 0's rows
    j = job()
    out = pipe.plan(j)
    got = [([pipe.members[mf.member].name for mf in k.outputs], [(round(a, 2), round(b, 2)) for a, b in chunks]) for k, chunks in out]
    assert got == [(["a", "b"], ALL), (["c"], ALL[1:])]
    first, second = out[0][0], out[1][0]
    assert first is j and second is not j and second.path == j.path and second.ident == "rec"
    assert first.siblings is second.siblings and first.siblings == [2, 0]
    assert first.track is not second.track and second.rf is second.outputs[0].rf
    assert [mf.fresh for mf in first.outputs] == [True, True] and [mf.fresh for mf in second.outputs] == [False]
    first.track.close()
    second.track.close()


def test_a_recording_finished_for_every_member_is_not_opened(planner, monkeypatch):
    pipe, job, write = planner
    for name in "abc":
        write(name, R.SUFFIX_COMPLETE, EVERY_START)

    def opened(path):
        raise AssertionError("the recording was opened")
    monkeypatch.setattr(P, "open_track", opened)
    assert pipe.plan(job()) == [] and pipe.report.files_skipped == 1


def test_jobs_without_members_plan_as_before(planner, tmp_path):
    pipe, _, _ = planner
    lone = P.FileJob(str(tmp_path / "rec.wav"), "rec", "rec.wav", R.ResultFile(str(tmp_path / "lone" / "rec")))
    out = pipe.plan(lone)
    assert len(out) == 1 and out[0][0] is lone and lone.outputs is None and [tuple(map(float, c)) for c in out[0][1]] == ALL
    lone.track.close()
