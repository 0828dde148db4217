"""analyze() with an ensemble on the GPU: an ensemble's model directory is analysed like any model - its tree is the CSV of the
combined rows, under its own manifest, classes, digits and threshold - and in a list of models its tree is byte for byte the lone
run's.  Then the whole workflow once: cross_validate_head -> save_ensemble -> HipEngine(modelname=...) -> predict, and the
drop-in plugin."""
import ctypes as C
import os
import wave

import numpy as np
import pytest

from buzzdetect_amd import _lib, framing, modeldir as G, results as R, train as T, weights as W
from oracle import yamnet_oracle as O

pytestmark = pytest.mark.gpu

CHUNK = 2.88
SECONDS = 7.0                                           # chunks of 3, 3 and 2 windows
WAVS = ("one", os.path.join("site", "two"))
CLASSES = ["x", "ins_buzz", "z"]
NAMES = ["model_cv", "model_general_v3"]
MODES = {"act": {}, "det": {"precision": 0.9}, "buzz": {"classes_out": ["ins_buzz"]}}


def write_wav(path, x, rate=16000):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes((np.clip(x, -1, 1 - 2 ** -15) * 32768.0).round().astype("<i2").tobytes())


def quantised(x):
    return (np.clip(x, -1, 1 - 2 ** -15) * 32768.0).round().astype(np.int16).astype(np.float32) / 32768.0


def tree(root):
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


def mean_host(member_rows):
    """bd_ensemble_combine_host, `mean`, of [rows of member 0, rows of member 1, ...]."""
    k, (n, c) = len(member_rows), member_rows[0].shape
    wide = np.ascontiguousarray(np.concatenate(member_rows, axis=1), dtype=np.float32)
    outs = (_lib.bd_ensemble_output * 1)()
    outs[0].first_member, outs[0].n_members, outs[0].combine = 0, k, _lib.COMBINE_KINDS["mean"]
    mf = (C.c_int32 * (k + 1))(*[c * m for m in range(k + 1)])
    out = np.empty((n, c), np.float32)
    _lib.check(_lib.load().bd_ensemble_combine_host(wide.ctypes.data, n, k * c, outs, 1, mf, out.ctypes.data, c))
    return out


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """Audio (two WAVs, one 44.1 kHz stereo FLAC), the ensemble `model_cv` = the mean of three folds, the combined rows of every
    chunk of the WAVs (from the folds as a plain set, combined on the host), and the lone runs of both models in three modes."""
    from buzzdetect_amd.analyze import analyze
    from buzzdetect_amd.engine import HipEngine
    from tools import flacgen
    root = tmp_path_factory.mktemp("ensemble_analyze")
    folds = {f"fold{i}": W.HeadWeights(G.glorot_layers([3], ["linear"], seed=80 + i), CLASSES) for i in range(3)}
    audio = {rel: O.synthetic_audio(int(16000 * SECONDS), seed=60 + k) for k, rel in enumerate(WAVS)}
    for rel, x in audio.items():
        write_wav(str(root / "audio" / (rel + ".wav")), x)
    (root / "audio" / "stereo.flac").write_bytes(flacgen.encode(flacgen.test_signal(int(44100 * 5.3), 2, 16, seed=4), 44100, 16,
                                                                blocksize=4608, mode="mid_side"))
    chunks = framing.gaps_to_chunklist([(0, SECONDS)], CHUNK)
    combined = {}
    plain = HipEngine(modelname=None, heads=folds)
    try:
        for rel, x in audio.items():
            for chunk in chunks:
                a, b = framing.chunk_sample_range(chunk, 16000)
                parts = plain.split(plain.predict(quantised(x)[a:b], 0.96))
                combined[rel, chunk] = mean_host([np.ascontiguousarray(parts[n]) for n in folds])
    finally:
        plain.close()
    buzz = np.concatenate([rows[:, 1] for rows in combined.values()])
    threshold = round(float(np.median(buzz)), 2)        # splits these recordings' windows; the packaged model's is another
    table = T.METRICS_HEADER + f"\n{threshold - 1},0.5,0.9,0.1\n{threshold},0.9,0.5,0.01\n{threshold + 1},0.99,0.1,0.001\n"
    T.save_ensemble(str(root / "models" / "model_cv"), list(folds.values()), names=list(folds), metrics=table)
    mp = pytest.MonkeyPatch()
    mp.setenv("BUZZDETECT_MODELS_DIR", str(root / "models"))
    lone = {}
    for mode, kw in MODES.items():
        for name in NAMES:
            out = root / f"lone_{mode}" / name
            rep = analyze(name, chunklength=CHUNK, dir_audio=str(root / "audio"), dir_out=str(out), analyzers_gpu=1, **kw)
            assert rep.files_done == 3 and rep.end_reason == "completed"
            lone[mode, name] = (rep, tree(out), open(out / "buzzdetect_manifest.json").read())
    yield root, lone, combined, chunks, threshold
    mp.undo()


def expected_csv(combined, chunks, rel, threshold=None, classes_out="all"):
    head, parts = b"", []
    for chunk in chunks:
        rows = combined[rel, chunk]
        if threshold is None:
            head, body = R.activation_csv(rows, CLASSES, 0.96, 2, chunk[0], classes_out, 2)
        else:
            head, body = R.detection_csv(rows, threshold, CLASSES, 0.96, 2, chunk[0])
        parts.append(body)
    return head + b"".join(parts)


def test_an_ensembles_tree_is_the_csv_of_the_combined_rows(scene):
    root, lone, combined, chunks, threshold = scene
    assert len(chunks) == 3 and [combined[WAVS[0], c].shape[0] for c in chunks] == [3, 3, 2]
    for rel in WAVS:
        assert lone["act", "model_cv"][1][rel + "_buzzdetect.csv"] == expected_csv(combined, chunks, rel)
        assert lone["buzz", "model_cv"][1][rel + "_buzzdetect.csv"] == expected_csv(combined, chunks, rel, classes_out=["ins_buzz"])
        assert lone["det", "model_cv"][1][rel + "_buzzdetect.csv"] == expected_csv(combined, chunks, rel, threshold=threshold)
    assert lone["act", "model_cv"][1]["one_buzzdetect.csv"].startswith(b"start,activation_x,activation_ins_buzz,activation_z\n")
    assert "stereo_buzzdetect.csv" in lone["act", "model_cv"][1]
    # the manifest is the ensemble's own: its name, its classes
    import json
    manifest = json.loads(lone["act", "model_cv"][2])
    assert manifest == R.build_manifest("model_cv", 1, None, CLASSES)


def test_precision_takes_the_threshold_from_the_ensembles_own_metrics(scene):
    root, lone, combined, chunks, threshold = scene
    path = W.load_head("model_cv").metrics_path
    assert path == str(root / "models" / "model_cv" / "tests" / "metrics.csv")
    assert R.threshold_for_precision("model_cv", 0.9, metrics_path=path) == threshold
    assert threshold != R.threshold_for_precision("model_general_v3", 0.9)
    det = b"".join(lone["det", "model_cv"][1][rel + "_buzzdetect.csv"] for rel in WAVS)
    assert det.count(b",1\n") > 0 and det.count(b",0\n") > 0          # the median splits the windows


@pytest.mark.parametrize("mode", sorted(MODES))
def test_a_list_with_an_ensemble_writes_the_lone_runs_trees(scene, mode):
    from buzzdetect_amd.analyze import analyze
    root, lone, _, _, _ = scene
    out = root / f"set_{mode}"
    common = dict(chunklength=CHUNK, dir_audio=str(root / "audio"), analyzers_gpu=1, **MODES[mode])
    rep = analyze(NAMES, dir_out=str(out), **common)
    assert rep.files_done == 3 and rep.end_reason == "completed" and rep.chunks == lone[mode, "model_cv"][0].chunks
    for name in NAMES:
        _, files, manifest = lone[mode, name]
        assert len(files) == 3 and tree(out / name) == files, f"{name}: the set's tree differs from the lone run's"
        assert open(out / name / "buzzdetect_manifest.json").read() == manifest
    if mode == "act":
        # a lone run over the set's folders accepts the manifests and rewrites nothing, and the other way round
        before = mtimes(out)
        for name in NAMES:
            again = analyze(name, dir_out=str(out / name), **common)
            assert again.files_done == 0 and again.chunks == 0 and again.files_skipped == 3
        rerun = analyze(NAMES, dir_out=str(out), **common)
        assert rerun.chunks == 0 and rerun.files_skipped == 3 and mtimes(out) == before
        # resume is per name: the ensemble lost one file, only that one comes back
        (out / "model_cv" / "one_buzzdetect.csv").unlink()
        rep = analyze(NAMES, dir_out=str(out), **common)
        assert rep.chunks == 3 and rep.files_done == 1 and rep.files_skipped == 2
        after = mtimes(out)
        assert all(after[k] == v for k, v in before.items() if k != os.path.join("model_cv", "one_buzzdetect.csv"))
        assert tree(out / "model_cv") == lone["act", "model_cv"][1]


def test_cross_validation_to_predictions(tmp_path):
    """cross_validate_head -> save_ensemble -> HipEngine(modelname=...) -> predict: the host combine of the three folds' lone
    predictions, by bytes."""
    from buzzdetect_amd.engine import HipEngine
    rng = np.random.default_rng(3)
    n, classes = 200, ["ambient", "ins_buzz"]
    targets = rng.choice(2, n, p=[0.6, 0.4]).astype(np.int32)
    x = (np.maximum(rng.normal(size=(n, 1024)), 0) * 0.5).astype(np.float32)
    x[np.arange(n), targets] += 1.0
    cv = T.cross_validate_head(x, targets, classes, folds=3, epochs=2, batch_size=64, seed=1)
    entry = cv.entries[cv.best]
    assert len(entry.fits) == 3
    path = T.save_ensemble(str(tmp_path / "models" / "model_cv"), entry.fits, metrics=entry.metrics("ins_buzz"))
    audio = O.synthetic_audio(15360 * 5 + 240, seed=9)
    eng = HipEngine(modelname="model_cv", models_dir=str(tmp_path / "models"))
    try:
        assert isinstance(eng.head, W.EnsembleWeights) and eng.classes == classes and list(eng.head.members) == ["member0", "member1", "member2"]
        got = eng.predict(audio, 0.96).numpy().copy()
    finally:
        eng.close()
    alone = []
    for k, fit in enumerate(entry.fits):
        lone = HipEngine(modelname=f"member{k}", models_dir=os.path.join(path, "members"))
        try:
            assert np.array_equal(lone.head.kernel, fit.head.kernel)
            alone.append(lone.predict(audio, 0.96).numpy().copy())
        finally:
            lone.close()
    assert got.shape == (5, 2) and got.tobytes() == mean_host(alone).tobytes()
    assert not np.array_equal(alone[0], alone[1])
    assert np.isfinite(R.threshold_for_precision("model_cv", 0.5, tolerance=1.0, metrics_path=eng.head.metrics_path))


def test_the_plugin_of_an_ensemble_predicts_through_the_overlay(dropin_cwd, tmp_path, monkeypatch):
    from src import config as cfg
    from src.inference.models import load_model
    from buzzdetect_amd.engine import HipEngine
    models = tmp_path / "models"
    folds = [W.HeadWeights(G.glorot_layers([24, 4], ["relu", "linear"], seed=90 + i), ["a", "b", "ins_buzz", "d"]) for i in range(2)]
    T.save_ensemble(str(models / "model_cv"), folds, combine="mean_probability", link="softmax", digits_results=4)
    monkeypatch.setattr(cfg, "DIR_MODELS", str(models))
    monkeypatch.setenv("BUZZDETECT_MODELS_DIR", str(models))
    model = load_model("model_cv", framehop_prop=1.0, initialize=True)
    assert type(model).__name__ == "Model" and model.digits_results == 4 and model.config["classes"] == ["a", "b", "ins_buzz", "d"]
    x = O.synthetic_audio(15360 * 5 + 240, seed=11)
    got = model.predict(x).numpy()
    eng = HipEngine(modelname="model_cv", models_dir=str(models))
    try:
        ref = eng.predict(x, 0.96).numpy()
    finally:
        eng.close()
    assert got.shape == (5, 4) and got.tobytes() == ref.tobytes()
    assert np.allclose(np.exp(got.astype(np.float64)).sum(1), 1.0, atol=1e-5)       # the log of a mean of softmaxes
