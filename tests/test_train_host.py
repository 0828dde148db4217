"""The head trainer's host side (buzzdetect_amd/train.py, buzzdetect_amd/modeldir.py) and the restatement the GPU tests
compare with (tests/train_oracle.py): no GPU needed."""
import hashlib
import os

import numpy as np
import pytest

from buzzdetect_amd import modeldir, results, train, weights
from tests import train_oracle as T
from tools import modelgen as G


def tanh_stack(rng):
    return [(rng.normal(0, 0.05, (1024, 5)), rng.normal(0, 0.1, 5), "tanh"), (rng.normal(0, 0.5, (5, 3)), rng.normal(0, 0.1, 3), "linear")]


@pytest.mark.parametrize("loss", ("categorical", "binary"))
def test_the_restatements_gradients_match_central_differences(loss):
    rng = np.random.default_rng(5)
    layers = tanh_stack(rng)
    x = np.maximum(rng.normal(size=(7, 1024)), 0) * 0.5
    targets = rng.integers(0, 3, 7) if loss == "categorical" else rng.integers(0, 2, (7, 3)).astype(np.float64)
    _, grads = T.gradients(layers, x, targets, loss)
    h, worst = 1e-6, 0.0
    for li in range(2):
        for pi in range(2):
            p, g = layers[li][pi], grads[li][pi]
            flat = [np.unravel_index(i, p.shape) for i in rng.choice(p.size, min(p.size, 40), replace=False)]
            for at in flat:
                keep = p[at]
                p[at] = keep + h
                up = T.mean_loss(layers, x, targets, loss)
                p[at] = keep - h
                down = T.mean_loss(layers, x, targets, loss)
                p[at] = keep
                worst = max(worst, abs((up - down) / (2 * h) - g[at]))
    scale = max(np.abs(g).max() for pair in grads for g in pair)
    print(f"{loss}: max |analytic - central difference| = {worst:.3e}, max |gradient| = {scale:.3e}")
    assert scale > 1e-3
    assert worst <= 1e-8 * max(scale, 1.0)        # h^2 f''' / 6 ~ 1e-12 and rounding eps / h ~ 1e-10, both far below


@pytest.mark.parametrize("loss", ("categorical", "binary"))
def test_the_losses_survive_large_logits(loss):
    z = np.array([[1000.0, -1000.0, 0.0], [-800.0, 900.0, 5.0]])
    t = np.array([0, 2]) if loss == "categorical" else np.array([[1.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    for dtype in (np.float64, np.float32):
        value, delta = T.loss_and_delta(z, t, loss, dtype)
        assert np.isfinite(value) and np.isfinite(delta).all() and value.dtype == dtype and delta.dtype == dtype


def test_float32_restatement_stays_in_float32():
    rng = np.random.default_rng(2)
    layers = T.cast_layers(tanh_stack(rng), np.float32)
    x = (np.maximum(rng.normal(size=(9, 1024)), 0) * 0.5).astype(np.float32)
    out = T.train(layers, x, [(np.arange(9), rng.integers(0, 3, 9))] * 2, "categorical", T.Adam(dtype=np.float32), np.float32)
    assert all(k.dtype == np.float32 and b.dtype == np.float32 for k, b, _ in out)
    ref = T.train(layers, x, [(np.arange(9), rng.integers(0, 3, 9))] * 2, "categorical", T.Adam())
    assert all(k.dtype == np.float64 for k, _, _ in ref)


# ---------------------------------------------------------------------------------------------------- metrics_table
def parse(text):
    lines = text.splitlines()
    assert lines[0] == '"threshold","precision","sensitivity","fpr"' and text.endswith("\n")
    return [line.split(",") for line in lines[1:]]


def test_metrics_table_counts_on_hand_made_logits():
    #          detected at >= 1.24: one positive; 1.236 and 1.244 both round to 1.24, 1.236 lies below its own threshold
    logits = [1.244, 1.236, 0.5, 0.5, -0.2, -1.0]
    positives = [1, 1, 0, 1, 0, 0]
    rows = parse(train.metrics_table(logits, positives))
    assert [r[0] for r in rows] == ["1.24", "0.5", "-0.2", "-1"]
    assert rows[0] == ["1.24", "1", train._num(1 / 3), "0"]                       # 1.244 alone
    assert rows[1] == ["0.5", "0.75", "1", train._num(1 / 3)]                     # + 1.236, 0.5 (neg), 0.5 (pos): TP 3, FP 1
    assert rows[2] == ["-0.2", "0.6", "1", train._num(2 / 3)]
    assert rows[3] == ["-1", "0.5", "1", "1"]


def test_metrics_table_leaves_precision_empty_where_nothing_is_detected():
    rows = parse(train.metrics_table([0.116, -0.3], [1, 0]))               # 0.116 rounds up to 0.12: no logit reaches it
    assert rows[0] == ["0.12", "", "0", "0"]
    assert rows[1] == ["-0.3", "0.5", "1", "1"]


def test_metrics_table_of_a_class_without_positives():
    rows = parse(train.metrics_table([0.3, 0.1, 0.1], [0, 0, 0]))
    assert rows == [["0.3", "0", "", train._num(1 / 3)], ["0.1", "0", "", "1"]]


def test_threshold_for_precision_reads_the_table_unchanged(tmp_path):
    rng = np.random.default_rng(3)
    positives = rng.integers(0, 2, 400).astype(bool)
    logits = rng.normal(size=400) + 2.0 * positives
    text = train.metrics_table(logits, positives)
    path = tmp_path / "metrics.csv"
    path.write_text(text)
    rows = [(float(t), float(p)) for t, p, _, _ in parse(text) if p != ""]
    want = 0.9
    near = [t for t, p in rows if abs(p - want) <= 0.005]
    assert near, "the example has thresholds near the requested precision"
    got = results.threshold_for_precision("model_fit", want, metrics_path=str(path))
    assert got == pytest.approx(np.mean(near), abs=1e-12)
    thresholds = [t for t, _ in rows]
    assert thresholds == sorted(thresholds, reverse=True) and len(set(thresholds)) == len(thresholds)


# ---------------------------------------------------------------------------------------------------- save_model
def example_fit(rng):
    layers = [(rng.normal(size=(1024, 33)).astype(np.float32), rng.normal(size=33).astype(np.float32), "relu"),
              (rng.normal(size=(33, 3)).astype(np.float32), rng.normal(size=3).astype(np.float32), "linear")]
    return train.FitResult(weights.HeadWeights(layers, ["ambient", "ins_buzz", "mech_plane"]), {"loss": [1.0, 0.5]})


def test_save_model_round_trips_through_read_model_dir(tmp_path):
    fit = example_fit(np.random.default_rng(8))
    table = train.metrics_table([0.3, -0.2, 0.7], [1, 0, 1])
    path = train.save_model(str(tmp_path / "models" / "model_fit"), fit, metrics=table, embeddername="yamnet", digits_results=3)
    head = weights.read_model_dir(path, "model_fit")
    assert len(head.layers) == 2
    for (k, b, a), (k0, b0, a0) in zip(head.layers, fit.head.layers):
        assert a == a0 and k.dtype == np.float32 and k.tobytes() == k0.tobytes() and b.tobytes() == b0.tobytes()
    assert head.classes == ["ambient", "ins_buzz", "mech_plane"] and head.embeddername == "yamnet" and head.digits_results == 3
    assert head.metrics_path == os.path.join(path, "tests", "metrics.csv")
    with open(head.metrics_path) as f:
        assert f.read() == table
    assert os.path.exists(os.path.join(path, "model.py"))
    again = weights.load_head("model_fit", models_dir=str(tmp_path / "models"))
    assert again.layers[1][0].tobytes() == fit.head.layers[1][0].tobytes()


# ---------------------------------------------------------------------------------------------------- the writer's move
def directory_digest(path):
    h = hashlib.sha256()
    for root, dirs, files in sorted(os.walk(path)):
        dirs.sort()
        for name in sorted(files):
            full = os.path.join(root, name)
            h.update(os.path.relpath(full, path).replace(os.sep, "/").encode() + b"\0")
            with open(full, "rb") as f:
                h.update(f.read() + b"\0")
    return h.hexdigest()


# sha256 over (relative path, bytes) of every file, recorded from tools/modelgen.py's writer before it moved into the package
WRITER_DIGESTS = {
    "relu_256_13": (dict(seed=11), "e33495243c4483c062d6553b1a44a13d06ea1050606159774c4f56dcb3f2e883"),
    "tanh_relu_100_37_5": (dict(seed=3, digits_results=4, embeddername="yamnet"),
                           "7e3dcf628c279db879e123f029218b1a56fb9f4aa07f3e71c6b3024a5d61d0f1"),
    "softmax_64_10": (dict(seed=5, classes=[f"c{i}" for i in range(10)], model="mine"),
                      "6e7cdac7a988da6565a0c35a5f7c8751035d5cf882d9ce3881829150f48d58f3"),
}


@pytest.mark.parametrize("name", sorted(WRITER_DIGESTS))
@pytest.mark.parametrize("module", (G, modeldir), ids=("tools.modelgen", "buzzdetect_amd.modeldir"))
def test_the_moved_writer_gives_the_bytes_it_gave_before(tmp_path, module, name):
    kw, digest = WRITER_DIGESTS[name]
    kw = dict(kw)
    seed = kw.pop("seed")
    widths, acts = module.EXAMPLE_STACKS[name]
    out = str(tmp_path / name)
    module.write_model_dir(out, module.glorot_layers(widths, acts, seed=seed), seed=seed, **kw)
    module.write_model_py(out, name)
    assert directory_digest(out) == digest
    assert G.write_model_dir is modeldir.write_model_dir and G.saved_model_bytes is modeldir.saved_model_bytes


# ---------------------------------------------------------------------------------------------------- argument errors
def good(n=12, c=3):
    rng = np.random.default_rng(0)
    return dict(embeddings=rng.random((n, 1024), dtype=np.float32), targets=rng.integers(0, c, n),
                classes=[f"class_{i}" for i in range(c)])


BAD = {
    "embedding width": lambda a: a.update(embeddings=a["embeddings"][:, :1000]),
    "embedding rank": lambda a: a.update(embeddings=a["embeddings"][0]),
    "embedding dtype": lambda a: a.update(embeddings=a["embeddings"].astype(np.int32)),
    "no rows": lambda a: a.update(embeddings=a["embeddings"][:0], targets=a["targets"][:0]),
    "target count": lambda a: a.update(targets=a["targets"][:-1]),
    "float labels for categorical": lambda a: a.update(targets=a["targets"].astype(np.float32)),
    "label too large": lambda a: a["targets"].__setitem__(3, 3),
    "negative label": lambda a: a["targets"].__setitem__(3, -1),
    "binary targets' width is not len(classes)": lambda a: a.update(loss="binary", targets=np.zeros((12, 4), np.float32)),
    "binary targets' shape": lambda a: a.update(loss="binary"),
    "non-finite embedding": lambda a: a["embeddings"].__setitem__((5, 17), np.nan),
    "infinite embedding": lambda a: a["embeddings"].__setitem__((0, 0), np.inf),
    "non-finite binary target": lambda a: a.update(loss="binary", targets=np.full((12, 3), np.nan, np.float32)),
    "unsupported activation": lambda a: a.update(hidden=(16,), activations=("gelu",)),
    "softmax as a hidden activation": lambda a: a.update(hidden=(16,), activations=("softmax",)),
    "activations and hidden disagree": lambda a: a.update(hidden=(16, 8), activations=("relu",)),
    "hidden width": lambda a: a.update(hidden=(4096,), activations=("relu",)),
    "too many layers": lambda a: a.update(hidden=(8,) * 8, activations=("relu",) * 8),
    "no classes": lambda a: a.update(classes=[]),
    "loss": lambda a: a.update(loss="hinge"),
    "optimizer": lambda a: a.update(optimizer="rmsprop"),
    "learning rate": lambda a: a.update(learning_rate=0.0),
    "epochs": lambda a: a.update(epochs=0),
    "batch size": lambda a: a.update(batch_size=0),
    "validation width": lambda a: a.update(validation=(a["embeddings"][:, :5], a["targets"])),
    "validation labels": lambda a: a.update(validation=(a["embeddings"], a["targets"] + 3)),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_fit_head_refuses_bad_arguments_before_any_device_work(what, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    monkeypatch.setattr(train, "Trainer", no_device)
    args = good()
    BAD[what](args)
    with pytest.raises(ValueError):
        train.fit_head(**args)


def test_good_arguments_pass_the_checks():
    a = good()
    classes, widths, acts, data, val = train.check_fit_arguments(a["embeddings"], a["targets"], a["classes"], (16,), ("tanh",),
                                                                 "categorical", "adam", 1e-3, 2, 8, (a["embeddings"], a["targets"]))
    assert widths == [16, 3] and acts == ["tanh", "linear"] and data[0] == 12 and data[3].dtype == np.int32 and val[0] == 12


def test_glorot_layers_are_seeded_and_zero_biased():
    a = train.glorot_layers(np.random.default_rng(4), [33, 13], ["relu", "linear"])
    b = train.glorot_layers(np.random.default_rng(4), [33, 13], ["relu", "linear"])
    assert [k.shape for k, _, _ in a] == [(1024, 33), (33, 13)]
    for (k, bias, _), (k2, _, _) in zip(a, b):
        lim = np.sqrt(6.0 / sum(k.shape))
        assert k.dtype == np.float32 and k.tobytes() == k2.tobytes() and not bias.any()
        assert np.abs(k).max() <= lim and np.abs(k).max() > 0.9 * lim
