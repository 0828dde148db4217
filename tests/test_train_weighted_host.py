"""Row weights, weight decay, learning-rate schedules and early stopping of the head trainer, host side (buzzdetect_amd/train.py,
include/buzzdetect_train.h) and the restatement the GPU tests compare with (tests/train_oracle_weighted.py): no GPU needed."""
import os
import re

import numpy as np
import pytest

from buzzdetect_amd import _lib, train
from buzzdetect_amd.train import balanced_class_weights, check_fit_weighting, learning_rates
from tests import train_oracle as T
from tests import train_oracle_weighted as TW

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- the restatement
def tanh_stack(rng):
    return [(rng.normal(0, 0.05, (1024, 5)), rng.normal(0, 0.1, 5), "tanh"), (rng.normal(0, 0.5, (5, 3)), rng.normal(0, 0.1, 3), "linear")]


@pytest.mark.parametrize("loss", ("categorical", "binary"))
def test_the_weighted_gradients_match_central_differences(loss):
    rng = np.random.default_rng(5)
    layers = tanh_stack(rng)
    x = np.maximum(rng.normal(size=(7, 1024)), 0) * 0.5
    targets = rng.integers(0, 3, 7) if loss == "categorical" else rng.integers(0, 2, (7, 3)).astype(np.float64)
    w = np.array([0.0, 0.25, 1.0, 50.0, 1.0, 0.25, 50.0])
    _, grads = TW.gradients(layers, x, targets, loss, w)
    h, worst = 1e-6, 0.0
    for li in range(2):
        for pi in range(2):
            p, g = layers[li][pi], grads[li][pi]
            for at in [np.unravel_index(i, p.shape) for i in rng.choice(p.size, min(p.size, 40), replace=False)]:
                keep = p[at]
                p[at] = keep + h
                up = TW.mean_loss(layers, x, targets, loss, w)
                p[at] = keep - h
                down = TW.mean_loss(layers, x, targets, loss, w)
                p[at] = keep
                worst = max(worst, abs((up - down) / (2 * h) - g[at]))
    scale = max(np.abs(g).max() for pair in grads for g in pair)
    print(f"{loss}: max |analytic - central difference| = {worst:.3e}, max |gradient| = {scale:.3e}")
    assert scale > 1e-3
    assert worst <= 1e-8 * max(scale, 1.0)        # h^2 f''' / 6 ~ 1e-12 x 50 and rounding eps / h ~ 1e-10 x 50, both below


@pytest.mark.parametrize("loss", ("categorical", "binary"))
def test_weights_of_one_are_the_unweighted_restatement_and_the_loss_divides_by_the_rows(loss):
    rng = np.random.default_rng(6)
    layers = tanh_stack(rng)
    x = np.maximum(rng.normal(size=(9, 1024)), 0) * 0.5
    targets = rng.integers(0, 3, 9) if loss == "categorical" else rng.integers(0, 2, (9, 3)).astype(np.float64)
    value, grads = TW.gradients(layers, x, targets, loss, np.ones(9))
    value0, grads0 = T.gradients(layers, x, targets, loss)
    assert abs(value - value0) <= 1e-15 * abs(value0)
    for (a, b), (a0, b0) in zip(grads, grads0):
        for got, want in ((a, a0), (b, b0)):                # x / B against x * (1 / B): an ulp of the terms, not of a sum that cancels
            assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max()
    # sum_over_batch_size: doubling every weight doubles the loss (a division by the weights' sum would leave it unchanged)
    assert abs(TW.mean_loss(layers, x, targets, loss, np.full(9, 2.0)) - 2 * value0) <= 1e-14 * value0
    # a row of weight zero contributes nothing, but still counts in B
    w = np.ones(9)
    w[4] = 0.0
    keep = np.arange(9) != 4
    assert abs(TW.mean_loss(layers, x, targets, loss, w) * 9 - T.mean_loss(layers, x[keep], targets[keep], loss) * 8) <= 1e-13


def test_the_decay_shrinks_kernels_and_leaves_biases():
    rng = np.random.default_rng(7)
    layers = T.cast_layers(tanh_stack(rng), np.float64)
    zero = [(np.zeros_like(k), np.zeros_like(b)) for k, b, _ in layers]
    decay = float(np.float32(1e-2) * np.float32(0.5))
    out = TW.SgdW(1e-2, 0.5).apply(layers, zero)
    for (k, b, _), (k0, b0, _) in zip(out, layers):
        assert np.array_equal(k, k0 - decay * k0) and np.array_equal(b, b0)
    out = TW.AdamW(1e-2, 0.5).apply(layers, zero)          # zero gradients: Adam's own update is 0 / (0 + eps)
    for (k, b, _), (k0, b0, _) in zip(out, layers):
        assert np.array_equal(k, k0 - decay * k0) and np.array_equal(b, b0)
    f32 = TW.SgdW(1e-2, 0.5, np.float32).apply(T.cast_layers(layers, np.float32), [(a.astype(np.float32), b.astype(np.float32)) for a, b in zero])
    assert all(k.dtype == np.float32 and b.dtype == np.float32 for k, b, _ in f32)


# ---------------------------------------------------------------------------------------------------- balanced weights
def test_balanced_class_weights_by_hand():
    w = balanced_class_weights(np.array([0, 0, 0, 0, 0, 0, 2, 2]), 3)       # counts 6, 0, 2: 8 / (3 x 6), absent, 8 / (3 x 2)
    assert w.dtype == np.float64 and w.shape == (3,)
    assert w[0] == 8 / 18 and w[1] == 0.0 and w[2] == 8 / 6
    assert np.array_equal(balanced_class_weights([1, 0, 1, 0], 2), [1.0, 1.0])
    labels = np.random.default_rng(1).integers(0, 5, 1000)
    w = balanced_class_weights(labels, 5)
    assert np.allclose(np.bincount(labels) * w, 1000 / 5, rtol=1e-15)        # every class carries the same total weight
    for bad in (np.array([0.0, 1.0]), np.array([[0, 1]]), np.array([], dtype=np.int64), np.array([0, 3])):
        with pytest.raises(ValueError):
            balanced_class_weights(bad, 3)


# ---------------------------------------------------------------------------------------------------- header and table
def test_the_binding_table_lists_every_prototype_of_the_header():
    header = open(os.path.join(REPO, "include", "buzzdetect_train.h")).read()
    declared = sorted(re.findall(r"^BD_API [^;(]*?(bd_\w+)\(", header, re.M))
    assert declared == sorted(_lib.TRAIN_PROTOTYPES)
    assert int(re.search(r"#define BD_TRAIN_ABI_VERSION (\d+)", header).group(1)) == _lib.TRAIN_ABI_VERSION == 2
    new = {"bd_trainer_step_weighted": 8, "bd_trainer_loss_weighted": 9, "bd_trainer_set_weight_decay": 2,
           "bd_trainer_set_learning_rate": 2, "bd_trainer_snapshot": 2, "bd_trainer_restore": 2}
    for name, n_args in new.items():
        assert name in declared and len(_lib.TRAIN_PROTOTYPES[name][1]) == n_args
    # additive: what was there stays as it was
    assert len(_lib.TRAIN_PROTOTYPES["bd_trainer_step"][1]) == 7 and len(_lib.TRAIN_PROTOTYPES["bd_trainer_loss"][1]) == 8
    assert [f[0] for f in _lib.bd_train_optimizer._fields_] == ["kind", "learning_rate", "beta_1", "beta_2", "epsilon", "reserved"]
    assert "Out of scope: dropout" in header and "class or sample weights" not in header


def test_the_new_entry_points_refuse_bad_arguments_before_anything_is_enqueued():
    lib = _lib.load()
    calls = {
        "bd_trainer_step_weighted": lambda: lib.bd_trainer_step_weighted(None, None, 1024, None, None, None, 1, None),
        "bd_trainer_loss_weighted": lambda: lib.bd_trainer_loss_weighted(None, None, 1024, None, None, None, 1, None, None),
        "bd_trainer_set_weight_decay": lambda: lib.bd_trainer_set_weight_decay(None, 0.0),
        "bd_trainer_set_learning_rate": lambda: lib.bd_trainer_set_learning_rate(None, 1e-3),
        "bd_trainer_snapshot": lambda: lib.bd_trainer_snapshot(None, None),
        "bd_trainer_restore": lambda: lib.bd_trainer_restore(None, None),
    }
    for name, call in calls.items():
        assert call() == -1 and name.encode() in lib.bd_last_error()          # BD_EINVAL, and the message says who
    assert lib.bd_train_abi_version() == 2


# ---------------------------------------------------------------------------------------------------- argument errors
def good(n=12, c=3):
    rng = np.random.default_rng(0)
    return dict(embeddings=rng.random((n, 1024), dtype=np.float32), targets=np.arange(n) % c,
                classes=[f"class_{i}" for i in range(c)], epochs=3)


def binary(a):
    a.update(loss="binary", targets=np.zeros((12, 3), np.float32))


BAD = {
    "sample_weight length": lambda a: a.update(sample_weight=np.ones(11)),
    "sample_weight rank": lambda a: a.update(sample_weight=np.ones((12, 1))),
    "sample_weight negative": lambda a: a.update(sample_weight=np.r_[np.ones(11), -0.5]),
    "sample_weight nan": lambda a: a.update(sample_weight=np.r_[np.ones(11), np.nan]),
    "sample_weight infinite": lambda a: a.update(sample_weight=np.r_[np.ones(11), np.inf]),
    "sample_weight all zero": lambda a: a.update(sample_weight=np.zeros(12)),
    "sample_weight not numbers": lambda a: a.update(sample_weight=["a"] * 12),
    "sample_weight negative, binary loss": lambda a: (binary(a), a.update(sample_weight=-np.ones(12))),
    "class_weight with the binary loss": lambda a: (binary(a), a.update(class_weight="balanced")),
    "class_weight sequence with the binary loss": lambda a: (binary(a), a.update(class_weight=[1.0, 1.0, 1.0])),
    "class_weight unknown word": lambda a: a.update(class_weight="auto"),
    "class_weight unknown class name": lambda a: a.update(class_weight={"class_0": 1.0, "class_9": 2.0}),
    "class_weight length": lambda a: a.update(class_weight=[1.0, 2.0]),
    "class_weight negative": lambda a: a.update(class_weight=[1.0, -2.0, 1.0]),
    "class_weight negative in a dict": lambda a: a.update(class_weight={"class_1": -2.0}),
    "class_weight nan": lambda a: a.update(class_weight=[1.0, np.nan, 1.0]),
    "class_weight zero on every class present": lambda a: a.update(class_weight=[0.0, 0.0, 0.0]),
    "class_weight x sample_weight zero on every row": lambda a: a.update(class_weight=[1.0, 0.0, 0.0],
                                                                         sample_weight=(np.arange(12) % 3 != 0).astype(np.float64)),
    "weight_decay negative": lambda a: a.update(weight_decay=-1e-4),
    "weight_decay nan": lambda a: a.update(weight_decay=np.nan),
    "learning rate zero": lambda a: a.update(learning_rate=0.0),
    "learning rate negative in a sequence": lambda a: a.update(learning_rate=[1e-3, -1e-3, 1e-3]),
    "learning rate sequence too short": lambda a: a.update(learning_rate=[1e-3, 1e-3]),
    "learning rate sequence too long": lambda a: a.update(learning_rate=[1e-3] * 4),
    "learning rate callable returns zero": lambda a: a.update(learning_rate=lambda epoch: 1e-3 * (2 - epoch)),
    "learning rate callable returns nan": lambda a: a.update(learning_rate=lambda epoch: float("nan")),
    "patience negative": lambda a: a.update(early_stopping={"patience": -1}),
    "patience missing": lambda a: a.update(early_stopping={"min_delta": 0.1}),
    "patience not an integer": lambda a: a.update(early_stopping={"patience": 1.5}),
    "min_delta negative": lambda a: a.update(early_stopping={"patience": 1, "min_delta": -0.1}),
    "early_stopping unknown key": lambda a: a.update(early_stopping={"patience": 1, "monitor": "loss"}),
    "early_stopping not a dict": lambda a: a.update(early_stopping=3),
    "restore_best not a bool": lambda a: a.update(early_stopping={"patience": 1, "restore_best": "yes"}),
    "validation weights' length": lambda a: a.update(validation=(a["embeddings"], a["targets"], np.ones(5))),
    "validation weights negative": lambda a: a.update(validation=(a["embeddings"], a["targets"], -np.ones(12))),
    "validation of four": lambda a: a.update(validation=(a["embeddings"], a["targets"], np.ones(12), None)),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_fit_head_refuses_the_new_arguments_before_any_device_work(what, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    monkeypatch.setattr(train, "Trainer", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    args = good()
    BAD[what](args)
    with pytest.raises(ValueError):
        train.fit_head(**args)


def test_class_weight_with_the_binary_loss_points_to_sample_weight():
    args = good()
    binary(args)
    with pytest.raises(ValueError, match="sample_weight"):
        train.fit_head(class_weight={"class_0": 2.0}, **args)


def test_good_new_arguments_pass_the_checks_and_reach_the_device(monkeypatch):
    class Reached(Exception):
        pass

    def trainer(*a, **k):
        raise Reached()
    monkeypatch.setattr(train, "Trainer", trainer)
    a = good()
    for kw in (dict(sample_weight=np.linspace(0, 2, 12)), dict(class_weight="balanced"), dict(class_weight={"class_1": 3.0}),
               dict(class_weight=(1.0, 2.0, 0.0)), dict(weight_decay=1e-2), dict(learning_rate=[1e-3, 5e-4, 1e-4]),
               dict(learning_rate=lambda epoch: 1e-3 / (1 + epoch)), dict(early_stopping={"patience": 0}),
               dict(early_stopping={"patience": 2, "min_delta": 0.01, "restore_best": False}),
               dict(validation=(a["embeddings"], a["targets"], np.ones(12)))):
        with pytest.raises(Reached):
            train.fit_head(**a, **kw)


def test_row_weights_are_one_float32_product_of_class_and_sample_weight():
    classes = ["a", "b", "c"]
    labels = np.array([0, 0, 0, 0, 0, 0, 2, 2], dtype=np.int32)
    sw = np.array([1.0, 0.1, 0.3, 1.0, 2.0, 0.7, 0.9, 1.1])
    row_w, val_w, rates, decay, stop = check_fit_weighting(classes, "categorical", 2, 1e-3, labels, sample_weight=sw,
                                                           class_weight="balanced")
    cw = balanced_class_weights(labels, 3).astype(np.float32)
    assert row_w.dtype == np.float32 and row_w.tobytes() == (cw[labels] * sw.astype(np.float32)).tobytes()
    assert val_w is None and rates == [1e-3, 1e-3] and decay == 0.0 and stop is None
    # "balanced", its dict and its per-row weights are one thing
    as_dict = {name: float(w) for name, w in zip(classes, balanced_class_weights(labels, 3))}
    by_name = check_fit_weighting(classes, "categorical", 2, 1e-3, labels, class_weight=as_dict)[0]
    by_word = check_fit_weighting(classes, "categorical", 2, 1e-3, labels, class_weight="balanced")[0]
    by_row = check_fit_weighting(classes, "categorical", 2, 1e-3, labels, sample_weight=balanced_class_weights(labels, 3)[labels])[0]
    assert by_name.tobytes() == by_word.tobytes() == by_row.tobytes()
    # a class the dict does not name weighs 1
    assert np.array_equal(check_fit_weighting(classes, "categorical", 2, 1e-3, labels, class_weight={"c": 4.0})[0],
                          np.where(labels == 2, 4.0, 1.0).astype(np.float32))
    # nothing given: no weights at all (the unweighted kernels run)
    assert check_fit_weighting(classes, "categorical", 2, 1e-3, labels)[0] is None
    assert check_fit_weighting(classes, "categorical", 2, 1e-3, labels, early_stopping={"patience": np.int64(3)})[4] == (3, 0.0, True)


def test_learning_rates_of_a_float_a_sequence_and_a_callable():
    assert learning_rates(1e-3, 3) == [1e-3] * 3
    assert learning_rates(np.float32(0.5), 2) == [0.5, 0.5]
    assert learning_rates((1e-3, 1e-4), 2) == [1e-3, 1e-4]
    assert learning_rates(np.array([1e-3, 1e-4]), 2) == [1e-3, 1e-4]
    seen = []
    assert learning_rates(lambda e: seen.append(e) or 1e-3 * 0.5 ** e, 3) == [1e-3, 5e-4, 2.5e-4] and seen == [0, 1, 2]
    with pytest.raises(ValueError):
        learning_rates(1e-60, 1)                  # positive in double, zero as the device's float


def test_fit_result_says_nothing_about_early_stopping_by_default():
    fit = train.FitResult(head=None)
    assert fit.best_epoch is None and fit.stopped_epoch is None and fit.history == {}
