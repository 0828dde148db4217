"""The bank of heads, host side (include/buzzdetect_bank.h, buzzdetect_amd/train.py: TrainerBank, fit_heads, cross_validate_head):
the binding table, NULL arguments, argument errors before any device work, the fold builder and the members' weights.  No GPU
needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from buzzdetect_amd import _lib, build, train
from buzzdetect_amd.train import balanced_class_weights, build_folds, check_cross_validation, fold_members

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- header and binding
def test_the_binding_table_lists_every_prototype_of_the_bank_header():
    header = open(os.path.join(REPO, "include", "buzzdetect_bank.h")).read()
    declared = sorted(re.findall(r"^BD_API [^;(]*?(bd_\w+)\(", header, re.M))
    assert declared == sorted(_lib.BANK_PROTOTYPES) and len(declared) == 17
    for name in declared:                                   # one ctypes argument per parameter of the prototype
        params = re.search(r"^BD_API [^;(]*?" + name + r"\(([^;]*?)\);", header, re.M | re.S).group(1)
        n_args = 0 if params.strip() == "void" else params.count(",") + 1
        assert len(_lib.BANK_PROTOTYPES[name][1]) == n_args, name
    assert int(re.search(r"#define BD_BANK_ABI_VERSION (\d+)", header).group(1)) == _lib.BANK_ABI_VERSION == 1
    assert int(re.search(r"#define BD_BANK_GROUP_COLUMNS (\d+)", header).group(1)) == _lib.BANK_GROUP_COLUMNS == _lib.TRAIN_FUSED_MAX_WIDTH
    assert int(re.search(r"#define BD_BANK_MAX_MEMBERS (\d+)", header).group(1)) == _lib.BANK_MAX_MEMBERS
    assert int(re.search(r"#define BD_BANK_MAX_WORKSPACE_BYTES (\d+)LL", header).group(1)) == _lib.BANK_MAX_WORKSPACE_BYTES
    assert not set(_lib.BANK_PROTOTYPES) & set(_lib.TRAIN_PROTOTYPES)
    lib = _lib.load()
    assert lib.bd_bank_abi_version() == 1 and lib.bd_train_abi_version() == 2


def test_the_trainer_and_the_bank_share_one_header_of_device_routines():
    assert "headbank.hip" in build.SOURCES and "headtrain_device.h" in build.HEADERS
    shared = open(os.path.join(build.CSRC, "headtrain_device.h")).read()
    for name in ("mma_chain", "forward_tile", "weight_grad_tile", "bias_grad_tile", "loss_row", "acc_row", "decayed", "apply_element",
                 "loss_sum_block"):
        assert re.search(r"\b" + name + r"\(", shared), name
        for source in ("headtrain.hip", "headbank.hip"):    # called, not defined again
            text = open(os.path.join(build.CSRC, source)).read()
            assert not re.search(r"__device__[^;{]*\b" + name + r"\(", text), f"{source} defines {name}"
    for source in ("headtrain.hip", "headbank.hip"):
        assert '#include "headtrain_device.h"' in open(os.path.join(build.CSRC, source)).read()
        assert '#include "headtrain_host.h"' in open(os.path.join(build.CSRC, source)).read()      # and one host side
    assert "__device__" not in open(os.path.join(build.CSRC, "headtrain_host.h")).read()


def test_every_bank_call_refuses_null_before_anything_is_enqueued():
    lib = _lib.load()
    handle, word = C.c_void_p(), C.c_float()
    opt = _lib.bd_train_optimizer(1, 1e-3, 0.9, 0.999, 1e-7, 0)
    layer = (_lib.bd_head_layer * 1)()
    calls = {
        "bd_bank_create": lambda: lib.bd_bank_create(0, None, 1, 0, C.byref(opt), 256, C.byref(handle)),
        "bd_bank_step": lambda: lib.bd_bank_step(None, None, 1024, None, None, None, 0, 1, None),
        "bd_bank_loss": lambda: lib.bd_bank_loss(None, None, 1024, None, None, None, 0, 1, None, None),
        "bd_bank_forward": lambda: lib.bd_bank_forward(None, None, 1024, None, 1, None, 64, None),
        "bd_bank_set_learning_rate": lambda: lib.bd_bank_set_learning_rate(None, 0, 1e-3),
        "bd_bank_set_weight_decay": lambda: lib.bd_bank_set_weight_decay(None, 0, 0.0),
        "bd_bank_set_frozen": lambda: lib.bd_bank_set_frozen(None, 0, 1),
        "bd_bank_snapshot": lambda: lib.bd_bank_snapshot(None, 0, None),
        "bd_bank_restore": lambda: lib.bd_bank_restore(None, 0, None),
        "bd_bank_read": lambda: lib.bd_bank_read(None, 0, None, None),
        "bd_bank_gradients": lambda: lib.bd_bank_gradients(None, 0, None, None),
        "bd_bank_mean_loss": lambda: lib.bd_bank_mean_loss(None, 0, C.byref(word)),
        "bd_bank_workspace_floats": lambda: lib.bd_bank_workspace_floats(None),
        "bd_bank_workspace_fill": lambda: lib.bd_bank_workspace_fill(None, 0),
        "bd_bank_workspace_read": lambda: lib.bd_bank_workspace_read(None, None, 0),
    }
    assert set(calls) == set(_lib.BANK_PROTOTYPES) - {"bd_bank_abi_version", "bd_bank_destroy"}
    for name, call in calls.items():
        assert call() == -1 and name.encode() in lib.bd_last_error(), name     # BD_EINVAL, and the message says who
    assert lib.bd_bank_create(0, layer, 1, 0, None, 256, C.byref(handle)) == -1 and b"bd_bank_create" in lib.bd_last_error()
    assert lib.bd_bank_create(0, layer, 1, 0, C.byref(opt), 256, None) == -1
    assert lib.bd_bank_destroy(None) == 0                   # like free(NULL) and bd_trainer_destroy


def test_bank_create_refuses_shapes_and_sizes_before_it_looks_for_a_device():
    lib = _lib.load()
    handle = C.c_void_p()
    opt = _lib.bd_train_optimizer(1, 1e-3, 0.9, 0.999, 1e-7, 0)

    def create(widths, max_batch=256, n_in=1024):
        k = np.zeros((1024, max(widths)), np.float32)
        arr = (_lib.bd_head_layer * len(widths))()
        for i, w in enumerate(widths):
            arr[i].kernel = k.ctypes.data_as(C.POINTER(C.c_float))
            arr[i].n_in, arr[i].n_out = n_in, w
        return lib.bd_bank_create(0, arr, len(widths), 0, C.byref(opt), max_batch, C.byref(handle))

    assert create([65]) == -1 and b"1..64" in lib.bd_last_error()
    assert create([0]) == -1
    assert create([3, 4]) == -1 and b"member 1" in lib.bd_last_error()
    assert create([3], n_in=512) == -1 and b"1024" in lib.bd_last_error()
    assert create([3], max_batch=0) == -1 and create([3], max_batch=65537) == -1
    # 4096 members of 64 outputs at the largest batch: 256 slices x 4096 groups of partials, far past the header's cap
    assert create([64] * 4096, max_batch=65536) == -4 and b"BD_BANK_MAX_WORKSPACE_BYTES" in lib.bd_last_error()     # BD_EWORKSPACE
    assert handle.value is None


# ---------------------------------------------------------------------------------------------------- argument errors
def good(n=24, c=3):
    rng = np.random.default_rng(0)
    return dict(embeddings=rng.random((n, 1024), dtype=np.float32), targets=np.arange(n) % c,
                classes=[f"class_{i}" for i in range(c)], epochs=3)


def binary(a):
    a.update(loss="binary", targets=np.zeros((24, 3), np.float32))


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    for name in ("Trainer", "TrainerBank"):
        monkeypatch.setattr(train, name, refuse)
    monkeypatch.setattr(_lib, "load", refuse)


BAD_MEMBERS = {
    "an unknown key": ([{}, {"learning_rate": 1e-3, "dropout": 0.5}], {}, r"members\[1\].*dropout"),
    "a member that is no dict": ([{}, {}, 3], {}, r"members\[2\]"),
    "no members": ([], {}, "at least one"),
    "class_weight with the binary loss": ([{}, {"class_weight": "balanced"}], "binary", r"members\[1\].*sample_weight"),
    "a negative decay": ([{"weight_decay": -1.0}], {}, r"members\[0\].*weight_decay"),
    "a rate sequence of the wrong length": ([{}, {}, {"learning_rate": [1e-3, 1e-4]}], {}, r"members\[2\].*learning_rate"),
    "sample weights of the wrong length": ([{"sample_weight": np.ones(5)}], {}, r"members\[0\].*sample_weight"),
    "a negative patience": ([{}, {"early_stopping": {"patience": -1}}], {}, r"members\[1\].*patience"),
    "a validation_weight without validation": ([{"validation_weight": np.ones(24)}], {}, r"members\[0\].*validation"),
}


@pytest.mark.parametrize("what", sorted(BAD_MEMBERS))
def test_fit_heads_refuses_bad_members_by_index_before_any_device_work(what, no_device):
    members, how, message = BAD_MEMBERS[what]
    args = good()
    if how == "binary":
        binary(args)
    with pytest.raises(ValueError, match=message):
        train.fit_heads(members=members, **args)


def test_fit_heads_refuses_shared_arguments_and_a_weighted_validation_tuple(no_device):
    a = good()
    with pytest.raises(ValueError, match="validation_weight"):
        train.fit_heads(members=[{}], validation=(a["embeddings"], a["targets"], np.ones(24)), **a)
    with pytest.raises(ValueError, match=r"members\[0\].*validation sample_weight"):
        train.fit_heads(members=[{"validation_weight": np.ones(5)}], validation=(a["embeddings"], a["targets"]), **a)
    with pytest.raises(ValueError):
        train.fit_heads(members=[{}], **dict(a, epochs=0))
    with pytest.raises(ValueError, match="64"):
        train.fit_heads(members=[{}], **dict(a, classes=[f"c{i}" for i in range(65)]))
    with pytest.raises(TypeError):
        train.fit_heads(members=[{}], learning_rate=1e-3, **a)          # a member's knob, not a shared one


def test_good_members_pass_the_checks_and_reach_the_device(monkeypatch):
    class Reached(Exception):
        pass

    def bank(members, *a, **k):
        assert len(members) == 6 and all(m[0] is members[0][0] for m in members)       # all members start equal
        raise Reached()
    monkeypatch.setattr(train, "TrainerBank", bank)
    a = good()
    members = [{}, {"learning_rate": [1e-3, 5e-4, 1e-4], "weight_decay": 1e-2}, {"class_weight": "balanced"},
               {"sample_weight": np.linspace(0, 2, 24)}, {"early_stopping": {"patience": 0}},
               {"early_stopping": {"patience": 2}, "validation_weight": np.ones(24)}]
    with pytest.raises(Reached):
        train.fit_heads(members=members, validation=(a["embeddings"], a["targets"]), **a)


def test_hidden_stacks_run_the_members_through_fit_head_one_after_another(monkeypatch):
    seen = []
    monkeypatch.setattr(train, "fit_head", lambda *a, **k: seen.append(k) or len(seen))
    a = good()
    vw = np.ones(24)
    out = train.fit_heads(members=[{"weight_decay": 1e-2}, {"validation_weight": vw}], hidden=(8,), activations=("relu",),
                          validation=(a["embeddings"], a["targets"]), seed=4, **a)
    assert out == [1, 2] and [k["seed"] for k in seen] == [4, 4] and all(k["hidden"] == (8,) for k in seen)
    assert seen[0]["weight_decay"] == 1e-2 and len(seen[0]["validation"]) == 2
    assert "validation_weight" not in seen[1] and seen[1]["validation"][2] is vw


def cv_good(n=60, c=3):
    a = good(n, c)
    a["targets"] = np.arange(n) % c
    return a


BAD_CV = {
    "fold_of_row and folds": (lambda a: a.update(fold_of_row=np.arange(60) % 3, folds=3), "not both"),
    "fold_of_row and groups": (lambda a: a.update(fold_of_row=np.arange(60) % 3, groups=np.arange(60) // 6), "not both"),
    "fold ids below the range": (lambda a: a.update(fold_of_row=np.arange(60) % 3 - 1), "0..K-1"),
    "fold ids past the range": (lambda a: a.update(fold_of_row=np.where(np.arange(60) == 0, 10 ** 6, np.arange(60) % 3)), "0..K-1"),
    "fold ids that are no integers": (lambda a: a.update(fold_of_row=np.arange(60) % 3 * 1.0), "integers"),
    "fold_of_row of the wrong length": (lambda a: a.update(fold_of_row=np.arange(59) % 3), "shape"),
    "an empty fold": (lambda a: a.update(fold_of_row=np.arange(60) % 2 * 2), "fold 1 holds no rows"),
    "one fold only": (lambda a: a.update(fold_of_row=np.zeros(60, np.int64)), "one fold"),
    "more folds than groups": (lambda a: a.update(folds=4, groups=np.arange(60) // 20), "4 folds but only 3 groups"),
    "more folds than rows": (lambda a: a.update(folds=61), "61 folds but only 60 rows"),
    "one fold asked for": (lambda a: a.update(folds=1), ">= 2"),
    "groups of the wrong length": (lambda a: a.update(groups=np.arange(59)), "one group per row"),
    # class 2's rows all lie in fold 1: fold 1's training side has none
    "a class absent from a training side": (lambda a: a.update(fold_of_row=np.where(np.arange(60) % 3 == 2, 1, np.arange(60) // 3 % 3)),
                                            r'fold 1 has no row of class 2 \("class_2"\)'),
    "an unknown grid key": (lambda a: a.update(grid=[{}, {"momentum": 0.9}]), r"grid\[1\].*momentum"),
    "validation_weight in the grid": (lambda a: a.update(grid=[{"validation_weight": np.ones(60)}]), r"grid\[0\].*validation_weight"),
    "an empty grid": (lambda a: a.update(grid=[]), "at least one"),
    "a bad knob in the grid": (lambda a: a.update(grid=[{}, {"weight_decay": -1.0}]), r"members\[5\].*weight_decay"),
    "class_weight with the binary loss": (lambda a: a.update(loss="binary", targets=np.zeros((60, 3), np.float32), grid=[{"class_weight": "balanced"}]),
                                          r"grid\[0\].*sample_weight"),
    "an unknown shared argument": (lambda a: a.update(hidden=(8,)), "hidden"),
}


@pytest.mark.parametrize("what", sorted(BAD_CV))
def test_cross_validate_head_refuses_before_any_device_work(what, no_device):
    change, message = BAD_CV[what]
    args = cv_good()
    change(args)
    with pytest.raises(ValueError, match=message):
        train.cross_validate_head(**args)


# ---------------------------------------------------------------------------------------------------- the fold builder
def test_stratified_folds_hold_every_row_out_once_and_split_every_class_within_one():
    rng = np.random.default_rng(3)
    labels = rng.choice(4, 1003, p=[0.7, 0.2, 0.09, 0.01])
    for folds in (2, 5, 7):
        f = build_folds(labels, "categorical", folds, seed=11)
        assert f.dtype == np.int32 and f.shape == labels.shape and f.min() == 0 and f.max() == folds - 1      # each row: one fold
        for c in range(4):
            count = np.bincount(f[labels == c], minlength=folds)
            assert count.max() - count.min() <= 1, (folds, c, count)
        total = np.bincount(f, minlength=folds)
        assert total.max() - total.min() <= 1                # the deal of a class starts where the last one ended
    multi_hot = rng.integers(0, 2, (101, 3)).astype(np.float32)
    f = build_folds(multi_hot, "binary", 4, seed=11)         # nothing to stratify by: all rows dealt round-robin
    assert np.array_equal(np.bincount(f), [26, 25, 25, 25])


def test_grouped_folds_split_no_group_and_fill_the_emptiest_fold_with_the_largest_group_left():
    rng = np.random.default_rng(4)
    sizes = [50, 40, 31, 30, 12, 12, 7, 5, 3, 1]
    names = [f"rec_{i}.wav" for i in range(len(sizes))]
    groups = rng.permutation(np.repeat(names, sizes))
    labels = rng.integers(0, 2, groups.size)
    f = build_folds(labels, "categorical", 3, groups=groups, seed=2)
    for name in names:
        assert np.unique(f[groups == name]).size == 1        # no group is split
    # restated: largest first, each to the fold with the fewest rows so far (lowest fold on a tie); the two groups of 12 may swap
    held = [0, 0, 0]
    for s in sizes:
        held[int(np.argmin(held))] += s
    assert sorted(np.bincount(f, minlength=3)) == sorted(held)
    for loss, t in (("categorical", labels), ("binary", np.zeros((groups.size, 2), np.float32))):
        assert np.array_equal(build_folds(t, loss, 3, groups=groups, seed=2), f)       # labels are not looked at
    assert np.array_equal(build_folds(labels, "categorical", 3, groups=list(groups), seed=2), f)


def test_the_same_seed_gives_the_same_folds_from_a_generator_that_is_not_the_fits():
    labels = np.random.default_rng(5).integers(0, 3, 300)
    state = np.random.get_state()[1].copy()
    a, b, other = build_folds(labels, folds=5, seed=7), build_folds(labels, folds=5, seed=7), build_folds(labels, folds=5, seed=8)
    assert np.array_equal(a, b) and not np.array_equal(a, other)
    assert np.array_equal(np.random.get_state()[1], state)   # the global generator is not touched either
    # restated with the generator the docstring names ...
    rng, want, start = np.random.default_rng([7, train.FOLD_SEED_STREAM]), np.empty(300, np.int32), 0
    for c in range(3):
        rows = np.flatnonzero(labels == c)
        rows = rows[rng.permutation(rows.size)]
        want[rows] = (start + np.arange(rows.size)) % 5
        start = (start + rows.size) % 5
    assert np.array_equal(a, want)
    # ... whose stream is not the fit's: default_rng(seed) deals the rows differently, and the fit's own draws stay what they are
    fit_rng, mine = np.random.default_rng(7), np.random.default_rng([7, train.FOLD_SEED_STREAM])
    assert not np.array_equal(fit_rng.permutation(300), mine.permutation(300))
    first = train.glorot_layers(np.random.default_rng(7), [3], ["linear"])[0][0]
    build_folds(labels, folds=5, seed=7)
    assert np.array_equal(train.glorot_layers(np.random.default_rng(7), [3], ["linear"])[0][0], first)


# ---------------------------------------------------------------------------------------------------- the members' weights
def test_member_weights_and_in_fold_balanced_class_weights_equal_their_definitions():
    rng = np.random.default_rng(6)
    n, classes = 90, ["a", "b", "c"]
    labels = rng.choice(3, n, p=[0.6, 0.3, 0.1]).astype(np.int32)
    fold_of_row = build_folds(labels, folds=3, seed=1)
    sw = rng.uniform(0.5, 2.0, n)
    members = fold_members(labels, classes, "categorical", fold_of_row, 3,
                           {"sample_weight": sw, "class_weight": "balanced", "weight_decay": 1e-3, "learning_rate": 2e-3})
    assert len(members) == 3
    for k, member in enumerate(members):
        inside = fold_of_row != k
        assert np.array_equal(member["sample_weight"], sw.astype(np.float32).astype(np.float64) * inside)
        assert np.array_equal(member["validation_weight"], (fold_of_row == k).astype(np.float32))
        count = np.bincount(labels[inside], minlength=3)
        assert np.array_equal(member["class_weight"], inside.sum() / (3.0 * count))        # N_in / (C count_c), in-fold labels only
        assert not np.array_equal(member["class_weight"], balanced_class_weights(labels, 3))
        assert member["weight_decay"] == 1e-3 and member["learning_rate"] == 2e-3 and "early_stopping" not in member
        # what the device gets: one float32 product per row, zero on the held-out rows
        row_w = train.check_fit_weighting(classes, "categorical", 2, 1e-3, labels, n, member["validation_weight"],
                                          member["sample_weight"], member["class_weight"])[0]
        want = member["class_weight"].astype(np.float32)[labels] * (sw.astype(np.float32) * inside.astype(np.float32))
        assert row_w.tobytes() == want.tobytes() and not row_w[~inside].any() and row_w[inside].all()
    # without sample weights the training side weighs 1; a dict is spelled out in the classes' order, a class not named weighs 1
    plain = fold_members(labels, classes, "categorical", fold_of_row, 3, {"class_weight": {"c": 4.0}})
    for k, member in enumerate(plain):
        assert np.array_equal(member["sample_weight"], (fold_of_row != k).astype(np.float64))
        assert np.array_equal(member["class_weight"], [1.0, 1.0, 4.0])
    assert "class_weight" not in fold_members(labels, classes, "categorical", fold_of_row, 3, {})[0]


def test_the_members_of_a_grid_are_grid_major_and_a_callers_folds_are_taken_as_they_are():
    labels = (np.arange(60) % 3).astype(np.int32)
    mine = (np.arange(60) // 3 % 4).astype(np.int64)
    f, k, grid, members = check_cross_validation(labels, ["a", "b", "c"], "categorical", None, None, mine,
                                                 ({}, {"weight_decay": 1e-2}), 0, {"learning_rate": 5e-4})
    assert k == 4 and f.dtype == np.int32 and np.array_equal(f, mine) and len(members) == 8
    for g in range(2):
        for fold in range(4):
            member = members[g * 4 + fold]
            assert np.array_equal(member["validation_weight"], mine == fold) and member["learning_rate"] == 5e-4
            assert member.get("weight_decay") == (1e-2 if g else None)
    f5 = check_cross_validation(labels, ["a", "b", "c"], "categorical", None, None, None, ({},), 3, {})
    assert f5[1] == 5 and np.array_equal(f5[0], build_folds(labels, folds=5, seed=3))      # five folds when nothing is said
