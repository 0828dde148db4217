"""The bank of Dense stacks, host side (include/buzzdetect_stackbank.h, buzzdetect_amd/train.py: TrainerStackBank, fit_stacks,
cross_validate_stack): the binding table, NULL arguments, the shapes and sizes bd_stackbank_create refuses before it looks for a
device, argument errors before any device work, and the pins of the one-layer bank that must still hold.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from buzzdetect_amd import _lib, build, train

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE = -1, -4


# ---------------------------------------------------------------------------------------------------- header and binding
def test_the_binding_table_lists_every_prototype_of_the_stack_bank_header():
    header = open(os.path.join(REPO, "include", "buzzdetect_stackbank.h")).read()
    declared = sorted(re.findall(r"^BD_API [^;(]*?(bd_\w+)\(", header, re.M))
    assert declared == sorted(_lib.STACKBANK_PROTOTYPES) and len(declared) == 17
    for name in declared:                                   # one ctypes argument per parameter of the prototype
        params = re.search(r"^BD_API [^;(]*?" + name + r"\(([^;]*?)\);", header, re.M | re.S).group(1)
        n_args = 0 if params.strip() == "void" else params.count(",") + 1
        assert len(_lib.STACKBANK_PROTOTYPES[name][1]) == n_args, name
    assert int(re.search(r"#define BD_STACKBANK_ABI_VERSION (\d+)", header).group(1)) == _lib.STACKBANK_ABI_VERSION == 1
    assert int(re.search(r"#define BD_STACKBANK_MAX_WORKSPACE_BYTES (\d+)LL", header).group(1)) == _lib.STACKBANK_MAX_WORKSPACE_BYTES \
        == 8 << 30
    others = set(_lib.BANK_PROTOTYPES) | set(_lib.TRAIN_PROTOTYPES)
    assert not set(_lib.STACKBANK_PROTOTYPES) & others and len(_lib.BANK_PROTOTYPES) == 17
    # one entry point of the stack bank per entry point of the bank, under its own name
    assert {n.replace("bd_stackbank_", "") for n in _lib.STACKBANK_PROTOTYPES} == {n.replace("bd_bank_", "") for n in _lib.BANK_PROTOTYPES}
    lib = _lib.load()
    assert lib.bd_stackbank_abi_version() == 1
    assert lib.bd_bank_abi_version() == 1 and lib.bd_train_abi_version() == 2      # the older ABIs did not move


def test_the_stack_bank_calls_the_shared_device_routines_and_defines_none():
    assert "stackbank.hip" in build.SOURCES and "headtrain_device.h" in build.HEADERS
    assert os.path.join("..", "..", "include", "buzzdetect_stackbank.h") in build.HEADERS
    shared = open(os.path.join(build.CSRC, "headtrain_device.h")).read()
    text = open(os.path.join(build.CSRC, "stackbank.hip")).read()
    assert '#include "headtrain_device.h"' in text
    # its kernels are the layer-by-layer route's, which it includes: what holds for the file holds for the two together
    assert '#include "headtrain_stack.h"' in text and "headtrain_stack.h" in build.HEADERS
    text += open(os.path.join(build.CSRC, "headtrain_stack.h")).read()
    assert '#include "headtrain_host.h"' in text and "headtrain_host.h" in build.HEADERS       # the shared host side
    for name in ("mma_chain", "forward_tile", "input_grad_tile", "weight_grad_tile", "bias_grad_tile", "loss_row", "acc_row",
                 "loss_sum_block", "sum_partials", "decayed", "apply_element"):
        assert re.search(r"\b" + name + r"\(", shared), name
        assert not re.search(r"__device__[^;{]*\b" + name + r"\(", text), f"stackbank.hip defines {name}"
    for name in ("forward_tile", "input_grad_tile", "weight_grad_tile", "bias_grad_tile", "loss_row", "loss_sum_block", "sum_partials",
                 "apply_element"):                          # called (decayed is apply_element's)
        assert re.search(r"\b" + name + r"(<\w+>)?\(", text), f"stackbank.hip does not call {name}"
    assert not re.search(r"\batomic", text, re.I)           # nothing is added atomically


def test_every_stack_bank_call_refuses_null_before_anything_is_enqueued():
    lib = _lib.load()
    handle, word = C.c_void_p(), C.c_float()
    opt = _lib.bd_train_optimizer(1, 1e-3, 0.9, 0.999, 1e-7, 0)
    layer = (_lib.bd_head_layer * 1)()
    calls = {
        "bd_stackbank_create": lambda: lib.bd_stackbank_create(0, None, 1, 1, 0, C.byref(opt), 256, C.byref(handle)),
        "bd_stackbank_step": lambda: lib.bd_stackbank_step(None, None, 1024, None, None, None, 0, 1, None),
        "bd_stackbank_loss": lambda: lib.bd_stackbank_loss(None, None, 1024, None, None, None, 0, 1, None, None),
        "bd_stackbank_forward": lambda: lib.bd_stackbank_forward(None, None, 1024, None, 1, None, 64, None),
        "bd_stackbank_set_learning_rate": lambda: lib.bd_stackbank_set_learning_rate(None, 0, 1e-3),
        "bd_stackbank_set_weight_decay": lambda: lib.bd_stackbank_set_weight_decay(None, 0, 0.0),
        "bd_stackbank_set_frozen": lambda: lib.bd_stackbank_set_frozen(None, 0, 1),
        "bd_stackbank_snapshot": lambda: lib.bd_stackbank_snapshot(None, 0, None),
        "bd_stackbank_restore": lambda: lib.bd_stackbank_restore(None, 0, None),
        "bd_stackbank_read": lambda: lib.bd_stackbank_read(None, 0, 0, None, None),
        "bd_stackbank_gradients": lambda: lib.bd_stackbank_gradients(None, 0, 0, None, None),
        "bd_stackbank_mean_loss": lambda: lib.bd_stackbank_mean_loss(None, 0, C.byref(word)),
        "bd_stackbank_workspace_floats": lambda: lib.bd_stackbank_workspace_floats(None),
        "bd_stackbank_workspace_fill": lambda: lib.bd_stackbank_workspace_fill(None, 0),
        "bd_stackbank_workspace_read": lambda: lib.bd_stackbank_workspace_read(None, None, 0),
    }
    assert set(calls) == set(_lib.STACKBANK_PROTOTYPES) - {"bd_stackbank_abi_version", "bd_stackbank_destroy"}
    for name, call in calls.items():
        assert call() == EINVAL and name.encode() in lib.bd_last_error(), name      # and the message says who
    assert lib.bd_stackbank_create(0, layer, 1, 1, 0, None, 256, C.byref(handle)) == EINVAL and b"bd_stackbank_create" in lib.bd_last_error()
    assert lib.bd_stackbank_create(0, layer, 1, 1, 0, C.byref(opt), 256, None) == EINVAL
    assert lib.bd_stackbank_destroy(None) == 0              # like free(NULL) and bd_bank_destroy


def test_stack_bank_create_refuses_shapes_and_sizes_before_it_looks_for_a_device():
    lib = _lib.load()
    handle = C.c_void_p()
    opt = _lib.bd_train_optimizer(1, 1e-3, 0.9, 0.999, 1e-7, 0)
    k = np.zeros(16, np.float32)                            # never read: every call below is refused on its numbers

    def create(members, max_batch=256, n_layers=None, acts=None, first_in=1024, patch=None):
        """members: one list of widths per member; layer l reads the width before it unless ``patch`` = {(m, l): n_in}."""
        n_layers = len(members[0]) if n_layers is None else n_layers
        arr = (_lib.bd_head_layer * max(1, sum(len(m) for m in members)))()
        i = 0
        for m, widths in enumerate(members):
            for l, w in enumerate(widths):
                arr[i].kernel = k.ctypes.data_as(C.POINTER(C.c_float))
                arr[i].n_in = (patch or {}).get((m, l), first_in if l == 0 else widths[l - 1])
                arr[i].n_out = w
                arr[i].activation = _lib.HEAD_ACTIVATIONS[(acts or ["relu"] * len(widths))[l]]
                i += 1
        return lib.bd_stackbank_create(0, arr, len(members), n_layers, 0, C.byref(opt), max_batch, C.byref(handle))

    for widths in ([0], [2049], [8, 0], [2049, 3]):
        assert create([widths]) == EINVAL and b"1..2048" in lib.bd_last_error(), widths
    assert create([[3]], n_layers=0) == EINVAL and b"1..8" in lib.bd_last_error()
    assert create([[4] * 9]) == EINVAL and b"1..8" in lib.bd_last_error()
    assert create([[3]], first_in=512) == EINVAL and b"1024" in lib.bd_last_error()
    assert create([[8, 3]], patch={(0, 1): 9}) == EINVAL and b"layer 1" in lib.bd_last_error() and b"width before" in lib.bd_last_error()
    assert create([[8, 3], [8, 3], [8, 4]]) == EINVAL and b"member 2" in lib.bd_last_error()
    assert create([[8, 3], [9, 3]]) == EINVAL and b"member 1" in lib.bd_last_error()
    assert create([[8, 3]], acts=["softmax", "linear"]) == EINVAL and b"hidden activations" in lib.bd_last_error()
    assert create([[3]], max_batch=0) == EINVAL and create([[3]], max_batch=65537) == EINVAL
    assert create([[3]] * 4097) == EINVAL and b"4096" in lib.bd_last_error()
    # 4096 members of eight 2048-wide layers at the largest batch: some 50 TB, far past the header's cap
    assert create([[2048] * 8] * 4096, max_batch=65536) == EWORKSPACE
    message = lib.bd_last_error()
    assert b"BD_STACKBANK_MAX_WORKSPACE_BYTES" in message and b"4096 members" in message and b"2048, 2048" in message \
        and b"max_batch 65536" in message
    # ... and not far past it: a member 1024 -> 2048 -> 13 at batch 4096 needs some 245 MB (5 x 2.1 M floats of parameters, slots
    # and snapshot, 2 x 8.4 M of activations and deltas, 16 slices x 2.1 M of partials), 40 of them 9.8 GB
    assert create([[2048, 13]] * 40, max_batch=4096) == EWORKSPACE and b"40 members of widths 2048, 13" in lib.bd_last_error()
    assert handle.value is None


# ---------------------------------------------------------------------------------------------------- argument errors
def good(n=24, c=3):
    rng = np.random.default_rng(0)
    return dict(embeddings=rng.random((n, 1024), dtype=np.float32), targets=np.arange(n) % c,
                classes=[f"class_{i}" for i in range(c)], epochs=3)


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    for name in ("Trainer", "TrainerBank", "TrainerStackBank"):
        monkeypatch.setattr(train, name, refuse)
    monkeypatch.setattr(_lib, "load", refuse)


BAD_STACKS = {
    "a bad member key": (dict(members=[{}, {"dropout": 0.5}], hidden=(8,), activations=("relu",)), r"members\[1\].*dropout"),
    "a bad knob of a member": (dict(members=[{"weight_decay": -1.0}], hidden=(8,), activations=("relu",)), r"members\[0\].*weight_decay"),
    "no members": (dict(members=[], hidden=(8,), activations=("relu",)), "at least one"),
    "activations that do not match hidden": (dict(members=[{}], hidden=(8, 4), activations=("relu",)), "2 hidden widths but 1 activations"),
    "a softmax hidden layer": (dict(members=[{}], hidden=(8,), activations=("softmax",)), "softmax is not a hidden activation"),
    "an unknown activation": (dict(members=[{}], hidden=(8,), activations=("gelu",)), "gelu"),
    "a width past the engine's": (dict(members=[{}], hidden=(2049,), activations=("relu",)), "1..2048"),
    "nine layers": (dict(members=[{}], hidden=(4,) * 8, activations=("relu",) * 8), "9 layers"),
    "a weighted validation tuple": (dict(members=[{}], validation="weighted"), "validation_weight"),
}


@pytest.mark.parametrize("what", sorted(BAD_STACKS))
def test_fit_stacks_refuses_before_any_device_work(what, no_device):
    kw, message = BAD_STACKS[what]
    a = good()
    if kw.get("validation") == "weighted":
        kw = dict(kw, validation=(a["embeddings"], a["targets"], np.ones(24)))
    with pytest.raises(ValueError, match=message):
        train.fit_stacks(**a, **kw)


def cv_good(n=60, c=3):
    a = good(n, c)
    a.update(hidden=(8,), activations=("tanh",))
    return a


BAD_CV = {
    "a bad knob in the grid": (lambda a: a.update(grid=[{}, {"weight_decay": -1.0}]), r"members\[5\].*weight_decay"),
    "an unknown grid key": (lambda a: a.update(grid=[{}, {"momentum": 0.9}]), r"grid\[1\].*momentum"),
    "class_weight with the binary loss": (lambda a: a.update(loss="binary", targets=np.zeros((60, 3), np.float32), grid=[{"class_weight": "balanced"}]),
                                          r"grid\[0\].*sample_weight"),
    "fold_of_row and folds": (lambda a: a.update(fold_of_row=np.arange(60) % 3, folds=3), "not both"),
    "activations that do not match hidden": (lambda a: a.update(activations=()), "1 hidden widths but 0 activations"),
    "a softmax hidden layer": (lambda a: a.update(activations=("softmax",)), "softmax is not a hidden activation"),
    "an unknown shared argument": (lambda a: a.update(dropout=0.5), "dropout"),
    "an empty grid": (lambda a: a.update(grid=[]), "at least one"),
}


@pytest.mark.parametrize("what", sorted(BAD_CV))
def test_cross_validate_stack_refuses_before_any_device_work(what, no_device):
    change, message = BAD_CV[what]
    args = cv_good()
    change(args)
    with pytest.raises(ValueError, match=message):
        train.cross_validate_stack(**args)


def test_good_stacks_pass_the_checks_and_reach_the_stack_bank(monkeypatch):
    class Reached(Exception):
        pass

    def bank(members, loss, optimizer, learning_rate, max_batch, device):
        assert len(members) == 3 and all(m is members[0] for m in members)     # all members start equal: one set of Glorot values
        assert [k.shape for k, _, _ in members[0]] == [(1024, 8), (8, 70)] and [a for _, _, a in members[0]] == ["relu", "linear"]
        want = train.glorot_layers(np.random.default_rng(4), [8, 70], ["relu", "linear"])
        assert all(np.array_equal(k, wk) for (k, _, _), (wk, _, _) in zip(members[0], want))
        assert learning_rate == 2e-3 and max_batch == 16
        raise Reached()
    monkeypatch.setattr(train, "TrainerStackBank", bank)
    a = good(24, 70)                                        # more classes than the one-layer bank holds
    members = [{"learning_rate": [2e-3, 1e-3, 5e-4]}, {"class_weight": "balanced"}, {"early_stopping": {"patience": 1}}]
    with pytest.raises(Reached):
        train.fit_stacks(members=members, hidden=(8,), activations=("relu",), batch_size=16, seed=4, **a)
    a = good(80, 70)
    a["targets"] = np.arange(80) % 70

    def one_layer(members, loss, optimizer, learning_rate, max_batch, device):
        assert len(members) == 2 and [k.shape for k, _, _ in members[0]] == [(1024, 70)]
        raise Reached()
    monkeypatch.setattr(train, "TrainerStackBank", one_layer)
    with pytest.raises(Reached):                            # hidden=() with 70 classes: what fit_heads refuses
        train.fit_stacks(members=[{}, {}], **a)
    with pytest.raises(ValueError, match="64"):
        train.fit_heads(members=[{}, {}], **a)


# ---------------------------------------------------------------------------------------------------- the old pins
def test_the_one_layer_bank_keeps_its_pins(monkeypatch):
    a = good()
    with pytest.raises(ValueError, match="hidden"):
        train.cross_validate_head(hidden=(8,), **a)
    seen = []
    monkeypatch.setattr(train, "fit_head", lambda *args, **k: seen.append(k) or len(seen))
    monkeypatch.setattr(train, "TrainerStackBank", lambda *args, **k: pytest.fail("fit_heads(hidden=...) went to the stack bank"))
    out = train.fit_heads(members=[{"weight_decay": 1e-2}, {}], hidden=(8,), activations=("relu",), seed=4, **a)
    assert out == [1, 2] and [k["seed"] for k in seen] == [4, 4] and all(k["hidden"] == (8,) for k in seen)
    assert seen[0]["weight_decay"] == 1e-2
