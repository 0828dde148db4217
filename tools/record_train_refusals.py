"""Record what the three training families (bd_trainer_*, bd_bank_*, bd_stackbank_*) answer when they refuse a call.

    python tools/record_train_refusals.py [tests/golden/train_refusals.json]

The fixture maps a case name to ``[return code, bd_last_error() text]``.  It is recorded once, at the commit whose messages are
the contract, and ``tests/test_train_shared_host.py`` replays ``cases()`` against the library as it is built now and compares
bytes: a refactor of the host side may not move a word.  Every case is refused before a device is looked for, except the
``passes every check`` ones, which reach the device lookup (and are compared only where there is no device).
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from buzzdetect_amd import _lib  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "train_refusals.json")
NEEDS_NO_DEVICE = " passes every check"                   # suffix of the cases whose answer depends on the machine
_KERNEL = np.zeros((1024, 2048), np.float32)                # larger than any layer a case that reads it has


def _optimizer(**changes):
    values = dict(kind=1, learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7)
    values.update(changes)
    return _lib.bd_train_optimizer(values["kind"], values["learning_rate"], values["beta_1"], values["beta_2"], values["epsilon"], 0)


def _layers(members, acts=None, first_in=1024, patch=None, no_kernel=()):
    """A ``bd_head_layer`` array of ``members`` (one list of widths each), layer l reading the width before it unless
    ``patch`` = {(member, layer): n_in}; ``acts`` = {(member, layer): name} (default relu); ``no_kernel``: (member, layer)s."""
    arr = (_lib.bd_head_layer * max(1, sum(len(m) for m in members)))()
    i = 0
    for m, widths in enumerate(members):
        for l, w in enumerate(widths):
            if (m, l) not in no_kernel:
                arr[i].kernel = _KERNEL.ctypes.data_as(C.POINTER(C.c_float))
            arr[i].n_in = (patch or {}).get((m, l), first_in if l == 0 else widths[l - 1])
            arr[i].n_out = w
            arr[i].activation = _lib.HEAD_ACTIVATIONS[(acts or {}).get((m, l), "relu")]
            i += 1
    return arr


def cases(lib):
    """({name: a call that returns the entry point's return code and leaves its message in ``bd_last_error()``}, the handle
    every ``*_create`` among them writes to: still None after a refusal)."""
    handle, word = C.c_void_p(), C.c_float()
    opt = _optimizer()
    one = (_lib.bd_head_layer * 1)()
    out = {}

    # ---- null handles and null arguments, as the three refuses-null tests call them
    nulls = {
        "bd_trainer_create": lambda: lib.bd_trainer_create(0, None, 1, 0, C.byref(opt), 256, C.byref(handle)),
        "bd_trainer_step": lambda: lib.bd_trainer_step(None, None, 1024, None, None, 1, None),
        "bd_trainer_loss": lambda: lib.bd_trainer_loss(None, None, 1024, None, None, 1, None, None),
        "bd_trainer_step_weighted": lambda: lib.bd_trainer_step_weighted(None, None, 1024, None, None, None, 1, None),
        "bd_trainer_loss_weighted": lambda: lib.bd_trainer_loss_weighted(None, None, 1024, None, None, None, 1, None, None),
        "bd_trainer_set_weight_decay": lambda: lib.bd_trainer_set_weight_decay(None, 0.0),
        "bd_trainer_set_learning_rate": lambda: lib.bd_trainer_set_learning_rate(None, 1e-3),
        "bd_trainer_snapshot": lambda: lib.bd_trainer_snapshot(None, None),
        "bd_trainer_restore": lambda: lib.bd_trainer_restore(None, None),
        "bd_trainer_gradients": lambda: lib.bd_trainer_gradients(None, 0, None, None),
        "bd_trainer_read": lambda: lib.bd_trainer_read(None, 0, None, None),
        "bd_trainer_logits": lambda: lib.bd_trainer_logits(None, 1, None),
        "bd_trainer_mean_loss": lambda: lib.bd_trainer_mean_loss(None, 0, C.byref(word)),
        "bd_trainer_set_fusion": lambda: lib.bd_trainer_set_fusion(None, 1),
        "bd_trainer_workspace_floats": lambda: lib.bd_trainer_workspace_floats(None),
        "bd_trainer_workspace_fill": lambda: lib.bd_trainer_workspace_fill(None, 0),
        "bd_trainer_workspace_read": lambda: lib.bd_trainer_workspace_read(None, None, 0),
    }
    for family in ("bd_bank_", "bd_stackbank_"):
        f = lambda name, family=family: getattr(lib, family + name)     # noqa: E731
        layer_args = (0,) if family == "bd_stackbank_" else ()          # the stack bank's calls name a layer, its create n_layers
        nulls.update({
            family + "create": lambda f=f, n=len(layer_args) * (1,): f("create")(0, None, 1, *n, 0, C.byref(opt), 256, C.byref(handle)),
            family + "step": lambda f=f: f("step")(None, None, 1024, None, None, None, 0, 1, None),
            family + "loss": lambda f=f: f("loss")(None, None, 1024, None, None, None, 0, 1, None, None),
            family + "forward": lambda f=f: f("forward")(None, None, 1024, None, 1, None, 64, None),
            family + "set_learning_rate": lambda f=f: f("set_learning_rate")(None, 0, 1e-3),
            family + "set_weight_decay": lambda f=f: f("set_weight_decay")(None, 0, 0.0),
            family + "set_frozen": lambda f=f: f("set_frozen")(None, 0, 1),
            family + "snapshot": lambda f=f: f("snapshot")(None, 0, None),
            family + "restore": lambda f=f: f("restore")(None, 0, None),
            family + "read": lambda f=f, layer_args=layer_args: f("read")(None, 0, *layer_args, None, None),
            family + "gradients": lambda f=f, layer_args=layer_args: f("gradients")(None, 0, *layer_args, None, None),
            family + "mean_loss": lambda f=f: f("mean_loss")(None, 0, C.byref(word)),
            family + "workspace_floats": lambda f=f: f("workspace_floats")(None),
            family + "workspace_fill": lambda f=f: f("workspace_fill")(None, 0),
            family + "workspace_read": lambda f=f: f("workspace_read")(None, None, 0),
        })
    for name, call in nulls.items():
        out[name + ": null"] = call
    out["bd_trainer_create: null optimizer"] = lambda: lib.bd_trainer_create(0, one, 1, 0, None, 256, C.byref(handle))
    out["bd_trainer_create: null out"] = lambda: lib.bd_trainer_create(0, one, 1, 0, C.byref(opt), 256, None)
    out["bd_bank_create: null optimizer"] = lambda: lib.bd_bank_create(0, one, 1, 0, None, 256, C.byref(handle))
    out["bd_bank_create: null out"] = lambda: lib.bd_bank_create(0, one, 1, 0, C.byref(opt), 256, None)
    out["bd_stackbank_create: null optimizer"] = lambda: lib.bd_stackbank_create(0, one, 1, 1, 0, None, 256, C.byref(handle))
    out["bd_stackbank_create: null out"] = lambda: lib.bd_stackbank_create(0, one, 1, 1, 0, C.byref(opt), 256, None)

    # ---- what *_create refuses on its numbers, before it looks for a device
    def trainer(widths=(3,), loss=0, max_batch=256, n_layers=None, o=None, **layers):
        arr = _layers([list(widths)], **layers)
        o = o if o is not None else opt
        return lambda: lib.bd_trainer_create(0, arr, len(widths) if n_layers is None else n_layers, loss, C.byref(o), max_batch,
                                             C.byref(handle))

    def bank(widths=(3,), loss=0, max_batch=256, n_members=None, o=None, **layers):
        arr = _layers([[w] for w in widths], **layers)
        o = o if o is not None else opt
        return lambda: lib.bd_bank_create(0, arr, len(widths) if n_members is None else n_members, loss, C.byref(o), max_batch,
                                          C.byref(handle))

    def stackbank(members=((3,),), loss=0, max_batch=256, n_layers=None, n_members=None, o=None, **layers):
        arr = _layers([list(m) for m in members], **layers)
        o = o if o is not None else opt
        return lambda: lib.bd_stackbank_create(0, arr, len(members) if n_members is None else n_members,
                                               len(members[0]) if n_layers is None else n_layers, loss, C.byref(o), max_batch,
                                               C.byref(handle))

    for who, create in (("bd_trainer_create", trainer), ("bd_bank_create", bank), ("bd_stackbank_create", stackbank)):
        out[who + ": loss 2"] = create(loss=2)
        out[who + ": optimizer kind 2"] = create(o=_optimizer(kind=2))
        out[who + ": rate 0"] = create(o=_optimizer(learning_rate=0.0))
        out[who + ": rate NaN"] = create(o=_optimizer(learning_rate=float("nan")))
        out[who + ": rate inf"] = create(o=_optimizer(learning_rate=float("inf")))
        out[who + ": Adam beta_1 1"] = create(o=_optimizer(beta_1=1.0))
        out[who + ": Adam beta_2 -0.1"] = create(o=_optimizer(beta_2=-0.1))
        out[who + ": Adam epsilon 0"] = create(o=_optimizer(epsilon=0.0))
        out[who + ": max_batch 0"] = create(max_batch=0)
        out[who + ": max_batch 65537"] = create(max_batch=65537)
        out[who + ": first n_in 512"] = create(first_in=512)
        out[who + ": no kernel"] = create(no_kernel={(0, 0)})
        out[who + NEEDS_NO_DEVICE] = create()
    for who, create, wrap in (("bd_trainer_create", trainer, lambda w: w), ("bd_stackbank_create", stackbank, lambda w: (w,))):
        out[who + ": n_layers 0"] = create(n_layers=0)
        out[who + ": n_layers 9"] = create(wrap((4,) * 9))
        out[who + ": width 0"] = create(wrap((0,)))
        out[who + ": width 2049"] = create(wrap((2049,)))
        out[who + ": hidden width 0"] = create(wrap((0, 3)))
        out[who + ": hidden width 2049"] = create(wrap((2049, 3)))
        out[who + ": last width 0"] = create(wrap((8, 0)))
        out[who + ": broken n_in chain"] = create(wrap((8, 3)), patch={(0, 1): 9})
        out[who + ": softmax on a hidden layer"] = create(wrap((8, 3)), acts={(0, 0): "softmax", (0, 1): "linear"})
        out[who + ": no kernel in layer 1"] = create(wrap((8, 3)), no_kernel={(0, 1)})
    for who, create, member in (("bd_bank_create", bank, 3), ("bd_stackbank_create", stackbank, (3,))):
        out[who + ": 0 members"] = create(n_members=0)
        out[who + ": 4097 members"] = create((member,) * 4097)
    out["bd_bank_create: n_out 0"] = bank((0,))
    out["bd_bank_create: n_out 65"] = bank((65,))
    out["bd_bank_create: member 1 of another width"] = bank((3, 4))
    out["bd_bank_create: member 2 without a kernel"] = bank((3, 3, 3), no_kernel={(2, 0)})
    out["bd_bank_create: workspace of 4096 members"] = bank((64,) * 4096, max_batch=65536)
    out["bd_stackbank_create: member 2 of another width"] = stackbank(((8, 3), (8, 3), (8, 4)))
    out["bd_stackbank_create: member 1 of another hidden width"] = stackbank(((8, 3), (9, 3)))
    out["bd_stackbank_create: member 1 of another hidden activation"] = stackbank(((8, 3), (8, 3)), acts={(1, 0): "tanh"})
    out["bd_stackbank_create: member 2, layer 1 with a broken n_in chain"] = stackbank(((8, 3),) * 3, patch={(2, 1): 9})
    out["bd_stackbank_create: workspace of 4096 members"] = stackbank(((2048,) * 8,) * 4096, max_batch=65536)
    out["bd_stackbank_create: workspace of 40 members"] = stackbank(((2048, 13),) * 40, max_batch=4096)
    return out, handle


def record(lib):
    """{case: [return code, message]}; a handle a case created (a machine with a device) is destroyed again."""
    table, handle = cases(lib)
    result = {}
    for name, call in table.items():
        rc = int(call())
        result[name] = [rc, lib.bd_last_error().decode() if rc < 0 else ""]
        if handle.value:
            getattr(lib, name.split("create")[0] + "destroy")(handle)
            handle.value = None
    return result


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(path, "w") as f:
        json.dump(record(_lib.load()), f, indent=1, sort_keys=True)
        f.write("\n")
    print(path)
