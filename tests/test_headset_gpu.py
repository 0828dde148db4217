"""A set of heads behind one embedder pass on the GPU (include/buzzdetect_headset.h, csrc/headset.hip): every member's columns
against an engine that carries this member alone - the fused head for one linear layer of at most 64 outputs, bd_head_attach's
stack for everything else.  The contract is bit identity: np.array_equal on the bytes, no tolerance, in all three arithmetic
modes of the CNN, at every position of a pass."""
import ctypes as C

import numpy as np
import pytest

from buzzdetect_amd import modeldir as G
from oracle import yamnet_oracle as O

pytestmark = pytest.mark.gpu

HOP = 15360
MODES = ("f32", "f16x3", "f16")
WINDOW_COUNTS = (1, 31, 33, 64, 65, 1024, 1025)      # 32-row tile edges, 64-row workgroup edges, a full pass, + a ragged pass of one

# both routes, several depths: (widths, activations)
MIXED = {
    "lin1": ([1], ["linear"]),                        # fused route
    "lin13": ([13], ["linear"]),
    "lin32": ([32], ["linear"]),
    "lin64": ([64], ["linear"]),
    "lin65": ([65], ["linear"]),                      # stack route, a single layer
    "sig13": ([13], ["sigmoid"]),
    "relu_33_2": ([33, 2], ["relu", "linear"]),
    "tanh_relu_100_37_5": G.EXAMPLE_STACKS["tanh_relu_100_37_5"],      # K no multiple of 32 at depths 1 and 2
    "softmax_31_7": ([31, 7], ["relu", "softmax"]),
}


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def audio():
    return O.synthetic_audio(HOP * 1025 + 240, seed=77)


def write_models(root, specs, seed0=20):
    for i, (name, (widths, acts)) in enumerate(specs.items()):
        G.write_model_dir(str(root / name), G.glorot_layers(widths, acts, seed=seed0 + i))
    return str(root)


class Lone:
    """Engines that carry one model each, made on first use, and their rows per (name, mode, windows), computed once."""

    def __init__(self, models_dir, audio):
        self.models_dir, self.audio, self.engines, self.rows = models_dir, audio, {}, {}

    def engine(self, name):
        from buzzdetect_amd.engine import HipEngine
        if name not in self.engines:
            self.engines[name] = HipEngine(modelname=name, models_dir=self.models_dir)
        return self.engines[name]

    def predict(self, name, mode, windows):
        key = (name, mode, windows)
        if key not in self.rows:
            eng = self.engine(name)
            eng.set_pointwise_mode(mode)
            rows = eng.predict(self.audio[: HOP * windows + 240], 0.96).numpy().copy()
            rows.setflags(write=False)
            self.rows[key] = rows
        return self.rows[key]

    def close(self):
        for e in self.engines.values():
            e.close()


@pytest.fixture(scope="module")
def mixed(tmp_path_factory, audio):
    from buzzdetect_amd.engine import HipEngine
    models = write_models(tmp_path_factory.mktemp("headset_models"), MIXED)
    lone = Lone(models, audio)
    names = list(MIXED)
    fwd = HipEngine(modelname=names, models_dir=models)
    rev = HipEngine(modelname=names[::-1], models_dir=models)
    yield fwd, rev, lone
    for e in (fwd, rev):
        e.close()
    lone.close()


def test_the_set_describes_its_members(mixed):
    fwd, rev, lone = mixed
    total = sum(w[-1] for w, _ in MIXED.values())
    assert fwd.head is None and list(fwd.members) == list(MIXED) and fwd.n_classes == total == len(fwd.classes)
    assert fwd._lib.bd_headset_members(fwd._handle) == len(MIXED) and fwd._lib.bd_headset_outputs(fwd._handle) == total
    assert fwd._lib.bd_head_outputs(fwd._handle) == 0
    at = 0
    for name, (widths, _) in MIXED.items():
        assert fwd.member_columns[name] == slice(at, at + widths[-1])
        assert fwd.classes[at] == f"{name}/{fwd.members[name].classes[0]}"
        at += widths[-1]
    assert list(rev.member_columns) == list(MIXED)[::-1] and rev.member_columns["softmax_31_7"] == slice(0, 7)
    # the routes the lone engines take are the two the contract names
    for name in MIXED:
        eng = lone.engine(name)
        assert (eng._lib.bd_head_outputs(eng._handle) == 0) == (name in ("lin1", "lin13", "lin32", "lin64"))


@pytest.mark.parametrize("windows", WINDOW_COUNTS)
@pytest.mark.parametrize("mode", MODES)
def test_every_member_has_the_bits_of_its_lone_engine(mixed, audio, mode, windows):
    fwd, rev, lone = mixed
    x = audio[: HOP * windows + 240]
    for eng in (fwd, rev):
        eng.set_pointwise_mode(mode)
        rows = eng.predict(x, 0.96).numpy()
        assert rows.shape == (windows, eng.n_classes) and rows.dtype == np.float32
        parts = eng.split(rows)
        assert list(parts) == list(eng.members)
        for name, got in parts.items():
            ref = lone.predict(name, mode, windows)
            assert same_bytes(np.ascontiguousarray(got), ref), \
                f"{name} ({'reversed' if eng is rev else 'forward'} set, {mode}, {windows} windows) differs from its lone engine"
    assert np.isfinite(rows).all()


@pytest.mark.parametrize("mode", ("f32", "f16x3"))
def test_a_window_gives_the_same_bits_alone_and_inside_a_pass(mixed, audio, mode):
    fwd, _, _ = mixed
    fwd.set_pointwise_mode(mode)
    inside = fwd.predict(audio, 0.96).numpy().copy()
    assert inside.shape == (1025, fwd.n_classes)
    for k in (0, 517, 1023, 1024):
        alone = fwd.predict(audio[HOP * k: HOP * k + 15600], 0.96).numpy()
        assert alone.shape == (1, fwd.n_classes)
        for name, cols in fwd.member_columns.items():
            assert same_bytes(alone[0, cols], inside[k, cols]), f"{name}: window {k} alone differs from itself inside 1025 windows"


@pytest.mark.parametrize("name", ("lin13", "tanh_relu_100_37_5"))
def test_a_set_of_one_is_the_lone_engine(mixed, audio, name):
    from buzzdetect_amd.engine import HipEngine
    _, _, lone = mixed
    eng = HipEngine(modelname=[name], models_dir=lone.models_dir)
    try:
        assert eng.head is None and list(eng.members) == [name]
        for mode in MODES:
            eng.set_pointwise_mode(mode)
            got = eng.predict(audio[: HOP * 65 + 240], 0.96).numpy()
            assert same_bytes(got, lone.predict(name, mode, 65))
    finally:
        eng.close()


@pytest.mark.parametrize("mode", ("f32", "f16x3"))
def test_the_one_kernel_per_op_plan_gives_the_default_plans_bits(mixed, audio, mode):
    """bd_set_fusion(0, 0) ends a pass in walk_layers: pool alone, then the set with its scratch behind the pooled rows - the
    other way into the set."""
    _, rev, lone = mixed
    x = audio[: HOP * 65 + 240]
    rev.set_pointwise_mode(mode)
    rev.set_fusion(stem=False, separable=False)
    try:
        per_op = rev.predict(x, 0.96).numpy().copy()                            # pooled rows in the workspace
        per_op_b, _ = rev.predict_batch([x], 0.96, want_embeddings=True)        # pooled rows in the caller's embeddings
    finally:
        rev.set_fusion()
    assert same_bytes(per_op, per_op_b[0].numpy())
    for name, got in rev.split(per_op).items():
        assert same_bytes(np.ascontiguousarray(got), lone.predict(name, mode, 65)), name


def test_twenty_members(tmp_path_factory, audio):
    """20 x (1024 -> 96 -> 13): depth 0 takes 1920 of the 2048 floats the hidden activations of one depth may take."""
    from buzzdetect_amd.engine import HipEngine
    specs = {f"m{i:02d}": ([96, 13], ["relu", "linear"]) for i in range(20)}
    models = write_models(tmp_path_factory.mktemp("headset_twenty"), specs, seed0=100)
    x = audio[: HOP * 65 + 240]
    eng = HipEngine(modelname=list(specs), models_dir=models)
    try:
        parts = eng.split(eng.predict(x, 0.96))
    finally:
        eng.close()
    for name in specs:
        lone = HipEngine(modelname=name, models_dir=models)
        try:
            ref = lone.predict(x, 0.96).numpy()
        finally:
            lone.close()
        assert same_bytes(np.ascontiguousarray(parts[name]), ref), name
    assert not same_bytes(np.ascontiguousarray(parts["m00"]), np.ascontiguousarray(parts["m01"]))


def test_embeddings_and_logits_together(mixed, audio):
    from buzzdetect_amd.engine import HipEngine
    fwd, _, lone = mixed
    x = audio[: HOP * 65 + 240]
    headless = HipEngine(modelname=None)
    try:
        for mode in ("f32", "f16x3"):
            fwd.set_pointwise_mode(mode)
            headless.set_pointwise_mode(mode)
            logits, embs = fwd.predict_batch([x], 0.96, want_embeddings=True)
            assert same_bytes(embs[0].numpy(), headless.embed(x, 0.96).numpy())
            for name, got in fwd.split(logits[0]).items():
                assert same_bytes(np.ascontiguousarray(got), lone.predict(name, mode, 65)), name
    finally:
        headless.close()


def test_nothing_outside_the_rows_is_written(mixed, audio):
    import torch
    fwd, _, _ = mixed
    fwd.set_pointwise_mode("f16x3")
    windows, total = 33, fwd.n_classes
    front = (total + 3) // 4 * 4                          # a guard row in front (rounded: the rows stay 16-byte aligned) ...
    buf = torch.full((front + (windows + 1) * total,), -7777.25, dtype=torch.float32, device=fwd.device)   # ... and one behind
    assert buf.data_ptr() % 16 == 0
    out = buf[front: front + windows * total].view(windows, total)
    with torch.cuda.device(fwd.device):
        _, logits, _ = fwd.launch([fwd.to_device(audio[: HOP * windows + 240])], HOP, 96, False, True, out=out)
        torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:front] == -7777.25).all() and (host[front + windows * total:] == -7777.25).all()
    assert not (host[front: front + windows * total] == -7777.25).any()      # ... and every element inside is


def test_the_same_call_twice_and_on_a_second_engine_concurrently(mixed, audio):
    import torch
    from buzzdetect_amd.engine import HipEngine
    fwd, _, lone = mixed
    fwd.set_pointwise_mode("f16x3")
    x = audio[: HOP * 65 + 240]
    first = fwd.predict(x, 0.96).numpy().copy()
    assert same_bytes(first, fwd.predict(x, 0.96).numpy())
    other = HipEngine(modelname=list(MIXED), models_dir=lone.models_dir)
    try:
        s1, s2 = torch.cuda.Stream(fwd.device), torch.cuda.Stream(fwd.device)
        with torch.cuda.stream(s1):
            a = fwd.predict(x, 0.96)
        with torch.cuda.stream(s2):
            b = other.predict(x, 0.96)
        assert same_bytes(a.numpy(), first) and same_bytes(b.numpy(), first)
    finally:
        other.close()


# ---------------------------------------------------------------------------------------------------- C-side refusals
def attach(eng, stacks):
    """bd_headset_attach with stacks = [[(kernel, bias, activation)]]: (return code, bd_last_error)."""
    from buzzdetect_amd import _lib
    arr = (_lib.bd_headset_member * max(len(stacks), 1))()
    keep = []
    for m, layers in enumerate(stacks):
        la = (_lib.bd_head_layer * len(layers))()
        for i, (k, b, act) in enumerate(layers):
            keep += [k, b]
            la[i].kernel = k.ctypes.data_as(C.POINTER(C.c_float))
            la[i].bias = b.ctypes.data_as(C.POINTER(C.c_float))
            la[i].n_in, la[i].n_out = k.shape
            la[i].activation = _lib.HEAD_ACTIVATIONS[act]
        keep.append(la)
        arr[m].layers, arr[m].n_layers = la, len(layers)
    rc = eng._lib.bd_headset_attach(eng._handle, arr, len(stacks))
    return rc, eng._lib.bd_last_error().decode()


def small(widths, acts, seed=1):
    return G.glorot_layers(widths, acts, seed=seed)


EINVAL = -1
REFUSED = {
    "no members": (lambda: [], "1..64 members, not 0"),
    "65 members": (lambda: [small([1], ["linear"])] * 65, "1..64 members, not 65"),
    "a hidden softmax in member 3": (lambda: [small([2], ["linear"])] * 3 + [small([8, 2], ["softmax", "linear"])],
                                     "member 3 layer 0: softmax on a hidden layer"),
    "hidden widths over the limit": (lambda: [small([128, 2], ["relu", "linear"])] * 16 + [small([8, 2], ["relu", "linear"])],
                                     "depth 0: the hidden widths (each rounded up to 32) sum to 2080"),
    "outputs over the limit": (lambda: [small([1024], ["sigmoid"])] * 2 + [small([1], ["linear"])], "outputs sum to 2049"),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_the_library_refuses(what):
    from buzzdetect_amd.engine import HipEngine
    make, message = REFUSED[what]
    eng = HipEngine(modelname=None)
    try:
        rc, said = attach(eng, make())
        assert rc == EINVAL and message in said, said
        assert eng._lib.bd_headset_members(eng._handle) == 0 and eng._lib.bd_headset_outputs(eng._handle) == 0
    finally:
        eng.close()


def test_the_library_refuses_an_engine_that_has_a_head_a_stack_or_a_set(engine, mixed):
    fwd, _, lone = mixed
    member = [small([3], ["linear"])]
    rc, said = attach(engine, member)                    # the packaged fused head
    assert rc == EINVAL and "already has a head" in said and engine._lib.bd_headset_members(engine._handle) == 0
    stack = lone.engine("lin65")
    rc, said = attach(stack, member)
    assert rc == EINVAL and "already has a stack" in said and stack._lib.bd_headset_members(stack._handle) == 0
    rc, said = attach(fwd, member)
    assert rc == EINVAL and "already has a set" in said and fwd._lib.bd_headset_members(fwd._handle) == len(MIXED)
