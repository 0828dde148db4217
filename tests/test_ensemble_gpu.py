"""Ensembles of heads on the GPU (include/buzzdetect_ensemble.h, csrc/ensemble.hip): an engine that carries ensembles against a
plain set engine of the same members.  `mean` is bit identity with bd_ensemble_combine_host of the plain set's rows;
`mean_probability` sits within 8 x the float32 error of the float64 statement of the same rows (train.combine_logits: the bound
is the number format's error on these very rows, not a constant).  Pass-through units keep the bits of their lone engines, and an
engine without an ensemble runs the launches it always ran."""
import ctypes as C

import numpy as np
import pytest

from buzzdetect_amd import _lib, modeldir as G, train as T, weights as W
from oracle import yamnet_oracle as O

pytestmark = pytest.mark.gpu

HOP = 15360
MODES = ("f32", "f16x3", "f16")
WINDOW_COUNTS = (1, 31, 33, 64, 65, 1025)        # the combine kernel's 4-row workgroup edges, a full pass + a ragged pass of one
EINVAL = -1

# members: name -> (members, widths, activations).  Both routes of a set: one linear layer of at most 64 outputs runs on the fused
# kernel, everything else as a stack.
GROUPS = {
    "fused13": (3, [13], ["linear"]),
    "fused64": (2, [64], ["linear"]),
    "stack_33_2": (3, [33, 2], ["relu", "linear"]),
    "lin65": (2, [65], ["linear"]),                  # stack route, a single layer
    "softmax_64_7": (2, [64, 7], ["relu", "softmax"]),   # `mean` only: the soft vote takes linear last layers
}
COMBINES = (("mean", None), ("mean_probability", "softmax"), ("mean_probability", "sigmoid"))


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def head(widths, acts, seed):
    return W.HeadWeights(G.glorot_layers(widths, acts, seed=seed), [f"c{i}" for i in range(widths[-1])])


def members_of(group, seed0=300):
    k, widths, acts = GROUPS[group]
    base = seed0 + 10 * list(GROUPS).index(group)
    return {f"m{i}": head(widths, acts, base + i) for i in range(k)}


def ensemble_of(members, combine, link):
    first = next(iter(members.values()))
    return W.EnsembleWeights(dict(members), combine, link, list(first.classes))


def combine_host(wide, groups):
    """bd_ensemble_combine_host of wide rows: groups = [(members, width, combine, link)] in the rows' order."""
    lib = _lib.load()
    outs = (_lib.bd_ensemble_output * len(groups))()
    first, at = [0], 0
    for o, (k, width, combine, link) in enumerate(groups):
        outs[o].first_member, outs[o].n_members = at, k
        outs[o].combine, outs[o].link = _lib.COMBINE_KINDS[combine], _lib.LINKS[link]
        at += k
        for _ in range(k):
            first.append(first[-1] + width)
    wide = np.ascontiguousarray(wide, dtype=np.float32)
    assert wide.shape[1] == first[-1]
    out = np.empty((wide.shape[0], sum(g[1] for g in groups)), np.float32)
    mf = (C.c_int32 * len(first))(*first)
    _lib.check(lib.bd_ensemble_combine_host(wide.ctypes.data, wide.shape[0], wide.shape[1], outs, len(groups), mf, out.ctypes.data,
                                            out.shape[1]))
    return out


def check_unit(got, wide, k, combine, link, what):
    """One ensemble's rows `got` against its members' rows `wide` = [windows, k * c] from a plain set."""
    n, c = got.shape
    if combine == "mean":
        assert same_bytes(np.ascontiguousarray(got), combine_host(wide, [(k, c, "mean", None)])), f"{what}: mean differs from the host combine"
        return None
    z = wide.reshape(n, k, c)
    ref = T.combine_logits(z, combine, link, dtype=np.float64)
    bound = 8.0 * float(np.abs(T.combine_logits(z, combine, link, dtype=np.float32).astype(np.float64) - ref).max())
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{what}: error {err:.3g}, bound {bound:.3g}, {8 * err / bound if bound else float('nan'):.2f} x the float32 statement's error")
    assert np.isfinite(got).all() and err <= bound, f"{what}: {err} > {bound}"
    return err, bound


@pytest.fixture(scope="module")
def audio():
    return O.synthetic_audio(HOP * 1025 + 240, seed=77)


@pytest.fixture(scope="module")
def engines(audio):
    """`plain`: every member of GROUPS as a set without an ensemble.  `big`: one unit per (group, combine) - 13 ensembles over 32
    members, 923 wide columns reduced to 439 public ones."""
    from buzzdetect_amd.engine import HipEngine
    plain_heads, units = {}, {}
    for group in GROUPS:
        for m, h in members_of(group).items():
            plain_heads[f"{group}/{m}"] = h
    for combine, link in COMBINES:
        for group in GROUPS:
            if combine == "mean" or group != "softmax_64_7":
                units[f"{group}:{combine}:{link}"] = ensemble_of(members_of(group), combine, link)
    plain = HipEngine(modelname=None, heads=plain_heads)
    big = HipEngine(modelname=None, heads=units)
    yield plain, big, units
    plain.close()
    big.close()


def test_the_engine_describes_its_units(engines):
    plain, big, units = engines
    lib = big._lib
    assert plain.members is not None and lib.bd_ensemble_count(plain._handle) == 0 == lib.bd_ensemble_outputs(plain._handle)
    assert list(big.members) == list(units) and big.head is None
    public = sum(len(u.classes) for u in units.values())
    wide = sum(len(u.classes) * len(u.members) for u in units.values())
    assert big.n_classes == public == len(big.classes) == lib.bd_ensemble_outputs(big._handle) == 439
    assert lib.bd_headset_outputs(big._handle) == wide == 923 and lib.bd_headset_members(big._handle) == 32
    assert lib.bd_ensemble_count(big._handle) == len(units) == 13
    at, first, count = 0, C.c_int32(), C.c_int32()
    for o, (name, u) in enumerate(units.items()):
        assert big.member_columns[name] == slice(at, at + len(u.classes))
        assert lib.bd_ensemble_columns(big._handle, o, C.byref(first), C.byref(count)) == 0
        assert (first.value, count.value) == (at, len(u.classes))
        at += len(u.classes)
    assert lib.bd_ensemble_columns(big._handle, 13, C.byref(first), C.byref(count)) == EINVAL
    # the workspace is the one a set already takes
    assert lib.bd_workspace_bytes(big._handle, HOP * 1025 + 240, HOP, 96) == lib.bd_workspace_bytes(plain._handle, HOP * 1025 + 240, HOP, 96)


@pytest.mark.parametrize("windows", WINDOW_COUNTS)
@pytest.mark.parametrize("mode", MODES)
def test_every_ensemble_is_the_combine_of_the_plain_sets_rows(engines, audio, mode, windows):
    plain, big, units = engines
    x = audio[: HOP * windows + 240]
    for eng in (plain, big):
        eng.set_pointwise_mode(mode)
    wide = plain.split(plain.predict(x, 0.96))
    rows = big.predict(x, 0.96).numpy()
    assert rows.shape == (windows, 439) and rows.dtype == np.float32 and np.isfinite(rows).all()
    for name, got in big.split(rows).items():
        group, combine, link = name.split(":")
        k = GROUPS[group][0]
        member_rows = np.concatenate([wide[f"{group}/m{i}"] for i in range(k)], axis=1)
        check_unit(got, member_rows, k, combine, None if link == "None" else link, f"{name} ({mode}, {windows} windows)")


@pytest.mark.parametrize("k", (1, 2, 5, 20))
def test_k_members_of_13_classes(audio, k):
    """K x (1024 -> 13) under the three combines in one engine; K = 20 puts 3 x 260 wide columns into 3 x 13 public ones."""
    from buzzdetect_amd.engine import HipEngine
    x = audio[: HOP * 65 + 240]
    members = {f"m{i}": head([13], ["linear"], 500 + i) for i in range(k)}
    plain = HipEngine(modelname=None, heads=members)
    try:
        wide = plain.predict(x, 0.96).numpy().copy()
    finally:
        plain.close()
    assert wide.shape == (65, 13 * k)
    eng = HipEngine(modelname=None, heads={f"{c}:{l}": ensemble_of(members, c, l) for c, l in COMBINES})
    try:
        assert eng._lib.bd_headset_outputs(eng._handle) == 3 * 13 * k and eng.n_classes == 39
        parts = eng.split(eng.predict(x, 0.96))
    finally:
        eng.close()
    for (combine, link), got in zip(COMBINES, parts.values()):
        check_unit(got, wide, k, combine, link, f"K={k} {combine}/{link}")
    if k == 1:
        assert same_bytes(np.ascontiguousarray(parts["mean:None"]), wide)          # a mean of one is the member


# ---------------------------------------------------------------------------------------------------- model directories, mixed sets
MIXED = ["model_general_v3", "cv3", "stack", "cv2"]


@pytest.fixture(scope="module")
def mixed(tmp_path_factory, audio):
    """models/: an ensemble of 3 and one of 2 (written by save_ensemble), a plain stack; the packaged model beside them.  The set
    in both orders, and every unit's lone engine with its rows at 65 windows per mode."""
    from buzzdetect_amd.engine import HipEngine
    root = tmp_path_factory.mktemp("ensemble_models")
    T.save_ensemble(str(root / "cv3"), list(members_of("fused13").values()), combine="mean_probability", link="softmax",
                    names=["fold0", "fold1", "fold2"])
    T.save_ensemble(str(root / "cv2"), [head([40, 5], ["tanh", "linear"], 71), head([24, 5], ["relu", "linear"], 72)])
    G.write_model_dir(str(root / "stack"), G.glorot_layers([33, 2], ["relu", "linear"], seed=73))
    mp = pytest.MonkeyPatch()
    mp.setenv("BUZZDETECT_MODELS_DIR", str(root))
    x = audio[: HOP * 65 + 240]
    lone, rows = {}, {}
    for name in MIXED:
        lone[name] = HipEngine(modelname=name)
        for mode in MODES:
            lone[name].set_pointwise_mode(mode)
            rows[name, mode] = lone[name].predict(x, 0.96).numpy().copy()
    fwd, rev = HipEngine(modelname=MIXED), HipEngine(modelname=MIXED[::-1])
    yield fwd, rev, lone, rows, x
    for e in [fwd, rev] + list(lone.values()):
        e.close()
    mp.undo()


def test_an_ensemble_directory_is_an_ordinary_model(mixed):
    fwd, _, lone, rows, _ = mixed
    eng = lone["cv3"]
    assert isinstance(eng.head, W.EnsembleWeights) and eng.members is None and eng.member_columns is None
    assert eng.classes == [f"c{i}" for i in range(13)] and eng.n_classes == 13 and rows["cv3", "f32"].shape == (65, 13)
    assert eng._lib.bd_headset_members(eng._handle) == 3 and eng._lib.bd_ensemble_outputs(eng._handle) == 13
    assert eng._lib.bd_head_outputs(eng._handle) == 0
    with pytest.raises(RuntimeError, match="split"):
        eng.split(rows["cv3", "f32"])
    assert list(fwd.members) == MIXED and isinstance(fwd.members["cv2"], W.EnsembleWeights)
    assert fwd.member_columns == {"model_general_v3": slice(0, 13), "cv3": slice(13, 26), "stack": slice(26, 28), "cv2": slice(28, 33)}
    assert fwd.classes[13] == "cv3/c0" and fwd._lib.bd_headset_members(fwd._handle) == 7


@pytest.mark.parametrize("mode", MODES)
def test_every_unit_of_a_mixed_set_has_the_bits_of_its_lone_engine_in_both_orders(mixed, mode):
    fwd, rev, _, rows, x = mixed
    for eng in (fwd, rev):
        eng.set_pointwise_mode(mode)
        parts = eng.split(eng.predict(x, 0.96))
        assert list(parts) == list(eng.members)
        for name, got in parts.items():
            assert same_bytes(np.ascontiguousarray(got), rows[name, mode]), \
                f"{name} ({'reversed' if eng is rev else 'forward'} set, {mode}) differs from its lone engine"
    assert not same_bytes(rows["cv3", mode], rows["model_general_v3", mode])


def test_a_lone_ensemble_is_the_combine_of_its_members_lone_predictions(mixed):
    from buzzdetect_amd.engine import HipEngine
    _, _, lone, rows, x = mixed
    alone = []
    for h in lone["cv2"].head.members.values():
        eng = HipEngine(modelname=None, head=h)
        try:
            alone.append(eng.predict(x, 0.96).numpy().copy())
        finally:
            eng.close()
    assert same_bytes(rows["cv2", "f16x3"], combine_host(np.concatenate(alone, axis=1), [(2, 5, "mean", None)]))


def test_nothing_outside_the_rows_is_written(mixed, audio):
    import torch
    fwd, _, _, _, _ = mixed
    fwd.set_pointwise_mode("f16x3")
    windows, total = 33, fwd.n_classes
    front = (total + 3) // 4 * 4
    buf = torch.full((front + (windows + 1) * total,), -7777.25, dtype=torch.float32, device=fwd.device)
    out = buf[front: front + windows * total].view(windows, total)
    with torch.cuda.device(fwd.device):
        fwd.launch([fwd.to_device(audio[: HOP * windows + 240])], HOP, 96, False, True, out=out)
        torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:front] == -7777.25).all() and (host[front + windows * total:] == -7777.25).all()
    assert not (host[front: front + windows * total] == -7777.25).any()


def test_the_same_call_twice_and_two_engines_on_two_streams(mixed):
    import torch
    from buzzdetect_amd.engine import HipEngine
    fwd, _, _, _, x = mixed
    fwd.set_pointwise_mode("f16x3")
    first = fwd.predict(x, 0.96).numpy().copy()
    assert same_bytes(first, fwd.predict(x, 0.96).numpy())
    other = HipEngine(modelname=MIXED)
    try:
        s1, s2 = torch.cuda.Stream(fwd.device), torch.cuda.Stream(fwd.device)
        with torch.cuda.stream(s1):
            a = fwd.predict(x, 0.96)
        with torch.cuda.stream(s2):
            b = other.predict(x, 0.96)
        assert same_bytes(a.numpy(), first) and same_bytes(b.numpy(), first)
    finally:
        other.close()


@pytest.mark.parametrize("mode", ("f32", "f16x3"))
def test_a_window_gives_the_same_rows_alone_and_inside_1025(engines, audio, mode):
    _, big, _ = engines
    big.set_pointwise_mode(mode)
    inside = big.predict(audio, 0.96).numpy().copy()
    assert inside.shape == (1025, 439)
    for k in (0, 517, 1023, 1024):
        alone = big.predict(audio[HOP * k: HOP * k + 15600], 0.96).numpy()
        assert same_bytes(alone[0], inside[k]), f"window {k} alone differs from itself inside 1025 windows"


def test_embeddings_and_logits_together(engines, audio):
    plain, big, _ = engines
    x = audio[: HOP * 65 + 240]
    for mode in ("f32", "f16x3"):
        for eng in (plain, big):
            eng.set_pointwise_mode(mode)
        logits, embs = big.predict_batch([x], 0.96, want_embeddings=True)
        _, plain_embs = plain.predict_batch([x], 0.96, want_embeddings=True)
        assert embs[0].numpy().shape == (65, 1024) and same_bytes(embs[0].numpy(), plain_embs[0].numpy())
        assert same_bytes(logits[0].numpy(), big.predict(x, 0.96).numpy())


def test_the_one_kernel_per_op_plan_gives_the_default_plans_bits(engines, audio):
    """bd_set_fusion(0, 0) ends a pass in walk_layers: the set's scratch, the wide row included, sits behind the pooled rows in
    the smaller of the two buffers."""
    _, big, _ = engines
    x = audio[: HOP * 65 + 240]
    big.set_pointwise_mode("f16x3")
    want = big.predict(x, 0.96).numpy().copy()
    big.set_fusion(stem=False, separable=False)
    try:
        assert same_bytes(big.predict(x, 0.96).numpy(), want)
    finally:
        big.set_fusion()


def slot28(eng, x):
    """Launches in profile slot 28 (the head) of one predict."""
    eng.profile_enable(True)
    try:
        eng.profile_read()
        rows = eng.predict(x, 0.96).numpy().copy()
        _, launches = eng.profile_read()
    finally:
        eng.profile_enable(False)
    return int(launches[28]), rows


def test_an_engine_without_an_ensemble_never_runs_the_combine_launch(engines, mixed, audio):
    plain, big, _ = engines
    _, _, lone, rows, x = mixed
    for eng in (plain, big, lone["model_general_v3"], lone["stack"], lone["cv3"]):
        eng.set_pointwise_mode("f16x3")
    # the packaged model: the fused head, one launch; a lone stack: one per layer - and the bytes of an unprofiled run
    n, got = slot28(lone["model_general_v3"], x)
    assert n == 1 and same_bytes(got, rows["model_general_v3", "f16x3"])
    n, got = slot28(lone["stack"], x)
    assert n == 2 and same_bytes(got, rows["stack", "f16x3"])
    # a plain set: one launch per depth of its deepest stack (2), the softmax rows, the fused members - whatever its size
    n_plain, _ = slot28(plain, x[: HOP * 65 + 240])
    assert n_plain == 2 + 1 + 1
    # an ensemble: the same, and the combine - one more, whatever the number of members and outputs
    n_big, _ = slot28(big, x)
    assert n_big == n_plain + 1
    n, _ = slot28(lone["cv3"], x)                      # three fused members, one output: the fused launch and the combine
    assert n == 2


# ---------------------------------------------------------------------------------------------------- C-side refusals
def attach_set(eng, stacks):
    arr = (_lib.bd_headset_member * len(stacks))()
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
    _lib.check(eng._lib.bd_headset_attach(eng._handle, arr, len(stacks)))


def attach_ensemble(eng, specs):
    """bd_ensemble_attach with specs = [(first_member, n_members, combine, link)] (codes): (return code, bd_last_error)."""
    outs = (_lib.bd_ensemble_output * max(len(specs), 1))()
    for o, (first, k, combine, link) in enumerate(specs):
        outs[o].first_member, outs[o].n_members, outs[o].combine, outs[o].link = first, k, combine, link
    rc = eng._lib.bd_ensemble_attach(eng._handle, outs, len(specs))
    return rc, eng._lib.bd_last_error().decode()


NONE, MEAN, PROB = 0, 1, 2
SOFTMAX, SIGMOID = 1, 2
# the set under every refusal: 0, 1 linear 13; 2 linear 5; 3 sigmoid 13; 4, 5 relu -> softmax 7
REFUSAL_SET = [([13], ["linear"]), ([13], ["linear"]), ([5], ["linear"]), ([13], ["sigmoid"]), ([8, 7], ["relu", "softmax"]),
               ([8, 7], ["relu", "softmax"])]
TAIL = [(2, 1, NONE, 0), (3, 1, NONE, 0), (4, 2, MEAN, 0)]
REFUSED = {
    "no output": ([], "1..64 outputs, not 0"),
    "a gap": ([(0, 1, NONE, 0), (2, 1, NONE, 0)], "output 1 starts at member 2, the outputs before it end at member 1"),
    "an overlap": ([(0, 2, MEAN, 0), (1, 1, NONE, 0)], "output 1 starts at member 1, the outputs before it end at member 2"),
    "members left over": ([(0, 2, MEAN, 0)] + TAIL[:2], "the outputs cover members 0..3, the set has 6"),
    "members beyond the set": ([(0, 2, MEAN, 0)] + TAIL[:2] + [(4, 3, MEAN, 0)], "output 3 takes members 4..6, the set has 6"),
    "no member": ([(0, 0, MEAN, 0)], "output 0 has 0 members"),
    "different widths": ([(0, 3, MEAN, 0)], "output 0: member 2 gives 5 outputs, member 0 gives 13"),
    "different widths in output 2": ([(0, 2, MEAN, 0), (2, 1, NONE, 0), (3, 2, MEAN, 0)], "output 2: member 4 gives 7 outputs, member 3 gives 13"),
    "mean_probability over a sigmoid": ([(0, 2, MEAN, 0), (2, 1, NONE, 0), (3, 1, PROB, SIGMOID), (4, 2, MEAN, 0)],
                                        "output 2: BD_COMBINE_MEAN_PROBABILITY takes members whose last layer is linear; member 3"),
    "mean_probability over a softmax": ([(0, 2, MEAN, 0), (2, 1, NONE, 0), (3, 1, NONE, 0), (4, 2, PROB, SOFTMAX)],
                                        "output 3: BD_COMBINE_MEAN_PROBABILITY takes members whose last layer is linear; member 4"),
    "mean_probability without a link": ([(0, 2, PROB, 0)] + TAIL, "output 0: BD_COMBINE_MEAN_PROBABILITY needs a link"),
    "an unknown combine": ([(0, 2, 3, 0)] + TAIL, "output 0: unknown combine 3"),
    "an unknown link": ([(0, 2, PROB, 3)] + TAIL, "output 0: unknown link 3"),
    "none with two members": ([(0, 2, NONE, 0)] + TAIL, "output 0: BD_COMBINE_NONE passes one member through, not 2"),
}


def test_the_library_refuses_and_the_engine_stays_usable(audio):
    from buzzdetect_amd.engine import HipEngine
    x = audio[: HOP * 5 + 240]
    eng = HipEngine(modelname=None)
    try:
        rc, said = attach_ensemble(eng, [(0, 1, NONE, 0)])
        assert rc == EINVAL and "has no set of heads" in said, said
        attach_set(eng, [G.glorot_layers(w, a, seed=600 + i) for i, (w, a) in enumerate(REFUSAL_SET)])
        eng.n_classes = 58
        before = eng.predict(x, 0.96).numpy().copy()
        for what, (specs, message) in sorted(REFUSED.items()):
            rc, said = attach_ensemble(eng, specs)
            assert rc == EINVAL and message in said, (what, said)
            assert eng._lib.bd_ensemble_count(eng._handle) == 0 == eng._lib.bd_ensemble_outputs(eng._handle), what
        assert same_bytes(eng.predict(x, 0.96).numpy(), before)              # still the plain set it was
        # members of one output whose last activations differ, at equal widths
        rc, said = attach_ensemble(eng, [(0, 2, MEAN, 0), (2, 1, NONE, 0), (3, 1, NONE, 0), (4, 2, MEAN, 0)])
        assert rc == 0, said
        rc, said = attach_ensemble(eng, [(0, 2, MEAN, 0)] + TAIL)
        assert rc == EINVAL and "already has an ensemble" in said, said
        eng.n_classes = 13 + 5 + 13 + 7
        after = eng.predict(x, 0.96).numpy()
        assert same_bytes(after[:, 13:31], before[:, 26:44])                 # the two pass-through members
        assert same_bytes(after, combine_host(before, [(2, 13, "mean", None), (1, 5, "none", None), (1, 13, "none", None),
                                                       (2, 7, "mean", None)]))
    finally:
        eng.close()
    eng = HipEngine(modelname=None)
    try:
        attach_set(eng, [G.glorot_layers([13], [a], seed=610 + i) for i, a in enumerate(("linear", "sigmoid"))])
        rc, said = attach_ensemble(eng, [(0, 2, MEAN, 0)])
        assert rc == EINVAL and "output 0: member 1 ends in activation 2, member 0 in 0" in said, said
        assert eng._lib.bd_ensemble_count(eng._handle) == 0
    finally:
        eng.close()
