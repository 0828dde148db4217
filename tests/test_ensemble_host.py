"""Ensembles of heads without a device (include/buzzdetect_ensemble.h): header, binding and exports agree; the host statement of
the combine pass (bd_ensemble_combine_host) against NumPy - `mean` by bits, `mean_probability` within 8 x the float32 error of
the same formulas (the rule of DESIGN.md 15: the bound is the number format's own error on these inputs, not a constant); the
model directory round trip; every refusal of the library's host side, the loader, save_ensemble and check_head_set; the writer's
view of a set that holds an ensemble."""
import ctypes as C
import json
import os
import re
import shutil
import wave

import numpy as np
import pytest

from buzzdetect_amd import _lib, build, modeldir as G, pipeline as P, results as R, train as T, weights as W

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
EINVAL = -1


def declared(header):
    text = open(os.path.join(INCLUDE, header)).read()
    return sorted(set(re.findall(r"^BD_API[^;(]*?\b(bd_[a-z_0-9]+)\s*\(", text, flags=re.M)))


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------------- the ABI
def test_header_binding_and_library_list_the_same_functions():
    build.build(verbose=False)
    lib = _lib.load()
    names = declared("buzzdetect_ensemble.h")
    assert names == sorted(_lib.ENSEMBLE_PROTOTYPES) and len(names) == 6
    raw = C.CDLL(_lib.library_path())
    for name in names:
        assert hasattr(raw, name), f"{name} not exported"
    assert lib.bd_ensemble_abi_version() == _lib.ENSEMBLE_ABI_VERSION == 1
    text = open(os.path.join(INCLUDE, "buzzdetect_ensemble.h")).read()
    assert re.search(r"#define\s+BD_ENSEMBLE_ABI_VERSION\s+1\b", text)
    for kind, code in _lib.COMBINE_KINDS.items():
        assert re.search(rf"#define\s+BD_COMBINE_{kind.upper()}\s+{code}\b", text)
    for link, code in _lib.LINKS.items():
        assert re.search(rf"#define\s+BD_LINK_{(link or 'none').upper()}\s+{code}\b", text)
    assert C.sizeof(_lib.bd_ensemble_output) == 16
    # nothing went into the headers that were there
    assert lib.bd_abi_version() == 5 and len(declared("buzzdetect_hip.h")) == 44 == len(_lib.PROTOTYPES)
    assert lib.bd_headset_abi_version() == 1 and len(declared("buzzdetect_headset.h")) == 5
    assert "ensemble.hip" in build.SOURCES and "ensemble_device.h" in build.HEADERS


# ---------------------------------------------------------------------------------------------------- the host combine
def combine_host(wide, groups, widths, ld_out=None, fill=-7777.25, member_first=None):
    """bd_ensemble_combine_host over groups = [(n_members, combine, link)] of members `widths[o]` wide each: (rc, out, message).
    `out` starts filled with `fill`."""
    lib = _lib.load()
    outs = (_lib.bd_ensemble_output * max(len(groups), 1))()
    first, at = [0], 0
    for o, ((k, combine, link), width) in enumerate(zip(groups, widths)):
        outs[o].first_member, outs[o].n_members = at, k
        outs[o].combine = _lib.COMBINE_KINDS.get(combine, combine)
        outs[o].link = _lib.LINKS.get(link, link)
        at += max(k, 0)
        for _ in range(max(k, 0)):
            first.append(first[-1] + width)
    if member_first is not None:
        first = member_first
    mf = (C.c_int32 * len(first))(*first)
    ld_out = sum(widths) if ld_out is None else ld_out
    wide = np.ascontiguousarray(wide, dtype=np.float32)
    out = np.full((wide.shape[0], ld_out), fill, np.float32)
    rc = lib.bd_ensemble_combine_host(wide.ctypes.data, wide.shape[0], wide.shape[1], outs, len(groups), mf, out.ctypes.data, ld_out)
    return rc, out, lib.bd_last_error().decode()


def mean_loop(z):
    """[N, K, C] float32: members added in order, times float32(1) / float32(K)."""
    total = z[:, 0].copy()
    for m in range(1, z.shape[1]):
        total = total + z[:, m]
    return total * (np.float32(1) / np.float32(z.shape[1]))


def special(rng, shape):
    """float32 values spread over +-10 with +-0, denormals and 1e30 sprinkled in."""
    z = rng.uniform(-10, 10, shape).astype(np.float32)
    flat = z.reshape(-1)
    picks = rng.permutation(flat.size)
    for i, v in enumerate((0.0, -0.0, 1e-45, -1e-45, 1.1e-38, -3e-39, 1e30, -1e30, 1e30)):
        flat[picks[i::9][: max(1, flat.size // 40)]] = np.float32(v)
    return z


@pytest.mark.parametrize("windows", (1, 257))
@pytest.mark.parametrize("c", (1, 13, 64, 65))
@pytest.mark.parametrize("k", (1, 2, 3, 5, 64))
def test_mean_has_the_bits_of_a_float32_loop_in_member_order(k, c, windows):
    rng = np.random.default_rng(1000 * k + 10 * c + windows)
    z = special(rng, (windows, k, c))
    rc, out, said = combine_host(z.reshape(windows, k * c), [(k, "mean", None)], [c])
    assert rc == 0, said
    with np.errstate(over="ignore"):
        ref = mean_loop(z)
    assert same_bytes(out, ref)
    assert same_bytes(T.combine_logits(z, "mean", None, dtype=np.float32), ref)
    if k == 1:
        assert same_bytes(out, z[:, 0])                      # times 1.0f: the member itself
    rc, again, _ = combine_host(z.reshape(windows, k * c), [(k, "mean", None)], [c])
    assert same_bytes(out, again)


def float32_bound(z, link):
    """8 x the largest deviation of the float32 NumPy statement from the float64 one on these inputs, and the float64 rows."""
    ref = T.combine_logits(z, "mean_probability", link, dtype=np.float64)
    f32 = T.combine_logits(z, "mean_probability", link, dtype=np.float32)
    assert f32.dtype == np.float32 and ref.dtype == np.float64
    return 8.0 * float(np.abs(f32.astype(np.float64) - ref).max()), ref


@pytest.mark.parametrize("link", ("softmax", "sigmoid"))
@pytest.mark.parametrize("c", (13, 64, 65))
@pytest.mark.parametrize("k", (1, 2, 3, 5, 64))
def test_mean_probability_sits_within_8x_the_float32_error_of_the_float64_statement(k, c, link):
    rng = np.random.default_rng(77 * k + c)
    z = rng.uniform(-10, 10, (257, k, c)).astype(np.float32)
    bound, ref = float32_bound(z, link)
    rc, out, said = combine_host(z.reshape(257, k * c), [(k, "mean_probability", link)], [c])
    assert rc == 0, said
    err = float(np.abs(out.astype(np.float64) - ref).max())
    print(f"mean_probability/{link} K={k} C={c}: error {err:.3g}, bound {bound:.3g}, ratio to the float32 statement {8 * err / bound:.2f}")
    assert bound > 0 and err <= bound
    # the float64 statement is the formula itself
    p = np.exp(z.astype(np.float64))
    if link == "softmax":
        direct = np.log((p / p.sum(2, keepdims=True)).mean(1))
    else:
        q = (p / (1 + p)).mean(1)
        direct = np.log(q) - np.log1p(-q)
    assert np.allclose(ref, direct, rtol=0, atol=1e-9)


@pytest.mark.parametrize("link", ("softmax", "sigmoid"))
def test_mean_probability_stays_finite_at_80_and_identical_members_give_the_member(link):
    rng = np.random.default_rng(5)
    c, k = 13, 5
    one = rng.choice(np.float32([-80, 80]), (64, 1, c)) + rng.uniform(-1, 1, (64, 1, c)).astype(np.float32)
    same = np.repeat(one.astype(np.float32), k, axis=1)                  # identical members
    mixed = rng.choice(np.float32([-80, 80]), (64, k, c)).astype(np.float32)     # members that contradict each other at +-80
    z = np.concatenate([same, mixed])
    bound, ref = float32_bound(z, link)
    rc, out, said = combine_host(z.reshape(128, k * c), [(k, "mean_probability", link)], [c])
    assert rc == 0, said
    assert np.isfinite(out).all() and np.isfinite(ref).all()
    assert float(np.abs(out.astype(np.float64) - ref).max()) <= bound
    m = one[:, 0].astype(np.float64)
    top = m.max(1, keepdims=True)
    own = m - (top + np.log(np.exp(m - top).sum(1, keepdims=True))) if link == "softmax" else m      # its log-softmax / its logit
    assert float(np.abs(out[:64].astype(np.float64) - own).max()) <= bound
    # the very ends of float32 stay finite too
    ends = np.float32([[[3e38, -3e38], [-3e38, 3e38]]])
    rc, out, _ = combine_host(ends.reshape(1, 4), [(2, "mean_probability", link)], [2])
    assert rc == 0 and np.isfinite(out).all()


def test_pass_through_columns_are_copied_and_nothing_else_is_written():
    rng = np.random.default_rng(9)
    # a pass-through of 7, a mean of 3 x 5, a pass-through of 65, a soft vote of 2 x 4: 7 + 15 + 65 + 8 wide, 7 + 5 + 65 + 4 public
    groups = [(1, "none", None), (3, "mean", None), (1, "none", None), (2, "mean_probability", "softmax")]
    widths = [7, 5, 65, 4]
    wide = special(rng, (33, 95))
    rc, out, said = combine_host(wide, groups, widths, ld_out=81 + 6)
    assert rc == 0, said
    assert same_bytes(out[:, :7], wide[:, :7]) and same_bytes(out[:, 12:77], wide[:, 22:87])
    with np.errstate(over="ignore"):
        assert same_bytes(out[:, 7:12], mean_loop(wide[:, 7:22].reshape(33, 3, 5)))
    assert (out[:, 81:] == -7777.25).all() and not (out[:, 77:81] == -7777.25).any()
    # a wide row with columns behind the members: the stride is ld_wide, not the members' sum
    padded = np.concatenate([wide, np.full((33, 5), 3.0, np.float32)], axis=1)
    rc, again, _ = combine_host(padded, groups, widths, ld_out=87)
    assert rc == 0 and same_bytes(again, out)


REFUSED_BY_THE_LIBRARY = {
    "no output": ([], [], "1..64 members in all, not none"),
    "no member in output 1": ([(2, "mean", None), (0, "mean", None)], [3, 3], "output 1 has 0 members, at least 1 is needed"),
    "an unknown combine": ([(2, 7, None)], [3], "output 0: unknown combine 7"),
    "an unknown link": ([(2, "mean_probability", 9)], [3], "output 0: unknown link 9"),
    "none with two members": ([(1, "none", None), (2, "none", None)], [3, 3], "output 1: BD_COMBINE_NONE passes one member through, not 2"),
    "mean_probability without a link": ([(2, "mean_probability", None)], [3], "output 0: BD_COMBINE_MEAN_PROBABILITY needs a link"),
    "a link on a mean": ([(2, "mean", "softmax")], [3], "output 0: a link goes with BD_COMBINE_MEAN_PROBABILITY only"),
}


@pytest.mark.parametrize("what", sorted(REFUSED_BY_THE_LIBRARY))
def test_the_host_combine_refuses_and_writes_nothing(what):
    groups, widths, message = REFUSED_BY_THE_LIBRARY[what]
    wide = np.ones((4, 16), np.float32)
    rc, out, said = combine_host(wide, groups, widths, ld_out=8)
    assert rc == EINVAL and message in said, said
    assert (out == -7777.25).all()


def test_the_host_combine_refuses_outputs_that_do_not_tile_the_members_and_unequal_widths():
    lib = _lib.load()
    wide = np.ones((4, 16), np.float32)
    out = np.full((4, 8), -7777.25, np.float32)

    def call(specs, first):
        outs = (_lib.bd_ensemble_output * len(specs))()
        for o, (f, k) in enumerate(specs):
            outs[o].first_member, outs[o].n_members, outs[o].combine = f, k, _lib.COMBINE_KINDS["mean"]
        mf = (C.c_int32 * len(first))(*first)
        rc = lib.bd_ensemble_combine_host(wide.ctypes.data, 4, 16, outs, len(specs), mf, out.ctypes.data, 8)
        return rc, lib.bd_last_error().decode()
    rc, said = call([(0, 2), (3, 1)], [0, 2, 4, 6, 8])                 # a gap: member 2 belongs to nobody
    assert rc == EINVAL and "output 1 starts at member 3, the outputs before it end at member 2" in said, said
    rc, said = call([(0, 2), (1, 2)], [0, 2, 4, 6, 8])                 # an overlap
    assert rc == EINVAL and "output 1 starts at member 1" in said, said
    rc, said = call([(0, 2), (2, 2)], [0, 2, 4, 6, 9])                 # widths 2, 2 | 2, 3
    assert rc == EINVAL and "output 1: member 3 gives 3 outputs, member 2 gives 2" in said, said
    rc, said = call([(0, 2)], [0, 8, 17])                              # beyond the wide row
    assert rc == EINVAL and "member 1 takes columns 8..17 of 16" in said, said
    assert (out == -7777.25).all()
    rc, said = call([(0, 2), (2, 2)], [0, 2, 4, 6, 8])
    assert rc == 0 and (out[:, :4] == 1.0).all() and (out[:, 4:] == -7777.25).all()


# ---------------------------------------------------------------------------------------------------- directory and loader
CLASSES13 = [f"c{i}" for i in range(13)]


def head(widths, acts, seed=1, embedder="yamnet_k2", classes=None):
    layers = G.glorot_layers(widths, acts, seed=seed)
    return W.HeadWeights(layers, classes or [f"c{i}" for i in range(widths[-1])], embeddername=embedder)


def test_save_ensemble_round_trips_through_load_head(tmp_path):
    fits = [head([13], ["linear"], 1), head([40, 13], ["relu", "linear"], 2), T.FitResult(head([13], ["linear"], 3), {}, None, None)]
    table = T.METRICS_HEADER + "\n0.5,0.9,0.8,0.01\n"
    path = T.save_ensemble(str(tmp_path / "model_cv"), fits, combine="mean_probability", link="softmax",
                           names=["fold0", "fold1", "fold2"], metrics=table, digits_results=3)
    assert sorted(os.listdir(path)) == ["config_model.json", "members", "model.py", "tests"]      # no variables/ at the top
    cfg = json.load(open(os.path.join(path, "config_model.json")))
    assert cfg == {"classes": CLASSES13, "embeddername": "yamnet_k2", "digits_results": 3,
                   "ensemble": {"combine": "mean_probability", "link": "softmax", "members": ["fold0", "fold1", "fold2"]}}
    assert 'modelname = "model_cv"' in open(os.path.join(path, "model.py")).read()
    ens = W.load_head("model_cv", str(tmp_path))
    assert isinstance(ens, W.EnsembleWeights) and list(ens.members) == ["fold0", "fold1", "fold2"]
    assert (ens.combine, ens.link, ens.classes, ens.embeddername, ens.digits_results) == ("mean_probability", "softmax", CLASSES13,
                                                                                          "yamnet_k2", 3)
    assert ens.fused is False and ens.source == path
    assert ens.metrics_path == os.path.join(path, "tests", "metrics.csv") and open(ens.metrics_path).read() == table
    assert R.threshold_for_precision("model_cv", 0.9, metrics_path=ens.metrics_path) == 0.5
    for got, fit in zip(ens.members.values(), fits):
        want = fit.head if isinstance(fit, T.FitResult) else fit
        assert [a for _, _, a in got.layers] == [a for _, _, a in want.layers] and got.classes == CLASSES13
        for (k1, b1, _), (k2, b2, _) in zip(got.layers, want.layers):
            assert same_bytes(k1, k2) and same_bytes(b1, b2)
    # every member is a model of its own
    for name, fit in zip(ens.members, fits):
        lone = W.load_head(name, os.path.join(path, "members"))
        assert isinstance(lone, W.HeadWeights) and same_bytes(lone.layers[0][0], ens.members[name].layers[0][0])
    # the defaults: a mean, member0 .., a metrics file with the header alone
    plain = W.load_head("m", os.path.dirname(T.save_ensemble(str(tmp_path / "m"), fits[:2])))
    assert (plain.combine, plain.link, list(plain.members)) == ("mean", None, ["member0", "member1"])
    assert open(plain.metrics_path).read() == T.METRICS_HEADER + "\n"
    # a plain model directory still loads as it did
    G.write_model_dir(str(tmp_path / "lone"), G.glorot_layers([13], ["linear"], seed=4))
    assert isinstance(W.load_head("lone", str(tmp_path)), W.HeadWeights)


SAVE_REFUSED = {
    "no fit": (lambda: [], {}, "at least one fit"),
    "different classes": (lambda: [head([13], ["linear"]), head([13], ["linear"], classes=CLASSES13[::-1])], {}, "member 'member1' has classes"),
    "different widths": (lambda: [head([13], ["linear"]), head([2], ["linear"])], {}, "member 'member1' has classes"),
    "different last activations": (lambda: [head([13], ["linear"]), head([13], ["sigmoid"])], {}, "member 'member1' ends in 'sigmoid'"),
    "an unknown combine": (lambda: [head([13], ["linear"])], {"combine": "median"}, "unknown combine 'median'"),
    "a link on a mean": (lambda: [head([13], ["linear"])], {"link": "softmax"}, "goes with combine \"mean_probability\" only"),
    "mean_probability without a link": (lambda: [head([13], ["linear"])], {"combine": "mean_probability"}, 'needs link "softmax" or "sigmoid"'),
    "an unknown link": (lambda: [head([13], ["linear"])], {"combine": "mean_probability", "link": "probit"}, "not 'probit'"),
    "mean_probability over a softmax": (lambda: [head([8, 13], ["relu", "softmax"])] * 2, {"combine": "mean_probability", "link": "softmax"},
                                        "member 'member0' ends in 'softmax'"),
    "65 members": (lambda: [head([13], ["linear"])] * 65, {}, "1..64 members, not 65"),
    "a nested ensemble": (lambda: [W.EnsembleWeights({"a": head([13], ["linear"])}, "mean", None, CLASSES13)], {}, "ensembles do not nest"),
    "names that do not fit": (lambda: [head([13], ["linear"])] * 2, {"names": ["a"]}, "a name of its own"),
    "a name with a path": (lambda: [head([13], ["linear"])], {"names": ["../a"]}, "plain directory name"),
    "hidden widths over the limit": (lambda: [head([160, 13], ["relu", "linear"])] * 13, {}, "depth 0: the hidden widths"),
}


@pytest.mark.parametrize("what", sorted(SAVE_REFUSED))
def test_save_ensemble_refuses_and_writes_nothing(what, tmp_path):
    make, kwargs, message = SAVE_REFUSED[what]
    with pytest.raises(ValueError, match=re.escape(message)):
        T.save_ensemble(str(tmp_path / "models" / "e"), make(), **kwargs)
    assert not (tmp_path / "models").exists()


@pytest.fixture()
def saved(tmp_path):
    T.save_ensemble(str(tmp_path / "e"), [head([13], ["linear"], s) for s in (1, 2, 3)], names=["a", "b", "c"])
    return tmp_path


def edit_config(path, change):
    cfg = json.load(open(path))
    change(cfg)
    json.dump(cfg, open(path, "w"))


def test_the_loader_refuses_a_missing_member_naming_it(saved):
    shutil.rmtree(saved / "e" / "members" / "b")
    with pytest.raises(W.UnsupportedHeadError, match=r"config_model\.json: member 'b' has no model directory .*members.b"):
        W.load_head("e", str(saved))


def test_the_loader_refuses_members_whose_classes_differ(saved):
    edit_config(saved / "e" / "members" / "c" / "config_model.json", lambda c: c.update(classes=CLASSES13[::-1]))
    with pytest.raises(W.UnsupportedHeadError, match=r"config_model\.json: member 'c' has classes"):
        W.load_head("e", str(saved))


def test_the_loader_refuses_classes_that_differ_from_the_ensembles(saved):
    edit_config(saved / "e" / "config_model.json", lambda c: c.update(classes=["x"] + CLASSES13[1:]))
    with pytest.raises(W.UnsupportedHeadError, match=r"member 'a' has classes"):
        W.load_head("e", str(saved))


def test_the_loader_refuses_members_on_different_embedders(saved):
    edit_config(saved / "e" / "members" / "b" / "config_model.json", lambda c: c.update(embeddername="yamnet"))
    with pytest.raises(W.UnsupportedHeadError, match=r"member 'b' is on embedder 'yamnet', the ensemble on 'yamnet_k2'"):
        W.load_head("e", str(saved))


def test_the_loader_refuses_a_nested_ensemble(saved):
    edit_config(saved / "e" / "members" / "a" / "config_model.json",
                lambda c: c.update(ensemble={"combine": "mean", "link": None, "members": ["x"]}))
    with pytest.raises(W.UnsupportedHeadError, match=r"members.a.config_model\.json: member 'a' is an ensemble itself"):
        W.load_head("e", str(saved))


def test_the_loader_refuses_more_than_64_members_before_reading_any(saved):
    edit_config(saved / "e" / "config_model.json", lambda c: c["ensemble"].update(members=[f"m{i}" for i in range(65)]))
    with pytest.raises(W.UnsupportedHeadError, match=r"1\.\.64 members, not 65"):
        W.load_head("e", str(saved))


@pytest.mark.parametrize("spec, message", [
    ({"combine": "median"}, "unknown combine 'median'"),
    ({"combine": "mean", "link": "sigmoid"}, 'goes with combine "mean_probability" only'),
    ({"combine": "mean_probability", "link": None}, 'needs link "softmax" or "sigmoid"'),
    ({"combine": "mean_probability", "link": "probit"}, "not 'probit'"),
    ({"members": "a"}, '"ensemble" must be'),
    ({"members": ["a", "a"]}, "members named twice: a"),
])
def test_the_loader_refuses_the_combine_and_link_rules(saved, spec, message):
    edit_config(saved / "e" / "config_model.json", lambda c: c["ensemble"].update(spec))
    with pytest.raises(W.UnsupportedHeadError, match=re.escape(message)) as info:
        W.load_head("e", str(saved))
    assert "config_model.json" in str(info.value)


def test_the_loader_refuses_mean_probability_over_members_that_are_not_linear(tmp_path):
    G.write_ensemble_dir(str(tmp_path / "e"), {"a": G.glorot_layers([13], ["sigmoid"], 1), "b": G.glorot_layers([13], ["sigmoid"], 2)},
                         CLASSES13, "mean_probability", "sigmoid")
    with pytest.raises(W.UnsupportedHeadError, match=r"member 'a' ends in 'sigmoid'"):
        W.load_head("e", str(tmp_path))
    edit_config(tmp_path / "e" / "config_model.json", lambda c: c["ensemble"].update(combine="mean", link=None))
    assert W.load_head("e", str(tmp_path)).combine == "mean"       # a mean takes any common last activation


# ---------------------------------------------------------------------------------------------------- sets that hold ensembles
def ensemble(k, widths, acts, seed=10, **kw):
    return W.EnsembleWeights({f"m{i}": head(widths, acts, seed + i, embedder=kw.get("embeddername", "yamnet_k2")) for i in range(k)}, kw.pop("combine", "mean"), kw.pop("link", None),
                             [f"c{i}" for i in range(widths[-1])], **kw)


def test_check_head_set_returns_the_public_columns_and_applies_the_limits_to_the_members():
    units = {"g": head([13], ["linear"]), "cv": ensemble(5, [13], ["linear"]), "s": head([33, 2], ["relu", "linear"]),
             "cv2": ensemble(2, [40, 7], ["relu", "softmax"])}
    assert W.check_head_set(units) == {"g": slice(0, 13), "cv": slice(13, 26), "s": slice(26, 28), "cv2": slice(28, 35)}
    assert list(W.expand_head_set(units)) == ["g", "cv/m0", "cv/m1", "cv/m2", "cv/m3", "cv/m4", "s", "cv2/m0", "cv2/m1"]
    # without an ensemble: what it always returned
    assert W.check_head_set({"g": units["g"], "s": units["s"]}) == {"g": slice(0, 13), "s": slice(13, 15)}
    # 13 x (1024 -> 160 -> 13): 2080 floats of hidden activations at depth 0
    with pytest.raises(ValueError, match=r"depth 0: the hidden widths \(each rounded up to 32\) sum to 2080.*cv/m0 160"):
        W.check_head_set({"cv": ensemble(13, [160, 13], ["relu", "linear"])})
    assert W.check_head_set({"cv": ensemble(12, [160, 13], ["relu", "linear"]), "g": units["g"]}) == {"cv": slice(0, 13), "g": slice(13, 26)}
    # 64 members in all, whoever they belong to
    with pytest.raises(ValueError, match="at most 64 models, not 65"):
        W.check_head_set({"a": ensemble(60, [2], ["linear"]), "b": ensemble(5, [2], ["linear"])})
    # 2048 wide outputs: 2 x 1024 are the limit, whatever the public width
    big = ensemble(2, [1024], ["sigmoid"])
    assert W.check_head_set({"big": big}) == {"big": slice(0, 1024)}
    with pytest.raises(ValueError, match="outputs sum to 2049"):
        W.check_head_set({"big": big, "one": head([1], ["linear"])})
    with pytest.raises(ValueError, match=r"share one embedder: 'g' is on 'yamnet_k2', 'cv' on 'yamnet'"):
        W.check_head_set({"g": units["g"], "cv": ensemble(2, [13], ["linear"], embeddername="yamnet")})
    with pytest.raises(W.UnsupportedHeadError, match=r"model 'cv': member 'm1' has classes"):
        bad = ensemble(2, [13], ["linear"])
        bad.members["m1"].classes = CLASSES13[::-1]
        W.check_head_set({"g": units["g"], "cv": bad})


def test_the_engine_refuses_an_ensemble_before_any_device_work(monkeypatch):
    import torch
    from buzzdetect_amd import engine as E

    def touched(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    monkeypatch.setattr(E._lib, "load", touched)
    monkeypatch.setattr(torch.cuda, "is_available", touched)
    monkeypatch.setattr(W, "load_embedder_blob", touched)
    with pytest.raises(ValueError, match="depth 0: the hidden widths"):
        E.HipEngine(head=ensemble(13, [160, 13], ["relu", "linear"]))
    with pytest.raises(ValueError, match="ends in 'softmax'"):
        E.HipEngine(heads={"g": head([13], ["linear"]),
                           "cv": ensemble(2, [8, 13], ["relu", "softmax"], combine="mean_probability", link="softmax")})


@pytest.fixture()
def folders(tmp_path):
    """models/: an ensemble of three folds with its own metrics and digits, and a plain model beside it."""
    root = tmp_path / "models"
    table = T.METRICS_HEADER + "\n1.25,0.95,0.5,0.01\n0.5,0.9,0.8,0.02\n"
    T.save_ensemble(str(root / "model_cv"), [head([2], ["linear"], s, classes=["ins_buzz", "other"]) for s in (1, 2, 3)],
                    combine="mean_probability", link="softmax", metrics=table, digits_results=3)
    G.write_model_dir(str(root / "plain"), G.glorot_layers([13], ["linear"], seed=2))
    return str(root)


def test_the_writer_sees_an_ensemble_as_one_model_of_the_set(folders, tmp_path):
    from buzzdetect_amd.analyze import member_dirs, set_members
    heads = W.load_head_set(["model_cv", "plain"], folders)
    assert isinstance(heads["model_cv"], W.EnsembleWeights)
    members = set_members(heads, "all", None)
    assert [(m.name, m.columns, m.digits_results, m.threshold) for m in members] == [("model_cv", slice(0, 2), 3, None),
                                                                                     ("plain", slice(2, 15), 2, None)]
    assert members[0].classes == ["ins_buzz", "other"] == members[0].classes_out
    det = set_members(heads, "all", 0.95)
    assert det[0].threshold == 1.25                      # from the ensemble's own tests/metrics.csv
    dirs = member_dirs(["model_cv", "plain"], str(tmp_path / "out"))
    for m in members:
        assert R.check_or_write_manifest(dirs[m.name], R.build_manifest(m.name, 1, None, m.classes_out)) == (True, None)
    lone = R.build_manifest("model_cv", 1, None, list(heads["model_cv"].classes))      # what analyze("model_cv") builds
    assert R.check_or_write_manifest(dirs["model_cv"], lone) == (True, None)
    with pytest.raises(ValueError, match=r"model 'model_cv' has no class 'c0'"):
        set_members(heads, ["c0"], None)


def test_the_planner_resumes_an_ensemble_and_a_plain_model_each_by_its_own_files(folders, tmp_path):
    from buzzdetect_amd.analyze import set_jobs, set_members
    with wave.open(str(tmp_path / "rec.wav"), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.zeros(int(16000 * 25.0), "<i2").tobytes())
    members = set_members(W.load_head_set(["model_cv", "plain"], folders), "all", None)
    pipe = P.Pipeline(make_engine=None, classes=["model_cv/ins_buzz", "model_cv/other"] + [f"plain/c{i}" for i in range(13)],
                      framehop_s=0.96, hop=15360, step=96, chunklength=9.6, framelength_s=0.96, digits_time=2, digits_results=3,
                      classes_out="all", threshold=None, readers=1, analyzers=1, pin_memory=False, members=members)
    dirs = {n: str(tmp_path / "out" / n) for n in ("model_cv", "plain")}

    def plan():
        out = pipe.plan(set_jobs([(str(tmp_path / "rec.wav"), "rec")], members, dirs)[0])
        for j, _ in out:
            j.track.close()
        return [([members[mf.member].name for mf in j.outputs], [(round(a, 2), round(b, 2)) for a, b in chunks]) for j, chunks in out]
    every = [(0.0, 9.6), (9.6, 19.2), (19.2, 25.0)]
    assert plan() == [(["model_cv", "plain"], every)]
    starts = [round(0.96 * i, 2) for i in range(26)]
    os.makedirs(dirs["model_cv"])
    with open(os.path.join(dirs["model_cv"], "rec" + R.SUFFIX_PARTIAL), "w") as f:        # the ensemble has chunk 0 already
        f.write("start,activation_ins_buzz,activation_other\n" + "".join(f"{s:.2f},0.5,0.5\n" for s in starts[:10]))
    assert sorted(plan()) == [(["model_cv"], every[1:]), (["plain"], every)]
    os.remove(os.path.join(dirs["model_cv"], "rec" + R.SUFFIX_PARTIAL))
    with open(os.path.join(dirs["model_cv"], "rec" + R.SUFFIX_COMPLETE), "w") as f:       # ... now all of it
        f.write("start,activation_ins_buzz,activation_other\n" + "".join(f"{s:.2f},0.5,0.5\n" for s in starts))
    assert plan() == [(["plain"], every)]
