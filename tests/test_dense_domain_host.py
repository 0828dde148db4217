"""The case tables of tests/dense_cases.py without a device: every entry touches the limit it is there for (asserted from the
tables themselves, so that an edit cannot quietly move a case off its edge), the library's host-side checks accept each set, the
float64 reference alone meets the precondition of the 1e-4 gate on the oracle's embeddings, the float32 chain restatement is
what it says, and bd_ensemble_combine_host holds to NumPy at the widths and member counts of the ensemble cases."""
import numpy as np
import pytest

from buzzdetect_amd import train as T, weights as W
from tests import dense_cases as K
from tests import train_oracle
from tests.test_ensemble_host import combine_host, float32_bound, mean_loop, same_bytes, special

ACTIVATIONS = ("linear", "relu", "sigmoid", "tanh", "softmax")


# ---------------------------------------------------------------------------------------------------- the tables
def test_the_limits_are_the_headers():
    import os
    import re
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    head, headset = open(os.path.join(inc, "buzzdetect_head.h")).read(), open(os.path.join(inc, "buzzdetect_headset.h")).read()
    assert int(re.search(r"#define\s+BD_HEAD_MAX_LAYERS\s+(\d+)", head).group(1)) == K.MAX_LAYERS == 8
    assert int(re.search(r"#define\s+BD_HEAD_MAX_WIDTH\s+(\d+)", head).group(1)) == K.MAX_WIDTH == K.SET_ROW == 2048
    assert int(re.search(r"#define\s+BD_HEADSET_MAX_MEMBERS\s+(\d+)", headset).group(1)) == K.MAX_MEMBERS == 64


def test_every_stack_is_one_attach_accepts_and_names_its_edge():
    for name, c in K.STACKS.items():
        assert 1 <= len(c.widths) <= K.MAX_LAYERS and len(c.acts) == len(c.widths) == len(c.targets), name
        assert all(1 <= w <= K.MAX_WIDTH for w in c.widths), name
        assert all(a in ACTIVATIONS for a in c.acts) and "softmax" not in c.acts[:-1], name
        assert c.why.strip(), name
    seeds = [c.seed for c in K.STACKS.values()]
    assert len(set(seeds)) == len(seeds)


def test_the_stacks_cover_every_width_depth_and_activation_the_issue_names():
    stacks = K.STACKS.values()
    last = {c.widths[-1] for c in stacks}
    hidden = {w for c in stacks for w in c.widths[:-1]}          # a hidden layer's N and the next layer's K
    assert {1, 31, 32, 33, 63, 64, 65, 2047, 2048} <= last
    assert {1, 31, 32, 33, 63, 64, 65, 2047, 2048} <= hidden
    assert {1, 2, 3, 4, 5, 8, 9, 31, 32, 33, 2047, 2048} <= hidden
    assert K.STACKS["deep8_2048"].widths == [2048] * 8 and len(set(K.STACKS["deep8_2048"].acts)) >= 4
    assert K.STACKS["deep8_mixed"].widths == [2048, 1, 2047, 33, 64, 3, 65, 13]
    # a softmax behind 8 layers (the row pass reads region 1), behind 7 (region 0), and on a single layer
    assert [len(K.STACKS[n].widths) for n in (K.DEEP_SM8, K.DEEP_SM7, "sm2")] == [8, 7, 1]
    assert all(K.STACKS[n].acts[-1] == "softmax" for n in (K.DEEP_SM8, K.DEEP_SM7, "sm2"))
    assert {1, 2, 63, 64, 65, 129, 2048} <= {c.widths[-1] for c in stacks if c.acts[-1] == "softmax"}
    assert {a for c in stacks for a in c.acts[:-1]} == set(ACTIVATIONS) - {"softmax"}
    assert {c.acts[-1] for c in stacks} == set(ACTIVATIONS)
    wide_hidden = {a for c in stacks for w, a in zip(c.widths[:-1], c.acts[:-1]) if w == 2048}
    assert {"sigmoid", "tanh"} <= wide_hidden
    assert {len(K.STACKS[n].widths) for n in K.DEPTHS} == set(range(1, 9))
    # scale: about 1e3 on a last sigmoid, tanh and softmax and on a hidden layer; about 1e-6 throughout
    big = {(c.acts[i], i + 1 == len(c.widths)) for c in stacks for i, t in enumerate(c.targets) if t >= 1e3}
    assert {("sigmoid", True), ("tanh", True), ("softmax", True), ("tanh", False), ("sigmoid", False)} <= big
    assert sum(all(t <= 1e-6 for t in c.targets) for c in stacks) >= 3
    assert all(K.is_scaled(n) for n in K.SCALED) and not any(K.is_scaled(n) for n in K.EDGES + K.WIDE + K.DEPTHS + K.SOFTMAX)


@pytest.mark.parametrize("name", sorted(K.SETS))
def test_a_set_touches_the_limits_it_says(name):
    s = K.SETS[name]
    assert len(s.members) == len(set(s.members)) and all(m in K.STACKS for m in s.members)
    assert 1 <= len(s.members) <= K.MAX_MEMBERS and K.set_outputs(s.members) <= K.MAX_WIDTH
    hidden = K.set_hidden(s.members)
    assert all(v <= K.SET_ROW for v in hidden.values())
    if s.outputs is not None:
        assert K.set_outputs(s.members) == s.outputs == 2048
    if s.hidden is not None:
        depth, floats = s.hidden
        assert hidden[depth] == floats == 2048
    if s.n_members is not None:
        assert len(s.members) == s.n_members == 64
    assert K.set_fused_classes(s.members) == s.fused
    assert not set(s.members) & set(K.LONE_ONLY)


def test_the_sets_cover_what_the_issue_names():
    sets = K.SETS
    assert any(s.n_members == 64 for s in sets.values())
    assert any(s.outputs == 2048 for s in sets.values())
    # one depth exactly full while another stays small
    hidden = K.set_hidden(sets["hidden_full"].members)
    assert hidden[0] == 2048 and hidden[1] == 512 and max(hidden) == 1
    assert {len(K.STACKS[m].widths) for m in sets["depths"].members if not K.is_fused(m)} == set(range(1, 9))
    assert sorted(s.fused for s in sets.values() if s.fused > 1) == [64, 65, 128, 129]
    assert {K.STACKS[m].widths[0] for s in sets.values() for m in s.members if K.is_fused(m)} == {1, 15, 16, 17, 64}
    # a fused member between two stack-route members
    for name in ("edges", "softmaxes", "depths", "scaled"):
        m = sets[name].members
        assert any(K.is_fused(m[i]) and not K.is_fused(m[i - 1]) and not K.is_fused(m[i + 1]) for i in range(1, len(m) - 1)), name
        assert not K.is_fused(m[0]) and not K.is_fused(m[-1])
    assert all(r in sets for r in K.REVERSED)
    # every stack runs somewhere: in a set, or among those that need an engine of their own
    in_sets = {m for s in sets.values() for m in s.members} | {m for e in K.ENSEMBLES for m in K.ensemble_members(e)}
    assert set(K.STACKS) == in_sets | set(K.LONE_ONLY)


def test_the_accepting_twins_of_the_refusals():
    """tests/test_headset_gpu.py::REFUSED one step back: 64 members where 65 are refused, 2048 outputs where 2049 are, a depth
    of 2048 hidden floats where 2080 are."""
    assert len(K.SETS["full64"].members) + 1 == 65
    assert K.set_outputs(K.SETS["out2048"].members) + 1 == 2049 == K.set_outputs(K.SETS["out2047_lin1"].members) + 1
    assert K.set_hidden(K.SETS["hidden_full"].members)[0] + 32 == 2080


@pytest.mark.parametrize("name", sorted(K.ENSEMBLES))
def test_an_ensemble_is_one_the_library_takes(name):
    members = K.ensemble_members(name)
    assert len(members) <= K.MAX_MEMBERS and K.set_outputs(members) <= K.MAX_WIDTH
    for unit, names, combine, link in K.ENSEMBLES[name].units:
        assert len({K.STACKS[m].widths[-1] for m in names}) == 1 and len({K.STACKS[m].acts[-1] for m in names}) == 1, unit
        if combine is None:
            assert len(names) == 1
        elif combine == "mean_probability":
            assert link in ("softmax", "sigmoid") and K.STACKS[names[0]].acts[-1] == "linear" and len(names) >= 2
        else:
            assert combine == "mean" and link is None


def test_the_ensembles_cover_what_the_issue_names():
    units = [(len(names), K.STACKS[names[0]].widths[-1], combine, link)
             for e in K.ENSEMBLES.values() for _, names, combine, link in e.units]
    assert (64, 13, "mean_probability", "softmax") in units and (64, 13, "mean", None) in units
    assert {1, 64, 65, 1024} <= {w for k, w, c, _ in units if c is not None and k >= 2}
    assert K.set_outputs(K.ensemble_members("w1024_softmax")) == 2048
    side = K.ENSEMBLES["side_by_side"].units
    assert {(c, l) for _, _, c, l in side} == {("mean", None), ("mean_probability", "softmax"), ("mean_probability", "sigmoid"),
                                              (None, None)}
    assert any(c == "mean_probability" and l == "softmax" and w > 64 for _, w, c, l in units)


def test_the_host_side_checks_accept_every_set_and_ensemble():
    """weights.check_head_set is the library's rule said in Python: the cases must pass it before any device sees them."""
    shapes = {}

    def light(name):              # a head of the case's shape without its weights (the check reads shapes and classes only)
        c = K.STACKS[name]
        if name not in shapes:
            ls, k = [], 1024
            for w, a in zip(c.widths, c.acts):
                ls.append((np.broadcast_to(np.float32(0), (k, w)), np.zeros(w, np.float32), a))
                k = w
            shapes[name] = W.HeadWeights(ls, [f"c{i}" for i in range(c.widths[-1])])
        return shapes[name]

    for name, s in K.SETS.items():
        cols = W.check_head_set({m: light(m) for m in s.members})
        assert max(c.stop for c in cols.values()) == K.set_outputs(s.members), name
    for name, e in K.ENSEMBLES.items():
        units = {}
        for unit, names, combine, link in e.units:
            units[unit] = light(names[0]) if combine is None else \
                W.EnsembleWeights({m: light(m) for m in names}, combine, link, list(light(names[0]).classes))
        cols = W.check_head_set(units)
        assert max(c.stop for c in cols.values()) == sum(K.STACKS[names[0]].widths[-1] for _, names, _, _ in e.units), name


# ---------------------------------------------------------------------------------------------------- generator and restatements
def test_layers_scales_glorot_layers_per_layer():
    from buzzdetect_amd import modeldir
    base = modeldir.glorot_layers([7, 3], ["relu", "linear"], seed=5, gain=1.0)
    got = K.layers([7, 3], ["relu", "linear"], 5, [2.0, 0.5], [1.0, 0.25])
    for (k0, b0, a0), (k, b, a), g, bg in zip(base, got, (2.0, 0.5), (1.0, 0.25)):
        assert a == a0 and k.dtype == b.dtype == np.float32
        assert np.array_equal(k, k0 * np.float32(g)) and np.array_equal(b, b0 * np.float32(bg))


def test_the_chain_restatement_on_a_stack_small_enough_to_check_by_hand():
    """1024 -> 3 -> 2 with two live inputs: every number below is worked out by hand."""
    x = np.zeros((2, 1024), np.float32)
    x[0, 0], x[0, 1023] = 1.0, 2.0
    x[1, 0], x[1, 1023] = -1.0, 0.5
    k0 = np.zeros((1024, 3), np.float32)
    k0[0], k0[1023] = (1.0, -2.0, 0.5), (0.25, 1.0, -1.0)
    b0 = np.float32([0.5, 0.0, -1.0])
    k1 = np.float32([[1.0, -1.0], [2.0, 0.5], [-4.0, 0.25]])
    b1 = np.float32([0.25, -0.25])
    stack = [(k0, b0, "relu"), (k1, b1, "linear")]
    # row 0: pre = (1 + 0.5 + 0.5, -2 + 2, 0.5 - 2 - 1) = (2, 0, -2.5) -> relu (2, 0, 0) -> (2 + 0.25, -2 - 0.25)
    # row 1: pre = (-1 + 0.125 + 0.5, 2 + 0.5, -0.5 - 0.5 - 1) = (-0.375, 2.5, -2) -> (0, 2.5, 0) -> (5.25, 1)
    by_hand = np.float64([[2.25, -2.25], [5.25, 1.0]])
    taps = []
    f64 = K.stack_f64(x, stack, taps)
    f32 = K.stack_f32_chain(x, stack)
    assert f64.dtype == np.float64 and np.array_equal(f64, by_hand)
    assert np.array_equal(taps[0], np.float64([[2.0, 0.0, -2.5], [-0.375, 2.5, -2.0]]))
    assert f32.dtype == np.float32 and np.array_equal(f32.astype(np.float64), by_hand)      # dyadic values: no rounding at all
    # and with weights that do round: equal to float32 rounding, far from exactly
    rng = np.random.default_rng(3)
    stack = K.layers([3, 2], ["tanh", "softmax"], 9, [4.0, 4.0])
    x = (np.maximum(rng.normal(size=(5, 1024)), 0) * 0.5).astype(np.float32)
    f64, f32 = K.stack_f64(x, stack), K.stack_f32_chain(x, stack)
    dev = np.abs(f32.astype(np.float64) - f64).max()
    assert 0 < dev <= 64 * 2.0 ** -24 * 1024 ** 0.5


def test_float32_restatement_stays_in_float32():
    rng = np.random.default_rng(2)
    x = (np.maximum(rng.normal(size=(9, 1024)), 0) * 0.5).astype(np.float64)          # even from float64 inputs and weights
    for acts in (["relu", "sigmoid", "tanh", "linear"], ["tanh", "softmax"]):
        stack = [(k.astype(np.float64), b.astype(np.float64), a) for k, b, a in K.layers([9, 5, 4, 3][:len(acts)], acts, 4, [4.0] * len(acts))]
        out = K.stack_f32_chain(x, stack)
        assert out.dtype == np.float32
        ref = K.stack_f64(x, stack)
        assert ref.dtype == np.float64
        # float32 arithmetic shows: the chain deviates from float64 by float32 rounding, not by nothing
        assert 0 < np.abs(out.astype(np.float64) - ref).max() < 1e-4


def test_the_chain_is_not_the_blocked_sum():
    """Why the yardstick is the chain: on a 2048-term row it deviates from float64 several times more than NumPy's @ does."""
    rng = np.random.default_rng(8)
    x = rng.uniform(0, 1, (16, 1024)).astype(np.float32)
    stack = K.layers([2048, 64], ["linear", "linear"], 3, [1.0, 1.0])
    ref = K.stack_f64(x, stack)
    chain = np.abs(K.stack_f32_chain(x, stack).astype(np.float64) - ref).max()
    h = x @ stack[0][0] + stack[0][1]
    blocked = np.abs((h @ stack[1][0] + stack[1][1]).astype(np.float64) - ref).max()
    print(f"chain {chain:.3g}, blocked {blocked:.3g}")
    assert chain > blocked


# ---------------------------------------------------------------------------------------------------- the precondition, on the CPU
def pre_activation_maxima(name, emb):
    """[layer][prefix] of max |pre-activation| over the first 1, 33 and 65 rows of the float64 stack."""
    taps = []
    K.stack_f64(emb, K.stack_layers(name), taps)
    return [[float(np.abs(t[:w]).max()) for w in K.WINDOW_COUNTS] for t in taps]


@pytest.mark.parametrize("name", sorted(n for n in K.STACKS if not K.is_scaled(n)))
def test_the_reference_alone_meets_the_precondition(name):
    """On the oracle's embeddings every layer's largest |pre-activation| lies in 1.5..50 for 1, 33 and 65 windows: inside the
    gate's 1..100 with room for the engine's own embeddings.  And float32 itself leaves the gate room: the chain restatement
    deviates from float64 by at most a quarter of it (a case whose weights carry a float32 chain past the gate would measure
    the case, not the kernel)."""
    maxima = pre_activation_maxima(name, K.oracle_embeddings())
    print(name, [[round(v, 2) for v in layer] for layer in maxima])
    assert all(1.5 <= v <= 50.0 for layer in maxima for v in layer), maxima
    stack = K.stack_layers(name)
    dev = np.abs(K.stack_f32_chain(K.oracle_embeddings(), stack).astype(np.float64) - K.stack_f64(K.oracle_embeddings(), stack)).max()
    assert dev <= K.CHAIN_ROOM, f"{name}: the float32 chain itself deviates by {dev}"


@pytest.mark.parametrize("name", K.SCALED)
def test_a_scaled_case_reaches_its_scale(name):
    c = K.STACKS[name]
    taps = []
    ref = K.stack_f64(K.oracle_embeddings(), K.stack_layers(name), taps)
    for t, target in zip(taps, c.targets):
        assert target / 30 <= np.abs(t).max() <= target * 30, (name, np.abs(t).max(), target)
    assert np.isfinite(ref).all()
    got32 = ref.astype(np.float32)
    if max(c.targets) >= 1e3 and c.acts[-1] in ("sigmoid", "tanh") and c.targets[-1] >= 1e3:
        ends = (0.0, 1.0) if c.acts[-1] == "sigmoid" else (-1.0, 1.0)
        assert all((got32 == e).mean() > 0.2 for e in ends), "both saturated ends are reached, exactly, in many places"
    if name == "big_softmax129":
        assert ((got32 == 1.0).sum(axis=1) == 1).mean() > 0.5 and (got32 == 0.0).mean() > 0.9


# ---------------------------------------------------------------------------------------------------- the ensemble's host routine
@pytest.mark.parametrize("k, c", ((64, 13), (3, 1), (2, 64), (2, 65), (2, 129), (2, 1024)))
def test_host_mean_has_the_bits_of_a_float32_loop_at_the_new_widths(k, c):
    rng = np.random.default_rng(100 * k + c)
    z = special(rng, (33, k, c))
    rc, out, said = combine_host(z.reshape(33, k * c), [(k, "mean", None)], [c])
    assert rc == 0, said
    with np.errstate(over="ignore"):
        ref = mean_loop(z)
    assert same_bytes(out, ref) and same_bytes(T.combine_logits(z, "mean", None, dtype=np.float32), ref)


@pytest.mark.parametrize("link", ("softmax", "sigmoid"))
@pytest.mark.parametrize("k, c", ((64, 13), (3, 1), (2, 64), (2, 65), (2, 129), (2, 1024), (64, 32)))
def test_host_mean_probability_at_the_new_widths(k, c, link):
    rng = np.random.default_rng(7 * k + c)
    z = rng.uniform(-10, 10, (33, k, c)).astype(np.float32)
    bound, ref = float32_bound(z, link)
    rc, out, said = combine_host(z.reshape(33, k * c), [(k, "mean_probability", link)], [c])
    assert rc == 0, said
    err = float(np.abs(out.astype(np.float64) - ref).max())
    print(f"mean_probability/{link} K={k} C={c}: error {err:.3g}, bound {bound:.3g}")
    if c == 1 and link == "softmax":
        assert bound == 0 and np.array_equal(out, np.zeros_like(out))        # the softmax of one class is 1, its log 0
    else:
        assert bound > 0 and err <= bound


def test_host_combine_of_the_side_by_side_case_keeps_every_unit_in_its_columns():
    units = K.ENSEMBLES["side_by_side"].units
    groups = [(len(names), combine or "none", link) for _, names, combine, link in units]
    widths = [K.STACKS[names[0]].widths[-1] for _, names, _, _ in units]
    rng = np.random.default_rng(12)
    wide = rng.uniform(-10, 10, (5, sum(g[0] * w for g, w in zip(groups, widths)))).astype(np.float32)
    rc, out, said = combine_host(wide, groups, widths)
    assert rc == 0, said
    at_w = at_o = 0
    for (k, combine, link), w in zip(groups, widths):
        rc, alone, _ = combine_host(wide[:, at_w:at_w + k * w], [(k, combine, link)], [w])
        assert rc == 0 and same_bytes(np.ascontiguousarray(out[:, at_o:at_o + w]), alone), (combine, link, w)
        at_w, at_o = at_w + k * w, at_o + w
    assert at_o == out.shape[1]
    assert train_oracle.bound(out, out.astype(np.float64))[1] == 0.0       # (the margin routine the GPU tests use, unchanged)
