"""The host side of detection calling (include/buzzdetect_calls.h, buzzdetect_amd/calls.py), no device needed: the host exports
against the NumPy restatement of the definitions (tests/calls_cases.py) in every bit, hand cases with the answer written out,
the plain threshold against results.detection_table, the bins with the derived bound of the sum's order, what is refused, and
call_results over a hand-written result tree."""
import math
import os
import re

import numpy as np
import pytest

from buzzdetect_amd import _lib, calls, dataset, results
from tests import calls_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = _lib.CALLS_TILE
A = 96


def test_prototypes_are_the_header():
    with open(os.path.join(ROOT, "include", "buzzdetect_calls.h")) as f:
        header = f.read()
    names = sorted(re.findall(r"^BD_API [^;(]*?(bd_\w+)\(", header, re.M))
    assert names == sorted(_lib.CALLS_PROTOTYPES) and len(names) == 5
    for name in names:
        args = re.search(r"BD_API [^;(]*?" + name + r"\(([^;]*)\);", header).group(1)
        n_args = 0 if args.strip() == "void" else args.count(",") + 1
        assert len(_lib.CALLS_PROTOTYPES[name][1]) == n_args, name
    assert _lib.load().bd_calls_abi_version() == _lib.CALLS_ABI_VERSION == 1
    for word, value in (("BD_CALLS_TILE", _lib.CALLS_TILE), ("BD_CALLS_MAX_COLUMNS", _lib.CALLS_MAX_COLUMNS),
                        ("BD_CALLS_EVENT_FIELDS", _lib.CALLS_EVENT_FIELDS)):
        assert int(re.search(r"#define " + word + r" (\d+)", header).group(1)) == value
    assert "#define BD_CALLS_MAX_WINDOWS (1 << 20)" in header and _lib.CALLS_MAX_WINDOWS == 1 << 20
    assert calls.RULE.itemsize == 16 == __import__("ctypes").sizeof(_lib.bd_calls_rule)


# ---------------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("which", ("rows", "columns"))
@pytest.mark.parametrize("c", (1, 3))
def test_host_exports_are_the_definitions(c, which):
    seen = set()
    for w in (0, 1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        x, t, a, rules = K.draw(1000 * c + w, w, c, A)
        assert len(set(rules)) == c or c == 1
        rng = np.random.default_rng(w)
        seg = K.even_segments(rng, w, 7)
        want = K.call_numpy(x, t, a, rules, seg)
        xs = K.layout(x, which)
        marks, events = calls.events_host(xs, t, a, rules)
        counts, values = calls.bins_host(xs, marks, seg)
        assert marks.dtype == np.uint8 and np.array_equal(marks, want[0]), (w, c)
        assert K.same_events(events, want[1]), (w, c)
        assert np.array_equal(counts, want[2]), (w, c)
        assert np.array_equal(values.view(np.uint32), want[3].view(np.uint32)), (w, c)
        seen |= set(np.unique(marks).tolist()) | {("kept", int(k)) for e in events for k in e[:, 4]}
    assert seen == {0, 1, 2, 3, ("kept", 0), ("kept", 1)}                # the cases reach every mark, kept and dropped events


def test_a_column_can_hold_more_than_half_as_many_events_as_windows():
    x, t, a, _ = K.draw(5, 400, 1, A)
    t = (np.arange(400) * 10 * A).astype(np.int32)                        # every step a hole
    x[:] = np.where(np.isnan(x) | (x <= 0), np.float32(1.0), x)
    marks, events = calls.events_host(x, t, A, [(0.0, 0.0, A, 0)])
    assert len(events[0]) == 400 > 200 and (marks == 3).all()


# ---------------------------------------------------------------------------------------------------- hand cases
def run(x, rule, t=None, adjacent=A):
    x = np.asarray(x, np.float32)[:, None]
    t = np.arange(x.shape[0], dtype=np.int32) * A if t is None else np.asarray(t, np.int32)
    marks, events = calls.events_host(x, t, adjacent, [rule])
    m, e = K.events_numpy(x[:, 0], t, adjacent, rule)
    assert np.array_equal(marks[0], m) and np.array_equal(events[0], e)
    return marks[0].tolist(), events[0].tolist()


def test_all_on_and_all_off():
    assert run([2.0] * 10, (1.0, 1.0, A, 0)) == ([3] + [2] * 9, [[0, 9, 10, 0, 1]])
    assert run([0.0] * 10, (1.0, 1.0, A, 0)) == ([0] * 10, [])
    assert run([], (1.0, 1.0, A, 0)) == ([], [])


def test_alternating_scores_give_an_event_every_other_window():
    w = 9
    marks, events = run([2.0, 0.0] * 4 + [2.0], (1.0, 1.0, A, 0))
    assert marks == [3, 0] * 4 + [3]
    assert len(events) == math.ceil(w / 2) and events == [[i, i, 1, i, 1] for i in range(0, w, 2)]


def test_every_step_a_hole_makes_every_window_an_event():
    w = 7
    marks, events = run([2.0] * w, (1.0, 1.0, A, 0), t=200 * np.arange(w))
    assert marks == [3] * w and len(events) == w and events == [[i, i, 1, i, 1] for i in range(w)]
    # the same scores between the thresholds after a first ON window: a hole switches the state off
    marks, events = run([2.0] + [0.5] * 3, (1.0, 0.0, A, 0), t=[0, 96, 300, 396])
    assert marks == [3, 2, 0, 0] and events == [[0, 1, 2, 0, 1]]


def test_a_stretch_between_the_thresholds_longer_than_a_tile_keeps_the_state():
    n = TILE + 10
    marks, events = run([2.0] + [0.5] * n + [-1.0], (1.0, 0.0, A, 0))
    assert marks == [3] + [2] * n + [0] and events == [[0, n, n + 1, 0, 1]]
    marks, events = run([-1.0] + [0.5] * n + [2.0], (1.0, 0.0, A, 0))
    assert marks == [0] * (n + 1) + [3] and events == [[n + 1, n + 1, 1, n + 1, 1]]


def test_a_gap_of_exactly_link_ticks_merges_and_one_more_does_not():
    x, t = [2.0, 0.0, 2.0], [0, 96, 300]
    assert run(x, (1.0, 1.0, 300, 0), t=t) == ([3, 0, 2], [[0, 2, 2, 0, 1]])
    assert run(x, (1.0, 1.0, 299, 0), t=t) == ([3, 0, 3], [[0, 0, 1, 0, 1], [2, 2, 1, 2, 1]])


def test_an_extent_of_exactly_min_extent_is_kept_and_one_tick_less_is_dropped():
    x = [0.0, 2.0, 2.0, 2.0, 0.0, 2.0]
    assert run(x, (1.0, 1.0, A, 192)) == ([0, 3, 2, 2, 0, 1], [[1, 3, 3, 1, 1], [5, 5, 1, 5, 0]])
    assert run(x, (1.0, 1.0, A, 193)) == ([0, 1, 1, 1, 0, 1], [[1, 3, 3, 1, 0], [5, 5, 1, 5, 0]])


def test_a_peak_tie_goes_to_the_earlier_window():
    assert run([1.5, 2.0, 2.0, 1.5], (1.0, 1.0, A, 0))[1] == [[0, 3, 4, 1, 1]]
    assert run([-0.0, 0.0, -0.0], (-1.0, -1.0, A, 0))[1] == [[0, 2, 3, 0, 1]]
    assert run([1.5, np.inf, 3.0, np.inf], (1.0, 1.0, A, 0))[1] == [[0, 3, 4, 1, 1]]
    # an OFF window an event bridges does not take the peak, whatever its score (here a NaN and a low one)
    assert run([1.5, np.nan, 0.5, 1.25], (1.0, 1.0, 3 * A, 0)) == ([3, 0, 0, 2], [[0, 3, 2, 0, 1]])


def test_the_plain_threshold_is_detection_table():
    rng = np.random.default_rng(12)
    logits = rng.normal(size=(500, 3)).astype(np.float32)
    logits[::17, 1] = np.float32(-0.25)                                    # scores equal to the threshold: not detected
    classes, threshold = ["ambient", "ins_buzz", "other"], -0.25
    table = results.detection_table(logits, threshold, classes, 0.96, 2, 199.68)
    t = calls.ticks(table["start"].to_numpy())
    a = calls.adjacent_ticks(0.96)
    assert a == 96 and (np.diff(t) == 96).all()
    marks, _ = calls.events_host(logits[:, 1:2], t, a, [calls.Rule(threshold)])
    assert calls.Rule(threshold).packed(a) == (-0.25, -0.25, 96, 0)
    assert np.array_equal((marks[0] >= 2).astype(int), table[results.COLUMN_DETECTIONS].to_numpy())
    assert 0 < (marks[0] >= 2).sum() < 500 and not (marks == 1).any()


# ---------------------------------------------------------------------------------------------------- bins
SIZES = (0, 1, 63, 64, 65, 4097)


def test_bins_of_every_size_with_seg_not_covering_the_sequence():
    seg = np.concatenate([[5], 5 + np.cumsum(SIZES)]).astype(np.int32)
    w = int(seg[-1]) + 5
    x, t, a, rules = K.draw(77, w, 2, A)
    marks, _ = calls.events_host(x, t, a, rules)
    counts, values = calls.bins_host(x, marks, seg)
    want = K.call_numpy(x, t, a, rules, seg)
    assert np.array_equal(counts, want[2]) and np.array_equal(values.view(np.uint32), want[3].view(np.uint32))
    assert counts[:, 0].tolist() == [[0, 0]] * 2 and values[:, 0, 0].tolist() == [0.0] * 2 and np.isneginf(values[:, 0, 1]).all()
    assert np.isnan(values[:, -1, 0]).all() and (values[:, -1, 0].view(np.uint32) == 0x7FC00000).all()
    assert (counts[:, :, 0].sum(axis=1) == (marks[:, 5:w - 5] >= 2).sum(axis=1)).all()
    # a bin of NaNs alone has no maximum; -0.0 alone counts as +0.0
    odd = np.array([[np.nan], [np.nan], [-0.0], [-1.0]], np.float32)
    _, v = calls.bins_host(odd, np.zeros((1, 4), np.uint8), [0, 2, 3, 4])
    assert np.isneginf(v[0, 0, 1]) and v[0, 1, 1].tobytes() == np.float32(0.0).tobytes() and v[0, 2, 1] == -1.0


def test_the_sum_is_within_the_bound_of_its_order():
    """Lane l adds ceil(n / 64) terms at most, the butterfly six more: every partial sum is rounded once, so the result lies
    within (ceil(n / 64) + 6) * 2^-24 * sum |x| of the exact sum, to first order (the factor 1.01 covers the higher orders)."""
    rng = np.random.default_rng(8)
    seg = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    w = int(seg[-1])
    x = (rng.normal(size=(w, 3)) * rng.choice([1e-3, 1.0, 1e4], size=(w, 3))).astype(np.float32)
    x[:, 2] = np.abs(x[:, 2])
    _, values = calls.bins_host(x, np.zeros((3, w), np.uint8), seg)
    worst = 0.0
    for c in range(3):
        for b, n in enumerate(SIZES):
            part = x[seg[b]:seg[b + 1], c].astype(np.float64)
            bound = 1.01 * (math.ceil(n / 64) + 6) * 2.0 ** -24 * np.abs(part).sum()
            err = abs(float(values[c, b, 0]) - part.sum())
            if n:
                worst = max(worst, err / bound)
            assert err <= bound, (c, n, err, bound)
            assert values[c, b, 1] == (part.max() if n else -np.inf)
    print("largest observed error of a bin sum, as a fraction of its bound:", worst)
    assert 0 < worst <= 1


# ---------------------------------------------------------------------------------------------------- refusals
def refused(fn, *args):
    rc = fn(*args)
    assert rc < 0
    return rc, _lib.load().bd_last_error().decode()


@pytest.mark.parametrize("device_entry", (False, True))
def test_bad_arguments_are_refused_by_name_and_nothing_is_written(device_entry):
    """Also for the device entry points: these checks come before anything touches the device (the pointers here are host
    arrays); bd_calls_events reads the rules back only after them."""
    lib = _lib.load()
    x = np.ones((8, 3), np.float32)
    t = (np.arange(8) * A).astype(np.int32)
    rules = calls.pack_rules([(1.0, 0.0, A, 0)] * 3, A)
    marks, events, n = np.full((3, 8), 9, np.uint8), np.full((3, 8, 5), 9, np.int32), np.full(3, 9, np.int32)
    seg = np.array([0, 4, 8], np.int32)
    counts, values = np.full((3, 2, 2), 9, np.int32), np.full((3, 2, 2), 9, np.float32)
    tail = (None,) if device_entry else ()
    ev = lib.bd_calls_events if device_entry else lib.bd_calls_events_host
    bn = lib.bd_calls_bins if device_entry else lib.bd_calls_bins_host

    def events_call(**over):
        a = dict(x=x.ctypes.data, w=8, c=3, rs=3, cs=1, t=t.ctypes.data, adjacent=A, rules=rules.ctypes.data, marks=marks.ctypes.data,
                 events=events.ctypes.data, n=n.ctypes.data)
        a.update(over)
        return refused(ev, a["x"], a["w"], a["c"], a["rs"], a["cs"], a["t"], a["adjacent"], a["rules"], a["marks"], a["events"], a["n"],
                       *tail)

    def bins_call(**over):
        a = dict(x=x.ctypes.data, w=8, c=3, rs=3, cs=1, marks=marks.ctypes.data, seg=seg.ctypes.data, b=2, counts=counts.ctypes.data,
                 values=values.ctypes.data)
        a.update(over)
        return refused(bn, a["x"], a["w"], a["c"], a["rs"], a["cs"], a["marks"], a["seg"], a["b"], a["counts"], a["values"], *tail)

    for call in (events_call, bins_call):
        for over, word in ((dict(w=-1), "windows"), (dict(w=(1 << 20) + 1), "windows"), (dict(c=0), "columns"), (dict(c=65), "columns"),
                           (dict(rs=0), "row_stride"), (dict(cs=0), "col_stride"), (dict(x=None), "x is null"),
                           (dict(marks=None), "marks")):
            rc, text = call(**over)
            assert rc == -1 and word in text, (over, text)
    for over, word in ((dict(adjacent=0), "adjacent"), (dict(t=None), "t is null"), (dict(rules=None), "rules"),
                       (dict(events=None), "events"), (dict(n=None), "n_events")):
        rc, text = events_call(**over)
        assert rc == -1 and word in text, (over, text)
    for over, word in ((dict(b=-1), "bins"), (dict(b=(1 << 20) + 1), "bins"), (dict(seg=None), "seg"), (dict(counts=None), "counts"),
                       (dict(values=None), "values")):
        rc, text = bins_call(**over)
        assert rc == -1 and word in text, (over, text)
    if not device_entry:
        for rule, word in (((np.nan, 0.0, A, 0), "rules[1].high"), ((1.0, np.nan, A, 0), "rules[1].low"),
                           ((0.0, 1.0, A, 0), "rules[1].high is below low"), ((1.0, 0.0, A - 1, 0), "rules[1].link"),
                           ((1.0, 0.0, A, -1), "rules[1].min_extent")):
            bad = np.array([(1.0, 0.0, A, 0), rule, (1.0, 0.0, A, 0)], dtype=calls.RULE)
            rc, text = events_call(rules=bad.ctypes.data)
            assert rc == -1 and word in text, text
        for bad_seg in ([-1, 4, 8], [0, 5, 4], [0, 4, 9]):
            rc, text = bins_call(seg=np.array(bad_seg, np.int32).ctypes.data)
            assert rc == -1 and "seg[" in text, text
        # infinite thresholds are rules like any other
        assert calls.events_host(x, t, A, [(np.inf, -np.inf, A, 0)] * 3)[0].sum() == 0
    assert (marks == 9).all() and (events == 9).all() and (n == 9).all() and (counts == 9).all() and (values == 9).all()


def test_the_python_layer_refuses_what_the_library_cannot_see():
    x = np.ones((4, 1), np.float32)
    with pytest.raises(ValueError, match="strictly increasing"):
        calls.events_host(x, [0, 96, 96, 192], A, [calls.Rule(0.5)])
    with pytest.raises(ValueError, match="ticks for"):
        calls.events_host(x, [0, 96], A, [calls.Rule(0.5)])
    with pytest.raises(ValueError, match="rules for"):
        calls.events_host(x, [0, 96, 192, 288], A, [calls.Rule(0.5)] * 2)
    with pytest.raises(ValueError, match="high >= low"):
        calls.Rule(0.5, 0.75)
    with pytest.raises(ValueError, match="high >= low"):
        calls.pack_rules([(0.0, 1.0, A, 0)], A)
    with pytest.raises(ValueError, match="merge_gap_s"):
        calls.Rule(0.5, merge_gap_s=-1.0)
    with pytest.raises(ValueError, match="below a tick"):
        calls.adjacent_ticks(0.005)
    for bad in (0.0, -60.0, 0.015, 0.001):
        with pytest.raises(ValueError, match="multiple of 0.01"):
            calls.bin_ticks(bad)
    assert calls.bin_ticks(60.0) == 6000 and calls.bin_ticks(0.07) == 7 and calls.bin_ticks(3600) == 360000
    assert calls.adjacent_ticks(0.96) == 96 and calls.adjacent_ticks(0.48) == 48 and calls.adjacent_ticks(0.96 * 0.35) == 34
    assert calls.Rule(1.0, 0.5, merge_gap_s=2.0, min_duration_s=1.5).packed(48) == (1.0, 0.5, 248, 54)
    assert calls.Rule(1.0, min_duration_s=0.5).packed(96) == (1.0, 1.0, 96, 0)


# ---------------------------------------------------------------------------------------------------- result trees
def write_tree(root, framehop_prop, files):
    manifest = results.build_manifest("model_general_v3", framehop_prop, None, ["ambient", "ins_buzz"])
    ok, _ = results.check_or_write_manifest(str(root), manifest)
    assert ok
    for ident, text in files.items():
        path = os.path.join(str(root), ident + results.SUFFIX_COMPLETE)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)


def read(root, ident, suffix):
    with open(os.path.join(str(root), ident + suffix)) as f:
        return f.read()


def test_call_results_on_a_tree_at_framehop_1(tmp_path):
    write_tree(tmp_path / "tree", 1.0, {
        "a": "start,activation_ambient,activation_ins_buzz\n0.0,0.0,0.6\n0.96,0.0,0.4\n1.92,0.0,0.3\n2.88,0.0,0.7\n",
        "site/b": "start,activation_ambient,activation_ins_buzz\n0.0,0.0,0.1\n0.96,0.0,0.1\n"})
    got = calls.call_results(str(tmp_path / "tree"), {"ins_buzz": calls.Rule(0.5, 0.35)})
    assert got.classes == ["ins_buzz"] and got.messages == [] and list(got.bins) == ["a", "site/b"]
    assert got.events == [[("a", 0.0, 1.92, 2, 2, pytest.approx(0.6), 0.0), ("a", 2.88, 3.84, 1, 1, pytest.approx(0.7), 2.88)]]
    a = got.bins["a"]
    assert a.bin_start.tolist() == [0.0] and a.windows.tolist() == [4] and a.counts.tolist() == [[[3, 2]]]
    assert a.values[0, 0].tolist() == [pytest.approx(2.0), np.float32(0.7)]
    assert got.bins["site/b"].counts.tolist() == [[[0, 0]]]
    out = tmp_path / "called"
    got.to_csv(str(out))
    assert read(out, "a", calls.SUFFIX_EVENTS) == ("class,start,end,windows,detected,peak,peak_start\n"
                                                   "ins_buzz,0.0,1.92,2,2,0.6,0.0\nins_buzz,2.88,3.84,1,1,0.7,2.88\n")
    assert read(out, "a", calls.SUFFIX_BINS) == ("bin_start,windows,detected_ins_buzz,events_ins_buzz,mean_ins_buzz,max_ins_buzz\n"
                                                 "0.0,4,3,2,0.5,0.7\n")
    assert read(out, "site/b", calls.SUFFIX_EVENTS) == "class,start,end,windows,detected,peak,peak_start\n"
    assert read(out, "site/b", calls.SUFFIX_BINS).splitlines()[1] == "0.0,2,0,0,0.1,0.1"
    with pytest.raises(ValueError, match="activation_nobody"):
        calls.call_results(str(tmp_path / "tree"), {"nobody": calls.Rule(0.5)})


def test_call_results_at_framehop_half_with_the_doubled_step_at_a_chunk_edge(tmp_path):
    """Starts 198.72 -> 199.68: the last window of the 199.68 s chunk and the first of the next lie two hops apart, a hole."""
    write_tree(tmp_path / "tree", 0.5, {
        "a": "start,activation_ambient,activation_ins_buzz\n0.0,0.0,0.1\n0.48,0.0,0.2\n0.96,0.0,0.3\n",
        "site/b": "start,activation_ambient,activation_ins_buzz\n197.76,0.1,0.9\n198.24,0.7,0.9\n198.72,0.6,0.9\n199.68,0.8,0.9\n"
                  "200.16,0.2,0.2\n200.64,0.65,0.9\n"})
    rules = {"ins_buzz": calls.Rule(0.5), "ambient": calls.Rule(0.5, merge_gap_s=0.5, min_duration_s=1.5)}
    got = calls.call_results(str(tmp_path / "tree"), rules, bin_s=100.0)
    assert got.classes == ["ins_buzz", "ambient"]
    buzz, ambient = got.events
    assert [e[:5] + e[6:] for e in buzz] == [("site/b", 197.76, 199.68, 3, 3, 197.76), ("site/b", 199.68, 200.64, 1, 1, 199.68),
                                             ("site/b", 200.64, 201.6, 1, 1, 200.64)]
    assert [e[:5] + e[6:] for e in ambient] == [("site/b", 198.24, 201.6, 5, 4, 199.68)]
    assert ambient[0][5] == np.float32(0.8) and all(e[5] == np.float32(0.9) for e in buzz)
    b = got.bins["site/b"]
    assert b.bin_start.tolist() == [100.0, 200.0] and b.windows.tolist() == [4, 2]
    assert b.counts.tolist() == [[[4, 2], [1, 1]], [[3, 1], [1, 0]]]
    out = tmp_path / "called"
    got.to_csv(str(out))
    assert read(out, "site/b", calls.SUFFIX_BINS) == (
        "bin_start,windows,detected_ins_buzz,events_ins_buzz,mean_ins_buzz,max_ins_buzz,detected_ambient,events_ambient,mean_ambient,"
        "max_ambient\n100.0,4,4,2,0.9,0.9,3,1,0.55,0.8\n200.0,2,1,1,0.55,0.9,1,0,0.425,0.65\n")
    assert read(out, "site/b", calls.SUFFIX_EVENTS).splitlines()[1:] == [
        "ins_buzz,197.76,199.68,3,3,0.9,197.76", "ins_buzz,199.68,200.64,1,1,0.9,199.68", "ins_buzz,200.64,201.6,1,1,0.9,200.64",
        "ambient,198.24,201.6,5,4,0.8,199.68"]
    assert read(out, "a", calls.SUFFIX_BINS).splitlines()[1] == "0.0,3,0,0,0.2,0.3,0,0,0.0,0.0"
    # events -> annotation rows -> dataset.read_annotations
    path = str(tmp_path / "pseudo.csv")
    rows = got.annotations({"ambient": "background"}, path=path)
    assert rows == [("site/b", 197.76, 199.68, "ins_buzz"), ("site/b", 199.68, 200.64, "ins_buzz"),
                    ("site/b", 200.64, 201.6, "ins_buzz"), ("site/b", 198.24, 201.6, "background")]
    back = dataset.read_annotations(path)
    assert sorted((i, a, b, l) for i, v in back.items() for a, b, l in v) == sorted(rows)
    assert got.annotations()[3][3] == "ambient"
    with pytest.raises(ValueError, match="nobody"):
        got.annotations({"nobody": "x"})
