"""The host side of the threshold sweep (include/buzzdetect_eval.h, buzzdetect_amd/evaluate.py), no device needed: the host
export against the NumPy restatement of the definitions (tests/eval_cases.py) in every word, Curve.table() against
train.metrics_table byte for byte, a hand case with the table written out, the metrics against formulas restated here, what is
refused, and the matching of events against annotated pieces on hand cases."""
import os
import re

import numpy as np
import pytest

from buzzdetect_amd import _lib, calls, evaluate as E, results, train
from tests import eval_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prototypes_are_the_header():
    with open(os.path.join(ROOT, "include", "buzzdetect_eval.h")) as f:
        header = f.read()
    names = sorted(re.findall(r"^BD_API [^;(]*?(bd_\w+)\(", header, re.M))
    assert names == sorted(_lib.EVAL_PROTOTYPES) and len(names) == 4
    for name in names:
        args = re.search(r"BD_API [^;(]*?" + name + r"\(([^;]*)\);", header).group(1)
        n_args = 0 if args.strip() == "void" else args.count(",") + 1
        assert len(_lib.EVAL_PROTOTYPES[name][1]) == n_args, name
    lib = _lib.load()
    assert lib.bd_eval_abi_version() == _lib.EVAL_ABI_VERSION == 1
    for word, value in (("BD_EVAL_BINS", _lib.EVAL_BINS), ("BD_EVAL_PLANES", _lib.EVAL_PLANES), ("BD_EVAL_TAILS", _lib.EVAL_TAILS),
                        ("BD_EVAL_SLICE", _lib.EVAL_SLICE), ("BD_EVAL_MAX_COLUMNS", _lib.EVAL_MAX_COLUMNS),
                        ("BD_EVAL_MAX_LABELS", _lib.EVAL_MAX_LABELS)):
        assert int(re.search(r"#define " + word + r" (\d+)", header).group(1)) == value
    assert "#define BD_EVAL_K_MIN (-8192)" in header and _lib.EVAL_K_MIN == -8192 == K.K_MIN and K.BINS == _lib.EVAL_BINS
    assert "#define BD_EVAL_MAX_WINDOWS (1 << 24)" in header and _lib.EVAL_MAX_WINDOWS == 1 << 24
    assert lib.bd_eval_state_bytes(13) == 13 * (3 * 16384 + 4) * 4
    assert lib.bd_eval_state_bytes(0) == -1 and "columns = 0" in lib.bd_last_error().decode()


# ---------------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("which", ("rows", "columns"))
@pytest.mark.parametrize("c", (1, 5))
def test_host_export_is_the_definition(c, which):
    tails = np.zeros(4, np.int64)
    for w in (0, 1, 63, 64, 65, 1023, 1024, 1025):
        x, labels, label_of = K.draw(100 * c + w, w, c)
        if c > 1:
            label_of[1] = -1                                   # a column that is not evaluated
            label_of[3] = label_of[0]                          # two score columns on one label column
        want = K.sweep_numpy(x, labels, label_of)
        hist, tail = E.sweep_host(K.layout(x, which), labels, label_of, labels.shape[1])
        assert hist.dtype == np.uint32 and np.array_equal(hist, want[0]), (w, c)
        assert np.array_equal(tail, want[1]), (w, c)
        if c > 1:
            assert not hist[1].any() and not tail[1].any()
        tails += tail.sum(axis=0).astype(np.int64)
    assert (tails > 0).all()                                   # the cases reach every word of tail


def test_the_range_ends_where_the_header_says():
    x = np.array([-81.92, 81.91, -81.925, 81.915, 81.92], np.float32)[:, None]
    labels = np.ones((5, 1), np.uint8)
    hist, tail = E.sweep_host(x, labels, [0], 1)
    want = K.sweep_numpy(x, labels, [0])
    assert np.array_equal(hist, want[0]) and np.array_equal(tail, want[1])
    # float32(-81.92) lies a hair above -8192 / 100.0 and float32(81.91) a hair above 8191 / 100.0: the first and the last bin;
    # 81.915 and float32(81.92) (a hair below 8192 / 100.0: kf = 8191) both round to the row 8192, which is out of range
    assert hist[0, 2, 0] == 1 and hist[0, 1, 0] == 1 and hist[0, 2, K.BINS - 1] == 1 and hist[0, 1, K.BINS - 1] == 1
    assert hist.sum() == 4 and tail[0].tolist() == [0, 0, 1, 2]


def test_two_updates_are_one_update_of_the_concatenation():
    x, labels, label_of = K.draw(7, 1025, 4)
    whole = E.sweep_host(x, labels, label_of, labels.shape[1])
    state = E.sweep_host(x[:400], labels[:400], label_of, labels.shape[1])
    state = E.sweep_host(x[400:], labels[400:], label_of, labels.shape[1], state)
    assert np.array_equal(state[0], whole[0]) and np.array_equal(state[1], whole[1])


# ---------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("kind", K.KINDS)
def test_table_is_metrics_table_byte_for_byte(kind):
    for seed, n, share in ((0, 1, 1.0), (1, 2, 0.5), (2, 700, 0.3), (3, 700, 0.0), (4, 700, 1.0), (5, 3000, 0.02)):
        rng = np.random.default_rng(1000 * K.KINDS.index(kind) + seed)
        z = K.draw_logits(rng, n, kind, spread=40 if seed == 5 else 300)
        positives = rng.random(n) < share
        hist, tail = E.sweep_host(z[:, None], positives.astype(np.uint8)[:, None], [0], 1)
        curve = E.Curve.from_counts(hist[0], tail[0], kind)
        assert curve.table() == K.normalised(train.metrics_table(z, positives)), (kind, seed)
        assert curve.n_pos == positives.sum() and curve.n_neg == n - positives.sum()
        assert (np.diff(curve.thresholds) < 0).all()


def test_a_hand_case_with_the_table_written_out():
    # 0.006 rounds UP to the row 0.01, which it does not reach itself: that row detects the three logits above it
    z = np.array([1.0, 0.5, 0.5, 0.006, -1.0], np.float32)
    positives = np.array([1, 1, 0, 0, 0], np.uint8)
    hist, tail = E.sweep_host(z[:, None], positives[:, None], [0], 1)
    curve = E.Curve.from_counts(hist[0], tail[0])
    assert curve.thresholds.tolist() == [1.0, 0.5, 0.01, -1.0]
    assert curve.tp.tolist() == [1, 2, 2, 2] and curve.fp.tolist() == [0, 1, 1, 3] and (curve.n_pos, curve.n_neg) == (2, 3)
    assert curve.table() == ('"threshold","precision","sensitivity","fpr"\n'
                             "1,1,0.5,0\n"
                             "0.5,0.666666666666667,1,0.333333333333333\n"
                             "0.01,0.666666666666667,1,0.333333333333333\n"
                             "-1,0.4,1,1\n")
    assert curve.table() == train.metrics_table(z, positives)
    # skipped rows count for nothing; without positives the sensitivity cell is empty
    labels = np.array([2, 7, 0, 0, 0], np.uint8)
    hist, tail = E.sweep_host(z[:, None], labels[:, None], [0], 1)
    assert tail[0].tolist() == [2, 0, 0, 0]
    assert E.Curve.from_counts(hist[0], tail[0]).table() == train.metrics_table(z[2:], labels[2:]) == \
        '"threshold","precision","sensitivity","fpr"\n0.5,0,,0.333333333333333\n0.01,0,,0.333333333333333\n-1,0,,1\n'


def drawn_curve(seed, n=2000, share=0.2):
    rng = np.random.default_rng(seed)
    positives = rng.random(n) < share
    z = (rng.normal(0.0, 1.0, n) + 1.5 * positives).astype(np.float32)
    hist, tail = E.sweep_host(z[:, None], positives.astype(np.uint8)[:, None], [0], 1)
    return E.Curve.from_counts(hist[0], tail[0]), z, positives


def test_threshold_for_precision_is_results_reading_the_same_text(tmp_path):
    seen = 0
    for seed in range(4):
        curve, _, _ = drawn_curve(seed)
        path = tmp_path / f"metrics_{seed}.csv"
        path.write_text(curve.table())
        for p, tolerance in ((0.95, 0.01), (0.9, 0.01), (0.5, 0.05), (0.3, 0.2), (0.999, 0.0001), (2.0, 0.01)):
            want = results.threshold_for_precision("unused", p, tolerance, metrics_path=str(path))
            got = curve.threshold_for_precision(p, tolerance)
            assert (np.isnan(want) and np.isnan(got)) or got == want, (seed, p)
            seen += not np.isnan(want)
    assert seen >= 8


def test_metrics_against_the_formulas_restated_on_the_same_counts():
    for seed in range(4):
        curve, _, _ = drawn_curve(10 + seed, share=(0.2, 0.5, 0.01, 0.9)[seed])
        tp, fp = [int(v) for v in curve.tp], [int(v) for v in curve.fp]
        ap, area, best, r_prev, fpr_prev = 0.0, 0.0, (None, -1.0), 0.0, 0.0
        for t, a, b in zip(curve.thresholds, tp, fp):
            r, f = a / curve.n_pos, b / curve.n_neg
            if a + b:
                ap += (r - r_prev) * (a / (a + b))
            area += (f - fpr_prev) * (r + r_prev) / 2.0
            f1 = 2 * a / (2 * a + b + (curve.n_pos - a))
            if f1 > best[1]:
                best = (float(t), f1)
            r_prev, fpr_prev = r, f
        # (both sides are float64 on the same integers: the margin is for the order of the roundings, not a measurement)
        assert curve.average_precision() == pytest.approx(ap, rel=1e-12, abs=0)
        assert curve.auc() == pytest.approx(area, rel=1e-12, abs=0)
        assert curve.best_f1()[0] == best[0] and curve.best_f1()[1] == pytest.approx(best[1], rel=1e-12, abs=0)
        assert 0.5 < curve.auc() < 1.0 and 0.0 < curve.average_precision() <= 1.0
    # a tie in F1 goes to the higher threshold; no positives, no negatives: NaN
    tie = E.Curve(np.array([2.0, 1.0]), np.array([1, 1]), np.array([0, 0]), 1, 0)
    assert tie.best_f1() == (2.0, 1.0) and np.isnan(tie.auc()) and tie.average_precision() == 1.0
    none = E.Curve(np.array([1.0]), np.array([0]), np.array([1]), 0, 1)
    assert np.isnan(none.average_precision()) and np.isnan(none.auc()) and none.best_f1() == (1.0, 0.0)


def test_evaluate_logits_on_host_logits(tmp_path):
    rng = np.random.default_rng(3)
    n, classes = 600, ["ambient", "ins_buzz", "mech"]
    targets = rng.integers(0, 3, n)
    logits = rng.normal(0, 1, (n, 6)).astype(np.float32)
    keep = rng.random(n) < 0.8
    found = E.evaluate_logits(logits, targets, classes, keep=keep, names=["a", "b"])
    assert list(found.curves) == [(m, c) for m in ("a", "b") for c in classes]
    for i, model in enumerate(("a", "b")):
        for j, name in enumerate(classes):
            want = K.normalised(train.metrics_table(logits[keep, 3 * i + j], targets[keep] == j))
            assert found.curves[(model, name)].table() == want
    multi = (rng.random((n, 3)) < 0.3).astype(np.float32)
    one = E.evaluate_logits(np.asfortranarray(logits[:, :3]), multi, classes)
    assert one.curves[("model", "mech")].table() == K.normalised(train.metrics_table(logits[:, 2], multi[:, 2] == 1))
    rows = found.summary()
    assert [r["model"] for r in rows] == ["a"] * 3 + ["b"] * 3 and rows[0]["events"] is None
    assert rows[1]["n_pos"] == int((targets[keep] == 1).sum()) and rows[1]["auc"] == found.curves[("a", "ins_buzz")].auc()
    found.to_csv(str(tmp_path / "out"))
    assert (tmp_path / "out" / "metrics_a_ins_buzz.csv").read_text() == found.curves[("a", "ins_buzz")].table()
    assert len((tmp_path / "out" / "summary.csv").read_text().splitlines()) == 7
    paths = found.write_metrics(str(tmp_path / "models"))
    assert paths == [str(tmp_path / "models" / m / "tests" / "metrics.csv") for m in ("a", "b")]
    curve = found.curves[("b", "ins_buzz")]
    got = results.threshold_for_precision("b", 0.35, 0.1, metrics_path=paths[1])
    assert got == curve.threshold_for_precision(0.35, 0.1) and not np.isnan(got)
    with pytest.raises(FileExistsError, match="overwrite=True"):
        found.write_metrics(str(tmp_path / "models"))
    found.write_metrics(str(tmp_path / "models"), overwrite=True)
    with pytest.raises(ValueError, match="class_name 'bird'"):
        found.write_metrics(str(tmp_path / "models"), class_name="bird")


# ---------------------------------------------------------------------------------------------------- refusals
def test_a_column_with_rows_outside_the_table_is_refused_by_name_and_count():
    for value, word in ((np.inf, "non-finite"), (np.nan, "non-finite"), (-90.0, "below -81.92"), (82.0, "above 81.91")):
        x = np.array([0.0, value, value, 1.0], np.float32)[:, None]
        hist, tail = E.sweep_host(x, np.ones((4, 1), np.uint8), [0], 1)
        assert hist[0, 2].sum() == 2
        with pytest.raises(ValueError, match=f"column 'm/ins_buzz': 2 labelled rows with a logit {word}"):
            E.Curve.from_counts(hist[0], tail[0], "m/ins_buzz")
    with pytest.raises(ValueError, match="column 'model/b': 1 labelled rows with a logit non-finite"):
        E.evaluate_logits(np.array([[0.0, np.nan]], np.float32), np.array([0]), ["a", "b"])
    # a skipped row may hold anything
    found = E.evaluate_logits(np.array([[0.0, np.nan], [1.0, 2.0]], np.float32), np.array([0, 1]), ["a", "b"], keep=np.array([False, True]))
    assert found.curves[("model", "b")].thresholds.tolist() == [2.0]


def test_python_refusals_name_the_argument():
    x, labels = np.zeros((4, 2), np.float32), np.zeros((4, 1), np.uint8)
    for args, word in (((x.astype(np.float64), labels, [0, 0], 1), "scores must be float32"),
                       ((x, labels, [0, 1], 1), r"label_of\[1\] = 1, allowed are -1..0"),
                       ((x, labels, [0, -2], 1), r"label_of\[1\] = -2"),
                       ((x, labels, [0], 1), "label_of names 1 columns, scores has 2"),
                       ((x, labels, [0, 0], 0), "n_labels = 0"),
                       ((x, labels, [0, 0], 2), r"labels must be uint8 \[4, 2\]"),
                       ((x, labels.astype(np.int32), [0, 0], 1), r"labels must be uint8 \[4, 1\], not int32"),
                       ((x, labels, [0, 0], 1, (np.zeros((2, 3, 8), np.uint32), np.zeros((2, 4), np.uint32))), "state must be")):
        with pytest.raises(ValueError, match=word):
            E.sweep_host(*args)
    z, t = np.zeros((5, 4), np.float32), np.zeros(5, np.int64)
    for args, kw, word in (((z, t, ["a", "b", "c"]), {}, r"logits must be \[N, M \* 3\]"),
                           ((z, t, ["a", "a"]), {}, "classes"),
                           ((z, t + 2, ["a", "b"]), {}, "targets must be labels in 0..1"),
                           ((z, t.astype(np.float32), ["a", "b"]), {}, "targets must be int labels"),
                           ((z, np.full((5, 2), 0.5), ["a", "b"]), {}, "zeros and ones"),
                           ((z, t, ["a", "b"]), {"names": ["m"]}, "names must name the 2 models"),
                           ((z, t, ["a", "b"]), {"keep": np.ones(4, bool)}, r"keep must be bool \[5\]")):
        with pytest.raises(ValueError, match=word):
            E.evaluate_logits(*args, **kw)
    with pytest.raises(ValueError, match="min_event_overlap = 0"):
        E.match_events(np.zeros((0, 2)), np.zeros((0, 2)), 0)
    # evaluate_recordings: before any engine is built
    for kw, word in (({"min_overlap": 0.0}, "min_overlap"), ({"min_event_overlap": 0}, "min_event_overlap = 0"),
                     ({"rules": {"ins_buzz": (1.0, 0.0)}}, "rules must map classes to calls.Rule"),
                     ({"modelname": ["a", "a"]}, "modelname must list"), ({"framehop_prop": 0.001}, "framehop")):
        with pytest.raises(ValueError, match=word):
            E.evaluate_recordings("nowhere", {}, **kw)


def test_the_library_refuses_by_name_before_it_reads_anything():
    lib = _lib.load()
    x, labels, label_of = np.zeros((4, 2), np.float32), np.zeros((4, 1), np.uint8), np.zeros(2, np.int32)
    hist, tail = np.zeros((2, 3, K.BINS), np.uint32), np.zeros((2, 4), np.uint32)
    good = [x.ctypes.data, 4, 2, 2, 1, labels.ctypes.data, 1, label_of.ctypes.data, hist.ctypes.data, tail.ctypes.data]
    assert lib.bd_eval_accumulate_host(*good) == 0 and hist.sum() == 16
    for at, value, word in ((1, -1, "windows = -1"), (1, (1 << 24) + 1, "windows = 16777217"), (2, 0, "columns = 0"),
                            (2, 2049, "columns = 2049"), (6, 0, "n_labels = 0"), (6, 2049, "n_labels = 2049"),
                            (3, 0, "row_stride is 0"), (4, 0, "col_stride is 0"), (0, None, "x is null"),
                            (0, x.ctypes.data + 2, "x is null or misaligned"), (5, None, "labels is null"),
                            (7, None, "label_of is null"), (8, None, "hist is null"), (9, None, "tail is null"),
                            (9, tail.ctypes.data + 1, "tail is null or misaligned")):
        args = list(good)
        args[at] = value
        assert lib.bd_eval_accumulate_host(*args) == -1 and word in lib.bd_last_error().decode(), word
        # the device entry point checks the same arguments the same way, before it touches the device
        assert lib.bd_eval_accumulate(*args, None) == -1 and word in lib.bd_last_error().decode(), word
    label_of[1] = 1
    assert lib.bd_eval_accumulate_host(*good) == -1 and "label_of[1] = 1, allowed are -1..0" in lib.bd_last_error().decode()
    assert hist.sum() == 16


# ---------------------------------------------------------------------------------------------------- events against pieces
def events_of(*rows):
    return np.array(rows, np.int32).reshape(-1, 5)                        # first, last, n_on, peak, kept


def test_an_event_touching_a_piece_by_one_tick_hits_and_by_zero_ticks_misses():
    t = np.array([4, 5], np.int32)                                        # an event of window w spans [t[w], t[w] + 96)
    piece = [(1.0, 2.0)]                                                  # [100, 200)
    labels = np.array([0, 0], np.uint8)
    zero = E.score_events(events_of((0, 0, 1, 0, 1)), np.array([3, 0]), t, piece, labels)
    assert (zero.events, zero.hits, zero.pieces, zero.found) == (1, 0, 1, 0) and zero.precision == 0.0 and zero.recall == 0.0
    one = E.score_events(events_of((1, 1, 1, 1, 1)), np.array([0, 3]), t, piece, labels)
    assert (one.events, one.hits, one.pieces, one.found) == (1, 1, 1, 1)
    two = E.score_events(events_of((1, 1, 1, 1, 1)), np.array([0, 3]), t, piece, labels, min_event_overlap=2)
    assert (two.hits, two.found) == (0, 0)
    # the same from the other side: [200, 296) against [100, 200) and [100, 201)
    t = np.array([200], np.int32)
    assert E.score_events(events_of((0, 0, 1, 0, 1)), np.array([3]), t, [(1.0, 2.0)], labels[:1]).hits == 0
    assert E.score_events(events_of((0, 0, 1, 0, 1)), np.array([3]), t, [(1.0, 2.01)], labels[:1]).hits == 1


def test_one_event_over_two_pieces_and_two_events_in_one_piece():
    t = (np.arange(10) * 96).astype(np.int32)
    labels = np.array([0, 1, 1, 2, 0, 1, 0, 0, 0, 0], np.uint8)
    marks = np.array([0, 3, 2, 2, 2, 0, 0, 0, 0, 0], np.uint8)
    got = E.score_events(events_of((1, 4, 4, 2, 1)), marks, t, [(1.0, 2.0), (4.0, 4.5), (1.5, 2.5)], labels)
    # pieces [100, 250) and [400, 450); the event spans [96, 480): one hit, both pieces found
    assert (got.events, got.hits, got.pieces, got.found) == (1, 1, 2, 2) and got.precision == 1.0 and got.recall == 1.0
    assert (got.tp, got.fp, got.fn) == (2, 1, 1)                          # the skipped window 3 counts for nothing
    marks = np.array([3, 0, 0, 3, 2, 0, 0, 0, 0, 0], np.uint8)
    got = E.score_events(events_of((0, 0, 1, 0, 1), (3, 4, 2, 3, 1)), marks, t, [(0.0, 9.0)], labels)
    assert (got.events, got.hits, got.pieces, got.found) == (2, 2, 1, 1)


def test_a_dropped_event_over_a_piece_finds_nothing():
    t = (np.arange(4) * 96).astype(np.int32)
    labels = np.array([0, 1, 0, 0], np.uint8)
    got = E.score_events(events_of((1, 1, 1, 1, 0)), np.array([0, 1, 0, 0], np.uint8), t, [(1.0, 1.9)], labels)
    assert (got.events, got.hits, got.pieces, got.found) == (0, 0, 1, 0)
    assert np.isnan(got.precision) and got.recall == 0.0 and (got.tp, got.fp, got.fn) == (0, 0, 1)
    none = E.score_events(events_of(), np.zeros(4, np.uint8), t, [], labels)
    assert (none.events, none.pieces) == (0, 0) and np.isnan(none.precision) and np.isnan(none.recall)
    assert E.pieces_ticks([(0.0, 0.004), (1.0, 2.0), (2.0, 3.0)]).tolist() == [[100, 300]]
    assert calls.KEPT == 4 and E.EVENT_TICKS == 96
