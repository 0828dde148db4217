"""buzzdetect_amd/dataset.py without a device: annotation files, window labels, the augmentation plan, save / load."""
import numpy as np
import pytest

from buzzdetect_amd import dataset as D

CLASSES = ["ambient", "ins_buzz", "mech_plane"]
W = D.WINDOW_SAMPLES


# ---------------------------------------------------------------------------------------------------- read_annotations
def write(tmp_path, text):
    p = tmp_path / "notes.csv"
    p.write_text(text)
    return str(p)


def test_read_annotations_reads_rows_in_any_column_order(tmp_path):
    notes = D.read_annotations(write(tmp_path, "label,ident,end,start\nins_buzz,site/a,15.1,12.4\n\nmech_plane,b,3,0\nins_buzz,site/a,20,19.5\n"))
    assert notes == {"site/a": [(12.4, 15.1, "ins_buzz"), (19.5, 20.0, "ins_buzz")], "b": [(0.0, 3.0, "mech_plane")]}


@pytest.mark.parametrize("text,line,what", [
    ("ident,start,stop,label\na,0,1,x\n", 1, "columns"),
    ("ident,start,end\na,0,1\n", 1, "columns"),
    ("", 1, "columns"),
    ("ident,start,end,label\na,0,1,x\na,2,2,x\n", 3, "not after"),
    ("ident,start,end,label\na,5,1,x\n", 2, "not after"),
    ("ident,start,end,label\na,zero,1,x\n", 2, "numbers"),
    ("ident,start,end,label\na,0,1\n", 2, "fields"),
    ("ident,start,end,label\na,-1,1,x\n", 2, "start >= 0"),
    ("ident,start,end,label\n,0,1,x\n", 2, "empty"),
])
def test_read_annotations_names_the_bad_line(tmp_path, text, line, what):
    with pytest.raises(ValueError, match=f"line {line}: .*{what}"):
        D.read_annotations(write(tmp_path, text))


# ---------------------------------------------------------------------------------------------------- label_windows
@pytest.mark.parametrize("hop", (0.96, 0.48))
def test_an_interval_ending_on_a_window_edge_does_not_meet_that_window(hop):
    k = 3 if hop == 0.96 else 6                                  # window k starts at 2.88 s in both hops
    edge = k * hop
    t, keep = D.label_windows(12, hop, [(edge - 0.96, 2.88, "ins_buzz")], CLASSES, background="ambient")
    starts = np.arange(12) * hop
    for w in range(12):
        overlap = min(starts[w] + 0.96, 2.88) - max(starts[w], edge - 0.96)
        if starts[w] >= 2.88 - 1e-9 or overlap <= 1e-9:            # from the edge on (and before the interval): background
            assert keep[w] and t[w].tolist() == [1, 0, 0], w
        elif overlap >= 0.48 - 1e-9:
            assert keep[w] and t[w].tolist() == [0, 1, 0], w
        else:
            assert not keep[w] and not t[w].any(), w
    assert t[k].tolist() == [1, 0, 0] and t[k - 1].tolist() == [0, 1, 0]
    # ... and one starting exactly on a window's right edge does not meet it either
    t, keep = D.label_windows(4, 0.96, [(0.96, 1.92, "ins_buzz")], CLASSES, background="ambient")
    assert keep.all() and t.tolist() == [[1, 0, 0], [0, 1, 0], [1, 0, 0], [1, 0, 0]]


@pytest.mark.parametrize("hop", (0.96, 0.48))
def test_a_short_interval_inside_one_window_sets_its_class(hop):
    t, keep = D.label_windows(6, hop, [(1.0, 1.1, "ins_buzz")], CLASSES, min_overlap=1.0, background="ambient")
    starts = np.arange(6) * hop
    inside = (starts <= 1.0) & (starts + 0.96 >= 1.1)
    assert inside.sum() == (1 if hop == 0.96 else 2)
    assert keep.all()                                             # wholly inside or not met at all: nothing is ambiguous
    assert (t[inside, 1] == 1).all() and (t[~inside, 0] == 1).all() and (t.sum(axis=1) == 1).all()
    # straddling two windows 0.02 / 0.08: measured against min_overlap x 0.1 s
    t, keep = D.label_windows(3, 0.96, [(0.94, 1.04, "ins_buzz")], CLASSES, min_overlap=0.5, background="ambient")
    assert keep.tolist() == [False, True, True] and t.tolist() == [[0, 0, 0], [0, 1, 0], [1, 0, 0]]


def test_partial_overlap_below_the_threshold_is_ambiguous_and_long_events_fill_windows():
    t, keep = D.label_windows(5, 0.96, [(0.7, 3.0, "ins_buzz")], CLASSES, background="ambient")
    # window 0: 0.26 s of 0.96 -> ambiguous; 1, 2: full; 3: 0.12 s -> ambiguous; 4: untouched
    assert keep.tolist() == [False, True, True, False, True]
    assert t.tolist() == [[0, 0, 0], [0, 1, 0], [0, 1, 0], [0, 0, 0], [1, 0, 0]]


def test_two_classes_in_one_window_and_touching_intervals_merge():
    notes = [(0.0, 0.5, "ins_buzz"), (0.5, 1.0, "ins_buzz"), (0.2, 2.0, "mech_plane")]
    t, keep = D.label_windows(3, 0.96, notes, CLASSES, background="ambient")
    assert keep.tolist() == [True, True, False]                   # window 2 meets 0.08 s of the plane only
    assert t.tolist() == [[0, 1, 1], [0, 0, 1], [0, 0, 0]]        # window 1 meets 0.04 s of the merged 1.0 s buzz: not set
    with pytest.raises(ValueError, match="no class or several"):
        D.TrainingSet(None, t[keep], np.zeros(2, np.int32), ["a"], np.zeros(2), CLASSES).labels()


def test_without_a_background_class_untouched_windows_keep_zero_rows():
    t, keep = D.label_windows(3, 0.96, [(0.0, 0.96, "ins_buzz")], ["ins_buzz", "mech_plane"])
    assert keep.all() and t.tolist() == [[1, 0], [0, 0], [0, 0]]
    with pytest.raises(ValueError, match="not one of the classes"):
        D.label_windows(3, 0.96, [(0.0, 1.0, "bird")], CLASSES)
    with pytest.raises(ValueError, match="background"):
        D.label_windows(3, 0.96, [], CLASSES, background="quiet")


# ---------------------------------------------------------------------------------------------------- the plan
def layout():
    """Two recordings in one buffer: group 0 has two chunks (30 and 12.5 windows), group 1 one chunk of 20 windows."""
    chunks = [(0, 0.0, 30 * W, 0), (0, 28.8, 12 * W + 7000, 30 * W), (1, 0.0, 20 * W, 42 * W + 7000)]
    notes = {0: [(2.0, 5.9, "ins_buzz"), (30.0, 31.5, "mech_plane")], 1: [(4.8, 18.3, "ins_buzz")]}
    return chunks, notes


def test_find_clips_cuts_whole_windows():
    chunks, notes = layout()
    events, stretches = D.find_clips(chunks, notes, CLASSES, background="ambient", max_clip_s=9.6)
    # group 0 chunk 0: windows 2..5 carry the buzz (2: 0.88 s, 6: 0.14 s ambiguous); chunk 1: 30.0-31.5 -> window 1 (0.96) and 2 (0.54)
    # group 1: 4.8-18.3 -> windows 5..18 (14 windows; 19 has 0.06 s: ambiguous) cut at 10
    got = [(e.group, e.offset, e.windows) for e in events]
    assert got == [(0, 2 * W, 4), (0, 30 * W + W, 2), (1, 42 * W + 7000 + 5 * W, 10), (1, 42 * W + 7000 + 15 * W, 4)]
    assert events[0].targets.tolist() == [[0, 1, 0]] * 4 and events[1].targets.tolist() == [[0, 0, 1]] * 2
    assert np.allclose(events[1].starts, [29.76, 30.72]) and np.allclose(events[2].starts[:2], [4.8, 5.76])
    assert [(s.group, s.offset, s.windows) for s in stretches] == [
        (0, 0, 2), (0, 7 * W, 23), (0, 30 * W, 1), (0, 30 * W + 3 * W, 9), (1, 42 * W + 7000, 5)]


def test_the_same_seed_draws_the_same_plan_inside_the_buffers_and_clear_of_the_events():
    chunks, notes = layout()
    events, stretches = D.find_clips(chunks, notes, CLASSES, background="ambient", max_clip_s=9.6)
    kw = dict(snr_db=(0, 5, 10, 20), per_event=5, gain_db=(0.0, -6.0))
    plan = D.draw_plan(events, stretches, seed=11, **kw)
    again = D.draw_plan(events, stretches, seed=11, **kw)
    other = D.draw_plan(events, stretches, seed=12, **kw)
    assert plan.dtype == D.PLAN and plan.size == 4 * 5
    assert plan.tobytes() == again.tobytes() and plan.tobytes() != other.tobytes()
    total = 42 * W + 7000 + 20 * W
    chunk_of = {g_off: (g, s, n) for g, s, n, g_off in chunks}
    for row in plan:
        ev, st = events[row["event"]], stretches[row["stretch"]]
        assert row["group"] == ev.group and row["ev_off"] == ev.offset and row["n"] == ev.windows * W
        assert 0 <= row["ev_off"] and row["ev_off"] + row["n"] <= total
        assert st.offset <= row["nz_off"] and row["nz_off"] + row["n"] <= st.offset + st.windows * W <= total
        assert row["snr_db"] in (0, 5, 10, 20) and row["gain_db"] in (0.0, -6.0) and not row["dropped"]
        # the stretch in seconds of its recording meets no annotation of that recording
        base = max(off for off in chunk_of if off <= st.offset)
        g, chunk_start, _ = chunk_of[base]
        a = chunk_start + (row["nz_off"] - base) / 16000.0
        b = a + row["n"] / 16000.0
        assert g == st.group and all(b <= s + 1e-9 or a >= e - 1e-9 for s, e, _ in notes[g]), (a, b)
    assert len(set(plan["nz_off"].tolist())) > 10 and set(plan["snr_db"].tolist()) == {0, 5, 10, 20}
    clips = D.mix_descriptors(plan["ev_off"], plan["nz_off"], plan["n"], plan["snr_db"], plan["gain_db"])
    assert clips["out_off"].tolist() == (np.cumsum(plan["n"]) - plan["n"]).tolist()
    assert np.allclose(clips["ratio"], 10.0 ** (-plan["snr_db"] / 20.0)) and clips["ratio"].dtype == np.float32


def test_a_clip_longer_than_every_stretch_is_named():
    chunks, notes = layout()
    events, stretches = D.find_clips(chunks, notes, CLASSES, background="ambient", max_clip_s=30.0)
    assert max(e.windows for e in events) == 14
    with pytest.raises(ValueError, match=r"no background stretch of 14 windows .* 4\.80 s of rec/b"):
        D.draw_plan(events, [s for s in stretches if s.windows < 14], idents=["rec/a", "rec/b"])
    with pytest.raises(ValueError, match="at least one window"):
        D.find_clips(chunks, notes, CLASSES, background="ambient", max_clip_s=0.5)


# ---------------------------------------------------------------------------------------------------- sets
def make_set(n, idents, seed, plan=None):
    rng = np.random.default_rng(seed)
    t = np.zeros((n, 3), np.float32)
    t[np.arange(n), rng.integers(0, 3, n)] = 1
    return D.TrainingSet(rng.normal(size=(n, 1024)).astype(np.float32), t, rng.integers(0, len(idents), n).astype(np.int32),
                         list(idents), np.round(rng.uniform(0, 100, n), 2), CLASSES, plan, [f"note {seed}"])


def test_save_load_round_trip_without_pickles(tmp_path):
    chunks, notes = layout()
    events, stretches = D.find_clips(chunks, notes, CLASSES, background="ambient")
    plan = D.draw_plan(events, stretches, seed=1, per_event=2)
    ts = make_set(17, ["site/a", "b"], 5, plan)
    path = str(tmp_path / "set.npz")
    D.save(path, ts)
    with np.load(path, allow_pickle=False) as z:                  # every array loads with pickles refused
        assert all(z[k].dtype != object for k in z.files)
    back = D.load(path, device="cpu")
    assert back.embeddings.numpy().tobytes() == ts.embeddings.tobytes() and tuple(back.embeddings.shape) == (17, 1024)
    assert back.targets.tobytes() == ts.targets.tobytes() and back.groups.tobytes() == ts.groups.tobytes()
    assert back.starts.tobytes() == ts.starts.tobytes() and back.idents == ts.idents and back.classes == CLASSES
    assert back.plan.tobytes() == plan.tobytes() and back.messages == ["note 5"]
    assert back.labels().tolist() == ts.targets.argmax(axis=1).tolist()
    empty = D.TrainingSet(np.zeros((0, 1024), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.int32), [], np.zeros(0),
                          CLASSES)
    D.save(path, empty)
    back = D.load(path, device="cpu")
    assert len(back) == 0 and back.idents == [] and back.plan is None and back.messages == []


def test_concat_keeps_a_recording_in_one_group():
    a, b = make_set(5, ["x", "y"], 1), make_set(7, ["y", "z"], 2)
    both = D.concat(a, b)
    assert both.idents == ["x", "y", "z"] and len(both) == 12
    assert [both.idents[g] for g in both.groups] == [a.idents[g] for g in a.groups] + [b.idents[g] for g in b.groups]
    assert both.embeddings.numpy().tobytes() == a.embeddings.tobytes() + b.embeddings.tobytes()
    assert both.messages == ["note 1", "note 2"] and both.plan is None
    with pytest.raises(ValueError, match="classes differ"):
        D.concat(a, D.TrainingSet(a.embeddings, a.targets[:, :2], a.groups, a.idents, a.starts, CLASSES[:2]))
