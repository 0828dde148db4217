"""Detection calling on the GPU (csrc/calls.hip, buzzdetect_amd/calls.py): marks, events, counts, sums and maxima against the
host restatements in every bit on the generator's cases (tests/calls_cases.py) and on hand cases laid across wave and tile
edges, determinism, columns called together against one at a time, and memory hygiene between the guard words of
tests/gpu_guards.Guarded."""
import numpy as np
import pytest

from buzzdetect_amd import _lib, calls
from tests import calls_cases as K

pytestmark = pytest.mark.gpu

TILE = _lib.CALLS_TILE
A = 96
WINDOWS = (1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)


@pytest.fixture(scope="module")
def guarded_caller():
    import torch
    from tests.gpu_guards import Guarded
    assert torch.cuda.is_available()

    class GuardedCaller(calls.Caller):
        guards = Guarded()

        def _empty(self, shape, dtype):
            # (the rows of `events` beyond n_events stay as they were: test_memory_hygiene looks at them word by word)
            return self.guards.empty(shape, dtype, written=len(shape) != 3 or shape[2] != _lib.CALLS_EVENT_FIELDS,
                                     name=f"{tuple(shape)} {dtype}")

    return GuardedCaller


def on_device(x, which):
    import torch
    dev = torch.from_numpy(K.layout(x, which)).cuda()
    if which == "columns" and x.shape[0] > 1 and x.shape[1] > 1:
        assert dev.stride() == (1, x.shape[0])
    return dev


def same(got, marks, events, counts=None, values=None):
    assert got.marks.dtype == np.uint8 and np.array_equal(got.marks, marks)
    assert K.same_events(got.events, events)
    if counts is not None:
        assert np.array_equal(got.counts, counts)
        assert np.array_equal(got.values.view(np.uint32), values.view(np.uint32))


@pytest.mark.parametrize("which", ("rows", "columns"))
@pytest.mark.parametrize("c", (1, 2, 13, 64))
def test_device_is_host_in_every_output(guarded_caller, c, which):
    seen = set()
    for w in WINDOWS:
        x, t, a, rules = K.draw(7000 * c + w, w, c, A)
        seg = K.even_segments(np.random.default_rng(w), w, 7)
        marks, events = calls.events_host(x, t, a, rules)
        counts, values = calls.bins_host(x, marks, seg)
        caller = guarded_caller(rules)
        got = caller.call(on_device(x, which), t, a, seg)
        caller.guards.check()
        same(got, marks, events, counts, values)
        for col in range(c):
            assert np.array_equal(got.peaks[col].view(np.uint32), x[events[col][:, 3], col].view(np.uint32))
        seen |= set(np.unique(marks).tolist()) | {("kept", int(k)) for e in events for k in e[:, 4]}
    assert seen == {0, 1, 2, 3, ("kept", 0), ("kept", 1)}
    if c == 1 and which == "rows":                          # the first case once more against the definitions themselves
        x, t, a, rules = K.draw(7000 + 3 * TILE + 5, 3 * TILE + 5, 1, A)
        want = K.call_numpy(x, t, a, rules)
        assert np.array_equal(got.marks, want[0]) and K.same_events(got.events, want[1])


def hand_cases():
    """(name, x, t, rule): each laid across a tile edge and, 64 windows further, across a wave edge alone."""
    w = 3 * TILE + 70
    steady = (np.arange(w) * A).astype(np.int32)
    out = []
    for shift, where in ((0, "tile"), (64, "wave")):
        x = np.full(w, -1.0, np.float32)
        x[TILE - 3 + shift:3 * TILE + 3 + shift] = 2.0
        out.append((f"an event from one tile into the tile after the next ({where})", x, steady, (1.0, 1.0, A, 0)))
        x = np.full(w, -1.0, np.float32)
        x[TILE - 1 + shift] = 2.0
        x[TILE + shift:2 * TILE + 6 + shift] = 0.5
        out.append((f"a whole tile between the thresholds stays ON ({where})", x, steady, (1.0, 0.0, A, 0)))
        x = np.full(w, -1.0, np.float32)
        x[TILE + shift:2 * TILE + 6 + shift] = 0.5
        x[2 * TILE + 6 + shift] = 2.0
        out.append((f"a whole tile between the thresholds stays OFF ({where})", x, steady, (1.0, 0.0, A, 0)))
        x = np.full(w, -1.0, np.float32)
        x[[TILE - 2 + shift, TILE + 1 + shift]] = 2.0
        out.append((f"a gap of exactly link ticks merges ({where})", x, steady, (1.0, 1.0, 3 * A, 0)))
        out.append((f"a gap of link + 1 ticks does not ({where})", x, steady, (1.0, 1.0, 3 * A - 1, 0)))
        holed = steady.copy()
        holed[TILE + shift:] += 5
        holed[2 * TILE + shift:] += 1000
        x = np.full(w, 0.5, np.float32)
        x[[3, 2 * TILE - 5 + shift]] = 2.0
        out.append((f"a hole at a tile's first window switches the state off ({where})", x, holed, (1.0, 0.0, A + 4, 3 * A)))
        x = np.full(w, 2.0, np.float32)
        x[TILE + shift] = 3.0
        x[2 * TILE + shift] = 3.0
        out.append((f"a peak tie two tiles apart goes to the earlier window ({where})", x, steady, (1.0, 1.0, A, 0)))
    return out


def test_hand_cases_across_wave_and_tile_edges(guarded_caller):
    facts = {}
    for name, x, t, rule in hand_cases():
        marks, events = calls.events_host(x[:, None], t, A, [rule])
        seg = np.arange(0, x.shape[0] + 1, 67, dtype=np.int32)
        counts, values = calls.bins_host(x[:, None], marks, seg)
        caller = guarded_caller([rule])
        got = caller.call(on_device(x[:, None], "rows"), t, A, seg)
        caller.guards.check()
        same(got, marks, events, counts, values)
        facts[name] = got.events[0].tolist()
    for shift, where in ((0, "tile"), (64, "wave")):
        assert facts[f"an event from one tile into the tile after the next ({where})"] == \
            [[TILE - 3 + shift, 3 * TILE + 2 + shift, 2 * TILE + 6, TILE - 3 + shift, 1]]
        assert facts[f"a whole tile between the thresholds stays ON ({where})"] == \
            [[TILE - 1 + shift, 2 * TILE + 5 + shift, TILE + 7, TILE - 1 + shift, 1]]
        assert facts[f"a whole tile between the thresholds stays OFF ({where})"] == \
            [[2 * TILE + 6 + shift] * 2 + [1, 2 * TILE + 6 + shift, 1]]
        assert facts[f"a gap of exactly link ticks merges ({where})"] == [[TILE - 2 + shift, TILE + 1 + shift, 2, TILE - 2 + shift, 1]]
        assert len(facts[f"a gap of link + 1 ticks does not ({where})"]) == 2
        # (the step of A + 5 ticks at the tile's first window is a hole: the state the in-between scores kept goes off)
        assert facts[f"a hole at a tile's first window switches the state off ({where})"] == \
            [[3, TILE - 1 + shift, TILE - 3 + shift, 3, 1], [2 * TILE - 5 + shift, 2 * TILE - 1 + shift, 5, 2 * TILE - 5 + shift, 1]]
        assert facts[f"a peak tie two tiles apart goes to the earlier window ({where})"] == \
            [[0, 3 * TILE + 69, 3 * TILE + 70, TILE + shift, 1]]


def test_the_same_call_twice_gives_the_same_bytes(guarded_caller):
    x, t, a, rules = K.draw(99, 3 * TILE + 5, 13, A)
    seg = K.even_segments(np.random.default_rng(1), x.shape[0], 50)
    caller = guarded_caller(rules)
    dev = on_device(x, "columns")
    one, two = caller.call(dev, t, a, seg), caller.call(dev, t, a, seg)
    caller.guards.check()
    same(two, one.marks, one.events, one.counts, one.values)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(one.peaks, two.peaks))


def test_columns_called_together_are_the_columns_called_alone(guarded_caller):
    x, t, a, rules = K.draw(123, 2 * TILE + 77, 5, A)
    seg = K.even_segments(np.random.default_rng(2), x.shape[0], 9)
    dev = on_device(x, "rows")
    whole = guarded_caller(rules).call(dev, t, a, seg)
    for col in range(5):
        alone = guarded_caller(rules[col:col + 1]).call(dev[:, col:col + 1], t, a, seg)
        same(alone, whole.marks[col:col + 1], whole.events[col:col + 1], whole.counts[col:col + 1], whole.values[col:col + 1])
    guarded_caller.guards.check()


def test_an_empty_sequence_and_no_bins(guarded_caller):
    import torch
    caller = guarded_caller([(1.0, 0.0, A, 0)] * 3)
    got = caller.call(torch.zeros((0, 3), dtype=torch.float32, device="cuda"), np.zeros(0, np.int32), A, np.zeros(1, np.int32))
    assert got.marks.shape == (3, 0) and [e.shape for e in got.events] == [(0, 5)] * 3 and got.counts.shape == (3, 0, 2)
    got = caller.call(torch.zeros((0, 3), dtype=torch.float32, device="cuda"), np.zeros(0, np.int32), A, np.zeros(3, np.int32))
    assert got.counts.tolist() == [[[0, 0]] * 2] * 3 and got.values[:, :, 0].tolist() == [[0.0] * 2] * 3
    assert np.isneginf(got.values[:, :, 1]).all()
    x = np.ones((5, 3), np.float32)
    got = caller.call(x, (np.arange(5) * A).astype(np.int32), A)
    assert got.counts is None and got.values is None and got.marks.tolist() == [[0] * 5] * 3
    caller.guards.check()


def test_the_device_entry_refuses_bad_rules_before_any_launch():
    import torch
    from tests.gpu_guards import Guarded
    lib, guards = _lib.load(), Guarded()
    x = torch.ones((8, 2), dtype=torch.float32, device="cuda")
    t = torch.arange(8, dtype=torch.int32, device="cuda") * A
    marks = guards.empty((2, 8), torch.uint8, written=False)
    events = guards.empty((2, 8, 5), torch.int32, written=False)
    n_events = guards.empty((2,), torch.int32, written=False)
    for rule, word in (((1.0, 0.0, A - 1, 0), "rules[1].link"), ((0.0, 1.0, A, 0), "rules[1].high is below low"),
                       ((np.nan, 0.0, A, 0), "rules[1].high"), ((1.0, 0.0, A, -1), "rules[1].min_extent")):
        bad = np.array([(1.0, 0.0, A, 0), rule], dtype=calls.RULE)
        rules = torch.from_numpy(bad.view(np.int32).reshape(-1, 4).copy()).cuda()
        rc = lib.bd_calls_events(x.data_ptr(), 8, 2, 2, 1, t.data_ptr(), A, rules.data_ptr(), marks.data_ptr(), events.data_ptr(),
                                 n_events.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == -1 and word in lib.bd_last_error().decode()
    for view in (marks, events, n_events):
        assert (view.cpu().numpy().view(np.uint8).reshape(-1, 4) == np.array([0x45, 0x23, 0xC1, 0x7F], np.uint8)).all()
    guards.check(written=False)


def test_memory_hygiene():
    """Outputs between guard words: marks, n_events, counts and values fully written, events exactly up to n_events[c] rows and
    not one word beyond, no guard word changed."""
    import torch
    from tests.gpu_guards import SENTINEL, Guarded, _signed
    w, c, b = TILE + 1, 3, 5
    x, t, a, rules = K.draw(31, w, c, A)
    seg = np.array([0, 10, 10, TILE - 1, TILE + 1, TILE + 1], np.int32)
    lib, guards = _lib.load(), Guarded()
    x_dev, t_dev, seg_dev = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(seg).cuda()
    rules_dev = torch.from_numpy(calls.pack_rules(rules, a).view(np.int32).reshape(-1, 4).copy()).cuda()
    marks = guards.empty((c, w), torch.uint8, name="marks")
    events = guards.empty((c, w, 5), torch.int32, name="events", written=False)
    n_events = guards.empty((c,), torch.int32, name="n_events")
    counts = guards.empty((c, b, 2), torch.int32, name="counts")
    values = guards.empty((c, b, 2), torch.float32, name="values")
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.bd_calls_events(x_dev.data_ptr(), w, c, c, 1, t_dev.data_ptr(), a, rules_dev.data_ptr(), marks.data_ptr(),
                                   events.data_ptr(), n_events.data_ptr(), stream))
    _lib.check(lib.bd_calls_bins(x_dev.data_ptr(), w, c, c, 1, marks.data_ptr(), seg_dev.data_ptr(), b, counts.data_ptr(),
                                 values.data_ptr(), stream))
    torch.cuda.synchronize()
    n, rows = n_events.cpu().numpy(), events.cpu().numpy()
    host_marks, host_events = calls.events_host(x, t, a, rules)
    assert np.array_equal(marks.cpu().numpy(), host_marks) and (marks.cpu().numpy() <= 3).all()
    assert n.tolist() == [len(e) for e in host_events] and 0 < n.min() and n.max() < w
    for col in range(c):
        assert np.array_equal(rows[col, :n[col]], host_events[col])
        assert (rows[col, :n[col]] != _signed(SENTINEL)).all(), "a word of an event's row was not written"
        assert (rows[col, n[col]:] == _signed(SENTINEL)).all(), "a word beyond the last event's row was written"
    host_counts, host_values = calls.bins_host(x, host_marks, seg)
    assert np.array_equal(counts.cpu().numpy(), host_counts)
    assert np.array_equal(values.cpu().numpy().view(np.uint32), host_values.view(np.uint32))
    guards.check(written=True)
