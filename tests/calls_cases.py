"""Inputs and NumPy restatements shared by tests/test_calls_host.py and tests/test_calls_gpu.py (a plain module, like
cluster_cases.py): the definitions of include/buzzdetect_calls.h written out as the sequential loop over one column and as the
lane chains of one bin in float32 NumPy, and the generator of small-value-set cases in which ties, in-between scores, holes and
special values dominate."""
import numpy as np

VALUES = np.array([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0], np.float32)
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0], np.float32)
QUIET_NAN = np.uint32(0x7FC00000)


# ---------------------------------------------------------------------------------------------------- the definitions
def events_numpy(x, t, adjacent, rule):
    """One column: (marks uint8 [W], events int32 [n, 5]: first, last, n_on, peak, kept) by the sequential definition."""
    high, low, link, min_extent = rule
    high, low = np.float32(high), np.float32(low)
    t = [int(v) for v in t]
    w_all = len(t)
    marks = np.zeros(w_all, np.uint8)
    events = []
    on, cur = False, None
    for w in range(w_all):
        if w > 0 and t[w] - t[w - 1] > adjacent:
            on = False
        v = x[w]
        if v > high:
            on = True
        elif not (v > low):
            on = False
        marks[w] = 1 if on else 0
        if on:
            if cur is not None and t[w] - t[cur[1]] <= link:
                cur[1] = w
                cur[2] += 1
                if v > x[cur[3]]:
                    cur[3] = w
            else:
                if cur is not None:
                    events.append(cur)
                cur = [w, w, 1, w]
    if cur is not None:
        events.append(cur)
    rows = np.zeros((len(events), 5), np.int32)
    for i, (first, last, n_on, peak) in enumerate(events):
        kept = t[last] - t[first] >= min_extent
        rows[i] = (first, last, n_on, peak, int(kept))
        if kept:
            span = marks[first:last + 1]
            span[span == 1] = 2
            marks[first] = 3
    return marks, rows


def bins_numpy(x, marks, seg):
    """One column: (counts int32 [B, 2], values float32 [B, 2]) with the sum's lanes and butterfly spelled out."""
    seg = [int(s) for s in seg]
    b_all = len(seg) - 1
    counts, values = np.zeros((b_all, 2), np.int32), np.zeros((b_all, 2), np.float32)
    lanes = np.arange(64)
    for b in range(b_all):
        lo, hi = seg[b], seg[b + 1]
        part, m = x[lo:hi], marks[lo:hi]
        counts[b] = ((m >= 2).sum(), (m == 3).sum())
        v = np.zeros(64, np.float32)
        with np.errstate(invalid="ignore"):
            for at in range(0, hi - lo, 64):
                chunk = part[at:at + 64]
                v[:chunk.shape[0]] = v[:chunk.shape[0]] + chunk
            for step in (32, 16, 8, 4, 2, 1):
                v = v + v[lanes ^ step]
        assert v.dtype == np.float32
        values[b, 0] = v[0]
        real = part[~np.isnan(part)]
        values[b, 1] = (real.max() + np.float32(0.0)) if real.size else -np.inf           # (-0.0 + 0.0 is +0.0)
    bits = values[:, 0].view(np.uint32)
    bits[np.isnan(values[:, 0])] = QUIET_NAN
    return counts, values


def call_numpy(x, t, adjacent, rules, seg=None):
    """All columns: (marks [C, W], events per column, counts [C, B, 2], values [C, B, 2])."""
    marks, events, counts, values = [], [], [], []
    for c, rule in enumerate(rules):
        m, e = events_numpy(x[:, c], t, adjacent, rule)
        marks.append(m)
        events.append(e)
        if seg is not None:
            k, v = bins_numpy(x[:, c], m, seg)
            counts.append(k)
            values.append(v)
    w = x.shape[0]
    return (np.stack(marks) if marks else np.zeros((0, w), np.uint8), events,
            np.stack(counts) if counts else None, np.stack(values) if values else None)


# ---------------------------------------------------------------------------------------------------- the generator
def draw_rule(rng, a):
    low = float(rng.choice([-1.0, 0.0, 0.5]))
    high = low + float(rng.choice([0.0, 0.5, 1.5]))
    link = a + int(rng.choice([0, a, 2 * a + 8, 10 * a]))
    return (high, low, link, int(rng.choice([0, a, a + 1, 5 * a])))


def draw(seed, w, c, a=96):
    """(x float32 [w, c] C-contiguous, t int32 [w], adjacent, rules [c]): scores from VALUES with about one special in sixteen,
    steps from {a, a, a, 2a, 10a}, a different rule per column."""
    rng = np.random.default_rng(seed)
    x = rng.choice(VALUES, size=(w, c))
    special = rng.random(size=(w, c)) < 1 / 16
    x[special] = rng.choice(SPECIALS, size=int(special.sum()))
    steps = rng.choice(np.array([a, a, a, 2 * a, 10 * a]), size=w)
    t = (int(rng.integers(0, 1000)) + np.cumsum(steps) - steps[:1].sum()).astype(np.int32) if w else np.zeros(0, np.int32)
    return np.ascontiguousarray(x, np.float32), t, a, [draw_rule(rng, a) for _ in range(c)]


def layout(x, which):
    """The same matrix window-major ("rows": [W][C]) or column-major ("columns": a column's windows are consecutive)."""
    return np.ascontiguousarray(x) if which == "rows" else np.ascontiguousarray(x.T).T


def even_segments(rng, w, bins):
    """B + 1 non-decreasing offsets inside 0..w that need not cover the sequence; some bins are empty."""
    return np.sort(rng.integers(0, w + 1, size=bins + 1)).astype(np.int32)


def same_events(got, want):
    return len(got) == len(want) and all(g.shape == e.shape and np.array_equal(g, e) for g, e in zip(got, want))
