"""Inputs and NumPy restatements shared by the neighbour-list and propagation tests (a plain module, like cluster_cases.py):
the contracts of include/buzzdetect_knn.h and include/buzzdetect_propagate.h spelled out in float32 NumPy, independent of the
library - a fused multiply-add made from float64 by rounding to odd, the chain of a dot in its documented order, the key format,
the weights, a step and the read-out as plain loops."""
import functools

import numpy as np

DIM = 1024
F = np.float32
NORM_FLOOR = np.float32(1e-30)
SLICE = 256


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, correctly rounded: the product of two float32 is exact in float64; the sum is rounded to
    odd in float64 (its error is known exactly), and 53 bits rounded to odd round to 24 bits as the exact sum would."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        t = s - p
        err = (p - (s - t)) + (c - t)
        even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
        nudge = np.isfinite(s) & np.isfinite(err) & (err != 0) & even
        s = np.where(nudge, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def chain_order():
    """The channel of every step of a dot's chain: groups of eight ascending, inside a group 0, 4, 1, 5, 2, 6, 3, 7."""
    return np.array([8 * g + c for g in range(DIM // 8) for c in (0, 4, 1, 5, 2, 6, 3, 7)])


def dots(q, c):
    """dot(i, j) float32 [Wq, Wc] by the documented chain, from 0."""
    q, c = np.asarray(q, np.float32), np.asarray(c, np.float32)
    acc = np.zeros((q.shape[0], c.shape[0]), np.float32)
    for ch in chain_order():
        acc = fma32(q[:, ch][:, None], c[:, ch][None, :], acc)
    return acc


def norms(e):
    """bd_search_norms: lane l adds e[l + 64 j]^2, j ascending, by fused multiply-adds from 0; the butterfly m = 32 .. 1."""
    e = np.asarray(e, np.float32)
    v = np.zeros((e.shape[0], 64), np.float32)
    for j in range(DIM // 64):
        x = e[:, 64 * j:64 * j + 64]
        v = fma32(x, x, v)
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ m]
    assert v.dtype == np.float32
    return v[:, 0].copy()


def sims(q, c, metric):
    """sim(i, j) float32 [Wq, Wc]: the dot, or the dot over one rounded product of the two roots; 0 below the norm floor."""
    d = dots(q, c)
    if metric == "dot":
        return d
    n2q, n2c = norms(q), norms(c)
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.sqrt(n2q)[:, None] * np.sqrt(n2c)[None, :]
        assert den.dtype == np.float32
        s = d / den
    assert s.dtype == np.float32
    s[n2q < NORM_FLOOR, :] = 0.0
    s[:, n2c < NORM_FLOOR] = 0.0
    return s


def canonical(s):
    s = np.array(s, np.float32)
    s[np.isnan(s)] = -np.inf
    s[s == 0] = 0.0
    return s


def make_keys(s, ids):
    """The key of (score, id): the monotone map of the score's bits above 0xFFFFFFFF - id."""
    b = bits(canonical(s)).astype(np.uint64)
    m = np.where(b & np.uint64(0x80000000), ~b & np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))
    return (m << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(ids, np.uint64))


def knn_numpy(q, c, k, metric="cosine", exclude_self=False, q_base=0, c_base=0, s=None):
    """keys uint64 [Wq, k]: per row a stable sort of the candidates on (-sim, id), the k first, zeros behind them."""
    s = canonical(sims(q, c, metric) if s is None else s)
    ids = c_base + np.arange(c.shape[0], dtype=np.int64)
    keys = np.zeros((q.shape[0], k), np.uint64)
    for i in range(q.shape[0]):
        keep = ids != q_base + i if exclude_self else np.ones(ids.shape[0], bool)
        order = np.lexsort((ids[keep], -s[i][keep].astype(np.float64)))[:k]
        keys[i, :order.shape[0]] = make_keys(s[i][keep][order], ids[keep][order])
    return keys


def special_rows(w, seed=3):
    """[w, 1024] rows with what the lists must order: duplicates (rows 1 and w - 1 equal row 0 where they exist), a zero row, a
    NaN row, a row of tiny norm."""
    rng = np.random.default_rng(seed)
    e = (np.abs(rng.normal(size=(4, DIM)))[rng.integers(0, 4, size=w)] + 0.5 * rng.normal(size=(w, DIM))).astype(np.float32)
    if w > 1:
        e[1] = e[0]
    if w > 8:
        e[w - 1] = e[0]
        e[3] = 0.0
        e[5, 100] = np.nan
        e[7] = 1e-20
    return e


# ---------------------------------------------------------------------------------------------------- propagation
def weights_numpy(ids, sims_, power):
    ids, s = np.asarray(ids, np.int32), np.asarray(sims_, np.float32)
    x = np.where(s > 0, s, np.float32(0.0)).astype(np.float32)
    w = x.copy()
    for _ in range(power - 1):
        w = w * x
    assert w.dtype == np.float32
    rows = np.broadcast_to(np.arange(ids.shape[0], dtype=np.int32)[:, None], ids.shape)
    return np.where(ids < 0, rows, ids).astype(np.int32), np.where(ids < 0, np.float32(0.0), w).astype(np.float32)


def step_numpy(row_start, nbr, w, f_in, y, alpha):
    n, c = f_in.shape
    out = np.zeros((n, c), np.float32)
    one = np.float32(1.0)
    for i in range(n):
        acc, den = np.zeros(c, np.float32), np.float32(0.0)
        for e in range(row_start[i], row_start[i + 1]):
            acc = fma32(np.full(c, w[e], np.float32), f_in[nbr[e]], acc)
            den = np.float32(den + w[e])
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = (acc / den).astype(np.float32) if den > 0 else np.zeros(c, np.float32)
        out[i] = fma32(np.full(c, alpha[i], np.float32), mean, (one - alpha[i]) * y[i])
    moved = np.abs(out - f_in)
    moved[np.isnan(moved)] = np.inf
    delta = np.array([moved[a:a + SLICE].max() for a in range(0, n, SLICE)], np.float32)
    return out, delta


def readout_numpy(f):
    n, c = f.shape
    lanes = np.arange(64)
    reach, label = np.zeros(n, np.float32), np.zeros(n, np.int32)
    confidence, margin = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for i in range(n):
        v = np.zeros(64, np.float32)
        v[:c] = f[i]
        with np.errstate(invalid="ignore", over="ignore"):
            for m in (32, 16, 8, 4, 2, 1):
                v = v + v[lanes ^ m]
        reach[i] = v[0]
        o = np.where(np.isnan(f[i]), -np.inf, f[i]).astype(np.float32)
        top = int(np.argmax(o))                       # the first of equal values: the lowest class
        second = np.float32(0.0) if c == 1 else np.delete(o, top).max()
        if v[0] == 0 or not np.isfinite(v[0]):
            label[i] = -1
            continue
        label[i] = top
        with np.errstate(invalid="ignore", over="ignore"):
            confidence[i] = o[top] / v[0]
            margin[i] = np.float32(o[top] - second) / v[0]
    return reach, label, confidence, margin


def graph_case(classes, seed=11, n=310):
    """A CSR graph of n rows (two slices) with a row of degree 0 (row 0), one of degree 1 (row 1), a hub of degree 300 (row 2);
    alpha among 0, 0.25 and 1; F_in with an all-zero row (row 4) and a tie between classes (row 5); targets one-hot on the rows
    that are clamped.  Returns (row_start, nbr, w, f_in, y, alpha)."""
    rng = np.random.default_rng(seed)
    degree = rng.integers(2, 9, size=n)
    degree[0], degree[1], degree[2] = 0, 1, 300
    row_start = np.zeros(n + 1, np.int64)
    np.cumsum(degree, out=row_start[1:])
    nbr = rng.integers(0, n, size=int(row_start[-1])).astype(np.int32)
    w = (rng.random(nbr.shape[0]) ** 4).astype(np.float32)
    w[rng.random(nbr.shape[0]) < 0.05] = 0.0
    f_in = rng.random((n, classes)).astype(np.float32)
    f_in[4] = 0.0
    f_in[5] = 0.25
    alpha = rng.choice(np.array([0.0, 0.25, 1.0], np.float32), size=n)
    y = np.zeros((n, classes), np.float32)
    y[np.arange(n), rng.integers(0, classes, size=n)] = 1.0
    y[alpha == 1.0] = 0.0
    return row_start, nbr, w, f_in, y, alpha


@functools.lru_cache(maxsize=None)
def planted_lists(w, clusters, k):
    """The lists of cluster_cases.fixture(w, clusters) by the host restatement (held to NumPy by tests/test_knn_host.py):
    (rows, truth, ids int32 [w, k], sims float32 [w, k]).  Computed once; do not change what it returns."""
    from buzzdetect_amd import propagate
    from tests import cluster_cases
    e, truth = cluster_cases.fixture(w, clusters)
    keys = propagate.knn_update_host(np.zeros((w, k), np.uint64), e, e, metric="cosine", exclude_self=True)
    ids, s = propagate.decode_keys(keys)
    return e, truth, ids, s
