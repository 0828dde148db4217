"""Inputs and NumPy restatements shared by the t-SNE tests and tools/make_tsne_golden.py (a plain module, like
propagate_cases.py; nothing here comes from the library): the contract of include/buzzdetect_tsne.h spelled out twice.

  * attract32, repulse32, update32, slice_sum32: float32 with the stated orders, one rounding per operation, the fused
    multiply-add made from float64 by rounding to odd - what the host restatements must equal in every bit.
  * affinities, joint, kl, fit: plain vectorised NumPy in a dtype of choice (float64: the truth; float32: the yardstick of the
    8x rule and of the golden file), sums in NumPy's own order.
  * the constructed coordinates, sign cases and graphs, purity10 and preservation."""
import numpy as np

F = np.float32
SLICE = 2048
ROWS_PER_BLOCK = 256
BISECTIONS = 64


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, correctly rounded: the product of two float32 is exact in float64; the sum is rounded to
    odd in float64 (its error is known exactly), and 53 bits rounded to odd round to 24 bits (or fewer, for a subnormal) as the
    exact sum would."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        p = a * b
        s = p + c
        t = s - p
        err = (p - (s - t)) + (c - t)
        even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
        nudge = np.isfinite(s) & np.isfinite(err) & (err != 0) & even
        s = np.where(nudge, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


# ---------------------------------------------------------------------------------------------------- float32, stated orders
def q32(dx, dy):
    with np.errstate(over="ignore", under="ignore"):
        q = F(1.0) / fma32(dy, dy, fma32(dx, dx, F(1.0)))
    assert q.dtype == np.float32
    return q


def repulse32(y):
    """(rep [N, 2], z [N]): per (row, slice) one chain over j ascending from 0; j == i takes part with q = 0; the slices'
    partials in ascending order from 0.  All rows at once, a Python loop over j."""
    y = np.asarray(y, np.float32)
    n = y.shape[0]
    x0, x1 = y[:, 0].copy(), y[:, 1].copy()
    rx, ry, rz = (np.zeros(n, np.float32) for _ in range(3))
    with np.errstate(over="ignore", under="ignore"):
        for first in range(0, n, SLICE):
            fx, fy, fz = (np.zeros(n, np.float32) for _ in range(3))
            for j in range(first, min(first + SLICE, n)):
                dx, dy = x0 - x0[j], x1 - x1[j]
                q = q32(dx, dy)
                q[j] = 0.0
                fz = fz + q
                q2 = q * q
                fx, fy = fma32(q2, dx, fx), fma32(q2, dy, fy)
            rx, ry, rz = rx + fx, ry + fy, rz + fz
    assert rx.dtype == rz.dtype == np.float32
    return np.stack([rx, ry], axis=1), rz


def butterfly32(v):
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ m]
    assert v.dtype == np.float32
    return v[0]


def attract32(row_start, nbr, P, y):
    """attr [N, 2]: lane l takes edges l, l + 64, .. of the row in stored order by fused multiply-adds from 0; one butterfly."""
    y = np.asarray(y, np.float32)
    n = y.shape[0]
    out = np.zeros((n, 2), np.float32)
    for i in range(n):
        lo, hi = int(row_start[i]), int(row_start[i + 1])
        acc = np.zeros((64, 2), np.float32)
        for first in range(lo, hi, 64):
            e = np.arange(first, min(first + 64, hi))
            lane = e - first
            dx, dy = y[i, 0] - y[nbr[e], 0], y[i, 1] - y[nbr[e], 1]
            w = P[e] * q32(dx, dy)
            assert w.dtype == np.float32
            acc[lane, 0] = fma32(w, dx, acc[lane, 0])
            acc[lane, 1] = fma32(w, dy, acc[lane, 1])
        out[i] = butterfly32(acc[:, 0].copy()), butterfly32(acc[:, 1].copy())
    return out


def slice_sum32(col):
    """Slices of 2048 rows: lane l adds rows first + l + 64 u, u ascending, from 0; the butterfly; the slices in order from 0."""
    col = np.asarray(col, np.float32)
    n = col.shape[0]
    slices = (n + SLICE - 1) // SLICE
    padded = np.zeros(slices * SLICE, np.float32)
    padded[:n] = col
    total = F(0.0)
    for s in range(slices):
        v = np.zeros(64, np.float32)
        for u in range(SLICE // 64):
            v = v + padded[s * SLICE + 64 * u:s * SLICE + 64 * u + 64]
        total = F(total + butterfly32(v))
    return total


def update32(y, v, gain, attr, rep, z, exaggeration, momentum, rate, min_gain=0.01):
    """(y, v, gain, Z) after one update, every step one float32 operation."""
    y, v, gain, attr, rep = (np.asarray(a, np.float32) for a in (y, v, gain, attr, rep))
    ex, mom, rate, floor = F(exaggeration), F(momentum), F(rate), F(min_gain)
    total = slice_sum32(z)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        g = F(4.0) * (ex * attr - rep / total)
        assert g.dtype == np.float32
        differ = (g > 0) != (v > 0)
        gain = np.fmax(np.where(differ, gain + F(0.2), gain * F(0.8)), floor).astype(np.float32)
        v = fma32(np.full_like(v, mom), v, -((rate * gain) * g))
        y = y + v
        n = F(y.shape[0])
        mean = np.array([slice_sum32(y[:, 0]) / n, slice_sum32(y[:, 1]) / n], np.float32)
        y = y - mean[None, :]
    assert y.dtype == v.dtype == gain.dtype == np.float32
    return y, v, gain, total


# ---------------------------------------------------------------------------------------------------- plain, any dtype
def usable(ids, sims):
    return (np.asarray(ids) >= 0) & np.isfinite(np.asarray(sims, np.float64))


def affinities(ids, sims, perplexity, dt):
    """(p [N, k], beta [N]) in dtype dt: 64 bisection steps from beta = 1, doubling while unbounded."""
    ok = usable(ids, sims)
    s = np.where(ok, np.asarray(sims, np.float32), 0).astype(dt)
    d = np.maximum(dt(0), dt(2) - dt(2) * s)
    d = np.where(ok, d, np.inf)
    with np.errstate(invalid="ignore"):
        d = np.where(ok, d - d.min(axis=1, keepdims=True), 0).astype(dt)
    m = ok.sum(axis=1)
    n = d.shape[0]
    beta, lo, hi = np.ones(n, dt), np.zeros(n, dt), np.full(n, np.inf, dt)
    target = np.log(dt(perplexity))

    def terms(beta):
        with np.errstate(under="ignore"):
            return np.where(ok, np.exp(-(d * beta[:, None])), 0).astype(dt)

    with np.errstate(invalid="ignore", divide="ignore", under="ignore", over="ignore"):
        for _ in range(BISECTIONS):
            e = terms(beta)
            total = e.sum(axis=1)
            h = np.log(total) + beta * (d * e).sum(axis=1) / total
            big = h > target
            lo, hi = np.where(big, beta, lo), np.where(big, hi, beta)
            beta = np.where(np.isinf(hi), beta * dt(2), dt(0.5) * (lo + hi)).astype(dt)
        e = terms(beta)
        p = e / e.sum(axis=1, keepdims=True)
        short = (m > 0) & (m <= perplexity)
        p = np.where(short[:, None], ok / np.maximum(m, 1)[:, None].astype(dt), p)
        p = np.where((m == 0)[:, None], 0, p)
        beta = np.where(short | (m == 0), 0, beta)
    assert p.dtype == dt and beta.dtype == dt
    return p, beta


def perplexity_of(p):
    """exp(entropy) of every row of p, in float64."""
    p = np.asarray(p, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.exp(-(np.where(p > 0, p * np.log(p), 0)).sum(axis=1))


def joint(ids, p):
    """(row_start int64, nbr int32, P float32): (p_j|i + p_i|j) / (2 N) in float64, rounded once; rows ascend; zeros left out."""
    ids = np.asarray(ids)
    n = ids.shape[0]
    dense = np.zeros((n, n), np.float64)
    for i in range(n):
        for s, j in enumerate(ids[i]):
            if j >= 0 and j != i:
                dense[i, j] += float(p[i, s])
    dense = ((dense + dense.T) / (2.0 * n)).astype(np.float32)
    i, j = np.nonzero(dense)
    row_start = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(i, minlength=n), out=row_start[1:])
    return row_start, j.astype(np.int32), dense[i, j]


def dense_of(row_start, nbr, P, dt):
    n = row_start.shape[0] - 1
    dense = np.zeros((n, n), dt)
    dense[np.repeat(np.arange(n), np.diff(row_start)), nbr] = P
    return dense


def forces(dense, y, dt):
    """(attr, rep, z per row, q) of the dense P at y, vectorised."""
    diff = y[:, None, :] - y[None, :, :]
    q = dt(1) / (dt(1) + (diff * diff).sum(axis=2))
    np.fill_diagonal(q, 0)
    attr = ((dense * q)[:, :, None] * diff).sum(axis=1)
    rep = ((q * q)[:, :, None] * diff).sum(axis=1)
    return attr.astype(dt), rep.astype(dt), q.sum(axis=1).astype(dt), q


def kl(row_start, nbr, P, y, dt):
    """sum_e P_e (log P_e - log q_e + log Z) in dtype dt."""
    y = np.asarray(y).astype(dt)
    n = y.shape[0]
    src = np.repeat(np.arange(n), np.diff(row_start))
    diff = y[src] - y[nbr]
    q = dt(1) / (dt(1) + (diff * diff).sum(axis=1))
    _, _, z, _ = forces(np.zeros((n, n), dt), y, dt)
    big = np.asarray(P).astype(dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(big > 0, big * (np.log(big) - np.log(q) + np.log(z.sum())), 0).sum()


def fit(row_start, nbr, P, init, dt, n_iter=750, exaggeration_iter=250, early_exaggeration=12.0, momentum=(0.5, 0.8), rate=None,
        min_gain=0.01):
    """The layout loop, plain and vectorised in dtype dt: (y, kl)."""
    dense = dense_of(row_start, nbr, np.asarray(P), dt)
    y = np.asarray(init).astype(dt)
    n = y.shape[0]
    v, gain = np.zeros_like(y), np.ones_like(y)
    rate = dt(max(n / early_exaggeration / 4.0, 50.0) if rate is None else rate)
    for it in range(n_iter):
        ex = dt(early_exaggeration if it < exaggeration_iter else 1.0)
        mom = dt(momentum[0] if it < exaggeration_iter else momentum[1])
        attr, rep, z, _ = forces(dense, y, dt)
        g = dt(4) * (ex * attr - rep / z.sum())
        differ = (g > 0) != (v > 0)
        gain = np.maximum(np.where(differ, gain + dt(0.2), gain * dt(0.8)), dt(min_gain)).astype(dt)
        v = (mom * v - rate * gain * g).astype(dt)
        y = y + v
        y = (y - y.mean(axis=0)).astype(dt)
    return y, kl(row_start, nbr, P, y, dt)


# ---------------------------------------------------------------------------------------------------- quality
def _map_neighbours(y, k):
    y = np.asarray(y, np.float64)
    d = ((y[:, None, :] - y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    return np.argsort(d, axis=1, kind="stable")[:, :k]


def purity10(y, truth):
    """The share of a window's 10 nearest map neighbours that carry its label."""
    truth = np.asarray(truth)
    return float((truth[_map_neighbours(y, 10)] == truth[:, None]).mean())


def preservation(y, ids, k=10):
    """The mean share of a window's k best list entries among its k nearest map neighbours."""
    near = _map_neighbours(y, k)
    shares = []
    for i in range(near.shape[0]):
        best = ids[i, :k][ids[i, :k] >= 0]
        if best.size:
            shares.append(np.isin(best, near[i]).sum() / best.size)
    return float(np.mean(shares))


def pca_plane(e):
    """The first two principal components of the rows by NumPy's SVD, float64."""
    x = np.asarray(e, np.float64)
    x = x - x.mean(axis=0)
    _, _, vt = np.linalg.svd(x, full_matrices=False)
    return x @ vt[:2].T


def start_of(plane):
    """The PCA start: scaled in float64 so that the first coordinate's standard deviation is 1e-4."""
    return (plane / plane[:, 0].std() * 1e-4).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- constructed cases
SCALES = ("start", "converged", "mix")


def coords(n, scale, seed=5, special=True):
    """[n, 2] float32 at one of three scales (the 1e-4 start, a converged map of span about 20, a mix of both) with, where
    there is room: coincident points (rows 1 and n - 1 equal row 0), a point at 1e10 (q * q is a subnormal there) and one at
    1e15 (q * q underflows to 0)."""
    rng = np.random.default_rng(seed + n)
    y = rng.normal(size=(n, 2))
    if scale == "start":
        y *= 1e-4
    elif scale == "converged":
        y *= 6.0
    else:
        y *= np.where(rng.random(n) < 0.5, 1e-4, 6.0)[:, None]
    y = y.astype(np.float32)
    if special and n > 1:
        y[1] = y[0]
    if special and n > 8:
        y[n - 1] = y[0]
        y[4] = (1e10, -1e10)
        y[6] = (-3.0, 1e15)
    return y


def graph_case(seed=11, n=310):
    """A CSR graph of n rows with a row of degree 0 (row 0), one of degree 1 (row 1), a hub of degree 300 (row 2: several rounds
    a lane), zero weights among the edges: (row_start, nbr, P)."""
    rng = np.random.default_rng(seed)
    degree = rng.integers(2, 9, size=n)
    degree[0], degree[1], degree[2] = 0, 1, 300
    row_start = np.zeros(n + 1, np.int64)
    np.cumsum(degree, out=row_start[1:])
    nbr = rng.integers(0, n, size=int(row_start[-1])).astype(np.int32)
    P = (rng.random(nbr.shape[0]) ** 4 / n).astype(np.float32)
    P[rng.random(nbr.shape[0]) < 0.05] = 0.0
    return row_start, nbr, P


def update_case(n, seed=9):
    """(y, v, gain, attr, rep, z) with every sign pairing of gradient and velocity in the first rows: g = 0 (attr = rep = 0)
    against v = 0, +0 and -0, g > 0 and g < 0 against v of either sign and 0, and gains sitting at the floor."""
    rng = np.random.default_rng(seed + n)
    y = (6.0 * rng.normal(size=(n, 2))).astype(np.float32)
    v = (0.1 * rng.normal(size=(n, 2))).astype(np.float32)
    gain = (0.01 + rng.random((n, 2)) * 2).astype(np.float32)
    attr = (1e-4 * rng.normal(size=(n, 2))).astype(np.float32)
    rep = (rng.normal(size=(n, 2))).astype(np.float32)
    z = (1.0 + rng.random(n) * n).astype(np.float32)
    for r, (a, rp, vel) in enumerate(((0.0, 0.0, 0.0), (0.0, 0.0, -0.0), (-0.0, 0.0, 0.0), (0.0, 0.0, 0.3), (1e-3, 0.0, 0.0),
                                      (1e-3, 0.0, 0.2), (1e-3, 0.0, -0.2), (-1e-3, 0.0, 0.2), (-1e-3, 0.0, -0.2))):
        if r < n:
            attr[r], rep[r], v[r] = a, rp, vel
    gain[min(9, n - 1)] = 0.01                         # at the floor: x 0.8 would take it below
    gain[min(10, n - 1)] = 0.0105
    return y, v, gain, attr, rep, z


def lists_case(n, k, seed=21):
    """Lists [n, k] of random cosine similarities, best first, with the rows the calibration must survive (where they exist):
    row 0 empty, row 1 with one neighbour, row 2 all duplicates (sim = 1 everywhere), row 3 with non-finite similarities among
    finite ones, row 4 short of any perplexity above 2 (two neighbours)."""
    rng = np.random.default_rng(seed + 64 * n + k)
    ids = np.stack([rng.permutation(n - 1)[:k] if n - 1 >= k else np.concatenate([rng.permutation(n - 1), -np.ones(k - n + 1, int)])
                    for _ in range(n)]).astype(np.int32)
    ids[ids >= np.arange(n)[:, None]] += 1             # no row lists itself
    sims = np.sort(1.0 - rng.random((n, k)) ** 2 * 0.6, axis=1)[:, ::-1].astype(np.float32)
    sims[ids < 0] = 0.0
    if n > 8:
        ids[0], sims[0] = -1, 0.0
        ids[1, 1:], sims[1, 1:] = -1, 0.0
        sims[2] = 1.0
        sims[3, ::3] = (np.nan, np.inf, -np.inf)[k % 3] if k > 0 else 0
        ids[4, 2:], sims[4, 2:] = -1, 0.0
    return ids, sims
