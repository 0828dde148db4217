"""Inputs and the NumPy restatement shared by tests/test_eval_host.py and tests/test_eval_gpu.py (a plain module, like
calls_cases.py): the definitions of include/buzzdetect_eval.h written out with np.bincount over kf and kr - not the library's
routine - and the generator whose logits sit where the two integers can go wrong: on the 0.01 grid, halfway between two grid
points, one ulp either side of a grid point, at and just beyond the ends of the range, and the values that are no number."""
import numpy as np

BINS, K_MIN, K_MAX = 16384, -8192, 8191
KINDS = ("normal", "grid", "half", "ulp")
EDGE = np.array([-81.92, 81.91], np.float32)                      # the ends of the range as float32
SPECIALS = np.concatenate([
    np.array([np.inf, -np.inf, np.nan, -0.0, 0.0], np.float32),
    EDGE, np.nextafter(EDGE, np.float32(np.inf)), np.nextafter(EDGE, np.float32(-np.inf)),
    np.array([81.915, 81.92, 81.925, -81.925, -81.93, 1e30, -1e30, 3.4e38], np.float32)])
LABELS = np.array([0, 1, 2, 7], np.uint8)


# ---------------------------------------------------------------------------------------------------- the definitions
def rows_numpy(z32):
    """(kf, kr) as float64 of finite float32 logits: kr = rint(z * 100.0); kf = max{k : k / 100.0 <= z}, found among the five
    integers around floor(z * 100.0)."""
    z = np.asarray(z32, np.float32).astype(np.float64)
    kr = np.rint(z * 100.0)
    base = np.floor(z * 100.0)
    kf = np.full(z.shape, -np.inf)
    for step in (-2, -1, 0, 1, 2):
        k = base + step
        kf = np.where(k / 100.0 <= z, np.maximum(kf, k), kf)
    assert np.isfinite(kf).all() and ((kr == kf) | (kr == kf + 1)).all()
    return kf, kr


def sweep_numpy(x, labels, label_of):
    """(hist uint32 [C, 3, BINS], tail uint32 [C, 4]) of float32 x [W, C], uint8 labels [W, L] and label_of [C]."""
    w, c = x.shape
    hist, tail = np.zeros((c, 3, BINS), np.uint32), np.zeros((c, 4), np.uint32)
    for col in range(c):
        if label_of[col] < 0:
            continue
        lab = labels[:, label_of[col]]
        z = x[:, col]
        used = lab <= 1
        finite = np.isfinite(z)
        kf, kr = rows_numpy(np.where(finite, z, np.float32(0)))
        below = finite & ((kf < K_MIN) | (kr < K_MIN))
        above = finite & ~below & ((kf > K_MAX) | (kr > K_MAX))
        inside = used & finite & ~below & ~above
        tail[col] = ((~used).sum(), (used & ~finite).sum(), (used & below).sum(), (used & above).sum())
        for plane, rows, k in ((0, inside & (lab == 0), kf), (1, inside & (lab == 1), kf), (2, inside, kr)):
            hist[col, plane] = np.bincount((k[rows] - K_MIN).astype(np.int64), minlength=BINS)
        assert int(tail[col].sum()) + int(hist[col, 2].sum()) == w == int(tail[col].sum()) + int(hist[col, :2].sum())
    return hist, tail


# ---------------------------------------------------------------------------------------------------- the generator
def draw_logits(rng, n, kind, spread=300):
    """float32 [n] of one kind: normal; k / 100; (k + 0.5) / 100; nextafter of k / 100 towards either side."""
    k = rng.integers(-spread, spread + 1, size=n)
    if kind == "normal":
        return rng.normal(0.0, 2.0, size=n).astype(np.float32)
    if kind == "grid":
        return (k / 100.0).astype(np.float32)
    if kind == "half":
        return ((k + 0.5) / 100.0).astype(np.float32)
    assert kind == "ulp"
    side = rng.choice(np.array([-np.inf, np.inf], np.float32), size=n)
    return np.nextafter((k / 100.0).astype(np.float32), side)


def draw(seed, w, c, n_labels=None, specials=True):
    """(x float32 [w, c] C-contiguous, labels uint8 [w, L], label_of int32 [c]): every column a mix of the four kinds, about one
    value in sixteen from SPECIALS; labels from {0, 1, 2, 7}; label_of shares label columns when c > L."""
    rng = np.random.default_rng(seed)
    n_labels = max(1, (c + 1) // 2) if n_labels is None else n_labels
    x = np.empty((w, c), np.float32)
    for col in range(c):
        parts = np.stack([draw_logits(rng, w, kind) for kind in KINDS])
        x[:, col] = parts[rng.integers(0, len(KINDS), size=w), np.arange(w)]
    if specials:
        special = rng.random(size=(w, c)) < 1 / 16
        x[special] = rng.choice(SPECIALS, size=int(special.sum()))
    labels = rng.choice(LABELS, size=(w, n_labels), p=[0.5, 0.3, 0.1, 0.1]).astype(np.uint8)
    label_of = rng.integers(0, n_labels, size=c).astype(np.int32)
    return x, labels, label_of


def layout(x, which):
    """The same matrix window-major ("rows": [W][C]) or column-major ("columns": a column's windows are consecutive)."""
    return np.ascontiguousarray(x) if which == "rows" else np.ascontiguousarray(x.T).T


def normalised(table):
    """A metrics table with a leading ``-0,`` replaced by ``0,`` (np.unique sometimes keeps -0.0 for the zero row)."""
    return "\n".join("0," + line[3:] if line.startswith("-0,") else line for line in table.split("\n"))
