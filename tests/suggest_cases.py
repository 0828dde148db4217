"""What tests/test_suggest_host.py and tests/test_suggest_gpu.py share: the cases, their inputs, and statements of
include/buzzdetect_suggest.h in NumPy that share nothing with the library - the acquisition at any dtype (float64 is the
reference, float32 the yardstick of the 8 x rule of DESIGN §15) and the greedy pick as a plain loop."""
import numpy as np

# (members, classes, scale of the N(0, 1) logits, target column or None, link)
ACQUIRE_CASES = (
    (2, 2, 1.0, None, "softmax"),
    (2, 13, 3.0, None, "softmax"),
    (5, 13, 3.0, None, "softmax"),
    (5, 13, 30.0, None, "softmax"),
    (64, 64, 3.0, None, "softmax"),
    (3, 2, 80.0, None, "softmax"),
    (5, 13, 3.0, 4, "softmax"),
    (5, 1, 3.0, 0, "sigmoid"),
)
ONE_MEMBER_CASE = (1, 13, 3.0, None, "softmax")          # BALD is exactly 0 there: held under a check of its own
ACQUIRE_WINDOWS = 257


def case_id(case):
    m, c, scale, target, link = case
    return f"M{m}-C{c}-x{scale:g}-{'all' if target is None else 't%d' % target}-{link}"


def case_logits(case, windows=ACQUIRE_WINDOWS):
    """float32 [W, M, C]; one generator per case, seeded by the case."""
    m, c, scale, target, _ = case
    rng = np.random.default_rng([m, c, int(scale), 99 if target is None else target])
    return (rng.normal(size=(windows, m, c)) * scale).astype(np.float32)


def as_wide(z):
    """[W, M, C] -> ([W, M * C] with the members side by side, member_first, C)."""
    w, m, c = z.shape
    return np.ascontiguousarray(z.reshape(w, m * c)), [i * c for i in range(m)], c


def _xlogx(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x > 0, x * np.log(np.where(x > 0, x, 1)), x * 0)


def acquire_numpy(z, link, target, dtype):
    """The three scores [3, W] of logits [W, M, C], every operation at ``dtype``: the formulas as one writes them down."""
    z = np.asarray(z).astype(dtype)
    members, classes = z.shape[1], z.shape[2]
    if link == "sigmoid":
        q = 1 / (1 + np.exp(-z[:, :, target]))
        p = np.stack([q, 1 - q], axis=-1)
    else:
        e = np.exp(z - z.max(axis=-1, keepdims=True))
        p = e / e.sum(axis=-1, keepdims=True)
        if target is not None:
            q = p[:, :, target]
            p = np.stack([q, 1 - q], axis=-1)
    assert p.dtype == dtype
    scale = np.log(dtype(classes if target is None else 2))
    pbar = p.sum(axis=1) / dtype(members)
    h_bar = -_xlogx(pbar).sum(axis=-1)
    h_members = -_xlogx(p).sum(axis=-1).sum(axis=1) / dtype(members)
    ordered = np.sort(pbar, axis=-1)
    out = np.stack([h_bar / scale, 1 - (ordered[:, -1] - ordered[:, -2]), np.maximum(h_bar - h_members, 0) / scale])
    assert out.dtype == dtype
    return np.clip(out, 0, 1)


def deviations(got, z, link, target):
    """Per strategy: (largest deviation of ``got`` from float64, that of the float32 NumPy statement)."""
    want = acquire_numpy(z, link, target, np.float64)
    plain = acquire_numpy(z, link, target, np.float32)
    assert plain.dtype == np.float32 and want.dtype == np.float64
    return np.abs(got.astype(np.float64) - want).max(axis=1), np.abs(plain.astype(np.float64) - want).max(axis=1)


# ---------------------------------------------------------------------------------------------------- the pick
def pick_numpy(sim, gain, d0, k):
    """The loop of include/buzzdetect_suggest.h in NumPy float32: (picked, value, dist)."""
    sim, gain = np.asarray(sim, np.float32), np.asarray(gain, np.float32)
    n = gain.size
    d = np.ones(n, np.float32) if d0 is None else np.array(d0, np.float32)
    chosen = np.zeros(n, bool)
    picked, value, dist = np.zeros(k, np.int32), np.zeros(k, np.float32), np.zeros(k, np.float32)
    one, zero = np.float32(1), np.float32(0)
    for t in range(k):
        with np.errstate(invalid="ignore"):
            g = gain * d
        rank = np.where(np.isnan(g), np.float32(-np.inf), g)      # (-0.0 == +0.0 already)
        rest = np.flatnonzero(~chosen)
        won = int(rest[np.argmax(rank[rest])])                   # argmax: the first of equal values
        chosen[won] = True
        picked[t], value[t], dist[t] = won, g[won], d[won]
        d = np.fmin(d, np.fmax(one - sim[won, :n], zero))
    return picked, value, dist


PICK_SIZES = (1, 2, 63, 64, 65, 1024)


def pick_inputs(n, kind, seed=5):
    """(sim float32 [n, n], gain [n], d0 [n] or None) of one kind of input."""
    rng = np.random.default_rng([seed, n])
    sim = rng.uniform(-1, 1, (n, n)).astype(np.float32)
    np.fill_diagonal(sim, 1.0)
    gain = rng.uniform(0, 1, n).astype(np.float32)
    d0 = None
    if kind == "equal":
        gain[:] = 0.5
        sim[:] = 0.0                                             # nothing discounts anything: the picks ascend
        np.fill_diagonal(sim, 1.0)
    elif kind == "duplicates":                                   # candidates 2 j and 2 j + 1 are the same row
        for j in range(0, n - 1, 2):
            sim[j + 1, :] = sim[j, :]
            sim[:, j + 1] = sim[:, j]
            sim[j, j + 1] = sim[j + 1, j] = sim[j + 1, j + 1] = 1.0
            gain[j + 1] = gain[j]
        sim = np.minimum(sim, sim.T)
        np.clip(sim, -1.0, 0.5, out=sim)                         # everything else stays at a distance of at least 0.5
        for j in range(0, n - 1, 2):
            sim[j, j + 1] = sim[j + 1, j] = 1.0
        np.fill_diagonal(sim, 1.0)
        gain = gain * 0.5 + 0.5
    elif kind == "d0":
        d0 = rng.uniform(0, 1, n).astype(np.float32)
        d0[rng.integers(0, n, max(1, n // 4))] = 0.0
    elif kind == "specials":
        for i, v in zip(rng.permutation(n)[:3], (np.nan, -0.0, -0.25)):
            gain[i] = v
    else:
        assert kind == "random"
    return np.ascontiguousarray(sim), gain.astype(np.float32), d0


PICK_KINDS = ("random", "equal", "duplicates", "d0", "specials")


def same_bytes(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()
