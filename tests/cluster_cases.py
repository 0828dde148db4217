"""Inputs and NumPy restatements shared by tests/test_cluster_host.py and tests/test_cluster_gpu.py (a plain module, like
gpu_guards.py): the planted fixture, the constructed-label case, and the chunked sums and slice statistics of
include/buzzdetect_cluster.h spelled out in float32 NumPy."""
import numpy as np

from buzzdetect_amd import _lib, search

CHUNK = 256
SIZES = (0, 1, 255, 256, 257, 513)              # members per cluster: the chunk edges, an empty cluster, a third chunk
FIXTURES = ((1025, 5), (1025, 33), (257, 65), (64, 1), (33, 32))
NORM_FLOOR = np.float32(_lib.SEARCH_NORM_FLOOR)


def fixture(w, k):
    """The planted partition: (E float32 [w, 1024], truth [w]); the starting centroids are E[:k], one of every cluster."""
    rng = np.random.default_rng(2025)
    centres = 2.0 * np.abs(rng.normal(size=(k, 1024)))
    truth = rng.integers(0, k, size=w)
    truth[:k] = np.arange(k)
    e = (centres[truth] + 0.5 * rng.normal(size=(w, 1024))).astype(np.float32)
    return e, truth


def candidates64(e, c, metric):
    """t[w][j] in float64 for centroids c (already at unit length for a cosine), and the rows' squared norms."""
    e64, c64 = e.astype(np.float64), c.astype(np.float64)
    s = e64 @ c64.T
    n2 = (e64 * e64).sum(axis=1)
    t = (c64 * c64).sum(axis=1)[None, :] - 2.0 * s if metric == "euclidean" else -s
    return t, n2


def distance64(t_best, n2, metric):
    if metric == "euclidean":
        return np.maximum(n2 + t_best, 0.0)
    return 1.0 - (-t_best) / np.sqrt(n2)


def constructed(seed=7):
    """1282 rows in clusters of SIZES members, interleaved; row `zero` is all zeros and lies in the cluster of 255.  Returns
    (E, labels int32, prev float32 [6, 1024], zero)."""
    rng = np.random.default_rng(seed)
    labels = np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int32)
    rng.shuffle(labels)
    w = labels.shape[0]
    e = (2.0 * np.abs(rng.normal(size=(len(SIZES), 1024)))[labels] + 0.5 * rng.normal(size=(w, 1024))).astype(np.float32)
    zero = int(np.flatnonzero(labels == 2)[100])
    e[zero] = 0.0
    prev = rng.normal(size=(len(SIZES), 1024)).astype(np.float32)
    return e, labels, prev, zero


def centroids_numpy(e, order, offsets, metric, prev):
    """The chunks and chains spelled out: float32 arrays, one rounding per operation, members in the order of `order`.  The
    norm chain (fused multiply-adds NumPy cannot spell) is search.norms_host, which tests/test_search_host.py holds to float64."""
    k = prev.shape[0]
    n2 = search.norms_host(e)
    one = np.float32(1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        rinv = np.where(n2 < NORM_FLOOR, np.float32(0.0), one / np.sqrt(n2)).astype(np.float32)
    out = np.zeros((k, 1024), np.float32)
    for j in range(k):
        members = order[offsets[j]:offsets[j + 1]]
        total = None
        for at in range(0, members.shape[0], CHUNK):
            part = np.zeros(1024, np.float32)
            for r in members[at:at + CHUNK]:
                x = e[r] * rinv[r] if metric == "cosine" else e[r]
                assert x.dtype == np.float32
                part = part + x
            total = part if total is None else total + part
        if total is None:
            out[j] = prev[j]
            continue
        assert total.dtype == np.float32
        if metric == "cosine":
            m2 = search.norms_host(total[None, :])[0]
            out[j] = prev[j] if m2 < NORM_FLOOR else total / np.sqrt(m2)
        else:
            out[j] = total / np.float32(members.shape[0])
    return out


def stats_numpy(dist, labels, prev_labels):
    """Slices of 256: lane l adds rows l, l + 64, l + 128, l + 192 from 0.0f, the 64 sums meet in the butterfly m = 32 .. 1."""
    w = dist.shape[0]
    slices = (w + 255) // 256
    d = np.zeros(slices * 256, np.float32)
    d[:w] = dist
    differs = np.zeros(slices * 256, bool)
    differs[:w] = labels != prev_labels
    lanes = np.arange(64)
    partial, changed = np.zeros(slices, np.float32), np.zeros(slices, np.int32)
    for s in range(slices):
        v = np.zeros(64, np.float32)
        for u in range(4):
            v = v + d[256 * s + 64 * u:256 * s + 64 * u + 64]
        for m in (32, 16, 8, 4, 2, 1):
            v = v + v[lanes ^ m]
        assert v.dtype == np.float32
        partial[s] = v[0]
        changed[s] = differs[256 * s:256 * s + 256].sum()
    return partial, changed
