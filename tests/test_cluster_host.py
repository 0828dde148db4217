"""The host side of k-means clustering (include/buzzdetect_cluster.h, buzzdetect_amd/cluster.py), no device needed: the order
against np.argsort, the chunked sums against a spelled-out float32 loop in every bit and against float64 under the 8 x rule
(DESIGN §15), the slice statistics, what is refused, the results' files, and the k-means++ draw."""
import csv
import os
import re

import numpy as np
import pytest

from buzzdetect_amd import _lib, cluster, dataset, search
from tests import cluster_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ("euclidean", "cosine")


def test_prototypes_are_the_header():
    with open(os.path.join(ROOT, "include", "buzzdetect_cluster.h")) as f:
        header = f.read()
    names = sorted(re.findall(r"^BD_API [^;(]*?(bd_\w+)\(", header, re.M))
    assert names == sorted(_lib.CLUSTER_PROTOTYPES) and len(names) == 9
    for name in names:
        args = re.search(r"BD_API [^;(]*?" + name + r"\(([^;]*)\);", header).group(1)
        n_args = 0 if args.strip() == "void" else args.count(",") + 1
        assert len(_lib.CLUSTER_PROTOTYPES[name][1]) == n_args, name
    assert _lib.load().bd_cluster_abi_version() == _lib.CLUSTER_ABI_VERSION == 1
    for word, value in (("BD_CLUSTER_MAX_CLUSTERS", _lib.CLUSTER_MAX_CLUSTERS), ("BD_CLUSTER_DIM", _lib.CLUSTER_DIM),
                        ("BD_CLUSTER_CHUNK", _lib.CLUSTER_CHUNK), ("BD_CLUSTER_STAT_SLICE", _lib.CLUSTER_STAT_SLICE),
                        ("BD_CLUSTER_ORDER_SLICE", _lib.CLUSTER_ORDER_SLICE)):
        assert int(re.search(r"#define " + word + r" (\d+)", header).group(1)) == value
    assert "#define BD_CLUSTER_MAX_ROWS (1 << 24)" in header and _lib.CLUSTER_MAX_ROWS == 1 << 24
    assert _lib.CLUSTER_METRICS == {"euclidean": 0, "cosine": 1}


# ---------------------------------------------------------------------------------------------------- order
@pytest.mark.parametrize("w,k", ((1, 1), (63, 2), (64, 3), (1025, 5), (4097, 33), (3000, 1024)))
def test_order_is_the_stable_argsort(w, k):
    rng = np.random.default_rng(w + k)
    labels = rng.integers(0, k, size=w).astype(np.int32)
    order, offsets = cluster.order_host(labels, k)
    assert order.tolist() == np.argsort(labels, kind="stable").tolist()
    assert offsets.tolist() == [0] + np.cumsum(np.bincount(labels, minlength=k)).tolist()
    same = np.full(w, k - 1, np.int32)                                   # every row in the last cluster
    order, offsets = cluster.order_host(same, k)
    assert order.tolist() == list(range(w)) and offsets.tolist() == [0] * k + [w]


def test_order_of_the_constructed_labels():
    _, labels, _, _ = cases.constructed()
    order, offsets = cluster.order_host(labels, len(cases.SIZES))
    assert np.diff(offsets).tolist() == list(cases.SIZES)
    assert order.tolist() == np.argsort(labels, kind="stable").tolist()


# ---------------------------------------------------------------------------------------------------- centroids
@pytest.fixture(scope="module")
def built():
    """The constructed case once: rows, labels, order, offsets, previous centroids, the zero row, the rows' norms."""
    e, labels, prev, zero = cases.constructed()
    order, offsets = cluster.order_host(labels, len(cases.SIZES))
    return e, labels, order, offsets, prev, zero, search.norms_host(e)


@pytest.mark.parametrize("metric", METRICS)
def test_centroids_are_the_spelled_out_chains_in_every_bit(built, metric):
    e, labels, order, offsets, prev, zero, n2 = built
    if metric == "cosine":
        prev = cluster.normalise_centroids(prev, metric)
    cent, packed, c2 = cluster.centroids_host(e, n2, order, offsets, metric, prev)
    want = cases.centroids_numpy(e, order, offsets, metric, prev)
    assert cent.tobytes() == want.tobytes()
    assert cent[0].tobytes() == prev[0].tobytes()                        # the empty cluster keeps its centroid's bits
    assert cent[1].tobytes() == (e[order[0]] if metric == "euclidean" else want[1]).tobytes()      # one member: itself
    assert packed.tobytes() == search.pack_queries(cent).tobytes()
    assert c2.tobytes() == search.norms_host(cent).tobytes()
    assert n2[zero] == 0.0 and labels[zero] == 2
    if metric == "cosine":
        assert np.abs(c2[1:] - 1.0).max() < 1e-6


@pytest.mark.parametrize("metric", METRICS)
def test_centroids_against_float64_under_the_8x_rule(built, metric):
    """DESIGN §15.  The yardstick is the plain float32 NumPy restatement: the members' rows (for a cosine times the float32
    reciprocal of their float32 length) summed by ndarray.sum over the member axis, then divided; its deviation is counted as
    at least 1e-7 of the largest float64 centroid element (float32's epsilon on the result)."""
    e, labels, order, offsets, prev, zero, n2 = built
    if metric == "cosine":
        prev = cluster.normalise_centroids(prev, metric)
    cent, _, _ = cluster.centroids_host(e, n2, order, offsets, metric, prev)
    live = [j for j, n in enumerate(cases.SIZES) if n]
    want, plain = np.zeros((len(live), 1024)), np.zeros((len(live), 1024), np.float32)
    e64 = e.astype(np.float64)
    for i, j in enumerate(live):
        rows = np.flatnonzero(labels == j)
        if metric == "cosine":
            length = np.sqrt((e64[rows] ** 2).sum(axis=1, keepdims=True))
            total = np.divide(e64[rows], length, out=np.zeros_like(e64[rows]), where=length > 0).sum(axis=0)
            want[i] = total / np.sqrt((total * total).sum())
            l32 = np.sqrt((e[rows] * e[rows]).sum(axis=1, keepdims=True, dtype=np.float32))
            t32 = np.divide(e[rows], l32, out=np.zeros_like(e[rows]), where=l32 > 0).sum(axis=0, dtype=np.float32)
            plain[i] = t32 / np.sqrt((t32 * t32).sum(dtype=np.float32))
        else:
            want[i] = e64[rows].mean(axis=0)
            plain[i] = e[rows].sum(axis=0, dtype=np.float32) / np.float32(rows.size)
    assert plain.dtype == np.float32
    dev = np.abs(cent[live].astype(np.float64) - want).max()
    ref = max(np.abs(plain.astype(np.float64) - want).max(), 1e-7 * np.abs(want).max())
    print(f"{metric}: host deviation {dev:.3e}, float32 NumPy deviation {ref:.3e}, ratio {dev / ref:.2f}")
    assert dev <= 8.0 * ref


def test_a_cosine_sum_without_direction_keeps_the_previous_centroid():
    """Two opposite rows cancel exactly: m2 = 0 is below the norm floor."""
    rng = np.random.default_rng(3)
    e = np.zeros((3, 1024), np.float32)
    e[0] = rng.normal(size=1024)
    e[1] = -e[0]
    e[2] = rng.normal(size=1024)
    prev = cluster.normalise_centroids(rng.normal(size=(2, 1024)), "cosine")
    order, offsets = cluster.order_host(np.array([0, 0, 1], np.int32), 2)
    cent, _, c2 = cluster.centroids_host(e, search.norms_host(e), order, offsets, "cosine", prev)
    assert cent[0].tobytes() == prev[0].tobytes() and cent[1].tobytes() != prev[1].tobytes()
    assert c2.tobytes() == search.norms_host(cent).tobytes()


# ---------------------------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("w", (1, 255, 256, 257, 1025))
def test_stats_are_the_spelled_out_slices(w):
    rng = np.random.default_rng(w)
    dist = (np.abs(rng.normal(size=w)) * rng.choice([1e-3, 1.0, 1e3], size=w)).astype(np.float32)
    labels = rng.integers(0, 4, size=w).astype(np.int32)
    prev = labels.copy()
    flip = rng.random(w) < 0.3
    prev[flip] = (prev[flip] + 1) % 4
    partial, changed = cluster.stats_host(dist, labels, prev)
    want_p, want_c = cases.stats_numpy(dist, labels, prev)
    assert partial.tobytes() == want_p.tobytes() and changed.tolist() == want_c.tolist()
    assert changed.sum() == flip.sum() and partial.shape == ((w + 255) // 256,)
    assert abs(partial.astype(np.float64).sum() - dist.astype(np.float64).sum()) <= 1e-6 * dist.astype(np.float64).sum()


# ---------------------------------------------------------------------------------------------------- refusals
def refused(fn, *args):
    rc = fn(*args)
    assert rc < 0
    return rc, _lib.load().bd_last_error().decode()


def aligned(n, dtype=np.float32):
    raw = np.zeros(n + 4, dtype)
    return raw[(-raw.ctypes.data // raw.itemsize) % 4:][:n]


@pytest.mark.parametrize("device_entry", (False, True))
def test_bad_arguments_are_refused_by_name(device_entry):
    """Also for the device entry points: the checks come before anything touches the device, so nothing is launched (the
    pointers here are host arrays) and nothing is written."""
    lib = _lib.load()
    e, prev, cent = aligned(4 * 1024), aligned(2 * 1024), aligned(2 * 1024)
    packed = aligned(32 * 1024)
    n2, c2 = np.ones(4, np.float32), np.full(2, 7.0, np.float32)
    labels, order, offsets = np.zeros(4, np.int32), np.full(4, 9, np.int32), np.array([0, 2, 4], np.int32)
    ws = aligned(1 << 16)
    tail = (ws.ctypes.data, ws.nbytes, None) if device_entry else ()

    def order_call(w, k, lab=labels.ctypes.data, ordr=order.ctypes.data, off=offsets.ctypes.data):
        return refused(lib.bd_cluster_order if device_entry else lib.bd_cluster_order_host, lab, w, k, ordr, off, *tail)

    def cent_call(w, k, metric, **kw):
        a = dict(e=e.ctypes.data, n2=n2.ctypes.data, order=order.ctypes.data, offsets=offsets.ctypes.data, prev=prev.ctypes.data,
                 centroids=cent.ctypes.data, packed=packed.ctypes.data, c2=c2.ctypes.data)
        a.update(kw)
        fn = lib.bd_cluster_centroids if device_entry else lib.bd_cluster_centroids_host
        return refused(fn, a["e"], w, a["n2"], a["order"], a["offsets"], k, metric, a["prev"], a["centroids"], a["packed"], a["c2"],
                       *tail)

    for w, k, word in ((4, 0, "n_clusters = 0"), (4, 1025, "n_clusters = 1025"), (-1, 2, "rows = -1"),
                       ((1 << 24) + 1, 2, "rows = 16777217")):
        for rc, text in (order_call(w, k), cent_call(w, k, 0)):
            assert rc == -1 and word in text, text
    for metric in (2, -1):
        rc, text = cent_call(4, 2, metric)
        assert rc == -1 and "metric" in text
    for name in ("labels", "order", "offsets"):
        rc, text = order_call(4, 2, **{{"labels": "lab", "order": "ordr", "offsets": "off"}[name]: None})
        assert rc == -1 and name in text and "null" in text, text
    for name in ("e", "order", "offsets", "prev", "centroids", "packed", "c2"):
        rc, text = cent_call(4, 2, 0, **{name: None})
        assert rc == -1 and name in text and "null" in text, text
    rc, text = cent_call(4, 2, 1, n2=None)                                # a cosine reads the norms
    assert rc == -1 and "n2" in text
    for name, good in (("e", e), ("prev", prev), ("centroids", cent), ("packed", packed)):
        rc, text = cent_call(4, 2, 0, **{name: good.ctypes.data + 4})
        assert rc == -1 and name in text and "aligned" in text, text
    assert (order == 9).all() and (c2 == 7.0).all() and not cent.any()
    if device_entry:
        rc, text = refused(lib.bd_cluster_order, labels.ctypes.data, 4, 2, order.ctypes.data, offsets.ctypes.data, ws.ctypes.data, 16,
                           None)
        assert rc == -4 and "workspace_bytes" in text
        rc, text = refused(lib.bd_cluster_order, labels.ctypes.data, 4, 2, order.ctypes.data, offsets.ctypes.data, None, 1 << 16, None)
        assert rc == -1 and "workspace_dev" in text
    else:
        rc, text = refused(lib.bd_cluster_order_host, np.array([0, 2, 1, 0], np.int32).ctypes.data, 4, 2, order.ctypes.data,
                           offsets.ctypes.data)
        assert rc == -5 and "labels[1] = 2" in text
        rc, text = cent_call(4, 2, 0, offsets=np.array([0, 3, 2], np.int32).ctypes.data)
        assert rc == -5 and "offsets" in text
        rc, text = cent_call(4, 2, 0, order=np.array([0, 1, 2, 4], np.int32).ctypes.data)
        assert rc == -5 and "order[3] = 4" in text


def test_assign_stats_and_the_workspace_query_refuse_before_any_launch():
    lib = _lib.load()
    e, packed = aligned(4 * 1024), aligned(32 * 1024)
    n2, c2, dist = np.ones(4, np.float32), np.ones(2, np.float32), np.full(4, 7.0, np.float32)
    labels, prev = np.full(4, 9, np.int32), np.zeros(4, np.int32)

    def assign(w, k, metric, **kw):
        a = dict(e=e.ctypes.data, n2=n2.ctypes.data, packed=packed.ctypes.data, c2=c2.ctypes.data, labels=labels.ctypes.data,
                 dist=dist.ctypes.data)
        a.update(kw)
        return refused(lib.bd_cluster_assign, a["e"], w, a["n2"], a["packed"], a["c2"], k, metric, a["labels"], a["dist"], None)

    for args, word in (((4, 0, 0), "n_clusters"), ((4, 1025, 1), "n_clusters"), ((-1, 2, 0), "rows"), (((1 << 24) + 1, 2, 0), "rows"),
                       ((4, 2, 2), "metric"), ((4, 2, -1), "metric")):
        rc, text = assign(*args)
        assert rc == -1 and word in text, text
    for name in ("e", "n2", "packed", "c2", "labels", "dist"):
        rc, text = assign(4, 2, 0, **{name: None})
        assert rc == -1 and name + "_dev is null" in text, text
    for name, good in (("e", e), ("packed", packed)):
        rc, text = assign(4, 2, 1, **{name: good.ctypes.data + 4})
        assert rc == -1 and name + "_dev" in text and "aligned" in text, text
    assert (labels == 9).all() and (dist == 7.0).all()
    partial, changed = np.full(1, 7.0, np.float32), np.full(1, 9, np.int32)
    for device_entry in (False, True):
        fn = lib.bd_cluster_stats if device_entry else lib.bd_cluster_stats_host
        tail = (None,) if device_entry else ()
        for w in (-1, (1 << 24) + 1):
            rc, text = refused(fn, dist.ctypes.data, labels.ctypes.data, prev.ctypes.data, w, partial.ctypes.data, changed.ctypes.data,
                               *tail)
            assert rc == -1 and "rows" in text
        for at, name in enumerate(("dist", "labels", "prev_labels", None, "partial", "changed")):
            if name is None:
                continue
            args = [dist.ctypes.data, labels.ctypes.data, prev.ctypes.data, 4, partial.ctypes.data, changed.ctypes.data]
            args[at] = None
            rc, text = refused(fn, *args, *tail)
            assert rc == -1 and name + " is null" in text, text
    assert partial[0] == 7.0 and changed[0] == 9
    assert lib.bd_cluster_workspace_bytes(4, 0) == -1 and lib.bd_cluster_workspace_bytes(4, 1025) == -1
    assert lib.bd_cluster_workspace_bytes(-1, 4) == -1 and lib.bd_cluster_workspace_bytes((1 << 24) + 1, 4) == -1
    # first chunks (K + 1 ints), a count per (slice of 1024 rows, cluster), a 4 KB row per possible chunk; each part to 256 bytes
    assert lib.bd_cluster_workspace_bytes(1025, 5) == 256 + 256 + (1025 // 256 + 5) * 4096
    assert lib.bd_cluster_workspace_bytes(262144, 256) == 1280 + 256 * 256 * 4 + (1024 + 256) * 4096
    with pytest.raises(ValueError):
        cluster.KMeans(0)
    with pytest.raises(ValueError):
        cluster.KMeans(3, metric="manhattan")
    with pytest.raises(ValueError):
        cluster.KMeans(3, init=np.zeros((2, 1024), np.float32))


# ---------------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("w,k", cases.FIXTURES)
@pytest.mark.parametrize("metric", METRICS)
def test_the_planted_fixture_has_wide_margins(w, k, metric):
    """What lets tests/test_cluster_gpu.py hold every row's label to float64: from the starting centroids E[:k] the best and the
    second-best candidate of every row lie at least 0.26 (n2 + max c2) apart (Euclidean), and float32 agrees with float64."""
    e, truth = cases.fixture(w, k)
    c = cluster.normalise_centroids(e[:k], metric)
    t, n2 = cases.candidates64(e, c, metric)
    assert (t.argmin(axis=1) == truth).all()
    s32 = e @ c.T
    t32 = (c * c).sum(axis=1, dtype=np.float32)[None, :] - np.float32(2) * s32 if metric == "euclidean" else -s32
    assert t32.dtype == np.float32 and (t32.argmin(axis=1) == truth).all()
    if k > 1:
        two = np.sort(t, axis=1)[:, :2]
        scale = n2 + (c.astype(np.float64) ** 2).sum(axis=1).max() if metric == "euclidean" else np.sqrt(n2)
        margin = ((two[:, 1] - two[:, 0]) / scale).min()
        print(f"({w}, {k}) {metric}: smallest margin {margin:.3f}")
        # a cosine's candidates are compared on the scale |E[w]| of a score; a float32 score of 1024 terms is off by at most
        # 1024 * 2^-24 = 6e-5 of that, so 1e-3 already separates float32 from float64
        assert margin >= (0.26 if metric == "euclidean" else 1e-3)


# ---------------------------------------------------------------------------------------------------- results
def result():
    labels = [0, 1, 0, 0, 1, 0]
    dist = [0.5, 0.25, 0.125, 0.5, 0.75, 0.125]
    return cluster.ClusterResult(labels, dist, [4, 2, 0], ["site/a", "b"], [0, 0, 0, 1, 1, 1], [0.0, 0.96, 1.92, 0.0, 0.48, 199.68],
                                 centroids=np.arange(3 * 1024, dtype=np.float32).reshape(3, 1024), metric="euclidean",
                                 messages=["a message"])


def test_result_csv_and_representatives(tmp_path):
    res = result()
    path = str(tmp_path / "clusters.csv")
    res.to_csv(path)
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["ident", "start", "end", "cluster", "distance"]
    assert rows[1:] == [["site/a", "0.0", "0.96", "0", "0.5"], ["site/a", "0.96", "1.92", "1", "0.25"],
                        ["site/a", "1.92", "2.88", "0", "0.125"], ["b", "0.0", "0.96", "0", "0.5"],
                        ["b", "0.48", "1.44", "1", "0.75"], ["b", "199.68", "200.64", "0", "0.125"]]
    reps = res.representatives(3)
    # nearest first; windows 2 and 5 tie at 0.125 and 0 and 3 at 0.5: the lower window id first
    assert reps[0] == [("site/a", 1.92, 0.125), ("b", 199.68, 0.125), ("site/a", 0.0, 0.5)]
    assert reps[1] == [("site/a", 0.96, 0.25), ("b", 0.48, 0.75)] and reps[2] == []
    assert [len(r) for r in res.representatives(1)] == [1, 1, 0] and len(res.representatives()[0]) == 4
    with pytest.raises(ValueError):
        cluster.ClusterResult([0, 1], [0.5], [1, 1], ["a"], [0, 0], [0.0, 0.96])


def test_result_annotations_read_back(tmp_path):
    res = result()
    path = str(tmp_path / "first.csv")
    rows = res.annotations({0: "ins_buzz", 1: "ambient"}, path=path)
    assert rows == [("site/a", 0.0, 0.96, "ins_buzz"), ("site/a", 0.96, 1.92, "ambient"), ("site/a", 1.92, 2.88, "ins_buzz"),
                    ("b", 0.0, 0.96, "ins_buzz"), ("b", 0.48, 1.44, "ambient"), ("b", 199.68, 200.64, "ins_buzz")]
    back = dataset.read_annotations(path)
    assert sorted((i, a, b, l) for i, v in back.items() for a, b, l in v) == sorted(rows)
    assert res.annotations({0: "ins_buzz"}, max_distance=0.125) == [("site/a", 1.92, 2.88, "ins_buzz"), ("b", 199.68, 200.64, "ins_buzz")]
    assert res.annotations({1: "x"}, max_distance=0.5) == [("site/a", 0.96, 1.92, "x")]
    assert res.annotations({}) == []
    with pytest.raises(ValueError):
        res.annotations({3: "nothing"})


def test_save_and_load_round_trip(tmp_path):
    res = result()
    path = str(tmp_path / "centres.npz")
    res.save(path)
    model = cluster.load(path)
    assert model.metric == "euclidean" and model.counts.tolist() == [4, 2, 0] and model.counts.dtype == np.int64
    assert model.centroids.dtype == np.float32 and model.centroids.tobytes() == res.centroids.tobytes()
    km = cluster.KMeans.from_model(model)
    assert km.n_clusters == 3 and km.metric == "euclidean" and km.centroids.tobytes() == res.centroids.tobytes()
    again = str(tmp_path / "again.npz")
    km.model().save(again)
    assert cluster.load(again).centroids.tobytes() == res.centroids.tobytes()
    with pytest.raises(RuntimeError):
        cluster.ClusterResult([0], [0.5], [1], ["a"], [0], [0.0]).save(path)


# ---------------------------------------------------------------------------------------------------- k-means++
def test_the_draw_sequence_of_a_seed():
    """One rng.random() a draw against the float64 cumulative sum; rows that weigh nothing are never drawn."""
    d = np.array([0.0, 3.0, np.nan, 1.0, np.inf, 0.0, 4.0, -1.0, 2.0], np.float32)
    weights = np.array([0.0, 3.0, 0.0, 1.0, 0.0, 0.0, 4.0, 0.0, 2.0])
    rng, twin = np.random.default_rng(11), np.random.default_rng(11)
    got = [cluster.kmeanspp_draw(rng, d) for _ in range(200)]
    cum = np.cumsum(weights)
    want = [int(np.searchsorted(cum, twin.random() * cum[-1], side="right")) for _ in range(200)]
    assert got == want and set(got) == {1, 3, 6, 8}
    share = np.bincount(got, minlength=9) / 200.0
    assert abs(share[6] - 0.4) < 0.1 and abs(share[1] - 0.3) < 0.1
    # nothing weighs anything: uniform over all rows, by rng.integers
    rng, twin = np.random.default_rng(5), np.random.default_rng(5)
    assert [cluster.kmeanspp_draw(rng, np.zeros(7)) for _ in range(20)] == [int(twin.integers(7)) for _ in range(20)]
    assert cluster.kmeanspp_draw(np.random.default_rng(0), [0.0, 0.0, 5.0]) == 2


def test_plus_plus_recovers_the_planted_partition_in_numpy():
    """The draw of KMeans(init="k-means++", seed=0) on the (1025, 5) fixture, restated in float64 NumPy: the five chosen rows
    come from five different clusters, for both metrics (what tests/test_cluster_gpu.py then expects of the device)."""
    e, truth = cases.fixture(1025, 5)
    for metric in METRICS:
        rng = np.random.default_rng(0)
        chosen = [int(rng.integers(1025))]
        nearest = None
        for _ in range(4):
            c = cluster.normalise_centroids(e[chosen[-1]:chosen[-1] + 1], metric)
            t, n2 = cases.candidates64(e, c, metric)
            d = cases.distance64(t[:, 0], n2, metric)
            nearest = d if nearest is None else np.minimum(nearest, d)
            chosen.append(cluster.kmeanspp_draw(rng, nearest.astype(np.float32)))
        print(metric, chosen, truth[chosen])
        assert sorted(truth[chosen].tolist()) == [0, 1, 2, 3, 4]
