"""k-means clustering on the GPU (csrc/cluster.hip, buzzdetect_amd/cluster.py): assign against the device's own bd_search_scores
in every bit (the matrix chain is restated on the host nowhere) and against float64 on the planted fixture, the order, the
centroids and the statistics against their host restatements in every bit, KMeans.fit on the fixture, and cluster_recordings /
assign_recordings against KMeans over engine.embed of the same chunks.  Every buffer a kernel writes comes from
tests/gpu_guards.Guarded: the guard words must stay untouched and every output element must be written."""
import os
import wave

import numpy as np
import pytest

from buzzdetect_amd import _lib, cluster, dataset as D, framing, search
from tests import cluster_cases as cases

pytestmark = pytest.mark.gpu

METRICS = ("euclidean", "cosine")
FLOOR = np.float32(_lib.SEARCH_NORM_FLOOR)


def guarded():
    from tests.gpu_guards import Guarded
    return Guarded("cuda")


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def corpus():
    """The (1025, 65) fixture's rows on both sides; cases with fewer rows or clusters take its first ones."""
    import torch
    assert torch.cuda.is_available()
    e, truth = cases.fixture(1025, 65)
    return e, truth, upload(e)


class Centres:
    """A centroid set as assign takes it: normalised on the host, packed, with its squared norms, uploaded."""

    def __init__(self, rows, metric, normalise=True):
        self.metric = metric
        self.rows = cluster.normalise_centroids(rows, metric) if normalise else np.ascontiguousarray(rows, np.float32)
        self.k = self.rows.shape[0]
        self.c2 = search.norms_host(self.rows)
        self.packed_dev, self.c2_dev = upload(search.pack_queries(self.rows)), upload(self.c2)


def dev_norms(g, e_dev):
    import torch
    w = int(e_dev.shape[0])
    n2 = g.empty((w,), torch.float32, name="n2")
    for at in range(0, w, _lib.SEARCH_MAX_WINDOWS):                      # bd_search_norms takes 2^20 rows a call
        n = min(_lib.SEARCH_MAX_WINDOWS, w - at)
        _lib.check(_lib.load().bd_search_norms(e_dev[at:at + n].data_ptr(), n, n2[at:at + n].data_ptr(), stream()))
    return n2


def dev_assign(g, e_dev, c):
    """(labels, dist, n2) as NumPy, from guarded buffers."""
    import torch
    w = int(e_dev.shape[0])
    n2 = dev_norms(g, e_dev)
    labels, dist = g.empty((w,), torch.int32, name="labels"), g.empty((w,), torch.float32, name="dist")
    _lib.check(_lib.load().bd_cluster_assign(e_dev.data_ptr(), w, n2.data_ptr(), c.packed_dev.data_ptr(), c.c2_dev.data_ptr(), c.k,
                                             _lib.CLUSTER_METRICS[c.metric], labels.data_ptr(), dist.data_ptr(), stream()))
    out = labels.cpu().numpy(), dist.cpu().numpy(), n2.cpu().numpy()
    g.check()
    return out


def dev_scores(g, e_dev, c):
    """S = bd_search_scores(BD_SEARCH_DOT) of the same rows and the same packed centroids, [W, K]."""
    import torch
    w = int(e_dev.shape[0])
    s = g.empty((w, c.k), torch.float32, name="scores")
    _lib.check(_lib.load().bd_search_scores(e_dev.data_ptr(), w, c.packed_dev.data_ptr(), c.k, _lib.SEARCH_METRICS["dot"], None,
                                            s.data_ptr(), c.k, 1, stream()))
    out = s.cpu().numpy()
    g.check()
    return out


def expected_from_scores(s, n2, c):
    """The header's formulas in float32 NumPy on the device's score bits: (labels, dist)."""
    assert s.dtype == np.float32 and n2.dtype == np.float32
    t = c.c2[None, :] - np.float32(2.0) * s if c.metric == "euclidean" else -s
    t = np.where(np.isnan(t), np.float32(np.inf), t).astype(np.float32)
    labels = t.argmin(axis=1).astype(np.int32)                           # the first of equal minima: the lower j
    best = t[np.arange(t.shape[0]), labels]
    with np.errstate(invalid="ignore", divide="ignore"):
        if c.metric == "euclidean":
            dist = np.fmax(n2 + best, np.float32(0.0))
        else:
            dist = np.where(n2 < FLOOR, np.float32(1.0), np.float32(1.0) - (-best) / np.sqrt(n2))
    return labels, dist.astype(np.float32)


# ---------------------------------------------------------------------------------------------------- assign
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", (1, 2, 31, 32, 33, 65))
@pytest.mark.parametrize("w", (1, 31, 32, 33, 257, 1025))
def test_assign_is_the_argmin_of_the_search_scores_in_every_bit(corpus, w, k, metric):
    """Centroids are rows 500 .. 500 + k of the corpus (random rows: many near ties), one row is zero and one is tiny."""
    e, _, e_dev = corpus
    rows = e_dev[:w].clone()
    if w > 4:
        rows[4] = 0.0
        rows[2] *= 1e-19                                                 # below the norm floor
    g = guarded()
    c = Centres(e[500:500 + k], metric)
    labels, dist, n2 = dev_assign(g, rows, c)
    want_l, want_d = expected_from_scores(dev_scores(g, rows, c), n2, c)
    assert labels.tolist() == want_l.tolist()
    assert dist.tobytes() == want_d.tobytes()
    assert labels.min() >= 0 and labels.max() < k
    if w > 4 and metric == "cosine":
        assert dist[4] == 1.0 and dist[2] == 1.0
    if w > 4 and metric == "euclidean":
        assert dist[4] == c.c2[labels[4]] and labels[4] == int(np.argmin(c.c2))


@pytest.mark.parametrize("metric", METRICS)
def test_ties_go_to_the_lower_centroid_and_nan_never_wins(corpus, metric):
    import torch
    e, truth, e_dev = corpus
    g = guarded()
    same = Centres(np.repeat(e[7:8], 3, axis=0), metric)                 # three identical centroids: every candidate ties
    labels, dist, _ = dev_assign(g, e_dev[:257].contiguous(), same)
    assert (labels == 0).all()
    rows = e[:40].copy()
    rows[[33, 35]] = rows[[1, 2]]                                        # centroids 33 and 35 repeat 1 and 2, far behind them
    twins = Centres(rows[:40], metric)
    labels, dist, n2 = dev_assign(g, e_dev, twins)
    assert not np.isin(labels, (33, 35)).any() and (labels == 1).any() and (labels == 2).any()
    want_l, want_d = expected_from_scores(dev_scores(g, e_dev, twins), n2, twins)
    assert labels.tolist() == want_l.tolist() and dist.tobytes() == want_d.tobytes()
    # a NaN row: every candidate is +INFINITY, the label is 0; a NaN centroid is never anybody's nearest
    bad = e_dev[:65].clone()
    bad[5, 100] = float("nan")
    cent = e[:3].copy()
    cent[1, 3] = np.nan
    c = Centres(cent, metric, normalise=False)
    labels, dist, n2 = dev_assign(g, bad, c)
    assert labels[5] == 0 and not (labels == 1).any() and set(labels.tolist()) == {0, 2}
    assert np.isnan(n2[5]) and (dist[5] == 0.0 if metric == "euclidean" else np.isnan(dist[5]))
    keep = np.arange(65) != 5
    want_l, want_d = expected_from_scores(dev_scores(g, bad, c), n2, c)
    assert labels.tolist() == want_l.tolist() and dist[keep].tobytes() == want_d[keep].tobytes()
    assert torch.cuda.is_available()


@pytest.mark.parametrize("metric", METRICS)
def test_a_row_is_assigned_the_same_wherever_it_sits_and_whatever_follows_its_centroid(corpus, metric):
    e, truth, e_dev = corpus
    g = guarded()
    c = Centres(e[:33], metric)
    labels, dist, _ = dev_assign(g, e_dev, c)
    for w in (1, 33, 200):
        alone_l, alone_d, _ = dev_assign(g, e_dev[3:3 + w].contiguous(), c)
        assert alone_l.tolist() == labels[3:3 + w].tolist() and alone_d.tobytes() == dist[3:3 + w].tobytes(), w
    perm = np.concatenate([[0], 1 + np.random.default_rng(1).permutation(32)])      # centroid 0 stays, the others move
    moved = Centres(c.rows[perm], metric, normalise=False)
    moved_l, moved_d, _ = dev_assign(g, e_dev, moved)
    assert perm[moved_l].tolist() == labels.tolist() and moved_d.tobytes() == dist.tobytes()
    assert (labels == truth % 33).sum() > 0 and len(set(labels.tolist())) == 33


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("w,k", cases.FIXTURES)
def test_assign_against_float64_on_the_planted_fixture(w, k, metric):
    """Every row's label is the float64 label (tests/test_cluster_host.py shows the margins that make this fair), and the
    distances obey DESIGN §15: the device's largest deviation from float64 is at most 8 x that of the plain float32 NumPy
    restatement (E @ C.T, then the header's formula), whose deviation is counted as at least 1e-7 max(n2 + c2) for the
    Euclidean distance - float32's epsilon on the operands that cancel - and, for the cosine distance, whose cancelling
    operands are 1 and a cosine, as at least 1e-7.  Measured on an MI355X: ratios 1.74 - 3.01, and 5.57 / 5.24 for K = 1 (NumPy
    takes a single column by a more accurate vector dot); the table is in DESIGN §23."""
    e, truth = cases.fixture(w, k)
    g = guarded()
    c = Centres(e[:k], metric)
    labels, dist, n2 = dev_assign(g, upload(e), c)
    t64, n64 = cases.candidates64(e, c.rows, metric)
    assert labels.tolist() == t64.argmin(axis=1).tolist() == truth.tolist()
    want = cases.distance64(t64.min(axis=1), n64, metric)
    s32 = e @ c.rows.T
    n32 = (e * e).sum(axis=1, dtype=np.float32)
    c32 = (c.rows * c.rows).sum(axis=1, dtype=np.float32)
    t32 = c32[None, :] - np.float32(2.0) * s32 if metric == "euclidean" else -s32
    plain = (np.maximum(n32 + t32.min(axis=1), np.float32(0.0)) if metric == "euclidean"
             else np.float32(1.0) - (-t32.min(axis=1)) / np.sqrt(n32))
    assert plain.dtype == np.float32
    floor = 1e-7 * (n64.max() + (c.rows.astype(np.float64) ** 2).sum(axis=1).max()) if metric == "euclidean" else 1e-7
    dev = np.abs(dist.astype(np.float64) - want).max()
    ref = max(np.abs(plain.astype(np.float64) - want).max(), floor)
    print(f"({w}, {k}) {metric}: device deviation {dev:.3e}, float32 NumPy deviation {ref:.3e}, ratio {dev / ref:.2f}")
    assert dev <= 8.0 * ref


# ---------------------------------------------------------------------------------------------------- order, centroids, stats
def dev_update(g, e_dev, n2_dev, labels, prev, metric):
    """bd_cluster_order and bd_cluster_centroids on guarded buffers, the workspace exactly as large as asked for and poisoned
    with NaNs.  Returns (order, offsets, centroids, packed, c2) as NumPy."""
    import torch
    from tests.gpu_guards import NAN
    lib = _lib.load()
    w, k = int(e_dev.shape[0]), prev.shape[0]
    labels_dev, prev_dev = upload(labels), upload(prev)
    order, offsets = g.empty((w,), torch.int32, name="order"), g.empty((k + 1,), torch.int32, name="offsets")
    ws_bytes = _lib.check(lib.bd_cluster_workspace_bytes(w, k))
    ws = g.empty((ws_bytes,), torch.uint8, fill=NAN, name="workspace")
    _lib.check(lib.bd_cluster_order(labels_dev.data_ptr(), w, k, order.data_ptr(), offsets.data_ptr(), ws.data_ptr(), ws_bytes,
                                    stream()))
    cent = g.empty((k, 1024), torch.float32, name="centroids")
    packed = g.empty((_lib.check(lib.bd_search_packed_floats(k)),), torch.float32, name="packed")
    c2 = g.empty((k,), torch.float32, name="c2")
    _lib.check(lib.bd_cluster_centroids(e_dev.data_ptr(), w, n2_dev.data_ptr(), order.data_ptr(), offsets.data_ptr(), k,
                                        _lib.CLUSTER_METRICS[metric], prev_dev.data_ptr(), cent.data_ptr(), packed.data_ptr(),
                                        c2.data_ptr(), ws.data_ptr(), ws_bytes, stream()))
    out = tuple(t.cpu().numpy() for t in (order, offsets, cent, packed, c2))
    g.check()
    return out


def check_update(e, labels, prev, metric):
    g = guarded()
    e_dev = upload(e)
    n2_dev = dev_norms(g, e_dev)
    n2 = n2_dev.cpu().numpy()
    order, offsets, cent, packed, c2 = dev_update(g, e_dev, n2_dev, labels, prev, metric)
    want_order, want_offsets = cluster.order_host(labels, prev.shape[0])
    assert order.tolist() == want_order.tolist() and offsets.tolist() == want_offsets.tolist()
    want_cent, want_packed, want_c2 = cluster.centroids_host(e, n2, want_order, want_offsets, metric, prev)
    assert cent.tobytes() == want_cent.tobytes()
    assert packed.tobytes() == want_packed.tobytes() == search.pack_queries(cent).tobytes()
    assert c2.tobytes() == want_c2.tobytes() == search.norms_host(cent).tobytes()
    return cent, offsets


@pytest.mark.parametrize("metric", METRICS)
def test_order_and_centroids_of_constructed_labels_are_the_host_restatements(metric):
    e, labels, prev, zero = cases.constructed()
    prev = cluster.normalise_centroids(prev, metric)
    cent, offsets = check_update(e, labels, prev, metric)
    assert np.diff(offsets).tolist() == list(cases.SIZES) and cent[0].tobytes() == prev[0].tobytes()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("w,k", ((1025, 33), (4099, 65), (33, 32)))
def test_order_centroids_and_stats_of_a_real_assign_are_the_host_restatements(w, k, metric):
    """(4099, 65): five slices of the order's 1024 rows, the last one of three rows; centroids from random rows leave clusters
    of every size, usually an empty one."""
    import torch
    rng = np.random.default_rng(w)
    e = cases.fixture(1025, 65)[0][rng.integers(0, 1025, size=w)] if w > 1025 else cases.fixture(w, k)[0]
    e = np.ascontiguousarray(e + (0.01 * rng.normal(size=e.shape)).astype(np.float32))
    g = guarded()
    c = Centres(e[rng.integers(0, w, size=k)], metric)
    labels, dist, n2 = dev_assign(g, upload(e), c)
    check_update(e, labels, c.rows, metric)
    prev = labels.copy()
    prev[::3] = (prev[::3] + 1) % k
    slices = (w + 255) // 256
    partial, changed = g.empty((slices,), torch.float32, name="partial"), g.empty((slices,), torch.int32, name="changed")
    dist_dev, labels_dev, prev_dev = upload(dist), upload(labels), upload(prev)
    _lib.check(_lib.load().bd_cluster_stats(dist_dev.data_ptr(), labels_dev.data_ptr(), prev_dev.data_ptr(), w,
                                            partial.data_ptr(), changed.data_ptr(), stream()))
    got_p, got_c = partial.cpu().numpy(), changed.cpu().numpy()
    g.check()
    want_p, want_c = cluster.stats_host(dist, labels, prev)
    assert got_p.tobytes() == want_p.tobytes() and got_c.tolist() == want_c.tolist()
    assert got_c.sum() == (labels != prev).sum() and (k == 1 or got_c.sum() > 0)


@pytest.mark.parametrize("metric", METRICS)
def test_rows_whose_element_offsets_pass_2_to_the_31(metric):
    """W * 1024 passes 2^31 from 2 097 152 rows on (8 GB of rows; the project has fixed a 32-bit wrap before).  2^21 zero rows,
    then 300 rows of the fixture: the tail is assigned as it is alone, ordered behind the zero rows, and its clusters' centroids
    are the host restatement's over the tail alone (the same members in the same order)."""
    import torch
    tail_rows = 300
    w = (1 << 21) + tail_rows
    e, truth = cases.fixture(1025, 5)
    tail = np.ascontiguousarray(e[:tail_rows])
    big = torch.zeros((w, 1024), dtype=torch.float32, device="cuda")
    big[w - tail_rows:] = upload(tail)
    g = guarded()
    c = Centres(e[:5], metric)
    labels, dist, n2 = dev_assign(g, big, c)
    alone_l, alone_d, _ = dev_assign(g, upload(tail), c)
    assert labels[-tail_rows:].tolist() == alone_l.tolist() == truth[:tail_rows].tolist()
    assert dist[-tail_rows:].tobytes() == alone_d.tobytes()
    assert (labels[:-tail_rows] == labels[0]).all() and (dist[:-tail_rows] == dist[0]).all()
    # the zero rows in cluster 0, the tail in clusters 1 .. 4
    tail_labels = (1 + truth[:tail_rows] % 4).astype(np.int32)
    made = np.concatenate([np.zeros(1 << 21, np.int32), tail_labels])
    order, offsets, cent, packed, c2 = dev_update(g, big, upload(n2), made, c.rows, metric)
    want_order, want_offsets = cluster.order_host(tail_labels, 5)
    assert offsets.tolist() == [0] + ((1 << 21) + want_offsets[1:]).tolist()
    assert (order[:1 << 21] == np.arange(1 << 21)).all() and order[1 << 21:].tolist() == ((1 << 21) + want_order).tolist()
    want_cent, _, want_c2 = cluster.centroids_host(tail, search.norms_host(tail), want_order, want_offsets, metric, c.rows)
    assert cent[1:].tobytes() == want_cent[1:].tobytes() and c2[1:].tobytes() == want_c2[1:].tobytes()
    # 2^21 zero rows: their mean is zero, and a cosine sum without direction keeps the previous centroid
    assert cent[0].tobytes() == (np.zeros(1024, np.float32) if metric == "euclidean" else c.rows[0]).tobytes()
    assert packed.tobytes() == search.pack_queries(cent).tobytes() and c2.tobytes() == search.norms_host(cent).tobytes()


# ---------------------------------------------------------------------------------------------------- KMeans
class GuardedKMeans(cluster.KMeans):
    """Every buffer of a fit between guard words; the workspace is poisoned and need not be written whole."""
    guards = None

    def _empty(self, shape, dtype):
        import torch
        from tests.gpu_guards import NAN, SENTINEL, Guarded
        if GuardedKMeans.guards is None:
            GuardedKMeans.guards = Guarded("cuda")
        scratch = dtype == torch.uint8
        return self.guards.empty(shape, dtype, fill=NAN if scratch else SENTINEL, name=f"{tuple(shape)} {dtype}")


def same_fit(a, b):
    return (a.centroids.tobytes() == b.centroids.tobytes() and a.labels.tobytes() == b.labels.tobytes()
            and a.distances.tobytes() == b.distances.tobytes() and a.inertia_history == b.inertia_history)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("w,k", cases.FIXTURES)
def test_fit_recovers_the_planted_partition_in_two_iterations(w, k, metric):
    e, truth = cases.fixture(w, k)
    e_dev = upload(e)
    km = GuardedKMeans(k, metric=metric, init=e[:k]).fit(e_dev)
    GuardedKMeans.guards.check()
    assert km.labels.tolist() == truth.tolist() and km.n_iter == 2 and len(km.inertia_history) == 2
    assert km.inertia_history[1] <= km.inertia_history[0]
    assert km.counts.tolist() == np.bincount(truth, minlength=k).tolist()
    assert abs(km.inertia_history[1] - km.distances.astype(np.float64).sum()) <= 1e-6 * km.inertia_history[1]
    again = GuardedKMeans(k, metric=metric, init=e[:k]).fit(e)             # from the host array: the same bits
    GuardedKMeans.guards.check()
    assert same_fit(km, again)
    labels, distances = km.assign(e_dev)
    GuardedKMeans.guards.check()
    assert labels.tobytes() == km.labels.tobytes() and distances.tobytes() == km.distances.tobytes()
    # the centroids are the host restatement's over the final partition, from the first ones
    order, offsets = cluster.order_host(truth.astype(np.int32), k)
    first = cluster.normalise_centroids(e[:k], metric)
    want, _, _ = cluster.centroids_host(e, search.norms_host(e), order, offsets, metric, first)
    assert km.centroids.tobytes() == want.tobytes()


@pytest.mark.parametrize("metric", METRICS)
def test_plus_plus_and_restarts_on_the_planted_fixture(metric):
    """Seed 0 draws one row of every planted cluster (tests/test_cluster_host.py restates the draw in NumPy), so the partition
    is recovered: purity 1.0.  n_init = 3 is the best of seeds 0, 1, 2."""
    e, truth = cases.fixture(1025, 5)
    e_dev = upload(e)
    km = GuardedKMeans(5, metric=metric, seed=0).fit(e_dev)
    GuardedKMeans.guards.check(written=False)
    purity = sum(np.bincount(truth[km.labels == c], minlength=5).max() for c in range(5)) / 1025.0
    assert purity == 1.0 and sorted(km.counts.tolist()) == sorted(np.bincount(truth).tolist())
    assert all(a >= b for a, b in zip(km.inertia_history, km.inertia_history[1:])) and km.n_iter >= 2
    assert same_fit(km, GuardedKMeans(5, metric=metric, seed=0).fit(e_dev))
    singles = [km] + [GuardedKMeans(5, metric=metric, seed=s, init_rows=300).fit(e_dev) for s in (1, 2)]
    singles[0] = GuardedKMeans(5, metric=metric, seed=0, init_rows=300).fit(e_dev)       # a subsample of 300 of the 1025 rows
    best = min(singles, key=lambda m: m.inertia_history[-1])
    three = GuardedKMeans(5, metric=metric, seed=0, init_rows=300, n_init=3).fit(e_dev)
    GuardedKMeans.guards.check(written=False)
    assert three.inertia_history[-1] == min(m.inertia_history[-1] for m in singles)
    assert three.labels.tobytes() == best.labels.tobytes() and three.centroids.tobytes() == best.centroids.tobytes()
    one = GuardedKMeans(5, metric=metric, max_iter=1, init=e[:5]).fit(e_dev)             # one iteration: labels of the first centres
    GuardedKMeans.guards.check(written=False)
    assert one.n_iter == 1 and one.labels.tolist() == truth.tolist()
    assert one.centroids.tobytes() == cluster.normalise_centroids(e[:5], metric).tobytes()


# ---------------------------------------------------------------------------------------------------- end to end
W16 = D.WINDOW_SAMPLES
CHUNK = 4.8                       # five windows per chunk


def write_wav(path, pcm16, rate):
    pcm16 = np.asarray(pcm16, "<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if pcm16.ndim == 1 else pcm16.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm16.tobytes())


def to_s16(x):
    return (np.clip(x, -1, 1 - 2 ** -15) * 32768.0).round().astype(np.int16)


@pytest.fixture(scope="module")
def folder(tmp_path_factory, engine):
    """Three recordings of about ten windows (16 kHz mono, 44.1 kHz stereo, 16 kHz mono) and, per hop (whole and half), every
    chunk as analyze cuts it - at 16 kHz mono on the device, in the order the recordings are walked - with the (ident, start)
    analyze writes for each of its windows."""
    import pandas as pd
    from buzzdetect_amd.analyze import analyze
    from buzzdetect_amd.engine import hop_samples, patch_step
    from oracle import yamnet_oracle as O
    root = tmp_path_factory.mktemp("cluster")
    audio = root / "audio"
    (audio / "site").mkdir(parents=True)
    a = to_s16(O.synthetic_audio(10 * W16 + 3000, seed=21))
    left = O.synthetic_audio(int(44100 * 9.7), seed=22)
    b = to_s16(np.stack([left, 0.5 * np.roll(left, 441)], axis=1))
    c = to_s16(O.synthetic_audio(9 * W16 + 8000, seed=23))
    write_wav(audio / "a.wav", a, 16000)
    write_wav(audio / "site" / "b.wav", b, 44100)
    write_wav(audio / "c.wav", c, 16000)
    pcm = {"a": (a, 16000), "site/b": (b, 44100), "c": (c, 16000)}
    order = [ident for _, ident in D._recordings(str(audio), {}, False, [])]
    assert sorted(order) == sorted(pcm)
    per_hop = {}
    for prop in (1.0, 0.5):
        out = root / f"out{prop}"
        rep = analyze("model_general_v3", chunklength=CHUNK, dir_audio=str(audio), dir_out=str(out), engine=engine,
                      framehop_prop=prop)
        assert rep.files_done == 3
        hop_s = 0.96 * prop
        chunks, where = [], []
        for ident in order:
            x, rate = pcm[ident]
            starts = np.sort(pd.read_csv(os.path.join(out, ident + "_buzzdetect.csv"))["start"].to_numpy())
            at = 0
            for edge in framing.gaps_to_chunklist([(0, x.shape[0] / rate)], framing.round_chunklength(CHUNK)):
                lo, hi = framing.chunk_sample_range(edge, rate)
                hi = min(hi, x.shape[0])
                if hi <= lo:
                    continue
                part = x[lo:hi]
                dev = engine.resample(part, rate, 16000) if rate != 16000 else engine.to_device(part.astype(np.float32) / 32768.0)
                n = engine.num_windows(int(dev.numel()), hop_samples(hop_s), patch_step(hop_s))
                chunks.append(dev)
                where += [(ident, float(s)) for s in starts[at:at + n]]
                at += n
            assert at == starts.size
        per_hop[prop] = (chunks, where)
    return str(audio), per_hop


@pytest.mark.parametrize("prop", (1.0, 0.5))
def test_cluster_recordings_is_kmeans_over_engine_embed(engine, folder, monkeypatch, tmp_path, prop):
    import torch
    dir_audio, per_hop = folder
    chunks, where = per_hop[prop]
    monkeypatch.setattr(cluster, "KMeans", GuardedKMeans)
    rows = torch.cat([engine.embed(c, 0.96 * prop).device_tensor() for c in chunks]).contiguous()
    assert rows.shape[0] == len(where) and (25 <= len(where) <= 35 if prop == 1.0 else 50 <= len(where) <= 70)
    for metric in METRICS:
        got = cluster.cluster_recordings(dir_audio, 3, metric=metric, engine=engine, chunklength=CHUNK, framehop_prop=prop, seed=4)
        ref = GuardedKMeans(3, metric=metric, seed=4, device=engine.device).fit(rows)
        GuardedKMeans.guards.check(written=False)
        assert got.messages == [] and got.metric == metric
        assert got.labels.tobytes() == ref.labels.tobytes() and got.distances.tobytes() == ref.distances.tobytes()
        assert got.centroids.tobytes() == ref.centroids.tobytes() and got.counts.tolist() == ref.counts.tolist()
        assert [(got.recordings[r], float(s)) for r, s in zip(got.recording_of, got.starts)] == where
        assert got.counts.sum() == len(where)
        reps = got.representatives(2)
        for c in range(3):
            mine = np.flatnonzero(ref.labels == c)
            if not mine.size:
                assert reps[c] == []
                continue
            first = mine[np.lexsort((mine, ref.distances[mine].astype(np.float64)))][0]
            assert reps[c][0] == (*where[first], float(ref.distances[first]))
        # saved centres label the folder again, streamed: the same labels and distances
        path = str(tmp_path / f"centres_{metric}.npz")
        got.save(path)
        again = cluster.assign_recordings(dir_audio, path, engine=engine, chunklength=CHUNK, framehop_prop=prop)
        GuardedKMeans.guards.check(written=False)
        assert again.labels.tobytes() == got.labels.tobytes() and again.distances.tobytes() == got.distances.tobytes()
        assert again.starts.tolist() == got.starts.tolist() and again.counts.tolist() == got.counts.tolist()
    with pytest.raises(ValueError, match=r"max_windows = 2 windows \(\d+ counted"):
        cluster.cluster_recordings(dir_audio, 2, engine=engine, chunklength=CHUNK, framehop_prop=prop, max_windows=2)
