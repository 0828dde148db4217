"""The neighbour lists on the GPU (csrc/knn.hip): bd_knn_update against its host restatement in every key and against NumPy
divisions of the device's own bd_search_scores dots, the invariances of the contract, rows past the 32-bit element offsets,
guarded and poisoned memory, and the lists against float64 on the planted fixture.  Every buffer the kernel writes comes from
tests/gpu_guards.Guarded."""
import numpy as np
import pytest

from buzzdetect_amd import _lib, propagate, search
from tests import cluster_cases, propagate_cases as cases

pytestmark = pytest.mark.gpu

METRICS = ("cosine", "dot")


def guarded():
    from tests.gpu_guards import Guarded
    return Guarded("cuda")


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_norms(e_dev):
    import torch
    w = int(e_dev.shape[0])
    n2 = torch.empty((w,), dtype=torch.float32, device="cuda")
    for at in range(0, w, _lib.SEARCH_MAX_WINDOWS):                      # bd_search_norms takes 2^20 rows a call
        n = min(_lib.SEARCH_MAX_WINDOWS, w - at)
        _lib.check(_lib.load().bd_search_norms(e_dev[at:at + n].data_ptr(), n, n2[at:at + n].data_ptr(), stream()))
    return n2


def dev_update(g, q_dev, c_dev, k, metric="cosine", exclude_self=False, q_base=0, c_base=0, keys=None, pattern=None, fill=None,
               n2=None):
    """One bd_knn_update with a guarded state and a guarded workspace of exactly the bytes the library asks for, prefilled with
    `pattern`.  `keys`: the state to go on from (a guarded tensor), else a new zero-filled one (`fill`: another first content).
    Returns the state (on the device)."""
    import torch
    from tests.gpu_guards import BACK, ZERO
    lib = _lib.load()
    wq, wc = int(q_dev.shape[0]), int(c_dev.shape[0])
    if keys is None:
        keys = g.empty((wq, k), torch.int64, fill=ZERO if fill is None else fill, name="keys")
    nbytes = _lib.check(lib.bd_knn_workspace_bytes(wq, wc))
    ws = g.empty((nbytes,), torch.uint8, fill=ZERO if pattern is None else pattern, back=BACK, name="workspace")
    n2_q, n2_c = n2 if n2 is not None else (dev_norms(q_dev), dev_norms(c_dev))
    _lib.check(lib.bd_knn_update(q_dev.data_ptr(), wq, n2_q.data_ptr(), q_base, c_dev.data_ptr(), wc, n2_c.data_ptr(), c_base,
                                 _lib.KNN_METRICS[metric], int(exclude_self), keys.data_ptr(), k, ws.data_ptr(), nbytes, stream()))
    return keys


def as_keys(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def corpus():
    """The (1025, 5) fixture's rows on both sides, and 1025 other rows (many near ties within a planted cluster)."""
    import torch
    assert torch.cuda.is_available()
    e, _ = cluster_cases.fixture(1025, 5)
    other = np.ascontiguousarray(e[::-1] * np.float32(0.5) + np.roll(e, 7, axis=0) * np.float32(0.5))
    return e, upload(e), other, upload(other)


# ---------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("wq,wc,k", ((1, 1, 1), (1, 1025, 64), (31, 33, 15), (32, 32, 16), (33, 31, 17), (127, 129, 63), (128, 128, 64),
                                     (129, 127, 16), (257, 1025, 64), (1025, 257, 1), (1025, 1025, 16), (1025, 1025, 17)))
def test_update_equals_the_host_restatement_in_every_key(corpus, wq, wc, k, metric):
    """The same array on both sides (with and without the row itself) and another array as candidates."""
    e, e_dev, other, other_dev = corpus
    g = guarded()
    for c, c_dev, exclude_self in ((e, e_dev, True), (e, e_dev, False), (other, other_dev, False)):
        got = as_keys(dev_update(g, e_dev[:wq], c_dev[:wc], k, metric, exclude_self))
        g.check(written=False)
        want = propagate.knn_update_host(np.zeros((wq, k), np.uint64), e[:wq], c[:wc], metric=metric, exclude_self=exclude_self)
        assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("metric", METRICS)
def test_sims_are_numpy_divisions_of_the_search_scores(corpus, metric):
    """dot(i, j) is what bd_search_scores(BD_SEARCH_DOT) stores for row i against query row j: the lists are the stable sort of
    float32 NumPy divisions of those bits."""
    import torch
    e, e_dev, _, _ = corpus
    wq, wc, k = 1025, 1024, 16
    g = guarded()
    packed = upload(search.pack_queries(e[:wc]))
    s = g.empty((wq, wc), torch.float32, name="scores")
    _lib.check(_lib.load().bd_search_scores(e_dev.data_ptr(), wq, packed.data_ptr(), wc, _lib.SEARCH_METRICS["dot"], None,
                                            s.data_ptr(), wc, 1, stream()))
    dots = s.cpu().numpy()
    assert dots[:wc].tobytes() == np.ascontiguousarray(dots[:wc].T).tobytes()                     # bit-symmetric
    if metric == "cosine":
        n2 = dev_norms(e_dev).cpu().numpy()
        den = np.sqrt(n2)[:, None] * np.sqrt(n2[:wc])[None, :]
        assert den.dtype == np.float32
        sims = dots / den
    else:
        sims = dots
    want = cases.knn_numpy(e, e[:wc], k, metric, True, s=sims)
    got = as_keys(dev_update(g, e_dev, e_dev[:wc], k, metric, True))
    g.check()
    assert got.tobytes() == want.tobytes()
    assert cases.dots(e[:3], e[:40]).tobytes() == dots[:3, :40].tobytes()                         # and the chain is the header's


@pytest.mark.parametrize("metric", METRICS)
def test_special_rows(metric):
    """Duplicates, a zero row, a NaN row, a row below the norm floor, fewer candidates than k, ids up to the last one."""
    rows = cases.special_rows(257)
    rows_dev = upload(rows)
    g = guarded()
    for wc, k, exclude_self in ((257, 16, True), (257, 64, False), (9, 16, True), (9, 16, False)):
        got = as_keys(dev_update(g, rows_dev, rows_dev[:wc], k, metric, exclude_self))
        want = propagate.knn_update_host(np.zeros((257, k), np.uint64), rows, rows[:wc], metric=metric, exclude_self=exclude_self)
        assert got.tobytes() == want.tobytes()
        assert ((got != 0).sum(axis=1) == np.minimum(k, wc - (exclude_self & (np.arange(257) < wc)))).all()
    last = 0xFFFFFFFF
    got = as_keys(dev_update(g, rows_dev[:33], rows_dev[:129], 16, metric, True, q_base=last - 33, c_base=last - 129))
    want = propagate.knn_update_host(np.zeros((33, 16), np.uint64), rows[:33], rows[:129], metric=metric, exclude_self=True,
                                     q_base_id=last - 33, c_base_id=last - 129)
    g.check(written=False)
    assert got.tobytes() == want.tobytes() and (got != 0).all()


# ---------------------------------------------------------------------------------------------------- invariances
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("block", (1, 100, 128))
def test_one_call_equals_the_candidates_split_into_blocks_in_any_order(corpus, block, metric):
    e, e_dev, _, _ = corpus
    wq, wc, k = 300, 300 if block == 1 else 1025, 16
    g = guarded()
    whole = as_keys(dev_update(g, e_dev[:wq], e_dev[:wc], k, metric, True))
    n2 = dev_norms(e_dev)
    keys = None
    for a in np.random.default_rng(block).permutation(np.arange(0, wc, block)):
        b = min(int(a) + block, wc)
        keys = dev_update(g, e_dev[:wq], e_dev[a:b], k, metric, True, c_base=int(a), keys=keys, n2=(n2[:wq], n2[a:b]))
    g.check(written=False)
    assert as_keys(keys).tobytes() == whole.tobytes()


@pytest.mark.parametrize("metric", METRICS)
def test_a_row_keeps_its_list_elsewhere_and_sims_are_symmetric(corpus, metric):
    e, e_dev, _, _ = corpus
    k = 16
    g = guarded()
    whole = as_keys(dev_update(g, e_dev, e_dev, k, metric, True))
    moved = as_keys(dev_update(g, e_dev[700:763].contiguous(), e_dev, k, metric, True, q_base=700))     # another place, other company
    shuffled = np.random.default_rng(1).permutation(1025)[:200]
    picked = as_keys(dev_update(g, e_dev[upload(shuffled)].contiguous(), e_dev, k, metric, False))
    g.check()
    assert moved.tobytes() == whole[700:763].tobytes()
    with_self = as_keys(dev_update(g, e_dev, e_dev, k, metric, False))
    assert picked.tobytes() == with_self[shuffled].tobytes()
    ids, sims = propagate.decode_keys(whole)
    both = 0
    for i in range(1025):
        for slot, j in enumerate(ids[i]):
            back = np.flatnonzero(ids[j] == i)
            if back.size:
                both += 1
                assert cases.bits(sims[i, slot]) == cases.bits(sims[j, back[0]])
    assert both > 1000                                                   # (not vacuous: with dot products hubs take many lists)


def test_rows_whose_element_offsets_pass_2_to_the_31():
    """W * 1024 passes 2^31 from 2 097 152 rows on (8 GB of rows).  2^21 zero rows, then 300 rows of the fixture: as candidates
    and as queries the tail gives the lists it gives alone, with its ids moved by 2^21."""
    import torch
    tail_rows, front, k = 300, 1 << 21, 4
    e, _ = cluster_cases.fixture(1025, 5)
    tail = np.ascontiguousarray(e[:tail_rows])
    big = torch.zeros((front + tail_rows, 1024), dtype=torch.float32, device="cuda")
    big[front:] = upload(tail)
    g = guarded()
    alone = as_keys(dev_update(g, upload(tail), upload(tail), k, "cosine", True, q_base=front, c_base=front))
    n2 = dev_norms(big)
    # every row as a candidate (the zero rows have similarity 0 with everything, the tail's neighbours more)
    got = as_keys(dev_update(g, big[front:], big, k, "cosine", True, q_base=front, n2=(n2[front:], n2)))
    assert got.tobytes() == alone.tobytes()
    # every row as a query
    got = as_keys(dev_update(g, big, big[front:], k, "cosine", True, c_base=front, n2=(n2, n2[front:])))
    g.check()
    assert got[front:].tobytes() == alone.tobytes()
    zero_row = cases.make_keys(np.zeros(k, np.float32), front + np.arange(k))     # all ties at 0: the lowest ids
    assert (got[:front] == zero_row[None, :]).all()


# ---------------------------------------------------------------------------------------------------- memory hygiene
@pytest.mark.parametrize("metric", METRICS)
def test_nothing_outside_is_touched_and_the_workspace_content_does_not_matter(corpus, metric):
    """A state prefilled with the sentinel is k equal keys of a tiny negative similarity: every slot of it is beaten by the
    candidates here (all similarities are positive), so every word of the state must have been written."""
    from tests.gpu_guards import PATTERNS, SENTINEL
    e, e_dev, other, other_dev = corpus
    want = None
    for pattern in PATTERNS:
        g = guarded()
        got = [as_keys(dev_update(g, e_dev[:wq], other_dev[:wc], k, metric, False, pattern=pattern, fill=SENTINEL))
               for wq, wc, k in ((129, 257, 16), (1025, 130, 64), (33, 1025, 1))]
        g.check(written=True)
        want = got if want is None else want
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    fresh = propagate.knn_update_host(np.zeros((129, 16), np.uint64), e[:129], other[:257], metric=metric)
    assert want[0].tobytes() == fresh.tobytes()


# ---------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("clusters", (5, 33))
def test_neighbours_against_float64(clusters):
    """Near ties make the float32 and the float64 neighbour sets differ legitimately, so: every neighbour the device lists has
    a float64 similarity of at least the float64 k-th best of its row minus eps, eps = 8 x the largest difference between a
    float32 NumPy similarity and the float64 one (the yardstick is NumPy's float32, not the code under test)."""
    e, _ = cluster_cases.fixture(1025, clusters)
    k = 16
    g = guarded()
    e_dev = upload(e)
    ids, sims = propagate.decode_keys(as_keys(dev_update(g, e_dev, e_dev, k, "cosine", True)))
    g.check(written=False)
    e64 = e.astype(np.float64)
    n64 = np.sqrt((e64 * e64).sum(axis=1))
    s64 = (e64 @ e64.T) / (n64[:, None] * n64[None, :])
    n32 = np.sqrt((e * e).sum(axis=1))
    s32 = (e @ e.T) / (n32[:, None] * n32[None, :])
    assert s32.dtype == np.float32
    eps = 8.0 * np.abs(s32.astype(np.float64) - s64).max()
    np.fill_diagonal(s64, -np.inf)
    kth = np.sort(s64, axis=1)[:, -k]
    listed = s64[np.arange(1025)[:, None], ids]
    worst = (kth[:, None] - listed).max()
    print(f"clusters {clusters}: eps {eps:.3e}, the worst listed neighbour lies {worst:.3e} below the float64 k-th best, "
          f"device sims differ from float64 by at most {np.abs(sims.astype(np.float64) - listed).max():.3e}")
    assert (ids >= 0).all() and (ids != np.arange(1025)[:, None]).all() and worst <= eps
