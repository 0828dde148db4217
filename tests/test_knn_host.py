"""The host side of the neighbour lists (include/buzzdetect_knn.h, buzzdetect_amd/propagate.py), no device needed:
bd_knn_update_host against an independent NumPy statement in every key (tests/propagate_cases.py), the invariances of the
contract, the decoding, the symmetrised graph, and what is refused."""
import os
import re

import numpy as np
import pytest

from buzzdetect_amd import _lib, propagate
from tests import propagate_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ("cosine", "dot")


def test_prototypes_are_the_header():
    with open(os.path.join(ROOT, "include", "buzzdetect_knn.h")) as f:
        header = f.read()
    names = sorted(re.findall(r"^BD_API [^;(]*?(bd_\w+)\(", header, re.M))
    assert names == sorted(_lib.KNN_PROTOTYPES) and len(names) == 5
    for name in names:
        args = re.search(r"BD_API [^;(]*?" + name + r"\(([^;]*)\);", header).group(1)
        n_args = 0 if args.strip() == "void" else args.count(",") + 1
        assert len(_lib.KNN_PROTOTYPES[name][1]) == n_args, name
    assert _lib.load().bd_knn_abi_version() == _lib.KNN_ABI_VERSION == 1
    for word, value in (("BD_KNN_MAX_K", _lib.KNN_MAX_K), ("BD_KNN_DIM", _lib.KNN_DIM)):
        assert int(re.search(r"#define " + word + r" (\d+)", header).group(1)) == value
    assert "#define BD_KNN_MAX_ROWS (1 << 22)" in header and _lib.KNN_MAX_ROWS == 1 << 22
    assert _lib.KNN_METRICS == {"dot": 0, "cosine": 1}


def test_the_numpy_fused_multiply_add_rounds_once():
    """The yardstick's own yardstick.  2^36 + 1 = 4097 x 16773121, both factors float32: their product scaled by 2^-60 is
    2^-24 + 2^-60 exactly.  Added to 1 the exact sum lies just above a float32 tie and rounds up; a float64 addition drops the
    2^-60, lands on the tie, and the cast rounds to even - the double rounding a fused multiply-add does not have."""
    a, b, one = np.float32(4097 * 2.0 ** -30), np.float32(16773121 * 2.0 ** -30), np.float32(1.0)
    assert np.float64(a) * np.float64(b) == 2.0 ** -24 + 2.0 ** -60
    assert np.float32(np.float64(a) * np.float64(b) + 1.0) == one                        # twice rounded
    assert cases.fma32(a, b, one) == np.float32(1.0 + 2.0 ** -23)                        # once
    assert cases.fma32(-a * np.float32(0.5), b, one) == np.float32(1.0 - 2.0 ** -24)     # below the tie 1 - 2^-25: down
    assert np.float32(np.float64(-a * np.float32(0.5)) * np.float64(b) + 1.0) == one
    x = np.array([1.5, -2.25, 3.0], np.float32)
    assert cases.fma32(x, x, x).tolist() == [3.75, 2.8125, 12.0]                         # exact cases stay exact
    assert np.isnan(cases.fma32(np.float32(np.nan), one, one)) and np.isinf(cases.fma32(np.float32(np.inf), one, one))


@pytest.fixture(scope="module")
def rows():
    return cases.special_rows(257)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("wq,wc,k", ((1, 1, 1), (1, 33, 16), (33, 1, 2), (33, 33, 64), (129, 33, 63), (33, 129, 16), (257, 257, 16),
                                     (129, 257, 64), (257, 129, 1)))
def test_update_host_equals_numpy_in_every_key(rows, wq, wc, k, metric):
    """Fewer candidates than k leave empty slots; rows 0, 1 and the last are equal (the lower id first); row 3 is zero, row 5
    holds a NaN, row 7 lies below the norm floor."""
    q, c = rows[:wq], rows[257 - wc:]
    for exclude_self in (False, True):
        base = 257 - wc if exclude_self else 1000            # with exclude_self the ids are the rows' own numbers
        want = cases.knn_numpy(q, c, k, metric, exclude_self, 0, base)
        got = propagate.knn_update_host(np.zeros((wq, k), np.uint64), q, c, metric=metric, exclude_self=exclude_self, c_base_id=base)
        assert got.tobytes() == want.tobytes()
        if not exclude_self:
            assert ((got != 0).sum(axis=1) == min(k, wc)).all()


def test_special_rows_order(rows):
    k = 16
    keys = propagate.knn_update_host(np.zeros((257, k), np.uint64), rows, rows, metric="cosine", exclude_self=True)
    ids, sims = propagate.decode_keys(keys)
    assert ids[0, :2].tolist() == [1, 256] and ids[1, :2].tolist() == [0, 256] and ids[256, :2].tolist() == [0, 1]
    assert sims[0, 0] == sims[1, 0] == sims[256, 1]                      # duplicates: the same bits, the lower id first
    assert (sims[3] == 0).all() and ids[3].tolist() == [i for i in range(k + 1) if i != 3]       # a zero row: all ties at 0
    assert (sims[7] == 0).all()                                          # below the norm floor
    # a NaN row: 0 with the rows below the floor, -inf (the NaN's place) with the others, the lower id first
    assert ids[5, :2].tolist() == [3, 7] and (sims[5, :2] == 0).all() and np.isneginf(sims[5, 2:]).all()
    assert ids[5, 2:].tolist() == [i for i in range(k + 1) if i not in (3, 5, 7)]
    assert not (ids[[0, 1, 2, 4]] == 5).any()                            # and a NaN row is nobody's neighbour here
    assert (np.arange(257)[:, None] != ids).all()


@pytest.mark.parametrize("metric", METRICS)
def test_one_call_equals_any_split_and_rows_do_not_depend_on_their_place(rows, metric):
    k = 16
    whole = propagate.knn_update_host(np.zeros((129, k), np.uint64), rows[:129], rows, metric=metric, exclude_self=True)
    split = np.zeros((129, k), np.uint64)
    for a, b in ((200, 257), (0, 1), (1, 100), (100, 200)):
        propagate.knn_update_host(split, rows[:129], rows[a:b], metric=metric, exclude_self=True, c_base_id=a)
    assert split.tobytes() == whole.tobytes()
    moved = propagate.knn_update_host(np.zeros((20, k), np.uint64), rows[40:60], rows, metric=metric, exclude_self=True, q_base_id=40)
    assert moved.tobytes() == whole[40:60].tobytes()


@pytest.mark.parametrize("metric", METRICS)
def test_similarities_are_bit_symmetric(rows, metric):
    s = cases.sims(rows[:65], rows[:65], metric)
    assert s.tobytes() == np.ascontiguousarray(s.T).tobytes()
    ids, sims = propagate.decode_keys(propagate.knn_update_host(np.zeros((257, 16), np.uint64), rows, rows, metric=metric,
                                                                exclude_self=True))
    both = 0
    for i in range(257):
        for slot, j in enumerate(ids[i]):
            back = np.flatnonzero(ids[j] == i)
            if back.size:
                both += 1
                assert cases.bits(sims[i, slot]) == cases.bits(sims[j, back[0]])
    assert both > 500


def test_base_ids_up_to_the_last_one(rows):
    last = 0xFFFFFFFF
    q, c = rows[:33], rows[:129]
    want = cases.knn_numpy(q, c, 16, "cosine", True, last - 33, last - 129)
    got = propagate.knn_update_host(np.zeros((33, 16), np.uint64), q, c, exclude_self=True, q_base_id=last - 33, c_base_id=last - 129)
    assert got.tobytes() == want.tobytes() and (got != 0).all()
    # query i has id last - 33 + i, which is candidate 96 + i: left out
    assert ((np.uint64(last) - (got & np.uint64(last))) != (last - 33 + np.arange(33, dtype=np.uint64))[:, None]).all()
    with pytest.raises(_lib.BuzzdetectHipError, match="bd_knn_decode_host.*holds id"):
        propagate.decode_keys(got)


def test_decode():
    keys = cases.make_keys(np.array([0.5, -0.0, np.nan, -2.0], np.float32), np.array([7, 0, 3, 0x7FFFFFFF]))
    ids, sims = propagate.decode_keys(np.concatenate([keys, np.zeros(2, np.uint64)]).reshape(2, 3))
    assert ids.tolist() == [[7, 0, 3], [0x7FFFFFFF, -1, -1]]
    assert sims.tobytes() == np.array([[0.5, 0.0, -np.inf], [-2.0, 0.0, 0.0]], np.float32).tobytes()


# ---------------------------------------------------------------------------------------------------- the symmetrised graph
def test_symmetrised_has_every_reverse_once_and_is_idempotent():
    _, _, ids, sims = cases.planted_lists(1025, 5, 16)
    ids, sims = ids.copy(), sims.copy()
    ids[10, 12:], sims[10, 12:] = -1, 0.0                                # a row with empty slots
    g = propagate.KnnGraph(ids, sims, ["r"], np.zeros(1025, np.int64), np.arange(1025) * 0.96)
    s = g.symmetrised()
    src = np.repeat(np.arange(1025), np.diff(s.row_start))
    edges = {(int(i), int(j)): cases.bits(v).item() for i, j, v in zip(src, s.nbr, s.sims)}
    assert len(edges) == s.nbr.shape[0]                                  # no duplicates
    assert all(edges[(j, i)] == b for (i, j), b in edges.items())        # every reverse, with the same weight bits
    for i in range(1025):
        for j, v in zip(ids[i], sims[i]):
            if j >= 0:
                assert edges[(i, int(j))] == cases.bits(v).item()
    assert set(edges) == {(i, int(j)) for i in range(1025) for j in ids[i] if j >= 0} | \
        {(int(j), i) for i in range(1025) for j in ids[i] if j >= 0}
    for i in (0, 10, 500, 1024):                                         # descending similarity, then ascending id
        a, b = s.row_start[i], s.row_start[i + 1]
        assert np.lexsort((s.nbr[a:b], -s.sims[a:b].astype(np.float64))).tolist() == list(range(b - a))
    again = s.symmetrised()
    assert again.row_start.tobytes() == s.row_start.tobytes() and again.nbr.tobytes() == s.nbr.tobytes()
    assert again.sims.tobytes() == s.sims.tobytes()


def test_graph_files_and_lookups(tmp_path):
    _, _, ids, sims = cases.planted_lists(1025, 5, 16)
    ids, sims = ids[:40] % 40, sims[:40].copy()
    sims[3, 0], ids[3, 0] = 0.9995, 8
    g = propagate.KnnGraph(ids, sims, ["a", "site/b"], np.repeat([0, 1], 20), np.tile(np.arange(20) * 0.96, 2).round(2), "cosine")
    path = str(tmp_path / "g.npz")
    g.save(path)
    h = propagate.KnnGraph.load(path)
    assert h.ids.tobytes() == g.ids.tobytes() and h.sims.tobytes() == g.sims.tobytes() and h.recordings == g.recordings
    assert h.starts.tolist() == g.starts.tolist() and h.metric == "cosine" and h.k == 16
    assert h.row_of("site/b", 2.88) == 23
    near = h.neighbours("a", 2.88)
    assert near[0] == ("a", 7.68, float(np.float32(0.9995))) and len(near) == 16
    with pytest.raises(KeyError):
        h.neighbours("a", 2.5)
    dup = h.duplicates(0.999)
    assert (("a", 2.88), ("a", 7.68), float(np.float32(0.9995))) in dup


# ---------------------------------------------------------------------------------------------------- what is refused
def call_update(lib, host, **over):
    a = dict(q=np.zeros((4, 1024), np.float32), wq=4, n2q=np.ones(4, np.float32), qb=0, c=np.zeros((4, 1024), np.float32), wc=4,
             n2c=np.ones(4, np.float32), cb=0, metric=1, ex=0, keys=np.full((4, 64), 9, np.uint64), k=2)
    a.update(over)
    ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)
    args = [ptr(a["q"]), a["wq"], ptr(a["n2q"]), a["qb"], ptr(a["c"]), a["wc"], ptr(a["n2c"]), a["cb"], a["metric"], a["ex"],
            ptr(a["keys"]), a["k"]]
    if host:
        return lib.bd_knn_update_host(*args), a["keys"]
    return lib.bd_knn_update(*args, a.get("ws", 4096), a.get("ws_bytes", 1 << 20), None), a["keys"]


@pytest.mark.parametrize("host", (True, False))
def test_limits_are_refused_with_the_argument_named(host):
    """The device entry point refuses before it launches: these calls need no device (the pointers are never followed)."""
    lib = _lib.load()
    cases_ = [(dict(k=0), "k = 0"), (dict(k=65), "k = 65"), (dict(wq=(1 << 22) + 1), "query_rows"), (dict(wc=-1), "candidate_rows"),
              (dict(qb=-1), "q_base_id"), (dict(cb=0xFFFFFFFF - 3), "c_base_id"), (dict(metric=2), "metric"),
              (dict(ex=2), "exclude_self"), (dict(q=None), "queries is null"), (dict(c=None), "candidates is null"),
              (dict(n2q=None), "n2_q"), (dict(n2c=None), "n2_c"), (dict(keys=None), "keys is null")]
    if not host:
        q = np.zeros((5, 1024), np.float32)
        cases_ += [(dict(q=q.ctypes.data + 4), "queries is not 16-byte aligned"), (dict(ws=None), "workspace is null"),
                   (dict(ws=4104), "workspace is not 16-byte aligned"), (dict(ws_bytes=511), "workspace_bytes = 511, needed are 512")]
    for over, text in cases_:
        rc, keys = call_update(lib, host, **over)
        assert rc < 0, over
        assert text in lib.bd_last_error().decode(), (over, lib.bd_last_error().decode())
        assert keys is None or (keys == 9).all()                         # nothing written
    assert lib.bd_knn_workspace_bytes(4, 4) == 512 and lib.bd_knn_workspace_bytes(65, 129) == 512 + 768
    assert lib.bd_knn_workspace_bytes(-1, 4) < 0 and "query_rows" in lib.bd_last_error().decode()
    assert lib.bd_knn_workspace_bytes(4, (1 << 22) + 1) < 0 and "candidate_rows" in lib.bd_last_error().decode()
    # no rows on either side: nothing to do, nothing touched
    rc, keys = call_update(lib, host, wq=0, q=None)
    assert rc == 0 and (keys == 9).all()
    with pytest.raises(ValueError, match="metric"):
        propagate.Neighbours(4, metric="euclidean")
    with pytest.raises(ValueError, match="k must be"):
        propagate.Neighbours(65)
