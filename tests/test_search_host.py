"""The host side of search by example (include/buzzdetect_search.h, buzzdetect_amd/search.py), no device needed: the row norms
against float64, the selection against np.lexsort on every key bit, decoding, what is refused, and hits -> annotation rows."""
import os
import re

import numpy as np
import pytest

from buzzdetect_amd import _lib, dataset, search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 2, 63, 64, 65, 1024)
VALUES = np.array([-2.5, -1.0, 0.0, 0.25, 0.5, 1.0, 3.0], np.float32)          # 7 distinct scores: ties dominate
SPECIALS = np.array([-0.0, 0.0, -np.inf, np.inf, np.nan], np.float32)


def test_prototypes_are_the_header():
    with open(os.path.join(ROOT, "include", "buzzdetect_search.h")) as f:
        header = f.read()
    names = sorted(re.findall(r"^BD_API [^;(]*?(bd_\w+)\(", header, re.M))
    assert names == sorted(_lib.SEARCH_PROTOTYPES) and len(names) == 9
    for name in names:
        args = re.search(r"BD_API [^;(]*?" + name + r"\(([^;]*)\);", header).group(1)
        n_args = 0 if args.strip() == "void" else args.count(",") + 1
        assert len(_lib.SEARCH_PROTOTYPES[name][1]) == n_args, name
    assert _lib.load().bd_search_abi_version() == _lib.SEARCH_ABI_VERSION == 1
    for word, value in (("BD_SEARCH_MAX_QUERIES", _lib.SEARCH_MAX_QUERIES), ("BD_SEARCH_MAX_K", _lib.SEARCH_MAX_K),
                        ("BD_SEARCH_DIM", _lib.SEARCH_DIM)):
        assert int(re.search(r"#define " + word + r" (\d+)", header).group(1)) == value == 1024


# ---------------------------------------------------------------------------------------------------- norms
def test_norms_against_float64():
    """16 chain steps and 6 tree steps of one rounding each on non-negative terms: at most 23 * 2^-24 < 2e-6 relative."""
    rng = np.random.default_rng(3)
    e = rng.normal(size=(70, 1024)).astype(np.float32)
    e[1] *= 1e-12
    e[2] *= 1e12
    e[3] = 0.0                                                   # an all-zero row
    e[4, ::2] *= 1e-6                                            # mixed magnitudes inside one row
    e[5, :64] *= 1e5
    e[6] = 0.0
    e[6, 1023] = 3.0
    got = search.norms_host(e)
    want = (e.astype(np.float64) ** 2).sum(axis=1)
    assert got.dtype == np.float32 and got[3] == 0.0 and got[6] == 9.0
    live = want > 0
    rel = np.abs(got[live].astype(np.float64) - want[live]) / want[live]
    print("largest relative error of the norms:", rel.max())
    assert rel.max() <= 2e-6
    assert search.norms_host(np.zeros((0, 1024), np.float32)).size == 0


# ---------------------------------------------------------------------------------------------------- selection
def canonical(scores):
    s = np.array(scores, np.float32, copy=True)
    s[np.isnan(s)] = -np.inf
    s[s == 0] = 0.0
    return s


def expected_keys(scores, ids, k):
    """The k best of the candidates by np.lexsort on (id, -score), as keys built here from the issue's definition."""
    s = canonical(scores)
    order = np.lexsort((ids, -s.astype(np.float64)))[:k]
    bits = s[order].view(np.uint32).astype(np.uint64)
    high = np.where(bits & 0x80000000, ~bits & 0xFFFFFFFF, bits | 0x80000000)
    keys = np.zeros(k, np.uint64)
    keys[:order.size] = (high << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - ids[order].astype(np.uint64))
    return keys


def draw(rng, w, q):
    s = rng.choice(VALUES, size=(w, q))
    if w:
        at = rng.integers(0, w, size=(min(w, 40), q))
        for c in range(q):
            s[at[:, c], c] = rng.choice(SPECIALS, size=at.shape[0])
    return np.ascontiguousarray(s, np.float32)


@pytest.mark.parametrize("q", (1, 3))
@pytest.mark.parametrize("k", KS)
def test_selection_is_lexsort_in_every_key_bit(k, q):
    rng = np.random.default_rng(100 * k + q)
    for w in sorted({0, 1, k - 1, k, k + 1, 4097}):
        for base in (0, 1000, 0xFFFFFFFF - w):
            s = draw(rng, w, q)
            keys = search.update_host(np.zeros((q, k), np.uint64), s, base)
            ids = base + np.arange(w, dtype=np.int64)
            for c in range(q):
                want = expected_keys(s[:, c], ids, k)
                assert keys[c].tobytes() == want.tobytes(), (k, w, q, base, c)
            assert ((keys != 0).sum(axis=1) == min(k, w)).all()
    # a second pass merges with the state; a transposed (query-major) matrix is read by its strides
    a, b = draw(rng, 300, q), draw(rng, 77, q)
    keys = search.update_host(np.zeros((q, k), np.uint64), a, 5)
    keys = search.update_host(keys, np.ascontiguousarray(b.T).T, 305)
    for c in range(q):
        want = expected_keys(np.concatenate([a[:, c], b[:, c]]), 5 + np.arange(377, dtype=np.int64), k)
        assert keys[c].tobytes() == want.tobytes()


@pytest.mark.parametrize("k", KS)
def test_pass_splits_leave_the_same_state(k):
    rng = np.random.default_rng(k)
    s = draw(rng, 4097, 3)
    once = search.update_host(np.zeros((3, k), np.uint64), s, 7)
    split, at = np.zeros((3, k), np.uint64), 0
    for n in (1, 31, 32, 33, 4000):
        search.update_host(split, s[at:at + n], 7 + at)
        at += n
    assert at == 4097 and once.tobytes() == split.tobytes()


def test_decoding_inverts_the_keys_and_leaves_empty_slots_out():
    rng = np.random.default_rng(9)
    s = draw(rng, 50, 2)
    s[:5, 0] = SPECIALS
    keys = search.update_host(np.zeros((2, 64), np.uint64), s, 123)
    scores, ids, real = search.decode_keys(keys)
    assert real == 100 and scores.shape == ids.shape == (2, 64)
    assert np.isneginf(scores[:, 50:]).all() and (ids[:, 50:] == 0xFFFFFFFF).all()
    got_s, got_i = search.decode_result(keys)
    assert got_s.shape == got_i.shape == (2, 50) and got_i.dtype == np.int64
    for c in range(2):
        want_s = canonical(s[:, c])
        order = np.lexsort((np.arange(50), -want_s.astype(np.float64)))
        assert got_i[c].tolist() == (123 + order).tolist()
        assert got_s[c].tobytes() == want_s[order].tobytes()               # -0.0 came back as +0.0, NaN as -inf
        # and back again: the decoded pairs give the keys
        assert expected_keys(got_s[c], got_i[c], 64)[:50].tobytes() == keys[c, :50].tobytes()
    assert search.decode_result(np.zeros((3, 5), np.uint64))[0].shape == (3, 0)


# ---------------------------------------------------------------------------------------------------- refusals
def refused(fn, *args):
    rc = fn(*args)
    assert rc < 0
    return rc, _lib.load().bd_last_error().decode()


@pytest.mark.parametrize("device_entry", (False, True))
def test_bad_arguments_are_refused_by_name_and_leave_the_state(device_entry):
    """Also for bd_search_update itself: the checks come before anything touches the device, so nothing is launched (the
    pointers here are host arrays)."""
    lib = _lib.load()
    s = np.ones((8, 3), np.float32)
    keys = np.arange(1, 3 * 1024 + 1, dtype=np.uint64).reshape(3, 1024)
    before = keys.copy()

    def call(w, q, base, k):
        tail = (None,) if device_entry else ()
        fn = lib.bd_search_update if device_entry else lib.bd_search_update_host
        return refused(fn, s.ctypes.data, w, q, 3, 1, base, keys.ctypes.data, k, *tail)

    for (w, q, base, k), code, word in (((8, 0, 0, 4), -1, "n_queries"), ((8, 1025, 0, 4), -1, "n_queries"),
                                        ((8, 3, 0, 0), -1, "k = 0"), ((8, 3, 0, 1025), -1, "k = 1025"),
                                        ((8, 3, 0xFFFFFFFF - 7, 4), -5, "base_id + windows"), ((8, 3, -1, 4), -1, "base_id"),
                                        (((1 << 20) + 1, 3, 0, 4), -1, "windows"), ((-1, 3, 0, 4), -1, "windows")):
        rc, text = call(w, q, base, k)
        assert rc == code and word in text, (rc, text)
        assert keys.tobytes() == before.tobytes()
    fn = lib.bd_search_update if device_entry else lib.bd_search_update_host
    tail = (None,) if device_entry else ()
    rc, text = refused(fn, s.ctypes.data, 8, 3, 0, 1, 0, keys.ctypes.data, 4, *tail)
    assert rc == -1 and "row_stride" in text
    rc, text = refused(fn, s.ctypes.data, 8, 3, 3, 0, 0, keys.ctypes.data, 4, *tail)
    assert rc == -1 and "col_stride" in text
    rc, text = refused(fn, s.ctypes.data, 8, 3, 3, 1, 0, None, 4, *tail)
    assert rc == -1 and "keys" in text
    rc, text = refused(fn, None, 8, 3, 3, 1, 0, keys.ctypes.data, 4, *tail)
    assert rc == -1 and "scores" in text
    assert keys.tobytes() == before.tobytes()
    # the last id itself is allowed
    small = np.zeros((3, 4), np.uint64)
    if not device_entry:
        rising = np.ascontiguousarray(np.arange(24, dtype=np.float32).reshape(8, 3))
        assert lib.bd_search_update_host(rising.ctypes.data, 8, 3, 3, 1, 0xFFFFFFFF - 8, small.ctypes.data, 4) == 0
        assert search.decode_result(small)[1][:, 0].tolist() == [0xFFFFFFFE] * 3 and (small != 0).all()


def test_scores_and_packing_refuse_before_any_launch():
    lib = _lib.load()
    e = np.zeros((4, 1024), np.float32)
    qp = np.zeros(32 * 1024 + 4, np.float32)
    qp = qp[(-qp.ctypes.data // 4) % 4:][:32 * 1024]                      # 16-byte aligned
    out = np.full(16, 7.0, np.float32)

    def scores(w, q, metric, rs=3, cs=1):
        return refused(lib.bd_search_scores, e.ctypes.data, w, qp.ctypes.data, q, metric, e.ctypes.data, out.ctypes.data, rs, cs, None)

    for args, word in (((4, 3, 2), "metric"), ((4, 3, -1), "metric"), ((4, 0, 1), "n_queries"), ((4, 1025, 0), "n_queries"),
                       ((-1, 3, 0), "windows"), ((4, 3, 1, 0, 1), "row_stride"), ((4, 3, 1, 3, 0), "col_stride")):
        rc, text = scores(*args)
        assert rc == -1 and word in text, text
    assert (out == 7.0).all()
    assert lib.bd_search_packed_floats(0) == -1 and lib.bd_search_packed_floats(1025) == -1
    assert lib.bd_search_packed_floats(1) == lib.bd_search_packed_floats(32) == 32 * 1024
    assert lib.bd_search_packed_floats(33) == 64 * 1024
    with pytest.raises(ValueError):
        search.pack_queries(np.zeros((3, 1000), np.float32))
    with pytest.raises(ValueError):
        search.normalise_queries(np.zeros((3, 1024)), "euclid")


def test_packing_is_the_dense_fragment_order():
    """packed[((t * 128 + s) * 64 + l) * 4 + j] = query 32 t + (l & 31), element 8 s + 4 (l >> 5) + j; zero past Q."""
    rng = np.random.default_rng(2)
    q = rng.normal(size=(33, 1024)).astype(np.float32)
    p = search.pack_queries(q).reshape(2, 128, 64, 4)
    t, s, l, j = np.meshgrid(np.arange(2), np.arange(128), np.arange(64), np.arange(4), indexing="ij")
    row, col = 32 * t + (l & 31), 8 * s + 4 * (l >> 5) + j
    want = np.where(row < 33, q[np.minimum(row, 32), col], 0.0).astype(np.float32)
    assert p.tobytes() == want.tobytes()


def test_cosine_queries_are_normalised_in_double():
    rng = np.random.default_rng(4)
    q = rng.normal(size=(3, 1024)) * np.array([[1e-3], [1.0], [1e4]])
    q[1] = 0.0
    n = search.normalise_queries(q, "cosine")
    assert n.dtype == np.float32 and (n[1] == 0).all()
    assert n[0].tobytes() == (q[0] / np.sqrt((q[0] * q[0]).sum())).astype(np.float32).tobytes()
    assert search.normalise_queries(q.astype(np.float32), "dot").tobytes() == q.astype(np.float32).tobytes()
    assert search.normalise_queries(q[0], "dot").shape == (1, 1024)


# ---------------------------------------------------------------------------------------------------- results
def test_hits_become_annotations_that_read_back(tmp_path):
    hits = [[("site1/rec_a", 0.0, 0.99), ("site1/rec_a", 199.68, 0.5), ("rec b", 12.48, 0.25)],
            [("rec b", 12.48, 0.9), ("site1/rec_a", 0.96, 0.1)]]
    res = search.SearchResult(hits, ["a message"])
    path = str(tmp_path / "found.csv")
    rows = res.annotations("ins_buzz", path=path)
    assert rows == [("site1/rec_a", 0.0, 0.96, "ins_buzz"), ("site1/rec_a", 199.68, 200.64, "ins_buzz"),
                    ("rec b", 12.48, 13.44, "ins_buzz"), ("site1/rec_a", 0.96, 1.92, "ins_buzz")]
    back = dataset.read_annotations(path)
    assert sorted((i, a, b, l) for i, v in back.items() for a, b, l in v) == sorted(rows)
    # a label per query keeps the window both found, once under each label; length is the caller's
    rows = res.annotations(["buzz", "other"], length=0.5, path=path)
    assert ("rec b", 12.48, 12.98, "buzz") in rows and ("rec b", 12.48, 12.98, "other") in rows and len(rows) == 5
    back = dataset.read_annotations(path)
    assert sorted((i, a, b, l) for i, v in back.items() for a, b, l in v) == sorted(rows)
    with pytest.raises(ValueError):
        res.annotations(["one"])
    # the labelled windows are the hit windows: label_windows sets exactly the window that starts at the hit
    targets, keep = dataset.label_windows(20, 0.96, [(a, b, l) for a, b, l in back["rec b"] if l == "buzz"], ["buzz"])
    assert targets[:, 0].tolist() == [1.0 if i == 13 else 0.0 for i in range(20)]


def test_hits_csv(tmp_path):
    import csv
    res = search.SearchResult([[("a", 0.96, 0.5)], [("b", 1.92, -1.25), ("a", 0.0, -2.0)]], [], ["ins_buzz", "ambient"])
    path = str(tmp_path / "hits.csv")
    res.to_csv(path)
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["query", "rank", "ident", "start", "end", "score"]
    assert rows[1:] == [["ins_buzz", "0", "a", "0.96", "1.92", "0.5"], ["ambient", "0", "b", "1.92", "2.88", "-1.25"],
                        ["ambient", "1", "a", "0.0", "0.96", "-2.0"]]


def test_index_maps_ids_to_analyze_starts():
    from buzzdetect_amd import framing
    index = search._Index(0.96)
    index.add("one", 0, [0.0, 199.68], [208, 5])
    index.add("empty", 213, [0.0], [0])
    index.add("two", 213, [0.0], [10])
    assert index.lookup(0) == ("one", 0.0) and index.lookup(207) == ("one", framing.window_starts(208, 0.0, 0.96)[207])
    assert index.lookup(208) == ("one", 199.68) and index.lookup(212) == ("one", framing.window_starts(5, 199.68, 0.96)[4])
    assert index.lookup(213) == ("two", 0.0) and index.lookup(222) == ("two", 8.64)
