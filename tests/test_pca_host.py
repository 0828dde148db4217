"""The PCA's host side without a device (include/buzzdetect_pca.h, buzzdetect_amd/pca.py): the host restatements against
independent NumPy statements of the header - in every bit where the order of operations is NumPy's to repeat, within 8 x the
float32 statement's own deviation from float64 for the Gram matrix -, the mathematics of ``finish``, the model's round trip,
every argument refusal of the entry points, and MapResult's text byte for byte."""
import ctypes as C

import numpy as np
import pytest

from buzzdetect_amd import _lib, cluster, dataset, pca, search
from tests import pca_cases as cases

DIM = cases.DIM
bits = cases.bits
EINVAL, EWORKSPACE = -1, -4


@pytest.fixture(scope="module")
def rows():
    e, _ = cases.planted(1025, seed=3, channels=128)
    return e, search.norms_host(e), e[:300].mean(axis=0).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- sums
@pytest.mark.parametrize("r", (0, 1, 255, 256, 257, 513))
def test_sums_host_is_the_sequential_float32_sum(rows, r):
    e, n2, shift = rows
    e, n2 = e[:r], n2[:r]
    rng = np.random.default_rng(r)
    picks = [None, rng.permutation(r).astype(np.int32), np.sort(rng.choice(r, size=r // 2, replace=False)).astype(np.int32)]
    for sh in (None, shift):
        for pick in picks:
            got = pca.sums_host(e, n2, sh, pick)
            assert got.shape == (((r if pick is None else len(pick)) + 255) // 256, DIM)
            assert np.array_equal(bits(got), bits(cases.sums_f32(e, sh, pick)))
    if r > 1:
        holed = e.copy()
        holed[r // 2, 9] = np.inf                                       # one absent row adds exactly nothing
        got = pca.sums_host(holed, search.norms_host(holed), shift)
        assert np.isfinite(got).all() and np.array_equal(bits(got), bits(cases.sums_f32(holed, shift)))


# ---------------------------------------------------------------------------------------------------- gram
@pytest.mark.parametrize("r", (1, 2, 3, 1025))
def test_gram_host_against_float64_within_the_bound_and_symmetric(rows, r):
    e, n2, shift = rows
    e, n2 = e[:r], n2[:r]
    got = pca.gram_host(e, n2, shift)
    assert np.array_equal(bits(got), bits(got.T))
    live = 128                                                          # the fixture's other channels are zero ...
    exact = cases.gram_f64(e, shift)
    assert not got[live:].any() and not got[:, live:].any() and not exact[live:].any()      # ... and stay so
    statement = np.abs(cases.gram_f32_sequential(e, shift, channels=live) - exact[:live, :live]).max()
    device = np.abs(got[:live, :live] - exact[:live, :live]).max()
    print(f"gram_host R={r}: restatement {device:.3e}, float32 statement {statement:.3e}, largest entry {np.abs(exact).max():.1f}")
    assert statement > 0 and device <= cases.BOUND * statement


def test_gram_host_accumulate_pick_and_absent_rows(rows):
    e, n2, shift = rows
    a = pca.gram_host(e[:1024], n2[:1024], shift)
    b = pca.gram_host(e[1024:], n2[1024:], shift)
    both = pca.gram_host(e[1024:], n2[1024:], shift, into=a.copy())
    assert np.array_equal(bits(both), bits((a + b).astype(np.float32)))  # gram_old + T
    ident = np.arange(e.shape[0], dtype=np.int32)
    assert np.array_equal(bits(pca.gram_host(e, n2, shift, ident)), bits(pca.gram_host(e, n2, shift)))
    holed, zeroed = e[:300].copy(), e[:300].copy()
    holed[100, 7] = np.nan
    zeroed[100] = 0.0
    got = pca.gram_host(holed, search.norms_host(holed))
    assert np.isfinite(got).all()
    assert np.array_equal(bits(got), bits(pca.gram_host(zeroed, search.norms_host(zeroed))))
    # a tile's chain is the fmaf chain: against exact products summed with one rounding a step, on a few elements
    t = cases.terms(e[:5], shift).astype(np.float64)
    chain = np.zeros((4, 4), np.float32)
    for row in t:
        chain = (np.multiply.outer(row[:4], row[40:44]) + chain.astype(np.float64)).astype(np.float32)
    assert np.array_equal(bits(pca.gram_host(e[:5], n2[:5], shift)[:4, 40:44]), bits(chain))


# ---------------------------------------------------------------------------------------------------- project
@pytest.mark.parametrize("d", (1, 2, 33, 64))
def test_project_host_is_the_headers_arithmetic(rows, d):
    e = rows[0][:200].copy()
    e[50, 100] = np.nan
    rng = np.random.default_rng(d)
    q, _ = np.linalg.qr(rng.standard_normal((DIM, d)))
    comps = np.ascontiguousarray(q.T, np.float32)
    mean = rows[0].mean(axis=0).astype(np.float32)
    mv = (comps.astype(np.float64) @ mean.astype(np.float64)).astype(np.float32)
    scale = rng.uniform(0.5, 2.0, d).astype(np.float32)
    with np.errstate(invalid="ignore"):
        scores = (e @ comps.T).astype(np.float32)                       # any scores will do: they are an input here
    y, resid = pca.project_host(e, scores, mv, scale, mean)
    want_y, want_r = cases.project_f32(e, scores, mv, scale, mean)
    assert np.array_equal(bits(y), bits(want_y)) and np.array_equal(bits(resid), bits(want_r))
    assert np.isnan(y[50]).all() and np.isnan(resid[50])
    assert np.isfinite(np.delete(y, 50, axis=0)).all() and np.isfinite(np.delete(resid, 50)).all()
    y_only, none = pca.project_host(e, scores, mv, scale, mean, residual=False)
    assert none is None and np.array_equal(bits(y_only), bits(y))


# ---------------------------------------------------------------------------------------------------- finish
def test_finish_host_is_cov_and_eigh_in_float64():
    e, directions = cases.planted(600, seed=8, channels=96)
    x = e.astype(np.float64)
    shift = x[:50].mean(axis=0).astype(np.float32)
    t = x - shift.astype(np.float64)
    comps, mean, values, total = pca.finish_host(t.T @ t, t.sum(axis=0), 600, shift, 3)
    cov = np.cov(x, rowvar=False)
    want_values, want_vectors = np.linalg.eigh(cov)
    assert np.allclose(values, want_values[::-1][:3], rtol=1e-10)
    assert np.allclose(mean, x.mean(axis=0), atol=1e-12) and np.isclose(total, np.trace(cov), rtol=1e-12)
    for j in range(3):
        v = comps[j]
        assert abs(abs(v @ want_vectors[:, -1 - j]) - 1.0) < 1e-9 and abs(abs(v @ directions[j]) - 1.0) < 2e-2
        assert v[np.argmax(np.abs(v))] > 0


def test_finish_host_sign_rule_takes_the_lowest_index_among_ties():
    g = np.zeros((DIM, DIM))
    g[3, 3] = g[9, 9] = 2.0
    g[3, 9] = g[9, 3] = -1.0                                            # top eigenvector (e3 - e9) / sqrt 2: a tie in magnitude
    comps, _, values, _ = pca.finish_host(g, np.zeros(DIM), 2, np.zeros(DIM, np.float32), 1)
    assert np.isclose(values[0], 3.0) and comps[0][3] > 0 > comps[0][9]


def test_finish_and_whiten_refusals():
    g = np.eye(DIM)
    with pytest.raises(ValueError, match="at least 2 rows"):
        pca.finish_host(g, np.zeros(DIM), 1, np.zeros(DIM, np.float32), 2)
    with pytest.raises(ValueError, match="at least 2 rows"):
        pca.PCA(2).finish()
    for bad in (0, 65):
        with pytest.raises(ValueError, match="n_components"):
            pca.PCA(bad)
    model = pca.PCAModel(np.eye(2, DIM, dtype=np.float32), np.zeros(DIM, np.float32), np.array([1.0, 0.0]), 1.0, 10, whiten=True)
    with pytest.raises(ValueError, match="not positive"):
        model.constants()
    model.whiten = False
    mv, scale = model.constants()
    assert np.array_equal(scale, np.ones(2, np.float32)) and mv.dtype == np.float32
    model = pca.PCAModel(np.eye(2, DIM, dtype=np.float32), np.full(DIM, 0.5, np.float32), np.array([4.0, 0.25]), 5.0, 10, whiten=True)
    mv, scale = model.constants()
    assert np.array_equal(scale, np.array([0.5, 2.0], np.float32)) and np.array_equal(mv, np.array([0.5, 0.5], np.float32))
    assert np.allclose(model.explained_variance_ratio, [0.8, 0.05])


def test_model_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    model = pca.PCAModel(rng.standard_normal((3, DIM)).astype(np.float32), rng.standard_normal(DIM).astype(np.float32),
                         np.array([3.0, 2.0, 1.0]), 7.5, 4096, whiten=True)
    path = str(tmp_path / "m.npz")
    model.save(path)
    back = pca.load(path)
    assert np.array_equal(bits(back.components), bits(model.components)) and np.array_equal(bits(back.mean), bits(model.mean))
    assert np.array_equal(back.explained_variance, model.explained_variance)
    assert (back.total_variance, back.n_rows, back.whiten) == (7.5, 4096, True)
    assert pca.PCA.from_model(back).model() is back
    assert np.array_equal(pca.sample_rows(100, 10, 3), pca.sample_rows(100, 10, 3)) and pca.sample_rows(10, 10) is None


# ---------------------------------------------------------------------------------------------------- refusals
def refused(rc, code, word):
    text = _lib.load().bd_last_error().decode()
    assert rc == code, (rc, text)
    assert word in text, text


def test_every_argument_refusal_runs_without_a_device():
    lib = _lib.load()
    assert lib.bd_pca_abi_version() == _lib.PCA_ABI_VERSION == 1
    assert (_lib.PCA_DIM, _lib.PCA_MAX_COMPONENTS, _lib.PCA_MAX_ROWS, _lib.PCA_SLICE, _lib.PCA_SUM_SLICE) == (1024, 64, 1 << 18, 1024, 256)
    buf = np.zeros(4 * DIM + 64, np.float32)
    a = buf.ctypes.data + (-buf.ctypes.data) % 16                       # a 16-byte aligned address that is never read
    big = 1 << 18
    assert lib.bd_pca_workspace_bytes(0) == 0 and lib.bd_pca_workspace_bytes(1) == 528 * 4096
    assert lib.bd_pca_workspace_bytes(1025) == 2 * 528 * 4096 and lib.bd_pca_workspace_bytes(big) == 256 * 528 * 4096
    refused(lib.bd_pca_workspace_bytes(big + 1), EINVAL, "R")
    refused(lib.bd_pca_workspace_bytes(-1), EINVAL, "R")

    for host, fn in ((False, lib.bd_pca_sums), (True, lib.bd_pca_sums_host)):
        tail = () if host else (None,)
        assert fn(None, 0, None, 0, None, None, None, *tail) == 0       # nothing to do, nothing looked at
        refused(fn(a, 4, None, -1, a, None, a, *tail), EINVAL, "R =")
        refused(fn(a, big + 1, None, big + 1, a, None, a, *tail), EINVAL, "R =")
        refused(fn(a, 0, None, 1, a, None, a, *tail), EINVAL, "rows_total")
        refused(fn(a, 4, None, 5, a, None, a, *tail), EINVAL, "without a pick")
        refused(fn(None, 4, None, 4, a, None, a, *tail), EINVAL, "e is null")
        refused(fn(a + 4, 4, None, 4, a, None, a, *tail), EINVAL, "e is not 16-byte")
        refused(fn(a, 4, a + 2, 4, a, None, a, *tail), EINVAL, "pick")
        refused(fn(a, 4, None, 4, None, None, a, *tail), EINVAL, "n2 is null")
        refused(fn(a, 4, None, 4, a, a + 4, a, *tail), EINVAL, "shift is not 16-byte")
        refused(fn(a, 4, None, 4, a, None, None, *tail), EINVAL, "partial is null")
    for host, fn in ((False, lib.bd_pca_gram), (True, lib.bd_pca_gram_host)):
        tail = () if host else (a, 1 << 40, None)
        assert fn(None, 0, None, 0, None, None, 0, None, *(() if host else (None, 0, None))) == 0
        refused(fn(a, 4, None, 4, a, None, 2, a, *tail), EINVAL, "accumulate")
        refused(fn(a, 4, None, -1, a, None, 0, a, *tail), EINVAL, "R =")
        refused(fn(a, 4, None, big + 1, a, None, 0, a, *tail), EINVAL, "R =")
        refused(fn(a, 4, None, 5, a, None, 0, a, *tail), EINVAL, "without a pick")
        refused(fn(None, 4, None, 4, a, None, 0, a, *tail), EINVAL, "e is null")
        refused(fn(a, 4, None, 4, None, None, 0, a, *tail), EINVAL, "n2 is null")
        refused(fn(a, 4, None, 4, a, a + 8, 0, a, *tail), EINVAL, "shift")
        refused(fn(a, 4, None, 4, a, None, 0, None, *tail), EINVAL, "gram is null")
    refused(lib.bd_pca_gram(a, 4, None, 4, a, None, 0, a + 4, a, 1 << 40, None), EINVAL, "gram is not 16-byte")
    refused(lib.bd_pca_gram(a, 4, None, 4, a, None, 0, a, None, 1 << 40, None), EINVAL, "workspace is null")
    refused(lib.bd_pca_gram(a, 4, None, 4, a, None, 0, a, a, 528 * 4096 - 1, None), EWORKSPACE, "needed are 2162688")
    for host, fn in ((False, lib.bd_pca_project), (True, lib.bd_pca_project_host)):
        tail = () if host else (None,)
        name = "scores" if host else "packed"
        assert fn(None, 0, None, 1, None, None, None, None, None, *tail) == 0
        refused(fn(a, 1, a, 0, a, a, a, a, a, *tail), EINVAL, "d = 0")
        refused(fn(a, 1, a, 65, a, a, a, a, a, *tail), EINVAL, "d = 65")
        refused(fn(a, -1, a, 2, a, a, a, a, a, *tail), EINVAL, "W = -1")
        refused(fn(a, (1 << 20) + 1, a, 2, a, a, a, a, a, *tail), EINVAL, "W =")
        refused(fn(None, 1, a, 2, a, a, a, a, a, *tail), EINVAL, "e is null")
        refused(fn(a, 1, None, 2, a, a, a, a, a, *tail), EINVAL, name + " is null")
        refused(fn(a, 1, a, 2, None, a, a, a, a, *tail), EINVAL, "mv is null")
        refused(fn(a, 1, a, 2, a, None, a, a, a, *tail), EINVAL, "scale is null")
        refused(fn(a, 1, a, 2, a, a, a + 4, a, a, *tail), EINVAL, "mean is not 16-byte")
        refused(fn(a, 1, a, 2, a, a, a, None, a, *tail), EINVAL, "y is null")
        refused(fn(a, 1, a, 2, a, a, a, a, a + 1, *tail), EINVAL, "resid is not 4-byte")
    refused(lib.bd_pca_project(a, 1, a + 4, 2, a, a, a, a, a, None), EINVAL, "packed is not 16-byte")

    e = np.zeros((4, DIM), np.float32)
    n2 = np.zeros(4, np.float32)
    for bad in (-1, 4):
        with pytest.raises(_lib.BuzzdetectHipError, match="pick\\[1\\]") as err:
            pca.sums_host(e, n2, None, np.array([0, bad], np.int32))
        assert "BD_ERANGE" in str(err.value)
        with pytest.raises(_lib.BuzzdetectHipError, match="pick\\[1\\]"):
            pca.gram_host(e, n2, None, np.array([0, bad], np.int32))


# ---------------------------------------------------------------------------------------------------- MapResult
def hand_made():
    coords = np.array([[1.5, -2.0], [0.25, 0.5], [3.0, 4.0], [0.0, 0.0], [-1.0, 1.0]], np.float32)
    residual = np.array([0.5, 2.0, np.nan, 2.0, 0.125], np.float32)
    return pca.MapResult(coords, residual, ["site/a", "b"], [0, 0, 0, 1, 1], [0.0, 0.96, 1.92, 0.0, 0.96])


def test_map_result_text_byte_for_byte(tmp_path):
    found = hand_made()
    path = tmp_path / "map.csv"
    found.to_csv(str(path))
    assert path.read_bytes() == (b"ident,start,end,pc1,pc2,residual\r\n"
                                 b"site/a,0.0,0.96,1.5,-2.0,0.5\r\n"
                                 b"site/a,0.96,1.92,0.25,0.5,2.0\r\n"
                                 b"site/a,1.92,2.88,3.0,4.0,nan\r\n"
                                 b"b,0.0,0.96,0.0,0.0,2.0\r\n"
                                 b"b,0.96,1.92,-1.0,1.0,0.125\r\n")
    labels = cluster.ClusterResult([2, 0, 1, 1, 0], np.zeros(5), [2, 2, 1], ["site/a", "b"], [0, 0, 0, 1, 1], found.starts)
    found.to_csv(str(path), clusters=labels)
    lines = path.read_bytes().split(b"\r\n")
    assert lines[0] == b"ident,start,end,pc1,pc2,residual,cluster" and lines[1] == b"site/a,0.0,0.96,1.5,-2.0,0.5,2"
    assert lines[5] == b"b,0.96,1.92,-1.0,1.0,0.125,0" and lines[6] == b""
    short = cluster.ClusterResult([2, 0], np.zeros(2), [1, 0, 1], ["b"], [0, 0], [0.0, 0.96])
    with pytest.raises(ValueError, match="not the same walk"):
        found.to_csv(str(path), clusters=short)
    with pytest.raises(ValueError):
        pca.MapResult(np.zeros((3, 2)), np.zeros(4), ["a"], [0] * 4, [0.0] * 4)


def test_map_result_outliers_and_annotations(tmp_path):
    found = hand_made()
    assert found.outliers(3) == [("site/a", 0.96, 2.0), ("b", 0.0, 2.0), ("site/a", 0.0, 0.5)]     # ties: the earlier window
    everything = found.outliers(10)
    assert [w[:2] for w in everything] == [("site/a", 0.96), ("b", 0.0), ("site/a", 0.0), ("b", 0.96), ("site/a", 1.92)]
    assert np.isnan(everything[-1][2]) and found.outliers(0) == []      # NaN last
    path = tmp_path / "review.csv"
    got = found.annotations("review", 2, path=str(path))
    assert got == [("site/a", 0.96, 1.92, "review"), ("b", 0.0, 0.96, "review")]
    assert path.read_bytes() == b"ident,start,end,label\r\nsite/a,0.96,1.92,review\r\nb,0.0,0.96,review\r\n"
    assert dataset.read_annotations(str(path)) == {"site/a": [(0.96, 1.92, "review")], "b": [(0.0, 0.96, "review")]}
