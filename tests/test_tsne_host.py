"""The host side of the neighbour-preserving map (include/buzzdetect_tsne.h, buzzdetect_amd/tsne.py), no device needed:
attraction, repulsion and update against the NumPy statement in every bit (tests/tsne_cases.py), the calibration's special rows,
the symmetric P, what is refused, the rows left out, the results' files, and the whole loop on the host routines against the
golden file and the PCA plane."""
import json
import os
import re

import numpy as np
import pytest

from buzzdetect_amd import _lib, tsne
from buzzdetect_amd.propagate import KnnGraph
from tests import propagate_cases, tsne_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    return C.bits(a).tobytes() == C.bits(b).tobytes()


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "tsne_quality.json")) as f:
        return json.load(f)


def test_prototypes_are_the_header():
    with open(os.path.join(ROOT, "include", "buzzdetect_tsne.h")) as f:
        header = f.read()
    names = sorted(re.findall(r"^BD_API [^;(]*?(bd_\w+)\(", header, re.M))
    assert names == sorted(_lib.TSNE_PROTOTYPES) and len(names) == 12
    for name in names:
        args = re.search(r"BD_API [^;(]*?" + name + r"\(([^;]*)\);", header).group(1)
        n_args = 0 if args.strip() == "void" else args.count(",") + 1
        assert len(_lib.TSNE_PROTOTYPES[name][1]) == n_args, name
    assert _lib.load().bd_tsne_abi_version() == _lib.TSNE_ABI_VERSION == 1
    for word, value in (("BD_TSNE_MAX_K", _lib.TSNE_MAX_K), ("BD_TSNE_SLICE", _lib.TSNE_SLICE),
                        ("BD_TSNE_ROWS_PER_BLOCK", _lib.TSNE_ROWS_PER_BLOCK), ("BD_TSNE_BISECTIONS", _lib.TSNE_BISECTIONS)):
        assert int(re.search(r"#define " + word + r" (\d+)", header).group(1)) == value
    assert "#define BD_TSNE_MAX_ROWS (1 << 20)" in header and _lib.TSNE_MAX_ROWS == 1 << 20
    assert (C.SLICE, C.ROWS_PER_BLOCK, C.BISECTIONS) == (_lib.TSNE_SLICE, _lib.TSNE_ROWS_PER_BLOCK, _lib.TSNE_BISECTIONS)


# ---------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("n", (1, 2, 65, 257, C.SLICE + 1))
def test_repulse_host_is_the_numpy_statement(n):
    for scale in C.SCALES if n < 1000 else ("mix",):
        y = C.coords(n, scale)
        rep, z = tsne.repulse_host(y)
        want_rep, want_z = C.repulse32(y)
        assert same_bits(rep, want_rep) and same_bits(z, want_z), scale
        if n > 8:
            assert z[0] >= 2 and np.isfinite(rep).all()                 # the coincident points count in z and push nothing
            q2 = np.float32(C.q32(y[0, :1] - y[4, :1], y[0, 1:] - y[4, 1:])[0]) ** 2
            assert 0 < q2 < np.finfo(np.float32).tiny                   # the point at 1e10: a subnormal q * q, kept as one


def test_attract_host_is_the_numpy_statement():
    row_start, nbr, big = C.graph_case()
    for scale in C.SCALES:
        y = C.coords(310, scale)
        got = tsne.attract_host(tsne.JointGraph(row_start, nbr, big), y)
        assert same_bits(got, C.attract32(row_start, nbr, big, y)), scale
        assert (got[0] == 0).all()                                      # degree 0


@pytest.mark.parametrize("n", (11, 1025, 2 * C.SLICE + 3))
def test_update_host_is_the_numpy_statement(n):
    y, v, gain, attr, rep, z = C.update_case(n)
    for exaggeration, momentum in ((12.0, 0.5), (1.0, 0.8)):
        got = tsne.update_host(y, v, gain, attr, rep, z, exaggeration, momentum, 50.0)
        want = C.update32(y, v, gain, attr, rep, z, exaggeration, momentum, 50.0)
        for a, b, name in zip(got, want, ("y", "v", "gain", "Z")):
            assert same_bits(a, b), name
    new_y, new_v, new_gain, _ = got
    # g = 0 against v = 0 of either sign: the signs agree, the gain shrinks; nothing moves but by the mean
    assert same_bits(new_gain[:3], np.maximum(gain[:3] * np.float32(0.8), np.float32(0.01))) and (new_v[:3] == 0).all()
    assert new_gain[9, 0] == np.float32(0.01) or new_gain[9, 0] == np.float32(0.01) + np.float32(0.2)      # the floor holds
    assert (new_gain >= np.float32(0.01)).all()
    # the mean is removed, within rounding: a column's float32 sum errs by at most (32 + 6 + slices) roundings of its partial sums
    assert abs(new_y.astype(np.float64).mean(axis=0)).max() <= 64 * np.abs(new_y).max() * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------- P
def test_affinities_host_special_rows_and_perplexity():
    for k, perplexity in ((1, 1.0), (16, 5.0), (48, 16.0), (64, 16.0)):
        ids, sims = C.lists_case(257, k)
        p, beta = tsne.affinities_host(ids, sims, perplexity)
        p64, beta64 = C.affinities(ids, sims, perplexity, np.float64)
        ok = C.usable(ids, sims)
        assert np.isfinite(p).all() and (p[~ok] == 0).all() and (p >= 0).all()
        assert (p[0] == 0).all() and beta[0] == 0                                       # the empty row
        assert p[1, 0] == 1 and (p[1, 1:] == 0).all() and beta[1] == 0                  # one neighbour
        if k > 1:
            assert same_bits(p[2], np.full(k, np.float32(1.0) / np.float32(k)))         # all duplicates: uniform
            assert same_bits(p[4, :2], np.full(2, np.float32(0.5))) and (p[4, 2:] == 0).all()   # short of the perplexity
            assert abs(p[3].sum() - 1) < 1e-6 and (p[3][~ok[3]] == 0).all()             # non-finite similarities are absent
        # p <= 1 comes from an exponential, a sum of at most 64 terms and a division, at a beta that 64 bisection steps fix to
        # float32 resolution: a few units of 2^-24 each; 32 units bound them all (the device goes by the 8 x rule instead)
        assert np.abs(p - p64).max() < 32 * 2.0 ** -24
        reachable = ok.sum(axis=1) > perplexity
        reachable[2] = False                                                            # d = 0 everywhere: perplexity k
        if reachable.any():
            # the entropy is held to float32 rounding of log(64) + beta A / S, a few 1e-6; the perplexity is 16 times that
            assert np.abs(C.perplexity_of(p)[reachable] - perplexity).max() < 1e-4
            assert np.allclose(beta[reachable], beta64[reachable], rtol=1e-4)


def test_joint_probabilities():
    ids, sims = C.lists_case(257, 16)
    p, _ = tsne.affinities_host(ids, sims, 5.0)
    g = tsne.joint_probabilities(ids, p)
    row_start, nbr, big = C.joint(ids, p)
    assert np.array_equal(g.row_start, row_start) and np.array_equal(g.nbr, nbr) and same_bits(g.P, big)
    src = np.repeat(np.arange(257), np.diff(g.row_start))
    both = {(int(i), int(j)): C.bits(v) for i, j, v in zip(src, g.nbr, g.P)}
    assert all(both[(j, i)] == v for (i, j), v in both.items())                         # both directions, the same bits
    for i in range(257):
        assert (np.diff(g.nbr[g.row_start[i]:g.row_start[i + 1]]) > 0).all()            # rows ascend
    assert g.row_start[1] - g.row_start[0] > 0                                           # row 0 lists nobody but is listed
    rows_with_p = (p.sum(axis=1) > 0).sum()
    # sum P = (rows whose p sums to 1) / N, each row sum within float32 rounding of its k terms
    assert abs(g.P.astype(np.float64).sum() - rows_with_p / 257) < 257 * 17 * 2.0 ** -24 / 257


# ---------------------------------------------------------------------------------------------------- refusals
def test_argument_errors_without_a_device():
    lib = _lib.load()
    p = lambda a: a.ctypes.data
    n, k = 6, 4
    ids = np.tile(np.arange(1, k + 1, dtype=np.int32), (n, 1)) % n
    sims = np.full((n, k), 0.5, np.float32)
    out, beta = np.full((n, k), 9, np.float32), np.full(n, 9, np.float32)
    row_start = np.arange(n + 1, dtype=np.int64) * k
    y = np.zeros((n, 2), np.float32)
    nine = np.full((n, 2), 9, np.float32)
    z = np.full(n, 9, np.float32)
    ws = np.zeros(int(lib.bd_tsne_workspace_bytes(n)) + 16, np.uint8)
    wsp = (p(ws) + 15) // 16 * 16
    nbytes = int(lib.bd_tsne_workspace_bytes(n))
    assert lib.bd_tsne_workspace_bytes(-1) < 0 and lib.bd_tsne_workspace_bytes((1 << 20) + 1) < 0 and nbytes > 0
    for host in (True, False):
        tail = () if host else (None,)
        aff = lib.bd_tsne_affinities_host if host else lib.bd_tsne_affinities
        good = dict(ids=p(ids), sims=p(sims), rows=n, k=k, perplexity=2.0, p=p(out), beta=p(beta))
        for over, text in ((dict(k=0), "k = 0"), (dict(k=65), "k = 65"), (dict(rows=-1), "rows = -1"), (dict(rows=(1 << 20) + 1), "rows ="),
                           (dict(perplexity=0.5), "perplexity"), (dict(perplexity=float("nan")), "perplexity"),
                           (dict(ids=None), "ids is null"), (dict(sims=p(sims) + 2), "sims is not 4-byte aligned"),
                           (dict(p=None), "p is null"), (dict(beta=None), "beta is null")):
            assert aff(*{**good, **over}.values(), *tail) < 0 and text in lib.bd_last_error().decode(), text
        assert (out == 9).all() and (beta == 9).all()
        att = lib.bd_tsne_attract_host if host else lib.bd_tsne_attract
        good = dict(row_start=p(row_start), nbr=p(ids), P=p(sims), rows=n, edges=n * k, y=p(y), attr=p(nine))
        for over, text in ((dict(edges=-1), "edges = -1"), (dict(rows=-3), "rows = -3"), (dict(row_start=None), "row_start is null"),
                           (dict(row_start=p(row_start) + 4), "row_start is not 8-byte aligned"), (dict(nbr=None), "nbr is null"),
                           (dict(P=None), "p is null"), (dict(y=p(y) + 4), "y is not 8-byte aligned"), (dict(attr=None), "attr is null")):
            assert att(*{**good, **over}.values(), *tail) < 0 and text in lib.bd_last_error().decode(), text
        rep_args = (dict(y=p(y), rows=n, rep=p(nine), z=p(z)) if host else
                    dict(y=p(y), rows=n, rep=p(nine), z=p(z), ws=wsp, nbytes=nbytes))
        rep = lib.bd_tsne_repulse_host if host else lib.bd_tsne_repulse
        cases = [(dict(rows=-1), "rows = -1"), (dict(y=None), "y is null"), (dict(rep=p(nine) + 4), "rep is not 8-byte aligned"),
                 (dict(z=None), "z is null")]
        if not host:
            cases += [(dict(ws=None), "workspace is null"), (dict(ws=wsp + 4), "workspace is not 16-byte aligned"),
                      (dict(nbytes=nbytes - 1), "workspace_bytes")]
        for over, text in cases:
            assert rep(*{**rep_args, **over}.values(), *tail) < 0 and text in lib.bd_last_error().decode(), text
        upd = lib.bd_tsne_update_host if host else lib.bd_tsne_update
        good = dict(y=p(nine), v=p(nine), gain=p(nine), attr=p(y), rep=p(y), z=p(z), rows=n, ex=1.0, mom=0.5, rate=50.0, floor=0.01,
                    total=None)
        if not host:
            good.update(ws=wsp, nbytes=nbytes)
        cases = [(dict(rows=-1), "rows = -1"), (dict(y=None), "y is null"), (dict(v=None), "v is null"), (dict(gain=None), "gain is null"),
                 (dict(attr=None), "attr is null"), (dict(rep=None), "rep is null"), (dict(z=None), "z is null")]
        if not host:
            cases += [(dict(nbytes=16), "workspace_bytes"), (dict(ws=None), "workspace is null")]
        for over, text in cases:
            assert upd(*{**good, **over}.values(), *tail) < 0 and text in lib.bd_last_error().decode(), text
        kl = np.full(1, 9, np.float32)
        div = lib.bd_tsne_kl_host if host else lib.bd_tsne_kl
        good = dict(row_start=p(row_start), nbr=p(ids), P=p(sims), rows=n, edges=n * k, y=p(y), z=p(z), kl=p(kl))
        if not host:
            good.update(ws=wsp, nbytes=nbytes)
        for over, text in ((dict(edges=-1), "edges = -1"), (dict(z=None), "z is null"), (dict(kl=None), "kl is null"), (dict(y=None), "y is null")):
            assert div(*{**good, **over}.values(), *tail) < 0 and text in lib.bd_last_error().decode(), text
        assert (nine == 9).all() and (z == 9).all() and (kl == 9).all()
    # the host restatements look at the graph before they walk it
    rc = lib.bd_tsne_attract_host(p(row_start), p(ids), p(sims), n, n * k - 1, p(y), p(nine))
    assert _lib.ERROR_NAMES[rc] == "BD_ERANGE"
    assert "not from 0 to edges" in lib.bd_last_error().decode()
    bad = ids.copy()
    bad[1, 1] = n
    assert lib.bd_tsne_attract_host(p(row_start), p(bad), p(sims), n, n * k, p(y), p(nine)) < 0
    assert "nbr[5] = 6 is no row" in lib.bd_last_error().decode()
    down = row_start.copy()
    down[3] = 1
    assert lib.bd_tsne_kl_host(p(down), p(ids), p(sims), n, n * k, p(y), p(z), p(kl)) < 0
    assert "does not ascend" in lib.bd_last_error().decode() and (nine == 9).all()


def test_schedule_refusals():
    s = tsne.Schedule()
    assert (s.perplexity, s.early_exaggeration, s.exaggeration_iter, s.n_iter, s.momentum, s.learning_rate, s.min_gain) == \
        (16, 12, 250, 750, (0.5, 0.8), "auto", 0.01)
    assert s.rate(1025) == 50.0 and s.rate(48000) == 1000.0
    assert s.at(249) == (12.0, 0.5) and s.at(250) == (1.0, 0.8)
    s.check_k(48)
    with pytest.raises(ValueError, match="3 x perplexity"):
        s.check_k(47)
    with pytest.raises(ValueError, match="at most 64"):
        tsne.Schedule(perplexity=2).check_k(65)
    for bad in (dict(perplexity=0.5), dict(perplexity=float("nan")), dict(early_exaggeration=0.0), dict(n_iter=100), dict(n_iter=-1),
                dict(exaggeration_iter=-1), dict(momentum=(0.5, 1.0)), dict(momentum=(0.5,)), dict(learning_rate=0.0),
                dict(learning_rate=float("inf")), dict(min_gain=0.0)):
        with pytest.raises(ValueError):
            tsne.Schedule(**bad)
    with pytest.raises(ValueError, match=r"\[N, 2\]"):
        tsne.repulse_host(np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError, match="rows"):
        tsne.attract_host(tsne.JointGraph(np.zeros(3, np.int64), [], []), np.zeros((3, 2), np.float32))


# ---------------------------------------------------------------------------------------------------- rows left out
def test_leave_out_compacts_the_lists():
    n, k = 12, 3
    ids = np.stack([(np.arange(1, k + 1) + i) % n for i in range(n)]).astype(np.int32)
    sims = np.full((n, k), 0.5, np.float32)
    init = np.random.default_rng(1).normal(size=(n, 2)).astype(np.float32)
    init[4, 1] = np.nan                                  # no finite start
    ids[7], sims[7] = -1, 0.0                            # no neighbour, and ...
    ids[ids == 7] = -1                                   # ... in nobody's list
    sims[9] = np.nan                                     # no usable neighbour, but rows 6 and 8 list it: it stays
    keep, ids_c, sims_c, messages = tsne.leave_out(ids, sims, init)
    assert np.flatnonzero(~keep).tolist() == [4, 7] and len(messages) == 2 and "1 windows" in messages[0]
    assert ids_c.shape == (10, k) and sims_c.shape == (10, k)
    old = np.flatnonzero(keep)
    for row, i in enumerate(old):
        want = [int(np.flatnonzero(old == j)[0]) if j >= 0 and j not in (4, 7) else -1 for j in ids[i]]
        assert ids_c[row].tolist() == want
    # a row that only the NaN row listed, and that lists only it, goes too
    ids2 = ids.copy()
    ids2[3] = (4, -1, -1)
    ids2[ids2 == 3] = -1
    ids2[4] = (3, 5, 6)
    keep2, _, _, _ = tsne.leave_out(ids2, sims, init)
    assert not keep2[3] and not keep2[4]
    keep3, ids3, _, none = tsne.leave_out(ids[:0], sims[:0], init[:0])
    assert keep3.shape == (0,) and ids3.shape == (0, k) and none == []


# ---------------------------------------------------------------------------------------------------- results
def result_case(n=7):
    rng = np.random.default_rng(3)
    ids = np.stack([rng.permutation(np.delete(np.arange(n), i))[:3] for i in range(n)]).astype(np.int32)
    sims = rng.random((n, 3)).astype(np.float32)
    recording_of = np.array([0, 0, 0, 1, 1, 1, 1])
    starts = np.array([0.0, 0.96, 1.92, 0.0, 0.96, 1.92, 2.88])
    graph = KnnGraph(ids, sims, ["a", "site/b"], recording_of, starts)
    coords = rng.normal(size=(n, 2)).astype(np.float32)
    coords[5] = np.nan
    return tsne.LayoutResult(coords, 0.75, graph, ["a", "site/b"], recording_of, starts, ["1 windows have no finite start"])


def test_to_csv_save_and_load(tmp_path):
    import csv
    from types import SimpleNamespace
    found = result_case()
    path = str(tmp_path / "layout.csv")
    found.to_csv(path)
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["ident", "start", "end", "x", "y"] and len(rows) == 8
    assert rows[2] == ["a", "0.96", "1.92", repr(float(found.coords[1, 0])), repr(float(found.coords[1, 1]))]
    assert rows[6][3:] == ["nan", "nan"]
    found.to_csv(path, clusters=SimpleNamespace(labels=np.arange(7)))
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0][-1] == "cluster" and [r[-1] for r in rows[1:]] == [str(i) for i in range(7)]
    with pytest.raises(ValueError, match="not the same walk"):
        found.to_csv(path, clusters=SimpleNamespace(labels=np.arange(6)))
    found.clusters = SimpleNamespace(labels=np.arange(7, dtype=np.int32))
    saved = str(tmp_path / "layout.npz")
    found.save(saved)
    back = tsne.LayoutResult.load(saved)
    assert same_bits(back.coords, found.coords) and back.kl == found.kl and back.recordings == found.recordings
    assert np.array_equal(back.recording_of, found.recording_of) and np.array_equal(back.starts, found.starts)
    assert back.messages == found.messages and np.array_equal(back.clusters.labels, np.arange(7))
    assert np.array_equal(back.graph.ids, found.graph.ids) and same_bits(back.graph.sims, found.graph.sims)
    with np.load(saved, allow_pickle=False) as z:                                        # no pickle inside
        assert all(z[name].dtype != object for name in z.files)
    # the result's own preservation is the test module's on the windows that are on the map
    on = np.isfinite(found.coords).all(axis=1)
    remap = np.full(7, -1)
    remap[on] = np.arange(on.sum())
    ids_on = np.where(found.graph.ids[on] >= 0, remap[found.graph.ids[on]], -1)
    want = []
    near = np.argsort(((found.coords[on][:, None] - found.coords[on][None]) ** 2).sum(axis=2) + np.diag(np.full(6, np.inf)), axis=1)[:, :2]
    for i in range(6):
        best = found.graph.ids[on][i, :2]
        want.append(np.isin(remap[best], near[i]).sum() / 2)
    assert found.preservation(k=2) == pytest.approx(np.mean(want))
    assert ids_on.shape == (6, 3)


# ---------------------------------------------------------------------------------------------------- the whole loop
def test_fit_host_quality_against_golden_and_pca():
    g = golden()["513x32"]
    e, truth, ids, sims = propagate_cases.planted_lists(513, 32, 48)
    schedule = tsne.Schedule(perplexity=16, exaggeration_iter=100, n_iter=250)
    schedule.check_k(48)
    p, _ = tsne.affinities_host(ids, sims, 16.0)
    joint = tsne.joint_probabilities(ids, p)
    plane = C.pca_plane(e)
    y, kl, history = tsne.fit_host(joint, C.start_of(plane), schedule, report_every=125)
    purity, kept = C.purity10(y, truth), C.preservation(y, ids)
    m_purity = max(8 * abs(g["float32"]["purity10"] - g["float64"]["purity10"]), 0.01)
    m_kept = max(8 * abs(g["float32"]["preservation"] - g["float64"]["preservation"]), 0.01)
    r = max(8 * abs(g["float32"]["kl"] - g["float64"]["kl"]) / g["float64"]["kl"], 0.01)
    print(f"fit_host 513: purity {purity} (golden {g['float64']['purity10']}, margin {m_purity}), preservation {kept} "
          f"(golden {g['float64']['preservation']}, margin {m_kept}), kl {kl} (golden {g['float64']['kl']}, r {r})")
    assert np.isfinite(y).all() and abs(y.astype(np.float64).mean(axis=0)).max() <= 64 * np.abs(y).max() * 2.0 ** -24
    assert purity >= g["float64"]["purity10"] - m_purity
    assert kept >= g["float64"]["preservation"] - m_kept
    assert kl <= g["float64"]["kl"] * (1 + r)
    assert purity > C.purity10(plane, truth) and kept > C.preservation(plane, ids)      # strictly above the PCA plane
    assert [it for it, _ in history] == [125, 250] and history[-1][1] == float(kl)
    assert float(kl) == pytest.approx(float(C.kl(joint.row_start, joint.nbr, joint.P, y, np.float64)), rel=1e-4)
