"""The host side of label propagation (include/buzzdetect_propagate.h, buzzdetect_amd/propagate.py), no device needed: the
weights, a step and the read-out against independent NumPy loops in every bit (tests/propagate_cases.py), what is refused, and
the results' files."""
import os
import re

import numpy as np
import pytest

from buzzdetect_amd import _lib, dataset, propagate
from tests import propagate_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = (1, 2, 13, 64)


def test_prototypes_are_the_header():
    with open(os.path.join(ROOT, "include", "buzzdetect_propagate.h")) as f:
        header = f.read()
    names = sorted(re.findall(r"^BD_API [^;(]*?(bd_\w+)\(", header, re.M))
    assert names == sorted(_lib.PROPAGATE_PROTOTYPES) and len(names) == 7
    for name in names:
        args = re.search(r"BD_API [^;(]*?" + name + r"\(([^;]*)\);", header).group(1)
        n_args = 0 if args.strip() == "void" else args.count(",") + 1
        assert len(_lib.PROPAGATE_PROTOTYPES[name][1]) == n_args, name
    assert _lib.load().bd_propagate_abi_version() == _lib.PROPAGATE_ABI_VERSION == 1
    for word, value in (("BD_PROPAGATE_MAX_CLASSES", _lib.PROPAGATE_MAX_CLASSES), ("BD_PROPAGATE_MAX_POWER", _lib.PROPAGATE_MAX_POWER),
                        ("BD_PROPAGATE_SLICE", _lib.PROPAGATE_SLICE)):
        assert int(re.search(r"#define " + word + r" (\d+)", header).group(1)) == value
    assert "#define BD_PROPAGATE_MAX_ROWS (1 << 24)" in header and _lib.PROPAGATE_MAX_ROWS == 1 << 24


@pytest.mark.parametrize("power", (1, 2, 4, 16))
def test_weights_equal_numpy_in_every_bit(power):
    rng = np.random.default_rng(power)
    sims = rng.uniform(-0.2, 1.0, size=(37, 16)).astype(np.float32)
    sims[0, :4] = [np.nan, -np.inf, np.inf, -0.0]
    ids = rng.integers(0, 37, size=(37, 16)).astype(np.int32)
    ids[5, 9:], ids[6, :] = -1, -1                                       # empty slots: the row itself, weight 0
    nbr, w = propagate.weights_host(ids, sims, power)
    want_nbr, want_w = cases.weights_numpy(ids, sims, power)
    assert nbr.tobytes() == want_nbr.tobytes() and w.tobytes() == want_w.tobytes()
    assert (nbr[6] == 6).all() and (w[6] == 0).all() and w[0, 0] == 0 and w[0, 1] == 0 and np.isinf(w[0, 2])
    assert (w >= 0).all()


@pytest.mark.parametrize("classes", CLASSES)
def test_step_equals_numpy_in_every_bit(classes):
    row_start, nbr, w, f_in, y, alpha = cases.graph_case(classes)
    assert np.diff(row_start)[:3].tolist() == [0, 1, 300] and set(alpha.tolist()) == {0.0, 0.25, 1.0}
    out, delta = propagate.step_host(row_start, nbr, w, f_in, y, alpha)
    want, want_delta = cases.step_numpy(row_start, nbr, w, f_in, y, alpha)
    assert out.tobytes() == want.tobytes() and delta.tobytes() == want_delta.tobytes() and delta.shape == (2,)
    assert (out[alpha == 0] == y[alpha == 0]).all()                      # a clamped row is its label
    assert (out[0] == 0).all() or alpha[0] != 1                          # degree 0, unlabelled: nothing arrives
    f_in[7, 0] = np.nan                                                  # a NaN moves infinitely far
    _, delta = propagate.step_host(row_start, nbr, w, f_in, y, alpha)
    assert np.isinf(delta[0])


@pytest.mark.parametrize("classes", CLASSES)
def test_readout_equals_numpy_in_every_bit(classes):
    _, _, _, f, _, _ = cases.graph_case(classes, seed=5)
    f[6] = np.nan
    f[8, 0] = np.inf
    if classes > 1:
        f[9] = 0.0
        f[9, classes - 1] = 0.5                                          # one class only: confidence and margin 1
        f[10, :] = 0.125
        f[10, 0] = np.nan                                                # a NaN class never wins, and the reach is not finite
    got = propagate.readout_host(f)
    want = cases.readout_numpy(f)
    for g, w_ in zip(got, want):
        assert g.tobytes() == w_.tobytes()
    reach, label, confidence, margin = got
    assert label[4] == -1 and reach[4] == 0 and confidence[4] == 0 and margin[4] == 0       # an all-zero row
    assert label[5] == 0 and (margin[5] == 0 or classes == 1)            # a tie goes to the lower class
    assert label[6] == -1 and label[8] == -1
    assert label.max() < classes and ((label >= 0) == (np.isfinite(reach) & (reach != 0))).all()
    if classes > 1:
        assert label[9] == classes - 1 and confidence[9] == 1 and margin[9] == 1 and label[10] == -1


def test_steps_converge_on_a_chain():
    """0 - 1 - 2 - 3 - 4 in a row, the ends labelled with different classes: the harmonic solution is linear in the position."""
    ids = np.array([[1, -1], [0, 2], [1, 3], [2, 4], [3, -1]], np.int32)
    nbr, w = propagate.weights_host(ids, np.ones((5, 2), np.float32), 4)
    y, alpha = propagate.targets_of([0, 4], [0, 1], 5, 2)
    f = y.copy()
    for _ in range(200):
        f, delta = propagate.step_host(np.arange(6) * 2, nbr, w, f, y, alpha)
    assert delta.max() < 1e-6
    assert np.abs(f[:, 1] - np.arange(5) / 4).max() < 1e-4 and np.abs(f.sum(axis=1) - 1).max() < 1e-5
    reach, label, confidence, margin = propagate.readout_host(f)
    assert label.tolist() == [0, 0, 0, 1, 1] or label.tolist() == [0, 0, 1, 1, 1]


def test_limits_are_refused_with_the_argument_named():
    lib = _lib.load()
    n, c, k = 6, 3, 2
    ids, sims = np.zeros((n, k), np.int32), np.ones((n, k), np.float32)
    nbr, w = np.full((n, k), 9, np.int32), np.full((n, k), 9, np.float32)
    p = lambda x: None if x is None else x.ctypes.data
    for host in (True, False):
        weights = lib.bd_propagate_weights_host if host else lib.bd_propagate_weights
        tail = () if host else (None,)
        for args, text in (((p(ids), p(sims), n, 0, 4, p(nbr), p(w)), "k = 0"), ((p(ids), p(sims), n, 65, 4, p(nbr), p(w)), "k = 65"),
                           ((p(ids), p(sims), n, k, 0, p(nbr), p(w)), "power = 0"), ((p(ids), p(sims), n, k, 17, p(nbr), p(w)), "power = 17"),
                           ((p(ids), p(sims), -1, k, 4, p(nbr), p(w)), "rows = -1"), ((None, p(sims), n, k, 4, p(nbr), p(w)), "ids is null"),
                           ((p(ids), None, n, k, 4, p(nbr), p(w)), "sims is null"), ((p(ids), p(sims), n, k, 4, None, p(w)), "nbr is null"),
                           ((p(ids), p(sims), n, k, 4, p(nbr), None), "w is null")):
            assert weights(*args, *tail) < 0 and text in lib.bd_last_error().decode(), text
        assert (nbr == 9).all() and (w == 9).all()
        row_start = np.arange(n + 1, dtype=np.int64) * k
        f_in, y, alpha = np.zeros((n, c), np.float32), np.zeros((n, c), np.float32), np.ones(n, np.float32)
        f_out, delta = np.full((n, c), 9, np.float32), np.full(1, 9, np.float32)
        step = lib.bd_propagate_step_host if host else lib.bd_propagate_step
        good = dict(row_start=p(row_start), nbr=p(ids), w=p(sims), rows=n, edges=n * k, f_in=p(f_in), y=p(y), alpha=p(alpha), classes=c,
                    f_out=p(f_out), delta=p(delta))
        for over, text in ((dict(classes=0), "classes = 0"), (dict(classes=65), "classes = 65"), (dict(edges=-1), "edges = -1"),
                           (dict(rows=(1 << 24) + 1), "rows ="), (dict(row_start=None), "row_start is null"),
                           (dict(row_start=p(row_start) + 4), "row_start is not 8-byte aligned"), (dict(nbr=None), "nbr is null"),
                           (dict(w=None), "w is null"), (dict(f_in=None), "f_in is null"), (dict(y=None), "y is null"),
                           (dict(alpha=None), "alpha is null"), (dict(f_out=None), "f_out is null"), (dict(delta=None), "delta is null"),
                           (dict(f_out=p(f_in)), "f_out is f_in")):
            assert step(*{**good, **over}.values(), *tail) < 0 and text in lib.bd_last_error().decode(), text
        assert (f_out == 9).all() and (delta == 9).all()
        reach, label = np.full(n, 9, np.float32), np.full(n, 9, np.int32)
        readout = lib.bd_propagate_readout_host if host else lib.bd_propagate_readout
        good = dict(f=p(f_in), rows=n, classes=c, reach=p(reach), label=p(label), confidence=p(reach), margin=p(reach))
        for over, text in ((dict(classes=0), "classes = 0"), (dict(classes=65), "classes = 65"), (dict(rows=-2), "rows = -2"),
                           (dict(f=None), "f is null"), (dict(reach=None), "reach is null"), (dict(label=None), "label is null"),
                           (dict(confidence=None), "confidence is null"), (dict(margin=None), "margin is null")):
            assert readout(*{**good, **over}.values(), *tail) < 0 and text in lib.bd_last_error().decode(), text
        assert (reach == 9).all() and (label == 9).all()
    # the host restatement looks at the graph before it walks it
    bad = ids.copy()
    bad[2, 1] = n
    f_out = np.full((n, c), 9, np.float32)
    assert lib.bd_propagate_step_host(p(row_start), p(bad), p(sims), n, n * k, p(f_in), p(y), p(alpha), c, p(f_out), p(delta)) < 0
    assert "nbr[5] = 6 is no row" in lib.bd_last_error().decode() and (f_out == 9).all()
    down = row_start.copy()
    down[3] = 1
    assert lib.bd_propagate_step_host(p(down), p(ids), p(sims), n, n * k, p(f_in), p(y), p(alpha), c, p(f_out), p(delta)) < 0
    assert "does not ascend" in lib.bd_last_error().decode()
    with pytest.raises(ValueError, match="power"):
        propagate.Propagator(power=17)
    with pytest.raises(ValueError, match="clamp"):
        propagate.targets_of([0], [0], 4, 2, clamp=0.0)
    with pytest.raises(ValueError, match="out of range"):
        propagate.targets_of([4], [0], 4, 2)


def test_result_files(tmp_path):
    n = 6
    res = propagate.PropagationResult(
        labels=np.array([0, 1, -1, 1, 0, 1], np.int32), confidence=np.array([1, 0.95, 0, 0.6, 0.99, 0.92], np.float32),
        margin=np.array([1, 0.9, 0, 0.2, 0.98, 0.84], np.float32), reach=np.array([1, 0.8, 0, 0.9, 0.3, 0.7], np.float32),
        scores=np.zeros((n, 2), np.float32), iterations=7, classes=["ambient", "ins_buzz"],
        annotated=np.array([True, False, False, False, False, False]), recordings=["a", "site/b"],
        recording_of=np.array([0, 0, 0, 1, 1, 1]), starts=np.array([0.0, 0.96, 1.92, 0.0, 0.96, 1.92]))
    path = str(tmp_path / "p.csv")
    res.to_csv(path)
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0] == "ident,start,end,label,confidence,margin,reach" and len(lines) == 7
    assert lines[2].startswith("a,0.96,1.92,ins_buzz,0.949999") and lines[3].startswith("a,1.92,2.88,,0.0,0.0,0.0")
    out = str(tmp_path / "more.csv")
    rows = res.annotations(path=out)                                     # 0 was annotated, 3 is unsure, 4 was hardly reached
    assert rows == [("a", 0.96, 1.92, "ins_buzz"), ("site/b", 1.92, 2.88, "ins_buzz")]
    assert dataset.read_annotations(out) == {"a": [(0.96, 1.92, "ins_buzz")], "site/b": [(1.92, 2.88, "ins_buzz")]}
    assert [r[0] for r in res.annotations(min_confidence=0.5, min_reach=0.2)] == ["a", "site/b", "site/b", "site/b"]
    assert "not tuned" in propagate.PropagationResult.annotations.__doc__
