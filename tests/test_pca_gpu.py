"""The streaming PCA on the GPU (csrc/pca.hip, buzzdetect_amd/pca.py): the column sums, the Gram matrix and the projection
against their host restatements in every bit - for the Gram matrix that is the guide's statement about the exact-f32 matrix
instruction, a k-ordered fmaf chain - and against float64 within 8 x the deviation of the plain float32 statement on the same
data; then PCA.fit / partial_fit / transform on 4096 planted rows against a float64 PCA.  Every buffer a kernel writes comes
from tests/gpu_guards.Guarded: the guard words must stay untouched, every output element must be written, and the workspace
starts as NaNs.

Observed on gfx950 (deviation from float64 over that of the float32 statement; the bound is 8): see DESIGN.md section 31."""
import numpy as np
import pytest

from buzzdetect_amd import _lib, pca, search
from tests import pca_cases as cases

pytestmark = pytest.mark.gpu

DIM = cases.DIM
bits = cases.bits


def guarded():
    from tests.gpu_guards import Guarded
    return Guarded("cuda")


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


@pytest.fixture(scope="module")
def corpus():
    """4096 planted rows on both sides, their squared norms (host restatement, equal to the device's by test_search_gpu), a
    shift near their mean, and the device's norms."""
    import torch
    assert torch.cuda.is_available()
    e, directions = cases.planted(4096, seed=11)
    n2 = search.norms_host(e)
    shift = e[:1000].mean(axis=0).astype(np.float32)
    return dict(e=e, directions=directions, n2=n2, shift=shift, e_dev=upload(e), n2_dev=upload(n2), shift_dev=upload(shift))


def dev_sums(g, e_dev, n2_dev, r, pick_dev=None, shift_dev=None):
    import torch
    partial = g.empty(((r + 255) // 256, DIM), torch.float32, name="partial")
    _lib.check(_lib.load().bd_pca_sums(e_dev.data_ptr(), int(e_dev.shape[0]), ptr(pick_dev), r, n2_dev.data_ptr(), ptr(shift_dev),
                                       partial.data_ptr(), stream()))
    out = partial.cpu().numpy()
    g.check()
    return out


def dev_gram(g, e_dev, n2_dev, r, pick_dev=None, shift_dev=None, into=None, check=True):
    """bd_pca_gram into a guarded matrix (or ``into``, accumulating), its workspace exactly as large as asked for and full of
    NaNs.  Returns (matrix as NumPy, the device tensor)."""
    import torch
    from tests.gpu_guards import NAN
    lib = _lib.load()
    gram = g.empty((DIM, DIM), torch.float32, name="gram") if into is None else into
    ws_bytes = _lib.check(lib.bd_pca_workspace_bytes(r))
    assert ws_bytes == (r + 1023) // 1024 * _lib.PCA_TILES * 1024 * 4
    ws = g.empty((ws_bytes,), torch.uint8, fill=NAN, name="workspace")
    _lib.check(lib.bd_pca_gram(e_dev.data_ptr(), int(e_dev.shape[0]), ptr(pick_dev), r, n2_dev.data_ptr(), ptr(shift_dev),
                               0 if into is None else 1, gram.data_ptr(), ws.data_ptr(), ws_bytes, stream()))
    out = gram.cpu().numpy()
    if check:
        g.check()
    return out, gram


# ---------------------------------------------------------------------------------------------------- sums
@pytest.mark.parametrize("r", (1, 255, 256, 257, 1025))
def test_sums_equal_the_host_restatement_in_every_bit(corpus, r):
    pick = np.sort(np.random.default_rng(r).choice(4096, size=r, replace=False)).astype(np.int32)[::-1].copy()
    for shift, shift_dev in ((None, None), (corpus["shift"], corpus["shift_dev"])):
        got = dev_sums(guarded(), corpus["e_dev"], corpus["n2_dev"], r, upload(pick), shift_dev)
        want = pca.sums_host(corpus["e"], corpus["n2"], shift, pick)
        assert np.array_equal(bits(got), bits(want))


# ---------------------------------------------------------------------------------------------------- gram
@pytest.mark.parametrize("r", (1, 2, 3, 1023, 1024, 1025))
def test_gram_equals_the_fmaf_chains_of_the_host_in_every_bit(corpus, r):
    e_dev, n2_dev = corpus["e_dev"][:r].contiguous(), corpus["n2_dev"][:r].contiguous()
    got, _ = dev_gram(guarded(), e_dev, n2_dev, r, shift_dev=corpus["shift_dev"])
    want = pca.gram_host(corpus["e"][:r], corpus["n2"][:r], corpus["shift"])
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(got), bits(got.T))                       # both triangles, the diagonal tiles' own included


def test_gram_through_a_pick_over_three_slices_twice_and_symmetric(corpus):
    r = 2049
    pick = np.random.default_rng(5).permutation(4096)[:r].astype(np.int32)
    pick_dev = upload(pick)
    got, _ = dev_gram(guarded(), corpus["e_dev"], corpus["n2_dev"], r, pick_dev, corpus["shift_dev"])
    again, _ = dev_gram(guarded(), corpus["e_dev"], corpus["n2_dev"], r, pick_dev, corpus["shift_dev"])
    want = pca.gram_host(corpus["e"], corpus["n2"], corpus["shift"], pick)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(got), bits(again))
    assert np.array_equal(bits(got), bits(got.T))


def test_gram_identity_pick_and_no_shift(corpus):
    r = 1025
    ident = upload(np.arange(r, dtype=np.int32))
    plain, _ = dev_gram(guarded(), corpus["e_dev"], corpus["n2_dev"], r)
    picked, _ = dev_gram(guarded(), corpus["e_dev"], corpus["n2_dev"], r, ident)
    assert np.array_equal(bits(plain), bits(picked))
    assert np.array_equal(bits(plain), bits(pca.gram_host(corpus["e"][:r], corpus["n2"][:r])))


def test_gram_accumulates_halves_as_defined(corpus):
    """Two calls over halves cut at a multiple of 1024: gram_old + T, where each T is its own chain over P_s."""
    g = guarded()
    e, n2, shift = corpus["e"], corpus["n2"], corpus["shift"]
    first, gram = dev_gram(g, corpus["e_dev"][:2048], corpus["n2_dev"][:2048], 2048, shift_dev=corpus["shift_dev"], check=False)
    both, _ = dev_gram(g, corpus["e_dev"][2048:3073].contiguous(), corpus["n2_dev"][2048:3073].contiguous(), 1025,
                       shift_dev=corpus["shift_dev"], into=gram)
    t0 = pca.gram_host(e[:2048], n2[:2048], shift)
    t1 = pca.gram_host(e[2048:3073], n2[2048:3073], shift)
    assert np.array_equal(bits(first), bits(t0))
    assert np.array_equal(bits(both), bits((t0 + t1).astype(np.float32)))
    host = pca.gram_host(e[2048:3073], n2[2048:3073], shift, into=t0.copy())
    assert np.array_equal(bits(both), bits(host))
    assert np.array_equal(bits(both), bits(both.T))


def test_gram_leaves_an_absent_row_out_exactly(corpus):
    r = 1025
    e = corpus["e"][:r].copy()
    e[513, 700] = np.nan
    n2 = search.norms_host(e)
    assert not np.isfinite(n2[513]) and np.isfinite(np.delete(n2, 513)).all()
    got, _ = dev_gram(guarded(), upload(e), upload(n2), r)
    assert np.isfinite(got).all()
    assert np.array_equal(bits(got), bits(pca.gram_host(e, n2)))
    zeroed = e.copy()
    zeroed[513] = 0.0                                                   # fmaf(0, 0, acc) == acc: the row's steps fall out
    assert np.array_equal(bits(got), bits(pca.gram_host(zeroed, search.norms_host(zeroed))))
    sums = dev_sums(guarded(), upload(e), upload(n2), r)
    assert np.array_equal(bits(sums), bits(pca.sums_host(zeroed, search.norms_host(zeroed))))


def test_gram_against_float64_within_the_bound(corpus):
    r = 1025
    e, shift = corpus["e"][:r], corpus["shift"]
    got, _ = dev_gram(guarded(), corpus["e_dev"][:r].contiguous(), corpus["n2_dev"][:r].contiguous(), r, shift_dev=corpus["shift_dev"])
    exact = cases.gram_f64(e, shift)
    statement = np.abs(cases.gram_f32_sequential(e, shift) - exact).max()
    device = np.abs(got - exact).max()
    print(f"gram R={r}: device {device:.3e}, float32 statement {statement:.3e}, ratio {device / statement:.3f}, "
          f"largest entry {np.abs(exact).max():.1f}")
    assert statement > 0
    assert device <= cases.BOUND * statement


# ---------------------------------------------------------------------------------------------------- project
def projection(corpus, d, seed=0):
    """A model of d orthonormal components with a scale per component, as bd_pca_project takes it, on both sides."""
    rng = np.random.default_rng(100 + d + seed)
    q, _ = np.linalg.qr(rng.standard_normal((DIM, d)))
    comps = np.ascontiguousarray(q.T, np.float32)
    mean = corpus["e"].mean(axis=0).astype(np.float32)
    mv = (comps.astype(np.float64) @ mean.astype(np.float64)).astype(np.float32)
    scale = rng.uniform(0.3, 2.0, d).astype(np.float32)
    dev = tuple(upload(a) for a in (search.pack_queries(comps), mv, scale, mean))
    return comps, mean, mv, scale, dev


def dev_project(e_dev, d, dev, residual=True):
    import torch
    g = guarded()
    lib = _lib.load()
    w = int(e_dev.shape[0])
    packed, mv, scale, mean = dev
    y = g.empty((w, d), torch.float32, name="y")
    resid = g.empty((w,), torch.float32, name="resid") if residual else None
    s = g.empty((w, d), torch.float32, name="scores")
    _lib.check(lib.bd_pca_project(e_dev.data_ptr(), w, packed.data_ptr(), d, mv.data_ptr(), scale.data_ptr(), mean.data_ptr(),
                                  y.data_ptr(), ptr(resid), stream()))
    _lib.check(lib.bd_search_scores(e_dev.data_ptr(), w, packed.data_ptr(), d, _lib.SEARCH_METRICS["dot"], None, s.data_ptr(), d, 1,
                                    stream()))
    out = y.cpu().numpy(), None if resid is None else resid.cpu().numpy(), s.cpu().numpy()
    g.check()
    return out


@pytest.mark.parametrize("d", (1, 2, 32, 33, 64))
@pytest.mark.parametrize("w", (1, 31, 32, 33, 1025))
def test_project_equals_the_host_restatement_fed_with_the_search_scores(corpus, w, d):
    comps, mean, mv, scale, dev = projection(corpus, d)
    e = corpus["e"][:w].copy()
    if w >= 33:
        e[w // 2, 5] = np.nan                                           # a NaN row spoils itself alone
    y, resid, s = dev_project(upload(e), d, dev)
    want_y, want_r = pca.project_host(e, s, mv, scale, mean)
    assert np.array_equal(bits(y), bits(want_y)) and np.array_equal(bits(resid), bits(want_r))
    ind_y, ind_r = cases.project_f32(e, s, mv, scale, mean)            # and NumPy's own float32 statement of the header
    assert np.array_equal(bits(y), bits(ind_y)) and np.array_equal(bits(resid), bits(ind_r))
    bad = np.zeros(w, bool)
    if w >= 33:
        bad[w // 2] = True
    assert np.isnan(y[bad]).all() and np.isnan(resid[bad]).all()
    assert np.isfinite(y[~bad]).all() and np.isfinite(resid[~bad]).all() and (resid[~bad] >= 0).all()
    y_only, none, _ = dev_project(upload(e), d, dev, residual=False)    # resid may be null
    assert none is None and np.array_equal(bits(y_only), bits(y))


@pytest.mark.parametrize("d", (2, 64))
def test_project_gives_a_row_the_same_bits_wherever_it_sits(corpus, d):
    _, _, _, _, dev = projection(corpus, d)
    w = 1025
    e = corpus["e"][1000:1000 + w].copy()
    places = (0, 31, 32, w - 1)
    for p in places:
        e[p] = corpus["e"][7]
    y, resid, _ = dev_project(upload(e), d, dev)
    alone_y, alone_r, _ = dev_project(upload(corpus["e"][7:8]), d, dev)
    for p in places:
        assert np.array_equal(bits(y[p]), bits(alone_y[0])) and bits(resid[p:p + 1])[0] == bits(alone_r)[0]


@pytest.mark.parametrize("d", (2, 64))
def test_project_against_float64_within_the_bound(corpus, d):
    comps, mean, mv, scale, dev = projection(corpus, d)
    w = 1025
    e = corpus["e"][:w]
    y, resid, _ = dev_project(corpus["e_dev"][:w].contiguous(), d, dev)
    exact_y, exact_r = cases.project_f64(e, comps, mean, scale)
    # the plain float32 statement of the header's formulas: the dot product and the centred norm summed channel after channel
    f = np.float32
    s32 = np.zeros((w, d), f)
    c32 = np.zeros(w, f)
    for c in range(DIM):
        s32 += np.multiply.outer(e[:, c], comps[:, c])
        x = e[:, c] - mean[c]
        c32 += x * x
    u32 = s32 - mv[None, :]
    st_y = u32 * scale[None, :]
    q32 = np.zeros(w, f)
    for j in range(d):
        q32 += u32[:, j] * u32[:, j]
    st_r = np.fmax(c32 - q32, f(0))
    for name, got, st, exact in (("y", y, st_y, exact_y), ("resid", resid, st_r, exact_r)):
        device, statement = np.abs(got - exact).max(), np.abs(st - exact).max()
        print(f"project d={d} {name}: device {device:.3e}, float32 statement {statement:.3e}, ratio {device / statement:.3f}")
        assert statement > 0 and device <= cases.BOUND * statement


# ---------------------------------------------------------------------------------------------------- PCA
def away(a, b):
    """1 - |cos| of two directions, without the cancellation of 1 - x: |a -+ b|^2 / 2 for unit vectors."""
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    return 0.5 * min(((a - b) ** 2).sum(), ((a + b) ** 2).sum())


@pytest.fixture(scope="module")
def fits(corpus):
    e = corpus["e"]
    exact = cases.pca_reference(e, 4, np.float64)
    single = cases.pca_reference(e, 4, np.float32)
    fitted = pca.PCA(3).fit(corpus["e_dev"])
    return exact, single, fitted


def test_fit_finds_the_planted_components_as_well_as_float32_numpy_does(corpus, fits):
    (comps64, values64), (comps32, values32), fitted = fits
    assert values64[3] < 0.05 * values64[2]                             # the data's own property, in float64 first
    for j in range(3):
        assert away(comps64[j], corpus["directions"][j]) < 1e-2
    assert fitted.n_rows == 4096 and fitted.n_skipped == 0
    for j in range(3):
        statement, device = away(comps32[j], comps64[j]), away(fitted.components[j].astype(np.float64), comps64[j])
        rel32 = abs(values32[j] - values64[j]) / values64[j]
        rel = abs(fitted.explained_variance[j] - values64[j]) / values64[j]
        print(f"component {j}: 1 - |cos| device {device:.3e}, float32 PCA {statement:.3e}; variance device {rel:.3e}, "
              f"float32 PCA {rel32:.3e}")
        assert device <= cases.BOUND * statement
        assert rel <= cases.BOUND * rel32
        v = fitted.components[j]
        assert v[np.argmax(np.abs(v))] > 0                              # the sign rule
    total64 = np.var(corpus["e"].astype(np.float64), axis=0, ddof=1).sum()
    assert np.allclose(fitted.explained_variance_ratio, values64[:3] / total64, rtol=1e-6)
    assert np.isclose(fitted.total_variance, total64, rtol=1e-6)


def test_partial_fit_in_pieces_agrees_and_repeats_in_every_bit(corpus, fits):
    (comps64, _), (comps32, _), fitted = fits
    cuts = (0, 1000, 3000, 4096)

    def pieces():
        p = pca.PCA(3)
        for a, b in zip(cuts, cuts[1:]):
            p.partial_fit(corpus["e_dev"][a:b].contiguous())
        return p.finish()

    one, two = pieces(), pieces()
    assert np.array_equal(bits(one.components), bits(two.components)) and np.array_equal(bits(one.mean), bits(two.mean))
    assert np.array_equal(one.explained_variance, two.explained_variance)
    for j in range(3):
        statement = away(comps32[j], comps64[j])
        assert away(one.components[j].astype(np.float64), comps64[j]) <= cases.BOUND * statement
        assert away(one.components[j].astype(np.float64), fitted.components[j].astype(np.float64)) <= cases.BOUND * statement


def test_fit_rows_is_the_fit_of_those_rows_taken_by_hand(corpus):
    rows = pca.sample_rows(4096, 1024, 3)
    assert rows.shape == (1024,) and np.all(np.diff(rows) > 0)
    sampled = pca.PCA(3).fit(corpus["e_dev"], fit_rows=1024, seed=3)
    by_hand = pca.PCA(3).fit(upload(corpus["e"][rows]))
    assert sampled.n_rows == by_hand.n_rows == 1024
    assert np.array_equal(bits(sampled.components), bits(by_hand.components))
    assert np.array_equal(bits(sampled.mean), bits(by_hand.mean))
    assert np.array_equal(sampled.explained_variance, by_hand.explained_variance)


def test_transform_is_the_projection_kernel_and_skips_no_row(corpus, fits):
    fitted = fits[2]
    e = corpus["e"][:300].copy()
    e[17, 3] = np.inf
    y, resid = fitted.transform(upload(e), residual=True)
    assert y.shape == (300, 3) and resid.shape == (300,)
    assert np.isnan(y[17]).all() and np.isnan(resid[17]) and np.isfinite(np.delete(y, 17, axis=0)).all()
    # (the kernel's accuracy is held to its bound above; here only that transform hands it the model's constants: a wrong
    # mean, mv or component would be off by the size of the coordinates, about 1, not by float32 roundings of sums near 400)
    exact_y, exact_r = cases.project_f64(np.delete(e, 17, axis=0), fitted.components, fitted.mean, np.ones(3, np.float32))
    assert np.abs(np.delete(y, 17, axis=0) - exact_y).max() < 1e-3 and np.abs(np.delete(resid, 17) - exact_r).max() < 1e-2
    white = pca.PCA.from_model(pca.PCAModel(fitted.components, fitted.mean, fitted.explained_variance, fitted.total_variance,
                                            fitted.n_rows, whiten=True))
    yw = white.transform(corpus["e_dev"])
    assert np.allclose(yw.std(axis=0, ddof=1), 1.0, rtol=1e-3)
