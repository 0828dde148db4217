"""The neighbour-preserving map on the GPU (csrc/tsne.hip, buzzdetect_amd/tsne.py): repulsion, attraction and update against
their host restatements in every bit on the constructed cases of tests/tsne_cases.py, the affinities and the divergence against
float64 under the 8 x rule, thirty iterations of TSNE.fit against fit_host in every bit, the quality on the planted partition
against the golden file and the PCA plane, and the rows left out.  Every buffer a kernel writes comes from
tests/gpu_guards.Guarded, and every output word is written."""
import json
import os

import numpy as np
import pytest

from buzzdetect_amd import _lib, tsne
from tests import propagate_cases, tsne_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLICE, BLOCK = _lib.TSNE_SLICE, _lib.TSNE_ROWS_PER_BLOCK
REPULSE_SIZES = (1, 2, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 1025, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 3)


def guarded():
    from tests.gpu_guards import Guarded
    return Guarded("cuda")


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    return C.bits(a).tobytes() == C.bits(b).tobytes()


def workspace(g, n):
    """Exactly the bytes the library asks for, full of NaNs: nothing may be read before it is written."""
    import torch
    from tests.gpu_guards import NAN
    nbytes = _lib.check(_lib.load().bd_tsne_workspace_bytes(n))
    return g.empty((nbytes,), torch.uint8, fill=NAN, name="workspace"), nbytes


def dev_repulse(g, y):
    import torch
    n = y.shape[0]
    rep, z = g.empty((n, 2), torch.float32, name="rep"), g.empty((n,), torch.float32, name="z")
    ws, nbytes = workspace(g, n)
    y_dev = upload(y)
    _lib.check(_lib.load().bd_tsne_repulse(y_dev.data_ptr(), n, rep.data_ptr(), z.data_ptr(), ws.data_ptr(), nbytes, stream()))
    torch.cuda.synchronize()
    return rep.cpu().numpy(), z.cpu().numpy()


class GuardedTSNE(tsne.TSNE):
    """Every buffer of a fit between guard words; the workspace starts as NaNs."""
    guards = None

    def _guards(self):
        from tests.gpu_guards import Guarded
        if GuardedTSNE.guards is None:
            GuardedTSNE.guards = Guarded("cuda")
        return GuardedTSNE.guards

    def _empty(self, shape, dtype):
        return self._guards().empty(shape, dtype, name=f"{tuple(shape)} {dtype}")

    def _workspace(self, nbytes):
        import torch
        from tests.gpu_guards import NAN
        return self._guards().empty((max(int(nbytes), 16),), torch.uint8, fill=NAN, name="workspace")


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "tsne_quality.json")) as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("n", REPULSE_SIZES)
def test_repulse_equals_the_host_restatement(n):
    g = guarded()
    for scale in C.SCALES:
        y = C.coords(n, scale)
        rep, z = dev_repulse(g, y)
        want_rep, want_z = tsne.repulse_host(y)
        assert same_bits(rep, want_rep) and same_bits(z, want_z), scale
        if n > 8:
            assert z[0] >= 2 and np.isfinite(rep).all()                 # coincident points: q = 1, no force, counted in z
    g.check()


def test_the_block_a_row_falls_in_does_not_matter():
    """Rows at the same place in different workgroups' blocks walk the same candidates: their forces have the same bits (their z
    may differ: each leaves out itself, at another point of the chain)."""
    n = 4 * BLOCK + 1
    y = C.coords(n, "converged", special=False)
    for block in range(1, 4):
        y[block * BLOCK + 3] = y[3]
        y[block * BLOCK + 200] = y[70]
    g = guarded()
    rep, z = dev_repulse(g, y)
    g.check()
    for block in range(1, 4):
        assert same_bits(rep[block * BLOCK + 3], rep[3]) and same_bits(rep[block * BLOCK + 200], rep[70])
    assert same_bits(rep, tsne.repulse_host(y)[0])


def test_attract_equals_the_host_restatement():
    import torch
    row_start, nbr, big = C.graph_case()
    g = guarded()
    for scale in C.SCALES:
        y = C.coords(310, scale)
        attr = g.empty((310, 2), torch.float32, name="attr")
        held = [upload(a) for a in (row_start, nbr, big, y)]
        _lib.check(_lib.load().bd_tsne_attract(held[0].data_ptr(), held[1].data_ptr(), held[2].data_ptr(), 310, nbr.shape[0],
                                               held[3].data_ptr(), attr.data_ptr(), stream()))
        got = attr.cpu().numpy()
        assert same_bits(got, tsne.attract_host(tsne.JointGraph(row_start, nbr, big), y)), scale
        assert (got[0] == 0).all()
    g.check()


@pytest.mark.parametrize("n", (11, 1025, 2 * SLICE + 3))
def test_update_equals_the_host_restatement(n):
    import torch
    y, v, gain, attr, rep, z = C.update_case(n)
    g = guarded()
    for exaggeration, momentum in ((12.0, 0.5), (1.0, 0.8)):
        state = [g.empty((n, 2), torch.float32, name=name) for name in ("y", "v", "gain")]
        for t, a in zip(state, (y, v, gain)):
            t.copy_(upload(a))
        total = g.empty((1,), torch.float32, name="total")
        ws, nbytes = workspace(g, n)
        held = [upload(a) for a in (attr, rep, z)]
        _lib.check(_lib.load().bd_tsne_update(*(t.data_ptr() for t in state), *(t.data_ptr() for t in held), n, exaggeration, momentum,
                                              50.0, 0.01, total.data_ptr(), ws.data_ptr(), nbytes, stream()))
        want = tsne.update_host(y, v, gain, attr, rep, z, exaggeration, momentum, 50.0)
        for t, b, name in zip(state + [total], want, ("y", "v", "gain", "Z")):
            assert same_bits(t.cpu().numpy(), b), name
    g.check()


# ---------------------------------------------------------------------------------------------------- the 8 x rule
@pytest.mark.parametrize("k", (1, 16, 48, 64))
def test_affinities_and_kl_under_the_8x_rule(k):
    """Deviation from the float64 statement at most 8 x the plain float32 NumPy statement's; the affinities are rule-bound, not
    bit-equal to the host restatement.  Observed on an MI355X, device over NumPy float32, for k = 1, 16, 48, 64:
    affinities 0 / 0, 1.05, 1.39, 1.36; the achieved perplexity's miss -, 1.03, 1.07, 1.21; the divergence 2.1, 1.0, 0.84, 1.0."""
    import torch
    n = 1025
    perplexity = min(16.0, max(1.0, float(k // 3)))
    ids, sims = C.lists_case(n, k)
    g = guarded()
    t = GuardedTSNE(tsne.Schedule(perplexity=perplexity))
    p, beta = t.affinities(ids, sims)
    p64, _ = C.affinities(ids, sims, perplexity, np.float64)
    p32, _ = C.affinities(ids, sims, perplexity, np.float32)
    ok = C.usable(ids, sims)
    assert np.isfinite(p).all() and (p[~ok] == 0).all() and (p[0] == 0).all() and beta[0] == 0
    err, err32 = np.abs(p - p64).max(), np.abs(p32 - p64).max()
    print(f"affinities k={k}: device {err:.3e}, NumPy float32 {err32:.3e}, ratio {err / err32 if err32 else 0:.2f}")
    assert err <= 8 * err32
    reachable = ok.sum(axis=1) > perplexity
    reachable[2] = False                                 # all duplicates: d = 0 everywhere, the perplexity is the count
    if reachable.any():
        miss = np.abs(C.perplexity_of(p)[reachable] - perplexity).max()
        miss32 = np.abs(C.perplexity_of(p32)[reachable] - perplexity).max()
        print(f"perplexity k={k}: device misses by {miss:.3e}, NumPy float32 by {miss32:.3e}, ratio {miss / miss32:.2f}")
        assert miss <= 8 * miss32
    host_p, _ = tsne.affinities_host(ids, sims, perplexity)
    print(f"affinities k={k}: device against the host restatement {np.abs(p - host_p).max():.3e}")

    joint = tsne.joint_probabilities(ids, p)
    y = C.coords(n, "converged", special=False)
    _, z = tsne.repulse_host(y)
    kl = g.empty((1,), torch.float32, name="kl")
    ws, nbytes = workspace(g, n)
    held = [upload(a) for a in (joint.row_start, joint.nbr, joint.P, y, z)]
    edges = joint.n_edges
    _lib.check(_lib.load().bd_tsne_kl(held[0].data_ptr(), held[1].data_ptr() if edges else None, held[2].data_ptr() if edges else None,
                                      n, edges, held[3].data_ptr(), held[4].data_ptr(), kl.data_ptr(), ws.data_ptr(), nbytes, stream()))
    got = float(kl.item())
    kl64 = float(C.kl(joint.row_start, joint.nbr, joint.P, y, np.float64))
    kl32 = float(C.kl(joint.row_start, joint.nbr, joint.P, y, np.float32))
    print(f"kl k={k}: device {got!r}, float64 {kl64!r}, NumPy float32 {kl32!r}, host {float(tsne.kl_host(joint, y, z))!r}")
    assert abs(got - kl64) <= 8 * abs(kl32 - kl64)
    g.check()
    GuardedTSNE.guards.check()


# ---------------------------------------------------------------------------------------------------- the loop
@pytest.fixture(scope="module")
def planted():
    """The lists of the (1025, 32) fixture at k = 48, from the host restatement the device lists equal in every bit."""
    return propagate_cases.planted_lists(1025, 32, 48)


@pytest.mark.parametrize("n", (1025, SLICE + 1))
def test_thirty_iterations_equal_fit_host(planted, n):
    if n == 1025:
        e, _, ids, sims = planted
        init = C.start_of(C.pca_plane(e))
    else:
        ids, sims = C.lists_case(n, 48)
        init = C.coords(n, "start", special=False)
    schedule = tsne.Schedule(perplexity=16, exaggeration_iter=15, n_iter=30)
    t = GuardedTSNE(schedule)
    assert t.fit((ids, sims), init, report_every=10) is t.coords
    GuardedTSNE.guards.check()
    keep = t.keep_
    want, want_kl, history = tsne.fit_host(t.joint_, init[keep], schedule, report_every=10)
    assert same_bits(t.coords[keep], want) and np.isnan(t.coords[~keep]).all()
    assert [it for it, _ in t.kl_history] == [10, 20, 30] == [it for it, _ in history]
    assert t.kl_ == pytest.approx(float(want_kl), rel=1e-4) and t.kl_history[-1][1] == t.kl_
    assert np.isfinite(want).all() and (want != init[keep]).any(axis=1).all()                      # every row moved


def test_twenty_iterations_against_float64():
    n = 310
    ids, sims = C.lists_case(n, 48)
    init = C.coords(n, "start", special=False)
    schedule = tsne.Schedule(perplexity=16, exaggeration_iter=10, n_iter=20)
    t = GuardedTSNE(schedule)
    t.fit((ids, sims), init)
    GuardedTSNE.guards.check()
    keep, j = t.keep_, t.joint_
    y64, _ = C.fit(j.row_start, j.nbr, j.P, init[keep], np.float64, n_iter=20, exaggeration_iter=10)
    y32, _ = C.fit(j.row_start, j.nbr, j.P, init[keep], np.float32, n_iter=20, exaggeration_iter=10)
    err, err32 = np.abs(t.coords[keep] - y64).max(), np.abs(y32 - y64).max()
    print(f"twenty iterations: device {err:.3e}, NumPy float32 {err32:.3e} from float64 (span {np.abs(y64).max():.3e}), "
          f"ratio {err / err32:.2f}")
    assert err <= 8 * err32


@pytest.mark.parametrize("where", ("device", "host"))
def test_quality_on_the_planted_partition(planted, where):
    g = golden()["1025x32"]
    e, truth, ids, sims = planted
    plane = C.pca_plane(e)
    init = C.start_of(plane)
    schedule = tsne.Schedule(perplexity=16, exaggeration_iter=250, n_iter=500)
    if where == "device":
        t = GuardedTSNE(schedule)
        y = t.fit((ids, sims), init)
        GuardedTSNE.guards.check()
        assert t.keep_.all() and t.messages == []
        kl = t.kl_
    else:
        p, _ = tsne.affinities_host(ids, sims, 16.0)
        y, kl, _ = tsne.fit_host(tsne.joint_probabilities(ids, p), init, schedule)
    purity, kept = C.purity10(y, truth), C.preservation(y, ids)
    m_purity = max(8 * abs(g["float32"]["purity10"] - g["float64"]["purity10"]), 0.01)
    m_kept = max(8 * abs(g["float32"]["preservation"] - g["float64"]["preservation"]), 0.01)
    r = max(8 * abs(g["float32"]["kl"] - g["float64"]["kl"]) / g["float64"]["kl"], 0.01)
    print(f"{where} 1025: purity {purity} (golden {g['float64']['purity10']}, margin {m_purity}), preservation {kept} "
          f"(golden {g['float64']['preservation']}, margin {m_kept}), kl {kl} (golden {g['float64']['kl']}, r {r})")
    assert np.isfinite(y).all()
    # the mean is 0 within rounding: the float32 sum of a column errs by at most (32 + 6 + 1) roundings of its partial sums, the
    # subtraction by half an ulp of the span
    assert abs(y.astype(np.float64).mean(axis=0)).max() <= 64 * np.abs(y).max() * 2.0 ** -24
    assert purity >= g["float64"]["purity10"] - m_purity
    assert kept >= g["float64"]["preservation"] - m_kept
    assert float(kl) <= g["float64"]["kl"] * (1 + r)
    assert purity > C.purity10(plane, truth) and kept > C.preservation(plane, ids)                # strictly above the PCA plane


def test_a_row_left_out_changes_nothing_else():
    n = 310
    ids, sims = C.lists_case(n, 48)
    init = C.coords(n, "start", special=False)
    init[17, 0] = np.nan
    schedule = tsne.Schedule(perplexity=16, exaggeration_iter=5, n_iter=10)
    t = GuardedTSNE(schedule)
    t.fit((ids, sims), init)
    keep, ids_c, sims_c, messages = tsne.leave_out(ids, sims, init)
    assert not keep[17] and keep.sum() == n - 1 and t.messages == messages and len(messages) == 1
    without = GuardedTSNE(schedule)
    without.fit((ids_c, sims_c), init[keep])
    GuardedTSNE.guards.check()
    assert without.keep_.all() and without.messages == []
    assert same_bits(t.coords[keep], without.coords) and np.isnan(t.coords[~keep]).all() and np.isfinite(without.coords).all()
    assert t.kl_ == without.kl_
