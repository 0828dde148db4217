"""Label propagation on the GPU (csrc/propagate.hip, buzzdetect_amd/propagate.py): the weights, a step and the read-out against
their host restatements in every bit - on the constructed cases of tests/propagate_cases.py and on a real graph of 1025 rows,
fixed-k and symmetrised - thirty steps back and forth, Propagator against float64 under the 8 x rule, and the planted partition.
Every buffer a kernel writes comes from tests/gpu_guards.Guarded."""
import numpy as np
import pytest

from buzzdetect_amd import _lib, propagate
from tests import cluster_cases, propagate_cases as cases

pytestmark = pytest.mark.gpu

CLASSES = (1, 2, 13, 64)


def guarded():
    from tests.gpu_guards import Guarded
    return Guarded("cuda")


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_weights(g, ids, sims, power):
    import torch
    nbr, w = g.empty(ids.shape, torch.int32, name="nbr"), g.empty(ids.shape, torch.float32, name="w")
    ids_dev, sims_dev = upload(ids), upload(sims)                        # (alive until the kernel has run)
    _lib.check(_lib.load().bd_propagate_weights(ids_dev.data_ptr(), sims_dev.data_ptr(), ids.shape[0], ids.shape[1], power,
                                                nbr.data_ptr(), w.data_ptr(), stream()))
    torch.cuda.synchronize()
    return nbr, w


def dev_step(g, row_start, nbr, w, f_in, y, alpha, f_out=None):
    """One bd_propagate_step on device tensors; F_out and delta are guarded.  Returns (F_out, delta) on the device."""
    import torch
    n, c = int(f_in.shape[0]), int(f_in.shape[1])
    if f_out is None:
        f_out = g.empty((n, c), torch.float32, name="f_out")
    delta = g.empty(((n + 255) // 256,), torch.float32, name="delta")
    _lib.check(_lib.load().bd_propagate_step(row_start.data_ptr(), nbr.data_ptr(), w.data_ptr(), n, int(nbr.numel()), f_in.data_ptr(),
                                             y.data_ptr(), alpha.data_ptr(), c, f_out.data_ptr(), delta.data_ptr(), stream()))
    return f_out, delta


def dev_readout(g, f):
    import torch
    n = int(f.shape[0])
    out = [g.empty((n,), dtype, name=name) for name, dtype in (("reach", torch.float32), ("label", torch.int32),
                                                               ("confidence", torch.float32), ("margin", torch.float32))]
    _lib.check(_lib.load().bd_propagate_readout(f.data_ptr(), n, int(f.shape[1]), *(t.data_ptr() for t in out), stream()))
    return [t.cpu().numpy() for t in out]


class GuardedPropagator(propagate.Propagator):
    """Every buffer of a fit between guard words."""
    guards = None

    def _empty(self, shape, dtype):
        from tests.gpu_guards import Guarded
        if GuardedPropagator.guards is None:
            GuardedPropagator.guards = Guarded("cuda")
        return self.guards.empty(shape, dtype, name=f"{tuple(shape)} {dtype}")


# ---------------------------------------------------------------------------------------------------- bits, constructed cases
@pytest.mark.parametrize("power", (1, 4, 16))
def test_weights_equal_the_host_restatement(power):
    rng = np.random.default_rng(power)
    sims = rng.uniform(-0.2, 1.0, size=(1025, 17)).astype(np.float32)
    sims[0, :4] = [np.nan, -np.inf, np.inf, -0.0]
    ids = rng.integers(0, 1025, size=(1025, 17)).astype(np.int32)
    ids[5, 9:], ids[6, :] = -1, -1
    g = guarded()
    nbr, w = dev_weights(g, ids, sims, power)
    want_nbr, want_w = propagate.weights_host(ids, sims, power)
    got_nbr, got_w = nbr.cpu().numpy(), w.cpu().numpy()
    g.check()
    assert got_nbr.tobytes() == want_nbr.tobytes() and got_w.tobytes() == want_w.tobytes()


@pytest.mark.parametrize("classes", CLASSES)
def test_step_and_readout_equal_the_host_restatements(classes):
    row_start, nbr, w, f_in, y, alpha = cases.graph_case(classes)
    f_in[7, 0] = np.nan if classes == 13 else f_in[7, 0]
    g = guarded()
    out, delta = dev_step(g, *(upload(a) for a in (row_start, nbr, w, f_in, y, alpha)))
    want, want_delta = propagate.step_host(row_start, nbr, w, f_in, y, alpha)
    got, got_delta = out.cpu().numpy(), delta.cpu().numpy()
    assert got.tobytes() == want.tobytes() and got_delta.tobytes() == want_delta.tobytes()
    f = f_in.copy()
    f[6], f[8, 0] = np.nan, np.inf
    read = dev_readout(g, upload(f))
    g.check()
    for a, b in zip(read, propagate.readout_host(f)):
        assert a.tobytes() == b.tobytes()
    assert read[1][4] == -1 and read[1][5] == 0


# ---------------------------------------------------------------------------------------------------- bits, a real graph
@pytest.fixture(scope="module")
def real():
    """The lists of the (1025, 5) fixture at k = 16 (from the host restatement, which tests/test_knn_gpu.py holds the device
    to), the labels of the planted set-up, and both graphs with their host weights."""
    e, truth, ids, sims = cases.planted_lists(1025, 5, 16)
    labelled = np.union1d(np.arange(0, 1025, 8), np.arange(5))
    y, alpha = propagate.targets_of(labelled, truth[labelled], 1025, 5)
    nbr, w = propagate.weights_host(ids, sims, 4)
    sym = propagate.lists_csr(ids, sims).symmetrised()
    _, sym_w = propagate.weights_host(sym.nbr.reshape(-1, 1), sym.sims.reshape(-1, 1), 4)
    graphs = {"lists": (np.arange(1026, dtype=np.int64) * 16, nbr.reshape(-1), w.reshape(-1)),
              "symmetrised": (sym.row_start, sym.nbr, sym_w.reshape(-1))}
    return truth, ids, sims, labelled, y, alpha, graphs


@pytest.mark.parametrize("which", ("lists", "symmetrised"))
def test_thirty_steps_back_and_forth_equal_thirty_host_steps(real, which):
    import torch
    _, _, _, _, y, alpha, graphs = real
    row_start, nbr, w = graphs[which]
    g = guarded()
    dev = [upload(a) for a in (row_start, nbr, w)]
    y_dev, alpha_dev = upload(y), upload(alpha)
    f = [g.empty((1025, 5), torch.float32, name="f0"), g.empty((1025, 5), torch.float32, name="f1")]
    f[0].copy_(y_dev)
    host = y.copy()
    for it in range(30):
        _, delta = dev_step(g, *dev, f[it & 1], y_dev, alpha_dev, f_out=f[(it & 1) ^ 1])
        host, host_delta = propagate.step_host(row_start, nbr, w, host, y, alpha)
        if it in (0, 1, 29):
            assert f[(it & 1) ^ 1].cpu().numpy().tobytes() == host.tobytes() and delta.cpu().numpy().tobytes() == host_delta.tobytes()
    read = dev_readout(g, f[0])
    g.check()
    for a, b in zip(read, propagate.readout_host(host)):
        assert a.tobytes() == b.tobytes()
    assert (read[0] > 0).all() and (read[1] >= 0).all()


@pytest.mark.parametrize("which", ("lists", "symmetrised"))
def test_propagator_is_the_kernels_in_a_loop(real, which):
    _, ids, sims, _, y, alpha, graphs = real
    row_start, nbr, w = graphs[which]
    graph = (ids, sims) if which == "lists" else propagate.lists_csr(ids, sims).symmetrised()
    p = GuardedPropagator(power=4, max_iter=12, tol=0.0).fit(graph, y, alpha)
    GuardedPropagator.guards.check()
    host = y.copy()
    deltas = []
    for _ in range(12):
        host, d = propagate.step_host(row_start, nbr, w, host, y, alpha)
        deltas.append(float(d.max()))
    assert p.iterations == 12 and p.scores.tobytes() == host.tobytes() and p.delta_history == deltas
    for a, b in zip((p.reach, p.labels, p.confidence, p.margin), propagate.readout_host(host)):
        assert a.tobytes() == b.tobytes()
    early = GuardedPropagator(power=4, max_iter=50, tol=deltas[5]).fit(graph, y, alpha)      # stops at the first step that small
    GuardedPropagator.guards.check()
    assert early.iterations == next(i + 1 for i, d in enumerate(deltas) if d <= deltas[5])


# ---------------------------------------------------------------------------------------------------- values
def steps_numpy(ids, sims, y, alpha, steps, dtype):
    """The same steps in plain NumPy of one precision (the sums as NumPy makes them): the yardstick and the reference."""
    w = np.where(ids < 0, 0, np.maximum(sims.astype(dtype), 0) ** 4).astype(dtype)
    nbr = np.where(ids < 0, 0, ids)
    y, alpha = y.astype(dtype), alpha.astype(dtype)[:, None]
    den = w.sum(axis=1, keepdims=True)
    f = y.copy()
    for _ in range(steps):
        acc = (w[:, :, None] * f[nbr]).sum(axis=1)
        mean = np.divide(acc, den, out=np.zeros_like(acc), where=den > 0)
        f = alpha * mean + (1 - alpha) * y
        assert f.dtype == dtype
    return f


@pytest.mark.parametrize("clusters", (5, 33))
def test_propagation_against_float64(clusters):
    """The device's graph taken as given: after 30 steps F deviates from float64 by at most 8 x what float32 NumPy deviates."""
    e, truth = cluster_cases.fixture(1025, clusters)
    ids, sims = propagate.Neighbours(16).update(upload(e)).lists()
    labelled = np.union1d(np.arange(0, 1025, 8), np.arange(clusters))
    y, alpha = propagate.targets_of(labelled, truth[labelled], 1025, clusters)
    p = GuardedPropagator(power=4, max_iter=30, tol=0.0).fit((ids, sims), y, alpha)
    GuardedPropagator.guards.check()
    f64 = steps_numpy(ids, sims, y, alpha, 30, np.float64)
    f32 = steps_numpy(ids, sims, y, alpha, 30, np.float32)
    yard = np.abs(f32.astype(np.float64) - f64).max()
    mine = np.abs(p.scores.astype(np.float64) - f64).max()
    print(f"clusters {clusters}: device {mine:.3e}, float32 NumPy {yard:.3e}, ratio {mine / yard:.2f}")
    assert p.iterations == 30 and mine <= 8.0 * yard


@pytest.mark.parametrize("k", (8, 16))
@pytest.mark.parametrize("clusters", (5, 33))
def test_the_planted_partition_is_recovered(clusters, k):
    """Rows 0, 8, 16, ... and the first row of every class are labelled; a directed graph, power 4.  After 2 steps a label has
    reached every row; after 40 every unlabelled row has its planted class."""
    e, truth = cluster_cases.fixture(1025, clusters)
    ids, sims = propagate.Neighbours(k).update(upload(e)).lists()
    labelled = np.union1d(np.arange(0, 1025, 8), np.arange(clusters))
    y, alpha = propagate.targets_of(labelled, truth[labelled], 1025, clusters)
    two = GuardedPropagator(power=4, max_iter=2, tol=0.0).fit((ids, sims), y, alpha)
    assert two.iterations == 2 and (two.reach > 0).all()
    p = GuardedPropagator(power=4, max_iter=40, tol=0.0).fit((ids, sims), y, alpha)
    GuardedPropagator.guards.check()
    print(f"clusters {clusters}, k {k}: smallest reach {p.reach.min():.3f}, smallest confidence {p.confidence.min():.3f}")
    assert p.iterations == 40 and p.labels.tolist() == truth.tolist()
    # hidden labelled rows are unlabelled rows like the others: right wherever a label arrives (on directed lists not everywhere)
    names = [str(c) for c in range(clusters)]
    got = propagate.holdout_accuracy((ids, sims), labelled, truth[labelled], names, repeats=2, max_iter=10)
    assert got["accuracy"] == 1.0 and 0.5 < got["coverage"] <= 1.0
    assert sum(n for _, _, n in got["per_class"].values()) == 2 * round(0.2 * labelled.shape[0])
    assert repr(got) == repr(propagate.holdout_accuracy((ids, sims), labelled, truth[labelled], names, repeats=2, max_iter=10))
