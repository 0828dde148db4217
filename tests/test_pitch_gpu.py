"""bd_pitch_windows on the GPU against bd_pitch_windows_host: every bit of values, voiced and frames, on the host test's windows,
at the edges of a chunk, under permutations of sel, twice, with and without frames - in guarded buffers (tests/gpu_guards.py):
guard words intact, every output word written.  The chunk and sel lie in guarded buffers of their exact size too, so a read
beyond either meets sentinel NaNs and shows in the comparison."""
import numpy as np
import pytest

from buzzdetect_amd import pitch
from tests import pitch_cases as P
from tests.gpu_guards import Guarded

pytestmark = pytest.mark.gpu

W = P.WINDOW


def word_view(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def chunk():
    """The accuracy cases and the exactness windows of the host test, end to end: 79 windows at step 15 360."""
    dirty = P.buzz(233.0, P.HARMONICS["five"], seed=5)
    dirty[5000] = np.nan
    two = np.concatenate([P.periodic(40)[:W // 2], P.periodic(50)[:W // 2]])
    extra = [P.periodic(16), P.periodic(200), np.full(W, 3.0, np.float32), dirty, P.noise(1), np.zeros(W, np.float32), two]
    return np.concatenate([c[2] for c in P.accuracy_cases()] + extra)


class Rig:
    """A tracker whose every buffer is guarded; ``run`` tracks on the device, checks the guards and returns NumPy."""

    def __init__(self, lags=None):
        self.tracker = pitch.PitchTracker()
        if lags is not None:
            self.tracker.lag_lo, self.tracker.lag_hi = lags
            self.tracker.params = pitch.params(*lags)
        self.guards = Guarded(self.tracker.device)
        self.tracker._empty = lambda shape, dtype: self.guards.empty(shape, dtype)

    def run(self, x, sel, step, want_frames=True):
        import torch
        x, sel = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(sel, np.int32)
        x_dev = self.guards.empty(x.shape, torch.float32, written=False)
        sel_dev = self.guards.empty(sel.shape, torch.int32, written=False)
        x_dev.copy_(torch.from_numpy(x))
        sel_dev.copy_(torch.from_numpy(sel))
        got = self.tracker.track(x_dev, sel_dev, step, want_frames=want_frames)
        self.guards.check(written=True)
        assert np.array_equal(x_dev.cpu().numpy().view(np.uint32), x.view(np.uint32)) and np.array_equal(sel_dev.cpu().numpy(), sel)
        return got

    def same_as_host(self, x, sel, step):
        got = self.run(x, sel, step)
        want = self.tracker.track_host(x, sel, step, want_frames=True)
        for name, a, b in zip(("f0", "clarity", "voiced", "frames"), got, want):
            assert a.shape == b.shape and a.dtype == b.dtype, name
            bad = np.flatnonzero((word_view(a) != word_view(b)).reshape(len(sel), -1).any(axis=1))
            assert bad.size == 0, f"{name}: {bad.size} of {len(sel)} windows differ, first sel[{bad[0]}] = {sel[bad[0]]}"
        return got


@pytest.fixture(scope="module")
def rig():
    return Rig()


@pytest.mark.parametrize("step", (15360, 7680))
@pytest.mark.parametrize("s", (1, 2, 63, 65))
def test_the_device_has_the_hosts_bits(rig, chunk, s, step):
    windows = (chunk.shape[0] - W) // step + 1
    rng = np.random.default_rng(100 * s + step)
    sel = rng.integers(-2, windows + 3, size=s)                       # unsorted, repeated, beyond both ends
    if s >= 63:
        sel[:6] = [windows, -1, 5, 5, 1 << 30, -(1 << 31)]
    f0, clarity, voiced, frames = rig.same_as_host(chunk, sel, step)
    silent = (sel < 0) | (sel.astype(np.int64) * step >= chunk.shape[0])
    assert (voiced[silent] == 0).all() and np.isnan(f0[silent]).all() and not frames[silent].any()


def test_all_of_the_hosts_windows(rig, chunk):
    """Every accuracy and exactness window once, in order: the device's f0 is the host's, so it meets the host test's bounds."""
    f0, clarity, voiced, frames = rig.same_as_host(chunk, np.arange(chunk.shape[0] // W), W)
    assert (voiced[:72] == 29).all() and voiced[72] == 29 and voiced[74] == 0 and voiced[75] == 27


@pytest.mark.parametrize("lags", ((1, 1), (1, 511), (511, 511)))
def test_the_lag_ranges_at_the_limits(chunk, lags):
    rig = Rig(lags)
    low = np.concatenate([P.buzz(32.0, P.HARMONICS["five"], seed=4), P.periodic(511), P.periodic(2)])
    rig.same_as_host(np.concatenate([chunk[70 * W:], low]), [0, 3, 9, 10, 11, 2, 4, 6], W)


def test_frames_that_tie_in_f0(chunk):
    """The host test's tied windows (lag_lo = lag_hi = 20: every voiced frame has the same f0 and its own clarity): the
    thread that ranks in the middle of the order (f0, frame) stores the window, as on the host."""
    rig = Rig((20, 20))
    spans = ((0, 28), (0, 11), (9, 21), (17, 28))
    f0, clarity, voiced, frames = rig.same_as_host(np.concatenate([P.tied_window(a, b) for a, b in spans]), [3, 0, 2, 1], W)
    assert voiced.tolist() == [12, 29, 13, 12] and (word_view(f0) == word_view(np.float32(P.RATE / 20.5))).all()
    for at, (a, b) in zip((1, 3, 2, 0), spans):
        assert word_view(clarity[at:at + 1]) == word_view(frames[at, a + (b - a) // 2, 1:2])


@pytest.mark.parametrize("step", (15360, 7680))
@pytest.mark.parametrize("n_samples", (1, 1023, 15360, 15361, 3 * 15360 + 700))
def test_chunks_that_end_inside_a_window(rig, chunk, n_samples, step):
    x = chunk[20 * W:20 * W + n_samples]
    windows = -(-n_samples // step)
    rig.same_as_host(x, np.arange(-1, windows + 2), step)


def test_permutations_single_windows_repeats_and_frames(rig, chunk):
    x = chunk[60 * W:66 * W + 700]
    sel = np.arange(13)
    first = rig.run(x, sel, 7680)
    again = rig.run(x, sel, 7680)
    for a, b in zip(first, again):
        assert np.array_equal(word_view(a), word_view(b))                                   # two runs are identical
    order = np.random.default_rng(7).permutation(13)
    moved = rig.run(x, sel[order], 7680)
    for a, b in zip(first, moved):
        assert np.array_equal(word_view(a[order]), word_view(b))                            # a window's place does not matter
    for k in (0, 7, 12):
        alone = rig.run(x, [k], 7680)
        for a, b in zip(first, alone):
            assert np.array_equal(word_view(a[k:k + 1]), word_view(b))                      # nor does its company
    bare = rig.run(x, sel, 7680, want_frames=False)
    assert len(bare) == 3
    for a, b in zip(first, bare):
        assert np.array_equal(word_view(a), word_view(b))                                   # frames or not: the same values


def test_nothing_selected_launches_nothing(rig, chunk):
    import torch
    got = rig.tracker.track(torch.from_numpy(chunk[:W]).to(rig.tracker.device), np.zeros(0, np.int32), W, want_frames=True)
    rig.guards.check(written=False)
    assert [g.shape for g in got] == [(0,), (0,), (0,), (0, 29, 2)]
