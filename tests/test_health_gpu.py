"""bd_health_levels and bd_health_spectrum on the GPU against their host restatements: every bit of every record, of power and
of bad_frames, in guarded buffers (tests/gpu_guards.py) - guard words intact, every output word written (the workspace's too),
inputs unchanged.  The inputs lie in guarded buffers of their exact size, so a read beyond them meets sentinel words and shows
in the comparison."""
import numpy as np
import pytest

from buzzdetect_amd import _lib, health
from tests import health_cases as K
from tests.gpu_guards import Guarded

pytestmark = pytest.mark.gpu

N_FRAMES = (1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 700)


class Rig:
    """A meter whose every device buffer is guarded."""

    def __init__(self):
        self.meter = health.HealthMeter()
        self.guards = Guarded(self.meter.device)
        self.meter._empty = lambda shape, dtype: self.guards.empty(shape, dtype)

    def levels(self, x, edges, p):
        import torch
        x = np.ascontiguousarray(x)
        x_dev = self.guards.empty(x.shape, torch.int16 if x.dtype == np.int16 else torch.float32, written=False)
        x_dev.copy_(torch.from_numpy(x))
        records = self.meter.launch_levels(x_dev, edges, p)
        self.guards.check(written=True)
        assert x_dev.cpu().numpy().tobytes() == x.tobytes()
        return records.cpu().numpy().view(health.RECORD)[..., 0]

    def levels_same_as_host(self, x, edges, p):
        got = self.levels(x, edges, p)
        want = health.levels_records_host(x, edges, p)
        assert got.shape == want.shape
        for name in health.RECORD.names:
            bad = np.argwhere(got[name].view(np.uint32) != want[name].view(np.uint32))
            assert bad.size == 0, f"{name}: {bad.shape[0]} records differ, first (segment, channel) {bad[0].tolist()}: " \
                                  f"{got[name][tuple(bad[0])]} != {want[name][tuple(bad[0])]}"
        return got

    def spectrum(self, x, fedges, bedges):
        import torch
        x = np.ascontiguousarray(x, np.float32)
        self.meter.bedges = np.ascontiguousarray(bedges, np.int32)
        x_dev = self.guards.empty(x.shape, torch.float32, written=False)
        x_dev.copy_(torch.from_numpy(x))
        power, bad = self.meter.launch_spectrum(x_dev, fedges)
        self.guards.check(written=True)
        assert x_dev.cpu().numpy().tobytes() == x.tobytes()
        return power.cpu().numpy(), bad.cpu().numpy()

    def spectrum_same_as_host(self, x, fedges, bedges):
        got = self.spectrum(x, fedges, bedges)
        want = health.spectrum_host(x, fedges, bedges, self.meter.tables)
        assert got[0].shape == want[0].shape and np.array_equal(got[1], want[1])
        bad = np.argwhere(got[0].view(np.uint32) != want[0].view(np.uint32))
        assert bad.size == 0, f"power: {bad.shape[0]} values differ, first (segment, band) {bad[0].tolist()}"
        return got


@pytest.fixture(scope="module")
def rig():
    return Rig()


def coarse(n, ch, dtype, seed):
    """Few values, many at full scale: runs of every short length, of both signs, across every segment edge."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(-4, 5, size=(n, ch)) * 8192).clip(-32768, 32767).astype(np.int16)
    x[rng.random((n, ch)) < 0.3] = 32767
    long = rng.integers(0, max(n - 1, 1))
    x[long:long + 9000, ch - 1] = -32768                                   # a run through whole segments
    return x if dtype == np.int16 else (x.astype(np.float32) / np.float32(32768.0))


@pytest.mark.parametrize("dtype", (np.int16, np.float32))
@pytest.mark.parametrize("ch", (1, 2, 3, 8))
def test_levels_have_the_hosts_bits(rig, dtype, ch):
    p = K.params(clip_run=2, flat_run=3)
    for n in N_FRAMES:
        x = coarse(n, ch, dtype, 100 * ch + n % 97)
        if dtype == np.float32 and n > 64:
            x[[5, n - 2], 0] = [np.nan, np.inf]
        for edges in (K.ones_edges(n), K.maximal_edges(n), K.random_edges(n, n)):
            rig.levels_same_as_host(x, edges, p)
    x = K.live(4097, ch, 5, dtype)
    rig.levels_same_as_host(x, K.random_edges(4097, 1), K.params())


@pytest.mark.parametrize("dtype", (np.int16, np.float32))
def test_the_constructed_runs(rig, dtype):
    x, want = K.constructed()
    x = x if dtype == np.int16 else (x.astype(np.float32) / np.float32(32768.0))
    for edges in (K.maximal_edges(K.CONSTRUCTED_N), K.random_edges(K.CONSTRUCTED_N, 9)):
        got = rig.levels_same_as_host(x, edges, K.params())
        for name, total in want.items():
            assert np.array_equal(got[name].astype(np.int64).sum(axis=0), total), name
    rig.levels_same_as_host(x[:400], K.ones_edges(400), K.params())


def test_two_level_runs_are_identical_and_no_segments_write_nothing(rig):
    import torch
    x = coarse(3 * 4096 + 700, 3, np.int16, 1)
    edges = K.random_edges(x.shape[0], 3)
    first, again = rig.levels(x, edges, K.params()), rig.levels(x, edges, K.params())
    assert first.tobytes() == again.tobytes()
    empty = torch.zeros((0, 2), dtype=torch.int16, device=rig.meter.device)
    records = rig.meter.launch_levels(empty, np.zeros(1, np.int64), K.params())
    rig.guards.check(written=False)
    assert tuple(records.shape) == (0, 2, 10)
    with pytest.raises(_lib.BuzzdetectHipError, match=r"edges\[1\]"):
        rig.meter.launch_levels(torch.zeros((10, 2), dtype=torch.int16, device=rig.meter.device), np.asarray([0, 5, 5, 10]), K.params())


def test_levels_beyond_the_32_bit_offsets():
    """8 channels of int16, 2^27 + 5 frames: the bytes of the last segments lie beyond 2^31.  The chunk repeats a pattern of 1000
    frames (no divisor of 4096) with a high plateau, a stuck stretch, a low plateau and a long high run.  From frame
    E = 2^27 - 9192 on (E mod 1000 = 536: frames 535 and 536 are live in every channel, so the host's carry, which starts at
    zero there, is the device's) the records are the host's on that tail alone; n_full and peak of the whole chunk are torch's."""
    import torch
    n = (1 << 27) + 5
    period, ch = 1000, 8
    base = K.live(period, ch, 31)
    base[100:105, 0] = 32767
    base[300:312, 1] = 1234
    base[500:503, 2] = -32768
    base[600:900, 3] = 32767
    assert (base[0] != base[-1]).all() and (base[535] != base[536]).all() and (np.abs(base[[535, 536]].astype(np.int32)) < 32767).all()
    dev = torch.device("cuda", torch.cuda.current_device())
    x_dev = torch.from_numpy(base).to(dev).repeat(n // period + 1, 1)[:n].contiguous()
    start = (1 << 27) - 9192
    edges = np.concatenate([np.arange(0, start, 4096), np.arange(start, 1 << 27, 1500), [1 << 27, (1 << 27) + 2, n]]).astype(np.int64)
    meter = health.HealthMeter()
    guards = Guarded(dev)
    meter._empty = lambda shape, dtype: guards.empty(shape, dtype)
    p = K.params()
    records = meter.launch_levels(x_dev, edges, p)
    guards.check(written=True)
    got = records.cpu().numpy().view(health.RECORD)[..., 0]
    first = int(np.searchsorted(edges, start))
    assert edges[first] == start and edges[-3] * ch * 2 == 1 << 31           # the last two segments lie wholly beyond
    tail = x_dev[start:].cpu().numpy()
    want = health.levels_records_host(tail, edges[first:] - start, p)
    for name in health.RECORD.names:
        assert np.array_equal(got[first:][name].view(np.uint32), want[name].view(np.uint32)), name
    full = ((x_dev == 32767) | (x_dev == -32768)).sum(dim=0).cpu().numpy()
    assert np.array_equal(got["n_full"].astype(np.int64).sum(axis=0), full) and full[0] > 5 * (n // period)
    peak = torch.maximum(x_dev.amax(dim=0).to(torch.int32), -x_dev.amin(dim=0).to(torch.int32)).cpu().numpy()
    assert np.array_equal(got["peak"].max(axis=0), (peak.astype(np.float32) / np.float32(32768.0)))
    assert got["n"].astype(np.int64).sum(axis=0).tolist() == [n] * ch


# ---------------------------------------------------------------------------------------------------- spectrum
def signal(n, seed=3):
    rng = np.random.default_rng(seed)
    return (K.tone(440.0, 0.3, n) + K.tone(3333.3, 0.1, n, 1.0) + (0.05 * rng.standard_normal(n)).astype(np.float32)).astype(np.float32)


BANDS = {1: np.asarray([0, 513], np.int32), 8: health.band_bins(health.DEFAULT_BANDS)[1],
         64: np.concatenate([np.arange(0, 512, 8), [513]]).astype(np.int32)}


@pytest.mark.parametrize("b", (1, 8, 64))
def test_spectrum_has_the_hosts_bits(rig, b):
    assert BANDS[b].shape[0] == b + 1 and BANDS[b][0] == 0 and BANDS[b][-1] == 513
    for n in (1024, 1535, 1536, 1024 + 63 * 512, 1024 + 64 * 512, 1024 + 64 * 512 + 511):
        x = signal(n, n)
        frames = K.frames_of(n)
        for length in (1, 63, 64):
            rig.spectrum_same_as_host(x, K.frame_edges(frames, length), BANDS[b])
        rig.spectrum_same_as_host(x, K.frame_edges(frames, 64, seed=n), BANDS[b])
    inner = np.asarray([1, 2, 64, 65, 300, 512], np.int32)                 # edges that touch neither end
    rig.spectrum_same_as_host(signal(5000), K.frame_edges(K.frames_of(5000), 3), inner)


def test_non_finite_frames_twice_and_nothing_to_do(rig):
    n = 1024 + 64 * 512
    x = signal(n)
    x[3] = np.nan                                                          # the first frame
    x[n - 1] = np.inf                                                      # the last
    for length in (1, 64):
        fedges = K.frame_edges(65, length)
        power, bad = rig.spectrum_same_as_host(x, fedges, BANDS[8])
        assert bad.sum() == 2 and np.isfinite(power).all()
        again = rig.spectrum(x, fedges, BANDS[8])
        assert again[0].tobytes() == power.tobytes() and np.array_equal(again[1], bad)
    power, bad = rig.spectrum(signal(1023), np.zeros(1, np.int64), BANDS[8])
    assert power.shape == (0, 8) and bad.shape == (0,)
