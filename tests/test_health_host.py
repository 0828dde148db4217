"""The host side of recording health (include/buzzdetect_health.h, buzzdetect_amd/health.py), no device: header, binding and
exports, every refusal with its argument named, bd_health_levels_host against the sequential NumPy statement of
tests/health_cases.py and on runs whose counts are written down by construction, different cuts of one chunk,
bd_health_spectrum_host on known answers and against np.fft.rfft under the 8 x rule of DESIGN §15, and HealthMeter's host path
over chunks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from buzzdetect_amd import _lib, health
from tests import health_cases as K

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_bindings_cover_the_header():
    with open(os.path.join(REPO, "include", "buzzdetect_health.h")) as f:
        header = f.read()
    protos = re.findall(r"^BD_API [^;(]*?(bd_\w+)\(([^;]*?)\);", header, re.M | re.S)
    names = sorted(n for n, _ in protos)
    assert names == sorted(_lib.HEALTH_PROTOTYPES) and len(names) == 8
    for name, args in protos:
        n_args = 0 if args.strip() == "void" else args.count(",") + 1
        assert len(_lib.HEALTH_PROTOTYPES[name][1]) == n_args, name
    lib = _lib.load()
    assert lib.bd_health_abi_version() == _lib.HEALTH_ABI_VERSION == int(re.search(r"BD_HEALTH_ABI_VERSION (\d+)", header).group(1))
    for name in ("S16", "F32", "MAX_CHANNELS", "SEGMENT", "SUM_DEPTH", "FRAME", "HOP", "BINS", "SEGMENT_FRAMES", "MAX_BANDS", "TABLE_FLOATS"):
        assert int(re.search(rf"#define BD_HEALTH_{name} (\d+)", header).group(1)) == getattr(_lib, "HEALTH_" + name), name
    for name in ("MAX_SEGMENTS", "MAX_RUN"):
        assert 1 << int(re.search(rf"#define BD_HEALTH_{name} \(1 << (\d+)\)", header).group(1)) == getattr(_lib, "HEALTH_" + name)
    fields = re.search(r"typedef struct bd_health_record \{(.*?)\} bd_health_record;", header, re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [n for n, _ in _lib.bd_health_record._fields_] == list(health.RECORD.names)
    assert C.sizeof(_lib.bd_health_record) == health.RECORD.itemsize == 40
    fields = re.search(r"typedef struct bd_health_level_params \{(.*?)\} bd_health_level_params;", header, re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [n for n, _ in _lib.bd_health_level_params._fields_]


# ---------------------------------------------------------------------------------------------------- levels
def same_as_numpy(x, edges, p=None):
    p = K.S16_PARAMS if p is None else p
    got = health.levels_records_host(x, edges, health.level_params(**p))
    want = K.levels_numpy(x, edges, **p)
    for name in K.INT_FIELDS:
        assert np.array_equal(got[name], want[name]), name
    assert np.array_equal(bits(got["peak"]), bits(want["peak"]))
    for name, weight in (("sum", "abs"), ("sumsq", "sq")):
        err, bound = np.abs(got[name].astype(np.float64) - want[name]), _lib.HEALTH_SUM_DEPTH * EPS * want[weight]
        assert (err <= bound).all(), (name, float((err - bound).max()))
    return got


@pytest.mark.parametrize("dtype", (np.int16, np.float32))
@pytest.mark.parametrize("ch", (1, 2, 3))
def test_random_chunks_against_the_sequential_statement(dtype, ch):
    n = 2 * K.SEG + 333
    rng = np.random.default_rng(10 * ch + (dtype == np.int16))
    # coarse values: plenty of full-scale samples, of repeats and of runs of every short length
    x = (rng.integers(-4, 5, size=(n, ch)) * 8192).clip(-32768, 32767).astype(np.int16)
    x[rng.random((n, ch)) < 0.3] = 32767
    x = x if dtype == np.int16 else (x.astype(np.float32) / np.float32(32768.0))
    for edges in (K.maximal_edges(n), K.random_edges(n, 5), K.ones_edges(700)):
        part = x[:edges[-1]]
        same_as_numpy(part, edges, dict(K.S16_PARAMS, clip_run=2, flat_run=3))
        same_as_numpy(part, edges, dict(K.S16_PARAMS, clip_run=1, flat_run=2))
    same_as_numpy(K.live(n, ch, 3, dtype), K.random_edges(n, 6))


def test_non_finite_samples_are_counted_and_enter_as_zero():
    x = K.live(5000, 2, 4, np.float32)
    x[[7, 8, 9, 4500], 0] = [np.nan, np.inf, -np.inf, np.nan]
    x[10:20, 1] = np.nan                                    # ten zeros in a row: a stuck run of FLAT_RUN or more
    got = same_as_numpy(x, K.maximal_edges(5000))
    assert got["nonfinite"].tolist() == [[3, 10], [1, 0]] and got["flat"].tolist() == [[0, 10], [0, 0]]
    assert np.isfinite(got["sum"]).all() and np.isfinite(got["peak"]).all()


def test_constructed_runs_have_the_counts_written_down():
    x, want = K.constructed()
    for edges in (K.maximal_edges(K.CONSTRUCTED_N), K.random_edges(K.CONSTRUCTED_N, 9)):
        got = same_as_numpy(x, edges)
        for name, total in want.items():
            assert np.array_equal(got[name].sum(axis=0), total), name
        as_f32 = health.levels_records_host(x.astype(np.float32) / np.float32(32768.0), edges, K.params())
        assert got.tobytes() == as_f32.tobytes()            # one arithmetic path behind the conversion
    got = health.levels_records_host(x, K.maximal_edges(K.CONSTRUCTED_N), K.params())
    # each sample is counted in its own segment, a run in the segment of its first sample
    assert got["clipped"][:, 1].tolist() == [6, 1 + 3, 4096, 4096, 4096, 2] and got["clip_runs"][:, 1].tolist() == [1, 1, 0, 0, 0, 0]
    assert got["clipped"][:, 2].tolist() == [6, 2, 0, 0, 0, 0] and got["flat_runs"][:, 2].tolist() == [1, 0, 0, 0, 0, 0]
    assert got["flat"][:, 3].tolist() == [4096] * 5 + [700] and got["flat_runs"][:, 3].tolist() == [1, 0, 0, 0, 0, 0]
    # segments of length 1
    ones = same_as_numpy(x[:400], K.ones_edges(400))
    assert ones["clipped"][:, 0].sum() == 2 * (3 + 4) + 6 and ones["clip_runs"][:, 0].sum() == 6 and (ones["flat"][:, 3] == 1).all()
    assert ones["flat_runs"][:, 3].tolist() == [1] + [0] * 399


def test_stuck_runs_at_the_threshold():
    for flat_run in (2, 8, 50):
        x = K.live(1000, 1, flat_run)
        x[100:100 + flat_run - 1] = 77
        x[300:300 + flat_run] = 77
        x[600:600 + flat_run + 1] = -77
        got = same_as_numpy(x, K.random_edges(1000, flat_run), dict(K.S16_PARAMS, flat_run=flat_run))
        assert got["flat"].sum() == 2 * flat_run + 1 and got["flat_runs"].sum() == 2


def test_different_cuts_of_one_chunk():
    x, _ = K.constructed()
    cuts = [K.maximal_edges(K.CONSTRUCTED_N), K.random_edges(K.CONSTRUCTED_N, 1), K.random_edges(K.CONSTRUCTED_N, 2)]
    got = [health.levels_records_host(x, e, K.params()) for e in cuts]
    for g in got[1:]:
        for name in K.INT_FIELDS:
            assert np.array_equal(g[name].sum(axis=0), got[0][name].sum(axis=0)), name
        assert np.array_equal(g["peak"].max(axis=0), got[0]["peak"].max(axis=0))
    # a segment's sums do not change when the other segments are cut differently: segment 4096..8192 in two tables
    a = np.asarray([0, 4096, 8192, 12288, 16384, 20480, K.CONSTRUCTED_N], np.int64)
    b = np.asarray([0, 1, 700, 4096, 8192, 8193, 12000, 16000, 20000, K.CONSTRUCTED_N], np.int64)
    ra, rb = health.levels_records_host(x, a, K.params()), health.levels_records_host(x, b, K.params())
    assert np.array_equal(bits(ra["sum"][1]), bits(rb["sum"][3])) and np.array_equal(bits(ra["sumsq"][1]), bits(rb["sumsq"][3]))
    alone = health.levels_records_host(x[4096:8192], np.asarray([0, 4096], np.int64), K.params())
    assert np.array_equal(bits(ra["sum"][1]), bits(alone["sum"][0])) and np.array_equal(bits(ra["sumsq"][1]), bits(alone["sumsq"][0]))
    one = health.levels_records_host(x[4096:8192, 1].copy(), np.asarray([0, 4096], np.int64), K.params())      # nor on the other channels
    assert bits(one["sum"])[0, 0] == bits(ra["sum"])[1, 1]


def test_refused_level_arguments_name_the_argument():
    lib = _lib.load()
    x, edges, records = np.zeros((100, 2), np.int16), np.asarray([0, 60, 100], np.int64), np.zeros((2, 2), health.RECORD)
    p = K.params()

    def call(dtype=0, n=100, ch=2, s=2, x_at=x.ctypes.data, e_at=edges.ctypes.data, p_at=C.addressof(p), r_at=records.ctypes.data):
        rc = lib.bd_health_levels_host(x_at, dtype, n, ch, e_at, s, p_at, r_at)
        return rc, lib.bd_last_error().decode()

    assert call()[0] == 0
    for kwargs, word in (({"dtype": 2}, "dtype"), ({"ch": 0}, "channels"), ({"ch": 9}, "channels"), ({"s": -1}, "n_segments"),
                         ({"n": 1}, "n_frames"), ({"n": 3 * 4096}, "n_frames"), ({"p_at": None}, "params"), ({"x_at": None}, "x is"),
                         ({"x_at": x.ctypes.data + 1}, "x is"), ({"e_at": None}, "edges is"), ({"r_at": None}, "records is"),
                         ({"n": 99}, "edges[2]")):
        rc, text = call(**kwargs)
        assert rc == -1 and word in text, (kwargs, text)
    for bad, word in ((dict(clip_hi=-1.0), "clip_lo"), (dict(clip_hi=float("nan")), "clip_lo"), (dict(clip_run=0), "clip_run"),
                      (dict(flat_run=1), "flat_run"), (dict(flat_run=_lib.HEALTH_MAX_RUN + 1), "flat_run")):
        with pytest.raises(_lib.BuzzdetectHipError, match=word):
            health.levels_records_host(x, edges, K.params(**bad))
    for table, word in (([1, 60, 100], r"edges\[0\]"), ([0, 60, 60, 100], r"edges\[1\]"), ([0, 5000, 5001], r"edges\[0\]")):
        with pytest.raises(_lib.BuzzdetectHipError, match=word):
            health.levels_records_host(np.zeros((table[-1], 1), np.int16), np.asarray(table, np.int64), p)
    records[:] = 7
    assert call(n=0, s=0, x_at=None, e_at=None, r_at=None)[0] == 0 and records.tobytes() == np.full_like(records, 7).tobytes()
    assert lib.bd_health_levels_workspace_bytes(10, 3) == 3 * 10 * 3 * 3 * 20 and lib.bd_health_levels_workspace_bytes(1, 9) == -1


# ---------------------------------------------------------------------------------------------------- spectrum
TABLES = health.tables()


def test_tables_are_the_double_values_rounded_once():
    k = np.arange(512)
    assert np.array_equal(bits(TABLES[:1024]), bits(K.hann().astype(np.float32)))
    assert np.array_equal(bits(TABLES[1024:1536]), bits(np.cos(2 * np.pi * k / 1024).astype(np.float32)))
    assert np.array_equal(bits(TABLES[1536:]), bits((-np.sin(2 * np.pi * k / 1024)).astype(np.float32)))


def test_a_sine_on_a_bin_centre_and_the_full_cover():
    x = K.tone(1000.0, 0.5, 1024 + 7 * 512)
    fedges = K.frame_edges(8, 1)
    _, bedges = health.band_bins((0, 500, 1500, 8000))
    power, bad = health.spectrum_host(x, fedges, bedges, TABLES)
    assert not bad.any() and np.allclose(power[:, 1], 0.5 ** 2 / 2, rtol=1e-5) and (power[:, [0, 2]] < 1e-9).all()
    rng = np.random.default_rng(1)
    x = (0.2 * rng.standard_normal(1024 + 7 * 512)).astype(np.float32)
    power, _ = health.spectrum_host(x, fedges, bedges, TABLES)
    w = K.hann()
    for f in range(8):
        want = ((w * x[512 * f:512 * f + 1024].astype(np.float64)) ** 2).sum() / (w * w).sum()
        assert abs(power[f].astype(np.float64).sum() / want - 1) < 1e-5


def test_a_frame_with_a_nan_is_left_out_and_counted():
    x = K.accuracy_inputs()["tone in noise"]
    dirty = x.copy()
    dirty[2100] = np.nan                                    # frames 3 (1536..2559) and 4 (2048..3071)
    _, bedges = health.band_bins(health.DEFAULT_BANDS)
    clean, none = health.spectrum_host(x, K.frame_edges(16, 1), bedges, TABLES)
    got, bad = health.spectrum_host(dirty, K.frame_edges(16, 1), bedges, TABLES)
    rest = [f for f in range(16) if f not in (3, 4)]
    assert not none.any() and bad.tolist() == [int(f in (3, 4)) for f in range(16)]
    assert np.array_equal(bits(got[rest]), bits(clean[rest])) and not got[[3, 4]].any()
    whole, bad = health.spectrum_host(dirty, K.frame_edges(16, 64), bedges, TABLES)
    assert bad.tolist() == [2] and np.isfinite(whole).all()
    p, isbad = K.frame_powers_f64(dirty)
    want, _ = K.band_sums(p, isbad, K.frame_edges(16, 64), bedges, np.float64)
    assert np.allclose(whole, want, rtol=1e-4)


@pytest.mark.parametrize("name", sorted(K.accuracy_inputs()))
def test_band_powers_against_rfft_under_the_eight_times_rule(name):
    """The deviation of a band power from float64 np.fft.rfft, relative to the segment's whole power, is held to 8 x that of the
    plain float32 radix-2 NumPy transform of tests/health_cases.py on the same input."""
    x = K.accuracy_inputs()[name]
    _, bedges = health.band_bins(health.DEFAULT_BANDS)
    worst = {}
    for length in (1, 5, 16):
        fedges = K.frame_edges(16, length)
        p64, bad = K.frame_powers_f64(x)
        ref, _ = K.band_sums(p64, bad, fedges, bedges, np.float64)
        plain, _ = K.band_sums(K.frame_powers_f32(x), bad, fedges, bedges, np.float32)
        got, none = health.spectrum_host(x, fedges, bedges, TABLES)
        scale = ref.sum(axis=1, keepdims=True)
        mine, theirs = float((np.abs(got - ref) / scale).max()), float((np.abs(plain - ref) / scale).max())
        worst[length] = (mine, theirs)
        print(f"{name}, segments of {length}: host {mine:.3g}, float32 NumPy {theirs:.3g}, ratio {mine / theirs:.3g}")
        assert not none.any() and theirs > 0 and mine <= 8 * theirs


def test_refused_spectrum_arguments_name_the_argument():
    lib = _lib.load()
    x, fedges, bedges = np.zeros(2048, np.float32), np.asarray([0, 2, 3], np.int64), np.asarray([0, 10, 513], np.int32)
    power, bad = np.zeros((2, 2), np.float32), np.zeros(2, np.int32)

    def call(n=2048, t=2, b=2, x_at=x.ctypes.data, f_at=fedges.ctypes.data, b_at=bedges.ctypes.data, t_at=TABLES.ctypes.data,
             p_at=power.ctypes.data, bad_at=bad.ctypes.data):
        rc = lib.bd_health_spectrum_host(x_at, n, f_at, t, b_at, b, t_at, p_at, bad_at)
        return rc, lib.bd_last_error().decode()

    assert call()[0] == 0
    for kwargs, word in (({"n": -1}, "n ="), ({"t": 4}, "n_segments"), ({"t": -1}, "n_segments"), ({"b": 0}, "n_bands"), ({"b": 65}, "n_bands"),
                         ({"b_at": None}, "bedges is"), ({"x_at": None}, "x16k is"), ({"f_at": None}, "fedges is"), ({"t_at": None}, "tables is"),
                         ({"p_at": None}, "power is"), ({"bad_at": None}, "bad_frames is"), ({"n": 1536}, "fedges[2]")):
        rc, text = call(**kwargs)
        assert rc == -1 and word in text, (kwargs, text)
    for table in ([0, 10, 10], [5, 4, 6], [0, 10, 514], [-1, 10, 20]):
        with pytest.raises(_lib.BuzzdetectHipError, match="bedges"):
            health.spectrum_host(x, fedges, np.asarray(table, np.int32), TABLES)
    power[:] = 7
    assert call(n=1023, t=0, f_at=None, p_at=None, bad_at=None)[0] == 0 and (power == 7).all()
    with pytest.raises(ValueError, match="ascending"):
        health.band_bins((0, 100, 100))
    with pytest.raises(ValueError, match="ascending"):
        health.band_bins((0, 9000))
    hz, edges = health.band_bins(health.DEFAULT_BANDS)
    assert edges.tolist() == [0, 4, 8, 16, 32, 64, 128, 256, 513] and hz[-1] == 8000.0 and health.band_bins((0, 60, 130))[0].tolist() == [0, 62.5, 125]


# ---------------------------------------------------------------------------------------------------- HealthMeter
def test_segments_are_cut_in_integer_arithmetic():
    edges, seg_bins = health.cut_segments(44099, 100000, 44100, 100, 4096)
    assert edges[0] == 0 and edges[-1] == 100000 and (np.diff(edges) >= 1).all() and (np.diff(edges) <= 4096).all()
    at = 44099 + np.arange(100000)
    want = (100 * at) // (44100 * 100)
    assert np.array_equal(np.repeat(seg_bins, np.diff(edges)), want) and seg_bins.tolist()[0] == 0 and seg_bins[-1] == 3
    assert health.cut_segments(5, 0, 16000, 6000, 4096)[0].tolist() == [0]
    fedges, fbins = health.frame_segments(16000 * 59, 16000 * 3, 6000)
    starts = 16000 * 59 + 512 * np.arange(K.frames_of(48000))
    assert np.array_equal(np.repeat(fbins, np.diff(fedges)), starts // 960000) and (np.diff(fedges) <= 64).all()


@pytest.mark.parametrize("rate, ch", ((16000, 1), (48000, 2)))
def test_bins_that_straddle_chunks_merge_to_the_table_of_one_chunk(rate, ch):
    """bin_s = 1.0 and chunks of 1.92 s: every second bin lies in two chunks.  No run crosses a chunk end here, so the merged
    integer fields and the peak are those of the recording as one chunk; the float32 sums of differently cut segments differ
    within the bound of the summation order."""
    n = int(5.3 * rate)
    x = K.live(n, ch, rate)
    x[1000:1010, 0] = 32767
    x[int(2.5 * rate):int(2.53 * rate), ch - 1] = 0          # 0.03 s of digital silence: above flat_s = 0.02 s
    meter = health.HealthMeter(bin_s=1.0)
    whole = meter.levels_host(x, rate, 0)
    cuts = [int(round(1.92 * k, 2) * rate) for k in range(3)] + [n]
    parts = [meter.levels_host(x[a:b], rate, a) for a, b in zip(cuts[:-1], cuts[1:])]
    merged = health.merge_levels(parts)
    assert np.array_equal(merged.bins, whole.bins) and whole.bins.tolist() == [0, 1, 2, 3, 4, 5]
    for name in health.COUNTS:
        assert np.array_equal(merged.counts[name], whole.counts[name]), name
    assert whole.counts["clipped"][:, 0].tolist() == [10, 0, 0, 0, 0, 0] and whole.counts["flat"][2, ch - 1] == int(2.53 * rate) - int(2.5 * rate)
    assert whole.counts["n"][:, 0].tolist() == [rate] * 5 + [n - 5 * rate]
    assert np.array_equal(merged.peak, whole.peak)
    v = x.astype(np.float64) / 32768.0
    for b in range(6):
        part = v[b * rate:(b + 1) * rate]
        for got in (merged, whole):
            assert (np.abs(got.sum[b] - part.sum(axis=0)) <= _lib.HEALTH_SUM_DEPTH * EPS * np.abs(part).sum(axis=0)).all()
            assert (np.abs(got.sumsq[b] - (part * part).sum(axis=0)) <= _lib.HEALTH_SUM_DEPTH * EPS * (part * part).sum(axis=0)).all()


def test_a_result_writes_its_tables_and_flags_and_a_store_is_refused(tmp_path):
    meter = health.HealthMeter(bin_s=1.0, bands=(0, 125, 250, 2000, 8000))
    rate = 16000
    x = K.live(3 * rate, 1, 8)
    x[100:400, 0] = 32767                                   # bin 0: clipped
    x[rate:2 * rate, 0] = 0                                 # bin 1: digital silence
    pcm = (x[:, 0].astype(np.float32) / np.float32(32768.0))
    rec = health.recording_health(meter.levels_host(x, rate), meter.spectrum_host(pcm, 0.0), rate, meter.bin_ticks)
    result = health.HealthResult(meter.band_hz, {"site/a": rec}, bin_s=meter.bin_s)
    assert rec.bin_start.tolist() == [0.0, 1.0, 2.0] and rec.seconds.tolist() == [1.0, 1.0, 1.0]
    assert rec.clipped[:, 0].tolist() == [300, 0, 0] and rec.clip_runs[:, 0].tolist() == [1, 0, 0] and rec.flat[1, 0] == rate
    assert rec.rms_dbfs[1, 0] == -np.inf and abs(rec.peak_dbfs[0, 0] - 20 * np.log10(32767 / 32768)) < 1e-9
    assert rec.frames.tolist() == [32, 31, 29] and not rec.bad_frames.any()
    flags = result.flags()["site/a"]
    assert [(u, why) for _, u, why in flags] == [(False, ("clipped",)), (False, ("flat", "silent")), (True, ())]
    wind = result.flags(band_rules={"flat spectrum": ((0, 125), (250, 2000), -60.0)})["site/a"]
    assert "flat spectrum" in wind[2][2] and not wind[2][1]
    with pytest.raises(ValueError, match="band edges"):
        result.flags(band_rules={"wind": ((0, 100), (250, 2000), 20.0)})
    table = result.table()
    assert len(table) == 3 and table.dtype.names[:3] == ("ident", "bin_start", "channel") and table.dtype.names[-1] == "band_2000_8000"
    result.to_csv(str(tmp_path))
    lines = (tmp_path / "site" / ("a" + health.SUFFIX_HEALTH)).read_text().splitlines()
    assert lines[0] == ",".join(health.HEALTH_COLUMNS) and len(lines) == 4
    assert lines[2].startswith("1.0,0,1.0,-inf,-inf,0.000000,0,0,0,16000,1,0")
    ltsa = (tmp_path / "site" / ("a" + health.SUFFIX_LTSA)).read_text().splitlines()
    assert ltsa[0] == "bin_start,frames,bad_frames,band_0_125,band_125_250,band_250_2000,band_2000_8000" and len(ltsa) == 4
    assert ltsa[1].split(",")[:3] == ["0.0", "32", "0"]
    (tmp_path / "emb").mkdir()
    (tmp_path / "emb" / "store.json").write_text("{}")
    with pytest.raises(ValueError, match="holds no audio"):
        health.health_recordings(str(tmp_path / "emb"))
