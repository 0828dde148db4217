"""bd_pitch_windows_host (include/buzzdetect_pitch.h) on the CPU: accuracy against the generator's nominal fundamental, agreement
with the float64 NumPy restatement of tests/pitch_cases.py frame by frame, exactness cases on whole-number samples, the edges of
a chunk, the parameters' limits and refusals, and pitch.event_wingbeats on hand-made window tables."""
import ctypes as C

import numpy as np
import pytest

from tests import pitch_cases as P
from buzzdetect_amd import _lib, pitch

W = P.WINDOW


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def par(**changes):
    return pitch.params(**{**P.DEFAULTS, **changes})


@pytest.fixture(scope="module")
def cases():
    """(the accuracy cases, what the host routine makes of them: f0, clarity, voiced, frames)."""
    found = P.accuracy_cases()
    chunk = np.concatenate([c[2] for c in found])
    return found, pitch.track_host(chunk, np.arange(len(found)), W, want_frames=True)


def test_every_synthetic_buzz_is_voiced_and_within_3_percent(cases):
    found, (f0, clarity, voiced, frames) = cases
    assert len(found) == 6 * 3 * 2 * 2
    for k, (name, nominal, _) in enumerate(found):
        print(name, f0[k], voiced[k], abs(f0[k] / nominal - 1))
        assert voiced[k] == 29, name
        assert abs(f0[k] / nominal - 1) <= 0.03, name
        assert 0.5 <= clarity[k] <= 1.0, name


def test_noise_and_silence_have_no_voiced_frame():
    chunk = np.concatenate([P.noise(1), np.zeros(W, np.float32), P.noise(2, amplitude=0.9)])
    f0, clarity, voiced, frames = pitch.track_host(chunk, [0, 1, 2], W, want_frames=True)
    assert np.array_equal(voiced, [0, 0, 0]) and np.array_equal(bits(f0), [P.QUIET_NAN] * 3) and np.array_equal(bits(clarity), [0] * 3)
    assert not frames[:, :, 0].any() and not frames[1].any()


def test_frames_agree_with_the_float64_statement(cases):
    """At most 1 % of the frames may differ in voicing or integer lag; on the others the relative f0 error against float64 is
    held to 8 x the deviation of a plain float32 NumPy statement of the same definition."""
    found, (_, _, _, frames) = cases
    differ, total, mine, plain = 0, 0, 0.0, 0.0
    for k, (name, _, window) in enumerate(found):
        ref = P.window_numpy(window, P.DEFAULTS, np.float64)[3]
        f32 = P.window_numpy(window, P.DEFAULTS, np.float32)[3]
        for f in range(P.FRAMES):
            total += 1
            voiced, lag, f0, clarity = ref[f]
            got = float(frames[k, f, 0])
            # the host's integer lag is read off its refined f0, which lies within half a lag of it: a pick one lag away with
            # the refinement clamped towards the reference would sit at exactly 0.5 and count as the same lag here; the
            # relative f0 bound below then catches it
            if (got != 0) != voiced or (voiced and abs(P.RATE / got - lag) > 0.5 + 1e-3):
                differ += 1
                continue
            if voiced:
                mine = max(mine, abs(got / f0 - 1))
                assert abs(float(frames[k, f, 1]) - clarity) < 1e-4
                if f32[f][0] and f32[f][1] == lag:
                    plain = max(plain, abs(f32[f][2] / f0 - 1))
    print(f"frames that differ: {differ} of {total}; relative f0 error: host {mine:.3g}, float32 NumPy {plain:.3g}, "
          f"ratio {mine / plain:.3g}")
    assert total == 72 * 29 and differ <= 0.01 * total
    assert plain > 0 and mine <= 8 * plain


@pytest.mark.parametrize("period", (16, 57, 200))
def test_an_exact_period_picks_its_own_lag_not_a_multiple(period):
    """Whole-number samples of exact period T: y[j] == y[j + T] bit for bit, so n is exactly 1 at T, 2 T, ..: the tie rule."""
    f0, clarity, voiced, frames = pitch.track_host(P.periodic(period), [0], W, want_frames=True)
    assert voiced[0] == 29 and np.array_equal(bits(frames[0, :, 1]), bits(np.ones(29)))
    assert (np.abs(P.RATE / frames[0, :, 0] - period) <= 0.5).all()
    assert abs(P.RATE / f0[0] - period) <= 0.5 and clarity[0] == 1.0
    ref = P.window_numpy(P.periodic(period), P.DEFAULTS)
    assert [fr[1] for fr in ref[3]] == [period] * 29


def test_a_constant_frame_is_unvoiced():
    f0, clarity, voiced, frames = pitch.track_host(np.full(W, 3.0, np.float32), [0], W, want_frames=True)
    assert voiced[0] == 0 and bits(f0)[0] == P.QUIET_NAN and not frames.any()


def test_one_nan_spoils_only_the_frames_that_hold_it():
    clean = P.buzz(233.0, P.HARMONICS["five"], seed=5)
    dirty = clean.copy()
    dirty[5000] = np.nan                                   # frames 8 (4096..5119) and 9 (4608..5631)
    a = pitch.track_host(clean, [0], W, want_frames=True)
    b = pitch.track_host(dirty, [0], W, want_frames=True)
    rest = [f for f in range(29) if f not in (8, 9)]
    assert a[2][0] == 29 and b[2][0] == 27
    assert not b[3][0, 8:10].any() and np.array_equal(bits(a[3][0, rest]), bits(b[3][0, rest]))
    ref = P.window_numpy(dirty, P.DEFAULTS)
    assert [fr[0] for fr in ref[3]] == [f not in (8, 9) for f in range(29)]


@pytest.mark.parametrize("n_samples", (0, 1, 1023, 5000, W - 1, W + 1))
def test_a_window_cut_by_the_chunks_end_reads_zeros(n_samples):
    whole = P.buzz(180.0, P.HARMONICS["weak"], seed=9, n=2 * W)
    padded = np.concatenate([whole[:n_samples], np.zeros(3 * W, np.float32)])
    cut = pitch.track_host(whole[:n_samples], [0, 1, 2], W, want_frames=True)
    full = pitch.track_host(padded, [0, 1, 2], W, want_frames=True)
    for a, b in zip(cut, full):
        assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))
    assert cut[2][2] == 0 and bits(cut[0])[2] == P.QUIET_NAN
    if n_samples < 1024:
        assert cut[2][0] <= 2
    if n_samples == 0:
        assert not cut[2].any()


@pytest.mark.parametrize("first, last", ((0, 28), (0, 11), (9, 21), (17, 28)))
def test_frames_that_tie_in_f0_are_ordered_by_frame(first, last):
    """The voiced frames are exactly ``first .. last``, all with the same f0 and pairwise different clarities, so the lower
    median of the order (f0, frame) is frame first + (count - 1) // 2 and no other: an order that broke the tie by the later
    frame, or a rank that counted equals, would carry another frame's clarity.  Odd and even counts, voiced frames at the
    window's start, middle and end; the float64 statement picks the same frame."""
    p = {**P.DEFAULTS, "lag_lo": 20, "lag_hi": 20, "min_voiced": 1}
    window = P.tied_window(first, last)
    f0, clarity, voiced, frames = pitch.track_host(window, [0], W, pitch.params(**p), want_frames=True)
    on = [f for f in range(29) if frames[0, f, 0] != 0]
    assert on == list(range(first, last + 1)) and voiced[0] == last + 1 - first
    assert len(set(bits(frames[0, on, 0]).tolist())) == 1 and len(set(bits(frames[0, on, 1]).tolist())) == len(on)
    assert bits(frames[0, on[0], 0]) == bits(np.float32(P.RATE / 20.5))
    middle = first + (len(on) - 1) // 2
    assert bits(f0)[0] == bits(frames[0, middle, 0]) and bits(clarity)[0] == bits(frames[0, middle, 1])
    want_f0, want_clarity, want_voiced, ref = P.window_numpy(window, p)
    assert [fr[0] for fr in ref] == [f in on for f in range(29)] and want_voiced == len(on)
    assert want_f0 == P.RATE / 20.5 and want_clarity == ref[middle][3]
    assert abs(float(clarity[0]) - want_clarity) < 1e-5 < min(abs(ref[f][3] - want_clarity) for f in on if f != middle)


def test_the_window_takes_the_lower_median_of_distinct_values():
    """Half a window at period 40 and half at period 50, the same reversed, and a window cut after nine frames: frames of many
    different f0 (the refinement moves with the frame's phase).  The window's pair is that of the frame at place
    (voiced - 1) // 2 by value, and the float64 statement picks the same frame."""
    two = np.concatenate([P.periodic(40)[:W // 2], P.periodic(50)[:W // 2]])
    for window in (two, two[::-1].copy(), np.concatenate([P.periodic(57)[:9 * 512], np.zeros(W - 9 * 512, np.float32)])):
        f0, clarity, voiced, frames = pitch.track_host(window, [0], W, par(min_voiced=1), want_frames=True)
        order = sorted((float(frames[0, f, 0]), f) for f in range(29) if frames[0, f, 0] != 0)
        assert len(order) == voiced[0] >= 1
        f = order[(len(order) - 1) // 2][1]
        assert bits(f0)[0] == bits(frames[0, f, 0]) and bits(clarity)[0] == bits(frames[0, f, 1])
        want_f0, want_clarity, want_voiced, ref = P.window_numpy(window, {**P.DEFAULTS, "min_voiced": 1})
        assert want_voiced == voiced[0] and abs(float(f0[0]) / want_f0 - 1) < 1e-5 and abs(float(clarity[0]) - want_clarity) < 1e-5


def test_min_voiced_at_its_limits():
    tone = P.buzz(233.0, seed=3)
    some = np.concatenate([tone[:3 * 512], np.zeros(W - 3 * 512, np.float32)])
    chunk = np.concatenate([tone, some])
    f0, _, voiced = pitch.track_host(chunk, [0, 1], W, par(min_voiced=1))
    assert voiced[0] == 29 and 1 <= voiced[1] < 29 and not np.isnan(f0).any()
    f0, clarity, again = pitch.track_host(chunk, [0, 1], W, par(min_voiced=29))
    assert np.array_equal(again, voiced) and not np.isnan(f0[0]) and bits(f0)[1] == P.QUIET_NAN and bits(clarity)[1] == 0


@pytest.mark.parametrize("lags", ((1, 1), (1, 511), (511, 511), (16, 200)))
def test_lag_ranges_agree_with_the_float64_statement(lags):
    p = {**P.DEFAULTS, "lag_lo": lags[0], "lag_hi": lags[1]}
    windows = [P.buzz(233.0, P.HARMONICS["five"], seed=11), P.periodic(2), P.periodic(511), P.buzz(40.0, seed=12), P.noise(13),
               P.buzz(7000.0, seed=14)]
    f0, clarity, voiced, frames = pitch.track_host(np.concatenate(windows), np.arange(len(windows)), W, par(lag_lo=lags[0], lag_hi=lags[1]),
                                                   want_frames=True)
    # lag_hi = 1 can voice nothing: the lobe must end at lag 1 for the search to start there, and then n[1] < 0 is the maximum
    assert (voiced.sum() == 0) if lags == (1, 1) else (voiced == 29).any()
    differ = 0
    for k, window in enumerate(windows):
        ref = P.window_numpy(window, p)
        for f in range(29):
            was, lag, want, c = ref[3][f]
            got = float(frames[k, f, 0])
            if (got != 0) != was or (was and abs(P.RATE / got - lag) > 0.5 + 1e-3):
                differ += 1
            elif was:
                assert abs(got / want - 1) < 1e-4 and lags[0] - 0.5 <= P.RATE / got <= lags[1] + 0.5
    assert differ <= 0.01 * 29 * len(windows)


def test_the_result_of_a_window_does_not_depend_on_sel():
    chunk = np.concatenate([P.buzz(110.0, seed=1), P.noise(2), P.buzz(470.0, P.HARMONICS["weak"], seed=3)])[:-700]
    alone = [pitch.track_host(chunk, [k], 7680, want_frames=True) for k in range(6)]
    sel = [5, 0, 3, 3, -1, 6, 2, 1 << 30, 4, 1, 0, -(1 << 31)]
    got = pitch.track_host(chunk, sel, 7680, want_frames=True)
    for at, k in enumerate(sel):
        if 0 <= k < 6:
            for a, b in zip(got, alone[k]):
                assert np.array_equal(np.asarray(a[at]).view(np.uint32), np.asarray(b[0]).view(np.uint32))
        else:
            assert got[2][at] == 0 and bits(got[0])[at] == P.QUIET_NAN and not got[3][at].any()


@pytest.mark.parametrize("changes, word", (({"lag_lo": 0}, "lag_lo"), ({"lag_lo": 201}, "lag_lo"), ({"lag_hi": 512}, "lag_hi"),
                                           ({"pick_ratio": 0.0}, "pick_ratio"), ({"pick_ratio": 1.5}, "pick_ratio"),
                                           ({"clarity_min": 0.0}, "clarity_min"), ({"clarity_min": float("nan")}, "clarity_min"),
                                           ({"min_voiced": 0}, "min_voiced"), ({"min_voiced": 30}, "min_voiced"),
                                           ({"rate_hz": 0.0}, "rate_hz")))
def test_refused_parameters_name_the_argument(changes, word):
    with pytest.raises(_lib.BuzzdetectHipError, match=word):
        pitch.track_host(np.zeros(100, np.float32), [0], W, par(**changes))


def test_refused_arguments_name_the_argument():
    lib = _lib.load()
    x, sel, values, voiced = np.zeros(100, np.float32), np.zeros(4, np.int32), np.zeros((4, 2), np.float32), np.zeros(4, np.int32)
    p = par()

    def call(n_samples=100, n_sel=4, step=W, x_at=x.ctypes.data, sel_at=sel.ctypes.data, p_at=C.addressof(p), values_at=values.ctypes.data,
             voiced_at=voiced.ctypes.data, frames_at=None):
        rc = lib.bd_pitch_windows_host(x_at, n_samples, sel_at, n_sel, step, p_at, values_at, voiced_at, frames_at)
        return rc, lib.bd_last_error().decode()

    assert call()[0] == 0
    for kwargs, word in (({"n_sel": -1}, "n_sel"), ({"n_sel": _lib.PITCH_MAX_SELECTED + 1}, "n_sel"), ({"n_samples": -1}, "n_samples"),
                         ({"step": 0}, "step_samples"), ({"step": _lib.PITCH_MAX_STEP + 1}, "step_samples"), ({"p_at": None}, "params"),
                         ({"x_at": None}, "x is"), ({"sel_at": None}, "sel is"), ({"values_at": None}, "values is"),
                         ({"voiced_at": None}, "voiced is"), ({"frames_at": values.ctypes.data + 2}, "frames is")):
        rc, text = call(**kwargs)
        assert rc == -1 and word in text, (kwargs, text)
    values[:] = 7
    assert call(n_sel=0, sel_at=None, values_at=None, voiced_at=None)[0] == 0 and (values == 7).all()       # nothing written
    with pytest.raises(ValueError, match="fmin"):
        pitch.lag_range(10.0, 1000.0)
    assert pitch.lag_range(80.0, 1000.0) == (16, 200)


def test_event_wingbeats_on_hand_made_tables():
    nan = np.nan
    #                 0    1      2      3    4      5      6    7    8      9
    f0 = np.array([nan, 200.0, 210.0, nan, 190.0, 205.0, nan, nan, 300.0, 300.0], np.float32)
    clarity = np.array([0, 0.9, 0.8, 0, 0.7, 0.6, 0, 0, 0.5, 0.4], np.float32)
    marks = np.array([0, 3, 2, 2, 0, 2, 0, 3, 3, 2], np.uint8)
    rows = np.array([[1, 5, 4, 2, 1],        # ON 1, 2, 3, 5 (4 is OFF, 3 unvoiced): 200, 210, 205 -> median 205
                     [7, 7, 1, 7, 1],        # its one window is unvoiced
                     [8, 9, 2, 8, 1]],       # 300, 300: the tie goes to the earlier window
                    np.int32)
    got = pitch.event_wingbeats(rows, marks, f0, clarity)
    assert got[0] == (205.0, 200.0, 210.0, float(np.float32(0.6)), 3)
    assert np.isnan(got[1][:3]).all() and got[1][3:] == (0.0, 0)
    assert got[2] == (300.0, 300.0, 300.0, 0.5, 2)
    assert pitch.event_wingbeats(rows[:1, :], marks, np.where(np.arange(10) == 5, nan, f0).astype(np.float32), clarity)[0] \
        == (200.0, 200.0, 210.0, float(np.float32(0.9)), 2)                                           # even count: the lower one
    assert pitch.event_wingbeats(np.zeros((0, 5), np.int32), marks, f0, clarity) == []
    assert pitch.lower_median(np.array([3.0, 1.0, 1.0, 2.0])) == 2


def test_a_result_writes_and_reads_back_and_a_store_is_refused(tmp_path):
    import pandas as pd
    f32 = lambda v: float(np.float32(v))
    result = pitch.WingbeatResult(["ins_buzz"], [[("a", 2.88, 7.68, 5, 5, 3.97, 2.88, f32(181.3), f32(180.1), f32(183.2), f32(0.93), 5),
                                                  ("site/b", 1.0, 1.96, 1, 1, 1.234, 1.0, float("nan"), float("nan"), float("nan"), 0.0, 0)]],
                                  idents=["a", "quiet", "site/b"])
    assert result.calls() == [[("a", 2.88, 7.68, 5, 5, 3.97, 2.88), ("site/b", 1.0, 1.96, 1, 1, 1.234, 1.0)]]
    table = result.table()
    assert table.dtype.names[2:] == pitch.WINGBEAT_COLUMNS[1:] and list(table["ident"]) == ["a", "site/b"]
    result.to_csv(str(tmp_path))
    back = {i: pd.read_csv(tmp_path / (i + pitch.SUFFIX_WINGBEAT)) for i in result.idents}
    assert all(list(t.columns) == list(pitch.WINGBEAT_COLUMNS) for t in back.values()) and len(back["quiet"]) == 0
    assert np.float32(back["a"].f0[0]) == np.float32(181.3) and np.float32(back["a"].clarity[0]) == np.float32(0.93)
    assert back["a"].peak[0] == 3.97 and back["a"].voiced_windows[0] == 5 and back["a"].start[0] == 2.88
    assert np.isnan(back["site/b"].f0[0]) and np.isnan(back["site/b"].f0_max[0]) and back["site/b"].voiced_windows[0] == 0
    deep = "/".join(c * 120 for c in "abc")                              # an ident of 362 characters keeps its rows
    long = pitch.WingbeatResult(["ins_buzz"], [[(deep,) + result.events[0][0][1:]]], idents=[deep])
    long.to_csv(str(tmp_path / "long"))
    assert len(pd.read_csv(tmp_path / "long" / (deep + pitch.SUFFIX_WINGBEAT))) == 1 and long.table()["ident"][0] == deep
    (tmp_path / "emb").mkdir()
    (tmp_path / "emb" / "store.json").write_text("{}")
    with pytest.raises(ValueError, match="holds no audio"):
        pitch.wingbeat_recordings(str(tmp_path / "emb"), thresholds={"ins_buzz": 0.0})
