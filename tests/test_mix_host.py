"""bd_mix_host (include/buzzdetect_mix.h, csrc/mixaug.hip) against a float64 NumPy mix: no device.

The SNR a mixture achieves, 10 log10(sum (a ev)^2 / sum (b nz)^2) with the sums in float64, must lie within 1e-3 dB of the
request.  The float32 power sums (256 chains of at most 16 fused multiply-adds per slice, an 8-level tree, at most 64 slices
in ascending order for 2^18 samples) err by about 1e-6 relative, about 1e-5 dB, so the bound leaves two orders of margin and
still fails for any wrong formula (the nearest wrong ones - power for amplitude, the gain on one part only - are dBs away).
Every case prints what it observed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from buzzdetect_amd import _lib, build, dataset

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "buzzdetect_mix.h")
BOUND_DB = 1e-3


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def sources(n, seed, ev_scale=0.2, nz_scale=0.05):
    rng = np.random.default_rng(seed)
    t = np.arange(n + 64) / 16000.0
    ev = (ev_scale * np.sin(2 * np.pi * 220.0 * t) * (1 + 0.3 * rng.normal(size=t.size))).astype(np.float32)
    nz = (nz_scale * rng.normal(size=n + 77)).astype(np.float32)
    return ev, nz


def achieved_db(out, ev, nz, clip, power):
    """The event and background parts of the mixture, separated with the b the library's own (Pe, Pn) imply, in float64."""
    n, eo, zo = int(clip["n"]), int(clip["ev_off"]), int(clip["nz_off"])
    e, z = ev[eo:eo + n].astype(np.float64), nz[zo:zo + n].astype(np.float64)
    a = float(clip["ev_gain"])
    mixed = out[int(clip["out_off"]): int(clip["out_off"]) + n].astype(np.float64)
    part_b = mixed - a * e                                   # = b nz up to the output's float32 rounding
    b = float(part_b @ z / (z @ z))
    return 10 * np.log10(np.sum((a * e) ** 2) / np.sum((b * z) ** 2)), b


def test_header_and_binding_list_the_same_functions_and_constants(lib):
    text = open(HEADER).read()
    names = sorted(set(re.findall(r"^BD_API[^;(]*?\b(bd_[a-z_0-9]+)\s*\(", text, flags=re.M)))
    assert names == sorted(_lib.MIX_PROTOTYPES)
    consts = dict(re.findall(r"#define\s+(BD_MIX_[A-Z_]+)\s+([-0-9.ef]+)", text))
    assert int(consts["BD_MIX_SLICE"]) == _lib.MIX_SLICE and int(consts["BD_MIX_ABI_VERSION"]) == _lib.MIX_ABI_VERSION
    assert float(consts["BD_MIX_POWER_FLOOR"].rstrip("f")) == _lib.MIX_POWER_FLOOR
    assert int(consts["BD_MIX_FLAG_SILENT_BACKGROUND"]) == _lib.MIX_FLAG_SILENT_BACKGROUND
    assert int(consts["BD_MIX_MAX_CLIPS"]) == _lib.MIX_MAX_CLIPS
    assert lib.bd_mix_abi_version() == _lib.MIX_ABI_VERSION and C.sizeof(_lib.bd_mix_clip) == 40


@pytest.mark.parametrize("n", (15360, 3 * _lib.MIX_SLICE + 5, 1 << 18))
@pytest.mark.parametrize("snr_db,gain_db", [(-10.0, 0.0), (0.0, 0.0), (20.0, 0.0), (5.0, -6.0)])
def test_requested_snr_is_reached(lib, n, snr_db, gain_db):
    ev, nz = sources(n, seed=n % 1000 + int(snr_db))
    clips = dataset.mix_descriptors([33], [41], [n], [snr_db], [gain_db])
    out, power, flags = dataset.mix_host(ev, nz, clips)
    got, b = achieved_db(out, ev, nz, clips[0], power[0])
    e, z = ev[33:33 + n].astype(np.float64), nz[41:41 + n].astype(np.float64)
    pe, pn = np.mean(e * e), np.mean(z * z)
    a = 10.0 ** (gain_db / 20.0)
    ref = a * e + 10.0 ** (-snr_db / 20.0) * np.sqrt(pe / pn) * a * z
    print(f"n={n} snr={snr_db:+.0f} dB gain={gain_db:+.0f} dB: achieved {got:+.7f} dB, deviation {got - snr_db:+.2e} dB; "
          f"Pe rel err {abs(power[0, 0] - pe) / pe:.2e}, Pn rel err {abs(power[0, 1] - pn) / pn:.2e}; "
          f"max|out - f64 mix| = {np.abs(out - ref).max():.2e}")
    assert flags[0] == 0
    assert abs(got - snr_db) <= BOUND_DB
    assert abs(power[0, 0] - pe) <= 1e-5 * pe and abs(power[0, 1] - pn) <= 1e-5 * pn
    # b carries half of each power sum's relative error (worst case (16 + 8 + 64) roundings of 2^-24 each = 5.2e-6) and three
    # roundings of its own, the output two more: 6e-6 of the largest value
    assert np.abs(out - ref).max() <= 6e-6 * np.abs(ref).max()
    # the gain moves both parts: the event part alone is a ev
    assert np.abs((out.astype(np.float64) - b * z) - a * e).max() <= 1e-6


def test_ratio_zero_is_the_event_alone(lib):
    ev, nz = sources(5000, seed=1)
    clips = dataset.mix_descriptors([3], [5], [5000], [np.inf], [-6.0])
    assert clips["ratio"][0] == 0.0
    out, power, flags = dataset.mix_host(ev, nz, clips)
    assert flags[0] == 0 and power[0, 1] > 0
    assert out.tobytes() == (clips["ev_gain"][0] * ev[3:5003]).astype(np.float32).tobytes()
    print(f"ratio 0: output is ev_gain * ev bit for bit; ev_gain = {clips['ev_gain'][0]:.7f}")


def test_silent_background_sets_the_flag_and_adds_nothing(lib):
    ev, nz = sources(5000, seed=2)
    nz[:] = 0.0
    nz[100:200] = 1e-12                                       # mean square 2e-26: below the floor, yet not zero
    clips = dataset.mix_descriptors([0], [0], [5000], [0.0], [0.0])
    out, power, flags = dataset.mix_host(ev, nz, clips)
    print(f"silent background: Pn = {power[0, 1]:.3e} (floor {_lib.MIX_POWER_FLOOR:.0e}), flags = {flags[0]}")
    assert flags[0] == _lib.MIX_FLAG_SILENT_BACKGROUND and power[0, 1] < _lib.MIX_POWER_FLOOR
    assert out.tobytes() == ev[:5000].tobytes()


def test_silent_event_gets_no_background(lib):
    ev, nz = sources(5000, seed=3)
    ev[:] = 0.0
    clips = dataset.mix_descriptors([0], [0], [5000], [0.0], [0.0])
    out, power, flags = dataset.mix_host(ev, nz, clips)
    assert flags[0] == 0 and power[0, 0] == 0.0 and not out.any() and np.isfinite(out).all()


def test_bad_descriptors_are_refused_and_named(lib):
    ev, nz = sources(1000, seed=4)
    out = np.full(2000, 7.0, np.float32)

    def refuse(match, **fields):
        clips = dataset.mix_descriptors([0, 10], [0, 10], [500, 500], [0.0, 0.0], [0.0, 0.0])
        for k, v in fields.items():
            clips[k][1] = v
        with pytest.raises(_lib.BuzzdetectHipError, match=match) as err:
            dataset.mix_host(ev, nz, clips, out=out)
        assert err.value.code == -1 and "clip 1" in str(err.value)
        assert (out == 7.0).all()                             # nothing was written, clip 0 included

    refuse("event range", ev_off=ev.size - 499)
    refuse("background range", nz_off=nz.size - 499)
    refuse("output range", out_off=out.size - 499)
    refuse("n < 1", n=0)
    refuse("negative offset", nz_off=-1)
    refuse("overlaps", out_off=499)
    refuse("finite", ratio=np.float32(np.nan))
    assert lib.bd_mix_workspace_bytes(None, 0) == 256
    none = np.zeros(0, dataset.MIX_CLIP)
    dataset.mix_host(ev, nz, none, out=out)                   # no clips: nothing happens
    assert (out == 7.0).all()
