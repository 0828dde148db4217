"""Cases for the pitch tests (a plain module): a seeded generator of synthetic buzzes, and a NumPy restatement of the definition
in include/buzzdetect_pitch.h written from the definition (sums as NumPy takes them), in float64 as the oracle and in float32 as
the yardstick of what a change of summation order alone does."""
import numpy as np

from buzzdetect_amd import _lib

RATE = 16000.0
WINDOW = _lib.PITCH_WINDOW
FRAMES = _lib.PITCH_FRAMES
FRAME = _lib.PITCH_FRAME
HALF = _lib.PITCH_INTEGRATION
QUIET_NAN = 0x7FC00000

FUNDAMENTALS = (85.0, 110.0, 180.0, 233.0, 470.0, 990.0)
HARMONICS = {"five": (1.0, 0.5, 0.33, 0.25, 0.2), "weak": (0.15, 1.0, 0.7, 0.5, 0.35), "pure": (1.0,)}
SNRS_DB = (20.0, 3.0)
DCS = (0.0, 2.0)
DEFAULTS = dict(lag_lo=16, lag_hi=200, pick_ratio=0.8, clarity_min=0.5, min_voiced=8, rate_hz=RATE)


def buzz(f0, harmonics=(1.0,), vibrato=0.02, snr_db=20.0, dc=0.0, seed=0, n=WINDOW, amplitude=0.1, vibrato_hz=6.0):
    """float32 [n]: harmonics h = 1, 2, .. of amplitudes ``harmonics`` (scaled so that the strongest is ``amplitude``) on a
    fundamental that swings by +/- ``vibrato`` (a fraction) at ``vibrato_hz``, random phases, white noise ``snr_db`` below the
    signal's power, and an offset of ``dc`` times the amplitude."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / RATE
    inst = f0 * (1.0 + vibrato * np.sin(2 * np.pi * vibrato_hz * t + rng.uniform(0, 2 * np.pi)))
    phase = 2 * np.pi * np.cumsum(inst) / RATE
    a = np.asarray(harmonics, np.float64)
    a = amplitude * a / a.max()
    s = sum(ah * np.sin((h + 1) * phase + rng.uniform(0, 2 * np.pi)) for h, ah in enumerate(a))
    noise = rng.standard_normal(n) * np.sqrt(np.mean(s * s) / 10.0 ** (snr_db / 10.0))
    return (s + noise + dc * amplitude).astype(np.float32)


def noise(seed=0, n=WINDOW, amplitude=0.1):
    return (amplitude * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def accuracy_cases():
    """(name, nominal f0, window) over the fundamentals, harmonic sets, SNRs and offsets, with +/- 2 % vibrato."""
    out = []
    for i, f0 in enumerate(FUNDAMENTALS):
        for j, (hname, h) in enumerate(HARMONICS.items()):
            for k, snr in enumerate(SNRS_DB):
                for l, dc in enumerate(DCS):
                    out.append((f"{f0:g}Hz-{hname}-{snr:g}dB-dc{dc:g}", f0,
                                buzz(f0, h, 0.02, snr, dc, seed=1000 + ((i * 3 + j) * 2 + k) * 2 + l)))
    return out


def window_of(x, k, step):
    """Window k of chunk x as the definition reads it: zero at and beyond the chunk's end, silence for a negative k."""
    out = np.zeros(WINDOW, x.dtype)
    lo = int(k) * int(step)
    if k >= 0 and lo < x.shape[0]:
        part = x[lo:lo + WINDOW]
        out[:part.shape[0]] = part
    return out


def frame_numpy(frame, p, dtype=np.float64):
    """One frame by the definition: (voiced, lag i or -1, f0 or 0, clarity), every sum a NumPy sum in ``dtype``."""
    lag_lo, lag_hi = p["lag_lo"], p["lag_hi"]
    x = np.asarray(frame).astype(dtype)
    with np.errstate(all="ignore"):
        mu = x.sum(dtype=dtype) / dtype(FRAME)
        y = x - mu
        shifted = np.lib.stride_tricks.sliding_window_view(y, HALF)[:lag_hi + 2]                  # [tau, j] = y[j + tau]
        cross = (shifted * y[:HALF]).sum(axis=1, dtype=dtype)
        energy = (shifted * shifted).sum(axis=1, dtype=dtype)
        m = energy[0] + energy
        if not (np.isfinite(x).all() and np.isfinite(mu) and np.isfinite(m).all()):
            return False, -1, 0.0, 0.0
        n = np.where(m > 0, dtype(2) * cross / np.where(m > 0, m, 1), dtype(0)).astype(dtype)
    below = np.flatnonzero(n[1:lag_hi + 1] < 0)
    if below.size == 0:
        return False, -1, 0.0, 0.0
    s = max(lag_lo, int(below[0]) + 1)
    if s > lag_hi:
        return False, -1, 0.0, 0.0
    nmax = n[s:lag_hi + 1].max()
    if not nmax >= dtype(p["clarity_min"]):
        return False, -1, 0.0, float(nmax)
    thr = dtype(p["pick_ratio"]) * nmax
    j = s + int(np.flatnonzero(n[s:lag_hi + 1] >= thr)[0])
    e = j
    while e + 1 <= lag_hi and n[e + 1] >= thr:
        e += 1
    i = j + int(np.argmax(n[j:e + 1]))                                                           # (the first of equal maxima)
    den = n[i - 1] - dtype(2) * n[i] + n[i + 1]
    d = dtype(0)
    if den < 0:
        d = min(max(dtype(0.5) * (n[i - 1] - n[i + 1]) / den, dtype(-0.5)), dtype(0.5))
    return True, i, float(dtype(p["rate_hz"]) / (dtype(i) + d)), float(n[i])


def window_numpy(window, p, dtype=np.float64):
    """A window by the definition: (f0 or NaN, clarity, voiced, frames) with frames a list of ``frame_numpy``'s tuples."""
    frames = [frame_numpy(window[HALF * f:HALF * f + FRAME], p, dtype) for f in range(FRAMES)]
    voiced = [(fr[2], f) for f, fr in enumerate(frames) if fr[0]]
    if len(voiced) < p["min_voiced"]:
        return float("nan"), 0.0, len(voiced), frames
    _, f = sorted(voiced)[(len(voiced) - 1) // 2]
    return frames[f][2], frames[f][3], len(voiced), frames


def periodic(period, n=WINDOW, seed=0, amplitude=1000):
    """float32 [n] of whole numbers with the exact period ``period``: a rounded sine, so that the lag-0 lobe ends before it."""
    base = np.round(amplitude * np.sin(2 * np.pi * (np.arange(period) + 0.25) / period))
    return np.tile(base, n // period + 1)[:n].astype(np.float32)


def tied_window(first, last):
    """A 776.7 Hz tone (period 20.6 samples) over frames ``first .. last`` of a window, silence around it (frame ``last``
    holds it in its first half only and is still voiced).  Tracked at lag_lo = lag_hi = 20 the refinement is clamped at +0.5 in every voiced frame, so all of them have f0 = 16000 / 20.5 in the
    same bits while the noise gives each its own clarity: a tie whose order shows in the window's clarity."""
    x = buzz(RATE / 20.6, (1.0,), vibrato=0.0, snr_db=20.0, seed=3)
    x[:first * 512] = 0
    x[(last + 1) * 512:] = 0
    return x
