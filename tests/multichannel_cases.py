"""Inputs shared by tests/test_multichannel_host.py and tests/test_multichannel_gpu.py (a plain module, like gpu_guards.py):
[n, C] signals whose channels can be told apart, and one filter design per rate ratio for the float64 oracle."""
import functools

import numpy as np

from oracle import resample_oracle as RO

DC = 0.25                          # on the last channel: a dropped, repeated or mis-strided channel moves the mean by >= DC / C


def marked(n, channels, seed):
    """float32 [n, C]: channel c is independent noise of amplitude 0.1 (c + 1) / C, the last channel carries DC on top.  The
    mean stays inside (-1, 1); leaving a channel out, reading one twice or dividing by another count moves it by DC / C or
    more (0.03 at eight channels), four orders above any tolerance of the resampler tests."""
    rng = np.random.default_rng(seed)
    amp = 0.1 * (np.arange(channels) + 1.0) / channels
    x = rng.standard_normal((n, channels)) * amp
    x[:, -1] += DC
    return x.astype(np.float32)


def marked_s16(n, channels, seed):
    """The same signal as 16-bit PCM."""
    return (np.clip(marked(n, channels, seed), -1.0, 1.0 - 2.0 ** -15) * 32768.0).round().astype(np.int16)


def full_scale_s16(n, channels, seed):
    """Uniform full-scale integers with two runs of frames at +32767 and -32768 on every channel (test_resample.py's
    test_s16_pcm_is_exact_in_the_split), the runs scaled to the length."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-32768, 32767, size=(n, channels), dtype=np.int16)
    q[n // 30:n // 10] = 32767
    q[n // 10:n // 6] = -32768
    return q


def as_float(x):
    """What the device stage makes of 16-bit PCM before the mean: value / 32768 in float32 (libsndfile's float read)."""
    x = np.asarray(x)
    return x.astype(np.float32) / 32768.0 if x.dtype == np.int16 else x


def in_order_mean(x):
    """The float32 channel mean as one running sum in channel order and one division."""
    x = as_float(x)
    m = np.zeros(x.shape[0], np.float32)
    for c in range(x.shape[1]):
        m = m + x[:, c]
    return m / np.float32(x.shape[1])


def row_sum_mean(x):
    """np_row_sum (buzzdetect_amd/csrc/bd_internal.h) over the count, one float32 operation at a time: the running sum below
    eight channels; from eight on eight running sums over blocks of eight, folded as a tree, the rest in order."""
    x = as_float(x)
    n = x.shape[1]
    if n < 8:
        return in_order_mean(x)
    r = [x[:, k] for k in range(8)]
    i = 8
    while i + 8 <= n:
        r = [r[k] + x[:, i + k] for k in range(8)]
        i += 8
    s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for c in range(i, n):
        s = s + x[:, c]
    assert s.dtype == np.float32
    return (np.float32(0.0) + s) / np.float32(n)


_taps = functools.lru_cache(maxsize=4)(RO.taps)


def oracle(x, rate_in, quality="hq"):
    """RO.resample (np.mean(axis=1) in float32, then the float64 filter) with the filter of a ratio designed once per run:
    RO.taps takes seconds for an irreducible ratio.  The cached arrays are only read."""
    saved = RO.taps
    RO.taps = _taps
    try:
        return RO.resample(as_float(x), rate_in, quality=quality)
    finally:
        RO.taps = saved
