"""Cases and independent NumPy statements for recording health (include/buzzdetect_health.h), shared by the host and the GPU
tests: the levels as a sequential per-sample loop over maximal runs (sums in float64), the spectrum through np.fft.rfft in
float64, a plain float32 radix-2 transform as the yardstick of float32 error (not the header's algorithm: complex64 arithmetic,
twiddles from np.exp, stages as array operations), and the chunks the run rules are constructed on."""
import numpy as np

from buzzdetect_amd import health

SEG = 4096
FRAME, HOP, BINS = 1024, 512, 513
CLIP_RUN, FLAT_RUN = 3, 8
S16_PARAMS = dict(clip_hi=32767.0 / 32768.0, clip_lo=-1.0, clip_run=CLIP_RUN, flat_run=FLAT_RUN)
INT_FIELDS = ("n", "nonfinite", "n_full", "clipped", "clip_runs", "flat", "flat_runs")


def params(**changes):
    return health.level_params(**{**S16_PARAMS, **changes})


def maximal_edges(n, seg=SEG):
    return np.concatenate([np.arange(0, n, seg), [n]]).astype(np.int64)


def ones_edges(n):
    return np.arange(n + 1, dtype=np.int64)


def random_edges(n, seed, seg=SEG):
    rng = np.random.default_rng(seed)
    edges = [0]
    while edges[-1] < n:
        edges.append(min(n, edges[-1] + int(rng.choice([1, 2, 15, 16, 17, 255, 256, 257, 1000, seg - 1, seg]))))
    return np.asarray(edges, np.int64)


def as_float(x):
    """How a chunk enters: int16 * 2^-15; a non-finite float32 as +0.0 (and where those were)."""
    if x.dtype == np.int16:
        return x.astype(np.float32) * np.float32(2.0 ** -15), np.zeros(x.shape, bool)
    bad = ~np.isfinite(x)
    return np.where(bad, np.float32(0), x).astype(np.float32), bad


def run_marks(member, key, need):
    """Sequentially over one channel: (the samples in maximal runs of at least ``need`` members with equal keys, the first
    samples of those runs)."""
    n = member.shape[0]
    counted, first = np.zeros(n, bool), np.zeros(n, bool)
    i = 0
    while i < n:
        if not member[i]:
            i += 1
            continue
        j = i + 1
        while j < n and member[j] and key[j] == key[j - 1]:
            j += 1
        if j - i >= need:
            counted[i:j] = True
            first[i] = True
        i = j
    return counted, first


def levels_numpy(x, edges, clip_hi, clip_lo, clip_run, flat_run):
    """{field: [S, ch]}: integers exactly, peak as float32, sum / sumsq in float64, abs / sq: the sums of |x| and x^2 in float64."""
    x = x[:, None] if x.ndim == 1 else x
    v, bad = as_float(x)
    s, ch = edges.shape[0] - 1, x.shape[1]
    out = {k: np.zeros((s, ch), np.int64) for k in INT_FIELDS}
    out.update(peak=np.zeros((s, ch), np.float32), sum=np.zeros((s, ch)), sumsq=np.zeros((s, ch)), abs=np.zeros((s, ch)), sq=np.zeros((s, ch)))
    hi, lo = np.float32(clip_hi), np.float32(clip_lo)
    for c in range(ch):
        col = v[:, c]
        zero = np.zeros(col.shape[0], np.uint32)
        marks = [run_marks(col >= hi, zero, clip_run), run_marks(col <= lo, zero, clip_run),
                 run_marks(np.ones(col.shape[0], bool), col.view(np.uint32), flat_run)]
        for k in range(s):
            a, b = int(edges[k]), int(edges[k + 1])
            part = col[a:b].astype(np.float64)
            out["n"][k, c] = b - a
            out["nonfinite"][k, c] = bad[a:b, c].sum()
            out["peak"][k, c] = np.abs(col[a:b]).max()
            out["sum"][k, c], out["sumsq"][k, c] = part.sum(), (part * part).sum()
            out["abs"][k, c], out["sq"][k, c] = np.abs(part).sum(), (part * part).sum()
            out["n_full"][k, c] = ((col[a:b] >= hi) | (col[a:b] <= lo)).sum()
            out["clipped"][k, c] = marks[0][0][a:b].sum() + marks[1][0][a:b].sum()
            out["clip_runs"][k, c] = marks[0][1][a:b].sum() + marks[1][1][a:b].sum()
            out["flat"][k, c] = marks[2][0][a:b].sum()
            out["flat_runs"][k, c] = marks[2][1][a:b].sum()
    return out


def live(n, ch, seed, dtype=np.int16):
    """Noise well inside full scale in which no two neighbours of a channel are equal."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-12000, 12000, size=(n, ch)).astype(np.int16)
    same = np.flatnonzero((x[1:] == x[:-1]).any(axis=1)) + 1
    x[same] += 1 + (same % 2)[:, None].astype(np.int16) * 2            # (an odd and an even step: neighbours of neighbours stay apart)
    while (x[1:] == x[:-1]).any():
        at = np.flatnonzero((x[1:] == x[:-1]).any(axis=1)) + 1
        x[at] += 5
    return x if dtype == np.int16 else (x.astype(np.float32) / np.float32(32768.0))


CONSTRUCTED_N = 5 * SEG + 700


def constructed():
    """(int16 [21180, 4], expected chunk totals per channel {field: [4]}), for clip_run = 3 and flat_run = 8, by construction:
    ch0  plateaus of 1, 2, 3, 4 samples at +FS (from 100, 110, 120, 130) and at -FS (200 ..): only those of 3 and 4 count;
         3 high directly followed by 3 low (300..305): two runs; a high run 4090..4095 (it ends with segment 0);
         stuck stretches of 7, 8 and 9 samples of 8192 (1000, 1100, 1200): those of 8 and 9 count
    ch1  a high run 4090..4096 (one sample into segment 1); a low run 8189..20481: through the whole segments 2, 3 and 4
    ch2  a high run 4090..4097: 8 samples, so it is a stuck run too
    ch3  dead: zeros, one stuck run that is the whole chunk"""
    n = CONSTRUCTED_N
    x = live(n, 4, seed=77)
    hi, lo = np.int16(32767), np.int16(-32768)
    for k, at in enumerate((100, 110, 120, 130)):
        x[at:at + k + 1, 0] = hi
        x[at + 100:at + 100 + k + 1, 0] = lo
    x[300:303, 0], x[303:306, 0] = hi, lo
    x[4090:4096, 0] = hi
    for k, at in enumerate((1000, 1100, 1200)):
        x[at:at + 7 + k, 0] = 8192
    x[4090:4097, 1] = hi
    x[8189:20482, 1] = lo
    x[4090:4098, 2] = hi
    x[:, 3] = 0
    want = {
        "n_full": [2 * (1 + 2 + 3 + 4) + 6 + 6, 7 + 12293, 8, 0],
        "clipped": [2 * (3 + 4) + 6 + 6, 7 + 12293, 8, 0],
        "clip_runs": [4 + 2 + 1, 2, 1, 0],
        "flat": [8 + 9, 12293, 8, n],
        "flat_runs": [2, 1, 1, 1],
        "nonfinite": [0, 0, 0, 0],
        "n": [n] * 4,
    }
    return x, {k: np.asarray(v, np.int64) for k, v in want.items()}


def records_fields(records):
    """A RECORD array [S, ch] as {field: [S, ch]}."""
    return {k: records[k] for k in records.dtype.names}


# ---------------------------------------------------------------------------------------------------- spectrum
def frames_of(n):
    return (n - FRAME) // HOP + 1 if n >= FRAME else 0


def frame_edges(frames, length, seed=None):
    if seed is None:
        return np.concatenate([np.arange(0, frames, length), [frames]]).astype(np.int64) if frames else np.zeros(1, np.int64)
    rng = np.random.default_rng(seed)
    edges = [0]
    while edges[-1] < frames:
        edges.append(min(frames, edges[-1] + int(rng.integers(1, length + 1))))
    return np.asarray(edges, np.int64)


def hann(dtype=np.float64):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(FRAME) / FRAME)).astype(dtype)


def frame_powers_f64(x):
    """P [F, 513] in float64 through np.fft.rfft, and which frames hold a non-finite sample."""
    f = frames_of(x.shape[0])
    w = hann()
    idx = HOP * np.arange(f)[:, None] + np.arange(FRAME)[None, :]
    fr = x.astype(np.float64)[idx] if f else np.zeros((0, FRAME))
    bad = ~np.isfinite(fr).all(axis=1)
    spec = np.fft.rfft(np.where(bad[:, None], 0.0, fr) * w, axis=1)
    c = np.full(BINS, 2.0)
    c[0] = c[-1] = 1.0
    return c * (spec.real ** 2 + spec.imag ** 2) / (FRAME * (w * w).sum()), bad


def fft_radix2_f32(y):
    """A plain float32 radix-2 transform of the rows of y [F, 1024]: complex64 throughout."""
    n = y.shape[1]
    bits = n.bit_length() - 1
    rev = np.array([int(format(i, f"0{bits}b")[::-1], 2) for i in range(n)])
    z = y[:, rev].astype(np.complex64)
    for s in range(bits):
        half = 1 << s
        tw = np.exp(-2j * np.pi * np.arange(half) / (2 * half)).astype(np.complex64)
        z = z.reshape(y.shape[0], -1, 2, half)
        t = (z[:, :, 1, :] * tw).astype(np.complex64)
        z = np.stack([z[:, :, 0, :] + t, z[:, :, 0, :] - t], axis=2).astype(np.complex64).reshape(y.shape[0], n)
    return z


def frame_powers_f32(x):
    """The same definition in plain float32 NumPy over fft_radix2_f32 (finite input)."""
    f = frames_of(x.shape[0])
    w = hann(np.float32)
    idx = HOP * np.arange(f)[:, None] + np.arange(FRAME)[None, :]
    z = fft_radix2_f32(x.astype(np.float32)[idx] * w)[:, :BINS]
    c = np.full(BINS, 2.0, np.float32)
    c[0] = c[-1] = 1.0
    return (c * (z.real * z.real + z.imag * z.imag) * np.float32(1.0 / (FRAME * 384.0))).astype(np.float32)


def band_sums(p, bad, fedges, bedges, dtype):
    """power [T, B]: per segment the good frames' band powers, summed in ``dtype``; bad_frames [T]."""
    t, b = fedges.shape[0] - 1, bedges.shape[0] - 1
    out, n_bad = np.zeros((t, b), dtype), np.zeros(t, np.int32)
    for k in range(t):
        rows = np.arange(fedges[k], fedges[k + 1])
        good = rows[~bad[rows]]
        n_bad[k] = rows.shape[0] - good.shape[0]
        for j in range(b):
            out[k, j] = p[good, bedges[j]:bedges[j + 1]].astype(dtype).sum(dtype=dtype)
    return out, n_bad


def tone(freq, amplitude, n, phase=0.0):
    return (amplitude * np.sin(2.0 * np.pi * freq * np.arange(n) / 16000.0 + phase)).astype(np.float32)


def accuracy_inputs():
    """name -> 16 frames' worth of 16 kHz samples: tones, noise and a quiet 1e-4 signal."""
    n = FRAME + 15 * HOP
    rng = np.random.default_rng(2024)
    noise = rng.standard_normal(n).astype(np.float32)
    return {
        "tone 1 kHz": tone(1000.0, 0.5, n),
        "tones off the bin centres": tone(233.0, 0.4, n) + tone(1877.7, 0.2, n, 1.0) + tone(6510.3, 0.1, n, 2.0),
        "noise": (0.1 * noise).astype(np.float32),
        "tone in noise": tone(440.0, 0.3, n) + (0.01 * noise).astype(np.float32),
        "quiet 1e-4": (1e-4 * noise).astype(np.float32) + tone(300.0, 1e-4, n),
    }
