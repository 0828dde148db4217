"""Fixtures and independent restatements for the PCA tests (tests/test_pca_host.py, tests/test_pca_gpu.py): rows that look like
YAMNet's with three planted directions, and the header's arithmetic (include/buzzdetect_pca.h) written again in NumPy, in
float32 for the exact comparisons and in float64 for the bounds.

The bound of every float comparison is the project's own: 8 x the deviation of the plain float32 statement of the same
quantity (a sequential sum, row after row) from float64 on the same data - never a figure taken from the code under test."""
import numpy as np

DIM = 1024
PLANTED_SD = (3.0, 2.0, 1.0)
BOUND = 8.0


def planted(w, seed=0, channels=DIM):
    """float32 [w, 1024]: a non-negative base row |N(0.5, 0.3)|, three planted orthonormal directions with standard deviations
    3, 2 and 1, and 0.1 N(0, 1) noise.  With ``channels`` < 1024 only that many leading channels are non-zero (the CPU tests'
    way to seconds).  Returns (rows, directions float64 [3, 1024])."""
    rng = np.random.default_rng(seed)
    base = np.abs(rng.normal(0.5, 0.3, channels))
    q, _ = np.linalg.qr(rng.standard_normal((channels, 3)))
    z = rng.standard_normal((w, 3)) * np.array(PLANTED_SD)
    x = base[None, :] + z @ q.T + 0.1 * rng.standard_normal((w, channels))
    rows = np.zeros((w, DIM), np.float32)
    rows[:, :channels] = x.astype(np.float32)
    directions = np.zeros((3, DIM))
    directions[:, :channels] = q.T
    return rows, directions


def present(e):
    """Which rows the device keeps: those whose squared norm is finite."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.isfinite((e.astype(np.float32) ** 2).sum(axis=1, dtype=np.float32)) & np.isfinite(e).all(axis=1)


def terms(e, shift=None, pick=None):
    """float32 [R, 1024]: t(r, c) of the header, absent rows as zeros."""
    rows = e if pick is None else e[pick]
    t = rows if shift is None else (rows - shift[None, :].astype(np.float32)).astype(np.float32)
    return np.where(present(rows)[:, None], t, np.float32(0.0)).astype(np.float32)


def sums_f32(e, shift=None, pick=None):
    """partial[s][c] of bd_pca_sums, sequentially in float32: float32 [ceil(R / 256), 1024]."""
    t = terms(e, shift, pick)
    out = np.zeros(((t.shape[0] + 255) // 256, DIM), np.float32)
    for s in range(out.shape[0]):
        acc = np.zeros(DIM, np.float32)
        for row in t[256 * s:256 * s + 256]:
            acc = acc + row
        out[s] = acc
    return out


def gram_f64(e, shift=None, pick=None):
    t = terms(e, shift, pick).astype(np.float64)
    return t.T @ t


def gram_f32_sequential(e, shift=None, pick=None, channels=DIM):
    """The float32 statement the bound is taken from: acc += outer(t_r, t_r), row after row, products and sums rounded
    separately; over the leading ``channels`` only ([channels, channels])."""
    t = terms(e, shift, pick)[:, :channels]
    acc = np.zeros((channels, channels), np.float32)
    for row in t:
        acc += np.multiply.outer(row, row)
    return acc


def project_f32(e, scores, mv, scale, mean):
    """y and resid of bd_pca_project from the stored scores, in float32 NumPy with the header's order of operations."""
    f = np.float32
    e, scores = e.astype(f), scores.astype(f)
    w, d = scores.shape
    with np.errstate(invalid="ignore", over="ignore"):
        x = (e - mean[None, :].astype(f)).astype(f)
        # lane l: x[l + 64 j]^2 by fused multiply-add, j ascending, from 0 - exact in float64, rounded once
        lanes = np.zeros((w, 64), f)
        for j in range(DIM // 64):
            v = x[:, 64 * j:64 * j + 64].astype(np.float64)
            lanes = (v * v + lanes.astype(np.float64)).astype(f)        # 24-bit squares are exact in float64; one rounding
        for m in (32, 16, 8, 4, 2, 1):
            lanes = (lanes + lanes[:, np.arange(64) ^ m]).astype(f)
        c2 = lanes[:, 0]
        u = (scores - mv[None, :].astype(f)).astype(f)
        y = (u * scale[None, :].astype(f)).astype(f)
        q = np.zeros(w, f)
        for j in range(d):
            q = (q + (u[:, j] * u[:, j]).astype(f)).astype(f)
        resid = np.fmax((c2 - q).astype(f), f(0.0))
        ok = np.isfinite(c2)
    nan = f(np.nan)
    return np.where(ok[:, None], y, nan).astype(f), np.where(ok, resid, nan).astype(f)


def project_f64(e, components, mean, scale):
    x = e.astype(np.float64) - mean.astype(np.float64)[None, :]
    u = x @ components.astype(np.float64).T
    return u * scale.astype(np.float64)[None, :], np.maximum((x * x).sum(axis=1) - (u * u).sum(axis=1), 0.0)


def pca_reference(e, d, dtype):
    """PCA of the rows by covariance and eigh in ``dtype``: (components [d, 1024] float64, eigenvalues [d] float64)."""
    x = e.astype(dtype)
    mean = x.sum(axis=0, dtype=dtype) / dtype(x.shape[0])
    x = (x - mean).astype(dtype)
    c = (x.T @ x / dtype(x.shape[0] - 1)).astype(dtype)
    values, vectors = np.linalg.eigh(c)
    top = np.argsort(values)[::-1][:d]
    return vectors[:, top].T.astype(np.float64), values[top].astype(np.float64)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
