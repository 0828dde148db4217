#!/usr/bin/env python3
"""Time one layout iteration of the neighbour-preserving map (attract + repulse + update, include/buzzdetect_tsne.h) on the
device at N = 16 384, 65 536 and 262 144 windows with E = 48 N edges: medians of 5 samples with their spread, every sample a
batch of iterations long enough to time.  Beside them: the repulsion alone and its pair rate against the issue-rate estimate
(about 20 vector instructions a pair on 16 384 lanes at 2.4 GHz), a torch float32 statement of the same iteration in row
blocks, and bd_knn_update (k = 48, cosine) on as many 1024-dimensional rows.  One JSON line per size.

    python tools/tsne_bench.py [--sizes 16384,65536,262144] [--samples 5] [--no-torch] [--no-knn]

There is no CPU path: without a HIP device this fails."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from buzzdetect_amd import _lib, propagate  # noqa: E402

EDGES_PER_ROW = 48
ESTIMATE_PAIRS_PER_S = 16384 * 2.4e9 / 20          # the estimate the pair rate goes against; not a measurement
TARGET_S = 0.25                                    # a sample is at least about this long


def timed(torch, fn, repeats):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(repeats):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e-3 / repeats


def samples(torch, fn, n_samples):
    """Seconds per call: warm up, size the batch from one call, then n_samples batches."""
    fn()
    once = timed(torch, fn, 1)
    repeats = max(1, int(np.ceil(TARGET_S / max(once, 1e-6))))
    got = sorted(timed(torch, fn, repeats) for _ in range(n_samples))
    return {"median_s": float(np.median(got)), "min_s": got[0], "max_s": got[-1], "batch": repeats}


def torch_iteration(torch, y, v, gain, src, nbr, big, rate, block):
    """The same iteration as plain torch float32 in blocks of `block` rows (its own summation order)."""
    n = y.shape[0]
    rep, z = torch.empty_like(y), torch.empty(n, device=y.device)
    for a in range(0, n, block):
        diff = y[a:a + block, None, :] - y[None, :, :]
        q = 1.0 / (1.0 + (diff * diff).sum(dim=2))
        rows = torch.arange(a, min(a + block, n), device=y.device)
        q[rows - a, rows] = 0.0
        z[a:a + block] = q.sum(dim=1)
        rep[a:a + block] = ((q * q)[:, :, None] * diff).sum(dim=1)
    d = y[src] - y[nbr]
    w = big / (1.0 + (d * d).sum(dim=1))
    attr = torch.zeros_like(y).index_add_(0, src, w[:, None] * d)
    g = 4.0 * (12.0 * attr - rep / z.sum())
    gain = torch.where((g > 0) != (v > 0), gain + 0.2, gain * 0.8).clamp_(min=0.01)
    v = 0.5 * v - rate * gain * g
    y = y + v
    return y - y.mean(dim=0), v, gain


def run(torch, n, n_samples, with_torch, with_knn):
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(n)
    edges = EDGES_PER_ROW * n
    y0 = torch.from_numpy((6.0 * rng.normal(size=(n, 2))).astype(np.float32)).to(dev)
    row_start = torch.arange(n + 1, dtype=torch.int64, device=dev) * EDGES_PER_ROW
    nbr = torch.from_numpy(rng.integers(0, n, size=edges).astype(np.int32)).to(dev)
    big = torch.from_numpy((rng.random(edges) / edges).astype(np.float32)).to(dev)
    y, v, gain = y0.clone(), torch.zeros_like(y0), torch.ones_like(y0)
    attr, rep, z = torch.empty_like(y0), torch.empty_like(y0), torch.empty(n, device=dev)
    nbytes = _lib.check(lib.bd_tsne_workspace_bytes(n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rate = 1e-3                                     # the positions barely move: every sample times the same map

    def repulse():
        _lib.check(lib.bd_tsne_repulse(y.data_ptr(), n, rep.data_ptr(), z.data_ptr(), ws.data_ptr(), nbytes, stream))

    def iteration():
        _lib.check(lib.bd_tsne_attract(row_start.data_ptr(), nbr.data_ptr(), big.data_ptr(), n, edges, y.data_ptr(), attr.data_ptr(),
                                       stream))
        repulse()
        _lib.check(lib.bd_tsne_update(y.data_ptr(), v.data_ptr(), gain.data_ptr(), attr.data_ptr(), rep.data_ptr(), z.data_ptr(), n,
                                      12.0, 0.5, rate, 0.01, None, ws.data_ptr(), nbytes, stream))

    out = {"rows": n, "edges": edges, "workspace_bytes": nbytes, "iteration": samples(torch, iteration, n_samples),
           "repulse": samples(torch, repulse, n_samples)}
    pairs = float(n) * float(n - 1)
    out["repulse"]["pairs_per_s"] = pairs / out["repulse"]["median_s"]
    out["repulse"]["of_estimate"] = out["repulse"]["pairs_per_s"] / ESTIMATE_PAIRS_PER_S
    assert torch.isfinite(y).all()
    if with_torch:
        src = torch.arange(n, device=dev).repeat_interleave(EDGES_PER_ROW)
        state = [y0.clone(), torch.zeros_like(y0), torch.ones_like(y0)]
        block = max(1, (1 << 26) // n)

        def plain():
            state[:] = torch_iteration(torch, *state, src, nbr.long(), big, rate, block)

        out["torch_float32"] = samples(torch, plain, n_samples if n <= 65536 else 1)
        out["torch_float32"]["block_rows"] = block
        out["torch_float32"]["over_device"] = out["torch_float32"]["median_s"] / out["iteration"]["median_s"]
        del src, state
    if with_knn:
        rows = torch.from_numpy(rng.normal(size=(min(n, 1 << 14), 1024)).astype(np.float32)).to(dev)
        rows = rows.repeat((n + rows.shape[0] - 1) // rows.shape[0], 1)[:n].contiguous()
        rows += 0.01 * torch.randn(rows.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(n))

        def lists():
            propagate.Neighbours(EDGES_PER_ROW, "cosine", device=dev).update(rows)

        out["knn_update"] = samples(torch, lists, n_samples if n <= 65536 else 1)
        out["knn_update"]["over_iteration"] = out["knn_update"]["median_s"] / out["iteration"]["median_s"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="16384,65536,262144")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-knn", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tsne_bench: no HIP device visible to PyTorch; there is no CPU path")
    print(json.dumps({"device": torch.cuda.get_device_name(), "estimate_pairs_per_s": ESTIMATE_PAIRS_PER_S,
                      "estimate_is": "issue-rate arithmetic, not a measurement"}), flush=True)
    for n in (int(s) for s in args.sizes.split(",")):
        print(json.dumps(run(torch, n, args.samples, not args.no_torch, not args.no_knn)), flush=True)


if __name__ == "__main__":
    main()
