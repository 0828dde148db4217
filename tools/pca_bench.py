"""The PCA's three kernels (bd_pca_gram, bd_pca_sums, bd_pca_project) on rows resident on the device, beside the same products in
torch float32 on the same device and beside the embedder pass that produces that many rows; timed in turns in one process with
HIP events (median of 5 turns after 2 warm-up turns, each with its spread: the largest minus the smallest turn).

    python tools/pca_bench.py [--rows 262144] [--project-rows 65536] [--reps 5] [--warmup 2] [--embed-windows 4096]

Prints one JSON line.  `gram_ms` is bd_pca_gram with a shift over `--rows` rows (the finishing pass included), `gram_tflops`
counts 2 R 1024^2 flop for it - the full product, of which the kernel computes the 528 of 1024 tiles -, `torch_gram_ms` is
(X - m).T @ (X - m) with the centred copy made inside the timing (`torch_gram_matmul_ms`: the product alone, from a centred
copy made before), `torch_gram_over_ours` their ratio.  `sums_ms` and `sums_gbps` (4 KB a row read once), `torch_sums_ms`.
`project` per d: `ms`, `tflops` of 2 W 32 ceil(d / 32) 1024 flop, `torch_ms` of (X - m) @ V.T plus the residual's two row
sums.  `embed_ms` is engine.launch of `--embed-windows` windows repeated until `--rows` windows are embedded.  The yardstick is
torch's product, never the code under test."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def once(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_of(fn, warmup, reps):
    """(median, spread) in ms of `reps` turns after `warmup`."""
    turns = [once(fn) for _ in range(warmup + reps)][warmup:]
    return float(np.median(turns)), float(max(turns) - min(turns))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--project-rows", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--embed-windows", type=int, default=4096)
    args = ap.parse_args()
    os.environ.setdefault("BUZZDETECT_SYNTHETIC_WEIGHTS", "1")
    import torch
    from buzzdetect_amd import _lib, dataset as D, search
    from buzzdetect_amd.engine import HipEngine, hop_samples, patch_step
    if not torch.cuda.is_available():
        raise SystemExit("pca_bench needs a HIP device: a time taken anywhere else says nothing")
    if not 1 <= args.rows <= _lib.PCA_MAX_ROWS:
        raise SystemExit(f"--rows must be in 1..{_lib.PCA_MAX_ROWS}: one call of bd_pca_gram is timed")
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream().cuda_stream
    w = args.rows
    gen = torch.Generator(device=dev).manual_seed(2025)
    base = torch.randn((1024,), generator=gen, device=dev).abs()
    e = torch.empty((w, 1024), dtype=torch.float32, device=dev)
    for at in range(0, w, 65536):                                        # (in slabs: the noise is a temporary of the slab's size)
        n = min(65536, w - at)
        e[at:at + n] = base + 0.5 * torch.randn((n, 1024), generator=gen, device=dev)
    n2 = torch.empty((w,), dtype=torch.float32, device=dev)
    _lib.check(lib.bd_search_norms(e.data_ptr(), w, n2.data_ptr(), stream))
    mean = e.mean(dim=0).contiguous()
    gram = torch.empty((1024, 1024), dtype=torch.float32, device=dev)
    partial = torch.empty(((w + 255) // 256, 1024), dtype=torch.float32, device=dev)
    ws_bytes = _lib.check(lib.bd_pca_workspace_bytes(w))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)

    def ours_gram():
        _lib.check(lib.bd_pca_gram(e.data_ptr(), w, None, w, n2.data_ptr(), mean.data_ptr(), 0, gram.data_ptr(), ws.data_ptr(),
                                   ws_bytes, stream))

    def ours_sums():
        _lib.check(lib.bd_pca_sums(e.data_ptr(), w, None, w, n2.data_ptr(), mean.data_ptr(), partial.data_ptr(), stream))

    def torch_gram():
        x = e - mean
        return x.T @ x

    out = {"rows": w, "reps": args.reps, "warmup": args.warmup}
    ms, spread = median_of(ours_gram, args.warmup, args.reps)
    out.update({"gram_ms": round(ms, 3), "gram_spread_ms": round(spread, 3), "gram_tflops": round(2.0 * w * 1024 * 1024 / ms / 1e9, 2)})
    theirs, spread = median_of(torch_gram, args.warmup, args.reps)
    out.update({"torch_gram_ms": round(theirs, 3), "torch_gram_spread_ms": round(spread, 3), "torch_gram_over_ours": round(theirs / ms, 3)})
    out["max_gram_difference_to_torch"] = float((torch_gram() - gram).abs().max())      # both did the work
    del ws
    torch.cuda.empty_cache()
    x = e - mean
    alone, spread = median_of(lambda: x.T @ x, args.warmup, args.reps)
    out.update({"torch_gram_matmul_ms": round(alone, 3), "torch_gram_matmul_spread_ms": round(spread, 3),
                "torch_gram_matmul_tflops": round(2.0 * w * 1024 * 1024 / alone / 1e9, 2)})
    del x
    ms, spread = median_of(ours_sums, args.warmup, args.reps)
    theirs, tspread = median_of(lambda: (e - mean).sum(dim=0), args.warmup, args.reps)
    out.update({"sums_ms": round(ms, 4), "sums_spread_ms": round(spread, 4), "sums_gbps": round(w * 4096.0 / ms / 1e6, 1),
                "torch_sums_ms": round(theirs, 4), "torch_sums_spread_ms": round(tspread, 4)})

    wp = min(args.project_rows, w, _lib.SEARCH_MAX_WINDOWS)
    ep = e[:wp]
    out["project_rows"] = wp
    out["project"] = []
    for d in (2, 64):
        q, _ = np.linalg.qr(np.random.default_rng(d).standard_normal((1024, d)))
        comps = np.ascontiguousarray(q.T, np.float32)
        v = torch.from_numpy(comps).to(dev)
        packed = torch.from_numpy(search.pack_queries(comps)).to(dev)
        mv = (v.double() @ mean.double()).float().contiguous()
        scale = torch.ones((d,), dtype=torch.float32, device=dev)
        y = torch.empty((wp, d), dtype=torch.float32, device=dev)
        resid = torch.empty((wp,), dtype=torch.float32, device=dev)

        def ours_project():
            _lib.check(lib.bd_pca_project(ep.data_ptr(), wp, packed.data_ptr(), d, mv.data_ptr(), scale.data_ptr(), mean.data_ptr(),
                                          y.data_ptr(), resid.data_ptr(), stream))

        def torch_project():
            x = ep - mean
            u = x @ v.T
            return u, ((x * x).sum(dim=1) - (u * u).sum(dim=1)).clamp_min(0.0)

        ms, spread = median_of(ours_project, args.warmup, args.reps)
        theirs, tspread = median_of(torch_project, args.warmup, args.reps)
        u, r = torch_project()
        out["project"].append({"d": d, "ms": round(ms, 4), "spread_ms": round(spread, 4),
                               "tflops": round(2.0 * wp * 32 * ((d + 31) // 32) * 1024 / ms / 1e9, 2),
                               "gbps": round(wp * 4096.0 / ms / 1e6, 1), "torch_ms": round(theirs, 4),
                               "torch_spread_ms": round(tspread, 4), "torch_over_ours": round(theirs / ms, 3),
                               "max_difference_to_torch": float(max((u - y).abs().max(), (r - resid).abs().max()))})
    del e, ep
    torch.cuda.empty_cache()
    # the embedder pass that makes as many rows
    per_part = max(1, args.embed_windows // 64)
    n_parts = args.embed_windows // per_part
    rng = np.random.default_rng(0)
    audio = torch.from_numpy((0.1 * rng.standard_normal(n_parts * per_part * D.WINDOW_SAMPLES)).astype(np.float32)).cuda()
    pieces = list(audio.split(per_part * D.WINDOW_SAMPLES))
    engine = HipEngine(modelname=None)
    try:
        hop, step = hop_samples(0.96), patch_step(0.96)
        emb, _, _ = engine.launch(pieces, hop, step, True, False)
        per_launch = int(emb.shape[0])
        launches = (w + per_launch - 1) // per_launch
        embed_ms, spread = median_of(lambda: [engine.launch(pieces, hop, step, True, False) for _ in range(launches)], args.warmup,
                                     args.reps)
    finally:
        engine.close()
    out.update({"embed_windows": launches * per_launch, "embed_launches": launches, "embed_ms": round(embed_ms, 3),
                "embed_spread_ms": round(spread, 3), "embed_over_gram": round(embed_ms / out["gram_ms"], 2)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
