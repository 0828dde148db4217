"""One Lloyd iteration of cluster.KMeans (assign, statistics, order, centroids) on rows resident on the device, beside the same
iteration written in torch on the same device and beside the embedder pass that produces that many rows; K = 64 and K = 256, both
metrics, timed in turns in one process with HIP events (median of 5 turns after 2 warm-up turns).

    python tools/cluster_bench.py [--rows 262144] [--clusters 64 256] [--reps 5] [--warmup 2] [--embed-windows 4096]

Prints one JSON line.  Per (K, metric): `iteration_ms` (the four steps enqueued back to back), `assign_ms`, `stats_ms`,
`order_ms`, `centroids_ms` (each alone), `torch_ms` (E @ C.T, argmin, the distances' sum, index_add_ and the division; for a
cosine over rows brought to unit length once, outside the timing), `torch_over_ours`, and `max_centroid_difference_to_torch`
(both moved the same centroids from the same start; rows near a tie may go either way, so it says only that both did the work).  `embed_ms` is engine.launch of
`--embed-windows` windows repeated until `--rows` windows are embedded, and `embed_over_iteration` its ratio to each iteration.
To compare with: assign is 2 W K 1024 flop on the exact-f32 matrix instruction (`assign_tflops`), and the sum pass reads E once
(`centroids_gbps` counts those 4 KB per row alone)."""
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
    return float(np.median([once(fn) for _ in range(warmup + reps)][warmup:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--clusters", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--embed-windows", type=int, default=4096)
    args = ap.parse_args()
    os.environ.setdefault("BUZZDETECT_SYNTHETIC_WEIGHTS", "1")
    import torch
    from buzzdetect_amd import _lib, cluster, dataset as D
    from buzzdetect_amd.engine import HipEngine, hop_samples, patch_step
    if not torch.cuda.is_available():
        raise SystemExit("cluster_bench needs a HIP device: a time taken anywhere else says nothing")
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream().cuda_stream
    w = args.rows
    gen = torch.Generator(device=dev).manual_seed(2025)
    out = {"rows": w, "reps": args.reps, "warmup": args.warmup, "cases": []}
    for k in args.clusters:
        centres = 2.0 * torch.randn((k, 1024), generator=gen, device=dev).abs()
        truth = torch.randint(0, k, (w,), generator=gen, device=dev)
        e = torch.empty((w, 1024), dtype=torch.float32, device=dev)
        for at in range(0, w, 65536):                                    # (in slabs: the noise is a temporary of the slab's size)
            n = min(65536, w - at)
            e[at:at + n] = centres[truth[at:at + n]] + 0.5 * torch.randn((n, 1024), generator=gen, device=dev)
        del centres, truth
        for metric in ("euclidean", "cosine"):
            km = cluster.KMeans(k, metric=metric, device=dev)
            km._open(e)
            n2 = km._norms(e)
            first = cluster.normalise_centroids(e[:k].cpu().numpy(), metric)
            sets = [cluster._Centres(km, k).upload(first), cluster._Centres(km, k)]
            slices = (w + 255) // 256
            labels, prev = torch.empty((w,), dtype=torch.int32, device=dev), torch.full((w,), -1, dtype=torch.int32, device=dev)
            dist = torch.empty((w,), dtype=torch.float32, device=dev)
            stats = torch.empty((2, slices), dtype=torch.int32, device=dev)
            order, offsets = torch.empty((w,), dtype=torch.int32, device=dev), torch.empty((k + 1,), dtype=torch.int32, device=dev)
            ws_bytes = _lib.check(lib.bd_cluster_workspace_bytes(w, k))
            ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
            mid = _lib.CLUSTER_METRICS[metric]

            def assign():
                km._assign(e, n2, sets[0], k, labels, dist)

            def statistics():
                _lib.check(lib.bd_cluster_stats(dist.data_ptr(), labels.data_ptr(), prev.data_ptr(), w, stats[0].data_ptr(),
                                                stats[1].data_ptr(), stream))

            def ordering():
                _lib.check(lib.bd_cluster_order(labels.data_ptr(), w, k, order.data_ptr(), offsets.data_ptr(), ws.data_ptr(),
                                                ws_bytes, stream))

            def centroids():
                _lib.check(lib.bd_cluster_centroids(e.data_ptr(), w, n2.data_ptr(), order.data_ptr(), offsets.data_ptr(), k, mid,
                                                    sets[0].rows.data_ptr(), sets[1].rows.data_ptr(), sets[1].packed.data_ptr(),
                                                    sets[1].c2.data_ptr(), ws.data_ptr(), ws_bytes, stream))

            def iteration():
                assign()
                statistics()
                ordering()
                centroids()

            # the same iteration in torch: for a cosine over unit rows prepared once
            rows = e if metric == "euclidean" else e / n2.sqrt().clamp_min(1e-15)[:, None]
            c = sets[0].rows.clone()
            c2 = (c * c).sum(dim=1)
            r2 = (rows * rows).sum(dim=1)

            def torch_iteration():
                s = rows @ c.T
                t = c2[None, :] - 2.0 * s if metric == "euclidean" else -s
                best, lab = t.min(dim=1)
                d = (r2 + best).clamp_min(0.0) if metric == "euclidean" else 1.0 + best
                inertia = d.sum(dtype=torch.float64)
                total = torch.zeros_like(c).index_add_(0, lab, rows)
                counts = torch.bincount(lab, minlength=k).clamp_min(1).to(torch.float32)
                new = total / counts[:, None] if metric == "euclidean" else total / total.norm(dim=1, keepdim=True).clamp_min(1e-15)
                return new, inertia

            ours = median_of(iteration, args.warmup, args.reps)
            parts = {name: median_of(fn, args.warmup, args.reps) for name, fn in
                     (("assign_ms", assign), ("stats_ms", statistics), ("order_ms", ordering), ("centroids_ms", centroids))}
            theirs = median_of(torch_iteration, args.warmup, args.reps)
            new, _ = torch_iteration()
            agree = float((new - sets[1].rows).abs().max())               # both moved the same centroids from the same start
            case = {"clusters": k, "metric": metric, "iteration_ms": round(ours, 4), "torch_ms": round(theirs, 4),
                    "torch_over_ours": round(theirs / ours, 3), "max_centroid_difference_to_torch": agree,
                    "assign_tflops": round(2.0 * w * k * 1024 / parts["assign_ms"] / 1e9, 2),
                    "centroids_gbps": round(w * 4096.0 / parts["centroids_ms"] / 1e6, 1)}
            case.update({name: round(v, 4) for name, v in parts.items()})
            out["cases"].append(case)
            del rows, ws, sets
        del e
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
        embed_ms = median_of(lambda: [engine.launch(pieces, hop, step, True, False) for _ in range(launches)], args.warmup, args.reps)
    finally:
        engine.close()
    out.update({"embed_windows": launches * per_launch, "embed_launches": launches, "embed_ms": round(embed_ms, 3)})
    for case in out["cases"]:
        case["embed_over_iteration"] = round(embed_ms / case["iteration_ms"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
