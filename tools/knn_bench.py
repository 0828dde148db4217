"""The k-nearest-neighbour lists of rows resident on the device (bd_knn_update, k = 16, cosine), beside the same lists made the
only way the library could before - bd_search_scores + bd_search_update in blocks of 1024 query rows - and beside torch.mm +
torch.topk in blocks; and one bd_propagate_step.  Timed in turns in one process with HIP events (median of 5 turns after a
warm-up turn, with the fastest and the slowest).

    python tools/knn_bench.py [--rows 65536 262144] [--k 16] [--reps 5] [--warmup 1] [--step-rows 262144] [--classes 13]

Prints one JSON line.  Per row count: `knn_ms` (the whole bd_knn_update, roots included) and `knn_tflops` (2 W W 1024 flop on
the exact-f32 matrix instruction: the walk bd_cluster_assign does, for which tools/cluster_bench.py reports its own figure),
`composed_ms` (the queries of every block packed and uploaded beforehand, outside the timing), `composed_over_knn`, `torch_ms`
(unit rows prepared outside the timing), `torch_over_knn`, and `share_of_ids_equal` (the share of list slots in which the
fused and the composed route name the same row: the composed route divides by the query's root beforehand, so near ties may
swap).  `step_ms`: one bd_propagate_step over the lists at `--step-rows` rows and `--classes` classes; `step_gbps` counts the
edges (8 bytes each), the gathered rows of F (4 C bytes an edge) and F_out, Y and alpha once."""
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


def turns(fn, warmup, reps):
    t = [once(fn) for _ in range(warmup + reps)][warmup:]
    return float(np.median(t)), float(min(t)), float(max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[65536, 262144])
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--step-rows", type=int, default=262144)
    ap.add_argument("--classes", type=int, default=13)
    args = ap.parse_args()
    import torch
    from buzzdetect_amd import _lib, propagate, search
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench needs a HIP device: a time taken anywhere else says nothing")
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device=dev).manual_seed(2025)
    k = args.k
    out = {"k": k, "reps": args.reps, "warmup": args.warmup, "cases": []}
    for w in args.rows:
        centres = 2.0 * torch.randn((64, 1024), generator=gen, device=dev).abs()
        e = torch.empty((w, 1024), dtype=torch.float32, device=dev)
        for at in range(0, w, 65536):                                    # (in slabs: the noise is a temporary of the slab's size)
            n = min(65536, w - at)
            e[at:at + n] = centres[torch.randint(0, 64, (n,), generator=gen, device=dev)] + 0.5 * torch.randn((n, 1024), generator=gen, device=dev)
        nb = propagate.Neighbours(k, exclude_self=False, device=dev)
        nb._open(e)
        n2 = nb._norms(e)
        keys = torch.zeros((w, k), dtype=torch.int64, device=dev)
        ws_bytes = _lib.check(lib.bd_knn_workspace_bytes(w, w))
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)

        def fused():
            keys.zero_()
            _lib.check(lib.bd_knn_update(e.data_ptr(), w, n2.data_ptr(), 0, e.data_ptr(), w, n2.data_ptr(), 0, _lib.KNN_METRICS["cosine"],
                                         0, keys.data_ptr(), k, ws.data_ptr(), ws_bytes, stream))

        # the composed route: the search divides a score by the row's root only, so a block's queries are its rows brought to
        # unit length beforehand; the lists agree with the fused ones up to that rounding, the work is the same
        blocks = [(a, min(a + 1024, w)) for a in range(0, w, 1024)]
        unit = e / n2.sqrt().clamp_min(1e-15)[:, None]
        packed = [torch.from_numpy(search.pack_queries(unit[a:b].cpu().numpy())).to(dev) for a, b in blocks]
        scores = torch.empty((1024, w), dtype=torch.float32, device=dev)             # query-major, as search.py keeps a pass
        keys2 = torch.zeros((w, k), dtype=torch.int64, device=dev)

        def composed():
            keys2.zero_()
            for (a, b), p in zip(blocks, packed):
                for at in range(0, w, _lib.SEARCH_MAX_WINDOWS):
                    n = min(_lib.SEARCH_MAX_WINDOWS, w - at)
                    _lib.check(lib.bd_search_scores(e[at:at + n].data_ptr(), n, p.data_ptr(), b - a, _lib.SEARCH_METRICS["cosine"],
                                                    n2[at:at + n].data_ptr(), scores[:, at:].data_ptr(), 1, w, stream))
                    _lib.check(lib.bd_search_update(scores[:, at:].data_ptr(), n, b - a, 1, w, at, keys2[a:b].data_ptr(), k, stream))

        def torch_route():
            for a, b in blocks:
                torch.topk(unit[a:b] @ unit.T, k, dim=1)

        f_ms = turns(fused, args.warmup, args.reps)
        c_ms = turns(composed, args.warmup, args.reps)
        t_ms = turns(torch_route, args.warmup, args.reps)
        ids_f = propagate.decode_keys(keys.cpu().numpy().view(np.uint64))[0]
        ids_c = propagate.decode_keys(keys2.cpu().numpy().view(np.uint64))[0]
        out["cases"].append({"rows": w, "knn_ms": round(f_ms[0], 3), "knn_ms_min_max": [round(f_ms[1], 3), round(f_ms[2], 3)],
                             "knn_tflops": round(2.0 * w * w * 1024 / f_ms[0] / 1e9, 2),
                             "composed_ms": round(c_ms[0], 3), "composed_ms_min_max": [round(c_ms[1], 3), round(c_ms[2], 3)],
                             "composed_over_knn": round(c_ms[0] / f_ms[0], 3),
                             "torch_ms": round(t_ms[0], 3), "torch_ms_min_max": [round(t_ms[1], 3), round(t_ms[2], 3)],
                             "torch_over_knn": round(t_ms[0] / f_ms[0], 3),
                             "share_of_ids_equal": round(float((ids_f == ids_c).mean()), 6)})
        if w == args.step_rows or w == args.rows[-1] and "step_ms" not in out:
            c = args.classes
            ids, sims = propagate.decode_keys(keys.cpu().numpy().view(np.uint64))
            p = propagate.Propagator(device=dev)
            p._open(e)
            row_start, nbr, wt = p._graph((ids, sims))
            y = torch.zeros((w, c), dtype=torch.float32, device=dev)
            y[torch.arange(0, w, 8, device=dev), torch.arange(0, w, 8, device=dev) % c] = 1.0
            alpha = torch.ones((w,), dtype=torch.float32, device=dev)
            alpha[::8] = 0.0
            f_in, f_out = y.clone(), torch.empty_like(y)
            delta = torch.empty(((w + 255) // 256,), dtype=torch.float32, device=dev)

            def step():
                _lib.check(lib.bd_propagate_step(row_start.data_ptr(), nbr.data_ptr(), wt.data_ptr(), w, int(nbr.numel()),
                                                 f_in.data_ptr(), y.data_ptr(), alpha.data_ptr(), c, f_out.data_ptr(), delta.data_ptr(),
                                                 stream))

            s_ms = turns(step, args.warmup, args.reps)
            moved = w * k * (8.0 + 4.0 * c) + w * (8.0 * c + 12.0)
            out.update({"step_rows": w, "classes": c, "step_ms": round(s_ms[0], 4), "step_ms_min_max": [round(s_ms[1], 4), round(s_ms[2], 4)],
                        "step_gbps": round(moved / s_ms[0] / 1e6, 1)})
        del e, unit, packed, scores, keys, keys2, ws
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
