"""The three costs of "what to annotate next" (buzzdetect_amd/suggest.py), each the median of 5 after a warm-up, timed with HIP
events in one process as tools/search_bench.py does it:

    acquire   bd_suggest_acquire on 1 048 576 windows of M = 5 members x C = 13 classes, beside the time HBM needs for the bytes
              it reads and writes (8 TB/s)
    pick      bd_search_norms + bd_search_scores + bd_suggest_pick at n = 1024 candidates, k = 256 (and the pick alone)
    update    one Suggester.update of 4096 rows (three members of 13 classes, pool 800; the 8 KB read-back included) beside the
              embedder pass of 4096 windows and beside what top_windows does with the same rows: the heads and a selection-only
              Searcher.update_scores

    python tools/suggest_bench.py [--reps 5] [--warmup 2]

Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8.0e12


def once(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_of(fn, warmup, reps):
    times = [once(fn) for _ in range(warmup + reps)][warmup:]
    return round(float(np.median(times)), 4), [round(t, 4) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--acquire-windows", type=int, default=1 << 20)
    args = ap.parse_args()
    os.environ.setdefault("BUZZDETECT_SYNTHETIC_WEIGHTS", "1")
    import torch
    from buzzdetect_amd import dataset as D, search, suggest, train, weights
    from buzzdetect_amd.engine import HipEngine, hop_samples, patch_step
    if not torch.cuda.is_available():
        raise SystemExit("suggest_bench needs a HIP device: a time taken anywhere else says nothing")
    out = {}
    rng = np.random.default_rng(0)
    gen = torch.Generator(device="cuda").manual_seed(0)

    # 1. the acquisition alone
    w, m, c = args.acquire_windows, 5, 13
    wide = torch.randn((w, m * c), generator=gen, device="cuda") * 3.0
    scores = torch.empty((3, w), dtype=torch.float32, device="cuda")
    first = [i * c for i in range(m)]
    ms, every = median_of(lambda: suggest.acquire_device(wide, first, c, "softmax", None, out=scores), args.warmup, args.reps)
    moved = w * (m * c + 3) * 4
    out.update(acquire_windows=w, acquire_members=m, acquire_classes=c, acquire_ms=ms, acquire_ms_all=every,
               acquire_bytes=moved, acquire_hbm_ms=round(moved / HBM_BYTES_PER_S * 1e3, 4),
               acquire_gbytes_per_s=round(moved / (ms * 1e-3) / 1e9, 1))
    tms, _ = median_of(lambda: suggest.acquire_device(wide, first, c, "softmax", 4, out=scores), args.warmup, args.reps)
    out.update(acquire_target_ms=tms)
    del wide, scores

    # 2. similarities and the pick
    n, k = 1024, 256
    rows = torch.randn((n, 1024), generator=gen, device="cuda").abs().contiguous()
    among = search.Searcher(rows.cpu().numpy(), k=1, metric="cosine")
    sim = torch.empty((n, n), dtype=torch.float32, device="cuda")
    gain = torch.rand((n,), generator=gen, device="cuda")

    def scores_and_pick():
        among._score(rows, sim, 1, n)
        suggest.pick_device(sim, gain, None, k)

    ms, every = median_of(scores_and_pick, args.warmup, args.reps)
    pick_ms, _ = median_of(lambda: suggest.pick_device(sim, gain, None, k), args.warmup, args.reps)
    out.update(pick_candidates=n, pick_k=k, scores_and_pick_ms=ms, scores_and_pick_ms_all=every, pick_alone_ms=pick_ms,
               pick_us_per_step=round(pick_ms * 1e3 / k, 3))

    # 3. one update of a Suggester beside the embedder pass and beside top_windows' heads + selection
    windows = 4096
    classes = [f"c{i}" for i in range(13)]
    heads = {f"m{i}": weights.HeadWeights(train.glorot_layers(np.random.default_rng(i), [13], ["linear"]), list(classes)) for i in range(3)}
    per_part = windows // 64
    audio = torch.from_numpy((0.1 * rng.standard_normal(windows * D.WINDOW_SAMPLES)).astype(np.float32)).cuda()
    parts = list(audio.split(per_part * D.WINDOW_SAMPLES))
    engine = HipEngine(modelname=None, heads=heads)
    try:
        hop, step = hop_samples(0.96), patch_step(0.96)
        emb, _, _ = engine.launch(parts, hop, step, True, False)
        emb = emb.contiguous()
        turns = args.warmup + args.reps
        fresh = [suggest.Suggester(engine, strategy="bald", pool=800) for _ in range(turns)]
        later = suggest.Suggester(engine, strategy="bald", pool=800)
        later.update(emb)
        column = torch.tensor([4], dtype=torch.int64, device="cuda")
        pickers = [search.Searcher(None, k=100, device=engine.device, n_queries=1) for _ in range(turns)]
        first_ms, later_ms, embed_ms, top_ms, acquire_ms = [], [], [], [], []
        for turn in range(turns):
            f = once(lambda: fresh[turn].update(emb))              # an empty pool: every key and 800 rows enter
            s = once(lambda: later.update(emb))                    # a pool that holds these rows' scores already: nothing enters
            e = once(lambda: engine.launch(parts, hop, step, True, False))
            t = once(lambda: pickers[turn].update_scores(engine.score_rows(emb).index_select(1, column)))
            a = once(lambda: later.acquire(emb))
            if turn >= args.warmup:
                first_ms.append(f)
                later_ms.append(s)
                embed_ms.append(e)
                top_ms.append(t)
                acquire_ms.append(a)
    finally:
        engine.close()
    med = lambda v: round(float(np.median(v)), 4)
    out.update(update_windows=int(emb.shape[0]), update_pool=800, update_ms=med(first_ms), update_ms_all=[round(v, 4) for v in first_ms],
               later_pass_update_ms=med(later_ms), embed_ms=med(embed_ms), top_windows_update_ms=med(top_ms),
               heads_and_acquire_ms=med(acquire_ms), update_over_embed=round(med(first_ms) / med(embed_ms), 4))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
