"""One Searcher.update beside the embedder pass that feeds it: 4096 windows against Q = 64 queries with k = 100 (norms, scores
and selection: three launches), and the engine.launch(..., want_embeddings=True) of the same 4096 windows, timed in turns in one
process with HIP events (median of 5 turns after 2 warm-up turns).

    python tools/search_bench.py [--windows 4096] [--queries 64] [--k 100] [--reps 5] [--warmup 2]

Prints one JSON line: both medians, every repeat, and `update_over_embed`.  `update_ms` starts from an empty state every time
(the first pass of a search); `later_pass_update_ms` repeats the update on a state that already holds better hits, where the
selector skips most batches; `worst_case_update_ms` is the first-pass update on rows sorted so that every batch of the selector
holds a new best (no batch is skipped); `norms_and_scores_ms` and `selection_ms` are the two halves alone, `queued_update_ms` one
of 20 updates enqueued back to back.  The expectation to confirm or refute: the update is launch-latency sized -
2 x 4096 x 64 x 1024 = 0.5 GFLOP against the several hundred of the pass."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    os.environ.setdefault("BUZZDETECT_SYNTHETIC_WEIGHTS", "1")
    import torch
    from buzzdetect_amd import dataset as D, search
    from buzzdetect_amd.engine import HipEngine, hop_samples, patch_step
    if not torch.cuda.is_available():
        raise SystemExit("search_bench needs a HIP device: a time taken anywhere else says nothing")
    per_part = max(1, args.windows // 64)
    n_parts = args.windows // per_part
    rng = np.random.default_rng(0)
    audio = torch.from_numpy((0.1 * rng.standard_normal(n_parts * per_part * D.WINDOW_SAMPLES)).astype(np.float32)).cuda()
    parts = list(audio.split(per_part * D.WINDOW_SAMPLES))
    engine = HipEngine(modelname=None)
    try:
        hop, step = hop_samples(0.96), patch_step(0.96)
        emb, _, counts = engine.launch(parts, hop, step, True, False)
        windows = int(emb.shape[0])
        queries = emb[:: max(1, windows // args.queries)][: args.queries].cpu().numpy()
        turns = args.warmup + args.reps
        searcher = search.Searcher(queries, k=args.k, metric="cosine", device=engine.device)
        first = [search.Searcher(queries, k=args.k, metric="cosine", device=engine.device) for _ in range(turns)]
        update_ms, steady_ms, embed_ms = [], [], []
        for turn in range(turns):
            u = once(lambda: first[turn].update(emb))             # an empty state: the first pass of a search
            s = once(lambda: searcher.update(emb))                # a state that already holds better: most batches are skipped
            e = once(lambda: engine.launch(parts, hop, step, True, False))
            if turn >= args.warmup:
                update_ms.append(u)
                steady_ms.append(s)
                embed_ms.append(e)
        # the parts alone: norms + scores (row-major here), and the selection from an empty state on those scores
        ready = searcher.scores(emb)
        scores_ms = [once(lambda: searcher.scores(emb)) for _ in range(turns)][args.warmup:]
        pickers = [search.Searcher(None, k=args.k, device=engine.device, n_queries=int(queries.shape[0])) for _ in range(turns)]
        select_ms = [once(lambda s=s: s.update_scores(ready)) for s in pickers][args.warmup:]
        # back to back, nothing waited for in between: what one update adds to a queue that is never empty
        torch.cuda.synchronize()
        queued_ms = once(lambda: [searcher.update(emb) for _ in range(20)]) / 20.0
        # the selector's worst case: ascending scores for query 0, so no batch is skipped there
        order = searcher.scores(emb)[:, 0].argsort()
        rising = emb.index_select(0, order).contiguous()
        fresh = [search.Searcher(queries, k=args.k, metric="cosine", device=engine.device) for _ in range(turns)]
        worst_ms = [once(lambda s=s: s.update(rising)) for s in fresh][args.warmup:]        # (an empty state each: a second call skips)
    finally:
        engine.close()
    u, e = float(np.median(update_ms)), float(np.median(embed_ms))
    print(json.dumps({"windows": windows, "queries": int(queries.shape[0]), "k": args.k,
                      "update_ms": round(u, 4), "update_ms_all": [round(v, 4) for v in update_ms],
                      "embed_ms": round(e, 4), "embed_ms_all": [round(v, 4) for v in embed_ms],
                      "update_over_embed": round(u / e, 4),
                      "later_pass_update_ms": round(float(np.median(steady_ms)), 4),
                      "worst_case_update_ms": round(float(np.median(worst_ms)), 4),
                      "norms_and_scores_ms": round(float(np.median(scores_ms)), 4),
                      "selection_ms": round(float(np.median(select_ms)), 4), "queued_update_ms": round(queued_ms, 4),
                      "update_gflop": round(2.0 * windows * queries.shape[0] * 1024 / 1e9, 3)}))


if __name__ == "__main__":
    main()
