"""One Sweep.update on resident logits beside the embedder pass that produces as many windows, beside the host restatement and
beside train.metrics_table: 1 048 576 windows x 13 columns, timed in turns in one process (median of 5 turns after 2 warm-up
turns, every turn's value kept).

    python tools/eval_bench.py [--windows 1048576] [--columns 13] [--reps 5] [--warmup 2]

Prints one JSON line.  `update_rows_ms` / `update_columns_ms`: one Sweep.update on [W][C] logits / on the same matrix column-major,
labels already on the device, by HIP events (it includes the read-back of label_of that bd_eval_accumulate checks).
`one_bin_ms`: the same on a matrix whose every row falls into one bin (every LDS add of a workgroup on one word).
`host_ms`: evaluate.sweep_host on the same logits by the host clock.  `metrics_table_ms`: train.metrics_table on each of the
columns in turn, by the host clock.  `embed_ms`: engine.launch(..., want_embeddings=True) over launch sets of 4096 windows that
add up to the same number of windows, by HIP events.  The logits are smoothed noise as tools/calls_bench.py draws it, so the bins
are as concentrated as a model's: `bins_used` says how many rows of the table a column has.  There is no expectation to meet,
only numbers to read."""
import argparse
import json
import os
import sys
import time

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


def clocked(fn):
    start = time.perf_counter()
    out = fn()
    return (time.perf_counter() - start) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1 << 20)
    ap.add_argument("--columns", type=int, default=13)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    os.environ.setdefault("BUZZDETECT_SYNTHETIC_WEIGHTS", "1")
    import torch
    from buzzdetect_amd import dataset as D, evaluate as E, train
    from buzzdetect_amd.engine import HipEngine, hop_samples, patch_step
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs a HIP device: a time taken anywhere else says nothing")
    w, c = args.windows, args.columns
    rng = np.random.default_rng(0)
    noise = rng.standard_normal((w + 4, c))
    logits = np.ascontiguousarray(sum(noise[i:i + w] for i in range(5)) / np.sqrt(5.0), np.float32)
    labels = (rng.random((w, c)) < 0.05).astype(np.uint8)
    label_of = np.arange(c, dtype=np.int32)
    flat = np.full((w, c), 0.5, np.float32)
    sets = -(-w // 4096)
    audio = torch.from_numpy((0.1 * rng.standard_normal(64 * 64 * D.WINDOW_SAMPLES)).astype(np.float32)).cuda()
    parts = list(audio.split(64 * D.WINDOW_SAMPLES))
    engine = HipEngine(modelname=None)
    try:
        hop, step = hop_samples(0.96), patch_step(0.96)
        rows = torch.from_numpy(logits).to(engine.device)
        columns = rows.t().contiguous().t()
        one_bin = torch.from_numpy(flat).to(engine.device)
        labels_dev = torch.from_numpy(labels).to(engine.device)
        sweeps = {name: E.Sweep(label_of, c, device=engine.device) for name in ("rows", "columns", "one_bin")}
        times = {name: [] for name in ("update_rows_ms", "update_columns_ms", "one_bin_ms", "host_ms", "metrics_table_ms", "embed_ms")}
        turns = args.warmup + args.reps
        for turn in range(turns):
            got = {"update_rows_ms": once(lambda: sweeps["rows"].update(rows, labels_dev)),
                   "update_columns_ms": once(lambda: sweeps["columns"].update(columns, labels_dev)),
                   "one_bin_ms": once(lambda: sweeps["one_bin"].update(one_bin, labels_dev)),
                   "embed_ms": once(lambda: [engine.launch(parts, hop, step, True, False) for _ in range(sets)])}
            got["host_ms"], host = clocked(lambda: E.sweep_host(logits, labels, label_of, c))
            got["metrics_table_ms"], tables = clocked(lambda: [train.metrics_table(logits[:, i], labels[:, i] == 1) for i in range(c)])
            if turn >= args.warmup:
                for name, value in got.items():
                    times[name].append(value)
        state = {name: s.counts() for name, s in sweeps.items()}
        equal = all(np.array_equal(state[name][0], np.uint32(turns) * host[0]) and np.array_equal(state[name][1], np.uint32(turns) * host[1])
                    for name in ("rows", "columns"))
        one = E.sweep_host(flat, labels, label_of, c)
        equal = equal and np.array_equal(state["one_bin"][0], np.uint32(turns) * one[0])
        curves = E.curves_of(host[0], host[1], label_of)
        same_text = all(curve.table() == "\n".join("0," + line[3:] if line.startswith("-0,") else line for line in text.split("\n"))
                        for curve, text in zip(curves, tables))
    finally:
        engine.close()
    out = {"windows": w, "columns": c, "slices": -(-w // E._lib.EVAL_SLICE), "bins_used": int(np.median([len(k.thresholds) for k in curves])),
           "device_equals_host": bool(equal), "table_equals_metrics_table": bool(same_text), "embed_windows": sets * 4096}
    for name, values in times.items():
        out[name] = round(float(np.median(values)), 4)
        out[name + "_all"] = [round(v, 4) for v in values]
    out["update_rows_over_embed"] = round(out["update_rows_ms"] / out["embed_ms"], 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
