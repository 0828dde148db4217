"""One Caller.call on resident logits beside the embedder pass that produces as many windows and beside the host restatement:
90 000 windows (a recording-day at hop 0.96 s) x 13 columns, bins of 60 s, timed in turns in one process (median of 5 turns after
2 warm-up turns).

    python tools/calls_bench.py [--windows 90000] [--columns 13] [--bin-s 60] [--reps 5] [--warmup 2]

Prints one JSON line.  `call_ms`: a whole Caller.call by the host clock - the upload of ticks and bin offsets, the scan, the
finishing pass, the bins pass and the read-back of marks, events and bins (it ends in device-to-host copies, which wait for the
stream).  `launches_ms`: bd_calls_events + bd_calls_bins alone on buffers that are already there, by HIP events (it includes the
read-back of the rules bd_calls_events checks).  `embed_ms`: engine.launch(..., want_embeddings=True) over launch sets of 4096
windows that add up to the same number of windows, by HIP events.  `host_ms`: calls.events_host + calls.bins_host on the same
logits by the host clock.  The logits are smoothed noise (an event lasts a few windows), high and low the 70th and 40th percentile
of a column, events bridged over 2 s and kept from 1.5 s: `events` says how many that gives.  The scan is latency-bound by design
(one workgroup per column, ceil(windows / 1024) tiles one after the other): there is no expectation to meet, only numbers to read."""
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
    import torch
    torch.cuda.synchronize()
    start = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - start) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=90000)
    ap.add_argument("--columns", type=int, default=13)
    ap.add_argument("--bin-s", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    os.environ.setdefault("BUZZDETECT_SYNTHETIC_WEIGHTS", "1")
    import torch
    from buzzdetect_amd import _lib, calls, dataset as D
    from buzzdetect_amd.engine import HipEngine, hop_samples, patch_step
    if not torch.cuda.is_available():
        raise SystemExit("calls_bench needs a HIP device: a time taken anywhere else says nothing")
    w, c = args.windows, args.columns
    rng = np.random.default_rng(0)
    noise = rng.standard_normal((w + 4, c))
    logits = np.ascontiguousarray(sum(noise[i:i + w] for i in range(5)) / np.sqrt(5.0), np.float32)
    rules = [calls.Rule(float(np.percentile(logits[:, i], 70)), float(np.percentile(logits[:, i], 40)), 2.0, 1.5) for i in range(c)]
    t = calls.ticks(np.round(np.arange(w) * 0.96, 2))
    adjacent = calls.adjacent_ticks(0.96)
    _, seg = calls.bin_segments(t, calls.bin_ticks(args.bin_s))
    # the embedder's share: launch sets of 64 parts x 64 windows until the windows are covered
    sets = -(-w // 4096)
    audio = torch.from_numpy((0.1 * rng.standard_normal(64 * 64 * D.WINDOW_SAMPLES)).astype(np.float32)).cuda()
    parts = list(audio.split(64 * D.WINDOW_SAMPLES))
    engine = HipEngine(modelname=None)
    try:
        hop, step = hop_samples(0.96), patch_step(0.96)
        caller = calls.Caller(rules, device=engine.device)
        dev = torch.from_numpy(logits).to(engine.device)
        lib = _lib.load()
        t_dev, seg_dev = torch.from_numpy(t).to(engine.device), torch.from_numpy(seg).to(engine.device)
        rules_dev = caller._rules_dev(adjacent)
        marks = torch.empty((c, w), dtype=torch.uint8, device=engine.device)
        events = torch.empty((c, w, 5), dtype=torch.int32, device=engine.device)
        n_events = torch.empty((c,), dtype=torch.int32, device=engine.device)
        b = int(seg.shape[0]) - 1
        counts = torch.empty((c, b, 2), dtype=torch.int32, device=engine.device)
        values = torch.empty((c, b, 2), dtype=torch.float32, device=engine.device)
        stream = torch.cuda.current_stream(engine.device).cuda_stream

        def launches():
            _lib.check(lib.bd_calls_events(dev.data_ptr(), w, c, c, 1, t_dev.data_ptr(), adjacent, rules_dev.data_ptr(),
                                           marks.data_ptr(), events.data_ptr(), n_events.data_ptr(), stream))
            _lib.check(lib.bd_calls_bins(dev.data_ptr(), w, c, c, 1, marks.data_ptr(), seg_dev.data_ptr(), b, counts.data_ptr(),
                                         values.data_ptr(), stream))

        def host():
            m, found = calls.events_host(logits, t, adjacent, rules)
            return found, calls.bins_host(logits, m, seg)

        call_ms, launch_ms, embed_ms, host_ms = [], [], [], []
        for turn in range(args.warmup + args.reps):
            k, got = clocked(lambda: caller.call(dev, t, adjacent, seg))
            l = once(launches)
            e = once(lambda: [engine.launch(parts, hop, step, True, False) for _ in range(sets)])
            h, (found, (host_counts, host_values)) = clocked(host)
            if turn >= args.warmup:
                call_ms.append(k)
                launch_ms.append(l)
                embed_ms.append(e)
                host_ms.append(h)
        equal = (all(np.array_equal(p, q) for p, q in zip(got.events, found)) and np.array_equal(got.counts, host_counts)
                 and np.array_equal(got.values.view(np.uint32), host_values.view(np.uint32)))
    finally:
        engine.close()
    med = lambda v: round(float(np.median(v)), 4)          # noqa: E731
    print(json.dumps({"windows": w, "columns": c, "bins": b, "tiles": -(-w // _lib.CALLS_TILE),
                      "events": int(sum(len(f) for f in found)), "kept": int(sum(int(f[:, 4].sum()) for f in found)),
                      "device_equals_host": bool(equal),
                      "call_ms": med(call_ms), "call_ms_all": [round(v, 4) for v in call_ms],
                      "launches_ms": med(launch_ms), "launches_ms_all": [round(v, 4) for v in launch_ms],
                      "embed_ms": med(embed_ms), "embed_ms_all": [round(v, 4) for v in embed_ms], "embed_windows": sets * 4096,
                      "host_ms": med(host_ms), "host_ms_all": [round(v, 4) for v in host_ms],
                      "launches_over_embed": round(float(np.median(launch_ms)) / float(np.median(embed_ms)), 5)}))


if __name__ == "__main__":
    main()
