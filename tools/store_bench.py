"""The embedding store on the MI355X: one JSON line.

    python tools/store_bench.py [--minutes 60] [--reps 5] [--out DIR]

codec    bd_rows_encode and bd_rows_decode alone for each codec, in calls of 4096 and of 65 536 rows on buffers allocated once:
         microseconds per 4096 rows (HIP events around enough calls for half a second of work, after a warm-up; the median of
         `--reps` such timings and their spread), and the bytes the call must move (rows + records) per second as a fraction of
         the 8 TB/s HBM peak.  The small calls show the launch overhead, the large ones the kernels' streaming rate.
score    `--minutes` of 16-bit 48 kHz mono WAV (one-minute signal, repeated; recordings of ten minutes) embedded once per codec, then
         in one process and in turn, `--reps` rounds of: analyze() on the audio, score_store() on each codec's store (its files in
         the page cache: they were just written and read).  Windows per second of wall time, median and spread, and each
         store's ratio to the audio route of its own rounds.  Same model, same engine, same machine, same run.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
import wave

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK = 8e12
ROWS = 4096
LARGE = 65536
CODECS = ("f32", "h", "b")
RATE = 48000


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def bench_codec(reps: int) -> dict:
    """The two entry points called straight through the ABI on buffers allocated once, so that a timing holds the call's two
    memsets and its kernel and nothing of the allocator.  Calls of 4096 rows are short enough for the host's enqueue rate to
    show; calls of 65 536 rows (LARGE) give the kernels' streaming rate, reported per 4096 rows as well."""
    import torch
    from buzzdetect_amd import _lib, store
    lib = _lib.load()
    rng = np.random.default_rng(3)
    block = torch.from_numpy((rng.random((ROWS, 1024)) ** 3 * 6).astype(np.float32)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    for n in (ROWS, LARGE):
        rows = block.repeat(n // ROWS, 1).contiguous()
        back = torch.empty_like(rows)
        sums = torch.empty((store.slices_of(n), 2), dtype=torch.int64, device="cuda")
        flags = torch.empty(1, dtype=torch.int32, device="cuda")
        for codec in CODECS:
            code, rb = _lib.ROWS_CODECS[codec], store.record_bytes(codec)
            records = torch.empty((n, rb), dtype=torch.uint8, device="cuda")
            moved = n * (4096 + rb)

            def encode():
                _lib.check(lib.bd_rows_encode(rows.data_ptr(), n, code, records.data_ptr(), sums.data_ptr(), flags.data_ptr(), stream))

            def decode():
                _lib.check(lib.bd_rows_decode(records.data_ptr(), n, code, back.data_ptr(), sums.data_ptr(), stream))

            for what, call in (("encode", encode), ("decode", decode)):
                for _ in range(20):
                    call()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                calls = max(20, int(0.5 / max(time.perf_counter() - t0, 1e-6)))
                times = []
                for _ in range(reps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(calls):
                        call()
                    b.record()
                    b.synchronize()
                    times.append(a.elapsed_time(b) * 1e3 / calls * ROWS / n)
                us = spread(times)
                out[f"{what}_{codec}_{n}"] = {"us_per_4096_rows": us, "rows_per_call": n, "bytes_moved_per_call": moved,
                                              "calls_per_timing": calls,
                                              "hbm_peak_fraction": moved * ROWS / n / (us["median"] * 1e-6) / HBM_PEAK}
            if codec != "f32":
                assert int(flags.cpu()[0]) == 0
    return out


def write_audio(root: str, minutes: int) -> None:
    rng = np.random.default_rng(17)
    t = np.arange(RATE * 60) / RATE
    minute = 0.2 * np.sin(2 * np.pi * 220 * t) * (0.5 + 0.5 * np.sin(2 * np.pi * 0.7 * t)) + 0.05 * rng.standard_normal(t.size)
    pcm = (np.clip(minute, -1, 1 - 2 ** -15) * 32768).astype("<i2").tobytes()
    os.makedirs(root, exist_ok=True)
    for k in range(0, minutes, 10):
        with wave.open(os.path.join(root, f"rec{k // 10:04d}.wav"), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(RATE)
            for _ in range(min(10, minutes - k)):
                w.writeframes(pcm)


def bench_score(minutes: int, reps: int, work: str) -> dict:
    import torch
    from buzzdetect_amd import store
    from buzzdetect_amd.analyze import analyze
    from buzzdetect_amd.engine import HipEngine
    audio = os.path.join(work, "audio")
    write_audio(audio, minutes)
    engine = HipEngine()
    out = {"minutes": minutes}
    try:
        for codec in CODECS:
            t0 = time.perf_counter()
            rep = store.embed_recordings(audio, os.path.join(work, f"emb_{codec}"), codec=codec, engine=engine)
            torch.cuda.synchronize()
            out[f"embed_{codec}"] = {"seconds": time.perf_counter() - t0, "windows": rep.windows,
                                     "bytes": sum(os.path.getsize(r.path) for r in store.Store(os.path.join(work, f"emb_{codec}")).recordings)}
        rates = {k: [] for k in ("audio",) + CODECS}
        for r in range(reps + 1):                            # round 0 warms every route up and is not counted
            for route in rates:
                dir_out = os.path.join(work, f"out_{route}")
                shutil.rmtree(dir_out, ignore_errors=True)
                t0 = time.perf_counter()
                if route == "audio":
                    rep = analyze(dir_audio=audio, dir_out=dir_out, engine=engine)
                else:
                    rep = store.score_store(os.path.join(work, f"emb_{route}"), "model_general_v3", dir_out, engine=engine)
                torch.cuda.synchronize()
                if r:
                    rates[route].append(rep.windows / (time.perf_counter() - t0))
        for route, v in rates.items():
            out[f"windows_per_s_{route}"] = spread(v)
        for codec in CODECS:
            out[f"ratio_{codec}"] = spread([s / a for s, a in zip(rates[codec], rates["audio"])])
    finally:
        engine.close()
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to DIR/store_bench.json")
    args = ap.parse_args()
    os.environ.setdefault("BUZZDETECT_SYNTHETIC_WEIGHTS", "1")      # developer tool: timing on the seeded stand-in weights
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("store_bench.py measures on a GPU; none is visible")
    work = tempfile.mkdtemp(prefix="store_bench_")
    try:
        result = {"codec": bench_codec(args.reps), "score": bench_score(args.minutes, args.reps, work)}
    finally:
        shutil.rmtree(work, ignore_errors=True)
    line = json.dumps(result)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "store_bench.json"), "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
