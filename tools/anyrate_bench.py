"""The any-ratio resampler on the MI355X: one JSON line.

    python tools/anyrate_bench.py [--hours 4] [--reps 3] [--out DIR]

kernel   engine.resample alone on a 600 s chunk of mono 16-bit PCM at 47 999 Hz and 768 kHz (anyrate_kernel) and, for
         comparison, 48 000 Hz (bd_resample's matrix-core path): HIP events, three rounds of the three in turn in one process,
         the best of each; microseconds per chunk, the fraction of the vector FMA peak the filter's multiply-adds amount to
         and the fraction of the HBM peak the chunk's bytes (input read + output written) amount to.
analyze  analyze() on `--hours` of 47 999 Hz mono 16-bit WAV and on a 48 000 Hz WAV of the same sample count, in one
         process: a warm-up call each, then `--reps` rounds of the two in turn; audio-seconds per second of wall time, every
         round's rate (the spread) and the ratio of the bests.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools import pcmgen as G  # noqa: E402

HBM_PEAK = 8e12
FMA_PEAK = 157.3e12 / 2           # vector f32 fused multiply-adds per second
PERIOD = 48000 * 60


def bench_kernel(rounds: int = 3) -> dict:
    import torch
    from buzzdetect_amd.engine import HipEngine
    from oracle import resample_oracle as RO
    engine = HipEngine()
    dev = engine.device
    gen = torch.Generator(device=dev).manual_seed(1)
    cases = {}
    for rate in (47999, 768000, 48000):
        n = rate * 600
        q = torch.randint(-20000, 20000, (n,), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
        out = engine.resample(q, rate)                        # first use: designs and uploads the ratio's table
        cases[rate] = (q, torch.empty_like(out))
    torch.cuda.synchronize()
    best = {rate: float("inf") for rate in cases}
    for _ in range(rounds):
        for rate, (q, out) in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            reps = 4
            e0.record()
            for _ in range(reps):
                engine.resample(q, rate, out=out)
            e1.record()
            e1.synchronize()
            best[rate] = min(best[rate], e0.elapsed_time(e1) / 1e3 / reps)
    res = {}
    for rate, (q, out) in cases.items():
        up, down = RO.ratio(rate, 16000)
        max_rate = max(up, down)
        fp, fs = (e / max_rate for e in RO.hq_band_edges())
        half = (int(np.ceil((RO.HQ_DESIGN_ATTENUATION_DB - 7.95) / (2.285 * np.pi * (fs - fp)))) + 1) // 2
        taps = 2 * (half // up) + 1                           # multiply-adds the definition needs per output
        rows = 1 if up <= 256 else 4                          # ... and what the kernel spends (cubic: four rows)
        t = best[rate]
        res[str(rate)] = {"us": round(t * 1e6, 1), "audio_s_per_s": round(600.0 / t), "taps_per_output": taps,
                          "fma_fraction": round(out.numel() * taps * (rows if rate != 48000 else 1) / t / FMA_PEAK, 3),
                          "hbm_fraction": round((q.numel() * 2 + out.numel() * 4) / t / HBM_PEAK, 4)}
    engine.close()
    return {"kernel_600s_mono_s16": res}


def write_wav(path: str, rate: int, n: int) -> None:
    pcm = G.test_signal(PERIOD, 1, 16, seed=11).astype(np.int16)
    reps = n // PERIOD + 1
    body = (pcm.astype("<i2").tobytes() * reps)[: 2 * n]
    data = G.wav16(pcm[:8], rate)
    head = data[:44]
    head = head[:4] + (36 + len(body)).to_bytes(4, "little") + head[8:40] + len(body).to_bytes(4, "little")
    with open(path, "wb") as f:
        f.write(head)
        f.write(body)


def bench_analyze(hours: float, reps: int, root: str) -> dict:
    from buzzdetect_amd.analyze import analyze
    from buzzdetect_amd.engine import HipEngine
    n = int(48000 * 3600 * hours)
    engines = [HipEngine(), HipEngine()]
    dirs = {}
    for rate in (48000, 47999):
        dirs[rate] = os.path.join(root, str(rate))
        os.makedirs(dirs[rate], exist_ok=True)
        write_wav(os.path.join(dirs[rate], "long.wav"), rate, n)

    def once(rate: int, tag: str):
        out = os.path.join(root, "out_" + tag)
        t = time.perf_counter()
        rep = analyze("model_general_v3", chunklength=600, dir_audio=dirs[rate], dir_out=out, engines=engines)
        dt = time.perf_counter() - t
        shutil.rmtree(out, ignore_errors=True)
        assert rep.files_done == 1, rep.messages
        return rep.audio_seconds / dt, {k: round(v, 3) for k, v in rep.busy.items()}

    rates = {48000: [], 47999: []}
    busy = {}
    for rate in rates:
        once(rate, "warm")
    for _ in range(reps):
        for rate in rates:
            x, busy[rate] = once(rate, str(rate))
            rates[rate].append(x)
    for e in engines:
        e.close()
    best = {k: max(v) for k, v in rates.items()}
    return {"analyze_hours": hours, "analyze_reps": reps,
            "analyze": {"audio_s_per_s_47999": round(best[47999]), "audio_s_per_s_48000": round(best[48000]),
                        "over_48000": round(best[47999] / best[48000], 3), "rates_47999": [round(x) for x in rates[47999]],
                        "rates_48000": [round(x) for x in rates[48000]], "busy_47999": busy[47999], "busy_48000": busy[48000]}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the JSON line here too")
    args = ap.parse_args()
    os.environ.setdefault("BUZZDETECT_SYNTHETIC_WEIGHTS", "1")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("anyrate_bench: needs an MI355X")
    result = {"metric": "anyrate_resample"}
    result.update(bench_kernel())
    if args.hours > 0:
        root = tempfile.mkdtemp(prefix="anyrate_bench.")
        try:
            result.update(bench_analyze(args.hours, args.reps, root))
        finally:
            shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
