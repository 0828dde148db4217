"""FLAC decode on the MI355X: one JSON line.

    python tools/flac_bench.py [--hours 4] [--reps 2] [--out DIR]

decode   bd_flac_decode alone on a 600 s chunk of 48 kHz mono 16-bit (LPC order 8, block 4096): audio-seconds per second,
         timed with HIP events after warm-up over at least one second of work.
analyze  analyze() on the same `--hours` of audio as FLAC and as WAV, alternating, in one process (audio-seconds per
         second of wall time each, the best of `--reps`), and their ratio.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import shutil
import struct
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools import flacgen as G  # noqa: E402

RATE = 48000
PERIOD = 4096 * 704               # ~60 s of signal, repeated: the writer reuses the bodies of repeated frames


def signal(n: int) -> np.ndarray:
    base = G.test_signal(PERIOD, 1, 16, seed=11).astype(np.int16)
    return np.tile(base, (n // PERIOD + 1, 1))[:n]


def write_wav(path: str, pcm: np.ndarray) -> None:
    data_len = pcm.size * 2
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + data_len) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, RATE, RATE * 2, 2, 16))
        f.write(b"data" + struct.pack("<I", data_len))
        for a in range(0, pcm.shape[0], 1 << 24):
            f.write(pcm[a: a + (1 << 24)].astype("<i2").tobytes())


def bench_decode() -> dict:
    import torch
    from buzzdetect_amd import _lib
    lib = _lib.load()
    n = RATE * 600
    data, offs = G.encode(signal(n), RATE, 16, blocksize=4096, subframe_kind=("lpc", 8), return_offsets=True)
    start = offs[0][1]
    body = np.frombuffer(data[start:], np.uint8)
    si = _lib.bd_flac_streaminfo(4096, 4096, RATE, 1, 16, 0, n)
    dev = torch.device("cuda", 0)
    comp = torch.zeros(body.size + 8, dtype=torch.uint8, device=dev)
    comp[: body.size].copy_(torch.from_numpy(body.copy()))
    ws = torch.empty(_lib.check(lib.bd_flac_workspace_bytes(C.byref(si), body.size, n)), dtype=torch.uint8, device=dev)
    out = torch.empty((n, 1), dtype=torch.int16, device=dev)
    status = torch.zeros(C.sizeof(_lib.bd_flac_status), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)

    def once():
        _lib.check(lib.bd_flac_decode(comp.data_ptr(), body.size, C.byref(si), 0, n, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                      status.data_ptr(), stream.cuda_stream))

    for _ in range(3):
        once()
    stream.synchronize()
    st = _lib.bd_flac_status.from_buffer_copy(status.cpu().numpy().tobytes())
    ok = st.samples == n and bool(torch.equal(out[:, 0].cpu(), torch.from_numpy(signal(n)[:, 0])))
    reps, elapsed = 4, 0.0
    while elapsed < 1.0:
        reps *= 2
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            once()
        e1.record(stream)
        e1.synchronize()
        elapsed = e0.elapsed_time(e1) / 1e3
    per = elapsed / reps
    return {"decode_audio_s_per_s": 600.0 / per, "decode_us_per_600s_chunk": per * 1e6, "decode_bit_exact": ok,
            "compressed_bytes_per_600s": int(body.size), "decode_reps": reps}


def bench_analyze(hours: float, reps: int, root: str) -> dict:
    from buzzdetect_amd.analyze import analyze
    from buzzdetect_amd.engine import HipEngine
    n = int(RATE * 3600 * hours)
    pcm = signal(n)
    for d in ("flac", "wav"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    t0 = time.perf_counter()
    with open(os.path.join(root, "flac", "long.flac"), "wb") as f:
        f.write(G.encode(pcm, RATE, 16, blocksize=4096, subframe_kind=("lpc", 8), seektable=RATE * 10))
    write_wav(os.path.join(root, "wav", "long.wav"), pcm)
    gen_s = time.perf_counter() - t0
    del pcm
    engines = [HipEngine(), HipEngine()]
    rates = {"flac": [], "wav": []}
    busy = {}
    for r in range(reps + 1):                        # round 0 warms both paths up
        for kind in ("flac", "wav"):
            out = os.path.join(root, f"out_{kind}_{r}")
            t = time.perf_counter()
            rep = analyze("model_general_v3", chunklength=600, dir_audio=os.path.join(root, kind), dir_out=out, engines=engines)
            dt = time.perf_counter() - t
            if r:
                rates[kind].append(rep.audio_seconds / dt)
                busy[kind] = {k: round(v, 3) for k, v in rep.busy.items()}
            shutil.rmtree(out, ignore_errors=True)
    for e in engines:
        e.close()
    best = {k: max(v) for k, v in rates.items()}
    return {"analyze_hours": hours, "analyze_flac_audio_s_per_s": best["flac"], "analyze_wav_audio_s_per_s": best["wav"],
            "analyze_flac_over_wav": best["flac"] / best["wav"], "analyze_rates": rates, "analyze_busy": busy,
            "fixture_seconds": round(gen_s, 1)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None, help="write the JSON line here too")
    args = ap.parse_args()
    os.environ.setdefault("BUZZDETECT_SYNTHETIC_WEIGHTS", "1")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("flac_bench: needs an MI355X")
    result = {"metric": "flac_decode"}
    result.update(bench_decode())
    root = tempfile.mkdtemp(prefix="flac_bench.")
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
