"""pcmio's decoders on the MI355X: one JSON line.

    python tools/pcm_bench.py [--hours 4] [--reps 2] [--out DIR]

decode   bd_pcm_decode alone on a 600 s chunk of 48 kHz stereo for each codec / layout: microseconds per chunk (HIP events
         after warm-up over at least half a second of work), output bytes per second as a fraction of the 8 TB/s HBM peak,
         and for ADPCM the waves per SIMD of the decode launch.
analyze  analyze() on `--hours` of 48 kHz mono audio in each format and as a 16-bit WAV of the same samples, in one process:
         after a warm-up call, `--reps` rounds of (WAV, format) in turn; audio-seconds per second of wall time, the best of
         the rounds for each, and the format's ratio to the WAV of its own rounds.  One format's file (and the WAV) exists at
         a time.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time
from typing import Tuple

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools import pcmgen as G  # noqa: E402

RATE = 48000
HBM_PEAK = 8e12
PERIOD = 48000 * 60               # one minute of signal, repeated


def signal(n: int, ch: int = 1) -> np.ndarray:
    base = G.test_signal(PERIOD, ch, 16, seed=11).astype(np.int16)
    return np.tile(base, (n // PERIOD + 1, 1))[:n]


def tiled(data: bytes, block: int, nblk: int) -> bytes:
    """`data` (whole blocks of `block` bytes) repeated to nblk blocks: ADPCM blocks are independent."""
    have = len(data) // block
    return (data * (nblk // have + 1))[: nblk * block]


def chunk_of(kind: str, n: int):
    """(bd_pcm_format, bytes) of n frames of 48 kHz stereo."""
    from buzzdetect_amd import _lib, pcmio
    if kind in ("ima", "ms"):
        ba = 2048
        spb = G.ima_spb(ba, 2) if kind == "ima" else G.ms_spb(ba, 2)
        nblk = -(-n // spb)
        src = signal(spb * 64, 2)
        data, _ = G.ima_encode(src, ba) if kind == "ima" else G.ms_encode(src, ba)
        fmt = pcmio.make_format(_lib.PCM_IMA_ADPCM if kind == "ima" else _lib.PCM_MS_ADPCM, 2, block_align=ba,
                                samples_per_block=spb, coefs=G.MS_COEFS if kind == "ms" else ())
        return fmt, tiled(data, ba, nblk)
    x = signal(n, 2)
    if kind in ("ulaw", "alaw"):
        return pcmio.make_format(_lib.PCM_ULAW if kind == "ulaw" else _lib.PCM_ALAW, 2, 1), G.g711(x, kind)
    if kind == "f32be":
        return pcmio.make_format(_lib.PCM_FLOAT, 2, 4, big_endian=True), G.floats(x / 32768.0, 4, True)
    width = {"be16": 2, "be24": 3, "u8": 1}[kind]
    v = x.astype(np.int64) << 8 if width == 3 else (x.astype(np.int64) >> 8 if width == 1 else x)
    return pcmio.make_format(_lib.PCM_LINEAR, 2, width, big_endian=True, signed=width != 1), G.linear(v, width, True, width != 1)


def bench_decode() -> dict:
    import torch
    from buzzdetect_amd import _lib, pcmio
    lib = _lib.load()
    n = RATE * 600
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    stream = torch.cuda.current_stream(dev)
    res = {}
    for kind in ("ima", "ms", "ulaw", "alaw", "be16", "u8", "be24", "f32be"):
        fmt, data = chunk_of(kind, n)
        body = np.frombuffer(data, np.uint8)
        comp = torch.zeros((body.size + 3) // 4 * 4 + 8, dtype=torch.uint8, device=dev)
        comp[: body.size].copy_(torch.from_numpy(body.copy()))
        ws = torch.zeros(256, dtype=torch.uint8, device=dev)
        s16 = pcmio.out_is_s16(fmt)
        out = torch.empty((n, 2), dtype=torch.int16 if s16 else torch.float32, device=dev)
        status = torch.zeros(C.sizeof(_lib.bd_pcm_status), dtype=torch.uint8, device=dev)

        def once():
            _lib.check(lib.bd_pcm_decode(comp.data_ptr(), body.size, C.byref(fmt), 0, n, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                         status.data_ptr(), stream.cuda_stream))

        for _ in range(3):
            once()
        stream.synchronize()
        st = _lib.bd_pcm_status.from_buffer_copy(status.cpu().numpy().tobytes())
        # bit-exact against the host decoder on the first 10 s (the whole chunk is tests/test_pcm_gpu.py's)
        k = RATE * 10
        host = np.zeros((k, 2), np.int16 if s16 else np.float32)
        hst = _lib.bd_pcm_status()
        nb = -(-k // fmt.samples_per_block) * fmt.block_align
        _lib.check(lib.bd_pcm_decode_host(body.ctypes.data, nb, C.byref(fmt), 0, k, host.ctypes.data, C.byref(hst)))
        ok = st.samples == n and out[:k].cpu().numpy().tobytes() == host.tobytes()
        reps, elapsed = 2, 0.0
        while elapsed < 0.5:
            reps *= 2
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                once()
            e1.record(stream)
            e1.synchronize()
            elapsed = e0.elapsed_time(e1) / 1e3
        per = elapsed / reps
        out_bytes = out.numel() * out.element_size()
        r = {"us": round(per * 1e6, 1), "audio_s_per_s": round(600.0 / per), "in_mb": round(body.size / 1e6, 1),
             "out_mb": round(out_bytes / 1e6, 1), "out_gb_s": round(out_bytes / per / 1e9, 1),
             "hbm_fraction": round((out_bytes + body.size) / per / HBM_PEAK, 3), "bit_exact": ok}
        if fmt.samples_per_block > 1:
            lanes = -(-n // fmt.samples_per_block) * 2
            r["waves_per_simd"] = round(-(-lanes // 64) / (4 * cus), 2)
        res[kind] = r
        del comp, out
    return {"decode_600s_48k_stereo": res}


def write_format(path: str, kind: str, n: int) -> None:
    """n frames (a multiple of PERIOD) of signal() in `kind`: one period encoded, its bytes repeated (every encoding here is
    per sample or per independent block)."""
    pcm, reps = signal(PERIOD), n // PERIOD
    if kind == "wav":
        data = G.wav16(pcm, RATE)
        head, body = data[:44], data[44:]
        data = head[:40] + (len(body) * reps).to_bytes(4, "little") + body * reps
        data = data[:4] + (len(data) - 8).to_bytes(4, "little") + data[8:]
    elif kind == "aiff":
        data = G.aiff(G.linear(pcm, 2, True) * reps, RATE, 1, n, 16)
    elif kind == "w64":
        data = G.w64(G.fmt_body(1, 1, RATE, 16, 2), pcm.astype("<i2").tobytes() * reps)
    elif kind == "au_ulaw":
        data = G.au(G.g711(pcm, "ulaw") * reps, RATE, 1, 1)
    elif kind == "wav_alaw":
        data = G.wave(G.fmt_body(6, 1, RATE, 8, 1), G.g711(pcm, "alaw") * reps)
    elif kind == "au_24":
        data = G.au(G.linear(pcm.astype(np.int64) << 8, 3, True) * reps, RATE, 1, 4)
    elif kind in ("wav_ima", "wav_ms"):
        ba = 1024
        spb = G.ima_spb(ba, 1) if kind == "wav_ima" else G.ms_spb(ba, 1)
        src = pcm[: spb * (PERIOD // spb)]
        enc, _ = G.ima_encode(src, ba) if kind == "wav_ima" else G.ms_encode(src, ba)
        fmt = G.fmt_ima(1, RATE, ba, spb) if kind == "wav_ima" else G.fmt_ms(1, RATE, ba, spb)
        data = G.wave(fmt, tiled(enc, ba, -(-n // spb)), fact=n)
    else:
        raise ValueError(kind)
    with open(path, "wb") as f:
        f.write(data)


FORMATS = ("aiff", "w64", "au_ulaw", "wav_alaw", "wav_ima", "wav_ms", "au_24")
EXT = {"wav": ".wav", "aiff": ".aiff", "w64": ".w64", "au_ulaw": ".au", "wav_alaw": ".wav", "au_24": ".au", "wav_ima": ".wav",
       "wav_ms": ".wav"}


def bench_analyze(hours: float, reps: int, root: str) -> dict:
    from buzzdetect_amd.analyze import analyze
    from buzzdetect_amd.engine import HipEngine
    n = max(1, round(RATE * 3600 * hours / PERIOD)) * PERIOD
    engines = [HipEngine(), HipEngine()]

    wav_dir = os.path.join(root, "wav")
    os.makedirs(wav_dir, exist_ok=True)
    write_format(os.path.join(wav_dir, "long.wav"), "wav", n)

    def once(d: str, tag: str) -> Tuple[float, dict]:
        out = os.path.join(root, "out_" + tag)
        t = time.perf_counter()
        rep = analyze("model_general_v3", chunklength=600, dir_audio=d, dir_out=out, engines=engines)
        dt = time.perf_counter() - t
        shutil.rmtree(out, ignore_errors=True)
        return rep.audio_seconds / dt, {k: round(v, 3) for k, v in rep.busy.items()}

    once(wav_dir, "warm")
    res = {}
    for kind in FORMATS:
        d = os.path.join(root, kind)
        os.makedirs(d, exist_ok=True)
        write_format(os.path.join(d, "long" + EXT[kind]), kind, n)
        once(d, "warm")                              # one warm-up call of the format, then WAV and format in turn
        rates = {"wav": [], kind: []}
        busy = {}
        for r in range(reps):
            rates["wav"].append(once(wav_dir, "wav")[0])
            x, busy = once(d, kind)
            rates[kind].append(x)
        shutil.rmtree(d, ignore_errors=True)
        best = {k: max(v) for k, v in rates.items()}
        res[kind] = {"audio_s_per_s": round(best[kind]), "wav_audio_s_per_s": round(best["wav"]),
                     "over_wav": round(best[kind] / best["wav"], 3), "rates": [round(x) for x in rates[kind]],
                     "wav_rates": [round(x) for x in rates["wav"]], "busy": busy}
    for e in engines:
        e.close()
    return {"analyze_hours": hours, "analyze_reps": reps, "analyze": res}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None, help="write the JSON line here too")
    args = ap.parse_args()
    os.environ.setdefault("BUZZDETECT_SYNTHETIC_WEIGHTS", "1")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pcm_bench: needs an MI355X")
    result = {"metric": "pcm_decode"}
    result.update(bench_decode())
    root = tempfile.mkdtemp(prefix="pcm_bench.")
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
