"""What pitch tracking costs beside embedding: the time of one ``bd_pitch_windows`` launch over 1024 selected windows at the
default lags (16..200), and the time ``engine.launch`` takes to embed 1024 windows on the same device, each the median of 5 runs
after 2 warm-up runs, timed with events on the stream.  Prints one JSON line; no threshold is set on either number.

    python tools/pitch_bench.py
"""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

os.environ.setdefault("BUZZDETECT_SYNTHETIC_WEIGHTS", "1")      # developer tool: timing on the seeded stand-in weights
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WINDOWS = 1024
PARTS = 8
RUNS, WARMUP = 5, 2


def timed(torch, fn):
    times = []
    for i in range(WARMUP + RUNS):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        if i >= WARMUP:
            times.append(start.elapsed_time(end))
    return statistics.median(times), times


def main():
    import torch
    from buzzdetect_amd import _lib, pitch
    from buzzdetect_amd.engine import HipEngine, hop_samples, patch_step
    lib = _lib.load()
    engine = HipEngine(embeddername="yamnet_k2", modelname=None)
    try:
        per = WINDOWS // PARTS
        n = per * _lib.PITCH_WINDOW + 240                               # exactly `per` windows a part at a hop of 0.96 s
        rng = np.random.default_rng(0)
        t = np.arange(n) / 16000.0
        parts = [engine.to_device((0.1 * np.sin(2 * np.pi * (120.0 + 60.0 * i) * t) + 0.03 * rng.standard_normal(n)).astype(np.float32))
                 for i in range(PARTS)]
        hop, step = hop_samples(0.96), patch_step(0.96)
        counts = [engine.num_windows(n, hop, step) for _ in parts]
        assert sum(counts) == WINDOWS, counts
        embed_ms, embed_all = timed(torch, lambda: engine.launch(parts, hop, step, want_embeddings=True, want_logits=False))

        tracker = pitch.PitchTracker(device=engine.device)
        x = torch.cat([p[:per * _lib.PITCH_WINDOW] for p in parts])
        sel = torch.arange(WINDOWS, dtype=torch.int32, device=engine.device)
        values = torch.empty((WINDOWS, 2), dtype=torch.float32, device=engine.device)
        voiced = torch.empty((WINDOWS,), dtype=torch.int32, device=engine.device)
        stream = torch.cuda.current_stream(engine.device)

        def track():
            _lib.check(lib.bd_pitch_windows(x.data_ptr(), int(x.numel()), sel.data_ptr(), WINDOWS, _lib.PITCH_WINDOW,
                                            C.addressof(tracker.params), values.data_ptr(), voiced.data_ptr(), None, stream.cuda_stream))

        track_ms, track_all = timed(torch, track)
        print(json.dumps({"windows": WINDOWS, "lags": [tracker.lag_lo, tracker.lag_hi], "track_ms": round(track_ms, 4),
                          "embed_ms": round(embed_ms, 4), "track_over_embed": round(track_ms / embed_ms, 4),
                          "track_runs_ms": [round(v, 4) for v in track_all], "embed_runs_ms": [round(v, 4) for v in embed_all],
                          "voiced_windows": int((voiced.cpu() == _lib.PITCH_FRAMES).sum()), "device": torch.cuda.get_device_name(engine.device)}))
    finally:
        engine.close()


if __name__ == "__main__":
    main()
