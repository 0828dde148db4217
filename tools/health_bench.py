"""What recording health costs: (1) one ``bd_health_levels`` call (its three launches) on 600 s of 48 kHz stereo 16-bit audio cut
into maximal segments - microseconds per call and the bytes of the chunk, which the call reads twice, against the 8 TB/s HBM
peak; (2) one ``bd_health_spectrum`` launch on a 200 s chunk at 16 kHz beside ``engine.launch`` embedding the same chunk.  Each
the median of 5 runs after 2 warm-up runs, timed with events on the stream, with the spread.  Prints one JSON line; no threshold
is set on any number.

    python tools/health_bench.py
"""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

os.environ.setdefault("BUZZDETECT_SYNTHETIC_WEIGHTS", "1")      # developer tool: timing on the seeded stand-in weights
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RUNS, WARMUP = 5, 2
HBM_PEAK = 8.0e12                                               # bytes per second


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
    from buzzdetect_amd import _lib, health
    from buzzdetect_amd.engine import HipEngine, hop_samples, patch_step
    lib = _lib.load()
    engine = HipEngine(embeddername="yamnet_k2", modelname=None)
    try:
        meter = health.HealthMeter(device=engine.device)
        stream = torch.cuda.current_stream(engine.device)

        rate, seconds, ch = 48000, 600, 2
        n = rate * seconds
        raw = torch.randint(-20000, 20000, (n, ch), dtype=torch.int16, device=engine.device)
        edges, _ = meter.level_segments(n, rate, 0)
        s = edges.shape[0] - 1
        edges_dev = torch.from_numpy(edges).to(engine.device)
        records = torch.empty((s, ch, 10), dtype=torch.int32, device=engine.device)
        need = _lib.check(lib.bd_health_levels_workspace_bytes(s, ch))
        workspace = torch.empty(need, dtype=torch.uint8, device=engine.device)
        p = meter.params(True, rate)

        def levels():
            _lib.check(lib.bd_health_levels(raw.data_ptr(), _lib.HEALTH_S16, n, ch, edges_dev.data_ptr(), s, C.addressof(p), records.data_ptr(),
                                            workspace.data_ptr(), need, stream.cuda_stream))

        levels_ms, levels_all = timed(torch, levels)
        chunk_bytes = n * ch * 2

        n16 = 200 * 16000
        rng = np.random.default_rng(0)
        pcm = engine.to_device((0.1 * rng.standard_normal(n16)).astype(np.float32))
        fedges, _ = health.frame_segments(0, n16, meter.bin_ticks)
        t = fedges.shape[0] - 1
        fedges_dev = torch.from_numpy(fedges).to(engine.device)
        tables = torch.from_numpy(meter.tables).to(engine.device)
        power = torch.empty((t, meter.n_bands), dtype=torch.float32, device=engine.device)
        bad = torch.empty((t,), dtype=torch.int32, device=engine.device)

        def spectrum():
            _lib.check(lib.bd_health_spectrum(pcm.data_ptr(), n16, fedges_dev.data_ptr(), t, meter.bedges.ctypes.data, meter.n_bands,
                                              tables.data_ptr(), power.data_ptr(), bad.data_ptr(), stream.cuda_stream))

        spectrum_ms, spectrum_all = timed(torch, spectrum)
        hop, step = hop_samples(0.96), patch_step(0.96)
        embed_ms, embed_all = timed(torch, lambda: engine.launch([pcm], hop, step, want_embeddings=True, want_logits=False))
        print(json.dumps({
            "levels": {"seconds": seconds, "rate": rate, "channels": ch, "segments": s, "us_per_call": round(1e3 * levels_ms, 1),
                       "runs_us": [round(1e3 * v, 1) for v in levels_all], "chunk_bytes": chunk_bytes,
                       "share_of_hbm_peak_reading_the_chunk_twice": round(2 * chunk_bytes / (levels_ms * 1e-3) / HBM_PEAK, 4)},
            "spectrum": {"seconds": 200, "frames": int(fedges[-1]), "segments": t, "bands": meter.n_bands, "spectrum_ms": round(spectrum_ms, 4),
                         "embed_ms": round(embed_ms, 4), "spectrum_over_embed": round(spectrum_ms / embed_ms, 4),
                         "spectrum_runs_ms": [round(v, 4) for v in spectrum_all], "embed_runs_ms": [round(v, 4) for v in embed_all]},
            "device": torch.cuda.get_device_name(engine.device)}))
    finally:
        engine.close()


if __name__ == "__main__":
    main()
