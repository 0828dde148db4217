"""bd_mix beside the CNN it feeds: 64 clips of 10 windows mixed by one bd_mix call, and the engine.launch of the same 640
windows, each timed with HIP events (median of 5 calls after 2 warm-up calls).

    python tools/mix_bench.py [--clips 64] [--windows 10] [--reps 5] [--warmup 2]

Prints one JSON line.  `mix_bytes` is what the mix has to move, 3 x 4 x samples (two sources read, one output written; the
second pass's re-read is meant to hit the Infinity Cache), `mix_gbps` that over the mix time, `mix_share_of_hbm` that over the
6.3 TB/s a streaming kernel reaches on this part.  The expectation to report against: mixing costs a small fraction of
embedding the same windows."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_ACHIEVABLE = 6.3e12


def timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    os.environ.setdefault("BUZZDETECT_SYNTHETIC_WEIGHTS", "1")
    import torch
    from buzzdetect_amd import dataset as D
    from buzzdetect_amd.engine import HipEngine, hop_samples, patch_step
    if not torch.cuda.is_available():
        raise SystemExit("mix_bench needs a HIP device: a time taken anywhere else says nothing")
    n = args.windows * D.WINDOW_SAMPLES
    rng = np.random.default_rng(0)
    total = (args.clips + 1) * n + 977
    audio = torch.from_numpy((0.1 * rng.standard_normal(2 * total)).astype(np.float32)).cuda()
    ev, nz = audio[:total], audio[total:]
    ev_off = np.arange(args.clips) * n + 1                        # odd offsets: the general, unaligned case
    nz_off = np.arange(args.clips) * n + 3
    clips = D.mix_descriptors(ev_off, nz_off, np.full(args.clips, n), rng.choice([0.0, 5.0, 10.0, 20.0], args.clips),
                              np.zeros(args.clips))
    out = torch.empty(args.clips * n, dtype=torch.float32, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    mix_ms, mix_all = timed(lambda: D.mix_device(ev, nz, clips, out=out, workspace=ws), args.reps, args.warmup)
    engine = HipEngine(modelname=None)
    try:
        hop, step = hop_samples(0.96), patch_step(0.96)
        parts = [out[int(c["out_off"]): int(c["out_off"]) + n] for c in clips]
        cnn_ms, cnn_all = timed(lambda: engine.launch(parts, hop, step, True, False), args.reps, args.warmup)
    finally:
        engine.close()
    mix_bytes = 3 * 4 * args.clips * n
    print(json.dumps({"clips": args.clips, "windows": args.clips * args.windows, "samples": args.clips * n,
                      "mix_ms": round(mix_ms, 4), "mix_ms_all": [round(v, 4) for v in mix_all],
                      "cnn_ms": round(cnn_ms, 4), "cnn_ms_all": [round(v, 4) for v in cnn_all],
                      "mix_over_cnn": round(mix_ms / cnn_ms, 4), "mix_bytes": mix_bytes,
                      "mix_gbps": round(mix_bytes / (mix_ms * 1e-3) / 1e9, 1),
                      "mix_share_of_hbm": round(mix_bytes / (mix_ms * 1e-3) / HBM_ACHIEVABLE, 3)}))


if __name__ == "__main__":
    main()
