"""One engine carrying a set of M heads against M engines carrying one head each, run one after another
(buzzdetect_amd.engine.HipEngine(heads={...}) against HipEngine(head=...)), on the same device in the same process, alternating.

    python tools/headset_bench.py [--chunks 4] [--windows 1024] [--repeats 5] [--warmup 2] [--members 1 5 20]

Two shapes of member, 1024 -> 13 (the fused route) and 1024 -> 128 -> 13 (the stack route); a call is predict_batch of
`chunks` x `windows` windows of synthetic audio, timed with HIP events around the call on the current stream.  The serial side
is the yardstick: the same M models, each on its own engine, called one after the other - what comparing M models costs without
the set.  Prints one JSON line per (shape, M): the median milliseconds of both sides over the repeats, each side's spread, the
set's call in units of one lone call, and profile slot 28 (pool / head launches; bd_profile_read) of the set against the sum
over the lone engines, per call.  The embedder weights are the seeded stand-ins unless real ones are configured: the times do
not depend on their values.  A set the limits refuse (20 members of 1024 -> 128 -> 13: 2560 hidden floats at depth 0, 2048 allowed) is
reported as refused.  There is no gate on these numbers."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"1024-13": ([13], ["linear"]), "1024-128-13": ([128, 13], ["relu", "linear"])}
HOP = 15360


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--members", type=int, nargs="+", default=[1, 5, 20])
    args = ap.parse_args()
    os.environ.setdefault("BUZZDETECT_SYNTHETIC_WEIGHTS", "1")
    import torch
    from buzzdetect_amd import modeldir, weights
    from buzzdetect_amd.engine import HipEngine
    rng = np.random.default_rng(0)
    chunk = (rng.standard_normal(HOP * args.windows + 240) * 0.1).astype(np.float32)

    def timed(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end)

    def slot28(engines, fn):
        for e in engines:
            e.profile_enable(True)
            e.profile_read()
        fn()
        torch.cuda.synchronize()
        ms = sum(float(e.profile_read()[0][28]) for e in engines)
        for e in engines:
            e.profile_enable(False)
        return ms

    for shape, (widths, acts) in SHAPES.items():
        for m in args.members:
            heads = {f"m{i:02d}": weights.HeadWeights(modeldir.glorot_layers(widths, acts, seed=i), [f"c{k}" for k in range(widths[-1])])
                     for i in range(m)}
            try:
                weights.check_head_set(heads)
            except ValueError as exc:                    # (20 x 128 hidden floats pass the 2048 one depth may take)
                print(json.dumps({"shape": shape, "members": m, "refused": str(exc).split(":")[0] + ": " + str(exc).split(":")[1].strip()}), flush=True)
                continue
            one = HipEngine(heads=heads)
            alone = [HipEngine(head=h) for h in heads.values()]
            try:
                parts = [one.to_device(chunk) for _ in range(args.chunks)]

                def run_set():
                    one.predict_batch(parts, 0.96)

                def run_serial():
                    for e in alone:
                        e.predict_batch(parts, 0.96)

                for _ in range(args.warmup):
                    run_set()
                    run_serial()
                torch.cuda.synchronize()
                t_set, t_serial = [], []
                for _ in range(args.repeats):
                    t_set.append(timed(run_set))
                    t_serial.append(timed(run_serial))
                set_ms, serial_ms = float(np.median(t_set)), float(np.median(t_serial))
                print(json.dumps({"shape": shape, "members": m, "windows": args.chunks * args.windows,
                                  "set_ms": round(set_ms, 3), "serial_ms": round(serial_ms, 3),
                                  "one_lone_call_ms": round(serial_ms / m, 3),
                                  "set_in_lone_calls": round(set_ms / (serial_ms / m), 3),
                                  "serial_over_set": round(serial_ms / set_ms, 2),
                                  "set_ms_spread": [round(min(t_set), 3), round(max(t_set), 3)],
                                  "serial_ms_spread": [round(min(t_serial), 3), round(max(t_serial), 3)],
                                  "one_lone_call_ms_spread": [round(min(t_serial) / m, 3), round(max(t_serial) / m, 3)],
                                  "slot28_set_ms": round(slot28([one], run_set), 3),
                                  "slot28_lone_sum_ms": round(slot28(alone, run_serial), 3)}), flush=True)
            finally:
                one.close()
                for e in alone:
                    e.close()


if __name__ == "__main__":
    main()
