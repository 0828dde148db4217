"""One engine carrying an ensemble of K heads (buzzdetect_amd.engine.HipEngine(head=EnsembleWeights)) against the plain set of
the same K members (HipEngine(heads={...}): how the same K columns were reached before there were ensembles - the difference is
the combine launch) and against K engines carrying one member each, run one after another; on the same device in the same
process, alternating.

    python tools/ensemble_bench.py [--chunks 4] [--windows 1024] [--repeats 5] [--warmup 2] [--members 5 20] [--combine mean]

Two shapes of member, 1024 -> 13 (the fused route) and 1024 -> 128 -> 13 (the stack route; at K = 20 the set's limits refuse it:
2560 hidden floats at depth 0, 2048 allowed - reported as refused); a call is predict_batch of `chunks` x `windows` windows of
synthetic audio, timed with HIP events around the call on the current stream.  Prints one JSON line per (shape, K): the median
milliseconds of the three sides over the repeats, each side's spread, the ensemble's call in units of one lone call, and profile
slot 28 (the head launches; bd_profile_read) of the ensemble against the plain set, per call.  The embedder weights are the seeded
stand-ins unless real ones are configured: the times do not depend on their values.  There is no gate on these numbers."""
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
    ap.add_argument("--members", type=int, nargs="+", default=[5, 20])
    ap.add_argument("--combine", default="mean", choices=["mean", "softmax", "sigmoid"])
    args = ap.parse_args()
    os.environ.setdefault("BUZZDETECT_SYNTHETIC_WEIGHTS", "1")
    import torch
    from buzzdetect_amd import modeldir, weights
    from buzzdetect_amd.engine import HipEngine
    rng = np.random.default_rng(0)
    chunk = (rng.standard_normal(HOP * args.windows + 240) * 0.1).astype(np.float32)
    combine, link = ("mean", None) if args.combine == "mean" else ("mean_probability", args.combine)

    def timed(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end)

    def slot28(engine, fn):
        engine.profile_enable(True)
        engine.profile_read()
        fn()
        torch.cuda.synchronize()
        ms, launches = engine.profile_read()
        engine.profile_enable(False)
        return float(ms[28]), int(launches[28])

    for shape, (widths, acts) in SHAPES.items():
        for k in args.members:
            classes = [f"c{i}" for i in range(widths[-1])]
            heads = {f"m{i:02d}": weights.HeadWeights(modeldir.glorot_layers(widths, acts, seed=i), classes) for i in range(k)}
            ens = weights.EnsembleWeights(heads, combine, link, classes)
            try:
                weights.check_head_set({"ensemble": ens})
            except ValueError as exc:                    # (20 x 128 hidden floats pass the 2048 one depth may take)
                print(json.dumps({"shape": shape, "members": k, "refused": str(exc).split(":")[0] + ": " + str(exc).split(":")[1].strip()}),
                      flush=True)
                continue
            one = HipEngine(head=ens)
            plain = HipEngine(heads=heads)
            alone = [HipEngine(head=h) for h in heads.values()]
            try:
                parts = [one.to_device(chunk) for _ in range(args.chunks)]

                def run_ensemble():
                    one.predict_batch(parts, 0.96)

                def run_set():
                    plain.predict_batch(parts, 0.96)

                def run_serial():
                    for e in alone:
                        e.predict_batch(parts, 0.96)

                for _ in range(args.warmup):
                    run_ensemble()
                    run_set()
                    run_serial()
                torch.cuda.synchronize()
                t_ens, t_set, t_serial = [], [], []
                for _ in range(args.repeats):
                    t_ens.append(timed(run_ensemble))
                    t_set.append(timed(run_set))
                    t_serial.append(timed(run_serial))
                ens_ms, set_ms, serial_ms = (float(np.median(t)) for t in (t_ens, t_set, t_serial))
                s28_ens, n28_ens = slot28(one, run_ensemble)
                s28_set, n28_set = slot28(plain, run_set)
                print(json.dumps({"shape": shape, "members": k, "combine": args.combine, "windows": args.chunks * args.windows,
                                  "ensemble_ms": round(ens_ms, 3), "set_ms": round(set_ms, 3), "serial_ms": round(serial_ms, 3),
                                  "ensemble_minus_set_ms": round(ens_ms - set_ms, 3),
                                  "one_lone_call_ms": round(serial_ms / k, 3),
                                  "ensemble_in_lone_calls": round(ens_ms / (serial_ms / k), 3),
                                  "serial_over_ensemble": round(serial_ms / ens_ms, 2),
                                  "ensemble_ms_spread": [round(min(t_ens), 3), round(max(t_ens), 3)],
                                  "set_ms_spread": [round(min(t_set), 3), round(max(t_set), 3)],
                                  "serial_ms_spread": [round(min(t_serial), 3), round(max(t_serial), 3)],
                                  "slot28_ensemble_ms": round(s28_ens, 3), "slot28_set_ms": round(s28_set, 3),
                                  "slot28_ensemble_launches": n28_ens, "slot28_set_launches": n28_set}), flush=True)
            finally:
                one.close()
                plain.close()
                for e in alone:
                    e.close()


if __name__ == "__main__":
    main()
