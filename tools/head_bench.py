"""What a classifier head costs: its microseconds per 1024-window pass (profile slot 28) and the windows/s of the predict loop
bench.py times (one launch set per 1024-window chunk into caller-owned rows), for the packaged model_general_v3 and for
generated dense stacks.  GPU box.

    python tools/head_bench.py [--models v3 256-13 1024-1024-64 521] [--tree DIR] [--reps 3] [--chunks 60]

``--tree DIR``: import buzzdetect_amd from another checkout (an A/B against a parent commit runs ``--models v3`` on both trees,
alternating).  The head's share is stated against the exact-f32 matrix peak of the MI355X, 157.3 TFLOP/s.
"""
import argparse
import hashlib
import json
import os
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--models", nargs="+", default=["v3", "256-13", "1024-1024-64", "521"])
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--chunks", type=int, default=60)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
os.environ.setdefault("BUZZDETECT_SYNTHETIC_WEIGHTS", "1")      # developer tool: timing on the seeded stand-in weights

import numpy as np   # noqa: E402
import torch   # noqa: E402

from buzzdetect_amd.engine import HipEngine, hop_samples, patch_step   # noqa: E402

F32_MATRIX_PEAK = 157.3e12
dev = torch.device("cuda", 0)
hop, step = hop_samples(0.96), patch_step(0.96)
g = torch.Generator(device="cpu").manual_seed(11)
pcm = (torch.randn(1024 * hop + 240, generator=g) * 0.1).to(dev)


def engine_for(spec: str, root: str):
    if spec == "v3":
        return HipEngine(device=0), 1024 * 13
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import modelgen
    widths = [int(w) for w in spec.split("-")]
    layers = modelgen.glorot_layers(widths, ["relu"] * (len(widths) - 1) + ["linear"], seed=1)
    modelgen.write_model_dir(os.path.join(root, "model_" + spec), layers)
    macs = sum(k.shape[0] * k.shape[1] for k, _, _ in layers)
    return HipEngine(modelname="model_" + spec, models_dir=root, device=0), macs


def loop(eng, out, n):
    for _ in range(n):
        eng.launch([pcm], hop, step, False, True, out=out)


with tempfile.TemporaryDirectory() as root:
    for spec in args.models:
        eng, macs = engine_for(spec, root)
        out = torch.empty((1024, eng.n_classes), device=dev)
        loop(eng, out, 10)
        torch.cuda.synchronize()
        digest = hashlib.sha256(np.ascontiguousarray(out.cpu().numpy()).tobytes()).hexdigest()[:16]
        rates = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            loop(eng, out, args.chunks)
            torch.cuda.synchronize()
            rates.append(args.chunks * 1024 / (time.perf_counter() - t0))
        eng.profile_enable(True)
        loop(eng, out, 20)
        torch.cuda.synchronize()
        ms, launches = eng.profile_read()
        eng.profile_enable(False)
        head_us = 1e3 * ms[28] / 20
        pass_us = 1e3 * ms[1:].sum() / 20
        print(json.dumps({"model": spec, "tree": os.path.abspath(args.tree), "digest": digest,
                          "windows_per_s": [round(r) for r in rates], "head_us_per_pass": round(head_us, 2),
                          "head_launches_per_pass": int(launches[28]) // 20, "cnn_and_head_us_per_pass": round(pass_us, 1),
                          "head_share": round(head_us / pass_us, 4), "head_mflop_per_window": round(2e-6 * macs, 3),
                          "head_fraction_of_f32_matrix_peak": round(2.0 * macs * 1024 / (head_us * 1e-6) / F32_MATRIX_PEAK, 4)}),
              flush=True)
        eng.close()
