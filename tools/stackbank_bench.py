"""One epoch of a bank of M Dense stacks against M epochs of the lone trainer run one after another
(buzzdetect_amd.train.TrainerStackBank against buzzdetect_amd.train.Trainer), on the same device in the same process,
alternating.

    python tools/stackbank_bench.py [--rows 16384] [--classes 13] [--hidden 128] [--repeats 5] [--warmup 2]

Random embeddings [rows, 1024], a fresh permutation's batches, row weights for every member (a fold of a cross-validation is row
weights), 1024 -> hidden (relu) -> classes, Adam.  An "epoch" is the steps of one pass over the rows, enqueued back to back and
waited for once - what fit_head and fit_stacks do between two host reads.  The serial side is the yardstick: M trainers, each
stepping through the epoch on its own - the path fit_heads(hidden=...) takes.  Prints one JSON line per (batch, M): the median
milliseconds of both sides over the repeats, their ratio, the ratio's spread over the repeats (each repeat's serial time over
the bank time measured right before it), and the bank's epoch in units of one serial epoch."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--classes", type=int, default=13)
    ap.add_argument("--hidden", type=int, nargs="*", default=[128])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--members", type=int, nargs="+", default=[1, 5, 20])
    args = ap.parse_args()
    import torch
    from buzzdetect_amd import train
    rng = np.random.default_rng(0)
    n, c = args.rows, args.classes
    X = torch.from_numpy((np.maximum(rng.normal(size=(n, 1024)), 0) * 0.5).astype(np.float32)).cuda()
    perm = torch.from_numpy(rng.permutation(n).astype(np.int32)).cuda()
    T = torch.from_numpy(rng.integers(0, c, n).astype(np.int32)).cuda()
    widths = list(args.hidden) + [c]
    layers = train.glorot_layers(rng, widths, ["relu"] * len(args.hidden) + ["linear"])

    def epoch(step, weights_of):
        for at in range(0, n, batch):
            b = min(batch, n - at)
            step(X, perm[at:at + b], T[at:at + b], b, weights_of(at, b))
        torch.cuda.synchronize()

    for batch in args.batches:
        for m in args.members:
            W = torch.from_numpy(rng.choice(np.array([0.0, 1.0, 1.0, 1.0, 2.0], np.float32), (m, n))).cuda()
            bank = train.TrainerStackBank([layers] * m, "categorical", "adam", 1e-3, max_batch=batch)
            alone = [train.Trainer(layers, "categorical", "adam", 1e-3, max_batch=batch) for _ in range(m)]
            rows_of = [W[j].contiguous() for j in range(m)]
            try:
                def run_bank():
                    epoch(bank.step, lambda at, b: W[:, at:at + b])

                def run_serial():
                    for j, tr in enumerate(alone):
                        epoch(tr.step, lambda at, b: rows_of[j][at:at + b])

                for _ in range(args.warmup):
                    run_bank()
                    run_serial()
                t_bank, t_serial = [], []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    run_bank()
                    t1 = time.perf_counter()
                    run_serial()
                    t2 = time.perf_counter()
                    t_bank.append(t1 - t0)
                    t_serial.append(t2 - t1)
                bank_ms, serial_ms = 1e3 * float(np.median(t_bank)), 1e3 * float(np.median(t_serial))
                ratios = [s / b for s, b in zip(t_serial, t_bank)]
                print(json.dumps({"rows": n, "widths": widths, "batch": batch, "members": m, "steps_per_epoch": -(-n // batch),
                                  "bank_epoch_ms": round(bank_ms, 3), "serial_epochs_ms": round(serial_ms, 3),
                                  "one_serial_epoch_ms": round(serial_ms / m, 3), "serial_over_bank": round(serial_ms / bank_ms, 2),
                                  "serial_over_bank_spread": [round(min(ratios), 2), round(max(ratios), 2)],
                                  "bank_in_serial_epochs": round(bank_ms / (serial_ms / m), 2),
                                  "bank_ms_spread": [round(1e3 * min(t_bank), 3), round(1e3 * max(t_bank), 3)],
                                  "serial_ms_spread": [round(1e3 * min(t_serial), 3), round(1e3 * max(t_serial), 3)]}), flush=True)
            finally:
                bank.close()
                for tr in alone:
                    tr.close()


if __name__ == "__main__":
    main()
