#!/usr/bin/env python3
"""sha256 of what lone trainers leave behind on a fixed grid of cases: run before and after a change of the training route
that must not move a bit (kernel and launch rewrites of the same arithmetic), on the same machine, and compare.

    python tools/train_digest.py [--quiet]

The grid is that of tests/test_stackbank_gpu.py: shapes (13,), (70,), (33, 2), (64, 13), (65, 31, 13) behind 1024 inputs
(hidden layers relu), B = 1, 255, 257, 513, both losses, SGD and Adam, row weights absent and present (present: with a weight
decay too), and for the one shape the fused kernel takes both routes.  Each trainer steps three times on gathered rows; its
parameters and gradients of every layer, the logits of the last step, the batch loss of one more pass and the running mean of
the three steps go into the case's digest (one line each) and all of them into the last line's.
"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SHAPES = ((13,), (70,), (33, 2), (64, 13), (65, 31, 13))
BATCHES = (1, 255, 257, 513)
ROWS, STEPS, FUSED_MAX_WIDTH = 700, 3, 64


def main():
    import torch
    from buzzdetect_amd import train
    quiet = "--quiet" in sys.argv[1:]
    rng = np.random.default_rng(20)
    X = torch.from_numpy((np.maximum(rng.normal(size=(ROWS, 1024)), 0) * 0.5).astype(np.float32)).cuda()
    whole = hashlib.sha256()
    cases = 0
    for shape in SHAPES:
        layers = train.glorot_layers(rng, list(shape), ["relu"] * (len(shape) - 1) + ["linear"])
        layers = [(k, (0.1 * rng.normal(size=k.shape[1])).astype(np.float32), act) for k, _, act in layers]
        fusable = len(shape) == 1 and shape[0] <= FUSED_MAX_WIDTH
        for batch in BATCHES:
            rows = [torch.from_numpy(rng.integers(0, ROWS, batch).astype(np.int32)).cuda() for _ in range(STEPS)]
            labels = [torch.from_numpy(rng.integers(0, shape[-1], batch).astype(np.int32)).cuda() for _ in range(STEPS)]
            multi = [torch.from_numpy((rng.random((batch, shape[-1])) < 0.3).astype(np.float32)).cuda() for _ in range(STEPS)]
            weights = [torch.from_numpy(rng.choice(np.array([0.0, 0.5, 1.0, 3.0], np.float32), batch)).cuda() for _ in range(STEPS)]
            for loss in ("categorical", "binary"):
                targets = labels if loss == "categorical" else multi
                for optimizer in ("sgd", "adam"):
                    for weighted in (False, True):
                        for fused in ((True, False) if fusable else (False,)):
                            tr = train.Trainer(layers, loss, optimizer, 1e-2, max_batch=batch)
                            tr.set_fusion(fused)
                            if weighted:
                                tr.set_weight_decay(0.01)
                            for s in range(STEPS):
                                tr.step(X, rows[s], targets[s], batch, weights[s] if weighted else None)
                            h = hashlib.sha256()
                            for l in range(len(shape)):
                                for a in tr.read(l) + tr.gradients(l):
                                    h.update(np.ascontiguousarray(a).tobytes())
                            h.update(np.ascontiguousarray(tr.logits(batch)).tobytes())
                            batch_loss = tr.loss_of(X, rows[0], targets[0], batch, weights[0] if weighted else None)
                            h.update(np.array([batch_loss, tr.mean_loss()], np.float32).tobytes())
                            tr.close()
                            whole.update(h.digest())
                            cases += 1
                            if not quiet:
                                print("x".join(map(str, shape)), batch, loss, optimizer, "weighted" if weighted else "plain",
                                      "fused" if fused else "layers", h.hexdigest()[:16], flush=True)
    print("all", cases, "cases", whole.hexdigest(), flush=True)


if __name__ == "__main__":
    main()
