"""Time one training epoch of the packaged model's shape on resident embeddings, against torch on the same device.

    python tools/train_bench.py [--rows 1048576] [--batch 4096] [--classes 13] [--weighted]

Both sides: 1024 -> 13, Adam, softmax cross-entropy, one epoch over ``rows`` x 1024 float32 embeddings that already lie in
device memory, the shuffled batch gathered by row number.  Median of 5 epochs after 2 warm-up epochs, timed with HIP events.
Prints one JSON line; ``hbm_share`` is what one read of X per step (rows x 4096 bytes) makes of the 8 TB/s peak.

``--weighted`` times the same epoch with a weight per row (``bd_trainer_step_weighted``) as well, the two kinds of epoch
taking turns (plain, weighted, plain, ...: what drifts on the box drifts under both), and leaves torch out.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12


def timed(fn, warmup=2, reps=5):
    import torch
    times = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(times)), times


def timed_in_turns(fns, warmup=2, reps=5):
    """``timed`` for several epochs that take turns: [(median, times)] in the order of ``fns``."""
    import torch
    times = [[] for _ in fns]
    for i in range(warmup + reps):
        for fn, mine in zip(fns, times):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warmup:
                mine.append(a.elapsed_time(b) * 1e-3)
    return [(float(np.median(t)), t) for t in times]


def main():
    import torch
    from buzzdetect_amd import train
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--classes", type=int, default=13)
    ap.add_argument("--unfused", action="store_true", help="the layer-by-layer route instead of the fused kernel")
    ap.add_argument("--weighted", action="store_true", help="also time the epoch with a weight per row, in turns; no torch")
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn(a.rows, 1024, device="cuda", generator=gen).clamp_(min=0).mul_(0.5)
    labels = torch.randint(0, a.classes, (a.rows,), device="cuda", generator=gen, dtype=torch.int32)
    perm = torch.randperm(a.rows, device="cuda", generator=gen).to(torch.int32)
    layers = train.glorot_layers(np.random.default_rng(0), [a.classes], ["linear"])

    tr = train.Trainer(layers, "categorical", "adam", 1e-3, max_batch=a.batch)
    tr.set_fusion(not a.unfused)

    def ours():
        t_epoch = labels[perm.long()].contiguous()
        for at in range(0, a.rows, a.batch):
            b = min(a.batch, a.rows - at)
            tr.step(X, perm[at:at + b], t_epoch[at:at + b], b)

    if a.weighted:
        w = torch.rand(a.rows, device="cuda", generator=gen) * 4.0

        def ours_weighted():
            idx = perm.long()
            t_epoch, w_epoch = labels[idx].contiguous(), w[idx].contiguous()
            for at in range(0, a.rows, a.batch):
                b = min(a.batch, a.rows - at)
                tr.step(X, perm[at:at + b], t_epoch[at:at + b], b, w_epoch[at:at + b])

        (ours_s, ours_all), (w_s, w_all) = timed_in_turns([ours, ours_weighted])
        tr.close()
        print(json.dumps({"rows": a.rows, "batch": a.batch, "classes": a.classes, "fused": not a.unfused,
                          "epoch_s": ours_s, "epoch_s_all": ours_all, "weighted_epoch_s": w_s, "weighted_epoch_s_all": w_all,
                          "weighted_over_plain": w_s / ours_s, "rows_per_s": a.rows / ours_s,
                          "hbm_share": a.rows * 4096 / ours_s / HBM_PEAK}))
        return
    ours_s, ours_all = timed(ours)
    tr.close()

    model = torch.nn.Linear(1024, a.classes, device="cuda")
    with torch.no_grad():
        model.weight.copy_(torch.from_numpy(layers[0][0].T.copy()))
        model.bias.zero_()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, eps=1e-7)
    loss_fn = torch.nn.CrossEntropyLoss()
    labels64 = labels.long()

    def theirs():
        for at in range(0, a.rows, a.batch):
            rows = perm[at:at + a.batch].long()
            opt.zero_grad(set_to_none=True)
            loss_fn(model(X[rows]), labels64[rows]).backward()
            opt.step()

    torch_s, torch_all = timed(theirs)
    bytes_x = a.rows * 1024 * 4
    print(json.dumps({"rows": a.rows, "batch": a.batch, "classes": a.classes, "fused": not a.unfused,
                      "epoch_s": ours_s, "epoch_s_all": ours_all, "torch_epoch_s": torch_s, "torch_epoch_s_all": torch_all,
                      "speedup_vs_torch": torch_s / ours_s, "rows_per_s": a.rows / ours_s,
                      "hbm_share": bytes_x / ours_s / HBM_PEAK, "torch_hbm_share": bytes_x / torch_s / HBM_PEAK}))


if __name__ == "__main__":
    main()
