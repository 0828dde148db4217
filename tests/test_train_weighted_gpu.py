"""Row weights, decoupled weight decay, snapshots and early stopping of the head trainer on the GPU (include/buzzdetect_train.h,
csrc/headtrain.hip, buzzdetect_amd/train.py) against the restatement in tests/train_oracle_weighted.py.

Bound, as in tests/test_train_gpu.py: |gpu - f64| <= 8 x |f32 - f64| with the float32 restatement's deviation counted as at
least 1e-7 x max|f64| (train_oracle.bound).  Every such case prints its ratio |gpu - f64| / |f32 - f64|.  What must not move
at all - the unweighted route, the two routes of a one-layer stack, a restored snapshot, the same call twice - is compared
bit for bit.

Shapes: batches 1, 33, 257 and 513 cross the 32-row tile and the 256-row slice (one, two and three slices); 13 outputs take the
fused kernel, 64 is its limit, 70 is wider and leaves a ragged last column tile.  Data as in test_train_gpu.py."""
import numpy as np
import pytest

from buzzdetect_amd import _lib, train
from tests import train_oracle as T
from tests import train_oracle_weighted as TW

pytestmark = pytest.mark.gpu

N_ROWS = 1024
MAX_BATCH = 768                         # three slices
BATCHES = (1, 33, 257, 513)
STACKS = {
    "13": ([13], ["linear"], True),
    "13-unfused": ([13], ["linear"], False),
    "64relu-13": ([64, 13], ["relu", "linear"], True),
    "70": ([70], ["linear"], True),
}
LOSSES = ("categorical", "binary")
WEIGHTS = np.array([0.0, 0.25, 1.0, 50.0], dtype=np.float32)


@pytest.fixture(scope="module")
def data():
    import torch
    rng = np.random.default_rng(2025)
    x = (np.maximum(rng.normal(size=(N_ROWS, 1024)), 0) * 0.5).astype(np.float32)
    return x, torch.from_numpy(x).cuda()


def make_layers(widths, acts, seed):
    rng = np.random.default_rng(seed)
    layers = train.glorot_layers(rng, widths, acts)
    return [(k, rng.uniform(-0.1, 0.1, b.shape).astype(np.float32), a) for k, b, a in layers]


def make_targets(rng, n, c, loss):
    if loss == "categorical":
        return rng.integers(0, c, n).astype(np.int32)
    return rng.integers(0, 2, (n, c)).astype(np.float32)


def make_weights(rng, n, values=WEIGHTS):
    """Drawn from ``values``; a batch of more than one row has at least one of the smallest (0) and one of the largest."""
    w = rng.choice(values, n).astype(np.float32)
    if n > 1:
        w[0], w[-1] = values[0], values[-1]
    return w


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ratio_of(got, ref, f32, what):
    """Asserts the 8x rule for one array and returns the observed |gpu - f64| / |f32 - f64|."""
    limit, dev = T.bound(f32, ref)
    err = float(np.abs(np.asarray(got, dtype=np.float64) - ref).max())
    ratio = err / dev if dev > 0 else float("inf") if err > 0 else 0.0
    print(f"{what}: |gpu-f64|={err:.3e} |f32-f64|={dev:.3e} ratio={ratio:.2f} max|f64|={np.abs(ref).max():.3e} limit={limit:.3e}")
    assert np.isfinite(got).all(), what
    assert err <= limit, what
    return ratio


def bits(tr, n_layers):
    """Parameters and gradients of every layer, as bytes."""
    return [a.tobytes() for l in range(n_layers) for a in tr.read(l) + tr.gradients(l)]


# ---------------------------------------------------------------------------------------------------- 1. nothing moved
def step_through_the_weighted_entry_with_null(tr, X, rows, targets, B):
    x, ldx, r, t, b, stream = tr._batch(X, rows, targets, B)
    _lib.check(tr._lib.bd_trainer_step_weighted(tr._handle, x, ldx, r, t, None, b, stream))


@pytest.mark.parametrize("optimizer", ("sgd", "adam"))
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", ("13", "64relu-13", "70"))
def test_the_unweighted_step_keeps_its_bits_through_every_new_door(data, name, loss, optimizer):
    _, x_dev = data
    widths, acts, _ = STACKS[name]
    layers = make_layers(widths, acts, seed=7)
    lr = 1e-2 if optimizer == "sgd" else 1e-3
    rng = np.random.default_rng(17)
    batches = []
    for batch in (257, 33, 513):
        rows = rng.permutation(N_ROWS)[:batch].astype(np.int32)
        batches.append((batch, to_dev(rows), to_dev(make_targets(rng, batch, widths[-1], loss))))

    def run(how):
        tr = train.Trainer(layers, loss, optimizer, lr, max_batch=MAX_BATCH)
        try:
            if how == "decay 0":
                tr.set_weight_decay(0.0)
            if how == "same rate":
                tr.set_learning_rate(lr)
            for batch, rows, targets in batches:
                if how == "null":
                    step_through_the_weighted_entry_with_null(tr, x_dev, rows, targets, batch)
                elif how == "ones":
                    tr.step(x_dev, rows, targets, batch, to_dev(np.ones(batch, dtype=np.float32)))
                else:
                    tr.step(x_dev, rows, targets, batch)
            return bits(tr, len(layers)) + [np.float32(tr.mean_loss()).tobytes()]
        finally:
            tr.close()

    plain = run("plain")
    assert np.abs(np.frombuffer(plain[0], np.float32) - layers[0][0].ravel()).max() > 1e-5
    for how in ("null", "ones", "decay 0", "same rate"):
        assert run(how) == plain, how


def fit_arguments(loss, n=700):
    rng = np.random.default_rng(12)
    x = (np.maximum(rng.normal(size=(n, 1024)), 0) * 0.5).astype(np.float32)
    targets = make_targets(rng, n, 13, loss)
    return dict(embeddings=x, targets=targets, classes=[f"c{i}" for i in range(13)], loss=loss, epochs=2, batch_size=300, seed=4,
                validation=(x[:100], targets[:100]))


def same_head(a, b):
    return all(k.tobytes() == k2.tobytes() and bias.tobytes() == bias2.tobytes()
               for (k, bias, _), (k2, bias2, _) in zip(a.head.layers, b.head.layers)) and len(a.head.layers) == len(b.head.layers)


@pytest.mark.parametrize("loss", LOSSES)
def test_fit_head_with_the_new_arguments_at_their_defaults_is_todays_fit(loss):
    a = train.fit_head(**fit_arguments(loss))
    b = train.fit_head(**fit_arguments(loss))
    c = train.fit_head(sample_weight=None, class_weight=None, weight_decay=0.0, early_stopping=None, learning_rate=1e-3,
                       **fit_arguments(loss))
    assert same_head(a, b) and same_head(a, c) and a.history == b.history == c.history
    assert a.best_epoch is None and a.stopped_epoch is None and len(a.history["loss"]) == 2
    # and it is the fit the restatement makes without weights (test_train_gpu.py's check, on the history's last entry)
    rng = np.random.default_rng(4)
    layers = train.glorot_layers(rng, [13], ["linear"])
    args, opt = fit_arguments(loss), T.Adam()
    for _ in range(2):
        perm, total = rng.permutation(700), 0.0
        for at in range(0, 700, 300):
            rows = perm[at:at + 300]
            value, grads = T.gradients(layers, args["embeddings"][rows], args["targets"][rows], loss)
            total += value * len(rows)
            layers = opt.apply(T.cast_layers(layers, np.float64), grads)
    assert abs(a.history["loss"][1] - total / 700) <= 1e-5 * total / 700
    # weights of one through fit_head: the weighted kernels, the same bits
    d = train.fit_head(sample_weight=np.ones(700), **fit_arguments(loss))
    assert same_head(a, d) and a.history == d.history


# ---------------------------------------------------------------------------------------------------- 2. one step
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", sorted(STACKS))
def test_weighted_gradients_of_one_step_match_float64(data, name, loss, batch):
    """Two steps at learning rate 1e-30 (the parameters do not move): the second step's gradients, the running mean loss of
    the two, and the batch loss of the forward-only call, per way of naming the rows."""
    x, x_dev = data
    widths, acts, fused = STACKS[name]
    layers = make_layers(widths, acts, seed=7)
    f32_layers = T.cast_layers(layers, np.float32)
    rng = np.random.default_rng(batch)
    targets = make_targets(rng, batch, widths[-1], loss)
    w, w_first = make_weights(rng, batch), make_weights(rng, batch)[::-1].copy()
    perm = rng.permutation(N_ROWS)[:batch].astype(np.int32)
    if batch > 1:
        perm[-1] = perm[0]                                   # a repeated row, under two different weights
        assert (w == 0).any() and (w == 50).any()
    worst = 0.0
    for rows in (None, perm):
        xb = x[:batch] if rows is None else x[rows]
        how = f"{name} {loss} B={batch} rows={'perm' if rows is not None else 'none'}"
        value, ref = TW.gradients(layers, xb, targets, loss, w)
        value32, f32 = TW.gradients(f32_layers, xb, targets, loss, w, np.float32)
        first = TW.mean_loss(layers, xb, targets, loss, w_first)
        first32 = TW.mean_loss(f32_layers, xb, targets, loss, w_first, np.float32)
        tr = train.Trainer(layers, loss, "sgd", 1e-30, max_batch=MAX_BATCH)
        try:
            tr.set_fusion(fused)
            r_dev, t_dev, w_dev = None if rows is None else to_dev(rows), to_dev(targets), to_dev(w)
            tr.step(x_dev, r_dev, t_dev, batch, to_dev(w_first))
            tr.step(x_dev, r_dev, t_dev, batch, w_dev)
            got = [tr.gradients(l) for l in range(len(layers))]
            mean = tr.mean_loss()
            alone = tr.loss_of(x_dev, r_dev, t_dev, batch, w_dev)
        finally:
            tr.close()
        for l, (g, r, f) in enumerate(zip(got, ref, f32)):
            for what, j in (("dW", 0), ("db", 1)):
                assert f[j].dtype == np.float32 and g[j].shape == r[j].shape
                worst = max(worst, ratio_of(g[j], r[j], f[j], f"{how} layer {l} {what}"))
        worst = max(worst, ratio_of(np.float32(alone), np.float64(value), value32, f"{how} batch loss"))
        worst = max(worst, ratio_of(np.float32(mean), np.float64((first + value) / 2),
                                    (np.float64(first32) + np.float64(value32)) / 2, f"{how} mean loss of two steps"))
    print(f"worst ratio |gpu-f64| / |f32-f64|: {worst:.2f}")


# ---------------------------------------------------------------------------------------------------- 3. the two routes
@pytest.mark.parametrize("batch", (257, 513))
@pytest.mark.parametrize("width", (13, 64))
@pytest.mark.parametrize("loss", LOSSES)
def test_the_fused_kernel_gives_the_layer_by_layer_bits_with_weights(data, loss, width, batch):
    _, x_dev = data
    layers = make_layers([width], ["linear"], seed=3)
    out = {}
    for fused in (True, False):
        rng = np.random.default_rng(5)
        tr = train.Trainer(layers, loss, "adam", 1e-3, max_batch=MAX_BATCH)
        try:
            tr.set_fusion(fused)
            tr.set_weight_decay(1e-2)
            for _ in range(3):
                rows = rng.permutation(N_ROWS)[:batch].astype(np.int32)
                tr.step(x_dev, to_dev(rows), to_dev(make_targets(rng, batch, width, loss)), batch, to_dev(make_weights(rng, batch)))
            out[fused] = bits(tr, 1) + [tr.logits(batch).tobytes(), np.float32(tr.mean_loss()).tobytes()]
            moved = float(np.abs(tr.read(0)[0] - layers[0][0]).max())
        finally:
            tr.close()
    assert out[True] == out[False]
    assert moved > 1e-4


# ---------------------------------------------------------------------------------------------------- 4. weight zero
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", ("13", "13-unfused", "64relu-13"))
def test_rows_of_weight_zero_contribute_exactly_nothing_and_the_decay_skips_biases(data, name, loss):
    _, x_dev = data
    widths, acts, fused = STACKS[name]
    layers = make_layers(widths, acts, seed=11)
    lr, wd, batch = 1e-2, 0.37, 257
    rng = np.random.default_rng(3)
    tr = train.Trainer(layers, loss, "sgd", lr, max_batch=MAX_BATCH)
    try:
        tr.set_fusion(fused)
        tr.set_weight_decay(wd)
        tr.step(x_dev, to_dev(rng.permutation(N_ROWS)[:batch].astype(np.int32)), to_dev(make_targets(rng, batch, 13, loss)), batch,
                to_dev(np.zeros(batch, dtype=np.float32)))
        got = [(tr.read(l), tr.gradients(l)) for l in range(len(layers))]
        mean = tr.mean_loss()
    finally:
        tr.close()
    decay = np.float32(lr) * np.float32(wd)                  # one float32 product
    assert mean == 0.0
    for (k0, b0, _), ((k, b), (dk, db)) in zip(layers, got):
        assert not dk.any() and not db.any()                 # every element +0.0 or -0.0
        want = k0 - decay * k0                               # float32: a product, then a difference
        assert want.dtype == np.float32 and k.tobytes() == want.tobytes()
        assert np.abs(k - k0).max() > 1e-5                   # the decay did act
        assert b.tobytes() == b0.tobytes()


# ---------------------------------------------------------------------------------------------------- 5. twenty steps
STEP_WEIGHTS = np.array([0.0, 0.25, 1.0, 4.0], dtype=np.float32)    # mean 1.3: the step stays as long as the unweighted test's


@pytest.mark.parametrize("optimizer", ("sgd", "adam"))
@pytest.mark.parametrize("loss", LOSSES)
def test_twenty_decayed_weighted_steps_move_the_weights_as_float64_does(data, loss, optimizer):
    x, x_dev = data
    widths, acts, _ = STACKS["64relu-13"]
    layers = make_layers(widths, acts, seed=9)
    rng = np.random.default_rng(31)
    pool, batch, wd = N_ROWS, 257, 1e-2
    pool_targets, pool_weights = make_targets(rng, pool, 13, loss), make_weights(rng, pool, STEP_WEIGHTS)
    batches = []
    for _ in range(20):
        rows = rng.permutation(pool)[:batch].astype(np.int32)
        batches.append((rows, pool_targets[rows], pool_weights[rows]))
    lr = 1e-2 if optimizer == "sgd" else 1e-3

    def opt(dtype):
        return TW.SgdW(lr, wd, dtype) if optimizer == "sgd" else TW.AdamW(lr, wd, dtype)

    ref = TW.train(layers, x, batches, loss, opt(np.float64))
    f32 = TW.train(layers, x, batches, loss, opt(np.float32), np.float32)
    undecayed = TW.train(layers, x, batches, loss, TW.SgdW(lr, 0.0) if optimizer == "sgd" else TW.AdamW(lr, 0.0))
    losses_ref = [TW.mean_loss(l, x, pool_targets, loss, pool_weights) for l in (layers, ref)]
    losses_f32 = [TW.mean_loss(T.cast_layers(l, np.float32), x, pool_targets, loss, pool_weights, np.float32) for l in (layers, f32)]
    tr = train.Trainer(layers, loss, optimizer, lr, max_batch=N_ROWS)
    try:
        tr.set_weight_decay(wd)
        t_dev, w_dev = to_dev(pool_targets), to_dev(pool_weights)
        losses = [tr.loss_of(x_dev, None, t_dev, pool, w_dev)]
        for rows, targets, w in batches:
            tr.step(x_dev, to_dev(rows), to_dev(targets), batch, to_dev(w))
        losses.append(tr.loss_of(x_dev, None, t_dev, pool, w_dev))
        got = [tr.read(l) for l in range(len(layers))]
    finally:
        tr.close()
    worst = 0.0
    for l, (g, r, f, start, u) in enumerate(zip(got, ref, f32, layers, undecayed)):
        for what, j in (("kernel", 0), ("bias", 1)):
            moved = float(np.abs(r[j] - start[j]).max())
            print(f"layer {l} {what}: moved={moved:.3e} of which the decay {np.abs(r[j] - u[j]).max():.3e}")
            assert moved > 1e-4
            worst = max(worst, ratio_of(g[j], r[j], f[j], f"64relu-13 {loss} {optimizer} layer {l} {what}"))
        # the decay is in the reference: without it the kernels end further away than the bound allows
        assert np.abs(u[0] - r[0]).max() > 10 * T.bound(f[0], r[0])[0]
    for when, got_loss, r, f in zip(("before", "after"), losses, losses_ref, losses_f32):
        worst = max(worst, ratio_of(np.float32(got_loss), np.float64(r), f, f"64relu-13 {loss} {optimizer} loss {when}"))
    assert losses[1] < losses[0] and losses_ref[1] < losses_ref[0]
    print(f"worst ratio |gpu-f64| / |f32-f64|: {worst:.2f}")


# ---------------------------------------------------------------------------------------------------- 6. snapshots
@pytest.mark.parametrize("optimizer", ("sgd", "adam"))
@pytest.mark.parametrize("name", ("13", "64relu-13"))
def test_restore_brings_back_the_snapshot_bit_for_bit(data, name, optimizer):
    _, x_dev = data
    widths, acts, _ = STACKS[name]
    layers = make_layers(widths, acts, seed=5)
    rng = np.random.default_rng(8)
    batch = 257
    tr = train.Trainer(layers, "categorical", optimizer, 1e-2, max_batch=MAX_BATCH)

    def steps(n):
        for _ in range(n):
            rows = rng.permutation(N_ROWS)[:batch].astype(np.int32)
            tr.step(x_dev, to_dev(rows), to_dev(make_targets(rng, batch, 13, "categorical")), batch, to_dev(make_weights(rng, batch)))

    try:
        steps(2)
        tr.snapshot()
        kept = [tr.read(l) for l in range(len(layers))]
        steps(3)
        later = [tr.read(l) for l in range(len(layers))]
        grads = [tr.gradients(l) for l in range(len(layers))]
        pattern = 0x7FC12345
        tr.workspace_fill(pattern)
        tr.restore()
        back = [tr.read(l) for l in range(len(layers))]
        # what lies beside the parameters and the snapshot on the device: the gradients behind them, the workspace
        assert all(a.tobytes() == b.tobytes() for g, g2 in zip(grads, [tr.gradients(l) for l in range(len(layers))]) for a, b in zip(g, g2))
        assert (tr.workspace().view(np.uint32) == pattern).all()
        steps(1)                                             # and the trainer goes on from there
        after = [tr.read(l) for l in range(len(layers))]
        tr.restore()                                         # the snapshot is still the one taken
        again = [tr.read(l) for l in range(len(layers))]
    finally:
        tr.close()
    for k, l, b, a, g in zip(kept, later, back, after, again):
        for j in range(2):
            assert b[j].tobytes() == k[j].tobytes() and g[j].tobytes() == k[j].tobytes()
            assert l[j].tobytes() != k[j].tobytes() and a[j].tobytes() != k[j].tobytes()


def test_restore_without_a_snapshot_is_an_error_with_a_message():
    tr = train.Trainer(make_layers([13], ["linear"], seed=5), "categorical", "adam", 1e-3, max_batch=64)
    try:
        before = tr.read(0)
        rc = tr._lib.bd_trainer_restore(tr._handle, None)
        assert rc < 0 and b"snapshot" in tr._lib.bd_last_error()
        with pytest.raises(_lib.BuzzdetectHipError, match="snapshot"):
            tr.restore()
        assert tr.read(0)[0].tobytes() == before[0].tobytes()
        for bad, setter in ((-1.0, tr.set_weight_decay), (float("nan"), tr.set_weight_decay), (float("inf"), tr.set_weight_decay),
                            (0.0, tr.set_learning_rate), (-1e-3, tr.set_learning_rate), (float("inf"), tr.set_learning_rate)):
            with pytest.raises(_lib.BuzzdetectHipError):
                setter(bad)
    finally:
        tr.close()


# ---------------------------------------------------------------------------------------------------- 7. early stopping
def two_blobs(seed, n, positives, shift):
    """``n`` rows of the usual embeddings and their labels: a row is of class 1 with probability ``positives`` and then lies
    ``shift`` further along a fixed seeded direction (the rows' own spread along a direction is about 0.3)."""
    rng = np.random.default_rng(seed)
    direction = np.abs(np.random.default_rng(77).normal(size=1024))
    direction /= np.linalg.norm(direction)
    labels = (rng.random(n) < positives).astype(np.int32)
    x = np.maximum(rng.normal(size=(n, 1024)), 0) * 0.5 + shift * labels[:, None] * direction
    return x.astype(np.float32), labels


def stopping_arguments():
    x, labels = two_blobs(40, 512, 0.5, 6.0)
    vx, vlabels = two_blobs(41, 256, 0.5, 6.0)
    # labels swapped: what the fit learns is wrong here, more every epoch (the float64 restatement of this fit: val_loss 1.04,
    # 1.41, 1.89, 2.07, ... while the loss falls 0.70, 0.43, 0.28, 0.18, ...)
    return dict(embeddings=x, targets=labels, classes=["ambient", "ins_buzz"], batch_size=64, seed=2, learning_rate=3e-3,
                validation=(vx, 1 - vlabels))


def test_early_stopping_returns_the_best_epochs_head():
    fit = train.fit_head(epochs=10, early_stopping={"patience": 2}, **stopping_arguments())
    print(f"val_loss {fit.history['val_loss']} best {fit.best_epoch} stopped {fit.stopped_epoch}")
    val = fit.history["val_loss"]
    assert all(b > a for a, b in zip(val, val[1:])), "the validation loss rises from the second epoch on"
    assert fit.best_epoch == 0 and fit.stopped_epoch == fit.best_epoch + 2
    assert len(fit.history["loss"]) == len(val) == fit.stopped_epoch + 1
    best = train.fit_head(epochs=fit.best_epoch + 1, **stopping_arguments())
    assert same_head(fit, best) and best.history["val_loss"] == val[:1] and best.best_epoch is None
    # without restore_best: the head of the epoch it stopped at
    last = train.fit_head(epochs=10, early_stopping={"patience": 2, "restore_best": False}, **stopping_arguments())
    through = train.fit_head(epochs=fit.stopped_epoch + 1, **stopping_arguments())
    assert last.history == fit.history and (last.best_epoch, last.stopped_epoch) == (0, 2)
    assert same_head(last, through) and not same_head(last, fit)


def test_early_stopping_on_the_training_loss_and_with_a_min_delta():
    args = stopping_arguments()
    del args["validation"]
    # the training loss falls every epoch: nothing stops, the last epoch is the best and the head is the plain fit's
    fit = train.fit_head(epochs=4, early_stopping={"patience": 1}, **args)
    plain = train.fit_head(epochs=4, **args)
    loss = fit.history["loss"]
    assert loss == plain.history["loss"] and all(b < a for a, b in zip(loss, loss[1:]))
    assert (fit.best_epoch, fit.stopped_epoch) == (3, 3) and same_head(fit, plain)
    # a min_delta no epoch reaches after the first: best 0, stopped after `patience` more
    fit = train.fit_head(epochs=4, early_stopping={"patience": 1, "min_delta": 10.0}, **args)
    assert (fit.best_epoch, fit.stopped_epoch) == (0, 1) and fit.history["loss"] == loss[:2]
    assert same_head(fit, train.fit_head(epochs=1, **args))


# ---------------------------------------------------------------------------------------------------- 8. class weights
def test_class_weights_are_row_weights_and_a_rate_sequence_is_its_callable():
    rng = np.random.default_rng(14)
    n, classes = 600, ["ambient", "ins_buzz", "mech_plane"]
    labels = rng.choice(3, n, p=(0.8, 0.15, 0.05)).astype(np.int32)
    x = (np.maximum(rng.normal(size=(n, 1024)), 0) * 0.5).astype(np.float32)
    kw = dict(embeddings=x, targets=labels, classes=classes, hidden=(16,), activations=("relu",), epochs=2, batch_size=257, seed=6)
    cw = train.balanced_class_weights(labels, 3)
    word = train.fit_head(class_weight="balanced", **kw)
    named = train.fit_head(class_weight={c: float(w) for c, w in zip(classes, cw)}, **kw)
    listed = train.fit_head(class_weight=list(cw), **kw)
    by_row = train.fit_head(sample_weight=cw[labels], **kw)
    plain = train.fit_head(**kw)
    assert same_head(word, named) and same_head(word, listed) and same_head(word, by_row)
    assert word.history == named.history == listed.history == by_row.history
    assert not same_head(word, plain)
    # the history is the weighted loss per row, as the restatement has it
    rng2 = np.random.default_rng(6)
    layers = train.glorot_layers(rng2, [16, 3], ["relu", "linear"])
    perm = rng2.permutation(n)
    total, opt, w = 0.0, TW.AdamW(), cw.astype(np.float32)[labels]
    for at in range(0, n, 257):
        rows = perm[at:at + 257]
        value, grads = TW.gradients(layers, x[rows], labels[rows], "categorical", w[rows])
        total += value * len(rows)
        layers = opt.apply(T.cast_layers(layers, np.float64), grads)
    print(f"first epoch: weighted loss {word.history['loss'][0]:.8f} restatement {total / n:.8f} unweighted {plain.history['loss'][0]:.8f}")
    assert abs(word.history["loss"][0] - total / n) <= 1e-5 * total / n
    # schedules
    rates = [1e-3, 3e-4]
    seq = train.fit_head(learning_rate=rates, **kw)
    fn = train.fit_head(learning_rate=lambda epoch: rates[epoch], **kw)
    flat = train.fit_head(learning_rate=(1e-3, 1e-3), **kw)
    assert same_head(seq, fn) and seq.history == fn.history
    assert same_head(flat, plain) and not same_head(seq, plain)


# ---------------------------------------------------------------------------------------------------- 9. what it is for
RARE = dict(n=2000, positives=0.05, shift=2.0, epochs=6, batch_size=256, seed=3, learning_rate=1e-3)


def rare_sets():
    return two_blobs(50, RARE["n"], RARE["positives"], RARE["shift"]), two_blobs(51, RARE["n"], RARE["positives"], RARE["shift"])


def oracle_recalls():
    """The float64 restatement's fit of the rare class, without and with balanced weights: recall on the held-out set."""
    (x, labels), (hx, hlabels) = rare_sets()
    out = []
    for balanced in (False, True):
        w = train.balanced_class_weights(labels, 2).astype(np.float32)[labels] if balanced else np.ones(len(labels), np.float32)
        rng = np.random.default_rng(RARE["seed"])
        layers = train.glorot_layers(rng, [2], ["linear"])
        batches = []
        for _ in range(RARE["epochs"]):
            perm = rng.permutation(len(labels))
            batches += [(perm[at:at + 256], labels[perm[at:at + 256]], w[perm[at:at + 256]]) for at in range(0, len(labels), 256)]
        fitted = TW.train(layers, x, batches, "categorical", TW.AdamW(RARE["learning_rate"]))
        z = T.forward(fitted, hx)[-1]
        out.append(float((z[hlabels == 1].argmax(axis=1) == 1).mean()))
    return out


def test_balanced_class_weights_find_the_rare_class():
    # the float64 restatement alone, on the CPU: recall of the held-out positives 0.000 without weights (it says "ambient" to
    # every window), 0.677 with "balanced" (67 of 99); shift 1.5 gives 0.000 / 0.556, shift 2.5 0.000 / 0.828
    (x, labels), (hx, hlabels) = rare_sets()
    ref_plain, ref_balanced = oracle_recalls()
    gap = ref_balanced - ref_plain
    print(f"restatement: recall {ref_plain:.3f} unweighted, {ref_balanced:.3f} balanced (gap {gap:.3f}); "
          f"{int(hlabels.sum())} held-out positives")
    assert gap >= 0.1
    kw = dict(embeddings=x, targets=labels, classes=["ambient", "ins_buzz"], epochs=RARE["epochs"], batch_size=RARE["batch_size"],
              seed=RARE["seed"], learning_rate=RARE["learning_rate"])
    recalls = []
    for class_weight in (None, "balanced"):
        fit = train.fit_head(class_weight=class_weight, **kw)
        tr = train.Trainer(fit.head.layers, "categorical", max_batch=RARE["n"])
        try:
            tr.loss_of(to_dev(hx), None, to_dev(hlabels), RARE["n"])
            z = tr.logits(RARE["n"])
        finally:
            tr.close()
        recalls.append(float((z[hlabels == 1].argmax(axis=1) == 1).mean()))
    print(f"trainer: recall {recalls[0]:.3f} unweighted, {recalls[1]:.3f} balanced")
    assert recalls[1] - recalls[0] >= 0.5 * gap


# ---------------------------------------------------------------------------------------------------- 10. stray writes
@pytest.mark.parametrize("fused", (True, False))
def test_a_weighted_step_writes_nothing_it_does_not_own(fused):
    import torch
    rng = np.random.default_rng(6)
    named, batch = 300, 257
    x = torch.full((320, 1024), float("nan"), dtype=torch.float32).cuda()      # the rows beyond those named: a NaN pattern
    x[:named] = to_dev((np.maximum(rng.normal(size=(named, 1024)), 0) * 0.5).astype(np.float32))
    before = x.cpu().numpy().copy()
    layers = make_layers([13], ["linear"], seed=3)
    rows = rng.integers(0, named, batch).astype(np.int32)
    targets = rng.integers(0, 13, batch).astype(np.int32)
    w = make_weights(rng, batch)
    guarded = torch.full((batch + 64,), float("nan"), dtype=torch.float32).cuda()   # the weights, and a guard region behind them
    guarded[:batch] = to_dev(w)
    guard_before = guarded.cpu().numpy().copy()
    out = []
    for w_dev in (guarded[:batch], to_dev(w)):                                 # with the guard behind, and alone
        tr = train.Trainer(layers, "categorical", "sgd", 1e-2, max_batch=MAX_BATCH)
        try:
            tr.set_fusion(fused)
            tr.set_weight_decay(1e-2)
            pattern = 0x7FC12345                                               # a NaN with a payload no kernel produces
            tr.workspace_fill(pattern)
            tr.step(x, to_dev(rows), to_dev(targets), batch, w_dev)
            ws = tr.workspace()
            dw, db = tr.gradients(0)
            tr.workspace_fill(pattern)
            tr.snapshot()
            tr.restore()
            assert (tr.workspace().view(np.uint32) == pattern).all()          # the copies stay in their buffers
            out.append((tr.read(0), (dw, db), tr.mean_loss()))
        finally:
            tr.close()
        owned = 1024 * 13 + 13                                                 # a slice's dW and db partial; B = 257 is two slices
        assert ws.size == (MAX_BATCH // _lib.TRAIN_SLICE_ROWS) * owned
        assert np.isfinite(ws[:2 * owned]).all() and np.isfinite(dw).all() and np.isfinite(db).all()
        assert (ws[:owned] + ws[owned:2 * owned]).tobytes() == np.concatenate([dw.ravel(), db]).tobytes()
        assert (ws[2 * owned:].view(np.uint32) == pattern).all()
    # nothing behind the weights was read into the results, nothing was written there or into X
    assert all(a.tobytes() == b.tobytes() for i in range(2) for a, b in zip(out[0][i], out[1][i])) and out[0][2] == out[1][2]
    assert np.isfinite(out[0][2])
    assert guarded.cpu().numpy().tobytes() == guard_before.tobytes()
    assert x.cpu().numpy().tobytes() == before.tobytes()


# ---------------------------------------------------------------------------------------------------- 11. same bits
@pytest.mark.parametrize("loss", LOSSES)
def test_a_weighted_decayed_early_stopped_fit_twice_gives_the_same_bits(loss):
    def fit():
        a = fit_arguments(loss)
        rng = np.random.default_rng(1)
        return train.fit_head(sample_weight=make_weights(rng, 700), class_weight="balanced" if loss == "categorical" else None,
                              weight_decay=1e-2, early_stopping={"patience": 1, "min_delta": 1e-3},
                              **{**a, "epochs": 6, "hidden": (40,), "activations": ("tanh",), "learning_rate": [3e-3] * 3 + [1e-3] * 3,
                                 "validation": a["validation"] + (np.linspace(0.0, 2.0, 100),)})
    a, b = fit(), fit()
    print(f"{loss}: history {a.history} best {a.best_epoch} stopped {a.stopped_epoch}")
    assert same_head(a, b) and a.history == b.history and (a.best_epoch, a.stopped_epoch) == (b.best_epoch, b.stopped_epoch)
    assert a.best_epoch is not None and len(a.history["loss"]) == len(a.history["val_loss"]) == a.stopped_epoch + 1
    assert np.isfinite(a.history["loss"]).all() and np.isfinite(a.history["val_loss"]).all()
    start = train.glorot_layers(np.random.default_rng(4), [40, 13], ["tanh", "linear"])
    assert np.abs(a.head.layers[0][0] - start[0][0]).max() > 1e-4
