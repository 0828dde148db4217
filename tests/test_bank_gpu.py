"""The bank of one-layer heads on the GPU (include/buzzdetect_bank.h, csrc/headbank.hip, buzzdetect_amd/train.py: TrainerBank,
fit_heads, cross_validate_head).

The yardstick is the lone trainer: member m of a bank equals, bit for bit, the ``Trainer`` that got the same calls with row m of
the weights (both run csrc/headtrain_device.h).  One member is also held against the float64 restatement
(tests/train_oracle_weighted.py) under train_oracle.bound: |gpu - f64| <= 8 x |f32 - f64|.

Shapes: C = 2, 13, 32, 33, 64 outputs give 32, 4, 2, 1 and 1 members per group of 64 columns - 13 crosses a 32-column tile
inside a member, 32 fills two tiles exactly, 33 leaves a partial second tile; M = 1, 5, 9 members: a lone one, and last groups
partly filled; B = 1, 255, 257, 513 rows: below, at the edge of and past a 256-row slice, and three slices."""
import numpy as np
import pytest

from buzzdetect_amd import _lib, train
from tests import train_oracle as T
from tests import train_oracle_weighted as TW

pytestmark = pytest.mark.gpu

N_ROWS = 1024
MAX_BATCH = 768                         # three slices
WIDTHS, MEMBERS, BATCHES = (2, 13, 32, 33, 64), (1, 5, 9), (1, 255, 257, 513)
WEIGHTS = np.array([0.0, 0.25, 1.0, 50.0], dtype=np.float32)


def covering_cases():
    """40 of the 60 (C, M, B), with rows gathered or not, the loss, the optimizer and the weights cycling at periods that share no
    factor with the walk: the assertions below say what the subset covers."""
    cases, i = [], 0
    for ci, c in enumerate(WIDTHS):
        for mi, m in enumerate(MEMBERS):
            for bi, b in enumerate(BATCHES):
                i += 1
                if (ci + mi + bi) % 3 == 2:
                    continue
                n = len(cases)
                cases.append((c, m, b, n % 2 == 0, ("categorical", "binary")[n // 2 % 2], ("sgd", "adam")[(n // 4 + ci) % 2],
                              n % 5 not in (1, 4)))
    return cases


CASES = covering_cases()
assert len(CASES) == 40
for column, values in ((0, WIDTHS), (1, MEMBERS), (2, BATCHES)):
    for value in values:                # every C, M and B meets both ways of naming rows, both losses, both optimizers, weights or none
        for flag in (3, 4, 5, 6):
            assert len({case[flag] for case in CASES if case[column] == value}) == 2, (column, value, flag)
assert {(c, m) for c, m, *_ in CASES} == {(c, m) for c in WIDTHS for m in MEMBERS}
assert {(c, b) for c, _, b, *_ in CASES} == {(c, b) for c in WIDTHS for b in BATCHES}


@pytest.fixture(scope="module")
def data():
    import torch
    rng = np.random.default_rng(2025)
    x = (np.maximum(rng.normal(size=(N_ROWS, 1024)), 0) * 0.5).astype(np.float32)
    return x, torch.from_numpy(x).cuda()


def make_member(c, seed):
    rng = np.random.default_rng(seed)
    k, b, _ = train.glorot_layers(rng, [c], ["linear"])[0]
    return k, rng.uniform(-0.1, 0.1, b.shape).astype(np.float32)


def make_targets(rng, n, c, loss):
    if loss == "categorical":
        return rng.integers(0, c, n).astype(np.int32)
    return rng.integers(0, 2, (n, c)).astype(np.float32)


def make_weights(rng, m, n):
    """[m, n] drawn from WEIGHTS; every member's batch of more than one row has a zero and a 50."""
    w = rng.choice(WEIGHTS, (m, n)).astype(np.float32)
    if n > 1:
        for j in range(m):
            w[j, (3 * j) % n], w[j, (3 * j + 1) % n] = 0.0, 50.0
    else:
        w[0, 0] = 0.25                  # the first member's only row counts: its step moves something
    return w


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rate_of(optimizer, member, step=0):
    return (1e-2 if optimizer == "sgd" else 1e-3) * (1 + 0.5 * member) / (1 + step)


def decay_of(member):
    return 0.0 if member % 3 == 0 else 1e-2 * member          # some members decay, each its own; some do not


def make_steps(rng, c, m, batch, gathered, loss, weighted, n_steps=3):
    steps = []
    for _ in range(n_steps):
        rows = rng.permutation(N_ROWS)[:batch].astype(np.int32) if gathered else None
        steps.append((None if rows is None else to_dev(rows), to_dev(make_targets(rng, batch, c, loss)),
                      to_dev(make_weights(rng, m, batch)) if weighted else None))
    return steps


def run_bank(x_dev, members, loss, optimizer, batch, steps, frozen_at=None):
    """Every step: logits and batch losses of the members as they stand, then the step, each member at its own rate and decay,
    the rates changing between the steps with nothing read in between.  ``frozen_at`` = {step: [(member, frozen), ...]}."""
    import torch
    m, c = len(members), members[0][0].shape[1]
    bank = train.TrainerBank(members, loss, optimizer, rate_of(optimizer, 0), max_batch=MAX_BATCH)
    out = {"logits": [], "loss": []}
    try:
        for j in range(m):
            bank.set_weight_decay(j, decay_of(j))
        logits = torch.zeros((batch, m * c), dtype=torch.float32, device="cuda")
        losses = torch.zeros(m, dtype=torch.float32, device="cuda")
        for s, (rows, targets, w) in enumerate(steps):
            for j, frozen in (frozen_at or {}).get(s, ()):
                bank.freeze(j, frozen)
            for j in range(m):
                bank.set_learning_rate(j, rate_of(optimizer, j, s))
            bank.forward_into(x_dev, rows, batch, logits)
            bank.loss_into(x_dev, rows, targets, batch, losses, w)
            bank.step(x_dev, rows, targets, batch, w)
            out["logits"].append(logits.cpu().numpy().reshape(batch, m, c).copy())
            out["loss"].append(losses.cpu().numpy().copy())
        out["mean"] = bank.mean_loss()
        out["params"] = [bank.read(j) for j in range(m)]
        out["grads"] = [bank.gradients(j) for j in range(m)]
    finally:
        bank.close()
    return out


def run_trainer(x_dev, member, j, loss, optimizer, batch, steps, skip=()):
    """The trainer member j stands for: the same calls with row j of the weights; the steps in ``skip`` it does not get."""
    tr = train.Trainer([member + ("linear",)], loss, optimizer, rate_of(optimizer, 0), max_batch=MAX_BATCH)
    out = {"logits": [], "loss": []}
    try:
        tr.set_weight_decay(decay_of(j))
        for s, (rows, targets, w) in enumerate(steps):
            wj = None if w is None else w[j].contiguous()
            tr.set_learning_rate(rate_of(optimizer, j, s))
            out["loss"].append(np.float32(tr.loss_of(x_dev, rows, targets, batch, wj)))
            out["logits"].append(tr.logits(batch))
            if s not in skip:
                tr.step(x_dev, rows, targets, batch, wj)
        out["mean"] = np.float32(tr.mean_loss())
        out["params"], out["grads"] = tr.read(0), tr.gradients(0)
    finally:
        tr.close()
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_member_is_trainer(bank, j, alone, how):
    for s in range(len(alone["loss"])):
        assert same_bits(bank["logits"][s][:, j, :], alone["logits"][s]), f"{how}: logits of member {j}, step {s}"
        assert same_bits(bank["loss"][s][j], alone["loss"][s]), f"{how}: batch loss of member {j}, step {s}"
    assert same_bits(bank["mean"][j], alone["mean"]), f"{how}: running mean loss of member {j}"
    for pair, name in ((0, "kernel"), (1, "bias")):
        assert same_bits(bank["params"][j][pair], alone["params"][pair]), f"{how}: {name} of member {j}"
        assert same_bits(bank["grads"][j][pair], alone["grads"][pair]), f"{how}: {name} gradient of member {j}"


# ---------------------------------------------------------------------------------------------------- 1. bank = M trainers
@pytest.mark.parametrize("c,m,batch,gathered,loss,optimizer,weighted", CASES)
def test_a_member_of_a_bank_is_the_lone_trainer_bit_for_bit(data, c, m, batch, gathered, loss, optimizer, weighted):
    _, x_dev = data
    members = [make_member(c, 100 + j) for j in range(m)]
    steps = make_steps(np.random.default_rng(c * 1000 + m * 10 + batch), c, m, batch, gathered, loss, weighted)
    bank = run_bank(x_dev, members, loss, optimizer, batch, steps)
    how = f"C={c} M={m} B={batch} {'gathered' if gathered else 'rows 0..'} {loss} {optimizer} {'weighted' if weighted else 'plain'}"
    assert np.abs(bank["params"][0][0] - members[0][0]).max() > 1e-6, how        # the steps moved something
    for j in range(m):
        assert_member_is_trainer(bank, j, run_trainer(x_dev, members[j], j, loss, optimizer, batch, steps), how)
    assert all(np.isfinite(g).all() for pair in bank["grads"] for g in pair)


def test_a_members_bits_do_not_depend_on_its_place_or_its_company(data):
    """The same head as member 0 of 1, member 3 of 5 (last of a full group of four) and member 8 of 9 (alone in the last group)."""
    _, x_dev = data
    c, batch, loss = 13, 257, "categorical"
    head = make_member(c, 7)
    results = []
    for m, place in ((1, 0), (5, 3), (9, 8)):
        members = [make_member(c, 200 + j) for j in range(m)]
        members[place] = head
        rng = np.random.default_rng(3)
        rows, targets, w = to_dev(rng.permutation(N_ROWS)[:batch].astype(np.int32)), to_dev(make_targets(rng, batch, c, loss)), \
            make_weights(rng, 1, batch)
        weights = np.ones((m, batch), np.float32)
        weights[place] = w[0]
        bank = train.TrainerBank(members, loss, "adam", 1e-3, max_batch=MAX_BATCH)
        try:
            for _ in range(2):
                bank.step(x_dev, rows, targets, batch, to_dev(weights))
            results.append(bank.read(place) + bank.gradients(place) + (bank.mean_loss()[place],))
        finally:
            bank.close()
    for other in results[1:]:
        assert all(same_bits(a, b) for a, b in zip(results[0], other))


# ---------------------------------------------------------------------------------------------------- 2. frozen, snapshot
@pytest.mark.parametrize("optimizer", ("sgd", "adam"))
def test_a_frozen_member_keeps_its_bits_and_continues_as_a_trainer_that_skipped_the_steps(data, optimizer):
    _, x_dev = data
    c, m, batch, loss = 13, 5, 257, "categorical"
    members = [make_member(c, 300 + j) for j in range(m)]
    steps = make_steps(np.random.default_rng(9), c, m, batch, True, loss, True, n_steps=5)
    # member 1 sits out steps 1 and 2, member 4 (alone in the second group) steps 2 .. 4
    bank = run_bank(x_dev, members, loss, optimizer, batch, steps, frozen_at={1: [(1, True)], 2: [(4, True)], 3: [(1, False)]})
    skipped = {1: (1, 2), 4: (2, 3, 4)}
    for j in range(m):
        assert_member_is_trainer(bank, j, run_trainer(x_dev, members[j], j, loss, optimizer, batch, steps, skipped.get(j, ())),
                                 f"{optimizer}, member {j}")
    import torch
    lone = train.TrainerBank(members, loss, optimizer, 1e-2, max_batch=MAX_BATCH)
    try:
        rows, targets, w = steps[0]
        lone.freeze(2)
        before = [lone.read(j) for j in range(m)]
        lone.step(x_dev, rows, targets, batch, w)
        after = [lone.read(j) for j in range(m)]
        assert same_bits(before[2][0], after[2][0]) and same_bits(before[2][1], after[2][1])
        assert all(not same_bits(before[j][0], after[j][0]) for j in (0, 1, 3, 4))
        assert lone.mean_loss(reset=False)[2] == 0.0 and all(lone.mean_loss(reset=False)[j] > 0 for j in (0, 1, 3, 4))
        losses = torch.zeros(m, dtype=torch.float32, device="cuda")
        lone.loss_into(x_dev, rows, targets, batch, losses, w)
        assert losses.cpu().numpy()[2] > 0                   # a frozen member's loss is still computed
    finally:
        lone.close()


def test_snapshot_and_restore_are_per_member(data):
    _, x_dev = data
    c, m, batch, loss = 13, 5, 255, "binary"
    members = [make_member(c, 400 + j) for j in range(m)]
    (rows, targets, w), = make_steps(np.random.default_rng(10), c, m, batch, False, loss, True, n_steps=1)
    bank = train.TrainerBank(members, loss, "adam", 1e-2, max_batch=MAX_BATCH)
    try:
        with pytest.raises(_lib.BuzzdetectHipError, match="bd_bank_restore: no snapshot of member 3"):
            bank.restore(3)
        bank.step(x_dev, rows, targets, batch, w)
        first = [bank.read(j) for j in range(m)]
        bank.snapshot(1)
        bank.snapshot(4)
        with pytest.raises(_lib.BuzzdetectHipError, match="member 3"):
            bank.restore(3)                                  # its neighbours' snapshots are not its own
        bank.step(x_dev, rows, targets, batch, w)
        second = [bank.read(j) for j in range(m)]
        assert all(not same_bits(first[j][0], second[j][0]) for j in range(m))
        bank.restore(1)
        now = [bank.read(j) for j in range(m)]
        for j in range(m):                                   # member 1 is back, kernel and bias; nobody else moved
            want = first if j == 1 else second
            assert same_bits(now[j][0], want[j][0]) and same_bits(now[j][1], want[j][1]), j
        bank.restore(4)
        assert same_bits(bank.read(4)[0], first[4][0]) and same_bits(bank.read(0)[0], second[0][0])
        with pytest.raises(_lib.BuzzdetectHipError, match="no such member"):
            bank.snapshot(5)
    finally:
        bank.close()


# ---------------------------------------------------------------------------------------------------- 3. nothing outside
@pytest.mark.parametrize("c,m", ((13, 5), (33, 2), (2, 33)))
def test_poisoned_workspace_and_guards_change_nothing_and_stay_intact(data, c, m):
    """A NaN pattern in the dW-partial workspace and around the two outputs: 13 x 5 leaves 12 pad columns in the first group and
    51 in the second, 33 x 2 leaves 31 in each, 2 x 33 fills a group and leaves 62."""
    import torch
    _, x_dev = data
    batch, loss, poison = 257, "categorical", 0x7FC0BEEF
    members = [make_member(c, 500 + j) for j in range(m)]
    (rows, targets, w), = make_steps(np.random.default_rng(11), c, m, batch, True, loss, True, n_steps=1)

    def run(poisoned):
        bank = train.TrainerBank(members, loss, "adam", 1e-3, max_batch=MAX_BATCH)
        try:
            fill = float("nan") if poisoned else 0.0
            logits = torch.full((batch + 4, m * c + 9), fill, dtype=torch.float32, device="cuda")
            losses = torch.full((m + 16,), fill, dtype=torch.float32, device="cuda")
            if poisoned:
                bank.workspace_fill(poison)
                assert (bank.workspace().view(np.uint32) == poison).all()
            bank.step(x_dev, rows, targets, batch, w)
            bank.forward_into(x_dev, rows, batch, logits[2:2 + batch, :m * c])
            bank.loss_into(x_dev, rows, targets, batch, losses[8:8 + m], w)
            bank.step(x_dev, rows, targets, batch, w)
            got = [bank.read(j) + bank.gradients(j) for j in range(m)], bank.mean_loss()
            return got, logits.cpu().numpy(), losses.cpu().numpy(), bank.workspace()
        finally:
            bank.close()

    (clean, clean_mean), clean_logits, clean_losses, _ = run(False)
    (got, mean), logits, losses, ws = run(True)
    assert same_bits(mean, clean_mean) and np.isfinite(mean).all()
    for a, b in zip(got, clean):
        assert all(same_bits(x, y) and np.isfinite(x).all() for x, y in zip(a, b))
    inside = np.zeros(logits.shape, bool)
    inside[2:2 + batch, :m * c] = True
    assert same_bits(logits[inside], clean_logits[inside]) and np.isfinite(logits[inside]).all()
    assert np.isnan(logits[~inside]).all()                   # the guard rows and columns around the logits
    assert same_bits(losses[8:8 + m], clean_losses[8:8 + m]) and np.isnan(losses[:8]).all() and np.isnan(losses[8 + m:]).all()
    # the workspace beyond what two slices of this batch wrote still holds the pattern: the third slice's partials, and the
    # columns past each group's last member
    mpg = 64 // c
    groups = (m + mpg - 1) // mpg
    ws = ws.view(np.uint32).reshape(3, groups, 1025 * 64)
    assert (ws[2] == poison).all()
    for g in range(groups):
        used = 1025 * min(mpg, m - g * mpg) * c
        assert (ws[:2, g, :used] != poison).all() and (ws[:2, g, used:] == poison).all()


# ---------------------------------------------------------------------------------------------------- 4. float64
@pytest.mark.parametrize("loss", ("categorical", "binary"))
def test_a_member_of_a_weighted_bank_matches_the_float64_restatement(data, loss):
    x, x_dev = data
    c, m, batch, j = 13, 5, 257, 3
    members = [make_member(c, 600 + i) for i in range(m)]
    rng = np.random.default_rng(12)
    rows = rng.permutation(N_ROWS)[:batch].astype(np.int32)
    targets, w = make_targets(rng, batch, c, loss), make_weights(rng, m, batch)
    layers = [members[j] + ("linear",)]
    value, ref = TW.gradients(layers, x[rows], targets, loss, w[j])
    value32, f32 = TW.gradients(T.cast_layers(layers, np.float32), x[rows], targets, loss, w[j], np.float32)
    bank = train.TrainerBank(members, loss, "sgd", 1e-30, max_batch=MAX_BATCH)
    try:
        bank.step(x_dev, to_dev(rows), to_dev(targets), batch, to_dev(w))
        got, mean = bank.gradients(j), bank.mean_loss()[j]
    finally:
        bank.close()
    for what, g, r, f in (("dW", got[0], ref[0][0], f32[0][0]), ("db", got[1], ref[0][1], f32[0][1]),
                          ("loss", np.array([mean]), np.array([value]), np.array([value32]))):
        limit, dev = T.bound(f, r)
        err = float(np.abs(np.asarray(g, dtype=np.float64) - r).max())
        print(f"{loss} member {j} {what}: |gpu-f64|={err:.3e} |f32-f64|={dev:.3e} limit={limit:.3e}")
        assert np.isfinite(g).all() and err <= limit, what


# ---------------------------------------------------------------------------------------------------- 5. fit_heads
def same_fit(a, b):
    return all(k.tobytes() == k2.tobytes() and bias.tobytes() == bias2.tobytes() and act == act2
               for (k, bias, act), (k2, bias2, act2) in zip(a.head.layers, b.head.layers)) \
        and len(a.head.layers) == len(b.head.layers) and a.history == b.history \
        and a.best_epoch == b.best_epoch and a.stopped_epoch == b.stopped_epoch


@pytest.mark.parametrize("loss", ("categorical", "binary"))
def test_fit_heads_gives_every_member_the_fit_fit_head_gives_it(loss):
    rng = np.random.default_rng(13)
    n, c = 600, 3
    x = (np.maximum(rng.normal(size=(n + 150, 1024)), 0) * 0.5).astype(np.float32)
    targets = make_targets(rng, n + 150, c, loss)
    shared = dict(classes=["a", "b", "c"], loss=loss, epochs=4, batch_size=256, seed=5)
    validation = (x[n:], targets[n:])
    members = [
        {"learning_rate": [1e-2, 5e-3, 2e-3, 1e-3], "weight_decay": 1e-2},
        {"class_weight": "balanced"} if loss == "categorical" else {"weight_decay": 0.3, "learning_rate": lambda e: 1e-3 / (1 + e)},
        {"sample_weight": rng.choice(WEIGHTS, n), "early_stopping": {"patience": 0}, "learning_rate": 0.3},
        {"early_stopping": {"patience": 2, "min_delta": 1e-4}, "validation_weight": rng.choice(WEIGHTS, 150), "learning_rate": 0.1},
        {"early_stopping": {"patience": 1, "restore_best": False}, "learning_rate": 3e-3},
    ]
    banked = train.fit_heads(x[:n], targets[:n], members=members, validation=validation, **shared)
    assert len(banked) == 5
    for i, member in enumerate(members):
        kw = {k: v for k, v in member.items() if k != "validation_weight"}
        alone = train.fit_head(x[:n], targets[:n], validation=validation + ((member["validation_weight"],) if "validation_weight" in member
                                                                            else ()), **shared, **kw)
        print(f"{loss} member {i}: epochs run {len(alone.history['loss'])}, best {alone.best_epoch}, stopped {alone.stopped_epoch}")
        assert same_fit(banked[i], alone), f"member {i}"
        assert banked[i].head.classes == ["a", "b", "c"] and banked[i].head.layers[0][0].shape == (1024, 3)
    assert len(banked[0].history["loss"]) == 4 and banked[0].best_epoch is None
    assert any(len(fit.history["loss"]) < 4 for fit in banked), "no member stopped early: the test does not see a frozen member"
    assert all(same_fit(a, b) for a, b in zip(banked, train.fit_heads(x[:n], targets[:n], members=members, validation=validation, **shared)))
    # without a validation set the monitored value is the training loss
    plain = train.fit_heads(x[:n], targets[:n], members=members[:3], **shared)
    for i in range(3):
        assert same_fit(plain[i], train.fit_head(x[:n], targets[:n], **shared, **members[i])), f"member {i}, no validation"


# ---------------------------------------------------------------------------------------------------- 6. cross-validation
def test_cross_validate_head_is_the_fits_it_stands_for(tmp_path):
    import torch
    from buzzdetect_amd.engine import HipEngine
    rng = np.random.default_rng(14)
    n, c, folds = 900, 3, 3
    classes = ["ambient", "ins_buzz", "rain"]
    targets = rng.choice(c, n, p=[0.6, 0.25, 0.15]).astype(np.int32)
    x = (np.maximum(rng.normal(size=(n, 1024)), 0) * 0.5).astype(np.float32)
    x[np.arange(n), targets] += 1.0                          # something to learn
    groups = np.array([f"rec_{i}.wav" for i in rng.permutation(n) % 9])
    grid = [{"class_weight": "balanced", "weight_decay": 1e-2}, {"learning_rate": 1e-2, "early_stopping": {"patience": 1}}]
    shared = dict(epochs=3, batch_size=256, seed=6)
    cv = train.cross_validate_head(x, targets, classes, folds=folds, groups=groups, grid=grid, **shared)
    f = cv.fold_of_row
    assert np.array_equal(f, train.build_folds(targets, "categorical", folds, groups, 6))
    assert all(np.unique(f[groups == g]).size == 1 for g in np.unique(groups)) and len(cv.entries) == 2 and cv.grid == grid
    x_dev = torch.from_numpy(x).cuda()
    for g, entry in enumerate(cv.entries):
        members = train.fold_members(targets, classes, "categorical", f, folds, grid[g])
        want = np.empty((n, c), np.float32)
        for k in range(folds):
            kw = {key: v for key, v in members[k].items() if key != "validation_weight"}
            alone = train.fit_head(x, targets, classes, validation=(x, targets, members[k]["validation_weight"]), **shared, **kw)
            assert same_fit(entry.fits[k], alone), f"grid {g}, fold {k}"
            # the held-out rows' logits, from a trainer loaded with the member's head
            tr = train.Trainer(alone.head.layers, max_batch=n)
            try:
                tr.loss_of(x_dev, None, torch.from_numpy(targets).cuda(), n)
                want[f == k] = tr.logits(n)[f == k]
            finally:
                tr.close()
        assert same_bits(entry.oof_logits, want), f"grid {g}"
        for i, name in enumerate(classes):
            assert entry.metrics(name) == train.metrics_table(want[:, i], targets == i)
        best = [fit.history["val_loss"][fit.best_epoch] if fit.best_epoch is not None else min(fit.history["val_loss"]) for fit in entry.fits]
        assert entry.fold_best == best
    assert cv.best == int(np.argmin([np.mean(e.fold_best) for e in cv.entries]))
    # the caller's own folds are taken as they are, and give the same members
    again = train.cross_validate_head(x, targets, classes, fold_of_row=f, grid=grid[1:], **shared)
    assert same_bits(again.entries[0].oof_logits, cv.entries[1].oof_logits) and again.best == 0
    # the final model is the user's own fit on all rows with grid[best]
    final = train.fit_head(x, targets, classes, **shared, **cv.grid[cv.best])
    models = tmp_path / "models"
    train.save_model(str(models / "model_cv"), final, metrics=cv.entries[cv.best].metrics("ins_buzz"))
    eng = HipEngine(modelname="model_cv", models_dir=str(models))
    try:
        assert eng.classes == classes
    finally:
        eng.close()
