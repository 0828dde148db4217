"""The bank of Dense stacks on the GPU (include/buzzdetect_stackbank.h, csrc/stackbank.hip, buzzdetect_amd/train.py:
TrainerStackBank, fit_stacks, cross_validate_stack).

The yardstick is the lone trainer: member m of a bank equals, bit for bit, the ``Trainer`` created from its layers that got the
same calls with row m of the weights (both run csrc/headtrain_device.h).  No tolerance is involved.  One member is also held
against the float64 restatement (tests/train_oracle_weighted.py) under train_oracle.bound: |gpu - f64| <= 8 x |f32 - f64|.

Shapes, the smallest at which each mechanism can still go wrong: (13,) one layer; (70,) one layer past the one-layer bank's 64
columns; (33, 2) a second layer that reduces over K = 33 - a partial group of 32 - with activation rows 64 floats apart;
(64, 13) exactly one 64-column workgroup; (65, 31, 13) three layers with partial tiles on both sides of 32 and 64; (1, 1)
degenerate widths.  M = 1, 5, 65 members: 65 crosses the 64 members of one launch (with the small shapes only).  B = 1, 255,
257, 513 rows: below, at the edge of and past a 256-row slice, and three slices."""
import numpy as np
import pytest

from buzzdetect_amd import _lib, train
from tests import train_oracle as T
from tests import train_oracle_weighted as TW

pytestmark = pytest.mark.gpu

N_ROWS = 1024
MAX_BATCH = 768                         # three slices
SHAPES = ((13,), (70,), (33, 2), (64, 13), (65, 31, 13), (1, 1))
SMALL = ((13,), (33, 2), (1, 1))        # the shapes that 65 members go with
MEMBERS, BATCHES = (1, 5, 65), (1, 255, 257, 513)
WEIGHTS = np.array([0.0, 0.25, 1.0, 50.0], dtype=np.float32)
HIDDEN = ("relu", "tanh", "sigmoid", "linear")


def covering_cases():
    """24 of the 72 (shape, M, B) - every (shape, B), the members cycling - with rows gathered or not, the loss, the optimizer
    and the weights cycling at their own periods: the assertions below say what the subset covers."""
    cases = []
    for si, shape in enumerate(SHAPES):
        for bi, b in enumerate(BATCHES):
            n = len(cases)
            m = MEMBERS[(si + bi) % 3]
            if m == 65 and shape not in SMALL:
                m = MEMBERS[(si + bi + 1) % 3]
            cases.append((shape, m, b, (n + si) % 2 == 0, ("categorical", "binary")[(n // 2 + si) % 2],
                          ("sgd", "adam")[(n // 4 + bi + n // 2) % 2], n % 5 not in (1, 4)))
    return cases


CASES = covering_cases()
assert len(CASES) <= 24
for column, values in ((0, SHAPES), (1, MEMBERS), (2, BATCHES)):
    for value in values:                # every shape, M and B meets both ways of naming rows, both losses, both optimizers, weights or none
        for flag in (3, 4, 5, 6):
            assert len({case[flag] for case in CASES if case[column] == value}) == 2, (column, value, flag)
assert {(s, b) for s, _, b, *_ in CASES} == {(s, b) for s in SHAPES for b in BATCHES}
assert all(s in SMALL for s, m, *_ in CASES if m == 65)


@pytest.fixture(scope="module")
def data():
    import torch
    rng = np.random.default_rng(2025)
    x = (np.maximum(rng.normal(size=(N_ROWS, 1024)), 0) * 0.5).astype(np.float32)
    return x, torch.from_numpy(x).cuda()


def activations_of(shape, turn=0):
    """The hidden layers' activations, cycling through HIDDEN from ``turn`` on; the last layer is linear."""
    return [HIDDEN[(turn + l) % 4] for l in range(len(shape) - 1)] + ["linear"]


def make_member(shape, acts, seed):
    rng = np.random.default_rng(seed)
    return [(k, rng.uniform(-0.1, 0.1, b.shape).astype(np.float32), a) for k, b, a in train.glorot_layers(rng, shape, acts)]


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
    return (1e-2 if optimizer == "sgd" else 1e-3) * (1 + 0.5 * (member % 7)) / (1 + step)


def decay_of(member):
    return 0.0 if member % 3 == 0 else 1e-2 * (member % 11)       # some members decay, each its own; some do not


def make_steps(rng, c, m, batch, gathered, loss, weighted, n_steps=3):
    steps = []
    for _ in range(n_steps):
        rows = rng.permutation(N_ROWS)[:batch].astype(np.int32) if gathered else None
        steps.append((None if rows is None else to_dev(rows), to_dev(make_targets(rng, batch, c, loss)),
                      to_dev(make_weights(rng, m, batch)) if weighted else None))
    return steps


def run_bank(x_dev, members, loss, optimizer, batch, steps, frozen_at=None):
    """Every step: logits and batch losses of the members as they stand, then the step, each member at its own rate and decay.
    The rates change between the enqueued steps and nothing is read before the last one is enqueued.  ``frozen_at`` =
    {step: [(member, frozen), ...]}."""
    import torch
    m, n_layers, c = len(members), len(members[0]), members[0][-1][0].shape[1]
    bank = train.TrainerStackBank(members, loss, optimizer, rate_of(optimizer, 0), max_batch=MAX_BATCH)
    out = {}
    try:
        for j in range(m):
            bank.set_weight_decay(j, decay_of(j))
        logits = torch.zeros((len(steps), batch, m * c), dtype=torch.float32, device="cuda")
        losses = torch.zeros((len(steps), m), dtype=torch.float32, device="cuda")
        for s, (rows, targets, w) in enumerate(steps):
            for j, frozen in (frozen_at or {}).get(s, ()):
                bank.freeze(j, frozen)
            for j in range(m):
                bank.set_learning_rate(j, rate_of(optimizer, j, s))
            bank.forward_into(x_dev, rows, batch, logits[s])
            bank.loss_into(x_dev, rows, targets, batch, losses[s], w)
            bank.step(x_dev, rows, targets, batch, w)
        out["logits"] = logits.cpu().numpy().reshape(len(steps), batch, m, c)
        out["loss"] = losses.cpu().numpy()
        out["mean"] = bank.mean_loss()
        out["params"] = [[bank.read(j, l) for l in range(n_layers)] for j in range(m)]
        out["grads"] = [[bank.gradients(j, l) for l in range(n_layers)] for j in range(m)]
    finally:
        bank.close()
    return out


def run_trainer(x_dev, member, j, loss, optimizer, batch, steps, skip=()):
    """The trainer member j stands for: the same calls with row j of the weights; the steps in ``skip`` it does not get."""
    tr = train.Trainer(member, loss, optimizer, rate_of(optimizer, 0), max_batch=MAX_BATCH)
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
        out["params"] = [tr.read(l) for l in range(len(member))]
        out["grads"] = [tr.gradients(l) for l in range(len(member))]
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
    for l in range(len(alone["params"])):
        for pair, name in ((0, "kernel"), (1, "bias")):
            assert same_bits(bank["params"][j][l][pair], alone["params"][l][pair]), f"{how}: layer {l} {name} of member {j}"
            assert same_bits(bank["grads"][j][l][pair], alone["grads"][l][pair]), f"{how}: layer {l} {name} gradient of member {j}"


# ---------------------------------------------------------------------------------------------------- 1. bank = M trainers
@pytest.mark.parametrize("shape,m,batch,gathered,loss,optimizer,weighted", CASES)
def test_a_member_of_a_stack_bank_is_the_lone_trainer_bit_for_bit(data, shape, m, batch, gathered, loss, optimizer, weighted):
    _, x_dev = data
    acts = activations_of(shape, turn=CASES.index((shape, m, batch, gathered, loss, optimizer, weighted)))
    members = [make_member(shape, acts, 100 + j) for j in range(m)]
    steps = make_steps(np.random.default_rng(sum(shape) * 1000 + m * 10 + batch), shape[-1], m, batch, gathered, loss, weighted)
    bank = run_bank(x_dev, members, loss, optimizer, batch, steps)
    how = f"{shape} {acts} M={m} B={batch} {'gathered' if gathered else 'rows 0..'} {loss} {optimizer} {'weighted' if weighted else 'plain'}"
    if not (shape[-1] == 1 and loss == "categorical"):       # (the softmax of one class has no gradient); the steps moved something
        assert any(np.abs(bank["params"][0][l][p] - members[0][l][p]).max() > 0 for l in range(len(shape)) for p in range(2)), how
    for j in range(m):
        assert_member_is_trainer(bank, j, run_trainer(x_dev, members[j], j, loss, optimizer, batch, steps), how)
    assert all(np.isfinite(g).all() for member in bank["grads"] for pair in member for g in pair)


# ---------------------------------------------------------------------------------------------------- 2. placement
def test_a_members_bits_do_not_depend_on_its_place_or_its_company(data):
    """The same stack as member 0 of 1, member 3 of 5 and member 64 of 65 (the first of the second launch)."""
    _, x_dev = data
    shape, batch, loss = (33, 2), 257, "categorical"
    acts = activations_of(shape, 1)
    stack = make_member(shape, acts, 7)
    results = []
    for m, place in ((1, 0), (5, 3), (65, 64)):
        members = [make_member(shape, acts, 200 + j) for j in range(m)]
        members[place] = stack
        rng = np.random.default_rng(3)
        rows, targets, w = to_dev(rng.permutation(N_ROWS)[:batch].astype(np.int32)), to_dev(make_targets(rng, batch, 2, loss)), \
            make_weights(rng, 1, batch)
        weights = np.ones((m, batch), np.float32)
        weights[place] = w[0]
        bank = train.TrainerStackBank(members, loss, "adam", 1e-3, max_batch=MAX_BATCH)
        try:
            for _ in range(2):
                bank.step(x_dev, rows, targets, batch, to_dev(weights))
            results.append(sum((bank.read(place, l) + bank.gradients(place, l) for l in range(2)), ()) + (bank.mean_loss()[place],))
        finally:
            bank.close()
    assert len(results[0]) == 9
    for other in results[1:]:
        assert all(same_bits(a, b) for a, b in zip(results[0], other))


# ---------------------------------------------------------------------------------------------------- 3. frozen, snapshot
@pytest.mark.parametrize("m,place", ((1, 0), (65, 64)))
def test_a_frozen_member_alone_in_its_launch_skips_the_steps_too(data, m, place):
    """A launch of exactly one member (a bank of one; member 64 of 65) leaves a frozen member's backward launches out on the
    host instead of returning from them: the member still continues as the trainer that skipped those steps."""
    _, x_dev = data
    shape, batch, loss = (33, 2), 257, "categorical"
    acts = activations_of(shape, 2)
    members = [make_member(shape, acts, 400 + j) for j in range(m)]
    steps = make_steps(np.random.default_rng(11), 2, m, batch, True, loss, True, n_steps=4)
    bank = run_bank(x_dev, members, loss, "adam", batch, steps, frozen_at={1: [(place, True)], 3: [(place, False)]})
    assert_member_is_trainer(bank, place, run_trainer(x_dev, members[place], place, loss, "adam", batch, steps, (1, 2)), f"M={m}")
    if m > 1:                                                # its neighbour in the other launch took every step
        assert_member_is_trainer(bank, 0, run_trainer(x_dev, members[0], 0, loss, "adam", batch, steps), f"M={m}, member 0")


@pytest.mark.parametrize("optimizer", ("sgd", "adam"))
def test_a_frozen_member_keeps_every_layer_and_continues_as_a_trainer_that_skipped_the_steps(data, optimizer):
    _, x_dev = data
    shape, m, batch, loss = (33, 2), 5, 257, "categorical"
    acts = activations_of(shape, 0)
    members = [make_member(shape, acts, 300 + j) for j in range(m)]
    steps = make_steps(np.random.default_rng(9), 2, m, batch, True, loss, True, n_steps=5)
    # member 1 sits out steps 1 and 2, member 4 steps 2 .. 4
    bank = run_bank(x_dev, members, loss, optimizer, batch, steps, frozen_at={1: [(1, True)], 2: [(4, True)], 3: [(1, False)]})
    skipped = {1: (1, 2), 4: (2, 3, 4)}
    for j in range(m):
        assert_member_is_trainer(bank, j, run_trainer(x_dev, members[j], j, loss, optimizer, batch, steps, skipped.get(j, ())),
                                 f"{optimizer}, member {j}")
    import torch
    lone = train.TrainerStackBank(members, loss, optimizer, 1e-2, max_batch=MAX_BATCH)
    try:
        rows, targets, w = steps[0]
        lone.freeze(2)
        before = [[lone.read(j, l) for l in range(2)] for j in range(m)]
        lone.step(x_dev, rows, targets, batch, w)
        after = [[lone.read(j, l) for l in range(2)] for j in range(m)]
        for l in range(2):
            assert same_bits(before[2][l][0], after[2][l][0]) and same_bits(before[2][l][1], after[2][l][1])
            assert all(not same_bits(before[j][l][0], after[j][l][0]) for j in (0, 1, 3, 4))
            assert not lone.gradients(2, l)[0].any() and lone.gradients(0, l)[0].any()     # no gradient was written for it
        assert lone.mean_loss(reset=False)[2] == 0.0 and all(lone.mean_loss(reset=False)[j] > 0 for j in (0, 1, 3, 4))
        losses = torch.zeros(m, dtype=torch.float32, device="cuda")
        logits = torch.zeros((batch, m * 2), dtype=torch.float32, device="cuda")
        lone.loss_into(x_dev, rows, targets, batch, losses, w)
        lone.forward_into(x_dev, rows, batch, logits)
        assert losses.cpu().numpy()[2] > 0 and logits.cpu().numpy()[:, 4:6].any()      # a frozen member is still reported
    finally:
        lone.close()


def test_snapshot_and_restore_are_per_member_and_cover_every_layer(data):
    _, x_dev = data
    shape, m, batch, loss = (65, 31, 13), 5, 255, "binary"
    acts = activations_of(shape, 2)
    members = [make_member(shape, acts, 400 + j) for j in range(m)]
    (rows, targets, w), = make_steps(np.random.default_rng(10), 13, m, batch, False, loss, True, n_steps=1)
    bank = train.TrainerStackBank(members, loss, "adam", 1e-2, max_batch=MAX_BATCH)

    def read_all():
        return [[bank.read(j, l) for l in range(3)] for j in range(m)]

    try:
        with pytest.raises(_lib.BuzzdetectHipError, match="BD_EINVAL: bd_stackbank_restore: no snapshot of member 3"):
            bank.restore(3)
        bank.step(x_dev, rows, targets, batch, w)
        first = read_all()
        bank.snapshot(1)
        bank.snapshot(4)
        with pytest.raises(_lib.BuzzdetectHipError, match="member 3"):
            bank.restore(3)                                  # its neighbours' snapshots are not its own
        bank.step(x_dev, rows, targets, batch, w)
        second = read_all()
        assert all(not same_bits(first[j][l][0], second[j][l][0]) for j in range(m) for l in range(3))
        bank.restore(1)
        now = read_all()
        for j in range(m):                                   # member 1 is back, every kernel and bias; nobody else moved
            want = first if j == 1 else second
            assert all(same_bits(now[j][l][p], want[j][l][p]) for l in range(3) for p in range(2)), j
        bank.restore(4)
        assert all(same_bits(bank.read(4, l)[0], first[4][l][0]) and same_bits(bank.read(0, l)[0], second[0][l][0]) for l in range(3))
        with pytest.raises(_lib.BuzzdetectHipError, match="no such member"):
            bank.snapshot(5)
        with pytest.raises(ValueError, match="no layer 3"):
            bank.read(0, 3)
    finally:
        bank.close()


# ---------------------------------------------------------------------------------------------------- 4. nothing outside
@pytest.mark.parametrize("shape,m", (((13,), 5), ((65, 31, 13), 3), ((33, 2), 65)))
def test_poisoned_workspace_and_guards_change_nothing_and_stay_intact(data, shape, m):
    """A NaN pattern in the dW-partial workspace, NaN columns past M C up to ldl and NaN rows past B around forward_into's
    output, NaN words around loss_into's."""
    import torch
    _, x_dev = data
    batch, loss, poison, c = 257, "categorical", 0x7FC00000, shape[-1]
    acts = activations_of(shape, 3)
    members = [make_member(shape, acts, 500 + j) for j in range(m)]
    (rows, targets, w), = make_steps(np.random.default_rng(11), c, m, batch, True, loss, True, n_steps=1)

    def run(poisoned):
        bank = train.TrainerStackBank(members, loss, "adam", 1e-3, max_batch=MAX_BATCH)
        try:
            fill = float("nan") if poisoned else 0.0
            logits = torch.full((batch + 4, m * c + 9), fill, dtype=torch.float32, device="cuda")
            losses = torch.full((m + 16,), fill, dtype=torch.float32, device="cuda")
            if poisoned:
                bank.workspace_fill(poison)
                assert (bank.workspace().view(np.uint32) == poison).all()
            bank.step(x_dev, rows, targets, batch, w)
            bank.forward_into(x_dev, rows, batch, logits[2:2 + batch, :m * c])      # ldl = M C + 9
            bank.loss_into(x_dev, rows, targets, batch, losses[8:8 + m], w)
            bank.step(x_dev, rows, targets, batch, w)
            got = [bank.read(j, l) + bank.gradients(j, l) for j in range(m) for l in range(len(shape))], bank.mean_loss()
            return got, logits.cpu().numpy(), losses.cpu().numpy()
        finally:
            bank.close()

    (clean, clean_mean), clean_logits, clean_losses = run(False)
    (got, mean), logits, losses = run(True)
    (again, again_mean), again_logits, again_losses = run(True)
    assert same_bits(mean, clean_mean) and same_bits(again_mean, mean) and np.isfinite(mean).all()
    for a, b, d in zip(got, clean, again):
        assert all(same_bits(x, y) and same_bits(x, z) and np.isfinite(x).all() for x, y, z in zip(a, b, d))
    inside = np.zeros(logits.shape, bool)
    inside[2:2 + batch, :m * c] = True
    assert same_bits(logits[inside], clean_logits[inside]) and np.isfinite(logits[inside]).all() and logits[inside].any()
    assert np.isnan(logits[~inside]).all()                   # the guard rows and columns around the logits
    assert same_bits(losses[8:8 + m], clean_losses[8:8 + m]) and np.isnan(losses[:8]).all() and np.isnan(losses[8 + m:]).all()
    assert logits.tobytes() == again_logits.tobytes() and losses.tobytes() == again_losses.tobytes()


# ---------------------------------------------------------------------------------------------------- 5. float64
def ratio_of(got, ref, f32, what):
    """Asserts the 8x rule for one array and returns the observed |gpu - f64| / |f32 - f64|."""
    limit, dev = T.bound(f32, ref)
    err = float(np.abs(np.asarray(got, dtype=np.float64) - ref).max())
    ratio = err / dev if dev > 0 else float("inf") if err > 0 else 0.0
    print(f"{what}: |gpu-f64|={err:.3e} |f32-f64|={dev:.3e} ratio={ratio:.2f} limit={limit:.3e}")
    assert np.isfinite(got).all(), what
    assert err <= limit, what
    return ratio


@pytest.mark.parametrize("loss", ("categorical", "binary"))
def test_the_gradients_of_a_member_of_a_weighted_bank_match_the_float64_restatement(data, loss):
    x, x_dev = data
    shape, m, batch, j = (33, 2), 3, 257, 1
    acts = activations_of(shape, 1)                          # tanh
    members = [make_member(shape, acts, 600 + i) for i in range(m)]
    rng = np.random.default_rng(12)
    rows = rng.permutation(N_ROWS)[:batch].astype(np.int32)
    targets, w = make_targets(rng, batch, 2, loss), make_weights(rng, m, batch)
    value, ref = TW.gradients(members[j], x[rows], targets, loss, w[j])
    value32, f32 = TW.gradients(T.cast_layers(members[j], np.float32), x[rows], targets, loss, w[j], np.float32)
    bank = train.TrainerStackBank(members, loss, "sgd", 1e-30, max_batch=MAX_BATCH)
    try:
        bank.step(x_dev, to_dev(rows), to_dev(targets), batch, to_dev(w))
        got, mean = [bank.gradients(j, l) for l in range(2)], bank.mean_loss()[j]
    finally:
        bank.close()
    worst = ratio_of(np.array([mean]), np.array([value]), np.array([value32]), f"{loss} member {j} loss")
    for l in range(2):
        for what, p in (("dW", 0), ("db", 1)):
            worst = max(worst, ratio_of(got[l][p], ref[l][p], f32[l][p], f"{loss} member {j} layer {l} {what}"))
    print(f"worst ratio |gpu-f64| / |f32-f64|: {worst:.2f}")


@pytest.mark.parametrize("optimizer", ("sgd", "adam"))
def test_twenty_decayed_weighted_steps_move_a_member_as_float64_does(data, optimizer):
    """The hidden layer is tanh: the 8x rule measures how far float32 sums of the same terms in another order drift from float64,
    and that is a statement about a smooth function of those sums.  A relu has a kink: with relu, this seed and Adam the float64
    fit itself passes a pre-activation of 6.7e-8 on a row that counts (step 4, unit 32; sgd: 2.2e-6 at step 9) - inside the
    rounding of a 1024-term float32 sum - so whether that row's derivative is 0 or 1 is not a property the reference defines,
    and Adam's normalisation turns the flip into a learning rate's worth of difference (1.9e-3 observed against a 6.2e-6
    limit, with every bit still the lone trainer's).  The relu stacks are held to the lone trainer bit for bit above, and the
    lone trainer to float64 in tests/test_train_weighted_gpu.py."""
    x, x_dev = data
    shape, m, batch, j, loss, wd = (33, 2), 3, 257, 1, "categorical", 1e-2
    acts = activations_of(shape, 1)                          # tanh
    members = [make_member(shape, acts, 700 + i) for i in range(m)]
    rng = np.random.default_rng(31)
    pool_targets, pool_weights = make_targets(rng, N_ROWS, 2, loss), make_weights(rng, m, N_ROWS)
    batches = []
    for _ in range(20):
        rows = rng.permutation(N_ROWS)[:batch].astype(np.int32)
        batches.append((rows, pool_targets[rows], pool_weights[:, rows]))
    lr = 1e-2 if optimizer == "sgd" else 1e-3

    def opt(dtype):
        return TW.SgdW(lr, wd, dtype) if optimizer == "sgd" else TW.AdamW(lr, wd, dtype)

    mine = [(rows, targets, w[j]) for rows, targets, w in batches]
    ref = TW.train(members[j], x, mine, loss, opt(np.float64))
    f32 = TW.train(members[j], x, mine, loss, opt(np.float32), np.float32)
    bank = train.TrainerStackBank(members, loss, optimizer, lr, max_batch=MAX_BATCH)
    try:
        for i in range(m):
            bank.set_weight_decay(i, wd if i == j else 0.0)
        for rows, targets, w in batches:
            bank.step(x_dev, to_dev(rows), to_dev(targets), batch, to_dev(w))
        got = [bank.read(j, l) for l in range(2)]
    finally:
        bank.close()
    worst = 0.0
    for l in range(2):
        for what, p in (("kernel", 0), ("bias", 1)):
            assert float(np.abs(ref[l][p] - members[j][l][p]).max()) > 1e-4         # the fit moved it
            worst = max(worst, ratio_of(got[l][p], ref[l][p], f32[l][p], f"(33, 2) {optimizer} member {j} layer {l} {what}"))
    print(f"worst ratio |gpu-f64| / |f32-f64|: {worst:.2f}")


# ---------------------------------------------------------------------------------------------------- 6. fit_stacks = fit_head
def same_fit(a, b):
    return all(k.tobytes() == k2.tobytes() and bias.tobytes() == bias2.tobytes() and act == act2
               for (k, bias, act), (k2, bias2, act2) in zip(a.head.layers, b.head.layers)) \
        and len(a.head.layers) == len(b.head.layers) and a.history == b.history \
        and a.best_epoch == b.best_epoch and a.stopped_epoch == b.stopped_epoch


def fit_data(loss, c, seed=13, n=600, n_val=150):
    rng = np.random.default_rng(seed)
    x = (np.maximum(rng.normal(size=(n + n_val, 1024)), 0) * 0.5).astype(np.float32)
    targets = make_targets(rng, n + n_val, c, loss)
    members = [
        {"learning_rate": [1e-2, 5e-3, 2e-3, 1e-3], "weight_decay": 1e-2, **({"class_weight": "balanced"} if loss == "categorical" else {})},
        {"sample_weight": np.where(rng.random(n) < 0.3, 0.0, rng.choice(WEIGHTS, n)), "learning_rate": 3e-3},
        {"early_stopping": {"patience": 0}, "learning_rate": 0.3},
        {"early_stopping": {"patience": 2, "min_delta": 1e-4}, "validation_weight": rng.choice(WEIGHTS, n_val), "learning_rate": 0.1},
    ]
    return x[:n], targets[:n], (x[n:], targets[n:]), members


@pytest.mark.parametrize("loss", ("categorical", "binary"))
def test_fit_stacks_gives_every_member_the_fit_fit_head_gives_it(loss):
    x, targets, validation, members = fit_data(loss, 3)
    shared = dict(classes=["a", "b", "c"], hidden=(16,), activations=("relu",), loss=loss, epochs=4, batch_size=256, seed=5)
    banked = train.fit_stacks(x, targets, members=members, validation=validation, **shared)
    assert len(banked) == 4
    for i, member in enumerate(members):
        kw = {k: v for k, v in member.items() if k != "validation_weight"}
        alone = train.fit_head(x, targets, validation=validation + ((member["validation_weight"],) if "validation_weight" in member else ()),
                               **shared, **kw)
        print(f"{loss} member {i}: epochs run {len(alone.history['loss'])}, best {alone.best_epoch}, stopped {alone.stopped_epoch}")
        assert same_fit(banked[i], alone), f"member {i}"
        assert banked[i].head.classes == ["a", "b", "c"]
        assert [(k.shape, a) for k, _, a in banked[i].head.layers] == [((1024, 16), "relu"), ((16, 3), "linear")]
    assert len(banked[0].history["loss"]) == 4 and banked[0].best_epoch is None
    assert any(len(fit.history["loss"]) < 4 for fit in banked), "no member stopped early: the test does not see a frozen member"
    assert all(same_fit(a, b) for a, b in zip(banked, train.fit_stacks(x, targets, members=members, validation=validation, **shared)))


# ---------------------------------------------------------------------------------------------------- 7. fit_stacks = fit_heads
@pytest.mark.parametrize("loss", ("categorical", "binary"))
def test_fit_stacks_without_hidden_layers_gives_the_one_layer_banks_bits(loss):
    classes = [f"class_{i}" for i in range(13)]
    x, targets, validation, members = fit_data(loss, 13, seed=15)
    shared = dict(classes=classes, loss=loss, epochs=4, batch_size=256, seed=5, validation=validation)
    stacks, heads = train.fit_stacks(x, targets, members=members, **shared), train.fit_heads(x, targets, members=members, **shared)
    assert len(stacks) == len(heads) == 4
    for i, (a, b) in enumerate(zip(stacks, heads)):
        assert same_fit(a, b) and a.head.layers[0][0].shape == (1024, 13), f"member {i}"


# ---------------------------------------------------------------------------------------------------- 8. cross-validation
def test_cross_validate_stack_is_the_fits_it_stands_for(tmp_path):
    import torch
    from buzzdetect_amd import results, weights
    from buzzdetect_amd.engine import HipEngine
    rng = np.random.default_rng(14)
    n, c, folds = 900, 3, 3
    classes = ["ambient", "ins_buzz", "rain"]
    targets = rng.choice(c, n, p=[0.6, 0.25, 0.15]).astype(np.int32)
    x = (np.maximum(rng.normal(size=(n, 1024)), 0) * 0.5).astype(np.float32)
    x[np.arange(n), targets] += 1.0                          # something to learn
    groups = np.array([f"rec_{i}.wav" for i in rng.permutation(n) % 9])
    grid = [{"class_weight": "balanced", "weight_decay": 1e-2}, {"learning_rate": 1e-2, "early_stopping": {"patience": 1}}]
    shape = dict(hidden=(16,), activations=("relu",))
    shared = dict(epochs=3, batch_size=256, seed=6)
    cv = train.cross_validate_stack(x, targets, classes, folds=folds, groups=groups, grid=grid, **shape, **shared)
    f = cv.fold_of_row
    assert np.array_equal(f, train.build_folds(targets, "categorical", folds, groups, 6))
    assert all(np.unique(f[groups == g]).size == 1 for g in np.unique(groups)) and len(cv.entries) == 2 and cv.grid == grid
    x_dev, t_dev = torch.from_numpy(x).cuda(), torch.from_numpy(targets).cuda()
    for g, entry in enumerate(cv.entries):
        members = train.fold_members(targets, classes, "categorical", f, folds, grid[g])
        want = np.empty((n, c), np.float32)
        for k in range(folds):
            kw = {key: v for key, v in members[k].items() if key != "validation_weight"}
            alone = train.fit_head(x, targets, classes, validation=(x, targets, members[k]["validation_weight"]), **shape, **shared, **kw)
            assert same_fit(entry.fits[k], alone) and len(alone.head.layers) == 2, f"grid {g}, fold {k}"
            tr = train.Trainer(alone.head.layers, max_batch=n)         # the held-out rows' logits, from a lone trainer
            try:
                tr.loss_of(x_dev, None, t_dev, n)
                want[f == k] = tr.logits(n)[f == k]
            finally:
                tr.close()
        assert same_bits(entry.oof_logits, want), f"grid {g}"
        for i, name in enumerate(classes):
            assert entry.metrics(name) == train.metrics_table(want[:, i], targets == i)
        best = [fit.history["val_loss"][fit.best_epoch] if fit.best_epoch is not None else min(fit.history["val_loss"]) for fit in entry.fits]
        assert entry.fold_best == best
    assert cv.best == int(np.argmin([np.mean(e.fold_best) for e in cv.entries]))
    # the table of the out-of-fold logits parses where analyze looks for a threshold
    metrics = tmp_path / "metrics.csv"
    metrics.write_text(cv.entries[cv.best].metrics("ins_buzz"))
    assert np.isfinite(results.threshold_for_precision("model_cv", 0.5, tolerance=2.0, metrics_path=str(metrics)))     # every row
    # the final model is the user's own fit on all rows with grid[best] and the shape; the engine loads what was saved
    final = train.fit_head(x, targets, classes, **shape, **shared, **cv.grid[cv.best])
    models = tmp_path / "models"
    train.save_model(str(models / "model_cv"), final, metrics=cv.entries[cv.best].metrics("ins_buzz"))
    loaded = weights.load_head("model_cv", models_dir=str(models))
    assert len(loaded.layers) == 2 and all(k.tobytes() == k2.tobytes() and b.tobytes() == b2.tobytes() and a == a2
                                           for (k, b, a), (k2, b2, a2) in zip(loaded.layers, final.head.layers))
    eng = HipEngine(modelname="model_cv", models_dir=str(models))
    try:
        assert eng.classes == classes
    finally:
        eng.close()
