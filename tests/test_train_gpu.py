"""The head trainer on the GPU (include/buzzdetect_train.h, csrc/headtrain.hip, buzzdetect_amd/train.py) against the float64
restatement in tests/train_oracle.py.

Bound (gradients, updated weights, losses): |gpu - f64| <= 8 x |f32 - f64|, where f32 is the same restatement run in float32 on
the CPU - both are float32 sums of the same terms in different orders; 8 is the margin for the matrix unit's other
association - and the float32 deviation counts as at least 1e-7 x max|f64|, so that an exactly-zero float32 error does not
demand bit equality (train_oracle.bound).  Every case prints what it observed.

Data: rng.normal embeddings through max(., 0) * 0.5 (real embeddings are non-negative); no audio except in the last test."""
import numpy as np
import pytest

from buzzdetect_amd import _lib, train
from tests import train_oracle as T

pytestmark = pytest.mark.gpu

N_ROWS = 2048
MAX_BATCH = 1536                        # six whole slices
SLICE = _lib.TRAIN_SLICE_ROWS           # 256: batches 257 and 1025 straddle a slice boundary, 33 and 1025 the 32-row tile
BATCHES = (1, 33, 257, 1025, MAX_BATCH)
STACKS = {
    "13": ([13], ["linear"]),
    "1": ([1], ["linear"]),
    "33relu-13": ([33, 13], ["relu", "linear"]),
    "256tanh-64sigmoid-13": ([256, 64, 13], ["tanh", "sigmoid", "linear"]),
}
WIDE = ([2048, 13], ["relu", "linear"])
LOSSES = ("categorical", "binary")


@pytest.fixture(scope="module")
def data():
    import torch
    rng = np.random.default_rng(2024)
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


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_gradients(name, x, x_dev, layers, loss, batch, report):
    """One step at learning rate 1e-30 (the parameters do not move) per way of naming the rows; gradients against float64."""
    rng = np.random.default_rng(batch)
    c = layers[-1][0].shape[1]
    targets = make_targets(rng, batch, c, loss)
    perm = rng.permutation(N_ROWS)[:batch].astype(np.int32)
    if batch > 1:
        perm[-1] = perm[0]                                   # a repeated row
    worst = 0.0
    for rows in (None, perm):
        xb = x[:batch] if rows is None else x[rows]
        _, ref = T.gradients(layers, xb, targets, loss)
        _, f32 = T.gradients(T.cast_layers(layers, np.float32), xb.astype(np.float32), targets, loss, np.float32)
        tr = train.Trainer(layers, loss, "sgd", 1e-30, max_batch=MAX_BATCH)
        try:
            tr.step(x_dev, None if rows is None else to_dev(rows), to_dev(targets), batch)
            got = [tr.gradients(l) for l in range(len(layers))]
        finally:
            tr.close()
        for l, (g, r, f) in enumerate(zip(got, ref, f32)):
            for what, gv, rv, fv in (("dW", g[0], r[0], f[0]), ("db", g[1], r[1], f[1])):
                assert fv.dtype == np.float32 and gv.shape == rv.shape
                limit, dev = T.bound(fv, rv)
                err = float(np.abs(gv.astype(np.float64) - rv).max())
                ratio = err / dev if dev > 0 else float("inf") if err > 0 else 0.0
                report.append((ratio, name))
                print(f"{name} {loss} B={batch} rows={'perm' if rows is not None else 'none'} layer {l} {what}: "
                      f"|gpu-f64|={err:.3e} |f32-f64|={dev:.3e} ratio={ratio:.2f} max|f64|={np.abs(rv).max():.3e} limit={limit:.3e}")
                assert np.isfinite(gv).all()
                assert err <= limit, f"{name} {loss} B={batch} layer {l} {what}"
                worst = max(worst, err / limit if limit > 0 else 0.0)
    return worst


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", sorted(STACKS))
def test_gradients_of_one_step_match_float64(data, name, loss, batch):
    x, x_dev = data
    widths, acts = STACKS[name]
    report = []
    check_gradients(name, x, x_dev, make_layers(widths, acts, seed=7), loss, batch, report)
    print(f"worst ratio |gpu-f64| / |f32-f64|: {max(r for r, _ in report):.2f}")


@pytest.mark.parametrize("loss", LOSSES)
def test_gradients_of_a_wide_hidden_layer(data, loss):
    x, x_dev = data
    report = []
    check_gradients("2048relu-13", x, x_dev, make_layers(*WIDE, seed=7), loss, 33, report)
    print(f"worst ratio |gpu-f64| / |f32-f64|: {max(r for r, _ in report):.2f}")


@pytest.mark.parametrize("optimizer", ("sgd", "adam"))
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", ("13", "33relu-13"))
def test_twenty_steps_move_the_weights_as_float64_does(data, name, loss, optimizer):
    x, x_dev = data
    widths, acts = STACKS[name]
    layers = make_layers(widths, acts, seed=9)
    rng = np.random.default_rng(31)
    pool, batch, c = 1024, 257, widths[-1]
    pool_targets = make_targets(rng, pool, c, loss)
    batches = []
    for _ in range(20):
        rows = rng.permutation(pool)[:batch].astype(np.int32)
        batches.append((rows, pool_targets[rows]))
    lr = 1e-2 if optimizer == "sgd" else 1e-3

    def opt(dtype):
        return T.Sgd(lr, dtype) if optimizer == "sgd" else T.Adam(lr, dtype=dtype)

    ref = T.train(layers, x, batches, loss, opt(np.float64))
    f32 = T.train(layers, x.astype(np.float32), batches, loss, opt(np.float32), np.float32)
    losses_ref = [T.mean_loss(l, x[:pool], pool_targets, loss) for l in (layers, ref)]
    losses_f32 = [T.mean_loss(T.cast_layers(l, np.float32), x[:pool], pool_targets, loss, np.float32)
                  for l in (layers, f32)]
    tr = train.Trainer(layers, loss, optimizer, lr, max_batch=MAX_BATCH)
    try:
        t_dev = to_dev(pool_targets)
        losses = [tr.loss_of(x_dev, None, t_dev, pool)]
        for rows, targets in batches:
            tr.step(x_dev, to_dev(rows), to_dev(targets), batch)
        losses.append(tr.loss_of(x_dev, None, t_dev, pool))
        got = [tr.read(l) for l in range(len(layers))]
    finally:
        tr.close()
    for l, (g, r, f, start) in enumerate(zip(got, ref, f32, layers)):
        for what, j in (("kernel", 0), ("bias", 1)):
            limit, dev = T.bound(f[j], r[j])
            err = float(np.abs(g[j].astype(np.float64) - r[j]).max())
            moved = float(np.abs(r[j] - start[j]).max())
            print(f"{name} {loss} {optimizer} layer {l} {what}: |gpu-f64|={err:.3e} |f32-f64|={dev:.3e} moved={moved:.3e} "
                  f"limit={limit:.3e}")
            assert moved > 1e-4
            assert err <= limit, f"layer {l} {what}"
    for when, got_loss, r, f in zip(("before", "after"), losses, losses_ref, losses_f32):
        limit, dev = T.bound(f, r)
        print(f"{name} {loss} {optimizer} loss {when}: gpu={got_loss:.8f} f64={r:.8f} |gpu-f64|={abs(got_loss - r):.3e} "
              f"|f32-f64|={dev:.3e} limit={limit:.3e}")
        assert abs(got_loss - r) <= limit
    assert losses[1] < losses[0] and losses_ref[1] < losses_ref[0]


def fit_arguments(loss, n=700):
    rng = np.random.default_rng(12)
    x = (np.maximum(rng.normal(size=(n, 1024)), 0) * 0.5).astype(np.float32)
    targets = make_targets(rng, n, 13, loss)
    return dict(embeddings=x, targets=targets, classes=[f"c{i}" for i in range(13)], loss=loss, epochs=2, batch_size=300, seed=4,
                validation=(x[:100], targets[:100]))


@pytest.mark.parametrize("loss", LOSSES)
def test_fit_head_twice_gives_the_same_bits(loss):
    a = train.fit_head(**fit_arguments(loss))
    b = train.fit_head(**fit_arguments(loss))
    assert len(a.history["loss"]) == 2 and len(a.history["val_loss"]) == 2
    assert a.history == b.history and a.history["loss"][1] < a.history["loss"][0]
    for (k, bias, act), (k2, bias2, _) in zip(a.head.layers, b.head.layers):
        assert act == "linear" and k.tobytes() == k2.tobytes() and bias.tobytes() == bias2.tobytes()
    start = train.glorot_layers(np.random.default_rng(4), [13], ["linear"])
    assert np.abs(a.head.layers[0][0] - start[0][0]).max() > 1e-4
    # the history is the restatement's: mean loss of the steps, weighted by their rows (ragged last batch included)
    rng = np.random.default_rng(4)
    layers = train.glorot_layers(rng, [13], ["linear"])
    args = fit_arguments(loss)
    opt, mean = T.Adam(), []
    for _ in range(2):
        perm = rng.permutation(700)
        total = 0.0
        for at in range(0, 700, 300):
            rows = perm[at:at + 300]
            value, grads = T.gradients(layers, args["embeddings"][rows], args["targets"][rows], loss)
            total += value * len(rows)
            layers = opt.apply(T.cast_layers(layers, np.float64), grads)
        mean.append(total / 700)
    val = T.mean_loss(layers, args["embeddings"][:100], args["targets"][:100], loss)
    print(f"{loss}: history {a.history} restatement {mean} val {val}")
    assert np.allclose(a.history["loss"], mean, rtol=1e-5, atol=0) and abs(a.history["val_loss"][1] - val) <= 1e-5 * val


@pytest.mark.parametrize("width", (13, 1, 40, 64))
@pytest.mark.parametrize("loss", LOSSES)
def test_the_fused_one_layer_kernel_gives_the_layer_by_layer_bits(data, loss, width):
    x, x_dev = data
    layers = make_layers([width], ["linear"], seed=3)
    out = {}
    for fused in (True, False):
        rng_b = np.random.default_rng(5)
        tr = train.Trainer(layers, loss, "adam", 1e-3, max_batch=MAX_BATCH)
        try:
            tr.set_fusion(fused)
            for batch in (1025, 33, 257, MAX_BATCH):
                rows = rng_b.permutation(N_ROWS)[:batch].astype(np.int32)
                tr.step(x_dev, to_dev(rows), to_dev(make_targets(rng_b, batch, width, loss)), batch)
            out[fused] = (tr.read(0), tr.gradients(0), tr.logits(MAX_BATCH), tr.mean_loss())
        finally:
            tr.close()
    (p, g, z, m), (p2, g2, z2, m2) = out[True], out[False]
    assert z.tobytes() == z2.tobytes() and m == m2
    assert g[0].tobytes() == g2[0].tobytes() and g[1].tobytes() == g2[1].tobytes()
    assert p[0].tobytes() == p2[0].tobytes() and p[1].tobytes() == p2[1].tobytes()
    moved = float(np.abs(p[0] - layers[0][0]).max())
    if loss == "categorical" and width == 1:
        assert moved == 0.0 and not g[0].any()         # the softmax of one logit is 1 whatever it is: the gradient is exactly zero
    else:
        assert moved > 1e-4


@pytest.mark.parametrize("fused", (True, False))
def test_a_ragged_batch_writes_nothing_it_does_not_own(fused):
    import torch
    rng = np.random.default_rng(6)
    named = 40
    x = torch.full((64, 1024), float("nan"), dtype=torch.float32).cuda()       # the rows beyond those named: a NaN pattern
    x[:named] = to_dev((np.maximum(rng.normal(size=(named, 1024)), 0) * 0.5).astype(np.float32))
    before = x.cpu().numpy().copy()
    layers = make_layers([13], ["linear"], seed=3)
    rows = rng.integers(0, named, 33).astype(np.int32)
    tr = train.Trainer(layers, "categorical", "sgd", 1e-2, max_batch=MAX_BATCH)
    try:
        tr.set_fusion(fused)
        pattern = 0x7FC12345                                                  # a NaN with a payload no kernel produces
        tr.workspace_fill(pattern)
        tr.step(x, to_dev(rows), to_dev(rng.integers(0, 13, 33).astype(np.int32)), 33)
        ws = tr.workspace()
        dw, db = tr.gradients(0)
    finally:
        tr.close()
    owned = 1024 * 13 + 13                                                    # slice 0's dW and db partial
    assert ws.size == (MAX_BATCH // SLICE) * owned
    assert np.isfinite(ws[:owned]).all() and np.isfinite(dw).all() and np.isfinite(db).all()
    assert ws[:1024 * 13].tobytes() == dw.tobytes() and ws[1024 * 13:owned].tobytes() == db.tobytes()   # one slice: the sum is it
    assert (ws[owned:].view(np.uint32) == pattern).all()
    assert x.cpu().numpy().tobytes() == before.tobytes()


# ---------------------------------------------------------------------------------------------------- end to end
HOP = 15360
WINDOWS = 64
TONE_LEVEL = 0.3        # the bursts' level as oracle.yamnet_oracle.synthetic_audio makes them.  The test asserts that the float64
                        # restatement separates the two kinds at this level before it relies on it; should that fail on the
                        # engine's embeddings, this is the constant to raise (two_kinds adds the difference to the bursts)


def two_kinds():
    """64 windows cut at the tone bursts of synthetic_audio (0.5 s of every 5 s) and 64 cut between them."""
    from oracle import yamnet_oracle as O
    audio = O.synthetic_audio(5 * 16000 * WINDOWS + HOP + 240, seed=99).astype(np.float64)
    if TONE_LEVEL != 0.3:
        t = np.arange(audio.size) / 16000.0
        audio = np.clip(audio + (TONE_LEVEL - 0.3) * np.sin(2 * np.pi * 220.0 * t) * (np.mod(t, 5.0) < 0.5), -1.0, 1.0 - 2.0 ** -23)
    tone = np.concatenate([audio[5 * 16000 * k: 5 * 16000 * k + HOP] for k in range(WINDOWS)] + [audio[-240:]])
    noise = np.concatenate([audio[5 * 16000 * k + 32000: 5 * 16000 * k + 32000 + HOP] for k in range(WINDOWS)] + [audio[-240:]])
    return tone.astype(np.float32), noise.astype(np.float32)


def test_embed_fit_save_load_analyze(engine, tmp_path):
    import wave
    import pandas as pd
    import torch
    from buzzdetect_amd.analyze import analyze
    from buzzdetect_amd.engine import HipEngine
    tone, noise = two_kinds()
    emb = torch.cat([engine.embed(tone, 0.96).device_tensor(), engine.embed(noise, 0.96).device_tensor()])
    assert emb.shape == (2 * WINDOWS, 1024)
    is_tone = np.arange(2 * WINDOWS) < WINDOWS
    targets = np.stack([~is_tone, is_tone], axis=1).astype(np.float32)          # ambient, ins_buzz
    fit_rows = np.arange(2 * WINDOWS) % 2 == 0                                  # train on half, hold the other half out
    held = ~fit_rows
    x_fit, x_held = emb[torch.from_numpy(fit_rows).cuda()].contiguous(), emb[torch.from_numpy(held).cuda()].contiguous()
    kw = dict(classes=["ambient", "ins_buzz"], loss="binary", epochs=40, batch_size=16, seed=21, learning_rate=1e-3)
    fit = train.fit_head(x_fit, targets[fit_rows], **kw)
    assert fit.history["loss"][-1] < fit.history["loss"][0]

    # the float64 restatement trained with the same seed and batches, alone: does it separate the two kinds?
    x_host = emb.cpu().numpy()
    rng = np.random.default_rng(21)
    layers = train.glorot_layers(rng, [2], ["linear"])
    n_fit = int(fit_rows.sum())
    batches = []
    for _ in range(40):
        perm = rng.permutation(n_fit)
        batches += [(perm[at:at + 16], targets[fit_rows][perm[at:at + 16]]) for at in range(0, n_fit, 16)]
    ref = T.train(layers, x_host[fit_rows], batches, "binary", T.Adam())
    ref_logits = T.forward(ref, x_host[held])[-1]
    ref_acc = float(((ref_logits[:, 1] > 0) == is_tone[held]).mean())
    print(f"restatement: held-out accuracy {ref_acc:.3f} at tone level {TONE_LEVEL}")
    assert ref_acc >= 0.9

    # the trainer's own forward pass on the held-out windows
    tr = train.Trainer(fit.head.layers, "binary", max_batch=WINDOWS)
    try:
        tr.loss_of(x_held, None, to_dev(targets[held]), WINDOWS)
        logits = tr.logits(WINDOWS)
    finally:
        tr.close()
    acc = float(((logits[:, 1] > 0) == is_tone[held]).mean())
    print(f"trainer: held-out accuracy {acc:.3f}; max|logit - restatement| = {np.abs(logits - ref_logits).max():.3e}")
    assert acc >= ref_acc - 1.0 / WINDOWS

    models = tmp_path / "models"
    table = train.metrics_table(logits[:, 1], is_tone[held])
    train.save_model(str(models / "model_fit"), fit, metrics=table)
    eng = HipEngine(modelname="model_fit", models_dir=str(models))
    try:
        assert eng.classes == ["ambient", "ins_buzz"]
        got = np.concatenate([eng.predict(tone, 0.96).numpy(), eng.predict(noise, 0.96).numpy()])[held]
    finally:
        eng.close()
    delta = float(np.abs(got - logits).max())
    print(f"engine logits vs trainer forward: max|delta| = {delta:.3e}, max|logit| = {np.abs(logits).max():.3f}")
    assert delta <= 1e-4                                                        # the project's logit gate

    (tmp_path / "audio").mkdir()
    with wave.open(str(tmp_path / "audio" / "rec.wav"), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes((np.clip(tone[: HOP * 8 + 240], -1, 1 - 2 ** -15) * 32768.0).round().astype("<i2").tobytes())
    precisions = [float(r.split(",")[1]) for r in table.splitlines()[1:] if r.split(",")[1] != ""]
    rep = analyze("model_fit", precision=max(precisions), chunklength=200, dir_audio=str(tmp_path / "audio"),
                  dir_out=str(tmp_path / "out"), dir_models=str(models), analyzers_gpu=1)
    assert rep.files_done == 1
    out = pd.read_csv(tmp_path / "out" / "rec_buzzdetect.csv")
    assert list(out.columns) == ["start", "detections_ins_buzz"] and len(out) == 8
