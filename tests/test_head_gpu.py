"""The dense-stack head on the GPU (include/buzzdetect_head.h, csrc/headmlp.hip): bd_head_attach + predict against a float64
restatement of the stack fed with the engine's own float32 embeddings, bit identity with the fused head and across pass
positions, more than 64 outputs through analyze(), thresholds from the model's own metrics, and the plugin overlay.

Bound: |delta| <= 1e-4 per output, the project's logit gate (README, accuracy row); every case prints what it observed."""
import os
import wave

import numpy as np
import pytest

from oracle import yamnet_oracle as O
from tests.dense_cases import stack_f64
from tools import modelgen as G

pytestmark = pytest.mark.gpu

HOP = 15360
WINDOW_COUNTS = (1, 31, 1024, 1025, 4096)
MODES = ("f32", "f16x3", "f16")
LOGIT_GATE = 1e-4


@pytest.fixture(scope="module")
def audio():
    """Enough 16 kHz audio for 1025 windows in one chunk (a chunk is limited to 2^24 samples; 4096 windows are four chunks)."""
    return O.synthetic_audio(HOP * 1025 + 240, seed=77)


def chunks_for(audio, windows):
    if windows <= 1025:
        return [audio[: HOP * windows + 240]]
    assert windows % 1024 == 0
    return [audio[: HOP * 1024 + 240]] * (windows // 1024)


def make_engine(tmp_path_factory, name, layers, **kw):
    from buzzdetect_amd.engine import HipEngine
    root = tmp_path_factory.mktemp("models_" + name)
    G.write_model_dir(str(root / name), layers, **kw)
    return HipEngine(modelname=name, models_dir=str(root))


@pytest.fixture(scope="module", params=sorted(G.EXAMPLE_STACKS))
def stack_engine(request, tmp_path_factory):
    widths, acts = G.EXAMPLE_STACKS[request.param]
    layers = G.glorot_layers(widths, acts, seed=11)
    eng = make_engine(tmp_path_factory, request.param, layers)
    yield eng, layers
    eng.close()


@pytest.mark.parametrize("windows", WINDOW_COUNTS)
@pytest.mark.parametrize("mode", MODES)
def test_stack_matches_float64_on_the_engines_own_embeddings(stack_engine, audio, mode, windows):
    eng, layers = stack_engine
    assert eng.n_classes == layers[-1][0].shape[1] and eng._lib.bd_head_outputs(eng._handle) == eng.n_classes
    eng.set_pointwise_mode(mode)
    try:
        logits, embs = eng.predict_batch(chunks_for(audio, windows), 0.96, want_embeddings=True)
    finally:
        eng.set_pointwise_mode("f16x3")
    got = np.concatenate([r.numpy() for r in logits])
    emb = np.concatenate([e.numpy() for e in embs])
    assert got.shape == (windows, eng.n_classes) and emb.shape == (windows, 1024) and got.dtype == np.float32
    ref = stack_f64(emb, layers)
    # pre-activations O(1-10), as model_general_v3's are (weights Glorot-scaled): the gate is not met by vanishing outputs
    pre = np.abs(emb.astype(np.float64) @ layers[0][0].astype(np.float64)).max()
    delta = np.abs(got - ref).max()
    print(f"head[{'-'.join(str(k.shape[1]) for k, _, _ in layers)}] mode={mode} windows={windows}: max|delta|={delta:.3e} "
          f"max|pre-activation 0|={pre:.2f}")
    assert 1.0 <= pre <= 100.0
    assert delta <= LOGIT_GATE
    if layers[-1][2] == "softmax":
        dsum = np.abs(got.astype(np.float64).sum(axis=1) - 1.0).max()
        print(f"  softmax rows: max|sum - 1|={dsum:.3e}")
        assert dsum <= 1e-5


def test_packaged_head_from_a_generated_directory_is_bit_identical(engine, tmp_path_factory, audio):
    import torch
    from buzzdetect_amd import weights as W
    packaged = W.load_head()
    gen = make_engine(tmp_path_factory, "model_general_v3", packaged.layers, classes=packaged.classes)
    try:
        assert gen.head.source != W.DATA_DIR and gen._lib.bd_head_outputs(gen._handle) == 0      # the fused head, not a stack
        x = audio[: HOP * 40 + 240]
        for mode in MODES:
            engine.set_pointwise_mode(mode)
            gen.set_pointwise_mode(mode)
            a, b = engine.predict(x, 0.96), gen.predict(x, 0.96)
            a.numpy(), b.numpy()
            assert a.shape == (40, 13) and torch.equal(a.tensor, b.tensor)
    finally:
        engine.set_pointwise_mode("f16x3")
        gen.close()


@pytest.mark.parametrize("mode", ("f32", "f16x3"))
def test_a_window_gives_the_same_bits_alone_and_inside_passes(tmp_path_factory, audio, mode):
    widths, acts = G.EXAMPLE_STACKS["tanh_relu_100_37_5"]
    eng = make_engine(tmp_path_factory, "identity", G.glorot_layers(widths, acts, seed=11))
    try:
        eng.set_pointwise_mode(mode)
        in_1025 = eng.predict(audio, 0.96).numpy()                       # a pass of 1024 and a ragged pass of one window
        in_1024 = eng.predict(audio[: HOP * 1024 + 240], 0.96).numpy()   # one full pass
        assert in_1025.shape == (1025, 5) and in_1024.shape == (1024, 5)
        assert in_1025[:1024].tobytes() == in_1024.tobytes()
        for k in (0, 517, 1023, 1024):
            alone = eng.predict(audio[HOP * k: HOP * k + 15600], 0.96).numpy()
            assert alone.shape == (1, 5)
            assert alone[0].tobytes() == in_1025[k].tobytes(), f"window {k} alone differs from itself inside 1025 windows"
            if k < 1024:
                assert alone[0].tobytes() == in_1024[k].tobytes()
    finally:
        eng.close()


@pytest.mark.parametrize("mode", ("f32", "f16x3"))
@pytest.mark.parametrize("name", ("tanh_relu_100_37_5", "softmax_64_10"))
def test_the_one_kernel_per_op_plan_gives_the_default_plans_bits(tmp_path_factory, audio, mode, name):
    """bd_set_fusion(0, 0) ends a pass in walk_layers: pool alone, then the stack with its hidden activations behind the pooled
    rows - the other way into the stack.  The fused launch sets are bit-identical to the kernels they replace, so are the rows."""
    widths, acts = G.EXAMPLE_STACKS[name]
    eng = make_engine(tmp_path_factory, "perop_" + name, G.glorot_layers(widths, acts, seed=11))
    try:
        eng.set_pointwise_mode(mode)
        x = audio[: HOP * 70 + 240]
        default = eng.predict(x, 0.96).numpy().copy()
        default_b, emb_b = eng.predict_batch([x], 0.96, want_embeddings=True)
        eng.set_fusion(stem=False, separable=False)
        per_op = eng.predict(x, 0.96).numpy().copy()                      # pooled rows in the workspace
        per_op_b, emb_p = eng.predict_batch([x], 0.96, want_embeddings=True)   # pooled rows in the caller's embeddings
        assert default.shape == (70, widths[-1])
        assert emb_b[0].numpy().tobytes() == emb_p[0].numpy().tobytes()
        assert per_op.tobytes() == default.tobytes()
        assert per_op_b[0].numpy().tobytes() == default.tobytes() == default_b[0].numpy().tobytes()
    finally:
        eng.close()


def test_a_narrow_linear_stack_has_the_bits_of_its_columns_in_a_wide_one(audio):
    """bd_head_attach itself on two engines made without a head: one linear layer 1024 -> 13, and one 1024 -> 65 whose first 13
    columns are that layer.  An output depends only on its row of A, its column of W and the k order of the matrix-core walk, so
    the 13 columns are byte-equal - unless a stack of at most 64 linear outputs ever ran as a fused-route member, whose sum
    has another order."""
    from buzzdetect_amd.engine import HipEngine
    (kernel, bias, _), = G.glorot_layers([65], ["linear"], seed=23)
    stacks = {13: [(np.ascontiguousarray(kernel[:, :13]), bias[:13].copy(), "linear")], 65: [(kernel, bias, "linear")]}
    x = audio[: HOP * 65 + 240]
    rows = {}
    for n, layers in stacks.items():
        eng = HipEngine(modelname=None)
        try:
            eng.n_classes = n                            # what _attach_stack holds bd_head_outputs to
            eng._attach_stack(layers)
            assert eng._lib.bd_head_outputs(eng._handle) == n and eng._lib.bd_headset_members(eng._handle) == 0
            rows[n] = eng.predict(x, 0.96).numpy().copy()
        finally:
            eng.close()
    assert rows[13].shape == (65, 13) and rows[65].shape == (65, 65) and rows[13].dtype == np.float32
    assert np.abs(rows[13]).max() > 0.0
    assert rows[13].tobytes() == np.ascontiguousarray(rows[65][:, :13]).tobytes()


def write_wav(path, x, rate=16000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes((np.clip(x, -1, 1 - 2 ** -15) * 32768.0).round().astype("<i2").tobytes())


def quantised(x):
    return (np.clip(x, -1, 1 - 2 ** -15) * 32768.0).round().astype(np.int16).astype(np.float32) / 32768.0


def test_more_than_64_outputs_through_analyze(tmp_path, audio):
    import pandas as pd
    from buzzdetect_amd.analyze import analyze
    from buzzdetect_amd.engine import HipEngine
    models = tmp_path / "models"
    layers = G.glorot_layers([200], ["linear"], seed=4)
    G.write_model_dir(str(models / "model_wide"), layers, digits_results=3)
    x = audio[: HOP * 12 + 240]
    (tmp_path / "audio").mkdir()
    write_wav(tmp_path / "audio" / "rec.wav", x)
    rep = analyze("model_wide", chunklength=200, dir_audio=str(tmp_path / "audio"), dir_out=str(tmp_path / "out"),
                  dir_models=str(models), analyzers_gpu=1)
    assert rep.files_done == 1
    table = pd.read_csv(tmp_path / "out" / "rec_buzzdetect.csv")
    eng = HipEngine(modelname="model_wide", models_dir=str(models))
    try:
        assert eng.n_classes == 200
        assert list(table.columns) == ["start"] + ["activation_" + c for c in eng.classes]
        pred = eng.predict(quantised(x), 0.96).numpy()
    finally:
        eng.close()
    assert pred.shape == (12, 200) and len(table) == 12
    assert np.array_equal(table.iloc[:, 1:].to_numpy().astype(np.float32), pred.round(3))
    assert not np.array_equal(pred.round(3), pred.round(2))              # three decimals, from the model's config


def test_detections_use_the_models_own_metrics(tmp_path, audio):
    import pandas as pd
    from buzzdetect_amd.analyze import analyze
    from buzzdetect_amd.engine import HipEngine
    models = tmp_path / "models"
    widths, acts = G.EXAMPLE_STACKS["relu_256_13"]
    layers = G.glorot_layers(widths, acts, seed=9)
    G.write_model_dir(str(models / "model_mine"), layers)
    x = audio[: HOP * 30 + 240]
    eng = HipEngine(modelname="model_mine", models_dir=str(models))
    try:
        buzz = eng.predict(quantised(x), 0.96).numpy()[:, eng.classes.index("ins_buzz")]
    finally:
        eng.close()
    threshold = round(float(np.median(buzz)), 2)                         # a threshold that splits this recording's windows
    expect = (buzz > threshold).astype(int)
    assert 0 < expect.sum() < len(expect)
    (models / "model_mine" / "tests" / "metrics.csv").write_text(
        '"threshold","precision","sensitivity","fpr"\n'
        f"{threshold - 1},0.5,0.9,0.1\n{threshold},0.9,0.5,0.01\n{threshold + 1},0.99,0.1,0.001\n")
    (tmp_path / "audio").mkdir()
    write_wav(tmp_path / "audio" / "rec.wav", x)
    analyze("model_mine", precision=0.9, chunklength=200, dir_audio=str(tmp_path / "audio"), dir_out=str(tmp_path / "out"),
            dir_models=str(models), analyzers_gpu=1)
    table = pd.read_csv(tmp_path / "out" / "rec_buzzdetect.csv")
    assert list(table.columns) == ["start", "detections_ins_buzz"]
    assert table["detections_ins_buzz"].tolist() == expect.tolist()


def test_a_generated_plugin_predicts_through_the_overlay(dropin_cwd, tmp_path, monkeypatch, audio):
    from src import config as cfg
    from src.inference.models import load_model
    from buzzdetect_amd.engine import HipEngine
    models = tmp_path / "models"
    widths, acts = G.EXAMPLE_STACKS["softmax_64_10"]
    G.write_model_dir(str(models / "model_mine"), G.glorot_layers(widths, acts, seed=6), digits_results=4)
    G.write_model_py(str(models / "model_mine"), "model_mine", digits_results=4)
    monkeypatch.setattr(cfg, "DIR_MODELS", str(models))
    model = load_model("model_mine", framehop_prop=1.0, initialize=True)
    assert type(model).__name__ == "Model" and model.digits_results == 4 and len(model.config["classes"]) == 10
    x = audio[: HOP * 5 + 240]
    got = model.predict(x).numpy()
    eng = HipEngine(modelname="model_mine", models_dir=str(models))
    try:
        ref = eng.predict(x, 0.96).numpy()
    finally:
        eng.close()
    assert got.shape == (5, 10) and got.tobytes() == ref.tobytes()
