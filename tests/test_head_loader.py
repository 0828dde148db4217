"""The model-directory reader (weights.load_head / dense_chain / bundle_layer_entries) on the CPU: the recorded graph of the
reference's model_general_v3, directories written by tools/modelgen.py, the lookup order and every refusal."""
import os

import numpy as np
import pytest

from buzzdetect_amd import weights as W
from tools import make_head_fixture, modelgen as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_graph_model_general_v3.json")


def test_recorded_reference_graph_is_one_linear_layer():
    nodes, index = make_head_fixture.load(GOLDEN)
    assert len(nodes) == 162
    chain = W.dense_chain(nodes)
    assert chain == [("linear", True, "generaltest_general/dense/MatMul")]
    (kern, bias), = W.bundle_layer_entries(index, len(chain))
    assert kern.name == "layer_with_weights-0/kernel/.ATTRIBUTES/VARIABLE_VALUE" and tuple(kern.shape) == (1024, 13)
    assert bias.name == "layer_with_weights-0/bias/.ATTRIBUTES/VARIABLE_VALUE" and tuple(bias.shape) == (13,)
    # the optimizer's slots have the same shapes and are not what was taken
    decoys = [e for e in index.values() if tuple(e.shape) == (1024, 13) and e.name != kern.name]
    assert len(decoys) == 2 and all(e.name.startswith("optimizer/") for e in decoys)


def test_generated_directory_of_the_packaged_head_gives_the_packaged_bytes(tmp_path):
    packaged = W.load_head()
    G.write_model_dir(str(tmp_path / "model_general_v3"), packaged.layers, classes=packaged.classes)
    got = W.load_head("model_general_v3", models_dir=str(tmp_path))
    assert got.source == str(tmp_path / "model_general_v3") and got.fused
    data = os.path.join(os.path.dirname(W.__file__), "data")
    assert got.kernel.astype("<f4").tobytes() == open(os.path.join(data, "head_model_general_v3_kernel_1024x13.f32"), "rb").read()
    assert got.bias.astype("<f4").tobytes() == open(os.path.join(data, "head_model_general_v3_bias_13.f32"), "rb").read()
    assert got.classes == packaged.classes and got.embeddername == "yamnet_k2" and got.digits_results == 2


@pytest.mark.parametrize("name", sorted(G.EXAMPLE_STACKS))
def test_generated_stacks_round_trip(tmp_path, name):
    widths, acts = G.EXAMPLE_STACKS[name]
    layers = G.glorot_layers(widths, acts, seed=5)
    classes = [f"c{i}" for i in range(widths[-1])]
    G.write_model_dir(str(tmp_path / name), layers, classes=classes, embeddername="yamnet", digits_results=4)
    head = W.load_head(name, models_dir=str(tmp_path))
    assert [a for _, _, a in head.layers] == acts
    for (k, b, _), (k2, b2, _) in zip(layers, head.layers):
        assert k2.dtype == np.float32 and np.array_equal(k, k2) and np.array_equal(b, b2)
    assert head.classes == classes and head.digits_results == 4 and head.embeddername == "yamnet"
    assert head.metrics_path == str(tmp_path / name / "tests" / "metrics.csv")
    assert head.fused is False
    with pytest.raises(AttributeError, match="stack"):
        head.kernel


def test_matmul_without_biasadd_gets_a_zero_bias(tmp_path):
    layers = G.glorot_layers([7, 3], ["relu", "linear"], seed=2)
    G.write_model_dir(str(tmp_path / "m"), layers, faults=["no_bias"])
    head = W.load_head("m", models_dir=str(tmp_path))
    assert not head.layers[0][1].any() and head.layers[0][1].shape == (7,)
    assert np.array_equal(head.layers[1][1], layers[1][1])


def test_lookup_order_and_error_text(tmp_path, monkeypatch):
    layers = G.glorot_layers([3], ["linear"], seed=1)
    cwd, env, given = tmp_path / "cwd", tmp_path / "env", tmp_path / "given"
    for root, cls in ((cwd / "models", "from_cwd"), (env, "from_env"), (given, "from_given")):
        G.write_model_dir(str(root / "model_mine"), layers, classes=[cls, "b", "c"])
    cwd.mkdir(exist_ok=True)
    monkeypatch.chdir(cwd)
    monkeypatch.setenv(W.MODELS_ENV, str(env))
    assert W.load_head("model_mine", models_dir=str(given)).classes[0] == "from_given"
    assert W.load_head("model_mine").classes[0] == "from_cwd"
    monkeypatch.chdir(tmp_path)
    assert W.load_head("model_mine").classes[0] == "from_env"
    # the packaged model comes last, for model_general_v3 alone, and only without an explicit models_dir
    assert W.load_head("model_general_v3").source == W.DATA_DIR
    with pytest.raises(FileNotFoundError) as ei:
        W.load_head("model_general_v3", models_dir=str(given))
    assert str(given / "model_general_v3") in str(ei.value)
    monkeypatch.delenv(W.MODELS_ENV)
    with pytest.raises(FileNotFoundError) as ei:
        W.load_head("model_other")
    text = str(ei.value)
    for place in (str(tmp_path / "models" / "model_other"), os.path.join(W.PACKAGED_OVERLAY, "models", "model_other"),
                  W.MODELS_ENV):
        assert place in text
    monkeypatch.setenv(W.MODELS_ENV, str(env))
    with pytest.raises(FileNotFoundError) as ei:
        W.load_head("model_other")
    assert str(env / "model_other") in str(ei.value)


def _refused(tmp_path, match, layers=None, **kw):
    layers = layers or G.glorot_layers([20, 4], ["relu", "linear"], seed=3)
    G.write_model_dir(str(tmp_path / "m"), layers, **kw)
    with pytest.raises(W.UnsupportedHeadError, match=match) as ei:
        W.load_head("m", models_dir=str(tmp_path))
    assert str(tmp_path / "m") in str(ei.value)          # the file it was read from


def test_refuses_unknown_op(tmp_path):
    _refused(tmp_path, "unsupported op LeakyRelu", faults=["leaky_relu"])


def test_refuses_transpose_b(tmp_path):
    _refused(tmp_path, "transpose_b=true", faults=["transpose_b"])


def test_refuses_shape_that_does_not_chain(tmp_path):
    a = G.glorot_layers([20], ["relu"], seed=1)
    b = G.glorot_layers([4], ["linear"], seed=1, n_in=19)
    _refused(tmp_path, r"\(19, 4\).*gives 20", layers=a + b)


def test_refuses_first_layer_that_does_not_start_at_the_embedding(tmp_path):
    _refused(tmp_path, r"\(512, 4\).*gives 1024", layers=G.glorot_layers([4], ["linear"], seed=1, n_in=512))


def test_refuses_float64_kernel(tmp_path):
    _refused(tmp_path, "dtype 2, not float32", faults=["float64"])
    _refused(tmp_path, "dtype 2, not float32", faults=["float64", "float64_graph"])


def test_refuses_softmax_on_a_hidden_layer(tmp_path):
    _refused(tmp_path, "Softmax on hidden layer 0", layers=G.glorot_layers([20, 4], ["softmax", "linear"], seed=3))


def test_refuses_nine_layers(tmp_path):
    _refused(tmp_path, "9 Dense layers, at most 8", layers=G.glorot_layers([8] * 9, ["relu"] * 8 + ["linear"], seed=3))
    G.write_model_dir(str(tmp_path / "ok"), G.glorot_layers([8] * 8, ["relu"] * 7 + ["linear"], seed=3))
    assert len(W.load_head("ok", models_dir=str(tmp_path)).layers) == 8


def test_refuses_width_2049(tmp_path):
    _refused(tmp_path, "width 2049, outside 1..2048", layers=G.glorot_layers([2049, 4], ["relu", "linear"], seed=3))
    G.write_model_dir(str(tmp_path / "ok"), G.glorot_layers([2048, 4], ["relu", "linear"], seed=3))
    assert W.load_head("ok", models_dir=str(tmp_path)).layers[0][0].shape == (1024, 2048)


def test_refuses_classes_that_do_not_match_the_last_width(tmp_path):
    _refused(tmp_path, "3 classes but the last layer .* has width 4", classes=["a", "b", "c"])


def test_refuses_bundle_without_graph(tmp_path):
    _refused(tmp_path, "no readable graph", graph=False)
    (tmp_path / "m" / "saved_model.pb").write_bytes(b"\x0a\xff\xff")       # not a SavedModel
    with pytest.raises(W.UnsupportedHeadError, match="no readable graph"):
        W.load_head("m", models_dir=str(tmp_path))


def test_abi_table_matches_the_header():
    import re
    from buzzdetect_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "buzzdetect_head.h")).read()
    assert sorted(re.findall(r"^BD_API [^;(]*?(bd_\w+)\(", header, re.M)) == sorted(_lib.HEAD_PROTOTYPES)
    assert int(re.search(r"#define BD_HEAD_ABI_VERSION (\d+)", header).group(1)) == _lib.HEAD_ABI_VERSION
    assert int(re.search(r"#define BD_HEAD_MAX_LAYERS (\d+)", header).group(1)) == W.HEAD_MAX_LAYERS == _lib.HEAD_MAX_LAYERS
    assert int(re.search(r"#define BD_HEAD_MAX_WIDTH (\d+)", header).group(1)) == W.HEAD_MAX_WIDTH == _lib.HEAD_MAX_WIDTH
    for name, code in _lib.HEAD_ACTIVATIONS.items():
        assert int(re.search(rf"#define BD_HEAD_{name.upper()} (\d+)", header).group(1)) == code
