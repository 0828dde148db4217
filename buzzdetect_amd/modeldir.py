"""Write a trained-model directory in the reference's layout from Python, without TensorFlow (``train.save_model`` and
``tools/modelgen.py`` both write through here).

``write_model_dir`` lays down what ``buzzdetect_amd.weights.read_model_dir`` reads - and what a Keras ``model.save()`` of
a Sequential of Dense layers leaves behind, as far as that reader looks:

    config_model.json                        classes, embeddername, digits_results
    saved_model.pb                           SavedModel{MetaGraphDef{GraphDef{nodes, FunctionDefLibrary}}}: the variables and
                                             the serving call in the main graph; in the library the signature wrapper and
                                             ``__inference__wrapped_model_N`` with the inlined body under the node names Keras
                                             gives them (``<model>/dense_1/MatMul/ReadVariableOp``, ``.../MatMul``,
                                             ``.../BiasAdd``, ``.../Relu``, ``Identity``, ``NoOp``)
    variables/variables.index                TensorBundle index: a LevelDB table (one data block, block trailers with masked
                                             CRC-32C, 48-byte footer) of BundleEntryProto values
    variables/variables.data-00000-of-00001  the tensors: ``layer_with_weights-k/{kernel,bias}`` and, as a real bundle has
                                             them, optimizer slots of the same shapes (decoys: filled with other values)
    tests/metrics.csv                        threshold / precision / sensitivity / fpr rows

Written from the formats (protobuf wire format, the TensorBundle and LevelDB table layouts as ``artifacts.py`` restates them),
not from any existing file.  ``faults`` plants what the reader must refuse (tests/test_head_loader.py).
"""
from __future__ import annotations

import json
import os
import struct
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

ACTIVATION_OPS = {"relu": "Relu", "sigmoid": "Sigmoid", "tanh": "Tanh", "softmax": "Softmax"}
DT_FLOAT, DT_DOUBLE, DT_STRING, DT_INT64, DT_RESOURCE = 1, 2, 7, 9, 20
_TABLE_MAGIC = 0xDB4775248B80FB57


# --------------------------------------------------------------------------- protobuf wire format
def varint(v: int) -> bytes:
    if v < 0:
        v += 1 << 64
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def f_varint(fno: int, v: int) -> bytes:
    return varint(fno << 3) + varint(v)


def f_bytes(fno: int, payload: bytes) -> bytes:
    return varint(fno << 3 | 2) + varint(len(payload)) + payload


def f_str(fno: int, text: str) -> bytes:
    return f_bytes(fno, text.encode())


def shape_proto(dims: Sequence[int]) -> bytes:
    return b"".join(f_bytes(2, f_varint(1, d)) for d in dims)


def attr_type(dtype: int) -> bytes:
    return f_varint(6, dtype)


def attr_bool(v: bool) -> bytes:
    return f_varint(5, 1 if v else 0)


def attr_shape(dims: Sequence[int]) -> bytes:
    return f_bytes(7, shape_proto(dims))


def attr_func(name: str) -> bytes:
    return f_bytes(10, f_str(1, name))


def node(name: str, op: str, inputs: Sequence[str] = (), attrs: Optional[Dict[str, bytes]] = None) -> bytes:
    out = f_str(1, name) + f_str(2, op) + b"".join(f_str(3, i) for i in inputs)
    for k in sorted(attrs or {}):
        out += f_bytes(5, f_str(1, k) + f_bytes(2, attrs[k]))
    return out


def function(name: str, args: Sequence[Tuple[str, int]], result: str, nodes: Sequence[bytes], ret: str) -> bytes:
    sig = f_str(1, name) + b"".join(f_bytes(2, f_str(1, a) + f_varint(3, t)) for a, t in args)
    sig += f_bytes(3, f_str(1, result) + f_varint(3, DT_FLOAT))
    return f_bytes(1, sig) + b"".join(f_bytes(3, n) for n in nodes) + f_bytes(4, f_str(1, result) + f_str(2, ret))


# --------------------------------------------------------------------------- the graph
def layer_scope(k: int) -> str:
    return "dense" if k == 0 else f"dense_{k}"


def saved_model_bytes(widths: Sequence[int], activations: Sequence[str], model: str = "sequential", n_in: int = 1024,
                      faults: Sequence[str] = (), dtype: int = DT_FLOAT) -> bytes:
    """``faults``: "leaky_relu" (a LeakyRelu behind layer 0), "transpose_b" (on the last MatMul), "no_bias" (layer 0 has no
    BiasAdd: not a fault, the reader gives it zeros)."""
    main: List[bytes] = []
    resources: List[str] = []
    dims = [n_in] + list(widths)
    for k, w in enumerate(widths):
        for leaf, shape in (("kernel", [dims[k], w]), ("bias", [w])):
            # the optimizer's slots first, as a saved training run has them, then the variable itself
            for slot in ("Adam/v/", "Adam/m/", ""):
                name = f"{slot}{layer_scope(k)}/{leaf}"
                main.append(node(name, "VarHandleOp", (), {"dtype": attr_type(dtype), "shape": attr_shape(shape),
                                                           "shared_name": f_str(2, name)}))
                main.append(node(name + "/Read/ReadVariableOp", "ReadVariableOp", (name,), {"dtype": attr_type(dtype)}))
            resources.append(f"{layer_scope(k)}/{leaf}")
    wrapped, wrapper = "__inference__wrapped_model_1017", "__inference_signature_wrapper_1084"
    main.append(node("serving_default_input", "Placeholder", (), {"dtype": attr_type(dtype), "shape": attr_shape([-1, n_in])}))
    main.append(node("StatefulPartitionedCall", "StatefulPartitionedCall", ["serving_default_input"] + resources,
                     {"f": attr_func(wrapper)}))
    main.append(node("NoOp", "NoOp"))

    body: List[bytes] = []
    args: List[Tuple[str, int]] = [("input", dtype)]
    reads: List[str] = []
    cur = "input"
    for k, (w, act) in enumerate(zip(widths, activations)):
        scope = f"{model}/{layer_scope(k)}"
        res_k = f"{model}_{layer_scope(k)}_matmul_readvariableop_resource"
        res_b = f"{model}_{layer_scope(k)}_biasadd_readvariableop_resource"
        args += [(res_k, DT_RESOURCE), (res_b, DT_RESOURCE)]
        body.append(node(f"{scope}/MatMul/ReadVariableOp", "ReadVariableOp", (res_k,), {"dtype": attr_type(dtype)}))
        reads.append(f"{scope}/MatMul/ReadVariableOp")
        mm = {"T": attr_type(dtype), "transpose_a": attr_bool(False),
              "transpose_b": attr_bool("transpose_b" in faults and k == len(widths) - 1)}
        body.append(node(f"{scope}/MatMul", "MatMul", (cur, f"{scope}/MatMul/ReadVariableOp:value:0"), mm))
        cur = f"{scope}/MatMul:product:0"
        if not ("no_bias" in faults and k == 0):
            body.append(node(f"{scope}/BiasAdd/ReadVariableOp", "ReadVariableOp", (res_b,), {"dtype": attr_type(dtype)}))
            reads.append(f"{scope}/BiasAdd/ReadVariableOp")
            body.append(node(f"{scope}/BiasAdd", "BiasAdd", (cur, f"{scope}/BiasAdd/ReadVariableOp:value:0"),
                             {"T": attr_type(dtype)}))
            cur = f"{scope}/BiasAdd:output:0"
        if "leaky_relu" in faults and k == 0:
            body.append(node(f"{scope}/LeakyRelu", "LeakyRelu", (cur,), {"T": attr_type(dtype)}))
            cur = f"{scope}/LeakyRelu:activations:0"
        if act != "linear":
            op = ACTIVATION_OPS[act]
            body.append(node(f"{scope}/{op}", op, (cur,), {"T": attr_type(dtype)}))
            cur = f"{scope}/{op}:{'softmax' if op == 'Softmax' else 'activations' if op == 'Relu' else 'y'}:0"
    body.append(node("Identity", "Identity", (cur, "^NoOp"), {"T": attr_type(dtype)}))
    body.append(node("NoOp", "NoOp", ["^" + r for r in reads]))
    unknown = [("unknown" if i == 0 else f"unknown_{i - 1}", DT_RESOURCE) for i in range(1, len(args))]
    wrap_body = [node("StatefulPartitionedCall", "StatefulPartitionedCall", ["input"] + [u for u, _ in unknown],
                      {"f": attr_func(wrapped)}),
                 node("Identity", "Identity", ("StatefulPartitionedCall:output:0", "^NoOp"), {"T": attr_type(dtype)}),
                 node("NoOp", "NoOp", ("^StatefulPartitionedCall",))]
    library = f_bytes(1, function(wrapped, args, "identity", body, "Identity:output:0"))
    library += f_bytes(1, function(wrapper, [("input", dtype)] + unknown, "identity", wrap_body, "Identity:output:0"))
    graph = b"".join(f_bytes(1, n) for n in main) + f_bytes(2, library)
    return f_varint(1, 1) + f_bytes(2, f_bytes(2, graph))


# --------------------------------------------------------------------------- the TensorBundle
def _crc32c_table() -> List[int]:
    table = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
        table.append(c)
    return table


_CRC_TABLE = _crc32c_table()


def crc32c(data: bytes) -> int:
    c = 0xFFFFFFFF
    for b in data:
        c = _CRC_TABLE[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def masked_crc(data: bytes) -> int:
    c = crc32c(data)
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def table_block(entries: Sequence[Tuple[bytes, bytes]]) -> bytes:
    """A LevelDB block in which every entry is its own restart point (no key is prefix-compressed)."""
    out, restarts = bytearray(), []
    for key, val in entries:
        restarts.append(len(out))
        out += varint(0) + varint(len(key)) + varint(len(val)) + key + val
    for r in restarts or [0]:
        out += struct.pack("<I", r)
    out += struct.pack("<I", len(restarts) or 1)
    return bytes(out)


def bundle_bytes(tensors: Sequence[Tuple[str, np.ndarray]]) -> Tuple[bytes, bytes]:
    """(variables.index, variables.data-00000-of-00001) for ``tensors`` = [(name, array)]."""
    data = bytearray()
    entries: List[Tuple[bytes, bytes]] = [(b"", f_varint(1, 1) + f_varint(2, 0) + f_bytes(3, f_varint(1, 1)))]   # BundleHeaderProto
    dtypes = {np.dtype(np.float32): DT_FLOAT, np.dtype(np.float64): DT_DOUBLE, np.dtype(np.int64): DT_INT64}
    for name, arr in sorted(tensors, key=lambda t: t[0].encode()):
        raw = np.ascontiguousarray(arr).astype(arr.dtype.newbyteorder("<")).tobytes()
        val = f_varint(1, dtypes[arr.dtype]) + f_bytes(2, shape_proto(arr.shape)) + f_varint(3, 0)
        val += f_varint(4, len(data)) + f_varint(5, len(raw)) + varint(6 << 3 | 5) + struct.pack("<I", masked_crc(raw))
        entries.append((name.encode(), val))
        data += raw

    def with_trailer(block: bytes) -> bytes:       # compression type 0 + masked CRC-32C of block and type
        return block + b"\0" + struct.pack("<I", masked_crc(block + b"\0"))

    blocks = bytearray()
    data_block = table_block(entries)
    handles = []
    for block in (data_block, table_block([])):      # the entries, then an empty metaindex
        handles.append(varint(len(blocks)) + varint(len(block)))
        blocks += with_trailer(block)
    index_block = table_block([(entries[-1][0] + b"\xff", handles[0])])
    index_handle = varint(len(blocks)) + varint(len(index_block))
    blocks += with_trailer(index_block)
    footer = handles[1] + index_handle
    footer += b"\0" * (40 - len(footer)) + struct.pack("<Q", _TABLE_MAGIC)
    return bytes(blocks) + footer, bytes(data)


# --------------------------------------------------------------------------- a model directory
def glorot_layers(widths: Sequence[int], activations: Sequence[str], seed: int, n_in: int = 1024, gain: float = 4.0):
    """Seeded Dense layers, Glorot-uniform kernels times ``gain``: with embeddings of a few tenths (what YAMNet's pooled ReLU
    outputs are) the pre-activations come out O(1-10), as model_general_v3's do."""
    rng = np.random.default_rng(seed)
    layers, fan_in = [], n_in
    for w, act in zip(widths, activations):
        lim = gain * np.sqrt(6.0 / (fan_in + w))
        layers.append((rng.uniform(-lim, lim, (fan_in, w)).astype(np.float32),
                       rng.uniform(-0.5, 0.5, w).astype(np.float32), act))
        fan_in = w
    return layers


def default_metrics(n: int = 60) -> str:
    """A precision curve that rises with the threshold, in the columns of the reference's tests/metrics.csv."""
    rows = ['"threshold","precision","sensitivity","fpr"']
    for i in range(n):
        t = round(-3.0 + 0.1 * i, 2)
        rows.append(f"{t},{round(min(1.0, 0.4 + 0.0102 * i), 4)},{round(max(0.0, 1.0 - i / n), 4)},{round(max(0.0, 0.2 - i / (5 * n)), 4)}")
    return "\n".join(rows) + "\n"


def write_model_dir(path: str, layers, classes: Optional[Sequence[str]] = None, embeddername: str = "yamnet_k2",
                    digits_results: int = 2, metrics: Optional[str] = None, faults: Sequence[str] = (), seed: int = 0,
                    graph: bool = True, model: str = "sequential") -> str:
    """``layers`` = [(kernel [in, out], bias [out], activation)].  ``faults``: those of ``saved_model_bytes``, plus
    "float64" (the bundle's tensors in float64), "float64_graph" (the graph's dtypes).  ``graph=False`` leaves saved_model.pb out."""
    f64 = "float64" in faults
    widths = [k.shape[1] for k, _, _ in layers]
    acts = [a for _, _, a in layers]
    if classes is None:
        classes = [f"class_{i:03d}" for i in range(widths[-1])]
        if widths[-1] > 8:
            classes[8] = "ins_buzz"
    os.makedirs(os.path.join(path, "variables"), exist_ok=True)
    os.makedirs(os.path.join(path, "tests"), exist_ok=True)
    with open(os.path.join(path, "config_model.json"), "w") as f:
        json.dump({"classes": list(classes), "embeddername": embeddername, "digits_results": digits_results}, f)
    if graph:
        with open(os.path.join(path, "saved_model.pb"), "wb") as f:
            f.write(saved_model_bytes(widths, acts, model, layers[0][0].shape[0], faults,
                                      DT_DOUBLE if "float64_graph" in faults else DT_FLOAT))
    rng = np.random.default_rng(seed + 7919)
    dt = np.float64 if f64 else np.float32
    tensors: List[Tuple[str, np.ndarray]] = [("optimizer/_iterations/.ATTRIBUTES/VARIABLE_VALUE", np.array(1234, np.int64)),
                                             ("optimizer/_learning_rate/.ATTRIBUTES/VARIABLE_VALUE", np.array(1e-3, np.float32))]
    slot = 1
    for k, (kern, bias, _) in enumerate(layers):
        tensors.append((f"layer_with_weights-{k}/kernel/.ATTRIBUTES/VARIABLE_VALUE", np.asarray(kern, dt)))
        tensors.append((f"layer_with_weights-{k}/bias/.ATTRIBUTES/VARIABLE_VALUE", np.asarray(bias, dt)))
        for arr in (kern, kern, bias, bias):       # Adam's m and v of each variable: same shapes, other values
            tensors.append((f"optimizer/_variables/{slot}/.ATTRIBUTES/VARIABLE_VALUE",
                            rng.standard_normal(np.shape(arr)).astype(dt)))
            slot += 1
    index, data = bundle_bytes(tensors)
    with open(os.path.join(path, "variables", "variables.index"), "wb") as f:
        f.write(index)
    with open(os.path.join(path, "variables", "variables.data-00000-of-00001"), "wb") as f:
        f.write(data)
    with open(os.path.join(path, "tests", "metrics.csv"), "w") as f:
        f.write(metrics if metrics is not None else default_metrics())
    return path


def write_ensemble_dir(path: str, members, classes: Sequence[str], combine: str = "mean", link: Optional[str] = None,
                       embeddername: str = "yamnet_k2", digits_results: int = 2, metrics: Optional[str] = None) -> str:
    """An ensemble's model directory (``weights.read_ensemble_dir``): ``members`` = {name: layers as ``write_model_dir`` takes
    them}, each written as an ordinary model directory ``members/<name>/``; ``config_model.json`` carries the usual keys and
    ``"ensemble": {"combine", "link", "members"}``; ``tests/metrics.csv`` is the ensemble's own.  No ``variables/`` at the top."""
    os.makedirs(os.path.join(path, "tests"), exist_ok=True)
    for name, layers in members.items():
        write_model_dir(os.path.join(path, "members", name), layers, classes=classes, embeddername=embeddername,
                        digits_results=digits_results, metrics=metrics)
    with open(os.path.join(path, "config_model.json"), "w") as f:
        json.dump({"classes": list(classes), "embeddername": embeddername, "digits_results": digits_results,
                   "ensemble": {"combine": combine, "link": link, "members": list(members)}}, f)
    with open(os.path.join(path, "tests", "metrics.csv"), "w") as f:
        f.write(metrics if metrics is not None else default_metrics())
    return path


# the stacks the tests and tools/head_bench.py use: name -> (widths, activations)
EXAMPLE_STACKS = {
    "relu_256_13": ([256, 13], ["relu", "linear"]),
    "tanh_relu_100_37_5": ([100, 37, 5], ["tanh", "relu", "linear"]),
    "sigmoid_521": ([521], ["sigmoid"]),
    "softmax_64_10": ([64, 10], ["relu", "softmax"]),
}


MODEL_PY = '''"""{name} on the MI355X engine: the dense stack beside this file, loaded by buzzdetect_amd.weights.load_head."""
from src.inference import hip_model


class Model(hip_model.HipModel):
    modelname = "{name}"
    embeddername = "{embedder}"
    digits_results = {digits}
'''


def write_model_py(path: str, name: str, embeddername: str = "yamnet_k2", digits_results: int = 2) -> str:
    """The plugin file a user puts beside the weights: a HipModel subclass with three class attributes."""
    out = os.path.join(path, "model.py")
    with open(out, "w") as f:
        f.write(MODEL_PY.format(name=name, embedder=embeddername, digits=digits_results))
    return out
