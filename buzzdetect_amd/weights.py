"""Weights for the analyze hot path, kept in the reference's own on-disk layout.

The YAMNet embedder weights are one flat little-endian f32 blob with exactly the
byte layout of the reference TensorBundle payload
(``embedders/yamnet_k2/models/yamnet_wholehop/variables/variables.data-00000-of-00001``,
12 869 376 B; table in ``data/embedder_manifest.json``): conv1 kernel ``[3,3,1,32]``
then its BN ``beta / moving_mean / moving_variance``; then for each of the 13
separable layers (``embedders/yamnet/yamnet.py:77-93``) depthwise kernel
``[3,3,C,1]``, its BN triple, pointwise kernel ``[1,1,Cin,Cout]``, its BN triple.
The C-ABI (``include/buzzdetect_hip.h``) takes that blob unchanged and folds the
BatchNorms itself, so a user who owns the real file can hand it straight in.

That file is NOT part of the reference checkout (``.MISSING_LARGE_BLOBS``).  ``load_embedder_blob`` looks for it
where the reference loads its SavedModel - next to the embedder plugin (``embedders/yamnet_k2/embedder.py:14-24``:
``models/yamnet_wholehop`` / ``models/yamnet_halfhop``; ``embedders/yamnet/embedder.py:25-31``: beside ``embedder.py``) -
then in ``BUZZDETECT_YAMNET_VARIABLES``, and FAILS when there is none, as the reference does when its model directory is
missing.  ``synthetic_embedder_blob`` (seeded stand-ins in the same layout) is used only on an explicit opt-in -
``synthetic=True`` or ``BUZZDETECT_SYNTHETIC_WEIGHTS=1``, which the tests, ``bench.py`` and ``smoke()`` set - and says
so with a WARNING on logger ``buzzdetect``: result files written with it are noise in the reference's format.
"""
from __future__ import annotations

import json
import logging
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

DATA_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")

# (stride, filters) of the 14 layers, embedders/yamnet/yamnet.py:77-93
LAYER_DEFS: Tuple[Tuple[int, int], ...] = (
    (2, 32), (1, 64), (2, 128), (1, 128), (2, 256), (1, 256), (2, 512),
    (1, 512), (1, 512), (1, 512), (1, 512), (1, 512), (2, 1024), (1, 1024),
)
EMBEDDER_BLOB_FLOATS = 3_217_344
BN_EPSILON = 1e-4  # embedders/yamnet/params.py:48
SYNTHETIC_SEED = 20260723


def manifest() -> dict:
    with open(os.path.join(DATA_DIR, "embedder_manifest.json")) as f:
        return json.load(f)


def blob_table() -> List[Tuple[str, Tuple[int, ...], int]]:
    """(name, shape, float offset) of every embedder tensor, in blob order."""
    return [(t["name"], tuple(t["shape"]), t["offset"] // 4) for t in manifest()["tensors"]]


def expected_table() -> List[Tuple[str, Tuple[int, ...], int]]:
    """The same table derived from LAYER_DEFS alone (what the C++ side assumes)."""
    out = []
    off = 0

    def add(name, shape):
        nonlocal off
        out.append((name, shape, off))
        n = 1
        for d in shape:
            n *= d
        off += n

    def bn(k, c):
        for part in ("beta", "moving_mean", "moving_variance"):
            add(f"layer_with_weights-{k}/{part}", (c,))

    add("layer_with_weights-0/kernel", (3, 3, 1, LAYER_DEFS[0][1]))
    bn(1, LAYER_DEFS[0][1])
    cin = LAYER_DEFS[0][1]
    k = 2
    for _, cout in LAYER_DEFS[1:]:
        add(f"layer_with_weights-{k}/depthwise_kernel", (3, 3, cin, 1))
        bn(k + 1, cin)
        add(f"layer_with_weights-{k + 2}/kernel", (1, 1, cin, cout))
        bn(k + 3, cout)
        k += 4
        cin = cout
    return out


def synthetic_embedder_blob(seed: int = SYNTHETIC_SEED) -> np.ndarray:
    """Seeded stand-in weights in the reference blob layout:
    He-normal kernels, BN mean~N(0,0.1), var~U(0.5,1.5), beta~N(0,0.1)."""
    rng = np.random.default_rng(seed)
    blob = np.empty(EMBEDDER_BLOB_FLOATS, dtype=np.float32)
    for name, shape, off in expected_table():
        n = int(np.prod(shape))
        leaf = name.rsplit("/", 1)[1]
        if leaf == "kernel":
            fan_in = shape[0] * shape[1] * shape[2]
            v = rng.standard_normal(n) * np.sqrt(2.0 / fan_in)
        elif leaf == "depthwise_kernel":
            v = rng.standard_normal(n) * np.sqrt(2.0 / (shape[0] * shape[1]))
        elif leaf == "moving_variance":
            v = rng.uniform(0.5, 1.5, n)
        else:  # beta, moving_mean
            v = rng.standard_normal(n) * 0.1
        blob[off:off + n] = v.astype(np.float32)
    return blob


VARIABLES_DATA = "variables.data-00000-of-00001"
VARIABLES_ENV = "BUZZDETECT_YAMNET_VARIABLES"
SYNTHETIC_ENV = "BUZZDETECT_SYNTHETIC_WEIGHTS"
PACKAGED_OVERLAY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin")
_log = logging.getLogger("buzzdetect")


def plugin_variables(plugin_dir: str, engine_embedder: str, framehop_prop=None) -> List[str]:
    """Where the embedder weights sit relative to an embedder plugin's directory, in the reference's own layout.

    ``yamnet_k2`` (embedders/yamnet_k2/embedder.py:14-24): ``models/yamnet_wholehop`` for framehop_prop 1,
    ``models/yamnet_halfhop`` for 0.5 (the two SavedModels hold the same variables; without a hop both are tried);
    ``yamnet`` (embedders/yamnet/embedder.py:25-31 loads ``yamnet.keras`` beside the plugin, an HDF5 archive this
    package cannot read without h5py): the TensorBundle of the same weights the checkout keeps beside it,
    ``variables/variables.data-00000-of-00001``."""
    if engine_embedder == "yamnet_k2":
        subs = {1: ("yamnet_wholehop",), 0.5: ("yamnet_halfhop",)}.get(framehop_prop, ("yamnet_wholehop", "yamnet_halfhop"))
        return [os.path.join(plugin_dir, "models", sub, "variables", VARIABLES_DATA) for sub in subs]
    return [os.path.join(plugin_dir, "variables", VARIABLES_DATA)]


def default_candidates(engine_embedder: str, framehop_prop=None) -> List[str]:
    """Plugin directories a bare ``HipEngine()`` / ``analyze()`` looks in: ``embedders/<name>`` under the working directory
    (how buzzdetect resolves plugins, src/config.py:23), then the overlay shipped inside this package."""
    out: List[str] = []
    for root in (os.getcwd(), PACKAGED_OVERLAY):
        for c in plugin_variables(os.path.join(root, "embedders", engine_embedder), engine_embedder, framehop_prop):
            if c not in out:
                out.append(c)
    return out


RAW_TAIL_MAX = 1 << 16      # bytes a data shard may carry behind the 54 tensors (the saved object graph)


def read_variables(path: str) -> np.ndarray:
    """The embedder blob from a ``variables.data-00000-of-00001``.  With its ``variables.index`` beside it every tensor is
    looked up by name and checked (shape, float32) and the blob is assembled in the order the C ABI expects, whatever order
    the file keeps; without one the file must BE that layout."""
    index_path = os.path.join(os.path.dirname(path), "variables.index")
    if os.path.exists(index_path):
        from . import artifacts
        index = artifacts.read_bundle_index(index_path)
        blob = np.empty(EMBEDDER_BLOB_FLOATS, dtype=np.float32)
        for name, shape, off in expected_table():
            key = name + "/.ATTRIBUTES/VARIABLE_VALUE"
            entry = index.get(key) or index.get(name)
            if entry is None:
                raise ValueError(f"{index_path}: no tensor {name}")
            if tuple(entry.shape) != tuple(shape) or entry.dtype != 1:
                raise ValueError(f"{index_path}: {name} is {entry.shape} dtype {entry.dtype}, expected float32 {shape}")
            blob[off:off + entry.count] = artifacts.read_bundle_tensor(path, entry).reshape(-1)
        return blob
    # No index: the file is taken to BE the blob in the C ABI's order.  That is an assumption about bytes nobody named, so it
    # is said out loud and checked as far as the layout allows: the size is the payload plus at most a small object-graph
    # tail (a TensorBundle data shard of this model is 12 869 376 bytes + < 64 KiB), every value is finite, and the slices
    # that must be BatchNorm moving variances are all positive - an unrelated or re-ordered bundle fails that at once.
    size = os.path.getsize(path)
    need = EMBEDDER_BLOB_FLOATS * 4
    if size < need or size > need + RAW_TAIL_MAX:
        raise ValueError(f"{path}: {size} bytes without a variables.index beside it; a raw embedder payload is {need} bytes "
                         f"(+ at most {RAW_TAIL_MAX} of object graph)")
    raw = np.fromfile(path, dtype="<f4", count=EMBEDDER_BLOB_FLOATS).astype(np.float32)
    if not np.isfinite(raw).all():
        raise ValueError(f"{path}: non-finite values where the embedder weights should be (no variables.index to look tensors up by)")
    for name, shape, off in expected_table():
        if name.endswith("moving_variance"):
            n = int(np.prod(shape))
            if not (raw[off:off + n] > 0).all():
                raise ValueError(f"{path}: the slice that should be {name} is not all positive - this file is not the embedder "
                                 f"payload in blob order (put its variables.index beside it)")
    _log.warning("embedder weights: %s has no variables.index beside it; read as the raw payload in blob order "
                 "(size, finiteness and BatchNorm-variance slices checked)", path)
    return raw


def synthetic_allowed(synthetic: Optional[bool] = None) -> bool:
    if synthetic is not None:
        return bool(synthetic)
    return os.environ.get(SYNTHETIC_ENV, "").strip().lower() in ("1", "true", "yes")


def load_embedder_blob(path: Optional[str] = None, candidates=(), synthetic: Optional[bool] = None) -> np.ndarray:
    """The embedder weights, in this order: ``path`` (must exist); the first of ``candidates`` that exists (the plugin's
    own directory, ``plugin_variables``); ``$BUZZDETECT_YAMNET_VARIABLES``; seeded synthetic weights ONLY when opted in
    (``synthetic=True`` or ``BUZZDETECT_SYNTHETIC_WEIGHTS=1``), with a WARNING.  Otherwise ``FileNotFoundError`` naming
    every place looked at - never a silent fallback."""
    if path:
        return read_variables(path)
    tried = []
    for c in candidates:
        tried.append(c)
        if os.path.exists(c):
            _log.info(f"embedder weights: {c}")
            return read_variables(c)
    env = os.environ.get(VARIABLES_ENV)
    if env:
        _log.info(f"embedder weights: {env} (${VARIABLES_ENV})")
        return read_variables(env)
    if synthetic_allowed(synthetic):
        _log.warning("SYNTHETIC embedder weights (seeded random stand-ins, seed %d): no %s was found and synthetic weights "
                     "were asked for (synthetic=True or %s=1).  Results are NOT YAMNet's - fit for tests and throughput "
                     "measurements only.", SYNTHETIC_SEED, VARIABLES_DATA, SYNTHETIC_ENV)
        return synthetic_embedder_blob()
    raise FileNotFoundError(
        "YAMNet embedder weights not found.  Looked for " + ", ".join(tried or ["(no plugin directory given)"]) +
        f"; ${VARIABLES_ENV} is not set.  Put the checkout's {VARIABLES_DATA} there (the reference loads its SavedModel from "
        f"the same directory), point ${VARIABLES_ENV} at it, or opt in to seeded synthetic weights with {SYNTHETIC_ENV}=1.")


def split_blob(blob: np.ndarray) -> Dict[str, np.ndarray]:
    blob = np.asarray(blob)
    if blob.size != EMBEDDER_BLOB_FLOATS:
        raise ValueError(f"embedder blob has {blob.size} floats, expected {EMBEDDER_BLOB_FLOATS}")
    out = {}
    for name, shape, off in expected_table():
        n = int(np.prod(shape))
        out[name] = blob[off:off + n].reshape(shape)
    return out


def load_mel(embeddername: str = "yamnet_k2") -> np.ndarray:
    """The graph-baked ``[257,64]`` mel matrix (features.py:50-55).  The Keras-3
    ``yamnet`` SavedModel carries a float-noise variant of the yamnet_k2 one."""
    fn = {"yamnet_k2": "mel_yamnet_k2_257x64.f32", "yamnet": "mel_yamnet_keras3_257x64.f32"}[embeddername]
    return np.fromfile(os.path.join(DATA_DIR, fn), dtype="<f4").reshape(257, 64).astype(np.float32)


HEAD_INPUT = 1024           # the embedding a head starts from
HEAD_MAX_LAYERS = 8
HEAD_MAX_WIDTH = 2048
HEAD_FUSED_MAX = 64         # one linear layer up to this width stays on the head fused behind the pool (BD_MAX_CLASSES)
MODELS_ENV = "BUZZDETECT_MODELS_DIR"
PACKAGED_MODEL = "model_general_v3"
ACTIVATION_OPS = {"Relu": "relu", "Sigmoid": "sigmoid", "Tanh": "tanh", "Softmax": "softmax"}
_VALUE = "/.ATTRIBUTES/VARIABLE_VALUE"


class UnsupportedHeadError(ValueError):
    """A model directory was found but its classifier is not a stack this engine runs (1..8 Dense layers from the
    1024-wide embedding, float32, widths 1..2048, linear / ReLU / sigmoid / tanh, softmax last): the message names the
    op, shape or dtype and the file it was read from."""


@dataclass
class HeadWeights:
    """A classifier head: ``layers`` = [(kernel [in, out], bias [out], activation)], in order from the embedding.
    ``kernel`` / ``bias`` are those of a head that is one linear layer (``model_general_v3``)."""
    layers: List[Tuple[np.ndarray, np.ndarray, str]]
    classes: List[str]
    embeddername: str = "yamnet_k2"
    digits_results: int = 2
    metrics_path: Optional[str] = None
    source: str = ""

    def _single(self) -> Tuple[np.ndarray, np.ndarray, str]:
        if len(self.layers) != 1 or self.layers[0][2] != "linear":
            raise AttributeError("kernel / bias exist for a head of one linear layer; this one is a stack (see .layers)")
        return self.layers[0]

    @property
    def kernel(self) -> np.ndarray:
        return self._single()[0]

    @property
    def bias(self) -> np.ndarray:
        return self._single()[1]

    @property
    def fused(self) -> bool:
        """Does this head run on the kernel fused behind the pool (one linear layer of at most 64 outputs)?"""
        return len(self.layers) == 1 and self.layers[0][2] == "linear" and self.layers[0][0].shape[1] <= HEAD_FUSED_MAX


ENSEMBLE_COMBINES = ("mean", "mean_probability")
ENSEMBLE_LINKS = ("softmax", "sigmoid")


@dataclass
class EnsembleWeights:
    """An ensemble of heads over one embedder (include/buzzdetect_ensemble.h): the ordered ``members`` = {name: HeadWeights},
    reduced on the device to ONE row of ``len(classes)`` logits per window.  ``combine`` = "mean" (the float32 mean of the
    members' outputs, any common last activation; ``link`` None) or "mean_probability" (soft voting over members whose last
    layer is linear, returned in the domain thresholds are taken in: ``link`` = "softmax" gives the log of the mean softmax,
    "sigmoid" the logit of the mean sigmoid).  Everything else is what a ``HeadWeights`` carries, so ``analyze`` and the
    drop-in model treat it as an ordinary model."""
    members: "Dict[str, HeadWeights]"
    combine: str
    link: Optional[str]
    classes: List[str]
    embeddername: str = "yamnet_k2"
    digits_results: int = 2
    metrics_path: Optional[str] = None
    source: str = ""

    fused = False               # never the head fused behind the pool: its members run as a set


def check_ensemble(ens: EnsembleWeights, where: str = "ensemble") -> None:
    """What ``bd_ensemble_attach`` would refuse about one ensemble, and what the library cannot see (classes, embedders),
    said with the members' names before any device work (``UnsupportedHeadError``; ``where`` names the file or model)."""
    if ens.combine not in ENSEMBLE_COMBINES:
        raise UnsupportedHeadError(f"{where}: unknown combine {ens.combine!r}; an ensemble combines by " + " or ".join(ENSEMBLE_COMBINES))
    if ens.combine == "mean" and ens.link is not None:
        raise UnsupportedHeadError(f'{where}: link {ens.link!r} goes with combine "mean_probability" only; "mean" takes null')
    if ens.combine == "mean_probability" and ens.link not in ENSEMBLE_LINKS:
        raise UnsupportedHeadError(f'{where}: combine "mean_probability" needs link "softmax" or "sigmoid", not {ens.link!r}')
    if not 1 <= len(ens.members) <= HEADSET_MAX_MEMBERS:
        raise UnsupportedHeadError(f"{where}: an ensemble has 1..{HEADSET_MAX_MEMBERS} members, not {len(ens.members)}")
    first_name, first = next(iter(ens.members.items()))
    for name, head in ens.members.items():
        if isinstance(head, EnsembleWeights):
            raise UnsupportedHeadError(f"{where}: member {name!r} is an ensemble itself; ensembles do not nest")
        if list(head.classes) != list(ens.classes):
            raise UnsupportedHeadError(f"{where}: member {name!r} has classes {list(head.classes)}, the ensemble {list(ens.classes)}")
        if head.embeddername != ens.embeddername:
            raise UnsupportedHeadError(f"{where}: member {name!r} is on embedder {head.embeddername!r}, the ensemble on "
                                       f"{ens.embeddername!r}")
        n = int(head.layers[-1][0].shape[1])
        if n != len(ens.classes):
            raise UnsupportedHeadError(f"{where}: member {name!r} gives {n} outputs for {len(ens.classes)} classes")
        if head.layers[-1][2] != first.layers[-1][2]:
            raise UnsupportedHeadError(f"{where}: member {name!r} ends in {head.layers[-1][2]!r}, member {first_name!r} in "
                                       f"{first.layers[-1][2]!r}; the members of an ensemble share their last activation")
        if ens.combine == "mean_probability" and head.layers[-1][2] != "linear":
            raise UnsupportedHeadError(f'{where}: combine "mean_probability" takes members whose last layer is linear (it applies '
                                       f"the {ens.link} itself); member {name!r} ends in {head.layers[-1][2]!r}")


def expand_head_set(members: dict) -> "Dict[str, HeadWeights]":
    """The heads the library runs for ``members`` = {name: HeadWeights or EnsembleWeights}, in its order: a plain model under
    its own name, an ensemble's members - contiguous - as ``"<name>/<member>"``."""
    out = {}
    for name, head in members.items():
        if isinstance(head, EnsembleWeights):
            for m, h in head.members.items():
                out[f"{name}/{m}"] = h
        else:
            out[name] = head
    return out


HEADSET_MAX_MEMBERS = 64    # members of a set of heads (BD_HEADSET_MAX_MEMBERS)
HEADSET_ROW = 2048          # what the hidden activations of one depth of a set may take together, each width rounded up to 32


def load_head_set(names, models_dir: Optional[str] = None) -> "Dict[str, HeadWeights]":
    """The members of a set of heads by name, in the order given (``load_head`` each): ``{name: HeadWeights}``.  An empty list
    and a name given twice are refused with ``ValueError`` before anything is read."""
    names = list(names)
    if not names:
        raise ValueError("a set of heads needs at least one model name (the list is empty)")
    twice = sorted({n for n in names if names.count(n) > 1})
    if twice:
        raise ValueError(f"a set of heads names every model once; given twice: {', '.join(twice)}")
    return {n: load_head(n, models_dir) for n in names}


def check_head_set(members: "Dict[str, HeadWeights]") -> "Dict[str, slice]":
    """What ``bd_headset_attach`` would refuse, said with the models' names and before any device work (``ValueError``):
    no member or more than 64; members on different embedders; more than 2048 outputs in all; for some depth, more than 2048
    floats of hidden activations (the widths, each rounded up to 32, of the layers at that depth whose output is not the
    member's own - hidden layers and a last layer in front of a softmax; members of one linear layer of at most 64 outputs run
    on the fused kernel and take none).  Returns ``{name: slice}``, every member's columns of the logits."""
    if not members:
        raise ValueError("a set of heads needs at least one model (none given)")
    if any(isinstance(h, EnsembleWeights) for h in members.values()):
        return _check_units(members)
    if len(members) > HEADSET_MAX_MEMBERS:
        raise ValueError(f"a set of heads takes at most {HEADSET_MAX_MEMBERS} models, not {len(members)}")
    first_name, first = next(iter(members.items()))
    for name, head in members.items():
        if head.embeddername != first.embeddername:
            raise ValueError(f"the models of a set share one embedder: {first_name!r} is on {first.embeddername!r}, "
                             f"{name!r} on {head.embeddername!r}")
    columns, at = {}, 0
    for name, head in members.items():
        n = int(head.layers[-1][0].shape[1])
        if n != len(head.classes):
            raise ValueError(f"model {name!r}: {len(head.classes)} classes, but its last layer gives {n} outputs")
        columns[name] = slice(at, at + n)
        at += n
    if at > HEAD_MAX_WIDTH:
        raise ValueError(f"the models' outputs sum to {at}, more than {HEAD_MAX_WIDTH}: "
                         + ", ".join(f"{n} {c.stop - c.start}" for n, c in columns.items()))
    stacks = {n: h for n, h in members.items() if not h.fused}
    for d in range(max((len(h.layers) for h in stacks.values()), default=0)):
        took = {n: (int(h.layers[d][0].shape[1]) + 31) // 32 * 32 for n, h in stacks.items()
                if d < len(h.layers) and (d + 1 < len(h.layers) or h.layers[d][2] == "softmax")}
        if sum(took.values()) > HEADSET_ROW:
            raise ValueError(f"depth {d}: the hidden widths (each rounded up to 32) sum to {sum(took.values())}, more than "
                             f"{HEADSET_ROW}: " + ", ".join(f"{n} {w}" for n, w in took.items()))
    return columns


def _check_units(units: dict) -> "Dict[str, slice]":
    """``check_head_set`` where some values are ``EnsembleWeights``: every ensemble is checked on its own, the library's limits
    (64 members, 2048 outputs, the per-depth rule) apply to the underlying members (``expand_head_set``, named
    ``"<name>/<member>"``), and the columns returned are the PUBLIC ones - an ensemble takes ``len(classes)``, once."""
    first_name, first = next(iter(units.items()))
    for name, head in units.items():
        if isinstance(head, EnsembleWeights):
            check_ensemble(head, f"model {name!r}")
        if head.embeddername != first.embeddername:
            raise ValueError(f"the models of a set share one embedder: {first_name!r} is on {first.embeddername!r}, "
                             f"{name!r} on {head.embeddername!r}")
    check_head_set(expand_head_set(units))
    columns, at = {}, 0
    for name, head in units.items():
        n = len(head.classes)
        if not isinstance(head, EnsembleWeights) and n != int(head.layers[-1][0].shape[1]):
            raise ValueError(f"model {name!r}: {n} classes, but its last layer gives {int(head.layers[-1][0].shape[1])} outputs")
        columns[name] = slice(at, at + n)
        at += n
    return columns


def dense_chain(nodes, where: str = "saved_model.pb") -> List[Tuple[str, bool, str]]:
    """The Dense stack of a SavedModel graph, from its decoded nodes (``artifacts.saved_model_nodes``, or a recorded list
    of them): ``[(activation, has_bias, MatMul node name)]`` in order from the input.

    The serving signature's fully inlined body is the library function ``__inference__wrapped_model_*`` (Keras traces the
    whole model into it; the other functions call one another); a graph without one is read from the call-free function
    with the most ``MatMul`` nodes.  From the function's ``Identity`` result the chain is walked back to the input
    through ``MatMul``, ``BiasAdd``, ``Relu`` / ``Sigmoid`` / ``Tanh`` / ``Softmax`` and ``Identity``; anything else is
    refused by name, and the walk must end on an argument of the function that no ``ReadVariableOp`` reads (the input, not
    a variable).  Layers are paired with the bundle by POSITION (``bundle_layer_entries``: the k-th ``MatMul`` from the
    input takes ``layer_with_weights-k``), which is the order Keras numbers a Sequential's layers in; the resource arguments
    of the function carry no variable names to check that against."""
    by_fn: Dict[str, list] = {}
    for n in nodes:
        if n.function:
            by_fn.setdefault(n.function, []).append(n)
    calls = ("PartitionedCall", "StatefulPartitionedCall")
    inlined = {f: ns for f, ns in by_fn.items() if any(n.op == "MatMul" for n in ns) and not any(n.op in calls for n in ns)}
    wrapped = sorted(f for f in inlined if f.startswith("__inference__wrapped_model_"))
    if wrapped:
        fn = wrapped[0]
    elif inlined:
        fn = max(sorted(inlined), key=lambda f: sum(n.op == "MatMul" for n in inlined[f]))
    else:
        raise UnsupportedHeadError(f"{where}: no function with an inlined MatMul chain (not a Dense stack)")
    body = {n.name: n for n in by_fn[fn]}

    def producer(ref: str):
        return body.get(ref.split(":", 1)[0])

    def data_inputs(n):
        return [i for i in n.inputs if not i.startswith("^")]

    outs = [n for n in by_fn[fn] if n.op == "Identity" and n.name == "Identity"]
    if len(outs) != 1:
        raise UnsupportedHeadError(f"{where}: function {fn} has {len(outs)} results, a Dense stack has one")
    node = producer(data_inputs(outs[0])[0])
    layers: List[Tuple[str, bool, str]] = []       # built from the output backwards
    act, bias = "linear", False                    # what has been seen since the last MatMul
    last_ref = data_inputs(outs[0])[0]
    while node is not None:
        ins = data_inputs(node)
        if node.op == "Identity":
            pass
        elif node.op in ACTIVATION_OPS:
            if act != "linear" or bias:
                raise UnsupportedHeadError(f"{where}: {node.op} node {node.name} does not follow a Dense layer's MatMul / BiasAdd")
            act = ACTIVATION_OPS[node.op]
        elif node.op == "BiasAdd":
            if bias:
                raise UnsupportedHeadError(f"{where}: two BiasAdd nodes in a row at {node.name}")
            nxt = producer(ins[0])
            if nxt is None or nxt.op != "MatMul":
                raise UnsupportedHeadError(f"{where}: BiasAdd node {node.name} does not follow a MatMul")
            bias = True
        elif node.op == "MatMul":
            for attr in ("transpose_a", "transpose_b"):
                if node.attrs.get(attr):
                    raise UnsupportedHeadError(f"{where}: MatMul node {node.name} has {attr}=true")
            t = node.attrs.get("T")
            if isinstance(t, dict) and t.get("dtype") not in (None, 1):
                raise UnsupportedHeadError(f"{where}: MatMul node {node.name} has dtype {t.get('dtype')}, not float32 (1)")
            w = producer(ins[1]) if len(ins) > 1 else None
            if w is None or w.op != "ReadVariableOp":
                raise UnsupportedHeadError(f"{where}: the second operand of MatMul node {node.name} is not a variable")
            layers.append((act, bias, node.name))
            act, bias = "linear", False
        else:
            raise UnsupportedHeadError(f"{where}: unsupported op {node.op} (node {node.name}) in the classifier; a head is a "
                                       f"stack of MatMul, BiasAdd, Relu, Sigmoid, Tanh and a final Softmax")
        last_ref = ins[0] if ins else ""
        node = producer(ins[0]) if ins else None
    resources = {i for n in by_fn[fn] if n.op == "ReadVariableOp" for i in n.inputs}
    if not layers or ":" in last_ref or not last_ref or last_ref in resources:
        raise UnsupportedHeadError(f"{where}: the chain of function {fn} starts at {last_ref!r}, not at an input argument")
    if act != "linear" or bias:
        raise UnsupportedHeadError(f"{where}: an activation or BiasAdd sits on the input, before any MatMul")
    layers.reverse()
    if not layers:
        raise UnsupportedHeadError(f"{where}: function {fn} holds no MatMul between its input and its result")
    if len(layers) > HEAD_MAX_LAYERS:
        raise UnsupportedHeadError(f"{where}: {len(layers)} Dense layers, at most {HEAD_MAX_LAYERS} are supported")
    for k, (a, _, name) in enumerate(layers[:-1]):
        if a == "softmax":
            raise UnsupportedHeadError(f"{where}: Softmax on hidden layer {k} ({name}); softmax is supported on the last layer only")
    return layers


def bundle_layer_entries(index: dict, n_layers: int, where: str = "variables.index"):
    """``[(kernel entry, bias entry or None)]`` of Dense layers 0..n_layers-1: the k-th MatMul of the chain takes
    ``layer_with_weights-k/kernel`` and ``/bias`` - by NAME, so optimizer slots of the same shapes are never taken.
    Checks float32, rank, the width limit and that the shapes chain from the 1024-wide embedding."""
    out = []
    width = HEAD_INPUT
    for k in range(n_layers):
        name = f"layer_with_weights-{k}/kernel"
        kern = index.get(name + _VALUE) or index.get(name)
        if kern is None:
            raise UnsupportedHeadError(f"{where}: the graph has {n_layers} Dense layers but there is no tensor {name}")
        bias = index.get(f"layer_with_weights-{k}/bias" + _VALUE) or index.get(f"layer_with_weights-{k}/bias")
        for e in (kern, bias):
            if e is not None and e.dtype != 1:
                raise UnsupportedHeadError(f"{where}: {e.name} has dtype {e.dtype}, not float32 (1)")
        if len(kern.shape) != 2:
            raise UnsupportedHeadError(f"{where}: {kern.name} has shape {tuple(kern.shape)}, a Dense kernel is [in, out]")
        if kern.shape[0] != width:
            raise UnsupportedHeadError(f"{where}: {kern.name} has shape {tuple(kern.shape)} but the layer before it gives "
                                       f"{width} values (shapes must chain from the {HEAD_INPUT}-wide embedding)")
        width = int(kern.shape[1])
        if not 1 <= width <= HEAD_MAX_WIDTH:
            raise UnsupportedHeadError(f"{where}: {kern.name} has width {width}, outside 1..{HEAD_MAX_WIDTH}")
        if bias is not None and tuple(bias.shape) != (width,):
            raise UnsupportedHeadError(f"{where}: {bias.name} has shape {tuple(bias.shape)}, expected ({width},)")
        out.append((kern, bias))
    return out


def read_model_dir(path: str, modelname: str = "") -> HeadWeights:
    """A trained model directory in the reference's layout (``config_model.json``, ``saved_model.pb``, ``variables/``,
    ``tests/metrics.csv``): architecture from the graph, values from the bundle."""
    from . import artifacts
    cfg_path = os.path.join(path, "config_model.json")
    if not os.path.exists(cfg_path):
        raise FileNotFoundError(f"{cfg_path} not found: a model directory holds config_model.json with its classes")
    with open(cfg_path) as f:
        cfg = json.load(f)
    index_path, data_path = artifacts.bundle_paths(path)
    index = artifacts.read_bundle_index(index_path)
    pb = os.path.join(path, "saved_model.pb")
    nodes = None
    if os.path.exists(pb):
        try:
            nodes = artifacts.saved_model_nodes(pb)
        except (ValueError, IndexError, UnicodeDecodeError):
            nodes = None
    if not nodes:
        raise UnsupportedHeadError(f"{pb}: no readable graph beside {index_path}; the bundle holds the Dense layers' values "
                                   f"but not their activations, so the head cannot be built from it alone")
    chain = dense_chain(nodes, pb)
    layers = []
    for (act, has_bias, _), (kern, bias) in zip(chain, bundle_layer_entries(index, len(chain), index_path)):
        k = artifacts.read_bundle_tensor(data_path, kern).astype(np.float32)
        if has_bias and bias is None:
            raise UnsupportedHeadError(f"{index_path}: the graph adds a bias to {kern.name} but the bundle has none")
        b = (artifacts.read_bundle_tensor(data_path, bias).astype(np.float32) if has_bias
             else np.zeros(k.shape[1], dtype=np.float32))
        layers.append((k, b, act))
    classes = list(cfg["classes"])
    if len(classes) != layers[-1][0].shape[1]:
        raise UnsupportedHeadError(f"{cfg_path}: {len(classes)} classes but the last layer of {pb} has width "
                                   f"{layers[-1][0].shape[1]}")
    metrics = os.path.join(path, "tests", "metrics.csv")
    if not os.path.exists(metrics):
        packaged = os.path.join(DATA_DIR, f"metrics_{modelname}.csv")
        metrics = packaged if modelname and os.path.exists(packaged) else None
    return HeadWeights(layers, classes, cfg.get("embeddername", "yamnet_k2"), int(cfg.get("digits_results", 2)), metrics, path)


def read_ensemble_dir(path: str, modelname: str = "") -> EnsembleWeights:
    """An ensemble's model directory: ``config_model.json`` with the usual keys and ``"ensemble": {"combine", "link",
    "members": [...]}``, every member an ordinary model directory ``members/<member>/`` (``read_model_dir``), the ensemble's
    own ``tests/metrics.csv``.  No ``variables/`` of its own."""
    cfg_path = os.path.join(path, "config_model.json")
    with open(cfg_path) as f:
        cfg = json.load(f)
    spec = cfg.get("ensemble")
    if not isinstance(spec, dict) or not isinstance(spec.get("members"), list) or "classes" not in cfg:
        raise UnsupportedHeadError(f'{cfg_path}: "ensemble" must be {{"combine", "link", "members": [names]}} beside "classes"')
    names = [str(n) for n in spec["members"]]
    twice = sorted({n for n in names if names.count(n) > 1})
    if twice:
        raise UnsupportedHeadError(f"{cfg_path}: members named twice: {', '.join(twice)}")
    if not 1 <= len(names) <= HEADSET_MAX_MEMBERS:
        raise UnsupportedHeadError(f"{cfg_path}: an ensemble has 1..{HEADSET_MAX_MEMBERS} members, not {len(names)}")
    members = {}
    for name in names:
        sub = os.path.join(path, "members", name)
        sub_cfg = os.path.join(sub, "config_model.json")
        if os.path.basename(name) != name or not os.path.isdir(sub) or not os.path.exists(sub_cfg):
            raise UnsupportedHeadError(f"{cfg_path}: member {name!r} has no model directory {sub} (with config_model.json)")
        with open(sub_cfg) as f:
            if "ensemble" in json.load(f):
                raise UnsupportedHeadError(f"{sub_cfg}: member {name!r} is an ensemble itself; ensembles do not nest")
        members[name] = read_model_dir(sub, name)
    metrics = os.path.join(path, "tests", "metrics.csv")
    ens = EnsembleWeights(members, spec.get("combine"), spec.get("link"), list(cfg["classes"]), cfg.get("embeddername", "yamnet_k2"),
                          int(cfg.get("digits_results", 2)), metrics if os.path.exists(metrics) else None, path)
    check_ensemble(ens, cfg_path)
    return ens


def _is_ensemble_dir(path: str) -> bool:
    try:
        with open(os.path.join(path, "config_model.json")) as f:
            cfg = json.load(f)
    except (OSError, ValueError):
        return False
    return isinstance(cfg, dict) and "ensemble" in cfg


def model_candidates(modelname: str, models_dir: Optional[str] = None) -> List[str]:
    """Directories ``load_head`` looks at, in order: ``models_dir/<modelname>`` alone when ``models_dir`` is given;
    else ``models/<modelname>`` under the working directory (the reference's ``cfg.DIR_MODELS``),
    ``$BUZZDETECT_MODELS_DIR/<modelname>``, the overlay shipped inside this package."""
    if models_dir is not None:
        return [os.path.join(models_dir, modelname)]
    out = [os.path.join(os.getcwd(), "models", modelname)]
    env = os.environ.get(MODELS_ENV)
    if env:
        out.append(os.path.join(env, modelname))
    out.append(os.path.join(PACKAGED_OVERLAY, "models", modelname))
    return [c for i, c in enumerate(out) if c not in out[:i]]


def _packaged_head(modelname: str) -> HeadWeights:
    with open(os.path.join(DATA_DIR, f"config_{modelname}.json")) as f:
        cfg = json.load(f)
    n = len(cfg["classes"])
    k = np.fromfile(os.path.join(DATA_DIR, f"head_{modelname}_kernel_1024x{n}.f32"), dtype="<f4")
    b = np.fromfile(os.path.join(DATA_DIR, f"head_{modelname}_bias_{n}.f32"), dtype="<f4")
    metrics = os.path.join(DATA_DIR, f"metrics_{modelname}.csv")
    for c in model_candidates(modelname):          # a model directory without weights may still carry its own metrics
        if os.path.exists(os.path.join(c, "tests", "metrics.csv")):
            metrics = os.path.join(c, "tests", "metrics.csv")
            break
    return HeadWeights([(k.reshape(1024, n).astype(np.float32), b.astype(np.float32), "linear")], cfg["classes"],
                       cfg.get("embeddername", "yamnet_k2"), int(cfg.get("digits_results", 2)),
                       metrics if os.path.exists(metrics) else None, DATA_DIR)


def load_head(modelname: str = PACKAGED_MODEL, models_dir: Optional[str] = None) -> HeadWeights:
    """The classifier of ``modelname``: the first of ``model_candidates`` that holds a TensorBundle
    (``variables/variables.index``) is read with ``read_model_dir``; for ``model_general_v3`` alone (and no
    ``models_dir``) the head packaged with this engine (models/model_general_v3/variables, model.py:29) comes last.
    Nothing found: ``FileNotFoundError`` naming every place looked at - never a silent fallback."""
    tried = []
    for c in model_candidates(modelname, models_dir):
        if _is_ensemble_dir(c):          # an ensemble (read_ensemble_dir): its bundles sit under members/
            _log.info(f"classifier ensemble: {c}")
            return read_ensemble_dir(c, modelname)
        if os.path.exists(os.path.join(c, "variables", "variables.index")):
            _log.info(f"classifier head: {c}")
            return read_model_dir(c, modelname)
        tried.append(c + (" (no variables/variables.index)" if os.path.isdir(c) else ""))
    if modelname == PACKAGED_MODEL and models_dir is None:
        return _packaged_head(modelname)
    raise FileNotFoundError(
        f'model "{modelname}" not found.  Looked for ' + ", ".join(tried) +
        (f"; ${MODELS_ENV} is not set" if models_dir is None and not os.environ.get(MODELS_ENV) else "") +
        f".  A model directory holds config_model.json, saved_model.pb and variables/ (tools/modelgen.py writes one); only "
        f"{PACKAGED_MODEL} is packaged with the engine.")
