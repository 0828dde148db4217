"""Cases and NumPy restatements shared by tests/test_dense_domain_host.py and tests/test_dense_domain_gpu.py (a plain module, like
calls_cases.py): dense stacks, sets of heads and ensembles at the limits bd_head_attach, bd_headset_attach and
bd_ensemble_attach accept (include/buzzdetect_head.h, buzzdetect_headset.h, buzzdetect_ensemble.h), each table entry with the
code edge it is there for.

Weights: modeldir.glorot_layers at gain 1, then one gain per layer chosen ON THE CPU from the oracle's embeddings of the tests'
audio (`calibrated_gains`), so that the float64 reference alone puts every layer's largest |pre-activation| at the case's target,
for the first window alone, the first 33 and all 65.  An ordinary case aims at 4: a float32 chain of K terms that sum to about s
errs by about sqrt(K) * 2^-24 * s, 1e-5 for K = 2048 and s = 4, and every further layer passes an incoming error on times the
size of its weights, so the 1e-4 gate says something about a kernel only where float32 arithmetic itself stays well inside it.
That is asserted on the CPU (tests/test_dense_domain_host.py): an ordinary case's float32 chain restatement deviates from float64
by at most a quarter of the gate on the oracle's embeddings (CHAIN_ROOM).  A scaled case drives one layer to about 1e3, or all of
them to about 1e-6, and is held to 8 x the chain's own deviation instead.

Restatements: `stack_f64` (the reference, the one tests/test_head_gpu.py uses) and `stack_f32_chain`, every dot product as the
ascending-k chain in float32 - the yardstick `train_oracle.bound` multiplies by 8."""
import functools
from collections import namedtuple

import numpy as np

from buzzdetect_amd import modeldir, weights as W
from oracle import yamnet_oracle as O

HOP = 15360
AUDIO_SEED = 77
AUDIO_WINDOWS = 1025                      # the tests' audio: a full pass and a ragged pass of one window
WINDOW_COUNTS = (1, 33, 65)               # a ragged 32-row tile; a second 64-row workgroup with one row
ORDINARY = (1.0, 100.0)                   # the precondition of the 1e-4 gate: every layer's max |pre-activation| in here
LOGIT_GATE = 1e-4
DEFAULT_TARGET = 4.0
CHAIN_ROOM = LOGIT_GATE / 4               # what the float32 chain restatement itself may deviate by in an ordinary case

MAX_LAYERS, MAX_WIDTH, MAX_MEMBERS, FUSED_MAX, SET_ROW = (W.HEAD_MAX_LAYERS, W.HEAD_MAX_WIDTH, W.HEADSET_MAX_MEMBERS,
                                                          W.HEAD_FUSED_MAX, W.HEADSET_ROW)


# ---------------------------------------------------------------------------------------------------- audio and embeddings
@functools.lru_cache(maxsize=None)
def audio():
    x = O.synthetic_audio(HOP * AUDIO_WINDOWS + 240, seed=AUDIO_SEED)
    x.setflags(write=False)
    return x


def chunk(windows, first=0):
    """The samples of `windows` windows from window `first` on."""
    return audio()[HOP * first: HOP * (first + windows) + 240]


@functools.lru_cache(maxsize=None)
def oracle_embeddings():
    """The CPU oracle's float32 embeddings of the first 65 windows: what the gains are chosen from."""
    emb = O.embed(chunk(max(WINDOW_COUNTS)), W.synthetic_embedder_blob(), W.load_mel("yamnet_k2"), HOP, 96, np.float32)
    assert emb.shape == (max(WINDOW_COUNTS), 1024) and emb.dtype == np.float32
    emb.setflags(write=False)
    return emb


# ---------------------------------------------------------------------------------------------------- generator
def layers(widths, activations, seed, gains, bias_gains=None):
    """modeldir.glorot_layers at gain 1 with layer i's kernel times gains[i] (and its bias times bias_gains[i]), in float32."""
    assert len(widths) == len(activations) == len(gains)
    bias_gains = [1.0] * len(widths) if bias_gains is None else bias_gains
    out = []
    for (kernel, bias, act), g, bg in zip(modeldir.glorot_layers(widths, activations, seed=seed, gain=1.0), gains, bias_gains):
        out.append((kernel * np.float32(g), bias * np.float32(bg), act))
        assert out[-1][0].dtype == np.float32 and out[-1][1].dtype == np.float32
    return out


def calibrated_gains(widths, activations, seed, targets, emb=None):
    """(gains, bias_gains): layer i's gain puts sqrt(largest |x K| of the first row * largest |x K| of all rows) at targets[i],
    on the float64 stack over `emb` (default: the oracle's embeddings); a bias is scaled down with a target below 1."""
    x = np.asarray(oracle_embeddings() if emb is None else emb, dtype=np.float64)
    gains, bias_gains = [], []
    for (kernel, bias, act), target in zip(modeldir.glorot_layers(widths, activations, seed=seed, gain=1.0), targets):
        p = x @ kernel.astype(np.float64)
        first, whole = np.abs(p[0]).max(), np.abs(p).max()
        assert first > 0, "a dead first row cannot be scaled"
        g, bg = np.float32(target / np.sqrt(first * whole)), np.float32(min(1.0, target))
        gains.append(float(g))
        bias_gains.append(float(bg))
        x = stack_f64(x, [(kernel * g, bias * bg, act)])
    return gains, bias_gains


# ---------------------------------------------------------------------------------------------------- restatements
def stack_f64(emb, layers, taps=None):
    """The stack restated in float64 NumPy: y = act(x W + b) per layer.  `taps`: a list that takes every layer's
    pre-activations."""
    x = np.asarray(emb, dtype=np.float64)
    for kernel, bias, act in layers:
        x = x @ kernel.astype(np.float64) + bias.astype(np.float64)
        if taps is not None:
            taps.append(x)
        if act == "relu":
            x = np.maximum(x, 0.0)
        elif act == "sigmoid":
            with np.errstate(over="ignore"):
                x = 1.0 / (1.0 + np.exp(-x))
        elif act == "tanh":
            x = np.tanh(x)
        elif act == "softmax":
            e = np.exp(x - x.max(axis=1, keepdims=True))
            x = e / e.sum(axis=1, keepdims=True)
        else:
            assert act == "linear"
    return x


def stack_f32_chain(emb, layers):
    """The stack in float32 throughout, every dot product the ascending-k chain acc = acc + a[:, k] * w[k] (no BLAS: a blocked
    sum errs several times less on a 2048-term row than any sequential chain can), then bias, activation and softmax in float32."""
    one = np.float32(1)
    x = np.asarray(emb, dtype=np.float32)
    for kernel, bias, act in layers:
        w = np.asarray(kernel, dtype=np.float32)
        acc = np.zeros((x.shape[0], w.shape[1]), np.float32)
        for k in range(w.shape[0]):
            acc = acc + x[:, k, None] * w[k]
        x = acc + np.asarray(bias, dtype=np.float32)
        if act == "relu":
            x = np.maximum(x, np.float32(0))
        elif act == "sigmoid":
            with np.errstate(over="ignore"):
                x = one / (one + np.exp(-x))
        elif act == "tanh":
            x = np.tanh(x)
        elif act == "softmax":
            e = np.exp(x - x.max(axis=1, keepdims=True))
            x = e / e.sum(axis=1, keepdims=True, dtype=np.float32)
        else:
            assert act == "linear"
        assert x.dtype == np.float32 and acc.dtype == np.float32
    return x


# ---------------------------------------------------------------------------------------------------- stacks
Stack = namedtuple("Stack", "widths acts targets seed why")
STACKS = {}


def stack(name, widths, acts, why, targets=None, seed=None):
    assert name not in STACKS and len(widths) == len(acts)
    targets = [DEFAULT_TARGET] * len(widths) if targets is None else list(targets)
    STACKS[name] = Stack(list(widths), list(acts), targets, 1000 + len(STACKS) if seed is None else seed, why)
    return name


# hidden width h (the layer's N, the next layer's K) and last width n at the 32-column tile edge, the 64-column workgroup edge
# and the smallest K: the selects of dense_tile_walk, the round_up(K, 32) leading dimension, dense_tile_store's column guard
EDGES = [
    stack("h1_n31", [1, 31], ["tanh", "linear"], "K = 1: one live element in a 16-byte load; N = 31"),
    stack("h2_n33", [2, 33], ["sigmoid", "relu"], "K = 2; N = 33: a second tile of one column; relu last"),
    stack("h3_n1", [3, 1], ["tanh", "sigmoid"], "K = 3: below one float4; N = 1; sigmoid last"),
    stack("h4_n63", [4, 63], ["sigmoid", "tanh"], "K = 4: exactly the first lane-half's float4; N = 63; tanh last"),
    stack("h5_n65", [5, 65], ["tanh", "linear"], "K = 5: one element of the second lane-half; N = 65: a second workgroup tile"),
    stack("h8_n32", [8, 32], ["relu", "sigmoid"], "K = 8: one super-step; N = 32"),
    stack("h9_n64", [9, 64], ["sigmoid", "linear"], "K = 9: one element of the second super-step; N = 64"),
    stack("h31_n1", [31, 1], ["relu", "linear"], "K = 31, hidden N = 31; N = 1 linear last"),
    stack("h32_n33", [32, 33], ["tanh", "tanh"], "K = 32: no padding at all; N = 33"),
    stack("h33_n31", [33, 31], ["relu", "relu"], "K = 33: a second group of 32 k with one live element"),
    stack("h63_n65", [63, 65], ["sigmoid", "sigmoid"], "K = 63, hidden N = 63; N = 65 sigmoid last"),
    stack("h64_n63", [64, 63], ["relu", "linear"], "K = 64, hidden N = 64"),
    stack("h65_n64", [65, 64], ["tanh", "relu"], "K = 65, hidden N = 65: a hidden layer over two workgroup tiles"),
]

# one linear layer of at most 64 classes: the fused route of a set (head_set_kernel), the fused head of a lone engine
FUSED = {n: stack(f"lin{n}", [n], ["linear"], f"fused route, {n} classes") for n in (1, 15, 16, 17, 64)}
FUSED["16b"] = stack("lin16b", [16], ["linear"], "fused route, a second member of 16 classes")

# softmax rows: softmax_row strides a row by 64 lanes - one round, exactly one, one column of a second, two and one, 32 rounds
SOFTMAX = [
    stack("sm1", [40, 1], ["relu", "softmax"], "softmax of length 1: 1.0 in every row"),
    stack("sm2", [2], ["softmax"], "softmax of length 2 on a single layer: the row pass reads region 0 of a one-layer stack"),
    stack("sm63", [40, 63], ["tanh", "softmax"], "softmax of length 63: one lane idle"),
    stack("sm64", [33, 64], ["relu", "softmax"], "softmax of length 64: exactly a wave"),
]
DEEP_SM7 = stack("deep7_sm65", [100, 37, 64, 5, 33, 48, 65], ["tanh", "relu", "relu", "tanh", "relu", "sigmoid", "softmax"],
                 "7 layers ending in softmax: the row pass reads region 0; softmax of length 65")
DEEP_SM8 = stack("deep8_sm129", [64, 33, 65, 31, 32, 9, 40, 129],
                 ["relu", "tanh", "relu", "sigmoid", "relu", "tanh", "relu", "softmax"],
                 "8 layers ending in softmax: the row pass reads region 1; softmax of length 129, three rounds")

# depths 1..8 (7 and 8 are the two above)
DEPTHS = [
    stack("d1_sig13", [13], ["sigmoid"], "depth 1 on the stack route: straight from the embeddings to the logits"),
    stack("d2_relu_33_2", [33, 2], ["relu", "linear"], "depth 2", seed=1),
    stack("d3_100_37_5", [100, 37, 5], ["tanh", "relu", "linear"], "depth 3: K off a multiple of 32 at both hidden layers"),
    stack("d4", [48, 33, 17, 4], ["relu", "linear", "tanh", "linear"], "depth 4, a linear hidden layer"),
    stack("d5", [64, 40, 31, 9, 3], ["tanh", "relu", "sigmoid", "tanh", "relu"], "depth 5, relu last"),
    stack("d6", [96, 65, 33, 32, 8, 7], ["relu", "tanh", "relu", "sigmoid", "tanh", "tanh"], "depth 6, tanh last"),
    DEEP_SM7, DEEP_SM8,
]

# the declared maximum: these fill a depth of a set's scratch by themselves and run on engines of their own
WIDE = [
    stack("out2048", [2048], ["sigmoid"], "N = 2048 on the last layer: bd_head_outputs at BD_HEAD_MAX_WIDTH"),
    stack("out2047", [2047], ["tanh"], "N = 2047 on the last layer: the last tile one column short"),
    stack("hid2048", [2048, 2048, 13], ["tanh", "sigmoid", "linear"],
          "K = 2048 and hidden N = 2048 twice: tanh and sigmoid on a 2048-wide hidden layer, rows kHeadSetRow floats apart"),
    stack("hid2047", [2047, 65], ["sigmoid", "linear"],
          "K = 2047: the last 16-byte load of a row straddles a written and a never-written column"),
    stack("sm2048", [64, 2048], ["relu", "softmax"], "softmax of length 2048: 32 rounds per lane, region 2 of a set full"),
    stack("deep8_2048", [2048] * 8, ["relu", "tanh", "relu", "sigmoid", "relu", "tanh", "relu", "linear"],
          "8 layers, all 2048 wide: both scratch regions full at every depth, the largest scratch the engine addresses",
          targets=[DEFAULT_TARGET] * 8),
    stack("deep8_mixed", [2048, 1, 2047, 33, 64, 3, 65, 13], ["relu", "tanh", "sigmoid", "relu", "tanh", "tanh", "relu", "linear"],
          "8 layers whose leading dimension changes at every depth: 2048, 32, 2048, 64, 64, 32, 96"),
]
LONE_ONLY = ("hid2048", "hid2047", "deep8_2048", "deep8_mixed")        # beside anything else they would exceed a set's row

# scale: one layer at about 1e3 (exact 0, 1, +-1; a softmax with one 1.0 among zeros), or everything at about 1e-6
SCALED = [
    stack("big_sigmoid", [64, 33], ["relu", "sigmoid"], "sigmoid at |x| up to 1e3: expf over- and underflows", [DEFAULT_TARGET, 1e3]),
    stack("big_tanh", [33, 65], ["relu", "tanh"], "tanh at |x| up to 1e3: exactly +-1", [DEFAULT_TARGET, 1e3]),
    stack("big_softmax129", [64, 129], ["tanh", "softmax"], "softmax of length 129 over logits 1e3 apart: one 1.0 among zeros",
          [DEFAULT_TARGET, 1e3]),
    stack("big_hidden_tanh", [40, 13], ["tanh", "linear"], "a hidden tanh layer saturated at +-1 feeds the next layer", [1e3, DEFAULT_TARGET]),
    stack("big_hidden_sigmoid", [65, 7], ["sigmoid", "softmax"], "a hidden sigmoid layer saturated at 0 and 1", [1e3, DEFAULT_TARGET]),
    stack("tiny_sigmoid", [33], ["sigmoid"], "sigmoid at |x| about 1e-6: 0.5 and a few ulp", [1e-6]),
    stack("tiny_tanh_linear", [64, 13], ["tanh", "linear"], "tanh at |x| about 1e-6: tanh(x) = x", [1e-6, 1e-6]),
    stack("tiny_softmax65", [40, 65], ["relu", "softmax"], "softmax of length 65 over logits 1e-6 apart: 1 / 65 everywhere",
          [1e-6, 1e-6]),
]

# 64 x (1024 -> 32 -> 32): 64 members, outputs 64 * 32 = 2048, hidden widths of depth 0 64 * 32 = 2048 - three limits at once
FULL64 = [stack(f"full64_{i:02d}", [32, 32], [("relu", "tanh", "sigmoid")[i % 3], ("linear", "sigmoid", "relu", "tanh")[i % 4]],
                "one of 64 members: dense_set_kernel's tile table at 64 layers per depth") for i in range(64)]
# 16 x (1024 -> 128 -> 8 -> 3): depth 0 takes 16 * 128 = 2048 floats, depth 1 16 * 32 = 512
HIDDEN_FULL = [stack(f"hfull_{i:02d}", [128, 8, 3], ["relu", "tanh", "linear"], "one of 16 members whose first hidden layers fill a row")
               for i in range(16)]
# ensembles
ENS13 = [stack(f"ens13_{i:02d}", [13], ["linear"], "one of 64 fused members under one output") for i in range(64)]
ENS1 = [stack(f"ens1_{i}", [1], ["linear"], "member of an output of width 1") for i in range(3)]
ENS64 = [stack(f"ens64_{i}", [64], ["linear"], "member of an output of width 64: one round of the combine's lanes") for i in range(2)]
ENS65 = [stack(f"ens65_{i}", [65], ["linear"], "member of an output of width 65: a second round, on the stack route") for i in range(4)]
ENS129 = [stack(f"ens129_{i}", [48, 129], ["relu", "softmax"], "softmax member of a mean over 129 columns") for i in range(2)]
ENS1024 = [stack(f"ens1024_{i}", [1024], ["linear"], "member of an output of width 1024: 2 x 1024 = every wide column") for i in range(2)]


def is_scaled(name):
    lo, hi = ORDINARY
    return any(not lo <= t <= hi for t in STACKS[name].targets)


def is_fused(name):
    c = STACKS[name]
    return len(c.widths) == 1 and c.acts[0] == "linear" and c.widths[0] <= FUSED_MAX


@functools.lru_cache(maxsize=None)
def stack_layers(name):
    c = STACKS[name]
    gains, bias_gains = calibrated_gains(c.widths, c.acts, c.seed, c.targets)
    return layers(c.widths, c.acts, c.seed, gains, bias_gains)


def head(name):
    return W.HeadWeights(stack_layers(name), [f"c{i}" for i in range(STACKS[name].widths[-1])])


# ---------------------------------------------------------------------------------------------------- sets
Set = namedtuple("Set", "members why outputs hidden n_members fused")     # the limits a set is there to touch, or None
SETS = {}


def interleave(stacks, fused):
    """Fused members spread between stack-route members, never first or last."""
    out, fused = [], list(fused)
    for i, s in enumerate(stacks):
        out.append(s)
        if fused and i + 1 < len(stacks):
            out.append(fused.pop(0))
    assert not fused
    return out


def fused_members(*sizes):
    return [FUSED[s] for s in sizes]


SETS["edges"] = Set(interleave(EDGES, fused_members(1, 15, 16, 17, 64, "16b")),
                    "every tile-edge stack; 129 fused classes: a third group of one class; fused members between stacks",
                    None, None, None, 129)
SETS["softmaxes"] = Set(interleave(SOFTMAX + [DEEP_SM7, DEEP_SM8], fused_members(15, 17, 16, "16b", 64)),
                        "softmax rows of 1, 2, 63, 64, 65 and 129 packed in region 2; 128 fused classes: two full groups",
                        None, None, None, 128)
SETS["depths"] = Set(interleave(DEPTHS, fused_members(64, 1)),
                     "members of depths 1..8 in one set: a depth's launch with members that ended before it; 65 fused classes",
                     None, None, None, 65)
SETS["scaled"] = Set(interleave(SCALED, fused_members(64)), "the scaled stacks side by side; 64 fused classes: one full group",
                     None, None, None, 64)
SETS["full64"] = Set(FULL64, "64 members, 2048 outputs, 2048 hidden floats at depth 0", MAX_WIDTH, (0, SET_ROW), MAX_MEMBERS, 0)
SETS["hidden_full"] = Set(HIDDEN_FULL, "depth 0 full (16 x 128) while depth 1 stays small (16 x 32)", None, (0, SET_ROW), None, 0)
SETS["out2048"] = Set(["out2048"], "one member of 2048 outputs: a set's logits row at its widest", MAX_WIDTH, None, None, 0)
SETS["out2047_lin1"] = Set(["out2047", FUSED[1]], "2047 + 1 outputs: a fused column behind 2047 stack columns", MAX_WIDTH, None,
                           None, 1)
SETS["sm2048"] = Set(["sm2048"], "a softmax over 2048 columns: region 2 full", MAX_WIDTH, (1, SET_ROW), None, 0)
REVERSED = ("edges", "softmaxes", "depths", "scaled", "full64", "out2047_lin1")   # also attached in reverse order


def set_outputs(members):
    return sum(STACKS[m].widths[-1] for m in members)


def set_hidden(members):
    """Per depth, what bd_headset_attach adds up: the widths, each rounded up to 32, of the stack-route layers that are hidden or
    stand in front of a softmax."""
    sums = {}
    for m in members:
        c = STACKS[m]
        if is_fused(m):
            continue
        for d, (w, a) in enumerate(zip(c.widths, c.acts)):
            if d + 1 < len(c.widths) or a == "softmax":
                sums[d] = sums.get(d, 0) + (w + 31) // 32 * 32
    return sums


def set_fused_classes(members):
    return sum(STACKS[m].widths[-1] for m in members if is_fused(m))


# ---------------------------------------------------------------------------------------------------- ensembles
# name -> [(unit, members, combine, link)]; a unit with combine None is a plain model passed through
Ensemble = namedtuple("Ensemble", "units why")
ENSEMBLES = {
    "k64_mean": Ensemble([("all", ENS13, "mean", None)], "one output over 64 members"),
    "k64_softmax": Ensemble([("all", ENS13, "mean_probability", "softmax")],
                            "one output over 64 members, soft vote: every per-member LDS slot of the combine kernel in use"),
    "k64_sigmoid": Ensemble([("all", ENS13, "mean_probability", "sigmoid")], "one output over 64 members, sigmoid link"),
    "side_by_side": Ensemble([("w1_mean", ENS1, "mean", None),
                              ("w64_softmax", ENS64, "mean_probability", "softmax"),
                              ("through", ["d2_relu_33_2"], None, None),
                              ("w65_softmax", ENS65[:2], "mean_probability", "softmax"),
                              ("w65_sigmoid", ENS65[2:], "mean_probability", "sigmoid"),
                              ("w129_mean", ENS129, "mean", None)],
                             "widths 1, 64, 65 and 129; mean, both links and a pass-through side by side; the soft vote over rows "
                             "longer than 64"),
    "w1024_softmax": Ensemble([("all", ENS1024, "mean_probability", "softmax")],
                              "width 1024 with k = 2: the wide row at 2048 columns, 16 rounds of the soft vote's lanes"),
    "w1024_mean": Ensemble([("all", ENS1024, "mean", None)], "width 1024 with k = 2, mean"),
}


def ensemble_members(name):
    return [m for _, members, _, _ in ENSEMBLES[name].units for m in members]


def ensemble_heads(name):
    """{unit: HeadWeights or EnsembleWeights} for HipEngine(heads=...)."""
    out = {}
    for unit, members, combine, link in ENSEMBLES[name].units:
        if combine is None:
            out[unit] = head(members[0])
        else:
            first = head(members[0])
            out[unit] = W.EnsembleWeights({m: head(m) for m in members}, combine, link, list(first.classes))
    return out
