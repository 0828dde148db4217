"""Fit a classifier head on the GPU and save it as a model directory (include/buzzdetect_train.h, csrc/headtrain.hip;
many heads at once: include/buzzdetect_bank.h, csrc/headbank.hip; many stacks at once: include/buzzdetect_stackbank.h,
csrc/stackbank.hip; the host side the three share: csrc/headtrain_host.h, and ``_Handle`` here).

The bring-your-own-labels loop without a foreign toolchain:

    emb = engine.embed(samples, 0.96)                        # device-resident, [windows, 1024]
    fit = fit_head(emb, labels, classes=["ambient", "ins_buzz"], epochs=20)
    table = metrics_table(held_out_logits[:, 1], held_out_labels == 1)
    save_model("models/model_mine", fit, metrics=table)
    analyze(modelname="model_mine", precision=0.95)

``fit_head`` trains a stack of Dense layers - the stacks ``HipEngine`` runs - with softmax ("categorical") or sigmoid
("binary") cross-entropy from logits and SGD or Adam (Keras's defaults), every product in exact float32 on the matrix cores,
bit-reproducible: initial values and epoch permutations come from ``np.random.default_rng(seed)`` on the host, and the device
side adds nothing atomically and cuts the batch at fixed rows (``TRAIN_SLICE_ROWS``).

Imbalanced labels (an insect buzz is a few windows in a thousand): ``fit_head(..., class_weight="balanced", weight_decay=1e-4,
early_stopping={"patience": 3}, validation=(emb_val, labels_val))``.

* The weighted loss is Keras's ``sample_weight`` under ``sum_over_batch_size``: row r of a batch of B counts ``w_r`` times and
  the sum is divided by B (B C for the binary loss), not by the sum of the weights - ``loss = (1/B) sum_r w_r loss_r``,
  ``dz_r = w_r (softmax(z_r) - onehot_r) / B``.  A class weight is a row weight: ``w_r = class_weight[label_r] *
  sample_weight_r``, one float32 product on the host, moved to the device once and permuted per epoch beside the targets.
* Weight decay is decoupled (AdamW's): a kernel element - never a bias - becomes ``p - (lr * weight_decay) p`` and the
  optimizer's update is subtracted from that.  It is no term of the loss: the reported losses do not contain it.
* Order within a step: forward, weighted row losses and deltas, backward, then per parameter the gradient's sum, the decay,
  the SGD or Adam update.  Order within an epoch: the learning rate of the epoch is set, the steps run, the validation loss
  is computed, the epoch's one host read takes place, and - with ``early_stopping`` - that read decides: an improvement
  snapshots the parameters on the device, ``patience`` epochs without one end the fit, and the snapshot is what comes back.

Many heads in one pass (include/buzzdetect_bank.h, csrc/headbank.hip): ``fit_heads(emb, labels, classes, members)`` fits a list
of one-layer heads that differ only in rate, decay, weights and stopping - every member bit for bit the ``fit_head`` call it
stands for, each step's rows gathered once for all of them - and ``cross_validate_head(emb, labels, classes, folds=5,
groups=recordings, grid=[...])`` builds grouped, stratified folds, fits every (fold, grid entry) that way and returns
out-of-fold logits, ``metrics(class_name)`` for an honest threshold, and the grid entry to refit on all rows.  A fold is row
weights: held-out rows weigh 0 while fitting and are the only ones that weigh in ``val_loss``.

Heads with hidden layers, or with more than 64 classes, go the same way through a bank of whole stacks
(include/buzzdetect_stackbank.h, csrc/stackbank.hip): ``fit_stacks(..., hidden=(128,), activations=("relu",))`` and
``cross_validate_stack(...)`` are ``fit_heads`` and ``cross_validate_head`` with a shape, every member bit for bit its
``fit_head`` call.

Out of scope: dropout, penalties added to the loss, a per-class ``pos_weight`` for the binary loss, focal loss and label
smoothing, resuming a fit from a snapshot, ``.keras`` / ``.h5`` output, multi-GPU training, and training anything below the
embedding.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, modeldir, weights

HIDDEN_ACTIVATIONS = ("linear", "relu", "sigmoid", "tanh")
METRICS_HEADER = '"threshold","precision","sensitivity","fpr"'


@dataclass
class FitResult:
    """``head``: what ``HipEngine(head=...)`` and ``save_model`` take (the last layer linear: the engine's outputs are the
    logits the loss was computed from).  ``history``: per-epoch mean ``loss`` and, with a validation set, ``val_loss``, one
    entry per epoch that ran.  With ``early_stopping`` (None without): ``best_epoch``, the 0-based epoch of the best monitored
    value (None if no epoch's was a number), and ``stopped_epoch``, the last epoch that ran."""
    head: weights.HeadWeights
    history: Dict[str, List[float]] = field(default_factory=dict)
    best_epoch: Optional[int] = None
    stopped_epoch: Optional[int] = None


def glorot_layers(rng: np.random.Generator, widths: Sequence[int], activations: Sequence[str], n_in: int = _lib.EMBEDDING_SIZE):
    """Initial values as Keras's Dense has them: Glorot-uniform kernels, zero biases; one ``rng.uniform`` per layer in order."""
    layers, fan_in = [], n_in
    for w, act in zip(widths, activations):
        lim = np.sqrt(6.0 / (fan_in + w))
        layers.append((rng.uniform(-lim, lim, (fan_in, w)).astype(np.float32), np.zeros(w, dtype=np.float32), act))
        fan_in = w
    return layers


class _Handle:
    """What ``Trainer``, ``TrainerBank`` and ``TrainerStackBank`` share: the checks of loss, optimizer and device, the
    ``bd_head_layer`` arrays, the checks of a batch, the current stream and the handle's end.  ``_prefix``: the C entry points
    the methods call; ``_noun``: what the messages call the object."""

    _prefix = "bd_trainer_"
    _noun = "trainer"

    def _call(self, name, *args):
        return _lib.check(getattr(self._lib, self._prefix + name)(self._handle, *args))

    def _begin(self, loss: str, optimizer: str) -> None:
        self._handle = C.c_void_p()
        self._lib = _lib.load()
        if loss not in _lib.TRAIN_LOSSES:
            raise ValueError(f'loss must be one of {sorted(_lib.TRAIN_LOSSES)}, not "{loss}"')
        if optimizer not in _lib.TRAIN_OPTIMIZERS:
            raise ValueError(f'optimizer must be one of {sorted(_lib.TRAIN_OPTIMIZERS)}, not "{optimizer}"')

    def _on_device(self, loss: str, max_batch: int, device: Optional[int]) -> None:
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("buzzdetect_amd: no HIP device visible to PyTorch; the trainer has no CPU path")
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        self.loss = loss
        self.max_batch = int(max_batch)

    @staticmethod
    def _fill_layer(at, kernel, bias, activation, keep, what=None) -> None:
        """One ``bd_head_layer`` from (kernel, bias, activation); the float32 arrays it points to go to ``keep``.  ``what``
        (who and which shapes, for the message) asks for the shapes to be checked."""
        k = np.ascontiguousarray(kernel, dtype=np.float32)
        b = np.ascontiguousarray(bias, dtype=np.float32)
        if what is not None and (k.ndim != 2 or b.shape != (k.shape[1],)):
            raise ValueError(f"{what}, not {k.shape} and {b.shape}")
        keep += [k, b]
        at.kernel = k.ctypes.data_as(C.POINTER(C.c_float))
        at.bias = b.ctypes.data_as(C.POINTER(C.c_float))
        at.n_in, at.n_out = k.shape
        at.activation = _lib.HEAD_ACTIVATIONS[activation]

    def _create(self, arr, counts, optimizer, learning_rate, beta_1, beta_2, epsilon) -> None:
        import torch
        opt = _lib.bd_train_optimizer(_lib.TRAIN_OPTIMIZERS[optimizer], learning_rate, beta_1, beta_2, epsilon, 0)
        with torch.cuda.device(self.device):
            _lib.check(getattr(self._lib, self._prefix + "create")(self.device_index, arr, *counts, _lib.TRAIN_LOSSES[self.loss],
                                                                  C.byref(opt), self.max_batch, C.byref(self._handle)))

    def close(self) -> None:
        if getattr(self, "_handle", None) is not None and self._handle.value:
            getattr(self._lib, self._prefix + "destroy")(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check_batch(self, X, rows, targets, B):
        """(X, ldx, rows, targets) as the C calls take them; ``targets`` may be None where the call has none."""
        import torch
        if X.dtype != torch.float32 or X.dim() != 2 or X.stride(1) != 1 or X.device != self.device:
            raise ValueError(f"X must be a float32 [N, >= 1024] matrix on the {self._noun}'s device with unit column stride")
        if rows is not None and (rows.dtype != torch.int32 or not rows.is_contiguous() or rows.numel() < B):
            raise ValueError("rows must be a contiguous int32 tensor of at least B entries")
        if rows is None and X.shape[0] < B:
            raise ValueError("X has fewer than B rows")
        if targets is not None:
            want = torch.float32 if self.loss == "binary" else torch.int32
            if targets.dtype != want or not targets.is_contiguous() or targets.numel() < B * (self.n_out if self.loss == "binary" else 1):
                raise ValueError(f"targets must be a contiguous {want} tensor covering the batch")
        return (C.c_void_p(X.data_ptr()), X.stride(0), C.c_void_p(rows.data_ptr()) if rows is not None else None,
                C.c_void_p(targets.data_ptr()) if targets is not None else None)

    def workspace_fill(self, pattern: int) -> None:
        self._call("workspace_fill", pattern)

    def workspace(self) -> np.ndarray:
        out = np.empty(self._call("workspace_floats"), dtype=np.float32)
        self._call("workspace_read", out.ctypes.data_as(C.c_void_p), out.size)
        return out


class Trainer(_Handle):
    """``bd_trainer_*`` on torch tensors: ``layers`` = [(kernel [in, out], bias [out], activation)] are the initial values."""

    def __init__(self, layers, loss: str = "categorical", optimizer: str = "adam", learning_rate: float = 1e-3,
                 beta_1: float = 0.9, beta_2: float = 0.999, epsilon: float = 1e-7, max_batch: int = 256,
                 device: Optional[int] = None):
        import torch
        self._begin(loss, optimizer)
        self._on_device(loss, max_batch, device)
        self.shapes = [tuple(np.shape(k)) for k, _, _ in layers]
        self.n_out = self.shapes[-1][1]
        arr = (_lib.bd_head_layer * len(layers))()
        keep = []
        for i, (kernel, bias, activation) in enumerate(layers):
            self._fill_layer(arr[i], kernel, bias, activation, keep)
        self._create(arr, (len(layers),), optimizer, learning_rate, beta_1, beta_2, epsilon)
        with torch.cuda.device(self.device):
            self._loss_word = torch.zeros(1, dtype=torch.float32, device=self.device)

    def _batch(self, X, rows, targets, B, weights=None):
        import torch
        if weights is not None and (weights.dtype != torch.float32 or not weights.is_contiguous() or weights.numel() < B
                                    or weights.device != self.device):
            raise ValueError("weights must be a contiguous float32 tensor of at least B entries on the trainer's device")
        return self._check_batch(X, rows, targets, B) + (int(B), self._stream())

    def step(self, X, rows, targets, B: int, weights=None) -> None:
        """One optimisation step on ``B`` rows: ``rows`` (int32, device) names them in ``X``, or None for the first ``B``;
        ``targets`` are in batch order, and so are ``weights`` (float32, device: the rows' loss weights; None runs the
        unweighted kernels).  Enqueued on the current stream."""
        x, ldx, r, t, b, stream = self._batch(X, rows, targets, B, weights)
        if weights is None:
            self._call("step", x, ldx, r, t, b, stream)
        else:
            self._call("step_weighted", x, ldx, r, t, C.c_void_p(weights.data_ptr()), b, stream)

    def loss_into(self, X, rows, targets, B: int, out, weights=None) -> None:
        """Forward pass and mean (with ``weights``: weighted, still divided by ``B``) loss of the batch into the device float
        ``out[0]`` (no synchronisation)."""
        x, ldx, r, t, b, stream = self._batch(X, rows, targets, B, weights)
        if weights is None:
            self._call("loss", x, ldx, r, t, b, C.c_void_p(out.data_ptr()), stream)
        else:
            self._call("loss_weighted", x, ldx, r, t, C.c_void_p(weights.data_ptr()), b, C.c_void_p(out.data_ptr()), stream)

    def loss_of(self, X, rows, targets, B: int, weights=None) -> float:
        self.loss_into(X, rows, targets, B, self._loss_word, weights)
        return float(self._loss_word.cpu()[0])

    def set_weight_decay(self, weight_decay: float) -> None:
        """Decoupled decay of the steps from now on: kernels (not biases) shrink by ``lr * weight_decay`` of themselves
        before the optimizer's update.  0 switches it off."""
        self._call("set_weight_decay", float(weight_decay))

    def set_learning_rate(self, learning_rate: float) -> None:
        """The learning rate of the steps from now on."""
        self._call("set_learning_rate", float(learning_rate))

    def snapshot(self) -> None:
        """Copy the parameters (not Adam's slots, not the step count) to the trainer's second buffer, on the current stream."""
        self._call("snapshot", self._stream())

    def restore(self) -> None:
        """Copy the last ``snapshot`` back over the parameters, on the current stream; an error if there is none."""
        self._call("restore", self._stream())

    def _pair(self, name, layer: int) -> Tuple[np.ndarray, np.ndarray]:
        k, n = self.shapes[layer]
        w, b = np.empty((k, n), dtype=np.float32), np.empty(n, dtype=np.float32)
        self._call(name, layer, w.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p))
        return w, b

    def gradients(self, layer: int) -> Tuple[np.ndarray, np.ndarray]:
        """(dW, db) of the last step."""
        return self._pair("gradients", layer)

    def read(self, layer: int) -> Tuple[np.ndarray, np.ndarray]:
        """(kernel, bias) as they stand."""
        return self._pair("read", layer)

    def logits(self, B: int) -> np.ndarray:
        """The logits of the last ``step`` / ``loss_*`` call's ``B`` rows."""
        out = np.empty((B, self.n_out), dtype=np.float32)
        self._call("logits", B, out.ctypes.data_as(C.c_void_p))
        return out

    def mean_loss(self, reset: bool = True) -> float:
        """Mean training loss per row over the steps since the last reset (accumulated on the device)."""
        v = C.c_float()
        self._call("mean_loss", 1 if reset else 0, C.byref(v))
        return float(v.value)

    def set_fusion(self, fused: bool) -> None:
        self._call("set_fusion", 1 if fused else 0)


class TrainerBank(_Handle):
    """``bd_bank_*`` on torch tensors (include/buzzdetect_bank.h): ``members`` = [(kernel [1024, C], bias [C]), ...] are the
    initial values of M one-layer heads that share every step's rows, targets and batch order and keep their own parameters,
    slots, rate, decay, row weights, running loss, snapshot and frozen flag.  Member m is, bit for bit, the ``Trainer`` that
    got the same calls with row m of the weights."""

    _prefix = "bd_bank_"                # TrainerStackBank has the same entry points under its own
    _noun = "bank"

    def __init__(self, members, loss: str = "categorical", optimizer: str = "adam", learning_rate: float = 1e-3,
                 beta_1: float = 0.9, beta_2: float = 0.999, epsilon: float = 1e-7, max_batch: int = 256,
                 device: Optional[int] = None):
        self._begin(loss, optimizer)
        members = list(members)
        if not members:
            raise ValueError("a bank needs at least one member")
        self._on_device(loss, max_batch, device)
        self.n_members = len(members)
        arr = (_lib.bd_head_layer * len(members))()
        keep = []
        for i, member in enumerate(members):
            self._fill_layer(arr[i], member[0], member[1], "linear", keep, f"member {i}: a kernel [1024, C] and a bias [C]")
        self.n_out = int(arr[0].n_out)
        self._create(arr, (len(members),), optimizer, learning_rate, beta_1, beta_2, epsilon)

    def _batch(self, X, rows, targets, B, weights=None):
        import torch
        x, ldx, r, t = self._check_batch(X, rows, targets, B)
        w, ldw = None, 0
        if weights is not None:
            if weights.dtype != torch.float32 or weights.dim() != 2 or weights.shape[0] != self.n_members or weights.shape[1] < B \
                    or weights.stride(1) != 1 or weights.device != self.device or (self.n_members > 1 and weights.stride(0) < B):
                raise ValueError("weights must be a float32 [members, >= B] matrix on the bank's device with unit column stride")
            w, ldw = C.c_void_p(weights.data_ptr()), max(int(weights.stride(0)), int(B))
        return x, ldx, r, t, w, ldw, int(B)

    def step(self, X, rows, targets, B: int, weights=None) -> None:
        """One optimisation step of every member that is not frozen on ``B`` rows (``rows``, ``targets`` as ``Trainer.step``
        takes them, shared by the members).  ``weights``: float32 ``[members, >= B]`` on the device, row m member m's weights
        in batch order; None runs every member unweighted.  Enqueued on the current stream."""
        x, ldx, r, t, w, ldw, b = self._batch(X, rows, targets, B, weights)
        self._call("step", x, ldx, r, t, w, ldw, b, self._stream())

    def loss_into(self, X, rows, targets, B: int, out, weights=None) -> None:
        """Forward pass and every member's mean (weighted, still divided by ``B``) loss of the batch into the device floats
        ``out[:members]`` (no synchronisation)."""
        import torch
        if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < self.n_members or out.device != self.device:
            raise ValueError("out must be a contiguous float32 tensor of at least `members` entries on the bank's device")
        x, ldx, r, t, w, ldw, b = self._batch(X, rows, targets, B, weights)
        self._call("loss", x, ldx, r, t, w, ldw, b, C.c_void_p(out.data_ptr()), self._stream())

    def forward_into(self, X, rows, B: int, out) -> None:
        """Every member's logits of the batch into the device matrix ``out`` ``[>= B, >= members * C]``: member m's in columns
        ``m C .. m C + C`` (no synchronisation)."""
        import torch
        if out.dtype != torch.float32 or out.dim() != 2 or out.stride(1) != 1 or out.shape[0] < B \
                or out.shape[1] < self.n_members * self.n_out or out.device != self.device or out.stride(0) < out.shape[1]:
            raise ValueError("out must be a float32 [>= B, >= members * C] matrix on the bank's device with unit column stride")
        x, ldx, r, _, _, _, b = self._batch(X, rows, None, B)
        self._call("forward", x, ldx, r, b, C.c_void_p(out.data_ptr()), out.stride(0), self._stream())

    def set_learning_rate(self, member: int, learning_rate: float) -> None:
        """Member ``member``'s learning rate of the steps from now on."""
        self._call("set_learning_rate", int(member), float(learning_rate))

    def set_weight_decay(self, member: int, weight_decay: float) -> None:
        """Member ``member``'s decoupled decay of the steps from now on (0 switches it off)."""
        self._call("set_weight_decay", int(member), float(weight_decay))

    def freeze(self, member: int, frozen: bool = True) -> None:
        """A frozen member's parameters, slots, step count, gradients and running loss stay as they are while the others
        step; ``loss_into`` and ``forward_into`` still report it."""
        self._call("set_frozen", int(member), 1 if frozen else 0)

    def snapshot(self, member: int) -> None:
        """Copy the member's parameters (not Adam's slots, not the step count) to its snapshot, on the current stream."""
        self._call("snapshot", int(member), self._stream())

    def restore(self, member: int) -> None:
        """Copy the member's last ``snapshot`` back over its parameters, on the current stream; an error if it has none."""
        self._call("restore", int(member), self._stream())

    def _pair(self, name, member: int) -> Tuple[np.ndarray, np.ndarray]:
        w, b = np.empty((_lib.EMBEDDING_SIZE, self.n_out), dtype=np.float32), np.empty(self.n_out, dtype=np.float32)
        self._call(name, int(member), w.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p))
        return w, b

    def read(self, member: int) -> Tuple[np.ndarray, np.ndarray]:
        """(kernel, bias) of the member as they stand."""
        return self._pair("read", member)

    def gradients(self, member: int) -> Tuple[np.ndarray, np.ndarray]:
        """(dW, db) of the member's last step."""
        return self._pair("gradients", member)

    def mean_loss(self, reset: bool = True) -> np.ndarray:
        """float32[members]: every member's mean training loss per row over its steps since the last reset."""
        out = np.empty(self.n_members, dtype=np.float32)
        self._call("mean_loss", 1 if reset else 0, out.ctypes.data_as(C.c_void_p))
        return out


class TrainerStackBank(TrainerBank):
    """``bd_stackbank_*`` on torch tensors (include/buzzdetect_stackbank.h): ``members`` = [[(kernel, bias, activation), ...],
    ...] are the initial layers of M Dense stacks of one shape - what ``Trainer`` takes, M times.  ``TrainerBank``'s methods
    with the same meaning; ``read`` and ``gradients`` take the layer as well.  Member m is, bit for bit, the ``Trainer`` that
    got the same calls with row m of the weights."""

    _prefix = "bd_stackbank_"

    def __init__(self, members, loss: str = "categorical", optimizer: str = "adam", learning_rate: float = 1e-3,
                 beta_1: float = 0.9, beta_2: float = 0.999, epsilon: float = 1e-7, max_batch: int = 256,
                 device: Optional[int] = None):
        self._begin(loss, optimizer)
        members = [list(member) for member in members]
        if not members or not members[0]:
            raise ValueError("a bank needs at least one member of at least one layer")
        n_layers = len(members[0])
        self._on_device(loss, max_batch, device)
        self.n_members = len(members)
        arr = (_lib.bd_head_layer * (len(members) * n_layers))()
        keep = []
        for i, member in enumerate(members):
            if len(member) != n_layers:
                raise ValueError(f"member {i} has {len(member)} layers, member 0 has {n_layers}")
            for l, (kernel, bias, activation) in enumerate(member):
                self._fill_layer(arr[i * n_layers + l], kernel, bias, activation, keep,
                                 f"member {i}, layer {l}: a kernel [in, out] and a bias [out]")
        self.shapes = [(int(arr[l].n_in), int(arr[l].n_out)) for l in range(n_layers)]
        self.n_out = self.shapes[-1][1]
        self._create(arr, (len(members), n_layers), optimizer, learning_rate, beta_1, beta_2, epsilon)

    def _pair(self, name, member: int, layer: int) -> Tuple[np.ndarray, np.ndarray]:
        if not 0 <= int(layer) < len(self.shapes):
            raise ValueError(f"no layer {layer}: the members have {len(self.shapes)}")
        k, n = self.shapes[layer]
        w, b = np.empty((k, n), dtype=np.float32), np.empty(n, dtype=np.float32)
        self._call(name, int(member), int(layer), w.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p))
        return w, b

    def read(self, member: int, layer: int) -> Tuple[np.ndarray, np.ndarray]:
        """(kernel, bias) of the member's layer as they stand."""
        return self._pair("read", member, layer)

    def gradients(self, member: int, layer: int) -> Tuple[np.ndarray, np.ndarray]:
        """(dW, db) of the member's layer from its last step."""
        return self._pair("gradients", member, layer)


def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def _check_matrix(x, what: str):
    """(rows, host array or None, device tensor or None) of embeddings given as array, torch tensor or DeviceResult."""
    if hasattr(x, "device_tensor"):
        x = x.device_tensor()
    if _is_torch(x):
        import torch
        if x.dim() != 2 or x.shape[1] != _lib.EMBEDDING_SIZE or x.dtype != torch.float32:
            raise ValueError(f"{what} must be a float32 [N, {_lib.EMBEDDING_SIZE}] matrix, not {x.dtype} {tuple(x.shape)}")
        if x.shape[0] < 1:
            raise ValueError(f"{what} has no rows")
        if not bool(torch.isfinite(x).all()):
            raise ValueError(f"{what} holds a non-finite value")
        return x.shape[0], None, x
    a = np.asarray(x)
    if a.ndim != 2 or a.shape[1] != _lib.EMBEDDING_SIZE or a.dtype.kind != "f":
        raise ValueError(f"{what} must be a float [N, {_lib.EMBEDDING_SIZE}] matrix, not {a.dtype} {a.shape}")
    if a.shape[0] < 1:
        raise ValueError(f"{what} has no rows")
    a = np.ascontiguousarray(a, dtype=np.float32)
    if not np.isfinite(a).all():
        raise ValueError(f"{what} holds a non-finite value")
    return a.shape[0], a, None


def _check_targets(t, n: int, n_classes: int, loss: str, what: str) -> np.ndarray:
    if _is_torch(t):
        t = t.detach().cpu().numpy()
    t = np.asarray(t)
    if loss == "categorical":
        if t.shape != (n,) or t.dtype.kind not in "iu":
            raise ValueError(f"{what} must be integers of shape ({n},) for the categorical loss, not {t.dtype} {t.shape}")
        if t.size and (t.min() < 0 or t.max() >= n_classes):
            raise ValueError(f"{what} must lie in 0..{n_classes - 1}; found {int(t.min())}..{int(t.max())}")
        return np.ascontiguousarray(t, dtype=np.int32)
    if t.shape != (n, n_classes) or t.dtype.kind not in "fiub":
        raise ValueError(f"{what} must be a float [{n}, {n_classes}] matrix for the binary loss, not {t.dtype} {t.shape}")
    t = np.ascontiguousarray(t, dtype=np.float32)
    if not np.isfinite(t).all():
        raise ValueError(f"{what} holds a non-finite value")
    return t


def check_fit_arguments(embeddings, targets, classes, hidden, activations, loss, optimizer, learning_rate, epochs, batch_size,
                        validation):
    """Everything ``fit_head`` refuses, before any device work: returns the checked pieces."""
    classes = list(classes)
    if not classes or not all(isinstance(c, str) for c in classes):
        raise ValueError("classes must be a non-empty list of names")
    if loss not in _lib.TRAIN_LOSSES:
        raise ValueError(f'loss must be one of {sorted(_lib.TRAIN_LOSSES)}, not "{loss}"')
    if optimizer not in _lib.TRAIN_OPTIMIZERS:
        raise ValueError(f'optimizer must be one of {sorted(_lib.TRAIN_OPTIMIZERS)}, not "{optimizer}"')
    hidden, activations = [int(h) for h in hidden], list(activations)
    if len(hidden) != len(activations):
        raise ValueError(f"{len(hidden)} hidden widths but {len(activations)} activations")
    for a in activations:
        if a == "softmax":
            raise ValueError("softmax is not a hidden activation: it belongs to the loss (loss=\"categorical\")")
        if a not in HIDDEN_ACTIVATIONS:
            raise ValueError(f'unsupported activation "{a}": hidden layers are {", ".join(HIDDEN_ACTIVATIONS)}')
    widths = hidden + [len(classes)]
    if len(widths) > _lib.HEAD_MAX_LAYERS:
        raise ValueError(f"{len(widths)} layers; the engine runs at most {_lib.HEAD_MAX_LAYERS}")
    if any(w < 1 or w > _lib.HEAD_MAX_WIDTH for w in widths):
        raise ValueError(f"layer widths must lie in 1..{_lib.HEAD_MAX_WIDTH}, not {widths}")
    if int(epochs) < 1:
        raise ValueError("epochs must be at least 1")
    if not callable(learning_rate) and np.ndim(learning_rate) == 0:     # a schedule is check_fit_weighting's to check
        learning_rates(learning_rate, 1)
    if not 1 <= int(batch_size) <= _lib.TRAIN_MAX_BATCH:
        raise ValueError(f"batch_size must lie in 1..{_lib.TRAIN_MAX_BATCH}")
    n, host, dev = _check_matrix(embeddings, "embeddings")
    t = _check_targets(targets, n, len(classes), loss, "targets")
    val = None
    if validation is not None:
        if len(validation) not in (2, 3):
            raise ValueError("validation must be (embeddings, targets) or (embeddings, targets, sample_weight)")
        vn, vhost, vdev = _check_matrix(validation[0], "validation embeddings")
        val = (vn, vhost, vdev, _check_targets(validation[1], vn, len(classes), loss, "validation targets"))
    return classes, widths, activations + ["linear"], (n, host, dev, t), val


def balanced_class_weights(labels, n_classes: int) -> np.ndarray:
    """scikit-learn's "balanced" weights, ``N / (C * count_c)`` as float64[C]: every class that occurs carries the same total
    weight N / C.  A class without rows gets 0 (no row reads it)."""
    labels = np.asarray(labels)
    n_classes = int(n_classes)
    if labels.ndim != 1 or labels.size < 1 or labels.dtype.kind not in "iu":
        raise ValueError(f"labels must be a non-empty integer vector, not {labels.dtype} {labels.shape}")
    if n_classes < 1 or labels.min() < 0 or labels.max() >= n_classes:
        raise ValueError(f"labels must lie in 0..{n_classes - 1}")
    count = np.bincount(labels, minlength=n_classes).astype(np.float64)
    out = np.zeros(n_classes, dtype=np.float64)
    np.divide(float(labels.size), n_classes * count, out=out, where=count > 0)
    return out


def learning_rates(learning_rate, epochs: int) -> List[float]:
    """The rate of every epoch from a float, a sequence of ``epochs`` floats or a callable ``epoch -> float`` (called for
    0 .. epochs-1 here, on the host, before anything runs: a bad rate is refused before any device work)."""
    if callable(learning_rate):
        rates = [learning_rate(e) for e in range(epochs)]
    elif np.ndim(learning_rate) == 0:
        rates = [learning_rate] * epochs
    else:
        rates = list(learning_rate)
        if len(rates) != epochs:
            raise ValueError(f"learning_rate has {len(rates)} entries for {epochs} epochs")
    try:
        rates = [float(r) for r in rates]
    except (TypeError, ValueError):
        raise ValueError("learning_rate must be a number, a sequence of numbers or a callable that returns one") from None
    if not all(np.isfinite(r) and r > 0 and np.float32(r) > 0 and np.isfinite(np.float32(r)) for r in rates):
        raise ValueError("learning_rate must be positive and finite")
    return rates


def _check_weights(w, n: int, what: str) -> np.ndarray:
    if _is_torch(w):
        w = w.detach().cpu().numpy()
    w = np.asarray(w)
    if w.shape != (n,) or w.dtype.kind not in "fiu":
        raise ValueError(f"{what} must be numbers of shape ({n},), not {w.dtype} {w.shape}")
    w = np.ascontiguousarray(w, dtype=np.float32)
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError(f"{what} must be finite and not negative")
    if not w.any():
        raise ValueError(f"{what} are all zero: nothing would be learnt")
    return w


def check_fit_weighting(classes, loss, epochs, learning_rate, targets, val_rows=0, val_weight=None, sample_weight=None,
                        class_weight=None, weight_decay=0.0, early_stopping=None):
    """``check_fit_arguments``' sibling for what weighs, decays, schedules and stops a fit; ``targets`` as that function
    returned them, ``val_rows`` the validation set's rows and ``val_weight`` its third element.  Returns (row weights float32[N] or None, validation weights float32[VN] or None, the epochs' rates,
    weight_decay, early stopping as (patience, min_delta, restore_best) or None).  ``ValueError`` before any device work."""
    n, c = len(targets), len(classes)
    rates = learning_rates(learning_rate, int(epochs))
    weight_decay = float(weight_decay)
    if not (np.isfinite(weight_decay) and weight_decay >= 0 and np.isfinite(np.float32(weight_decay))):
        raise ValueError("weight_decay must be finite and not negative")
    row_w = _check_weights(sample_weight, n, "sample_weight") if sample_weight is not None else None
    if class_weight is not None:
        if loss != "categorical":
            raise ValueError('class_weight needs loss="categorical": multi-hot targets have no one class per row; '
                             "weigh the rows with sample_weight instead")
        if isinstance(class_weight, str):
            if class_weight != "balanced":
                raise ValueError(f'class_weight must be "balanced", a dict or a sequence, not "{class_weight}"')
            cw = balanced_class_weights(targets, c)
        elif isinstance(class_weight, dict):
            unknown = [k for k in class_weight if k not in classes]
            if unknown:
                raise ValueError(f"class_weight names unknown classes {unknown}; the classes are {classes}")
            cw = [class_weight.get(name, 1.0) for name in classes]      # a class not named weighs 1, as in Keras
        else:
            cw = class_weight
        try:
            cw = np.asarray(cw, dtype=np.float32)
        except (TypeError, ValueError):
            raise ValueError("class_weight must hold numbers") from None
        if cw.shape != (c,):
            raise ValueError(f"class_weight must have one entry per class ({c}), not shape {cw.shape}")
        if not np.isfinite(cw).all() or (cw < 0).any():
            raise ValueError("class_weight must be finite and not negative")
        per_row = cw[targets]
        row_w = per_row if row_w is None else per_row * row_w           # one float32 product per row
        if not np.isfinite(row_w).all():
            raise ValueError("class_weight x sample_weight overflows float32")
        if not row_w.any():
            raise ValueError("class_weight x sample_weight is zero on every row: nothing would be learnt")
    val_w = _check_weights(val_weight, int(val_rows), "validation sample_weight") if val_weight is not None else None
    stop = None
    if early_stopping is not None:
        if not isinstance(early_stopping, dict) or "patience" not in early_stopping:
            raise ValueError('early_stopping must be a dict with "patience" (and optionally "min_delta", "restore_best")')
        unknown = sorted(set(early_stopping) - {"patience", "min_delta", "restore_best"})
        if unknown:
            raise ValueError(f"early_stopping has unknown keys {unknown}")
        patience, min_delta = early_stopping["patience"], early_stopping.get("min_delta", 0.0)
        if isinstance(patience, bool) or not isinstance(patience, (int, np.integer)) or patience < 0:
            raise ValueError("early_stopping: patience must be an integer >= 0")
        if isinstance(min_delta, bool) or not isinstance(min_delta, (int, float, np.integer, np.floating)) \
                or not (np.isfinite(min_delta) and min_delta >= 0):
            raise ValueError("early_stopping: min_delta must be finite and not negative")
        restore_best = early_stopping.get("restore_best", True)
        if not isinstance(restore_best, (bool, np.bool_)):
            raise ValueError("early_stopping: restore_best must be True or False")
        stop = (int(patience), float(min_delta), bool(restore_best))
    return row_w, val_w, rates, weight_decay, stop


def fit_head(embeddings, targets, classes, hidden=(), activations=(), loss="categorical", optimizer="adam", learning_rate=1e-3,
             epochs=10, batch_size=256, seed=0, validation=None, device=None, sample_weight=None, class_weight=None,
             weight_decay=0.0, early_stopping=None) -> FitResult:
    """Train ``1024 -> hidden... -> len(classes)`` on ``embeddings`` ([N, 1024] float32: array, torch tensor or
    ``DeviceResult``; a device tensor is used where it is) and ``targets`` (``int[N]`` for ``loss="categorical"``, ``float[N, C]``
    multi-hot for ``"binary"``).  ``activations`` name the hidden layers' (linear, relu, sigmoid, tanh); the last layer is
    trained on raw logits and saved linear.  Glorot-uniform kernels, zero biases and one permutation per epoch come from
    ``np.random.default_rng(seed)`` in that order; the last batch of an epoch is ragged, not dropped.  ``validation`` =
    (embeddings, targets[, sample_weight]) adds ``val_loss`` to the history.  Same arguments, same bits.

    What the defaults leave off (with them the fit is bit for bit the one without these arguments):

    * ``sample_weight``: ``float[N]``, finite, >= 0, not all zero; either loss.  The batch loss is ``(1/B) sum_r w_r loss_r``
      (Keras's ``sum_over_batch_size``: divided by B, or B C for the binary loss, not by the weights' sum), and ``history``
      reports that weighted loss.
    * ``class_weight``: ``"balanced"`` (``balanced_class_weights``: N / (C count_c)), a ``{class name: weight}`` dict (a class
      not named weighs 1) or a sequence of C weights; categorical loss only.  Row r weighs ``class_weight[label_r] *
      sample_weight_r``, one float32 product on the host; the weights go to the device once and are permuted per epoch beside
      the targets.  Validation rows weigh their own third element or 1: class weights are for fitting.
    * ``weight_decay``: decoupled - each step first shrinks every kernel (no bias) element by ``lr * weight_decay`` of itself,
      then subtracts the optimizer's update.  Not a term of the loss.
    * ``learning_rate``: a float, a sequence of ``epochs`` floats, or a callable ``epoch -> float`` (called for every epoch
      number on the host before the first step); the epoch's rate is set before its first step.
    * ``early_stopping``: ``{"patience": int >= 0, "min_delta": float >= 0 (0), "restore_best": bool (True)}``.  Monitored:
      ``val_loss`` with a validation set, else ``loss``.  An epoch improves when ``monitored < best - min_delta``; then, and
      only then, the parameters are snapshot on the device.  ``patience`` epochs in a row without improvement end the fit, and
      with ``restore_best`` the head returned is the snapshot: the head of ``epochs=best_epoch + 1``.  The decision is taken at
      the epoch's one host read; no step waits for it.  ``FitResult.best_epoch`` / ``.stopped_epoch`` say what happened.

    ``ValueError`` before any device work: shapes, labels outside ``0..C-1``, an unsupported activation (softmax among the
    hidden ones included), non-finite inputs, ``len(classes) != C``; weights of the wrong length, negative, non-finite or all
    zero; unknown class names; ``class_weight`` with the binary loss; a negative decay; a rate that is not positive or a
    sequence of them that is not ``epochs`` long; a negative patience.

    Not offered: dropout, penalties added to the loss, ``pos_weight`` for the binary loss, focal loss, label smoothing,
    resuming from a snapshot, ``.keras`` / ``.h5`` output, multi-GPU training, training below the embedding."""
    classes, widths, acts, (n, host, dev, t_host), val = check_fit_arguments(
        embeddings, targets, classes, hidden, activations, loss, optimizer, learning_rate, epochs, batch_size, validation)
    w_host, vw_host, rates, weight_decay, stop = check_fit_weighting(
        classes, loss, epochs, learning_rate, t_host, val[0] if val is not None else 0,
        validation[2] if validation is not None and len(validation) == 3 else None, sample_weight, class_weight, weight_decay,
        early_stopping)
    import torch
    rng = np.random.default_rng(seed)
    layers = glorot_layers(rng, widths, acts)
    batch = int(batch_size)
    scheduled = callable(learning_rate) or np.ndim(learning_rate) != 0
    trainer = Trainer(layers, loss, optimizer, rates[0], max_batch=batch,
                      device=device if device is not None else (dev.device.index if dev is not None else None))
    best_epoch = stopped_epoch = None
    try:
        with torch.cuda.device(trainer.device):
            def resident(h, d):
                x = d if d is not None else torch.from_numpy(h)
                x = x.to(trainer.device)
                return x if x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 else x.contiguous().clone()

            if weight_decay:
                trainer.set_weight_decay(weight_decay)
            X = resident(host, dev)
            T = torch.from_numpy(t_host).to(trainer.device)
            Wt = torch.from_numpy(w_host).to(trainer.device) if w_host is not None else None
            w_epoch = VW = None
            if val is not None:
                VX, VT = resident(val[1], val[2]), torch.from_numpy(val[3]).to(trainer.device)
                if vw_host is not None:
                    VW = torch.from_numpy(vw_host).to(trainer.device)
                val_word = torch.zeros(1, dtype=torch.float32, device=trainer.device)
                val_sum = torch.zeros(1, dtype=torch.float64, device=trainer.device)
            history: Dict[str, List[float]] = {"loss": []}
            if val is not None:
                history["val_loss"] = []
            best, waited = float("inf"), 0
            for epoch in range(int(epochs)):
                if scheduled:
                    trainer.set_learning_rate(rates[epoch])
                perm = torch.from_numpy(rng.permutation(n).astype(np.int32)).to(trainer.device)
                t_epoch = T[perm.long()].contiguous()                   # targets in batch order, once per epoch
                if Wt is not None:
                    w_epoch = Wt[perm.long()].contiguous()              # and the rows' weights beside them
                for at in range(0, n, batch):
                    b = min(batch, n - at)
                    trainer.step(X, perm[at:at + b], t_epoch[at:at + b], b, w_epoch[at:at + b] if Wt is not None else None)
                if val is not None:
                    val_sum.zero_()
                    for at in range(0, val[0], batch):
                        b = min(batch, val[0] - at)
                        trainer.loss_into(VX[at:at + b], None, VT[at:at + b], b, val_word, VW[at:at + b] if VW is not None else None)
                        val_sum.add_(val_word.double(), alpha=b)
                history["loss"].append(trainer.mean_loss(reset=True))    # the one read of the epoch (waits for the stream)
                if val is not None:
                    history["val_loss"].append(float(val_sum.cpu()[0]) / val[0])
                if stop is not None:                                     # decided on what the epoch's read brought
                    patience, min_delta, _ = stop
                    monitored = history["val_loss" if val is not None else "loss"][-1]
                    stopped_epoch = epoch
                    if monitored < best - min_delta:
                        best, best_epoch, waited = monitored, epoch, 0
                        trainer.snapshot()
                    else:
                        waited += 1
                        if waited >= patience:
                            break
            if stop is not None and stop[2] and best_epoch is not None and best_epoch != stopped_epoch:
                trainer.restore()
            out = [trainer.read(l) + (a,) for l, a in enumerate(acts)]
    finally:
        trainer.close()
    return FitResult(weights.HeadWeights(out, classes, source="fit_head"), history, best_epoch, stopped_epoch)


MEMBER_KEYS = ("learning_rate", "weight_decay", "sample_weight", "class_weight", "early_stopping", "validation_weight")


def check_members(members, classes, loss, epochs, targets, val_rows=None):
    """What ``fit_heads`` refuses about its members, before any device work: ``check_fit_weighting`` of each, with the member's
    index in front of the message.  ``targets`` as ``check_fit_arguments`` returned them, ``val_rows`` the validation set's
    rows (None: there is none)."""
    members = list(members)
    if not members:
        raise ValueError("members must hold at least one dict")
    if len(members) > _lib.BANK_MAX_MEMBERS:
        raise ValueError(f"{len(members)} members; a bank holds at most {_lib.BANK_MAX_MEMBERS}")
    checked = []
    for i, member in enumerate(members):
        if not isinstance(member, dict):
            raise ValueError(f"members[{i}] must be a dict, not {type(member).__name__}")
        unknown = sorted(set(member) - set(MEMBER_KEYS), key=str)
        if unknown:
            raise ValueError(f"members[{i}] has unknown keys {unknown}; a member may set {', '.join(MEMBER_KEYS)}")
        if member.get("validation_weight") is not None and val_rows is None:
            raise ValueError(f"members[{i}] has a validation_weight, but there is no validation set")
        try:
            checked.append(check_fit_weighting(classes, loss, epochs, member.get("learning_rate", 1e-3), targets, val_rows or 0,
                                               member.get("validation_weight"), member.get("sample_weight"),
                                               member.get("class_weight"), member.get("weight_decay", 0.0),
                                               member.get("early_stopping")))
        except ValueError as exc:
            raise ValueError(f"members[{i}]: {exc}") from None
    return checked


def _member_fit_arguments(member, validation):
    """The keyword arguments with which ``fit_head`` runs a member of ``fit_heads`` on its own."""
    kw = {k: v for k, v in member.items() if k != "validation_weight"}
    if validation is not None:
        vw = member.get("validation_weight")
        kw["validation"] = tuple(validation[:2]) + ((vw,) if vw is not None else ())
    return kw


def fit_heads(embeddings, targets, classes, members, *, hidden=(), activations=(), loss="categorical", optimizer="adam", epochs=10,
              batch_size=256, seed=0, validation=None, device=None) -> List[FitResult]:
    """Fit ``len(members)`` heads ``1024 -> len(classes)`` in one pass over the data: the folds of a cross-validation, the
    entries of a sweep.  ``members`` is a list of dicts; a member may set ``learning_rate`` (float, sequence or callable),
    ``weight_decay``, ``sample_weight``, ``class_weight``, ``early_stopping`` - each as ``fit_head`` takes it - and
    ``validation_weight``, its own weights of the shared ``validation = (embeddings, targets)`` rows.  Everything else is
    shared: data, loss, optimizer, epochs, batch size and seed.

    ``fit_heads(..., members)[m]`` has the head bytes, ``history``, ``best_epoch`` and ``stopped_epoch`` of
    ``fit_head(embeddings, targets, classes, **shared, **members[m])`` with the member's ``validation_weight`` as the third
    element of ``validation``.  One ``np.random.default_rng(seed)`` gives the Glorot values, then one permutation per epoch:
    all members start equal and see the same batches, so each step gathers its rows of X once for all of them
    (``TrainerBank``).  An epoch has one host read - M training losses and M validation sums; early stopping is decided per
    member at that read: an improving member is snapshot, one out of patience is frozen, and the loop ends when every member
    is frozen or the epochs are done.

    ``hidden`` stacks are outside this bank: the members then run one after another through ``fit_head`` - same results, no
    sharing; ``fit_stacks`` fits them in one pass, and one-layer heads of more than 64 classes too.  ``ValueError`` before any device work, with the member's index: an unknown key and whatever ``fit_head`` refuses."""
    members = list(members)
    classes, widths, acts, (n, host, dev, t_host), val = check_fit_arguments(
        embeddings, targets, classes, hidden, activations, loss, optimizer, 1e-3, epochs, batch_size, validation)
    if validation is not None and len(validation) != 2:
        raise ValueError("validation must be (embeddings, targets): a member's weights of those rows are its validation_weight")
    checked = check_members(members, classes, loss, epochs, t_host, val[0] if val is not None else None)
    if len(widths) > 1:
        return [fit_head(embeddings, targets, classes, hidden=hidden, activations=activations, loss=loss, optimizer=optimizer,
                         epochs=epochs, batch_size=batch_size, seed=seed, device=device, **_member_fit_arguments(m, validation))
                for m in members]
    if widths[0] > _lib.TRAIN_FUSED_MAX_WIDTH:
        raise ValueError(f"a bank holds heads of at most {_lib.TRAIN_FUSED_MAX_WIDTH} classes, not {widths[0]}")
    rng = np.random.default_rng(seed)
    kernel, bias, _ = glorot_layers(rng, widths, acts)[0]
    bank = TrainerBank([(kernel, bias)] * len(members), loss, optimizer, checked[0][2][0], max_batch=int(batch_size),
                       device=device if device is not None else (dev.device.index if dev is not None else None))
    return _fit_members(bank, checked, rng, (n, host, dev, t_host), val, validation is not None and validation[0] is embeddings,
                        int(epochs), int(batch_size), classes, lambda m: [bank.read(m) + (acts[0],)])


def fit_stacks(embeddings, targets, classes, members, *, hidden=(), activations=(), loss="categorical", optimizer="adam", epochs=10,
               batch_size=256, seed=0, validation=None, device=None) -> List[FitResult]:
    """``fit_heads`` for heads of any shape ``fit_head`` takes: ``len(members)`` stacks ``1024 -> hidden... -> len(classes)``
    fitted in one pass (``TrainerStackBank``: include/buzzdetect_stackbank.h).  ``members`` and everything shared are as
    ``fit_heads`` takes them, and so are the checks, with ``members[i]:`` in front of a member's error.

    ``fit_stacks(..., members)[m]`` has the head bytes of every layer, ``history``, ``best_epoch`` and ``stopped_epoch`` of
    ``fit_head(embeddings, targets, classes, hidden=hidden, activations=activations, **shared, **members[m])`` with the member's
    ``validation_weight`` as the third element of ``validation``.  One ``np.random.default_rng(seed)`` gives the Glorot values
    of all layers in order, then one permutation per epoch; an epoch has one host read, at which early stopping is decided per
    member - snapshot on improvement, freeze when out of patience.

    ``hidden=()`` is allowed and takes any number of classes ``fit_head`` takes: the one-layer head of more than 64 classes
    that ``fit_heads`` refuses.  Up to 64 classes it gives ``fit_heads``'s bits.  ``ValueError`` before any device work."""
    members = list(members)
    classes, widths, acts, (n, host, dev, t_host), val = check_fit_arguments(
        embeddings, targets, classes, hidden, activations, loss, optimizer, 1e-3, epochs, batch_size, validation)
    if validation is not None and len(validation) != 2:
        raise ValueError("validation must be (embeddings, targets): a member's weights of those rows are its validation_weight")
    checked = check_members(members, classes, loss, epochs, t_host, val[0] if val is not None else None)
    rng = np.random.default_rng(seed)
    layers = glorot_layers(rng, widths, acts)
    bank = TrainerStackBank([layers] * len(members), loss, optimizer, checked[0][2][0], max_batch=int(batch_size),
                            device=device if device is not None else (dev.device.index if dev is not None else None))
    return _fit_members(bank, checked, rng, (n, host, dev, t_host), val, validation is not None and validation[0] is embeddings,
                        int(epochs), int(batch_size), classes, lambda m: [bank.read(m, l) + (a,) for l, a in enumerate(acts)])


def _fit_members(bank, checked, rng, data, val, validation_is_training, epochs, batch, classes, read_layers) -> List[FitResult]:
    """The epochs of ``fit_heads`` and ``fit_stacks``: ``bank`` (a ``TrainerBank`` or ``TrainerStackBank``, closed here) holds
    the members at their initial values, ``checked`` is ``check_members``' result, ``rng`` the generator behind the initial
    values, ``data`` and ``val`` are ``check_fit_arguments``', and ``read_layers(m)`` gives member m's layers for its head."""
    import torch
    n, host, dev, t_host = data
    M = len(checked)
    rates = [c[2] for c in checked]
    stops = [c[4] for c in checked]
    best_epoch: List[Optional[int]] = [None] * M
    stopped_epoch: List[Optional[int]] = [None] * M
    try:
        with torch.cuda.device(bank.device):
            def resident(h, d):
                x = d if d is not None else torch.from_numpy(h)
                x = x.to(bank.device)
                return x if x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 else x.contiguous().clone()

            def stacked(rows_of, length):                # [M, length]: a member without weights weighs every row 1
                if all(w is None for w in rows_of):
                    return None
                return torch.from_numpy(np.stack([w if w is not None else np.ones(length, dtype=np.float32) for w in rows_of])
                                        ).to(bank.device)

            for m, c in enumerate(checked):
                if c[3]:
                    bank.set_weight_decay(m, c[3])
            X = resident(host, dev)
            T = torch.from_numpy(t_host).to(bank.device)
            Wt = stacked([c[0] for c in checked], n)
            w_epoch = VW = None
            if val is not None:
                VX = X if validation_is_training else resident(val[1], val[2])
                VT = torch.from_numpy(val[3]).to(bank.device)
                VW = stacked([c[1] for c in checked], val[0])
                val_words = torch.zeros(M, dtype=torch.float32, device=bank.device)
                val_sums = torch.zeros(M, dtype=torch.float64, device=bank.device)
            histories: List[Dict[str, List[float]]] = [{"loss": [], **({"val_loss": []} if val is not None else {})} for _ in range(M)]
            best, waited, active = [float("inf")] * M, [0] * M, [True] * M
            for epoch in range(epochs):
                for m in range(M):
                    if active[m]:
                        bank.set_learning_rate(m, rates[m][epoch])
                perm = torch.from_numpy(rng.permutation(n).astype(np.int32)).to(bank.device)
                t_epoch = T[perm.long()].contiguous()
                if Wt is not None:
                    w_epoch = Wt[:, perm.long()].contiguous()
                for at in range(0, n, batch):
                    b = min(batch, n - at)
                    bank.step(X, perm[at:at + b], t_epoch[at:at + b], b, w_epoch[:, at:at + b] if Wt is not None else None)
                if val is not None:
                    val_sums.zero_()
                    for at in range(0, val[0], batch):
                        b = min(batch, val[0] - at)
                        bank.loss_into(VX[at:at + b], None, VT[at:at + b], b, val_words, VW[:, at:at + b] if VW is not None else None)
                        val_sums.add_(val_words.double(), alpha=b)
                losses = bank.mean_loss(reset=True)               # the one read of the epoch (waits for the stream)
                val_losses = val_sums.cpu().numpy() if val is not None else None
                for m in range(M):
                    if not active[m]:
                        continue
                    histories[m]["loss"].append(float(losses[m]))
                    if val is not None:
                        histories[m]["val_loss"].append(float(val_losses[m]) / val[0])
                    if stops[m] is not None:
                        patience, min_delta, _ = stops[m]
                        monitored = histories[m]["val_loss" if val is not None else "loss"][-1]
                        stopped_epoch[m] = epoch
                        if monitored < best[m] - min_delta:
                            best[m], best_epoch[m], waited[m] = monitored, epoch, 0
                            bank.snapshot(m)
                        else:
                            waited[m] += 1
                            if waited[m] >= patience:
                                active[m] = False
                                bank.freeze(m)
                if not any(active):
                    break
            out = []
            for m in range(M):
                if stops[m] is not None and stops[m][2] and best_epoch[m] is not None and best_epoch[m] != stopped_epoch[m]:
                    bank.restore(m)
                out.append(FitResult(weights.HeadWeights(read_layers(m), classes, source="fit_head"), histories[m],
                                     best_epoch[m], stopped_epoch[m]))
    finally:
        bank.close()
    return out


FOLD_SEED_STREAM = 0x666F6C64               # the fold builder's generator is default_rng([seed, this]): not the fit's default_rng(seed)


def build_folds(targets, loss: str = "categorical", folds: int = 5, groups=None, seed: int = 0) -> np.ndarray:
    """int32[N]: the fold that holds each row out, built from ``np.random.default_rng([seed, FOLD_SEED_STREAM])`` - a generator
    of its own, so the fit's draws from ``default_rng(seed)`` do not move.

    * without ``groups``, categorical loss: stratified - the rows of each class are shuffled and dealt round-robin, the deal of
      a class starting where the last one ended, so per class the folds' counts differ by at most 1;
    * without ``groups``, binary loss: all rows shuffled and dealt round-robin;
    * with ``groups`` (``[N]``, any hashable: the recording a window came from): whole groups are dealt, largest first (ties in
      shuffled order), each to the fold that holds the fewest rows so far (ties: the lowest fold).  No group is split; labels
      are not looked at.

    ``ValueError``: fewer than 2 folds, more folds than groups or rows, a fold left without rows."""
    t = np.asarray(targets)
    n = t.shape[0]
    if isinstance(folds, bool) or not isinstance(folds, (int, np.integer)) or folds < 2:
        raise ValueError("folds must be an integer >= 2")
    folds = int(folds)
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or seed < 0:
        raise ValueError("seed must be a non-negative integer")
    rng = np.random.default_rng([int(seed), FOLD_SEED_STREAM])
    fold_of_row = np.full(n, -1, dtype=np.int32)
    if groups is not None:
        groups = list(groups) if not isinstance(groups, np.ndarray) else groups.tolist()
        if len(groups) != n:
            raise ValueError(f"groups must name one group per row ({n}), not {len(groups)}")
        index: Dict[Any, int] = {}
        group_of_row = np.array([index.setdefault(g, len(index)) for g in groups], dtype=np.int64)
        if folds > len(index):
            raise ValueError(f"{folds} folds but only {len(index)} groups: a group is never split")
        size = np.bincount(group_of_row, minlength=len(index))
        order = rng.permutation(len(index))
        order = order[np.argsort(-size[order], kind="stable")]
        held = np.zeros(folds, dtype=np.int64)
        fold_of_group = np.empty(len(index), dtype=np.int32)
        for g in order:
            k = int(np.argmin(held))
            fold_of_group[g] = k
            held[k] += size[g]
        fold_of_row = fold_of_group[group_of_row]
    else:
        if folds > n:
            raise ValueError(f"{folds} folds but only {n} rows")
        strata = [np.flatnonzero(t == c) for c in np.unique(t)] if loss == "categorical" else [np.arange(n)]
        start = 0
        for rows in strata:
            rows = rows[rng.permutation(rows.size)]
            fold_of_row[rows] = (start + np.arange(rows.size)) % folds
            start = (start + rows.size) % folds
    empty = [k for k in range(folds) if not (fold_of_row == k).any()]
    if empty:
        raise ValueError(f"fold {empty[0]} holds no rows")
    return fold_of_row.astype(np.int32)


def check_folds(fold_of_row, n: int) -> Tuple[np.ndarray, int]:
    """A caller's ``fold_of_row`` as (int32[N], K): integers 0..K-1, K = the largest + 1 >= 2, every fold with rows."""
    f = np.asarray(fold_of_row.detach().cpu().numpy() if _is_torch(fold_of_row) else fold_of_row)
    if f.shape != (n,) or f.dtype.kind not in "iu":
        raise ValueError(f"fold_of_row must be integers of shape ({n},), not {f.dtype} {f.shape}")
    if f.min() < 0 or f.max() >= _lib.BANK_MAX_MEMBERS:
        raise ValueError(f"fold_of_row must lie in 0..K-1 (K <= {_lib.BANK_MAX_MEMBERS}); found {int(f.min())}..{int(f.max())}")
    k = int(f.max()) + 1
    if k < 2:
        raise ValueError("fold_of_row names one fold only: nothing would be left to train on")
    empty = [i for i in range(k) if not (f == i).any()]
    if empty:
        raise ValueError(f"fold {empty[0]} holds no rows")
    return f.astype(np.int32), k


def fold_members(targets, classes, loss, fold_of_row, folds: int, entry: Dict[str, Any]) -> List[Dict[str, Any]]:
    """The ``fit_heads`` members of one grid entry, fold 0 .. folds-1.  Member k trains with ``sample_weight_r x [fold_of_row[r]
    != k]`` and validates on the same rows with weight ``[fold_of_row[r] == k]``; its class weights - "balanced" included -
    are computed from the labels of its training side only and handed on as an explicit float64 vector."""
    n = len(fold_of_row)
    base = entry.get("sample_weight")
    if base is not None:
        base = _check_weights(base, n, "sample_weight").astype(np.float64)
    out = []
    for k in range(folds):
        train_side = fold_of_row != k
        member = {key: entry[key] for key in ("learning_rate", "weight_decay", "early_stopping") if key in entry}
        member["sample_weight"] = train_side.astype(np.float64) if base is None else base * train_side
        cw = entry.get("class_weight")
        if cw is not None:
            if loss != "categorical":
                raise ValueError('class_weight needs loss="categorical": multi-hot targets have no one class per row; '
                                 "weigh the rows with sample_weight instead")
            if isinstance(cw, str):
                if cw != "balanced":
                    raise ValueError(f'class_weight must be "balanced", a dict or a sequence, not "{cw}"')
                cw = balanced_class_weights(np.asarray(targets)[train_side], len(classes))
            elif isinstance(cw, dict):
                unknown = [name for name in cw if name not in classes]
                if unknown:
                    raise ValueError(f"class_weight names unknown classes {unknown}; the classes are {list(classes)}")
                cw = np.array([cw.get(name, 1.0) for name in classes], dtype=np.float64)
            member["class_weight"] = cw
        member["validation_weight"] = (~train_side).astype(np.float32)
        out.append(member)
    return out


@dataclass
class CrossValidationEntry:
    """One grid entry of ``cross_validate_head``.  ``oof_logits`` [N, C]: row r from the member that held r out.  ``fits``: the K
    folds' ``FitResult``.  ``fold_best``: per fold the monitored ``val_loss`` of its best epoch (with ``early_stopping``) or
    its lowest (without)."""
    oof_logits: np.ndarray
    fits: List[FitResult]
    fold_best: List[float]
    classes: List[str]
    positives: np.ndarray = field(repr=False, default=None)      # bool [N, C]

    def metrics(self, class_name: str) -> str:
        """``metrics_table`` of the out-of-fold logits of ``class_name`` against its rows: the text of ``tests/metrics.csv``."""
        if class_name not in self.classes:
            raise ValueError(f'no class "{class_name}"; the classes are {self.classes}')
        c = self.classes.index(class_name)
        return metrics_table(self.oof_logits[:, c], self.positives[:, c])


@dataclass
class CrossValidation:
    """``entries[g]`` belongs to ``grid[g]``; ``best`` is the grid index with the lowest mean of the folds' best ``val_loss``."""
    fold_of_row: np.ndarray
    grid: List[Dict[str, Any]]
    entries: List[CrossValidationEntry]
    best: int


def _fold_best(fit: FitResult) -> float:
    v = np.asarray(fit.history["val_loss"], dtype=np.float64)
    if fit.best_epoch is not None:
        return float(v[fit.best_epoch])
    return float(np.nanmin(v)) if np.isfinite(v).any() else float("inf")


def check_cross_validation(targets, classes, loss, folds, groups, fold_of_row, grid, seed, shared_member):
    """What ``cross_validate_head`` refuses about folds and grid, before any device work; ``targets`` as ``check_fit_arguments``
    returned them.  Returns (fold_of_row int32[N], K, grid as a list, the members, grid-major: entry g's fold k at g K + k)."""
    n = len(targets)
    if fold_of_row is not None:
        if folds is not None or groups is not None:
            raise ValueError("fold_of_row already says which fold holds each row out: give it, or folds / groups, not both")
        fold_of_row, k = check_folds(fold_of_row, n)
    else:
        k = 5 if folds is None else folds
        fold_of_row = build_folds(targets, loss, k, groups, seed)
        k = int(k)
    if loss == "categorical":
        for fold in range(k):
            count = np.bincount(np.asarray(targets)[fold_of_row != fold], minlength=len(classes))
            if (count == 0).any():
                c = int(np.flatnonzero(count == 0)[0])
                raise ValueError(f'the training side of fold {fold} has no row of class {c} ("{classes[c]}")')
    grid = list(grid)
    if not grid:
        raise ValueError("grid must hold at least one dict ({} fits with the defaults)")
    members = []
    for g, entry in enumerate(grid):
        if not isinstance(entry, dict):
            raise ValueError(f"grid[{g}] must be a dict, not {type(entry).__name__}")
        unknown = sorted(set(entry) - set(MEMBER_KEYS[:-1]), key=str)
        if unknown:
            raise ValueError(f"grid[{g}] has unknown keys {unknown}; an entry may set {', '.join(MEMBER_KEYS[:-1])}")
        try:
            members += fold_members(targets, classes, loss, fold_of_row, k, {**shared_member, **entry})
        except ValueError as exc:
            raise ValueError(f"grid[{g}]: {exc}") from None
    if len(members) > _lib.BANK_MAX_MEMBERS:
        raise ValueError(f"{k} folds x {len(grid)} grid entries = {len(members)} members; a bank holds at most {_lib.BANK_MAX_MEMBERS}")
    return fold_of_row, k, grid, members


def cross_validate_head(embeddings, targets, classes, *, folds=None, groups=None, fold_of_row=None, grid=({},), loss="categorical",
                        optimizer="adam", epochs=10, batch_size=256, seed=0, device=None, **shared) -> CrossValidation:
    """Grouped, stratified k-fold cross-validation of ``fit_head`` over a grid of its knobs, every fold of every grid entry
    fitted in one pass (``fit_heads``): out-of-fold logits for an honest ``metrics_table``, and the grid entry to refit with.

    Folds: ``fold_of_row`` (``int[N]`` in 0..K-1, the caller's), or ``folds`` (5 when not given) built by ``build_folds`` from
    ``seed`` and, if given, ``groups``.  Giving ``fold_of_row`` and ``folds`` / ``groups`` is an error, and so is a fold without
    rows and - categorical loss - a training side that lacks a class.

    ``grid``: dicts of ``learning_rate``, ``weight_decay``, ``sample_weight``, ``class_weight``, ``early_stopping``; ``shared``
    may set the same keys for every entry.  Member (k, g) is ``fold_members(...)[k]`` of entry g - a call ``fit_head`` can
    express, and bit for bit that call.  Two consequences of a fold being row weights: held-out rows still count in Keras's
    ``sum_over_batch_size`` denominator, so a fold's gradient is about (K-1)/K of a fit's on the training rows alone; and
    ``val_loss`` is n_heldout / N times the held-out rows' mean loss.

    The result's ``entries[g]`` hold ``oof_logits``, the K ``FitResult``, ``fold_best`` and ``metrics(class_name)``; ``best`` is
    the entry with the lowest mean ``fold_best``.  The final model stays the caller's own ``fit_head`` on all rows with
    ``grid[best]``.  Hidden layers are outside the bank and not offered here: ``cross_validate_stack`` takes them.

    The K folds are also the standard ensemble: ``save_ensemble(path, cv.entries[cv.best].fits,
    metrics=cv.entries[cv.best].metrics(cls))`` writes them as one model.  The out-of-fold table scores every row with its single
    held-out member, not with the mean of K, so it is a conservative estimate for the ensemble."""
    return _cross_validate(embeddings, targets, classes, (), (), folds, groups, fold_of_row, grid, loss, optimizer, epochs, batch_size,
                           seed, device, shared, fit_heads, lambda fits, **kw: TrainerBank([f.head.layers[0][:2] for f in fits], **kw))


def cross_validate_stack(embeddings, targets, classes, *, hidden=(), activations=(), folds=None, groups=None, fold_of_row=None,
                         grid=({},), loss="categorical", optimizer="adam", epochs=10, batch_size=256, seed=0, device=None,
                         **shared) -> CrossValidation:
    """``cross_validate_head`` for heads of any shape ``fit_head`` takes: ``1024 -> hidden... -> len(classes)`` with
    ``activations`` on the hidden layers (``hidden=()``: one layer of any number of classes).  Folds, grid, ``shared``, checks
    and the result are ``cross_validate_head``'s; every (fold, grid entry) is fitted in one pass by ``fit_stacks`` and is, bit
    for bit, the ``fit_head(..., hidden=hidden, activations=activations)`` call ``fold_members`` describes; the out-of-fold
    logits come from one forward pass of a ``TrainerStackBank`` loaded with the fitted members.  The final model stays the
    caller's own ``fit_head`` on all rows with ``grid[best]`` and the same shape.  ``ValueError`` before any device work, a grid
    entry's with ``grid[g]:`` in front.

    The K folds are also the standard ensemble: ``save_ensemble(path, cv.entries[cv.best].fits,
    metrics=cv.entries[cv.best].metrics(cls))`` writes them as one model.  The out-of-fold table scores every row with its single
    held-out member, not with the mean of K, so it is a conservative estimate for the ensemble."""
    def fit(*args, **kw):
        return fit_stacks(*args, hidden=hidden, activations=activations, **kw)
    return _cross_validate(embeddings, targets, classes, hidden, activations, folds, groups, fold_of_row, grid, loss, optimizer, epochs,
                           batch_size, seed, device, shared, fit, lambda fits, **kw: TrainerStackBank([f.head.layers for f in fits], **kw))


def _cross_validate(embeddings, targets, classes, hidden, activations, folds, groups, fold_of_row, grid, loss, optimizer, epochs,
                    batch_size, seed, device, shared, fit, bank_of) -> CrossValidation:
    """The body of ``cross_validate_head`` and ``cross_validate_stack``: ``fit`` is ``fit_heads`` or ``fit_stacks`` with the
    shape bound, ``bank_of(fits, ...)`` the bank that holds the fitted members for the out-of-fold forward pass."""
    unknown = sorted(set(shared) - set(MEMBER_KEYS[:-1]))
    if unknown:
        raise ValueError(f"unknown arguments {unknown}")
    classes, widths, acts, (n, host, dev, t_host), _ = check_fit_arguments(
        embeddings, targets, classes, hidden, activations, loss, optimizer, 1e-3, epochs, batch_size, None)
    fold_of_row, k, grid, members = check_cross_validation(t_host, classes, loss, folds, groups, fold_of_row, grid, seed, shared)
    fits = fit(embeddings, targets, classes, members, loss=loss, optimizer=optimizer, epochs=epochs, batch_size=batch_size,
               seed=seed, validation=(embeddings, targets), device=device)
    import torch
    batch = int(batch_size)
    bank = bank_of(fits, loss=loss, optimizer=optimizer, max_batch=batch,
                   device=device if device is not None else (dev.device.index if dev is not None else None))
    try:
        with torch.cuda.device(bank.device):
            X = (dev if dev is not None else torch.from_numpy(host)).to(bank.device)
            if not (X.stride(1) == 1 and X.stride(0) % 4 == 0 and X.data_ptr() % 16 == 0):
                X = X.contiguous().clone()
            c = len(classes)
            logits = torch.empty((n, len(members) * c), dtype=torch.float32, device=bank.device)
            for at in range(0, n, batch):
                b = min(batch, n - at)
                bank.forward_into(X[at:at + b], None, b, logits[at:at + b])
            logits = logits.cpu().numpy().reshape(n, len(members), c)
    finally:
        bank.close()
    positives = (t_host[:, None] == np.arange(c)[None, :]) if loss == "categorical" else (t_host != 0)
    entries = []
    for g in range(len(grid)):
        entry_fits = fits[g * k:(g + 1) * k]
        oof = logits[np.arange(n), g * k + fold_of_row, :].copy()
        entries.append(CrossValidationEntry(oof, entry_fits, [_fold_best(f) for f in entry_fits], classes, positives))
    best = int(np.argmin([np.mean(e.fold_best) for e in entries]))
    return CrossValidation(fold_of_row, grid, entries, best)


def _num(x: float) -> str:
    return f"{x:.15g}"


def metrics_table(logits, positives) -> str:
    """The reference's ``test_model`` product for one class, in the columns of ``tests/metrics.csv``: one row per distinct
    value of the logits rounded to 2 decimals, descending; a window counts as detected when its logit >= the threshold.
    precision = TP / detected (empty where nothing is detected: a threshold that rounding lifted above every logit),
    sensitivity = TP / positives (empty without positives), fpr = FP / negatives (empty without negatives).
    ``results.threshold_for_precision(..., metrics_path=...)`` reads the text as it is.  A sort and a cumulative sum on the
    host."""
    z = np.asarray(logits, dtype=np.float64).ravel()
    pos = np.asarray(positives).ravel().astype(bool)
    if z.shape != pos.shape or z.size == 0:
        raise ValueError("metrics_table takes as many logits as labels, at least one")
    if not np.isfinite(z).all():
        raise ValueError("metrics_table: a logit is not finite")
    order = np.argsort(-z, kind="stable")
    zs = z[order]
    tp_cum = np.concatenate([[0], np.cumsum(pos[order])])
    n_pos, n_neg = int(pos.sum()), int((~pos).sum())
    rows = [METRICS_HEADER]
    for t in np.unique(np.round(z, 2))[::-1]:
        detected = int(np.searchsorted(-zs, -t, side="right"))       # logits >= t
        tp = int(tp_cum[detected])
        fp = detected - tp
        rows.append(",".join((_num(float(t)), _num(tp / detected) if detected else "",
                              _num(tp / n_pos) if n_pos else "", _num(fp / n_neg) if n_neg else "")))
    return "\n".join(rows) + "\n"


def save_model(path: str, fit, metrics: Optional[str] = None, embeddername: str = "yamnet_k2", digits_results: int = 2) -> str:
    """Write ``fit`` (a ``FitResult`` or a ``weights.HeadWeights``) as the model directory ``path`` =
    ``<models>/<modelname>``: what ``HipEngine(modelname=..., models_dir=...)`` and ``analyze(modelname=...)`` load.
    ``metrics``: the text of ``tests/metrics.csv`` (``metrics_table`` of held-out windows); without it ``analyze`` can write
    activations but has no threshold for a precision."""
    head = fit.head if isinstance(fit, FitResult) else fit
    name = os.path.basename(os.path.normpath(path))
    modeldir.write_model_dir(path, head.layers, classes=head.classes, embeddername=embeddername, digits_results=digits_results,
                             metrics=metrics if metrics is not None else METRICS_HEADER + "\n")
    modeldir.write_model_py(path, name, embeddername=embeddername, digits_results=digits_results)
    return path


def combine_logits(member_logits, combine: str = "mean", link: Optional[str] = None, dtype=np.float64) -> np.ndarray:
    """What an ensemble gives for ``member_logits`` = ``[N, K, C]`` (row, member, class), in NumPy at ``dtype``: the statement of
    include/buzzdetect_ensemble.h's formulas that the tests hold the device against, and a user's way to a ``metrics_table`` of
    an ensemble on held-out rows.

    "mean": ``(z[:, 0] + z[:, 1] + ...) * (1 / K)``, added in member order.  "mean_probability" with ``link`` "softmax":
    ``log(mean_m softmax(z_m))``, with "sigmoid": ``logit(mean_m sigmoid(z_m))`` - both in the log domain (per-member
    log-sum-exp over the classes, then a log-sum-exp over the members), finite for every finite input."""
    dtype = np.dtype(dtype).type
    z = np.asarray(member_logits, dtype=dtype)
    if z.ndim != 3 or z.shape[1] < 1:
        raise ValueError(f"combine_logits takes [rows, members, classes], not {tuple(z.shape)}")
    k = z.shape[1]
    one = dtype(1)

    def lse(a, axis):
        m = a.max(axis=axis, keepdims=True)
        return (m + np.log(np.exp(a - m).sum(axis=axis, keepdims=True, dtype=dtype))).squeeze(axis)

    def log_sigmoid(x):
        return np.minimum(x, 0) - np.log1p(np.exp(-np.abs(x)))

    if combine == "mean":
        if link is not None:
            raise ValueError(f'link {link!r} goes with combine "mean_probability" only')
        total = z[:, 0].copy()
        for m in range(1, k):
            total += z[:, m]
        return total * (one / dtype(k))
    if combine != "mean_probability":
        raise ValueError(f"unknown combine {combine!r}; an ensemble combines by mean or mean_probability")
    with np.errstate(over="ignore", under="ignore"):
        if link == "softmax":
            a = np.maximum(z - lse(z, 2)[:, :, None], np.finfo(dtype).min)
            return lse(a, 1) - np.log(dtype(k))
        if link == "sigmoid":
            return lse(log_sigmoid(z), 1) - lse(log_sigmoid(-z), 1)
    raise ValueError(f'combine "mean_probability" needs link "softmax" or "sigmoid", not {link!r}')


def save_ensemble(path: str, fits, *, combine: str = "mean", link: Optional[str] = None, names=None, metrics: Optional[str] = None,
                  embeddername: str = "yamnet_k2", digits_results: int = 2) -> str:
    """Write ``fits`` (``FitResult`` / ``weights.HeadWeights`` with identical classes - the K folds of a cross-validation entry,
    the members of a sweep) as ONE model directory ``path`` = ``<models>/<modelname>`` that is an ensemble: every member an
    ordinary model directory under ``members/<name>/`` (``names``, default ``member0`` ..), ``config_model.json`` with the
    ``"ensemble"`` key.  ``HipEngine(modelname=...)``, ``analyze(modelname=...)`` and the drop-in model load it as they load any
    model and get the members combined on the device (``combine`` / ``link``: ``weights.EnsembleWeights``).  ``metrics`` as
    ``save_model`` takes it.  Everything is checked before anything is written (``ValueError``)."""
    heads = [f.head if isinstance(f, FitResult) else f for f in fits]
    if not heads:
        raise ValueError("save_ensemble needs at least one fit")
    names = [f"member{i}" for i in range(len(heads))] if names is None else [str(n) for n in names]
    if len(names) != len(heads) or len(set(names)) != len(names):
        raise ValueError(f"names must give every one of the {len(heads)} members a name of its own, not {names}")
    for n in names:
        if not n or os.path.basename(n) != n or n in (".", ".."):
            raise ValueError(f"member name {n!r} must be a plain directory name")
    ens = weights.EnsembleWeights(dict(zip(names, heads)), combine, link, list(heads[0].classes), embeddername, digits_results)
    for n, h in ens.members.items():            # the members are written on this embedder, whatever the fits say
        if isinstance(h, weights.EnsembleWeights):
            raise weights.UnsupportedHeadError(f"save_ensemble: member {n!r} is an ensemble itself; ensembles do not nest")
    same = weights.EnsembleWeights({n: weights.HeadWeights(h.layers, h.classes, embeddername) for n, h in ens.members.items()},
                                   combine, link, ens.classes, embeddername, digits_results)
    weights.check_ensemble(same, "save_ensemble")
    weights.check_head_set({os.path.basename(os.path.normpath(path)): same})
    text = metrics if metrics is not None else METRICS_HEADER + "\n"
    modeldir.write_ensemble_dir(path, {n: h.layers for n, h in same.members.items()}, same.classes, combine, link, embeddername,
                                digits_results, text)
    modeldir.write_model_py(path, os.path.basename(os.path.normpath(path)), embeddername=embeddername, digits_results=digits_results)
    return path
