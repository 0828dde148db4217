"""Fit a classifier head on the GPU and save it as a model directory (include/buzzdetect_train.h, csrc/headtrain.hip).

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


class Trainer:
    """``bd_trainer_*`` on torch tensors: ``layers`` = [(kernel [in, out], bias [out], activation)] are the initial values."""

    def __init__(self, layers, loss: str = "categorical", optimizer: str = "adam", learning_rate: float = 1e-3,
                 beta_1: float = 0.9, beta_2: float = 0.999, epsilon: float = 1e-7, max_batch: int = 256,
                 device: Optional[int] = None):
        import torch
        self._handle = C.c_void_p()
        self._lib = _lib.load()
        if loss not in _lib.TRAIN_LOSSES:
            raise ValueError(f'loss must be one of {sorted(_lib.TRAIN_LOSSES)}, not "{loss}"')
        if optimizer not in _lib.TRAIN_OPTIMIZERS:
            raise ValueError(f'optimizer must be one of {sorted(_lib.TRAIN_OPTIMIZERS)}, not "{optimizer}"')
        if not torch.cuda.is_available():
            raise RuntimeError("buzzdetect_amd: no HIP device visible to PyTorch; the trainer has no CPU path")
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        self.loss = loss
        self.max_batch = int(max_batch)
        self.shapes = [tuple(np.shape(k)) for k, _, _ in layers]
        self.n_out = self.shapes[-1][1]
        arr = (_lib.bd_head_layer * len(layers))()
        keep = []
        for i, (kernel, bias, activation) in enumerate(layers):
            k = np.ascontiguousarray(kernel, dtype=np.float32)
            b = np.ascontiguousarray(bias, dtype=np.float32)
            keep += [k, b]
            arr[i].kernel = k.ctypes.data_as(C.POINTER(C.c_float))
            arr[i].bias = b.ctypes.data_as(C.POINTER(C.c_float))
            arr[i].n_in, arr[i].n_out = k.shape
            arr[i].activation = _lib.HEAD_ACTIVATIONS[activation]
        opt = _lib.bd_train_optimizer(_lib.TRAIN_OPTIMIZERS[optimizer], learning_rate, beta_1, beta_2, epsilon, 0)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.bd_trainer_create(self.device_index, arr, len(layers), _lib.TRAIN_LOSSES[loss], C.byref(opt),
                                                   self.max_batch, C.byref(self._handle)))
            self._loss_word = torch.zeros(1, dtype=torch.float32, device=self.device)

    def close(self) -> None:
        if getattr(self, "_handle", None) is not None and self._handle.value:
            self._lib.bd_trainer_destroy(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _batch(self, X, rows, targets, B, weights=None):
        import torch
        if weights is not None and (weights.dtype != torch.float32 or not weights.is_contiguous() or weights.numel() < B
                                    or weights.device != self.device):
            raise ValueError("weights must be a contiguous float32 tensor of at least B entries on the trainer's device")
        if X.dtype != torch.float32 or X.dim() != 2 or X.stride(1) != 1 or X.device != self.device:
            raise ValueError("X must be a float32 [N, >= 1024] matrix on the trainer's device with unit column stride")
        if rows is not None and (rows.dtype != torch.int32 or not rows.is_contiguous() or rows.numel() < B):
            raise ValueError("rows must be a contiguous int32 tensor of at least B entries")
        want = torch.float32 if self.loss == "binary" else torch.int32
        if targets.dtype != want or not targets.is_contiguous() or targets.numel() < B * (self.n_out if self.loss == "binary" else 1):
            raise ValueError(f"targets must be a contiguous {want} tensor covering the batch")
        if rows is None and X.shape[0] < B:
            raise ValueError("X has fewer than B rows")
        return (C.c_void_p(X.data_ptr()), X.stride(0), C.c_void_p(rows.data_ptr()) if rows is not None else None,
                C.c_void_p(targets.data_ptr()), int(B), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))

    def step(self, X, rows, targets, B: int, weights=None) -> None:
        """One optimisation step on ``B`` rows: ``rows`` (int32, device) names them in ``X``, or None for the first ``B``;
        ``targets`` are in batch order, and so are ``weights`` (float32, device: the rows' loss weights; None runs the
        unweighted kernels).  Enqueued on the current stream."""
        x, ldx, r, t, b, stream = self._batch(X, rows, targets, B, weights)
        if weights is None:
            _lib.check(self._lib.bd_trainer_step(self._handle, x, ldx, r, t, b, stream))
        else:
            _lib.check(self._lib.bd_trainer_step_weighted(self._handle, x, ldx, r, t, C.c_void_p(weights.data_ptr()), b, stream))

    def loss_into(self, X, rows, targets, B: int, out, weights=None) -> None:
        """Forward pass and mean (with ``weights``: weighted, still divided by ``B``) loss of the batch into the device float
        ``out[0]`` (no synchronisation)."""
        x, ldx, r, t, b, stream = self._batch(X, rows, targets, B, weights)
        if weights is None:
            _lib.check(self._lib.bd_trainer_loss(self._handle, x, ldx, r, t, b, C.c_void_p(out.data_ptr()), stream))
        else:
            _lib.check(self._lib.bd_trainer_loss_weighted(self._handle, x, ldx, r, t, C.c_void_p(weights.data_ptr()), b,
                                                          C.c_void_p(out.data_ptr()), stream))

    def loss_of(self, X, rows, targets, B: int, weights=None) -> float:
        self.loss_into(X, rows, targets, B, self._loss_word, weights)
        return float(self._loss_word.cpu()[0])

    def set_weight_decay(self, weight_decay: float) -> None:
        """Decoupled decay of the steps from now on: kernels (not biases) shrink by ``lr * weight_decay`` of themselves
        before the optimizer's update.  0 switches it off."""
        _lib.check(self._lib.bd_trainer_set_weight_decay(self._handle, float(weight_decay)))

    def set_learning_rate(self, learning_rate: float) -> None:
        """The learning rate of the steps from now on."""
        _lib.check(self._lib.bd_trainer_set_learning_rate(self._handle, float(learning_rate)))

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def snapshot(self) -> None:
        """Copy the parameters (not Adam's slots, not the step count) to the trainer's second buffer, on the current stream."""
        _lib.check(self._lib.bd_trainer_snapshot(self._handle, self._stream()))

    def restore(self) -> None:
        """Copy the last ``snapshot`` back over the parameters, on the current stream; an error if there is none."""
        _lib.check(self._lib.bd_trainer_restore(self._handle, self._stream()))

    def _pair(self, fn, layer: int) -> Tuple[np.ndarray, np.ndarray]:
        k, n = self.shapes[layer]
        w, b = np.empty((k, n), dtype=np.float32), np.empty(n, dtype=np.float32)
        _lib.check(fn(self._handle, layer, w.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)))
        return w, b

    def gradients(self, layer: int) -> Tuple[np.ndarray, np.ndarray]:
        """(dW, db) of the last step."""
        return self._pair(self._lib.bd_trainer_gradients, layer)

    def read(self, layer: int) -> Tuple[np.ndarray, np.ndarray]:
        """(kernel, bias) as they stand."""
        return self._pair(self._lib.bd_trainer_read, layer)

    def logits(self, B: int) -> np.ndarray:
        """The logits of the last ``step`` / ``loss_*`` call's ``B`` rows."""
        out = np.empty((B, self.n_out), dtype=np.float32)
        _lib.check(self._lib.bd_trainer_logits(self._handle, B, out.ctypes.data_as(C.c_void_p)))
        return out

    def mean_loss(self, reset: bool = True) -> float:
        """Mean training loss per row over the steps since the last reset (accumulated on the device)."""
        v = C.c_float()
        _lib.check(self._lib.bd_trainer_mean_loss(self._handle, 1 if reset else 0, C.byref(v)))
        return float(v.value)

    def set_fusion(self, fused: bool) -> None:
        _lib.check(self._lib.bd_trainer_set_fusion(self._handle, 1 if fused else 0))

    def workspace_fill(self, pattern: int) -> None:
        _lib.check(self._lib.bd_trainer_workspace_fill(self._handle, pattern))

    def workspace(self) -> np.ndarray:
        out = np.empty(_lib.check(self._lib.bd_trainer_workspace_floats(self._handle)), dtype=np.float32)
        _lib.check(self._lib.bd_trainer_workspace_read(self._handle, out.ctypes.data_as(C.c_void_p), out.size))
        return out


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
