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

Out of scope: class or sample weights, dropout, regularisation, learning-rate schedules, early stopping, ``.keras`` / ``.h5``
output, multi-GPU training, and training anything below the embedding.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, modeldir, weights

HIDDEN_ACTIVATIONS = ("linear", "relu", "sigmoid", "tanh")
METRICS_HEADER = '"threshold","precision","sensitivity","fpr"'


@dataclass
class FitResult:
    """``head``: what ``HipEngine(head=...)`` and ``save_model`` take (the last layer linear: the engine's outputs are the
    logits the loss was computed from).  ``history``: per-epoch mean ``loss`` and, with a validation set, ``val_loss``."""
    head: weights.HeadWeights
    history: Dict[str, List[float]] = field(default_factory=dict)


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

    def _batch(self, X, rows, targets, B):
        import torch
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

    def step(self, X, rows, targets, B: int) -> None:
        """One optimisation step on ``B`` rows: ``rows`` (int32, device) names them in ``X``, or None for the first ``B``;
        ``targets`` are in batch order.  Enqueued on the current stream."""
        x, ldx, r, t, b, stream = self._batch(X, rows, targets, B)
        _lib.check(self._lib.bd_trainer_step(self._handle, x, ldx, r, t, b, stream))

    def loss_into(self, X, rows, targets, B: int, out) -> None:
        """Forward pass and mean loss of the batch into the device float ``out[0]`` (no synchronisation)."""
        x, ldx, r, t, b, stream = self._batch(X, rows, targets, B)
        _lib.check(self._lib.bd_trainer_loss(self._handle, x, ldx, r, t, b, C.c_void_p(out.data_ptr()), stream))

    def loss_of(self, X, rows, targets, B: int) -> float:
        self.loss_into(X, rows, targets, B, self._loss_word)
        return float(self._loss_word.cpu()[0])

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
    if not (np.isfinite(learning_rate) and learning_rate > 0):
        raise ValueError("learning_rate must be positive and finite")
    if int(epochs) < 1:
        raise ValueError("epochs must be at least 1")
    if not 1 <= int(batch_size) <= _lib.TRAIN_MAX_BATCH:
        raise ValueError(f"batch_size must lie in 1..{_lib.TRAIN_MAX_BATCH}")
    n, host, dev = _check_matrix(embeddings, "embeddings")
    t = _check_targets(targets, n, len(classes), loss, "targets")
    val = None
    if validation is not None:
        if len(validation) != 2:
            raise ValueError("validation must be (embeddings, targets)")
        vn, vhost, vdev = _check_matrix(validation[0], "validation embeddings")
        val = (vn, vhost, vdev, _check_targets(validation[1], vn, len(classes), loss, "validation targets"))
    return classes, widths, activations + ["linear"], (n, host, dev, t), val


def fit_head(embeddings, targets, classes, hidden=(), activations=(), loss="categorical", optimizer="adam", learning_rate=1e-3,
             epochs=10, batch_size=256, seed=0, validation=None, device=None) -> FitResult:
    """Train ``1024 -> hidden... -> len(classes)`` on ``embeddings`` ([N, 1024] float32: array, torch tensor or
    ``DeviceResult``; a device tensor is used where it is) and ``targets`` (``int[N]`` for ``loss="categorical"``, ``float[N, C]``
    multi-hot for ``"binary"``).  ``activations`` name the hidden layers' (linear, relu, sigmoid, tanh); the last layer is
    trained on raw logits and saved linear.  Glorot-uniform kernels, zero biases and one permutation per epoch come from
    ``np.random.default_rng(seed)`` in that order; the last batch of an epoch is ragged, not dropped.  ``validation`` =
    (embeddings, targets) adds ``val_loss`` to the history.  Same arguments, same bits.

    ``ValueError`` before any device work: shapes, labels outside ``0..C-1``, an unsupported activation (softmax among the
    hidden ones included), non-finite inputs, ``len(classes) != C``.

    Not offered: class or sample weights, dropout, regularisation, learning-rate schedules, early stopping, ``.keras`` /
    ``.h5`` output, multi-GPU training, training below the embedding."""
    classes, widths, acts, (n, host, dev, t_host), val = check_fit_arguments(
        embeddings, targets, classes, hidden, activations, loss, optimizer, learning_rate, epochs, batch_size, validation)
    import torch
    rng = np.random.default_rng(seed)
    layers = glorot_layers(rng, widths, acts)
    batch = int(batch_size)
    trainer = Trainer(layers, loss, optimizer, learning_rate, max_batch=batch,
                      device=device if device is not None else (dev.device.index if dev is not None else None))
    try:
        with torch.cuda.device(trainer.device):
            def resident(h, d):
                x = d if d is not None else torch.from_numpy(h)
                x = x.to(trainer.device)
                return x if x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 else x.contiguous().clone()

            X = resident(host, dev)
            T = torch.from_numpy(t_host).to(trainer.device)
            if val is not None:
                VX, VT = resident(val[1], val[2]), torch.from_numpy(val[3]).to(trainer.device)
                val_word = torch.zeros(1, dtype=torch.float32, device=trainer.device)
                val_sum = torch.zeros(1, dtype=torch.float64, device=trainer.device)
            history: Dict[str, List[float]] = {"loss": []}
            if val is not None:
                history["val_loss"] = []
            for _ in range(int(epochs)):
                perm = torch.from_numpy(rng.permutation(n).astype(np.int32)).to(trainer.device)
                t_epoch = T[perm.long()].contiguous()                   # targets in batch order, once per epoch
                for at in range(0, n, batch):
                    b = min(batch, n - at)
                    trainer.step(X, perm[at:at + b], t_epoch[at:at + b], b)
                if val is not None:
                    val_sum.zero_()
                    for at in range(0, val[0], batch):
                        b = min(batch, val[0] - at)
                        trainer.loss_into(VX[at:at + b], None, VT[at:at + b], b, val_word)
                        val_sum.add_(val_word.double(), alpha=b)
                history["loss"].append(trainer.mean_loss(reset=True))    # the one read of the epoch (waits for the stream)
                if val is not None:
                    history["val_loss"].append(float(val_sum.cpu()[0]) / val[0])
            out = [trainer.read(l) + (a,) for l, a in enumerate(acts)]
    finally:
        trainer.close()
    return FitResult(weights.HeadWeights(out, classes, source="fit_head"), history)


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
