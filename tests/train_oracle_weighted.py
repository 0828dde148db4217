"""tests/train_oracle.py with a weight per row and a decoupled weight decay (include/buzzdetect_train.h): the weighted losses,
their gradients, and SGD / Adam steps that first shrink the kernels.  ``dtype`` is the arithmetic, as there: float64 is the
reference, float32 the yardstick (tests/test_train_weighted_gpu.py).

Weighted loss (Keras's ``sample_weight`` with ``sum_over_batch_size``: divided by B, not by the weights' sum):

    categorical   loss = (1/B) sum_r w_r loss_r              dz_r  = w_r (softmax(z_r) - onehot_r) / B
    binary        loss = (1/(B C)) sum_r w_r sum_c loss_rc   dz_rc = w_r (sigmoid(z_rc) - t_rc) / (B C)

in the device's order of operations: ``scale_r = inv * w_r`` (one product, inv = 1/B or 1/(B C)), the delta is
``(...) * scale_r``, a row's loss is ``w_r * loss_r``.

Decay: ``decay = float32(lr) * float32(weight_decay)``, one float32 product; a kernel element (never a bias) becomes
``p - decay * p``, then the optimizer's update is subtracted from that.
"""
import numpy as np

from tests.train_oracle import Adam, Sgd, act_gradient, cast_layers, forward


def loss_and_delta(z, targets, loss, weights, dtype=np.float64):
    """(weighted mean loss, d loss / d logits)."""
    z = np.asarray(z, dtype=dtype)
    n, c = z.shape
    w = np.asarray(weights, dtype=dtype).reshape(n)
    if loss == "categorical":
        labels = np.asarray(targets).astype(np.int64)
        scale = (dtype(1) / dtype(n)) * w
        m = z.max(axis=1, keepdims=True)
        e = np.exp(z - m)
        s = e.sum(axis=1, keepdims=True)
        rows = w * ((m[:, 0] + np.log(s[:, 0])) - z[np.arange(n), labels])
        onehot = np.zeros_like(z)
        onehot[np.arange(n), labels] = 1
        return rows.sum() / dtype(n), (e / s - onehot) * scale[:, None]
    assert loss == "binary", loss
    t = np.asarray(targets, dtype=dtype)
    scale = (dtype(1) / (dtype(n) * dtype(c))) * w
    e = np.exp(-np.abs(z))
    rows = w * ((np.maximum(z, 0) - z * t) + np.log1p(e)).sum(axis=1)
    sig = np.where(z >= 0, 1 / (1 + e), e / (1 + e))
    return rows.sum() / dtype(n * c), (sig - t) * scale[:, None]


def mean_loss(layers, x, targets, loss, weights, dtype=np.float64):
    return loss_and_delta(forward(layers, x, dtype)[-1], targets, loss, weights, dtype)[0]


def gradients(layers, x, targets, loss, weights, dtype=np.float64):
    """(weighted mean loss, [(dW, db) per layer])."""
    ys = forward(layers, x, dtype)
    value, g = loss_and_delta(ys[-1], targets, loss, weights, dtype)
    grads = [None] * len(layers)
    for i in range(len(layers) - 1, -1, -1):
        grads[i] = (ys[i].T @ g, g.sum(axis=0))
        if i > 0:
            g = (g @ np.asarray(layers[i][0], dtype=dtype).T) * act_gradient(ys[i], layers[i - 1][2])
    return value, grads


def decay_factor(learning_rate, weight_decay, dtype):
    """lr * weight_decay as the host hands it to the device: one float32 product, then in the restatement's arithmetic."""
    return dtype(np.float32(learning_rate) * np.float32(weight_decay))


def decayed(layers, decay):
    return [(k - decay * k, b, a) for k, b, a in layers]


class SgdW(Sgd):
    def __init__(self, learning_rate=1e-2, weight_decay=0.0, dtype=np.float64):
        super().__init__(learning_rate, dtype)
        self.decay = decay_factor(learning_rate, weight_decay, dtype)

    def apply(self, layers, grads):
        return super().apply(decayed(layers, self.decay), grads)


class AdamW(Adam):
    """Keras's AdamW: the kernels shrink by lr * weight_decay (the plain rate, not the bias-corrected one), then Adam."""

    def __init__(self, learning_rate=1e-3, weight_decay=0.0, dtype=np.float64, **kw):
        super().__init__(learning_rate, dtype=dtype, **kw)
        self.decay = decay_factor(learning_rate, weight_decay, dtype)

    def apply(self, layers, grads):
        return super().apply(decayed(layers, self.decay), grads)


def train(layers, x, batches, loss, optimizer, dtype=np.float64):
    """Steps over ``batches`` = [(row numbers, targets in batch order, weights in batch order)]."""
    layers = cast_layers(layers, dtype)
    x = np.asarray(x, dtype=dtype)
    for rows, targets, weights in batches:
        _, grads = gradients(layers, x[rows], targets, loss, weights, dtype)
        layers = optimizer.apply(layers, grads)
    return layers
