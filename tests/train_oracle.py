"""A NumPy restatement of what the head trainer computes (include/buzzdetect_train.h): forward pass, both losses from logits in
their overflow-safe forms, backward pass, SGD and Keras's Adam.  ``dtype`` is the arithmetic: float64 is the reference, float32
the yardstick for what float32 sums of the same terms in another order may differ by (tests/test_train_gpu.py).

Layers are [(kernel [in, out], bias [out], activation)]; the last layer's activation is not applied (the losses read logits).
"""
import numpy as np


def act_forward(x, act):
    if act == "relu":
        return np.maximum(x, 0)
    if act == "sigmoid":
        return 1 / (1 + np.exp(-x))
    if act == "tanh":
        return np.tanh(x)
    assert act == "linear", act
    return x


def act_gradient(y, act):
    """d act / d pre-activation from the activation's value."""
    if act == "relu":
        return (y > 0).astype(y.dtype)
    if act == "sigmoid":
        return y * (1 - y)
    if act == "tanh":
        return 1 - y * y
    assert act == "linear", act
    return np.ones_like(y)


def cast_layers(layers, dtype):
    return [(np.asarray(k, dtype=dtype).copy(), np.asarray(b, dtype=dtype).copy(), a) for k, b, a in layers]


def forward(layers, x, dtype=np.float64):
    """[x, y_1, ..., logits]."""
    ys = [np.asarray(x, dtype=dtype)]
    for i, (k, b, act) in enumerate(layers):
        pre = ys[-1] @ np.asarray(k, dtype=dtype) + np.asarray(b, dtype=dtype)
        ys.append(pre if i == len(layers) - 1 else act_forward(pre, act))
    return ys


def loss_and_delta(z, targets, loss, dtype=np.float64):
    """(mean loss, d loss / d logits)."""
    z = np.asarray(z, dtype=dtype)
    n, c = z.shape
    if loss == "categorical":
        labels = np.asarray(targets).astype(np.int64)
        m = z.max(axis=1, keepdims=True)
        e = np.exp(z - m)
        s = e.sum(axis=1, keepdims=True)
        rows = (m[:, 0] + np.log(s[:, 0])) - z[np.arange(n), labels]
        onehot = np.zeros_like(z)
        onehot[np.arange(n), labels] = 1
        return rows.sum() / dtype(n), (e / s - onehot) / dtype(n)
    assert loss == "binary", loss
    t = np.asarray(targets, dtype=dtype)
    e = np.exp(-np.abs(z))
    rows = (np.maximum(z, 0) - z * t) + np.log1p(e)
    sig = np.where(z >= 0, 1 / (1 + e), e / (1 + e))
    return rows.sum() / dtype(n * c), (sig - t) / dtype(n * c)


def mean_loss(layers, x, targets, loss, dtype=np.float64):
    return loss_and_delta(forward(layers, x, dtype)[-1], targets, loss, dtype)[0]


def gradients(layers, x, targets, loss, dtype=np.float64):
    """(mean loss, [(dW, db) per layer])."""
    ys = forward(layers, x, dtype)
    value, g = loss_and_delta(ys[-1], targets, loss, dtype)
    grads = [None] * len(layers)
    for i in range(len(layers) - 1, -1, -1):
        grads[i] = (ys[i].T @ g, g.sum(axis=0))
        if i > 0:
            g = (g @ np.asarray(layers[i][0], dtype=dtype).T) * act_gradient(ys[i], layers[i - 1][2])
    return value, grads


class Sgd:
    def __init__(self, learning_rate=1e-2, dtype=np.float64):
        self.lr, self.dtype = dtype(np.float32(learning_rate)), dtype      # the rate as the device holds it

    def apply(self, layers, grads):
        return [(k - self.lr * dk, b - self.lr * db, a) for (k, b, a), (dk, db) in zip(layers, grads)]


class Adam:
    """Keras: m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, w -= lr sqrt(1 - b2^t) / (1 - b1^t) m / (sqrt(v) + eps)."""

    def __init__(self, learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7, dtype=np.float64):
        self.lr, self.dtype = float(learning_rate), dtype
        # the betas and epsilon as the device holds them (float32 values), in this restatement's arithmetic
        self.b1, self.b2, self.eps = dtype(np.float32(beta_1)), dtype(np.float32(beta_2)), dtype(np.float32(epsilon))
        self.t = 0
        self.slots = None

    def apply(self, layers, grads):
        dt = self.dtype
        if self.slots is None:
            self.slots = [[np.zeros_like(np.asarray(p, dtype=dt)) for p in (k, k, b, b)] for k, b, _ in layers]
        self.t += 1
        b1, b2 = float(np.float32(self.b1)), float(np.float32(self.b2))
        lr_t = dt(np.float32(float(np.float32(self.lr)) * np.sqrt(1.0 - b2 ** self.t) / (1.0 - b1 ** self.t)))
        out = []
        for (k, b, a), (dk, db), s in zip(layers, grads, self.slots):
            new = []
            for j, (p, g) in enumerate(((k, dk), (b, db))):
                s[2 * j] = self.b1 * s[2 * j] + (1 - self.b1) * g
                s[2 * j + 1] = self.b2 * s[2 * j + 1] + (1 - self.b2) * (g * g)
                new.append(p - lr_t * s[2 * j] / (np.sqrt(s[2 * j + 1]) + self.eps))
            out.append((new[0], new[1], a))
        return out


def train(layers, x, batches, loss, optimizer, dtype=np.float64):
    """Steps over ``batches`` = [(row numbers, targets in batch order)]: the layers after the last step."""
    layers = cast_layers(layers, dtype)
    x = np.asarray(x, dtype=dtype)
    for rows, targets in batches:
        _, grads = gradients(layers, x[rows], targets, loss, dtype)
        layers = optimizer.apply(layers, grads)
    return layers


def bound(f32_value, f64_value, factor=8.0, floor=1e-7):
    """What a float32 computation of the same terms in another order may differ from float64 by: ``factor`` x the float32
    restatement's own deviation; that deviation counts as at least ``floor`` x max |reference| (an exactly-zero float32 error
    must not demand bit equality)."""
    f64_value = np.asarray(f64_value, dtype=np.float64)
    dev = float(np.abs(np.asarray(f32_value, dtype=np.float64) - f64_value).max())
    return factor * max(dev, floor * float(np.abs(f64_value).max())), dev
