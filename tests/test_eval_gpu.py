"""The threshold sweep on the GPU (csrc/evalsweep.hip, buzzdetect_amd/evaluate.py): the device state against the host
routine's in every word on the generator's cases (tests/eval_cases.py) across the wave, workgroup and slice edges and both
layouts, a 16-bit counter at its maximum, slices adding to one word, untouched columns, columns together against one at a
time, the same call twice, a slice of a wider tensor, and memory hygiene between the guard words of tests/gpu_guards.Guarded."""
import functools

import numpy as np
import pytest

from buzzdetect_amd import _lib, evaluate as E
from tests import eval_cases as K

pytestmark = pytest.mark.gpu

SLICE = _lib.EVAL_SLICE
WINDOWS = (1, 64, 65, 1024, 1025, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 5)      # wave, workgroup and slice edges
assert WINDOWS[-1] == 65541


@functools.lru_cache(maxsize=None)
def case(c):
    """The largest case of c columns, drawn once and left unchanged; the smaller ones are its first rows."""
    return K.draw(500 + c, WINDOWS[-1], c)


@pytest.fixture(scope="module")
def guarded_sweep():
    import torch
    from tests.gpu_guards import Guarded
    assert torch.cuda.is_available()

    class GuardedSweep(E.Sweep):
        guards = Guarded()

        def _empty(self, shape, dtype):
            return self.guards.empty(shape, dtype, name=f"{tuple(shape)} {dtype}")

    return GuardedSweep


def on_device(x, which):
    import torch
    dev = torch.from_numpy(K.layout(x, which)).cuda()
    if which == "columns" and x.shape[0] > 1 and x.shape[1] > 1:
        assert dev.stride() == (1, x.shape[0])
    return dev


@pytest.mark.parametrize("which", ("rows", "columns"))
@pytest.mark.parametrize("c", (1, 2, 13, 64))
def test_device_state_is_the_host_state_in_every_word(guarded_sweep, c, which):
    x, labels, label_of = case(c)
    tails = np.zeros(4, np.int64)
    for w in WINDOWS:
        hist, tail = E.sweep_host(x[:w], labels[:w], label_of, labels.shape[1])
        sweep = guarded_sweep(label_of, labels.shape[1])
        sweep.update(on_device(x[:w], which), labels[:w])
        got = sweep.counts()
        sweep.guards.check()
        assert got[0].dtype == np.uint32 and np.array_equal(got[0], hist), (w, c)
        assert np.array_equal(got[1], tail), (w, c)
        tails += tail.sum(axis=0).astype(np.int64)
    assert (tails > 0).all()
    if c == 2 and which == "rows":                          # one case once more against the definitions themselves
        want = K.sweep_numpy(x, labels, label_of)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("w", (SLICE, 2 * SLICE + 5))
def test_every_row_of_a_column_in_one_bin(guarded_sweep, w):
    """A slice's 32 768 rows in one bin put a 16-bit counter at 0x8000, in the low half of its word (an even bin, column 0) and
    in the high half (an odd bin, column 1); 65 541 rows are three slices adding to the same global words."""
    import torch
    x = np.empty((w, 3), np.float32)
    x[:, 0], x[:, 1] = 0.5, 0.515                           # kf = kr = 50: bin 8242 (even); kf = kr = 51: bin 8243 (odd)
    x[:, 2] = np.where(np.arange(w) % 2 == 0, np.float32(0.5), np.float32(0.515))      # both halves of one word
    labels = np.stack([np.ones(w, np.uint8), np.zeros(w, np.uint8)], axis=1)
    label_of = np.array([0, 1, 0], np.int32)
    sweep = guarded_sweep(label_of, 2)
    sweep.update(torch.from_numpy(x).cuda(), labels)
    hist, tail = sweep.counts()
    sweep.guards.check()
    want = E.sweep_host(x, labels, label_of, 2)
    assert np.array_equal(hist, want[0]) and np.array_equal(tail, want[1]) and not tail.any()
    even, odd = 50 - K.K_MIN, 51 - K.K_MIN
    assert even % 2 == 0 and hist[0, 1, even] == w == hist[0, 2, even] and hist[0].sum() == 2 * w
    assert hist[1, 0, odd] == w == hist[1, 2, odd] and hist[1].sum() == 2 * w
    assert hist[2, 1, even] == (w + 1) // 2 and hist[2, 1, odd] == w // 2 and hist[2].sum() == 2 * w


def test_the_call_adds_and_a_column_without_labels_stays_bit_untouched():
    """Straight to the library with a state that starts as the guard pattern: evaluated columns end as pattern + counts, the
    column with label_of -1 keeps every bit, and no word in front of or behind hist and tail changes."""
    import torch
    from tests.gpu_guards import SENTINEL, Guarded
    w, c = SLICE + 77, 3
    x, labels, _ = K.draw(41, w, c, n_labels=2)
    label_of = np.array([1, -1, 0], np.int32)
    lib, guards = _lib.load(), Guarded()
    hist = guards.empty((c, 3, K.BINS), torch.int32, name="hist", written=False)
    tail = guards.empty((c, 4), torch.int32, name="tail", written=False)
    x_dev, labels_dev, of_dev = torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda(), torch.from_numpy(label_of).cuda()
    _lib.check(lib.bd_eval_accumulate(x_dev.data_ptr(), w, c, c, 1, labels_dev.data_ptr(), 2, of_dev.data_ptr(), hist.data_ptr(),
                                      tail.data_ptr(), torch.cuda.current_stream().cuda_stream))
    guards.check(written=False)
    got_hist, got_tail = hist.cpu().numpy().view(np.uint32), tail.cpu().numpy().view(np.uint32)
    want = E.sweep_host(x, labels, label_of, 2)
    assert want[0][0].any() and want[0][2].any() and not want[0][1].any()
    assert np.array_equal(got_hist, want[0] + np.uint32(SENTINEL)) and np.array_equal(got_tail, want[1] + np.uint32(SENTINEL))
    assert (got_hist[1] == SENTINEL).all() and (got_tail[1] == SENTINEL).all()


def test_the_device_entry_refuses_a_bad_label_of_before_any_launch():
    import torch
    from tests.gpu_guards import Guarded
    lib, guards = _lib.load(), Guarded()
    x = torch.ones((8, 2), dtype=torch.float32, device="cuda")
    labels = torch.ones((8, 1), dtype=torch.uint8, device="cuda")
    hist = guards.empty((2, 3, K.BINS), torch.int32, written=False)
    tail = guards.empty((2, 4), torch.int32, written=False)
    for bad, word in ((1, "label_of[1] = 1, allowed are -1..0"), (-2, "label_of[1] = -2")):
        of_dev = torch.tensor([0, bad], dtype=torch.int32, device="cuda")
        rc = lib.bd_eval_accumulate(x.data_ptr(), 8, 2, 2, 1, labels.data_ptr(), 1, of_dev.data_ptr(), hist.data_ptr(),
                                    tail.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == -1 and word in lib.bd_last_error().decode()
    for view in (hist, tail):
        assert (view.cpu().numpy().view(np.uint8).reshape(-1, 4) == np.array([0x45, 0x23, 0xC1, 0x7F], np.uint8)).all()
    guards.check(written=False)


def test_columns_together_are_the_columns_one_at_a_time(guarded_sweep):
    x, labels, label_of = case(13)
    w = SLICE + 1025
    dev = on_device(x[:w], "rows")
    whole = guarded_sweep(label_of, labels.shape[1])
    whole.update(dev, labels[:w])
    hist, tail = whole.counts()
    for col in range(13):
        alone = guarded_sweep(label_of[col:col + 1], labels.shape[1])
        alone.update(dev[:, col:col + 1], labels[:w])
        got = alone.counts()
        assert np.array_equal(got[0][0], hist[col]) and np.array_equal(got[1][0], tail[col]), col
    guarded_sweep.guards.check()


def test_the_same_call_twice_doubles_every_count_and_updates_add_up(guarded_sweep):
    x, labels, label_of = case(13)
    w = SLICE + 65
    dev = on_device(x[:w], "columns")
    sweep = guarded_sweep(label_of, labels.shape[1])
    sweep.update(dev, labels[:w])
    once = sweep.counts()
    sweep.update(dev, labels[:w])
    twice = sweep.counts()
    assert once[0].any() and np.array_equal(twice[0], 2 * once[0]) and np.array_equal(twice[1], 2 * once[1]) and sweep.rows == 2 * w
    parts = guarded_sweep(label_of, labels.shape[1])
    import torch
    for lo, hi in ((0, 0), (0, 1000), (1000, SLICE + 3), (SLICE + 3, w)):        # an empty update launches nothing
        parts.update(dev[lo:hi], torch.from_numpy(labels[lo:hi]))
    got = parts.counts()
    assert np.array_equal(got[0], once[0]) and np.array_equal(got[1], once[1])
    guarded_sweep.guards.check()


def test_a_slice_of_a_wider_tensor_and_the_curves(guarded_sweep):
    import torch
    from buzzdetect_amd import train
    rng = np.random.default_rng(5)
    w = 3000
    wide = rng.normal(0, 2, (w, 20)).astype(np.float32)
    labels = (rng.random((w, 5)) < 0.3).astype(np.uint8)
    dev = torch.from_numpy(wide).cuda()[:, 3:8]
    assert dev.stride() == (20, 1) and not dev.is_contiguous()
    sweep = guarded_sweep(np.arange(5, dtype=np.int32), 5)
    sweep.update(dev, labels)
    want = E.sweep_host(wide[:, 3:8], labels, np.arange(5), 5)
    got = sweep.counts()
    sweep.guards.check()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    curves = sweep.curves(list("abcde"))
    for col in range(5):
        assert curves[col].table() == K.normalised(train.metrics_table(wide[:, 3 + col], labels[:, col] == 1))
    found = E.evaluate_logits(dev, labels, list("abcde"))
    assert found.curves[("model", "c")].table() == curves[2].table()
    with pytest.raises(ValueError, match=r"scores must be a float32 \[W, 5\] tensor"):
        sweep.update(dev[:, :4], labels)
    sweep.close()
    with pytest.raises(ValueError, match="closed"):
        sweep.counts()
