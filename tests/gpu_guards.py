"""Guarded device memory for the hygiene tests (a plain module, imported by the tests that need it).

`Guarded.empty` hands out a view of exactly the requested size inside a larger arena of sentinel words, so that a kernel that
writes in front of or behind what it was given changes a word that belongs to the test, and `check` finds it.  `GuardedEngine`
is a `HipEngine` whose workspace is such a view of exactly the bytes the library asks for, prefilled with one of three
patterns, and whose result tensors are guarded and prefilled with the sentinel."""
import numpy as np

from buzzdetect_amd.engine import HipEngine

SENTINEL = 0x7FC12345            # a NaN payload no kernel produces (tests/test_mix_gpu.py's pattern)
FRONT = 64 << 10                 # bytes of sentinel words in front of every view
BACK = 64 << 10                  # ... and behind it
# behind a workspace: the largest tile (16 windows) times the largest per-window buffer (98304 floats = 393 216 bytes) is about
# 6 MiB, rounded up - an overrun of one tile stays inside the test's own allocation
BACK_WORKSPACE = 8 << 20

# fill patterns, as 32-bit words
ZERO = 0
NAN = 0x7FC17FC1                 # a NaN as f32 and as both f16 halves (v_max drops NaNs: a range maximum never sees them)
HUGE = 0x7B007B00                # 6.7e35 as f32, 57344 in each f16 half: finite everywhere, trips every range guard that looks
PATTERNS = (ZERO, NAN, HUGE)
PATTERN_NAMES = {ZERO: "ZERO", NAN: "NAN", HUGE: "HUGE", SENTINEL: "SENTINEL"}


def _signed(word: int) -> int:
    word &= 0xFFFFFFFF
    return word - (1 << 32) if word >= 1 << 31 else word


def _word_bytes(word: int) -> np.ndarray:
    return np.array([word & 0xFFFFFFFF], dtype="<u4").view(np.uint8)


class Guarded:
    """Device buffers between guard words.  Arenas stay referenced until `check`."""

    def __init__(self, device="cuda"):
        self.device = device
        self.whole = []          # (name, arena as int32, bytes of the view, fill word, expect it written)

    def empty(self, shape, dtype, fill=SENTINEL, back=BACK, name=None, written=True):
        """A `dtype` tensor of `shape`: exactly that many bytes of an int32 arena that starts as sentinel words everywhere, the
        view itself as `fill` words; 256-byte aligned.  `written`: whether `check(written=True)` expects every whole word of
        the view to have lost the sentinel (only asked of views that start as sentinels)."""
        import torch
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
        assert FRONT % 256 == 0 and back % 4 == 0
        inner = (nbytes + 3) // 4
        raw = torch.full((FRONT // 4 + inner + back // 4,), _signed(SENTINEL), dtype=torch.int32, device=self.device)
        assert raw.data_ptr() % 256 == 0 or not raw.is_cuda
        if fill != SENTINEL and inner:
            raw[FRONT // 4:FRONT // 4 + inner] = _signed(fill)
            if nbytes % 4:           # the bytes of the last word that lie behind the view are guard bytes
                tail = torch.from_numpy(_word_bytes(SENTINEL)[nbytes % 4:].copy()).to(raw.device)
                raw.view(torch.uint8)[FRONT + nbytes:FRONT + 4 * inner] = tail
        self.whole.append((name or f"buffer {len(self.whole)}", raw, nbytes, fill, written and fill == SENTINEL))
        view = raw.view(torch.uint8)[FRONT:FRONT + nbytes].view(dtype).view(*shape)
        assert view.data_ptr() % 256 == 0 or nbytes == 0 or not raw.is_cuda
        return view

    @staticmethod
    def _first_changed(words):
        """Index of the first int32 of `words` that is not the sentinel, or None; compared on the device."""
        bad = (words != _signed(SENTINEL)).nonzero()
        return int(bad[0, 0]) if bad.numel() else None

    def check(self, written=True):
        """Synchronises, then fails with the name and byte offset (relative to the view's first byte) of the first guard word
        that changed; with `written` also when a whole word inside a sentinel-prefilled view still holds the sentinel."""
        import torch
        torch.cuda.synchronize()
        assert self.whole, "nothing was allocated since the last check"
        whole, self.whole = self.whole, []
        for name, raw, nbytes, fill, expect_written in whole:
            at = self._first_changed(raw[:FRONT // 4])
            assert at is None, f"{name}: the guard word at byte offset {4 * at - FRONT} (in front of the buffer) changed"
            inner = (nbytes + 3) // 4
            if nbytes % 4:
                got = raw.view(torch.uint8)[FRONT + nbytes:FRONT + 4 * inner].cpu().numpy()
                assert np.array_equal(got, _word_bytes(SENTINEL)[nbytes % 4:]), \
                    f"{name}: a guard byte at byte offset {nbytes} (right behind the buffer) changed"
            at = self._first_changed(raw[FRONT // 4 + inner:])
            assert at is None, f"{name}: the guard word at byte offset {4 * (inner + at)} ({4 * (inner + at) - nbytes} bytes " \
                               f"behind the buffer's {nbytes}) changed"
            if written and expect_written and nbytes >= 4:
                left = (raw[FRONT // 4:FRONT // 4 + nbytes // 4] == _signed(SENTINEL)).nonzero()
                assert not left.numel(), f"{name}: the word at byte offset {4 * int(left[0, 0])} was not written " \
                                         f"({left.shape[0]} of {nbytes // 4} words were not)"


def grow(view, extra_bytes: int):
    """The uint8 `view` of a guarded arena, made `extra_bytes` longer into its back guard (negative control: a caller that
    hands the library more than the helper believes)."""
    return view.as_strided((view.numel() + int(extra_bytes),), (1,), view.storage_offset())


class GuardedEngine(HipEngine):
    """A HipEngine whose workspace is, for every call, a fresh guarded tensor of exactly the bytes the library asked for,
    filled with `pattern` (the library is told that exact size), and whose result tensors (embeddings, logits, stage taps)
    are guarded and start as sentinels.  `exact = False` switches both off: the engine then behaves as its base class does,
    with a workspace that only grows and keeps what earlier calls left in it."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.guards = Guarded(self.device)
        self.pattern = ZERO
        self.exact = True
        self.workspace_slack = 0         # negative controls: bytes handed to the library beyond what the helper guards,
        self.workspace_short = 0         # and bytes of what the library asked for that the helper counts as guard already

    def _ws(self, nbytes: int):
        import torch
        if not self.exact:
            return super()._ws(nbytes)
        extra = self.workspace_short + self.workspace_slack
        assert 0 <= extra <= BACK_WORKSPACE // 2 and self.workspace_short < nbytes
        ws = self.guards.empty((int(nbytes) - self.workspace_short,), torch.uint8, fill=self.pattern, back=BACK_WORKSPACE,
                               name=f"workspace ({PATTERN_NAMES[self.pattern]})")
        return grow(ws, extra) if extra else ws

    def _empty(self, shape):
        import torch
        if not self.exact:
            return super()._empty(shape)
        return self.guards.empty(shape, torch.float32, name=f"result {tuple(shape)}")

    def check_workspace(self, written=True):
        """No guard word of the workspaces and results handed out since the last check changed; every result word is written."""
        self.guards.check(written=written)
