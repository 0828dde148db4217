"""The device-side decoder state flacio.FlacDecoder and pcmio.PcmDecoder share (a module of its own: flacio imports pcmio)."""
from __future__ import annotations

import ctypes as C

from . import _lib


class DeviceDecoder:
    """One thread's device-side decoder state: the staged (compressed) bytes of a range, the workspace and the status
    record, all grown on demand and reused (the caller synchronises its stream before the next use).  A format names its
    status struct and its two ABI functions; the header those take is the track's (`track.header`)."""

    status_type = workspace_fn = decode_fn = None
    ws_zeroed = 0                     # bytes of a workspace that starts, and grows, zeroed (0: uninitialised, grown like `comp`)

    def __init__(self, torch, device):
        self._torch, self._device = torch, device
        lib = _lib.load()
        self._workspace_bytes, self._decode = getattr(lib, self.workspace_fn), getattr(lib, self.decode_fn)
        self.comp = None
        self.ws = torch.zeros(self.ws_zeroed, dtype=torch.uint8, device=device) if self.ws_zeroed else None
        self.status = torch.zeros(C.sizeof(self.status_type), dtype=torch.uint8, device=device)
        self.status_host = torch.zeros(C.sizeof(self.status_type), dtype=torch.uint8).pin_memory()

    def _grow(self, buf, nbytes: int, zeroed: bool = False):
        if buf is not None and buf.numel() >= nbytes:
            return buf
        if zeroed:
            return self._torch.zeros(nbytes, dtype=self._torch.uint8, device=self._device)
        return self._torch.empty(max(int(nbytes * 1.25), 1 << 20), dtype=self._torch.uint8, device=self._device)

    def staging(self, nbytes: int):
        """The device buffer a range of `nbytes` goes to (rounded up to 4 bytes, as the decode kernels read)."""
        self.comp = self._grow(self.comp, (nbytes + 3) // 4 * 4 + 8)
        return self.comp

    def decode(self, track, nbytes: int, first: int, n: int, out_ptr: int, stream) -> None:
        """Enqueue the decode of the staged range on `stream`; `result` reads the status once the stream is synchronised."""
        header = C.byref(track.header)
        self.ws = self._grow(self.ws, _lib.check(self._workspace_bytes(header, nbytes, n)), bool(self.ws_zeroed))
        _lib.check(self._decode(self.comp.data_ptr(), nbytes, header, first, n, out_ptr, self.ws.data_ptr(), self.ws.numel(),
                                self.status.data_ptr(), stream.cuda_stream))
        with self._torch.cuda.stream(stream):
            self.status_host.copy_(self.status, non_blocking=True)

    def result(self):
        return self.status_type.from_buffer_copy(self.status_host.numpy().tobytes())
