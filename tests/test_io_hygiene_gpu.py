"""Memory hygiene of the front end, the resamplers and the decoders, through the C ABI: outputs, workspaces and
status words between guard words and exactly as long as the headers say; NaNs, huge finite values, 0x7FFF words, 0xFF bytes and
valid-looking headers right behind an input's last sample or byte.  Results hold the bits of the same call on a copy of the
input followed by zeros (the decoders: the host decoder's samples and status, which sees nothing behind the range)."""
import ctypes as C

import numpy as np
import pytest

from buzzdetect_amd import _lib, pcmio
from oracle import yamnet_oracle as O
from tests.gpu_guards import BACK_WORKSPACE, HUGE, NAN, PATTERN_NAMES, ZERO, Guarded
from tools import flacgen as FG
from tools import pcmgen as PG

pytestmark = pytest.mark.gpu

HOP = 15360
TAIL = 4096                      # poisoned elements behind an input (then the arena's own guard words, NaNs as floats)
S16_POISON = 0x7FFF7FFF
FF = 0xFFFFFFFF


def stream_of(engine):
    import torch
    return torch.cuda.current_stream(engine.device).cuda_stream


def placed(guards, data, fill, offset=0, name="input"):
    """`data` (a flat array) on the device as a view `offset` elements into an arena of `fill` words, TAIL elements of them
    right behind its last element."""
    import torch
    data = np.ascontiguousarray(data)
    arena = guards.empty((offset + data.size + TAIL,), torch.from_numpy(data[:0].copy()).dtype, fill=fill, name=name)
    view = arena[offset:offset + data.size]
    if data.size:
        view.copy_(torch.from_numpy(data))
    return view


def same_bits(got, want, what):
    got, want = got.cpu().numpy(), want.cpu().numpy()
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), \
        f"{what}: {int((got.view(np.uint32) != want.view(np.uint32)).sum())} of {got.size} words differ"


# ---- front end

def run_frontend(engine, guards, x, fill):
    import torch
    view = placed(guards, x, fill, offset=4)                # 16 bytes into the arena
    assert view.data_ptr() % 16 == 0
    out = guards.empty((engine.num_frames(x.size, HOP), _lib.MEL_BANDS), torch.float32, name="log-mel")
    _lib.check(engine._lib.bd_frontend(engine._handle, view.data_ptr(), x.size, HOP, out.data_ptr(), stream_of(engine)))
    return out


@pytest.mark.parametrize("n", [0, 1, 399, 400, 15360, 15601, 64 * 160 + 240, 64 * 160 + 241])
def test_frontend_reads_zeros_behind_the_last_sample(engine, n):
    guards = Guarded(engine.device)
    x = O.synthetic_audio(max(n, 1), seed=n % 1000)[:n]
    want = run_frontend(engine, guards, x, ZERO)
    assert want.shape[0] >= 96
    for fill in (NAN, HUGE):
        same_bits(run_frontend(engine, guards, x, fill), want, f"log-mel with {PATTERN_NAMES[fill]} behind sample {n - 1}")
    guards.check()


@pytest.mark.parametrize("step", [96, 48, 29])
def test_patches_stay_inside_their_output(engine, step):
    import torch
    guards = Guarded(engine.device)
    logmel = engine.frontend(O.synthetic_audio(HOP * 2 + 15600, seed=5), HOP)
    t = logmel.shape[0]
    w = 1 + (t - _lib.PATCH_FRAMES) // step
    out = guards.empty((w, _lib.PATCH_FRAMES, _lib.MEL_BANDS), torch.float32, name="patches")
    _lib.check(engine._lib.bd_patches(engine._handle, logmel.data_ptr(), t, step, out.data_ptr(), stream_of(engine)))
    guards.check()
    same_bits(out, logmel.unfold(0, _lib.PATCH_FRAMES, step).permute(0, 2, 1).contiguous(), "patches")


# ---- resamplers

@pytest.fixture()
def engine_q(engine, request):
    engine.set_resample_quality(request.param)
    yield engine
    engine.set_resample_quality("hq")


def hold_resampler(engine, fn_f32, fn_s16, rate_in, channels, lengths):
    import torch
    lib = engine._lib

    def run(guards, fn, data, n, fill):
        view = placed(guards, data, fill)
        out = guards.empty((_lib.check(lib.bd_resample_length(n, rate_in, 16000)),), torch.float32, name="resampled")
        _lib.check(fn(engine._handle, view.data_ptr(), n, channels, rate_in, 16000, out.data_ptr(), stream_of(engine)))
        return out

    for n in lengths:
        guards = Guarded(engine.device)
        rng = np.random.default_rng(n + rate_in + channels)
        x = (0.5 * rng.standard_normal(n * channels)).astype(np.float32)
        want = run(guards, fn_f32, x, n, ZERO)
        assert want.numel() == -(-n * 16000 // rate_in)
        for fill in (NAN, HUGE):
            same_bits(run(guards, fn_f32, x, n, fill), want, f"{n} float frames, {PATTERN_NAMES[fill]} behind the last")
        q = rng.integers(-32768, 32767, size=n * channels, dtype=np.int16)
        want = run(guards, fn_s16, q, n, ZERO)
        same_bits(run(guards, fn_s16, q, n, S16_POISON), want, f"{n} 16-bit frames, 0x7FFF behind the last")
        guards.check()


# fir_mfma_kernel with one phase block (48 kHz) and many (44.1 kHz), the vector kernel (192 kHz at "hq", 44.1 kHz at "scipy"),
# decimate_kernel ("scipy" 48 kHz), convert_kernel (16 kHz)
RESAMPLE_CASES = [("hq", 48000), ("hq", 44100), ("hq", 192000), ("scipy", 48000), ("scipy", 44100), ("hq", 16000)]
RESAMPLE_LENGTHS = (1, 7, 61, 5374, 4096 * 3 + 1)           # tests/test_resample.py's test_integer_decimation_edges, the short ones


@pytest.mark.parametrize("channels", [1, 2, 3, 8])
@pytest.mark.parametrize("engine_q,rate_in", RESAMPLE_CASES, indirect=["engine_q"])
def test_resample_reads_zeros_behind_the_last_frame(engine_q, rate_in, channels):
    lib = engine_q._lib
    hold_resampler(engine_q, lib.bd_resample, lib.bd_resample_s16, rate_in, channels, RESAMPLE_LENGTHS)


@pytest.mark.parametrize("channels", [1, 2, 3, 8])
@pytest.mark.parametrize("rate_in", [47999, 768000])
def test_resample_any_reads_zeros_behind_the_last_frame(engine, rate_in, channels):
    lib = engine._lib
    assert lib.bd_anyrate_supported(rate_in, 16000, 1) == 1 and lib.bd_resample_supported(rate_in, 16000, 1) == 0
    hold_resampler(engine, lib.bd_resample_any, lib.bd_resample_any_s16, rate_in, channels, RESAMPLE_LENGTHS)


# ---- decoders: what lies behind the range's last byte

def trailing_variants(seg: bytes, header_like: bytes):
    """(name, workspace pattern, the bytes behind the range): 0xFF - a run of FLAC sync bits - and something that starts as a
    valid header does, repeated.  The 0 .. 3 bytes that round n_bytes up to a multiple of 4 are the first of them."""
    room = (-len(seg)) % 4 + TAIL
    return [("0xFF", NAN, b"\xff" * room), ("a valid header", HUGE, (header_like * (room // len(header_like) + 1))[:room])]


def staged(guards, seg: bytes, behind: bytes):
    import torch
    comp = guards.empty((len(seg) + len(behind),), torch.uint8, fill=FF, name="compressed range")
    comp.copy_(torch.from_numpy(np.frombuffer(seg + behind, np.uint8).copy()))
    return comp


def flac_device(guards, seg, behind, si, first, n, ws_fill, expect_all):
    import torch
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    comp = staged(guards, seg, behind)
    ws = guards.empty((_lib.check(lib.bd_flac_workspace_bytes(C.byref(si), len(seg), n)),), torch.uint8, fill=ws_fill,
                      back=BACK_WORKSPACE, name="flac workspace")
    out = guards.empty((n, si.channels), torch.int16 if si.bits_per_sample == 16 else torch.float32, name="samples",
                       written=expect_all)
    status = guards.empty((C.sizeof(_lib.bd_flac_status),), torch.uint8, name="status")
    stream = torch.cuda.current_stream(dev)
    _lib.check(lib.bd_flac_decode(comp.data_ptr(), len(seg), C.byref(si), first, n, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                  status.data_ptr(), stream.cuda_stream))
    stream.synchronize()
    st = _lib.bd_flac_status.from_buffer_copy(status.cpu().numpy().tobytes())
    got = out.cpu().numpy()
    guards.check()
    return got, st


def flac_host(seg, si, first, n):
    buf = np.frombuffer(seg, np.uint8)
    out = np.zeros((n, si.channels), np.int16 if si.bits_per_sample == 16 else np.float32)
    st = _lib.bd_flac_status()
    _lib.check(_lib.load().bd_flac_decode_host(buf.ctypes.data, buf.size, C.byref(si), first, n, out.ctypes.data, C.byref(st)))
    return out, st


def flac_fields(st):
    return (st.samples, st.stop_offset, st.first_sample, st.end_sample, st.reason, st.frames)


# three rows of tests/test_flac_gpu.py's MATRIX: 16-bit mid/side, 24-bit variable block size, escape-coded
FLAC_ROWS = {
    "16-bit mid/side": (16, 2, 4608, False, "mid_side", ("lpc", 12, 15), "rice2", 3, False),
    "24-bit variable": (24, 2, [4096, 1000, 65535, 16, 333], True, "mid_side", ("lpc", 16, 14), "rice", 0, False),
    "escape-coded": (16, 2, 576, False, "side_right", ("fixed", 3), "escape", 2, False),
}


@pytest.mark.parametrize("row", sorted(FLAC_ROWS))
def test_flac_decode_does_not_read_behind_its_range(row):
    bps, ch, bs, variable, mode, kind, method, po, wasted = FLAC_ROWS[row]
    n = 24_000
    pcm = FG.test_signal(n, ch, bps, seed=len(row))
    data, offs = FG.encode(pcm, 48000, bps, blocksize=bs, variable=variable, mode=mode, subframe_kind=kind, method=method,
                           porder=po, wasted=wasted, return_offsets=True)
    sizes = [bs] if np.isscalar(bs) else bs
    si = _lib.bd_flac_streaminfo(min(sizes), max(sizes), 48000, ch, bps, 0, n)
    header = data[offs[1][1]: offs[1][1] + 16]               # the start of a real frame of this stream: a header that parses
    assert _lib.load().bd_flac_parse_frame_header(header, len(header), C.byref(si), C.byref(_lib.bd_flac_frame_header())) > 0
    lengths = set()
    for a, m in [(0, n), (3, offs[2][0] - 3), (offs[1][0] + 7, 1000), (n - 5000, 5000)]:
        k = max(i for i, (s, _, _) in enumerate(offs) if s <= a)
        e = max(i for i, (s, _, _) in enumerate(offs) if s <= a + m - 1)
        seg = data[offs[k][1]: offs[e][2]]
        lengths.add(len(seg) % 4)
        want, sh = flac_host(seg, si, a, m)
        assert sh.samples == m and sh.reason == 0
        for name, ws_fill, behind in trailing_variants(seg, header):
            got, sd = flac_device(Guarded(), seg, behind, si, a, m, ws_fill, expect_all=True)
            assert flac_fields(sd) == flac_fields(sh), (a, m, name, flac_fields(sd), flac_fields(sh))
            assert got.tobytes() == want.tobytes(), (a, m, name)
    assert len(lengths) > 1                                  # ranges that do and do not end on a multiple of 4


def test_flac_crc_stop_stays_inside_its_buffers():
    """tests/test_flac_gpu.py's test_corrupted_crc16_stops_the_decode_there between guards: only the guards and the delivered
    prefix are held (what lies behind the prefix in `out` is nobody's)."""
    n = 4096 * 8
    pcm = FG.test_signal(n, 2, 16, seed=6)
    data, offs = FG.encode(pcm, 48000, 16, blocksize=4096, mode="mid_side", return_offsets=True)
    body = bytearray(data[offs[0][1]:])
    body[offs[5][2] - offs[0][1] - 1] ^= 0x5A               # the last CRC byte of frame 5
    body = bytes(body)
    si = _lib.bd_flac_streaminfo(4096, 4096, 48000, 2, 16, 0, n)
    want, sh = flac_host(body, si, 100, n - 100)
    assert sh.reason == 1 and sh.samples == 4096 * 5 - 100
    for name, ws_fill, behind in trailing_variants(body, body[:16]):
        got, sd = flac_device(Guarded(), body, behind, si, 100, n - 100, ws_fill, expect_all=False)
        assert sd.samples == sh.samples, name
        assert got[: sd.samples].tobytes() == want[: sh.samples].tobytes(), name


def pcm_device(guards, seg, behind, fmt, first, n, ws_fill, expect_all):
    import torch
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    comp = staged(guards, seg, behind)
    ws = guards.empty((_lib.check(lib.bd_pcm_workspace_bytes(C.byref(fmt), len(seg), n)),), torch.uint8, fill=ws_fill,
                      back=BACK_WORKSPACE, name="pcm workspace")
    out = guards.empty((n, fmt.channels), torch.int16 if pcmio.out_is_s16(fmt) else torch.float32, name="frames",
                       written=expect_all)
    # (bd_pcm_status ends in a reserved word: its fields are held against the host's, not its bytes against the sentinel)
    status = guards.empty((C.sizeof(_lib.bd_pcm_status),), torch.uint8, name="status", written=False)
    stream = torch.cuda.current_stream(dev)
    _lib.check(lib.bd_pcm_decode(comp.data_ptr(), len(seg), C.byref(fmt), first, n, out.data_ptr(),
                                 ws.data_ptr() if ws.numel() else None, ws.numel(), status.data_ptr(), stream.cuda_stream))
    stream.synchronize()
    st = _lib.bd_pcm_status.from_buffer_copy(status.cpu().numpy().tobytes())
    got = out.cpu().numpy()
    guards.check()
    return got, st


def pcm_host(seg, fmt, first, n):
    buf = np.frombuffer(seg, np.uint8)
    out = np.zeros((n, fmt.channels), np.int16 if pcmio.out_is_s16(fmt) else np.float32)
    st = _lib.bd_pcm_status()
    _lib.check(_lib.load().bd_pcm_decode_host(buf.ctypes.data, buf.size, C.byref(fmt), first, n, out.ctypes.data, C.byref(st)))
    return out, st


def pcm_fields(st):
    return (st.samples, st.end_sample, st.bad_block, st.reason)


def pcm_stream(kind, n):
    """(format, bytes) of n frames, from the generators tests/test_pcm_gpu.py uses."""
    ch = 2 if kind == "ms" else 1
    pcm = PG.test_signal(n, ch, 16, seed=7)
    if kind == "ima":
        data, spb = PG.ima_encode(pcm, 256)
        return pcmio.make_format(_lib.PCM_IMA_ADPCM, 1, block_align=256, samples_per_block=spb), data
    if kind == "ms":
        data, spb = PG.ms_encode(pcm, 356)
        return pcmio.make_format(_lib.PCM_MS_ADPCM, 2, block_align=356, samples_per_block=spb, coefs=PG.MS_COEFS), data
    if kind == "ulaw":
        return pcmio.make_format(_lib.PCM_ULAW, 1, 1), PG.g711(pcm, "ulaw")
    if kind == "f64be":
        return pcmio.make_format(_lib.PCM_FLOAT, 1, 8, big_endian=True), PG.floats(pcm / 32768.0, 8, True)
    assert kind == "be24"
    return pcmio.make_format(_lib.PCM_LINEAR, 1, 3, big_endian=True, signed=True), PG.linear(pcm << 8, 3, True, True)


@pytest.mark.parametrize("kind", ["be24", "f64be", "ulaw", "ima", "ms"])
def test_pcm_decode_does_not_read_behind_its_range(kind):
    """Per codec a range of whole blocks (every frame delivered and written) and one that ends inside a block (a prefix
    delivered, reason `truncated`)."""
    fmt, data = pcm_stream(kind, 12_000)
    spb, ba = fmt.samples_per_block, fmt.block_align
    blocks = 9 if spb > 1 else 3001                          # (odd: 24-bit and mu-law ranges that end off a multiple of 4)
    whole = data[ba: (1 + blocks) * ba]
    cut = data[ba: (1 + blocks) * ba + ba // 2 + 1]
    skip = 1 if spb > 1 else 0                               # the range starts one frame into its first block
    for seg, first, m, complete in ((whole, spb + skip, blocks * spb - skip, True), (cut, spb + skip, (blocks + 2) * spb - skip, False)):
        want, sh = pcm_host(seg, fmt, first, m)
        assert (sh.samples == m and sh.reason == 0) if complete else (sh.reason == 2 and 0 < sh.samples < m)
        for name, ws_fill, behind in trailing_variants(seg, seg[:16]):
            got, sd = pcm_device(Guarded(), seg, behind, fmt, first, m, ws_fill, expect_all=complete)
            assert pcm_fields(sd) == pcm_fields(sh), (kind, complete, name, pcm_fields(sd), pcm_fields(sh))
            assert got[: sd.samples].tobytes() == want[: sh.samples].tobytes(), (kind, complete, name)
