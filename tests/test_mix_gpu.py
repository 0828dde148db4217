"""bd_mix on the GPU (csrc/mixaug.hip) against bd_mix_host, its restatement in the same order of operations: every bit of the
mixtures, of (Pe, Pn) and of the flag words; nothing written outside the clips' output ranges; bad descriptors refused on the
host; two identical calls give identical bits."""
import numpy as np
import pytest

from buzzdetect_amd import _lib, dataset as D

pytestmark = pytest.mark.gpu

S = _lib.MIX_SLICE
LENGTHS = (1, 255, 256, 257, S - 1, S, S + 1, 3 * S + 5, 15360, 15600)
SENTINEL = 0x7FC12345            # a NaN with a payload no kernel produces


@pytest.fixture(scope="module")
def sources():
    import torch
    rng = np.random.default_rng(77)
    n = 6 * S + 40000
    t = np.arange(n) / 16000.0
    ev = (0.3 * np.sin(2 * np.pi * 220.0 * t) + 0.02 * rng.normal(size=n)).astype(np.float32)
    nz = (0.1 * rng.normal(size=n + 123)).astype(np.float32)
    nz[5000:9000] = 0.0                                  # a silent stretch
    ev[20000:21000] = 0.0                                # a silent event
    return ev, nz, torch.from_numpy(ev).cuda(), torch.from_numpy(nz).cuda()


def sentinel(n, dtype):
    import torch
    return torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda").view(dtype)


def run_both(sources, clips, tail=1000):
    """(device out with sentinel background, host out over a sentinel copy, ...): the whole buffers, to compare every element."""
    import torch
    ev, nz, ev_d, nz_d = sources
    size = int((clips["out_off"] + clips["n"]).max()) + tail
    out_d = sentinel(size, torch.float32)
    need = _lib.check(_lib.load().bd_mix_workspace_bytes(D._clip_pointer(clips), clips.size))
    ws = sentinel((need + 4096) // 4, torch.float32).view(torch.uint8)
    _, power_d, flags_d = D.mix_device(ev_d, nz_d, clips, out=out_d, workspace=ws)
    torch.cuda.synchronize()
    out_h = np.full(size, SENTINEL, np.int32).view(np.float32)
    _, power_h, flags_h = D.mix_host(ev, nz, clips, out=out_h)
    ws_tail = ws[need:].cpu().numpy().view(np.int32)
    assert (ws_tail == SENTINEL).all(), "bd_mix wrote behind the workspace it asked for"
    return out_d.cpu().numpy(), power_d.cpu().numpy(), flags_d.cpu().numpy().view(np.uint32), out_h, power_h, flags_h


def check_equal(got, clips):
    out_d, power_d, flags_d, out_h, power_h, flags_h = got
    owned = np.zeros(out_d.size, bool)
    for c in clips:
        owned[int(c["out_off"]): int(c["out_off"]) + int(c["n"])] = True
    assert (out_d.view(np.int32)[~owned] == SENTINEL).all(), "an element outside every clip's output range changed"
    assert (out_h.view(np.int32)[~owned] == SENTINEL).all()
    assert np.isfinite(out_d[owned]).all()
    for j, c in enumerate(clips):
        a, n = int(c["out_off"]), int(c["n"])
        assert out_d[a:a + n].tobytes() == out_h[a:a + n].tobytes(), f"clip {j} (n = {n}) differs from bd_mix_host"
    assert power_d.tobytes() == power_h.tobytes() and flags_d.tobytes() == flags_h.tobytes()


def test_every_path_length_in_one_call_packed_back_to_back(sources):
    n = np.array(LENGTHS)
    ev_off = 1 + 2 * np.arange(n.size) * 101                     # odd: never a multiple of 4, nor of the vector width
    nz_off = 9001 + 2 * np.arange(n.size) * 57                   # (behind the silent stretch)
    clips = D.mix_descriptors(ev_off, nz_off, n, [0, 5, 10, 20, -10, 0, 5, 10, 20, np.inf], [0, -6, 0, 3, 0, -6, 0, 0, -6, 0])
    assert clips["out_off"].tolist() == (np.cumsum(n) - n).tolist() and (clips["ev_off"] % 2 == 1).all()
    got = run_both(sources, clips)
    check_equal(got, clips)
    assert not got[2].any() and (got[1] > 0).all()
    # the last clip is the event alone
    ev = sources[0]
    a = int(clips["out_off"][-1])
    assert got[0][a:a + 15600].tobytes() == ev[int(ev_off[-1]): int(ev_off[-1]) + 15600].tobytes()


def test_sixty_four_clips_with_gaps_silence_and_stray_write_check(sources):
    rng = np.random.default_rng(5)
    n = rng.integers(1, 3 * S, 64)
    n[:4] = (1, 3 * S + 5, 15360, 257)
    ev_off = 2 * rng.integers(0, 10000, 64) + 1
    nz_off = 2 * rng.integers(4600, 14000, 64) + 1
    ev_off[7], n[7] = 20001, 900                                 # inside the silent event
    nz_off[9], n[9] = 5003, 3000                                 # inside the silent background
    clips = D.mix_descriptors(ev_off, nz_off, n, rng.choice([-10.0, 0.0, 5.0, 20.0], 64), rng.choice([0.0, -6.0], 64))
    clips["out_off"] += 3 * np.arange(64) + 5                    # gaps of three elements, five in front
    got = run_both(sources, clips)
    check_equal(got, clips)
    flags, power = got[2], got[1]
    assert flags[9] == _lib.MIX_FLAG_SILENT_BACKGROUND and power[9, 1] == 0.0 and power[7, 0] == 0.0 and flags[7] == 0
    assert flags.sum() == 1
    ev = sources[0]
    assert got[0][int(clips["out_off"][7]):][:900].tobytes() == np.zeros(900, np.float32).tobytes()
    a = int(clips["out_off"][9])
    assert got[0][a:a + 3000].tobytes() == (clips["ev_gain"][9] * ev[int(ev_off[9]): int(ev_off[9]) + 3000]).astype(np.float32).tobytes()


def test_one_clip_and_no_clip(sources):
    import torch
    clips = D.mix_descriptors([3], [9003], [2 * S + 1], [5.0], [0.0])
    check_equal(run_both(sources, clips), clips)
    out = sentinel(100, torch.float32)
    D.mix_device(sources[2], sources[3], np.zeros(0, D.MIX_CLIP), out=out)
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.int32) == SENTINEL).all()


def test_a_descriptor_past_the_end_is_refused_on_the_host(sources):
    """Not a fault test: the call must return BD_EINVAL before anything is launched."""
    import torch
    ev, nz, ev_d, nz_d = sources
    for field, value in (("ev_off", ev.size - 99), ("nz_off", nz.size - 99), ("out_off", 1000 - 99)):
        clips = D.mix_descriptors([1, 3], [9001, 9003], [100, 100], [0.0, 0.0], [0.0, 0.0])
        clips[field][1] = value
        out = sentinel(1000, torch.float32)
        with pytest.raises(_lib.BuzzdetectHipError, match="clip 1") as err:
            D.mix_device(ev_d, nz_d, clips, out=out)
        assert err.value.code == -1
        torch.cuda.synchronize()
        assert (out.cpu().numpy().view(np.int32) == SENTINEL).all()


def test_two_identical_calls_give_identical_bits(sources):
    import torch
    rng = np.random.default_rng(8)
    n = rng.integers(1, 4 * S, 32)
    clips = D.mix_descriptors(2 * rng.integers(0, 9000, 32) + 1, 2 * rng.integers(4600, 12000, 32) + 1, n,
                              rng.choice([0.0, 10.0], 32), np.zeros(32))
    runs = []
    for _ in range(2):
        out, power, flags = D.mix_device(sources[2], sources[3], clips)
        torch.cuda.synchronize()
        runs.append((out.cpu().numpy().tobytes(), power.cpu().numpy().tobytes(), flags.cpu().numpy().tobytes()))
    assert runs[0] == runs[1]
