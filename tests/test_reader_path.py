"""The reader's one chunk-read path (Pipeline._read_unit) holds its slot rules for every kind of track: a fill that raises
gives its slot back and the exception travels on; a unit wholly behind the end of a file cut short takes no slot, gives
none back and is dropped once.  Host-only stage: no device needed."""
import numpy as np
import pytest

from tools import flacgen as F
from tools import pcmgen as G

RATE, CHUNK = 16000, 2.0
KINDS = ["wav16", "wav24", "flac", "ima"]


def _file(kind: str, seconds: float) -> bytes:
    """`seconds` of 16 kHz mono as a 16-bit WAV, a 24-bit WAV, a 16-bit FLAC or an IMA-ADPCM WAV."""
    n = int(RATE * seconds)
    if kind == "wav24":
        return F.wav_bytes(F.test_signal(n, 1, 24, seed=21), RATE, 24)
    pcm = F.test_signal(n, 1, 16, seed=20)
    if kind == "wav16":
        return F.wav_bytes(pcm, RATE, 16)
    if kind == "flac":
        return F.encode(pcm, RATE, 16, blocksize=4096)
    data, spb = G.ima_encode(pcm, 1024)
    return G.wave(G.fmt_ima(1, RATE, 1024, spb), data, fact=n)


def _planned(tmp_path, kind: str, data: bytes):
    """The file through the planner of a host-only reader stage: (pipeline, job, its read units)."""
    from buzzdetect_amd import pipeline as P, results as R
    name = "a.flac" if kind == "flac" else "a.wav"
    (tmp_path / name).write_bytes(data)
    pipe = P.Pipeline(make_engine=None, classes=["a"], framehop_s=0.96, hop=15360, step=96, chunklength=CHUNK, framelength_s=0.96,
                      digits_time=2, digits_results=2, classes_out="all", threshold=None, readers=1, analyzers=1,
                      pin_memory=False, stream_buffer_depth=64)
    job = P.FileJob(str(tmp_path / name), "a", name, R.ResultFile(str(tmp_path / "out" / "a")))
    pipe._plan_file(job)
    units = []
    while not pipe.q_units.empty():
        units.append(pipe.q_units.get())
    return pipe, job, units


@pytest.mark.parametrize("kind", KINDS)
def test_a_fill_that_raises_gives_its_slot_back(tmp_path, monkeypatch, kind):
    pipe, job, units = _planned(tmp_path, kind, _file(kind, CHUNK))
    assert [u.chunk for u in units] == [(0.0, CHUNK)]
    free = pipe.pool._free.qsize()
    pipe._read_unit(units[0])                           # (the unit reads: what fails below is the patched call alone)
    task = pipe.q_analyze.get_nowait()
    assert task.frames == int(RATE * CHUNK) and pipe.pool._free.qsize() == free - 1
    pipe.pool.release(task.slot)

    def broken(*args, **kwargs):
        raise OSError("the disk went away")
    monkeypatch.setattr(job.track, "read_raw_into" if kind.startswith("wav") else "decode_host_into", broken)
    with pytest.raises(OSError, match="the disk went away"):
        pipe._read_unit(units[0])
    assert pipe.pool._free.qsize() == free and pipe.q_analyze.empty() and pipe.q_write.empty()
    assert job.outstanding == 1 and pipe.report.chunks == 1


@pytest.mark.parametrize("kind", KINDS)
def test_a_unit_behind_the_end_of_a_file_cut_short_takes_no_slot_and_is_dropped_once(tmp_path, monkeypatch, kind):
    data = _file(kind, 2 * CHUNK)
    pipe, job, units = _planned(tmp_path, kind, data[: int(len(data) * 0.3)])       # its header still declares 4 s
    assert [u.chunk for u in units] == [(0.0, CHUNK), (CHUNK, 2 * CHUNK)]
    assert 0 < job.track.frames < RATE * CHUNK and job.track.frames_declared == 2 * RATE * CHUNK
    calls = {"acquire": 0, "release": 0, "drop": 0}
    for owner, name in ((pipe.pool, "acquire"), (pipe.pool, "release"), (pipe, "_drop")):
        def counted(*args, _f=getattr(owner, name), _k=name.lstrip("_"), **kwargs):
            calls[_k] += 1
            return _f(*args, **kwargs)
        monkeypatch.setattr(owner, name, counted)
    free = pipe.pool._free.qsize()
    pipe._read_unit(units[1])
    assert calls == {"acquire": 0, "release": 0, "drop": 1}
    assert pipe.pool._free.qsize() == free and pipe.q_analyze.empty() and pipe.q_write.empty()
    assert job.outstanding == 1 and job.bad_read and pipe.report.chunks == 0
