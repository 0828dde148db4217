"""The embedding store on the host (include/buzzdetect_rows.h, buzzdetect_amd/store.py): bd_rows_encode_host / _decode_host against
an independent NumPy restatement in every byte and checksum word, the error bounds the header derives, the logit bound of the
packaged head under codec h in float64, and the file format - round trip, cut files, a flipped byte, stale .part files, the
refusals of other parameters.  No device is needed."""
import json
import os

import numpy as np
import pytest

from buzzdetect_amd import _lib, dataset, store

CODECS = ("f32", "h", "b")
FLT_MAX = np.float32(3.4028235e38)
QNAN = 0x7FC00000


# ---------------------------------------------------------------------------------------------------- the NumPy restatement
def np_encode(rows, codec):
    """Records, sums and the flags count by NumPy alone: np.frexp, np.ldexp, astype(np.float16), np.rint."""
    w = rows.shape[0]
    rb = {"f32": 4096, "h": 16 + 2048, "b": 16 + 1024}[codec]
    rec = np.zeros((w, rb), np.uint8)
    flags = 0
    for r in range(w):
        x = rows[r]
        bad = (not np.isfinite(x).all()) or (codec == "b" and bool((x < 0).any()))
        flags += int(bad)
        if codec == "f32":
            rec[r] = x.view(np.uint8)
            continue
        if bad:
            rec[r, :4] = np.array([-2 ** 31], "<i4").view(np.uint8)
            continue
        m = np.abs(x).max()
        _, p = np.frexp(m)
        e = 0 if m == 0 else int(p) - (15 if codec == "h" else 8)
        rec[r, :4] = np.array([e], "<i4").view(np.uint8)
        s = np.ldexp(x, np.int32(-e))
        assert s.dtype == np.float32
        if codec == "h":
            rec[r, 16:] = np.clip(s, np.float32(-32752), np.float32(32752)).astype(np.float16).view(np.uint8)
        else:
            rec[r, 16:] = np.minimum(np.float32(255), np.rint(s)).astype(np.uint8)
    return rec, np_sums(rec), flags


def np_sums(rec):
    w, rb = rec.shape
    out = np.zeros(((w + 255) // 256, 2), np.uint64)
    for s in range(out.shape[0]):
        words = np.ascontiguousarray(rec[256 * s:256 * (s + 1)]).reshape(-1).view("<u4").astype(np.uint64)
        with np.errstate(over="ignore"):
            out[s, 0] = words.sum(dtype=np.uint64)
            out[s, 1] = (words * np.arange(1, words.size + 1, dtype=np.uint64)).sum(dtype=np.uint64)
    return out


def np_decode(rec, codec):
    w = rec.shape[0]
    if codec == "f32":
        return np.ascontiguousarray(rec).view(np.float32).reshape(w, 1024).copy()
    out = np.zeros((w, 1024), np.float32)
    for r in range(w):
        e = int(np.ascontiguousarray(rec[r, :4]).view("<i4")[0])
        if e == -2 ** 31:
            out[r] = np.array([QNAN], np.uint32).view(np.float32)[0]
        elif codec == "h":
            out[r] = np.ldexp(np.ascontiguousarray(rec[r, 16:]).view(np.float16).astype(np.float32), np.int32(e))
        else:
            out[r] = np.ldexp(rec[r, 16:].astype(np.float32), np.int32(e))
    return out


# ---------------------------------------------------------------------------------------------------- rows
def edge_rows():
    """(rows, names): the cases the header decides, each a row."""
    rng = np.random.default_rng(77)
    base = (rng.random((12, 1024)) * 6).astype(np.float32)
    rows, names = [], []

    def add(name, x):
        rows.append(np.asarray(x, np.float32))
        names.append(name)
    add("zero", np.zeros(1024))
    x = base[0].copy(); x[0] = 7.25
    add("max first", x)
    x = base[1].copy(); x[1023] = 7.25
    add("max last", x)
    x = np.full(1024, 5.0, np.float32); x[::3] = np.ldexp(np.float32(5.0), -30); x[1::7] = np.ldexp(np.float32(5.0), -25)
    add("2^-30 below", x)
    x = (base[2] * np.float32(1e37)).astype(np.float32); x[400] = FLT_MAX
    add("FLT_MAX", x)
    x = base[3] / np.float32(8); x[5] = np.float32(0.99999); x[6] = np.float32(32761 / 32768); x[7] = np.float32(32759 / 32768)
    add("rounds to 2^15", x)                                # scaled 32767.67 and 32761 are clamped to 32752; 32759 rounds to it
    x = base[4].copy(); x[9] = np.float32(255.7 / 256 * 8)  # under b: scaled 255.7 -> rint 256 -> clamped to 255
    add("b clamp", x)
    add("small", base[5] * np.float32(2.0 ** -90))
    add("denormal", base[6] * np.float32(2.0 ** -140))
    x = base[7].copy(); x[77] = np.nan
    add("nan", x)
    x = base[8].copy(); x[1000] = np.inf
    add("inf", x)
    x = base[9].copy(); x[3::5] *= -1
    add("negative", x)
    x = base[10].copy(); x[0] = -0.0
    add("minus zero", x)
    return np.stack(rows), names


def all_rows(w):
    e, _ = edge_rows()
    rng = np.random.default_rng(5)
    fill = (rng.random((513, 1024)) ** 3 * 6).astype(np.float32)
    fill[:e.shape[0]] = e
    fill[255:258] = e[[1, 4, 9]]                             # cases either side of a slice boundary
    return fill[:w]


@pytest.mark.parametrize("w", (0, 1, 255, 256, 257, 513))
@pytest.mark.parametrize("codec", CODECS)
def test_host_codec_is_the_numpy_restatement_in_every_byte(codec, w):
    rows = all_rows(w)
    rec, sums, flags = store.encode_host(rows, codec)
    want_rec, want_sums, want_flags = np_encode(rows, codec)
    assert rec.shape == want_rec.shape and rec.tobytes() == want_rec.tobytes()
    assert sums.tobytes() == want_sums.tobytes() and flags == want_flags
    back, read = store.decode_host(rec, codec)
    assert back.tobytes() == np_decode(want_rec, codec).tobytes()
    assert read.tobytes() == want_sums.tobytes()
    if codec == "f32":
        assert back.tobytes() == rows.tobytes()


@pytest.mark.parametrize("codec", CODECS)
def test_rows_that_are_not_representable(codec):
    rows, names = edge_rows()
    rec, _, flags = store.encode_host(rows, codec)
    bad = {"nan", "inf"} | ({"negative"} if codec == "b" else set())
    assert flags == len(bad)
    back, _ = store.decode_host(rec, codec)
    for r, name in enumerate(names):
        if codec == "f32":
            assert back[r].tobytes() == rows[r].tobytes()
        elif name in bad:
            assert int(rec[r, :4].view("<i4")[0]) == _lib.ROWS_BAD_EXPONENT and not rec[r, 4:].any()
            assert (back[r].view(np.uint32) == QNAN).all()
        else:
            assert int(rec[r, :4].view("<i4")[0]) != _lib.ROWS_BAD_EXPONENT and np.isfinite(back[r]).all(), name
    if codec == "b":
        assert back[names.index("minus zero"), 0] == 0.0


def test_decided_edges():
    """The header's decisions: no code reaches 2^15 and FLT_MAX decodes to a finite float; b clamps to 255."""
    rows, names = edge_rows()
    rec, _, _ = store.encode_host(rows, "h")
    codes = np.ascontiguousarray(rec[:, 16:]).view(np.float16).astype(np.float32)
    good = [r for r, n in enumerate(names) if n not in ("nan", "inf")]
    assert np.abs(codes[good]).max() == 32752.0
    r = names.index("rounds to 2^15")
    assert codes[r, 5] == 32752.0 and codes[r, 6] == 32752.0 and codes[r, 7] == 32752.0
    r = names.index("FLT_MAX")
    assert int(rec[r, :4].view("<i4")[0]) == 113 and codes[r, 400] == 32752.0
    back, _ = store.decode_host(rec, "h")
    assert np.isfinite(back[r]).all() and back[r, 400] == np.ldexp(np.float32(32752), 113)
    for n in ("max first", "max last", "FLT_MAX", "small"):
        assert 2.0 ** 14 <= np.abs(codes[names.index(n)]).max() < 2.0 ** 15
    rec, _, _ = store.encode_host(rows, "b")
    r = names.index("b clamp")
    assert rec[r, 16 + 9] == 255 and 128 <= rec[r, 16:].max() <= 255
    r = names.index("FLT_MAX")
    assert int(rec[r, :4].view("<i4")[0]) == 120 and np.isfinite(store.decode_host(rec, "b")[0][r]).all()


def bound_rows():
    rows, names = edge_rows()
    keep = [r for r, n in enumerate(names) if n not in ("nan", "inf", "negative", "denormal", "minus zero")]
    rng = np.random.default_rng(64)
    seeded = (rng.random((64, 1024)) ** rng.integers(1, 6, size=(64, 1)) * rng.choice([1e-3, 1.0, 6.0, 4e4], size=(64, 1))).astype(np.float32)
    return np.concatenate([rows[keep], seeded])


def test_error_bounds_of_the_header_hold():
    rows = bound_rows()
    x = rows.astype(np.float64)
    m = np.abs(x).max(axis=1, keepdims=True)
    rec, _, flags = store.encode_host(rows, "h")
    assert flags == 0
    xh = store.decode_host(rec, "h")[0].astype(np.float64)
    assert (np.abs(xh - x) <= np.maximum(2.0 ** -11 * np.abs(x), 2.0 ** -39 * m)).all()
    rec, _, flags = store.encode_host(rows, "b")
    assert flags == 0
    xb = store.decode_host(rec, "b")[0].astype(np.float64)
    step = np.ldexp(1.0, np.ascontiguousarray(rec[:, :4]).view("<i4").astype(np.int64))          # 2^e per row
    err = np.abs(xb - x)
    nonzero = m[:, 0] > 0
    assert (err <= step).all() and (step[nonzero] <= m[nonzero] / 128).all()
    unclamped = x / step < 255.5
    assert (err[unclamped] <= (step / 2 * np.ones_like(x))[unclamped]).all()
    assert (~unclamped).any()                                # the clamp is among the cases


def test_logit_bound_of_the_packaged_head_under_h():
    """In float64 a logit moves by at most 2^-11 sum |w| |x| + 2^-39 m sum |w| (plus the float64 sums' own rounding, 2^-40 of the
    first term at most)."""
    from buzzdetect_amd import weights
    head = weights.load_head("model_general_v3")
    k = np.asarray(head.kernel, np.float64)
    if k.shape[0] != 1024:
        k = k.T
    rows = bound_rows()
    x = rows.astype(np.float64)
    m = np.abs(x).max(axis=1, keepdims=True)
    rec, _, _ = store.encode_host(rows, "h")
    xh = store.decode_host(rec, "h")[0].astype(np.float64)
    moved = np.abs(xh @ k - x @ k)
    bound = (2.0 ** -11 + 2.0 ** -40) * (np.abs(x) @ np.abs(k)) + 2.0 ** -39 * m * np.abs(k).sum(axis=0, keepdims=True)
    assert moved.shape == bound.shape and (moved <= bound).all()
    assert moved.max() > 0


# ---------------------------------------------------------------------------------------------------- the file
PARAMS = dict(embeddername="yamnet_k2", weights_sha256="ab" * 32, mode="f16x3", resample_quality=1, framehop_prop=1.0, chunklength=4.8)


def header_for(ident, counts, codec, **over):
    starts = np.cumsum([0] + list(counts[:-1])) * 0.96
    source = {"path": ident + ".wav", "size": 1234, "mtime_ns": 99, "rate": 16000, "channels": 1, "duration": float(sum(counts)) * 0.96}
    fields = dict(PARAMS, codec=codec)
    fields.update(over)
    return store.make_header(ident=ident, source=source, chunks=list(zip(starts, counts)), messages=["a note"], **fields)


def make_store(root, codec="h", w=600):
    rows = np.abs(all_rows(513))
    rows = rows[np.isfinite(rows).all(axis=1)]
    rows = np.concatenate([rows, rows])[:w]
    store.write_manifest(str(root))
    store.write_rows_host(os.path.join(root, "site", "b" + store.SUFFIX), rows, header_for("site/b", [300, 300 - (600 - w)], codec))
    store.write_rows_host(os.path.join(root, "a" + store.SUFFIX), rows[:7], header_for("a", [5, 2], codec))
    return rows


@pytest.mark.parametrize("codec", CODECS)
def test_round_trip(tmp_path, codec):
    rows = make_store(tmp_path, codec)
    st = store.Store(str(tmp_path))
    assert st.idents == ["a", "site/b"] and st.windows == 607 and len(st) == 2
    assert st.parameters == dict(PARAMS, codec=codec)
    assert st.verify() == 607
    b = st.recordings[1]
    assert b.header["chunks"] == [[0.0, 300], [300 * 0.96, 300]] and b.header["messages"] == ["a note"]
    assert b.layout.records % 4096 == 0 and b.layout.record_bytes == store.record_bytes(codec)
    assert b.rows_host().tobytes() == store.decode_host(store.encode_host(rows, codec)[0], codec)[0].tobytes()
    if codec == "f32":
        assert st.recordings[0].rows_host().tobytes() == rows[:7].tobytes()
    assert store.as_store(str(tmp_path)).idents == st.idents and store.as_store(st) is st
    assert store.as_store(str(tmp_path / "site")) is None    # a folder without store.json is audio


def test_a_cut_file_is_refused(tmp_path):
    make_store(tmp_path)
    path = os.path.join(tmp_path, "site", "b" + store.SUFFIX)
    whole = open(path, "rb").read()
    lay = store.RecordingFile(path).layout
    for cut in (10, 100, lay.records + 5 * lay.record_bytes + 17, lay.table + 8, len(whole) - 1):
        with open(path, "wb") as f:
            f.write(whole[:cut])
        with pytest.raises(store.StoreError, match="b.bdemb"):
            store.RecordingFile(path)
        with pytest.raises(store.StoreError, match="truncated|trailer"):
            store.Store(str(tmp_path))
    with open(path, "wb") as f:                              # cut in the records, then grown back to its length with zeros
        f.write(whole[:lay.records + 100] + bytes(len(whole) - lay.records - 100))
    with pytest.raises(store.StoreError, match="trailer"):
        store.RecordingFile(path)
    with open(path, "wb") as f:
        f.write(whole)
    assert store.Store(str(tmp_path)).verify() == 607


def test_a_flipped_byte_is_found_and_its_slice_named(tmp_path):
    make_store(tmp_path)
    path = os.path.join(tmp_path, "site", "b" + store.SUFFIX)
    lay = store.RecordingFile(path).layout
    with open(path, "r+b") as f:
        f.seek(lay.records + 300 * lay.record_bytes + 1000)
        byte = f.read(1)
        f.seek(-1, 1)
        f.write(bytes([byte[0] ^ 0x10]))
    st = store.Store(str(tmp_path))                          # the headers are whole: it opens
    with pytest.raises(store.StoreError, match=r"b\.bdemb: slice 1 "):
        st.verify()
    with pytest.raises(store.StoreError, match="slice 1 "):
        st.recordings[1].rows_host()
    assert st.recordings[0].verify() == 7


def test_a_part_file_is_ignored_and_rewritten(tmp_path):
    rows = make_store(tmp_path, "b")
    stale = os.path.join(tmp_path, "c" + store.SUFFIX + ".part")
    with open(stale, "wb") as f:
        f.write(b"half a file")
    st = store.Store(str(tmp_path))
    assert st.idents == ["a", "site/b"] and st.verify() == 607
    store.write_rows_host(os.path.join(tmp_path, "c" + store.SUFFIX), rows[:3], header_for("c", [3], "b"))
    assert not os.path.exists(stale)
    assert store.Store(str(tmp_path)).idents == ["a", "c", "site/b"]
    with pytest.raises(store.StoreError, match="not representable"):       # nothing is left behind by a refused recording
        store.write_rows_host(os.path.join(tmp_path, "d" + store.SUFFIX), -rows[:3] - 1, header_for("d", [3], "b"))
    assert not os.path.exists(os.path.join(tmp_path, "d" + store.SUFFIX)) and not os.path.exists(os.path.join(tmp_path, "d" + store.SUFFIX + ".part"))


def test_other_parameters_are_refused(tmp_path):
    rows = make_store(tmp_path)
    st = store.Store(str(tmp_path))
    st.check(None, 1.0, 4.8)
    st.check(None, 1.0, 4.81)                                # rounds to the same whole number of frames
    with pytest.raises(ValueError, match=r"framehop_prop=1\.0, chunklength=4\.8; asked for framehop_prop=0\.5, chunklength=4\.8"):
        st.check(None, 0.5, 4.8)
    with pytest.raises(ValueError, match=r"framehop_prop=1\.0, chunklength=4\.8; asked for framehop_prop=1\.0, chunklength=199\.68"):
        st.check(None, 1.0, 200)
    store.check_weights("here", st.parameters, "yamnet_k2", "ab" * 32)
    with pytest.raises(ValueError, match="other embedder weights"):
        store.check_weights("here", st.parameters, "yamnet_k2", "cd" * 32)
    with pytest.raises(ValueError, match="yamnet_k9"):
        store.check_weights("here", st.parameters, "yamnet_k9", "ab" * 32)
    with pytest.raises(ValueError, match="embedding store"):   # the mixer needs audio; refused before an engine is built
        dataset.augment(str(tmp_path), {}, ["ambient", "buzz"], background="ambient")
    store.write_rows_host(os.path.join(tmp_path, "z" + store.SUFFIX), rows[:3], header_for("z", [3], "h", framehop_prop=0.5))
    with pytest.raises(store.StoreError, match="framehop_prop"):
        store.Store(str(tmp_path))
    with pytest.raises(ValueError, match="codec"):
        store.encode_host(rows[:1], "q")
    with pytest.raises(ValueError):
        header_for("y", [3], "q")


def test_the_walk_hands_out_the_chunk_table_and_the_messages(tmp_path):
    make_store(tmp_path)
    store.write_manifest(str(tmp_path), ["conflicting names, skipped: x"], [("b.wav", "b", ["unreadable, skipped: b (why)"])], ["a", "b", "site/b", "x"])
    assert json.load(open(os.path.join(tmp_path, store.MANIFEST)))["format"] == store.FORMAT_VERSION
    st = store.Store(str(tmp_path))
    messages = []
    walk = st.walk(None, 1.0, 4.8, {"gone": [], "site/b": []}, False, messages)
    ident, chunks = next(walk)
    assert ident == "a" and [(c.group, c.start_s, c.pcm.first, c.pcm.windows) for c in chunks] == [(0, 0.0, 0, 5), (0, 5 * 0.96, 5, 2)]
    assert dataset._stored([c.pcm for c in chunks]) and dataset._part_windows(None, chunks[1].pcm, 0, 0) == 2
    ident, chunks = next(walk)
    assert ident == "site/b" and [c.group for c in chunks] == [1, 1] and chunks[1].pcm.first == 300
    assert list(walk) == []
    assert messages == ["conflicting names, skipped: x", "annotated, but no such recording: gone", "a note",
                        "unreadable, skipped: b (why)", "a note"]
    messages = []
    assert [i for i, _ in st.walk(None, 1.0, 4.8, {"site/b": []}, True, messages)] == ["site/b"]
    assert messages == ["conflicting names, skipped: x", "a note"]
