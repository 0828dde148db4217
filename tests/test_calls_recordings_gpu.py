"""calls.call_recordings end to end on the GPU: a folder with a 16 kHz WAV of three chunks, a 44.1 kHz stereo FLAC and a file below
the minimum size, called at framehop_prop 1.0 and 0.5, against calls.events_host / calls.bins_host over engine.predict of every
chunk as analyze cuts it, with ticks from framing.window_starts.  The synthetic weights give arbitrary logits, so the thresholds are
quantiles of the logits themselves: high the 70th, low the 40th percentile of a column, so that events exist."""
import os
import wave

import numpy as np
import pytest

from buzzdetect_amd import calls, dataset as D, framing

pytestmark = pytest.mark.gpu

W16 = D.WINDOW_SAMPLES
CHUNK = 20                         # rounds to 20.16 s: 21 windows a chunk at hop 0.96, 41 at hop 0.48
BIN_S = 10.0


def write_wav(path, pcm16, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.asarray(pcm16, "<i2").tobytes())


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from oracle import yamnet_oracle as O
    from tools import flacgen as G
    root = tmp_path_factory.mktemp("calls")
    audio = root / "audio"
    (audio / "site").mkdir(parents=True)
    a = (np.clip(O.synthetic_audio(52 * W16 + 3000, seed=21), -1, 1 - 2 ** -15) * 32768.0).round().astype(np.int16)
    b = G.test_signal(int(44100 * 9.7), 2, 16, seed=6)
    write_wav(audio / "a.wav", a, 16000)
    (audio / "site" / "b.flac").write_bytes(G.encode(b, 44100, 16, blocksize=4608, mode="mid_side"))
    write_wav(audio / "tiny.wav", a[:1000], 16000)
    return str(audio), {"a": (a, 16000), "site/b": (b, 44100)}, str(root)


def reference_logits(engine, pcm, framehop_s):
    """Per recording (starts, logits [W, n_classes]): engine.predict of every chunk as analyze cuts it."""
    out = {}
    for ident, (x, rate) in pcm.items():
        starts, rows = [], []
        for edge in framing.gaps_to_chunklist([(0, x.shape[0] / rate)], framing.round_chunklength(CHUNK)):
            lo, hi = framing.chunk_sample_range(edge, rate)
            hi = min(hi, x.shape[0])
            if hi <= lo:
                continue
            part = x[lo:hi]
            if rate != 16000:
                dev = engine.resample(part.astype(np.int16), rate, 16000)
            else:
                dev = engine.to_device(part.astype(np.float32) / 32768.0)
            logits = engine.predict(dev, framehop_s).numpy()
            rows.append(logits)
            starts.append(framing.window_starts(logits.shape[0], float(edge[0]), framehop_s, 2))
        out[ident] = (np.concatenate(starts), np.concatenate(rows).astype(np.float32))
    return out


@pytest.mark.parametrize("framehop_prop", (1.0, 0.5))
def test_call_recordings_is_the_host_calling_over_engine_predict(engine, folder, framehop_prop):
    import pandas as pd
    dir_audio, pcm, root = folder
    names = ["ins_buzz", next(c for c in engine.classes if c != "ins_buzz")]
    cols = [engine.classes.index(n) for n in names]
    framehop_s = 0.96 * framehop_prop
    ref = reference_logits(engine, pcm, framehop_s)
    every = np.concatenate([v[1] for v in ref.values()])
    assert every.shape[0] > 60
    highs = {n: float(np.percentile(every[:, c], 70)) for n, c in zip(names, cols)}
    lows = {n: float(np.percentile(every[:, c], 40)) for n, c in zip(names, cols)}
    got = calls.call_recordings(dir_audio, classes=names, thresholds=highs, low=lows, merge_gap_s=1.0, min_duration_s=1.5,
                                bin_s=BIN_S, engine=engine, framehop_prop=framehop_prop, chunklength=CHUNK)
    assert got.classes == names and sorted(got.bins) == sorted(pcm)
    assert len(got.messages) == 1 and "tiny" in got.messages[0] and "below minimum" in got.messages[0]
    adjacent = calls.adjacent_ticks(framehop_s)
    rules = [calls.Rule(highs[n], lows[n], 1.0, 1.5) for n in names]
    assert rules[0].packed(adjacent)[2:] == (adjacent + 100, 54)
    total = 0
    for ident, (starts, logits) in ref.items():
        x = np.ascontiguousarray(logits[:, cols])
        t = calls.ticks(starts)
        if framehop_prop == 0.5 and ident == "a":
            assert (np.diff(t) == 2 * adjacent).sum() == 2                 # the doubled step at both chunk edges: holes
        marks, events = calls.events_host(x, t, adjacent, rules)
        ids, seg = calls.bin_segments(t, calls.bin_ticks(BIN_S))
        counts, values = calls.bins_host(x, marks, seg)
        bins = got.bins[ident]
        assert np.array_equal(bins.counts, counts) and np.array_equal(bins.values.view(np.uint32), values.view(np.uint32))
        assert np.array_equal(bins.bin_start, ids * BIN_S) and np.array_equal(bins.windows, np.diff(seg))
        assert bins.windows.sum() == t.shape[0]
        known = set(starts.tolist())
        for c, name in enumerate(names):
            want = [(ident, float(starts[f]), round(float(starts[l]) + 0.96, 6), int(l - f + 1), int(n), float(x[p, c]),
                     float(starts[p])) for f, l, n, p, kept in events[c] if kept]
            mine = [e for e in got.events[c] if e[0] == ident]
            assert mine == want
            total += len(want)
            for e in mine:                                                 # values analyze would write
                assert e[1] in known and e[6] in known and round(e[2] - 0.96, 2) in known
    assert total > 0
    # the files read back to the same numbers
    out = os.path.join(root, f"called_{framehop_prop}")
    got.to_csv(out)
    for ident in pcm:
        table = pd.read_csv(os.path.join(out, ident + calls.SUFFIX_EVENTS))
        assert list(table.columns) == list(calls.EVENT_COLUMNS)
        mine = [(name, e) for name, found in zip(names, got.events) for e in found if e[0] == ident]
        assert len(table) == len(mine)
        for row, (name, e) in zip(table.itertuples(index=False), mine):
            assert (row[0], row.start, row.end, row.windows, row.detected, row.peak_start) == (name, e[1], e[2], e[3], e[4], e[6])
            assert row.peak == pytest.approx(float(np.round(np.float32(e[5]), 2)), rel=1e-6, abs=1e-6)
        table = pd.read_csv(os.path.join(out, ident + calls.SUFFIX_BINS))
        bins = got.bins[ident]
        assert np.array_equal(table["bin_start"].to_numpy(), bins.bin_start)
        assert np.array_equal(table["windows"].to_numpy(), bins.windows)
        for c, name in enumerate(names):
            assert np.array_equal(table[f"detected_{name}"].to_numpy(), bins.counts[c, :, 0])
            assert np.array_equal(table[f"events_{name}"].to_numpy(), bins.counts[c, :, 1])
            mean = bins.values[c, :, 0].astype(np.float64) / bins.windows
            assert np.allclose(table[f"mean_{name}"].to_numpy(), mean, atol=5.1e-5, rtol=0)
            assert np.allclose(table[f"max_{name}"].to_numpy(), np.round(bins.values[c, :, 1], 2), atol=1e-6, rtol=1e-6)
    rows = got.annotations(path=os.path.join(root, "pseudo.csv"))
    back = D.read_annotations(os.path.join(root, "pseudo.csv"))
    assert sorted((i, a, b, l) for i, v in back.items() for a, b, l in v) == sorted(rows) and len(rows) == total
