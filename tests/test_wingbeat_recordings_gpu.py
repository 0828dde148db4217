"""pitch.wingbeat_recordings end to end on the GPU: a folder with a WAV of ambient noise and two synthetic buzzes of different
fundamentals, and one of noise alone.  The synthetic weights give arbitrary embeddings, so the test makes the head: a linear
layer solved (least squares, minimum norm) from the embeddings of the folder's own windows so that ``ins_buzz`` is +4 on the
windows inside a planted buzz and -4 elsewhere.  The events must be those of calls.call_recordings under the same rules, every
event's f0 within 3 % of the planted fundamental, the quiet recording without an event, and the CSV must read back."""
import os
import wave

import numpy as np
import pytest

from buzzdetect_amd import calls, dataset as D, pitch, weights
from tests import pitch_cases as P

pytestmark = pytest.mark.gpu

W16 = D.WINDOW_SAMPLES
WINDOWS = 22                       # whole windows of a recording; the 2000 samples behind them make one more, padded
PLANTED = ((3, 8, 180.0, "five"), (14, 18, 470.0, "weak"))         # windows [first, end) and the fundamental in them
RULES = dict(thresholds={"ins_buzz": 0.0}, low={"ins_buzz": -2.0}, merge_gap_s=0.0, min_duration_s=1.5)


def write_wav(path, pcm16, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.asarray(pcm16, "<i2").tobytes())


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    assert W16 == P.WINDOW
    root = tmp_path_factory.mktemp("wingbeat")
    audio = root / "audio"
    audio.mkdir()
    n = WINDOWS * W16 + 2000
    buzzing = 0.01 * np.random.default_rng(31).standard_normal(n)
    for i, (first, end, f0, harmonics) in enumerate(PLANTED):
        buzzing[first * W16:end * W16] += P.buzz(f0, P.HARMONICS[harmonics], 0.02, 20.0, 0.0, seed=40 + i, n=(end - first) * W16, amplitude=0.2)
    quiet = 0.01 * np.random.default_rng(32).standard_normal(n)
    pcm = {"buzzing": (np.clip(buzzing, -1, 1 - 2 ** -15) * 32768.0).round().astype(np.int16),
           "quiet": (quiet * 32768.0).round().astype(np.int16)}
    for ident, x in pcm.items():
        write_wav(audio / f"{ident}.wav", x, 16000)
    return str(audio), pcm, str(root)


@pytest.fixture(scope="module")
def listener(engine, folder):
    """An engine whose head scores +4 inside the planted buzzes and -4 elsewhere, and those targets per recording."""
    from buzzdetect_amd.engine import HipEngine
    _, pcm, _ = folder
    rows, targets = [], {}
    for ident, x in pcm.items():
        e = engine.embed(engine.to_device(x.astype(np.float32) / 32768.0), 0.96).numpy()
        assert e.shape[0] == WINDOWS + 1
        t = np.full(e.shape[0], -4.0)
        if ident == "buzzing":
            for first, end, _, _ in PLANTED:
                t[first:end] = 4.0
        rows.append(e.astype(np.float64))
        targets[ident] = t
    e, t = np.concatenate(rows), np.concatenate(list(targets.values()))
    centre = e.mean(axis=0)
    w = np.linalg.lstsq(e - centre, t - t.mean(), rcond=None)[0]
    kernel = np.stack([-w, w], axis=1).astype(np.float32)
    bias = np.array([-(t.mean() - centre @ w), t.mean() - centre @ w], np.float32)
    eng = HipEngine(embeddername="yamnet_k2", head=weights.HeadWeights([(kernel, bias, "linear")], ["ambient", "ins_buzz"]))
    yield eng, targets
    eng.close()


def test_the_events_are_call_recordings_and_carry_the_planted_fundamentals(listener, folder):
    import pandas as pd
    eng, targets = listener
    dir_audio, pcm, root = folder
    scores = eng.predict(eng.to_device(pcm["buzzing"].astype(np.float32) / 32768.0), 0.96).numpy()[:, 1]
    print("ins_buzz of the buzzing recording:", np.round(scores, 2))
    assert ((scores > 0) == (targets["buzzing"] > 0)).all() and (np.abs(scores) > 2.5).all()       # the head does what it was made for
    got = pitch.wingbeat_recordings(dir_audio, engine=eng, **RULES)
    called = calls.call_recordings(dir_audio, engine=eng, **RULES)
    assert got.classes == called.classes == ["ins_buzz"] and got.idents == ["buzzing", "quiet"] and got.messages == called.messages
    assert got.calls() == called.events
    events = got.events[0]
    assert [e[0] for e in events] == ["buzzing", "buzzing"]                                          # the quiet recording: no event
    for e, (first, end, f0, _) in zip(events, PLANTED):
        print(e)
        assert (e[1], e[3], e[4]) == (round(first * 0.96, 2), end - first, end - first)
        assert abs(e[7] / f0 - 1) <= 0.03 and e[8] <= e[7] <= e[9] and e[11] == end - first and 0.5 <= e[10] <= 1.0
        assert abs(e[8] / f0 - 1) <= 0.03 and abs(e[9] / f0 - 1) <= 0.03
    table = got.table()
    assert table.shape == (2,) and list(table["class"]) == ["ins_buzz"] * 2 and np.array_equal(table["f0"], np.float32([e[7] for e in events]))
    out = os.path.join(root, "called")
    got.to_csv(out)
    back = pd.read_csv(os.path.join(out, "buzzing" + pitch.SUFFIX_WINGBEAT))
    assert list(back.columns) == list(pitch.WINGBEAT_COLUMNS) and len(back) == 2
    for row, e in zip(back.itertuples(index=False), events):
        assert (row[0], row.start, row.end, row.windows, row.detected, row.voiced_windows) == ("ins_buzz", e[1], e[2], e[3], e[4], e[11])
        assert (np.float32(row.f0), np.float32(row.f0_min), np.float32(row.f0_max), np.float32(row.clarity)) \
            == tuple(np.float32(v) for v in e[7:11])
        assert row.peak == pytest.approx(float(np.round(np.float32(e[5]), 2)), rel=1e-6, abs=1e-6)
    empty = pd.read_csv(os.path.join(out, "quiet" + pitch.SUFFIX_WINGBEAT))
    assert list(empty.columns) == list(pitch.WINGBEAT_COLUMNS) and len(empty) == 0


def test_an_embedding_store_is_refused(listener, folder):
    from buzzdetect_amd import store
    eng, _ = listener
    dir_audio, _, root = folder
    kept = os.path.join(root, "store")
    store.embed_recordings(dir_audio, kept, engine=eng)
    with pytest.raises(ValueError, match="holds no audio"):
        pitch.wingbeat_recordings(kept, engine=eng, **RULES)
    with pytest.raises(ValueError, match="holds no audio"):
        pitch.wingbeat_recordings(store.Store(kept), engine=eng, **RULES)
