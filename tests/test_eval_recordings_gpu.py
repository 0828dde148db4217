"""evaluate.evaluate_recordings end to end on the GPU: a folder with a 16 kHz WAV of three chunks, a 44.1 kHz stereo FLAC, a
recording the annotations do not mention and a file below the minimum size, evaluated at framehop_prop 1.0 and 0.5 against
evaluate.sweep_host over engine.predict of every chunk as analyze cuts it, with labels from dataset._label_at on
framing.window_starts; a list of two models against each alone; events against a matcher restated here over calls.events_host;
write_metrics read back by results.threshold_for_precision.  The synthetic weights give arbitrary logits, so the rules'
thresholds are quantiles of the logits themselves."""
import os
import wave

import numpy as np
import pytest

from buzzdetect_amd import calls, dataset as D, evaluate as E, framing, modeldir as G, results

pytestmark = pytest.mark.gpu

W16 = D.WINDOW_SAMPLES
CHUNK = 20                         # rounds to 20.16 s: 21 windows a chunk at hop 0.96, 41 at hop 0.48
NAMES = ["ins_buzz", "ambient_rain"]
# ident -> (start, end, label): whole windows, a straddle that leaves window 10 of "a" ambiguous at hop 0.96 (it holds 0.30 s of
# a 0.96 s piece, window 11 the other 0.66 s), an interval across the first chunk edge, a label that is not evaluated
NOTES = {"a": [(1.92, 4.8, "ins_buzz"), (10.26, 11.22, "ins_buzz"), (19.0, 22.5, "ins_buzz"), (30.0, 33.0, "ambient_rain"),
               (40.0, 41.0, "mech_plane"), (31.0, 32.2, "ins_buzz")],
         "site/b": [(0.0, 2.0, "ambient_rain"), (4.0, 6.5, "ins_buzz")],
         "ghost": [(0.0, 1.0, "ins_buzz")]}


def write_wav(path, pcm16, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.asarray(pcm16, "<i2").tobytes())


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from oracle import yamnet_oracle as O
    from tools import flacgen as F
    root = tmp_path_factory.mktemp("evaluate")
    audio = root / "audio"
    (audio / "site").mkdir(parents=True)
    a = (np.clip(O.synthetic_audio(52 * W16 + 3000, seed=21), -1, 1 - 2 ** -15) * 32768.0).round().astype(np.int16)
    b = F.test_signal(int(44100 * 9.7), 2, 16, seed=6)
    write_wav(audio / "a.wav", a, 16000)
    (audio / "site" / "b.flac").write_bytes(F.encode(b, 44100, 16, blocksize=4608, mode="mid_side"))
    write_wav(audio / "unmentioned.wav", a[:5 * W16], 16000)
    write_wav(audio / "tiny.wav", a[:1000], 16000)
    G.write_model_dir(str(root / "models" / "b"), G.glorot_layers([2], ["linear"], seed=2), classes=["other", "ins_buzz"])
    return str(audio), {"a": (a, 16000), "site/b": (b, 44100)}, str(root)


@pytest.fixture(scope="module")
def reference(engine, folder):
    """Per framehop and recording (starts, logits [W, n_classes], labels uint8 [W, 2]): engine.predict of every chunk as analyze
    cuts it; computed once, never changed."""
    _, pcm, _ = folder
    out = {}
    for prop in (1.0, 0.5):
        framehop_s = 0.96 * prop
        for ident, (x, rate) in pcm.items():
            starts, rows = [], []
            for edge in framing.gaps_to_chunklist([(0, x.shape[0] / rate)], framing.round_chunklength(CHUNK)):
                lo, hi = framing.chunk_sample_range(edge, rate)
                hi = min(hi, x.shape[0])
                if hi <= lo:
                    continue
                part = x[lo:hi]
                dev = engine.resample(part.astype(np.int16), rate, 16000) if rate != 16000 else \
                    engine.to_device(part.astype(np.float32) / 32768.0)
                logits = engine.predict(dev, framehop_s).numpy()
                rows.append(logits)
                starts.append(framing.window_starts(logits.shape[0], float(edge[0]), framehop_s, 2))
            starts = np.concatenate(starts)
            kept = [row for row in NOTES[ident] if row[2] in NAMES]
            targets, keep, _ = D._label_at(starts, kept, NAMES, 0.5, None)
            labels = targets.astype(np.uint8)
            labels[~keep] = 2
            out[prop, ident] = (starts, np.concatenate(rows).astype(np.float32), labels)
    return out


def same_curve(got, want):
    return (np.array_equal(got.thresholds, want.thresholds) and np.array_equal(got.tp, want.tp) and np.array_equal(got.fp, want.fp)
            and (got.n_pos, got.n_neg, got.n_skipped) == (want.n_pos, want.n_neg, want.n_skipped) and got.table() == want.table())


def host_curves(reference, prop, columns):
    """One Curve per (score column, label column) of ``columns`` by sweep_host over both recordings' reference logits."""
    state = None
    for ident in ("a", "site/b"):
        _, logits, labels = reference[prop, ident]
        x = np.ascontiguousarray(logits[:, [c for c, _ in columns]])
        state = E.sweep_host(x, labels, [l for _, l in columns], 2, state)
    return E.curves_of(*state, [l for _, l in columns])


@pytest.mark.parametrize("framehop_prop", (1.0, 0.5))
def test_evaluate_recordings_is_the_host_sweep_over_engine_predict(engine, folder, reference, framehop_prop):
    dir_audio, pcm, root = folder
    cols = [engine.classes.index(n) for n in NAMES]
    got = E.evaluate_recordings(dir_audio, NOTES, classes=NAMES, engine=engine, framehop_prop=framehop_prop, chunklength=CHUNK)
    assert list(got.curves) == [("model_general_v3", n) for n in NAMES] and got.events == {}
    said = "\n".join(got.messages)
    assert len(got.messages) == 3 and "tiny" in said and "annotated, but no such recording: ghost" in said
    assert "not evaluated, ignored: mech_plane" in said and "unmentioned" not in said
    want = host_curves(reference, framehop_prop, [(cols[0], 0), (cols[1], 1)])
    windows = sum(reference[framehop_prop, ident][0].shape[0] for ident in pcm)
    for name, curve in zip(NAMES, want):
        mine = got.curves[("model_general_v3", name)]
        assert same_curve(mine, curve), name
        assert mine.n_pos > 0 and mine.n_neg > 0 and mine.n_pos + mine.n_neg + mine.n_skipped == windows      # "unmentioned" is not in
    if framehop_prop == 1.0:
        labels = reference[1.0, "a"][2]
        assert labels[10].tolist() == [2, 2] and labels[11].tolist() == [1, 0] and labels[32].tolist() == [1, 1]
        assert got.curves[("model_general_v3", "ins_buzz")].n_skipped >= 1
    # without only_annotated the recording nobody mentions is all negative
    more = E.evaluate_recordings(dir_audio, NOTES, classes=NAMES[:1], engine=engine, framehop_prop=framehop_prop, chunklength=CHUNK,
                                 only_annotated=False)
    extra = more.curves[("model_general_v3", "ins_buzz")]
    assert extra.n_pos == want[0].n_pos and extra.n_neg > want[0].n_neg


def test_background_makes_untouched_windows_its_positives(engine, folder, reference):
    dir_audio, _, _ = folder
    got = E.evaluate_recordings(dir_audio, NOTES, classes=NAMES, background="ambient_rain", engine=engine, chunklength=CHUNK)
    plain = host_curves(reference, 1.0, [(engine.classes.index(n), l) for l, n in enumerate(NAMES)])
    rain = got.curves[("model_general_v3", "ambient_rain")]
    assert same_curve(got.curves[("model_general_v3", "ins_buzz")], plain[0])
    assert rain.n_pos > plain[1].n_pos and rain.n_pos + rain.n_neg == plain[1].n_pos + plain[1].n_neg


def test_a_list_of_models_gives_each_models_lone_curves(engine, folder, monkeypatch):
    dir_audio, _, root = folder
    monkeypatch.setenv("BUZZDETECT_MODELS_DIR", os.path.join(root, "models"))     # the packaged model stays reachable beside "b"
    both = E.evaluate_recordings(dir_audio, NOTES, ["model_general_v3", "b"], classes=["ins_buzz"], chunklength=CHUNK)
    assert list(both.curves) == [("model_general_v3", "ins_buzz"), ("b", "ins_buzz")]
    lone = E.evaluate_recordings(dir_audio, NOTES, classes=["ins_buzz"], engine=engine, chunklength=CHUNK)
    assert same_curve(both.curves[("model_general_v3", "ins_buzz")], lone.curves[("model_general_v3", "ins_buzz")])
    alone = E.evaluate_recordings(dir_audio, NOTES, "b", classes=["ins_buzz"], chunklength=CHUNK)
    assert same_curve(both.curves[("b", "ins_buzz")], alone.curves[("b", "ins_buzz")])
    assert not same_curve(both.curves[("b", "ins_buzz")], lone.curves[("model_general_v3", "ins_buzz")])
    with pytest.raises(ValueError, match="classes \\['ambient_rain'\\] are not among the classes of 'b'"):
        E.evaluate_recordings(dir_audio, NOTES, ["model_general_v3", "b"], classes=NAMES, chunklength=CHUNK)
    # the table lands where analyze(precision=...) looks, and reads back to the curve's own threshold
    curve = both.curves[("b", "ins_buzz")]
    seen = curve.tp + curve.fp > 0
    p = float(np.sort(curve.tp[seen] / (curve.tp + curve.fp)[seen])[int(seen.sum()) // 2])      # a precision some row has
    with pytest.raises(FileExistsError):
        both.write_metrics(os.path.join(root, "models"))
    paths = both.write_metrics(os.path.join(root, "models"), overwrite=True)
    assert paths[1] == os.path.join(root, "models", "b", "tests", "metrics.csv") and open(paths[1]).read() == curve.table()
    back = results.threshold_for_precision("b", p, 0.05, metrics_path=paths[1])
    assert back == curve.threshold_for_precision(p, 0.05) and not np.isnan(back)


def matched(spans, pieces, least=1):
    """(hits, found) by the plain double loop over integer ticks."""
    hits = sum(any(min(b, q) - max(a, p) >= least for p, q in pieces) for a, b in spans)
    found = sum(any(min(b, q) - max(a, p) >= least for a, b in spans) for p, q in pieces)
    return hits, found


def test_events_are_matched_as_the_loop_over_events_host_matches_them(engine, folder, reference):
    dir_audio, pcm, _ = folder
    col = engine.classes.index("ins_buzz")
    every = np.concatenate([reference[1.0, ident][1][:, col] for ident in pcm])
    rule = calls.Rule(float(np.percentile(every, 70)), float(np.percentile(every, 40)), merge_gap_s=1.0, min_duration_s=1.5)
    got = E.evaluate_recordings(dir_audio, NOTES, classes=NAMES, rules={"ins_buzz": rule}, engine=engine, chunklength=CHUNK)
    assert list(got.events) == [("model_general_v3", "ins_buzz")]
    adjacent = calls.adjacent_ticks(0.96)
    want = dict(events=0, hits=0, pieces=0, found=0, tp=0, fp=0, fn=0)
    for ident in pcm:
        starts, logits, labels = reference[1.0, ident]
        t = calls.ticks(starts)
        marks, events = calls.events_host(np.ascontiguousarray(logits[:, col:col + 1]), t, adjacent, [rule])
        spans = [(int(t[f]), int(t[l]) + 96) for f, l, _, _, kept in events[0] if kept]
        ticks = sorted((int(round(100 * a)), int(round(100 * b))) for a, b, label in NOTES[ident] if label == "ins_buzz")
        pieces = []
        for a, b in ticks:                                                 # the union, touching intervals merged
            if pieces and a <= pieces[-1][1]:
                pieces[-1][1] = max(pieces[-1][1], b)
            else:
                pieces.append([a, b])
        hits, found = matched(spans, pieces)
        called, lab = marks[0] >= 2, labels[:, 0]
        for key, value in (("events", len(spans)), ("hits", hits), ("pieces", len(pieces)), ("found", found),
                           ("tp", int((called & (lab == 1)).sum())), ("fp", int((called & (lab == 0)).sum())),
                           ("fn", int((~called & (lab == 1)).sum()))):
            want[key] += value
    score = got.events[("model_general_v3", "ins_buzz")]
    assert {k: getattr(score, k) for k in want} == want
    assert want["events"] > 0 and want["pieces"] == 5 and want["tp"] + want["fn"] > 0
    row = got.summary()[0]
    assert row["events"] == want["events"] and row["window_tp"] == want["tp"] and got.summary()[1]["events"] is None
