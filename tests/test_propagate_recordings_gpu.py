"""neighbour_graph and propagate_recordings end to end (buzzdetect_amd/propagate.py): a folder of synthetic WAVs against
bd_knn_update and Propagator over engine.embed of the same chunks, the index against analyze's start column, an embedding store
in place of the folder, and the annotations read back by dataset.read_annotations."""
import os
import wave

import numpy as np
import pytest

from buzzdetect_amd import dataset as D, framing, propagate, store

pytestmark = pytest.mark.gpu

W16 = D.WINDOW_SAMPLES
CHUNK = 4.8                       # five windows per chunk
CLASSES = ["ambient", "ins_buzz"]


def write_wav(path, pcm16, rate):
    pcm16 = np.asarray(pcm16, "<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if pcm16.ndim == 1 else pcm16.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm16.tobytes())


def to_s16(x):
    return (np.clip(x, -1, 1 - 2 ** -15) * 32768.0).round().astype(np.int16)


@pytest.fixture(scope="module")
def folder(tmp_path_factory, engine):
    """Three recordings of about ten windows (16 kHz mono, 44.1 kHz stereo, 16 kHz mono) and, per hop (whole and half), the rows
    engine.embed makes of every chunk as analyze cuts it, in the order the recordings are walked, with the (ident, start) analyze
    writes for each of its windows."""
    import pandas as pd
    import torch
    from buzzdetect_amd.analyze import analyze
    from buzzdetect_amd.engine import hop_samples, patch_step
    from oracle import yamnet_oracle as O
    root = tmp_path_factory.mktemp("propagate")
    audio = root / "audio"
    (audio / "site").mkdir(parents=True)
    a = to_s16(O.synthetic_audio(10 * W16 + 3000, seed=41))
    left = O.synthetic_audio(int(44100 * 9.7), seed=42)
    b = to_s16(np.stack([left, 0.5 * np.roll(left, 441)], axis=1))
    c = to_s16(O.synthetic_audio(9 * W16 + 8000, seed=43))
    write_wav(audio / "a.wav", a, 16000)
    write_wav(audio / "site" / "b.wav", b, 44100)
    write_wav(audio / "c.wav", c, 16000)
    pcm = {"a": (a, 16000), "site/b": (b, 44100), "c": (c, 16000)}
    order = [ident for _, ident in D._recordings(str(audio), {}, False, [])]
    per_hop = {}
    for prop in (1.0, 0.5):
        out = root / f"out{prop}"
        rep = analyze("model_general_v3", chunklength=CHUNK, dir_audio=str(audio), dir_out=str(out), engine=engine, framehop_prop=prop)
        assert rep.files_done == 3
        hop_s = 0.96 * prop
        chunks, where = [], []
        for ident in order:
            x, rate = pcm[ident]
            starts = np.sort(pd.read_csv(os.path.join(out, ident + "_buzzdetect.csv"))["start"].to_numpy())
            at = 0
            for edge in framing.gaps_to_chunklist([(0, x.shape[0] / rate)], framing.round_chunklength(CHUNK)):
                lo, hi = framing.chunk_sample_range(edge, rate)
                hi = min(hi, x.shape[0])
                if hi <= lo:
                    continue
                part = x[lo:hi]
                dev = engine.resample(part, rate, 16000) if rate != 16000 else engine.to_device(part.astype(np.float32) / 32768.0)
                n = engine.num_windows(int(dev.numel()), hop_samples(hop_s), patch_step(hop_s))
                chunks.append(dev)
                where += [(ident, float(s)) for s in starts[at:at + n]]
                at += n
            assert at == starts.size
        rows = torch.cat([engine.embed(c, hop_s).device_tensor() for c in chunks]).contiguous()
        assert rows.shape[0] == len(where)
        per_hop[prop] = (rows, where)
    return str(audio), per_hop, root


@pytest.mark.parametrize("prop", (1.0, 0.5))
def test_neighbour_graph_is_knn_update_over_engine_embed(engine, folder, prop, tmp_path):
    dir_audio, per_hop, _ = folder
    rows, where = per_hop[prop]
    for metric, k in (("cosine", 8), ("dot", 3)):
        got = propagate.neighbour_graph(dir_audio, k, metric=metric, engine=engine, chunklength=CHUNK, framehop_prop=prop)
        ids, sims = propagate.Neighbours(k, metric=metric, device=engine.device).update(rows).lists()
        assert got.messages == [] and got.metric == metric and got.k == k
        assert got.ids.tobytes() == ids.tobytes() and got.sims.tobytes() == sims.tobytes()
        assert [(got.recordings[r], float(s)) for r, s in zip(got.recording_of, got.starts)] == where        # analyze's starts
        assert (got.ids >= 0).all() and (got.ids != np.arange(len(where))[:, None]).all()
        want = propagate.knn_update_host(np.zeros((len(where), k), np.uint64), rows.cpu().numpy(), rows.cpu().numpy(), metric=metric,
                                         exclude_self=True)
        assert propagate.decode_keys(want)[0].tobytes() == ids.tobytes()
    near = got.neighbours(*where[3])
    assert [n[:2] for n in near] == [where[j] for j in got.ids[3]]
    path = str(tmp_path / "graph.npz")
    got.save(path)
    assert propagate.KnnGraph.load(path).ids.tobytes() == got.ids.tobytes()
    with pytest.raises(ValueError, match=r"max_windows = 2 windows \(\d+ counted"):
        propagate.neighbour_graph(dir_audio, 4, engine=engine, chunklength=CHUNK, framehop_prop=prop, max_windows=2)


def same(a, b):
    for name in ("labels", "confidence", "margin", "reach", "scores", "annotated", "recording_of", "starts"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    assert a.iterations == b.iterations and a.recordings == b.recordings and a.classes == b.classes


def test_propagate_recordings_is_the_propagator_over_those_rows(engine, folder, monkeypatch, tmp_path):
    dir_audio, per_hop, root = folder
    rows, where = per_hop[1.0]
    # a buzz in a.wav over windows 2 .. 3, ambience at its start; a buzz in c.wav; site/b stays unlabelled
    notes = {"a": [(0.0, 0.96, "ambient"), (1.92, 3.84, "ins_buzz")], "c": [(4.8, 5.76, "ins_buzz"), (0.0, 1.92, "ambient")]}
    labelled = [i for i, (ident, s) in enumerate(where) if (ident == "a" and s in (0.0, 1.92, 2.88)) or (ident == "c" and s in (0.0, 0.96, 4.8))]
    classes_of = {("a", 0.0): 0, ("a", 1.92): 1, ("a", 2.88): 1, ("c", 0.0): 0, ("c", 0.96): 0, ("c", 4.8): 1}
    labels = [classes_of[where[i]] for i in labelled]
    assert len(labelled) == 6
    ids, sims = propagate.Neighbours(4, device=engine.device).update(rows).lists()
    y, alpha = propagate.targets_of(labelled, labels, len(where), 2)
    for symmetric in (True, False):
        got = propagate.propagate_recordings(dir_audio, notes, CLASSES, k=4, symmetric=symmetric, engine=engine, chunklength=CHUNK,
                                             max_iter=20)
        graph = propagate.lists_csr(ids, sims).symmetrised() if symmetric else (ids, sims)
        ref = propagate.Propagator(power=4, max_iter=20, tol=1e-4, device=engine.device).fit(graph, y, alpha)
        assert got.messages == [] and got.graph.ids.tobytes() == ids.tobytes()
        assert np.flatnonzero(got.annotated).tolist() == labelled
        assert got.scores.tobytes() == ref.scores.tobytes() and got.labels.tobytes() == ref.labels.tobytes()
        assert got.confidence.tobytes() == ref.confidence.tobytes() and got.margin.tobytes() == ref.margin.tobytes()
        assert got.reach.tobytes() == ref.reach.tobytes() and got.iterations == ref.iterations
        assert [(got.recordings[r], float(s)) for r, s in zip(got.recording_of, got.starts)] == where
        assert (got.labels[labelled] == labels).all()                    # clamp 1: a labelled window keeps its label
    assert (got.reach <= 1.0 + 1e-5).all() and (got.reach[labelled] == 1).all()

    # a soft clamp and a given graph (nothing is embedded again)
    soft = propagate.propagate_recordings(dir_audio, notes, CLASSES, k=4, clamp=0.75, graph=got.graph, engine=engine, chunklength=CHUNK,
                                          max_iter=20)
    y2, alpha2 = propagate.targets_of(labelled, labels, len(where), 2, clamp=0.75)
    assert (alpha2[labelled] == 0.25).all()
    ref = propagate.Propagator(max_iter=20, device=engine.device).fit(propagate.lists_csr(ids, sims).symmetrised(), y2, alpha2)
    assert soft.scores.tobytes() == ref.scores.tobytes()

    # an embedding store with f32 rows in place of the folder: the same result, and no embedder launch
    sym = propagate.propagate_recordings(dir_audio, notes, CLASSES, k=4, engine=engine, chunklength=CHUNK, max_iter=20)
    emb = str(root / "emb_f32")
    store.embed_recordings(dir_audio, emb, codec="f32", chunklength=CHUNK, engine=engine)

    def launch(*args, **kwargs):
        raise AssertionError("an embedder launch on the store route")
    monkeypatch.setattr(engine, "launch", launch)
    stored = propagate.propagate_recordings(emb, notes, CLASSES, k=4, engine=engine, chunklength=CHUNK, max_iter=20)
    stored_graph = propagate.neighbour_graph(emb, 4, engine=engine, chunklength=CHUNK)
    monkeypatch.undo()
    same(stored, sym)
    assert stored_graph.ids.tobytes() == ids.tobytes() and stored_graph.sims.tobytes() == sims.tobytes()

    # the trusted windows go back in as annotations
    path = str(tmp_path / "more.csv")
    rows_out = sym.annotations(min_confidence=0.5, min_reach=0.0, path=path)
    read = D.read_annotations(path)
    assert sum(len(v) for v in read.values()) == len(rows_out) > 0
    assert sorted((ident, s, e, l) for ident, spans in read.items() for s, e, l in spans) == sorted(rows_out)
    assert not {(r[0], r[1]) for r in rows_out} & {where[i] for i in labelled}       # the annotated windows are left out
    sym.to_csv(str(tmp_path / "all.csv"))
    with open(tmp_path / "all.csv") as f:
        assert len(f.read().splitlines()) == 1 + len(where)
