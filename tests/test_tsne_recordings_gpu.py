"""layout_recordings end to end (buzzdetect_amd/tsne.py): a folder of a few short synthetic WAVs against TSNE.fit on
neighbour_graph's lists with the PCA start of map_recordings, an embedding store in place of the folder, the window index, what
is refused, and the CSV."""
import csv
import wave
from types import SimpleNamespace

import numpy as np
import pytest

from buzzdetect_amd import dataset as D, pca, propagate, store, tsne

pytestmark = pytest.mark.gpu

W16 = D.WINDOW_SAMPLES
CHUNK = 4.8                       # five windows per chunk
SCHEDULE = dict(perplexity=4, exaggeration_iter=20, n_iter=40)
K = 12


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
def folder(tmp_path_factory):
    """Three recordings of about ten windows: 16 kHz mono, 44.1 kHz stereo, 16 kHz mono."""
    from oracle import yamnet_oracle as O
    root = tmp_path_factory.mktemp("layout")
    audio = root / "audio"
    (audio / "site").mkdir(parents=True)
    left = O.synthetic_audio(int(44100 * 9.7), seed=52)
    write_wav(audio / "a.wav", to_s16(O.synthetic_audio(10 * W16 + 3000, seed=51)), 16000)
    write_wav(audio / "site" / "b.wav", to_s16(np.stack([left, 0.5 * np.roll(left, 441)], axis=1)), 44100)
    write_wav(audio / "c.wav", to_s16(O.synthetic_audio(9 * W16 + 8000, seed=53)), 16000)
    return str(audio), root


def test_layout_recordings_is_the_fit_over_the_graph_and_the_pca_start(engine, folder, monkeypatch, tmp_path):
    dir_audio, root = folder
    schedule = tsne.Schedule(**SCHEDULE)
    found = tsne.layout_recordings(dir_audio, k=K, schedule=schedule, engine=engine, chunklength=CHUNK)
    graph = propagate.neighbour_graph(dir_audio, K, engine=engine, chunklength=CHUNK)
    plane = pca.map_recordings(dir_audio, 2, engine=engine, chunklength=CHUNK)
    n = graph.ids.shape[0]
    assert n >= 25 and found.messages == [] and found.coords.shape == (n, 2) and np.isfinite(found.coords).all()
    assert found.graph.ids.tobytes() == graph.ids.tobytes() and found.graph.sims.tobytes() == graph.sims.tobytes()
    assert found.recordings == plane.recordings and found.starts.tobytes() == plane.starts.tobytes()
    assert found.recording_of.tobytes() == plane.recording_of.tobytes()
    start = tsne.scaled_start(plane.coords)
    assert start[:, 0].astype(np.float64).std() == pytest.approx(1e-4, rel=1e-5)
    ref = tsne.TSNE(schedule, device=engine.device)
    assert found.coords.tobytes() == ref.fit(graph, start).tobytes() and found.kl == ref.kl_ and np.isfinite(found.kl)
    assert 0 <= found.preservation(k=5) <= 1

    # the same graph without its rows, from a seeded start
    loose = tsne.layout_graph(graph, seed=3, schedule=schedule, device=engine.device)
    again = tsne.layout_graph(graph, seed=3, schedule=schedule, device=engine.device)
    assert loose.coords.tobytes() == again.coords.tobytes() and loose.coords.tobytes() != found.coords.tobytes()

    # an embedding store with f32 rows in place of the folder: the same bytes, and no embedder launch
    emb = str(root / "emb_f32")
    store.embed_recordings(dir_audio, emb, codec="f32", chunklength=CHUNK, engine=engine)

    def launch(*args, **kwargs):
        raise AssertionError("an embedder launch on the store route")
    monkeypatch.setattr(engine, "launch", launch)
    stored = tsne.layout_recordings(emb, k=K, schedule=schedule, engine=engine, chunklength=CHUNK)
    monkeypatch.undo()
    assert stored.coords.tobytes() == found.coords.tobytes() and stored.kl == found.kl
    assert stored.recordings == found.recordings and stored.starts.tobytes() == found.starts.tobytes()

    # what is refused
    with pytest.raises(ValueError, match=r"max_windows = 2 windows \(\d+ counted"):
        tsne.layout_recordings(dir_audio, k=K, schedule=schedule, engine=engine, chunklength=CHUNK, max_windows=2)
    with pytest.raises(ValueError, match="not the same walk"):
        tsne.layout_recordings(dir_audio, k=K, schedule=schedule, engine=engine, chunklength=CHUNK,
                               clusters=SimpleNamespace(labels=np.zeros(n + 1, np.int32)))
    with pytest.raises(ValueError, match="3 x perplexity"):
        tsne.layout_recordings(dir_audio, k=K, engine=engine, chunklength=CHUNK)            # the default perplexity asks k >= 48

    # the CSV, with and without clusters of the same walk
    path = tmp_path / "layout.csv"
    found.to_csv(str(path))
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["ident", "start", "end", "x", "y"] and len(rows) == 1 + n
    assert [r[0] for r in rows[1:]] == [found.recordings[r] for r in found.recording_of]
    labelled = tsne.layout_recordings(dir_audio, k=K, schedule=schedule, engine=engine, chunklength=CHUNK,
                                      clusters=SimpleNamespace(labels=np.arange(n, dtype=np.int32)))
    labelled.to_csv(str(path))
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0][-1] == "cluster" and [int(r[-1]) for r in rows[1:]] == list(range(n)) and len(rows) == 1 + n
    assert labelled.coords.tobytes() == found.coords.tobytes()
