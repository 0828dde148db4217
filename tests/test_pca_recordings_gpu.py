"""map_recordings / fit_recordings / project_recordings end to end (buzzdetect_amd/pca.py) on three short recordings with the
synthetic embedder weights: the map of a folder is PCA.fit(...).transform(...) over engine.embed of the same chunks in every
bit, its windows are analyze's, an f32 embedding store gives the same result as the audio, the streamed fit and projection
agree with the resident one within the float bound, and to_csv joins the clusters of the same walk."""
import csv
import os
import wave

import numpy as np
import pytest

from buzzdetect_amd import cluster, dataset as D, framing, pca, store
from tests import pca_cases as cases

pytestmark = pytest.mark.gpu

W16 = D.WINDOW_SAMPLES
CHUNK = 4.8                       # five windows per chunk


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
    """Three recordings of about ten windows (16 kHz mono, 44.1 kHz stereo, 16 kHz mono), every chunk as analyze cuts it - at
    16 kHz mono on the device, in the order the recordings are walked - with the (ident, start) analyze writes for each of its
    windows, and the rows engine.embed makes of those chunks."""
    import pandas as pd
    import torch
    from buzzdetect_amd.analyze import analyze
    from buzzdetect_amd.engine import hop_samples, patch_step
    from oracle import yamnet_oracle as O
    root = tmp_path_factory.mktemp("pca")
    audio = root / "audio"
    (audio / "site").mkdir(parents=True)
    a = to_s16(O.synthetic_audio(10 * W16 + 3000, seed=31))
    left = O.synthetic_audio(int(44100 * 9.7), seed=32)
    b = to_s16(np.stack([left, 0.5 * np.roll(left, 441)], axis=1))
    c = to_s16(O.synthetic_audio(9 * W16 + 8000, seed=33))
    write_wav(audio / "a.wav", a, 16000)
    write_wav(audio / "site" / "b.wav", b, 44100)
    write_wav(audio / "c.wav", c, 16000)
    pcm = {"a": (a, 16000), "site/b": (b, 44100), "c": (c, 16000)}
    order = [ident for _, ident in D._recordings(str(audio), {}, False, [])]
    out = root / "out"
    rep = analyze("model_general_v3", chunklength=CHUNK, dir_audio=str(audio), dir_out=str(out), engine=engine)
    assert rep.files_done == 3
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
            n = engine.num_windows(int(dev.numel()), hop_samples(0.96), patch_step(0.96))
            chunks.append(dev)
            where += [(ident, float(s)) for s in starts[at:at + n]]
            at += n
        assert at == starts.size
    rows = torch.cat([engine.embed(c, 0.96).device_tensor() for c in chunks]).contiguous()
    assert rows.shape[0] == len(where) and 25 <= len(where) <= 35
    return str(audio), rows, where, root


def same(a, b):
    assert a.coords.tobytes() == b.coords.tobytes() and a.residual.tobytes() == b.residual.tobytes()
    assert a.recordings == b.recordings and a.recording_of.tolist() == b.recording_of.tolist() and a.starts.tolist() == b.starts.tolist()
    assert a.model.components.tobytes() == b.model.components.tobytes() and a.model.mean.tobytes() == b.model.mean.tobytes()
    assert a.model.explained_variance.tolist() == b.model.explained_variance.tolist() and a.model.n_rows == b.model.n_rows


def test_map_recordings_is_fit_and_transform_over_engine_embed(engine, folder, tmp_path):
    dir_audio, rows, where, root = folder
    found = pca.map_recordings(dir_audio, 2, engine=engine, chunklength=CHUNK)
    ref = pca.PCA(2, device=engine.device).fit(rows)
    y, resid = ref.transform(rows, residual=True)
    assert found.messages == [] and found.coords.shape == (len(where), 2)
    assert found.coords.tobytes() == y.tobytes() and found.residual.tobytes() == resid.tobytes()
    assert found.model.components.tobytes() == ref.components.tobytes() and found.model.n_rows == len(where)
    assert [(found.recordings[r], float(s)) for r, s in zip(found.recording_of, found.starts)] == where      # analyze's starts
    assert np.isfinite(found.coords).all() and (found.residual >= 0).all()

    # a seeded sample, read where the rows lie
    sampled = pca.map_recordings(dir_audio, 2, engine=engine, chunklength=CHUNK, fit_rows=16, seed=5)
    import torch
    taken = torch.from_numpy(pca.sample_rows(len(where), 16, 5).astype(np.int64)).to(rows.device)
    by_hand = pca.PCA(2, device=engine.device).fit(rows.index_select(0, taken).contiguous())
    assert sampled.model.components.tobytes() == by_hand.components.tobytes() and sampled.model.n_rows == 16
    assert sampled.coords.tobytes() == by_hand.transform(rows).tobytes()

    # an embedding store with f32 rows in place of the folder
    emb = str(root / "emb_f32")
    store.embed_recordings(dir_audio, emb, codec="f32", chunklength=CHUNK, engine=engine)
    same(pca.map_recordings(emb, 2, engine=engine, chunklength=CHUNK), found)

    with pytest.raises(ValueError, match=r"max_windows = 2 windows \(\d+ counted"):
        pca.map_recordings(dir_audio, 2, engine=engine, chunklength=CHUNK, max_windows=2)

    # the clusters of the same walk, a label per row
    groups = cluster.cluster_recordings(dir_audio, 3, engine=engine, chunklength=CHUNK, seed=4)
    path = str(tmp_path / "map.csv")
    found.to_csv(path, clusters=groups)
    with open(path, newline="") as f:
        table = list(csv.reader(f))
    assert table[0] == ["ident", "start", "end", "pc1", "pc2", "residual", "cluster"] and len(table) == 1 + len(where)
    assert [int(r[6]) for r in table[1:]] == groups.labels.tolist()
    assert [(r[0], float(r[1])) for r in table[1:]] == where
    assert [np.float32(r[3]) for r in table[1:]] == found.coords[:, 0].tolist()
    kept = pca.map_recordings(dir_audio, 2, engine=engine, chunklength=CHUNK, clusters=groups)
    kept.to_csv(path)
    with open(path, newline="") as f:
        assert list(csv.reader(f)) == table
    worst = found.outliers(3)
    assert [w[2] for w in worst] == sorted(found.residual.tolist(), reverse=True)[:3] and worst[0][:2] == where[int(np.argmax(found.residual))]


def test_streamed_fit_and_projection_agree_with_the_resident_map(engine, folder, tmp_path):
    """fit_recordings cuts the rows by launch sets, so its Gram matrix is another sum of the same terms: the coordinates agree
    with float64's within 8 x the deviation of a NumPy float32 PCA of the same rows, as the resident map's do."""
    dir_audio, rows, where, _ = folder
    model = pca.fit_recordings(dir_audio, 2, engine=engine, chunklength=CHUNK)
    path = str(tmp_path / "model.npz")
    model.save(path)
    streamed = pca.project_recordings(dir_audio, path, engine=engine, chunklength=CHUNK)
    resident = pca.map_recordings(dir_audio, 2, engine=engine, chunklength=CHUNK)
    assert model.n_rows == len(where) and streamed.starts.tolist() == resident.starts.tolist()
    assert streamed.recordings == resident.recordings and streamed.recording_of.tolist() == resident.recording_of.tolist()
    # a saved model projects the same rows to the same bits, streamed or not
    again = pca.PCA.from_model(model, device=engine.device).transform(rows, residual=True)
    assert streamed.coords.tobytes() == again[0].tobytes() and streamed.residual.tobytes() == again[1].tobytes()

    e = rows.cpu().numpy()

    def signed(comps):
        return np.array([v if v[np.argmax(np.abs(v))] > 0 else -v for v in comps])

    def coords(dtype):
        """The header's formula, y = e . v - mean . v, on the components of a PCA in `dtype`; the dot products summed channel
        after channel in `dtype`."""
        comps = signed(cases.pca_reference(e, 2, dtype)[0]).astype(dtype)
        x = e.astype(dtype)
        mean = (x.sum(axis=0, dtype=dtype) / dtype(x.shape[0])).astype(dtype)
        s, mv = np.zeros((x.shape[0], 2), dtype), np.zeros(2, dtype)
        for c in range(x.shape[1]):
            s += np.multiply.outer(x[:, c], comps[:, c])
            mv += mean[c] * comps[:, c]
        return (s - mv[None, :]).astype(np.float64)

    exact = coords(np.float64)
    statement = np.abs(coords(np.float32) - exact).max()
    apart = np.abs(streamed.coords.astype(np.float64) - resident.coords).max()
    print(f"streamed and resident coordinates lie {apart:.3e} apart")
    for name, got in (("streamed", streamed), ("resident", resident)):
        device = np.abs(got.coords - exact).max()
        print(f"{name}: coordinates deviate {device:.3e} from float64, the float32 statement {statement:.3e}; largest {np.abs(exact).max():.3f}")
        assert statement > 0 and device <= cases.BOUND * statement
    assert apart <= cases.BOUND * statement
