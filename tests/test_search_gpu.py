"""Search by example on the GPU (csrc/simsearch.hip, buzzdetect_amd/search.py): the norms and the selection against their host
restatements in every bit, the scores against float64 under the 8 x rule of DESIGN §15 and independent of a row's or a query's
position, pass splits, and search_recordings / top_windows against engine.embed / engine.predict of the same chunks.  Every
buffer a kernel writes lies between guard words (a NaN payload no kernel produces) that must stay untouched."""
import os
import wave

import numpy as np
import pytest

from buzzdetect_amd import _lib, dataset as D, framing, search

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC12345            # tests/test_mix_gpu.py's pattern
GUARD = 64                       # words either side: 256 bytes, so the inside keeps a 16-byte alignment


class Guarded:
    """Device buffers with GUARD sentinel words in front and behind; the inside starts as sentinels too."""

    def __init__(self):
        self.whole = []

    def empty(self, shape, dtype, device="cuda"):
        import torch
        words = int(np.prod(shape)) * (2 if dtype == torch.int64 else 1)
        raw = torch.full((2 * GUARD + words,), SENTINEL, dtype=torch.int32, device=device)
        self.whole.append((raw, words))
        return raw[GUARD:GUARD + words].view(dtype).view(*shape)

    def check(self, written=True):
        import torch
        torch.cuda.synchronize()
        assert self.whole
        for raw, words in self.whole:
            host = raw.cpu().numpy()
            assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + words:] == SENTINEL).all(), "a guard word changed"
            if written:
                assert not (host[GUARD:GUARD + words] == SENTINEL).any(), "an output element was not written"
        self.whole = []


class GuardedSearcher(search.Searcher):
    guards = Guarded()

    def _empty(self, shape, dtype):
        return self.guards.empty(shape, dtype, self.device)


@pytest.fixture(scope="module")
def corpus():
    """1025 rows of mixed magnitude (one all zero, one below the norm floor) and 65 queries, on both sides."""
    import torch
    assert torch.cuda.is_available()
    rng = np.random.default_rng(2024)
    e = np.abs(rng.normal(size=(1025, 1024))).astype(np.float32) * rng.choice([0.03, 1.0, 30.0], size=(1025, 1))
    e = e.astype(np.float32)
    e[:, rng.integers(0, 1024, 300)] *= -1.0
    e[7] = 0.0
    e[40] = 1e-18
    q = rng.normal(size=(65, 1024)).astype(np.float32) + 0.5
    return e, q, torch.from_numpy(e).cuda(), None


def lib_norms(e_dev, guards):
    import torch
    n2 = guards.empty((e_dev.shape[0],), torch.float32)
    _lib.check(_lib.load().bd_search_norms(e_dev.data_ptr(), e_dev.shape[0], n2.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return n2


@pytest.mark.parametrize("w", (1, 31, 32, 33, 257))
def test_norms_are_the_host_norms_in_every_bit(corpus, w):
    e, _, e_dev, _ = corpus
    guards = Guarded()
    rows = e_dev[3:3 + w].contiguous()
    n2 = lib_norms(rows, guards)
    got = n2.cpu().numpy()
    guards.check()
    assert got.tobytes() == search.norms_host(e[3:3 + w]).tobytes()
    if w > 4:
        assert got[4] == 0.0


@pytest.fixture(scope="module")
def restatements(corpus):
    """Per metric: the float64 scores of rows 0 .. 256 against all 65 queries and the plain float32 NumPy restatement of the same
    product, each computed once; a case with Q queries is held against their first Q columns (the device's scores do not depend
    on which other queries there are)."""
    e, q = corpus[0][:257], corpus[1]
    out = {}
    for metric in ("dot", "cosine"):
        q32 = search.normalise_queries(q, metric)
        want = e.astype(np.float64) @ q32.astype(np.float64).T
        plain = e @ q32.T
        if metric == "cosine":
            n64 = (e.astype(np.float64) ** 2).sum(axis=1, keepdims=True)
            want = np.divide(want, np.sqrt(n64), out=np.zeros_like(want), where=n64 >= _lib.SEARCH_NORM_FLOOR)
            n32 = (e * e).sum(axis=1, keepdims=True, dtype=np.float32)
            plain = np.divide(plain, np.sqrt(n32), out=np.zeros_like(plain), where=n32 >= np.float32(_lib.SEARCH_NORM_FLOOR))
        assert plain.dtype == np.float32 and want.dtype == np.float64
        out[metric] = (q32, want, plain)
    return out


@pytest.mark.parametrize("metric", ("dot", "cosine"))
@pytest.mark.parametrize("nq", (1, 31, 32, 33, 65))
def test_scores_against_float64_under_the_8x_rule(corpus, restatements, nq, metric):
    """the device's largest deviation from float64 is at most 8 x that of the plain float32 NumPy restatement of the
    same inputs.  The restatement is ONE float32 matrix product over the 65 queries, shared by the cases (`restatements`).
    Measured on an MI355X: ratios 2.6 - 3.0 for every case.  (NumPy computes a product with a single query by another route, a
    vector dot whose error on these inputs is about 2.5 x smaller than its matrix product's; held against THAT, the one-query
    case measured 7.14 for dot and 4.48 for cosine - the device adds the 1024 terms of a score in one serial chain.)"""
    e, q, e_dev, _ = corpus
    rows = e_dev[:257].contiguous()
    q32, want, plain = restatements[metric]
    s = GuardedSearcher(q[:nq], k=5, metric=metric)
    assert s.queries.tobytes() == q32[:nq].tobytes()
    got = s.scores(rows).cpu().numpy()
    s.guards.check()
    assert got.shape == (257, nq)
    if metric == "cosine":
        assert (got[7] == 0).all() and (got[40] == 0).all() and np.abs(got).max() <= 1.0 + 1e-5
    dev = np.abs(got.astype(np.float64) - want[:, :nq]).max()
    ref = np.abs(plain[:, :nq].astype(np.float64) - want[:, :nq]).max()
    print(f"{metric}, Q = {nq}: device deviation {dev:.3e}, float32 NumPy deviation {ref:.3e}, ratio {dev / ref:.2f}")
    assert dev <= 8.0 * ref


@pytest.mark.parametrize("metric", ("dot", "cosine"))
def test_a_score_does_not_depend_on_where_its_row_or_its_query_sits(corpus, metric):
    import torch
    e, q, e_dev, _ = corpus
    r = 517
    s = GuardedSearcher(q[:33], k=5, metric=metric)
    alone = s.scores(e_dev[r:r + 1].contiguous()).cpu().numpy()
    for pos in (0, 31, 32, 1024):
        rows = e_dev.clone()
        rows[pos] = e_dev[r]
        assert s.scores(rows)[pos].cpu().numpy().tobytes() == alone[0].tobytes(), f"row at {pos}"
    s.guards.check()
    one = GuardedSearcher(q[64:65], k=5, metric=metric)
    column = one.scores(e_dev).cpu().numpy()[:, 0]
    for pos in (0, 31, 32, 64):
        qs = q[:65].copy()
        qs[[pos, 64]] = qs[[64, pos]]
        many = GuardedSearcher(qs, k=5, metric=metric)
        assert many.scores(e_dev).cpu().numpy()[:, pos].tobytes() == column.tobytes(), f"query at {pos}"
    one.guards.check()
    assert np.isfinite(column).all() and column.any() and torch.cuda.is_available()


@pytest.mark.parametrize("k", (1, 64, 65, 1024))
def test_selection_on_device_scores_is_the_host_selection(corpus, k):
    """Every row three times, 350 apart and in different passes: bit-equal scores meet, the lower id wins."""
    import torch
    e, q, e_dev, _ = corpus
    lib = _lib.load()
    rows = torch.cat([e_dev[:350]] * 3).contiguous()
    nq = 5
    s = GuardedSearcher(q[:nq], k=k, metric="cosine")
    guards = Guarded()
    keys_dev = guards.empty((nq, k), torch.int64).zero_()
    keys_host = np.zeros((nq, k), np.uint64)
    at = 0
    for n in (400, 400, 250):
        part = rows[at:at + n]
        scores = s.scores(part)
        _lib.check(lib.bd_search_update(scores.data_ptr(), n, nq, nq, 1, at, keys_dev.data_ptr(), k,
                                        torch.cuda.current_stream().cuda_stream))
        search.update_host(keys_host, scores.cpu().numpy(), at)
        assert s.update(part) == at
        at += n
    got = keys_dev.cpu().numpy().view(np.uint64)
    guards.check()
    assert got.tobytes() == keys_host.tobytes()
    assert s.keys().tobytes() == keys_host.tobytes()                      # the query-major path of Searcher.update
    s.guards.check()
    scores, ids = s.result()
    assert scores.shape == (nq, min(k, 1050))
    if k >= 64:
        for c in range(nq):
            assert ids[c, 1] == ids[c, 0] + 350 and ids[c, 2] == ids[c, 0] + 700 and ids[c, 0] < 350
            assert scores[c, 0] == scores[c, 1] == scores[c, 2] >= scores[c, 3]
    else:
        assert (ids[:, 0] < 350).all()


def test_logits_with_specials_select_as_on_the_host(corpus):
    """bd_search_update on a strided matrix with NaN, infinities and both zeros, W < k and W > one batch."""
    import torch
    rng = np.random.default_rng(6)
    for w, k in ((5, 64), (4097, 100), (3000, 1024)):
        wide = rng.choice(np.array([-1.0, 0.0, -0.0, 0.5, 2.0, np.inf, -np.inf, np.nan], np.float32), size=(w, 7))
        wide_dev = torch.from_numpy(wide).cuda()
        s = GuardedSearcher(None, k=k, n_queries=3)
        s.update_scores(wide_dev[:, 1:6:2])
        want = search.update_host(np.zeros((3, k), np.uint64), wide[:, 1:6:2], 0)
        assert s.keys().tobytes() == want.tobytes()
        s.guards.check()


def test_pass_splits_give_the_same_result(corpus):
    e, q, e_dev, _ = corpus
    once = GuardedSearcher(q[:5], k=100)
    assert once.update(e_dev) == 0
    split, at = GuardedSearcher(q[:5], k=100), 0
    for n in (1, 31, 32, 33, 928):
        assert split.update(e_dev[at:at + n]) == at
        at += n
    a, b = once.result(), split.result()
    once.guards.check()
    assert at == 1025 and a[0].shape == (5, 100)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert (np.diff(a[0], axis=1) <= 0).all()


# ---------------------------------------------------------------------------------------------------- end to end
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
    """Three recordings of about ten windows: 16 kHz mono, 44.1 kHz stereo, 16 kHz mono.  Also every chunk as analyze cuts it, at
    16 kHz mono on the device, in the order the recordings are walked, with the start column analyze writes."""
    import pandas as pd
    from buzzdetect_amd.analyze import analyze
    from buzzdetect_amd.engine import hop_samples, patch_step
    from oracle import yamnet_oracle as O
    root = tmp_path_factory.mktemp("search")
    audio = root / "audio"
    (audio / "site").mkdir(parents=True)
    a = to_s16(O.synthetic_audio(10 * W16 + 3000, seed=11))
    left = O.synthetic_audio(int(44100 * 9.7), seed=12)
    b = to_s16(np.stack([left, 0.5 * np.roll(left, 441)], axis=1))
    c = to_s16(O.synthetic_audio(9 * W16 + 8000, seed=13))
    write_wav(audio / "a.wav", a, 16000)
    write_wav(audio / "site" / "b.wav", b, 44100)
    write_wav(audio / "c.wav", c, 16000)
    pcm = {"a": (a, 16000), "site/b": (b, 44100), "c": (c, 16000)}
    rep = analyze("model_general_v3", chunklength=CHUNK, dir_audio=str(audio), dir_out=str(root / "out"), engine=engine)
    assert rep.files_done == 3
    order = [ident for _, ident in D._recordings(str(audio), {}, False, [])]
    assert sorted(order) == sorted(pcm)
    chunks, where = [], []
    for ident in order:
        x, rate = pcm[ident]
        starts = np.sort(pd.read_csv(os.path.join(root / "out", ident + "_buzzdetect.csv"))["start"].to_numpy())
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
    return str(audio), chunks, where


def test_search_recordings_is_a_searcher_over_engine_embed(engine, folder, monkeypatch):
    dir_audio, chunks, where = folder
    monkeypatch.setattr(search, "Searcher", GuardedSearcher)
    rows = [engine.embed(c, 0.96).device_tensor() for c in chunks]
    counts = [int(r.shape[0]) for r in rows]
    assert sum(counts) == len(where) and 25 <= len(where) <= 35
    pick, j = 3, 2                                                          # the query: window 2 of the fourth chunk
    wid = sum(counts[:pick]) + j
    queries = np.stack([rows[pick][j].cpu().numpy(), rows[0][0].cpu().numpy()])
    for metric in ("cosine", "dot"):
        got = search.search_recordings(dir_audio, queries, k=5, metric=metric, engine=engine, chunklength=CHUNK)
        ref = GuardedSearcher(queries, k=5, metric=metric, device=engine.device)
        for r in rows:
            ref.update(r)
        scores, ids = ref.result()
        GuardedSearcher.guards.check()
        assert got.messages == [] and len(got.hits) == 2
        for qi in range(2):
            assert [(i, s) for i, s, _ in got.hits[qi]] == [where[w] for w in ids[qi]]
            assert np.array([v for _, _, v in got.hits[qi]], np.float32).tobytes() == scores[qi].tobytes()
        if metric == "cosine":
            assert got.hits[0][0][:2] == where[wid] and got.hits[1][0][:2] == where[0]
            assert abs(got.hits[0][0][2] - 1.0) < 1e-5


def test_top_windows_is_a_top_k_over_engine_predict(engine, folder, monkeypatch):
    dir_audio, chunks, where = folder
    monkeypatch.setattr(search, "Searcher", GuardedSearcher)
    logits = np.concatenate([engine.predict(c, 0.96).numpy() for c in chunks])
    names = [engine.classes[3], engine.classes[0]]
    cols = [3, 0]
    ids = np.arange(logits.shape[0])
    for largest in (True, False):
        got = search.top_windows(dir_audio, classes=names, k=7, largest=largest, engine=engine, chunklength=CHUNK)
        GuardedSearcher.guards.check()
        assert got.names == names and got.messages == []
        for qi, col in enumerate(cols):
            v = logits[:, col]
            order = np.lexsort((ids, -v.astype(np.float64) if largest else v.astype(np.float64)))[:7]
            assert [(i, s) for i, s, _ in got.hits[qi]] == [where[w] for w in order]
            assert np.array([x for _, _, x in got.hits[qi]], np.float32).tobytes() == v[order].tobytes()


def test_queries_from_annotations_are_the_labelled_windows(engine, folder):
    dir_audio, chunks, where = folder
    ident = where[0][0]                                                     # the first recording walked; its first chunk has 5 windows
    rows = engine.embed(chunks[0], 0.96).numpy()
    notes = {ident: [(0.96, 1.46, "buzz"), (3 * 0.96, 3 * 0.96 + 0.5, "buzz"), (4 * 0.96 + 0.1, 4 * 0.96 + 0.4, "other")]}
    each = search.queries_from_annotations(dir_audio, notes, "buzz", engine=engine, chunklength=CHUNK)
    assert each.dtype == np.float32 and each.tobytes() == rows[[1, 3]].tobytes()
    mean = search.queries_from_annotations(dir_audio, notes, "buzz", reduce="mean", engine=engine, chunklength=CHUNK)
    assert mean.tobytes() == rows[[1, 3]].astype(np.float64).mean(axis=0, keepdims=True).astype(np.float32).tobytes()
    assert search.queries_from_annotations(dir_audio, notes, "other", engine=engine, chunklength=CHUNK).tobytes() == rows[4:5].tobytes()
    with pytest.raises(ValueError, match="nobody"):
        search.queries_from_annotations(dir_audio, notes, "nobody", engine=engine)
