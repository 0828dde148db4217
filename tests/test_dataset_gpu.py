"""buzzdetect_amd/dataset.py on the GPU, with the suite's synthetic weights: embed_annotated reads, chunks and embeds as analyze
does; augment's mixtures are bd_mix_host's, embedded as engine.embed embeds them; and the chain annotations -> embed_annotated +
augment -> fit_head -> save_model -> analyze finds tone bursts in a recording it has not seen."""
import os
import wave

import numpy as np
import pytest

from buzzdetect_amd import dataset as D, framing, train
from tests import train_oracle as T

pytestmark = pytest.mark.gpu

W = D.WINDOW_SAMPLES
CLASSES = ["ambient", "ins_buzz"]


def write_wav(path, pcm16):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.asarray(pcm16, "<i2").tobytes())


def to_s16(x):
    return (np.clip(x, -1, 1 - 2 ** -15) * 32768.0).round().astype(np.int16)


def chunk_ranges(frames, rate, chunklength):
    """analyze's chunks of a recording of `frames` frames: (chunk start in seconds, first frame, end frame)."""
    chunks = framing.gaps_to_chunklist([(0, frames / rate)], framing.round_chunklength(chunklength))
    out = []
    for c in chunks:
        a, b = framing.chunk_sample_range(c, rate)
        if min(b, frames) > a:
            out.append((float(c[0]), a, min(b, frames)))
    return out


def analyze_starts(engine, dir_audio, dir_out, ident, hop_prop, chunklength):
    import pandas as pd
    from buzzdetect_amd.analyze import analyze
    rep = analyze("model_general_v3", framehop_prop=hop_prop, chunklength=chunklength, dir_audio=str(dir_audio), dir_out=str(dir_out),
                  engine=engine)
    assert rep.files_done == 1
    return pd.read_csv(os.path.join(dir_out, ident + "_buzzdetect.csv"))["start"].to_numpy()


@pytest.mark.parametrize("hop_prop", (1.0, 0.5))
def test_embed_annotated_reads_chunks_and_embeds_as_analyze_does(engine, tmp_path, hop_prop):
    from oracle import yamnet_oracle as O
    pcm = to_s16(O.synthetic_audio(5 * W + 5000, seed=5))           # three chunks of two windows: 2 + 2 + 1.3
    write_wav(tmp_path / "audio" / "site" / "rec.wav", pcm)
    hop_s = 0.96 * hop_prop
    ts = D.embed_annotated(str(tmp_path / "audio"), {}, CLASSES, engine=engine, framehop_prop=hop_prop, chunklength=1.92,
                           background="ambient")
    ranges = chunk_ranges(pcm.size, 16000, 1.92)
    assert len(ranges) == 3 and ts.idents == ["site/rec"] and ts.messages == []
    want = [engine.embed(pcm[a:b].astype(np.float32) / 32768.0, hop_s).numpy() for _, a, b in ranges]
    whole = np.concatenate(want)
    assert ts.embeddings.cpu().numpy().tobytes() == whole.tobytes() and whole.any()
    starts = analyze_starts(engine, tmp_path / "audio", tmp_path / "out", "site/rec", hop_prop, 1.92)
    assert len(ts) == len(starts) == sum(len(w) for w in want)
    assert np.array_equal(ts.starts, np.sort(starts)) and (ts.groups == 0).all() and (ts.targets == [1, 0]).all()
    # labelled: a buzz over the second chunk's first window and 0.2 s of the next; that one is ambiguous and left out
    notes = {"site/rec": [(1.92, 3.08, "ins_buzz")]}
    lab = D.embed_annotated(str(tmp_path / "audio"), notes, CLASSES, engine=engine, framehop_prop=hop_prop, chunklength=1.92,
                            background="ambient")
    exact = np.concatenate([c0 + np.arange(len(w)) * hop_s for (c0, _, _), w in zip(ranges, want)])
    targets, keep, _ = D._label_at(exact, notes["site/rec"], CLASSES, 0.5, "ambient")
    assert 0 < keep.sum() < keep.size and targets[keep][:, 1].sum() >= 1
    assert lab.embeddings.cpu().numpy().tobytes() == whole[keep].tobytes()
    assert lab.targets.tobytes() == targets[keep].tobytes() and np.array_equal(lab.starts, ts.starts[keep])


def test_embed_annotated_on_stereo_flac_at_44100_is_the_analyze_path(engine, tmp_path):
    from tools import flacgen as G
    rate = 44100
    pcm = G.test_signal(int(rate * 5.3), 2, 16, seed=4)
    (tmp_path / "audio").mkdir()
    (tmp_path / "audio" / "f.flac").write_bytes(G.encode(pcm, rate, 16, blocksize=4608, mode="mid_side"))
    ts = D.embed_annotated(str(tmp_path / "audio"), {}, CLASSES, engine=engine, chunklength=1.92, background="ambient")
    ranges = chunk_ranges(pcm.shape[0], rate, 1.92)
    assert len(ranges) == 3
    want = np.concatenate([engine.embed(engine.resample(pcm[a:b].astype(np.int16), rate, 16000), 0.96).numpy() for _, a, b in ranges])
    assert ts.embeddings.cpu().numpy().tobytes() == want.tobytes() and want.any()
    starts = analyze_starts(engine, tmp_path / "audio", tmp_path / "out", "f", 1.0, 1.92)
    assert np.array_equal(ts.starts, np.sort(starts))


def bursts_recording(n_samples, seed):
    """synthetic_audio: 0.1 noise, a 0.5 s tone burst at 0.3 every 5 s; the bursts as annotation intervals."""
    from oracle import yamnet_oracle as O
    audio = O.synthetic_audio(int(n_samples), seed=seed)
    seconds = n_samples / 16000.0
    return to_s16(audio), [(5.0 * k, 5.0 * k + 0.5, "ins_buzz") for k in range(int(seconds // 5) + 1) if 5.0 * k + 0.5 <= seconds]


def test_augment_rows_are_engine_embed_of_the_host_mixtures(engine, tmp_path):
    pcm, notes = bursts_recording(40 * W, seed=17)
    # three events: the bursts at 5 and 10 s (one window each) and a long one of three whole windows; the other bursts stay unannotated
    notes = notes[1:3] + [(24.0, 27.2, "ins_buzz")]
    write_wav(tmp_path / "audio" / "r.wav", pcm)
    kw = dict(snr_db=(0, 10), per_event=2, gain_db=(0.0, -6.0), background="ambient", seed=3, engine=engine, chunklength=9.6)
    ts = D.augment(str(tmp_path / "audio"), {"r": notes}, CLASSES, **kw)
    again = D.augment(str(tmp_path / "audio"), {"r": notes}, CLASSES, **kw)
    assert ts.embeddings.cpu().numpy().tobytes() == again.embeddings.cpu().numpy().tobytes()
    assert ts.plan.tobytes() == again.plan.tobytes() and ts.targets.tobytes() == again.targets.tobytes()
    # the same layout, clips and plan on the host
    ranges = chunk_ranges(pcm.size, 16000, 9.6)
    assert len(ranges) >= 4
    audio = np.concatenate([pcm[a:b] for _, a, b in ranges]).astype(np.float32) / 32768.0
    layout, at = [], 0
    for c0, a, b in ranges:
        layout.append((0, c0, b - a, at))
        at += b - a
    events, stretches = D.find_clips(layout, {0: notes}, CLASSES, background="ambient")
    plan = D.draw_plan(events, stretches, snr_db=(0, 10), per_event=2, gain_db=(0.0, -6.0), seed=3)
    assert [e.windows for e in events] == [1, 1, 3] and plan.size == 6 and ts.plan.tobytes() == plan.tobytes()
    assert not plan["dropped"].any() and ts.messages == []
    got = ts.embeddings.cpu().numpy()
    at = 0
    for row in plan:
        clip = D.mix_descriptors([row["ev_off"]], [row["nz_off"]], [row["n"]], [row["snr_db"]], [row["gain_db"]])
        mixed, power, flags = D.mix_host(audio, audio, clip)
        want = engine.embed(mixed, 0.96).numpy()
        ev = events[row["event"]]
        assert want.shape[0] == ev.windows and flags[0] == 0 and power[0, 1] > 0
        assert got[at:at + ev.windows].tobytes() == want.tobytes(), f"mixture of event {row['event']} at {row['snr_db']} dB"
        assert ts.targets[at:at + ev.windows].tobytes() == ev.targets.tobytes() and (ev.targets[:, 1] == 1).all()
        assert np.array_equal(ts.starts[at:at + ev.windows], ev.starts) and (ts.groups[at:at + ev.windows] == row["group"]).all()
        at += ev.windows
    assert at == len(ts)


HOP = 15360
TONE_LEVEL = 0.6        # test_train_gpu.two_kinds' constant, raised as its comment says to: at 0.3 the float64 restatement does not
                        # separate a recording it has not seen on the synthetic weights' embeddings (held-out accuracy 0.50 after 40
                        # epochs, 0.91 after 80, noise recall 0.81; at 0.6: 1.00 from 80 epochs on, the same at 160)


def two_kinds(windows, seed):
    """test_train_gpu.two_kinds restated: `windows` windows cut at the tone bursts of synthetic_audio (0.5 s of every 5 s) and as
    many cut between them, each kind laid end to end as one recording."""
    from oracle import yamnet_oracle as O
    audio = O.synthetic_audio(5 * 16000 * windows + HOP + 240, seed=seed).astype(np.float64)
    t = np.arange(audio.size) / 16000.0
    audio = np.clip(audio + (TONE_LEVEL - 0.3) * np.sin(2 * np.pi * 220.0 * t) * (np.mod(t, 5.0) < 0.5), -1.0, 1.0 - 2.0 ** -23)
    tone = np.concatenate([audio[5 * 16000 * k: 5 * 16000 * k + HOP] for k in range(windows)] + [audio[-240:]])
    noise = np.concatenate([audio[5 * 16000 * k + 32000: 5 * 16000 * k + 32000 + HOP] for k in range(windows)] + [audio[-240:]])
    return tone.astype(np.float32), noise.astype(np.float32)


def test_annotations_to_a_model_that_finds_the_bursts_in_a_held_out_recording(engine, tmp_path):
    """At the size of test_train_gpu's end-to-end test: a recording of 64 windows that each begin with a burst, annotated, and one
    of 64 windows without; held out: a recording from another seed, 16 windows with bursts, then 16 without."""
    import pandas as pd
    from buzzdetect_amd.analyze import analyze
    tone, noise = two_kinds(64, seed=99)
    held_tone, held_noise = two_kinds(16, seed=7)
    write_wav(tmp_path / "train" / "tone.wav", to_s16(tone))
    write_wav(tmp_path / "train" / "noise.wav", to_s16(noise))
    write_wav(tmp_path / "held" / "h.wav", to_s16(np.concatenate([held_tone[: 16 * HOP], held_noise])))
    with open(tmp_path / "notes.csv", "w") as f:
        f.write("ident,start,end,label\n" + "".join(f"tone,{0.96 * k},{0.96 * k + 0.5},ins_buzz\n" for k in range(64)))
    notes = D.read_annotations(str(tmp_path / "notes.csv"))
    real = D.embed_annotated(str(tmp_path / "train"), notes, CLASSES, engine=engine, background="ambient")
    mixed = D.augment(str(tmp_path / "train"), notes, CLASSES, snr_db=(5, 10), per_event=2, background="ambient", seed=1, engine=engine)
    both = D.concat(real, mixed)
    assert real.idents == ["noise", "tone"] and real.targets.sum(axis=0).tolist() == [64, 64]
    assert len(mixed) == 2 * 64 and (mixed.targets[:, 1] == 1).all() and (mixed.groups == 1).all() and not mixed.plan["dropped"].any()
    assert len(both) == 256 and both.idents == ["noise", "tone"] and (both.groups[128:] == 1).all()
    held_notes = {"h": [(0.96 * k, 0.96 * k + 0.5, "ins_buzz") for k in range(16)]}
    held = D.embed_annotated(str(tmp_path / "held"), held_notes, CLASSES, engine=engine, background="ambient")
    is_tone = held.targets[:, 1] == 1
    assert len(held) == 32 and is_tone.tolist() == [True] * 16 + [False] * 16

    def scores(logit):
        """(accuracy, recall of the burst windows, recall of the others) of `logit > 0`."""
        hit = logit > 0
        return float((hit == is_tone).mean()), float(hit[is_tone].mean()), float((~hit)[~is_tone].mean())

    # the float64 restatement trained with the same seed and batches, alone: does it separate the two kinds?  100 epochs: the
    # mixtures (bursts under added noise) make the first epochs call everything a burst, and the fit has to run past that
    kw = dict(classes=CLASSES, loss="binary", epochs=100, batch_size=16, seed=21, learning_rate=1e-3)
    x_host, n_fit = both.embeddings.cpu().numpy(), len(both)
    rng = np.random.default_rng(21)
    layers = train.glorot_layers(rng, [2], ["linear"])
    batches = []
    for _ in range(100):
        perm = rng.permutation(n_fit)
        batches += [(perm[at:at + 16], both.targets[perm[at:at + 16]]) for at in range(0, n_fit, 16)]
    ref = T.train(layers, x_host, batches, "binary", T.Adam())
    ref_acc, ref_tone, ref_noise = scores(T.forward(ref, held.embeddings.cpu().numpy())[-1][:, 1])
    print(f"restatement: held-out accuracy {ref_acc:.3f}, recall of burst windows {ref_tone:.3f}, of the others {ref_noise:.3f} "
          f"at tone level {TONE_LEVEL} ({len(real)} real + {len(mixed)} mixed rows)")
    assert ref_acc >= 0.9                                           # as test_train_gpu asks of its two kinds

    fit = train.fit_head(both.embeddings, both.targets, **kw)
    assert fit.history["loss"][-1] < fit.history["loss"][0]
    train.save_model(str(tmp_path / "models" / "model_bursts"), fit, digits_results=4)
    rep = analyze("model_bursts", dir_audio=str(tmp_path / "held"), dir_out=str(tmp_path / "out"), dir_models=str(tmp_path / "models"),
                  analyzers_gpu=1)
    assert rep.files_done == 1
    out = pd.read_csv(tmp_path / "out" / "h_buzzdetect.csv")
    assert np.array_equal(np.sort(out["start"].to_numpy()), held.starts)
    acc, tone_found, noise_left = scores(out.sort_values("start")["activation_ins_buzz"].to_numpy())
    print(f"analyze with the fitted model: accuracy {acc:.3f}, recall of burst windows {tone_found:.3f}, of the others {noise_left:.3f}")
    assert tone_found >= ref_tone - 1.0 / 16 and noise_left >= ref_noise - 1.0 / 16 and acc >= 0.9
