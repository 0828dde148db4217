"""The probe weights of tests/cnn_probe.py, checked with the CPU oracle alone (no GPU): every channel of every CNN stage
is live on the signals the GPU tests use, the probe differs from the stock weights in BatchNorm shifts only, and a wrong
shift that the stock weights hide is caught with the probe ("Per-channel CNN parity on weights that leave no
channel dead")."""
import functools

import numpy as np

import cnn_probe as P
from buzzdetect_amd import weights as W
from oracle import yamnet_oracle as O


@functools.lru_cache(maxsize=None)
def _weights():
    base, mel = W.synthetic_embedder_blob(), W.load_mel("yamnet_k2")
    return base, P.live_blob(base, mel), mel


@functools.lru_cache(maxsize=None)
def _fused_taps():
    _, live, mel = _weights()
    return P.oracle_taps(P.fused_signal(65), live, mel)[0]


def _dead(taps):
    """Per stage: the channels that have no output above 1e-3 of the stage's median channel maximum."""
    return {s: np.flatnonzero(mx <= 1e-3 * np.median(mx)).tolist()
            for s, (_, mx) in enumerate(P.channel_report(taps)) if (mx <= 1e-3 * np.median(mx)).any()}


def test_every_channel_is_on_for_a_quarter_to_three_quarters_of_the_centring_signal():
    _, live, mel = _weights()
    taps, _ = P.oracle_taps(P.centring_signal(), live, mel)
    assert taps[0].shape[0] == 8
    for stage, (frac, _) in enumerate(P.channel_report(taps)):
        assert frac.min() >= 0.1 and frac.max() <= 0.9, (stage, frac.min(), frac.max())              # the condition
        assert frac.min() >= P.LIVE_LO and frac.max() <= P.LIVE_HI, (stage, frac.min(), frac.max())  # what live_blob built


def test_stock_weights_leave_many_channels_dead():
    """The reason for the probe, as recorded in DESIGN.md: channels per stage whose largest activation on the stage test's
    own input stays below 1e-2 with the stock weights."""
    base, _, mel = _weights()
    x = O.synthetic_audio(P.HOP * 3 + 500, seed=11)
    stock = [int((mx < 1e-2).sum()) for _, mx in P.channel_report(P.oracle_taps(x, base, mel)[0])]
    print(stock)
    assert stock == [0, 0, 0, 2, 2, 4, 0, 8, 8, 10, 7, 24, 53, 54, 49, 45, 18, 29, 32, 38, 24, 32, 26, 66, 159, 151, 88]


def test_every_channel_is_live_on_every_signal_the_gpu_tests_use():
    """On each signal of tests/test_cnn_channels_gpu.py every channel of every stage has an output above 1e-3 of the
    stage's median channel maximum.  One 3x2 map cannot switch 1024 channels on, so the one-window case of the fused-path
    test is five one-window inputs (windows 0..4 of the fused signal, each on its own) and is judged as that set."""
    _, live, mel = _weights()
    for name, x in (("held-out", P.held_out_signal()), ("noise", P.noise_signal())):
        assert not _dead(P.oracle_taps(x, live, mel)[0]), name
    fused = _fused_taps()
    assert fused[0].shape[0] == 65
    for windows in (5, 17, 65):
        assert not _dead([a[:windows] for a in fused]), windows
    assert P.ONE_WINDOW_INPUTS == 5 and not _dead([a[:P.ONE_WINDOW_INPUTS] for a in fused])
    # window w of a prefix is window w of the whole signal, and a window on its own is that window: what the above relies on
    assert np.abs(P.oracle_taps(P.fused_signal(5), live, mel)[0][26] - fused[26][:5]).max() < 1e-12
    assert np.abs(P.oracle_taps(P.one_window_input(3), live, mel)[0][26][0] - fused[26][3]).max() < 1e-12


def test_probe_differs_from_the_stock_weights_in_beta_only():
    base, live, _ = _weights()
    assert live.dtype == np.float32 and live.shape == base.shape and np.isfinite(live).all()
    changed = 0
    tb, tl = P.blob_views(base.copy()), P.blob_views(live.copy())
    assert set(tb) == set(O.split_blob(base))
    for name in tb:
        if name.endswith("/beta"):
            changed += int((tb[name] != tl[name]).sum())
        else:
            assert tb[name].tobytes() == tl[name].tobytes(), name
    assert changed > 4000, changed             # most channels of the deep stages sit outside [0.25, 0.75] with stock weights
    again = P.live_blob(base.copy(), W.load_mel("yamnet_k2"))
    assert again.tobytes() == live.tobytes()   # deterministic


def _perturbed(blob, stage, channel, delta=1e-2):
    out = np.array(blob, dtype=np.float32)
    P.blob_views(out)[f"layer_with_weights-{P.bn_of_stage(stage)}/beta"][channel] += np.float32(delta)
    return out


def test_a_wrong_shift_hidden_by_the_stock_weights_is_caught_with_the_probe():
    """One BatchNorm shift off by 1e-2, at a stage-25 and at a stage-13 channel that the stock weights keep dead.  With the
    stock weights the wrong network stays inside the suite's absolute 1e-4 at every stage and in the logits; with the probe
    the same mistake breaks the per-channel rule at that channel by more than a factor of ten.  (This is the test that fails
    if the probe is swapped for the stock weights: the second half then sees what the first half sees - nothing.)"""
    base, live, mel = _weights()
    head = W.load_head()
    x_stock = O.synthetic_audio(P.HOP * 3 + 500, seed=11)            # the input of test_every_cnn_stage_against_oracle
    x_live = P.held_out_signal()
    stock_taps, stock_emb = P.oracle_taps(x_stock, base, mel)
    live_taps, _ = P.oracle_taps(x_live, live, mel)
    live_taps32, _ = P.oracle_taps(x_live, live, mel, np.float32)
    for stage in (25, 13):
        mx = P.channel_report(stock_taps)[stage][1]
        dead = np.flatnonzero(mx == 0)
        assert dead.size >= 8, (stage, dead.size)
        c = int(dead[0])
        # stock weights: invisible
        taps, emb = P.oracle_taps(x_stock, _perturbed(base, stage, c), mel)
        for s in range(P.N_STAGES):
            assert np.abs(taps[s] - stock_taps[s]).max() < P.TOL_ABS, (stage, c, s)
        logits, ref = (O.dense_head(e, head.kernel, head.bias, np.float64) for e in (emb, stock_emb))
        assert np.abs(logits - ref).max() < P.TOL_ABS, (stage, c)
        # probe weights: the rule of the GPU test, applied to the wrong network in place of the GPU
        taps, _ = P.oracle_taps(x_live, _perturbed(live, stage, c), mel)
        err, ref_max = P.channel_errors(taps, live_taps)[stage]
        err32, _ = P.channel_errors(live_taps32, live_taps)[stage]
        bound = P.channel_bound(stage, err32, ref_max)
        assert err[c] > 10 * bound[c], (stage, c, err[c], bound[c])
        assert np.all(np.delete(err, c) == 0)                        # and it is that channel the rule points at
        _, misses = P.check_channels(taps, live_taps, live_taps32, "perturbed")
        assert misses and f"stage {stage} channel {c}:" in misses[0], misses


def test_channel_errors_and_report_on_a_made_up_stage():
    ref = np.zeros((2, 3, 2, 4))
    ref[1, 2, 1, 0], ref[0, 0, 0, 1], ref[0, 1, 0, 3] = 2.0, -3.0, 0.5
    got = ref.copy()
    got[1, 0, 1, 0] += 0.25
    got[0, 1, 0, 3] -= 0.125
    (err, mx), = P.channel_errors([got], [ref])
    assert err.tolist() == [0.25, 0.0, 0.0, 0.125] and mx.tolist() == [2.0, 3.0, 0.0, 0.5]
    (frac, top), = P.channel_report([ref])
    assert frac.tolist() == [1 / 12, 0.0, 0.0, 1 / 12] and top.tolist() == [2.0, 0.0, 0.0, 0.5]
    assert P.worst_position(got, ref, 0) == (1, 0, 1, True)
    m = P.border_mask(6, 4)
    assert m.sum() == 24 - 8 and not m[1:-1, 1:-1].any()
    (err_in, _), = P.channel_errors([np.ones((1, 6, 4, 1))], [np.where(m, 0.0, 1.0)[None, :, :, None]], [~m])
    assert err_in.tolist() == [0.0]
