"""Recordings of three to eight channels on the device: the general path of every kernel that takes the channel mean
(fir_mfma_kernel's CH = 0 and fir_slow8's last branch, mono_at's loop under resample_kernel / decimate_kernel /
convert_kernel, ar_mono's loop under anyrate_kernel) against the float64 oracle, on channels that can be told apart
(tests/multichannel_cases.py: a wrong stride, a dropped or repeated channel or a wrong divisor moves the output by 0.03 or
more).  The tolerances are those of tests/test_resample.py."""
import numpy as np
import pytest

from tests import multichannel_cases as MC

pytestmark = pytest.mark.gpu

# below and just over one eight-frame staging chunk, shorter than the filter, around one workgroup's outputs, and long enough
# that fir_mfma_kernel's persistent loop commits and refetches; every route reaches every length
LENGTHS = (1, 7, 9, 61, 5374, 4096 * 3 + 1, 100003)

# (quality, rate in) -> the kernel that runs
ROUTES = [("hq", 48000),        # fir_mfma_kernel, one phase block, 3:1
          ("hq", 32000),        # fir_mfma_kernel, one phase block, 2:1
          ("hq", 8000),         # fir_mfma_kernel, up-sampling
          ("hq", 44100),        # fir_mfma_kernel, many phase blocks: rows are separate pieces of the signal
          ("hq", 192000),       # resample_kernel (the vector kernel)
          ("hq", 16000),        # convert_kernel
          ("scipy", 48000),     # decimate_kernel 3:1
          ("scipy", 32000),     # decimate_kernel 2:1
          ("scipy", 44100),     # resample_kernel
          ("hq", 47999),        # anyrate_kernel, interpolated rows (bd_resample refuses the rate)
          ("hq", 768000)]       # anyrate_kernel, exact rows
CASES = [(q, r, c) for q, r in ROUTES for c in (3, 6, 8)] + [("hq", r, c) for r in (48000, 16000) for c in (4, 5, 7)]


def tolerance(quality, dtype, channels):
    """tests/test_resample.py:175, and test_s16_pcm_is_exact_in_the_split's bound where the 16-bit mean is exact in the
    hi + lo f16 split (a power-of-two count; three, five, six or seven channels leave a remainder of up to 5.3e-8)."""
    if quality == "scipy":
        return 2e-6
    return 1.5e-6 if dtype == "s16" and channels in (4, 8) else 5e-6


@pytest.fixture()
def engine_at(engine, request):
    """The session engine at the resampler quality the case asks for; back to the default ("hq") afterwards."""
    engine.set_resample_quality(request.param)
    yield engine, request.param
    engine.set_resample_quality("hq")


@pytest.mark.parametrize("dtype", ["f32", "s16"])
@pytest.mark.parametrize("engine_at,rate_in,channels", CASES, indirect=["engine_at"],
                         ids=[f"{q}-{r}-{c}ch" for q, r, c in CASES])
def test_every_route_matches_the_f64_oracle(engine_at, rate_in, channels, dtype):
    """engine.resample of [n, C] float32 and 16-bit PCM (the marked signal, and full-scale integers with runs at +32767 and
    -32768) against RO.resample: np.mean(axis=1) in float32, then the float64 filter."""
    engine, quality = engine_at
    tol = tolerance(quality, dtype, channels)
    for n in LENGTHS:
        seed = 1000 * channels + n % 997
        signals = {"marked": MC.marked(n, channels, seed)} if dtype == "f32" else \
            {"marked": MC.marked_s16(n, channels, seed), "full scale": MC.full_scale_s16(n, channels, seed)}
        for name, x in signals.items():
            got = engine.resample(x, rate_in).cpu().numpy()
            want = MC.oracle(x, rate_in, quality)
            assert got.shape == want.shape == (-(-n * 16000 // rate_in),)
            err = float(np.abs(got - want).max())
            print(f"{quality} {rate_in} Hz, {channels} channels, {dtype} {name}, {n} frames: max |d| = {err:.3g} (< {tol:g})")
            assert err < tol, (n, name, err)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("channels", [3, 4, 5, 6, 7, 8, 9, 16, 17])
@pytest.mark.parametrize("dtype", ["f32", "s16"])
def test_equal_rates_give_the_reference_mean_bit_for_bit(engine, dtype, channels):
    """At 16 kHz the stage is the downmix alone (convert_kernel: a float4 body and a scalar tail): every output has the bits
    of np.mean(x, axis=1) in float32, 16-bit PCM taken as value / 32768.  From eight channels on NumPy adds a row pairwise;
    np_row_sum (bd_internal.h) restates that order - one block of eight, a ragged tail (9), two blocks (16), both (17).
    A running sum in channel order, which the kernels held to before, has the reference's bits below eight channels only:
    at eight channels of float PCM it was 1 ulp of the mean off on the first frame tried and, where the channels cancel,
    thousands (tests/test_multichannel_host.py), so "within an ulp" was not a bound that order could meet."""
    for n in (1, 3, 4, 5, 1023, 1024, 1025):
        seed = 77 * channels + n
        signals = [MC.marked(n, channels, seed)] if dtype == "f32" else \
            [MC.marked_s16(n, channels, seed), MC.full_scale_s16(n, channels, seed)]
        for x in signals:
            got = engine.resample(x, 16000).cpu().numpy()
            want = np.mean(MC.as_float(x), axis=1)
            assert want.dtype == np.float32 and got.shape == want.shape
            ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
            print(f"{channels} channels, {dtype}, {n} frames: {int((got.view(np.uint32) != want.view(np.uint32)).sum())} of {n} "
                  f"outputs differ, by at most {float(ulps.max()):.3g} ulp of the mean")
            assert float(ulps.max()) <= 1.0
            assert same_bits(got, want), (n, dtype)


def test_a_cut_at_any_alignment_gives_the_outputs_of_the_whole(engine):
    """Six channels of 48 kHz 16-bit PCM: frames [k, k + m) of the recording, for k a multiple of the decimation (the same
    output grid) of every non-zero residue mod 8 - fir_chunk_at's eight-frame chunks then start on other frames of the
    recording - give the outputs of the whole recording, away from the filter's reach of the two cuts.  Where the cut lies
    16-byte aligned in the recording (k a multiple of 4: the entry points refuse other addresses) the kernel reads it in
    place, as a view of the device tensor; elsewhere a copy."""
    import torch
    from oracle import resample_oracle as RO
    n, m = 30011, 9001
    q = torch.from_numpy(MC.marked_s16(n, 6, 6)).to(engine.device)
    whole = engine.resample(q, 48000).cpu().numpy()
    _, half = RO.taps(1, 3)
    reach = half // 3 + 2                                    # outputs either side of a cut that see it
    assert 2 * reach < m // 3 // 2
    for k in (3, 6, 9, 12, 15, 18, 21, 36, 3 * 4099):
        assert k % 8 and k % 3 == 0
        cut = q[k:k + m] if k % 4 == 0 else q[k:k + m].clone()
        assert cut.data_ptr() % 16 == 0 and (cut.data_ptr() == q.data_ptr() + 12 * k) == (k % 4 == 0)
        part = engine.resample(cut, 48000).cpu().numpy()
        assert part.shape == (-(-m // 3),)
        j0 = k // 3
        err = float(np.abs(part[reach:-reach] - whole[j0 + reach:j0 + part.shape[0] - reach]).max())
        print(f"cut at frame {k}: max |d| = {err:.3g}")
        assert err < 5e-6, k
    want = MC.oracle(q.cpu().numpy(), 48000)
    assert np.abs(whole - want).max() < 5e-6


def test_six_channel_48k_pcm_end_to_end(engine, weights_bundle):
    """test_config5_input_48k_stereo_end_to_end with six channels of 16-bit PCM, a tone in one of them: device
    downmix / resample -> predict, against the float64 restatement of the same chain, inside the 1e-4 logit gate."""
    from oracle import resample_oracle as RO
    from oracle import yamnet_oracle as O
    t = np.arange(48000 * 3) / 48000.0
    rng = np.random.default_rng(6)
    x = 0.1 * rng.standard_normal((t.size, 6)) * (np.arange(6) + 1.0) / 6.0
    x[:, 4] += 0.6 * np.sin(2 * np.pi * 220 * t)
    q = (np.clip(x, -1, 1 - 2 ** -15) * 32768.0).round().astype(np.int16)
    mono = engine.resample(q, 48000)
    assert mono.shape[0] == 48000
    got = engine.predict(mono, 0.96).numpy()
    b = weights_bundle
    ref = O.predict(RO.resample(MC.as_float(q), 48000).astype(np.float32), b["blob"], b["mel"], b["head_kernel"], b["head_bias"],
                    15360, 96, np.float64)
    assert got.shape == ref.shape == (4, 13)
    err = float(np.abs(got - ref).max())
    print(f"six channels end to end: max |dlogit| = {err:.3g}")
    assert err < 1e-4
