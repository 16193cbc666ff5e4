"""sepkern/resample.py, the definition of the resampling front end (the `sr=` half of librosa.core.load), and its host-side
plumbing: the length rule, the plan, the fp64 reference against scipy.signal.upfirdn with the plan's own prototype filter,
tones, the wav readers and the collator of a mixed-rate batch, and sk_resample's argument checks.  CPU only.

The constants and the length rule are UNPINNED (neither resampy nor librosa is available to test against): what is held
here is that the polyphase tables, the closed-form first index and the host reference are one filter -- upfirdn convolves
the zero-stuffed signal with the whole prototype --, that this filter has unit DC gain, passes a tone and removes one above
the new Nyquist."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.io.wavfile
import scipy.signal

from conftest import PKG, ROOT

sys.path.insert(0, os.path.join(PKG, "archs"))
sys.path.insert(0, os.path.join(PKG, "steps"))

from sepkern import resample as R  # noqa: E402

PAIRS = [(16000, 8000), (48000, 8000), (44100, 8000), (11025, 8000), (8000, 16000)]


def test_out_len_is_the_exact_ceiling():
    cases = [(32000, 16000, 8000, 16000), (32001, 16000, 8000, 16001), (1, 16000, 8000, 1), (0, 16000, 8000, 0),
             (44100, 44100, 8000, 8000), (44101, 44100, 8000, 8001), (441, 44100, 8000, 80), (442, 44100, 8000, 81),
             (100, 44100, 8000, 19),                  # 100 * 80 = 8000 is not divisible by 441: 18.14 -> 19
             (11025, 11025, 8000, 8000), (1000, 11025, 8000, 726), (6, 48000, 8000, 1), (7, 48000, 8000, 2),
             (3000, 8000, 16000, 6000), (2 ** 31 - 1, 48000, 8000, 357913942), (10 ** 12 + 1, 44100, 8000, 181405895692)]
    for n, a, b, want in cases:
        assert R.out_len(n, a, b) == want, (n, a, b)
        L, M = R.ratio(a, b)
        assert R.out_len(n, a, b) == -((-n * L) // M)
        assert (R.out_len(n, a, b) - 1) * M < n * L <= R.out_len(n, a, b) * M or n == 0


def test_plan_shapes_and_dc_gain():
    want = {(16000, 8000): (1, 2, 257), (44100, 8000): (80, 441, 706), (48000, 8000): (1, 6, 769), (11025, 8000): (320, 441, 177),
            (8000, 16000): (2, 1, 129)}
    for a, b in PAIRS:
        pl = R.plan(a, b)
        assert (pl.L, pl.M, pl.ntaps) == want[(a, b)]
        assert pl is R.plan(a, b)                                          # cached per rate pair
        assert pl.taps.shape == (pl.L, pl.ntaps) and pl.taps.dtype == np.float64
        gain = pl.taps.sum(axis=1)
        assert np.abs(gain - 1.0).max() < 1e-6, (a, b, np.abs(gain - 1.0).max())
        # the closed-form first index: every input sample with a non-zero weight lies inside the row's ntaps columns
        n = np.arange(5 * pl.L + 7)
        t_first = (n * pl.M / pl.L - pl.first(n)) * pl.scale               # filter argument of the first and the last column
        t_last = (n * pl.M / pl.L - (pl.first(n) + pl.ntaps - 1)) * pl.scale
        assert np.all(t_first < R.NUM_ZEROS) and np.all((n * pl.M / pl.L - (pl.first(n) - 1)) * pl.scale >= R.NUM_ZEROS - 1e-9)
        assert np.all(t_last <= -R.NUM_ZEROS + pl.scale + 1e-9)
    with pytest.raises(ValueError):
        R.plan(8000, 8000)
    assert np.array_equal(R.resample_host(np.arange(5.0), 8000, 8000), np.arange(5.0))


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_host_reference_against_upfirdn(sr_in, sr_out):
    pl = R.plan(sr_in, sr_out)
    x = np.random.default_rng(sr_in + sr_out).standard_normal(3000)
    y = R.resample_host(x, sr_in, sr_out)
    assert len(y) == R.out_len(3000, sr_in, sr_out)
    u = scipy.signal.upfirdn(pl.prototype(), x, up=pl.L)                   # u[j] = sum_k x[k] h[j - half - k L]
    idx = np.arange(len(y)) * pl.M + pl.half
    ref = np.where(idx < len(u), u[np.minimum(idx, len(u) - 1)], 0.0)
    diff = np.abs(y - ref).max()
    print("resample_host vs upfirdn %d -> %d: max difference %.3g" % (sr_in, sr_out, diff))
    assert diff <= 1e-7


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_tones(sr_in, sr_out):
    n = np.arange(4 * sr_in // 10)
    y = R.resample_host(np.sin(2 * np.pi * 1000.0 * n / sr_in), sr_in, sr_out)
    m = np.arange(len(y))
    err = np.abs(y - np.sin(2 * np.pi * 1000.0 * m / sr_out))[400:-400].max()
    assert len(y) > 1200 and err <= 1e-6, err
    if sr_out < sr_in:                       # a tone at 1.1 x the output Nyquist is in the stop band
        y = R.resample_host(np.sin(2 * np.pi * (0.55 * sr_out) * n / sr_in), sr_in, sr_out)
        rms = np.sqrt(np.mean(y[400:-400] ** 2))
        print("%d -> %d: 1 kHz tone error %.3g, stop-band rms %.3g" % (sr_in, sr_out, err, rms))
        assert rms <= 1e-6, rms


def test_read_pcm_returns_the_files_own_rate(tmp_path):
    import extract_feats
    x = np.random.default_rng(1).integers(-3000, 3000, 16000).astype(np.int16)
    p = str(tmp_path / "a.wav")
    scipy.io.wavfile.write(p, 16000, x)
    got, fs = extract_feats.read_pcm(p)
    assert fs == 16000 and got.dtype == np.int16 and np.array_equal(got, x)
    # a segments cut is taken at the FILE's rate, by the rule of librosa.load(offset=, duration=)
    got, fs = extract_feats.read_pcm(p, 0.25, 0.5)
    assert fs == 16000 and np.array_equal(got, x[4000:12000])
    assert "not built" not in open(extract_feats.__file__).read()


def test_wav_frames_at_the_target_rate(tmp_path):
    from sepkern.data import wav_frames
    for n, fs in ((32001, 16000), (44100, 44100), (5000, 8000)):
        p = str(tmp_path / ("w%d.wav" % n))
        scipy.io.wavfile.write(p, fs, np.zeros(n, np.int16))
        assert wav_frames(p) == 1 + n // 128
        assert wav_frames(p, sample_rate=8000) == 1 + R.out_len(n, fs, 8000) // 128
        assert wav_frames(p, sample_rate=fs) == 1 + n // 128


def test_wav_collator_orders_a_mixed_rate_batch_by_target_rate_frames():
    import uPIT
    rng = np.random.default_rng(3)

    def utt(n, rate, short=0):
        return {"mix": rng.integers(-100, 100, n).astype(np.int16), "source1": rng.integers(-100, 100, n - short).astype(np.int16),
                "source2": rng.integers(-100, 100, n).astype(np.int16), "rate": rate}
    # native lengths 9000 @ 8 k, 16000 @ 16 k (8000 at 8 k), 44100 @ 44.1 k (8000 at 8 k: 63 frames, as the one before),
    # 30000 @ 48 k (5000 at 8 k): by native length the order would be 2, 3, 1, 0
    batch = [utt(9000, 8000), utt(16000, 16000), utt(44100, 44100), utt(30000, 48000)]
    frames = [1 + R.out_len(len(d["mix"]), d["rate"], 8000) // 128 for d in batch]
    assert frames == [71, 63, 63, 40]
    out = uPIT.WavCollator(8000)([dict(d) for d in batch])["pcm"]
    order = list(np.argsort(np.array(frames))[::-1])
    assert out["keys"] == ["mix", "source1", "source2"] and out["target_rate"] == 8000
    assert out["lens"] == [len(batch[i]["mix"]) for i in order] and out["rate"] == [batch[i]["rate"] for i in order]
    assert out["lens"][0] == 9000 and out["lens"][-1] == 30000
    got_frames = [1 + R.out_len(n, r, 8000) // 128 for n, r in zip(out["lens"], out["rate"])]
    assert got_frames == sorted(got_frames, reverse=True)
    assert out["flat"].dtype.is_floating_point is False
    assert np.array_equal(out["flat"].numpy(), np.concatenate([batch[i][k] for k in out["keys"] for i in order]))
    with pytest.raises(ValueError, match="must have the mixture's length"):
        uPIT.WavCollator(8000)([utt(16000, 16000), utt(32000, 16000, short=1)])
    with pytest.raises(ValueError, match="'rate'"):
        uPIT.WavCollator(8000)([{k: v for k, v in utt(16000, 16000).items() if k != "rate"}])
    # without a rate the collator is the one it was: no new keys
    plain = uPIT.WavCollator()([{k: v for k, v in d.items() if k != "rate"} for d in batch])["pcm"]
    assert sorted(plain) == ["flat", "keys", "lens"] and plain["lens"] == [44100, 30000, 16000, 9000]


def test_wav_train_set_records_the_rate(tmp_path):
    import uPIT
    root = tmp_path / "wav16k"
    for d in ("mix", "s1", "s2"):
        os.makedirs(str(root / d))
        scipy.io.wavfile.write(str(root / d / "u0.wav"), 16000, np.full(20000, len(d), np.int16))
    data = tmp_path / "data"
    os.makedirs(str(data))
    with open(str(data / "wav.scp"), "w") as f:
        f.write("u0 %s/mix/u0.wav\n" % root)
    old = uPIT.WavTrainSet(str(data))
    assert sorted(old[0]) == ["mix", "source1", "source2"] and old.frame_counts() == [1 + 20000 // 128]
    ds = uPIT.WavTrainSet(str(data), sample_rate=8000)
    item = ds[0]
    assert item["rate"] == 16000 and len(item["mix"]) == 20000 and item["mix"].dtype == np.int16
    assert ds.frame_counts() == [1 + 10000 // 128]
    pcm = ds.collator([item])["pcm"]
    assert pcm["rate"] == [16000] and pcm["target_rate"] == 8000 and pcm["lens"] == [20000]


def test_argument_errors_are_reported_not_thrown():
    from sepkern import _lib
    lib = _lib.load()
    one = C.c_void_p(256)            # any non-NULL address: every check below fails before a pointer is used
    err = lambda: lib.sk_last_error().decode()      # noqa: E731

    def call(L=1, M=2, ntaps=257, src=one, taps=one, out=one, nsig=1):
        return lib.sk_resample(src, 1, one, one, nsig, taps, L, M, ntaps, out, one, one, 1000, None)

    assert call(L=2, M=2, ntaps=129) == -1 and "sk_resample" in err() and "L == M" in err()
    assert call(L=0) == -1 and "sk_resample" in err()
    assert call(M=0) == -1 and "sk_resample" in err()
    assert call(L=2, M=4, ntaps=257) == -1 and "lowest terms" in err()
    assert call(ntaps=256) == -1 and "ntaps" in err()
    assert call(L=80, M=441, ntaps=707) == -1 and "ntaps" in err()
    for kw in ({"src": None}, {"taps": None}, {"out": None}):
        assert call(**kw) == -1 and "null pointer" in err()
    assert call(nsig=0) == -1
    assert call(L=1, M=200, ntaps=25601) == -1 and "LDS" in err()
