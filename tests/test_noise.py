"""Noisy dynamic mixing on the host: the fp64 definitions of sepkern/noise.py (identity, factors, the coherence of the generated
field), the float32 restatement of sk_diffuse_noise inside its unit -- and, with ONE fault switched on, far outside it --,
add_noise, the noise draws, the collator's 'noise' block, the driver's options and the entry points' refusals.  Run with -s for
the measured figures."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import PKG
import _noise_cases as nc
import _reverb_cases as rc

sys.path.insert(0, os.path.join(PKG, "archs"))
sys.path.insert(0, os.path.join(PKG, "steps"))

from sepkern import mixing, noise      # noqa: E402


# ------------------------------------------------------------------------------------------------ 1: identity and edges
@pytest.mark.parametrize("n", [1, 127, 128, 129, 511, 512, 513, 1663, 1664, 1665])
def test_identity_factors_return_the_input(n):
    """Every sample is covered by exactly four frames whose squared windows sum to 1.5: to 32 fp64 roundings of the largest sample."""
    x = np.random.default_rng(n).standard_normal((3, n))
    eye = np.broadcast_to(np.eye(3), (257, 3, 3))
    assert noise.num_frames(n) == -(-n // 128) + 3
    assert np.abs(noise.diffuse(x, eye) - x).max() <= 32 * 2.0 ** -53 * np.abs(x).max()
    w = noise.window()
    assert np.allclose(sum(w[128 * d:128 * d + 128] ** 2 for d in range(4)), noise.OLA, rtol=0, atol=1e-15)


# ------------------------------------------------------------------------------------------------ 2: factors
@pytest.mark.parametrize("name", sorted(nc.TIGHT))
def test_factors_of_the_tight_arrays(name):
    mics, rate = nc.TIGHT[name]
    G, L = noise.coherence(mics, rate), noise.factors(mics, rate)
    C_ = len(mics)
    A = (1.0 - noise.EPS) * G + noise.EPS * np.eye(C_)
    assert np.abs(L @ np.transpose(L, (0, 2, 1)) - A).max() <= 1e-12 and np.all(np.triu(L, 1) == 0.0)
    pivots = L[:, range(C_), range(C_)]
    print("%s: smallest pivot %.2e" % (name, pivots.min()))
    assert pivots.min() >= 1e-3
    assert np.all(G[0] == 1.0) and np.abs(L[0, :, 0] - 1.0).max() < 1e-6 and np.abs(L[0, 1:, 1:]).max() < 2e-3
    # float32 factors give the coherence back: the loading (2^-20) and a row of at most 8 products rounded at 2^-24
    L32 = L.astype(np.float32).astype(np.float64)
    back = np.abs(L32 @ np.transpose(L32, (0, 2, 1)) - G).max()
    print("%s: float32 factors reproduce Gamma to %.2e" % (name, back))
    assert back <= 2.0 ** -20 + 8 * 2.0 ** -24
    assert np.array_equal(noise.untri(noise.tri(L), C_), L)


def test_coherence_is_sinc_and_close_microphones_are_refused():
    G = noise.coherence(nc.line(2, 0.1), 8000)
    f = np.arange(257) * 8000 / 512
    x = 2 * f * 0.1 / 343.0
    assert np.allclose(G[1:, 0, 1], np.sin(np.pi * x[1:]) / (np.pi * x[1:]), rtol=0, atol=1e-15) and G[0, 0, 1] == 1.0
    for bad in (nc.line(2, 0.005), nc.line(9, 0.05), nc.line(1, 0.05)):
        with pytest.raises(ValueError):
            noise.factors(bad, 8000)


# ------------------------------------------------------------------------------------------------ 3: the generated field
# Measured (profiles/noise_mix.txt): the fp64 definition on the 4-microphone 5 cm line, 40 000 samples of white input, seeds
# [1234, 0..7]: the Welch estimate's band-averaged error (16-bin bands) against sinc is at worst 0.0595; single bins reach 0.205.
COH_WORST_OF_8 = 0.0595


@pytest.mark.parametrize("f32", [False, True])
def test_the_field_has_the_diffuse_coherence(f32):
    """A ninth seed, within 1.5 x the worst of the eight (the factor is for the seed spread); the white input itself is 1.0 away."""
    x = np.random.default_rng([1234, 8]).standard_normal((4, nc.COH_N)) * 0.1
    L = noise.factors(nc.COH_MICS, nc.RATE)
    y = noise.diffuse_f32(x.astype(np.float32), L) if f32 else noise.diffuse(x, L)
    band, single = nc.coherence_error(y)
    print("%s: band-averaged %.4f (allowed %.4f), single bin %.3f" % ("float32" if f32 else "fp64", band, 1.5 * COH_WORST_OF_8, single))
    assert band <= 1.5 * COH_WORST_OF_8
    assert nc.coherence_error(x)[0] > 0.9


# ------------------------------------------------------------------------------------------------ 4: the float32 restatement
# which case catches which fault: any length catches a shifted grid, transposed factors and the missing 1/1.5; the last frame
# carries weight only where the last hop is (nearly) full -- 1 664 --; the last halo frame of a tile reaches its hop 12, samples
# 1 536 on -- 1 663
FAULTS = {"shift_grid": 513, "drop_last_frame": 1664, "transpose_L": 513, "no_scale": 129, "drop_halo": 1663}


@pytest.mark.parametrize("C_", [2, 8])
def test_the_float32_restatement_stays_within_its_unit_and_one_fault_is_100_units_outside(C_):
    """Unit: 2^-24 sum_j max |x_j| (tests/_noise_cases.py gate).  The restatement stays within 4 units at every length of the GPU
    batch, int16 and float; each fault, in the case named above, is at least 100 units away."""
    worst = 0.0
    for u, n in enumerate(nc.LENGTHS):
        for pcm in (False, True):
            x, Lt, want, e32 = nc.batch_case(C_, u, pcm)
            unit = nc.gate(x, 0.0) / 2.0
            worst = max(worst, e32 / unit)
    print("C=%d: the restatement's error is at most %.2f units" % (C_, worst))
    assert worst <= 4.0
    for fault, n in FAULTS.items():
        u = nc.LENGTHS.index(n)
        x, Lt, want, e32 = nc.batch_case(C_, u, False)
        unit = nc.gate(x, 0.0) / 2.0
        off = float(np.abs(noise.diffuse_f32(x, noise.untri(Lt, C_), **{fault: True}) - want).max())
        print("C=%d %s at n=%d: %.0f units" % (C_, fault, n, off / unit))
        assert off >= 100.0 * unit, fault
    # int16 samples are their float32 copies
    x, Lt, _, _ = nc.batch_case(C_, 4, True)
    Lf = noise.untri(Lt, C_)
    assert np.array_equal(noise.diffuse_f32(x, Lf), noise.diffuse_f32(x.astype(np.float32) * np.float32(1.0 / 32768.0), Lf))


# ------------------------------------------------------------------------------------------------ 5: add_noise
def test_add_noise_reaches_the_requested_snr_and_handles_silence_and_clipping():
    rng = np.random.default_rng(3)
    y = [rng.standard_normal(5000) * 0.1, rng.standard_normal(5000) * 0.2]
    v = [rng.standard_normal(5000) * 0.03, rng.standard_normal(5000) * 0.5]
    for snr in (-3.0, 0.0, 6.0):
        out, a = noise.add_noise(y, v, noise.snr_to_amp(snr))
        got = 10.0 * np.log10(np.mean(y[0] ** 2) / np.mean((out[0] - y[0]) ** 2))
        assert abs(got - snr) < 1e-5 and a > 0.0                             # (amp and a are float32)
        assert np.allclose(out[1] - y[1], a * v[1], rtol=0, atol=1e-15)        # one gain for all channels
    assert noise.add_noise(y, [np.zeros(5000), v[1]], 1.0)[1] == 0.0
    assert noise.add_noise([np.full(5000, 2.0 ** -21), y[1]], v, 1.0)[1] == 0.0          # mean square 2^-42 < 2^-40
    out, a = noise.add_noise(y, v, 1.0, quantized=False)
    assert all(np.array_equal(o, q) for o, q in zip(noise.add_noise(y, [np.zeros(5000)] * 2, 1.0)[0], y))
    loud, _ = noise.add_noise([np.array([0.9, -0.9, 0.1])], [np.array([1.0, -1.0, 0.0])], 1.0, quantized=True)
    assert loud[0][0] == 32767.0 / 32768.0 and loud[0][1] == -1.0
    pcm, _ = noise.add_noise([np.array([3000, -20, 7], dtype=np.int16)], [np.array([100, 50, -3], dtype=np.int16)], 0.5, quantized=True)
    assert np.array_equal(pcm[0] * 32768.0, np.rint(pcm[0] * 32768.0))
    assert noise.snr_to_amp(20.0) == np.float32(0.1) and noise.SILENT == mixing.SILENT
    for bad in (([y[0]], v), ([y[0][:10]], [v[0]]), ([], [])):
        with pytest.raises(ValueError):
            noise.add_noise(bad[0], bad[1], 1.0)


# ------------------------------------------------------------------------------------------------ 6: draws and collator
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return rc.corpus(str(tmp_path_factory.mktemp("noisy")))


@pytest.fixture(scope="module")
def scp(tmp_path_factory):
    """Three recordings: one long, one shorter than any mixture (it wraps around), one in between."""
    return nc.noise_scp(str(tmp_path_factory.mktemp("noise")), [60000, 700, 9000])


def _array3():
    return np.array([[0.0, 0.0, 0.0], [0.05, 0.0, 0.0], [0.0, 0.08, 0.0]])


def test_items_with_noise_carry_what_plain_items_carry_bit_for_bit(data, scp):
    import scipy.io.wavfile
    import uPIT
    plain = uPIT.DynMixTrainSet(data, 2, seed=5, peak=(0.5, 0.9))
    ds = uPIT.DynMixTrainSet(data, 2, seed=5, peak=(0.5, 0.9), noise_scp=scp, noise_snr_db=(-3.0, 6.0))
    wrapped = 0
    for i in range(12):
        it, dry = ds[i], plain[i]
        assert sorted(it) == sorted(list(dry) + ["noise1", "noise_amp"]) and all(np.array_equal(it[k], dry[k]) for k in dry)
        assert ds.draw(i) == plain.draw(i)
        rng = np.random.default_rng([5, i, 3])                                  # the draws, from that generator alone
        snr = float(rng.uniform(-3.0, 6.0))
        path, m = ds.noises[int(rng.integers(len(ds.noises)))]
        st = int(rng.integers(m))
        assert ds.draw_noise(i) == (snr, [(path, st, m)]) and it["noise_amp"] == float(noise.snr_to_amp(snr))
        n = len(it["source1"])
        v = scipy.io.wavfile.read(path)[1]
        assert it["noise1"].dtype == np.int16 and np.array_equal(it["noise1"], v[(st + np.arange(n)) % m])
        wrapped += st + n > m
    assert wrapped >= 2
    # an array in a simulated room: one crop per microphone that travels, and the room is what it is without noise
    kw = dict(room_t60=(0.1, 0.3), array=_array3(), ipd_channels=(1, 2))
    arr, quiet = uPIT.DynMixTrainSet(data, 2, seed=5, noise_scp=scp, **kw), uPIT.DynMixTrainSet(data, 2, seed=5, **kw)
    it, dry = arr[3], quiet[3]
    assert sorted(it) == sorted(list(dry) + ["noise1", "noise2", "noise3", "noise_amp"]) and len(arr.draw_noise(3)[1]) == 3
    assert all(np.array_equal(it["room"][k], dry["room"][k]) for k in dry["room"])
    assert uPIT.DynMixTrainSet(data, 2, seed=5, noise_scp=scp, room_t60=(0.1, 0.3)).noise_channels() == 1
    # resampling: the crop is as long as the mixture at the working rate
    half = uPIT.DynMixTrainSet(data, 2, seed=5, sample_rate=4000, noise_scp=nc.noise_scp(os.path.dirname(scp) + "/r4", [5000], rate=4000))
    from sepkern.resample import out_len
    assert len(half[0]["noise1"]) == out_len(len(half[0]["source1"]), 8000, 4000)
    with pytest.raises(ValueError, match="noise recording.*8000 Hz.*4000 Hz"):
        uPIT.DynMixTrainSet(data, 2, sample_rate=4000, noise_scp=scp)
    with pytest.raises(ValueError, match="noise_snr_db"):
        uPIT.DynMixTrainSet(data, 2, noise_scp=scp, noise_snr_db=(6.0, -3.0))


def test_the_collators_noise_block_follows_the_batch_order_and_mixed_batches_are_refused(data, scp):
    import uPIT
    kw = dict(room_t60=(0.1, 0.3), array=_array3(), ipd_channels=(1, 2))
    ds, plain = uPIT.DynMixTrainSet(data, 2, seed=5, noise_scp=scp, **kw), uPIT.DynMixTrainSet(data, 2, seed=5, **kw)
    items = [ds[i] for i in range(5)]
    pcm = ds.collator(items)["pcm"]
    dry = plain.collator([plain[i] for i in range(5)])["pcm"]
    assert "noise" not in dry and sorted(pcm) == sorted(list(dry) + ["noise"])
    assert torch.equal(pcm["flat"], dry["flat"]) and all(pcm[k] == dry[k] for k in ("lens", "mixing", "keys"))
    order = np.argsort(np.array([1 + len(d["source1"]) // 128 for d in items]))[::-1]
    nz = pcm["noise"]
    assert sorted(nz) == ["amp", "flat", "lens"] and nz["lens"] == pcm["lens"] and nz["flat"].dtype == torch.int16
    assert nz["amp"] == [items[i]["noise_amp"] for i in order]
    want = np.concatenate([items[i]["noise%d" % (c + 1)] for c in range(3) for i in order])
    assert np.array_equal(nz["flat"].numpy(), want)
    with pytest.raises(ValueError, match="every item of its batch"):
        ds.collator([items[0], plain[1]])
    with pytest.raises(ValueError, match="every item of its batch"):
        ds.collator([items[0], {k: v for k, v in items[1].items() if k != "noise3"}])


# ------------------------------------------------------------------------------------------------ 7: the driver's options
def _conf(tmp_path, text):
    path = os.path.join(str(tmp_path), "conf%d" % abs(hash(text)))
    open(path, "w").write(text)
    return path


def test_train_qsub_noise_options_are_refused_before_anything_is_mixed(data, scp, tmp_path, monkeypatch):
    import train_qsub
    import uPIT
    base = ["uPIT", "0", data, "out"]
    for opt in (["--mix-noise-scp", scp], ["--mix-noise-snr", "0,5"]):
        with pytest.raises(SystemExit, match=opt[0] + ".*needs.*--dynamic-mix"):
            train_qsub.get_args(base + ["--wav-input"] + opt)
    dyn = base + ["--wav-input", "--dynamic-mix", "--seed", "3", "--prefetch", "0", "--num-workers", "0", "--batch-size", "3",
                  "--mixes-per-epoch", "6"]
    with pytest.raises(SystemExit, match="--mix-noise-snr.*needs.*--mix-noise-scp"):
        train_qsub.get_args(dyn + ["--mix-noise-snr", "0,5"])
    for bad in ("5,0", "5", "a,b"):
        with pytest.raises(SystemExit):
            train_qsub.get_args(dyn + ["--mix-noise-scp", scp, "--mix-noise-snr", bad])
    assert train_qsub.noise_options(train_qsub.get_args(dyn)) == {}
    # nothing below may read a file of the corpus
    monkeypatch.setattr(uPIT.DynMixTrainSet, "__getitem__", lambda self, idx: pytest.fail("an item was read"))
    mixit = _conf(tmp_path, "num_spk=2\nhidden_dim=64\nloss=mixit\n")
    with pytest.raises(SystemExit, match="--mix-noise-scp.*loss=mixit.*no longer the sum"):
        train_qsub.noisy_mixing(uPIT, train_qsub.get_args(dyn + ["--mix-noise-scp", scp, "--model-config", mixit]))
    mse = _conf(tmp_path, "num_spk=2\nhidden_dim=64\n")
    args = train_qsub.get_args(dyn + ["--mix-noise-scp", scp, "--mix-noise-snr", "0,5", "--model-config", mse])
    assert train_qsub.noisy_mixing(uPIT, args) and not train_qsub.noisy_mixing(uPIT, train_qsub.get_args(dyn + ["--model-config", mixit]))
    other = nc.noise_scp(os.path.join(str(tmp_path), "n16"), [4000], rate=16000)
    bad = train_qsub.get_args(dyn + ["--mix-noise-scp", other, "--model-config", mse])
    bad.ipd = {}
    with pytest.raises(SystemExit, match="--mix-noise-scp.*16000 Hz.*8000 Hz"):
        train_qsub.training_batches(uPIT, bad, 0, 1)
    args.ipd = {}
    ds = train_qsub.training_batches(uPIT, args, 0, 1)[0].dataset
    assert ds.noise_snr_db == (0.0, 5.0) and len(ds.noises) == 3
    plain = train_qsub.training_batches(uPIT, train_qsub.get_args(dyn + ["--model-config", mse]), 0, 1)[0].dataset
    assert plain.noises is None and plain.noise_snr_db == (-3.0, 6.0)


def test_the_entry_points_refuse_bad_arguments_before_they_touch_a_device():
    from sepkern import _lib
    nc.check_refusals(_lib.load())
