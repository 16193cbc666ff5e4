"""Inter-channel phase features on the host: the definition (sepkern/ipd.py) on known answers, the conf keys, the loader's
array batches (archs/uPIT.py WavTrainSet / WavCollator) and every start-up refusal.  No GPU."""
import argparse
import os
import sys

import numpy as np
import pytest

from conftest import PKG
from oracle import stft as OS

sys.path.insert(0, os.path.join(PKG, "archs"))
sys.path.insert(0, os.path.join(PKG, "steps"))

F = 257


# ------------------------------------------------------------------------------------------------ the definition
def _tone(n, k0, phase, amp=0.25):
    return (amp * np.cos(2.0 * np.pi * k0 * np.arange(n) / 512.0 + phase)).astype(np.float32)


@pytest.mark.parametrize("phi", [0.0, 0.7, -2.0, np.pi / 2, 3.0])
def test_a_tone_at_a_bin_centre_gives_cos_and_sin_of_its_phase_offset(phi):
    """x_r = cos(w n + 0.3), x_c = cos(w n + 0.3 + phi) at bin 40: the periodic Hann window's image of the negative frequency is
    exactly zero there, so on frames that do not touch the reflect padding (2 .. T-3) the features are (cos phi, sin phi) up to
    the float32 samples and the complex64 spectra of oracle/stft.py (1e-7 relative each; gate 1e-5)."""
    from sepkern import ipd
    n, k0 = 4096, 40
    Yr, Yc = OS.stft(_tone(n, k0, 0.3)), OS.stft(_tone(n, k0, 0.3 + phi))
    c, s = ipd.ipd(Yc, Yr)
    inner = slice(2, Yr.shape[1] - 2)
    assert np.abs(c[k0, inner] - np.cos(phi)).max() < 1e-5 and np.abs(s[k0, inner] - np.sin(phi)).max() < 1e-5


def _noise_spectra(seed, C=3, n=3000):
    rng = np.random.default_rng(seed)
    return np.stack([OS.stft(rng.standard_normal(n).astype(np.float32) * 0.1).T for _ in range(C)]).astype(np.complex128)


def test_gain_invariance_symmetry_and_unit_modulus():
    from sepkern import ipd
    Y = _noise_spectra(1)
    c, s = ipd.ipd(Y[1], Y[0])
    assert np.abs(c * c + s * s - 1.0).max() < 1e-12
    for gc, gr in ((3.0, 1.0), (1.0, 0.125), (1e-3, 7.0)):
        c2, s2 = ipd.ipd(gc * Y[1], gr * Y[0])
        assert np.abs(c2 - c).max() < 1e-12 and np.abs(s2 - s).max() < 1e-12
    cr, sr = ipd.ipd(Y[0], Y[1])
    assert np.array_equal(cr, c) and np.array_equal(sr, -s)
    c0, s0 = ipd.ipd(Y[0], Y[0])
    assert np.abs(c0 - 1.0).max() < 1e-12 and not s0.any()


def test_a_zero_channel_and_a_tiny_bin_give_zeros():
    from sepkern import ipd
    Y = _noise_spectra(2)
    for a, b in ((np.zeros_like(Y[1]), Y[0]), (Y[1], np.zeros_like(Y[0]))):
        c, s = ipd.ipd(a, b)
        assert not c.any() and not s.any()
    # the threshold is on the squared magnitude: 2^-51 squared is below 2^-100, 2^-49 squared above
    c, s = ipd.ipd(np.array([2.0 ** -51, 2.0 ** -49, 1.0]), np.array([1.0, 1.0, 2.0 ** -51 * 1j]))
    assert c.tolist() == [0.0, 1.0, 0.0] and s.tolist() == [0.0, 0.0, 0.0]


def test_feature_rows_layout():
    from sepkern import ipd
    Y = _noise_spectra(3, C=4)
    rows = ipd.feature_rows(Y, 1, [3, 0])
    assert rows.shape == (Y.shape[1], ipd.in_dim(2)) == (Y.shape[1], 1285)
    assert np.array_equal(rows[:, :F], np.abs(Y[1]))
    for p, ch in enumerate([3, 0]):
        (c0, c1), (s0, s1) = ipd.columns(p)
        c, s = ipd.ipd(Y[ch], Y[1])
        assert np.array_equal(rows[:, c0:c1], c) and np.array_equal(rows[:, s0:s1], s)
    with pytest.raises(ValueError, match="hold 4 channels"):
        ipd.feature_rows(Y, 0, [4])


def test_the_gpu_tests_signals_keep_the_end_to_end_tolerance_meaningful():
    """tests/test_gpu_ipd.py compares the kernel with this module on oracle spectra under 4 e (1/|Y_c| + 1/|Y_r|), e the existing
    STFT kernel's own error, and asserts that this exceeds 0.1 on fewer than 1 % of the elements.  Here, without a GPU: for the
    shared signals that holds up to e = 1e-4, thirty times what an fp32 FFT of these levels (|Y| < 64: a few 2^-24 x 64 = 4e-6)
    gives; and the oracle's own rounding -- it returns complex64, 2^-24 relative per part, so at most 2^-22 on a cos or sin --
    is below the tolerance at that e = 4e-6 wherever |Y| < 64 (4 x 4e-6 x 2 / 64 = 5e-7 > 2^-22 = 2.4e-7)."""
    import _ipd_cases as cases
    share = cases.tolerance_share(1e-4)
    print("share of elements whose end-to-end tolerance exceeds 0.1 at e = 1e-4: %.3g; at 4e-6: %.3g" % (share, cases.tolerance_share(4e-6)))
    assert share < cases.MAX_SHARE, share
    assert max(np.abs(sp).max() for sp in cases.case()["spec"]) < 64.0


# ------------------------------------------------------------------------------------------------ conf keys, widths, columns
def test_conf_parsing_and_its_errors():
    from sepkern import ipd
    assert ipd.parse_channels(None) == () and ipd.parse_channels("") == () and ipd.parse_channels(" ") == ()
    assert ipd.parse_channels("1,2,3") == (1, 2, 3) and ipd.parse_channels(" 3 , 1 ") == (3, 1) and ipd.parse_channels([2, 0], ref=1) == (2, 0)
    assert ipd.parse_ref("0") == 0 and ipd.parse_ref(" 2 ") == 2 and ipd.parse_ref(1) == 1
    for bad, text in (("1,,2", "empty entry"), ("1,x", "not a list of channel numbers"), ("1,1", "listed twice"), ("-1", "negative"),
                      ("0,1", "lists the reference channel"), ("1,2,3,4,5,6,7,8", "at most 7")):
        with pytest.raises(ValueError, match=text):
            ipd.parse_channels(bad, ref=0)
    with pytest.raises(ValueError, match="lists the reference channel ipd_ref = 2"):
        ipd.parse_channels("1,2", ref=2)
    for bad in ("x", "-1"):
        with pytest.raises(ValueError, match="ipd_ref"):
            ipd.parse_ref(bad)


def test_widths_and_column_ranges():
    from sepkern import ipd
    assert [ipd.in_dim(P) for P in (1, 2, 3, 7)] == [771, 1285, 1799, 3855]
    assert [ipd.padded_dim(P) for P in (1, 2, 7)] == [784, 1296, 3856]
    for bad in (0, 8):
        with pytest.raises(ValueError):
            ipd.in_dim(bad)
    assert ipd.columns(0) == ((257, 514), (514, 771)) and ipd.columns(1) == ((771, 1028), (1028, 1285))
    assert ipd.columns(6)[1][1] == ipd.in_dim(7)
    with pytest.raises(ValueError):
        ipd.columns(7)
    assert ipd.chan_keys(["mix", "source1", "chan2", "chan0", "channel", "chanx"]) == ["chan2", "chan0"]
    assert ipd.signal_keys(["mix", "source1", "source2", "chan2"]) == ["mix", "source1", "source2"]


# ------------------------------------------------------------------------------------------------ the loader
def _write_array_tree(root, lengths, C, S=2, seed=5, rate=8000, source_channels=None):
    """<root>/wav/{mix,s1,..}/<id>.wav and <root>/data/wav.scp: C-channel mixtures (C = 1: mono files), mono sources unless
    source_channels.  -> (data dir, [per utterance: (mix (n, C) int16, [source (n,) or (n, Cs) int16])])."""
    import scipy.io.wavfile
    rng = np.random.default_rng(seed)
    data = os.path.join(root, "data")
    os.makedirs(data)
    utts = []
    with open(os.path.join(data, "wav.scp"), "w") as scp:
        for u, n in enumerate(lengths):
            mix = rng.integers(-3000, 3000, size=(n, C)).astype(np.int16)
            shape = (n,) if source_channels is None else (n, source_channels)
            srcs = [rng.integers(-3000, 3000, size=shape).astype(np.int16) for _ in range(S)]
            utts.append((mix, srcs))
            for q, x in enumerate([mix[:, 0] if C == 1 else mix] + srcs):
                d = os.path.join(root, "wav", "mix" if q == 0 else "s%d" % q)
                os.makedirs(d, exist_ok=True)
                scipy.io.wavfile.write(os.path.join(d, "utt%02d.wav" % u), rate, x)
            scp.write("utt%02d %s\n" % (u, os.path.join(root, "wav", "mix", "utt%02d.wav" % u)))
    return data, utts


@pytest.mark.parametrize("chans", [(2,), (3, 1), (1, 2, 3)])
def test_the_collators_key_order_and_flat_layout(tmp_path, chans):
    import uPIT
    lengths, ref = [700, 1500, 900], 0
    data, utts = _write_array_tree(str(tmp_path), lengths, C=4)
    ts = uPIT.WavTrainSet(data, ipd_ref=ref, ipd_channels=",".join(str(c) for c in chans))
    item = ts[1]
    assert list(item) == ["mix", "source1", "source2"] + ["chan%d" % c for c in chans]
    pcm = ts.collator([ts[i] for i in range(len(ts))])["pcm"]
    assert pcm["keys"] == ["mix", "source1", "source2"] + ["chan%d" % c for c in chans]
    order = [1, 2, 0]                                  # longest first
    assert pcm["lens"] == [lengths[i] for i in order] and "rate" not in pcm
    want = [utts[i][0][:, ref] for i in order] + [utts[i][1][s] for s in range(2) for i in order] \
        + [utts[i][0][:, c] for c in chans for i in order]
    flat = pcm["flat"].numpy()
    assert flat.dtype == np.int16 and np.array_equal(flat, np.concatenate(want))
    # the mono batch of the reference channel is the head of the array batch
    mono = uPIT.WavCollator()([{k: v for k, v in ts[i].items() if not k.startswith("chan")} for i in range(len(ts))])["pcm"]
    assert mono["keys"] == pcm["keys"][:3] and mono["lens"] == pcm["lens"]
    assert np.array_equal(mono["flat"].numpy(), flat[:3 * sum(lengths)])


def test_another_reference_channel_and_multichannel_sources(tmp_path):
    import uPIT
    data, utts = _write_array_tree(str(tmp_path), [600, 500], C=3, source_channels=3)
    ts = uPIT.WavTrainSet(data, ipd_ref="2", ipd_channels="0")
    item = ts[0]
    assert np.array_equal(item["mix"], utts[0][0][:, 2]) and np.array_equal(item["chan0"], utts[0][0][:, 0])
    assert np.array_equal(item["source1"], utts[0][1][0][:, 2]) and np.array_equal(item["source2"], utts[0][1][1][:, 2])
    assert all(v.flags["C_CONTIGUOUS"] for v in item.values())


def test_a_mono_tree_gives_todays_dict_exactly(tmp_path):
    import uPIT
    lengths = [700, 1500, 900]
    data, utts = _write_array_tree(str(tmp_path), lengths, C=1)
    ts = uPIT.WavTrainSet(data)
    assert ts.ipd_channels == () and list(ts[0]) == ["mix", "source1", "source2"]
    batch = ts.collator([ts[i] for i in range(len(ts))])
    assert list(batch) == ["pcm"] and list(batch["pcm"]) == ["flat", "keys", "lens"]
    pcm = batch["pcm"]
    order = [1, 2, 0]
    assert pcm["keys"] == ["mix", "source1", "source2"] and pcm["lens"] == [lengths[i] for i in order]
    want = [utts[i][0][:, 0] for i in order] + [utts[i][1][s] for s in range(2) for i in order]
    assert np.array_equal(pcm["flat"].numpy(), np.concatenate(want))
    rated = uPIT.WavTrainSet(data, sample_rate=8000)
    assert list(rated[0]) == ["mix", "source1", "source2", "rate"]
    assert list(rated.collator([rated[0], rated[1]])["pcm"]) == ["flat", "keys", "lens", "rate", "target_rate"]


# ------------------------------------------------------------------------------------------------ refusals
def _args(tmp_path, conf, **kw):
    path = os.path.join(str(tmp_path), "model.conf")
    with open(path, "w") as f:
        f.write("".join("%s=%s\n" % kv for kv in conf.items()))
    return argparse.Namespace(model_config=path, wav_input=kw.get("wav_input", True), dynamic_mix=kw.get("dynamic_mix", False),
                              sample_rate=None)


def test_the_driver_refuses_at_start_up(tmp_path):
    import train_qsub
    import uPIT
    ok = _args(tmp_path, {"ipd_channels": "1,2", "ipd_ref": "0", "loss": "psa"})
    assert train_qsub.ipd_model(uPIT, ok) == {"ipd_ref": 0, "ipd_channels": (1, 2)}
    assert train_qsub.ipd_model(uPIT, _args(tmp_path, {"loss": "mse"}, wav_input=False)) == {}
    with pytest.raises(SystemExit, match="`ipd_channels` needs waveforms.*--wav-input"):
        train_qsub.ipd_model(uPIT, _args(tmp_path, {"ipd_channels": "1"}, wav_input=False))
    with pytest.raises(SystemExit, match="`ipd_channels` does not train with `loss=mixit`"):
        train_qsub.ipd_model(uPIT, _args(tmp_path, {"ipd_channels": "1", "loss": "mixit"}))
    with pytest.raises(SystemExit, match="`ipd_channels` does not train with `--dynamic-mix`"):
        train_qsub.ipd_model(uPIT, _args(tmp_path, {"ipd_channels": "1"}, dynamic_mix=True))
    with pytest.raises(SystemExit, match="lists the reference channel"):
        train_qsub.ipd_model(uPIT, _args(tmp_path, {"ipd_channels": "1", "ipd_ref": "1"}))
    for loss in ("mse", "psa", "tpsa", "dpcl", "sisdr"):
        assert train_qsub.ipd_model(uPIT, _args(tmp_path, {"ipd_channels": "3", "loss": loss}))["ipd_channels"] == (3,)


def test_the_data_set_is_checked_against_the_model_when_it_is_built(tmp_path):
    import train_qsub
    import uPIT
    mono, _ = _write_array_tree(os.path.join(str(tmp_path), "mono"), [600], C=1)
    arr, _ = _write_array_tree(os.path.join(str(tmp_path), "arr"), [600], C=3)
    args = _args(tmp_path, {"ipd_channels": "1,2"})
    args.ipd = train_qsub.ipd_model(uPIT, args)
    assert train_qsub.wav_train_set(uPIT, args, arr).ipd_channels == (1, 2)
    with pytest.raises(SystemExit, match="a mono batch cannot feed an IPD model"):
        train_qsub.wav_train_set(uPIT, args, mono)
    args.ipd = train_qsub.ipd_model(uPIT, _args(tmp_path, {"ipd_channels": "1,3"}))
    with pytest.raises(SystemExit, match=r"has 3 channel\(s\).*needs 4"):
        train_qsub.wav_train_set(uPIT, args, arr)
    args.ipd = {}
    assert train_qsub.wav_train_set(uPIT, args, mono).ipd_channels == ()
    with pytest.raises(SystemExit, match="has 3 channels and the model sees one.*ipd_channels"):
        train_qsub.wav_train_set(uPIT, args, arr)


def test_the_model_refuses_mixit_and_npz_features(tmp_path):
    import eval_qsub
    import uPIT
    with pytest.raises(ValueError, match="`ipd_channels` does not train with `loss=mixit`"):
        uPIT.SepDNN(0, ipd_channels="1", loss="mixit", hidden_dim="8", num_layers="1")
    model = uPIT.SepDNN(0, ipd_channels="2,1", hidden_dim="8", num_layers="1")
    assert model.in_dim == 1285 and model.feat_dim == 257 and model.out_dim == 514 and model.ipd_channels == (2, 1) and model.ipd_ref == 0
    assert tuple(model.blstm.weight_ih_l0.shape) == (32, 1285)
    mono = uPIT.SepDNN(0, hidden_dim="8", num_layers="1")
    assert mono.in_dim == 257 and mono.ipd_channels == ()
    args = _args(tmp_path, {"ipd_channels": "1"})
    with pytest.raises(SystemExit, match="separate_wav.py"):
        eval_qsub.refuse_ipd_model(uPIT, args)
    assert eval_qsub.refuse_ipd_model(uPIT, _args(tmp_path, {"loss": "mse"})) is None
    with pytest.raises(ValueError, match="separate_wav.py"):
        uPIT.estimate_masks(model, {"mix": None, "name": []})
    # batches against models: decided from the keys, before anything touches a device
    with pytest.raises(ValueError, match="the batch holds one channel"):
        uPIT._match_channels(model, [])
    with pytest.raises(ValueError, match="the model sees one channel"):
        uPIT._match_channels(mono, ["chan1"])
    with pytest.raises(ValueError, match="ask for chan2, chan1 in that order"):
        uPIT._match_channels(model, ["chan1", "chan2"])
    assert uPIT._match_channels(model, ["chan2", "chan1"]) is None and uPIT._match_channels(mono, []) is None
