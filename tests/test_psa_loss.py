"""The phase-sensitive uPIT losses (loss=psa / tpsa) without a device: the numpy restatement of the targets (sepkern/psa.py),
the conf key, the driver's early exit and the prefetcher's opt-in.  CPU only."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import PKG

sys.path.insert(0, os.path.join(PKG, "archs"))


def _spectra(S, seed, shape=(257, 40)):
    rng = np.random.default_rng(seed)
    srcs = [(rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * (0.1 + s) for s in range(S)]
    return sum(srcs), srcs


def _mag(Y):
    """|Y| as sepkern/psa.py forms it (np.abs goes through hypot, an ulp away here and there)."""
    return np.sqrt(Y.real * Y.real + Y.imag * Y.imag)


# ------------------------------------------------------------------------------------------------ 1: the targets
@pytest.mark.parametrize("S", [2, 3])
def test_psa_targets_properties(S):
    from sepkern import psa
    Y, srcs = _spectra(S, 10 + S)
    mag = _mag(Y)
    t = psa.psa_targets(Y, srcs)
    tc = psa.psa_targets(Y, srcs, clamp=True)
    assert len(t) == len(tc) == S and all(x.dtype == np.float64 and x.shape == Y.shape for x in t + tc)
    # linear in the source: the targets of sources that add up to the mixture add up to |Y|
    assert np.abs(sum(t) - mag).max() <= 1e-12 * mag.max()
    for s in range(S):
        # never more than the source itself
        assert np.all(np.abs(t[s]) <= np.abs(srcs[s]) * (1 + 1e-12))
        # |S| cos(theta_S - theta_Y)
        np.testing.assert_allclose(t[s], np.abs(srcs[s]) * np.cos(np.angle(srcs[s]) - np.angle(Y)), rtol=0, atol=1e-12 * mag.max())
        # the truncated form
        assert np.all(tc[s] >= 0.0) and np.all(tc[s] <= mag)
        assert np.array_equal(tc[s], np.clip(t[s], 0.0, mag))
    assert any((x < 0).any() for x in t)                  # (the plain form does go negative on such spectra)


def test_psa_targets_closed_cases():
    from sepkern import psa
    Y, _ = _spectra(2, 3)
    mag = _mag(Y)
    for c in (0.0, 0.25, 1.0, 3.0):
        for clamp in (False, True):
            got = psa.psa_targets(Y, [c * Y], clamp=clamp)[0]
            want = min(c, 1.0) * mag if clamp else c * mag
            assert np.abs(got - want).max() <= 1e-12 * mag.max()
    assert np.abs(psa.psa_targets(Y, [1j * Y])[0]).max() <= 1e-12 * mag.max()          # in quadrature: nothing along the mixture
    assert np.abs(psa.psa_targets(Y, [-Y])[0] + mag).max() <= 1e-12 * mag.max()
    assert not psa.psa_targets(Y, [-Y], clamp=True)[0].any()


def test_psa_targets_of_a_silent_mixture():
    from sepkern import psa
    Y = np.zeros((257, 3), dtype=np.complex128)
    Y[5, 1] = 1e-16 + 1e-16j                       # |Y|^2 = 2e-32 < 2^-100 = 7.9e-31: counts as silent
    Y[6, 1] = 1e-15                                # |Y|^2 = 1e-30: does not
    S = np.ones_like(Y) * (1.0 - 2.0j)
    with np.errstate(all="raise"):
        for clamp in (False, True):
            t = psa.psa_targets(Y, [S], clamp=clamp)[0]
            assert np.all(np.isfinite(t))
            assert t[6, 1] == (1e-15 if clamp else 1.0) and not np.delete(t.ravel(), 6 * 3 + 1).any()
        m = psa.ideal_psm(Y, S)
    assert np.all(np.isfinite(m)) and m[6, 1] == 1.0 and m.sum() == 1.0


# ------------------------------------------------------------------------------------------------ 2: the ideal mask
def test_ideal_psm():
    from sepkern import psa
    Y, srcs = _spectra(3, 7)
    mag = _mag(Y)
    for Ss in srcs:
        m = psa.ideal_psm(Y, Ss)
        assert m.dtype == np.float64 and np.all(m >= 0.0) and np.all(m <= 1.0)
        np.testing.assert_allclose(m, np.clip(psa.psa_targets(Y, [Ss])[0] / mag, 0.0, 1.0), rtol=0, atol=1e-12)
        np.testing.assert_allclose(m * mag, psa.psa_targets(Y, [Ss], clamp=True)[0], rtol=0, atol=1e-12 * mag.max())


# ------------------------------------------------------------------------------------------------ 3: the conf key
def test_loss_conf_key():
    import uPIT
    assert uPIT.LOSSES == ("mse", "sisdr", "psa", "tpsa")
    assert uPIT.parse_loss("psa") == "psa" and uPIT.parse_loss("tpsa") == "tpsa" and uPIT.parse_loss(" TPSA\n") == "tpsa"
    with pytest.raises(ValueError) as e:
        uPIT.parse_loss("sdr")
    assert "'mse' / 'sisdr' / 'psa' / 'tpsa'" in str(e.value)
    assert uPIT.NEEDS_WAVEFORMS == "`loss=sisdr` needs waveforms: train with `--wav-input`"
    assert uPIT.needs_waveforms("tpsa") == "`loss=tpsa` needs waveforms: train with `--wav-input`"


# ------------------------------------------------------------------------------------------------ 4: the driver
def test_driver_routes_the_phase_sensitive_losses(tmp_path):
    sys.path.insert(0, os.path.join(PKG, "steps"))
    import train_qsub
    import uPIT
    conf = tmp_path / "model.conf"
    base = ["uPIT", "0", str(tmp_path / "data"), str(tmp_path / "exp"), "--model-config", str(conf)]
    for kind in ("psa", "tpsa"):
        conf.write_text("num_spk=2\nloss=%s\n" % kind)
        with pytest.raises(SystemExit) as e:
            train_qsub.prefetch_targets(uPIT, train_qsub.get_args(base))
        assert "--wav-input" in str(e.value) and "loss=" + kind in str(e.value)
        args = train_qsub.get_args(base + ["--wav-input"])
        assert train_qsub.prefetch_targets(uPIT, args) == kind
        assert train_qsub.waveform_loss(uPIT, args) is False               # the waveforms are not kept for the loss
        assert train_qsub.waveform_loss(uPIT, train_qsub.get_args(base)) is False
    for text in ("num_spk=2\n", "loss=mse\n", "loss=sisdr\n"):
        conf.write_text(text)
        assert train_qsub.prefetch_targets(uPIT, train_qsub.get_args(base + ["--wav-input"])) is None
    conf.write_text("loss=mse\n")
    assert train_qsub.prefetch_targets(uPIT, train_qsub.get_args(base)) is None
    conf.write_text("loss=l1\n")
    with pytest.raises(ValueError):
        train_qsub.prefetch_targets(uPIT, train_qsub.get_args(base))

    class NoLosses:                 # an arch without the conf key (archs/RSH.py)
        pass
    assert train_qsub.prefetch_targets(NoLosses, train_qsub.get_args(base)) is None


def test_driver_hands_the_targets_to_the_prefetcher(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(PKG, "steps"))
    import train_qsub
    import sepkern.data
    seen = {}

    class Spy:
        def __init__(self, loader, device, **kw):
            seen.update(kw)
    monkeypatch.setattr(sepkern.data, "Prefetcher", Spy)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    args = train_qsub.get_args(["uPIT", "0", str(tmp_path), str(tmp_path)])
    args.keep_wave, args.prefetch_targets = False, "tpsa"
    train_qsub.staged([], args)
    assert seen["targets"] == "tpsa" and seen["keep_wave"] is False
    args.prefetch = 0
    assert train_qsub.staged([1], args) == [1]


def test_prefetcher_targets_without_a_device():
    from sepkern.data import Prefetcher
    from torch.nn.utils.rnn import pack_sequence
    assert Prefetcher([], "cpu").targets is None and Prefetcher([], "cpu", targets="tpsa").targets == "tpsa"
    with pytest.raises(ValueError, match="'psa' or 'tpsa'"):
        Prefetcher([], "cpu", targets="mse")
    with pytest.raises(ValueError, match="one of them"):
        Prefetcher([], "cpu", keep_wave=True, targets="psa")
    npz = {"mix": pack_sequence([torch.zeros(4, 257), torch.zeros(3, 257)]), "name": ["a", "b"]}
    with pytest.raises(ValueError, match="needs PCM batches"):
        Prefetcher.stage(npz, "cpu", targets="psa")
    assert Prefetcher.stage([1, 2], "cpu", targets="psa") == [1, 2]


def test_ops_refuse_cpu_tensors_and_bad_descriptions():
    from sepkern import _lib, ops
    with pytest.raises(_lib.SepkernError, match="no CPU path"):
        ops.stft_psa(torch.zeros(3000), [[0], [1000], [2000]], [1000], 2)
    lib = _lib.load()
    import ctypes as C
    one = C.c_void_p(256)            # any non-NULL address: every check below fails before a pointer is used

    def call(S=2, n_fft=512, ld=257, offs=one, base=None, nmin=1000, ws=one):
        return lib.sk_stft_psa(one, 1, one, one, 2, S, n_fft, 128, 0, offs, base, one, one, ld, 0, ws, nmin, 10, None)
    err = lambda: lib.sk_last_error().decode()      # noqa: E731
    for S in (0, 5):
        assert call(S=S) == -1 and "sk_stft_psa" in err() and "outside 1..4" in err()
    assert call(nmin=256) == -1 and "reflect" in err()
    assert call(ld=256) == -1 and "F = 257" in err()
    assert call(n_fft=1024) == -1 and "n_fft=512" in err()
    assert call(ws=None) == -1 and "null pointer" in err()
    assert call(offs=None) == -1 and call(base=one) == -1 and "one of them" in err()
