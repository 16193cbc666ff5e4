"""The mixture-invariant training loss without a device: the numpy restatement of its arithmetic (sepkern/mixit.py, from the
sums P, c, G) against torch fp64 autograd of the direct definition (tests/_mixit_oracle.py), its closed forms, the structure
of the mask gradient, the argument checks of the new entry points, the conf key and the driver's routes.  CPU only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import PKG
from oracle import stft as OS
import _mixit_oracle as MO

sys.path.insert(0, os.path.join(PKG, "archs"))


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


# ------------------------------------------------------------------------------------------------ 1: against autograd
@pytest.mark.parametrize("L", [256, 4096, 4224, 64000])
@pytest.mark.parametrize("M", [2, 3, 4])
def test_gram_form_matches_fp64_autograd_of_the_direct_definition(M, L):
    """Gates 1e-10 relative on the loss and on the gradient (tests/test_sisdr_loss.py's); the sums' own error is of the order
    of 1e-13 because err / P >= tau keeps the cancellation in err bounded."""
    from sepkern import mixit
    c = MO.noisy_partition(L, M, seed=100 * M + L % 97)
    refs = [OS.pcm16_to_float(x).astype(np.float64) for x in c["refs_pcm"]]
    res = mixit.mixit(c["ests"], refs, count=3.0)
    ests_t = [torch.tensor(e, dtype=torch.float64, requires_grad=True) for e in c["ests"]]
    loss, scores, bests = MO.loss_t([ests_t], [[torch.tensor(x) for x in refs]], mixit.tau_of(), count=3.0)
    loss.backward()
    assert res["best"] == bests[0] == c["code"]
    np.testing.assert_allclose(res["score"], scores[0].numpy(), rtol=1e-10, atol=1e-10)
    want = float(loss.detach())
    err_loss = abs(res["loss"] - want) / abs(want)
    grads = mixit.gradient(c["ests"], refs, res["best"], res["coef"])
    err_grad = _rel(np.concatenate(grads), np.concatenate([e.grad.numpy() for e in ests_t]))
    print("M=%d L=%d: loss %.3g, gradient %.3g relative (gate 1e-10)" % (M, L, err_loss, err_grad))
    assert err_loss <= 1e-10 and err_grad <= 1e-10
    # the same signal for every estimate of a group
    for k in range(M):
        for l in range(M):
            if ((res["best"] >> k) & 1) == ((res["best"] >> l) & 1):
                assert np.array_equal(grads[k], grads[l])
    # the count divides the loss and the coefficients
    res1 = mixit.mixit(c["ests"], refs)
    np.testing.assert_allclose(res["coef"], res1["coef"] / 3.0, rtol=1e-14)
    np.testing.assert_allclose(res["loss"], res1["loss"] / 3.0, rtol=1e-14)


# ------------------------------------------------------------------------------------------------ 2: closed forms
@pytest.mark.parametrize("snr_max", [30.0, 20.0])
def test_exact_partition_scores_snr_max_and_returns_its_code(snr_max):
    from sepkern import mixit
    rng = np.random.default_rng(2)
    for M, code in ((2, 1), (2, 2), (3, 5), (4, 6), (4, 14), (4, 8)):
        srcs = [rng.standard_normal(3000) for _ in range(M)]
        refs = [sum(s for k, s in enumerate(srcs) if ((code >> k) & 1) == n) for n in range(2)]
        res = mixit.mixit(srcs, refs, snr_max=snr_max)
        assert res["best"] == code
        # err is a rounding residue of the order of 1e-16 P against tau P >= 1e-3 P
        assert abs(res["score"][code] - snr_max) < 1e-9 and abs(res["loss"] + snr_max) < 1e-9
        assert np.all(np.isfinite(res["coef"])) and np.all(res["coef"] > 0.0)


def test_all_zero_estimates_score_the_threshold_and_return_code_zero():
    from sepkern import mixit
    rng = np.random.default_rng(3)
    refs = [rng.standard_normal(2000), rng.standard_normal(2000)]
    for M in (2, 3, 4):
        res = mixit.mixit([np.zeros(2000)] * M, refs)
        want = 10.0 * np.log10(1.0 / (1.0 + mixit.tau_of()))
        np.testing.assert_allclose(res["score"], want, rtol=0, atol=1e-12)
        assert res["best"] == 0                                   # every code scores the same: the first maximum
        assert len(res["score"]) == 1 << M


def test_a_silent_reference_gets_no_gradient_and_everything_is_finite():
    from sepkern import mixit
    rng = np.random.default_rng(4)
    x0 = rng.standard_normal(2000)
    ests = [x0 + 0.1 * rng.standard_normal(2000), np.zeros(2000), 0.05 * rng.standard_normal(2000)]
    res = mixit.mixit(ests, [x0, np.zeros(2000)])
    assert np.all(np.isfinite(res["score"])) and np.isfinite(res["loss"])
    # reference 1 is silent and met exactly by the zero estimate (or by an empty group): D_1 = 0
    assert ((res["best"] >> 2) & 1) == 0 and res["coef"][1] == 0.0 and res["coef"][0] > 0.0
    grads = mixit.gradient(ests, [x0, np.zeros(2000)], res["best"], res["coef"])
    assert all(np.all(np.isfinite(g)) for g in grads)
    for k in range(3):
        if (res["best"] >> k) & 1:
            assert not grads[k].any()
    # both silent, all estimates zero: zero coefficients, finite scores
    res = mixit.mixit([np.zeros(100)] * 2, [np.zeros(100)] * 2)
    assert np.all(res["coef"] == 0.0) and np.all(np.isfinite(res["score"])) and res["best"] == 0


def test_estimate_counts_outside_2_to_4_are_refused():
    from sepkern import mixit
    z = np.zeros(10)
    for M in (1, 5):
        with pytest.raises(ValueError, match="2..4"):
            mixit.mixit([z] * M, [z, z])
    with pytest.raises(ValueError):
        mixit.mixit([z, z], [z, z, z])


# ------------------------------------------------------------------------------------------------ 3: the mask gradient
def test_dmask_blocks_of_one_group_are_equal():
    """Through sisdr.istft_adjoint_mask_grad: the gradient signal of a group is one signal, the mixture spectrum is one
    spectrum, so the dmask blocks of the estimates of a group are the same array -- what lets one transform serve them all."""
    from sepkern import mixit, sisdr
    rng = np.random.default_rng(5)
    T, M, code = 21, 4, 0b0110
    L = 128 * (T - 1)
    c = MO.noisy_partition(L, M, seed=5, code=code)
    refs = [OS.pcm16_to_float(x).astype(np.float64) for x in c["refs_pcm"]]
    res = mixit.mixit(c["ests"], refs)
    assert res["best"] == code
    grads = mixit.gradient(c["ests"], refs, res["best"], res["coef"])
    X = OS.stft(rng.standard_normal(L + 100) * 0.1)[:, :T]
    dm = [sisdr.istft_adjoint_mask_grad(X, g) for g in grads]
    assert np.array_equal(dm[1], dm[2]) and np.array_equal(dm[0], dm[3])
    assert not np.array_equal(dm[0], dm[1]) and np.abs(dm[0]).max() > 0


# ------------------------------------------------------------------------------------------------ 4: argument checks
def test_entry_points_check_their_arguments_before_touching_a_device():
    from sepkern import _lib
    lib = _lib.load()
    buf = (C.c_float * 16)()
    one = C.cast(buf, C.c_void_p)

    def err():
        return lib.sk_last_error().decode()

    def fwd(M=2, est=one, ws=one, tau=1e-3):
        return lib.sk_mixit_fwd(est, one, one, 1, one, one, 2, M, 1000, None, tau, one, one, one, one, ws, None)

    def grad(M=2, n_fft=512, ld=514, coef=one):
        return lib.sk_mixit_mask_grad(one, one, one, 1, one, one, one, coef, one, one, one, 2, M, n_fft, 128, 10, one, ld, None)

    for call, name in ((fwd, "sk_mixit_fwd"), (grad, "sk_mixit_mask_grad")):
        for M in (1, 5):
            assert call(M=M) == -1
            assert name in err() and "outside 2..4" in err()
    assert grad(n_fft=1024) == -1 and "n_fft=512" in err()
    assert grad(ld=513) == -1 and "M*F = 514" in err()
    assert grad(M=4, ld=1027) == -1
    assert grad(coef=None) == -1 and "null pointer" in err()
    assert fwd(est=None) == -1 and "null pointer" in err()
    assert fwd(ws=None) == -1 and "null pointer" in err()
    assert fwd(tau=-0.5) == -1 and "tau" in err()
    assert lib.sk_mixit_workspace_bytes(2, 5, 1000) == 0 and lib.sk_mixit_workspace_bytes(2, 1, 1000) == 0
    assert lib.sk_mixit_workspace_bytes(0, 2, 1000) == 0
    assert lib.sk_mixit_workspace_bytes(32, 4, 64000) >= 32 * 16 * 20 * 8


def test_ops_refuse_cpu_tensors():
    from sepkern import _lib, ops
    from sepkern.packing import Packing
    pk = Packing([5, 3], "cpu")
    mixc = torch.zeros(8, 257, dtype=torch.complex64)
    z64, z32 = torch.zeros(4, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(_lib.SepkernError):
        ops.mixit_fwd(torch.zeros(10), z64, torch.zeros(10), z64, z32, 2, 5, 1e-3)
    with pytest.raises(_lib.SepkernError):
        ops.mixit_mask_grad(torch.zeros(10), z64, torch.zeros(10), z64, z32, torch.zeros(2, 2), torch.ones(1), mixc, pk, 2)


# ------------------------------------------------------------------------------------------------ 5: conf key, driver
def test_loss_conf_key():
    import uPIT
    assert uPIT.LOSSES == ("mse", "sisdr", "psa", "tpsa") and uPIT.MIXIT_LOSSES == ("mixit",)
    assert uPIT.parse_loss("mixit") == "mixit" and uPIT.parse_loss(" MixIT\n") == "mixit"
    for old in uPIT.LOSSES:
        assert uPIT.parse_loss(old) == old
    with pytest.raises(ValueError) as e:
        uPIT.parse_loss("sdr")
    assert "'mse' / 'sisdr' / 'psa' / 'tpsa' / 'mixit'" in str(e.value)
    assert uPIT.needs_waveforms("mixit") == "`loss=mixit` needs waveforms: train with `--wav-input`"


def test_driver_routes_mixit(tmp_path):
    sys.path.insert(0, os.path.join(PKG, "steps"))
    import train_qsub
    import uPIT
    conf = tmp_path / "model.conf"
    conf.write_text("num_spk=4\nloss=mixit\n")
    base = ["uPIT", "0", str(tmp_path / "data"), str(tmp_path / "exp"), "--model-config", str(conf)]
    with pytest.raises(SystemExit) as e:
        train_qsub.waveform_loss(uPIT, train_qsub.get_args(base))
    assert "loss=mixit" in str(e.value) and "--wav-input" in str(e.value)
    args = train_qsub.get_args(base + ["--wav-input"])
    assert train_qsub.waveform_loss(uPIT, args) is True and train_qsub.prefetch_targets(uPIT, args) is None
    # two recordings per example whatever num_spk is; every other loss mixes num_spk sources as before
    assert train_qsub.mixed_recordings(uPIT, args) == 2
    conf.write_text("num_spk=3\nloss=sisdr\n")
    assert train_qsub.mixed_recordings(uPIT, args) == 3
    conf.write_text("num_spk=3\n")
    assert train_qsub.mixed_recordings(uPIT, args) == 3 and train_qsub.waveform_loss(uPIT, args) is False
