"""The SI-SDR uPIT training loss without a device: the numpy restatement of its arithmetic (sepkern/sisdr.py) against the
scoring functions and against torch fp64 autograd, the argument checks of the new entry points, the conf key and the
prefetcher's opt-in.  CPU only."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import PKG
from oracle import stft as OS
import _sisdr_oracle as SO

sys.path.insert(0, os.path.join(PKG, "archs"))


# ------------------------------------------------------------------------------------------------ 1: PIT on SI-SDR
@pytest.mark.parametrize("S", [2, 3, 4])
def test_pit_si_sdr_agrees_with_the_scoring_functions(S):
    from sepkern import sisdr
    rng = np.random.default_rng(S)
    refs = [rng.standard_normal(4000) + 0.3 for _ in range(S)]
    order = list(range(1, S)) + [0]
    ests = [refs[order[k]] + 0.3 * rng.standard_normal(4000) - 0.1 for k in range(S)]
    res = sisdr.pit_si_sdr(ests, refs)
    for k in range(S):
        for i in range(S):
            assert abs(res["pair"][k, i] - sisdr.si_sdr(ests[k], refs[i])) < 1e-9
    assert abs(res["perm_score"].max() - sisdr.si_sdr_best_perm(ests, refs)) < 1e-9
    perms = list(itertools.permutations(range(S)))
    assert perms[res["best_perm"]] == tuple(order)
    assert abs(res["loss"] + res["perm_score"][res["best_perm"]]) < 1e-12
    assert np.all(np.isfinite(res["coef"])) and np.all(res["coef"][:, 0] != 0.0)
    # the count divides the loss and the coefficients (data parallel: the global utterance count)
    res4 = sisdr.pit_si_sdr(ests, refs, count=4.0)
    np.testing.assert_allclose(res4["coef"], res["coef"] / 4.0, rtol=1e-14)
    np.testing.assert_allclose(res4["loss"], res["loss"] / 4.0, rtol=1e-14)


def test_pit_si_sdr_first_maximum_on_an_exact_tie():
    from sepkern import sisdr
    rng = np.random.default_rng(0)
    r = rng.standard_normal(2000)
    e0, e1 = rng.standard_normal(2000), rng.standard_normal(2000)
    res = sisdr.pit_si_sdr([e0, e1], [r, r])            # both permutations score the same, bit for bit
    assert res["perm_score"][0] == res["perm_score"][1] and res["best_perm"] == 0
    res = sisdr.pit_si_sdr([e0, e0, e0], [r, r, r])
    assert len(set(res["perm_score"].tolist())) == 1 and res["best_perm"] == 0


def test_pit_si_sdr_silent_reference_and_exact_copy():
    from sepkern import sisdr
    rng = np.random.default_rng(1)
    e, r = rng.standard_normal(3000), rng.standard_normal(3000)
    silent = sisdr.pit_si_sdr([e, r], [np.zeros(3000), r])
    assert np.isfinite(silent["loss"]) and np.all(np.isfinite(silent["pair"])) and np.all(silent["coef"] == 0.0)
    assert abs(silent["pair"][0, 0] - sisdr.si_sdr(e, np.zeros(3000))) < 1e-9
    const = sisdr.pit_si_sdr([e], [np.full(3000, 0.25)])          # a constant reference is silent once its mean is removed
    assert np.isfinite(const["loss"]) and np.all(const["coef"] == 0.0)
    copy = sisdr.pit_si_sdr([r], [r])
    assert np.isfinite(copy["loss"]) and copy["pair"][0, 0] > 200.0 and np.all(copy["coef"] == 0.0)
    ortho = sisdr.pit_si_sdr([np.tile([1.0, -1.0], 8)], [np.tile([1.0, 1.0, -1.0, -1.0], 4)])      # a == 0 exactly
    assert np.isfinite(ortho["loss"]) and np.all(ortho["coef"] == 0.0)


# ------------------------------------------------------------------------------------------------ 2: closed forms vs autograd
def _case(n=5000, S=2, seed=3):
    c = SO.ratio_mask_case([n], S, seed)
    return c["specs"][0], c["masks"][0], c["refs_pcm"][0]


def test_torch_restatement_of_the_istft_matches_the_oracle():
    X, m, _ = _case()
    for s in range(m.shape[0]):
        got = SO.istft_t(torch.as_tensor(X).to(torch.complex128) * torch.as_tensor(m[s]).double()).numpy()
        ref = OS.istft(X * m[s])
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= 3e-6


@pytest.mark.parametrize("S,n", [(2, 5000), (3, 3333)])
def test_closed_form_gradient_matches_fp64_autograd(S, n):
    from sepkern import sisdr
    X, m, refs = _case(n, S, seed=3 + S)
    mt = torch.tensor(m, dtype=torch.float64, requires_grad=True)
    rs = [OS.pcm16_to_float(r).astype(np.float64) for r in refs]
    loss, info = SO.loss_from_masks([X], [mt], [rs])
    loss.backward()
    ests = [e.numpy() for e in info["ests"][0]]
    L = ests[0].shape[0]
    res = sisdr.pit_si_sdr(ests, [r[:L] for r in rs])
    assert res["best_perm"] == info["best"][0] and res["best_perm"] != 0
    assert abs(res["loss"] - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    np.testing.assert_allclose(res["pair"], info["pair"][0].numpy(), rtol=0, atol=1e-9)
    perm = list(itertools.permutations(range(S)))[res["best_perm"]]
    dmask = np.stack([sisdr.istft_adjoint_mask_grad(
        X, res["coef"][k, 0] * ests[k] + res["coef"][k, 1] * rs[perm[k]][:L] + res["coef"][k, 2]) for k in range(S)])
    ref = mt.grad.numpy()
    rel = np.linalg.norm(dmask - ref) / np.linalg.norm(ref)
    print("closed form vs fp64 autograd: relative L2 %.3g" % rel)
    assert np.linalg.norm(ref) > 0 and rel <= 1e-10


# ------------------------------------------------------------------------------------------------ 3: argument errors
def test_argument_errors_are_reported_not_thrown():
    from sepkern import _lib
    lib = _lib.load()
    one = C.c_void_p(256)            # any non-NULL address: every check below fails before a pointer is used
    err = lambda: lib.sk_last_error().decode()      # noqa: E731

    def istft(S=2, n_fft=512, ld=514, mix=one):
        return lib.sk_mask_istft_rows(mix, one, ld, one, one, 2, S, n_fft, 128, one, one, 10, None)

    def fwd(S=2, est=one, ws=one):
        return lib.sk_sisdr_pit_fwd(est, one, one, 1, one, one, 2, S, 1000, None, one, one, one, one, one, ws, None)

    def grad(S=2, n_fft=512, ld=514, coef=one):
        return lib.sk_sisdr_mask_grad(one, one, one, 1, one, one, one, coef, one, one, one, 2, S, n_fft, 128, 10, one, ld, None)

    for call, name in ((istft, "sk_mask_istft_rows"), (fwd, "sk_sisdr_pit_fwd"), (grad, "sk_sisdr_mask_grad")):
        for S in (0, 5):
            assert call(S=S) == -1
            assert name in err() and "outside 1..4" in err()
    for call, name in ((istft, "sk_mask_istft_rows"), (grad, "sk_sisdr_mask_grad")):
        assert call(n_fft=1024) == -1
        assert name in err() and "n_fft=512" in err()
        assert call(ld=513) == -1
        assert name in err() and "S*F = 514" in err()
        assert call(S=3, ld=770) == -1
    assert istft(mix=None) == -1 and "null pointer" in err()
    assert fwd(est=None) == -1 and "null pointer" in err()
    assert fwd(ws=None) == -1 and "null pointer" in err()
    assert grad(coef=None) == -1 and "null pointer" in err()
    assert lib.sk_sisdr_workspace_bytes(2, 5, 1000) == 0 and lib.sk_sisdr_workspace_bytes(0, 2, 1000) == 0
    assert lib.sk_sisdr_workspace_bytes(32, 2, 64000) >= 32 * 16 * 12 * 8


def test_ops_refuse_cpu_tensors():
    from sepkern import _lib, ops
    from sepkern.packing import Packing
    pk = Packing([5, 3], "cpu")
    mixc, mask = torch.zeros(8, 257, dtype=torch.complex64), torch.zeros(8, 514)
    with pytest.raises(_lib.SepkernError):
        ops.mask_istft_rows(mixc, mask, pk, 2)
    z64, z32 = torch.zeros(4, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(_lib.SepkernError):
        ops.sisdr_pit_fwd(torch.zeros(10), z64, torch.zeros(10), z64, z32, 2, 5)
    with pytest.raises(_lib.SepkernError):
        ops.sisdr_mask_grad(torch.zeros(10), z64, torch.zeros(10), z64, z32, torch.zeros(2, 2, 3), torch.ones(1), mixc, pk, 2)


# ------------------------------------------------------------------------------------------------ 4: conf key, prefetcher
def test_loss_conf_key():
    import uPIT
    assert uPIT.parse_loss("mse") == "mse" and uPIT.parse_loss("sisdr") == "sisdr" and uPIT.parse_loss(" SISDR\n") == "sisdr"
    with pytest.raises(ValueError) as e:
        uPIT.parse_loss("sdr")
    assert "'mse'" in str(e.value) and "'sisdr'" in str(e.value)
    assert "--wav-input" in uPIT.NEEDS_WAVEFORMS and "loss=sisdr" in uPIT.NEEDS_WAVEFORMS


def test_driver_refuses_sisdr_without_wav_input(tmp_path):
    sys.path.insert(0, os.path.join(PKG, "steps"))
    import train_qsub
    import uPIT
    conf = tmp_path / "model.conf"
    conf.write_text("num_spk=2\nloss=sisdr\n")
    base = ["uPIT", "0", str(tmp_path / "data"), str(tmp_path / "exp"), "--model-config", str(conf)]
    with pytest.raises(SystemExit) as e:
        train_qsub.waveform_loss(uPIT, train_qsub.get_args(base))
    assert "--wav-input" in str(e.value)
    assert train_qsub.waveform_loss(uPIT, train_qsub.get_args(base + ["--wav-input"])) is True
    conf.write_text("num_spk=2\n")
    assert train_qsub.waveform_loss(uPIT, train_qsub.get_args(base)) is False
    conf.write_text("loss=l1\n")
    with pytest.raises(ValueError):
        train_qsub.waveform_loss(uPIT, train_qsub.get_args(base))


def test_prefetcher_keep_wave_without_a_device():
    """What of the opt-in can be seen without a GPU: the flag is off by default and stored; a batch without PCM is refused
    where it is staged; batches that are not dicts pass through.  (Staging a PCM batch runs sk_stft: tests/test_gpu_sisdr.py.)"""
    from sepkern.data import Prefetcher
    from torch.nn.utils.rnn import pack_sequence
    assert Prefetcher([], "cpu").keep_wave is False and Prefetcher([], "cpu", keep_wave=True).keep_wave is True
    npz = {"mix": pack_sequence([torch.zeros(4, 257), torch.zeros(3, 257)]), "name": ["a", "b"]}
    with pytest.raises(ValueError, match="needs PCM batches"):
        Prefetcher.stage(npz, "cpu", keep_wave=True)
    assert Prefetcher.stage([1, 2], "cpu", keep_wave=True) == [1, 2]
    # the collator's PCM batch and the per-signal offsets the staged batch will carry
    import uPIT
    pcm = uPIT.WavCollator()([{"mix": np.zeros(700, np.int16), "source1": np.ones(700, np.int16), "source2": np.ones(700, np.int16)},
                             {"mix": np.zeros(900, np.int16), "source1": np.ones(900, np.int16), "source2": np.ones(900, np.int16)}])["pcm"]
    assert pcm["lens"] == [900, 700] and pcm["keys"] == ["mix", "source1", "source2"] and pcm["flat"].numel() == 3 * 1600
