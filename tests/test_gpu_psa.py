"""The phase-sensitive uPIT losses (loss=psa / tpsa) on the MI355X: sk_stft_psa against the existing STFT kernel, the numpy
restatement of the targets (sepkern/psa.py) and the CPU oracle (oracle/stft.py), and the arch routes end to end against the
CPU oracle network followed by the fp64 PIT-MSE on the oracle's targets.

One ragged batch, longest first: frame counts 165, 81, 80, 17, 16, 3 -- several workgroups (a workgroup walks 5 tiles of 16
frames = 80), a workgroup plus one frame, exactly a workgroup, a tile plus one, exactly a tile, and an utterance barely above
the reflect limit.  Run with -s for the measured figures."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import PKG
from oracle import stft as OS
from oracle import upit as OU

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(PKG, "archs"))
sys.path.insert(0, os.path.join(PKG, "steps"))

F = 257
LENGTHS = [21000, 10240, 10112, 2048, 1920, 300]
FRAMES = [165, 81, 80, 17, 16, 3]
CASES = [(2, "int16"), (2, "float32"), (3, "int16"), (3, "float32")]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def arch(dev):
    import uPIT
    return uPIT


def _signals(lengths, S, seed):
    """Per utterance [mix, source 1 .. S] int16: seeded Gaussian noise through a 4-tap moving average, source s at level
    0.1 (1 + s); the mixture is the sum (exact in int16 and, over 32768, in float32)."""
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        srcs = []
        for s in range(S):
            x = np.convolve(rng.standard_normal(n + 3), np.full(4, 0.25), mode="valid") * 0.1 * (1 + s)
            srcs.append(np.rint(x * 32768.0).astype(np.int64))
        mix = sum(srcs)
        assert max(np.abs(mix).max(), max(np.abs(x).max() for x in srcs)) < 32768
        out.append([mix.astype(np.int16)] + [x.astype(np.int16) for x in srcs])
    return out


@functools.lru_cache(maxsize=None)
def _case(S):
    """The batch's signals, their oracle spectra (257, T) -- computed once, shared, never written to."""
    sigs = _signals(LENGTHS, S, seed=70 + S)
    assert [OS.num_frames(n) for n in LENGTHS] == FRAMES
    spec = [[OS.stft(OS.pcm16_to_float(x)).astype(np.complex128) for x in utt] for utt in sigs]
    return dict(sigs=sigs, spec=spec)


def _flat(sigs, dtype, dev):
    """Key-major flat tensor (every mixture, then every source 1, ...) and the S + 1 offset lists."""
    nk, lens = len(sigs[0]), [len(u[0]) for u in sigs]
    flat = np.concatenate([u[q] for q in range(nk) for u in sigs])
    starts, total = np.concatenate([[0], np.cumsum(lens)[:-1]]), sum(lens)
    t = torch.from_numpy(OS.pcm16_to_float(flat) if dtype == "float32" else flat).to(dev)
    return t, [[int(q * total + st) for st in starts] for q in range(nk)], lens


def _run(sigs, dtype, dev, clamp=False, packed=True):
    from sepkern import ops
    from sepkern.packing import Packing
    flat, offs, lens = _flat(sigs, dtype, dev)
    pk = Packing([1 + n // 128 for n in lens], dev) if packed else None
    mix, tg = ops.stft_psa(flat, offs, lens, len(sigs[0]) - 1, pk=pk, clamp=clamp)
    return mix, tg, pk


@functools.lru_cache(maxsize=None)
def _batch(S, dtype, clamp=False):
    return _run(_case(S)["sigs"], dtype, torch.device("cuda", 0), clamp)


def _utt(rows, pk, j):
    """Rows of utterance j of a packed (Rp, F) tensor -> (T_j, F)."""
    T = int(pk.lens_host[j])
    return rows[torch.from_numpy(pk.offs_host[:T].astype(np.int64) + j).to(rows.device)]


@functools.lru_cache(maxsize=None)
def _sk_stft(S):
    """The existing kernel's complex spectra of every signal of the batch: [utterance][signal] (T, 257) complex128."""
    from sepkern import ops
    sigs = _case(S)["sigs"]
    flat = [torch.from_numpy(x).cuda() for utt in sigs for x in utt]
    out = [o.cpu().numpy().astype(np.complex128) for o in ops.stft_batch(flat, want_complex=True, layout="TF")]
    return [out[u * (S + 1):(u + 1) * (S + 1)] for u in range(len(sigs))]


# ------------------------------------------------------------------------------------------------ 1: the network's input
@pytest.mark.parametrize("S,dtype", CASES)
def test_mixture_rows_are_those_of_features_from_pcm(dev, S, dtype):
    from sepkern.data import features_from_pcm
    flat, _, lens = _flat(_case(S)["sigs"], dtype, dev)
    keys = ["mix"] + ["source%d" % (s + 1) for s in range(S)]
    ref_mix, ref_srcs, ref_pk = features_from_pcm({"flat": flat, "keys": keys, "lens": lens}, dev)
    mix, tg, pk = _batch(S, dtype)
    assert mix.shape == ref_mix.shape == (pk.Rp, F) and pk.R == ref_pk.R == sum(FRAMES)
    assert torch.equal(mix, ref_mix)
    assert len(tg) == S and all(t.shape == (pk.Rp, F) for t in tg)
    assert pk.Rp > pk.R and not mix[pk.R:].any() and not any(t[pk.R:].any() for t in tg)
    assert all(torch.isfinite(t).all() for t in tg)
    # the targets are not the magnitudes: they go negative, and never exceed the source
    assert all((t < 0).any() for t in tg) and all((t.abs() <= m * (1 + 1e-6)).all() for t, m in zip(tg, ref_srcs))


# ------------------------------------------------------------------------------------------------ 2: the formula, on sk_stft's spectra
@pytest.mark.parametrize("S,dtype", CASES)
def test_targets_are_the_formula_on_the_existing_kernels_spectra(dev, S, dtype):
    """|target - r| <= 8 x 2^-24 (|Sr Yr| + |Si Yi|) / |Y| + 2^-140, r the fp64 formula on sk_stft(want_complex=True)'s spectra
    of the same signals: two products, one addition, the reciprocal square root and one multiply, each rounded once, doubled."""
    from sepkern import psa
    mix, tg, pk = _batch(S, dtype)
    worst = 0.0
    for j, spectra in enumerate(_sk_stft(S)):
        Y = spectra[0]
        ref = psa.psa_targets(Y, spectra[1:])
        amag = np.sqrt(Y.real ** 2 + Y.imag ** 2)
        assert amag.min() > 0.0
        for s in range(S):
            Ss = spectra[1 + s]
            bound = 8.0 * 2.0 ** -24 * (np.abs(Ss.real * Y.real) + np.abs(Ss.imag * Y.imag)) / amag + 2.0 ** -140
            err = np.abs(_utt(tg[s], pk, j).cpu().numpy().astype(np.float64) - ref[s])
            worst = max(worst, float((err / bound).max()))
    print("S=%d %s: worst |target - formula on sk_stft's spectra| / bound = %.3f (gate 1)" % (S, dtype, worst))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ 3: end to end against the oracle
@functools.lru_cache(maxsize=None)
def _oracle_yardstick(S):
    """e_Y, e_S: the largest absolute errors of sk_stft's complex output against oracle/stft.py on the mixtures / the sources of
    this very batch; and the share of elements with |S| / |Y| > 100."""
    c, got = _case(S), _sk_stft(S)
    e_y = max(float(np.abs(g[0] - sp[0].T).max()) for g, sp in zip(got, c["spec"]))
    e_s = max(float(np.abs(g[q] - sp[q].T).max()) for g, sp in zip(got, c["spec"]) for q in range(1, S + 1))
    ratio = np.concatenate([(np.abs(sp[q]) / np.abs(sp[0])).ravel() for sp in c["spec"] for q in range(1, S + 1)])
    return e_y, e_s, float(np.mean(ratio > 100.0))


@pytest.mark.parametrize("S,dtype", CASES)
def test_targets_against_the_oracle_stft(dev, S, dtype):
    """Reference: psa_targets on oracle.stft.stft of the same samples.  Tolerance per element 4 (e_S + e_Y |S| / |Y|), e_S and
    e_Y the existing sk_stft's own worst errors against that oracle on these signals: the existing kernel is the yardstick, with
    a factor 4 for the two spectra that enter a quotient."""
    from sepkern import psa
    e_y, e_s, share = _oracle_yardstick(S)
    assert share < 0.01, share            # the conditioning term cannot swallow a failure
    c = _case(S)
    worst_abs = worst_rel = 0.0
    for clamp in (False, True):
        mix, tg, pk = _batch(S, dtype, clamp)
        for j, sp in enumerate(c["spec"]):
            ref = psa.psa_targets(sp[0], sp[1:], clamp=clamp)
            for s in range(S):
                tol = 4.0 * (e_s + e_y * np.abs(sp[1 + s]) / np.abs(sp[0]))
                err = np.abs(_utt(tg[s], pk, j).cpu().numpy().astype(np.float64).T - ref[s])
                worst_abs, worst_rel = max(worst_abs, float(err.max())), max(worst_rel, float((err / tol).max()))
    print("S=%d %s: sk_stft vs oracle e_Y %.3g e_S %.3g; |S|/|Y| > 100 on %.2g of the elements; worst target error %.3g, "
          "%.3f of its tolerance (gate 1)" % (S, dtype, e_y, e_s, share, worst_abs, worst_rel))
    assert worst_rel <= 1.0


# ------------------------------------------------------------------------------------------------ 4: the truncated form
@pytest.mark.parametrize("S,dtype", CASES)
def test_clamp_is_the_clamp_of_the_unclamped_targets(dev, S, dtype):
    mix, tg, _ = _batch(S, dtype)
    mixc, tgc, _ = _batch(S, dtype, True)
    assert torch.equal(mix, mixc)
    for t, tc in zip(tg, tgc):
        assert torch.equal(tc, torch.minimum(torch.maximum(t, torch.zeros_like(t)), mix))
        assert (tc < t).any() and (tc > t).any()


# ------------------------------------------------------------------------------------------------ 5: determinism
@pytest.mark.parametrize("S", [2, 3])
def test_bits_do_not_depend_on_the_batch_the_sample_format_or_the_run(dev, S):
    sigs = _case(S)["sigs"]
    mix, tg, pk = _batch(S, "int16")
    for other in (_batch(S, "float32"), _run(sigs, "int16", dev)):
        assert torch.equal(other[0], mix) and all(torch.equal(a, b) for a, b in zip(other[1], tg))
    for j in range(len(sigs)):
        m1, t1, pk1 = _run([sigs[j]], "int16", dev)
        assert torch.equal(m1[:pk1.R], _utt(mix, pk, j))
        for s in range(S):
            assert torch.equal(t1[s][:pk1.R], _utt(tg[s], pk, j)), (j, s)


# ------------------------------------------------------------------------------------------------ 6: per-utterance addressing
@pytest.mark.parametrize("S,dtype", CASES)
def test_per_utterance_blocks_hold_the_packed_rows(dev, S, dtype):
    mix, tg, pk = _batch(S, dtype, True)
    bmix, btg, none = _run(_case(S)["sigs"], dtype, dev, clamp=True, packed=False)
    assert none is None and bmix.shape == (sum(FRAMES), F) and all(t.shape == bmix.shape for t in btg)
    at = 0
    for j, T in enumerate(FRAMES):
        assert torch.equal(bmix[at:at + T], _utt(mix, pk, j))
        for s in range(S):
            assert torch.equal(btg[s][at:at + T], _utt(tg[s], pk, j))
        at += T


def test_a_callers_buffer_is_written_in_place(dev):
    from sepkern import ops
    from sepkern.packing import Packing
    S = 2
    flat, offs, lens = _flat(_case(S)["sigs"], "int16", dev)
    pk = Packing(FRAMES, dev)
    mix, tg, _ = _batch(S, "int16")
    bm, bt = torch.full((pk.Rp + 3, F + 7), 7.0, device=dev), torch.full((S, pk.Rp + 3, F + 7), 7.0, device=dev)
    ops.stft_psa(flat, offs, lens, S, pk=pk, out=(bm, bt))
    assert torch.equal(bm[:pk.R, :F], mix[:pk.R]) and all(torch.equal(bt[s, :pk.R, :F], tg[s][:pk.R]) for s in range(S))
    assert (bm[pk.R:] == 7.0).all() and (bm[:, F:] == 7.0).all() and (bt[:, pk.R:] == 7.0).all() and (bt[:, :, F:] == 7.0).all()


# ------------------------------------------------------------------------------------------------ 7: argument errors
def test_argument_errors(dev):
    from sepkern import _lib, ops
    S = 2
    flat, offs, lens = _flat(_case(S)["sigs"], "int16", dev)

    def untouched(out):
        torch.cuda.synchronize()
        return all((o == 7.0).all() for o in out)
    out = (torch.full((sum(FRAMES), F), 7.0, device=dev), torch.full((S, sum(FRAMES), F), 7.0, device=dev))
    with pytest.raises(_lib.SepkernError, match=r"code -1.*num_spk 0 outside 1\.\.4"):
        ops.stft_psa(flat, offs[:1], lens, 0, out=out)
    assert untouched(out)
    with pytest.raises(_lib.SepkernError, match=r"code -1.*256 samples.*reflect"):
        ops.stft_psa(flat, [o[:1] for o in offs], [256], S, out=out)
    assert untouched(out)
    narrow = (torch.full((sum(FRAMES), 256), 7.0, device=dev), torch.full((S, sum(FRAMES), 256), 7.0, device=dev))
    with pytest.raises(_lib.SepkernError, match=r"code -1.*rows of 256 floats"):
        ops.stft_psa(flat, offs, lens, S, out=narrow)
    assert untouched(narrow)
    with pytest.raises(_lib.SepkernError, match="length-sorted"):
        from sepkern.packing import Packing
        ops.stft_psa(flat, [o[::-1] for o in offs], lens[::-1], S, pk=Packing.from_lens(FRAMES[::-1], dev))


# ------------------------------------------------------------------------------------------------ 8: through the arch
ARCH_LENGTHS = LENGTHS[2:]            # the four shortest: 80, 17, 16, 3 frames


def _wav_batch(arch, sigs):
    return arch.WavCollator()([dict([("mix", u[0])] + [("source%d" % i, x) for i, x in enumerate(u[1:], 1)]) for u in sigs])


def _model(arch, kind, S=2, H=64, L=2, seed=8):
    torch.manual_seed(seed)
    model = arch.SepDNN(0, num_spk=str(S), hidden_dim=str(H), num_layers=str(L), loss=kind)
    model.cuda()
    model.train()
    return model


def _step(arch, model, batch, h0, c0):
    model.next_hidden = (h0.cuda(), c0.cuda())
    loss, norm = arch.compute_loss(model, 0, batch)
    loss.backward()
    return loss.detach().clone(), norm.clone(), {k: p.grad.clone() for k, p in model.named_parameters()}


def _write_tree(root, sigs, rate=8000):
    """<root>/wav/{mix,s1,..}/<id>.wav and <root>/data/wav.scp; ids sort like the utterances."""
    import scipy.io.wavfile
    data = os.path.join(root, "data")
    os.makedirs(data)
    ids = ["utt%02d" % u for u in range(len(sigs))]
    with open(os.path.join(data, "wav.scp"), "w") as scp:
        for i, utt in zip(ids, sigs):
            for q, x in enumerate(utt):
                d = os.path.join(root, "wav", "mix" if q == 0 else "s%d" % q)
                os.makedirs(d, exist_ok=True)
                scipy.io.wavfile.write(os.path.join(d, i + ".wav"), rate, x)
            scp.write("%s %s\n" % (i, os.path.join(root, "wav", "mix", i + ".wav")))
    return data, ids


@pytest.mark.parametrize("kind", ["psa", "tpsa"])
def test_arch_loss_matches_oracle_network_and_fp64_pit_mse(arch, dev, kind, tmp_path, monkeypatch):
    from sepkern import psa
    from sepkern.data import Prefetcher
    S, H, L = 2, 64, 2
    sigs = _case(S)["sigs"][2:]
    spec = _case(S)["spec"][2:]
    B = len(sigs)
    model = _model(arch, kind)
    orc = OU.OracleSepDNN(num_spk=S, hidden_dim=H, num_layers=L)
    orc.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    orc.train()
    h0, c0 = torch.randn(2 * L, B, H), torch.randn(2 * L, B, H)

    # the oracle: its network (float32, CPU) on |oracle STFT|, then PIT-MSE in fp64 on psa_targets of the oracle STFT
    pad = lambda rows: torch.nn.utils.rnn.pad_sequence([torch.from_numpy(np.ascontiguousarray(r.T)) for r in rows], batch_first=True)  # noqa: E731
    packed = torch.nn.utils.rnn.pack_sequence([torch.from_numpy(np.abs(sp[0]).astype(np.float32).T.copy()) for sp in spec])
    mask_out, _ = orc(packed, (h0, c0))
    tgs = [psa.psa_targets(sp[0], sp[1:], clamp=kind == "tpsa") for sp in spec]
    lo, no, losses, idx = OU.pit_mse(mask_out.double(), pad([np.abs(sp[0]).astype(np.float32).astype(np.float64) for sp in spec]),
                                     [pad([t[s] for t in tgs]) for s in range(S)], torch.tensor(FRAMES[2:]), S, F)
    lo.backward()
    two = torch.sort(losses, 0).values
    # no permutation is tied within what the loss gate lets through: the runner-up is at least 10 x 1e-5 away, relatively
    # (an untrained network's two masks are alike, so the margin is what the initial weights happen to give: 2e-4 .. 1e-1 here)
    assert float((two[1] / two[0]).min()) > 1.0 + 1e-4
    lo_v = float(lo.detach())

    batch = _wav_batch(arch, sigs)
    assert batch["pcm"]["lens"] == ARCH_LENGTHS
    loss, norm, grads = _step(arch, model, batch, h0, c0)
    lv = float(loss)
    print("arch loss=%s: loss %.8g (oracle %.8g), norm %d" % (kind, lv, lo_v, int(norm)))
    assert float(norm) == float(no) == sum(FRAMES[2:]) * F
    assert model.last_best_perm.cpu().tolist() == idx.tolist()
    assert abs(lv - lo_v) <= 1e-5 * abs(lo_v)
    og, worst = dict(orc.named_parameters()), 0.0
    for k, g in grads.items():
        ref = og[k].grad.double()
        err = float((g.cpu().double() - ref).norm() / (ref.norm() + 1e-30))
        worst = max(worst, err)
        assert err < 2e-4, (k, err)
    print("arch loss=%s: worst parameter-gradient relative L2 %.3g (gate 2e-4)" % (kind, worst))

    def same(got):
        assert torch.equal(got[0], loss) and torch.equal(got[1], norm)
        for k, g in got[2].items():
            assert torch.equal(g, grads[k]), k

    # the same batch staged by the prefetcher with the targets in place of the source magnitudes
    staged = list(Prefetcher([batch], dev, targets=kind))
    assert len(staged) == 1 and staged[0]["targets"] == kind and len(staged[0]["packed"][1]) == S and "pcm" not in staged[0]
    same(_step(arch, model, staged[0], h0, c0))
    other = "psa" if kind == "tpsa" else "tpsa"
    with pytest.raises(ValueError, match="staged with %r targets" % other):
        arch.compute_loss(model, 0, dict(staged[0], targets=other))

    # npz features written by extract_feats.py --psa-targets, trained with loss=mse
    import extract_feats
    data, ids = _write_tree(str(tmp_path), sigs)
    feats = os.path.join(str(tmp_path), "feats")
    monkeypatch.setattr(sys, "argv", ["extract_feats.py", data, "train", feats, "--psa-targets", "--writers", "2"]
                        + (["--psa-clamp"] if kind == "tpsa" else []))
    extract_feats.main()
    z = np.load(os.path.join(feats, ids[0] + ".npz"))
    assert sorted(z.files) == ["mix", "s1", "s2"] and all(z[k].shape == (F, FRAMES[2]) and z[k].dtype == np.float32 for k in z.files)
    ts = arch.TrainSet(data)
    npz_batch = ts.collator([ts[i] for i in range(len(ts))])
    model.loss_kind = "mse"
    same(_step(arch, model, npz_batch, h0, c0))
    # ... while a phase-sensitive model refuses such a batch: it cannot tell what the npz files hold
    model.loss_kind = kind
    with pytest.raises(ValueError, match="`loss=%s` needs waveforms: train with `--wav-input`" % kind):
        arch.compute_loss(model, 0, npz_batch)
    # evaluation mode / no_grad (the CV pass) goes the same way
    model.eval()
    with torch.no_grad():
        model.next_hidden = (h0.cuda(), c0.cuda())
        cv, cvn = arch.compute_cv_loss(model, 0, batch)
    assert np.isfinite(float(cv)) and float(cvn) == float(norm)


# ------------------------------------------------------------------------------------------------ 9: a batch at another rate
def test_a_16k_batch_is_resampled_in_front_of_the_kernel(dev):
    from sepkern import ops
    from sepkern.data import psa_features_from_pcm
    S, lens16 = 2, [6000, 3100]
    sigs = _signals(lens16, S, seed=9)
    flat, _, _ = _flat(sigs, "int16", dev)
    pcm = {"flat": flat, "keys": ["mix", "source1", "source2"], "lens": lens16, "rate": [16000, 16000], "target_rate": 8000}
    mix, tg, pk = psa_features_from_pcm(pcm, dev, clamp=True)
    at8k, outs = ops.pcm_to_rate(flat, lens16 * (S + 1), [16000] * (2 * (S + 1)), 8000)
    ns = outs[:2]
    assert ns == [3000, 1550] and pk.lens_host.tolist() == [1 + n // 128 for n in ns]
    total, starts = sum(ns), [0, ns[0]]
    rmix, rtg = ops.stft_psa(at8k, [[q * total + st for st in starts] for q in range(S + 1)], ns, S, pk=pk, clamp=True)
    assert torch.equal(mix, rmix) and all(torch.equal(a, b) for a, b in zip(tg, rtg))
    assert mix[:pk.R].min() > 0 and all(t[:pk.R].max() > 0 for t in tg)


# ------------------------------------------------------------------------------------------------ 10: isolation
def test_the_other_losses_never_reach_the_new_entry_point(arch, dev, monkeypatch):
    from sepkern import _lib
    calls = []
    real = _lib.call

    def spy(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    sigs = _case(2)["sigs"][2:]
    batch = _wav_batch(arch, sigs)
    h0, c0 = torch.randn(4, len(sigs), 64), torch.randn(4, len(sigs), 64)
    seen = {}
    for kind in ("mse", "sisdr", "psa"):
        del calls[:]
        _step(arch, _model(arch, kind), batch, h0, c0)
        seen[kind] = set(calls)
    assert "sk_stft" in seen["mse"] and "sk_stft" in seen["sisdr"] and "sk_pit_mse_fwd" in seen["mse"]
    assert "sk_stft_psa" not in seen["mse"] and "sk_stft_psa" not in seen["sisdr"]
    assert "sk_stft_psa" in seen["psa"] and "sk_stft" not in seen["psa"] and "sk_pack_rows" not in seen["psa"]
    assert {"sk_pit_mse_fwd", "sk_pit_mse_bwd"} <= seen["psa"]


# ------------------------------------------------------------------------------------------------ 11: it descends
def test_twenty_steps_descend(arch, dev):
    """Twenty fused clip + Adam steps of loss=tpsa on one fixed batch with fixed (h0, c0): the mean of the last five losses is
    below the mean of the first five (-s prints the curve)."""
    from sepkern.optim import ClipAdam
    sigs = _case(2)["sigs"][2:]
    batch = _wav_batch(arch, sigs)
    model = _model(arch, "tpsa", seed=11)
    opt = ClipAdam(model, lr=1e-3, max_norm=0.25)
    h0, c0 = torch.randn(4, len(sigs), 64, device=dev), torch.randn(4, len(sigs), 64, device=dev)
    curve = []
    for _ in range(20):
        model.next_hidden = (h0, c0)
        loss, _ = arch.compute_loss(model, 0, batch)
        loss.backward()
        opt.step()
        curve.append(float(loss.detach()))
    print("twenty steps, loss=tpsa: " + " ".join("%.5f" % v for v in curve))
    assert all(np.isfinite(curve)) and int(opt.scal[3]) == 0
    assert np.mean(curve[-5:]) < np.mean(curve[:5])


# ------------------------------------------------------------------------------------------------ 12: the oracle mask
def test_evaluate_oracle_psm(dev, tmp_path, monkeypatch):
    import evaluate_oracle
    from sepkern import ops, psa
    S = 2
    sigs = _signals([4000, 3000], S, seed=12)
    data, ids = _write_tree(str(tmp_path), sigs)
    with pytest.raises(ValueError, match="--hard-mask and --psm"):
        evaluate_oracle.main([data, "--psm", "--hard-mask"])
    applied = []
    real = ops.mask_istft

    def spy(specs, masks=None, **kw):
        applied.append([m.cpu().numpy().astype(np.float64) for m in masks[0]])
        return real(specs, masks, **kw)
    monkeypatch.setattr(ops, "mask_istft", spy)
    evaluate_oracle.main([data, "--psm"])
    out = os.path.join(data, "oracle_psm_mask_eval")
    for metric in ("SDR", "SIR", "SAR", "SISDR"):
        lines = open(os.path.join(out, "source_%ss.txt" % metric)).read().splitlines()
        assert [l.split(' ')[0] for l in lines] == ids and all(len(l.split(' ')) == 1 + S for l in lines)
        assert all(np.isfinite(float(v)) for l in lines for v in l.split(' ')[1:])
    assert not os.path.exists(os.path.join(data, "oracle_soft_mask_eval"))
    # the masks it applied: ideal_psm of the oracle spectra, within test 3's tolerance over |Y|
    assert len(applied) == len(sigs)
    worst = 0.0
    for utt, masks in zip(sigs, applied):
        sp = [OS.stft(OS.pcm16_to_float(x)).astype(np.complex128) for x in utt]
        got = [o.cpu().numpy().astype(np.complex128).T for o in
               ops.stft_batch([torch.from_numpy(x).to(dev) for x in utt], want_complex=True, layout="TF")]
        e_y = float(np.abs(got[0] - sp[0]).max())
        e_s = max(float(np.abs(g - s).max()) for g, s in zip(got[1:], sp[1:]))
        for s in range(S):
            assert masks[s].shape == sp[0].shape and masks[s].min() >= 0.0 and masks[s].max() <= 1.0
            tol = 4.0 * (e_s + e_y * np.abs(sp[1 + s]) / np.abs(sp[0])) / np.abs(sp[0])
            worst = max(worst, float((np.abs(masks[s] - psa.ideal_psm(sp[0], sp[1 + s])) / tol).max()))
    print("evaluate_oracle --psm: worst mask error %.3f of its tolerance (gate 1)" % worst)
    assert worst <= 1.0
