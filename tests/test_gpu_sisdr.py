"""The SI-SDR uPIT loss on the MI355X: sk_mask_istft_rows, sk_sisdr_pit_fwd and sk_sisdr_mask_grad against the CPU oracles
(oracle/stft.py, sepkern/sisdr.py, the torch fp64 autograd restatement in tests/_sisdr_oracle.py), and the arch route
loss=sisdr end to end against the CPU oracle network followed by that fp64 loss.

Gates: iSTFT 3e-6 absolute (tests/test_gpu_kernels.py's); pair 1e-4 dB; the mask gradient's relative-L2 error against fp64
autograd at most 4 x the error of the SAME graph evaluated in torch float32 on the CPU (measured per case, printed); the
full model at the project's gates (loss 1e-5 relative, parameter gradients 2e-4 relative L2).  Every permutation test first
asserts that the oracle's best score leads the runner-up by >= 3 dB in every utterance."""
import functools
import itertools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT
from oracle import stft as OS
from oracle import upit as OU
import _sisdr_oracle as SO

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "speech-separation_amd", "archs"))

F = 257
# samples per utterance, longest first: ~8 s ... ~0.5 s; frames 501, 261, 160 (a whole number of 16-frame tiles), 71, 38, 31
# (not multiples of 16; the last shorter than two tiles)
LENGTHS = [64000, 33333, 20352, 9000, 4800, 3900]
# the gradient kernel's tile loop at its own boundaries: frames 163 (two workgroups of 5 tiles + 3 frames), 81 (5 tiles + 1),
# 80 (exactly 5 tiles), 17 (a tile + 1), 16 (a tile), 3 (every hop an edge hop)
EDGE_LENGTHS = [20780, 10284, 10156, 2092, 1964, 300]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def arch(dev):
    import uPIT
    return uPIT


@functools.lru_cache(maxsize=None)
def _case(S, edge=False):
    return SO.ratio_mask_case(EDGE_LENGTHS if edge else LENGTHS, S, seed=40 + S)


@functools.lru_cache(maxsize=None)
def _oracle(S, edge=False):
    """fp64 autograd (loss, dmask per utterance, info) and the float32 evaluation's dmask of the same graph."""
    c = _case(S, edge)
    refs = [[OS.pcm16_to_float(r).astype(np.float64) for r in rs] for rs in c["refs_pcm"]]
    out = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        ms = [torch.tensor(m, dtype=dt, requires_grad=True) for m in c["masks"]]
        loss, info = SO.loss_from_masks(c["specs"], ms, refs, dtype=dt)
        loss.backward()
        out[name] = dict(loss=float(loss.detach()), dmask=[m.grad.double().numpy() for m in ms], info=info)
    return out


def _rows(c, dev, ld=None):
    """Packed rows of a case: Packing, mixc (Rp, F) complex64, mask (Rp, ld) float32 (source s in columns s F ..)."""
    from sepkern.packing import Packing
    S = c["masks"][0].shape[0]
    ld = S * F if ld is None else ld
    pk = Packing([X.shape[1] for X in c["specs"]], dev)
    mixc = np.zeros((pk.Rp, F), dtype=np.complex64)
    mask = np.zeros((pk.Rp, ld), dtype=np.float32)
    for j, (X, m) in enumerate(zip(c["specs"], c["masks"])):
        T = X.shape[1]
        rows = pk.offs_host[:T].astype(np.int64) + j
        mixc[rows] = X.T
        mask[rows, :S * F] = m.transpose(2, 0, 1).reshape(T, S * F)
    return pk, torch.from_numpy(mixc).to(dev), torch.from_numpy(mask).to(dev)


def _refs(c, dev, as_float):
    """One flat reference buffer (int16 PCM, or the same values as float32) and the offsets [j * S + i]."""
    flat = np.concatenate([r for rs in c["refs_pcm"] for r in rs])
    offs, at = [], 0
    for rs in c["refs_pcm"]:
        for r in rs:
            offs.append(at)
            at += len(r)
    t = torch.from_numpy(OS.pcm16_to_float(flat) if as_float else flat).to(dev)
    return t, torch.tensor(offs, dtype=torch.int64, device=dev)


def _dmask_rows(dm, pk, c):
    """(Rp, ld) packed gradient rows -> list of (S, F, T_j) arrays."""
    S = c["masks"][0].shape[0]
    dm = dm.cpu().numpy()
    out = []
    for j, X in enumerate(c["specs"]):
        T = X.shape[1]
        rows = pk.offs_host[:T].astype(np.int64) + j
        out.append(dm[rows, :S * F].reshape(T, S, F).transpose(1, 2, 0).astype(np.float64))
    return out


def _rel(got, ref):
    g, r = np.concatenate([x.ravel() for x in got]), np.concatenate([x.ravel() for x in ref])
    return float(np.linalg.norm(g - r) / np.linalg.norm(r))


def _forward(c, dev, as_float=False, count_dev=None):
    from sepkern import ops
    S = c["masks"][0].shape[0]
    pk, mixc, mask = _rows(c, dev)
    est, est_offs, offsets = ops.mask_istft_rows(mixc, mask, pk, S)
    ref, ref_offs = _refs(c, dev, as_float)
    nsamp = (pk.lens - 1) * 128
    res = ops.sisdr_pit_fwd(est, est_offs, ref, ref_offs, nsamp, S, 128 * (pk.T - 1), count_dev)
    return dict(pk=pk, mixc=mixc, mask=mask, est=est, est_offs=est_offs, offsets=offsets, ref=ref, ref_offs=ref_offs, res=res)


def _assert_margin(info, what):
    for j, m in enumerate(info["margin"]):
        assert m >= 3.0, "%s: utterance %d: the best permutation leads by %.2f dB only" % (what, j, m)


# ------------------------------------------------------------------------------------------------ 5: iSTFT on packed rows
@pytest.mark.parametrize("S", [2, 3, 4])
def test_mask_istft_rows_matches_oracle_and_mask_istft(dev, S):
    from sepkern import ops
    c = _case(S)
    pk, mixc, mask = _rows(c, dev)
    est, _, offsets = ops.mask_istft_rows(mixc, mask, pk, S)
    specs = [torch.from_numpy(np.ascontiguousarray(X)).to(dev) for X in c["specs"]]
    masks = [[torch.from_numpy(np.ascontiguousarray(m[s])).to(dev) for s in range(S)] for m in c["masks"]]
    other, _ = ops.mask_istft(specs, masks, want_pcm=False, want_float=True)
    est = est.cpu().numpy()
    worst = worst2 = 0.0
    for j, (X, m) in enumerate(zip(c["specs"], c["masks"])):
        L = 128 * (X.shape[1] - 1)
        for s in range(S):
            got = est[offsets[j * S + s]:offsets[j * S + s] + L]
            worst = max(worst, float(np.abs(got - OS.istft(X * m[s])).max()))
            worst2 = max(worst2, float(np.abs(got - other[j][s].cpu().numpy()).max()))
    print("S=%d: mask_istft_rows vs oracle istft %.3g, vs sk_mask_istft %.3g (gate 3e-6)" % (S, worst, worst2))
    assert worst <= 3e-6 and worst2 <= 3e-6


# ------------------------------------------------------------------------------------------------ 6: sums, PIT, finalize
@pytest.mark.parametrize("as_float", [False, True], ids=["int16", "float32"])
@pytest.mark.parametrize("S", [2, 3, 4])
def test_sisdr_pit_fwd(dev, S, as_float):
    from sepkern import ops, sisdr
    c = _case(S)
    _assert_margin(_oracle(S)["f64"]["info"], "S=%d" % S)
    f = _forward(c, dev, as_float)
    res, B = f["res"], len(LENGTHS)
    est = f["est"].cpu().numpy()
    pair = res["pair"].cpu().numpy()
    perms = list(itertools.permutations(range(S)))
    inverse = tuple(c["shuffle"].index(k) for k in range(S))          # refs[i] = source shuffle[i]: estimate k meets refs[inverse[k]]
    best_sum, worst = 0.0, 0.0
    for j, rs in enumerate(c["refs_pcm"]):
        L = 128 * (c["specs"][j].shape[1] - 1)
        es = [est[f["offsets"][j * S + k]:f["offsets"][j * S + k] + L] for k in range(S)]
        want = np.array([[sisdr.si_sdr(es[k], OS.pcm16_to_float(rs[i])[:L]) for i in range(S)] for k in range(S)])
        worst = max(worst, float(np.abs(pair[j] - want).max()))
        score = np.array([np.mean([want[k, p[k]] for k in range(S)]) for p in perms])
        assert int(res["best_perm"][j]) == int(np.argmax(score)) == perms.index(inverse) != 0
        assert int(res["best_perm"][j]) == _oracle(S)["f64"]["info"]["best"][j]
        np.testing.assert_allclose(res["perm_score"][:, j].cpu().numpy(), score, atol=1e-4)
        best_sum += score.max()
    print("S=%d %s: pair vs si_sdr on the device's estimates: %.3g dB (gate 1e-4)" % (S, "float32" if as_float else "int16", worst))
    assert worst <= 1e-4
    out = res["out"].cpu().numpy()
    assert out[1] == B
    np.testing.assert_allclose(out[2], best_sum, rtol=1e-6)
    np.testing.assert_allclose(out[0], -best_sum / B, rtol=1e-6)
    # against the fp64 oracle's own estimates: the float32 iSTFT's 3e-6 sits 80 dB below the estimates, the residuals the scores
    # measure up to 50 dB below them -- an uncorrelated 1e-3 of a residual's energy, 4e-3 dB of a score
    np.testing.assert_allclose(out[0], _oracle(S)["f64"]["loss"], atol=5e-3)
    assert torch.isfinite(res["coef"]).all()
    # a device scalar replaces the count (data parallel: the global utterance count)
    g = _forward(c, dev, as_float, count_dev=torch.full((1,), 2.0 * B, device=dev))["res"]
    np.testing.assert_allclose(g["out"].cpu().numpy(), [out[0] / 2, 2 * B, out[2]], rtol=1e-6)
    np.testing.assert_allclose(g["coef"].cpu().numpy(), res["coef"].cpu().numpy() / 2, rtol=1e-6)
    # two launches: bitwise equal
    again = _forward(c, dev, as_float)
    assert torch.equal(again["est"], f["est"])
    for k in ("pair", "perm_score", "best_perm", "out", "coef"):
        assert torch.equal(again["res"][k], res[k]), k
    # an utterance scored alone: bitwise what it scores inside the batch
    for j in (1, len(LENGTHS) - 1):
        solo = _forward({k: ([v[j]] if k != "shuffle" else v) for k, v in c.items()}, dev, as_float)
        L = 128 * (c["specs"][j].shape[1] - 1)
        assert torch.equal(solo["est"], f["est"][f["offsets"][j * S]:f["offsets"][j * S] + S * L])
        assert torch.equal(solo["res"]["pair"][0], res["pair"][j])
        assert torch.equal(solo["res"]["perm_score"][:, 0], res["perm_score"][:, j])
        assert int(solo["res"]["best_perm"][0]) == int(res["best_perm"][j])


# ------------------------------------------------------------------------------------------------ 7: the fused gradient
@pytest.mark.parametrize("as_float", [False, True], ids=["int16", "float32"])
@pytest.mark.parametrize("S", [2, 3, 4])
def test_sisdr_mask_grad_against_fp64_autograd(dev, S, as_float):
    """Measured on an MI355X (relative L2 against torch fp64 autograd; kernel / the same graph in torch float32 on the CPU):
    see profiles/sisdr_loss.txt, "mask gradient"."""
    from sepkern import ops
    c, orc = _case(S), _oracle(S)
    _assert_margin(orc["f64"]["info"], "S=%d" % S)
    f = _forward(c, dev, as_float)
    pk, res = f["pk"], f["res"]
    one = torch.ones(1, device=dev)
    args = (f["est"], f["est_offs"], f["ref"], f["ref_offs"], res["best_perm"], res["coef"])
    dm = ops.sisdr_mask_grad(*args, one, f["mixc"], pk, S)
    assert dm.shape == (pk.Rp, S * F) and torch.isfinite(dm).all()
    err = _rel(_dmask_rows(dm, pk, c), orc["f64"]["dmask"])
    err32 = _rel(orc["f32"]["dmask"], orc["f64"]["dmask"])
    print("S=%d %s: dmask relative L2 vs fp64 autograd: kernel %.3g, torch float32 on the CPU %.3g (gate: 4 x)"
          % (S, "float32" if as_float else "int16", err, err32))
    assert err <= 4.0 * err32
    # tail rows of a fresh (Rp, .) buffer are zero
    assert pk.Rp > pk.R and not dm[pk.R:].any()
    # gscale scales linearly
    dm3 = ops.sisdr_mask_grad(*args, torch.full((1,), 2.5, device=dev), f["mixc"], pk, S)
    assert float((dm3 - 2.5 * dm).norm() / (2.5 * dm).norm()) <= 1e-6
    # a caller's buffer: tail rows and padding columns are left alone, every valid element is written
    buf = torch.full((pk.Rp + 3, S * F + 3), 7.0, device=dev)
    ops.sisdr_mask_grad(*args, one, f["mixc"], pk, S, out=buf)
    assert (buf[pk.R:] == 7.0).all() and (buf[:, S * F:] == 7.0).all()
    assert torch.equal(buf[:pk.R, :S * F], dm[:pk.R])
    # each utterance's rows depend on that utterance alone.  (Not bit for bit: alone its coefficients are rounded to fp32 for
    # count 1 and scaled by a rounded 1/6, and A e + B r cancels down to 10^(-score/20) of its terms: 2^-24 x 10^(50/20) = 1.9e-5.)
    j = len(LENGTHS) - 1
    solo = _forward({k: ([v[j]] if k != "shuffle" else v) for k, v in c.items()}, dev, as_float)
    sres = solo["res"]
    dms = ops.sisdr_mask_grad(solo["est"], solo["est_offs"], solo["ref"], solo["ref_offs"], sres["best_perm"], sres["coef"],
                              torch.full((1,), 1.0 / len(LENGTHS), device=dev), solo["mixc"], solo["pk"], S)
    got = _dmask_rows(dms, solo["pk"], {"masks": [c["masks"][j]], "specs": [c["specs"][j]]})[0]
    want = _dmask_rows(dm, pk, c)[j]
    assert np.linalg.norm(got - want) <= 1.9e-5 * np.linalg.norm(want)


@pytest.mark.parametrize("as_float", [False, True], ids=["int16", "float32"])
@pytest.mark.parametrize("S", [2, 3, 4])
def test_sisdr_mask_grad_at_the_tile_loop_boundaries(dev, S, as_float):
    """EDGE_LENGTHS: the branches of the gradient kernels' shared tile loop, through the SI-SDR kernel.  On the CPU, for these
    inputs: the oracle's best permutation leads by >= 41.0 / 26.6 / 16.7 dB (S = 2 / 3 / 4), and the float32 evaluation of the
    graph sits 5.7e-7 / 4.7e-7 / 4.4e-7 (relative L2) from the fp64 one; the gate is 4 x that, as above."""
    from sepkern import ops
    c, orc = _case(S, True), _oracle(S, True)
    _assert_margin(orc["f64"]["info"], "S=%d" % S)
    B = len(EDGE_LENGTHS)
    assert [X.shape[1] for X in c["specs"]] == [163, 81, 80, 17, 16, 3]
    f = _forward(c, dev, as_float)
    pk, res = f["pk"], f["res"]
    assert [int(b) for b in res["best_perm"]] == list(orc["f64"]["info"]["best"])
    one = torch.ones(1, device=dev)
    args = (f["est"], f["est_offs"], f["ref"], f["ref_offs"], res["best_perm"], res["coef"])
    dm = ops.sisdr_mask_grad(*args, one, f["mixc"], pk, S)
    assert dm.shape == (pk.Rp, S * F) and torch.isfinite(dm).all()
    got = _dmask_rows(dm, pk, c)
    err = _rel(got, orc["f64"]["dmask"])
    err32 = _rel(orc["f32"]["dmask"], orc["f64"]["dmask"])
    print("S=%d %s: dmask relative L2 vs fp64 autograd: kernel %.3g, torch float32 on the CPU %.3g (gate: 4 x)"
          % (S, "float32" if as_float else "int16", err, err32))
    assert err <= 4.0 * err32
    # a second run gives the same bits
    assert torch.equal(ops.sisdr_mask_grad(*args, one, f["mixc"], pk, S), dm)
    # a caller's buffer: a canary in the rows >= R and the columns >= S F is untouched, every valid element is written
    buf = torch.full((pk.Rp + 3, S * F + 3), 7.0, device=dev)
    ops.sisdr_mask_grad(*args, one, f["mixc"], pk, S, out=buf)
    assert (buf[pk.R:] == 7.0).all() and (buf[:, S * F:] == 7.0).all()
    assert torch.equal(buf[:pk.R, :S * F], dm[:pk.R])
    # A = B = C = 0 gives exact zeros (a canary-filled buffer shows they were written)
    buf.fill_(7.0)
    ops.sisdr_mask_grad(f["est"], f["est_offs"], f["ref"], f["ref_offs"], res["best_perm"], torch.zeros_like(res["coef"]), one,
                        f["mixc"], pk, S, out=buf)
    assert not buf[:pk.R, :S * F].any() and (buf[pk.R:] == 7.0).all() and (buf[:, S * F:] == 7.0).all()
    # an utterance alone (with the batch's count) gives the bits it has inside the batch
    for j in (1, B - 1):
        solo_c = {k: ([v[j]] if k != "shuffle" else v) for k, v in c.items()}
        s = _forward(solo_c, dev, as_float, count_dev=torch.full((1,), float(B), device=dev))
        assert torch.equal(s["res"]["coef"][0], res["coef"][j]) and int(s["res"]["best_perm"][0]) == int(res["best_perm"][j])
        dms = ops.sisdr_mask_grad(s["est"], s["est_offs"], s["ref"], s["ref_offs"], res["best_perm"][j:j + 1].contiguous(),
                                  res["coef"][j:j + 1].contiguous(), one, s["mixc"], s["pk"], S)
        assert np.array_equal(_dmask_rows(dms, s["pk"], solo_c)[0], got[j])


# ------------------------------------------------------------------------------------------------ 8: through the arch
ARCH_LENGTHS = [9000, 7400, 6000, 4800, 3900, 3000]
# The references of test 8 are the initial estimates plus band-limited noise this far below them.  At 10 dB the estimates of an
# untrained network are so alike that the best permutation led by 2.0 .. 2.9 dB only (CPU oracle); at 15 dB by 4.4 .. 5.8 dB.
NOISE_DB = 15.0


def _arch_case(arch, S=2, H=64, L=2, seed=5):
    """Model, oracle network with the same weights, (h0, c0), the mixtures' PCM and -- from ONE oracle forward pass --
    references r_i = e_pi(i) + noise, quantised to int16 (references are data: the gradient flows through the estimates)."""
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    model = arch.SepDNN(0, num_spk=str(S), hidden_dim=str(H), num_layers=str(L), loss="sisdr")
    model.cuda()
    model.train()
    orc = OU.OracleSepDNN(num_spk=S, hidden_dim=H, num_layers=L)
    orc.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    orc.train()
    B = len(ARCH_LENGTHS)
    h0, c0 = torch.randn(2 * L, B, H), torch.randn(2 * L, B, H)
    mixes = [SO.to_pcm(np.sum(SO.band_sources(n, S, 700 + u), axis=0)) for u, n in enumerate(ARCH_LENGTHS)]
    specs = [OS.stft(OS.pcm16_to_float(m)) for m in mixes]
    packed = torch.nn.utils.rnn.pack_sequence([torch.from_numpy(np.abs(X).astype(np.float32).T.copy()) for X in specs])

    def masks_of(mask_out):
        return [mask_out[j, :X.shape[1]].reshape(X.shape[1], S, F).permute(1, 2, 0) for j, X in enumerate(specs)]

    with torch.no_grad():
        first, _ = orc(packed, (h0, c0))
    pi = list(range(1, S)) + [0]
    refs = []
    for X, m in zip(specs, masks_of(first)):
        es = [SO.istft_t(torch.as_tensor(X).to(torch.complex128) * m[s].double()).numpy() for s in range(S)]
        rs = []
        for i in range(S):
            e = es[pi[i]]
            noise = np.convolve(rng.standard_normal(e.shape[0] + 15), np.hanning(16), mode="valid")       # band-limited
            noise *= np.sqrt(np.mean(e ** 2) / np.mean(noise ** 2)) * 10.0 ** (-NOISE_DB / 20.0)
            rs.append(SO.to_pcm(e + noise))
        refs.append(rs)
    # (the extra forward pass moved the BatchNorm running statistics; the training-mode output does not read them)
    orc.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    return dict(model=model, orc=orc, h0=h0, c0=c0, mixes=mixes, specs=specs, packed=packed, refs=refs, masks_of=masks_of, S=S, pi=pi)


def _oracle_step(a):
    """Oracle network (float32, CPU) followed by the fp64 loss; parameter gradients left on a['orc']."""
    a["orc"].zero_grad()
    mask_out, _ = a["orc"](a["packed"], (a["h0"], a["c0"]))
    refs = [[OS.pcm16_to_float(r).astype(np.float64) for r in rs] for rs in a["refs"]]
    loss, info = SO.loss_from_masks(a["specs"], a["masks_of"](mask_out), refs)
    loss.backward()
    return float(loss.detach()), info


def _wav_batch(arch, a):
    samples = []
    for mix, rs in zip(a["mixes"], a["refs"]):
        L = 128 * (len(mix) // 128)
        d = {"mix": mix}
        for i, r in enumerate(rs):          # a source has its mixture's length (the loss reads the first 128 (T - 1) samples)
            d["source%d" % (i + 1)] = np.concatenate([r[:L], np.zeros(len(mix) - L, np.int16)])
        samples.append(d)
    return arch.WavCollator()(samples)


def test_arch_loss_sisdr_matches_oracle_network_and_fp64_loss(arch, dev):
    from sepkern.data import Prefetcher
    a = _arch_case(arch)
    lo, info = _oracle_step(a)
    _assert_margin(info, "arch")
    perms = list(itertools.permutations(range(a["S"])))
    assert all(perms[b] == tuple(a["pi"].index(k) for k in range(a["S"])) and b != 0 for b in info["best"])
    model, batch = a["model"], _wav_batch(arch, a)
    assert batch["pcm"]["lens"] == ARCH_LENGTHS
    model.next_hidden = (a["h0"].cuda(), a["c0"].cuda())
    loss, norm = arch.compute_loss(model, 0, batch)
    loss.backward()
    grads = {k: p.grad.clone() for k, p in model.named_parameters()}
    lv = float(loss.detach())
    print("arch loss=sisdr: loss %.6f dB (oracle %.6f), margins %s" % (lv, lo, ["%.1f" % m for m in info["margin"]]))
    assert float(norm) == len(ARCH_LENGTHS)
    assert model.last_best_perm.cpu().tolist() == info["best"]
    assert abs(lv - lo) <= 1e-5 * abs(lo)
    og = dict(a["orc"].named_parameters())
    worst = 0.0
    for k, g in grads.items():
        ref = og[k].grad.double()
        err = float((g.cpu().double() - ref).norm() / (ref.norm() + 1e-30))
        worst = max(worst, err)
        assert err < 2e-4, (k, err)
    print("arch loss=sisdr: worst parameter-gradient relative L2 %.3g (gate 2e-4)" % worst)
    # the same batch staged by the prefetcher with the waveforms kept: bit-identical
    staged = list(Prefetcher([batch], dev, keep_wave=True))
    assert len(staged) == 1 and "wave" in staged[0] and "packed" in staged[0] and staged[0]["packed"][1] == []
    model.next_hidden = (a["h0"].cuda(), a["c0"].cuda())
    loss2, norm2 = arch.compute_loss(model, 0, staged[0])
    loss2.backward()
    assert torch.equal(loss2.detach(), loss.detach()) and float(norm2) == float(norm)
    for k, p in model.named_parameters():
        assert torch.equal(p.grad, grads[k]), k
    # evaluation mode / no_grad (the CV pass) goes the same way
    model.eval()
    with torch.no_grad():
        cv, cvn = arch.compute_cv_loss(model, 0, batch)
    assert np.isfinite(float(cv)) and float(cvn) == len(ARCH_LENGTHS)


def test_arch_loss_sisdr_bf16_runs(arch, dev):
    """dtype=bf16 takes the same loss route (the loss reads the fp32 mask): finite, close to the fp32 model's loss."""
    a = _arch_case(arch)
    torch.manual_seed(5)
    m16 = arch.SepDNN(0, num_spk="2", hidden_dim="64", num_layers="2", loss="sisdr", dtype="bf16")
    m16.cuda()
    m16.load_state_dict(a["model"].state_dict())
    m16.train()
    batch = _wav_batch(arch, a)
    out = []
    for m in (a["model"], m16):
        m.next_hidden = (a["h0"].cuda(), a["c0"].cuda())
        loss, _ = arch.compute_loss(m, 0, batch)
        loss.backward()
        assert all(torch.isfinite(p.grad).all() for p in m.parameters())
        out.append(float(loss.detach()))
    print("loss=sisdr fp32 %.4f dB, bf16 %.4f dB" % tuple(out))
    assert np.isfinite(out[1]) and abs(out[1] - out[0]) < 1.0


# ------------------------------------------------------------------------------------------------ 9: the default is untouched
def _npz_samples(rng, lens, S):
    samples = []
    for n in lens:
        d = {"mix": np.abs(rng.standard_normal((n, F))).astype(np.float32)}
        for s in range(S):
            d["source%d" % (s + 1)] = np.abs(rng.standard_normal((n, F))).astype(np.float32) * 0.6
        samples.append(d)
    return samples


def test_npz_batches_and_the_default_loss(arch, dev):
    rng = np.random.default_rng(9)
    batch = arch.Collator("mix")(_npz_samples(rng, [14, 11, 9, 6], 2))
    h0, c0 = torch.randn(4, 4, 64), torch.randn(4, 4, 64)
    got = []
    for extra in ({}, {"loss": "mse"}):
        torch.manual_seed(9)
        model = arch.SepDNN(0, hidden_dim="64", num_layers="2", **extra)
        model.cuda()
        model.train()
        assert model.loss_kind == "mse"
        model.next_hidden = (h0.cuda(), c0.cuda())
        loss, norm = arch.compute_loss(model, 0, batch)
        loss.backward()
        got.append((loss.detach().clone(), norm.clone(), [p.grad.clone() for p in model.parameters()]))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert all(torch.equal(x, y) for x, y in zip(got[0][2], got[1][2]))
    torch.manual_seed(9)
    model = arch.SepDNN(0, hidden_dim="64", num_layers="2", loss="sisdr")
    model.cuda()
    with pytest.raises(ValueError, match="needs waveforms: train with `--wav-input`"):
        arch.compute_loss(model, 0, batch)
    with pytest.raises(ValueError, match="'mse' / 'sisdr'"):
        arch.SepDNN(0, hidden_dim="64", num_layers="2", loss="snr")


# ------------------------------------------------------------------------------------------------ 10: it descends
def test_forty_steps_descend(arch, dev):
    """Forty fused clip + Adam steps on one fixed batch (band-limited sources, their true waveforms as references, fixed
    (h0, c0)): the mean loss of the last five steps is below that of the first five.  The curve: profiles/sisdr_loss.txt."""
    from sepkern.optim import ClipAdam
    torch.manual_seed(10)
    S, lens = 2, [9000, 7400, 6000, 4800, 3900, 3000]
    samples = []
    for u, n in enumerate(lens):
        srcs = [SO.to_pcm(s) for s in SO.band_sources(n, S, 900 + u)]
        d = {"mix": SO.to_pcm(np.sum([s.astype(np.float64) for s in srcs], axis=0) / 32768.0)}
        for i, s in enumerate(srcs):
            d["source%d" % (i + 1)] = s
        samples.append(d)
    batch = arch.WavCollator()(samples)
    model = arch.SepDNN(0, num_spk=str(S), hidden_dim="64", num_layers="2", loss="sisdr")
    model.cuda()
    model.train()
    opt = ClipAdam(model, lr=1e-3, max_norm=0.25)
    h0, c0 = torch.randn(4, len(lens), 64, device=dev), torch.randn(4, len(lens), 64, device=dev)
    curve = []
    for _ in range(40):
        model.next_hidden = (h0, c0)
        loss, _ = arch.compute_loss(model, 0, batch)
        loss.backward()
        opt.step()
        curve.append(float(loss.detach()))
    print("forty steps, loss (negative SI-SDR, dB): " + " ".join("%.3f" % v for v in curve))
    assert all(np.isfinite(curve)) and int(opt.scal[3]) == 0
    assert np.mean(curve[-5:]) < np.mean(curve[:5])
