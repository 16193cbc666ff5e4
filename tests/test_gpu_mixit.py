"""The mixture-invariant loss on the MI355X: sk_mixit_fwd and sk_mixit_mask_grad against sepkern/mixit.py and the torch fp64
autograd restatement of the direct definition (tests/_mixit_oracle.py), and the arch route loss=mixit end to end against the
CPU oracle network followed by that fp64 loss.

Gates: every assignment score within 2^-23 max(1, |v|) dB of the fp64 value (the outputs are fp32 roundings of fp64 values; the
sums' own error is below 1e-13 relative because err / P >= tau); the best code equal in EVERY utterance, after asserting that
the reference's best score leads the runner-up by more than 1 dB in each; coefficients 2^-22 relative; the mask gradient's
relative-L2 error against fp64 at most 4 x the error of the SAME graph evaluated in torch float32 on the CPU (measured per
case, printed; profiles/mixit_loss.txt holds both); the full model at the project's gates (loss 1e-5 relative, parameter
gradients 2e-4 relative L2)."""
import functools
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT
from oracle import stft as OS
from oracle import upit as OU
import _sisdr_oracle as SO
import _mixit_oracle as MO

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "speech-separation_amd", "archs"))
sys.path.insert(0, os.path.join(PKG, "steps"))

F = 257
TAU = 1e-3                                # mixit_snr_max = 30 dB


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def arch(dev):
    import uPIT
    return uPIT


def _i64(v, dev):
    return torch.tensor(v, dtype=torch.int64, device=dev)


# ------------------------------------------------------------------------------------------------ 1: sums, search, finalize
# frames per utterance -> 128 (T - 1) samples: 256 (fewer than the 256 threads x 2), 4096 (exactly one chunk), 4224 (one chunk and
# a hop), 64000 (many chunks)
FWD_FRAMES = [501, 34, 33, 3]
SILENT = 1                                # this utterance's reference 1 is silent


@functools.lru_cache(maxsize=None)
def _fwd_case(M):
    """Noisy partitions with drawn codes and their fp64 reference (count = the batch's size)."""
    from sepkern import mixit
    utts = [MO.noisy_partition(128 * (T - 1), M, seed=10 * M + j, silent=1 if j == SILENT else None)
            for j, T in enumerate(FWD_FRAMES)]
    want = [mixit.mixit(u["ests"], [OS.pcm16_to_float(x).astype(np.float64) for x in u["refs_pcm"]], count=len(utts)) for u in utts]
    return utts, want


def _flat_inputs(utts, dev, as_float):
    est = torch.from_numpy(np.concatenate([e for u in utts for e in u["ests"]])).to(dev)
    pcm = np.concatenate([x for u in utts for x in u["refs_pcm"]])
    ref = torch.from_numpy(OS.pcm16_to_float(pcm) if as_float else pcm).to(dev)
    eo, ro, at, rt = [], [], 0, 0
    for u in utts:
        L = len(u["ests"][0])
        for _ in u["ests"]:
            eo.append(at)
            at += L
        for _ in range(2):
            ro.append(rt)
            rt += L
    nsamp = torch.tensor([len(u["ests"][0]) for u in utts], dtype=torch.int32, device=dev)
    return est, _i64(eo, dev), ref, _i64(ro, dev), nsamp


def _run_fwd(utts, M, dev, as_float, count_dev=None):
    from sepkern import ops
    est, eo, ref, ro, nsamp = _flat_inputs(utts, dev, as_float)
    return ops.mixit_fwd(est, eo, ref, ro, nsamp, M, max(len(u["ests"][0]) for u in utts), TAU, count_dev)


@pytest.mark.parametrize("as_float", [False, True], ids=["int16", "float32"])
@pytest.mark.parametrize("M", [2, 3, 4])
def test_mixit_fwd_against_fp64(dev, M, as_float):
    utts, want = _fwd_case(M)
    B = len(utts)
    for j, w in enumerate(want):          # no case may hide behind a near tie
        top = np.sort(w["score"])
        assert top[-1] - top[-2] > 1.0, "utterance %d: the best code leads by %.2f dB only" % (j, top[-1] - top[-2])
    assert want[SILENT]["P"][1] == 0.0 and want[SILENT]["coef"][1] == 0.0
    res = _run_fwd(utts, M, dev, as_float)
    score = res["assign_score"].cpu().numpy().astype(np.float64)
    assert score.shape == (1 << M, B)
    worst = 0.0
    for j, w in enumerate(want):
        tol = 2.0 ** -23 * np.maximum(1.0, np.abs(w["score"]))
        worst = max(worst, float((np.abs(score[:, j] - w["score"]) / tol).max()))
        assert int(res["best_code"][j]) == w["best"], (j, int(res["best_code"][j]), w["best"])
    print("M=%d %s: worst assignment score error %.3f of its gate 2^-23 max(1, |v|) dB; gaps %s dB"
          % (M, "float32" if as_float else "int16", worst, ["%.1f" % (np.sort(w["score"])[-1] - np.sort(w["score"])[-2]) for w in want]))
    assert worst <= 1.0
    coef = res["coef"].cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(coef))
    for j, w in enumerate(want):
        assert np.all(np.abs(coef[j] - w["coef"]) <= 2.0 ** -22 * np.abs(w["coef"])), (j, coef[j], w["coef"])
    assert coef[SILENT, 1] == 0.0
    out = res["out"].cpu().numpy().astype(np.float64)
    tot = sum(w["score"][w["best"]] for w in want)
    assert out[1] == B
    np.testing.assert_allclose(out[2], tot, rtol=2.0 ** -22)
    np.testing.assert_allclose(out[0], -tot / B, rtol=2.0 ** -22)
    # a device scalar replaces the count (data parallel: the global utterance count)
    g = _run_fwd(utts, M, dev, as_float, count_dev=torch.full((1,), 2.0 * B, device=dev))
    np.testing.assert_allclose(g["out"].cpu().numpy(), [out[0] / 2, 2 * B, out[2]], rtol=1e-6)
    np.testing.assert_allclose(g["coef"].cpu().numpy(), coef / 2, rtol=1e-6)
    # two launches: bitwise equal; int16 and float32 references hold the same values: bitwise equal
    again = _run_fwd(utts, M, dev, not as_float)
    for k in ("assign_score", "best_code", "out", "coef"):
        assert torch.equal(again[k], res[k]), k
    # an utterance scored alone (with the batch's count): bitwise what it scores inside the batch
    for j in (0, B - 1):
        solo = _run_fwd([utts[j]], M, dev, as_float, count_dev=torch.full((1,), float(B), device=dev))
        assert torch.equal(solo["assign_score"][:, 0], res["assign_score"][:, j])
        assert int(solo["best_code"][0]) == int(res["best_code"][j]) and torch.equal(solo["coef"][0], res["coef"][j])


# ------------------------------------------------------------------------------------------------ 2, 3: the fused gradient
# frames, longest first: three workgroups of 5 tiles, one workgroup's 5 tiles plus a frame, exactly 5 tiles, a tile plus a frame,
# one tile, and 3 frames (every hop an edge hop)
GRAD_FRAMES = [163, 81, 80, 17, 16, 3]
# per utterance: None = the code the forward kernel chose (the true partition), or a forced code: 0 and 2^M - 1 leave one group
# empty, 0b0001 / 0b1110 (M = 4) and 0b001 (M = 3) make a three- or two-member group of estimates that belong apart
FORCED = {2: [None, 0, 3, None, 2, None], 3: [None, 0, 7, 1, None, 6], 4: [None, 0, 15, 1, 14, None]}


def _true_code(M):
    return {2: 0b10, 3: 0b101, 4: 0b0110}[M]


@functools.lru_cache(maxsize=None)
def _grad_case(M):
    """tests/_sisdr_oracle.py's ratio-mask construction with M sources; reference n = the sum of the sources of group n."""
    c = SO.ratio_mask_case([128 * (T - 1) + 64 for T in GRAD_FRAMES], M, seed=60 + M)
    assert [X.shape[1] for X in c["specs"]] == GRAD_FRAMES
    code, refs = _true_code(M), []
    for rs in c["refs_pcm"]:
        srcs = [rs[c["shuffle"].index(k)].astype(np.int32) for k in range(M)]       # refs_pcm[i] = source shuffle[i]
        refs.append([sum(s for k, s in enumerate(srcs) if ((code >> k) & 1) == n).astype(np.int16) for n in range(2)])
    return dict(specs=c["specs"], masks=c["masks"], refs_pcm=refs)


def _rows(c, dev, M, ld=None):
    from sepkern.packing import Packing
    ld = M * F if ld is None else ld
    pk = Packing([X.shape[1] for X in c["specs"]], dev)
    mixc = np.zeros((pk.Rp, F), dtype=np.complex64)
    mask = np.zeros((pk.Rp, ld), dtype=np.float32)
    for j, (X, m) in enumerate(zip(c["specs"], c["masks"])):
        T = X.shape[1]
        rows = pk.offs_host[:T].astype(np.int64) + j
        mixc[rows] = X.T
        mask[rows, :M * F] = m.transpose(2, 0, 1).reshape(T, M * F)
    return pk, torch.from_numpy(mixc).to(dev), torch.from_numpy(mask).to(dev)


def _dmask_rows(dm, pk, c, M):
    dm = dm.cpu().numpy()
    out = []
    for j, X in enumerate(c["specs"]):
        T = X.shape[1]
        rows = pk.offs_host[:T].astype(np.int64) + j
        out.append(dm[rows, :M * F].reshape(T, M, F).transpose(1, 2, 0))
    return out


def _device_forward(c, dev, M, as_float=False, count=None):
    """mask_istft_rows + mixit_fwd of a case -> everything sk_mixit_mask_grad takes."""
    from sepkern import ops
    pk, mixc, mask = _rows(c, dev, M)
    est, est_offs, offsets = ops.mask_istft_rows(mixc, mask, pk, M)
    L = [128 * (X.shape[1] - 1) for X in c["specs"]]
    pcm = np.concatenate([x[:L[j]] for j, xs in enumerate(c["refs_pcm"]) for x in xs])
    ref = torch.from_numpy(OS.pcm16_to_float(pcm) if as_float else pcm).to(dev)
    ro, at = [], 0
    for n in L:
        ro += [at, at + n]
        at += 2 * n
    ref_offs = _i64(ro, dev)
    count_dev = None if count is None else torch.full((1,), float(count), device=dev)
    res = ops.mixit_fwd(est, est_offs, ref, ref_offs, (pk.lens - 1) * 128, M, 128 * (pk.T - 1), TAU, count_dev)
    return dict(pk=pk, mixc=mixc, est=est, est_offs=est_offs, offsets=offsets, ref=ref, ref_offs=ref_offs, res=res, L=L)


def _forced(c, f, M, dev):
    """(codes, best_code tensor, coef tensor) with FORCED[M] applied: a forced utterance's coefficients are sepkern/mixit.py's
    for that code, from the device's own estimates, rounded to float32 as the kernel rounds its own."""
    from sepkern import mixit
    B = len(c["specs"])
    codes = [int(v) for v in f["res"]["best_code"].cpu()]
    coef = f["res"]["coef"].cpu().numpy().copy()
    est = f["est"].cpu().numpy()
    for j, force in enumerate(FORCED[M]):
        if force is None:
            continue
        es = [est[f["offsets"][j * M + k]:f["offsets"][j * M + k] + f["L"][j]] for k in range(M)]
        P, cc, G = mixit.sums(es, [OS.pcm16_to_float(x[:f["L"][j]]).astype(np.float64) for x in c["refs_pcm"][j]])
        den = mixit.errors(P, cc, G, force) + TAU * P
        coef[j] = mixit.KAPPA / (B * (den + mixit.EPS))
        codes[j] = force
    return codes, torch.tensor(codes, dtype=torch.int32, device=dev), torch.from_numpy(coef.astype(np.float32)).to(dev)


@functools.lru_cache(maxsize=None)
def _grad_oracle(M, codes):
    c = _grad_case(M)
    refs = [[OS.pcm16_to_float(x).astype(np.float64) for x in xs] for xs in c["refs_pcm"]]
    out = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        ms = [torch.tensor(m, dtype=dt, requires_grad=True) for m in c["masks"]]
        loss, scores, bests = MO.loss_from_masks(c["specs"], ms, refs, TAU, dtype=dt, force=list(codes))
        loss.backward()
        out[name] = [m.grad.double().numpy() for m in ms]
    free = MO.loss_from_masks(c["specs"], [torch.tensor(m, dtype=torch.float64) for m in c["masks"]], refs, TAU)
    return out, free[1], free[2]


def _rel(got, ref):
    g, r = np.concatenate([x.ravel() for x in got]), np.concatenate([x.ravel() for x in ref])
    return float(np.linalg.norm(g - r) / np.linalg.norm(r))


@pytest.mark.parametrize("as_float", [False, True], ids=["int16", "float32"])
@pytest.mark.parametrize("M", [2, 3, 4])
def test_mixit_mask_grad_against_fp64_autograd(dev, M, as_float):
    """Measured on an MI355X (relative L2 against torch fp64 autograd; kernel / the same graph in torch float32 on the CPU):
    see profiles/mixit_loss.txt, "mask gradient"."""
    from sepkern import ops
    c = _grad_case(M)
    f = _device_forward(c, dev, M, as_float)
    pk, B = f["pk"], len(GRAD_FRAMES)
    codes, best, coef = _forced(c, f, M, dev)
    orc, scores, free_best = _grad_oracle(M, tuple(codes))
    for j, s in enumerate(scores):        # the free search: a clear lead, the constructed code, and the kernel's choice
        top = np.sort(s.numpy())
        assert top[-1] - top[-2] > 1.0, (j, top[-1] - top[-2])
        assert free_best[j] == _true_code(M) == int(f["res"]["best_code"][j])
    one = torch.ones(1, device=dev)
    args = (f["est"], f["est_offs"], f["ref"], f["ref_offs"], best, coef)
    dm = ops.mixit_mask_grad(*args, one, f["mixc"], pk, M)
    assert dm.shape == (pk.Rp, M * F) and torch.isfinite(dm).all()
    got = _dmask_rows(dm, pk, c, M)
    err = _rel(got, orc["f64"])
    err32 = _rel(orc["f32"], orc["f64"])
    print("M=%d %s codes %s: dmask relative L2 vs fp64 autograd: kernel %.3g, torch float32 on the CPU %.3g (gate: 4 x)"
          % (M, "float32" if as_float else "int16", codes, err, err32))
    assert err <= 4.0 * err32
    # the column blocks of one group hold the same bits; two groups differ
    for j, code in enumerate(codes):
        for k in range(M):
            for l in range(k + 1, M):
                same = np.array_equal(got[j][k], got[j][l])
                assert same == (((code >> k) & 1) == ((code >> l) & 1)), (j, code, k, l)
    # tail rows of a fresh (Rp, .) buffer are zero; a second run gives the same bits; gscale scales linearly
    assert pk.Rp > pk.R and not dm[pk.R:].any()
    assert torch.equal(ops.mixit_mask_grad(*args, one, f["mixc"], pk, M), dm)
    dm3 = ops.mixit_mask_grad(*args, torch.full((1,), 2.5, device=dev), f["mixc"], pk, M)
    assert float((dm3 - 2.5 * dm).norm() / (2.5 * dm).norm()) <= 1e-6
    # a caller's buffer: a canary in the rows >= R and the columns >= M F is untouched, every valid element is written
    buf = torch.full((pk.Rp + 3, M * F + 3), 7.0, device=dev)
    ops.mixit_mask_grad(*args, one, f["mixc"], pk, M, out=buf)
    assert (buf[pk.R:] == 7.0).all() and (buf[:, M * F:] == 7.0).all()
    assert torch.equal(buf[:pk.R, :M * F], dm[:pk.R])
    # D = 0 gives exact zeros (a canary-filled buffer shows they were written)
    buf.fill_(7.0)
    ops.mixit_mask_grad(f["est"], f["est_offs"], f["ref"], f["ref_offs"], best, torch.zeros_like(coef), one, f["mixc"], pk, M, out=buf)
    assert not buf[:pk.R, :M * F].any() and (buf[pk.R:] == 7.0).all() and (buf[:, M * F:] == 7.0).all()
    # an utterance alone (with the batch's count) gives the bits it has inside the batch
    for j in (1, B - 1):
        solo_c = {k: [v[j]] for k, v in c.items()}
        s = _device_forward(solo_c, dev, M, as_float, count=B)
        assert torch.equal(s["res"]["coef"][0], f["res"]["coef"][j]) and int(s["res"]["best_code"][0]) == int(f["res"]["best_code"][j])
        dms = ops.mixit_mask_grad(s["est"], s["est_offs"], s["ref"], s["ref_offs"], best[j:j + 1].contiguous(), coef[j:j + 1].contiguous(),
                                  one, s["mixc"], s["pk"], M)
        assert np.array_equal(_dmask_rows(dms, s["pk"], solo_c, M)[0], got[j])


# ------------------------------------------------------------------------------------------------ 4: through the arch
ARCH_LENGTHS = [9000, 7400, 6000, 4800, 3900, 3000]
ARCH_CODE = 0b0110                        # reference 0 = estimates 0 + 3, reference 1 = estimates 1 + 2
# The references are sums of the untrained network's initial estimates plus band-limited noise this far below them.  Those
# estimates are alike (every mask is near 1/2), so exchanging two of them costs little: at 25 dB of noise the constructed code
# led the runner-up by the margins the test prints (CPU oracle), all above the 1 dB it asserts.
NOISE_DB = 25.0


def _arch_case(arch, M=4, H=64, L=2, seed=5):
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    model = arch.SepDNN(0, num_spk=str(M), hidden_dim=str(H), num_layers=str(L), loss="mixit")
    model.cuda()
    model.train()
    orc = OU.OracleSepDNN(num_spk=M, hidden_dim=H, num_layers=L)
    orc.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    orc.train()
    B = len(ARCH_LENGTHS)
    h0, c0 = torch.randn(2 * L, B, H), torch.randn(2 * L, B, H)
    mixes = [SO.to_pcm(np.sum(SO.band_sources(n, M, 700 + u), axis=0)) for u, n in enumerate(ARCH_LENGTHS)]
    specs = [OS.stft(OS.pcm16_to_float(m)) for m in mixes]
    packed = torch.nn.utils.rnn.pack_sequence([torch.from_numpy(np.abs(X).astype(np.float32).T.copy()) for X in specs])

    def masks_of(mask_out):
        return [mask_out[j, :X.shape[1]].reshape(X.shape[1], M, F).permute(1, 2, 0) for j, X in enumerate(specs)]

    with torch.no_grad():
        first, _ = orc(packed, (h0, c0))
    refs = []
    for X, m in zip(specs, masks_of(first)):
        es = [SO.istft_t(torch.as_tensor(X).to(torch.complex128) * m[k].double()).numpy() for k in range(M)]
        xs = []
        for n in range(2):
            x = sum(e for k, e in enumerate(es) if ((ARCH_CODE >> k) & 1) == n)
            noise = np.convolve(rng.standard_normal(x.shape[0] + 15), np.hanning(16), mode="valid")       # band-limited
            noise *= np.sqrt(np.mean(x ** 2) / np.mean(noise ** 2)) * 10.0 ** (-NOISE_DB / 20.0)
            xs.append(SO.to_pcm(x + noise))
        refs.append(xs)
    # (the extra forward pass moved the BatchNorm running statistics; the training-mode output does not read them)
    orc.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    return dict(model=model, orc=orc, h0=h0, c0=c0, mixes=mixes, specs=specs, packed=packed, refs=refs, masks_of=masks_of, M=M)


def _oracle_step(a):
    a["orc"].zero_grad()
    mask_out, _ = a["orc"](a["packed"], (a["h0"], a["c0"]))
    refs = [[OS.pcm16_to_float(x).astype(np.float64) for x in xs] for xs in a["refs"]]
    loss, scores, bests = MO.loss_from_masks(a["specs"], a["masks_of"](mask_out), refs, TAU)
    loss.backward()
    margins = [float(np.sort(s.numpy())[-1] - np.sort(s.numpy())[-2]) for s in scores]
    return float(loss.detach()), bests, margins


def _wav_batch(arch, a):
    samples = []
    for mix, xs in zip(a["mixes"], a["refs"]):
        L = 128 * (len(mix) // 128)
        d = {"mix": mix}
        for n, x in enumerate(xs):          # a reference has its mixture's length (the loss reads the first 128 (T - 1) samples)
            d["source%d" % (n + 1)] = np.concatenate([x[:L], np.zeros(len(mix) - L, np.int16)])
        samples.append(d)
    return arch.WavCollator()(samples)


def test_arch_loss_mixit_matches_oracle_network_and_fp64_loss(arch, dev):
    from sepkern.data import Prefetcher
    a = _arch_case(arch)
    lo, bests, margins = _oracle_step(a)
    assert all(m > 1.0 for m in margins), margins
    assert bests == [ARCH_CODE] * len(ARCH_LENGTHS)
    model, batch = a["model"], _wav_batch(arch, a)
    assert batch["pcm"]["lens"] == ARCH_LENGTHS and batch["pcm"]["keys"] == ["mix", "source1", "source2"]
    model.next_hidden = (a["h0"].cuda(), a["c0"].cuda())
    loss, norm = arch.compute_loss(model, 0, batch)
    loss.backward()
    grads = {k: p.grad.clone() for k, p in model.named_parameters()}
    lv = float(loss.detach())
    print("arch loss=mixit: loss %.6f dB (oracle %.6f), margins %s" % (lv, lo, ["%.1f" % m for m in margins]))
    assert float(norm) == len(ARCH_LENGTHS)
    assert model.last_best_code.cpu().tolist() == bests
    assert abs(lv - lo) <= 1e-5 * abs(lo)
    og = dict(a["orc"].named_parameters())
    worst = 0.0
    for k, g in grads.items():
        ref = og[k].grad.double()
        err = float((g.cpu().double() - ref).norm() / (ref.norm() + 1e-30))
        worst = max(worst, err)
        assert err < 2e-4, (k, err)
    print("arch loss=mixit: worst parameter-gradient relative L2 %.3g (gate 2e-4)" % worst)
    # the same batch staged by the prefetcher with the waveforms kept: bit-identical
    staged = list(Prefetcher([batch], dev, keep_wave=True))
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


def test_arch_loss_mixit_bf16_runs(arch, dev):
    """dtype=bf16 takes the same loss route (the loss reads the fp32 mask): finite, close to the fp32 model's loss."""
    a = _arch_case(arch)
    torch.manual_seed(5)
    m16 = arch.SepDNN(0, num_spk="4", hidden_dim="64", num_layers="2", loss="mixit", dtype="bf16")
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
    print("loss=mixit fp32 %.4f dB, bf16 %.4f dB" % tuple(out))
    assert np.isfinite(out[1]) and abs(out[1] - out[0]) < 1.0


def test_arch_refuses_what_mixit_cannot_use(arch, dev):
    a = _arch_case(arch)
    batch = _wav_batch(arch, a)
    with pytest.raises(ValueError, match="outside 2..4"):
        arch.SepDNN(0, num_spk="5", hidden_dim="64", num_layers="2", loss="mixit")
    with pytest.raises(ValueError, match="outside 2..4"):
        arch.SepDNN(0, num_spk="1", hidden_dim="64", num_layers="2", loss="mixit")
    model = a["model"]
    # a batch with one recording, and one with three
    one = arch.WavCollator()([{"mix": m, "source1": m} for m in a["mixes"]])
    with pytest.raises(ValueError, match="loss=mixit: the batch holds no waveform source2"):
        arch.compute_loss(model, 0, one)
    three = arch.WavCollator()([{"mix": m, "source1": m, "source2": m, "source3": m} for m in a["mixes"]])
    with pytest.raises(ValueError, match="exactly source1 and source2"):
        arch.compute_loss(model, 0, three)
    npz = arch.Collator("mix")([{"mix": np.ones((6, F), np.float32), "source1": np.ones((6, F), np.float32),
                                 "source2": np.ones((6, F), np.float32)}])
    with pytest.raises(ValueError, match="`loss=mixit` needs waveforms: train with `--wav-input`"):
        arch.compute_loss(model, 0, npz)
    assert batch["pcm"]["keys"] == ["mix", "source1", "source2"]


# ------------------------------------------------------------------------------------------------ 5: routes
def test_only_mixit_reaches_the_new_entry_points(arch, dev, monkeypatch):
    from sepkern import _lib
    calls = []
    real = _lib.call

    def spy(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    a = _arch_case(arch)
    batch = _wav_batch(arch, a)
    B = len(ARCH_LENGTHS)
    seen = {}
    for kind, S in (("mse", 2), ("sisdr", 2), ("mixit", 4)):
        torch.manual_seed(3)
        model = arch.SepDNN(0, num_spk=str(S), hidden_dim="64", num_layers="2", loss=kind)
        model.cuda()
        model.train()
        model.next_hidden = (torch.randn(4, B, 64, device=dev), torch.randn(4, B, 64, device=dev))
        del calls[:]
        loss, _ = arch.compute_loss(model, 0, batch)
        loss.backward()
        assert np.isfinite(float(loss.detach()))
        seen[kind] = list(calls)
    for kind in ("mse", "sisdr"):
        assert not [n for n in seen[kind] if n.startswith("sk_mixit")], (kind, seen[kind])
    assert "sk_pit_mse_fwd" in seen["mse"] and "sk_sisdr_pit_fwd" in seen["sisdr"]
    for name in ("sk_mask_istft_rows", "sk_mixit_fwd", "sk_mixit_mask_grad"):
        assert seen["mixit"].count(name) == 1, (name, seen["mixit"])
    assert not [n for n in seen["mixit"] if n.startswith("sk_sisdr") or n.startswith("sk_pit")]


def _corpus(root, rate=8000, n_session=4, n_rec=2):
    """A Kaldi-style directory of 8 unlabelled recordings: utt2spk names the SESSION a recording comes from -- what must not be
    mixed with itself."""
    import scipy.io.wavfile
    from sepkern import synth
    os.makedirs(os.path.join(root, "wav"), exist_ok=True)
    scp, u2s = [], []
    for p in range(n_session):
        for k in range(n_rec):
            n = int((0.4 + 0.05 * ((3 * p + 5 * k) % 9)) * rate)
            x = np.rint(synth.speech_like(n, 300 + 10 * p + k) * (0.3 + 0.1 * k) * 32768.0).astype(np.int16)
            utt, path = "ses%d_%d" % (p, k), os.path.join(root, "wav", "ses%d_%d.wav" % (p, k))
            scipy.io.wavfile.write(path, rate, x)
            scp.append("%s %s\n" % (utt, path))
            u2s.append("%s ses%d\n" % (utt, p))
    open(os.path.join(root, "wav.scp"), "w").write("".join(scp))
    open(os.path.join(root, "utt2spk"), "w").write("".join(u2s))
    return root


def test_driver_trains_on_unlabelled_recordings_and_a_restart_continues_exactly(arch, tmp_path, monkeypatch):
    """steps/train_qsub.py --dynamic-mix with loss=mixit, num_spk=4: every example is a mixture of TWO recordings, the losses
    are finite, and a run restarted with --start-epoch 1 ends on exactly the uninterrupted run's loss lines and weights."""
    import train_qsub
    monkeypatch.setattr(train_qsub, "CHECKPOINT_EVERY", 1)
    corpus = _corpus(os.path.join(str(tmp_path), "corpus"))
    seen = []
    real = arch.compute_loss

    def spy(model, epoch, batch, *a):
        seen.append((epoch, batch["pcm"]["keys"], model.num_spk, model.loss_kind))
        return real(model, epoch, batch, *a)
    monkeypatch.setattr(arch, "compute_loss", spy)
    conf = os.path.join(str(tmp_path), "conf")
    open(conf, "w").write("hidden_dim=64\nnum_layers=2\nnum_spk=4\nloss=mixit\n")
    straight, resumed = os.path.join(str(tmp_path), "straight"), os.path.join(str(tmp_path), "resumed")
    common = ["uPIT", "0", corpus, None, "--model-config", conf, "--wav-input", "--dynamic-mix", "--batch-size", "2",
              "--mixes-per-epoch", "4", "--mix-max-samples", "4000", "--seed", "5", "--num-workers", "0", "--prefetch", "0"]

    def argv(out, *more):
        return [out if a is None else a for a in common] + list(more)
    train_qsub.main(argv(straight, "--num-epochs", "2"))
    assert len(seen) == 4 and all(s[1:] == (["source1", "source2"], 4, "mixit") for s in seen)
    lines = open(os.path.join(straight, "train_stats", "train_loss.txt")).read().splitlines()
    assert len(lines) == 2 and lines[0].startswith("001 ") and lines[1].startswith("002 ")
    assert all(np.isfinite(float(l.split()[1])) for l in lines)
    os.makedirs(os.path.join(resumed, "intermediate_models"))
    os.makedirs(os.path.join(resumed, "train_stats"))
    for name in ("001.mdl", "001.opt"):
        shutil.copy(os.path.join(straight, "intermediate_models", name), os.path.join(resumed, "intermediate_models", name))
    open(os.path.join(resumed, "train_stats", "train_loss.txt"), "w").write(lines[0] + "\n")
    train_qsub.main(argv(resumed, "--num-epochs", "2", "--start-epoch", "1"))
    assert open(os.path.join(resumed, "train_stats", "train_loss.txt")).read().splitlines() == lines
    a = torch.load(os.path.join(straight, "final.mdl"), map_location="cpu")
    b = torch.load(os.path.join(resumed, "final.mdl"), map_location="cpu")
    assert all(torch.equal(a[k], b[k]) for k in a)
