"""Dynamic mixing on the MI355X: sk_dynamic_mix against the numpy fp64 statement of its rule (sepkern/mixing.py), the
properties its one-workgroup-per-mixture form promises (bits that depend on neither batch, run nor sample format; nothing
written outside the stated ranges), and the route from a DynMixCollator batch through the unchanged front ends, the prefetcher
and the training driver.

The kernel's shapes: B = 3 mixtures of 40 003 (many strides of the 1024 threads and an odd tail), 1 000 (less than one stride) and
257 samples (the STFT's shortest legal length), S = 2, 3, 4, int16 and float32 samples, sources that overlap in the sample
buffer.  Run with -s for the measured figures."""
import functools
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(PKG, "archs"))
sys.path.insert(0, os.path.join(PKG, "steps"))

LENGTHS = [40003, 1000, 257]
EPS = 2.0 ** -24


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
def _pool():
    """50 000 int16 samples: seeded Gaussian noise through a 4-tap moving average at level 0.1, with a slow envelope (so that
    stretches of the pool differ in power).  Shared, never written to."""
    rng = np.random.default_rng(2024)
    x = np.convolve(rng.standard_normal(50003), np.full(4, 0.25), mode="valid") * 0.1
    x *= 0.6 + 0.4 * np.sin(np.arange(50000) / 2900.0)
    x = np.rint(x * 32768.0)
    assert np.abs(x).max() < 32768
    return x.astype(np.int16)


def _offsets(S):
    """S lists of B = 3 source offsets into the pool: the sources of a mixture overlap, and so do those of different mixtures."""
    return [[3001 * s, 100 + 333 * s, 45000 + 100 * s] for s in range(S)]


def _levels(S):
    amp = [[float(np.float32(10.0 ** (db / 20.0))) for db in (2.5 - s, -1.0 + 0.7 * s, 0.3 * s)] for s in range(S)]
    return amp, [0.9, 0.5, 0.73]


@functools.lru_cache(maxsize=None)
def _reference(S):
    """mixing.py in fp64 for the three mixtures: [(mixture, [sources], G)] -- computed once, shared, never written to."""
    from sepkern import mixing
    amp, peak = _levels(S)
    offs, pool = _offsets(S), _pool()
    return [mixing.mix([pool[offs[s][u]:offs[s][u] + n] for s in range(S)], [amp[s][u] for s in range(S)], peak[u])
            for u, n in enumerate(LENGTHS)]


def _pool_tensor(dtype, dev):
    p = _pool()
    return torch.from_numpy(p if dtype == "int16" else (p.astype(np.float32) / np.float32(32768.0))).to(dev)


def _run(S, dtype, dev, quantize=False, which=(0, 1, 2)):
    from sepkern import ops
    amp, peak = _levels(S)
    offs = _offsets(S)
    out, gains = ops.dynamic_mix(_pool_tensor(dtype, dev), [[offs[s][u] for u in which] for s in range(S)], [LENGTHS[u] for u in which],
                                 [[amp[s][u] for u in which] for s in range(S)], [peak[u] for u in which], quantize=quantize)
    torch.cuda.synchronize()
    return out, gains


def _signal(out, q, u, lens):
    total, starts = sum(lens), np.concatenate([[0], np.cumsum(lens)[:-1]])
    a = q * total + int(starts[u])
    return out[a:a + lens[u]]


# ------------------------------------------------------------------------------------------------ 1: against the fp64 statement
@pytest.mark.parametrize("S", [2, 3, 4])
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_kernel_against_mixing_py(S, dtype, dev):
    """Every source sample within (S + 6) 2^-24 peak, every mixture sample within S (2 S + 6) 2^-24 peak, every gain within
    (S + 5) 2^-24 relative: first-order bounds of the kernel's stated fp32 arithmetic (three roundings each on g and G, S + 1 in
    the fp32 maximum the scale divides by, one per product, S in the chain)."""
    out, gains = _run(S, dtype, dev)
    assert out.dtype == torch.float32 and out.numel() == (S + 1) * sum(LENGTHS) and gains.shape == (S, 3)
    out, gains = out.cpu().numpy().astype(np.float64), gains.cpu().numpy().astype(np.float64)
    _, peak = _levels(S)
    for u, (mix, srcs, G) in enumerate(_reference(S)):
        e_g = float(np.abs(gains[:, u] / G - 1.0).max())
        e_s = max(float(np.abs(_signal(out, 1 + s, u, LENGTHS) - srcs[s]).max()) for s in range(S))
        e_m = float(np.abs(_signal(out, 0, u, LENGTHS) - mix).max())
        top = max(np.abs(_signal(out, q, u, LENGTHS)).max() for q in range(S + 1))
        print("S=%d %s n=%5d: gains %.2f of (S+5) eps, sources %.2f of (S+6) eps peak, mixture %.2f of S(2S+6) eps peak, largest |.| / peak - 1 = %.1e"
              % (S, dtype, LENGTHS[u], e_g / ((S + 5) * EPS), e_s / ((S + 6) * EPS * peak[u]), e_m / (S * (2 * S + 6) * EPS * peak[u]),
                 top / peak[u] - 1.0))
        assert e_g <= (S + 5) * EPS
        assert e_s <= (S + 6) * EPS * peak[u]
        assert e_m <= S * (2 * S + 6) * EPS * peak[u]
        assert abs(top / peak[u] - 1.0) <= (S + 6) * EPS


# ------------------------------------------------------------------------------------------------ 2: quantize
@pytest.mark.parametrize("S", [2, 3])
def test_quantize_is_the_rule_applied_to_the_kernels_own_result(S, dev):
    from sepkern.data import features_from_pcm
    plain, g0 = _run(S, "int16", dev)
    quant, g1 = _run(S, "int16", dev, quantize=True)
    v = plain.cpu().numpy()
    want = (np.clip(np.rint(v * np.float32(32768.0)), -32768.0, 32767.0) / np.float32(32768.0)).astype(np.float32)
    assert np.array_equal(quant.cpu().numpy(), want) and torch.equal(g0, g1)
    assert not torch.equal(plain, quant)
    # on the int16 grid: as int16 PCM the batch gives the front end the bits the float form gives it
    k = quant * 32768.0
    assert torch.equal(k, k.round()) and float(k.abs().max()) <= 32767
    keys = ["mix"] + ["source%d" % (s + 1) for s in range(S)]
    a = features_from_pcm({"flat": quant, "keys": keys, "lens": LENGTHS}, dev)
    b = features_from_pcm({"flat": k.to(torch.int16), "keys": keys, "lens": LENGTHS}, dev)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1])) and len(a[1]) == S


# ------------------------------------------------------------------------------------------------ 3: what the bits do not depend on
@pytest.mark.parametrize("S", [2, 4])
def test_bits_do_not_depend_on_batch_run_or_sample_format(S, dev):
    out, gains = _run(S, "int16", dev)
    again, gains2 = _run(S, "int16", dev)
    assert torch.equal(out, again) and torch.equal(gains, gains2)
    asfloat, gains3 = _run(S, "float32", dev)
    assert torch.equal(out, asfloat) and torch.equal(gains, gains3)
    for u in range(3):
        alone, g = _run(S, "int16", dev, which=(u,))
        for q in range(S + 1):
            assert torch.equal(_signal(alone, q, 0, [LENGTHS[u]]), _signal(out, q, u, LENGTHS)), (u, q)
        assert torch.equal(g[:, 0], gains[:, u])


# ------------------------------------------------------------------------------------------------ 4: only the stated ranges are written
@pytest.mark.parametrize("quantize", [False, True])
def test_only_the_stated_ranges_of_out_are_written(quantize, dev):
    import ctypes as C
    from sepkern import _lib
    S, B, gap, canary = 3, 3, 5, 777.0
    amp, peak = _levels(S)
    offs = _offsets(S)
    want, _ = _run(S, "float32", dev, quantize=quantize)
    # signals in another order than the dense layout's, `gap` floats of canary before, between and after them
    order = [(q, u) for u in range(B) for q in range(S + 1)]
    out_offs, at = {}, gap
    for q, u in order:
        out_offs[(q, u)] = at
        at += LENGTHS[u] + gap
    buf = torch.full((at,), canary, device=dev)
    d64 = torch.tensor([offs[s][u] for s in range(S) for u in range(B)] + [out_offs[(q, u)] for q in range(S + 1) for u in range(B)],
                       dtype=torch.int64, device=dev)
    d_ns = torch.tensor(LENGTHS, dtype=torch.int32, device=dev)
    d_f = torch.tensor([a for row in amp for a in row] + peak, dtype=torch.float32, device=dev)
    pool = _pool_tensor("float32", dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    _lib.call("sk_dynamic_mix", p(pool), 0, p(d64), p(d_ns), B, S, p(d_f), p(d_f[S * B:]), int(quantize), p(buf), p(d64[S * B:]), None,
              C.c_void_p(torch.cuda.current_stream().cuda_stream))           # gains = NULL
    torch.cuda.synchronize()
    written = torch.zeros(at, dtype=torch.bool, device=dev)
    for (q, u), o in out_offs.items():
        assert torch.equal(buf[o:o + LENGTHS[u]], _signal(want, q, u, LENGTHS)), (q, u)
        written[o:o + LENGTHS[u]] = True
    assert int((~written).sum()) == gap * (len(order) + 1) and bool((buf[~written] == canary).all())
    assert torch.equal(pool, _pool_tensor("float32", dev))                  # the samples are read only


# ------------------------------------------------------------------------------------------------ 5: silence
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_silent_sources(dtype, dev):
    from sepkern import ops
    n = 1500
    flat = torch.cat([_pool_tensor(dtype, dev)[:2 * n], torch.zeros(n, dtype=torch.int16 if dtype == "int16" else torch.float32, device=dev)])
    # mixture 0: sources (live, silent, live); mixture 1: all silent; mixture 2: (silent, live, live)
    offs = [[0, 2 * n, 2 * n], [2 * n, 2 * n, n], [n, 2 * n, 0]]
    out, gains = ops.dynamic_mix(flat, offs, [n, n, n], [[1.0, 1.0, 1.0]] * 3, [0.9, 0.9, 0.8])
    out, gains = out.cpu(), gains.cpu()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gains).all())
    lens = [n, n, n]
    assert gains[1, 0] == 0 and not _signal(out, 2, 0, lens).any() and gains[0, 0] > 0 and gains[2, 0] > 0
    assert abs(float(max(_signal(out, q, 0, lens).abs().max() for q in range(4))) / 0.9 - 1.0) <= 9 * EPS
    assert not gains[:, 1].any() and not any(_signal(out, q, 1, lens).any() for q in range(4))
    assert gains[0, 2] == 0 and not _signal(out, 1, 2, lens).any()
    assert abs(float(max(_signal(out, q, 2, lens).abs().max() for q in range(4))) / 0.8 - 1.0) <= 9 * EPS


def test_ops_checks_its_arguments(dev):
    from sepkern import ops, _lib
    flat = _pool_tensor("int16", dev)
    ok = dict(src_offs=[[0, 10], [5, 20]], nsamp=[300, 400], amp=[[1, 1], [1, 1]], peak=[0.9, 0.9])
    ops.dynamic_mix(flat, **ok)
    for bad in (dict(src_offs=[[0, 49800], [5, 20]]), dict(amp=[[1, 1]]), dict(peak=[0.9]), dict(nsamp=[300, 0]),
                dict(src_offs=[[0, 10]] * 5, amp=[[1, 1]] * 5), dict(src_offs=[[0], [5]])):
        with pytest.raises(_lib.SepkernError):
            ops.dynamic_mix(flat, **dict(ok, **bad))
    with pytest.raises(_lib.SepkernError):
        ops.dynamic_mix(flat.cpu(), **ok)


# ------------------------------------------------------------------------------------------------ 6: through the front ends
def _corpus(root, rate=8000, n_spk=6, n_utt=3):
    """A Kaldi-style directory of single-speaker files: n_spk speakers x n_utt utterances of 0.4 .. 1.1 s of sepkern.synth's
    speech-like noise."""
    import scipy.io.wavfile
    from sepkern import synth
    os.makedirs(os.path.join(root, "wav"), exist_ok=True)
    scp, u2s = [], []
    for p in range(n_spk):
        for k in range(n_utt):
            n = int((0.4 + 0.04 * ((7 * p + 5 * k) % 18)) * rate)
            x = np.rint(synth.speech_like(n, 100 * p + k) * (0.3 + 0.1 * k) * 32768.0).astype(np.int16)
            utt, path = "spk%d_%d" % (p, k), os.path.join(root, "wav", "spk%d_%d.wav" % (p, k))
            scipy.io.wavfile.write(path, rate, x)
            scp.append("%s %s\n" % (utt, path))
            u2s.append("%s spk%d\n" % (utt, p))
    open(os.path.join(root, "wav.scp"), "w").write("".join(scp))
    open(os.path.join(root, "utt2spk"), "w").write("".join(u2s))
    return root


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return _corpus(str(tmp_path_factory.mktemp("dynmix")))


def _mixed_by_hand(pcm, dev):
    """The ordinary pcm batch (host float32, keys mix / source1 ..) that ops.dynamic_mix makes of a DynMixCollator batch."""
    from sepkern import ops
    ns, S = pcm["lens"], len(pcm["keys"])
    total, starts = sum(ns), [sum(ns[:j]) for j in range(len(ns))]
    out, _ = ops.dynamic_mix(pcm["flat"].to(dev), [[s * total + st for st in starts] for s in range(S)], ns, pcm["mixing"]["amp"],
                             pcm["mixing"]["peak"], quantize=pcm["mixing"]["quantize"])
    return {"flat": out.cpu(), "keys": ["mix"] + pcm["keys"], "lens": ns}


def _same_staged(a, b):
    assert sorted(k for k in a if k != "_keepalive") == sorted(k for k in b if k != "_keepalive")
    (m0, s0, p0), (m1, s1, p1) = a["packed"], b["packed"]
    assert torch.equal(m0, m1) and len(s0) == len(s1) and all(torch.equal(x, y) for x, y in zip(s0, s1))
    assert torch.equal(p0.lens, p1.lens) and p0.R == p1.R
    if "wave" in a:
        assert torch.equal(a["wave"]["mixc"], b["wave"]["mixc"]) and torch.equal(a["wave"]["flat"], b["wave"]["flat"])
        assert a["wave"]["nsamp"] == b["wave"]["nsamp"] and a["wave"]["sig_offs"] == b["wave"]["sig_offs"]


@pytest.mark.parametrize("quantize", [False, True])
def test_the_front_ends_are_reused_unchanged(quantize, arch, corpus, dev):
    from sepkern.data import Prefetcher
    ds = arch.DynMixTrainSet(corpus, 2, seed=3, snr_db=2.5, peak=(0.5, 0.9), quantize=quantize)
    batch = ds.collator([ds[i] for i in range(5)])
    byhand = {"pcm": _mixed_by_hand(batch["pcm"], dev)}
    for kw in (dict(), dict(targets="psa"), dict(keep_wave=True)):
        got = Prefetcher.stage(batch, dev, **kw)
        want = Prefetcher.stage(byhand, dev, **kw)
        torch.cuda.synchronize()
        assert "pcm" not in got and got["packed"][2].B == 5 and len(got["packed"][1]) == (0 if kw.get("keep_wave") else 2)
        _same_staged(got, want)
    # the whole prefetcher (its thread, its stream) hands over the same batch
    it = list(Prefetcher([batch], dev))
    _same_staged(it[0], Prefetcher.stage(byhand, dev))


def test_a_batch_without_mixing_never_reaches_the_new_entry_point(arch, corpus, dev, monkeypatch):
    from sepkern import _lib
    from sepkern.data import Prefetcher
    calls = []
    real = _lib.call

    def spy(name, *args):
        calls.append(name)
        return real(name, *args)
    ds = arch.DynMixTrainSet(corpus, 2, seed=3)
    batch = ds.collator([ds[i] for i in range(4)])
    byhand = {"pcm": _mixed_by_hand(batch["pcm"], dev)}
    monkeypatch.setattr(_lib, "call", spy)
    for kw in (dict(), dict(targets="tpsa"), dict(keep_wave=True)):
        del calls[:]
        Prefetcher.stage(byhand, dev, **kw)
        assert "sk_dynamic_mix" not in calls and ("sk_stft_psa" in calls or "sk_stft" in calls)
        del calls[:]
        Prefetcher.stage(batch, dev, **kw)
        assert calls[0] == "sk_dynamic_mix" and calls.count("sk_dynamic_mix") == 1


def test_a_16k_corpus_is_resampled_in_front_of_the_kernel(arch, dev, tmp_path, monkeypatch):
    from sepkern import _lib, ops
    from sepkern.data import features_from_pcm
    ds = arch.DynMixTrainSet(_corpus(str(tmp_path), rate=16000, n_spk=3, n_utt=2), 2, seed=1, sample_rate=8000)
    pcm = ds.collator([ds[i] for i in range(3)])["pcm"]
    assert pcm["rate"] == [16000] * 3 and pcm["target_rate"] == 8000
    calls = []
    real = _lib.call

    def spy(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    mix, srcs, pk = features_from_pcm(pcm, dev)
    assert [c for c in calls if c in ("sk_resample", "sk_dynamic_mix")] == ["sk_resample", "sk_dynamic_mix"]
    assert calls.index("sk_dynamic_mix") < calls.index("sk_stft")
    monkeypatch.setattr(_lib, "call", real)
    ns16, S = pcm["lens"], 2
    at8k, outs = ops.pcm_to_rate(pcm["flat"].to(dev), ns16 * S, [16000] * (3 * S), 8000)
    ns = outs[:3]
    assert ns == [-(-n // 2) for n in ns16] == outs[3:] and pk.lens_host.tolist() == [1 + n // 128 for n in ns]
    total, starts = sum(ns), [sum(ns[:j]) for j in range(3)]
    out, _ = ops.dynamic_mix(at8k, [[s * total + st for st in starts] for s in range(S)], ns, pcm["mixing"]["amp"], pcm["mixing"]["peak"])
    rmix, rsrcs, _ = features_from_pcm({"flat": out, "keys": ["mix", "source1", "source2"], "lens": ns}, dev)
    assert torch.equal(mix, rmix) and all(torch.equal(a, b) for a, b in zip(srcs, rsrcs)) and float(mix[:pk.R].min()) > 0


# ------------------------------------------------------------------------------------------------ 7: training on it
def test_twenty_steps_on_dynamic_batches_descend(arch, corpus, dev):
    """Twenty fused clip + Adam steps of loss=mse, every one on a freshly drawn batch, with fixed (h0, c0): the mean of the last
    five losses is below the mean of the first five (-s prints the curve)."""
    from sepkern.dist import MixDraws
    from sepkern.optim import ClipAdam
    from torch.utils.data import DataLoader
    ds = arch.DynMixTrainSet(corpus, 2, seed=11, mixes_per_epoch=16)
    draws = MixDraws(ds.mixes_per_epoch, 4, 0, 1)
    loader = DataLoader(ds, batch_sampler=draws, collate_fn=ds.collator, num_workers=0)
    torch.manual_seed(11)
    model = arch.SepDNN(0, hidden_dim="64", num_layers="2", loss="mse")
    model.cuda()
    model.train()
    opt = ClipAdam(model, lr=1e-3, max_norm=0.25)
    h0, c0 = torch.randn(4, 4, 64, device=dev), torch.randn(4, 4, 64, device=dev)
    curve, firsts = [], []
    for epoch in range(5):
        draws.set_epoch(epoch)
        for k, batch in enumerate(loader):
            if k == 0:
                firsts.append(batch["pcm"]["flat"][:257].clone())
            model.next_hidden = (h0, c0)
            loss, _ = arch.compute_loss(model, epoch, batch)
            loss.backward()
            opt.step()
            curve.append(float(loss.detach()))
    print("twenty steps on dynamic batches: " + " ".join("%.5f" % v for v in curve))
    assert len(curve) == 20 and all(np.isfinite(curve)) and int(opt.scal[3]) == 0
    assert not any(torch.equal(firsts[0], f) for f in firsts[1:])
    assert np.mean(curve[-5:]) < np.mean(curve[:5])


def test_driver_epochs_differ_and_a_restart_continues_exactly(arch, corpus, tmp_path, monkeypatch):
    """Two epochs of steps/train_qsub.py --dynamic-mix --seed: the epochs' first batches differ, and a run restarted with
    --start-epoch 1 from the first epoch's checkpoint ends its second epoch on exactly the uninterrupted run's loss and weights
    (the existing resume test's property, on this path; the driver's checkpoint cadence is set to every epoch for it)."""
    import train_qsub
    monkeypatch.setattr(train_qsub, "CHECKPOINT_EVERY", 1)
    seen = {}
    real = arch.compute_loss

    def spy(model, epoch, batch, *a):
        seen.setdefault(epoch, batch["pcm"])
        return real(model, epoch, batch, *a)
    monkeypatch.setattr(arch, "compute_loss", spy)
    conf = os.path.join(str(tmp_path), "conf")
    open(conf, "w").write("hidden_dim=64\nnum_layers=2\nnum_spk=2\n")
    straight, resumed = os.path.join(str(tmp_path), "straight"), os.path.join(str(tmp_path), "resumed")
    common = ["uPIT", "0", corpus, None, "--model-config", conf, "--wav-input", "--dynamic-mix", "--batch-size", "3",
              "--mixes-per-epoch", "6", "--mix-max-samples", "4000", "--seed", "5", "--num-workers", "0", "--prefetch", "0"]

    def argv(out, *more):
        return [out if a is None else a for a in common] + list(more)
    train_qsub.main(argv(straight, "--num-epochs", "2"))
    assert sorted(seen) == [0, 1] and seen[0]["keys"] == ["source1", "source2"] and "mixing" in seen[0]
    assert seen[0]["lens"] != seen[1]["lens"] or not torch.equal(seen[0]["flat"], seen[1]["flat"])
    assert seen[0]["mixing"]["amp"] != seen[1]["mixing"]["amp"]
    lines = open(os.path.join(straight, "train_stats", "train_loss.txt")).read().splitlines()
    assert len(lines) == 2 and lines[0].startswith("001 ") and lines[1].startswith("002 ")
    # the restart: the first epoch's checkpoint, optimizer state and loss line, then epoch 2 alone
    os.makedirs(os.path.join(resumed, "intermediate_models"))
    os.makedirs(os.path.join(resumed, "train_stats"))
    for name in ("001.mdl", "001.opt"):
        shutil.copy(os.path.join(straight, "intermediate_models", name), os.path.join(resumed, "intermediate_models", name))
    open(os.path.join(resumed, "train_stats", "train_loss.txt"), "w").write(lines[0] + "\n")
    first_of_epoch_2 = seen.pop(1)
    train_qsub.main(argv(resumed, "--num-epochs", "2", "--start-epoch", "1"))
    assert torch.equal(seen[1]["flat"], first_of_epoch_2["flat"]) and seen[1]["mixing"] == first_of_epoch_2["mixing"]
    assert open(os.path.join(resumed, "train_stats", "train_loss.txt")).read().splitlines() == lines
    a = torch.load(os.path.join(straight, "final.mdl"), map_location="cpu")
    b = torch.load(os.path.join(resumed, "final.mdl"), map_location="cpu")
    assert all(torch.equal(a[k], b[k]) for k in a)
