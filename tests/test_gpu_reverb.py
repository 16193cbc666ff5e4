"""Reverberant dynamic mixing on the MI355X: sk_fir_convolve against the fp64 definition (sepkern/reverb.py) inside a bound that
comes from the float32 restatement's own error, the properties its two-launch form promises (bits that depend on neither batch,
run nor sample format; nothing written outside the stated ranges), and the route from a DynMixCollator batch with 'reverb'
through the unchanged front ends and the training driver.

ONE launch of 14 jobs over one shared pool: signals of 257 (two blocks, the second of one sample), 1 000 (under one 16-block
tile), 4 355 (17 blocks + 3: crosses a tile) and 9 000 samples (more blocks than any RIR has partitions); RIRs of 1 (the identity),
256 (exactly one partition), 257 (a second partition of one tap), 700, 4 097 (more partitions than a tile has blocks) and 8 192
taps (the maximum; longer than most of the signals); delays 0, 256, 300 and L - 1; two jobs share a signal, two share a RIR.
tests/test_reverb.py shows that one wrong partition, block or delay at such shapes is at least 100 times outside the bound.
Run with -s for the measured ratios."""
import ctypes as C
import functools
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from conftest import PKG
import _reverb_cases as rc

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(PKG, "archs"))
sys.path.insert(0, os.path.join(PKG, "steps"))

TAPS = [1, 256, 257, 700, 4097, 8192]
# (signal offset in the pool, samples, taps, delay)
JOBS = [(0, 257, 1, 0), (100, 257, 8192, 8191), (300, 1000, 256, 0), (300, 1000, 257, 256), (1500, 1000, 700, 300),
        (2600, 4355, 4097, 0), (7000, 4355, 700, 699), (500, 4355, 257, 0), (3000, 9000, 8192, 300), (2000, 9000, 4097, 4096),
        (1000, 9000, 1, 0), (7100, 4355, 256, 255), (50, 257, 700, 256), (4000, 1000, 4097, 256)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def arch(dev):
    import uPIT
    return uPIT


def test_the_jobs_are_the_shapes_the_docstring_names():
    assert {n for _, n, _, _ in JOBS} == {257, 1000, 4355, 9000} and {L for _, _, L, _ in JOBS} == set(TAPS)
    assert {0, 256, 300} <= {d for _, _, _, d in JOBS} and sum(d == L - 1 and L > 1 for _, _, L, d in JOBS) >= 4
    assert all(0 <= d < L and o + n <= len(rc.pool()) for o, n, L, d in JOBS)
    assert JOBS[2][:2] == JOBS[3][:2] and JOBS[3][2] == JOBS[7][2]              # a shared signal, a shared RIR


@functools.lru_cache(maxsize=None)
def _rir_pool():
    """(all RIRs back to back, {taps: offset}).  Shared, never written to."""
    offs, at = {}, 0
    for L in TAPS:
        offs[L] = at
        at += L
    flat = np.concatenate([rc.rir(L) for L in TAPS])
    flat.setflags(write=False)
    return flat, offs


@functools.lru_cache(maxsize=None)
def _reference(j):
    """Job j: (the fp64 definition, the bound 2 max(e32, 2^-24 ||h|| max|x|), e32 in units of the gate).  e32 is the float32
    restatement's own error on this job: the yardstick is numpy's arithmetic, never the kernel's.  Computed once, shared."""
    from sepkern import reverb
    o, n, L, d = JOBS[j]
    x, h = rc.signal(n, o), rc.rir(L)
    want = reverb.convolve(x, h, d)
    e32 = float(np.abs(reverb.convolve_partitioned_f32(x, h, d).astype(np.float64) - want).max())
    g = rc.gate(x, h)
    want.setflags(write=False)
    return want, 2.0 * max(e32, g), e32 / g


def _pool_tensor(dtype, dev):
    p = rc.pool()
    return torch.from_numpy(p.copy() if dtype == "int16" else (p.astype(np.float32) / np.float32(32768.0))).to(dev)


def _run(dtype, dev, which=None):
    from sepkern import ops
    which = list(range(len(JOBS))) if which is None else list(which)
    rirs, roffs = _rir_pool()
    out, offs = ops.fir_convolve(_pool_tensor(dtype, dev), [JOBS[j][0] for j in which], [JOBS[j][1] for j in which],
                                 torch.from_numpy(rirs.copy()).to(dev), [roffs[JOBS[j][2]] for j in which], [JOBS[j][2] for j in which],
                                 [JOBS[j][3] for j in which])
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.numel() == sum(JOBS[j][1] for j in which) and len(offs) == len(which)
    return out, offs


@pytest.fixture(scope="module")
def batch16(dev):
    return _run("int16", dev)


# ------------------------------------------------------------------------------------------------ 1: against the definition
def test_every_job_is_within_twice_the_float32_restatements_error(batch16):
    """max|y - convolve_fp64| <= 2 max(e32, 2^-24 ||h||_2 max|x|) for every job; the factor 2 is for the kernel's 16 x 16 radix-4
    factorisation and its fused multiply-adds rounding differently from pocketfft."""
    out, offs = batch16
    y = out.cpu().numpy().astype(np.float64)
    worst = []
    for j, (o, n, L, d) in enumerate(JOBS):
        want, bound, e32 = _reference(j)
        err = float(np.abs(y[offs[j]:offs[j] + n] - want).max())
        g = rc.gate(rc.signal(n, o), rc.rir(L))
        print("job %2d n=%4d L=%4d d=%4d: kernel %.2f, float32 restatement %.2f of 2^-24 |h| max|x|; %.2f of the bound"
              % (j, n, L, d, err / g, e32, err / bound))
        worst.append(err / bound)
    assert np.isfinite(y).all() and max(worst) <= 1.0, worst


def test_the_identity_rir_returns_the_signal(batch16):
    out, offs = batch16
    for j in (0, 10):
        o, n, L, d = JOBS[j]
        x = rc.signal(n, o)
        assert (L, d) == (1, 0)
        err = float((out[offs[j]:offs[j] + n].cpu().double() - torch.from_numpy(x.astype(np.float64) / 32768.0)).abs().max())
        assert err <= _reference(j)[1] <= 16.0 * rc.gate(x, [1.0])


# ------------------------------------------------------------------------------------------------ 2: what the bits do not depend on
def test_bits_do_not_depend_on_batch_run_or_sample_format(batch16, dev):
    out, offs = batch16
    again, _ = _run("int16", dev)
    assert torch.equal(out, again)
    asfloat, _ = _run("float32", dev)
    assert torch.equal(out, asfloat)
    for j, (o, n, L, d) in enumerate(JOBS):
        alone, a = _run("int16", dev, which=(j,))
        assert a == [0] and torch.equal(alone, out[offs[j]:offs[j] + n]), j
    # another batch around a job, in another order
    some = [13, 5, 1, 8]
    part, po = _run("float32", dev, which=some)
    for q, j in enumerate(some):
        assert torch.equal(part[po[q]:po[q] + JOBS[j][1]], out[offs[j]:offs[j] + JOBS[j][1]]), j


# ------------------------------------------------------------------------------------------------ 3: only the stated ranges are written
def test_only_the_stated_ranges_of_out_are_written(batch16, dev):
    from sepkern import _lib
    want, offs = batch16
    J, gap, canary = len(JOBS), 5, 777.0
    order = list(reversed(range(J)))                     # outputs in another order than the jobs', canaries before, between, after
    out_offs, at = {}, gap
    for j in order:
        out_offs[j] = at
        at += JOBS[j][1] + gap
    buf = torch.full((at,), canary, device=dev)
    rirs, roffs = _rir_pool()
    pool, d_rir = _pool_tensor("float32", dev), torch.from_numpy(rirs.copy()).to(dev)
    i64 = lambda v: (C.c_int64 * J)(*v)  # noqa: E731
    i32 = lambda v: (C.c_int32 * J)(*v)  # noqa: E731
    ns, taps, delay = i32([j[1] for j in JOBS]), i32([j[2] for j in JOBS]), i32([j[3] for j in JOBS])
    nbytes = _lib.load().sk_fir_workspace_bytes(ns, taps, delay, J)
    assert nbytes > 0
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    ws[nbytes:] = 0x5A
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    _lib.call("sk_fir_convolve", p(pool), 0, i64([j[0] for j in JOBS]), ns, p(d_rir), i64([roffs[j[2]] for j in JOBS]), taps, delay, J,
              p(ws), p(buf), i64([out_offs[j] for j in range(J)]), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    written = torch.zeros(at, dtype=torch.bool, device=dev)
    for j in range(J):
        n = JOBS[j][1]
        assert torch.equal(buf[out_offs[j]:out_offs[j] + n], want[offs[j]:offs[j] + n]), j
        written[out_offs[j]:out_offs[j] + n] = True
    assert int((~written).sum()) == gap * (J + 1) and bool((buf[~written] == canary).all())
    assert bool((ws[nbytes:] == 0x5A).all())                                       # the workspace is as large as the query says
    assert torch.equal(pool, _pool_tensor("float32", dev)) and torch.equal(d_rir.cpu(), torch.from_numpy(rirs.copy()))


def test_ops_checks_its_arguments(dev):
    from sepkern import ops, _lib
    flat, rirs = _pool_tensor("int16", dev), torch.from_numpy(_rir_pool()[0].copy()).to(dev)
    ok = dict(in_offs=[0, 10], ns=[300, 400], rir_offs=[0, 1], taps=[1, 256], delay=[0, 255])
    ops.fir_convolve(flat, rir_flat=rirs, **ok)
    for bad in (dict(in_offs=[0, 11900]), dict(ns=[300, 0]), dict(taps=[1, 20000]), dict(delay=[0, 256]), dict(delay=[1, 0]),
                dict(taps=[1, 8193], rir_offs=[0, 0]), dict(rir_offs=[0]), dict(rir_offs=[-1, 0])):
        with pytest.raises(_lib.SepkernError):
            ops.fir_convolve(flat, rir_flat=rirs, **dict(ok, **bad))
    with pytest.raises(_lib.SepkernError):
        ops.fir_convolve(flat.cpu(), rir_flat=rirs, **ok)
    with pytest.raises(_lib.SepkernError):
        ops.fir_convolve(flat, rir_flat=rirs.double(), **ok)


# ------------------------------------------------------------------------------------------------ 4: the route
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return str(tmp_path_factory.mktemp("reverb"))            # _items writes one small tree per length below it


def _items(arch, corpus):
    """Three items of 4 355, 1 000 and 257 samples (each from a set whose speakers all have that length), S = 2, synthetic RIRs."""
    items = []
    for k, n in enumerate((4355, 1000, 257)):
        root = rc.corpus(os.path.join(corpus, "n%d" % n), n_spk=2, n_utt=1, lengths=[n, n])
        ds = arch.DynMixTrainSet(root, 2, seed=3 + k, peak=(0.5, 0.9), rir_synth=(0.05, 0.3))
        items.append(ds[k])
        assert len(items[-1]["source1"]) == n and len(items[-1]["rir1"]) >= 400
    return items


def test_a_reverberant_batch_through_the_front_end_is_the_rule_on_the_definition(arch, corpus, dev):
    """mixed_pcm's mixture and sources against mixing.mix of reverb.convolve of the dry sources, both fp64.  Bounds: dynamic
    mixing's own ((S + 6) 2^-24 peak per source sample, S (2 S + 6) 2^-24 peak per mixture sample) plus the convolution's gate
    2 max(e32, 2^-24 ||h|| max|x|) of each source scaled by that source's gain."""
    from sepkern import mixing, reverb
    from sepkern.data import features_from_pcm, mixed_pcm
    items = _items(arch, corpus)
    pcm = arch.DynMixCollator()(items)["pcm"]
    assert pcm["lens"] == [4355, 1000, 257] and "reverb" in pcm
    got = mixed_pcm(pcm, dev)
    torch.cuda.synchronize()
    assert got["keys"] == ["mix", "source1", "source2"] and got["lens"] == pcm["lens"]
    flat, total, S = got["flat"].cpu().numpy().astype(np.float64), sum(pcm["lens"]), 2
    at = 0
    for u, it in enumerate(items):
        n = pcm["lens"][u]
        wet, gates = [], []
        for s in range(S):
            x, h, d = it["source%d" % (s + 1)], it["rir%d" % (s + 1)], it["rir_delay"][s]
            w = reverb.convolve(x, h, d)
            e32 = float(np.abs(reverb.convolve_partitioned_f32(x, h, d).astype(np.float64) - w).max())
            wet.append(w)
            gates.append(2.0 * max(e32, rc.gate(x, h)))
        mix, srcs, G = mixing.mix(wet, it["amp"], it["peak"])
        peak = it["peak"]
        for s in range(S):
            err = float(np.abs(flat[(1 + s) * total + at:(1 + s) * total + at + n] - srcs[s]).max())
            bound = (S + 6) * rc.EPS * peak + G[s] * gates[s]
            print("n=%4d source %d (%4d taps): %.2f of its bound" % (n, s + 1, len(it["rir%d" % (s + 1)]), err / bound))
            assert err <= bound
        err = float(np.abs(flat[at:at + n] - mix).max())
        bound = S * (2 * S + 6) * rc.EPS * peak + sum(G[s] * gates[s] for s in range(S))
        print("n=%4d mixture: %.2f of its bound" % (n, err / bound))
        assert err <= bound
        # reverberant, not dry: the sources differ from the dry rule's by far more than any bound here
        assert float(np.abs(srcs[0] - mixing.mix([it["source1"], it["source2"]], it["amp"], peak)[1][0]).max()) > 1e-2 * peak
        at += n
    # the front end goes on from that batch exactly as from one that came mixed from disk
    a = features_from_pcm(pcm, dev)
    b = features_from_pcm({"flat": got["flat"], "keys": got["keys"], "lens": got["lens"]}, dev)
    assert torch.equal(a[0], b[0]) and len(a[1]) == 2 and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    assert bool(torch.isfinite(a[0]).all()) and float(a[0][:a[2].R].max()) > 0


def test_one_convolution_in_front_of_one_mixing_and_none_without_reverb(arch, corpus, dev, monkeypatch):
    from sepkern import _lib, ops
    from sepkern.data import Prefetcher, features_from_pcm, psa_features_from_pcm, wave_features_from_pcm
    items = _items(arch, corpus)
    wet = arch.DynMixCollator()(items)
    dry = arch.DynMixCollator()([{k: v for k, v in it.items() if not k.startswith("rir")} for it in items])
    assert "reverb" in wet["pcm"] and "reverb" not in dry["pcm"]
    seen, entry = [], []
    real_fir, real_mix, real_call = ops.fir_convolve, ops.dynamic_mix, _lib.call
    monkeypatch.setattr(ops, "fir_convolve", lambda *a, **k: (seen.append("fir_convolve"), real_fir(*a, **k))[1])
    monkeypatch.setattr(ops, "dynamic_mix", lambda *a, **k: (seen.append("dynamic_mix"), real_mix(*a, **k))[1])
    monkeypatch.setattr(_lib, "call", lambda name, *a: (entry.append(name), real_call(name, *a))[1])
    results = {}
    for name, fn in (("mse", features_from_pcm), ("wave", wave_features_from_pcm), ("psa", psa_features_from_pcm)):
        del seen[:], entry[:]
        results[name] = fn(wet["pcm"], dev)
        assert seen == ["fir_convolve", "dynamic_mix"] and entry[:2] == ["sk_fir_convolve", "sk_dynamic_mix"]
        assert entry.count("sk_fir_convolve") == 1 and entry.count("sk_dynamic_mix") == 1
        wet_entry = list(entry)
        del seen[:], entry[:]
        fn(dry["pcm"], dev)
        assert seen == ["dynamic_mix"] and entry == wet_entry[1:]            # the launches it made before, and no other
    torch.cuda.synchronize()
    # the three front ends see the same reverberant mixture
    assert torch.equal(results["mse"][0], results["wave"][0]) and torch.equal(results["mse"][0], results["psa"][0])
    assert all(bool(torch.isfinite(t).all()) for t in results["psa"][1]) and bool(torch.isfinite(results["wave"][3]["flat"]).all())
    # and the prefetcher stages such a batch like any other
    staged = Prefetcher.stage(wet, dev)
    assert "pcm" not in staged and torch.equal(staged["packed"][0], results["mse"][0])


# ------------------------------------------------------------------------------------------------ 5: training on it
def test_driver_trains_on_reverberant_mixtures_and_a_restart_continues_exactly(arch, tmp_path, monkeypatch):
    """Two epochs of steps/train_qsub.py --dynamic-mix --mix-rir-synth 0.2,0.6 on a 2 x 64 model, 8 mixtures per epoch: finite
    losses, batches that carry RIRs, and a run restarted with --start-epoch 1 ends on exactly the uninterrupted run's loss and
    weights (the checkpoint cadence is set to every epoch for it)."""
    import train_qsub
    data = rc.corpus(os.path.join(str(tmp_path), "data"), n_spk=4, n_utt=2, lengths=[5000 + 300 * i for i in range(8)])
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
    common = ["uPIT", "0", data, None, "--model-config", conf, "--wav-input", "--dynamic-mix", "--mix-rir-synth", "0.2,0.6",
              "--batch-size", "4", "--mixes-per-epoch", "8", "--mix-max-samples", "4000", "--seed", "5", "--num-workers", "0",
              "--prefetch", "0"]

    def argv(out, *more):
        return [out if a is None else a for a in common] + list(more)
    train_qsub.main(argv(straight, "--num-epochs", "2"))
    assert sorted(seen) == [0, 1] and "reverb" in seen[0] and "mixing" in seen[0]
    assert all(1600 <= t <= 4800 for row in seen[0]["reverb"]["taps"] for t in row)
    assert not torch.equal(seen[0]["reverb"]["flat"][:1600], seen[1]["reverb"]["flat"][:1600])
    lines = open(os.path.join(straight, "train_stats", "train_loss.txt")).read().splitlines()
    assert len(lines) == 2 and lines[0].startswith("001 ") and lines[1].startswith("002 ")
    assert all(np.isfinite(float(l.split()[1])) for l in lines)
    os.makedirs(os.path.join(resumed, "intermediate_models"))
    os.makedirs(os.path.join(resumed, "train_stats"))
    for name in ("001.mdl", "001.opt"):
        shutil.copy(os.path.join(straight, "intermediate_models", name), os.path.join(resumed, "intermediate_models", name))
    open(os.path.join(resumed, "train_stats", "train_loss.txt"), "w").write(lines[0] + "\n")
    first_of_epoch_2 = seen.pop(1)
    train_qsub.main(argv(resumed, "--num-epochs", "2", "--start-epoch", "1"))
    assert torch.equal(seen[1]["flat"], first_of_epoch_2["flat"]) and torch.equal(seen[1]["reverb"]["flat"], first_of_epoch_2["reverb"]["flat"])
    assert seen[1]["reverb"]["delay"] == first_of_epoch_2["reverb"]["delay"]
    assert open(os.path.join(resumed, "train_stats", "train_loss.txt")).read().splitlines() == lines
    a = torch.load(os.path.join(straight, "final.mdl"), map_location="cpu")
    b = torch.load(os.path.join(resumed, "final.mdl"), map_location="cpu")
    assert all(torch.equal(a[k], b[k]) for k in a)
