"""Noisy dynamic mixing on the MI355X: sk_diffuse_noise, sk_noise_factors and sk_add_noise through the C ABI over pools of
sentinels, against the fp64 definitions of sepkern/noise.py, and the route from a DynMixCollator batch with 'noise' through
mixed_pcm and the training driver.

sk_diffuse_noise runs ONE ragged batch per channel count and sample type (tests/_noise_cases.py LENGTHS): 1 sample, the hop edges
127 | 128 | 129, 513, one tile and its neighbours 1 663 | 1 664 | 1 665, and 3 329 = two tiles and a sample, every mixture with
factors of its own.  tests/test_noise.py shows that each one-fault switch of the float32 restatement is far outside the gate
used here.  Run with -s for the measured ratios."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from conftest import PKG
import _noise_cases as nc
import _reverb_cases as rc

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(PKG, "archs"))
sys.path.insert(0, os.path.join(PKG, "steps"))

B = len(nc.LENGTHS)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def arch(dev):
    import uPIT
    return uPIT


_RUNS = {}


def _batch(dev, C_, pcm):
    """The ragged batch of C channels, launched once per (C, sample type) and shared by the tests below."""
    if (C_, pcm) not in _RUNS:
        cases = [nc.batch_case(C_, u, pcm) for u in range(B)]
        _RUNS[(C_, pcm)] = nc.launch_diffuse(dev, [c[0] for c in cases], [c[1] for c in cases])
    return _RUNS[(C_, pcm)]


# ------------------------------------------------------------------------------------------------ 1: sk_diffuse_noise
@pytest.mark.parametrize("pcm", [False, True])
@pytest.mark.parametrize("C_", [2, 3, 4, 5, 6, 7, 8])
def test_diffuse_noise_is_within_twice_the_restatements_error_and_writes_only_its_ranges(C_, pcm, dev):
    """max |out - diffuse_fp64| <= 2 max(e32, u) per mixture (tests/_noise_cases.py gate: e32 the float32 restatement's own error
    for the same case, u = 2^-24 sum_j max |x_j| the unit floor -- tests/test_gpu_room.py's rule)."""
    outs, pool, written = _batch(dev, C_, pcm)
    worst = []
    for u, n in enumerate(nc.LENGTHS):
        x, Lt, want, e32 = nc.batch_case(C_, u, pcm)
        gate = nc.gate(x, e32)
        err = float(np.abs(outs[u].astype(np.float64) - want).max())
        print("C=%d %s n=%4d: kernel %.2e = %.3f of the gate (restatement %.2e, max |out| %.2f)"
              % (C_, "int16" if pcm else "float", n, err, err / gate, e32, np.abs(want).max()))
        worst.append(err / gate)
    assert np.isfinite(pool).all() and max(worst) <= 1.0, worst
    assert bool((pool[~written] == nc.CANARY).all()) and int((~written).sum()) == nc.GAP * (C_ * B + 1)
    assert not bool((pool[written] == nc.CANARY).any())


@pytest.mark.parametrize("C_", [2, 8])
def test_identity_factors_give_the_input_back(C_, dev):
    """Within 4 ulp of the largest sample, at every length of the batch."""
    xs = [nc.signals(C_, n, 7) for n in nc.LENGTHS]
    eye = np.broadcast_to(np.eye(C_, dtype=np.float32), (257, C_, C_))
    from sepkern import noise
    outs, _, _ = nc.launch_diffuse(dev, xs, [noise.tri(eye)] * B)
    for x, y in zip(xs, outs):
        tol = 4.0 * float(np.spacing(np.float32(np.abs(x).max())))
        err = float(np.abs(y.astype(np.float64) - x.astype(np.float64)).max())
        print("C=%d n=%4d: %.2e (4 ulp of the largest sample: %.2e)" % (C_, x.shape[1], err, tol))
        assert err <= tol


@pytest.mark.parametrize("C_, i, j, k0, k1", [(2, 1, 0, 0, 257), (5, 3, 1, 40, 90), (8, 7, 0, 0, 1), (8, 6, 6, 128, 129), (7, 4, 2, 200, 257)])
def test_one_hot_factors_reach_only_their_channel(C_, i, j, k0, k1, dev):
    """L zero but for L[i, j] = 1 on the bins [k0, k1): every other output channel is exactly zero, and channel i is input j
    through that band (the fp64 definition within the gate of the test above)."""
    from sepkern import noise
    Lf = np.zeros((257, C_, C_), dtype=np.float32)
    Lf[k0:k1, i, j] = 1.0
    us = [4, 7, 8]                                        # 513, 1 665 and 3 329 samples
    xs = [nc.signals(C_, nc.LENGTHS[u], 9) for u in us]
    outs, _, _ = nc.launch_diffuse(dev, xs, [noise.tri(Lf)] * len(us))
    for x, y in zip(xs, outs):
        assert all(not y[c].any() for c in range(C_) if c != i)
        want = noise.diffuse(x, Lf.astype(np.float64))
        e32 = float(np.abs(noise.diffuse_f32(x, Lf) - want).max())
        assert np.abs(want[i]).max() > 1e-3
        assert float(np.abs(y.astype(np.float64) - want).max()) <= nc.gate(x, e32)


@pytest.mark.parametrize("C_", [2, 5, 8])
def test_bits_do_not_depend_on_batch_order_run_or_sample_type(C_, dev):
    outs, _, _ = _batch(dev, C_, True)
    cases = [nc.batch_case(C_, u, True) for u in range(B)]
    again, _, _ = nc.launch_diffuse(dev, [c[0] for c in cases], [c[1] for c in cases])
    assert all(np.array_equal(a, b) for a, b in zip(outs, again))
    order = [8, 0, 5, 3, 7]
    part, _, _ = nc.launch_diffuse(dev, [cases[u][0] for u in order], [cases[u][1] for u in order])
    assert all(np.array_equal(part[q], outs[u]) for q, u in enumerate(order))
    for u in (0, 6, 8):
        alone, _, _ = nc.launch_diffuse(dev, [cases[u][0]], [cases[u][1]])
        assert np.array_equal(alone[0], outs[u]), u
    # the float32 copies of the int16 samples (x / 32768, exact) give the same bits
    asf, _, _ = nc.launch_diffuse(dev, [c[0].astype(np.float32) * np.float32(1.0 / 32768.0) for c in cases], [c[1] for c in cases])
    assert all(np.array_equal(a, b) for a, b in zip(outs, asf))
    # max_nsamp sizes the grid and cuts a longer signal: with 1 700 the two-tile mixture keeps its first 1 700 samples' bits
    cut, pool, _ = nc.launch_diffuse(dev, [cases[8][0]], [cases[8][1]], max_nsamp=1700)
    assert bool((cut[0][:, 1700:] == nc.CANARY).all()) and not bool((cut[0][:, :1700] == nc.CANARY).any())


# ------------------------------------------------------------------------------------------------ 2: sk_noise_factors
@pytest.mark.parametrize("B_, C_", [(1, 2), (3, 2), (1, 8), (3, 8), (17, 3)])
def test_noise_factors_against_fp64(B_, C_, dev):
    """To float32 rounding: |L - fp32(L_fp64)| <= 2^-23 |L| + 4e-9.  The first term is one float32 rounding flipped; the second is
    what two correct fp64 Cholesky factorisations of a matrix with condition 1 / eps = 2^20 may differ by (2^20 x a few 2^-53 of
    entries of size 1).  17 mixtures: two launches of 16."""
    from sepkern import noise, ops
    mics = np.stack([nc.mics_of(C_, u) for u in range(B_)])
    if C_ == 8 and B_ == 3:
        mics[1] = nc.TIGHT["line 8 x 2 cm at 8 kHz"][0] + 1.0
    L = ops.noise_factors(mics, nc.RATE, device=dev)
    torch.cuda.synchronize()
    assert tuple(L.shape) == (B_, 257, C_ * (C_ + 1) // 2) and L.dtype == torch.float32
    got = L.cpu().numpy().astype(np.float64)
    for u in range(B_):
        want = noise.tri(noise.factors(mics[u], nc.RATE))
        err = np.abs(got[u] - want.astype(np.float32).astype(np.float64))
        assert np.all(err <= 2.0 ** -23 * np.abs(want) + 4e-9), (u, float(err.max()))
        assert abs(got[u][0, 0] - 1.0) < 1e-6 and np.all(np.abs(got[u][0, [i * (i + 1) // 2 for i in range(C_)]] - 1.0) < 1e-6)


# ------------------------------------------------------------------------------------------------ 3: sk_add_noise
@pytest.mark.parametrize("pcm", [False, True])
@pytest.mark.parametrize("C_", [1, 2, 8])
def test_add_noise_against_fp64(C_, pcm, dev):
    """One batch of the 7 lengths + a silent-noise and a silent-mixture case.  The gain: |a - a_fp64| <= 2 ulp (the fp64 sums run in
    another order: 1e-13, then one rounding that may flip).  Every sample: |out - (a v + y)| <= 2^-24 (|a v| + |y|), one fused
    multiply-add.  Quantized = quantize(the unquantized result) exactly, with the clip reached: every mixture's last sample --
    alone in the last trip of its thread -- is the loudest and over full scale once the noise is on."""
    from sepkern import mixing, noise
    rng = np.random.default_rng(60 + C_)
    ns = nc.ADD_LENGTHS + [1500, 1500]
    ys, vs = [], []
    for u, n in enumerate(ns):
        y = (rng.standard_normal((C_, n)) * 0.1).astype(np.float32)
        v = rng.standard_normal((C_, n)) * 0.1
        y[:, -1], v[:, -1] = 0.9, 0.5
        if u == len(ns) - 2:
            v[0] = 0.0                                   # silent noise on the reference channel (loud on the others)
        if u == len(ns) - 1:
            y[0] = 1e-7                                  # mean square 1e-14 < 2^-40: a silent mixture
        ys.append(y)
        vs.append(np.clip(np.rint(v * 32768.0), -32768, 32767).astype(np.int16) if pcm else v.astype(np.float32))
    amp = [float(noise.snr_to_amp(s)) for s in np.linspace(-3.0, 6.0, len(ns))]
    plain, gains, pool, written = nc.launch_add(dev, ys, vs, amp, quantize=False)
    assert bool((pool[~written] == nc.CANARY).all())
    for u, n in enumerate(ns):
        want, a = noise.add_noise(list(ys[u]), list(vs[u]), amp[u])
        assert abs(float(gains[u]) - a) <= 2.0 * float(np.spacing(np.float32(a))), (u, gains[u], a)
        assert (a == 0.0) == (u >= len(ns) - 2)
        g, v64, y64 = float(gains[u]), mixing.as_float(vs[u]), ys[u].astype(np.float64)
        assert np.all(np.abs(plain[u] - (g * v64 + y64)) <= nc.EPS32 * (np.abs(g * v64) + np.abs(y64)))
        if a == 0.0:
            assert np.array_equal(plain[u], ys[u])
    quant, gq, pool, written = nc.launch_add(dev, ys, vs, amp, quantize=True, want_gains=False)
    assert bool((pool[~written] == nc.CANARY).all()) and bool((gq == nc.CANARY).all())          # gains_out = NULL: nothing stored
    for u in range(len(ns)):
        assert np.array_equal(quant[u].astype(np.float64), mixing.quantize(plain[u]))
    assert all(quant[u][0, -1] == np.float32(32767.0 / 32768.0) for u in range(len(nc.ADD_LENGTHS)))


def test_refusals_come_before_any_launch(dev):
    from sepkern import _lib, ops
    nc.check_refusals(_lib.load())
    x = torch.zeros(4000, device=dev)
    L = ops.noise_factors(nc.line(2, 0.05)[None], nc.RATE, device=dev)
    for bad in (dict(chan_offs=[[0]]), dict(chan_offs=[[0], [3000]]), dict(nsamp=[0]), dict(L=L[:, :100]), dict(flat=x.cpu())):
        with pytest.raises(_lib.SepkernError):
            ops.diffuse_noise(**dict(dict(flat=x, chan_offs=[[0], [2000]], nsamp=[1500], L=L), **bad))
    for bad in (dict(noise_offs=[[0], [0]]), dict(amp=[1.0, 1.0]), dict(sig_offs=[[3000]]), dict(noise=x.cpu())):
        with pytest.raises(_lib.SepkernError):
            ops.add_noise(**dict(dict(sig=x, sig_offs=[[0]], noise=x, noise_offs=[[2000]], nsamp=[1500], amp=[1.0]), **bad))
    with pytest.raises(_lib.SepkernError):
        ops.noise_factors(np.zeros((1, 2, 3)), nc.RATE, device=dev)                             # two microphones in one place
    with pytest.raises(_lib.SepkernError):
        ops.noise_factors(nc.line(9, 0.05)[None], nc.RATE, device=dev)


# ------------------------------------------------------------------------------------------------ 4: the route
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return str(tmp_path_factory.mktemp("noisy"))


@pytest.fixture(scope="module")
def scp(corpus):
    """Three recordings: one long, one shorter than most mixtures (it wraps around), one in between."""
    return nc.noise_scp(os.path.join(corpus, "noise"), [60000, 700, 9000])


def _array3():
    return np.array([[0.0, 0.0, 0.0], [0.05, 0.0, 0.0], [0.0, 0.08, 0.0]])


def _items(arch, corpus, scp, **kw):
    """Three items of 4 355, 1 000 and 257 samples, S = 2, with noise."""
    items = []
    for k, n in enumerate((4355, 1000, 257)):
        root = rc.corpus(os.path.join(corpus, "n%d" % n), n_spk=2, n_utt=1, lengths=[n, n])
        ds = arch.DynMixTrainSet(root, 2, seed=3 + k, peak=(0.5, 0.9), noise_scp=scp, noise_snr_db=(-3.0, 6.0), **kw)
        items.append(ds[k])
    return items


def _without_noise(items):
    return [{k: v for k, v in it.items() if not k.startswith("noise")} for it in items]


@pytest.mark.parametrize("kind", ["plain", "reverb", "mono room"])
def test_a_mono_batch_gets_its_crop_at_the_drawn_snr_and_clean_sources(kind, arch, corpus, scp, dev):
    from sepkern.data import mixed_pcm
    kw = {"plain": {}, "reverb": dict(rir_synth=(0.05, 0.1)), "mono room": dict(room_t60=(0.06, 0.12), room_dims=((3, 3, 2.5), (5, 4, 3)))}[kind]
    items = _items(arch, corpus, scp, **kw)
    col = arch.DynMixCollator()
    noisy, clean = mixed_pcm(col(items)["pcm"], dev), mixed_pcm(col(_without_noise(items))["pcm"], dev)
    torch.cuda.synchronize()
    ns, total = noisy["lens"], sum(noisy["lens"])
    assert noisy["keys"] == clean["keys"] == ["mix", "source1", "source2"] and ns == clean["lens"] == [4355, 1000, 257]
    assert torch.equal(noisy["flat"][total:], clean["flat"][total:])                       # the targets are the clean sources, bit for bit
    a, c = noisy["flat"][:total].cpu().numpy().astype(np.float64), clean["flat"][:total].cpu().numpy().astype(np.float64)
    at = 0
    for u, it in enumerate(items):
        n = ns[u]
        d = a[at:at + n] - c[at:at + n]
        snr = 10.0 * np.log10(np.mean(c[at:at + n] ** 2) / np.mean(d ** 2))
        want = -20.0 * np.log10(it["noise_amp"])
        print("%s n=%4d: snr %.4f dB, drawn %.4f dB" % (kind, n, snr, want))
        assert abs(snr - want) < 0.01                                                      # (a float32 difference of float32 signals)
        v = it["noise1"].astype(np.float64)
        assert abs(np.dot(d, v) / np.sqrt(np.dot(d, d) * np.dot(v, v))) > 0.999999         # and it is that crop
        at += n


def test_an_array_batch_gets_a_diffuse_field_at_the_reference_channels_gain(arch, corpus, scp, dev):
    from sepkern import ops
    from sepkern.data import mixed_pcm
    items = _items(arch, corpus, scp, room_t60=(0.06, 0.12), room_dims=((3, 3, 2.5), (5, 4, 3)), array=_array3(), ipd_ref=1, ipd_channels=(2, 0))
    col = arch.DynMixCollator()
    pcm = col(items)["pcm"]
    noisy, clean = mixed_pcm(pcm, dev), mixed_pcm(col(_without_noise(items))["pcm"], dev)
    ns, total = noisy["lens"], sum(noisy["lens"])
    assert noisy["keys"] == clean["keys"] == ["mix", "source1", "source2", "chan2", "chan0"]
    assert torch.equal(noisy["flat"][total:3 * total], clean["flat"][total:3 * total])
    # the field, made again from the same crops and microphones
    nz = pcm["noise"]
    starts = [sum(ns[:j]) for j in range(3)]
    L = ops.noise_factors(pcm["room"]["mics"], 8000, device=dev)
    field = ops.diffuse_noise(nz["flat"].to(dev), [[c * total + st for st in starts] for c in range(3)], ns, L)
    torch.cuda.synchronize()
    f = field.cpu().numpy().astype(np.float64)
    a, c = noisy["flat"].cpu().numpy().astype(np.float64), clean["flat"].cpu().numpy().astype(np.float64)
    for u, it in enumerate(items):
        n, st = ns[u], starts[u]
        ref_clean, f0 = c[st:st + n], f[st:st + n]
        gain = float(np.float32(it["noise_amp"] * np.sqrt(np.mean(ref_clean ** 2) / np.mean(f0 ** 2))))
        d0 = a[st:st + n] - ref_clean
        assert abs(10.0 * np.log10(np.mean(ref_clean ** 2) / np.mean(d0 ** 2)) + 20.0 * np.log10(it["noise_amp"])) < 0.01
        for k, q in enumerate((0, 3, 4)):                                                  # 'mix', 'chan2', 'chan0' <-> field channel k
            y, fk = c[q * total + st:q * total + st + n], f[k * total + st:k * total + st + n]
            got = a[q * total + st:q * total + st + n]
            # one fused multiply-add, and the gain within 2 ulp (the kernel's fp64 sums run in another order)
            assert np.all(np.abs(got - (gain * fk + y)) <= 2.0 ** -24 * (np.abs(gain * fk) + np.abs(y)) + 2.0 ** -22 * np.abs(gain * fk)), (u, k)


def test_a_batch_without_noise_makes_the_launches_it_made_and_noise_adds_its_own_behind_the_mixing(arch, corpus, scp, dev, monkeypatch):
    from sepkern import _lib
    from sepkern.data import features_from_pcm, psa_features_from_pcm, wave_features_from_pcm
    room = dict(room_t60=(0.06, 0.12), room_dims=((3, 3, 2.5), (5, 4, 3)))
    col = arch.DynMixCollator()
    mono_items = _items(arch, corpus, scp)
    array_items = _items(arch, corpus, scp, array=_array3(), ipd_channels=(1, 2), **room)
    entry = []
    real_call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (entry.append(name), real_call(name, *a))[1])
    new = {"sk_noise_factors", "sk_diffuse_noise", "sk_add_noise"}
    for fn in (features_from_pcm, wave_features_from_pcm, psa_features_from_pcm):
        del entry[:]
        fn(col(_without_noise(mono_items))["pcm"], dev)
        plain = list(entry)
        assert plain[0] == "sk_dynamic_mix" and not new & set(plain)
        del entry[:]
        fn(col(mono_items)["pcm"], dev)
        assert entry == ["sk_dynamic_mix", "sk_add_noise"] + plain[1:]
        del entry[:]
        fn(col(_without_noise(array_items))["pcm"], dev)
        quiet = list(entry)
        assert quiet[:4] == ["sk_room_rirs", "sk_fir_convolve", "sk_dynamic_mix", "sk_mix_channels"] and quiet[4:] == plain[1:]
        del entry[:]
        fn(col(array_items)["pcm"], dev)
        assert entry == quiet[:4] + ["sk_noise_factors", "sk_diffuse_noise", "sk_add_noise"] + quiet[4:]
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5: training on it
def test_driver_trains_on_noisy_mixtures_mono_and_array_and_a_restart_continues_exactly(arch, tmp_path, monkeypatch):
    """steps/train_qsub.py --dynamic-mix --mix-noise-scp: one epoch of a mono 2 x 64 model; two epochs of an IPD model
    (ipd_channels=1,2) with --mix-room-t60 --mix-array, and that run restarted with --start-epoch 1 ends on exactly the
    uninterrupted run's loss and weights."""
    import train_qsub
    data = rc.corpus(os.path.join(str(tmp_path), "data"), n_spk=4, n_utt=2, lengths=[5000 + 300 * i for i in range(8)])
    noise_list = nc.noise_scp(os.path.join(str(tmp_path), "noise"), [20000, 3000])
    array = os.path.join(str(tmp_path), "array.txt")
    open(array, "w").write("0 0 0\n0.05 0 0\n0 0.08 0\n")
    monkeypatch.setattr(train_qsub, "CHECKPOINT_EVERY", 1)
    seen = {}
    real = arch.compute_loss

    def spy(model, epoch, batch, *a):
        seen.setdefault(epoch, batch["pcm"])
        return real(model, epoch, batch, *a)
    monkeypatch.setattr(arch, "compute_loss", spy)
    mono, ipd = os.path.join(str(tmp_path), "mono"), os.path.join(str(tmp_path), "ipd")
    open(mono, "w").write("hidden_dim=64\nnum_layers=2\nnum_spk=2\n")
    open(ipd, "w").write("hidden_dim=64\nnum_layers=2\nnum_spk=2\nipd_channels=1,2\n")
    common = ["uPIT", "0", data, None, "--wav-input", "--dynamic-mix", "--mix-noise-scp", noise_list, "--mix-noise-snr", "0,10",
              "--batch-size", "4", "--mixes-per-epoch", "8", "--mix-max-samples", "4000", "--seed", "5", "--num-workers", "0", "--prefetch", "0"]

    def argv(out, *more):
        return [out if a is None else a for a in common] + list(more)
    first = os.path.join(str(tmp_path), "first")
    train_qsub.main(argv(first, "--model-config", mono, "--num-epochs", "1"))
    nz = seen.pop(0)["noise"]
    assert nz["flat"].numel() == sum(nz["lens"]) and all(10.0 ** -0.5 <= a <= 1.0 for a in nz["amp"])
    assert np.isfinite(float(open(os.path.join(first, "train_stats", "train_loss.txt")).read().split()[1]))
    straight, resumed = os.path.join(str(tmp_path), "straight"), os.path.join(str(tmp_path), "resumed")
    rooms = ["--model-config", ipd, "--mix-room-t60", "0.05,0.1", "--mix-array", array, "--num-epochs", "2"]
    train_qsub.main(argv(straight, *rooms))
    assert sorted(seen) == [0, 1] and seen[0]["room"]["chans"] == [1, 2] and seen[0]["noise"]["flat"].numel() == 3 * sum(seen[0]["noise"]["lens"])
    assert not torch.equal(seen[0]["noise"]["flat"][:1000], seen[1]["noise"]["flat"][:1000])
    lines = open(os.path.join(straight, "train_stats", "train_loss.txt")).read().splitlines()
    assert len(lines) == 2 and all(np.isfinite(float(l.split()[1])) for l in lines)
    os.makedirs(os.path.join(resumed, "intermediate_models"))
    os.makedirs(os.path.join(resumed, "train_stats"))
    for name in ("001.mdl", "001.opt"):
        shutil.copy(os.path.join(straight, "intermediate_models", name), os.path.join(resumed, "intermediate_models", name))
    open(os.path.join(resumed, "train_stats", "train_loss.txt"), "w").write(lines[0] + "\n")
    first_of_epoch_2 = seen.pop(1)
    train_qsub.main(argv(resumed, *rooms, "--start-epoch", "1"))
    assert torch.equal(seen[1]["flat"], first_of_epoch_2["flat"]) and torch.equal(seen[1]["noise"]["flat"], first_of_epoch_2["noise"]["flat"])
    assert seen[1]["noise"]["amp"] == first_of_epoch_2["noise"]["amp"]
    assert open(os.path.join(resumed, "train_stats", "train_loss.txt")).read().splitlines() == lines
    a = torch.load(os.path.join(straight, "final.mdl"), map_location="cpu")
    b = torch.load(os.path.join(resumed, "final.mdl"), map_location="cpu")
    assert all(torch.equal(a[k], b[k]) for k in a)
