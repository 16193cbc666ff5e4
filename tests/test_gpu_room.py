"""Simulated rooms on the MI355X: sk_room_rirs against the fp64 definition (sepkern/room.py ism_rir) inside a gate that comes
from the float32 restatement's own error, the properties its one-workgroup-per-job form promises (bits that depend on neither
batch, run nor order; nothing written outside the stated ranges), sk_mix_channels against fp64 and against sk_dynamic_mix's
own mixture, and the route from a DynMixCollator batch with 'room' through the front ends and the training driver.

ONE launch of 11 jobs (tests/_room_cases.py gpu_jobs) over one shared pool, 8 kHz:
   0  1 tap, the source 0.02 m from the microphone       1  33 taps, every wall absorbs (beta = 0), 0.02 m: support clipped at n < 0
   2  33 taps, the direct path beyond them: all zero     3  256 taps, beta = 0 on two walls
   4  257 taps, beta = 0.95                              5  700 taps, a small room with many images (2.2 x 2.0 x 2.1 m)
   6  700 taps, six different walls, scaled              7  4 097 taps, a large room with few images (12 x 10 x 4 m)
   8  4 097 taps, 6 x 5 x 3 m                            9  8 192 taps (the maximum), 10 x 8 x 4 m, beta = 0.95
  10  256 taps, anechoic, a direct path of exactly 40 samples scaled to 1
about 1.1 million images in all.  tests/test_room.py shows that one lost parity class, shell, tap shift or wrong exponent is at
least 100 units outside the restatement's own error.  Run with -s for the measured ratios."""
import ctypes as C
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from conftest import PKG
import _reverb_cases as rc
import _room_cases as rm

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(PKG, "archs"))
sys.path.insert(0, os.path.join(PKG, "steps"))

JOBS = rm.gpu_jobs()
GAP, CANARY = 7, 777.0


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
    assert {j[4] for j in JOBS} == {1, 33, 256, 257, 700, 4097, 8192} and len(JOBS) == 11
    assert all(b == 0.0 for b in JOBS[1][1]) and sorted(set(JOBS[3][1])) == [0.0, 0.9] and set(JOBS[9][1]) == {0.95}
    assert abs(np.linalg.norm(np.subtract(JOBS[1][2], JOBS[1][3])) - 0.02) < 1e-12
    assert sum(rm.gpu_reference(j)[3] for j in range(len(JOBS))) < 2_000_000
    assert rm.gpu_reference(5)[3] > 10_000 and rm.gpu_reference(7)[3] < 60_000 and rm.gpu_reference(2)[3] == 0


def _launch(dev, which=None):
    """The jobs `which` (default: all, in order) in ONE sk_room_rirs call over one pool filled with canaries, on a 0xFF-filled
    workspace of exactly the queried size -> (pool, {job: offset})."""
    from sepkern import _lib
    which = list(range(len(JOBS))) if which is None else list(which)
    offs, at = [], GAP
    for j in which:
        offs.append(at)
        at += JOBS[j][4] + GAP
    a = rm.host_arrays([JOBS[j] for j in which], offs=offs)
    q, _ = rm.entry_args(a, len(which), rm.RATE)
    nbytes = _lib.load().sk_room_workspace_bytes(*q)
    assert nbytes == -(-len(which) * 168 // 256) * 256 > 0          # the job table: 168 bytes per job, 256-aligned
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    pool = torch.full((at,), CANARY, device=dev)
    _, r = rm.entry_args(a, len(which), rm.RATE, C.c_void_p(ws.data_ptr()), C.c_void_p(pool.data_ptr()),
                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.call("sk_room_rirs", *r)
    torch.cuda.synchronize()
    return pool, dict(zip(which, offs))


@pytest.fixture(scope="module")
def batch(dev):
    return _launch(dev)


# ------------------------------------------------------------------------------------------------ 1: against the definition
def test_every_job_is_within_twice_the_float32_restatements_error(batch):
    """|h - ism_rir_fp64|[n] <= 2 max(e32[n], u[n]) at every tap: e32 the restatement's own error, u[n] = 2^-24 sum |A_i| over the
    images that cover n; the factor 2 is for fma contraction and the device's sinpi / cospi / rcp rounding differently from numpy."""
    pool, offs = batch
    h = pool.cpu().numpy().astype(np.float64)
    worst = []
    for j, job in enumerate(JOBS):
        want, gate, e32, images = rm.gpu_reference(j)
        got = h[offs[j]:offs[j] + job[4]]
        err = np.abs(got - want)
        live = gate > 0
        assert np.all(got[~live] == 0.0), j
        ratio = float(np.max(err[live] / gate[live])) if live.any() else 0.0
        print("job %2d %4d taps %7d images: kernel %.3f of the gate, float32 restatement %.2f u, %.1e of max |h|"
              % (j, job[4], images, ratio, e32, err.max() / max(np.abs(want).max(), 1e-300)))
        worst.append(ratio)
    assert np.isfinite(h).all() and max(worst) <= 1.0, worst


def test_exact_things(batch):
    pool, offs = batch
    assert bool((pool[offs[2]:offs[2] + 33] == 0).all())                                  # the direct path lies beyond the taps
    h = pool[offs[10]:offs[10] + 256].cpu().numpy().astype(np.float64)
    assert abs(h[40] - 1.0) < 4 * 2.0 ** -24 and np.abs(np.delete(h, 40)).max() < 4 * 2.0 ** -24
    # tau = 0.47: the support starts at n = -31, and tap 0 holds 1 / (4 pi 0.02) window(0.47) sinc(0.47) = 3.98 x 0.68
    assert abs(float(pool[offs[1]]) - 2.70) < 0.02 and float(pool[offs[0]]) > 2.0


# ------------------------------------------------------------------------------------------------ 2: what the bits do not depend on
def test_bits_do_not_depend_on_batch_run_or_order(batch, dev):
    pool, offs = batch
    again, _ = _launch(dev)
    assert torch.equal(pool, again)
    for j, job in enumerate(JOBS):
        alone, a = _launch(dev, which=(j,))
        assert torch.equal(alone[a[j]:a[j] + job[4]], pool[offs[j]:offs[j] + job[4]]), j
    some = [9, 3, 10, 0, 6, 5]
    part, po = _launch(dev, which=some)
    for j in some:
        assert torch.equal(part[po[j]:po[j] + JOBS[j][4]], pool[offs[j]:offs[j] + JOBS[j][4]]), j


def test_only_the_stated_ranges_are_written(batch):
    pool, offs = batch
    written = torch.zeros(pool.numel(), dtype=torch.bool, device=pool.device)
    for j, job in enumerate(JOBS):
        written[offs[j]:offs[j] + job[4]] = True
    assert int((~written).sum()) == GAP * (len(JOBS) + 1) and bool((pool[~written] == CANARY).all())
    assert not bool((pool[written] == CANARY).any())


def test_refusals_come_before_any_launch(dev):
    from sepkern import _lib, ops
    rm.check_refusals(_lib.load())
    L, b, s, m, n, sc = rm.GOOD
    rirs, offs = ops.room_rirs([L, L], [b, b], [s, s], [m, m], [n, 33], rm.RATE, device=dev)
    assert rirs.dtype == torch.float32 and rirs.numel() == n + 33 and offs == [0, n] and rirs.device == dev
    for bad in (dict(ntaps=[n, 0]), dict(rate=0.0), dict(rooms=[L, (5.0, 4.0, 0.0)]), dict(mics=[m, (6.0, 2.0, 1.5)])):
        kw = dict(dict(rooms=[L, L], betas=[b, b], srcs=[s, s], mics=[m, m], ntaps=[n, 33], rate=rm.RATE), **bad)
        with pytest.raises(_lib.SepkernError):
            ops.room_rirs(device=dev, **kw)
    with pytest.raises(_lib.SepkernError):
        ops.room_rirs([L], [b], [s], [m], [n], rm.RATE, device="cpu")


# ------------------------------------------------------------------------------------------------ 3: sk_mix_channels
MC_LENGTHS = [1, 255, 256, 257, 4095, 4096, 4097]          # its loop: 16 workgroups of 256 per signal, a second trip from 4 097 on


@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_mix_channels_against_fp64_and_the_reference_channel_is_dynamic_mixs_mixture(S, dev):
    """One batch of the 7 lengths, P = 2 channels + the reference fed as a third: |out - sum_s G_s x_s| <= S 2^-24 sum_s |G_s x_s|
    (S fused multiply-adds, one rounding each), G the gains sk_dynamic_mix returned; quantized = quantize(the unquantized result)
    exactly, with the clip reached on the louder channel."""
    from sepkern import mixing, ops
    rng = np.random.default_rng(40 + S)
    B, ns = len(MC_LENGTHS), MC_LENGTHS
    sig, offs, at = [], [[[0] * B for _ in range(3)] for _ in range(S)], 0      # channel 0: the reference, 1: another, 2: 3 x louder
    for s in range(S):
        for p in range(3):
            for u, n in enumerate(ns):
                x = (rng.standard_normal(n) * 0.1 * (3.0 if p == 2 else 1.0)).astype(np.float32)
                sig.append(x)
                offs[s][p][u] = at
                at += n
    flat = torch.from_numpy(np.concatenate(sig)).to(dev)
    amp, peak = [[1.0 + 0.1 * s] * B for s in range(S)], [0.9] * B
    total = sum(ns)
    for quant in (False, True):
        ref, gains = ops.dynamic_mix(flat, [offs[s][0] for s in range(S)], ns, amp, peak, quantize=quant)
        out = ops.mix_channels(flat, offs, ns, gains, quantize=quant)
        torch.cuda.synchronize()
        assert out.numel() == 3 * total and torch.equal(out[:total], ref[:total])           # bit for bit sk_dynamic_mix's mixture
        if not quant:
            plain, G = out.cpu().numpy().astype(np.float64), gains.cpu().numpy().astype(np.float64)
            at_u = 0
            for u, n in enumerate(ns):
                for p in range(3):
                    xs = [sig[(s * 3 + p) * B + u].astype(np.float64) for s in range(S)]
                    want = mixing.mix_channels([xs], G[:, u])[0]
                    bound = S * rc.EPS * sum(np.abs(G[s, u] * xs[s]) for s in range(S))
                    assert np.all(np.abs(plain[p * total + at_u:p * total + at_u + n] - want) <= bound), (u, p)
                at_u += n
        else:
            q = out.cpu().numpy().astype(np.float64)
            assert np.array_equal(q, mixing.quantize(plain))
            assert q[2 * total:].max() == 32767.0 / 32768.0 and q[2 * total:].min() == -1.0 and np.abs(q[:total]).max() <= 0.9 + 2.0 ** -15
    from sepkern import _lib
    for bad in (dict(chan_offs=[[[0] * B] * 8] * S), dict(nsamp=[0] * B), dict(gains=gains[:, :1]), dict(chan_offs=[[[at] * B]] * S)):
        with pytest.raises(_lib.SepkernError):
            ops.mix_channels(**dict(dict(flat=flat, chan_offs=offs, nsamp=ns, gains=gains), **bad))


# ------------------------------------------------------------------------------------------------ 4: the route
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return str(tmp_path_factory.mktemp("room"))


def _items(arch, corpus, **kw):
    """Three items of 4 355, 1 000 and 257 samples, S = 2, in rooms of their own with the 3-microphone array."""
    items = []
    for k, n in enumerate((4355, 1000, 257)):
        root = rc.corpus(os.path.join(corpus, "n%d" % n), n_spk=2, n_utt=1, lengths=[n, n])
        ds = arch.DynMixTrainSet(root, 2, seed=3 + k, peak=(0.5, 0.9), room_t60=(0.06, 0.12), room_dims=((3, 3, 2.5), (5, 4, 3)),
                                 array=rm.array3(), **kw)
        items.append(ds[k])
    return items


def test_the_reference_channel_is_the_reverberant_route_on_the_same_rirs(arch, corpus, dev):
    """mixed_pcm with 'room' = the existing route ('reverb') fed with sk_room_rirs' reference-microphone RIRs, bit for bit; the
    other channels within their bound of the fp64 chain ism_rir -> convolve -> mix / mix_channels."""
    from sepkern import mixing, ops, reverb, room
    from sepkern.data import mixed_pcm
    items = _items(arch, corpus, ipd_ref=1, ipd_channels=(2, 0))
    pcm = arch.DynMixCollator()(items)["pcm"]
    assert pcm["lens"] == [4355, 1000, 257] and pcm["room"]["chans"] == [2, 0]
    got = mixed_pcm(pcm, dev)
    torch.cuda.synchronize()
    S, B, ns, total = 2, 3, pcm["lens"], sum(pcm["lens"])
    assert got["keys"] == ["mix", "source1", "source2", "chan2", "chan0"] and got["lens"] == ns and got["flat"].numel() == 5 * total
    r = pcm["room"]
    # a. the existing route on the reference RIRs
    jobs = [(s, b) for s in range(S) for b in range(B)]
    scales = [4.0 * np.pi * np.linalg.norm(r["srcs"][b, s] - r["mics"][b, 0]) for s, b in jobs]
    rirs, roffs = ops.room_rirs([r["L"][b] for _, b in jobs], [r["beta"][b] for _, b in jobs], [r["srcs"][b, s] for s, b in jobs],
                                [r["mics"][b, 0] for _, b in jobs], [r["ntaps"][b] for _, b in jobs], r["rate"], scales=scales, device=dev)
    delay = [[room.direct_delay(r["srcs"][b, s], r["mics"][b, 0], r["rate"]) for b in range(B)] for s in range(S)]
    old = dict({k: v for k, v in pcm.items() if k != "room"},
               reverb={"flat": rirs, "offs": [roffs[s * B:(s + 1) * B] for s in range(S)], "taps": [list(r["ntaps"])] * S, "delay": delay})
    want = mixed_pcm(old, dev)
    assert want["keys"] == ["mix", "source1", "source2"] and torch.equal(want["flat"], got["flat"][:3 * total])
    # b. the other channels against fp64
    flat = got["flat"].cpu().numpy().astype(np.float64)
    at = 0
    for u, it in enumerate(items):
        n, rr = ns[u], it["room"]
        wet, eps = [[None] * 3 for _ in range(S)], [[0.0] * 3 for _ in range(S)]
        for s in range(S):
            x, d = it["source%d" % (s + 1)], delay[s][u]
            scale = 4.0 * np.pi * np.linalg.norm(rr["srcs"][s] - rr["mics"][0])
            for c in range(3):
                h, unit = room.ism_rir(rr["L"], rr["beta"], rr["srcs"][s], rr["mics"][c], rr["rate"], rr["ntaps"], scale, want_unit=True)
                e32 = np.abs(room.ism_rir_f32(rr["L"], rr["beta"], rr["srcs"][s], rr["mics"][c], rr["rate"], rr["ntaps"], scale) - h)
                wet[s][c] = reverb.convolve(x, h, d)
                c32 = float(np.abs(reverb.convolve_partitioned_f32(x, h, d).astype(np.float64) - wet[s][c]).max())
                xmax = float(np.abs(mixing.as_float(x)).max())
                # the convolution's own gate, and the RIR's gate carried through it as rc.gate carries h: the taps' roundings are
                # uncorrelated, so their sum against samples of at most max|x| is as large as the root of their squares' sum
                eps[s][c] = 2.0 * max(c32, rc.gate(x, h)) + xmax * float(np.sqrt(np.sum((2.0 * np.maximum(e32, unit)) ** 2)))
        mix, srcs, G = mixing.mix([wet[s][0] for s in range(S)], it["amp"], it["peak"])
        chans = mixing.mix_channels([[wet[s][c] for s in range(S)] for c in (1, 2)], G)
        # what the reference channel's own error does to the gains: relative, through the powers and through the peak
        rho = 2.0 * max(eps[s][0] / np.sqrt(np.mean(wet[s][0] ** 2)) for s in range(S)) + sum(G[s] * eps[s][0] for s in range(S)) / it["peak"]
        for p, c in enumerate((1, 2)):
            got_p = flat[(3 + p) * total + at:(3 + p) * total + at + n]
            size = sum(float(np.abs(G[s] * wet[s][c]).max()) for s in range(S))
            bound = S * (2 * S + 6) * rc.EPS * max(it["peak"], size) + sum(G[s] * eps[s][c] for s in range(S)) + rho * size
            err = float(np.abs(got_p - chans[p]).max())
            print("n=%4d chan %d: %.4f of its bound %.1e (max |chan| %.2f)" % (n, (2, 0)[p], err / bound, bound, np.abs(chans[p]).max()))
            assert err <= bound and bound < 1e-3 * np.abs(chans[p]).max()          # (and the bound is no licence)
        assert float(np.abs(flat[at:at + n] - mix).max()) <= S * (2 * S + 6) * rc.EPS * it["peak"] + sum(G[s] * eps[s][0] for s in range(S)) + rho * it["peak"]
        at += n


def test_in_an_anechoic_room_a_channel_lags_the_reference_by_the_geometric_time_difference(dev):
    """One source 47 samples (2.015 m) from the reference and 0.52 m more from the other microphone on the same line: 12.13
    samples later at 8 kHz."""
    from sepkern.data import mixed_pcm
    n, D47 = 3000, 47.0 * 343.0 / 8000.0
    x = torch.from_numpy(rc.signal(n, 500).copy())
    room = {"L": np.array([[6.0, 5.0, 3.0]]), "beta": np.zeros((1, 6)), "mics": np.array([[[1.0 + D47, 1.0, 1.0], [1.52 + D47, 1.0, 1.0]]]),
            "srcs": np.array([[[1.0, 1.0, 1.0]]]), "ntaps": [400], "rate": 8000, "chans": [1]}
    got = mixed_pcm({"flat": x, "keys": ["source1"], "lens": [n], "mixing": {"amp": [[1.0]], "peak": [0.5]}, "room": room}, dev)
    torch.cuda.synchronize()
    assert got["keys"] == ["mix", "source1", "chan1"]
    f = got["flat"].cpu().numpy().astype(np.float64)
    ref, chan = f[:n], f[2 * n:]
    lag = 0.52 * 8000 / 343.0
    assert abs(lag - round(lag)) < 0.2 and round(lag) == 12
    xc = [float(np.dot(chan[k:], ref[:n - k])) if k >= 0 else float(np.dot(chan[:n + k], ref[-k:])) for k in range(-30, 31)]
    assert int(np.argmax(xc)) - 30 == 12
    # the reference is the dry source at the peak (a unit direct path, aligned); the other channel is weaker by the distances' ratio
    dry = rc.signal(n, 500).astype(np.float64)
    assert np.abs(ref - dry * (0.5 / np.abs(dry).max())).max() < 1e-4
    assert abs(np.sqrt(np.mean(chan[100:] ** 2) / np.mean(ref[100:] ** 2)) - D47 / (D47 + 0.52)) < 0.02


def test_the_ipd_rows_of_a_room_batch_are_stft_ipd_on_the_mixed_signals(arch, corpus, dev):
    from sepkern import ops
    from sepkern.data import Prefetcher, features_from_pcm, ipd_rows_from_pcm, mixed_pcm
    items = _items(arch, corpus, ipd_channels=(1, 2))
    batch = arch.DynMixCollator()(items)
    pcm = batch["pcm"]
    res, wide = ipd_rows_from_pcm(pcm, dev)
    got = mixed_pcm(pcm, dev)
    ns, total = got["lens"], sum(got["lens"])
    starts = [sum(ns[:j]) for j in range(len(ns))]
    want, _ = ops.stft_ipd(got["flat"], [[q * total + st for st in starts] for q in (0, 3, 4)], ns, pk=res[2], want_mix=False)
    torch.cuda.synchronize()
    assert torch.equal(wide, want) and wide.shape[1] == 257 * 5 + 11 and bool(torch.isfinite(wide).all())
    plain = features_from_pcm({"flat": got["flat"], "keys": got["keys"], "lens": ns}, dev)
    assert torch.equal(res[0], plain[0]) and all(torch.equal(a, b) for a, b in zip(res[1], plain[1]))
    assert torch.equal(wide[:, :257], res[0])                                # the loss kernels' mixture rows are the magnitude columns
    assert float(wide[:res[2].R, 257:3 * 257].abs().max()) > 0.5             # phase features, not zeros
    staged = Prefetcher.stage(batch, dev)
    assert staged["ipd_keys"] == ["chan1", "chan2"] and torch.equal(staged["ipd"], wide) and torch.equal(staged["packed"][0], res[0])


def test_a_batch_without_a_room_takes_the_path_it_took_and_a_mono_room_never_mixes_channels(arch, corpus, dev, monkeypatch):
    from sepkern import _lib
    from sepkern.data import features_from_pcm, psa_features_from_pcm, wave_features_from_pcm
    items = _items(arch, corpus, ipd_channels=(1, 2))
    col = arch.DynMixCollator()
    array = col(items)["pcm"]
    mono = col([dict(it, room=dict(it["room"], mics=it["room"]["mics"][:1], chans=[])) for it in items])["pcm"]
    dry = col([{k: v for k, v in it.items() if k != "room"} for it in items])["pcm"]
    entry = []
    real_call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (entry.append(name), real_call(name, *a))[1])
    new = {"sk_room_rirs", "sk_room_workspace_bytes", "sk_mix_channels"}
    for fn in (features_from_pcm, wave_features_from_pcm, psa_features_from_pcm):
        del entry[:]
        fn(dry, dev)
        plain = list(entry)
        assert plain[0] == "sk_dynamic_mix" and not new & set(plain)
        del entry[:]
        fn(mono, dev)
        assert entry == ["sk_room_rirs", "sk_fir_convolve"] + plain            # one of each in front, and the launches it made before
        del entry[:]
        fn(array, dev)
        assert entry == ["sk_room_rirs", "sk_fir_convolve", "sk_dynamic_mix", "sk_mix_channels"] + plain[1:]
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5: training on it
def test_driver_trains_an_ipd_model_in_simulated_rooms_and_a_restart_continues_exactly(arch, tmp_path, monkeypatch):
    """Two epochs of steps/train_qsub.py --dynamic-mix --mix-room-t60 0.05,0.1 --mix-array on a 2 x 64 IPD model (ipd_channels=1,2),
    8 utterances: finite losses, batches that carry rooms, and a run restarted with --start-epoch 1 ends on exactly the
    uninterrupted run's loss and weights (the checkpoint cadence is set to every epoch for it)."""
    import train_qsub
    data = rc.corpus(os.path.join(str(tmp_path), "data"), n_spk=4, n_utt=2, lengths=[5000 + 300 * i for i in range(8)])
    array = os.path.join(str(tmp_path), "array.txt")
    open(array, "w").write("0 0 0\n0.05 0 0\n0 0.08 0\n")
    monkeypatch.setattr(train_qsub, "CHECKPOINT_EVERY", 1)
    seen = {}
    real = arch.compute_loss

    def spy(model, epoch, batch, *a):
        seen.setdefault(epoch, batch["pcm"])
        return real(model, epoch, batch, *a)
    monkeypatch.setattr(arch, "compute_loss", spy)
    conf = os.path.join(str(tmp_path), "conf")
    open(conf, "w").write("hidden_dim=64\nnum_layers=2\nnum_spk=2\nipd_channels=1,2\n")
    straight, resumed = os.path.join(str(tmp_path), "straight"), os.path.join(str(tmp_path), "resumed")
    common = ["uPIT", "0", data, None, "--model-config", conf, "--wav-input", "--dynamic-mix", "--mix-room-t60", "0.05,0.1",
              "--mix-array", array, "--batch-size", "4", "--mixes-per-epoch", "8", "--mix-max-samples", "4000", "--seed", "5",
              "--num-workers", "0", "--prefetch", "0"]

    def argv(out, *more):
        return [out if a is None else a for a in common] + list(more)
    train_qsub.main(argv(straight, "--num-epochs", "2"))
    assert sorted(seen) == [0, 1] and "room" in seen[0] and "mixing" in seen[0] and seen[0]["room"]["chans"] == [1, 2]
    assert all(400 <= t <= 800 for t in seen[0]["room"]["ntaps"]) and seen[0]["room"]["mics"].shape == (4, 3, 3)
    assert not np.array_equal(seen[0]["room"]["L"], seen[1]["room"]["L"])
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
    assert torch.equal(seen[1]["flat"], first_of_epoch_2["flat"])
    assert all(np.array_equal(seen[1]["room"][k], first_of_epoch_2["room"][k]) for k in ("L", "beta", "mics", "srcs"))
    assert open(os.path.join(resumed, "train_stats", "train_loss.txt")).read().splitlines() == lines
    a = torch.load(os.path.join(straight, "final.mdl"), map_location="cpu")
    b = torch.load(os.path.join(resumed, "final.mdl"), map_location="cpu")
    assert all(torch.equal(a[k], b[k]) for k in a)
