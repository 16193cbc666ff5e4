"""Simulated rooms on the host: the image-method definition (sepkern/room.py ism_rir) against closed forms, the float32
restatement of sk_room_rirs inside the unit the GPU test counts in -- and, with ONE fault switched on, at least 100 times
outside it --, the room draws, mixing.mix_channels, the collator's 'room' block, the driver's options and the entry points'
refusals.  Run with -s for the measured ratios."""
import argparse
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT
import _reverb_cases as rc
import _room_cases as rm

sys.path.insert(0, os.path.join(PKG, "archs"))
sys.path.insert(0, os.path.join(PKG, "steps"))

RATE, CS = rm.RATE, rm.C_SOUND
ROOM = (5.0, 4.0, 3.0)


def _kernel(tau, A, ntaps):
    """One image by the definition's words: taps floor(tau) - 31 .. + 32, A window(t) sinc(t), t = n - tau."""
    h = np.zeros(ntaps)
    for n in range(int(np.floor(tau)) - 31, int(np.floor(tau)) + 33):
        if 0 <= n < ntaps:
            t = n - tau
            h[n] += A * 0.5 * (1.0 + np.cos(2.0 * np.pi * t / 64.0)) * np.sinc(t)
    return h


# ------------------------------------------------------------------------------------------------ 1: closed forms of the definition
def test_an_anechoic_direct_path_of_exactly_40_samples_is_a_unit_impulse():
    from sepkern import room
    h = room.ism_rir(ROOM, [0.0] * 6, (1.0, 1.0, 1.0), (1.0 + rm.D40, 1.0, 1.0), RATE, 100, scale=4.0 * np.pi * rm.D40)
    rest = float(np.abs(np.delete(h, 40)).max())
    print("tap 40 = 1 %+.1e, the largest other tap %.1e" % (h[40] - 1.0, rest))
    assert abs(h[40] - 1.0) < 1e-12 and rest < 1e-12


def test_swapping_source_and_microphone_changes_nothing():
    from sepkern import room
    L, beta, a, b = (3.1, 2.6, 2.3), rm.SIX, (1.1, 0.9, 1.3), (2.2, 1.7, 0.8)
    assert 6000 < room.count_images(L, beta, a, b, RATE, 700) < 8000
    h1, h2 = room.ism_rir(L, beta, a, b, RATE, 700), room.ism_rir(L, beta, b, a, RATE, 700)
    err = float(np.abs(h1 - h2).max())
    print("reciprocity: %.1e of max |h| = %.2e" % (err, np.abs(h1).max()))
    assert err < 1e-12 and np.abs(h1).max() > 1e-3


def test_a_fractional_delay_gives_the_windowed_sinc_samples():
    from sepkern import room
    d = 40.3 * CS / RATE
    h = room.ism_rir(ROOM, [0.0] * 6, (1.0, 1.2, 1.0), (1.0, 1.2, 1.0 + d), RATE, 60, scale=2.0)
    tau = d * RATE / CS
    want = _kernel(tau, 2.0 / (4.0 * np.pi * d), 60)
    assert np.abs(h - want).max() < 1e-13 and np.count_nonzero(want) == 60 - 9 and abs(tau - 40.3) < 1e-9


def test_one_reflecting_wall_gives_two_images():
    from sepkern import room
    s, m = np.array([1.0, 1.2, 1.0]), np.array([2.5, 2.0, 1.4])
    h = room.ism_rir(ROOM, [0.7, 0.0, 0.0, 0.0, 0.0, 0.0], s, m, RATE, 400)
    d1 = float(np.linalg.norm(s - m))
    d2 = float(np.linalg.norm(np.array([-s[0], s[1], s[2]]) - m))
    want = _kernel(d1 * RATE / CS, 1.0 / (4.0 * np.pi * d1), 400) + _kernel(d2 * RATE / CS, 0.7 / (4.0 * np.pi * d2), 400)
    assert np.abs(h - want).max() < 1e-13 and d2 > d1
    assert room.count_images(ROOM, [0.7, 0.0, 0.0, 0.0, 0.0, 0.0], s, m, RATE, 400) == 2


def test_the_image_count_is_a_brute_force_triple_loops():
    from sepkern import room
    L, beta, s, m, ntaps = (3.0, 2.5, 2.2), (0.9, 0.8, 0.9, 0.0, 0.7, 0.9), (1.0, 1.1, 0.9), (2.1, 1.4, 1.3), 200
    M = room.image_range(L, RATE, ntaps)
    count = 0
    for mx in range(-M[0] - 1, M[0] + 2):                  # (one shell more than the stated range: it must hold nothing)
        for my in range(-M[1] - 1, M[1] + 2):
            for mz in range(-M[2] - 1, M[2] + 2):
                for p in range(8):
                    pp, mm = [(p >> a) & 1 for a in range(3)], (mx, my, mz)
                    R = [(1 - 2 * pp[a]) * s[a] + 2 * mm[a] * L[a] - m[a] for a in range(3)]
                    A = 1.0
                    for a in range(3):
                        for b_, e in ((beta[2 * a], abs(mm[a] - pp[a])), (beta[2 * a + 1], abs(mm[a]))):
                            A *= 1.0 if e == 0 else b_ ** e
                    tau = np.sqrt(sum(r * r for r in R)) * RATE / CS
                    inside = A != 0.0 and np.floor(tau) - 31 <= ntaps - 1
                    assert not inside or all(abs(mm[a]) <= M[a] for a in range(3))
                    count += int(inside)
    assert count == room.count_images(L, beta, s, m, RATE, ntaps) and count > 50


def test_eyring_beta_inverts_the_eyring_formula_and_bad_arguments_are_refused():
    from sepkern import room
    for L, t60 in (((6.0, 5.0, 3.0), 0.3), ((8.0, 6.0, 3.5), 0.5), ((3.0, 3.0, 2.5), 0.2)):
        beta = room.eyring_beta(L, t60)
        assert beta.shape == (6,) and len(set(beta.tolist())) == 1 and 0.0 < beta[0] < 1.0
        V, S = L[0] * L[1] * L[2], 2.0 * (L[0] * L[1] + L[1] * L[2] + L[0] * L[2])
        alpha = 1.0 - beta[0] ** 2
        assert abs((24.0 * np.log(10.0) / CS) * V / (-S * np.log(1.0 - alpha)) - t60) < 1e-12
    assert "NOMINAL" in room.eyring_beta.__doc__
    for bad in (dict(L=(0.0, 4.0, 3.0)), dict(beta=[1.1] * 6), dict(src=(5.0, 1.0, 1.0)), dict(mic=(1.0, 1.0, 0.0)),
                dict(mic=(1.005, 1.0, 1.0)), dict(rate=0.5), dict(ntaps=0), dict(ntaps=8193)):
        kw = dict(dict(L=ROOM, beta=[0.5] * 6, src=(1.0, 1.0, 1.0), mic=(2.0, 1.0, 1.0), rate=RATE, ntaps=100), **bad)
        with pytest.raises(ValueError):
            room.ism_rir(**kw)
    assert room.direct_delay((1.0, 1.0, 1.0), (1.0 + rm.D40 * 1.0124, 1.0, 1.0), RATE) == 40
    assert room.direct_delay((1.0, 1.0, 1.0), (1.0 + rm.D40 * 1.0126, 1.0, 1.0), RATE) == 41


# ------------------------------------------------------------------------------------------------ 2: the float32 restatement
@pytest.mark.parametrize("case", range(len(rm.F32_CASES)))
def test_the_float32_restatement_stays_within_the_unit_and_one_fault_is_100_times_outside(case):
    """|ism_rir_f32 - ism_rir| <= u[n] = 2^-24 sum |A_i| over the images that cover tap n; with ONE fault at least 100 u."""
    from sepkern import room
    L, beta, src, mic, ntaps = rm.F32_CASES[case]
    want, u = room.ism_rir(L, beta, src, mic, RATE, ntaps, want_unit=True)
    live = u > 0
    got = room.ism_rir_f32(L, beta, src, mic, RATE, ntaps)
    assert got.dtype == np.float32 and np.all(got[~live] == 0.0) and live.sum() > ntaps // 2
    ratio = float(np.max(np.abs(got[live] - want[live]) / u[live]))
    print("case %d (%d images): float32 %.2f u, %.1e of max |h|" % (case, room.count_images(L, beta, src, mic, RATE, ntaps), ratio,
                                                                   np.abs(got - want).max() / np.abs(want).max()))
    assert ratio <= 1.0
    for fault in rm.FAULTS:
        bad = room.ism_rir_f32(L, beta, src, mic, RATE, ntaps, **fault)
        r = float(np.max(np.abs(bad[live] - want[live]) / u[live]))
        print("   %-24s %.0f u" % (fault, r))
        assert r >= 100.0, fault
    assert np.array_equal(got, room.ism_rir_f32(L, beta, src, mic, RATE, ntaps))


def test_a_unit_built_from_the_taps_own_size_would_not_work():
    """At the sinc's zero crossings a float32 term is wrong by many times its own size: the unit has to come from |A|."""
    from sepkern import room
    h = room.ism_rir(ROOM, [0.0] * 6, (1.0, 1.0, 1.0), (1.0 + rm.D40, 1.0, 1.0), RATE, 100, scale=4.0 * np.pi * rm.D40)
    g = room.ism_rir_f32(ROOM, [0.0] * 6, (1.0, 1.0, 1.0), (1.0 + rm.D40, 1.0, 1.0), RATE, 100, scale=4.0 * np.pi * rm.D40)
    u = room.tap_unit(ROOM, [0.0] * 6, (1.0, 1.0, 1.0), (1.0 + rm.D40, 1.0, 1.0), RATE, 100, scale=4.0 * np.pi * rm.D40)
    assert np.all(np.abs(g - h) <= u) and abs(u[40] - 2.0 ** -24) < 1e-12 and u[80] == 0.0 and g[80] == 0.0


# ------------------------------------------------------------------------------------------------ 3: the draws
def test_draw_room_keeps_its_distances_and_is_a_function_of_the_rng():
    from sepkern import room
    arr = rm.array3()
    for seed in range(40):
        r = room.draw_room(np.random.default_rng(seed), (3, 3, 2.5), (8, 6, 4), (0.2, 0.6), arr, 3, margin=0.5, min_dist=0.7)
        again = room.draw_room(np.random.default_rng(seed), (3, 3, 2.5), (8, 6, 4), (0.2, 0.6), arr, 3, margin=0.5, min_dist=0.7)
        assert sorted(r) == sorted(again) and all(np.array_equal(r[k], again[k]) for k in r)
        L = r["L"]
        assert np.all(L >= (3, 3, 2.5)) and np.all(L <= (8, 6, 4)) and 0.2 <= r["t60"] <= 0.6 and 0.0 <= r["yaw"] < 2.0 * np.pi
        assert np.array_equal(r["beta"], room.eyring_beta(L, r["t60"]))
        for x in list(r["mics"]) + list(r["srcs"]) + [r["centre"]]:
            assert np.all(x >= 0.5) and np.all(x <= L - 0.5)
        assert r["mics"].shape == (3, 3) and r["srcs"].shape == (3, 3)
        assert all(np.linalg.norm(x - r["centre"]) >= 0.7 for x in r["srcs"])
        # the array is rotated about the vertical, not bent
        assert np.allclose(np.linalg.norm(r["mics"][1] - r["mics"][0]), 0.05) and np.allclose(r["mics"][:, 2], r["centre"][2])
        c, s = np.cos(r["yaw"]), np.sin(r["yaw"])
        assert np.allclose(r["mics"][1] - r["centre"], [0.05 * c, 0.05 * s, 0.0])
    a = room.draw_room(np.random.default_rng(1), (3, 3, 2.5), (8, 6, 4), (0.2, 0.6), arr, 2)
    b = room.draw_room(np.random.default_rng(2), (3, 3, 2.5), (8, 6, 4), (0.2, 0.6), arr, 2)
    assert not np.array_equal(a["L"], b["L"])
    with pytest.raises(ValueError, match="no place for a source"):
        room.draw_room(np.random.default_rng(0), (2, 2, 2), (2, 2, 2), (0.2, 0.3), arr, 1, margin=0.5, min_dist=3.0)
    with pytest.raises(ValueError, match="no place for the array"):
        room.draw_room(np.random.default_rng(0), (2, 2, 2), (2, 2, 2), (0.2, 0.3), arr * 30.0, 1, margin=0.5)
    with pytest.raises(ValueError, match="leaves nothing"):
        room.draw_room(np.random.default_rng(0), (1, 1, 1), (1, 1, 1), (0.2, 0.3), arr, 1, margin=0.5)


def test_read_array(tmp_path):
    from sepkern import room
    text = "# a triangle\n0 0 0\n0.05 0 0\n\n0 0.08 0   # the third\n"
    path = os.path.join(str(tmp_path), "array.txt")
    open(path, "w").write(text)
    assert np.array_equal(room.read_array(path), rm.array3()) and np.array_equal(room.read_array(text), rm.array3())
    for bad, word in (("0 0\n", "three numbers"), ("0 0 x\n", "three numbers"), ("", "0 microphones"), ("0 0 0\n" * 9, "9 microphones")):
        with pytest.raises(ValueError, match=word):
            room.read_array(bad + "\n")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return rc.corpus(str(tmp_path_factory.mktemp("room")))


def test_items_with_a_room_carry_what_plain_items_carry_bit_for_bit(data):
    import uPIT
    from sepkern import room
    plain = uPIT.DynMixTrainSet(data, 2, seed=5, peak=(0.5, 0.9))
    kw = dict(room_t60=(0.1, 0.3), array=rm.array3(), ipd_ref=1, ipd_channels=(2, 0))
    ds, again = uPIT.DynMixTrainSet(data, 2, seed=5, peak=(0.5, 0.9), **kw), uPIT.DynMixTrainSet(data, 2, seed=5, peak=(0.5, 0.9), **kw)
    taps = set()
    for i in range(10):
        it, dry = ds[i], plain[i]
        assert sorted(dry) == ["amp", "peak", "source1", "source2"] and sorted(it) == sorted(list(dry) + ["room"])
        assert all(np.array_equal(it[k], dry[k]) for k in dry) and ds.draw(i) == plain.draw(i)
        r = it["room"]
        want = room.draw_room(np.random.default_rng([5, i, 2]), (3, 3, 2.5), (8, 6, 4), (0.1, 0.3), rm.array3(), 2)
        assert sorted(r) == ["L", "beta", "chans", "mics", "ntaps", "rate", "srcs"] and r["chans"] == [2, 0] and r["rate"] == 8000
        assert np.array_equal(r["L"], want["L"]) and np.array_equal(r["beta"], want["beta"]) and np.array_equal(r["srcs"], want["srcs"])
        assert np.array_equal(r["mics"], want["mics"][[1, 2, 0]]) and r["mics"].dtype == np.float64      # only the listed ones travel
        assert r["ntaps"] == min(int(round(want["t60"] * 8000)), 8192) and 800 <= r["ntaps"] <= 2400
        assert all(np.array_equal(r[k], again[i]["room"][k]) for k in r)
        taps.add(r["ntaps"])
    assert len(taps) > 5
    mono = uPIT.DynMixTrainSet(data, 2, seed=5, room_t60=(0.1, 0.3))[0]["room"]
    assert mono["mics"].shape == (1, 3) and mono["chans"] == []
    for kw, word in ((dict(room_t60=(0.1, 0.3), rir_synth=(0.1, 0.2)), "give one of them"), (dict(array=rm.array3()), "need simulated rooms"),
                     (dict(ipd_channels=(1,)), "need simulated rooms"), (dict(room_t60=(0.3, 0.1)), "room_t60"),
                     (dict(room_t60=(0.1, 0.3), array=rm.array3(), ipd_channels=(3,)), "3 microphone"),
                     (dict(room_t60=(0.02, 0.3)), "direct path across the largest room")):
        with pytest.raises(ValueError, match=word):
            uPIT.DynMixTrainSet(data, 2, **kw)


def test_the_collators_room_block_follows_the_batch_order(data):
    import uPIT
    ds = uPIT.DynMixTrainSet(data, 2, seed=5, room_t60=(0.1, 0.3), array=rm.array3(), ipd_channels=(1, 2))
    plain = uPIT.DynMixTrainSet(data, 2, seed=5)
    items = [ds[i] for i in range(5)]
    pcm = ds.collator(items)["pcm"]
    dry = plain.collator([plain[i] for i in range(5)])["pcm"]
    assert "room" not in dry and sorted(pcm) == sorted(list(dry) + ["room"])
    assert torch.equal(pcm["flat"], dry["flat"]) and all(pcm[k] == dry[k] for k in ("lens", "mixing", "keys"))
    order = np.argsort(np.array([1 + len(d["source1"]) // 128 for d in items]))[::-1]
    r = pcm["room"]
    assert sorted(r) == ["L", "beta", "chans", "mics", "ntaps", "rate", "srcs"] and r["chans"] == [1, 2] and r["rate"] == 8000
    assert r["L"].shape == (5, 3) and r["beta"].shape == (5, 6) and r["mics"].shape == (5, 3, 3) and r["srcs"].shape == (5, 2, 3)
    for j, i in enumerate(order):
        want = items[i]["room"]
        assert all(np.array_equal(r[k][j], want[k]) for k in ("L", "beta", "mics", "srcs")) and r["ntaps"][j] == want["ntaps"]
        assert r["L"].dtype == np.float64
    with pytest.raises(ValueError, match="every item of its batch"):
        ds.collator([items[0], plain[1]])
    from sepkern.data import batch_chan_keys
    assert batch_chan_keys(pcm) == ["chan1", "chan2"] and batch_chan_keys(dry) == []
    assert batch_chan_keys({"keys": ["mix", "source1", "chan3"]}) == ["chan3"]


# ------------------------------------------------------------------------------------------------ 4: the other channels' rule
@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_mix_channels_is_the_sum_at_the_reference_channels_gains(S):
    from sepkern import mixing
    rng = np.random.default_rng(S)
    ref = [rng.standard_normal(500) * 0.1 for _ in range(S)]
    other = [[rng.standard_normal(500) * 0.1 for _ in range(S)] for _ in range(2)]
    amp = [1.0, 0.7, 1.3, 0.9][:S]
    mix, _, G = mixing.mix(ref, amp, 0.8)
    outs = mixing.mix_channels([ref] + other, G)
    assert np.array_equal(outs[0], mix) and len(outs) == 3
    for p in range(2):
        want = np.zeros(500)
        for s in range(S):
            want += G[s] * other[p][s]
        assert np.abs(outs[1 + p] - want).max() < 1e-15
    # quantized: the reference channel is mix's quantized mixture; a louder channel exceeds the peak and clips
    loud = [[40.0 * x for x in ref]]
    q = mixing.mix_channels([ref] + loud, G, quantized=True)
    assert np.array_equal(q[0], mixing.mix(ref, amp, 0.8, quantized=True)[0])
    assert q[1].max() == 32767.0 / 32768.0 and q[1].min() == -1.0 and np.abs(mix).max() <= 0.8 + 1e-12
    with pytest.raises(ValueError):
        mixing.mix_channels([ref[:-1] + [ref[-1][:-1]]] if S > 1 else [[]], G)


# ------------------------------------------------------------------------------------------------ 5: the driver's options
def _conf(tmp_path, text):
    path = os.path.join(str(tmp_path), "conf")
    open(path, "w").write(text)
    return path


def test_train_qsub_room_options(data, tmp_path):
    import train_qsub
    import uPIT
    array = os.path.join(str(tmp_path), "array.txt")
    open(array, "w").write("0 0 0\n0.05 0 0\n0 0.08 0\n")
    base = ["uPIT", "0", data, "out"]
    for opt in (["--mix-room-t60", "0.2,0.6"], ["--mix-array", array], ["--mix-room-dims", "3,3,2.5:5,4,3"]):
        with pytest.raises(SystemExit, match=opt[0] + ".*needs.*--dynamic-mix"):
            train_qsub.get_args(base + ["--wav-input"] + opt)
    dyn = base + ["--wav-input", "--dynamic-mix"]
    for other in (["--mix-rir-synth", "0.2,0.6"], ["--mix-rir-scp", "rir.scp"]):
        with pytest.raises(SystemExit, match="--mix-room-t60.*" + other[0] + ".*give one of them"):
            train_qsub.get_args(dyn + ["--mix-room-t60", "0.2,0.6"] + other)
    with pytest.raises(SystemExit, match="--mix-array.*needs.*--mix-room-t60"):
        train_qsub.get_args(dyn + ["--mix-array", array])
    with pytest.raises(SystemExit, match="--mix-room-dims.*needs.*--mix-room-t60"):
        train_qsub.get_args(dyn + ["--mix-room-dims", "3,3,2.5:5,4,3"])
    for bad in (["--mix-room-t60", "0.6,0.2"], ["--mix-room-t60", "0.2,0.6", "--mix-room-dims", "3,3:5,4,3"],
                ["--mix-room-t60", "0.2,0.6", "--mix-room-dims", "6,3,2.5:5,4,3"]):
        with pytest.raises(SystemExit):
            train_qsub.get_args(dyn + bad)
    assert train_qsub.room_options(train_qsub.get_args(dyn)) == {}
    rooms = dyn + ["--mix-room-t60", "0.05,0.1", "--seed", "3", "--prefetch", "0", "--num-workers", "0", "--batch-size", "3",
                   "--mixes-per-epoch", "6"]

    # an IPD model: only in simulated rooms with an array that has its microphones
    ipd = _conf(tmp_path, "num_spk=2\nhidden_dim=64\nipd_channels=1,2\n")
    with pytest.raises(SystemExit, match="^`ipd_channels` does not train with `--dynamic-mix`"):
        train_qsub.ipd_model(uPIT, train_qsub.get_args(dyn + ["--model-config", ipd]))
    with pytest.raises(SystemExit, match="^`ipd_channels` does not train with `--dynamic-mix`.*--mix-array"):
        train_qsub.ipd_model(uPIT, train_qsub.get_args(rooms + ["--model-config", ipd]))
    two = os.path.join(str(tmp_path), "two.txt")
    open(two, "w").write("0 0 0\n0.05 0 0\n")
    with pytest.raises(SystemExit, match="has 2 microphone.*needs 3"):
        train_qsub.ipd_model(uPIT, train_qsub.get_args(rooms + ["--model-config", ipd, "--mix-array", two]))
    with pytest.raises(SystemExit, match="--mix-array.*no file"):
        train_qsub.room_options(train_qsub.get_args(rooms + ["--mix-array", two + ".missing"]))
    args = train_qsub.get_args(rooms + ["--model-config", ipd, "--mix-array", array, "--mix-room-dims", "3,3,2.5:5,4,3"])
    args.ipd = train_qsub.ipd_model(uPIT, args)
    assert args.ipd == {"ipd_ref": 0, "ipd_channels": (1, 2)}
    loader, draws = train_qsub.training_batches(uPIT, args, 0, 1)
    ds = loader.dataset
    assert ds.room_t60 == (0.05, 0.1) and ds.room_dims == ((3.0, 3.0, 2.5), (5.0, 4.0, 3.0)) and ds.ipd_channels == (1, 2) and len(ds.array) == 3
    draws.set_epoch(0)
    batches = list(loader)
    assert len(batches) == 2 and all(b["pcm"]["room"]["chans"] == [1, 2] and b["pcm"]["room"]["mics"].shape == (3, 3, 3) for b in batches)
    assert all(400 <= t <= 800 for b in batches for t in b["pcm"]["room"]["ntaps"])

    # a mono model with rooms and no array: one microphone, wherever --mix-rir-synth trains
    for loss in ("mse", "psa", "sisdr", "mixit"):
        mono = _conf(tmp_path, "num_spk=2\nhidden_dim=64\nloss=%s\n" % loss)
        a = train_qsub.get_args(rooms + ["--model-config", mono])
        b = train_qsub.get_args(dyn + ["--mix-rir-synth", "0.05,0.1", "--model-config", mono])
        assert train_qsub.ipd_model(uPIT, a) == {} and train_qsub.waveform_loss(uPIT, a) == train_qsub.waveform_loss(uPIT, b)
        assert train_qsub.prefetch_targets(uPIT, a) == train_qsub.prefetch_targets(uPIT, b)
        a.ipd = {}
        ds = train_qsub.training_batches(uPIT, a, 0, 1)[0].dataset
        assert ds.room_t60 == (0.05, 0.1) and ds.array.shape == (1, 3) and ds[0]["room"]["chans"] == [] and not ds.reverb
    # without the options the set is built as before
    plain = train_qsub.training_batches(uPIT, train_qsub.get_args(dyn + ["--model-config", mono, "--prefetch", "0", "--num-workers", "0",
                                                                        "--seed", "3"]), 0, 1)[0].dataset
    assert plain.room_t60 is None and "room" not in plain[0]


def test_a_batch_to_be_mixed_without_a_room_keeps_its_error():
    from sepkern.data import ipd_rows_from_pcm
    with pytest.raises(ValueError, match="has one channel"):
        ipd_rows_from_pcm({"mixing": {}, "keys": ["source1", "source2"], "lens": [300], "flat": torch.zeros(600, dtype=torch.int16)}, "cpu")


# ------------------------------------------------------------------------------------------------ 6: the ABI
def test_header_library_and_ctypes_table_have_the_symbols():
    from sepkern import _lib
    text = open(os.path.join(ROOT, "include", "sepkern.h")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name, nargs in (("sk_room_rirs", 12), ("sk_room_workspace_bytes", 9), ("sk_mix_channels", 11)):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and len(_lib.PROTOTYPES[name][1]) == nargs
    assert _lib.PROTOTYPES["sk_room_workspace_bytes"][0] is C.c_size_t
    assert "room.hip" in open(os.path.join(PKG, "csrc", "Makefile")).read()


def test_the_entry_points_refuse_bad_arguments_before_they_touch_a_device():
    from sepkern import _lib
    lib = _lib.load()
    rm.check_refusals(lib)
    one = (C.c_int64 * 1)(0)
    for S, P, B, word in ((0, 1, 1, b"S = 0"), (5, 1, 1, b"S = 5"), (2, 0, 1, b"P = 0"), (2, 8, 1, b"P = 8"), (2, 1, 0, b"B = 0"),
                          (2, 1, 65536, b"B = 65536"), (2, 1, 1, b"null pointer")):
        assert lib.sk_mix_channels(None, one, None, B, S, P, None, 0, None, one, None) == -1 and word in lib.sk_last_error()
