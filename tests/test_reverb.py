"""Reverberant dynamic mixing without a GPU: the definition (sepkern/reverb.py convolve) against np.convolve, the float32
restatement of sk_fir_convolve's algorithm against the definition -- and against itself with one fault put in, which is what shows
that the shapes used here and in tests/test_gpu_reverb.py would catch a wrong partition, block or delay --, synthetic and measured
RIRs, the draws of archs/uPIT.py's DynMixTrainSet, DynMixCollator's 'reverb' block, the driver's options and the entry point's
argument checks."""
import ctypes as C
import os
import re
import sys
import wave

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT
import _reverb_cases as rc

sys.path.insert(0, os.path.join(PKG, "archs"))
sys.path.insert(0, os.path.join(PKG, "steps"))

CASES = rc.case_list([257, 1000, 4355], [1, 256, 257, 700, 4097])


def test_the_cases_cover_what_they_are_meant_to():
    assert len(CASES) == 3 * (1 + 2 + 2 + 4 + 4)
    assert any(L > n for n, L, d in CASES) and any(d == L - 1 and L > 1 for n, L, d in CASES) and (4355, 4097, 4096) in CASES


# ------------------------------------------------------------------------------------------------ 1: the definition
@pytest.mark.parametrize("n,L,d", CASES)
def test_convolve_is_np_convolve_cut_at_the_delay(n, L, d):
    from sepkern import reverb
    x, h = rc.signal(n, 100), rc.rir(L)
    y = reverb.convolve(x, h, d)
    want = np.convolve(x.astype(np.float64) / 32768.0, h.astype(np.float64))[d:d + n]
    assert y.dtype == np.float64 and y.shape == (n,)
    assert np.abs(y - want).max() <= 1e-12 * np.abs(want).max()
    # float samples are taken as they are
    assert np.array_equal(reverb.convolve(x.astype(np.float64) / 32768.0, h, d), y)


@pytest.mark.parametrize("d", [0, 1, 255, 256, 300, 4096])
def test_a_unit_impulse_at_the_delay_returns_the_signal(d):
    from sepkern import reverb
    h = np.zeros(d + 3, dtype=np.float32)
    h[d] = 1.0
    x = rc.signal(1000, 7)
    assert reverb.direct_delay(h) == d
    assert np.array_equal(reverb.convolve(x, h, d), x.astype(np.float64) / 32768.0)
    assert np.abs(reverb.convolve_partitioned_f32(x, h, d) - x / 32768.0).max() <= 8 * rc.gate(x, h)


def test_direct_delay_is_the_first_largest_tap_and_bad_arguments_are_refused():
    from sepkern import reverb
    assert reverb.direct_delay(np.array([0.1, -0.9, 0.9, 0.2])) == 1 and reverb.direct_delay([1.0]) == 0
    x, h = rc.signal(300), rc.rir(256)
    for bad in (-1, 256, 1000):
        with pytest.raises(ValueError, match="delay"):
            reverb.convolve(x, h, bad)
        with pytest.raises(ValueError, match="delay"):
            reverb.convolve_partitioned_f32(x, h, bad)
    with pytest.raises(ValueError):
        reverb.convolve(x[:0], h, 0)
    with pytest.raises(ValueError):
        reverb.convolve(x, h[:0], 0)


# ------------------------------------------------------------------------------------------------ 2: the float32 restatement
def _errors(n, L, d, **fault):
    from sepkern import reverb
    x, h = rc.signal(n, 100), rc.rir(L)
    y = reverb.convolve_partitioned_f32(x, h, d, **fault)
    assert y.dtype == np.float32 and y.shape == (n,)
    return float(np.abs(y.astype(np.float64) - reverb.convolve(x, h, d)).max()) / rc.gate(x, h)


@pytest.mark.parametrize("n,L,d", CASES)
def test_the_partitioned_float32_form_stays_within_8_gates(n, L, d):
    """Within 8 x 2^-24 ||h||_2 max|x| of the definition (measured 0.2 .. 4.3 of that unit at such shapes; a property of the
    restatement on numpy / scipy, not of the kernel)."""
    e = _errors(n, L, d)
    print("n=%4d L=%4d d=%4d: %.2f of 2^-24 |h| max|x|" % (n, L, d, e))
    assert e <= 8.0


def _blocks(n, d):
    return (d + n - 1) // 256 - d // 256 + 1


FAULTY = [(n, L, d) for n, L, d in CASES if -(-L // 256) >= 2 or _blocks(n, d) > 1]


@pytest.mark.parametrize("n,L,d", FAULTY)
def test_one_fault_in_the_algorithm_is_a_hundred_times_outside_that_bound(n, L, d):
    """Each fault alone, on every case with K >= 2 or more than one block: the block history started one block late, the delay
    off by one (either way), and the last partition dropped.  The last of them is only a fault where the definition reads that
    partition at all: tap k meets sample i + d - k of the signal for an output i in [0, n) only if |k - d| < n, so a last
    partition that starts at 256 (K - 1) >= d + n (a RIR longer than signal plus delay, e.g. n = 257, L = 4097, d = 0)
    multiplies nothing but the zeros beyond the signal, and leaving it out changes no output; those cases are skipped for that
    fault alone and checked to be exact instead."""
    K = -(-L // 256)
    assert _errors(n, L, d, late_history=True) >= 800.0
    assert _errors(n, L, d, delay_error=1) >= 800.0
    assert _errors(n, L, d, delay_error=-1) >= 800.0
    if 256 * (K - 1) - d < n:
        assert _errors(n, L, d, drop_last_partition=True) >= 800.0
    else:
        assert _errors(n, L, d, drop_last_partition=True) <= 8.0


def test_int16_and_float32_samples_give_the_restatement_the_same_bits():
    from sepkern import reverb
    x, h = rc.signal(1000, 5), rc.rir(700)
    a = reverb.convolve_partitioned_f32(x, h, 300)
    b = reverb.convolve_partitioned_f32(x.astype(np.float32) / np.float32(32768.0), h, 300)
    assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 3: RIRs
@pytest.mark.parametrize("t60,rate,drr", [(0.3, 8000, 5.0), (0.6, 8000, 0.0), (0.1, 16000, 15.0), (2.0, 8000, 10.0)])
def test_synthetic_rir(t60, rate, drr):
    from sepkern import reverb
    h = reverb.synthetic_rir(np.random.default_rng(3), t60, rate, drr)
    again = reverb.synthetic_rir(np.random.default_rng(3), t60, rate, drr)
    other = reverb.synthetic_rir(np.random.default_rng(4), t60, rate, drr)
    assert h.dtype == np.float32 and np.array_equal(h, again) and not np.array_equal(h, other)
    assert len(h) == min(int(round(t60 * rate)), reverb.MAX_TAPS) and reverb.MAX_TAPS == 8192
    assert h[0] == 1.0 and reverb.direct_delay(h) == 0
    tail = h[1:].astype(np.float64)
    assert abs(10.0 * np.log10(1.0 / np.sum(tail * tail)) - drr) <= 0.1
    # the envelope: the last tenth of a t60-long tail lies about 54 .. 60 dB below its first tenth
    if len(h) == int(round(t60 * rate)):
        m = len(tail) // 10
        drop = 10.0 * np.log10(np.mean(tail[:m] ** 2) / np.mean(tail[-m:] ** 2))
        assert 48.0 <= drop <= 60.0


def test_a_one_tap_synthetic_rir_is_the_identity():
    from sepkern import reverb
    assert np.array_equal(reverb.synthetic_rir(np.random.default_rng(0), 1.0 / 8000, 8000, 5.0), np.ones(1, dtype=np.float32))
    with pytest.raises(ValueError):
        reverb.synthetic_rir(np.random.default_rng(0), 1e-6, 8000, 5.0)


def _write_wav(path, data, rate, channels=1, width=2):
    with wave.open(path, "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(np.asarray(data).tobytes())


def test_load_rir(tmp_path):
    from sepkern import reverb
    t = str(tmp_path)
    pcm = np.array([0, 16384, -8192, 1, 0], dtype=np.int16)
    _write_wav(t + "/a.wav", pcm, 8000)
    h, cut = reverb.load_rir(t + "/a.wav", 8000)
    assert h.dtype == np.float32 and not cut and np.array_equal(h, pcm.astype(np.float32) / 32768.0)
    with pytest.raises(ValueError, match=re.escape(t + "/a.wav") + ".*8000 Hz.*16000"):
        reverb.load_rir(t + "/a.wav", 16000)
    _write_wav(t + "/stereo.wav", np.array([[1, 2], [3, 4]], dtype=np.int16), 8000, channels=2)
    with pytest.raises(ValueError, match="mono 16-bit"):
        reverb.load_rir(t + "/stereo.wav", 8000)
    _write_wav(t + "/bytes.wav", np.array([1, 2, 3], dtype=np.uint8), 8000, width=1)
    with pytest.raises(ValueError, match="mono 16-bit"):
        reverb.load_rir(t + "/bytes.wav", 8000)
    _write_wav(t + "/zero.wav", np.zeros(10, dtype=np.int16), 8000)
    with pytest.raises(ValueError, match="all-zero"):
        reverb.load_rir(t + "/zero.wav", 8000)
    _write_wav(t + "/empty.wav", np.zeros(0, dtype=np.int16), 8000)
    with pytest.raises(ValueError, match="empty"):
        reverb.load_rir(t + "/empty.wav", 8000)
    # npy: 1-D float, taken as it is; longer than MAX_TAPS is cut and said to be
    long = np.random.default_rng(0).standard_normal(9000)
    np.save(t + "/long.npy", long)
    h, cut = reverb.load_rir(t + "/long.npy", 8000)
    assert cut and h.dtype == np.float32 and np.array_equal(h, long[:8192].astype(np.float32))
    np.save(t + "/short.npy", long[:100].astype(np.float32))
    h, cut = reverb.load_rir(t + "/short.npy", 8000)
    assert not cut and np.array_equal(h, long[:100].astype(np.float32))
    np.save(t + "/2d.npy", np.ones((2, 5)))
    np.save(t + "/int.npy", np.ones(5, dtype=np.int32))
    np.save(t + "/zero.npy", np.zeros(5))
    for name, word in (("2d.npy", "1-D float"), ("int.npy", "1-D float"), ("zero.npy", "all-zero"), ("x.flac", "wav or a .npy")):
        with pytest.raises(ValueError, match=word):
            reverb.load_rir(t + "/" + name, 8000)
    open(t + "/rir.scp", "w").write("a %s/a.wav\n\nb %s/long.npy\n" % (t, t))
    rirs, ncut = reverb.read_rir_scp(t + "/rir.scp", 8000)
    assert len(rirs) == 2 and ncut == 1 and len(rirs[1]) == 8192


# ------------------------------------------------------------------------------------------------ 4: the draws and the collator
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return rc.corpus(str(tmp_path_factory.mktemp("reverb")))


def _same_item(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)


def test_reverberant_items_carry_what_plain_items_carry_bit_for_bit(data):
    import uPIT
    from sepkern import reverb
    plain = uPIT.DynMixTrainSet(data, 2, seed=5, peak=(0.5, 0.9))
    wet = uPIT.DynMixTrainSet(data, 2, seed=5, peak=(0.5, 0.9), rir_synth=(0.05, 0.2), rir_drr_db=(2.0, 12.0))
    again = uPIT.DynMixTrainSet(data, 2, seed=5, peak=(0.5, 0.9), rir_synth=(0.05, 0.2), rir_drr_db=(2.0, 12.0))
    assert not plain.reverb and wet.reverb
    items = [wet[i] for i in range(12)]
    for i, it in enumerate(items):
        dry = plain[i]
        assert sorted(dry) == ["amp", "peak", "source1", "source2"]
        assert sorted(it) == ["amp", "peak", "rir1", "rir2", "rir_delay", "source1", "source2"]
        assert all(np.array_equal(it[k], dry[k]) for k in dry) and wet.draw(i) == plain.draw(i)
        assert _same_item(it, again[i])
        for s in range(2):
            h = it["rir%d" % (s + 1)]
            assert h.dtype == np.float32 and 400 <= len(h) <= 1600 and h[0] == 1.0
            assert it["rir_delay"][s] == reverb.direct_delay(h) == 0
            drr = 10.0 * np.log10(1.0 / np.sum(h[1:].astype(np.float64) ** 2))
            assert 1.9 <= drr <= 12.1
    assert not any(_same_item(items[0], it) for it in items[1:])
    assert len({len(it["rir1"]) for it in items}) > 6 and not np.array_equal(items[0]["rir1"], items[0]["rir2"])
    other = uPIT.DynMixTrainSet(data, 2, seed=6, rir_synth=(0.05, 0.2))
    assert not np.array_equal(other[0]["rir1"], items[0]["rir1"])


def test_rir_prob_zero_gives_identity_rirs_and_a_half_gives_some(data):
    import uPIT
    off = uPIT.DynMixTrainSet(data, 3, seed=1, rir_synth=(0.05, 0.1), rir_prob=0.0)
    for i in range(4):
        it = off[i]
        assert it["rir_delay"] == [0, 0, 0] and all(np.array_equal(it["rir%d" % s], np.ones(1, dtype=np.float32)) for s in (1, 2, 3))
    half = uPIT.DynMixTrainSet(data, 2, seed=1, rir_synth=(0.05, 0.1), rir_prob=0.5)
    taps = [len(half[i]["rir%d" % s]) for i in range(20) for s in (1, 2)]
    assert 8 <= sum(t == 1 for t in taps) <= 32 and any(t > 1 for t in taps)


def test_rirs_from_an_scp_are_read_once_and_drawn_with_their_delay(data, tmp_path, capsys):
    import uPIT
    t = str(tmp_path)
    rng = np.random.default_rng(0)
    hs = []
    for j, (L, at) in enumerate([(300, 0), (9000, 40), (50, 7)]):
        h = rng.standard_normal(L) * 0.05
        h[at] = 1.0
        np.save("%s/r%d.npy" % (t, j), h)
        hs.append(h.astype(np.float32)[:8192])
    open(t + "/rir.scp", "w").write("".join("r%d %s/r%d.npy\n" % (j, t, j) for j in range(3)))
    ds = uPIT.DynMixTrainSet(data, 2, seed=2, rir_scp=t + "/rir.scp")
    assert "1 of the 3 RIRs" in capsys.readouterr().out and len(ds.rirs) == 3
    seen = set()
    for i in range(12):
        it = ds[i]
        for s in range(2):
            j = [k for k in range(3) if np.array_equal(hs[k], it["rir%d" % (s + 1)])]
            assert len(j) == 1 and it["rir_delay"][s] == (0, 40, 7)[j[0]]
            seen.add(j[0])
    assert seen == {0, 1, 2}
    # a wav RIR at another rate than the corpus's is refused when the set is built
    _write_wav(t + "/r16k.wav", np.array([100, 20000, 5], dtype=np.int16), 16000)
    open(t + "/bad.scp", "w").write("x %s/r16k.wav\n" % t)
    with pytest.raises(ValueError, match="r16k.wav.*16000 Hz.*8000"):
        uPIT.DynMixTrainSet(data, 2, rir_scp=t + "/bad.scp")
    assert len(uPIT.DynMixTrainSet(data, 2, rir_scp=t + "/bad.scp", sample_rate=16000).rirs) == 1
    with pytest.raises(ValueError, match="one of them"):
        uPIT.DynMixTrainSet(data, 2, rir_scp=t + "/rir.scp", rir_synth=(0.1, 0.2))
    with pytest.raises(ValueError, match="rir_prob"):
        uPIT.DynMixTrainSet(data, 2, rir_synth=(0.1, 0.2), rir_prob=1.5)
    with pytest.raises(ValueError, match="rir_synth"):
        uPIT.DynMixTrainSet(data, 2, rir_synth=(0.2, 0.1))


def test_the_collators_reverb_block_follows_the_batch_order(data):
    import uPIT
    wet = uPIT.DynMixTrainSet(data, 2, seed=5, rir_synth=(0.05, 0.2))
    plain = uPIT.DynMixTrainSet(data, 2, seed=5)
    items = [wet[i] for i in range(5)]
    pcm = wet.collator(items)["pcm"]
    dry = plain.collator([plain[i] for i in range(5)])["pcm"]
    assert "reverb" not in dry and sorted(pcm) == sorted(list(dry) + ["reverb"])
    assert torch.equal(pcm["flat"], dry["flat"]) and pcm["lens"] == dry["lens"] and pcm["mixing"] == dry["mixing"] and pcm["keys"] == dry["keys"]
    order = np.argsort(np.array([1 + len(d["source1"]) // 128 for d in items]))[::-1]
    assert pcm["lens"] == [len(items[i]["source1"]) for i in order]
    rv = pcm["reverb"]
    assert sorted(rv) == ["delay", "flat", "offs", "taps"] and rv["flat"].dtype == torch.float32 and rv["flat"].dim() == 1
    flat = rv["flat"].numpy()
    for s in range(2):
        for j, i in enumerate(order):
            h = items[i]["rir%d" % (s + 1)]
            assert rv["taps"][s][j] == len(h) and rv["delay"][s][j] == items[i]["rir_delay"][s]
            assert np.array_equal(flat[rv["offs"][s][j]:rv["offs"][s][j] + len(h)], h)
    assert sum(t for row in rv["taps"] for t in row) == len(flat)
    with pytest.raises(ValueError, match="every item of its batch"):
        wet.collator([items[0], plain[1]])


# ------------------------------------------------------------------------------------------------ 5: the driver's options
def test_train_qsub_reverb_options(data, tmp_path):
    import train_qsub
    import uPIT
    base = ["uPIT", "0", data, "out"]
    for opt in (["--mix-rir-synth", "0.2,0.6"], ["--mix-rir-scp", "rir.scp"], ["--mix-rir-prob", "0.5"]):
        with pytest.raises(SystemExit, match=opt[0] + ".*needs.*--dynamic-mix"):
            train_qsub.get_args(base + ["--wav-input"] + opt)
    dyn = base + ["--wav-input", "--dynamic-mix"]
    with pytest.raises(SystemExit, match="give one of them"):
        train_qsub.get_args(dyn + ["--mix-rir-synth", "0.2,0.6", "--mix-rir-scp", "rir.scp"])
    with pytest.raises(SystemExit, match="--mix-rir-prob.*needs"):
        train_qsub.get_args(dyn + ["--mix-rir-prob", "0.5"])
    with pytest.raises(SystemExit, match="probability"):
        train_qsub.get_args(dyn + ["--mix-rir-synth", "0.2,0.6", "--mix-rir-prob", "1.5"])
    with pytest.raises(SystemExit, match="--dynamic-mix.*needs.*--wav-input"):
        train_qsub.get_args(base + ["--dynamic-mix", "--mix-rir-synth", "0.2,0.6"])
    with pytest.raises(SystemExit):
        train_qsub.get_args(dyn + ["--mix-rir-synth", "0.6,0.2"])
    plain = train_qsub.get_args(dyn)
    assert plain.mix_rir_scp is None and plain.mix_rir_synth is None and train_qsub.reverb_options(plain) == {}
    conf = os.path.join(str(tmp_path), "conf")
    open(conf, "w").write("num_spk=2\nhidden_dim=64\n")
    args = train_qsub.get_args(dyn + ["--mix-rir-synth", "0.05,0.1", "--mix-rir-prob", "0.75", "--model-config", conf, "--seed", "3",
                                      "--prefetch", "0", "--num-workers", "0", "--batch-size", "3", "--mixes-per-epoch", "6"])
    assert args.mix_rir_synth == (0.05, 0.1) and train_qsub.reverb_options(args) == {"rir_synth": (0.05, 0.1), "rir_prob": 0.75}
    loader, draws = train_qsub.training_batches(uPIT, args, 0, 1)
    ds = loader.dataset
    assert ds.reverb and ds.rir_synth == (0.05, 0.1) and ds.rir_prob == 0.75 and ds.rir_rate == 8000
    draws.set_epoch(0)
    batches = list(loader)
    assert len(batches) == 2 and all("reverb" in b["pcm"] and len(b["pcm"]["reverb"]["taps"][1]) == 3 for b in batches)
    # without the options the set is built as before
    loader, _ = train_qsub.training_batches(uPIT, train_qsub.get_args(dyn + ["--model-config", conf, "--prefetch", "0", "--num-workers", "0",
                                                                            "--seed", "3"]), 0, 1)
    assert not loader.dataset.reverb


# ------------------------------------------------------------------------------------------------ 6: the ABI
def test_header_library_and_ctypes_table_have_both_symbols():
    from sepkern import _lib
    text = open(os.path.join(ROOT, "include", "sepkern.h")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("sk_fir_convolve", "sk_fir_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in _lib.PROTOTYPES
    assert len(_lib.PROTOTYPES["sk_fir_convolve"][1]) == 13 and _lib.PROTOTYPES["sk_fir_workspace_bytes"][0] is C.c_size_t


def _arrays(ns, taps, delay):
    J = len(ns)
    return ((C.c_int64 * J)(*([0] * J)), (C.c_int32 * J)(*ns), (C.c_int64 * J)(*([0] * J)), (C.c_int32 * J)(*taps), (C.c_int32 * J)(*delay),
            (C.c_int64 * J)(*([0] * J)))


def test_entry_point_refuses_bad_arguments_before_it_touches_a_device():
    from sepkern import _lib
    lib = _lib.load()

    def call(ns, taps, delay, J=None, null=()):
        io, n32, ro, t32, d32, oo = _arrays(ns, taps, delay)
        args = [None, 1, io, n32, None, ro, t32, d32, len(ns) if J is None else J, None, None, oo, None]
        for i in null:
            args[i] = None
        size = lib.sk_fir_workspace_bytes(None if 3 in null else n32, None if 6 in null else t32, None if 7 in null else d32, args[8])
        return lib.sk_fir_convolve(*args), lib.sk_last_error(), size

    for ns, taps, delay, word in (([300, 300], [700, 0], [0, 0], b"ntaps outside"), ([300], [8193], [0], b"ntaps outside"),
                                  ([300], [700], [700], b"delay outside"), ([300], [700], [-1], b"delay outside"),
                                  ([300], [1], [1], b"delay outside"), ([300, 0], [700, 700], [0, 0], b"nsamp outside"),
                                  ([-5], [700], [0], b"nsamp outside")):
        rc_, msg, size = call(ns, taps, delay)
        assert rc_ == -1 and word in msg and size == 0, (ns, taps, delay, msg)
    for J, word in ((0, b"J = 0"), (65536, b"J = 65536"), (-1, b"J = -1")):
        rc_, msg, size = call([300], [700], [0], J=J)
        assert rc_ == -1 and word in msg and size == 0
    for i in (2, 3, 5, 6, 7, 11):                                            # a job array (host) missing
        rc_, msg, _ = call([300], [700], [0], null=(i,))
        assert rc_ == -1 and b"job arrays" in msg
    assert lib.sk_fir_workspace_bytes(None, None, None, 1) == 0
    # good jobs, no device pointers: the last check
    rc_, msg, size = call([300, 9000], [700, 8192], [300, 8191])
    assert rc_ == -1 and b"null pointer" in msg
    # jobs (256-aligned) + (K + bx1 + 1) spectra of 264 float2: K = 3, bx1 = min(2, 2); K = 32, bx1 = min(67, 36)
    assert size == 256 + ((3 + 3) + (32 + 37)) * 264 * 8
    io, n32, ro, t32, d32, oo = _arrays([300], [700], [0])
    io[0] = -1
    assert lib.sk_fir_convolve(None, 0, io, n32, None, ro, t32, d32, 1, None, None, oo, None) == -1 and b"negative offset" in lib.sk_last_error()
