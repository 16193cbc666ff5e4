"""STOI / ESTOI as sepkern/stoi.py defines them (UNPINNED against any package: none is installed).  What holds the
definition: the band table, identity, gain invariance, the short-utterance value, the silent-frame count against a direct
computation, the score of independent sources and the ordering mixture > other source."""
import math

import numpy as np
import pytest

from sepkern import resample as R
from sepkern import stoi as ST
from sepkern import synth

TABLE = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109),
         (109, 138), (138, 174), (174, 219))


def _sources(u, n8=16000):
    """The float sources of synth.utterance(u, n8, 2) at 10 kHz."""
    _, _, srcs = synth.utterance(u, n8, 2)
    return [R.resample_host(s.astype(np.float64) / 32768.0, 8000, 10000) for s in srcs]


@pytest.fixture(scope="module")
def utts():
    return [_sources(u) for u in range(3)]


def test_constants_and_band_table():
    assert ST.BAND_EDGES == TABLE
    assert (ST.FS, ST.N_FRAME, ST.HOP, ST.NFFT, ST.NUM_BANDS, ST.N_SEG, ST.BETA, ST.DYN_RANGE) == (10000, 256, 128, 512, 15, 30, -15.0,
                                                                                                   40.0)
    assert ST.EPS == np.finfo(np.float64).eps
    i = np.arange(256)
    np.testing.assert_allclose(ST.WINDOW, 0.5 * (1 - np.cos(2 * np.pi * (i + 1) / 257)), rtol=0, atol=1e-15)


def test_framing_is_end_exclusive():
    assert [len(ST.frame_starts(n)) for n in (1, 256, 257, 384, 385, 512, 513)] == [0, 0, 1, 1, 2, 2, 3]


@pytest.mark.parametrize("extended", [False, True])
def test_identity_scores_one(utts, extended):
    for s1, _ in utts:
        assert abs(ST.stoi_host(s1, s1, extended=extended) - 1.0) < 1e-12


@pytest.mark.parametrize("extended", [False, True])
def test_invariant_to_a_positive_gain_on_the_estimate(utts, extended):
    s1, s2 = utts[0]
    est = s1 + 0.7 * s2
    base = ST.stoi_host(s1, est, extended=extended)
    for gain in (0.01, 3.0, 250.0):
        assert abs(ST.stoi_host(s1, gain * est, extended=extended) - base) < 1e-9


def test_too_few_frames_returns_the_customary_value():
    s1, s2 = _sources(0, 3000)                                           # 3750 samples: 28 frames
    d, e, T = ST.stoi_pair(s1, s1 + s2)
    assert T < 30 and d == 1e-5 and e == 1e-5
    assert ST.stoi_host(s1, s1 + s2) == 1e-5 and ST.stoi_host(s1, s1 + s2, extended=True) == 1e-5
    for n in (1, 256, 257):
        assert ST.stoi_pair(np.ones(n), np.ones(n)) == (1e-5, 1e-5, 0)
    assert ST.stoi_pair(np.zeros(9000), np.ones(9000)) == (1e-5, 1e-5, 0)     # an all-zero reference keeps no frame


def test_kept_frames_on_a_carved_gap_against_a_direct_computation(utts):
    x = utts[1][0].copy()
    a = len(x) // 3
    x[a:a + 1500] *= 1e-4
    # direct: every frame's energy from the window's formula, in a plain loop
    w = [0.5 * (1.0 - math.cos(2.0 * math.pi * (i + 1) / 257.0)) for i in range(256)]
    db = []
    for s in range(0, len(x) - 256, 128):
        db.append(10.0 * math.log10(sum((w[i] * x[s + i]) ** 2 for i in range(256))))
    kept = [i for i, v in enumerate(db) if v > max(db) - 40.0]
    got = ST.kept_frames(x)
    assert 0 < len(kept) < len(db) and list(got) == kept
    assert np.abs(ST.keep_margins(x)).min() > 1e-3                        # well-posed: no frame at the threshold
    assert ST.stoi_pair(x, x)[2] == len(kept) - 1
    # the kept frames are no longer adjacent
    assert np.any(np.diff(got) > 1)


def test_estoi_of_independent_sources_is_small(utts):
    for s1, s2 in utts:
        assert abs(ST.stoi_host(s1, s2, extended=True)) < 0.15
        assert abs(ST.stoi_host(s2, s1, extended=True)) < 0.15


def test_mixture_scores_above_the_other_source(utts):
    for s1, s2 in utts:
        mix = s1 + s2
        assert ST.stoi_host(s1, mix) > ST.stoi_host(s1, s2)
        assert ST.stoi_host(s2, mix) > ST.stoi_host(s2, s1)


def test_float32_evaluation_stays_close_to_float64(utts):
    """The gate of the GPU test is a multiple of this difference: it has to be far below what a definitional slip moves
    (6e-5 and more)."""
    for s1, s2 in utts:
        r, e = s1.astype(np.float32), (s1 + s2).astype(np.float32)
        for ext in (False, True):
            assert abs(ST.stoi_host(r, e, extended=ext, dtype=np.float32) - ST.stoi_host(r, e, extended=ext)) < 2.5e-6


def test_select_takes_the_first_maximum_in_permutation_order():
    mat = np.zeros((2, 2, 2))
    mat[..., 0] = [[0.5, 0.9], [0.9, 0.5]]
    mat[..., 1] = [[0.1, 0.2], [0.3, 0.4]]
    d, e, perm, fr = ST.select(mat, [40, 41])
    assert list(perm) == [1, 0] and list(d) == [0.9, 0.9] and list(e) == [0.3, 0.2] and list(fr) == [40, 41]
    mat[..., 0] = 0.7                                                     # a tie: the identity comes first
    assert list(ST.select(mat, [40, 41])[2]) == [0, 1]
    assert list(ST.select(mat, [40, 41], compute_permutation=False)[2]) == [0, 1]


def test_batch_function_names_the_host_function_without_a_gpu(monkeypatch):
    import torch
    from sepkern import _lib, stoi_gpu
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.SepkernError, match="stoi_host"):
        stoi_gpu.stoi_batch([np.zeros((2, 4000), np.float32)], [np.zeros((2, 4000), np.float32)], 8000)


def test_argument_errors_come_back_before_any_launch():
    from sepkern import _lib
    lib = _lib.load()
    assert lib.sk_stoi_workspace_bytes(4, 2, 40000) > 0
    assert lib.sk_stoi_workspace_bytes(4, 5, 40000) == 0 and lib.sk_stoi_workspace_bytes(0, 2, 40000) == 0
    assert lib.sk_stoi_workspace_bytes(4, 2, 0) == 0
    import ctypes
    offs, lens = (ctypes.c_int64 * 1)(0), (ctypes.c_int32 * 1)(4000)
    rc = lib.sk_stoi(None, None, offs, lens, 1, 5, None, None, None, None)
    assert rc == -1 and b"S = 5" in lib.sk_last_error()


def test_evaluate_sources_cli_on_the_host(tmp_path):
    """--stoi (without --gpu) writes the six STOI / ESTOI files from the host function; without the flag none of them."""
    import os
    import sys
    import scipy.io.wavfile
    from conftest import PKG
    sys.path.insert(0, os.path.join(PKG, "steps"))
    import evaluate_sources
    wav_root = tmp_path / "wav"
    ids = synth.write_wav_tree(str(wav_root), 2, num_spk=2, min_s=0.6, max_s=0.9, seed=3)
    data = tmp_path / "data"
    synth.write_data_dir(str(data), str(wav_root), ids)
    with open(data / "utt2num_spk", "w") as f:
        f.write("".join("%s 2\n" % i for i in ids))
    exp = {m: tmp_path / m for m in ("stoi", "plain")}
    want = {}
    for i in ids:
        srcs = [scipy.io.wavfile.read(str(wav_root / ("s%d" % (s + 1)) / (i + ".wav")))[1] for s in range(2)]
        ests = [np.clip(srcs[1 - s].astype(np.int32) + srcs[s] // 4, -32768, 32767).astype(np.int16) for s in range(2)]   # swapped
        for s in range(2):
            for d in exp.values():
                os.makedirs(d / "wav" / ("s%d" % (s + 1)), exist_ok=True)
                scipy.io.wavfile.write(str(d / "wav" / ("s%d" % (s + 1)) / (i + ".wav")), 8000, ests[s])
        want[i] = ST.stoi_sources(np.stack(srcs) / 32768.0, np.stack(ests) / 32768.0, 8000)
        assert list(want[i][2]) == [1, 0] and min(want[i][3]) >= 30
    evaluate_sources.main([str(data), str(exp["stoi"]), "--stoi"])
    evaluate_sources.main([str(data), str(exp["plain"])])
    a, b = sorted(os.listdir(exp["stoi"] / "results")), sorted(os.listdir(exp["plain"] / "results"))
    new = sorted(["session_STOIs.txt", "session_ESTOIs.txt", "source_STOIs.txt", "source_ESTOIs.txt", "STOI_stats.txt", "ESTOI_stats.txt"])
    assert sorted(set(a) - set(b)) == new and not [n for n in b if "STOI" in n]
    for k, name in enumerate(("source_STOIs.txt", "source_ESTOIs.txt")):
        lines = open(exp["stoi"] / "results" / name).read().splitlines()
        assert [l.split()[0] for l in lines] == ids
        for l in lines:
            assert [float(v) for v in l.split()[1:]] == [float(v) for v in want[l.split()[0]][k]]
