"""Batched BSS Eval on the GPU (sepkern/bsseval_gpu.py, csrc/bsseval.hip) against the host function
sepkern/bsseval.py: exact correlations, parity at 512 taps, the closed forms of test_bsseval.py, the host fallback,
determinism and the --gpu scoring CLI."""
import os
import sys

import numpy as np
import pytest
import scipy.io.wavfile
import scipy.signal
import torch

from sepkern import bsseval, ops, synth
from sepkern.bsseval_gpu import bss_eval_sources_batch

from conftest import PKG

sys.path.insert(0, os.path.join(PKG, "steps"))

pytestmark = pytest.mark.gpu

GATE_DB = 1e-3


def _pcm(x):
    return np.clip(np.round(np.asarray(x) * 32768.0), -32768, 32767).astype(np.int16)


def _corr_int(x, y, d):
    """sum_m x[m] y[m + d] in int64."""
    n = len(x)
    if d >= n or -d >= n:
        return 0
    if d >= 0:
        return int(np.dot(x[:n - d], y[d:]))
    return int(np.dot(x[-d:], y[:n + d]))


@pytest.mark.parametrize("S,taps,lens", [(2, 512, [300, 4099, 513]), (3, 37, [1000, 16, 257]), (1, 1, [5, 2048])])
def test_xcorr_is_exact_for_pcm(S, taps, lens):
    rng = np.random.default_rng(S * 1000 + taps)
    refs = [rng.integers(-32768, 32768, size=(S, n)).astype(np.int64) for n in lens]
    ests = [rng.integers(-32768, 32768, size=(S, n)).astype(np.int64) for n in lens]
    scale = 2.0 ** -15
    rcat = torch.tensor(np.concatenate([r.reshape(-1) for r in refs]) * scale, dtype=torch.float64, device="cuda")
    ecat = torch.tensor(np.concatenate([e.reshape(-1) for e in ests]) * scale, dtype=torch.float64, device="cuda")
    offs = np.concatenate(([0], np.cumsum([S * n for n in lens])[:-1])).tolist()
    xc = ops.bss_xcorr(rcat, ecat, offs, lens, S, taps).cpu().numpy()
    assert xc.shape == (len(lens), ops.bss_xc_len(S, taps))
    for u, (r, e) in enumerate(zip(refs, ests)):
        want = []
        for i in range(S):
            for j in range(i, S):
                want += [_corr_int(r[i], r[j], d) for d in range(-(taps - 1), taps)]
        for i in range(S):
            for k in range(S):
                want += [_corr_int(r[i], e[k], t) for t in range(taps)]
        want += [_corr_int(e[k], e[k], 0) for k in range(S)]
        want = np.array(want, dtype=np.float64) * 2.0 ** -30         # exact: every value < 2^53 units of 2^-30
        assert np.array_equal(xc[u], want), (u, np.flatnonzero(xc[u] != want)[:10])


def _estimates(refs, rng, leak=0.15, noise=0.05):
    """leakage of the other sources + a short filtered copy of the own source + white noise."""
    S, n = refs.shape
    est = np.empty_like(refs)
    for k in range(S):
        h = rng.standard_normal(24) * 0.2
        h[0] = 1.0
        own = scipy.signal.lfilter(h, [1.0], refs[k])
        other = sum(refs[j] for j in range(S) if j != k) * leak
        est[k] = own + other + noise * np.std(refs[k]) * rng.standard_normal(n)
    return est


def _parity_batch():
    rng = np.random.default_rng(7)
    refs, ests = [], []
    for u, (S, n) in enumerate([(2, 8000), (2, 12345), (3, 9001), (4, 7000)]):
        r = np.stack([synth.speech_like(n, 100 * u + s) for s in range(S)])
        refs.append(r)
        ests.append(_estimates(r, rng))
    # ill-conditioned: white noise through a cascaded one-pole low-pass (a = 0.99, twice)
    r = rng.standard_normal((2, 10000))
    for _ in range(2):
        r = scipy.signal.lfilter([1.0], [1.0, -0.99], r, axis=1)
    refs.append(r / np.abs(r).max())
    ests.append(_estimates(refs[-1], rng))
    return refs, ests


def test_parity_with_the_host_function_at_512_taps():
    refs, ests = _parity_batch()
    got = bss_eval_sources_batch(refs, ests)
    assert got.fallback == []
    worst = 0.0
    for u, (r, e) in enumerate(zip(refs, ests)):
        want = bsseval.bss_eval_sources(r, e)
        assert got[u][3].tolist() == want[3].tolist(), u
        for m in range(3):
            assert got[u][m].shape == want[m].shape and got[u][m].dtype == np.float64
            d = float(np.max(np.abs(got[u][m] - want[m])))
            worst = max(worst, d)
            assert d < GATE_DB, (u, m, got[u][m], want[m])
    print("max |GPU - host| over SDR/SIR/SAR: %.3g dB" % worst)
    # without the permutation search: the diagonal, as the host function returns it
    fixed = bss_eval_sources_batch(refs[:2], [e[::-1].copy() for e in ests[:2]], compute_permutation=False)
    for u in range(2):
        want = bsseval.bss_eval_sources(refs[u], ests[u][::-1], compute_permutation=False)
        assert fixed[u][3].tolist() == [0, 1]
        np.testing.assert_allclose(np.stack(fixed[u][:3]), np.stack(want[:3]), atol=GATE_DB, rtol=0)


@pytest.mark.parametrize("S,taps,lens", [(1, 5, [40, 300]), (2, 17, [300, 1000]), (3, 37, [1000, 2048]), (4, 21, [700, 701]),
                                         (2, 100, [900]), (1, 37, [30])])
def test_parity_at_orders_whose_last_panel_is_part_gram_part_identity(S, taps, lens):
    """bss_chol_kernel factors matrices padded with an identity to multiples of 16: S x taps = 5 -> 16, 34 -> 48, 111 -> 112,
    84 -> 96, 200 -> 208, 37 -> 48 here, and one source's 17 -> 32, 37 -> 48, 21 -> 32, 100 -> 112; n = 30 < taps = 37.
    Conditions on the inputs, asserted on the host result: more samples than unknowns (n + taps - 1 > S taps; with fewer the
    projection is exact and SAR is rounding noise, about 290 dB -- S = 4, taps = 37, n = 30 does that) and every SAR below
    60 dB.  (1, 37, [30]) has 66 samples for 37 unknowns: a margin of two between them, which every other case has, it cannot."""
    order, one = S * taps, taps
    assert order % 16 != 0
    print("S = %d, taps = %d: orders %d -> %d and %d -> %d" % (S, taps, order, -(-order // 16) * 16, one, -(-one // 16) * 16))
    rng = np.random.default_rng(100 * S + taps)
    refs = [rng.standard_normal((S, n)) for n in lens]
    ests = [_estimates(r, rng) for r in refs]
    want = [bsseval.bss_eval_sources(r, e, taps=taps) for r, e in zip(refs, ests)]
    for n, w in zip(lens, want):
        assert n + taps - 1 > S * taps and np.all(w[2] < 60.0), (n, w[2])
    got = bss_eval_sources_batch(refs, ests, taps=taps)
    assert got.fallback == []
    worst = 0.0
    for u in range(len(lens)):
        assert got[u][3].tolist() == want[u][3].tolist(), u
        for m in range(3):
            g, w = got[u][m], want[u][m]
            assert g.shape == w.shape == (S,)
            fin = np.isfinite(w)                                 # S = 1: no interference, SIR is +inf on both sides
            assert np.array_equal(g[~fin], w[~fin]) and fin.all() == (S > 1 or m != 1) and np.isfinite(g[fin]).all(), (u, m, g, w)
            if fin.any():
                worst = max(worst, float(np.max(np.abs(g[fin] - w[fin]))))
    print("S = %d, taps = %d, lengths %s: max |GPU - host| over SDR/SIR/SAR %.3g dB (gate %.3g)" % (S, taps, lens, worst, GATE_DB))
    assert worst < GATE_DB
    # a short and a long utterance in one batch: each has the bits it has alone
    for u in range(len(lens)):
        solo = bss_eval_sources_batch(refs[u:u + 1], ests[u:u + 1], taps=taps)
        assert solo.fallback == []
        for m in range(4):
            assert np.array_equal(solo[0][m], got[u][m]), (u, m)


def _dense_projection(refs, e, taps):
    n = refs.shape[1]
    cols = []
    for r in refs:
        for t in range(taps):
            c = np.zeros(n + taps - 1)
            c[t:t + n] = r
            cols.append(c)
    A = np.stack(cols, axis=1)
    y = np.concatenate((e, np.zeros(taps - 1)))
    return A @ np.linalg.lstsq(A, y, rcond=None)[0]


def test_closed_forms_on_the_gpu():
    # dense least squares, taps 8
    rng = np.random.default_rng(0)
    refs = rng.standard_normal((2, 300))
    e = 0.7 * refs[0] + 0.2 * np.roll(refs[1], 2) + 0.1 * rng.standard_normal(300)
    est = np.stack([e, refs[1] + 0.05 * rng.standard_normal(300)])
    taps = 8
    (sdr, sir, sar, perm), = bss_eval_sources_batch([refs], [est], taps=taps)
    assert perm.tolist() == [0, 1]
    p_all = _dense_projection(refs, e, taps)
    p_one = _dense_projection(refs[:1], e, taps)
    pad = np.concatenate((e, np.zeros(taps - 1)))
    want = [10 * np.log10(np.sum(p_one ** 2) / np.sum((pad - p_one) ** 2)),
            10 * np.log10(np.sum(p_one ** 2) / np.sum((p_all - p_one) ** 2)),
            10 * np.log10(np.sum(p_all ** 2) / np.sum((pad - p_all) ** 2))]
    np.testing.assert_allclose([sdr[0], sir[0], sar[0]], want, rtol=1e-7)

    # scaled and filtered copies, 512 taps
    rng = np.random.default_rng(1)
    refs = rng.standard_normal((2, 4000))
    refs[1, -40:] = 0
    h = rng.standard_normal(40)
    est = np.stack([0.3 * refs[0], np.convolve(refs[1], h)[:4000]])
    (sdr, sir, sar, perm), = bss_eval_sources_batch([refs], [est])
    assert perm.tolist() == [0, 1]
    assert np.all(sdr > 100) and np.all(sir > 100) and np.all(sar > 100)

    # orthogonal interference, taps 1
    rng = np.random.default_rng(2)
    a, b = rng.standard_normal(2000), rng.standard_normal(2000)
    b -= a * np.dot(a, b) / np.dot(a, a)
    (sdr, sir, sar, perm), = bss_eval_sources_batch([np.stack([a, b])], [np.stack([a + 0.1 * b, b + 0.5 * a])], taps=1)
    want0 = 10 * np.log10(np.dot(a, a) / (0.01 * np.dot(b, b)))
    want1 = 10 * np.log10(np.dot(b, b) / (0.25 * np.dot(a, a)))
    np.testing.assert_allclose(sir, [want0, want1], rtol=1e-9)
    np.testing.assert_allclose(sdr, sir, rtol=1e-6)
    assert np.all(sar > 150)

    # artifacts and the permutation search, taps 16
    rng = np.random.default_rng(3)
    refs = rng.standard_normal((3, 3000))
    clean = refs + 0.1 * rng.standard_normal((3, 3000))
    est = clean[[2, 0, 1]]
    (sdr, sir, sar, perm), (s2, i2, a2, p2) = bss_eval_sources_batch([refs, refs], [est, clean], taps=16)
    assert perm.tolist() == [1, 2, 0] and p2.tolist() == [0, 1, 2]
    np.testing.assert_allclose(sdr, s2, rtol=1e-9)
    np.testing.assert_allclose(sar, a2, rtol=1e-9)
    assert np.all(np.abs(sar - 20.0) < 1.0)
    (same, _, _, fixed), = bss_eval_sources_batch([refs], [est], compute_permutation=False, taps=16)
    assert fixed.tolist() == [0, 1, 2] and np.all(same < 0)
    want = bsseval.bss_eval_sources(refs, est, taps=16)
    for m in range(3):
        np.testing.assert_allclose((sdr, sir, sar)[m], want[m], atol=GATE_DB, rtol=0)


def test_rank_deficient_references_fall_back_to_the_host_function():
    """A pure tone and the same tone 5 samples later (zero tail, so the delayed copies coincide exactly): the Gram
    matrix of all sources is singular, the device factorisation reports it, and the utterance is re-scored on the
    host.  (A lone finite tone is NOT singular: its delayed copies differ at the edges.)"""
    rng = np.random.default_rng(11)
    n = 6000
    tone = np.sin(2 * np.pi * 440.0 / 8000.0 * np.arange(n))
    tone[-5:] = 0
    r_def = np.stack([tone, np.concatenate((np.zeros(5), tone[:-5]))])
    e_def = r_def + 0.1 * rng.standard_normal(r_def.shape)
    ok = [np.stack([synth.speech_like(7000, 50 + s) for s in range(2)]) for _ in range(2)]
    ok[1] = np.stack([synth.speech_like(5000, 60 + s) for s in range(2)])
    ok_est = [_estimates(r, rng) for r in ok]
    got = bss_eval_sources_batch([ok[0], r_def, ok[1]], [ok_est[0], e_def, ok_est[1]])
    assert got.fallback == [1] and got.n_fallback == 1
    want = bsseval.bss_eval_sources(r_def, e_def)
    for m in range(4):
        assert np.array_equal(got[1][m], want[m])
    for u, i in ((0, 0), (2, 1)):
        want = bsseval.bss_eval_sources(ok[i], ok_est[i])
        assert got[u][3].tolist() == want[3].tolist()
        np.testing.assert_allclose(np.stack(got[u][:3]), np.stack(want[:3]), atol=GATE_DB, rtol=0)


def test_results_do_not_depend_on_the_batch():
    refs, ests = _parity_batch()
    alone = bss_eval_sources_batch(refs[1:2], ests[1:2])[0]
    batch = bss_eval_sources_batch(refs, ests)
    again = bss_eval_sources_batch(refs[::-1], ests[::-1])
    for a, b, c in zip(alone, batch[1], again[len(refs) - 2]):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    # device-resident int16 and float32 inputs take the same path
    pcm = [torch.from_numpy(_pcm(r)).cuda() for r in refs[:2]]
    est32 = [torch.from_numpy(e.astype(np.float32)).cuda() for e in ests[:2]]
    got = bss_eval_sources_batch(pcm, est32)
    for u in range(2):
        want = bsseval.bss_eval_sources(_pcm(refs[u]).astype(np.float64) / 32768.0, ests[u].astype(np.float32))
        assert got[u][3].tolist() == want[3].tolist()
        np.testing.assert_allclose(np.stack(got[u][:3]), np.stack(want[:3]), atol=GATE_DB, rtol=0)


def _read_results(d):
    out = {}
    for name in sorted(os.listdir(d)):
        with open(os.path.join(d, name)) as f:
            out[name] = f.read().splitlines()
    return out


def test_evaluate_sources_cli_gpu_matches_the_default(tmp_path):
    import evaluate_sources
    wav_root = tmp_path / "wav"
    ids = synth.write_wav_tree(str(wav_root), 12, num_spk=2, min_s=1.0, max_s=3.0, seed=3)
    data = tmp_path / "data"
    synth.write_data_dir(str(data), str(wav_root), ids)
    with open(data / "utt2num_spk", "w") as f:
        f.write("".join("%s 2\n" % i for i in ids))
    rng = np.random.default_rng(5)
    exp = {m: tmp_path / m for m in ("cpu", "gpu")}
    for i in ids:
        srcs = [scipy.io.wavfile.read(str(wav_root / ("s%d" % (s + 1)) / (i + ".wav")))[1].astype(np.float64) for s in range(2)]
        for s in range(2):
            est = srcs[s] + 0.2 * srcs[1 - s] + 300.0 * rng.standard_normal(len(srcs[s]))
            for d in exp.values():
                os.makedirs(d / "wav" / ("s%d" % (s + 1)), exist_ok=True)
                scipy.io.wavfile.write(str(d / "wav" / ("s%d" % (s + 1)) / (i + ".wav")), 8000,
                                       np.clip(np.round(est), -32768, 32767).astype(np.int16))
    evaluate_sources.main([str(data), str(exp["cpu"])])
    evaluate_sources.main([str(data), str(exp["gpu"]), "--gpu", "--batch", "5"])
    a, b = _read_results(exp["cpu"] / "results"), _read_results(exp["gpu"] / "results")
    assert sorted(a) == sorted(b)
    for name in a:
        assert len(a[name]) == len(b[name]), name
        for la, lb in zip(a[name], b[name]):
            ka, *va = la.split()
            kb, *vb = lb.split()
            assert ka == kb and len(va) == len(vb), (name, la, lb)
            if "SISDR" in name:
                assert la == lb
            else:
                np.testing.assert_allclose([float(v) for v in vb], [float(v) for v in va], atol=GATE_DB, rtol=0)
    assert [l.split()[0] for l in b["source_SDRs.txt"]] == ids
