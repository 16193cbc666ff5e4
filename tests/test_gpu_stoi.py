"""sk_stoi on the MI355X (csrc/stoi.hip; sepkern/stoi_gpu.py; evaluate_sources.py --stoi) against the definition in
sepkern/stoi.py.

The gate is computed here, never fixed: g = 4 x the largest |stoi_host(dtype=float32) - stoi_host(dtype=float64)| over the
parity set -- the float32 error of the REFERENCE; the factor 4 because the kernel's 16 x 16 FFT and its band sums run in another
order than numpy's, so its error is of that size but not that value.  g must stay below 1e-5: every definitional slip tried
(a hanning(256) window, bands shifted by one bin, beta = -14, a 39 dB range, N = 31) moves a score by 6e-5 or more.
Where sk_resample runs in front (stoi_batch at 8 kHz, the CLI) its pinned tolerance (tests/test_gpu_resample.py:
|y - y64| <= (ntaps + 4) 2^-24 sum |h_k| |x_k| per sample) is added, propagated by a finite difference of the host function on
that very input.  profiles/stoi.txt records the measured g and the worst kernel error."""
import ctypes
import os
import sys

import numpy as np
import pytest
import scipy.io.wavfile
import torch

from sepkern import _lib, ops, synth
from sepkern import resample as R
from sepkern import stoi as ST
from sepkern.stoi_gpu import stoi_batch

from conftest import PKG

sys.path.insert(0, os.path.join(PKG, "steps"))

pytestmark = pytest.mark.gpu

LENS8 = (4000, 6000, 8000, 24000)


def _case(u, n8, S=2):
    """(refs, ests): fp32 (S, n) at 10 kHz.  Source 1 carries a gap (1500 samples from a third of its length scaled by 1e-4), so
    the kept frames are not adjacent; estimate 0 is the gapped source plus source 2, the others their own source plus half of
    the gapped one."""
    _, _, srcs = synth.utterance(u, n8, S)
    s = [R.resample_host(x.astype(np.float64) / 32768.0, 8000, 10000) for x in srcs]
    a = len(s[0]) // 3
    s[0][a:a + 1500] *= 1e-4
    refs = np.stack(s).astype(np.float32)
    ests = np.stack([refs[0] + refs[1]] + [refs[k] + np.float32(0.5) * refs[0] for k in range(1, S)])
    return refs, ests


def _host(refs, ests):
    m64, fr = ST.stoi_matrix(list(refs), list(ests))
    m32, fr32 = ST.stoi_matrix(list(refs), list(ests), dtype=np.float32)
    assert fr.tolist() == fr32.tolist()
    return m64, fr, float(np.abs(m64 - m32).max())


@pytest.fixture(scope="module")
def parity():
    """The parity set with its host scores, computed once: 12 two-speaker utterances and one three-speaker batch of mixed
    lengths.  g is the gate."""
    two = [_case(u, n8) for n8 in LENS8 for u in range(3)]
    three = [_case(u, n8, 3) for u, n8 in ((0, 4000), (1, 8000), (2, 6000))]
    for refs, _ in two + three:
        for r in refs:                                      # a condition on the INPUTS: no frame sits at the keep threshold
            assert np.abs(ST.keep_margins(r)).min() > 1e-3
    host2, host3 = [_host(*c) for c in two], [_host(*c) for c in three]
    g = 4.0 * max(h[2] for h in host2 + host3)
    frames = [int(f) for h in host2 for f in h[1]]
    assert min(frames) < 30 < max(frames)                   # the 1e-5 path and the scored path are both in the set
    return {"two": two, "three": three, "host2": host2, "host3": host3, "g": g}


def _gpu(cases):
    S = cases[0][0].shape[0]
    lens = [c[0].shape[1] for c in cases]
    offs = [int(v) for v in np.cumsum([0] + [S * n for n in lens[:-1]])]
    rcat = torch.from_numpy(np.concatenate([c[0].reshape(-1) for c in cases])).cuda()
    ecat = torch.from_numpy(np.concatenate([c[1].reshape(-1) for c in cases])).cuda()
    out, frames = ops.stoi(rcat, ecat, offs, lens, S)
    return out.cpu().numpy(), frames.cpu().numpy()


def test_gate_is_far_below_a_definitional_slip(parity):
    print("stoi gate g = %.3g" % parity["g"])
    assert 0.0 < parity["g"] < 1e-5


@pytest.mark.parametrize("name", ["two", "three"])
def test_parity_with_the_host_definition(parity, name):
    cases, host = parity[name], parity["host" + ("2" if name == "two" else "3")]
    out, frames = _gpu(cases)
    worst = 0.0
    for u, (m64, fr, _) in enumerate(host):
        assert frames[u].tolist() == fr.tolist(), (u, frames[u], fr)
        worst = max(worst, float(np.abs(out[u] - m64).max()))
    print("sk_stoi S=%d: worst |kernel - float64 host| = %.3g, gate g = %.3g" % (cases[0][0].shape[0], worst, parity["g"]))
    for u, (m64, fr, _) in enumerate(host):
        short = fr < 30
        assert np.all(out[u][:, short] == 1e-5)
        assert np.abs(out[u] - m64).max() <= parity["g"], (u, out[u], m64)


def test_identity_scores_one(parity):
    cases = [(c[0], c[0]) for c in parity["two"][3:]]
    out, frames = _gpu(cases)
    for u in range(len(cases)):
        assert frames[u].min() >= 30
        assert np.abs(np.diagonal(out[u], axis1=0, axis2=1) - 1.0).max() <= parity["g"]


def test_bits_depend_neither_on_the_batch_nor_on_the_run(parity):
    cases = parity["two"]
    alone, fa = _gpu([cases[7]])
    batch, fb = _gpu(cases[:3] + [cases[11]] + [cases[7]] + cases[4:7])
    again, _ = _gpu(cases[:3] + [cases[11]] + [cases[7]] + cases[4:7])
    assert np.array_equal(alone[0], batch[4]) and fa[0].tolist() == fb[4].tolist()
    assert np.array_equal(batch, again)


def test_degenerate_inputs_score_the_customary_value():
    rng = np.random.default_rng(0)
    long = (0.1 * rng.standard_normal((2, 9000))).astype(np.float32)
    cases = [((0.1 * rng.standard_normal((2, n))).astype(np.float32),) * 2 for n in (1, 256, 257)]
    zero = long.copy()
    zero[0] = 0.0
    cases.append((zero, long))
    out, frames = _gpu(cases)
    assert frames[:3].tolist() == [[0, 0]] * 3 and np.all(out[:3] == 1e-5)
    assert frames[3].tolist()[0] == 0 and frames[3][1] >= 30
    assert np.all(out[3][:, 0] == 1e-5) and abs(out[3][1, 1, 0] - 1.0) < 1e-5
    for u in range(4):
        want, fr = ST.stoi_matrix(list(cases[u][0]), list(cases[u][1]))
        assert fr.tolist() == frames[u].tolist() and np.abs(out[u] - want).max() < 1e-5


def test_five_sources_are_refused_before_a_launch():
    x = torch.zeros(5 * 4000, device="cuda")
    with pytest.raises(_lib.SepkernError, match=r"code -1.*S = 5"):
        ops.stoi(x, x, [0], [4000], 5)
    lib = _lib.load()
    offs, lens = (ctypes.c_int64 * 1)(0), (ctypes.c_int32 * 1)(4000)
    assert lib.sk_stoi(None, None, offs, lens, 1, 5, None, None, None, None) == -1
    assert lib.sk_stoi_workspace_bytes(1, 5, 4000) == 0


def _resampler_bound(x, pl):
    """The pinned per-sample tolerance of sk_resample for the fp64 signal x: (ntaps + 4) 2^-24 sum_k |h_k| |x_k|."""
    n = np.arange(pl.out_len(len(x)), dtype=np.int64)
    k0, ph = pl.first(n), pl.phase(n)
    left, right = max(0, -int(k0.min())), max(0, int(k0.max()) + pl.ntaps - len(x))
    xp = np.concatenate([np.zeros(left), np.abs(x), np.zeros(right)])
    cols = np.arange(pl.ntaps, dtype=np.int64)[None, :]
    return (pl.ntaps + 4) * 2.0 ** -24 * np.einsum("ij,ij->i", xp[k0[:, None] + left + cols], np.abs(pl.taps[ph]))


def _gate_through_the_resampler(refs8, ests8, seed=0):
    """(host matrix, frames, gate) for (S, n) fp64 signals at 8 kHz: gate = 4 x the float32 error of the host function on this
    input + the change of the host function when every 10 kHz sample moves by the resampler's full tolerance (random signs)."""
    pl = R.plan(8000, 10000)
    rng = np.random.default_rng(seed)
    r10 = [R.resample_host(x, 8000, 10000) for x in refs8]
    e10 = [R.resample_host(x, 8000, 10000) for x in ests8]
    for r in r10:
        assert np.abs(ST.keep_margins(r)).min() > 1e-3
    moved = lambda ys, xs: [y + _resampler_bound(x, pl) * rng.choice([-1.0, 1.0], len(y)) for y, x in zip(ys, xs)]  # noqa: E731
    m64, fr = ST.stoi_matrix(r10, e10)
    m32, _ = ST.stoi_matrix(r10, e10, dtype=np.float32)
    mfd, frd = ST.stoi_matrix(moved(r10, refs8), moved(e10, ests8))
    assert fr.tolist() == frd.tolist()
    return m64, fr, 4.0 * float(np.abs(m64 - m32).max()) + float(np.abs(mfd - m64).max())


def test_stoi_batch_from_int16_at_8k():
    pcm = []
    for u, n8 in enumerate((6000, 8000, 12000)):
        _, mix, srcs = synth.utterance(u, n8, 2)
        srcs = [s.copy() for s in srcs]
        a = n8 // 3
        srcs[0][a:a + 1200] //= 4096
        est = [np.clip(srcs[1].astype(np.int32) + srcs[0] // 3, -32768, 32767).astype(np.int16), mix]      # swapped on purpose
        pcm.append((np.stack(srcs), np.stack(est)))
    got = stoi_batch([torch.from_numpy(p[0]).cuda() for p in pcm], [p[1] for p in pcm], 8000)
    diag = stoi_batch([p[0] for p in pcm], [p[1] for p in pcm], 8000, compute_permutation=False)
    for u, (refs, ests) in enumerate(pcm):
        m64, fr, gate = _gate_through_the_resampler(refs.astype(np.float64) / 32768.0, ests.astype(np.float64) / 32768.0, seed=u)
        want = ST.select(m64, fr)
        print("stoi_batch utterance %d: gate %.3g, worst error %.3g" % (u, gate, max(np.abs(got[u][0] - want[0]).max(),
                                                                                     np.abs(got[u][1] - want[1]).max())))
        assert gate < 1e-4
        assert got[u][2].tolist() == want[2].tolist() == [1, 0] and got[u][3].tolist() == fr.tolist()
        assert np.abs(got[u][0] - want[0]).max() <= gate and np.abs(got[u][1] - want[1]).max() <= gate
        assert diag[u][2].tolist() == [0, 1]
        assert np.abs(diag[u][0] - np.diagonal(m64[..., 0])).max() <= gate
        # the host function at fs = 8000 is this same number
        assert ST.stoi_host(refs[0] / 32768.0, ests[1] / 32768.0, fs=8000) == m64[1, 0, 0]


def _read(d):
    return {name: open(os.path.join(d, name)).read().splitlines() for name in sorted(os.listdir(d))}


def test_evaluate_sources_cli_with_stoi(tmp_path):
    import evaluate_sources
    wav_root = tmp_path / "wav"
    ids = synth.write_wav_tree(str(wav_root), 4, num_spk=2, min_s=1.0, max_s=2.0, seed=3)
    data = tmp_path / "data"
    synth.write_data_dir(str(data), str(wav_root), ids)
    with open(data / "utt2num_spk", "w") as f:
        f.write("".join("%s 2\n" % i for i in ids))
    rng = np.random.default_rng(5)
    exp = {m: tmp_path / m for m in ("cpu", "gpu", "plain")}
    gates = {}
    for i in ids:
        srcs = [scipy.io.wavfile.read(str(wav_root / ("s%d" % (s + 1)) / (i + ".wav")))[1].astype(np.float64) for s in range(2)]
        ests = []
        for s in range(2):
            est = srcs[s] + 0.2 * srcs[1 - s] + 300.0 * rng.standard_normal(len(srcs[s]))
            ests.append(np.clip(np.round(est), -32768, 32767).astype(np.int16))
            for d in exp.values():
                os.makedirs(d / "wav" / ("s%d" % (s + 1)), exist_ok=True)
                scipy.io.wavfile.write(str(d / "wav" / ("s%d" % (s + 1)) / (i + ".wav")), 8000, ests[s])
        gates[i] = _gate_through_the_resampler([x / 32768.0 for x in srcs], [e.astype(np.float64) / 32768.0 for e in ests])[2]
    evaluate_sources.main([str(data), str(exp["cpu"]), "--stoi"])
    evaluate_sources.main([str(data), str(exp["gpu"]), "--gpu", "--stoi", "--batch", "3"])
    evaluate_sources.main([str(data), str(exp["plain"]), "--gpu"])
    a, b, c = (_read(exp[m] / "results") for m in ("cpu", "gpu", "plain"))
    new = sorted("%s_%ss.txt" % (k, m) for k in ("session", "source") for m in ("STOI", "ESTOI")) + ["ESTOI_stats.txt", "STOI_stats.txt"]
    assert sorted(set(b) - set(c)) == sorted(new) and sorted(a) == sorted(b)
    assert not [n for n in c if "STOI" in n]
    for name in new:
        if name.endswith("_stats.txt"):
            gate = max(gates.values())
            for la, lb in zip(a[name], b[name]):
                assert la.split()[0] == lb.split()[0] and abs(float(la.split()[1]) - float(lb.split()[1])) <= gate
            continue
        assert [l.split()[0] for l in a[name]] == [l.split()[0] for l in b[name]] == ids
        for la, lb in zip(a[name], b[name]):
            va, vb = [float(v) for v in la.split()[1:]], [float(v) for v in lb.split()[1:]]
            assert len(va) == len(vb) == (2 if name.startswith("source") else 1)
            assert 0.3 < min(va) and max(va) < 1.0
            assert np.abs(np.array(va) - np.array(vb)).max() <= gates[la.split()[0]], (name, la, lb)
