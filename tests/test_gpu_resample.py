"""sk_resample on the MI355X against sepkern/resample.py's fp64 reference, and the places a wav is opened: extract_feats on a
16 kHz tree, a loss=sisdr step from a 16 kHz WavTrainSet(sample_rate=8000) batch, and the same-rate path left as it was.

The kernel's gate is DERIVED, not measured: for every output sample
    |y_gpu - y_64| <= (ntaps + 4) 2^-24 sum_k |h_k| |x_k|,
the worst-case rounding of an fp32 dot product with fp32-rounded taps (one rounding per tap, one per product, ntaps - 1
additions, the final scale).  The measured rms error per case is printed; profiles/resample.txt records those figures."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG
from oracle import stft as OS

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(PKG, "archs"))
STEPS = os.path.join(PKG, "steps")
PAIRS = [(16000, 8000), (48000, 8000), (44100, 8000), (11025, 8000), (8000, 16000),
         (8000, 10000), (16000, 10000)]      # the ratios scoring uses (stoi_gpu._at_10k): L / M = 5 / 4 and 5 / 8, both on the 1024 tile
# Ratios steep enough to leave the 1024-output tile, or to fill its LDS (dynamic LDS per workgroup, limit 61 440 B):
#   96000 -> 8000   L = 1,  M = 12,  1537 taps: tile 1024 with 61 408 B (samples + the tap row)
#   44100 -> 2000   L = 20, M = 441, 2823 taps: tile 512 with 56 368 B, taps from global memory
#  192000 -> 8000   L = 1,  M = 24,  3073 taps: tile 256 with 49 072 B
STEEP = [(96000, 8000), (44100, 2000), (192000, 8000)]
TILES = {(96000, 8000): 1024, (44100, 2000): 512, (192000, 8000): 256}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch.device("cuda", 0)


def _n_for(pl, n_out):
    """The shortest input whose output has at least n_out samples (exactly n_out wherever the ratio allows)."""
    n = (n_out * pl.M) // pl.L
    while pl.out_len(n) < n_out:
        n += 1
    return n


def _tile(pl):
    """Outputs per workgroup, by csrc/resample.hip's rule: the largest of 1024, 512, 256 whose input span -- and, for L == 1,
    the tap row behind it -- fits 60 KB of LDS."""
    tile = 1024
    while tile > 256 and 4 * ((tile - 1) * pl.M // pl.L + 2 + pl.ntaps * (2 if pl.L == 1 else 1)) > 60 * 1024:
        tile //= 2
    return tile


def _lengths(pl, nsig, rng):
    """nsig input lengths: one shorter than the filter's half-width, ones whose outputs end one sample either side of a tile
    boundary and on it, the rest random."""
    half_width = pl.half // pl.L                                      # num_zeros / scale input samples
    t = _tile(pl)
    special = [max(3, half_width // 3), _n_for(pl, t - 1), _n_for(pl, t + 1), _n_for(pl, t), _n_for(pl, 2 * t + 1), 1]
    out = special[:nsig]
    lo = _n_for(pl, 250)
    while len(out) < nsig:
        out.append(int(rng.integers(max(2000, lo), max(9000, 5 * lo))))
    return out


def _abs_sum(x, pl):
    """sum_k |h_k| |x_k| per output sample (fp64), h = the plan's taps."""
    n = np.arange(pl.out_len(len(x)), dtype=np.int64)
    k0, ph = pl.first(n), pl.phase(n)
    left, right = max(0, -int(k0.min())), max(0, int(k0.max()) + pl.ntaps - len(x))
    xp = np.concatenate([np.zeros(left), np.abs(x), np.zeros(right)])
    cols = np.arange(pl.ntaps, dtype=np.int64)[None, :]
    out = np.empty(len(n))
    for a in range(0, len(n), 2048):
        b = min(len(n), a + 2048)
        out[a:b] = np.einsum("ij,ij->i", xp[k0[a:b, None] + left + cols], np.abs(pl.taps[ph[a:b]]))
    return out


@pytest.mark.parametrize("pcm16", [True, False], ids=["int16", "float32"])
@pytest.mark.parametrize("sr_in,sr_out", PAIRS + STEEP)
def test_kernel_against_the_fp64_reference(dev, sr_in, sr_out, pcm16):
    from sepkern import ops
    from sepkern import resample as R
    pl = R.plan(sr_in, sr_out)
    assert _tile(pl) == TILES.get((sr_in, sr_out), 1024)
    rng = np.random.default_rng(sr_in + 7 * sr_out + int(pcm16))
    worst, sq, cnt = 0.0, 0.0, 0
    for nsig in range(1, 8):                                          # ragged batches of 1 to 7 signals
        ns = _lengths(pl, nsig, rng)
        if pcm16:
            sigs = [rng.integers(-20000, 20000, n).astype(np.int16) for n in ns]
            host = [s.astype(np.float64) / 32768.0 for s in sigs]
        else:
            sigs = [(0.5 * rng.standard_normal(n)).astype(np.float32) for n in ns]
            host = [s.astype(np.float64) for s in sigs]
        flat = torch.from_numpy(np.concatenate(sigs)).to(dev)
        out, outs = ops.resample_batch(flat, ns, sr_in, sr_out)
        assert outs == [R.out_len(n, sr_in, sr_out) for n in ns] and out.dtype == torch.float32 and out.numel() == sum(outs)
        again, _ = ops.resample_batch(flat, ns, sr_in, sr_out)
        assert torch.equal(out, again)                                # fixed summation order: bit-identical from run to run
        got = out.cpu().numpy().astype(np.float64)
        at = 0
        for x, m in zip(host, outs):
            ref = R.resample_host(x, sr_in, sr_out)
            bound = (pl.ntaps + 4) * 2.0 ** -24 * _abs_sum(x, pl)
            err = np.abs(got[at:at + m] - ref)
            assert np.all(err <= bound), (sr_in, sr_out, nsig, len(x), float((err - bound).max()), int(np.argmax(err - bound)))
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            sq += float((err ** 2).sum())
            cnt += m
            at += m
    print("sk_resample %5d -> %5d %-7s: rms error %.3g, largest error / bound %.3f"
          % (sr_in, sr_out, "int16" if pcm16 else "float32", np.sqrt(sq / cnt), worst))


@pytest.mark.parametrize("sr_in,sr_out", [(16000, 8000), (44100, 8000), (8000, 16000)])
def test_output_length_and_nothing_written_beyond_it(dev, sr_in, sr_out):
    from sepkern import ops
    from sepkern import resample as R
    pl = R.plan(sr_in, sr_out)
    rng = np.random.default_rng(5)
    ns = [_n_for(pl, 1024), _n_for(pl, 1025), 777, _n_for(pl, 3000)]
    outs = [pl.out_len(n) for n in ns]
    sigs = [rng.integers(-9000, 9000, n).astype(np.int16) for n in ns]
    flat = torch.from_numpy(np.concatenate(sigs)).to(dev)
    gap, sentinel = 37, -123.5
    out_offs, acc = [], gap
    for m in outs:
        out_offs.append(acc)
        acc += m + gap
    out = torch.full((acc,), sentinel, dtype=torch.float32, device=dev)
    in_offs = [int(v) for v in np.cumsum([0] + ns[:-1])]
    ops.resample_into(flat, in_offs, ns, out, out_offs, outs, sr_in, sr_out)
    got = out.cpu().numpy()
    dense, _ = ops.resample_batch(flat, ns, sr_in, sr_out)
    dense = dense.cpu().numpy()
    written = np.zeros(acc, bool)
    at = 0
    for o, m in zip(out_offs, outs):
        assert np.array_equal(got[o:o + m], dense[at:at + m])
        written[o:o + m] = True
        at += m
    assert np.all(got[~written] == sentinel)
    # a signal whose n_out is smaller than the grid was sized for: the words after its last sample stay untouched
    short = torch.full((outs[3] + gap,), sentinel, dtype=torch.float32, device=dev)
    ops.resample_into(flat, [in_offs[3], in_offs[0]], [ns[3], ns[0]], short, [0, outs[3] + gap - 5], [outs[3], 5], sr_in, sr_out)
    s = short.cpu().numpy()
    assert np.array_equal(s[:outs[3]], dense[sum(outs[:3]):]) and np.all(s[outs[3]:outs[3] + gap - 5] == sentinel)
    assert np.array_equal(s[-5:], dense[:5])


def _pcm_batch(arch, rate, target, lens, seed=0):
    from sepkern import synth
    samples = []
    for u, n in enumerate(lens):
        _, mix, srcs = synth.utterance(seed + u, n, 2)
        d = {"mix": mix, "source1": srcs[0], "source2": srcs[1]}
        if target is not None:
            d["rate"] = rate
        samples.append(d)
    return arch.WavCollator(target)(samples)


def test_same_rate_batches_take_the_old_path_bit_for_bit(dev, monkeypatch):
    import uPIT
    from sepkern import _lib
    from sepkern.data import features_from_pcm, wave_features_from_pcm
    lens = [9000, 7400, 6000, 4800]
    plain = _pcm_batch(uPIT, 8000, None, lens)["pcm"]
    rated = _pcm_batch(uPIT, 8000, 8000, lens)["pcm"]
    assert "rate" not in plain and rated["rate"] == [8000] * 4 and rated["target_rate"] == 8000
    assert torch.equal(plain["flat"], rated["flat"])
    names, real = [], _lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    a = features_from_pcm(plain, dev)
    b = features_from_pcm(rated, dev)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1])) and len(a[1]) == 2
    wa = wave_features_from_pcm(plain, dev)
    wb = wave_features_from_pcm(rated, dev)
    assert torch.equal(wa[0], wb[0]) and torch.equal(wa[3]["mixc"], wb[3]["mixc"]) and torch.equal(wa[3]["flat"], wb[3]["flat"])
    assert wb[3]["flat"].dtype == torch.int16 and wa[3]["nsamp"] == wb[3]["nsamp"] == lens
    assert "sk_stft" in names and "sk_resample" not in names
    # ... and a batch at another rate does launch it, once per rate
    names.clear()
    other = _pcm_batch(uPIT, 16000, 8000, [2 * n for n in lens])["pcm"]
    c = wave_features_from_pcm(other, dev)
    assert names.count("sk_resample") == 1 and c[3]["flat"].dtype == torch.float32 and c[3]["nsamp"] == lens


def test_more_signals_than_one_launch_takes(dev):
    """sk_resample takes 65535 signals per launch; ops.resample_into sends more in several.  65 537 copies of one 5-sample
    signal: every copy's output equals the first one's, and that one is within the kernel's bound of the reference."""
    from sepkern import ops
    from sepkern import resample as R
    pl = R.plan(8000, 16000)
    nsig, x = 65537, np.array([0.5, -0.25, 0.125, 0.75, -0.5], dtype=np.float32)
    out, outs = ops.resample_batch(torch.from_numpy(np.tile(x, nsig)).to(dev), [len(x)] * nsig, 8000, 16000)
    assert outs == [10] * nsig
    got = out.cpu().numpy().reshape(nsig, 10)
    assert np.array_equal(got, np.broadcast_to(got[0], got.shape))
    ref = R.resample_host(x, 8000, 16000)
    assert np.all(np.abs(got[0] - ref) <= (pl.ntaps + 4) * 2.0 ** -24 * _abs_sum(x.astype(np.float64), pl))


def test_a_batch_of_mixed_rates(dev):
    """features_from_pcm on a batch of 8 kHz and 16 kHz utterances (ops.pcm_to_rate: one launch for the 16 kHz signals, the
    8 kHz ones only scaled) == sk_stft of the signals resampled on the host; and pcm_to_rate itself against resample_host under
    the kernel's derived bound, the 8 kHz signals exactly x / 32768."""
    import uPIT
    from sepkern import ops, synth
    from sepkern import resample as R
    from sepkern.data import features_from_pcm
    rates, lens8 = [16000, 8000, 8000, 16000, 8000], [9000, 7400, 6000, 4800, 3000]
    samples = []
    for u, (r, n) in enumerate(zip(rates, lens8)):
        _, mix, srcs = synth.utterance(40 + u, n * r // 8000, 2)
        samples.append({"mix": mix, "source1": srcs[0], "source2": srcs[1], "rate": r})
    pcm = uPIT.WavCollator(8000)(samples)["pcm"]
    assert pcm["rate"] == rates and pcm["target_rate"] == 8000
    nkeys, flat = len(pcm["keys"]), pcm["flat"].numpy()
    y, outs = ops.pcm_to_rate(pcm["flat"].to(dev), pcm["lens"] * nkeys, rates * nkeys, 8000)
    assert outs == lens8 * nkeys and y.dtype == torch.float32
    y = y.cpu().numpy()
    pl = R.plan(16000, 8000)
    host, ai, ao = [], 0, 0
    for n, r, m in zip(pcm["lens"] * nkeys, rates * nkeys, outs):
        x = flat[ai:ai + n].astype(np.float64) / 32768.0
        if r == 8000:
            assert np.array_equal(y[ao:ao + m], x.astype(np.float32))
            host.append(x.astype(np.float32))
        else:
            ref = R.resample_host(x, r, 8000)
            assert np.all(np.abs(y[ao:ao + m] - ref) <= (pl.ntaps + 4) * 2.0 ** -24 * _abs_sum(x, pl))
            host.append(ref.astype(np.float32))
        ai, ao = ai + n, ao + m
    got = features_from_pcm(pcm, dev)
    direct = features_from_pcm({"flat": torch.from_numpy(np.concatenate(host)), "keys": list(pcm["keys"]), "lens": lens8}, dev)
    # the same sk_stft launches on float32 signals that differ by the resampler's fp32 rounding: the STFT's own tolerance
    tol = 1e-5 * float(direct[0].abs().max())
    assert got[0].shape == direct[0].shape and float((got[0] - direct[0]).abs().max()) <= tol
    assert len(got[1]) == len(direct[1]) == 2
    for a, b in zip(got[1], direct[1]):
        assert a.shape == b.shape and float((a - b).abs().max()) <= tol


def _run(*cmd):
    env = dict(os.environ, SEPKERN_HOME=PKG, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable] + list(cmd), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "%s failed:\n%s\n%s" % (cmd[0], r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


def test_extract_feats_on_a_16k_tree(dev, tmp_path):
    """npz magnitudes of a tree written at 16 kHz == |oracle.stft(resample_host(x))| within the STFT's own tolerance against
    oracle/stft.py (tests/test_gpu_kernels.py, tests/test_gpu_pipeline.py: 1e-5 of the largest bin -- an expression there, not
    a name that could be imported)."""
    import scipy.io.wavfile
    from sepkern import synth
    from sepkern import resample as R
    root = str(tmp_path)
    wavroot, data = os.path.join(root, "wav16k"), os.path.join(root, "data", "syn16")
    ids = synth.write_wav_tree(wavroot, 4, num_spk=2, min_s=1.0, max_s=2.0, rate=16000)
    synth.write_data_dir(data, wavroot, ids)
    ftrain, ftest = os.path.join(root, "feats", "train"), os.path.join(root, "feats", "test")
    _run(os.path.join(STEPS, "extract_feats.py"), data, "train", ftrain)
    _run(os.path.join(STEPS, "extract_feats.py"), data, "test", ftest)
    for i in ids:
        z = np.load(os.path.join(ftrain, i + ".npz"))
        assert z.files == ["mix", "s1", "s2"]
        for key in z.files:
            fs, pcm = scipy.io.wavfile.read(os.path.join(wavroot, key, i + ".wav"))
            assert fs == 16000
            y = R.resample_host(pcm.astype(np.float64) / 32768.0, 16000, 8000)
            ref = np.abs(OS.stft(y))
            assert z[key].dtype == np.float32 and z[key].shape == ref.shape == (257, 1 + R.out_len(len(pcm), 16000, 8000) // 128)
            np.testing.assert_allclose(z[key], ref, atol=1e-5 * ref.max())
        zt = np.load(os.path.join(ftest, i + ".npz"))
        _, pcm = scipy.io.wavfile.read(os.path.join(wavroot, "mix", i + ".wav"))
        ref = OS.stft(R.resample_host(pcm.astype(np.float64) / 32768.0, 16000, 8000))
        assert zt.files == ["mix"] and zt["mix"].dtype == np.complex64
        np.testing.assert_allclose(zt["mix"], ref, atol=1e-5 * np.abs(ref).max())


def test_sisdr_step_from_a_16k_wav_train_set(dev, tmp_path):
    """One loss=sisdr step from a 16 kHz WavTrainSet(sample_rate=8000) batch == the step fed the host-resampled float signals at
    8 kHz directly, within tests/test_gpu_sisdr.py's relative tolerance for its loss (1e-5)."""
    import uPIT
    from sepkern import synth
    from sepkern import resample as R
    root = str(tmp_path)
    wavroot, data = os.path.join(root, "wav16k"), os.path.join(root, "data", "syn16")
    ids = synth.write_wav_tree(wavroot, 5, num_spk=2, min_s=0.6, max_s=1.5, rate=16000, seed=3)
    synth.write_data_dir(data, wavroot, ids)
    ds = uPIT.WavTrainSet(data, sample_rate=8000)
    items = [ds[i] for i in range(len(ds))]
    assert all(it["rate"] == 16000 for it in items)
    batch = ds.collator(items)
    pcm = batch["pcm"]
    B, native = len(items), pcm["lens"]
    lens8 = [R.out_len(n, 16000, 8000) for n in native]
    assert ds.frame_counts() == [1 + R.out_len(len(it["mix"]), 16000, 8000) // 128 for it in items]
    # the same batch, resampled on the host in fp64 and handed over as float32 at 8 kHz
    flat16 = pcm["flat"].numpy()
    sigs, at = [], 0
    for _ in pcm["keys"]:
        for n in native:
            sigs.append(R.resample_host(flat16[at:at + n].astype(np.float64) / 32768.0, 16000, 8000).astype(np.float32))
            at += n
    direct = {"pcm": {"flat": torch.from_numpy(np.concatenate(sigs)), "keys": list(pcm["keys"]), "lens": lens8}}

    torch.manual_seed(11)
    model = uPIT.SepDNN(0, num_spk="2", hidden_dim="64", num_layers="2", loss="sisdr")
    model.cuda()
    model.train()
    h0, c0 = torch.randn(4, B, 64, device=dev), torch.randn(4, B, 64, device=dev)
    got = []
    for b in (batch, direct):
        model.next_hidden = (h0, c0)
        loss, norm = uPIT.compute_loss(model, 0, b)
        loss.backward()
        assert float(norm) == B and all(torch.isfinite(p.grad).all() for p in model.parameters())
        got.append((float(loss.detach()), model.last_best_perm.cpu().tolist()))
    print("loss=sisdr from a 16 kHz tree: %.7f dB, from host-resampled floats: %.7f dB" % (got[0][0], got[1][0]))
    assert got[0][1] == got[1][1]
    assert abs(got[0][0] - got[1][0]) <= 1e-5 * abs(got[1][0])
    # the prefetcher stages the same batch with the same keys: bit-identical loss
    from sepkern.data import Prefetcher
    staged = list(Prefetcher([batch], dev, keep_wave=True))
    assert staged[0]["wave"]["flat"].dtype == torch.float32 and staged[0]["wave"]["nsamp"] == lens8
    model.next_hidden = (h0, c0)
    loss2, _ = uPIT.compute_loss(model, 0, staged[0])
    assert float(loss2.detach()) == got[0][0]
