"""Multi-channel separation end to end on the MI355X (sepkern/separate.py, steps/separate_wav.py --mvdr): the network and
sk_stitch see the reference channel only and give the bits of the mono call on it; the beamformed spectra, the weights and the
waveforms are those of ops.mvdr and ops.mask_istft_streams on what the call returns."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "speech-separation_amd", "archs"))

F = 257
W, HN = 40, 20
T = 101
LB, R, LOADING = 32, 1, 1e-3
DRIVER = os.path.join(PKG, "steps", "separate_wav.py")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def model(dev):
    import uPIT
    torch.manual_seed(13)
    m = uPIT.SepDNN(0, hidden_dim="64", num_layers="2", num_spk="2")
    m.cuda()
    m.eval()
    return m


def seeded(model, seed=5):
    model.hidden_generator = torch.Generator(device="cuda")
    model.hidden_generator.manual_seed(seed)
    return model


def array_pcm(frames, seed, extra=17, rate_factor=1):
    """(3, n) int16: one noise signal as three microphones hear it -- delayed by 0, 3 and 7 samples, scaled, each with its own noise."""
    rng = np.random.default_rng(seed)
    n = rate_factor * (128 * (frames - 1) + extra)
    x = rng.standard_normal(n + 8) * 3000.0
    chans = [g * x[8 - d:8 - d + n] + 150.0 * rng.standard_normal(n) for d, g in ((0, 1.0), (3, 0.8), (7, 1.2))]
    return torch.from_numpy(np.stack(chans).astype(np.int16))


def bits(t):
    return torch.view_as_real(t).view(torch.int32) if t.is_complex() else t.view(torch.int32) if t.dtype == torch.float32 else t


def separate(model, pcm, rate=8000, **kw):
    from sepkern.separate import separate_recording
    out = separate_recording(seeded(model), pcm, rate, W, HN, batch_windows=3, return_details=True, want_pcm=True,
                             mvdr_block_frames=LB, mvdr_context_blocks=R, mvdr_loading=LOADING, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("ref", [0, 2])
def test_the_array_path_is_the_mono_path_on_the_reference_channel_then_mvdr(dev, model, ref):
    from sepkern import ops
    pcm = array_pcm(T, seed=1)
    wav, pcm16, d = separate(model, pcm, ref_channel=ref)
    _, _, mono = separate(model, pcm[ref].contiguous())
    assert "Y" not in mono and tuple(d["Y"].shape) == (3, T, F) and tuple(d["stitched"].shape) == (T, 2 * F)
    assert torch.equal(bits(d["stitched"]), bits(mono["stitched"])) and torch.equal(d["perms"], mono["perms"])
    assert torch.equal(bits(d["mag"]), bits(mono["mag"])) and torch.equal(bits(d["Y"][ref]), bits(mono["mixc"]))
    for c in range(3):                                          # every channel's spectrum is its own STFT
        assert torch.equal(bits(d["Y"][c]), bits(ops.stft_batch([pcm[c].contiguous().to(dev)], want_complex=True)[0]))
    weights, Z, _ = ops.mvdr(d["Y"], d["stitched"], 2, LB, R, ref, LOADING)
    assert tuple(weights.shape) == (4, 2, F, 3) and tuple(Z.shape) == (2, T, F)
    assert torch.equal(bits(d["weights"]), bits(weights)) and torch.equal(bits(d["Z"]), bits(Z))
    assert bool(torch.isfinite(torch.view_as_real(Z)).all())
    ref_wav, ref_pcm = ops.mask_istft_streams(d["Z"], None, 2, want_pcm=True, want_float=True)
    assert tuple(wav.shape) == (2, 128 * (T - 1)) and torch.equal(bits(wav), bits(ref_wav)) and torch.equal(pcm16, ref_pcm)
    # the post-mask is sk_mask_istft's mask argument
    wav_p, pcm_p, d_p = separate(model, pcm, ref_channel=ref, mvdr_postmask=True)
    assert torch.equal(bits(d_p["Z"]), bits(Z))
    ref_wav, ref_pcm = ops.mask_istft_streams(d_p["Z"], d_p["stitched"], 2, want_pcm=True, want_float=True)
    assert torch.equal(bits(wav_p), bits(ref_wav)) and torch.equal(pcm_p, ref_pcm) and not torch.equal(bits(wav_p), bits(wav))
    # one seed, two runs: the same bits
    wav2, pcm2, d2 = separate(model, pcm, ref_channel=ref)
    assert torch.equal(bits(wav), bits(wav2)) and torch.equal(pcm16, pcm2) and torch.equal(bits(d["weights"]), bits(d2["weights"]))
    assert model.training is False


def test_sixteen_kilohertz_array_pcm_comes_back_at_eight(dev, model):
    from sepkern.resample import out_len
    pcm = array_pcm(60, seed=3, extra=301, rate_factor=2)
    n16 = int(pcm.shape[1])
    wav, pcm16, d = separate(model, pcm, rate=16000, ref_channel=1)
    n8 = out_len(n16, 16000, 8000)
    Tn = 1 + n8 // 128
    assert tuple(wav.shape) == tuple(pcm16.shape) == (2, 128 * (Tn - 1)) and tuple(d["Y"].shape) == (3, Tn, F)
    assert bool(torch.isfinite(wav).all()) and float(wav.abs().max()) > 0.0
    _, _, mono = separate(model, pcm[1].contiguous(), rate=16000)          # the batched resampler gives the mono call's bits
    assert torch.equal(bits(d["stitched"]), bits(mono["stitched"])) and torch.equal(bits(d["Y"][1]), bits(mono["mixc"]))
    wavf, _, _ = separate(model, pcm.to(torch.float32) / 32768.0, rate=16000, ref_channel=1)
    assert tuple(wavf.shape) == tuple(wav.shape) and bool(torch.isfinite(wavf).all())


def test_arguments_out_of_range_are_refused_before_any_work(dev, model):
    from sepkern.separate import separate_recording
    pcm = array_pcm(T, seed=1)
    for kw in (dict(ref_channel=3), dict(mvdr_block_frames=0), dict(mvdr_context_blocks=-1), dict(mvdr_loading=-1.0)):
        with pytest.raises(ValueError, match="mvdr"):
            separate_recording(model, pcm, 8000, W, HN, **kw)
    with pytest.raises(ValueError, match="channels"):
        separate_recording(model, pcm[:1], 8000, W, HN)


def run_driver(tmp_path, scp, out, *more):
    return subprocess.run([sys.executable, DRIVER, os.path.join(PKG, "archs", "uPIT.py"), "0", str(tmp_path / "model.pt"), str(scp),
                           str(tmp_path / out), "--model-config", str(tmp_path / "model.conf"), "--window-frames", str(W),
                           "--hop-frames", str(HN), "--batch-windows", "3", "--seed", "1", "--mvdr-block-frames", str(LB)] + list(more),
                          capture_output=True, text=True, timeout=600)


def driver_inputs(model, tmp_path):
    """model.pt, model.conf, arr.wav (3 channels) + arr.scp, and the same audio as ch0..2.wav + ch0..2.scp; -> the (3, n) samples."""
    import scipy.io.wavfile
    torch.save(model.state_dict(), str(tmp_path / "model.pt"))
    (tmp_path / "model.conf").write_text("hidden_dim=64\nnum_layers=2\nnum_spk=2\n")
    x = array_pcm(T, seed=21).numpy()
    scipy.io.wavfile.write(str(tmp_path / "arr.wav"), 8000, np.ascontiguousarray(x.T))          # (n, 3): one 3-channel file
    (tmp_path / "arr.scp").write_text("recA %s\n" % (tmp_path / "arr.wav"))
    for c in range(3):                                                                          # the same audio, a file per channel
        n = x.shape[1] + (5 if c == 1 else 0)                                                   # one channel longer: cut to the shortest
        scipy.io.wavfile.write(str(tmp_path / ("ch%d.wav" % c)), 8000, np.concatenate([x[c], np.zeros(n - x.shape[1], np.int16)]))
        (tmp_path / ("ch%d.scp" % c)).write_text("recA %s\n" % (tmp_path / ("ch%d.wav" % c)))
    return x


def test_the_driver_takes_an_array_as_one_file_or_as_one_scp_per_channel(dev, model, tmp_path):
    import scipy.io.wavfile
    driver_inputs(model, tmp_path)
    r = run_driver(tmp_path, tmp_path / "arr.scp", "out_file", "--mvdr", "--ref-channel", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    r = run_driver(tmp_path, tmp_path / "ch0.scp", "out_scps", "--mvdr", "--ref-channel", "1", "--mvdr-channel-scps",
                   "%s,%s" % (tmp_path / "ch1.scp", tmp_path / "ch2.scp"))
    assert r.returncode == 0, r.stderr[-2000:]
    outs = {}
    for out in ("out_file", "out_scps"):
        assert sorted(os.listdir(str(tmp_path / out))) == ["s1", "s2"]
        for src in ("s1", "s2"):
            rate, y = scipy.io.wavfile.read(str(tmp_path / out / src / "recA.wav"))
            assert rate == 8000 and y.dtype == np.int16 and y.shape == (128 * (T - 1),)
            outs[out, src] = y
    for src in ("s1", "s2"):
        assert np.array_equal(outs["out_file", src], outs["out_scps", src])
    assert not np.array_equal(outs["out_file", "s1"], outs["out_file", "s2"])


def test_without_mvdr_the_driver_refuses_a_multi_channel_file_as_before(dev, model, tmp_path, capsys, monkeypatch):
    driver_inputs(model, tmp_path)
    r = run_driver(tmp_path, tmp_path / "arr.scp", "out_refused")
    assert r.returncode != 0 and "arr.wav: only mono 16-bit PCM wav is supported" in r.stderr
    assert not os.path.exists(str(tmp_path / "out_refused"))
    # further scps without --mvdr: refused before anything is loaded (in this process: nothing is started)
    monkeypatch.setenv("SEPKERN_HOME", PKG)                     # what the driver sets on import, undone after the test
    monkeypatch.syspath_prepend(os.path.dirname(DRIVER))
    import separate_wav
    rc = separate_wav.main([os.path.join(PKG, "archs", "uPIT.py"), "0", str(tmp_path / "model.pt"), str(tmp_path / "ch0.scp"),
                            str(tmp_path / "out_refused"), "--mvdr-channel-scps", str(tmp_path / "ch1.scp")])
    assert rc == 1 and "--mvdr-channel-scps needs --mvdr" in capsys.readouterr().err
