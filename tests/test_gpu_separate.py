"""Windowed separation end to end on the MI355X (sepkern/separate.py, steps/separate_wav.py): a recording of one window gives the
bits of the existing path, a longer one the bits of sepkern/stitch.py's definition applied to the windows the network produced,
any-rate PCM goes through the resampler, and the driver writes wav files."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT
from sepkern import stitch as st

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "speech-separation_amd", "archs"))

F = 257
W, HN = 40, 20
DRIVER = os.path.join(PKG, "steps", "separate_wav.py")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch.device("cuda", 0)


def make_model(S):
    import uPIT
    torch.manual_seed(11 + S)
    model = uPIT.SepDNN(0, hidden_dim="64", num_layers="2", num_spk=str(S))
    model.cuda()
    model.eval()
    return model


def seeded(model, seed=5):
    model.hidden_generator = torch.Generator(device="cuda")
    model.hidden_generator.manual_seed(seed)
    return model


def pcm_of_frames(T, seed, extra=17):
    """int16 noise of 128 (T - 1) + extra samples: T frames."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy((rng.standard_normal(128 * (T - 1) + extra) * 3000.0).astype(np.int16))


def window_arrays(desc, lens, S):
    """The window masks as numpy (len_k, S F) arrays, read through the descriptors ops.stitch took."""
    out = []
    for (t, off, stride), n in zip(desc, lens):
        out.append(torch.as_strided(t, (n, S * F), (stride, 1), t.storage_offset() + off).cpu().numpy())
    return out


@pytest.mark.parametrize("S", [2, 3])
def test_one_window_gives_the_bits_of_the_existing_path(dev, S):
    """T <= W: sk_stft, forward_packed from the same seed, sk_mask_istft -- stitching one window is a copy."""
    from sepkern import ops
    from sepkern.packing import Packing
    from sepkern.separate import separate_recording
    model, pcm, T = make_model(S), pcm_of_frames(31, seed=1), 31
    wav, pcm16 = separate_recording(seeded(model), pcm, 8000, W, HN, want_float=True, want_pcm=True)
    x = pcm.to(dev)
    mag = ops.stft_batch([x])[0]
    spec = ops.stft_batch([x], want_complex=True, layout="FT")[0]
    assert tuple(mag.shape) == (T, F)
    seeded(model)
    with torch.no_grad():
        model.hidden = model.init_hidden(1)
        mask = model.forward_packed(mag, Packing(np.array([T], dtype=np.int32), dev))
    masks = [mask[:T, s * F:(s + 1) * F].t().contiguous() for s in range(S)]
    ref_wav, ref_pcm = ops.mask_istft([spec], [masks])
    torch.cuda.synchronize()
    assert tuple(wav.shape) == (S, 128 * (T - 1)) and wav.dtype == torch.float32 and pcm16.dtype == torch.int16
    for s in range(S):
        assert torch.equal(wav[s].view(torch.int32), ref_wav[0][s].view(torch.int32))
        assert torch.equal(pcm16[s], ref_pcm[0][s])


@pytest.mark.parametrize("S", [2, 3])
def test_a_long_recording_is_the_definition_applied_to_its_windows(dev, S):
    """T = 101 frames = 2.5 windows of 40 and one of O + 1 frames: batches of 3, 1 and the short window alone."""
    from sepkern import ops
    from sepkern.separate import separate_recording
    model, pcm, T = make_model(S), pcm_of_frames(101, seed=2), 101
    wav, _, d = separate_recording(seeded(model), pcm, 8000, W, HN, batch_windows=3, return_details=True)
    torch.cuda.synchronize()
    lens = st.window_lengths(T, W, HN)
    assert lens == [40, 40, 40, 40, 21] and len(d["masks"]) == 5
    assert len({t.data_ptr() for t, _, _ in d["masks"]}) == 3               # three batches, where the network wrote them
    windows = window_arrays(d["masks"], lens, S)
    out, perms, cost = st.stitch_reference(d["mag"].cpu().numpy(), windows, W, HN, st.default_ramp(W - HN))
    worst = min(sorted(st.best_permutation(c)[1])[1] / min(st.best_permutation(c)[1]) for c in cost)
    print("S=%d: second-best / best >= %.2f over the boundaries" % (S, worst))
    assert np.array_equal(d["perms"].cpu().numpy(), perms)
    assert np.max(np.abs(d["cost"].cpu().numpy() - cost) / cost) <= 1e-10
    assert np.array_equal(d["stitched"].cpu().numpy().view(np.uint32), out.view(np.uint32))
    # the waveforms are sk_mask_istft of that result (through the existing (257, T) route)
    spec = d["mixc"].t().contiguous()
    masks = [torch.from_numpy(np.ascontiguousarray(out[:, s * F:(s + 1) * F].T)).to(dev) for s in range(S)]
    ref_wav, _ = ops.mask_istft([spec], [masks], want_pcm=False)
    assert tuple(wav.shape) == (S, 128 * (T - 1))
    for s in range(S):
        assert torch.equal(wav[s].view(torch.int32), ref_wav[0][s].view(torch.int32))
    # one seed, two runs: the same bits
    wav2, _, d2 = separate_recording(seeded(model), pcm, 8000, W, HN, batch_windows=3, return_details=True)
    assert torch.equal(wav.view(torch.int32), wav2.view(torch.int32)) and torch.equal(d["perms"], d2["perms"])
    assert torch.equal(d["stitched"].view(torch.int32), d2["stitched"].view(torch.int32))
    assert model.training is False


def test_sixteen_kilohertz_pcm_is_resampled_to_eight(dev):
    from sepkern.resample import out_len
    from sepkern.separate import separate_recording
    model = make_model(2)
    rng = np.random.default_rng(3)
    n16 = 2 * (128 * 60) + 301
    pcm = torch.from_numpy((rng.standard_normal(n16) * 3000.0).astype(np.int16))
    wav, pcm16 = separate_recording(seeded(model), pcm, 16000, W, HN, want_pcm=True)
    n8 = out_len(n16, 16000, 8000)
    T = 1 + n8 // 128
    assert n8 == (n16 + 1) // 2 and tuple(wav.shape) == tuple(pcm16.shape) == (2, 128 * (T - 1))
    assert bool(torch.isfinite(wav).all()) and float(wav.abs().max()) > 0.0


def write_wav(path, T, seed):
    import scipy.io.wavfile
    scipy.io.wavfile.write(path, 8000, pcm_of_frames(T, seed).numpy())


def test_the_driver_writes_one_wav_per_source_and_recording(dev, tmp_path):
    import scipy.io.wavfile
    model = make_model(2)
    torch.save(model.state_dict(), str(tmp_path / "model.pt"))
    (tmp_path / "model.conf").write_text("hidden_dim=64\nnum_layers=2\nnum_spk=2\n")
    frames = {"recA": 101, "recB": 33}
    for i, (ID, T) in enumerate(frames.items()):
        write_wav(str(tmp_path / (ID + ".wav")), T, seed=20 + i)
    (tmp_path / "wav.scp").write_text("".join("%s %s\n" % (ID, tmp_path / (ID + ".wav")) for ID in frames))
    r = subprocess.run([sys.executable, DRIVER, os.path.join(PKG, "archs", "uPIT.py"), "0", str(tmp_path / "model.pt"),
                        str(tmp_path / "wav.scp"), str(tmp_path / "out"), "--model-config", str(tmp_path / "model.conf"),
                        "--window-frames", str(W), "--hop-frames", str(HN), "--batch-windows", "3", "--seed", "1"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "frames/s" in r.stderr and "real-time factor" in r.stderr
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["s1", "s2"]
    for src in ("s1", "s2"):
        for ID, T in frames.items():
            rate, x = scipy.io.wavfile.read(str(tmp_path / "out" / src / (ID + ".wav")))
            assert rate == 8000 and x.dtype == np.int16 and x.shape == (128 * (T - 1),)


def test_the_driver_refuses_the_rsh_arch_without_a_traceback(dev, tmp_path):
    (tmp_path / "wav.scp").write_text("")
    r = subprocess.run([sys.executable, DRIVER, os.path.join(PKG, "archs", "RSH.py"), "0", str(tmp_path / "no_model.pt"),
                        str(tmp_path / "wav.scp"), str(tmp_path / "out")], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert "separate_wav: the arch module RSH.py has no SepDNN.forward_packed; windowed separation runs the uPIT arch only" in r.stderr
    assert "Traceback" not in r.stderr and not os.path.exists(str(tmp_path / "out"))
