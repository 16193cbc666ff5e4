"""Separation with WPE in front, end to end on the MI355X (sepkern/separate.py, steps/separate_wav.py --wpe): X is ops.wpe's
bits on the spectra the call returns, the network sees sk_wpe's mag_out, everything downstream is the plain path's on X, and
without wpe the call gives the bits it gave before."""
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
WPE = dict(wpe_taps=4, wpe_delay=2, wpe_iterations=2, wpe_block_frames=48, wpe_context_frames=8, wpe_loading=1e-3)
WPE_ARGS = (4, 2, 2, 48, 8, 1e-3)
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


def array_pcm(frames, seed, extra=17):
    """(3, n) int16: one noise signal with an echo as three microphones hear it, each with its own noise."""
    rng = np.random.default_rng(seed)
    n = 128 * (frames - 1) + extra
    x = rng.standard_normal(n + 1000) * 2500.0
    chans = [g * (x[1000 - d:1000 - d + n] + 0.5 * x[1000 - d - e:1000 - d - e + n]) + 150.0 * rng.standard_normal(n)
             for d, g, e in ((0, 1.0, 700), (3, 0.8, 820), (7, 1.2, 930))]
    return torch.from_numpy(np.stack(chans).astype(np.int16))


def bits(t):
    return torch.view_as_real(t).view(torch.int32) if t.is_complex() else t.view(torch.int32) if t.dtype == torch.float32 else t


def separate(model, pcm, **kw):
    from sepkern.separate import separate_recording
    out = separate_recording(seeded(model), pcm, 8000, W, HN, batch_windows=3, return_details=True, want_pcm=True,
                             mvdr_block_frames=LB, mvdr_context_blocks=R, mvdr_loading=LOADING, **kw)
    torch.cuda.synchronize()
    return out


def stitched_from(model, mag):
    """The plain path's windows and sk_stitch on a given magnitude spectrogram."""
    from sepkern import ops, stitch as st
    from sepkern.separate import window_masks
    seeded(model)
    with torch.no_grad():
        windows = window_masks(model, mag, W, HN, 3)
    ramp = torch.from_numpy(st.default_ramp(W - HN)).to(mag.device)
    return ops.stitch(mag, windows, int(mag.shape[0]), W, HN, 2, ramp)[0]


def test_mono_with_wpe_is_ops_wpe_then_the_plain_path(dev, model):
    from sepkern import ops
    pcm = array_pcm(T, seed=1)[0].contiguous()
    wav, pcm16, d = separate(model, pcm, wpe=True, **WPE)
    _, _, plain = separate(model, pcm)
    assert tuple(d["Y"].shape) == tuple(d["X"].shape) == (1, T, F) and torch.equal(bits(d["Y"][0]), bits(plain["mixc"]))
    X, mag, _ = ops.wpe(d["Y"], *WPE_ARGS, ref=0, want_mag=True)
    assert torch.equal(bits(d["X"]), bits(X)) and torch.equal(bits(d["mag"]), bits(mag)) and torch.equal(bits(d["mixc"]), bits(X[0]))
    assert not torch.equal(bits(d["X"]), bits(d["Y"])) and bool(torch.isfinite(torch.view_as_real(X)).all())
    assert torch.equal(bits(d["stitched"]), bits(stitched_from(model, mag)))
    ref_wav, ref_pcm = ops.mask_istft_frames(X[0], d["stitched"], 2, want_pcm=True, want_float=True)
    assert tuple(wav.shape) == (2, 128 * (T - 1)) and torch.equal(bits(wav), bits(ref_wav)) and torch.equal(pcm16, ref_pcm)
    # one seed, two runs: the same bits
    wav2, pcm2, d2 = separate(model, pcm, wpe=True, **WPE)
    assert torch.equal(bits(wav), bits(wav2)) and torch.equal(pcm16, pcm2) and torch.equal(bits(d["X"]), bits(d2["X"]))


@pytest.mark.parametrize("ref", [0, 2])
def test_an_array_with_wpe_beamforms_the_dereverberated_spectra(dev, model, ref):
    from sepkern import ops
    pcm = array_pcm(T, seed=1)
    wav, pcm16, d = separate(model, pcm, ref_channel=ref, wpe=True, **WPE)
    _, _, plain = separate(model, pcm, ref_channel=ref)
    assert torch.equal(bits(d["Y"]), bits(plain["Y"]))                                             # Y is kept untouched
    X, mag, _ = ops.wpe(d["Y"], *WPE_ARGS, ref=ref, want_mag=True)
    assert torch.equal(bits(d["X"]), bits(X)) and torch.equal(bits(d["mag"]), bits(mag)) and torch.equal(bits(d["mixc"]), bits(X[ref]))
    assert torch.equal(bits(d["stitched"]), bits(stitched_from(model, mag)))
    weights, Z, _ = ops.mvdr(X, d["stitched"], 2, LB, R, ref, LOADING)
    assert torch.equal(bits(d["weights"]), bits(weights)) and torch.equal(bits(d["Z"]), bits(Z))
    ref_wav, ref_pcm = ops.mask_istft_streams(Z, None, 2, want_pcm=True, want_float=True)
    assert torch.equal(bits(wav), bits(ref_wav)) and torch.equal(pcm16, ref_pcm)
    # without the beamformer the masks are applied to the dereverberated reference channel
    wav_m, pcm_m, d_m = separate(model, pcm, ref_channel=ref, wpe=True, mvdr=False, **WPE)
    assert torch.equal(bits(d_m["X"]), bits(X)) and "Z" not in d_m
    ref_wav, ref_pcm = ops.mask_istft_frames(X[ref], d_m["stitched"], 2, want_pcm=True, want_float=True)
    assert torch.equal(bits(wav_m), bits(ref_wav)) and torch.equal(pcm_m, ref_pcm)


def test_without_wpe_the_calls_give_the_bits_of_before(dev, model):
    """wpe=False is the default: the mono and the array call are ops.stft_batch, the windows, ops.stitch and the iSTFT (or
    ops.mvdr) on Y, as tests/test_gpu_separate.py and tests/test_gpu_separate_mvdr.py pin them."""
    from sepkern import ops
    pcm = array_pcm(T, seed=2)
    for p in (pcm[1].contiguous(), pcm):
        wav, pcm16, d = separate(model, p)
        wav0, pcm0, d0 = separate(model, p, wpe=False, **WPE)
        assert "X" not in d and "X" not in d0
        assert torch.equal(bits(wav), bits(wav0)) and torch.equal(pcm16, pcm0) and torch.equal(bits(d["stitched"]), bits(d0["stitched"]))
        ref = p if p.dim() == 1 else p[0].contiguous()
        assert torch.equal(bits(d["mag"]), bits(ops.stft_batch([ref.to(dev)], want_complex=False)[0]))
        assert torch.equal(bits(d["mixc"]), bits(ops.stft_batch([ref.to(dev)], want_complex=True)[0]))
        assert torch.equal(bits(d["stitched"]), bits(stitched_from(model, d["mag"])))


def test_arguments_out_of_range_are_refused_before_any_work(dev, model):
    from sepkern.separate import separate_recording
    pcm = array_pcm(T, seed=1)
    for kw in (dict(wpe_taps=0), dict(wpe_taps=27), dict(wpe_delay=0), dict(wpe_iterations=9), dict(wpe_block_frames=0),
               dict(wpe_context_frames=-1), dict(wpe_block_frames=4097), dict(wpe_loading=-1.0)):
        with pytest.raises(ValueError, match="wpe"):
            separate_recording(model, pcm, 8000, W, HN, wpe=True, **kw)
    with pytest.raises(ValueError, match="needs mvdr or wpe"):
        separate_recording(model, pcm, 8000, W, HN, mvdr=False)


def run_driver(tmp_path, scp, out, *more):
    return subprocess.run([sys.executable, DRIVER, os.path.join(PKG, "archs", "uPIT.py"), "0", str(tmp_path / "model.pt"), str(scp),
                           str(tmp_path / out), "--model-config", str(tmp_path / "model.conf"), "--window-frames", str(W),
                           "--hop-frames", str(HN), "--batch-windows", "3", "--seed", "1", "--mvdr-block-frames", str(LB),
                           "--wpe-taps", "4", "--wpe-delay", "2", "--wpe-iterations", "2", "--wpe-block-frames", "48",
                           "--wpe-context-frames", "8"] + list(more), capture_output=True, text=True, timeout=600)


def driver_inputs(model, tmp_path):
    """model.pt, model.conf, arr.wav (3 channels) + arr.scp, and the same audio as ch0..2.wav + ch0..2.scp."""
    import scipy.io.wavfile
    torch.save(model.state_dict(), str(tmp_path / "model.pt"))
    (tmp_path / "model.conf").write_text("hidden_dim=64\nnum_layers=2\nnum_spk=2\n")
    x = array_pcm(T, seed=21).numpy()
    scipy.io.wavfile.write(str(tmp_path / "arr.wav"), 8000, np.ascontiguousarray(x.T))
    (tmp_path / "arr.scp").write_text("recA %s\n" % (tmp_path / "arr.wav"))
    for c in range(3):
        scipy.io.wavfile.write(str(tmp_path / ("ch%d.wav" % c)), 8000, x[c])
        (tmp_path / ("ch%d.scp" % c)).write_text("recA %s\n" % (tmp_path / ("ch%d.wav" % c)))


def read_outputs(tmp_path, out):
    import scipy.io.wavfile
    assert sorted(os.listdir(str(tmp_path / out))) == ["s1", "s2"]
    ys = []
    for src in ("s1", "s2"):
        rate, y = scipy.io.wavfile.read(str(tmp_path / out / src / "recA.wav"))
        assert rate == 8000 and y.dtype == np.int16 and y.shape == (128 * (T - 1),)
        ys.append(y)
    return ys


@pytest.mark.parametrize("mvdr", [False, True])
def test_the_driver_writes_the_same_files_for_one_array_file_and_for_three_scps(dev, model, tmp_path, mvdr):
    driver_inputs(model, tmp_path)
    more = ["--wpe", "--ref-channel", "1"] + (["--mvdr"] if mvdr else [])
    r = run_driver(tmp_path, tmp_path / "arr.scp", "out_file", *more)
    assert r.returncode == 0, r.stderr[-2000:]
    r = run_driver(tmp_path, tmp_path / "ch0.scp", "out_scps", *more, "--mvdr-channel-scps", "%s,%s" % (tmp_path / "ch1.scp", tmp_path / "ch2.scp"))
    assert r.returncode == 0, r.stderr[-2000:]
    a, b = read_outputs(tmp_path, "out_file"), read_outputs(tmp_path, "out_scps")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[0], a[1])


def test_the_driver_takes_wpe_on_a_mono_file(dev, model, tmp_path):
    driver_inputs(model, tmp_path)
    r = run_driver(tmp_path, tmp_path / "ch1.scp", "out_wpe", "--wpe")
    assert r.returncode == 0, r.stderr[-2000:]
    r = run_driver(tmp_path, tmp_path / "ch1.scp", "out_plain")
    assert r.returncode == 0, r.stderr[-2000:]
    a, b = read_outputs(tmp_path, "out_wpe"), read_outputs(tmp_path, "out_plain")
    assert not np.array_equal(a[0], b[0])                        # the dereverberation reached the output
