"""Separation with WPD beamformers in the beamformer's place, end to end on the MI355X (sepkern/separate.py,
steps/separate_wav.py --wpd): Z and the filters are ops.wpd's bits on the spectra and the masks the call returns, the wav is
ops.mask_istft_streams' bits of that Z, with wpe the network sees |X[ref]| while WPD still sees Y, and without wpd the call
gives the bits it gave before."""
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
CACGMM = dict(cacgmm_iterations=3, cacgmm_block_frames=40, cacgmm_context_frames=12, cacgmm_loading=1e-3)
CACGMM_ARGS = (3, 40, 12, 1e-3)
WPD = dict(wpd_taps=3, wpd_delay=2, wpd_iterations=2, wpd_block_frames=48, wpd_context_frames=8, wpd_loading=1e-3, wpd_floor=1e-6)
WPD_ARGS = (3, 2, 2, 48, 8, 1e-3, 1e-6)
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


@pytest.mark.parametrize("ref", [0, 2])
@pytest.mark.parametrize("postmask", [False, True])
def test_the_stitched_masks_steer_the_wpd_beamformers(dev, model, ref, postmask):
    from sepkern import ops
    pcm = array_pcm(T, seed=1)
    wav, pcm16, d = separate(model, pcm, ref_channel=ref, mvdr=False, wpd=True, wpd_postmask=postmask, **WPD)
    _, _, plain = separate(model, pcm, ref_channel=ref)
    for k in ("stitched", "mag", "mixc", "Y"):                                               # everything upstream keeps its bits
        assert torch.equal(bits(d[k]), bits(plain[k])), k
    assert "weights" not in d and "X" not in d and "cacgmm_masks" not in d
    Z, Wd = ops.wpd(d["Y"], d["stitched"], 2, *WPD_ARGS, ref=ref, want_W=True)
    assert tuple(d["Z"].shape) == (2, T, F) and tuple(d["wpd_weights"].shape) == (3, 2, F, 12)
    assert torch.equal(bits(d["Z"]), bits(Z)) and torch.equal(bits(d["wpd_weights"]), bits(Wd))
    assert bool(torch.isfinite(torch.view_as_real(Z)).all()) and not torch.equal(bits(Z), bits(plain["Z"]))
    ref_wav, ref_pcm = ops.mask_istft_streams(Z, d["stitched"] if postmask else None, 2, want_pcm=True, want_float=True)
    assert tuple(wav.shape) == (2, 128 * (T - 1)) and torch.equal(bits(wav), bits(ref_wav)) and torch.equal(pcm16, ref_pcm)
    # one seed, two runs: the same bits
    wav2, pcm2, d2 = separate(model, pcm, ref_channel=ref, mvdr=False, wpd=True, wpd_postmask=postmask, **WPD)
    assert torch.equal(bits(wav), bits(wav2)) and torch.equal(pcm16, pcm2) and torch.equal(bits(d["Z"]), bits(d2["Z"]))


@pytest.mark.parametrize("wpe", [False, True])
def test_with_cacgmm_its_masks_steer_and_with_wpe_the_network_sees_x_while_wpd_sees_y(dev, model, wpe):
    from sepkern import ops
    pcm = array_pcm(T, seed=1)
    more = dict(WPE, wpe=True) if wpe else {}
    wav, pcm16, d = separate(model, pcm, ref_channel=1, mvdr=False, wpd=True, cacgmm=True, **WPD, **CACGMM, **more)
    _, _, d0 = separate(model, pcm, ref_channel=1, mvdr=False, wpd=True, **WPD, **more)
    _, _, plain = separate(model, pcm, ref_channel=1)
    assert torch.equal(bits(d["Y"]), bits(plain["Y"])) and torch.equal(bits(d0["Y"]), bits(plain["Y"]))   # Y is kept untouched
    if wpe:
        X, mag, _ = ops.wpe(d["Y"], *WPE_ARGS, ref=1, want_mag=True)
        for dd in (d, d0):
            assert torch.equal(bits(dd["X"]), bits(X)) and torch.equal(bits(dd["mag"]), bits(mag)) and torch.equal(bits(dd["mixc"]), bits(X[1]))
        assert not torch.equal(bits(d["mag"]), bits(plain["mag"]))
    else:
        assert "X" not in d and torch.equal(bits(d["mag"]), bits(plain["mag"]))
    refined, _ = ops.cacgmm(d["X"] if wpe else d["Y"], d["stitched"], 2, *CACGMM_ARGS)
    assert torch.equal(bits(d["cacgmm_masks"]), bits(refined)) and "cacgmm_masks" not in d0
    for dd, steer in ((d, refined), (d0, d0["stitched"])):
        Z, Wd = ops.wpd(dd["Y"], steer, 2, *WPD_ARGS, ref=1, want_W=True)                    # on Y, with or without wpe
        assert torch.equal(bits(dd["Z"]), bits(Z)) and torch.equal(bits(dd["wpd_weights"]), bits(Wd))
    assert not torch.equal(bits(d["Z"]), bits(d0["Z"]))
    ref_wav, ref_pcm = ops.mask_istft_streams(d["Z"], None, 2, want_pcm=True, want_float=True)
    assert torch.equal(bits(wav), bits(ref_wav)) and torch.equal(pcm16, ref_pcm)


def test_without_wpd_the_calls_give_the_bits_of_before(dev, model):
    """wpd=False is the default: one cascade configuration (wpe, cacgmm, mvdr with the post-mask) with the keyword absent and
    with it False, every wpd_* argument set, gives the same bits, and they are the cascade's own calls on the details."""
    from sepkern import ops
    pcm = array_pcm(T, seed=2)
    cascade = dict(ref_channel=1, mvdr_postmask=True, wpe=True, cacgmm=True, **WPE, **CACGMM)
    wav, pcm16, d = separate(model, pcm, **cascade)
    wav0, pcm0, d0 = separate(model, pcm, wpd=False, wpd_postmask=True, **WPD, **cascade)
    assert sorted(d) == sorted(d0) and "wpd_weights" not in d
    for k in ("stitched", "cacgmm_masks", "weights", "Z", "X", "Y", "mag", "mixc"):
        assert torch.equal(bits(d[k]), bits(d0[k])), k
    assert torch.equal(bits(wav), bits(wav0)) and torch.equal(pcm16, pcm0)
    weights, Z, _ = ops.mvdr(d["X"], d["cacgmm_masks"], 2, LB, R, 1, LOADING)
    assert torch.equal(bits(d["weights"]), bits(weights)) and torch.equal(bits(d["Z"]), bits(Z))
    ref_wav, ref_pcm = ops.mask_istft_streams(Z, d["stitched"], 2, want_pcm=True, want_float=True)
    assert torch.equal(bits(wav), bits(ref_wav)) and torch.equal(pcm16, ref_pcm)


def test_a_mono_recording_an_mvdr_request_and_arguments_out_of_range_are_refused(dev, model):
    from sepkern.separate import separate_recording
    pcm = array_pcm(T, seed=1)
    with pytest.raises(ValueError, match="wpd needs a"):
        separate_recording(model, pcm[0].contiguous(), 8000, W, HN, wpd=True, mvdr=False)
    with pytest.raises(ValueError, match="wpd takes the beamformer's place"):
        separate_recording(model, pcm, 8000, W, HN, wpd=True, mvdr=True)
    with pytest.raises(ValueError, match="wpd takes the beamformer's place"):
        separate_recording(model, pcm, 8000, W, HN, wpd=True)                                # mvdr is on unless it is turned off
    with pytest.raises(ValueError, match="cacgmm needs"):
        separate_recording(model, pcm, 8000, W, HN, cacgmm=True, mvdr=False, wpe=True)
    for kw in (dict(wpd_taps=-1), dict(wpd_taps=26), dict(wpd_delay=0), dict(wpd_iterations=9), dict(wpd_block_frames=0),
               dict(wpd_context_frames=-1), dict(wpd_block_frames=4097), dict(wpd_loading=-1.0), dict(wpd_floor=0.0), dict(wpd_floor=2.0)):
        with pytest.raises(ValueError, match="wpd: "):
            separate_recording(model, pcm, 8000, W, HN, wpd=True, mvdr=False, **kw)


def test_the_driver_writes_the_functions_pcm_and_refuses_wpd_with_mvdr(dev, model, tmp_path):
    import scipy.io.wavfile
    torch.save(model.state_dict(), str(tmp_path / "model.pt"))
    (tmp_path / "model.conf").write_text("hidden_dim=64\nnum_layers=2\nnum_spk=2\n")
    x = array_pcm(T, seed=21)
    scipy.io.wavfile.write(str(tmp_path / "arr.wav"), 8000, np.ascontiguousarray(x.numpy().T))
    (tmp_path / "arr.scp").write_text("recA %s\n" % (tmp_path / "arr.wav"))
    common = [sys.executable, DRIVER, os.path.join(PKG, "archs", "uPIT.py"), "0", str(tmp_path / "model.pt"), str(tmp_path / "arr.scp")]
    r = subprocess.run(common + [str(tmp_path / "out"), "--model-config", str(tmp_path / "model.conf"), "--window-frames", str(W),
                                 "--hop-frames", str(HN), "--batch-windows", "3", "--seed", "1", "--ref-channel", "1", "--wpd",
                                 "--wpd-taps", "3", "--wpd-delay", "2", "--wpd-iterations", "2", "--wpd-block-frames", "48",
                                 "--wpd-context-frames", "8", "--wpd-loading", "1e-3", "--wpd-floor", "1e-6", "--wpd-postmask"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["s1", "s2"]
    from sepkern.separate import separate_recording
    _, want = separate_recording(seeded(model, seed=1), x, 8000, W, HN, batch_windows=3, want_float=False, want_pcm=True, ref_channel=1,
                                 mvdr=False, wpd=True, wpd_postmask=True, **WPD)
    _, plain = separate_recording(seeded(model, seed=1), x, 8000, W, HN, batch_windows=3, want_float=False, want_pcm=True, ref_channel=1,
                                  mvdr_postmask=True)
    want, plain = want.cpu().numpy(), plain.cpu().numpy()
    for s, src in enumerate(("s1", "s2")):
        rate, y = scipy.io.wavfile.read(str(tmp_path / "out" / src / "recA.wav"))
        assert rate == 8000 and y.dtype == np.int16 and y.shape == (128 * (T - 1),) and np.array_equal(y, want[s])
    assert not np.array_equal(want, plain)                       # the WPD beamformers reached the output
    r = subprocess.run(common + [str(tmp_path / "out2"), "--wpd", "--mvdr"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "--wpd takes the place of --mvdr" in r.stderr and not os.path.exists(str(tmp_path / "out2"))
