"""Separation with a model that sees the array (conf key ipd_channels; sepkern/separate.py, sepkern/ipd.py) on the MI355X: the
rows handed to the network are sk_ipd_rows of the spectra the masks are applied to -- Y, or X after WPE --, everything behind
the network is the path it was, and a mono model gives the bits it gave before."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "speech-separation_amd", "archs"))

F = 257
W, HN = 32, 16
T = 81                                     # about 2.5 windows of 32 frames: starts 0, 16, 32, 48 and a short last one
LB, R, LOADING = 32, 1, 1e-3
WPE = dict(wpe_taps=4, wpe_delay=2, wpe_iterations=2, wpe_block_frames=48, wpe_context_frames=8, wpe_loading=1e-3)
WPE_ARGS = (4, 2, 2, 48, 8, 1e-3)
CHANS = (2, 1)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch.device("cuda", 0)


def _make(ipd, ref=0):
    import uPIT
    torch.manual_seed(13)
    conf = dict(hidden_dim="64", num_layers="2", num_spk="2")
    if ipd:
        conf.update(ipd_channels=",".join(str(c) for c in CHANS), ipd_ref=str(ref))
    m = uPIT.SepDNN(0, **conf)
    m.cuda()
    m.eval()
    return m


@pytest.fixture(scope="module")
def model(dev):
    return _make(True)


@pytest.fixture(scope="module")
def mono_model(dev):
    return _make(False)


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


def separate(model, pcm, captured=None, monkeypatch=None, **kw):
    """separate_recording with the test's geometry; captured: a list that receives every tensor handed to window_masks."""
    from sepkern import separate as sp
    if captured is not None:
        real = sp.window_masks

        def spy(mdl, rows, *a):
            captured.append(rows)
            return real(mdl, rows, *a)
        monkeypatch.setattr(sp, "window_masks", spy)
    out = sp.separate_recording(seeded(model), pcm, 8000, W, HN, batch_windows=3, return_details=True, want_pcm=True,
                                mvdr_block_frames=LB, mvdr_context_blocks=R, mvdr_loading=LOADING, **kw)
    torch.cuda.synchronize()
    return out


def stitched_from(model, rows, mag):
    """The windows on given network rows and sk_stitch on the magnitudes."""
    from sepkern import ops, stitch as st
    from sepkern.separate import window_masks
    seeded(model)
    with torch.no_grad():
        windows = window_masks(model, rows, W, HN, 3)
    ramp = torch.from_numpy(st.default_ramp(W - HN)).to(mag.device)
    return ops.stitch(mag, windows, int(mag.shape[0]), W, HN, 2, ramp)[0]


@pytest.mark.parametrize("mode", ["plain", "mvdr", "wpe"])
def test_the_network_sees_sk_ipd_rows_of_the_spectra_the_masks_go_to(dev, model, monkeypatch, mode):
    from sepkern import ipd, ops
    pcm = array_pcm(T, seed=1)
    kw = dict(plain=dict(mvdr=False), mvdr=dict(mvdr=True), wpe=dict(mvdr=False, wpe=True, **WPE))[mode]
    seen = []
    wav, pcm16, d = separate(model, pcm, seen, monkeypatch, **kw)
    # Y, mag and mixc are the array path's of before; the rows are sk_ipd_rows of Y (of X after WPE) with those magnitudes
    flat = pcm.to(dev).contiguous().view(-1)
    n = int(pcm.shape[1])
    Y = torch.empty(3, T, F, dtype=torch.complex64, device=dev)
    ops.stft_batch(flat, want_complex=True, out=Y.view(-1), out_offs=[c * T * F for c in range(3)], stride_t=[F] * 3, stride_f=[1] * 3,
                   lengths=[n] * 3)
    if mode == "wpe":
        S, mag, _ = ops.wpe(Y, *WPE_ARGS, ref=0, want_mag=True)
        assert torch.equal(bits(d["X"]), bits(S)) and torch.equal(bits(d["Y"]), bits(Y))
    else:
        S, mag = Y, ops.stft_batch([pcm[0].contiguous().to(dev)], want_complex=False)[0]
    rows = ops.ipd_rows(S, 0, CHANS, mag)
    assert len(seen) == 1 and seen[0].shape == (T, ipd.padded_dim(2)) == (T, 1296)
    assert torch.equal(bits(seen[0]), bits(rows)) and torch.equal(bits(d["net_rows"]), bits(rows))
    assert torch.equal(bits(d["mag"]), bits(mag)) and torch.equal(bits(rows[:, :F]), bits(mag)) and torch.equal(bits(d["mixc"]), bits(S[0]))
    assert not rows[:, ipd.in_dim(2):].any() and bool(torch.isfinite(rows).all())
    (c0, c1), (s0, s1) = ipd.columns(0)
    assert float((rows[:, c0:c1] ** 2 + rows[:, s0:s1] ** 2 - 1.0).abs().max()) < 1e-5
    # behind the network nothing changed: stitching on the magnitudes, then the iSTFT or the beamformer
    assert tuple(d["stitched"].shape) == (T, 2 * F) and torch.equal(bits(d["stitched"]), bits(stitched_from(model, rows, mag)))
    if mode == "mvdr":
        weights, Z, _ = ops.mvdr(Y, d["stitched"], 2, LB, R, 0, LOADING)
        assert torch.equal(bits(d["Z"]), bits(Z))
        ref_wav, ref_pcm = ops.mask_istft_streams(Z, None, 2, want_pcm=True, want_float=True)
    else:
        assert "Z" not in d
        ref_wav, ref_pcm = ops.mask_istft_frames(S[0], d["stitched"], 2, want_pcm=True, want_float=True)
    assert tuple(wav.shape) == tuple(pcm16.shape) == (2, 128 * (T - 1)) and pcm16.dtype == torch.int16
    assert torch.equal(bits(wav), bits(ref_wav)) and torch.equal(pcm16, ref_pcm) and bool(torch.isfinite(wav).all())
    assert not torch.equal(pcm16[0], pcm16[1])
    # the phase columns reach the masks: with the listed channels exchanged the masks differ
    other = ops.ipd_rows(S, 0, CHANS[::-1], mag)
    assert not torch.equal(bits(stitched_from(model, other, mag)), bits(d["stitched"]))


def test_the_reference_channel_and_the_listed_channels_must_be_there(dev, model, mono_model):
    from sepkern.separate import separate_recording
    pcm = array_pcm(T, seed=1)
    with pytest.raises(ValueError, match="ref_channel = 1, but the model was trained with ipd_ref = 0"):
        separate_recording(model, pcm, 8000, W, HN, ref_channel=1)
    with pytest.raises(ValueError, match="the recording has 2 channels.*need channel 2"):
        separate_recording(model, pcm[:2], 8000, W, HN)
    with pytest.raises(ValueError, match=r"needs a \(C, n\) pcm"):
        separate_recording(model, pcm[0].contiguous(), 8000, W, HN)
    with pytest.raises(ValueError, match="needs mvdr or wpe"):            # a mono model still refuses an array without a beamformer
        separate_recording(mono_model, pcm, 8000, W, HN, mvdr=False)


def test_a_mono_model_gives_the_bits_of_before(dev, mono_model, monkeypatch):
    """The 1-D call and the array call of a model without ipd_channels: the network sees the magnitudes themselves, sk_ipd_rows
    is never called, and the outputs are the plain path's -- ops.stft_batch, the windows, ops.stitch, the iSTFT (or ops.mvdr)."""
    from sepkern import _lib, ops
    calls = []
    real = _lib.call

    def spy(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    pcm = array_pcm(T, seed=2)
    for p in (pcm[0].contiguous(), pcm):
        seen = []
        wav, pcm16, d = separate(mono_model, p, seen, monkeypatch)
        ref = p if p.dim() == 1 else p[0].contiguous()
        mag = ops.stft_batch([ref.to(dev)], want_complex=False)[0]
        assert len(seen) == 1 and seen[0] is d["mag"] and "net_rows" not in d and torch.equal(bits(d["mag"]), bits(mag))
        assert torch.equal(bits(d["stitched"]), bits(stitched_from(mono_model, mag, mag)))
        if p.dim() == 1:
            ref_wav, ref_pcm = ops.mask_istft_frames(d["mixc"], d["stitched"], 2, want_pcm=True, want_float=True)
        else:
            _, Z, _ = ops.mvdr(d["Y"], d["stitched"], 2, LB, R, 0, LOADING)
            ref_wav, ref_pcm = ops.mask_istft_streams(Z, None, 2, want_pcm=True, want_float=True)
        assert torch.equal(bits(wav), bits(ref_wav)) and torch.equal(pcm16, ref_pcm)
        monkeypatch.undo()
        monkeypatch.setattr(_lib, "call", spy)
    assert "sk_ipd_rows" not in calls and "sk_stft_ipd" not in calls and "sk_stitch" in calls
