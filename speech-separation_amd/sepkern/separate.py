"""Separating a recording of any length: windowed inference with stitched masks, PCM in and PCM out on the device.

The network is trained on chunks of a few hundred frames from a random initial state; a recording of minutes or hours is
therefore cut into overlapping windows of that length, which run through the network as uniform batches (the shape the
recurrence kernels are tuned for), and sk_stitch (sepkern/stitch.py) lines the windows' output orders up and cross-fades them.
One STFT of the WHOLE recording feeds every window (a per-window STFT would reflect-pad at every window edge), and one
mask-apply + iSTFT of the stitched masks gives the waveforms.  All window masks stay resident until they are stitched:
stitch.memory_bytes(T, W, Hn, S) = K W S 257 4 bytes, about 0.9 GB for an hour at S = 2.
"""
import numpy as np
import torch

from . import cacgmm as cg
from . import mvdr as mv
from . import ops
from . import stitch as st
from . import wpd as wd
from . import wpe as wp
from ._lib import SepkernError
from .packing import Packing

WORKING_RATE = 8000      # Hz: the rate the recipe's data (wav8k) and therefore its models work at


def window_masks(model, mag, window_frames, hop_frames, batch_windows):
    """The network on every window of mag (T, 257) -- or of an IPD model's wider input rows (T, ld), ops.ipd_rows --: -> [(tensor, offset, row stride)] per window, the descriptors ops.stitch
    takes.  Full windows go in uniform batches of up to batch_windows (window j of a batch of B is offset j * ld, stride B * ld
    of its packed output); a short last window runs as a batch of its own."""
    T, dev = int(mag.shape[0]), mag.device
    starts = st.window_starts(T, window_frames, hop_frames)
    lens = [min(window_frames, T - s0) for s0 in starts]
    full = [k for k in range(len(starts)) if lens[k] == window_frames]
    batches = [full[i:i + batch_windows] for i in range(0, len(full), batch_windows)]
    if len(full) < len(starts):
        batches.append([len(starts) - 1])
    windows = [None] * len(starts)
    for ks in batches:
        B, n = len(ks), lens[ks[0]]
        pk = Packing(np.full(B, n, dtype=np.int32), dev)
        # row (t, j) of the packed batch = frame starts[ks[j]] + t of the recording (an index copy: plumbing, no arithmetic)
        idx = (torch.arange(n, device=dev).unsqueeze(1) + torch.tensor([starts[k] for k in ks], device=dev).unsqueeze(0)).reshape(-1)
        x = pk.rows(mag.shape[1])
        torch.index_select(mag, 0, idx, out=x[:pk.R])
        model.hidden = model.init_hidden(B)
        # (masks_packed: the network's own tensor for a uPIT model; the k-means masks of a deep-clustering model's embeddings,
        # a fresh contiguous tensor -- its stride makes the descriptors either way)
        mask = model.masks_packed(x, pk)
        ld = int(mask.stride(0))
        for j, k in enumerate(ks):
            windows[k] = (mask, j * ld, B * ld)
    return windows


def separate_recording(model, pcm, sample_rate, window_frames=400, hop_frames=200, batch_windows=32, ramp=None,
                       working_rate=WORKING_RATE, want_float=True, want_pcm=False, return_details=False, ref_channel=0,
                       mvdr_block_frames=200, mvdr_context_blocks=1, mvdr_loading=1e-3, mvdr_postmask=False, mvdr=True,
                       wpe=False, wpe_taps=10, wpe_delay=3, wpe_iterations=3, wpe_block_frames=600, wpe_context_frames=0,
                       wpe_loading=1e-3, cacgmm=False, cacgmm_iterations=5, cacgmm_block_frames=200, cacgmm_context_frames=200,
                       cacgmm_loading=1e-3, wpd=False, wpd_taps=5, wpd_delay=3, wpd_iterations=2, wpd_block_frames=600,
                       wpd_context_frames=0, wpd_loading=1e-3, wpd_floor=1e-6, wpd_postmask=False):
    """model: a uPIT SepDNN on the GPU; pcm: 1-D tensor of the recording's samples, int16 PCM or float32, at sample_rate Hz
    (moved to the model's device if it is not there; resampled on the device when sample_rate is not working_rate, the rate the
    model was trained at).  -> (wav (S, L) float32 or None, pcm16 (S, L) int16 or None) at working_rate,
    L = 128 (T - 1) samples for the T = 1 + n // 128 frames of the n samples at working_rate; the int16 conversion is sk_mask_istft's
    (the reference's: truncated, wrapping).  ramp: (window_frames - hop_frames) float32 weights of the later window, default
    (o + 1) / (O + 1).  return_details: a third value, dict(masks = the window descriptors, stitched (T, S*257), perms, cost,
    mag, mixc).  Nothing synchronises with the host between PCM in and PCM out.
    pcm of shape (C, n), 2 <= C <= 8: the C microphones of an array, sample-aligned.  The network, the windows and sk_stitch see
    channel ref_channel only (its bits are those of the 1-D call on that channel); the stitched masks then steer one MVDR
    beamformer per stream and block of mvdr_block_frames frames over all channels (sk_mvdr, sepkern/mvdr.py: a context of
    mvdr_context_blocks blocks on either side, diagonal loading mvdr_loading), and the beamformed spectra are inverted --
    multiplied by the masks once more with mvdr_postmask.  The defaults (3.2 s blocks, 9.6 s of context) follow the segment
    lengths of the CSS literature; they are not tuned.  The details gain Y (C, T, 257), weights and Z.
    wpe: the spectra are dereverberated first (sk_wpe, sepkern/wpe.py: wpe_taps frames of every channel's past from wpe_delay
    frames back, wpe_iterations iterations, one filter per block of wpe_block_frames frames estimated on the block and
    wpe_context_frames on either side, loading wpe_loading).  A 1-D pcm becomes a (1, T, 257) spectrum; X = sk_wpe's output
    replaces Y everywhere downstream: the network sees |X[ref_channel]| (sk_wpe's mag_out), the masks are applied to
    X[ref_channel] (mixc), MVDR runs on X.  The details gain X and keep the untouched Y.  The defaults (10 taps, a delay of 3,
    3 iterations, 9.6 s blocks) are the literature's; they are not tuned.  mvdr=False with wpe and a (C, n) pcm dereverberates
    with all channels and masks the reference channel instead of beamforming.  Without wpe the calls are those of before.
    cacgmm: between the network and the beamformer the stitched masks are re-estimated from all channels (sk_cacgmm,
    sepkern/cacgmm.py: a cACGMM per block of cacgmm_block_frames frames and bin, fitted in cacgmm_iterations iterations on the
    block and cacgmm_context_frames on either side with the network's masks as its class prior, loading cacgmm_loading), on X
    with wpe.  It needs a (C, n) pcm and mvdr: the refined masks steer sk_mvdr and nothing else -- mvdr_postmask, the details'
    stitched and everything upstream keep the network's masks.  The details gain cacgmm_masks.  The defaults (5 iterations,
    3.2 s blocks with 3.2 s of context on either side) are untuned.  Without cacgmm the calls and their bits are those of before.
    wpd: one WPD convolutional beamformer per stream takes the beamformer's place (sk_wpd, sepkern/wpd.py: the present frame and
    wpd_taps frames of every channel's past from wpd_delay frames back, wpd_iterations iterations, one filter per block of
    wpd_block_frames frames estimated on the block and wpd_context_frames on either side, loading wpd_loading, power floor
    wpd_floor).  It needs a (C, n) pcm and mvdr=False: wpd together with mvdr is refused.  The stitched masks steer it, or
    sk_cacgmm's with cacgmm, which then needs mvdr or wpd.  With wpe the network and sk_cacgmm see X as above, but sk_wpd runs on
    the untouched Y: it is the joint solution on the observation.  Its spectra are inverted -- multiplied by the stitched masks
    once more with wpd_postmask.  The details gain Y, Z and wpd_weights.  The defaults (5 taps, a delay of 3, 2 iterations,
    9.6 s blocks, a floor of 1e-6) are the literature's; they are not tuned.  Without wpd the calls and their bits are those of
    before."""
    if not hasattr(model, "forward_packed"):
        raise SepkernError("separate_recording needs a model with forward_packed (the uPIT arch)")
    ipd_chans = [int(c) for c in getattr(model, "ipd_channels", ())]
    st.check_geometry(1, window_frames, hop_frames)
    if batch_windows < 1:
        raise ValueError("separate_recording: batch_windows = %d, at least 1 expected" % batch_windows)
    dev = model.lin.weight.device
    pcm = torch.as_tensor(pcm)
    if pcm.dim() not in (1, 2) or pcm.dtype not in (torch.int16, torch.float32):
        raise SepkernError("separate_recording: pcm must be a 1-D, or for an array a (C, n), int16 or float32 tensor")
    if wpd:
        if mvdr:
            raise ValueError("separate_recording: wpd takes the beamformer's place; pass mvdr=False with it")
        if pcm.dim() != 2:
            raise ValueError("separate_recording: wpd needs a (C, n) pcm")
        wd.check_arguments(int(pcm.shape[0]), int(model.num_spk), 1, int(wpd_taps), int(wpd_delay), int(wpd_iterations),
                           int(wpd_block_frames), int(wpd_context_frames), int(ref_channel), float(wpd_loading), float(wpd_floor))
    if cacgmm:
        if pcm.dim() != 2 or not (mvdr or wpd):
            raise ValueError("separate_recording: cacgmm needs a (C, n) pcm and mvdr or wpd")
        cg.check_arguments(int(pcm.shape[0]), int(model.num_spk), 1, int(cacgmm_iterations), int(cacgmm_block_frames),
                           int(cacgmm_context_frames), float(cacgmm_loading))
    if ipd_chans:
        if pcm.dim() != 2:
            raise ValueError("separate_recording: the model has ipd_channels = %s and needs a (C, n) pcm, the array it was trained "
                             "on" % ",".join(str(c) for c in ipd_chans))
        if int(ref_channel) != int(model.ipd_ref):
            raise ValueError("separate_recording: ref_channel = %d, but the model was trained with ipd_ref = %d: its masks belong "
                             "to that channel" % (int(ref_channel), int(model.ipd_ref)))
        if max(ipd_chans + [int(model.ipd_ref)]) >= int(pcm.shape[0]):
            raise ValueError("separate_recording: the recording has %d channels, the model's ipd_ref = %d and ipd_channels = %s "
                             "need channel %d" % (int(pcm.shape[0]), int(model.ipd_ref), ",".join(str(c) for c in ipd_chans),
                                                  max(ipd_chans + [int(model.ipd_ref)])))
    pcm = pcm.to(dev, non_blocking=True)
    if wpe:
        wp.check_arguments(int(pcm.shape[0]) if pcm.dim() == 2 else 1, 1, int(wpe_taps), int(wpe_delay), int(wpe_iterations),
                           int(wpe_block_frames), int(wpe_context_frames), int(ref_channel) if pcm.dim() == 2 else 0, float(wpe_loading))
    Y = None
    if pcm.dim() == 2:
        C, n = int(pcm.shape[0]), int(pcm.shape[1])
        if mvdr:
            mv.check_arguments(C, int(model.num_spk), 1, int(mvdr_block_frames), int(mvdr_context_blocks), int(ref_channel), float(mvdr_loading))
        elif not (wpe or wpd or ipd_chans):
            raise ValueError("separate_recording: a (C, n) pcm needs mvdr or wpe")
        flat = pcm.contiguous().view(-1)
        if int(sample_rate) != int(working_rate):           # all channels in one call
            if flat.dtype == torch.int16:
                flat, outs = ops.pcm_to_rate(flat, [n] * C, [int(sample_rate)] * C, int(working_rate))
            else:
                flat, outs = ops.resample_batch(flat, [n] * C, int(sample_rate), int(working_rate))
            n = int(outs[0])
        Tn = 1 + n // 128
        Y = torch.empty(C, Tn, 257, dtype=torch.complex64, device=dev)
        ops.stft_batch(flat, want_complex=True, out=Y.view(-1), out_offs=[c * Tn * 257 for c in range(C)], stride_t=[257] * C,
                       stride_f=[1] * C, lengths=[n] * C)
        pcm = flat[int(ref_channel) * n:(int(ref_channel) + 1) * n]
        mixc = Y[int(ref_channel)]
    else:
        if int(sample_rate) != int(working_rate):
            if pcm.dtype == torch.int16:
                pcm, _ = ops.pcm_to_rate(pcm, [pcm.numel()], [int(sample_rate)], int(working_rate))
            else:
                pcm, _ = ops.resample_batch(pcm.contiguous(), [pcm.numel()], int(sample_rate), int(working_rate))
        mixc = ops.stft_batch([pcm], want_complex=True)[0]          # (T, 257) complex64 rows of the whole recording
    X = None
    if wpe:
        ref = int(ref_channel) if Y is not None else 0
        Yw = Y if Y is not None else mixc.unsqueeze(0)
        X, mag, _ = ops.wpe(Yw, wpe_taps, wpe_delay, wpe_iterations, wpe_block_frames, wpe_context_frames, wpe_loading, ref=ref,
                            want_mag=True)
        mixc = X[ref]
    else:
        mag = ops.stft_batch([pcm], want_complex=False)[0]          # (T, 257): the bits the network was trained on
    T, S = int(mag.shape[0]), int(model.num_spk)
    O = window_frames - hop_frames
    ramp = torch.from_numpy(st.default_ramp(O)).to(dev) if ramp is None else torch.as_tensor(ramp, dtype=torch.float32).to(dev).contiguous()
    was_training = model.training
    model.eval()
    # an IPD model reads [ |ref| | cos, sin of every listed channel against ref ] (sepkern/ipd.py) of the spectra the masks will be
    # applied to -- X after wpe --, the magnitude columns being `mag` itself; stitching and everything behind it keep reading mag
    net_rows = ops.ipd_rows(Y if X is None else X, int(ref_channel), ipd_chans, mag) if ipd_chans else mag
    try:
        with torch.no_grad():
            windows = window_masks(model, net_rows, window_frames, hop_frames, batch_windows)
    finally:
        model.train(was_training)
    stitched, perms, cost = ops.stitch(mag, windows, T, window_frames, hop_frames, S, ramp)
    details = dict(masks=windows, stitched=stitched, perms=perms, cost=cost, mag=mag, mixc=mixc)
    if ipd_chans:
        details.update(net_rows=net_rows)
    if X is not None:
        details.update(X=X, Y=Yw)
    if wpd:
        steer = stitched
        if cacgmm:
            steer, _ = ops.cacgmm(Y if X is None else X, stitched, S, cacgmm_iterations, cacgmm_block_frames, cacgmm_context_frames,
                                  cacgmm_loading)
            details.update(cacgmm_masks=steer)
        Z, weights = ops.wpd(Y, steer, S, wpd_taps, wpd_delay, wpd_iterations, wpd_block_frames, wpd_context_frames, wpd_loading,
                             wpd_floor, ref=ref_channel, want_W=True)
        wav, pcm16 = ops.mask_istft_streams(Z, stitched if wpd_postmask else None, S, want_pcm=want_pcm, want_float=want_float)
        details.update(Y=Y, Z=Z, wpd_weights=weights)
    elif Y is None or not mvdr:
        wav, pcm16 = ops.mask_istft_frames(mixc, stitched, S, want_pcm=want_pcm, want_float=want_float)
    else:
        steer = stitched
        if cacgmm:
            steer, _ = ops.cacgmm(Y if X is None else X, stitched, S, cacgmm_iterations, cacgmm_block_frames, cacgmm_context_frames,
                                  cacgmm_loading)
            details.update(cacgmm_masks=steer)
        weights, Z, _ = ops.mvdr(Y if X is None else X, steer, S, mvdr_block_frames, mvdr_context_blocks, ref_channel, mvdr_loading)
        wav, pcm16 = ops.mask_istft_streams(Z, stitched if mvdr_postmask else None, S, want_pcm=want_pcm, want_float=want_float)
        details.update(Y=Y, weights=weights, Z=Z)
    if return_details:
        return wav, pcm16, details
    return wav, pcm16
