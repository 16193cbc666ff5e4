"""The eleven wrappers of sepkern/ops.py that take a signal batch (ONE flat 1-D tensor of samples, nested
lists of offsets, samples per utterance) refuse the same table of bad batches before anything is launched, and take the good
batch of the same shapes: B = 2 signals of 300 and 257 samples per list, the last one ending with its buffer.

What the table leaves out, because the wrapper has no such argument: resample_batch, pcm_to_rate and stft_batch(lengths=) take
no offsets -- lengths that end one sample past the buffer stand in for them; fir_convolve, resample_batch, pcm_to_rate and
add_noise have no `out`; stft_batch writes a caller's `out` through the caller's offsets and strides and cannot know its
size."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

NS = [300, 257]
TOTAL = sum(NS)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch.device("cuda", 0)


def _offs(K):
    return [[q * TOTAL, q * TOTAL + NS[0]] for q in range(K)]


def _pcm(K, dev, dtype=torch.int16):
    g = torch.Generator().manual_seed(K)
    x = torch.randint(-8000, 8000, (K * TOTAL,), generator=g, dtype=torch.int16)
    return (x if dtype == torch.int16 else x.to(torch.float32) / 32768.0).to(dev)


def _spec(name, dev):
    """-> (fn, good keyword arguments, the sample tensors' names, the lengths' name, the offset lists' names, (out's name, its
    size) or None)."""
    from sepkern import ipd, ops, resample
    outs = [resample.out_len(n, 16000, 8000) for n in NS]
    frames = sum(1 + n // 128 for n in NS)
    return {
        "dynamic_mix": (ops.dynamic_mix, dict(flat=_pcm(2, dev), src_offs=_offs(2), nsamp=NS, amp=[[1.0, 1.0], [0.5, 0.5]], peak=[0.9, 0.8]),
                        ["flat"], "nsamp", ["src_offs"], ("out", 3 * TOTAL)),
        "mix_channels": (ops.mix_channels, dict(flat=_pcm(2, dev, torch.float32), chan_offs=[[o] for o in _offs(2)], nsamp=NS,
                                                gains=torch.ones(2, 2, device=dev)), ["flat"], "nsamp", ["chan_offs"], ("out", TOTAL)),
        "diffuse_noise": (ops.diffuse_noise, dict(flat=_pcm(2, dev), chan_offs=_offs(2), nsamp=NS, L=torch.ones(2, 257, 3, device=dev)),
                          ["flat"], "nsamp", ["chan_offs"], ("out", 2 * TOTAL)),
        "add_noise": (ops.add_noise, dict(sig=_pcm(1, dev, torch.float32), sig_offs=_offs(1), noise=_pcm(1, dev), noise_offs=_offs(1),
                                          nsamp=NS, amp=[1.0, 0.5]), ["sig", "noise"], "nsamp", ["sig_offs", "noise_offs"], None),
        "fir_convolve": (ops.fir_convolve, dict(flat=_pcm(1, dev), in_offs=_offs(1)[0], ns=NS, rir_flat=_pcm(1, dev, torch.float32)[:40].clone(),
                                                rir_offs=[0, 20], taps=[20, 20], delay=[0, 3]), ["flat", "rir_flat"], "ns", ["in_offs", "rir_offs"], None),
        "resample_into": (ops.resample_into, dict(src=_pcm(1, dev), in_offs=_offs(1)[0], n_in=NS, out=torch.zeros(sum(outs), device=dev),
                                                  out_offs=[0, outs[0]], n_out=outs, sr_in=16000, sr_out=8000),
                          ["src"], "n_in", ["in_offs", "out_offs"], ("out", sum(outs))),
        "resample_batch": (ops.resample_batch, dict(flat=_pcm(1, dev), lengths=NS, sr_in=16000, sr_out=8000), ["flat"], "lengths", [], None),
        "pcm_to_rate": (ops.pcm_to_rate, dict(flat=_pcm(1, dev), lengths=NS, rates=[16000, 16000], target=8000), ["flat"], "lengths", [], None),
        "stft_batch": (ops.stft_batch, dict(wavs=_pcm(1, dev), lengths=NS), ["wavs"], "lengths", [], None),
        "stft_psa": (ops.stft_psa, dict(flat=_pcm(2, dev), sig_offs=_offs(2), nsamp=NS, S=1), ["flat"], "nsamp", ["sig_offs"],
                     ("out", (torch.zeros(frames, 257, device=dev), torch.zeros(1, frames, 257, device=dev)))),
        "stft_ipd": (ops.stft_ipd, dict(flat=_pcm(2, dev), sig_offs=_offs(2), nsamp=NS), ["flat"], "nsamp", ["sig_offs"],
                     ("out", (torch.zeros(frames, ipd.padded_dim(1), device=dev), torch.zeros(frames, 257, device=dev)))),
    }[name]


def _leaf_list(offs, last):
    """The first or the last innermost list of a nested list of offsets."""
    while isinstance(offs[0], list):
        offs = offs[-1 if last else 0]
    return offs


def _bad_calls(good, samples, lengths, offsets, out):
    for k in samples:
        x = good[k]
        yield "2-D %s" % k, {k: x.view(1, -1)}
        yield "strided %s" % k, {k: torch.stack([x, x], 1)[:, 0]}
        yield "float64 %s" % k, {k: x.double()}
    yield "no mixtures", {lengths: []}
    for k in offsets:
        short, neg, past = copy.deepcopy(good[k]), copy.deepcopy(good[k]), copy.deepcopy(good[k])
        del _leaf_list(short, True)[-1]
        _leaf_list(neg, False)[0] = -1
        _leaf_list(past, True)[-1] += 1
        yield "%s short by one" % k, {k: short}
        yield "a negative offset in %s" % k, {k: neg}
        yield "%s one sample past the buffer" % k, {k: past}
    if not offsets:
        yield "lengths one sample past the buffer", {lengths: [NS[0], NS[1] + 1]}
    if out is not None and isinstance(out[1], int):
        like = good["src" if "src" in good else "flat"]
        yield "out one element short", {out[0]: torch.zeros(out[1] - 1, device=like.device)}
        yield "float64 out", {out[0]: torch.zeros(out[1], dtype=torch.float64, device=like.device)}
    elif out is not None:
        first, second = out[1]
        yield "out one row short", {out[0]: (first[:-1], second)}
        yield "float64 out", {out[0]: (first.double(), second)}


@pytest.mark.parametrize("name", ["dynamic_mix", "mix_channels", "diffuse_noise", "add_noise", "fir_convolve", "resample_into",
                                  "resample_batch", "pcm_to_rate", "stft_batch", "stft_psa", "stft_ipd"])
def test_a_bad_signal_batch_is_refused_before_any_launch_and_the_good_one_runs(name, dev, monkeypatch):
    from sepkern import _lib
    fn, good, samples, lengths, offsets, out = _spec(name, dev)
    entry = []
    real_call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda entry_name, *a: (entry.append(entry_name), real_call(entry_name, *a))[1])
    n = 0
    for what, bad in _bad_calls(good, samples, lengths, offsets, out):
        with pytest.raises(_lib.SepkernError) as e:
            fn(**dict(good, **bad))
        assert not entry, (what, entry)
        assert "code " not in str(e.value), (what, str(e.value))                     # the wrapper's own refusal, not the C side's
        n += 1
    assert n >= 5
    fn(**good)
    torch.cuda.synchronize()
    assert entry and all(c.startswith("sk_") for c in entry), entry
