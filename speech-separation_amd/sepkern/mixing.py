"""Dynamic mixing: a training mixture made afresh from single-speaker utterances, with levels the host drew.

The rule is WSJ0-2mix's (Hershey et al. 2016, the create_wav_2speakers recipe): every source is normalised to unit power and
scaled by the amplitude drawn for it, and then the mixture and all of its sources are scaled by ONE factor, so that the largest
magnitude among them reaches a target peak.  Two choices differ from that recipe and are made on purpose: a source's power is
the plain mean square of its samples, not the ITU-T P.56 active speech level (no voice-activity model; the levels then depend on
how much silence an utterance holds), and a silent source (mean square below 2^-40) gets gain 0 where a division would give
NaN or an enormous gain.

For one mixture of S sources x_s with n samples each, linear amplitudes amp_s (the host computes 10^(snr_s / 20): the device
never calls pow) and a target `peak`:

    1.  P_s = (1/n) sum_n x_s[n]^2
    2.  g_s = amp_s / sqrt(P_s),  0 where P_s < 2^-40
    3.  m   = max_n max(|sum_s g_s x_s[n]|, max_s |g_s x_s[n]|);   c = peak / m,  0 where m == 0;   G_s = g_s c
    4.  source s = G_s x_s,   mixture = sum_s G_s x_s
    5.  quantize: every output v becomes clip(rint(32768 v), -32768, 32767) / 32768 -- exactly what would have come back from
        a 16-bit wav file of it.

x_s are float samples, or int16 PCM scaled by 1/32768.

Below: the numpy fp64 restatement of what sk_dynamic_mix (csrc/mix.hip) computes -- the documentation of its arithmetic, and what
tests/test_dynamic_mix.py and tests/test_gpu_dynamic_mix.py pin the kernel to.  The kernel forms g_s and c in fp64 and rounds
each once to fp32, forms G_s = g_s c, the products G_s x_s and the maximum m in fp32, and the mixture as the chain
fmaf(G_s, x_s, acc) with s ascending from acc = 0.
"""
import numpy as np

SILENT = 2.0 ** -40          # a source whose mean square is below this gets gain 0
MAX_SOURCES = 4


def as_float(x):
    """Samples as float64: int16 PCM is scaled by 1/32768 (sk_stft's convention), anything else is taken as it is."""
    x = np.asarray(x)
    return x.astype(np.float64) / 32768.0 if x.dtype == np.int16 else x.astype(np.float64)


def quantize(v):
    """Step 5: onto the int16 grid, as float."""
    return np.clip(np.rint(np.asarray(v, dtype=np.float64) * 32768.0), -32768.0, 32767.0) / 32768.0


def gains(sources, amp, peak):
    """Steps 1-3 -> the S final gains G_s (float64)."""
    xs = [as_float(x) for x in sources]
    if not 1 <= len(xs) <= MAX_SOURCES or len(amp) != len(xs) or any(x.ndim != 1 or x.shape != xs[0].shape or x.size < 1 for x in xs):
        raise ValueError("mixing: 1..%d sources of one length >= 1, and one amplitude for each" % MAX_SOURCES)
    g = []
    for x, a in zip(xs, amp):
        P = float(np.mean(x * x))
        g.append(float(a) / np.sqrt(P) if P >= SILENT else 0.0)
    m = max(float(np.abs(sum(gs * x for gs, x in zip(g, xs))).max()), max(float(np.abs(gs * x).max()) for gs, x in zip(g, xs)))
    c = float(peak) / m if m > 0.0 else 0.0
    return np.array([gs * c for gs in g], dtype=np.float64)


def mix(sources, amp, peak, quantized=False):
    """-> (mixture, [source_s], G): float64 arrays of the sources' length and the S gains."""
    G = gains(sources, amp, peak)
    outs = [Gs * as_float(x) for Gs, x in zip(G, sources)]
    mixture = sum(outs)
    if quantized:
        mixture, outs = quantize(mixture), [quantize(o) for o in outs]
    return mixture, outs, G


def mix_channels(channels, G, quantized=False):
    """The other channels of an array mixture (sk_mix_channels): channels[p][s] = source s as microphone p picked it up, G the
    gains `mix` / `gains` found on the REFERENCE channel -> [sum_s G_s x_{s,p}] per channel p, float64.  Levels and the peak are
    defined on the reference channel: another channel may exceed the peak (and clip when quantized).  The kernel forms the sum
    as mix's chain, fmaf(G_s, x_s, acc) with s ascending from acc = 0, so that the reference channel's own signals give `mix`'s
    mixture bit for bit."""
    G = [float(g) for g in G]
    outs = []
    for chan in channels:
        xs = [as_float(x) for x in chan]
        if len(xs) != len(G) or not 1 <= len(xs) <= MAX_SOURCES or any(x.ndim != 1 or x.shape != xs[0].shape or x.size < 1 for x in xs):
            raise ValueError("mixing: every channel holds one signal per gain, 1..%d of one length >= 1" % MAX_SOURCES)
        y = sum(g * x for g, x in zip(G, xs))
        outs.append(quantize(y) if quantized else y)
    return outs


def snr_to_amp(snr_db):
    """The linear amplitude of a level in dB, 10^(snr / 20), as float32 (what the host hands the kernel)."""
    return np.float32(10.0 ** (float(snr_db) / 20.0))
