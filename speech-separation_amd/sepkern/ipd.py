"""Inter-channel phase differences (IPDs) as network input: what lets the network tell two speakers apart by direction when
their spectra look alike (Yoshioka et al. 2018, "Multi-microphone neural speech separation for far-field multi-talker speech
recognition"; Wang, Le Roux, Hershey 2018, "Multi-channel deep clustering").

Y_r is the reference channel's STFT and Y_c a listed channel's, both as sk_stft defines them (oracle/stft.py).  Per frame and bin

    cos_c = Re(Y_c conj Y_r) / (|Y_c| |Y_r|)  =  cos(theta_c - theta_r)
    sin_c = Im(Y_c conj Y_r) / (|Y_c| |Y_r|)  =  sin(theta_c - theta_r)

both 0 where the fp32 |Y_c|^2 or |Y_r|^2 is below 2^-100.  A feature row of a model with P listed channels is

    [ |Y_r| (257) | cos_1 (257) | sin_1 (257) | ... | cos_P | sin_P ],       width 257 (1 + 2P),  P in 1..7

The conf keys of archs/uPIT.py: ipd_channels=1,2,3 (a non-empty list makes it an IPD model; the channels are distinct and none
is the reference) and ipd_ref=0 (the reference channel: the one whose magnitude the network sees, the masks are applied to and
the sources are scored on).  Without ipd_channels nothing changes anywhere.

The fp32 form the kernels of csrc/ipd.hip compute (ipd_feature, shared by sk_stft_ipd and sk_ipd_rows), a = Re, b = Im:
    num_cos = fma(a_c, a_r, b_c * b_r)          num_sin = fma(b_c, a_r, -(a_c * b_r))
    |Y|^2   = fma(a, a, b * b)                  feature = (num * rsq(|Y_c|^2)) * rsq(|Y_r|^2)
two reciprocal square roots, never one of the product: 2^-100 x 2^-100 underflows fp32.

Below: the numpy fp64 restatement -- the documentation of that arithmetic, and what tests/test_ipd.py and
tests/test_gpu_ipd.py pin the kernels to.
"""
import numpy as np

F = 257
TINY = 2.0 ** -100           # |Y|^2 below this (in the kernels: the fp32 value) -> both features 0
MAX_PAIRS = 7                # the fused kernel walks at most 8 signals per utterance: the reference and 7 more


def parse_ref(value):
    """The conf key `ipd_ref`: the reference channel, an integer >= 0 (default 0)."""
    try:
        ref = int(str(value).strip())
    except ValueError:
        raise ValueError("conf key ipd_ref: %r is not a channel number" % (value,))
    if ref < 0:
        raise ValueError("conf key ipd_ref: channel %d is negative" % ref)
    return ref


def parse_channels(value, ref=0):
    """The conf key `ipd_channels`: '1,2,3' (or a sequence of integers) -> (1, 2, 3); None / '' -> (): not an IPD model.
    At most 7 channels, each >= 0, distinct, none of them the reference."""
    if value is None:
        return ()
    if isinstance(value, str):
        parts = [p.strip() for p in value.replace(";", ",").split(",")]
        if not any(parts):
            return ()
        if not all(parts):
            raise ValueError("conf key ipd_channels: %r holds an empty entry" % (value,))
    else:
        parts = list(value)
    try:
        chans = tuple(int(p) for p in parts)
    except (TypeError, ValueError):
        raise ValueError("conf key ipd_channels: %r is not a list of channel numbers such as 1,2,3" % (value,))
    if len(chans) > MAX_PAIRS:
        raise ValueError("conf key ipd_channels: %d channels, at most %d" % (len(chans), MAX_PAIRS))
    if any(c < 0 for c in chans):
        raise ValueError("conf key ipd_channels: a channel of %r is negative" % (chans,))
    if len(set(chans)) != len(chans):
        raise ValueError("conf key ipd_channels: a channel of %r is listed twice" % (chans,))
    if int(ref) in chans:
        raise ValueError("conf key ipd_channels: %r lists the reference channel ipd_ref = %d" % (chans, int(ref)))
    return chans


def in_dim(P):
    """Width of a feature row with P listed channels: 257 (1 + 2P)."""
    P = int(P)
    if not 1 <= P <= MAX_PAIRS:
        raise ValueError("ipd: %d listed channels, 1..%d expected" % (P, MAX_PAIRS))
    return F * (1 + 2 * P)


def padded_dim(P):
    """in_dim(P) rounded up to a multiple of 16: the row stride at which the engine takes the rows as they are."""
    return (in_dim(P) + 15) // 16 * 16


def columns(p):
    """Column ranges of listed channel number p (0-based position in ipd_channels): ((cos lo, cos hi), (sin lo, sin hi)),
    half-open.  The magnitude is columns [0, 257)."""
    p = int(p)
    if not 0 <= p < MAX_PAIRS:
        raise ValueError("ipd: pair %d outside 0..%d" % (p, MAX_PAIRS - 1))
    lo = F * (1 + 2 * p)
    return (lo, lo + F), (lo + F, lo + 2 * F)


def chan_key(c):
    """The batch key under which the loader ships channel c of the mixture."""
    return "chan%d" % int(c)


def chan_keys(keys):
    """The 'chan<c>' keys of a batch's key list, in its order."""
    return [k for k in keys if k.startswith("chan") and k[4:].isdigit()]


def signal_keys(keys):
    """'mix' and 'source<N>' of a batch's key list: what the STFT front ends of sepkern/data.py count as signals."""
    return [k for k in keys if k == "mix" or (k.startswith("source") and k[6:].isdigit())]


def ipd(Yc, Yr):
    """(cos, sin) float64 of the phase difference of Yc against Yr (complex spectra of one shape)."""
    Yc = np.asarray(Yc, dtype=np.complex128)
    Yr = np.asarray(Yr, dtype=np.complex128)
    c2 = Yc.real * Yc.real + Yc.imag * Yc.imag
    r2 = Yr.real * Yr.real + Yr.imag * Yr.imag
    live = (c2 >= TINY) & (r2 >= TINY)
    den = np.where(live, np.sqrt(c2) * np.sqrt(r2), 1.0)
    re = Yc.real * Yr.real + Yc.imag * Yr.imag
    im = Yc.imag * Yr.real - Yc.real * Yr.imag
    return np.where(live, re / den, 0.0), np.where(live, im / den, 0.0)


def feature_rows(Y, ref, channels):
    """Y (C, T, 257) complex spectra -> (T, 257 (1 + 2P)) float64 feature rows for the reference `ref` and the listed channels."""
    Y = np.asarray(Y, dtype=np.complex128)
    C = Y.shape[0]
    channels = [int(c) for c in channels]
    if not 0 <= int(ref) < C or any(not 0 <= c < C for c in channels):
        raise ValueError("ipd.feature_rows: the spectra hold %d channels; ref %d, channels %r" % (C, ref, channels))
    out = np.zeros((Y.shape[1], in_dim(len(channels))))
    out[:, :F] = np.abs(Y[int(ref)])
    for p, c in enumerate(channels):
        (c0, c1), (s0, s1) = columns(p)
        out[:, c0:c1], out[:, s0:s1] = ipd(Y[c], Y[int(ref)])
    return out
