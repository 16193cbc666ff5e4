"""Reverberant dynamic mixing: a source convolved with a room impulse response (RIR) before the mixture is made.

The definition, for a signal x of n samples, a RIR h of L taps and a delay d, 0 <= d < L:

    y[i] = sum_{k=0}^{L-1} h[k] x[i + d - k],   0 <= i < n,   x = 0 outside [0, n)

which is np.convolve(x, h)[d : d + n]: the output keeps the source's length, and with d = direct_delay(h), the index of the
direct path, it stays time-aligned with the dry signal.  x are float samples, or int16 PCM scaled by 1/32768.

Below: `convolve`, that definition in fp64; `convolve_partitioned_f32`, the numpy float32 restatement of what sk_fir_convolve
(csrc/fir.hip) computes -- the documentation of its arithmetic and the yardstick of the GPU test's tolerance --; synthetic RIRs
and the reading of measured ones.  numpy only: the loader's worker processes import this, not torch.
"""
import numpy as np

from .mixing import as_float

P = 256                      # taps per partition = output samples per block; transforms are 2 P = 512 points
MAX_TAPS = 8192              # 1 s at 8 kHz, 32 partitions


def _check(x, h, delay):
    x, h = np.asarray(x), np.asarray(h)
    if x.ndim != 1 or h.ndim != 1 or x.size < 1 or h.size < 1:
        raise ValueError("reverb: a signal and a RIR of at least one sample each (1-D) expected")
    if not 0 <= int(delay) < h.size:
        raise ValueError("reverb: delay = %d outside [0, %d taps)" % (int(delay), h.size))
    return x, h, int(delay)


def convolve(x, h, delay=0):
    """The definition in fp64: np.convolve(x, h)[delay : delay + n]."""
    x, h, d = _check(x, h, delay)
    return np.convolve(as_float(x), np.asarray(h, dtype=np.float64))[d:d + x.size]


def direct_delay(h):
    """The index of the direct path: the first index of max |h|."""
    return int(np.argmax(np.abs(np.asarray(h))))


def convolve_partitioned_f32(x, h, delay, drop_last_partition=False, late_history=False, delay_error=0):
    """sk_fir_convolve's arithmetic in float32: uniformly partitioned overlap-save with the block grid on the FULL convolution's
    index.  K = ceil(L / 256) partitions, H_k = rfft512(taps [256 k, 256 k + 256) then 256 zeros); X_b = rfft512(x[256 (b - 1),
    256 (b + 1))), zero outside the signal; for every block b = d // 256 .. (d + n - 1) // 256
        Y_b = sum_k H_k X_{b-k},  k ascending over 0 .. min(K - 1, b)   (complex64; blocks that lie past the signal are zero)
    and full[256 b, 256 b + 256) = the last 256 samples of irfft512(Y_b); y[i] = full[d + i].  The transforms are scipy.fft's
    on float32 arrays (pocketfft keeps complex64); the kernel's are a 16 x 16 radix-4 factorisation with fused multiply-adds,
    which rounds differently: see tests/test_gpu_reverb.py for the bound that follows from this function's own error.

    The three keyword switches each put ONE fault into the algorithm (the last partition left out; the block history started
    one block late, X_0 taken as zero; the delay off by delay_error).  tests/test_reverb.py uses them to show that its shapes
    would catch such a fault; nothing else sets them."""
    import scipy.fft
    x, h, d = _check(x, h, delay)
    n, L = x.size, h.size
    xf = (x.astype(np.float32) * np.float32(1.0 / 32768.0)) if x.dtype == np.int16 else x.astype(np.float32)
    hf = h.astype(np.float32)
    d = d + int(delay_error)
    K = -(-L // P)
    b0, b1 = d // P, (d + n - 1) // P
    # x[-256 .. 256 (b1 + 1)): block b's 512 samples start at 256 b of this padded copy
    pad = np.zeros(P * (b1 + 2), dtype=np.float32)
    m = min(n, pad.size - P)
    pad[P:P + m] = xf[:m]
    hp = np.zeros(K * P, dtype=np.float32)
    hp[:L] = hf
    H = [scipy.fft.rfft(np.concatenate([hp[P * k:P * (k + 1)], np.zeros(P, dtype=np.float32)])) for k in range(K)]
    X = {}

    def spectrum(b):
        if b not in X:
            X[b] = scipy.fft.rfft(pad[P * b:P * b + 2 * P])
            assert X[b].dtype == np.complex64
        return X[b]
    y = np.zeros(n, dtype=np.float32)
    for b in range(max(b0, 0), b1 + 1):
        Y = np.zeros(P + 1, dtype=np.complex64)
        for k in range(0, min(K - 1, b) + 1):
            if drop_last_partition and k == K - 1:
                continue
            if late_history and b - k == 0:
                continue
            Y = Y + H[k] * spectrum(b - k)
        blk = scipy.fft.irfft(Y, 2 * P)[P:]
        assert blk.dtype == np.float32
        lo = P * b - d                                   # y index of the block's first sample
        a, e = max(lo, 0), min(lo + P, n)
        if e > a:
            y[a:e] = blk[a - lo:e - lo]
    return y


def synthetic_rir(rng, t60_s, rate, drr_db):
    """A float32 RIR of min(round(t60_s rate), MAX_TAPS) taps: a unit direct path at tap 0 and, from tap 1 on, Gaussian noise
    under the envelope 10^(-3 k / (t60_s rate)) (-60 dB at t60), scaled so that the direct-to-reverberant energy ratio is drr_db.
    A function of rng (a numpy Generator) and the arguments alone."""
    L = min(int(round(float(t60_s) * float(rate))), MAX_TAPS)
    if L < 1:
        raise ValueError("synthetic_rir: t60 = %r s at %r Hz leaves no tap" % (t60_s, rate))
    h = np.zeros(L, dtype=np.float64)
    h[0] = 1.0
    if L > 1:
        k = np.arange(1, L, dtype=np.float64)
        tail = rng.standard_normal(L - 1) * 10.0 ** (-3.0 * k / (float(t60_s) * float(rate)))
        e = float(np.sum(tail * tail))
        if e > 0.0:
            h[1:] = tail * np.sqrt(10.0 ** (-float(drr_db) / 10.0) / e)
    return h.astype(np.float32)


def load_rir(path, rate):
    """A measured RIR -> (float32 taps, truncated?).  `.wav`: mono 16-bit PCM at exactly `rate` Hz, scaled by 1/32768 (RIRs
    are not resampled: another rate is an error); `.npy`: a 1-D float array, taken to be at `rate`.  More than MAX_TAPS taps are
    cut to MAX_TAPS; an empty or all-zero RIR is an error."""
    path = str(path)
    if path.lower().endswith(".npy"):
        h = np.load(path, allow_pickle=False)
        if h.ndim != 1 or not np.issubdtype(h.dtype, np.floating):
            raise ValueError("%s: a RIR in .npy form is a 1-D float array (got %s of shape %s)" % (path, h.dtype, h.shape))
        h = h.astype(np.float32)
    elif path.lower().endswith(".wav"):
        import wave
        with wave.open(path, "rb") as w:
            if w.getnchannels() != 1 or w.getsampwidth() != 2:
                raise ValueError("%s: only mono 16-bit PCM wav is supported for a RIR" % path)
            if w.getframerate() != int(rate):
                raise ValueError("%s is sampled at %d Hz, the run works at %d Hz: RIRs are not resampled" % (path, w.getframerate(), int(rate)))
            h = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.float32) * np.float32(1.0 / 32768.0)
    else:
        raise ValueError("%s: a RIR is a .wav or a .npy file" % path)
    if h.size == 0 or not np.any(h) or not np.all(np.isfinite(h)):
        raise ValueError("%s: an empty, all-zero or non-finite RIR" % path)
    return np.ascontiguousarray(h[:MAX_TAPS]), h.size > MAX_TAPS


def read_rir_scp(path, rate):
    """Lines of `<rir-id> <path>` -> ([float32 taps], number truncated to MAX_TAPS)."""
    rirs, cut = [], 0
    for line in open(path):
        if not line.strip():
            continue
        _, f = line.rstrip("\n").split(" ", 1)
        h, was_cut = load_rir(f.strip(), rate)
        rirs.append(h)
        cut += int(was_cut)
    if not rirs:
        raise ValueError("%s lists no RIR" % path)
    return rirs, cut
