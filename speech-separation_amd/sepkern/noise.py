"""Noisy dynamic mixing: a noise recording added to a mono training mixture, and a spherically isotropic (diffuse) noise field
with the right inter-microphone coherence added to an array mixture, each at a drawn SNR.

The field follows Habets, Cohen & Gannot (2008): C mutually independent noise signals N_j are mixed per frequency so that the
result X has the coherence of a diffuse field between every pair of microphones.  With the library's own transform (n_fft = 512,
hop 128, periodic Hann), the microphones' distances d_ij, bins k = 0 .. 256 at f_k = k rate / 512 and c = 343 m/s:

    Gamma_k[i, j] = sinc(2 f_k d_ij / c),   sinc(x) = sin(pi x) / (pi x)
    L_k = the lower-triangular Cholesky factor of (1 - eps) Gamma_k + eps I,   eps = 2^-20
    X_i = sum_{j <= i} L_k[i, j] N_j            per frame and bin.

The loading is needed: at bin 0 Gamma is all ones, and for close microphones it is numerically rank-deficient at the low bins.
eps = 2^-20 keeps every fp64 pivot above 1e-3 for 8 microphones 2 cm apart at 8 kHz (the same line 1 cm apart at 16 kHz) and for
a 7-microphone circle of 4.25 cm radius at 8 kHz, and L_k rounded to float32 reproduces Gamma_k to 1.1e-6.

The transform pair of `diffuse`: x holds C signals of n >= 1 samples, zero outside [0, n); T = ceil(n / 128) + 3 frames, frame t
covering samples 128 (t - 3) .. 128 (t - 3) + 511; analysis and synthesis window are both the STFT's periodic Hann; synthesis is
the overlap-add of the windowed inverse transforms times 1 / 1.5, the exact sum of w^2 of this window at hop 128.  The output
is samples 0 .. n - 1, every one of them covered by exactly four frames: with L = I it is the input to 1e-15.

`add_noise` then sets the level: ONE gain for all channels, so that the field's coherence survives.

Below: `coherence`, `factors`, `diffuse` and `add_noise`, the definitions in fp64; `diffuse_f32`, the numpy float32 restatement
of what sk_diffuse_noise (csrc/noise.hip) computes -- the documentation of its arithmetic and the yardstick of the GPU test's
tolerance, as reverb.convolve_partitioned_f32 is for csrc/fir.hip.  numpy only: the loader's worker processes import this.
"""
import numpy as np

from .mixing import SILENT, as_float, quantize
from .room import C_SOUND, MAX_MICS, MIN_DIRECT

NFFT, HOP, NBIN = 512, 128, 257
EPS = 2.0 ** -20             # diagonal loading of the coherence matrix
TILE_HOPS = 13               # sk_diffuse_noise: hops a workgroup owns; it transforms the TILE_HOPS + 3 = 16 frames that touch them
OLA = 1.5                    # sum of w^2 over the four frames that cover a sample


def window():
    """The STFT's periodic Hann, fp64."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NFFT) / NFFT)


def _mics(mics):
    mics = np.asarray(mics, dtype=np.float64)
    if mics.ndim != 2 or mics.shape[1] != 3 or not 2 <= mics.shape[0] <= MAX_MICS:
        raise ValueError("noise: 2..%d microphones of 3 coordinates each expected" % MAX_MICS)
    d = np.sqrt(np.sum((mics[:, None, :] - mics[None, :, :]) ** 2, axis=-1))
    if not np.all(d[~np.eye(len(mics), dtype=bool)] >= MIN_DIRECT * (1.0 - 1e-9)):      # (a 1 cm grid is 1 cm apart, whatever its roundings)
        raise ValueError("noise: two microphones are less than %g m apart" % MIN_DIRECT)
    return d


def coherence(mics, rate):
    """Gamma (257, C, C) of a diffuse field at the microphones `mics` (C, 3) metres, fp64."""
    d = _mics(mics)
    f = np.arange(NBIN, dtype=np.float64) * float(rate) / NFFT
    return np.sinc(2.0 * f[:, None, None] * d[None, :, :] / C_SOUND)


def factors(mics, rate):
    """L (257, C, C), lower triangular: the Cholesky factors of (1 - eps) Gamma_k + eps I, fp64."""
    G = coherence(mics, rate)
    return np.linalg.cholesky((1.0 - EPS) * G + EPS * np.eye(G.shape[1])[None])


def tri(L):
    """L (257, C, C) -> the kernels' packing (257, C (C + 1) / 2): entry i (i + 1) / 2 + j holds L[i, j], j <= i."""
    L = np.asarray(L)
    i, j = np.tril_indices(L.shape[1])
    return np.ascontiguousarray(L[:, i, j])


def untri(Lt, C):
    """tri's inverse -> (257, C, C) with zeros above the diagonal."""
    Lt = np.asarray(Lt)
    L = np.zeros((Lt.shape[0], C, C), dtype=Lt.dtype)
    i, j = np.tril_indices(C)
    L[:, i, j] = Lt
    return L


def _check(x, L):
    x, L = np.asarray(x), np.asarray(L)
    if x.ndim != 2 or x.shape[1] < 1 or not 1 <= x.shape[0] <= MAX_MICS or L.shape != (NBIN, x.shape[0], x.shape[0]):
        raise ValueError("noise: C signals of one length >= 1 (C, n) and factors (257, C, C) expected")
    return x, L


def num_frames(n):
    return -(-int(n) // HOP) + 3


def diffuse(x, L):
    """The definition in fp64 -> (C, n)."""
    x, L = _check(x, L)
    C, n = x.shape
    T, w = num_frames(n), window()
    pad = np.zeros((C, HOP * (T - 1) + NFFT))
    pad[:, 3 * HOP:3 * HOP + n] = as_float(x)
    idx = HOP * np.arange(T)[:, None] + np.arange(NFFT)[None, :]
    N = np.fft.rfft(pad[:, idx] * w, axis=-1)                                  # (C, T, 257)
    X = np.einsum('kij,jtk->itk', np.tril(np.asarray(L, dtype=np.float64)), N)
    fr = np.fft.irfft(X, NFFT, axis=-1) * w
    out = np.zeros_like(pad)
    for t in range(T):
        out[:, HOP * t:HOP * t + NFFT] += fr[:, t]
    return out[:, 3 * HOP:3 * HOP + n] / OLA


def diffuse_f32(x, L, shift_grid=False, drop_last_frame=False, transpose_L=False, no_scale=False, drop_halo=False):
    """sk_diffuse_noise's arithmetic in float32 -> (C, n) float32.  Tile q owns hops 13 q .. 13 q + 12 and transforms the 16
    frames t = 13 q .. 13 q + 15 that touch them (frames past the last carry zeros); per frame and channel the windowed samples
    (float32 window times float32 sample) go through rfft512, the bins are mixed in place with i descending,
        X_i = fma(L[i, j], N_j, ...) with j ascending from L[i, 0] N_0        (float32 L, complex64 spectra)
    each X_i is inverted, windowed again, and a sample is the sum of its four frames in ascending frame order times fp32(2/3).
    The transforms are scipy.fft's on float32 arrays (pocketfft keeps complex64); the kernel's are the 16 x 16 radix-4
    factorisation of fft512.h with fused multiply-adds, which rounds differently: tests/test_gpu_noise.py bounds the kernel by
    this function's own error.  x: float samples or int16 PCM (scaled by 1/32768, exact).

    The keyword switches each put ONE fault into the algorithm (the frame grid shifted by one hop; the last frame of the signal
    dropped; L read transposed; the 1/1.5 left out; the last halo frame of every tile dropped).  tests/test_noise.py uses them
    to show that its cases would catch such a fault; nothing else sets them."""
    import scipy.fft
    x, L = _check(x, L)
    C, n = x.shape
    xf = (x.astype(np.float32) * np.float32(1.0 / 32768.0)) if x.dtype == np.int16 else x.astype(np.float32)
    Lf = np.tril(np.asarray(L)).astype(np.float32)
    if transpose_L:
        Lf = np.ascontiguousarray(np.transpose(Lf, (0, 2, 1)))
    w = window().astype(np.float32)
    T = num_frames(n)
    tiles = -(-n // (TILE_HOPS * HOP))
    lead = (3 + (1 if shift_grid else 0)) * HOP
    pad = np.zeros((C, lead + HOP * (TILE_HOPS * tiles + 3) + NFFT), dtype=np.float32)
    pad[:, 3 * HOP:3 * HOP + n] = xf
    y = np.zeros((C, n), dtype=np.float32)
    scale = np.float32(1.0) if no_scale else np.float32(2.0 / 3.0)
    for q in range(tiles):
        t0 = TILE_HOPS * q
        fr = np.zeros((C, 16, NFFT), dtype=np.float32)
        for g in range(16):
            t = t0 + g
            if t >= T or (drop_last_frame and t == T - 1) or (drop_halo and g == 15):
                continue
            s0 = HOP * t + (lead - 3 * HOP)
            N = [scipy.fft.rfft(pad[c, s0:s0 + NFFT] * w) for c in range(C)]
            assert N[0].dtype == np.complex64
            for i in range(C - 1, -1, -1):
                acc = Lf[:, i, 0] * N[0]
                for j in range(1, i + 1):
                    acc = acc + Lf[:, i, j] * N[j]
                v = scipy.fft.irfft(acc.astype(np.complex64), NFFT)
                assert v.dtype == np.float32
                fr[i, g] = v * w
        for h in range(TILE_HOPS):                       # hop t0 + h is covered by the tile's frames h .. h + 3
            a = HOP * (t0 + h)
            e = min(a + HOP, n)
            if e <= a:
                break
            acc = fr[:, h, 3 * HOP:4 * HOP]
            for d in range(1, 4):
                acc = acc + fr[:, h + d, (3 - d) * HOP:(4 - d) * HOP]
            y[:, a:e] = (acc * scale)[:, :e - a]
    return y


def add_noise(channels, noise, amp, quantized=False):
    """The noise v_c added to the mixture's channels y_c (the reference channel first, as dynamic_mix / mix_channels wrote them,
    already quantized if the batch asks for that) -> ([out_c] float64, a):
        P_y = mean(y_0^2),  P_v = mean(v_0^2)                                                          (fp64)
        a = fp32(amp sqrt(P_y / P_v)), 0 where either power is below 2^-40 (SILENT);   amp = 10^(-snr / 20) from the host
        out_c = a v_c + y_c    (the kernel: fmaf(a, v_c, y_c) in fp32),  then quantized as mixing.quantize does.
    Two choices are deliberate.  The SNR is that of the WHOLE MIXTURE over the noise, both on the reference channel -- not WHAM!'s
    rule, which sets the noise against the loudest speaker.  And the peak stays defined on the CLEAN mixture: the noisy one may
    exceed it and, quantized, clip -- a 16-bit mixture plus noise written to a 16-bit file is how WHAM! itself was made.  One
    gain serves all channels, so a diffuse field keeps its coherence."""
    ys, vs = [as_float(c) for c in channels], [as_float(v) for v in noise]
    if not 1 <= len(ys) <= MAX_MICS or len(vs) != len(ys) or any(s.ndim != 1 or s.shape != ys[0].shape or s.size < 1 for s in ys + vs):
        raise ValueError("noise: 1..%d channels and one noise signal for each, all of one length >= 1" % MAX_MICS)
    Py, Pv = float(np.mean(ys[0] * ys[0])), float(np.mean(vs[0] * vs[0]))
    a = float(np.float32(float(amp) * np.sqrt(Py / Pv))) if Py >= SILENT and Pv >= SILENT else 0.0
    outs = [a * v + y for y, v in zip(ys, vs)]
    if quantized:
        outs = [quantize(o) for o in outs]
    return outs, a


def snr_to_amp(snr_db):
    """The linear amplitude of the NOISE for a mixture-to-noise ratio in dB, 10^(-snr / 20), as float32."""
    return np.float32(10.0 ** (-float(snr_db) / 20.0))
