"""The cases tests/test_noise.py (CPU) and tests/test_gpu_noise.py share for noisy dynamic mixing (sepkern/noise.py, csrc/noise.hip):
arrays, signals, the cached fp64 references, and the launches of the three kernels through the C ABI over pools of sentinels."""
import ctypes as C
import functools
import os
import struct
import wave

import numpy as np

from sepkern import noise

RATE = 8000
GAP, CANARY = 5, 777.0
EPS32 = 2.0 ** -24

# sk_diffuse_noise: one sample, the hop edges, one tile (13 hops = 1 664 samples) and its neighbours, two tiles and a sample
LENGTHS = [1, 127, 128, 129, 513, 1663, 1664, 1665, 3329]
# sk_add_noise: one workgroup of 1 024 threads walks a mixture; one trip and its neighbours, four trips and their neighbours
ADD_LENGTHS = [1, 1023, 1024, 1025, 4095, 4096, 4097]


def line(C_, d):
    """C microphones d metres apart on the x axis."""
    return np.array([[d * i, 0.0, 0.0] for i in range(C_)])


def circle7(r=0.0425):
    """A centre microphone and six on a circle of radius r."""
    a = 2.0 * np.pi * np.arange(6) / 6.0
    return np.concatenate([np.zeros((1, 3)), np.stack([r * np.cos(a), r * np.sin(a), np.zeros(6)], axis=1)])


TIGHT = {"line 8 x 2 cm at 8 kHz": (line(8, 0.02), 8000), "line 8 x 1 cm at 16 kHz": (line(8, 0.01), 16000),
         "circle 7 x 4.25 cm at 8 kHz": (circle7(), 8000)}


def mics_of(C_, u):
    """The array of mixture u in the GPU batches: a line, 3 to 7 cm apart, turned out of the axis (no two mixtures share factors)."""
    m = line(C_, 0.03 + 0.005 * (u % 9))
    t = 0.3 * u
    rot = np.array([[np.cos(t), -np.sin(t), 0.0], [np.sin(t), np.cos(t), 0.0], [0.0, 0.0, 1.0]])
    return m @ rot.T + np.array([1.0, 2.0, 1.5])


def signals(C_, n, seed, pcm=False):
    """C independent white signals of n samples: float32 of unit variance x 0.25, or int16 at the same level."""
    x = np.random.default_rng([seed, C_, n]).standard_normal((C_, n)) * 0.25
    if pcm:
        return np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def batch_case(C_, u, pcm):
    """Mixture u (LENGTHS[u] samples) of the C-channel GPU batch -> (x, L float32 tri, the fp64 definition, the restatement's
    own max error).  The definition and the restatement see the float32 factors the kernel sees."""
    n = LENGTHS[u]
    x = signals(C_, n, 100 + u, pcm)
    Lt = noise.tri(noise.factors(mics_of(C_, u), RATE)).astype(np.float32)
    Lf = noise.untri(Lt, C_)
    want = noise.diffuse(x, Lf.astype(np.float64))
    e32 = float(np.abs(noise.diffuse_f32(x, Lf).astype(np.float64) - want).max())
    return x, Lt, want, e32


def gate(x, e32):
    """What the kernel may differ from the fp64 definition by, per mixture: 2 max(e32, u) -- e32 the float32 restatement's own
    error for the same case, u = 2^-24 sum_j max |x_j| the unit floor (tests/test_gpu_room.py's rule: every one of the C signals
    enters every output through factors of magnitude at most 1 -- the rows of L have unit norm -- and is rounded at least once at
    its own size; a restatement that happens to land closer than that, as it may on a one-sample signal, is no gate); the factor
    2 is for the kernel's other FFT factorisation, tables and contractions."""
    from sepkern.mixing import as_float
    return 2.0 * max(float(e32), EPS32 * float(np.sum(np.abs(as_float(x)).max(axis=1))))


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def launch_diffuse(dev, xs, Lts, max_nsamp=None):
    """ONE sk_diffuse_noise call: xs[u] (C, n_u) int16 or float32, Lts[u] (257, tri) float32 -> ([(C, n_u) float32 per mixture],
    the pool, the bool mask of what should have been written).  Inputs and outputs lie in pools with GAP sentinels around every
    signal; the inputs' sentinels are large, so a read past a signal's end would show in the result."""
    import torch
    from sepkern import _lib
    B, C_ = len(xs), xs[0].shape[0]
    pcm = xs[0].dtype == np.int16
    ns = [x.shape[1] for x in xs]
    in_offs, out_offs, at = [[0] * B for _ in range(C_)], [[0] * B for _ in range(C_)], GAP
    for c in range(C_):
        for u in range(B):
            in_offs[c][u] = out_offs[c][u] = at
            at += ns[u] + GAP
    host = np.full(at, 30000 if pcm else 1.0e6, dtype=np.int16 if pcm else np.float32)
    for c in range(C_):
        for u in range(B):
            host[in_offs[c][u]:in_offs[c][u] + ns[u]] = xs[u][c]
    pool_in = torch.from_numpy(host).to(dev)
    pool = torch.full((at,), CANARY, device=dev)
    L = torch.from_numpy(np.stack(Lts)).to(dev).contiguous()
    d64 = torch.tensor([o for row in in_offs for o in row] + [o for row in out_offs for o in row], dtype=torch.int64, device=dev)
    d_ns = torch.tensor(ns, dtype=torch.int32, device=dev)
    _lib.call("sk_diffuse_noise", _ptr(pool_in), int(pcm), _ptr(d64), _ptr(d_ns), B, C_, max(ns) if max_nsamp is None else max_nsamp,
              _ptr(L), _ptr(pool), _ptr(d64[C_ * B:]), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    h = pool.cpu().numpy()
    written = np.zeros(at, dtype=bool)
    outs = []
    for u in range(B):
        outs.append(np.stack([h[out_offs[c][u]:out_offs[c][u] + ns[u]] for c in range(C_)]))
        for c in range(C_):
            written[out_offs[c][u]:out_offs[c][u] + ns[u]] = True
    return outs, h, written


def launch_add(dev, ys, vs, amp, quantize, want_gains=True):
    """ONE sk_add_noise call: ys[u] (C, n_u) float32 mixtures, vs[u] (C, n_u) noise (int16 or float32) -> ([(C, n_u)], gains, the
    signal pool, the mask of what may have changed)."""
    import torch
    from sepkern import _lib
    B, C_ = len(ys), ys[0].shape[0]
    pcm = vs[0].dtype == np.int16
    ns = [y.shape[1] for y in ys]
    offs, at = [[0] * B for _ in range(C_)], GAP
    for c in range(C_):
        for u in range(B):
            offs[c][u] = at
            at += ns[u] + GAP
    hy = np.full(at, CANARY, dtype=np.float32)
    hv = np.full(at, 30000 if pcm else 1.0e6, dtype=np.int16 if pcm else np.float32)
    for c in range(C_):
        for u in range(B):
            hy[offs[c][u]:offs[c][u] + ns[u]] = ys[u][c]
            hv[offs[c][u]:offs[c][u] + ns[u]] = vs[u][c]
    sig, nz = torch.from_numpy(hy).to(dev), torch.from_numpy(hv).to(dev)
    d64 = torch.tensor([o for row in offs for o in row], dtype=torch.int64, device=dev)
    d_ns = torch.tensor(ns, dtype=torch.int32, device=dev)
    d_amp = torch.tensor([float(a) for a in amp], dtype=torch.float32, device=dev)
    gains = torch.full((B,), CANARY, device=dev)
    _lib.call("sk_add_noise", _ptr(sig), _ptr(d64), _ptr(nz), int(pcm), _ptr(d64), _ptr(d_ns), B, C_, _ptr(d_amp), int(quantize),
              _ptr(gains) if want_gains else None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    h = sig.cpu().numpy()
    written = np.zeros(at, dtype=bool)
    outs = []
    for u in range(B):
        outs.append(np.stack([h[offs[c][u]:offs[c][u] + ns[u]] for c in range(C_)]))
        for c in range(C_):
            written[offs[c][u]:offs[c][u] + ns[u]] = True
    return outs, gains.cpu().numpy(), h, written


def check_refusals(lib):
    """Every entry point refuses bad arguments with SK_EINVAL before anything is launched: nothing here is device memory, so a
    launch would fault rather than return."""
    one = C.c_void_p(8)            # a non-null pointer that is never followed
    mics = np.ascontiguousarray(line(3, 0.05))
    mp = mics.ctypes.data_as(C.c_void_p)
    near = np.ascontiguousarray(np.array([[0.0, 0.0, 0.0], [0.005, 0.0, 0.0], [0.1, 0.0, 0.0]]))
    bad = [("sk_noise_factors", (mp, 1, 1, 8000.0, one, None), b"C = 1"), ("sk_noise_factors", (mp, 1, 9, 8000.0, one, None), b"C = 9"),
           ("sk_noise_factors", (mp, 0, 3, 8000.0, one, None), b"B = 0"), ("sk_noise_factors", (mp, 1, 3, 0.0, one, None), b"rate"),
           ("sk_noise_factors", (None, 1, 3, 8000.0, one, None), b"null"), ("sk_noise_factors", (mp, 1, 3, 8000.0, None, None), b"null"),
           ("sk_noise_factors", (near.ctypes.data_as(C.c_void_p), 1, 3, 8000.0, one, None), b"apart"),
           ("sk_diffuse_noise", (one, 0, one, one, 1, 1, 100, one, one, one, None), b"C = 1"),
           ("sk_diffuse_noise", (one, 0, one, one, 1, 9, 100, one, one, one, None), b"C = 9"),
           ("sk_diffuse_noise", (one, 0, one, one, 0, 2, 100, one, one, one, None), b"B = 0"),
           ("sk_diffuse_noise", (one, 0, one, one, 65536, 2, 100, one, one, one, None), b"B = 65536"),
           ("sk_diffuse_noise", (one, 0, one, one, 1, 2, 0, one, one, one, None), b"max_nsamp"),
           ("sk_diffuse_noise", (one, 0, one, one, 1, 2, (1 << 30) + 1, one, one, one, None), b"max_nsamp"),
           ("sk_diffuse_noise", (None, 0, one, one, 1, 2, 100, one, one, one, None), b"null"),
           ("sk_diffuse_noise", (one, 0, one, one, 1, 2, 100, None, one, one, None), b"null"),
           ("sk_diffuse_noise", (one, 0, one, one, 1, 2, 100, one, None, one, None), b"null"),
           ("sk_add_noise", (one, one, one, 0, one, one, 1, 0, one, 0, None, None), b"C = 0"),
           ("sk_add_noise", (one, one, one, 0, one, one, 1, 9, one, 0, None, None), b"C = 9"),
           ("sk_add_noise", (one, one, one, 0, one, one, 0, 1, one, 0, None, None), b"B = 0"),
           ("sk_add_noise", (None, one, one, 0, one, one, 1, 1, one, 0, None, None), b"null"),
           ("sk_add_noise", (one, one, None, 0, one, one, 1, 1, one, 0, None, None), b"null"),
           ("sk_add_noise", (one, one, one, 0, one, one, 1, 1, None, 0, None, None), b"null")]
    for name, args, word in bad:
        rc = getattr(lib, name)(*args)
        assert rc == -1 and word in lib.sk_last_error(), (name, args, rc, lib.sk_last_error())


def write_wav(path, x, rate=RATE):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(struct.pack("<%dh" % len(x), *[int(v) for v in x]))


def noise_scp(root, lengths, rate=RATE, seed=11):
    """A list of noise recordings: white int16 noise at about -20 dBFS -> the scp's path."""
    os.makedirs(root, exist_ok=True)
    rng = np.random.default_rng(seed)
    lines = []
    for k, n in enumerate(lengths):
        path = os.path.join(root, "noise%d.wav" % k)
        write_wav(path, np.clip(np.rint(rng.standard_normal(n) * 3000.0), -32768, 32767).astype(np.int16), rate)
        lines.append("noise%d %s\n" % (k, path))
    scp = os.path.join(root, "noise.scp")
    open(scp, "w").writelines(lines)
    return scp


COH_MICS, COH_N, COH_BAND = line(4, 0.05), 40000, 16


def coherence_error(y, mics=COH_MICS, rate=RATE):
    """The Welch estimate (512-point periodic Hann frames at hop 128) of the real coherence between every pair of channels of
    y (C, n) against sinc(2 f d / c) -> (the largest band-averaged error over 16-bin bands of bins 0 .. 255 and all pairs, the
    largest error of a single bin)."""
    C_, n = y.shape
    T = (n - noise.NFFT) // noise.HOP + 1
    idx = noise.HOP * np.arange(T)[:, None] + np.arange(noise.NFFT)[None, :]
    Y = np.fft.rfft(np.asarray(y, dtype=np.float64)[:, idx] * noise.window(), axis=-1)          # (C, T, 257)
    S = np.einsum('itk,jtk->ijk', Y, np.conj(Y)) / T
    G = noise.coherence(mics, rate)
    band, single = 0.0, 0.0
    for i in range(C_):
        for j in range(i):
            err = (S[i, j].real / np.sqrt(S[i, i].real * S[j, j].real))[:256] - G[:256, i, j]
            single = max(single, float(np.abs(err).max()))
            band = max(band, float(np.abs(err.reshape(-1, COH_BAND).mean(axis=1)).max()))
    return band, single
