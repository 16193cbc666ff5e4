"""Dereverberation of a multi-channel recording by weighted prediction error (WPE): the definition, in numpy.

Far-field recordings carry the late reverberation of their room.  WPE (Nakatani et al. 2010; Yoshioka & Nakatani 2012) predicts
it, per frequency bin, from the channels' own past by a multi-channel linear filter whose taps start DELAY frames back -- so the
direct sound and the early reflections, which the recent past does not predict, stay -- and subtracts the prediction.  The filter
minimises the prediction error weighted by the inverse of the (unknown) power of the dereverberated signal, which is estimated
from the previous iteration's output.  It is the first stage of the CHiME-5/6 front ends and of the CSS recipes, in front of
mask estimation and beamforming.  This file states what sk_wpe (include/sepkern.h, csrc/wpe.hip) computes and restates it in
numpy fp64; tests/test_gpu_wpe.py holds the kernel to it.

UNPINNED, the way sepkern/stoi.py is: no third-party implementation (nara_wpe) is installed to compare against; the tests hold
the definition to closed forms, invariances and a dereverberation check of its own.

Inputs.  Y[c][t][f], complex64 spectra of C channels (1 <= C <= 8, F = 257 bins); K >= 1 taps; a delay D_ >= 1 frames;
D = C K <= 80; I iterations, 1 <= I <= 8; a block length Lb >= 1 frames, a context of Lc >= 0 frames, Lb + 2 Lc <= 4096; a
loading delta >= 0.

Blocks and windows.  nblk = ceil(T / Lb); block j holds frames [j Lb, min(T, (j + 1) Lb)); its window w_j is
[max(0, j Lb - Lc), min(T, (j + 1) Lb + Lc)).  Every (block, bin) is an independent problem on its window, and only the block's
own frames are written from it.

Stacked past.  y~(t)[k C + c] = Y[c][t - D_ - k][f], k = 0..K-1, zero where t - D_ - k < 0; frames before the window's start but
not before 0 are the recording's real frames.

Iterations.  x(0) = y.  For i = 1..I, over the window:
    lambda(t) = (sum_c |x(i-1)_c(t)|^2) / C          c ascending, fp64, operands widened first
    lambda_max = max_t lambda(t);   lambda(t) <- max(lambda(t), 1e-10 lambda_max);   w(t) = 1 / lambda(t)
    R = sum_t (w(t) y~(t)) y~(t)^H                     D x D Hermitian: the upper triangle is computed, the diagonal is real
    P = sum_t (w(t) y~(t)) y(t)^H                      D x C;  both sums t ascending
    R += (delta Re tr R / D) I
    G = R^-1 P                                         Cholesky factorisation R = U^H U, two triangular solves per column
    x(i)(t) = y(t) - G^H y~(t)                         fp64
Pass-through.  The cell's output is Y's own bits and G = 0 when, in any iteration, lambda_max == 0, Re tr R == 0 (before the
loading) or a component of G is not finite; a matrix that is not positive definite leaves NaN, which the last condition catches.

Output.  X[c][t][f] = complex64(x(I)_c(t)) for t in block j; mag[t][f] = |X[ref][t][f]| in float32, taken from the rounded
complex64 value; G (nblk, F, D, C) complex128 of the last iteration.

Conditioning.  R is positive semi-definite, so with delta > 0 its eigenvalues lie in [delta tr / D, tr (1 + delta / D)] and
cond(R) <= D / delta + 1 for every R that is not zero, however short the window.  With delta == 0 on a window of fewer than D
frames R is singular and the result is unspecified.

Arithmetic.  Everything above is real fp64 arithmetic with one rounding per product and per sum (no fused multiply-adds), a
complex product being its four real products and two sums, and every sum has one order, stated where it is coded below; the
kernel performs the same operations in the same order.

Out of the definition, on purpose: a power estimate smoothed over neighbouring frames (the "PSD context"), recursive / online
WPE, joint WPE and beamforming (WPD), and any tuning of taps, delay and iterations: no array data is at hand.  The joint
solution is a definition of its own, sepkern/wpd.py (sk_wpd), built on this file's windows, sums and solve.
"""
import numpy as np

F = 257
MAX_C = 8
MAX_D = 80
MAX_ITERATIONS = 8
MAX_WINDOW = 4096
LAMBDA_FLOOR = 1e-10


def num_blocks(T, block_frames):
    return -(-int(T) // int(block_frames))


def block_window(j, T, block_frames, context_frames):
    """(b0, b1, w0, w1): block j's frames [b0, b1) and its window [w0, w1)."""
    b0, b1 = min(T, j * block_frames), min(T, (j + 1) * block_frames)
    return b0, b1, max(0, j * block_frames - context_frames), min(T, (j + 1) * block_frames + context_frames)


def check_arguments(C, T, taps, delay, iterations, block_frames, context_frames, ref, loading):
    if not 1 <= C <= MAX_C:
        raise ValueError("wpe: C = %d channels outside 1..%d" % (C, MAX_C))
    if taps < 1 or delay < 1:
        raise ValueError("wpe: taps = %d, delay = %d, at least 1 expected" % (taps, delay))
    if C * taps > MAX_D:
        raise ValueError("wpe: C * taps = %d above %d" % (C * taps, MAX_D))
    if not 1 <= iterations <= MAX_ITERATIONS:
        raise ValueError("wpe: iterations = %d outside 1..%d" % (iterations, MAX_ITERATIONS))
    if T < 1 or block_frames < 1 or context_frames < 0:
        raise ValueError("wpe: T = %d frames, blocks of %d frames, a context of %d frames" % (T, block_frames, context_frames))
    if block_frames + 2 * context_frames > MAX_WINDOW:
        raise ValueError("wpe: a window of %d + 2 * %d frames, at most %d" % (block_frames, context_frames, MAX_WINDOW))
    if not 0 <= ref < C:
        raise ValueError("wpe: reference channel %d outside [0, %d)" % (ref, C))
    if not loading >= 0.0:
        raise ValueError("wpe: loading %r is negative or NaN" % (loading,))


def workspace_bytes(T, C, taps, block_frames, context_frames):
    """Bytes of device workspace sk_wpe needs: none -- R, P, G and the window's weights live in a workgroup's LDS."""
    return 0


def stacked_past(Y, t0, t1, taps, delay):
    """y~(t) for t in [t0, t1): (t1 - t0, F, C taps) complex128."""
    C = Y.shape[0]
    out = np.zeros((t1 - t0, F, C * taps), dtype=np.complex128)
    for k in range(taps):
        src = np.arange(t0, t1) - delay - k
        ok = src >= 0
        for c in range(C):
            out[ok, :, k * C + c] = Y[c, src[ok], :F]
    return out


def covariances(yt, y, w, pt=None, pw=None):
    """R (F, D, D), P (F, D, C): the weighted sums over the window, t ascending; yt (L, F, D), y (L, F, C), w (L, F).  Real
    arithmetic, one rounding per product and per sum: (w y~_a) conj(b) = (pr qr + pi qi) + i (pi qr - pr qi).
    With pt (L, F, Dp) and pw (L, F) the second sum is P = sum_t (pw(t) pt(t)) y(t)^H, (F, Dp, C), instead (sepkern/wpd.py)."""
    L, D, C = yt.shape[0], yt.shape[2], y.shape[2]
    tf = lambda a: np.ascontiguousarray(np.transpose(a, (0, 2, 1)))                # bins innermost: (L, D, F)
    ytr, yti, yr, yi = tf(yt.real), tf(yt.imag), tf(y.real), tf(y.imag)
    ptr, pti = (ytr, yti) if pt is None else (tf(pt.real), tf(pt.imag))
    pw = w if pw is None else pw
    Rr, Ri, t1, t2 = (np.zeros((D, D, F)) for _ in range(4))
    Pr, Pi, u1, u2 = (np.zeros((ptr.shape[1], C, F)) for _ in range(4))

    def add(pr, pi, qr, qi, re, im, a, b):
        np.multiply(pr, qr, out=a)
        np.multiply(pi, qi, out=b)
        a += b
        re += a
        np.multiply(pi, qr, out=a)
        np.multiply(pr, qi, out=b)
        a -= b
        im += a

    for t in range(L):
        pr, pi = (ytr[t] * w[t])[:, None, :], (yti[t] * w[t])[:, None, :]
        add(pr, pi, ytr[t][None], yti[t][None], Rr, Ri, t1, t2)
        if pt is not None:
            pr, pi = (ptr[t] * pw[t])[:, None, :], (pti[t] * pw[t])[:, None, :]
        add(pr, pi, yr[t][None], yi[t][None], Pr, Pi, u1, u2)
    Rr, Ri, Pr, Pi = (np.transpose(a, (2, 0, 1)) for a in (Rr, Ri, Pr, Pi))
    up = np.triu(np.ones((D, D), dtype=bool), 1)
    upper = np.where(up, Rr + 1j * Ri, 0.0)
    herm = upper + np.conj(np.swapaxes(upper, -1, -2))
    for a in range(D):
        herm[:, a, a] = Rr[:, a, a]
    return herm, Pr + 1j * Pi


def cholesky_solve(R, P):
    """G = R^-1 P for stacks (F, D, D), (F, D, C) through R = U^H U; NaN where R is not positive definite.  Only the upper
    triangle of R is read.  Real arithmetic in one order: an entry of U loses its products k ascending and is then scaled by
    1 / U[a][a]; the forward substitution subtracts i ascending, the backward one i descending."""
    D = R.shape[-1]
    Rr, Ri, Pr, Pi = R.real.copy(), R.imag.copy(), P.real.copy(), P.imag.copy()
    Ur, Ui = np.zeros_like(Rr), np.zeros_like(Rr)
    rinv = np.zeros((R.shape[0], D))
    with np.errstate(all="ignore"):
        for a in range(D):
            vr, vi = Rr[:, a, a:].copy(), Ri[:, a, a:].copy()
            for k in range(a):                                       # - conj(U[k][a]) U[k][b]
                ur, ui, br, bi = Ur[:, k, a, None], Ui[:, k, a, None], Ur[:, k, a:], Ui[:, k, a:]
                vr -= ur * br + ui * bi
                vi -= ur * bi - ui * br
            rinv[:, a] = 1.0 / np.sqrt(vr[:, 0])
            Ur[:, a, a + 1:], Ui[:, a, a + 1:] = vr[:, 1:] * rinv[:, a, None], vi[:, 1:] * rinv[:, a, None]
        Zr, Zi = np.zeros_like(Pr), np.zeros_like(Pr)
        for a in range(D):
            vr, vi = Pr[:, a].copy(), Pi[:, a].copy()
            for i in range(a):                                       # - conj(U[i][a]) z[i]
                ur, ui = Ur[:, i, a, None], Ui[:, i, a, None]
                vr -= ur * Zr[:, i] + ui * Zi[:, i]
                vi -= ur * Zi[:, i] - ui * Zr[:, i]
            Zr[:, a], Zi[:, a] = vr * rinv[:, a, None], vi * rinv[:, a, None]
        Gr, Gi = np.zeros_like(Pr), np.zeros_like(Pr)
        for a in range(D - 1, -1, -1):
            vr, vi = Zr[:, a].copy(), Zi[:, a].copy()
            for i in range(D - 1, a, -1):                            # - U[a][i] g[i]
                ur, ui = Ur[:, a, i, None], Ui[:, a, i, None]
                vr -= ur * Gr[:, i] - ui * Gi[:, i]
                vi -= ur * Gi[:, i] + ui * Gr[:, i]
            Gr[:, a], Gi[:, a] = vr * rinv[:, a, None], vi * rinv[:, a, None]
    return Gr + 1j * Gi


def residual(y, yt, G):
    """x = y - G^H y~ over a window: y (L, F, C), yt (L, F, D), G (F, D, C); the prediction is summed d ascending from zero,
    conj(g) y~ = (gr yr + gi yi) + i (gr yi - gi yr), then subtracted."""
    sr, si = np.zeros(y.shape), np.zeros(y.shape)
    for d in range(G.shape[1]):
        gr, gi, pr, pi = G[None, :, d, :].real, G[None, :, d, :].imag, yt[:, :, d, None].real, yt[:, :, d, None].imag
        sr += gr * pr + gi * pi
        si += gr * pi - gi * pr
    return (y.real - sr) + 1j * (y.imag - si)


def wpe_block(Y, j, taps, delay, iterations, block_frames, context_frames, loading):
    """Block j of Y (C, T, >= F) complex64 -> (X (C, b1 - b0, F) complex64, G (F, D, C) complex128, passed (F,) bool: the bins
    that are passed through, R (F, D, D): the loaded matrix of the last iteration)."""
    C, T = Y.shape[0], Y.shape[1]
    D = C * taps
    b0, b1, w0, w1 = block_window(j, T, block_frames, context_frames)
    yt = stacked_past(Y, w0, w1, taps, delay)
    y = np.ascontiguousarray(np.transpose(Y[:, w0:w1, :F], (1, 2, 0))).astype(np.complex128)            # (L, F, C)
    x = y
    passed = np.zeros(F, dtype=bool)
    G = np.zeros((F, D, C), dtype=np.complex128)
    R = np.zeros((F, D, D), dtype=np.complex128)
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            lam = np.zeros(x.shape[:2])
            for c in range(C):
                lam = lam + (x[:, :, c].real ** 2 + x[:, :, c].imag ** 2)
            lam = lam / C
            lmax = lam.max(axis=0)
            w = 1.0 / np.maximum(lam, LAMBDA_FLOOR * lmax)
            R, P = covariances(yt, y, w)
            tr = np.zeros(F)
            for a in range(D):
                tr = tr + R[:, a, a].real
            load = loading * tr / D
            for a in range(D):
                R[:, a, a] = R[:, a, a].real + load
            G = cholesky_solve(R, P)
            passed = passed | (lmax == 0.0) | (tr == 0.0) | ~np.isfinite(G.view(np.float64)).all(axis=(1, 2))
            x = residual(y, yt, G)
    G[passed] = 0.0
    X = np.transpose(x[b0 - w0:b1 - w0], (2, 0, 1)).astype(np.complex64)
    X[:, :, passed] = Y[:, b0:b1, :F][:, :, passed]
    return X, G, passed, R


def wpe_reference(Y, taps, delay, iterations, block_frames, context_frames, loading, ref=0, details=False):
    """Y (C, T, >= F) complex64 -> (X (C, T, F) complex64, mag (T, F) float32, G (nblk, F, D, C) complex128); with details a
    fourth value dict(passed (nblk, F) bool, R (nblk, F, D, D) complex128: the loaded matrices of the last iteration)."""
    Y = np.asarray(Y)
    if Y.ndim != 3 or Y.shape[2] < F or Y.dtype != np.complex64:
        raise ValueError("wpe: Y must be (C, T, >= 257) complex64")
    C, T = Y.shape[0], Y.shape[1]
    check_arguments(C, T, taps, delay, iterations, block_frames, context_frames, ref, loading)
    nblk, D = num_blocks(T, block_frames), C * taps
    X = np.zeros((C, T, F), dtype=np.complex64)
    G = np.zeros((nblk, F, D, C), dtype=np.complex128)
    passed = np.zeros((nblk, F), dtype=bool)
    R = np.zeros((nblk, F, D, D), dtype=np.complex128) if details else None
    for j in range(nblk):
        b0, b1, _, _ = block_window(j, T, block_frames, context_frames)
        X[:, b0:b1], G[j], passed[j], Rj = wpe_block(Y, j, taps, delay, iterations, block_frames, context_frames, loading)
        if details:
            R[j] = Rj
    mag = np.abs(X[ref])
    if details:
        return X, mag, G, dict(passed=passed, R=R)
    return X, mag, G
