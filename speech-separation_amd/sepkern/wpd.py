"""Mask-based WPD convolutional beamforming of a multi-channel recording: the definition, in numpy.

The cascade sk_wpe -> masks -> sk_mvdr is optimal stage by stage only: WPE's prediction filter is fitted to the mixture's power,
and MVDR is left with C degrees of freedom per bin.  The weighted power minimisation distortionless response (WPD) beamformer
(Nakatani & Kinoshita 2019; Nakatani et al. 2020, "Jointly optimal denoising, dereverberation, and source separation") solves
the three jointly: one filter per source over the present frame and the delayed past of all channels, fitted under that
source's own time-varying power and constrained to pass the source's direct image at the reference microphone; the form used
here needs no steering vector (Zhang et al. 2020).  This file states what sk_wpd (include/sepkern.h, csrc/wpd.hip) computes and
restates it in numpy fp64; tests/test_gpu_wpd.py holds the kernel to it.  The blocks and windows, the sums' arithmetic and the
Cholesky solve are sepkern/wpe.py's and are not restated here.

UNPINNED, the way sepkern/wpe.py is: no third-party implementation is installed to compare against; the tests hold the
definition to closed forms (K = 0 is a weighted MPDR beamformer, floor = 1 the unweighted convolutional MPDR), invariances and a
separation check of its own.

Inputs.  Y[c][t][f], complex64 spectra of C channels (2 <= C <= 8, F = 257 bins); mask (T, >= S 257) float32 with stream s in
columns s 257 .. (sk_stitch's or sk_cacgmm's output), 2 <= S <= 4; K >= 0 taps; a delay D_ >= 1 frames; D = C (K + 1) <= 80;
I iterations, 1 <= I <= 8; blocks and windows exactly sk_wpe's (wpe.block_window), Lb >= 1, Lc >= 0, Lb + 2 Lc <= 4096; a
reference channel ref; a loading delta >= 0; a power floor phi in (0, 1]; optionally a filter to start from,
W_in (nblk, S, F, D) complex128.

Stacked vector.  y_(t)[c] = Y[c][t][f] for c < C, y_(t)[C + k C + c] = Y[c][t - D_ - k][f] for k < K, zero where t - D_ - k < 0;
frames before the window's start but not before 0 are the recording's real frames.  y(t) is its first C entries.

Per (block j, bin f, stream s), on the window, every operand widened to fp64 first, with m(t) = mask[t][s 257 + f]:
  1. power    in iteration 1 without W_in:  lambda(t) = m(t) ((sum_c |y_c(t)|^2) / C), c ascending from zero
              otherwise:                    lambda(t) = zr^2 + zi^2 of z(t) = w^H y_(t) with the previous iteration's w or W_in,
                                            summed d ascending from zero, conj(w) y = (wr yr + wi yi) + i (wr yi - wi yr)
              lambda_max = max_t lambda(t);  lambda(t) <- max(lambda(t), phi lambda_max);  omega(t) = 1 / lambda(t)
  2. sums     R = sum_t (omega(t) y_(t)) y_(t)^H, D x D: the upper triangle is computed, the diagonal is real, t ascending;
              R += (delta Re tr R / D) I, the trace summed a ascending before the loading
              PHI = sum_t (m(t) y(t)) y(t)^H, C x C, t ascending: every entry is summed as it stands, the lower triangle too,
              so PHI is Hermitian up to the rounding of (m a) b against (m b) a.  It is not normalised: step 4 does not see
              its scale.  PHI~ = [PHI; 0] is D x C
  3. solve    G = R^-1 PHI~ by wpe.cholesky_solve
  4. filter   d = sum_{c < C} Re G[c][c], c ascending;  w = G[:, ref] / d, each component divided by the real d.  This is
              Souden's form: for a rank-one PHI = p a a^H it gives w^H [a; 0] = a_ref whatever R
  5. fallback the cell falls back to w = e_ref -- the reference channel passed through, the present frame only -- when in any
              iteration lambda_max == 0, Re tr R == 0 before the loading, Re tr PHI == 0, d is not > 0 or a component of w is
              not finite (a matrix that is not positive definite leaves NaN, which the last two catch)
Output.  Z[s][t][f] = complex64(w^H y_(t)) for t in block j, summed as in step 1; a cell that fell back stores Y[ref]'s own
bits.  W (nblk, S, F, D) complex128: the last iteration's w, e_ref in a cell that fell back.

Chaining.  One call of I iterations gives the bits of I calls of one iteration chained through W -> W_in in every cell that does
not fall back, and in those whose cause is in the data (a silent window, a mask that is zero over the window): a cell that fell
back for d or for a component that is not finite starts afresh from e_ref in a chained call.

Conditioning.  wpe.py's remark holds: R is positive semi-definite, so with delta > 0 cond(R) <= D / delta + 1 for every R that
is not zero, however short the window; with delta == 0 on a window of fewer than D frames R is singular and the result is
unspecified.  phi = 1 makes every weight the same number, phi = 1e-6 lets the quietest frames weigh 60 dB above the loudest.

Arithmetic.  As in wpe.py: real fp64 arithmetic, one rounding per product and per sum, no fused multiply-adds, every sum in
the one order stated; the kernel performs the same operations in the same order.

Out of the definition, on purpose: a noise class of its own (the sources' masks are all there is), a steering vector estimated
from an eigenvector, online or recursive estimation, and any tuning of taps, delay and floor -- no array corpus is at hand, so
the defaults (5 taps, a delay of 3, 2 iterations, a floor of 1e-6) are the literature's.
"""
import numpy as np

from . import wpe as wp
from .wpe import block_window, num_blocks  # noqa: F401  (the window rule is sk_wpe's)

F = wp.F
MIN_C, MAX_C = 2, wp.MAX_C
MIN_S, MAX_S = 2, 4
MAX_D = wp.MAX_D
MAX_ITERATIONS = wp.MAX_ITERATIONS
MAX_WINDOW = wp.MAX_WINDOW


def check_arguments(C, S, T, taps, delay, iterations, block_frames, context_frames, ref, loading, floor):
    if not MIN_C <= C <= MAX_C:
        raise ValueError("wpd: C = %d channels outside %d..%d" % (C, MIN_C, MAX_C))
    if not MIN_S <= S <= MAX_S:
        raise ValueError("wpd: S = %d streams outside %d..%d" % (S, MIN_S, MAX_S))
    if taps < 0:
        raise ValueError("wpd: taps = %d is negative" % taps)
    if delay < 1:
        raise ValueError("wpd: delay = %d, at least 1 expected" % delay)
    if C * (taps + 1) > MAX_D:
        raise ValueError("wpd: C * (taps + 1) = %d above %d" % (C * (taps + 1), MAX_D))
    if not 1 <= iterations <= MAX_ITERATIONS:
        raise ValueError("wpd: iterations = %d outside 1..%d" % (iterations, MAX_ITERATIONS))
    if T < 1 or block_frames < 1 or context_frames < 0:
        raise ValueError("wpd: T = %d frames, blocks of %d frames, a context of %d frames" % (T, block_frames, context_frames))
    if block_frames + 2 * context_frames > MAX_WINDOW:
        raise ValueError("wpd: a window of %d + 2 * %d frames, at most %d" % (block_frames, context_frames, MAX_WINDOW))
    if not 0 <= ref < C:
        raise ValueError("wpd: reference channel %d outside [0, %d)" % (ref, C))
    if not loading >= 0.0:
        raise ValueError("wpd: loading %r is negative or NaN" % (loading,))
    if not 0.0 < floor <= 1.0:
        raise ValueError("wpd: floor %r outside (0, 1] or NaN" % (floor,))


def workspace_bytes(T, C, S, taps, block_frames, context_frames):
    """Bytes of device workspace sk_wpd needs: none -- R, PHI~, G, the filter and the window's weights live in a workgroup's LDS."""
    return 0


def stacked(Y, t0, t1, taps, delay):
    """y_(t) for t in [t0, t1): (t1 - t0, F, C (taps + 1)) complex128, the present frame first."""
    y = np.ascontiguousarray(np.transpose(Y[:, t0:t1, :F], (1, 2, 0))).astype(np.complex128)
    if taps == 0:
        return y
    return np.concatenate([y, wp.stacked_past(Y, t0, t1, taps, delay)], axis=2)


def apply(w, yb):
    """z = w^H y_ over frames: w (F, D), yb (L, F, D) -> (L, F) complex128, summed d ascending from zero."""
    zr, zi = np.zeros(yb.shape[:2]), np.zeros(yb.shape[:2])
    for d in range(w.shape[1]):
        wr, wi, pr, pi = w[None, :, d].real, w[None, :, d].imag, yb[:, :, d].real, yb[:, :, d].imag
        zr += wr * pr + wi * pi
        zi += wr * pi - wi * pr
    return zr + 1j * zi


def wpd_block(Y, mask, j, s, taps, delay, iterations, block_frames, context_frames, ref, loading, floor, W_in=None):
    """Block j, stream s of Y (C, T, >= F) complex64 and mask (>= T, >= S F) float32; W_in (F, D) or None ->
    dict(Z (b1 - b0, F) complex64, W (F, D), G (F, D, C): the last iteration's unnormalised solution, d (F,), R (F, D, D): the
    loaded matrix of the last iteration, fallback (F,) bool)."""
    C, T = Y.shape[0], Y.shape[1]
    D = C * (taps + 1)
    b0, b1, w0, w1 = block_window(j, T, block_frames, context_frames)
    yb = stacked(Y, w0, w1, taps, delay)                                                     # (L, F, D)
    y = yb[:, :, :C]
    m = mask[w0:w1, s * F:(s + 1) * F].astype(np.float64)                                    # (L, F)
    w = None if W_in is None else np.asarray(W_in, dtype=np.complex128)
    fb = np.zeros(F, dtype=bool)
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            if w is None:
                lam = np.zeros(m.shape)
                for c in range(C):
                    lam = lam + (y[:, :, c].real ** 2 + y[:, :, c].imag ** 2)
                lam = m * (lam / C)
            else:
                z = apply(w, yb)
                lam = z.real * z.real + z.imag * z.imag
            lmax = lam.max(axis=0)
            om = 1.0 / np.maximum(lam, floor * lmax)
            R, Phi = wp.covariances(yb, y, om, pt=y, pw=m)
            tr, trp = np.zeros(F), np.zeros(F)
            for a in range(D):
                tr = tr + R[:, a, a].real
            for c in range(C):
                trp = trp + Phi[:, c, c].real
            load = loading * tr / D
            for a in range(D):
                R[:, a, a] = R[:, a, a].real + load
            rhs = np.zeros((F, D, C), dtype=np.complex128)
            rhs[:, :C] = Phi
            G = wp.cholesky_solve(R, rhs)
            d = np.zeros(F)
            for c in range(C):
                d = d + G[:, c, c].real
            w = G[:, :, ref].real / d[:, None] + 1j * (G[:, :, ref].imag / d[:, None])
            fb = fb | (lmax == 0.0) | (tr == 0.0) | (trp == 0.0) | ~(d > 0.0) | ~np.isfinite(w.view(np.float64)).all(axis=1)
        w[fb] = 0.0
        w[fb, ref] = 1.0
        Z = apply(w, yb[b0 - w0:b1 - w0]).astype(np.complex64)
    Z[:, fb] = Y[ref, b0:b1, :F][:, fb]
    return dict(Z=Z, W=w, G=G, d=d, R=R, fallback=fb)


def wpd_reference(Y, mask, S, taps, delay, iterations, block_frames, context_frames, loading, floor, ref=0, W_in=None,
                  details=False):
    """Y (C, T, >= F) complex64, mask (>= T, >= S F) float32 -> (Z (S, T, F) complex64, W (nblk, S, F, D) complex128); with
    details a third value dict(G (nblk, S, F, D, C), d (nblk, S, F), R (nblk, S, F, D, D), fallback (nblk, S, F) bool)."""
    Y, mask = np.asarray(Y), np.asarray(mask)
    if Y.ndim != 3 or Y.shape[2] < F or Y.dtype != np.complex64:
        raise ValueError("wpd: Y must be (C, T, >= 257) complex64")
    C, T = Y.shape[0], Y.shape[1]
    check_arguments(C, S, T, taps, delay, iterations, block_frames, context_frames, ref, loading, floor)
    if mask.ndim != 2 or mask.shape[0] < T or mask.shape[1] < S * F or mask.dtype != np.float32:
        raise ValueError("wpd: mask must be (>= T, >= S * 257) float32")
    nblk, D = num_blocks(T, block_frames), C * (taps + 1)
    if W_in is not None:
        W_in = np.asarray(W_in)
        if W_in.shape != (nblk, S, F, D) or W_in.dtype != np.complex128:
            raise ValueError("wpd: W_in must be (nblk, S, 257, D) complex128")
    Z = np.zeros((S, T, F), dtype=np.complex64)
    W = np.zeros((nblk, S, F, D), dtype=np.complex128)
    det = dict(G=np.zeros((nblk, S, F, D, C), dtype=np.complex128), d=np.zeros((nblk, S, F)),
               R=np.zeros((nblk, S, F, D, D), dtype=np.complex128), fallback=np.zeros((nblk, S, F), dtype=bool)) if details else None
    for j in range(nblk):
        b0, b1, _, _ = block_window(j, T, block_frames, context_frames)
        for s in range(S):
            r = wpd_block(Y, mask, j, s, taps, delay, iterations, block_frames, context_frames, ref, loading, floor,
                          None if W_in is None else W_in[j, s])
            Z[s, b0:b1], W[j, s] = r["Z"], r["W"]
            if details:
                for k in det:
                    det[k][j, s] = r[k]
    if details:
        return Z, W, det
    return Z, W
