"""Inputs shared by tests/test_wpd.py, tests/test_gpu_wpd.py and tests/test_gpu_separate_wpd.py: S reverberant sources per bin.

Y[c][t][f] = sum_s sum_u h_s,c[f][u] S_s[t - u][f] + white noise 30 dB below, rounded to complex64: every S_s is complex
Gaussian with a slowly varying envelope of its own rate and phase (tests/_wpe_cases.reverb_case's), h_s,c[f] a random filter of
12 frames decaying by 0.7 per frame whose first tap -- random too, it is what tells the sources apart in space -- is the
source's direct image.  The masks are the ideal ratio masks of the sources' (whole) images at the reference channel,
|x_s|^2 / sum_s' |x_s'|^2, rounded to float32.  Everything is O(1), so nothing under- or overflows in fp32 or fp64.

The tests use a loading of 1e-3 and a floor of 1e-6 (a few cases a floor of 1): cond(R) <= D / delta + 1, _wpe_cases.cond_bound.
"""
import numpy as np

from sepkern import wpd as wd
from _wpe_cases import cond_bound  # noqa: F401

F = wd.F
LOADING = 1e-3
FLOOR = 1e-6


def wpd_case(C, T, S, seed, ref=0, taps=12, decay=0.7, noise_db=-30.0):
    """-> dict(Y (C, T, F) complex64, mask (T, S F) float32, direct (S, T, F) complex128: the sources' direct images at the
    reference channel, image (S, T, F) complex128: their whole images there)."""
    rng = np.random.default_rng(seed)
    X = np.zeros((S, C, T, F), dtype=np.complex128)
    direct = np.zeros((S, T, F), dtype=np.complex128)
    for s in range(S):
        env = 0.2 + np.abs(np.sin(np.arange(T)[:, None] * rng.uniform(0.2, 0.6, (1, F)) + rng.uniform(0.0, 6.0, (1, F))))
        src = env * (rng.standard_normal((T, F)) + 1j * rng.standard_normal((T, F))) / np.sqrt(2.0)
        h = (rng.standard_normal((C, F, taps)) + 1j * rng.standard_normal((C, F, taps))) * decay ** np.arange(taps) / np.sqrt(2.0)
        for u in range(min(taps, T)):
            X[s, :, u:] += h[:, None, :, u] * src[None, :T - u]
        direct[s] = h[ref, None, :, 0] * src
    Y = X.sum(axis=0)
    sigma = np.sqrt(np.mean(np.abs(Y) ** 2) * 10.0 ** (noise_db / 10.0))
    Y += sigma * (rng.standard_normal(Y.shape) + 1j * rng.standard_normal(Y.shape)) / np.sqrt(2.0)
    p = np.abs(X[:, ref]) ** 2                                                        # (S, T, F)
    mask = np.ascontiguousarray(np.transpose(p / p.sum(axis=0), (1, 0, 2))).reshape(T, S * F).astype(np.float32)
    return dict(Y=Y.astype(np.complex64), mask=mask, direct=direct, image=X[:, ref])


def condition(R, fallback):
    """cond(R) of every cell that does not fall back (1 where it does), from the definition's own loaded R."""
    R = np.where(fallback[..., None, None], np.eye(R.shape[-1]), R)
    return np.linalg.cond(R)


def w_gate(det, C, ref):
    """The forward error of the solve carried through d and the division, per cell (nblk, S, F): with gG = D 2^-52 cond(R)
    max|G| an entry of G is off by at most gG, so d by at most C gG, and w = G[:, ref] / d by at most
    gG / d + max|G[:, ref]| C gG / d^2 = (gG / d) (1 + C max|G[:, ref]| / d) to first order.  -> (gate, cond)."""
    G, d, fb = det["G"], det["d"], det["fallback"]
    D = G.shape[-2]
    cond = condition(det["R"], fb)
    with np.errstate(all="ignore"):
        gG = D * 2.0 ** -52 * cond * np.max(np.abs(G), axis=(-2, -1))
        gate = (gG / d) * (1.0 + C * np.max(np.abs(G[..., ref]), axis=-1) / d)
    return np.where(fb, 0.0, gate), cond


def apply_filter(Y, W, taps, delay, block_frames):
    """z = w^H y_ per frame with the W (nblk, S, F, D) of the frame's block, in fp64: -> (z (S, T, F) complex128,
    bound (S, T, F) = sum_d |w_d| |y__d|)."""
    T = Y.shape[1]
    yb = wd.stacked(Y, 0, T, taps, delay)                                       # (T, F, D)
    Wt = W[np.arange(T) // block_frames]                                        # (T, S, F, D)
    z = np.einsum("tsfd,tfd->stf", np.conj(Wt), yb)
    bound = np.einsum("tsfd,tfd->stf", np.abs(Wt), np.abs(yb))
    return z, bound
