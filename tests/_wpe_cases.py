"""Inputs shared by tests/test_wpe.py, tests/test_gpu_wpe.py and tests/test_gpu_separate_wpe.py: reverberant spectra per bin.

Y[c][t][f] = sum_u h_c[f][u] S[t - u][f] + white noise 30 dB below, rounded to complex64: S is complex Gaussian with a slowly
varying envelope (the non-stationarity WPE's weights feed on), h_c[f] a random filter of 12 frames decaying by 0.7 per frame
with h_c[f][0] = 1.  Everything is O(1), so nothing under- or overflows in fp32 or fp64.

The tests use a loading of 1e-3: R is positive semi-definite, so with the loading its eigenvalues lie in
[delta tr / D, tr (1 + delta / D)] and cond(R) <= D / delta + 1 (80 001 at D = 80) for every window, however short.
"""
import numpy as np

from sepkern import wpe as wp

F = wp.F
LOADING = 1e-3


def reverb_case(C, T, seed, taps=12, decay=0.7, noise_db=-30.0):
    """-> Y (C, T, F) complex64."""
    rng = np.random.default_rng(seed)
    env = 0.2 + np.abs(np.sin(np.arange(T)[:, None] * rng.uniform(0.2, 0.6, (1, F)) + rng.uniform(0.0, 6.0, (1, F))))
    S = env * (rng.standard_normal((T, F)) + 1j * rng.standard_normal((T, F))) / np.sqrt(2.0)
    h = (rng.standard_normal((C, F, taps)) + 1j * rng.standard_normal((C, F, taps))) * decay ** np.arange(taps) / np.sqrt(2.0)
    h[:, :, 0] = 1.0
    Y = np.zeros((C, T, F), dtype=np.complex128)
    for u in range(min(taps, T)):
        Y[:, u:] += h[:, None, :, u] * S[None, :T - u]
    sigma = np.sqrt(np.mean(np.abs(Y) ** 2) * 10.0 ** (noise_db / 10.0))
    Y += sigma * (rng.standard_normal(Y.shape) + 1j * rng.standard_normal(Y.shape)) / np.sqrt(2.0)
    return Y.astype(np.complex64)


def cond_bound(D, loading):
    """D / delta + 1, which a rank-one R (a window with one non-zero stacked past) attains exactly, with the rounding of the
    computed condition number allowed for: the smallest singular value comes back with an absolute error of about D 2^-52 times
    the largest, a relative error of cond D 2^-52 <= 1.5e-9 in the quotient at D = 80; 1e-8 covers it."""
    return (D / loading + 1.0) * (1.0 + 1e-8)


def condition(R, passed):
    """cond(R) of every (block, f) that is not passed through (1 where it is), from the definition's own loaded R."""
    R = np.where(passed[..., None, None], np.eye(R.shape[-1]), R)
    return np.linalg.cond(R)


def apply_filter(Y, G, taps, delay, block_frames):
    """x = y - G^H y~ per frame with the G of the frame's block, in fp64: -> (x (C, T, F) complex128, bound (C, T, F) =
    |y| + sum_d |G[d][c]| |y~[d]|)."""
    C, T = Y.shape[0], Y.shape[1]
    yt = wp.stacked_past(Y, 0, T, taps, delay)                                  # (T, F, D)
    blk = np.arange(T) // block_frames
    Gt = G[blk]                                                                 # (T, F, D, C)
    x = np.transpose(Y[:, :, :F], (1, 2, 0)).astype(np.complex128) - np.einsum("tfdc,tfd->tfc", np.conj(Gt), yt)
    bound = np.abs(np.transpose(Y[:, :, :F], (1, 2, 0))).astype(np.float64) + np.einsum("tfdc,tfd->tfc", np.abs(Gt), np.abs(yt))
    return np.transpose(x, (2, 0, 1)), np.transpose(bound, (2, 0, 1))
