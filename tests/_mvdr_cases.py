"""Inputs shared by tests/test_mvdr.py, tests/test_gpu_mvdr.py and tests/test_gpu_separate_mvdr.py: a synthetic microphone array.

Y = sum_s a_s[f] X_s[t, f] + white noise 20 dB below the sources' mean power, rounded to complex64.  The steering vectors a_s
have magnitudes uniform in [0.5, 1.5] and uniform random phases; X_s is complex Gaussian on 60 % of the (t, f) cells and zero on
the others.  The masks are the ratio masks |X_s|^2 / sum_s' |X_s'|^2 (0 where nothing is active) plus 0.05 uniform(-1, 1), clipped
to [0, 1], float32, laid out (T, S F) as sk_stitch writes them.

The tests use a loading of 1e-3: N_s is positive semi-definite, so with the loading its eigenvalues lie in
[delta tr / C, tr (1 + delta / C)] and cond(N_s) <= C / delta + 1 (8 001 at C = 8) for every block, however short or silent.
The fp64 solve's error, about cond C 2^-52 <= 1.5e-11, is then far below the rounding of the weights to complex64.  With 1e-6 a
one-frame block, whose N_s has rank S - 1, reaches a condition number of 2e6.
"""
import numpy as np

from sepkern import mvdr as mv

F = mv.F
LOADING = 1e-3


def steering(C, S, rng):
    return (rng.uniform(0.5, 1.5, (S, F, C)) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, (S, F, C)))).astype(np.complex128)


def array_case(C, S, T, seed, noise_db=-20.0, active=0.6, mask_noise=0.05):
    """-> dict(Y (C, T, F) complex64, mask (T, S F) float32, a (S, F, C) complex128, X (S, T, F) complex128)."""
    rng = np.random.default_rng(seed)
    a = steering(C, S, rng)
    X = (rng.standard_normal((S, T, F)) + 1j * rng.standard_normal((S, T, F))) / np.sqrt(2.0)
    X = X * (rng.uniform(0.0, 1.0, (S, T, F)) < active)
    clean = np.einsum("sfc,stf->ctf", a, X)
    sigma = np.sqrt(np.mean(np.abs(clean) ** 2) * 10.0 ** (noise_db / 10.0))
    noise = sigma * (rng.standard_normal(clean.shape) + 1j * rng.standard_normal(clean.shape)) / np.sqrt(2.0)
    Y = (clean + noise).astype(np.complex64)
    p = np.abs(X) ** 2
    tot = p.sum(axis=0)
    ratio = np.where(tot > 0.0, p / np.where(tot > 0.0, tot, 1.0), 0.0)
    m = np.clip(ratio + mask_noise * rng.uniform(-1.0, 1.0, ratio.shape), 0.0, 1.0).astype(np.float32)
    mask = np.ascontiguousarray(np.transpose(m, (1, 0, 2)).reshape(T, S * F))
    return dict(Y=Y, mask=mask, a=a, X=X)


def cond_bound(C, loading):
    """C / delta + 1, which a rank-one N_s (a one-frame block at S = 2) attains exactly, with the rounding of the computed
    condition number allowed for: the smallest singular value comes back with an absolute error of about C 2^-52 times the
    largest, a relative error of cond C 2^-52 <= 1.5e-11 in the quotient; 1e-10 covers it."""
    return (C / loading + 1.0) * (1.0 + 1e-10)


def noise_condition(scm, loading):
    """cond(N_s) of every (block, s, f) whose N_s is not zero (1 where it is), from the definition's own N."""
    N, tr = mv.noise_matrices(scm, loading)
    N = np.where((tr == 0.0)[..., None, None], np.eye(N.shape[-1]), N)
    return np.linalg.cond(N)
