"""Inputs, the case list and the gates shared by tests/test_cacgmm.py, tests/test_gpu_cacgmm.py and
tests/test_gpu_separate_cacgmm.py.

Inputs.  S sources with non-stationary envelopes, a random rank-one steering vector per (source, bin), white noise 10 dB below
the sources: Y[c][t][f] = sum_k h_k[f][c] s_k[t][f] + noise, rounded to complex64.  The priors are the ideal ratio masks of the
sources' images pulled 35 % towards 0.5, with N(0, 0.1) noise added, clipped to [0, 1], float32.  Everything is O(1); the
loading is 1e-3, so every updated B has cond(B) <= C / delta + 1 (sepkern/cacgmm.py).

Gates.  An implementation is a callable impl(Y, prior, S, iterations, Lb, Lc, loading, B_in) -> (mask (T, S F) float32, B (nblk,
S, F, C, C) complex128).  The GPU test hands the kernel to the gates below; tests/test_cacgmm.py hands them the numpy
definition, which passes, and mutants of it, each of which fails one.

gate_posteriors: mask within 2^-23 gamma + 2^-149 of cacgmm_posteriors evaluated in numpy on the B the implementation
    RETURNED (for iterations == 0 on B_in).  2^-24 gamma is the rounding to float32; the fp64 error of gamma is twice that of
    l, which with cond(B) <= 8001 and |l| of order 100 is below 1e-9; 2^-149 is the subnormal floor.

gate_one_step: with iterations == 1, B within 2^-52 (Lw + c1 C^2 cond(B_in) + c2 max|l|) A of cacgmm_step on the same state,
    A[a][b] = C sum_t gamma_k |z_a| |z_b| / q_k / n_k from the reference, Lw the window's frames, c1 = 132, c2 = 40:
      - the sum.  B'[a][b] is a recursive sum of Lw products of a few roundings each, scaled: (Lw + 8) 2^-53 A.
      - q.  The computed factor has U^H U = B + dB, |dB| <= gamma_(C+1) |U^H| |U|, and a substitution is backward stable with
        gamma_C (Higham, Accuracy and Stability, 10.1 and 8.1; about 2 sqrt(2) times that for complex operands), so the
        relative error of q = z^H B^-1 z is at most 8 C^2 cond(B) 2^-53 = 4 C^2 cond(B) 2^-52 = e_q.  It reaches B' three ways:
        through 1 / q (e_q), through gamma (l has C log q, and d gamma / gamma = dl_k - sum_j gamma_j dl_j <= 2 max|dl|:
        2 C e_q) and through n_k (2 C e_q).  (4 C + 1) <= 33 at C = 8: c1 = 4 x 33 = 132.  The constant also covers the
        sum's + 8, the normalisation of z ((C + 4) 2^-53) and exp (1 ulp, twice).  The loading adds delta tr B' / C to the
        diagonal, with delta times the mean error of the diagonal: nothing beside the rest, except where a diagonal entry
        of A is below delta times the mean one (windows of a few frames); the gate does not count it there either and is
        then stricter than derived.
      - log.  The device library's log and exp are within 1 ulp (2^-52 relative); with the roundings of the three operations
        that make l, dl <= 2.5 x 2^-52 (|log p| + 2 |sum log U[a][a]| + C |log q|).  The gate asserts on the reference that
        these magnitudes sum to at most 4 max|l| (no cancellation to speak of: B' = C S / n has the scale at which log det
        and C log q are each O(l)), so dl <= 10 x 2^-52 max|l|, and gamma and n_k carry 2 dl each: c2 = 40.
    The constants are derived, not fitted: a kernel that follows the definition's order is off by a few units in the last
    place, far below the gate, and the mutants are off by 1e-3 of A and more, far above it.

gate_chaining: one call with iterations == 3 gives bit for bit the mask and B of three calls with iterations == 1 chained
    through B -> B_in, and iterations == 0 on that B reproduces the mask.  This pins the iteration loop to the single step;
    EM amplifies differences, so no end-to-end tolerance can be derived.
"""
import functools

import numpy as np

from sepkern import cacgmm as cg

F = cg.F
LOADING = 1e-3
C1, C2 = 132.0, 40.0

CS = [(2, 2), (3, 3), (4, 2), (5, 4), (8, 2), (8, 4)]
# (T, Lb, Lc): T < Lb; T = Lb; a last block of one frame; with a context; a context clipped at both ends; one-frame blocks;
# windows of two chunks of the kernel's 64 frames, the second one partial (104, 126 and 62 frames) and blocks of one chunk;
# blocks and windows of more than two chunks: block 0 is 150 frames (three chunks of the output walk) in a window of 190, block
# 1 is 80 frames in a window of 120
GEOMETRIES = [(9, 16, 0), (16, 16, 0), (33, 16, 0), (33, 16, 5), (40, 7, 100), (5, 1, 2), (150, 64, 40), (230, 150, 40)]
ITERATIONS = [0, 1, 3]


def spatial_case(C, S, T, seed, noise_db=-10.0):
    """-> (Y (C, T, F) complex64, prior (T, S F) float32, dominant (T, S, F) fp64: 1 for the source with the strongest image)."""
    rng = np.random.default_rng(seed)
    gauss = lambda *sh: (rng.standard_normal(sh) + 1j * rng.standard_normal(sh)) / np.sqrt(2.0)
    t = np.arange(T)[None, :, None]
    env = 0.05 + np.sin(t * rng.uniform(0.05, 0.4, (S, 1, F)) + rng.uniform(0.0, 6.0, (S, 1, F))) ** 2
    s = env * gauss(S, T, F)
    h = gauss(S, F, C)
    img = h.transpose(0, 2, 1)[:, :, None, :] * s[:, None]                              # (S, C, T, F)
    Y = img.sum(axis=0)
    sigma = np.sqrt(np.mean(np.abs(Y) ** 2) * 10.0 ** (noise_db / 10.0))
    Y = Y + sigma * gauss(C, T, F)
    power = np.mean(np.abs(img) ** 2, axis=1)                                           # (S, T, F)
    irm = power / power.sum(axis=0)
    m = np.clip(irm + 0.35 * (0.5 - irm) + 0.1 * rng.standard_normal(irm.shape), 0.0, 1.0)
    prior = np.ascontiguousarray(np.transpose(m, (1, 0, 2))).reshape(T, S * F).astype(np.float32)
    dominant = (power == power.max(axis=0)).astype(np.float64)
    return Y.astype(np.complex64), prior, np.ascontiguousarray(np.transpose(dominant, (1, 0, 2)))


@functools.lru_cache(maxsize=None)
def inputs(C, S, T):
    Y, prior, dom = spatial_case(C, S, T, seed=1000 * C + 100 * S + T)
    for a in (Y, prior, dom):
        a.setflags(write=False)
    return Y, prior, dom


def cond_bound(C, loading):
    """C / delta + 1, with the rounding of the computed condition number allowed for (tests/_wpe_cases.py)."""
    return (C / loading + 1.0) * (1.0 + 1e-8)


def definition(Y, prior, S, iterations, Lb, Lc, loading, B_in):
    mask, B, _ = cg.cacgmm_reference(Y, prior, S, iterations, Lb, Lc, loading, B_in=B_in)
    return mask, B


@functools.lru_cache(maxsize=4)
def two_iterations(C, S, T, Lb, Lc):
    """The state the reference reaches in two iterations: the B_in of the second one-step case."""
    Y, prior, _ = inputs(C, S, T)
    _, B, d = cg.cacgmm_reference(Y, prior, S, 2, Lb, Lc, LOADING)
    for st in d["states"]:
        assert float(np.max(np.linalg.cond(st))) <= cond_bound(C, LOADING)
    B.setflags(write=False)
    return B


@functools.lru_cache(maxsize=4)
def reference_step(C, S, T, Lb, Lc, from_identity):
    """cacgmm_step on the case's inputs from the identity or from two_iterations: computed once, shared, read-only."""
    Y, prior, _ = inputs(C, S, T)
    B_in = None if from_identity else two_iterations(C, S, T, Lb, Lc)
    _, _, Bn, d = cg.cacgmm_step(Y, prior, B_in, S, Lb, Lc, LOADING)
    cond = np.ones(Bn.shape[:3]) if B_in is None else np.linalg.cond(B_in)
    for a in (Bn, cond, d["A"], d["l_abs_max"], d["l_terms_max"]):
        a.setflags(write=False)
    return B_in, Bn, cond, d


def gate_posteriors(impl, C, S, gi, iterations, B_in=None):
    """-> (ok, the largest |mask - gamma| / (2^-23 gamma + 2^-149), mask, B)."""
    T, Lb, Lc = GEOMETRIES[gi]
    Y, prior, _ = inputs(C, S, T)
    mask, B = impl(Y, prior, S, iterations, Lb, Lc, LOADING, B_in)
    assert mask.shape == (T, S * F) and mask.dtype == np.float32 and B.shape == (cg.num_blocks(T, Lb), S, F, C, C)
    gamma = cg.cacgmm_posteriors(Y, prior, B if iterations else B_in, S, Lb)
    err = np.abs(mask.astype(np.float64) - gamma)
    bound = 2.0 ** -23 * gamma + 2.0 ** -149
    ok = bool(np.isfinite(mask).all() and np.all(err <= bound))
    return ok, float(np.max(err / bound)), mask, B


def gate_one_step(impl, C, S, gi, from_identity):
    """-> (ok, the largest |B - B_ref| / gate)."""
    T, Lb, Lc = GEOMETRIES[gi]
    Y, prior, _ = inputs(C, S, T)
    B_in, Bn, cond, d = reference_step(C, S, T, Lb, Lc, from_identity)
    assert float(np.max(cond)) <= cond_bound(C, LOADING)
    assert np.all(d["l_terms_max"] <= 4.0 * d["l_abs_max"])
    _, B = impl(Y, prior, S, 1, Lb, Lc, LOADING, B_in)
    lw = np.array([w1 - w0 for _, _, w0, w1 in (cg.block_window(j, T, Lb, Lc) for j in range(Bn.shape[0]))], dtype=np.float64)
    gate = 2.0 ** -52 * (lw[:, None, None] + C1 * C * C * cond + C2 * d["l_abs_max"][:, None, None])[..., None, None] * d["A"].real
    err = np.abs(B - Bn)
    ok = bool(np.isfinite(B.view(np.float64)).all() and np.all(err <= gate))
    with np.errstate(all="ignore"):
        ratio = float(np.max(np.where(gate > 0, err / gate, np.where(err > 0, np.inf, 0.0))))
    return ok, ratio


def gate_chaining(impl, C, S, gi):
    """-> ok."""
    T, Lb, Lc = GEOMETRIES[gi]
    Y, prior, _ = inputs(C, S, T)
    mask3, B3 = impl(Y, prior, S, 3, Lb, Lc, LOADING, None)
    B, mask = None, None
    for _ in range(3):
        mask, B = impl(Y, prior, S, 1, Lb, Lc, LOADING, B)
    mask0, B0 = impl(Y, prior, S, 0, Lb, Lc, LOADING, B3)
    return (mask3.tobytes() == mask.tobytes() and B3.tobytes() == B.tobytes() and mask0.tobytes() == mask3.tobytes()
            and B0.tobytes() == B3.tobytes())
