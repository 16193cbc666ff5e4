"""Mask-based MVDR beamforming of a multi-channel recording: the definition, in numpy.

The continuous-speech-separation recipes (Yoshioka et al. 2018; LibriCSS, Chen et al. 2020) do not stop at masking one
microphone: the network's masks weight the spatial covariance matrices of each separated stream and of everything else, and
an MVDR beamformer per stream is steered from them (Heymann et al. 2016; the reference-channel form of Souden et al. 2010,
which needs no steering vector).  This file states what sk_mvdr (include/sepkern.h, csrc/mvdr.hip) computes and restates it
in numpy; tests/test_gpu_mvdr.py holds the kernels to it.

Inputs.  Y[c][t][f], complex64 spectra of C channels (2 <= C <= 8, F = 257 bins); m_s[t][f] = mask[t][s F + f], float32, the
stitched mask of S streams (2 <= S <= 4); a block length Lb >= 1 frames, a context of R >= 0 blocks, a reference channel ref
and a diagonal loading delta >= 0.

Blocks.  nblk = ceil(T / Lb); block j holds frames [j Lb, min(T, (j + 1) Lb)).

Block statistics.  A_j[s][f] = sum_t m_s[t, f] y y^H with y = Y[:, t, f], t ascending over the block, every operand widened
to fp64 first.  Hermitian: the upper triangle is computed, the lower one is its conjugate, the diagonal is real.

Context.  PHI_s[j][f] = sum of A_j'[s][f] over j' in [max(0, j - R), min(nblk - 1, j + R)], j' ascending.  R >= nblk - 1 gives
one time-invariant beamformer for the whole recording.

Noise.  N_s = sum_{s' != s} PHI_s', s' ascending (summed, not total minus own), then N_s += (delta Re tr N_s / C) I.  Nothing
is normalised by the masks' sums: the weights below do not change with it.

Weights.  G = N_s^-1 PHI_s, d = Re tr G, W_s[j][f] = G[:, ref] / d.  W_s[j][f] = e_ref (the reference channel passed through)
where Re tr PHI_s == 0, Re tr N_s == 0 (before the loading) or not d > 1e-12.  The solves are an fp64 Cholesky factorisation
N = U^H U and two triangular solves per column of PHI_s; a matrix that is not positive definite gives NaN and with it the
fallback.  The weights are rounded to complex64, laid out (nblk, S, F, C).

Apply.  Z_s[t][f] = sum_c conj(W_s[block(t)][f][c]) Y[c][t][f]: fp32 arithmetic, c ascending, complex64, laid out (S, T, F).

With delta > 0 every N_s that is not zero has a condition number of at most C / delta + 1, however short or silent the block:
N is positive semi-definite, so its eigenvalues lie in [delta tr / C, tr (1 + delta / C)].

Out of the definition, on purpose: S = 1 (which needs a noise class), smoothing of the weights across block edges, the GEV and
rank-1 variants, dereverberation (WPE).  Masks re-estimated from all channels before they steer the beamformers are a stage of
their own in front of this one: sepkern/cacgmm.py (sk_cacgmm).
"""
import numpy as np

from .wpe import num_blocks  # noqa: F401  (one rule for the blocks of all four array kernels)

F = 257
MIN_C, MAX_C = 2, 8
MIN_S, MAX_S = 2, 4
D_MIN = 1e-12


def check_arguments(C, S, T, block_frames, context_blocks, ref, loading):
    if not MIN_C <= C <= MAX_C:
        raise ValueError("mvdr: C = %d channels outside %d..%d" % (C, MIN_C, MAX_C))
    if not MIN_S <= S <= MAX_S:
        raise ValueError("mvdr: S = %d streams outside %d..%d" % (S, MIN_S, MAX_S))
    if T < 1 or block_frames < 1 or context_blocks < 0:
        raise ValueError("mvdr: T = %d frames, blocks of %d frames, a context of %d blocks" % (T, block_frames, context_blocks))
    if not 0 <= ref < C:
        raise ValueError("mvdr: reference channel %d outside [0, %d)" % (ref, C))
    if not loading >= 0.0:
        raise ValueError("mvdr: loading %r is negative or NaN" % (loading,))


def block_statistics(Y, mask, S, block_frames):
    """A (nblk, S, F, C, C) complex128."""
    C, T = Y.shape[0], Y.shape[1]
    nblk = num_blocks(T, block_frames)
    y = np.ascontiguousarray(np.transpose(Y[:, :, :F], (1, 2, 0))).astype(np.complex128)        # (T, F, C)
    m = mask[:T, :S * F].astype(np.float64).reshape(T, S, F)
    upper = np.triu(np.ones((C, C), dtype=bool), 1)
    A = np.zeros((nblk, S, F, C, C), dtype=np.complex128)
    for j in range(nblk):
        for t in range(j * block_frames, min(T, (j + 1) * block_frames)):
            p = y[t, :, :, None] * np.conj(y[t, :, None, :])                                    # (F, C, C): y y^H
            for s in range(S):
                A[j, s] = A[j, s] + m[t, s, :, None, None] * p
    up = np.where(upper, A, 0.0)
    diag = np.zeros_like(A)
    for a in range(C):
        diag[..., a, a] = A[..., a, a].real
    return up + np.conj(np.swapaxes(up, -1, -2)) + diag


def context_sum(A, context_blocks):
    nblk = A.shape[0]
    scm = np.zeros_like(A)
    for j in range(nblk):
        for jj in range(max(0, j - context_blocks), min(nblk - 1, j + context_blocks) + 1):
            scm[j] = scm[j] + A[jj]
    return scm


def noise_matrices(scm, loading):
    """N (nblk, S, F, C, C) with the loading on the diagonal, and Re tr N before the loading."""
    S, C = scm.shape[1], scm.shape[-1]
    N = np.zeros_like(scm)
    for s in range(S):
        for o in range(S):
            if o != s:
                N[:, s] = N[:, s] + scm[:, o]
    tr = np.zeros(N.shape[:3], dtype=np.float64)
    for a in range(C):
        tr = tr + N[..., a, a].real
    load = loading * tr / C
    for a in range(C):
        N[..., a, a] = N[..., a, a].real + load
    return N, tr


def cholesky_solve(N, P):
    """G = N^-1 P for stacks (..., C, C) of Hermitian matrices through N = U^H U; NaN where N is not positive definite.  Only
    the upper triangles are read."""
    C = N.shape[-1]
    U = np.zeros_like(N)
    rinv = np.zeros(N.shape[:-2] + (C,), dtype=np.float64)
    with np.errstate(all="ignore"):
        for a in range(C):
            dd = N[..., a, a].real.copy()
            for k in range(a):
                dd = dd - (U[..., k, a].real ** 2 + U[..., k, a].imag ** 2)
            rinv[..., a] = 1.0 / np.sqrt(dd)
            for b in range(a + 1, C):
                v = N[..., a, b].copy()
                for k in range(a):
                    v = v - np.conj(U[..., k, a]) * U[..., k, b]
                U[..., a, b] = v * rinv[..., a]
        G = np.zeros_like(N)
        for k in range(C):
            z = np.zeros(N.shape[:-2] + (C,), dtype=np.complex128)
            for a in range(C):
                v = (P[..., a, k] if a <= k else np.conj(P[..., k, a])).copy()
                for i in range(a):
                    v = v - np.conj(U[..., i, a]) * z[..., i]
                z[..., a] = v * rinv[..., a]
            for a in range(C - 1, -1, -1):
                v = z[..., a].copy()
                for i in range(a + 1, C):
                    v = v - U[..., a, i] * G[..., i, k]
                G[..., a, k] = v * rinv[..., a]
    return G


def mvdr_weights(scm, ref, loading):
    """(nblk, S, F, C) complex64 weights of the context-summed matrices scm (nblk, S, F, C, C), and d, NaN where the fallback
    applies."""
    C = scm.shape[-1]
    N, trN = noise_matrices(scm, loading)
    trP = np.zeros(scm.shape[:3], dtype=np.float64)
    for a in range(C):
        trP = trP + scm[..., a, a].real
    G = cholesky_solve(N, scm)
    d = np.zeros(scm.shape[:3], dtype=np.float64)
    for a in range(C):
        d = d + G[..., a, a].real
    with np.errstate(all="ignore"):
        fallback = (trP == 0.0) | (trN == 0.0) | ~(d > D_MIN)
        W = G[..., :, ref] / d[..., None]
    e_ref = np.zeros(C, dtype=np.complex128)
    e_ref[ref] = 1.0
    W[fallback] = e_ref
    return W.astype(np.complex64), np.where(fallback, np.nan, d)


def apply_weights(Y, W, block_frames):
    """Z (S, T, F) complex64 in fp32 arithmetic, c ascending."""
    C, T = Y.shape[0], Y.shape[1]
    S = W.shape[1]
    blk = np.arange(T) // block_frames
    Z = np.zeros((S, T, F), dtype=np.complex64)
    for s in range(S):
        for c in range(C):
            Z[s] = Z[s] + np.conj(W[blk, s, :, c]) * Y[c, :, :F].astype(np.complex64)
    return Z


def mvdr_reference(Y, mask, S, block_frames, context_blocks, ref, loading):
    """Y (C, T, >= F) complex64, mask (T, >= S F) float32 -> (scm (nblk, S, F, C, C) complex128: the context-summed PHI_s before
    any loading, weights (nblk, S, F, C) complex64, Z (S, T, F) complex64)."""
    Y, mask = np.asarray(Y), np.asarray(mask)
    C, T = Y.shape[0], Y.shape[1]
    check_arguments(C, S, T, block_frames, context_blocks, ref, loading)
    if mask.shape[0] < T or mask.shape[1] < S * F or Y.shape[2] < F:
        raise ValueError("mvdr: Y must be (C, T, >= 257), mask (>= T, >= S * 257)")
    scm = context_sum(block_statistics(Y, mask, S, block_frames), context_blocks)
    W, _ = mvdr_weights(scm, ref, loading)
    return scm, W, apply_weights(Y, W, block_frames)


def workspace_bytes(T, C, S, block_frames):
    """Bytes of the block statistics sk_mvdr keeps between its first two launches: nblk S C (C + 1) / 2 complex128 per bin."""
    return num_blocks(T, block_frames) * S * (C * (C + 1) // 2) * 2 * F * 8
