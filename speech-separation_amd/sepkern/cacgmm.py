"""Mask-guided spatial clustering of a multi-channel recording with a cACGMM: the definition, in numpy.

The network's masks have seen one microphone.  The far-field recipes put a spatial mixture model between the mask estimator
and the beamformer, which re-estimates the masks from all channels: the complex angular central Gaussian mixture model
(cACGMM) of Ito et al. 2016 on the direction y / |y| of every time-frequency point, with the network's masks as the class
prior at every point (Nakatani et al. 2017; the "guided source separation" of the CHiME-5/6 front ends, Boeddeker et al.
2018).  Anchored like that the model sharpens the masks from the inter-channel evidence, cannot permute streams across bins
or blocks, and needs no training.  This file states what sk_cacgmm (include/sepkern.h, csrc/cacgmm.hip) computes and restates
it in numpy fp64; tests/test_gpu_cacgmm.py holds the kernel to it.

UNPINNED, the way sepkern/stoi.py and sepkern/wpe.py are: no third-party implementation (pb_bss) is installed to compare
against; the tests hold the definition to closed forms, invariances and a refinement check of its own.

Inputs.  Y[c][t][f], complex64 spectra of C channels (2 <= C <= 8, F = 257 bins; this may be sk_wpe's X); m_k[t][f] =
prior[t][k F + f], float32, the stitched masks of K = S streams (2 <= S <= 4); I iterations, 0 <= I <= 16; a block length
Lb >= 1 frames, a context of Lc >= 0 frames, Lb + 2 Lc <= 4096; a relative diagonal loading delta >= 0; optionally an initial
state B_in (nblk, S, F, C, C) complex128 of which only the upper triangle and the real part of the diagonal are read.

Blocks and windows (sk_wpe's rule).  nblk = ceil(T / Lb); block j holds frames [j Lb, min(T, (j + 1) Lb)); its window is
[max(0, j Lb - Lc), min(T, (j + 1) Lb + Lc)).  Every (block, bin) is an independent problem on its window, and only the block's
own frames are written from it.

Per (block, bin), every operand widened to fp64 first:
    n(t) = sum_c |y_c(t)|^2, c ascending.  A frame with n(t) == 0 is DEAD; otherwise z(t) = y(t) / sqrt(n(t)).
    p_k(t) = max(m_k, 1e-6) / sum_k' max(m_k', 1e-6), k' ascending.  Fixed over the iterations: this is the guide -- the class
             weights are the network's masks, not learned mixture weights.
    State: one Hermitian B_k per class; B_k = I at the start, or B_in.  A state is ADMITTED before it is used: B_k is
             factorised, B_k = U^H U, and class k is RESET to B_k = I where a pivot is not > 0 or not finite or an entry of U
             is not finite.  (An updated state is reset where n_k == 0 as well, below.)
    One pass with the state B, for every live frame:
        q_k(t) = || U_k^-H z(t) ||^2 by forward substitution, summed a ascending
        l_k(t) = (log p_k(t) - 2 sum_a log U_k[a][a]) - C log q_k(t)
        gamma_k(t) = e_k / sum_k' e_k', e_k = exp(l_k - max_k' l_k'), k' ascending
      Dead frames get gamma_k(t) = p_k(t) and take part in no sum.  While EVERY class of the cell is at the identity (bit for
      bit: the start without B_in, or after resets) the pass is the closed form q_k(t) = 1, gamma_k(t) = p_k(t).
    Update (the M-step of the same pass; q is that of the old B, as in Ito et al.):
        n_k = sum_t gamma_k(t);  S_k = sum_t (gamma_k(t) / q_k(t)) z z^H, t ascending over the window's live frames (upper
        triangle; the diagonal is real);  B_k' = S_k (C / n_k);  then B_k' += (delta Re tr B_k' / C) I;  B_k' is admitted as
        above, and reset where n_k == 0.
    `iterations` passes with update; then one last pass without update, over the block's own frames, writes
        mask_out[t][k F + f] = float32(gamma_k(t));   B_out[j][k][f] = the last state, a full Hermitian matrix, complex128.

Consequences.  With I = 0 and no B_in the output is float32(p).  With B = I the first pass has q = 1 and gamma = p, so one step
from the identity is B_k' = C sum_t p_k z z^H / sum_t p_k plus the loading.  The model is invariant to the scale of B (log det
and C log q cancel) and to any complex scalar on y(t) (z z^H does not see it); a power of two on y(t) changes no bit.  An
all-dead window gives p and B = I.

Conditioning.  S_k is positive semi-definite, so with delta > 0 the eigenvalues of an updated B_k lie in
[delta tr / C, tr (1 + delta / C)] and cond(B_k) <= C / delta + 1 -- sepkern/mvdr.py's argument for N_s.

Arithmetic.  Real fp64 arithmetic with one rounding per product and per sum (no fused multiply-adds), a complex product being
its four real products and two sums; every sum has one order, stated where it is coded below.  The kernel performs the same
operations in the same order; log and exp are the platform's (numpy's here, the device library's there).

Out of the definition, on purpose: a noise class (sk_mvdr would have to accept a class it sums into N_s but does not beamform),
learned mixture weights, permutation alignment across bins (the prior makes it unnecessary), S = 1, and any tuning of the
iterations, blocks and loading: no array data is at hand.
"""
import numpy as np

from .wpe import block_window, num_blocks  # noqa: F401  (the window rule is sk_wpe's)

F = 257
MIN_C, MAX_C = 2, 8
MIN_S, MAX_S = 2, 4
MAX_ITERATIONS = 16
MAX_WINDOW = 4096
PRIOR_FLOOR = 1e-6


def check_arguments(C, S, T, iterations, block_frames, context_frames, loading, ld_prior=None, ld_out=None, y_row_stride=None,
                    have_Y=True, have_prior=True, have_mask_out=True):
    """Raises ValueError, naming the argument, for everything sk_cacgmm answers with SK_EINVAL."""
    if not MIN_C <= C <= MAX_C:
        raise ValueError("cacgmm: C = %d channels outside %d..%d" % (C, MIN_C, MAX_C))
    if not MIN_S <= S <= MAX_S:
        raise ValueError("cacgmm: S = %d streams outside %d..%d" % (S, MIN_S, MAX_S))
    if T < 1:
        raise ValueError("cacgmm: T = %d frames, at least 1 expected" % T)
    if not 0 <= iterations <= MAX_ITERATIONS:
        raise ValueError("cacgmm: iterations = %d outside 0..%d" % (iterations, MAX_ITERATIONS))
    if block_frames < 1:
        raise ValueError("cacgmm: block_frames = %d, at least 1 expected" % block_frames)
    if context_frames < 0:
        raise ValueError("cacgmm: context_frames = %d is negative" % context_frames)
    if block_frames + 2 * context_frames > MAX_WINDOW:
        raise ValueError("cacgmm: a window of block_frames + 2 context_frames = %d frames, at most %d"
                         % (block_frames + 2 * context_frames, MAX_WINDOW))
    if not loading >= 0.0:
        raise ValueError("cacgmm: loading %r is negative or NaN" % (loading,))
    if ld_prior is not None and ld_prior < S * F:
        raise ValueError("cacgmm: ld_prior = %d below S*257 = %d" % (ld_prior, S * F))
    if ld_out is not None and ld_out < S * F:
        raise ValueError("cacgmm: ld_out = %d below S*257 = %d" % (ld_out, S * F))
    if y_row_stride is not None and y_row_stride < F:
        raise ValueError("cacgmm: y_row_stride = %d below 257" % y_row_stride)
    if not (have_Y and have_prior and have_mask_out):
        raise ValueError("cacgmm: null pointer (Y, prior or mask_out)")


def workspace_bytes(T, C, S, block_frames, context_frames):
    """Bytes of device workspace sk_cacgmm needs: none -- the state, its factors and a chunk of frames live in a workgroup's LDS."""
    return 0


def directions(Y, t0, t1):
    """z(t) of frames [t0, t1): -> (zr, zi (L, F, C) fp64, zero on dead frames; live (L, F) bool)."""
    y = np.ascontiguousarray(np.transpose(Y[:, t0:t1, :F], (1, 2, 0)))                    # (L, F, C) complex64
    yr, yi = y.real.astype(np.float64), y.imag.astype(np.float64)
    n = np.zeros(yr.shape[:2])
    for c in range(yr.shape[2]):
        n = n + (yr[:, :, c] * yr[:, :, c] + yi[:, :, c] * yi[:, :, c])
    live = n != 0.0
    s = np.sqrt(np.where(live, n, 1.0))[:, :, None]
    return np.where(live[:, :, None], yr / s, 0.0), np.where(live[:, :, None], yi / s, 0.0), live


def prior_weights(prior, S, t0, t1):
    """p_k(t) of frames [t0, t1): (L, S, F) fp64."""
    m = np.maximum(np.asarray(prior)[t0:t1, :S * F].astype(np.float64).reshape(t1 - t0, S, F), PRIOR_FLOOR)
    tot = np.zeros((t1 - t0, F))
    for k in range(S):
        tot = tot + m[:, k]
    return m / tot[:, None, :]


def hermitian(B):
    """The full Hermitian matrices of the upper triangles and real diagonals of B (..., C, C)."""
    C = B.shape[-1]
    up = np.where(np.triu(np.ones((C, C), dtype=bool), 1), B, 0.0)
    out = up + np.conj(np.swapaxes(up, -1, -2))
    for a in range(C):
        out[..., a, a] = B[..., a, a].real
    return out


def admit(B, extra_reset=None):
    """Factorise a state B (S, F, C, C) = U^H U and reset the classes that fail (or that extra_reset (S, F) marks) to I.
    -> dict(B: the admitted state, full Hermitian; Ur, Ui: the strictly upper part of U; rinv (S, F, C) = 1 / U[a][a];
    sld (S, F) = sum_a log U[a][a], a ascending; reset (S, F) bool; ident (F,) bool: every class of the bin is the identity).
    An entry of U loses its products k ascending and is then scaled by 1 / U[a][a]."""
    B = hermitian(np.asarray(B, dtype=np.complex128))
    C = B.shape[-1]
    Br, Bi = B.real, B.imag
    Ur, Ui = np.zeros(Br.shape), np.zeros(Br.shape)
    rinv, sld = np.zeros(Br.shape[:-1]), np.zeros(Br.shape[:-2])
    ok = np.ones(Br.shape[:-2], dtype=bool)
    with np.errstate(all="ignore"):
        for a in range(C):
            vr, vi = Br[..., a, a:].copy(), Bi[..., a, a:].copy()
            for k in range(a):                                       # - conj(U[k][a]) U[k][b]
                ur, ui, br, bi = Ur[..., k, a, None], Ui[..., k, a, None], Ur[..., k, a:], Ui[..., k, a:]
                vr -= ur * br + ui * bi
                vi -= ur * bi - ui * br
            dd = vr[..., 0]
            ok &= (dd > 0.0) & np.isfinite(dd)
            uaa = np.sqrt(dd)
            rinv[..., a] = 1.0 / uaa
            sld = sld + np.log(uaa)
            Ur[..., a, a + 1:], Ui[..., a, a + 1:] = vr[..., 1:] * rinv[..., a, None], vi[..., 1:] * rinv[..., a, None]
        ok &= np.isfinite(Ur).all(axis=(-2, -1)) & np.isfinite(Ui).all(axis=(-2, -1))
    reset = ~ok if extra_reset is None else (~ok | extra_reset)
    eye = np.eye(C)
    B = np.where(reset[..., None, None], eye, B)
    Ur, Ui = np.where(reset[..., None, None], 0.0, Ur), np.where(reset[..., None, None], 0.0, Ui)
    rinv, sld = np.where(reset[..., None], 1.0, rinv), np.where(reset, 0.0, sld)
    ident = (B == eye).all(axis=(-2, -1)).all(axis=0)
    return dict(B=B, Ur=Ur, Ui=Ui, rinv=rinv, sld=sld, reset=reset, ident=ident)


def e_step(zr, zi, live, p, st):
    """One pass over frames: zr, zi (L, F, C), live (L, F), p (L, S, F), st = admit(B).  -> (gamma, q, l: (L, S, F)); dead
    frames have gamma = p, q = 1, l = 0; so have the bins whose classes are all at the identity, but for l = log p."""
    L, S, C = p.shape[0], p.shape[1], zr.shape[2]
    q, l = np.zeros(p.shape), np.zeros(p.shape)
    with np.errstate(all="ignore"):
        for k in range(S):
            xr, xi = np.zeros(zr.shape), np.zeros(zr.shape)
            qk = np.zeros((L, F))
            for a in range(C):
                vr, vi = zr[:, :, a].copy(), zi[:, :, a].copy()
                for i in range(a):                                   # - conj(U[i][a]) x[i]
                    ur, ui = st["Ur"][k, None, :, i, a], st["Ui"][k, None, :, i, a]
                    vr -= ur * xr[:, :, i] + ui * xi[:, :, i]
                    vi -= ur * xi[:, :, i] - ui * xr[:, :, i]
                xr[:, :, a], xi[:, :, a] = vr * st["rinv"][k, None, :, a], vi * st["rinv"][k, None, :, a]
                qk = qk + (xr[:, :, a] * xr[:, :, a] + xi[:, :, a] * xi[:, :, a])
            q[:, k] = qk
            l[:, k] = (np.log(p[:, k]) - 2.0 * st["sld"][k][None]) - C * np.log(qk)
        lmax = l.max(axis=1)
        e = np.exp(l - lmax[:, None])
        tot = np.zeros((L, F))
        for k in range(S):
            tot = tot + e[:, k]
        gamma = e / tot[:, None]
    closed = ~live | st["ident"][None]
    keep = closed[:, None, :]
    return np.where(keep, p, gamma), np.where(keep, 1.0, q), np.where(keep, np.where(live[:, None, :], np.log(p), 0.0), l)


def m_step(zr, zi, live, gamma, q, loading):
    """The update from one window: -> admit(B') with Bu = B' before admission and n (S, F) besides.  (w z_a) conj(z_b) =
    (pr qr + pi qi) + i (pi qr - pr qi), t ascending; a dead frame adds zeros."""
    L, S, C = gamma.shape[0], gamma.shape[1], zr.shape[2]
    tf = lambda a: np.ascontiguousarray(np.transpose(a, (0, 2, 1)))                      # bins innermost: (L, C, F)
    zrt, zit = tf(zr), tf(zi)
    g = np.where(live[:, None, :], gamma, 0.0)
    w = np.where(live[:, None, :], gamma / q, 0.0)
    n = np.zeros((S, F))
    Sr, Si = np.zeros((S, C, C, F)), np.zeros((S, C, C, F))
    for t in range(L):
        n += g[t]
        qr, qi = zrt[t][None, None], zit[t][None, None]                                  # (1, 1, C, F): columns b
        pr, pi = zrt[t][None, :, None] * w[t][:, None, None], zit[t][None, :, None] * w[t][:, None, None]   # (S, C, 1, F)
        Sr += pr * qr + pi * qi
        Si += pi * qr - pr * qi
    with np.errstate(all="ignore"):
        cs = (C / n)[:, None, None]
        Br, Bi = Sr * cs, Si * cs
        tr = np.zeros((S, F))
        for a in range(C):
            tr = tr + Br[:, a, a]
        load = loading * tr / C
        for a in range(C):
            Br[:, a, a] = Br[:, a, a] + load
    Bu = hermitian(np.transpose(Br + 1j * Bi, (0, 3, 1, 2)))
    st = admit(Bu, extra_reset=(n == 0.0))
    st.update(Bu=Bu, n=n)
    return st


def _check_inputs(Y, prior, S):
    Y, prior = np.asarray(Y), np.asarray(prior)
    if Y.ndim != 3 or Y.shape[2] < F or Y.dtype != np.complex64:
        raise ValueError("cacgmm: Y must be (C, T, >= 257) complex64")
    if prior.ndim != 2 or prior.shape[0] < Y.shape[1] or prior.shape[1] < S * F or prior.dtype != np.float32:
        raise ValueError("cacgmm: prior must be (>= T, >= S*257) float32")
    return Y, prior


def _state(B, nblk, S, C):
    if B is None:
        return np.broadcast_to(np.eye(C, dtype=np.complex128), (nblk, S, F, C, C))
    B = np.asarray(B)
    if B.shape != (nblk, S, F, C, C):
        raise ValueError("cacgmm: the state must be (nblk, S, 257, C, C)")
    return B


def cacgmm_step(Y, prior, B, S, block_frames, context_frames, loading):
    """One pass with update from the state B (nblk, S, F, C, C) or None for the identity.  -> (gamma, q: lists of the blocks'
    (Lw, S, F) arrays over their windows, B' (nblk, S, F, C, C), details dict(l_abs_max (nblk,): the largest |l_k(t)|,
    l_terms_max (nblk,): the largest |log p| + 2 |sum_a log U[a][a]| + C |log q|, n (nblk, S, F), A (nblk, S, F, C, C) =
    C sum_t gamma_k |z_a| |z_b| / q_k / n_k: the sum of the magnitudes B' is made of, Bu: B' before admission))."""
    Y, prior = _check_inputs(Y, prior, S)
    C, T = Y.shape[0], Y.shape[1]
    check_arguments(C, S, T, 1, block_frames, context_frames, loading)
    nblk = num_blocks(T, block_frames)
    B = _state(B, nblk, S, C)
    gammas, qs = [], []
    Bn, Bu, A = (np.zeros((nblk, S, F, C, C), dtype=np.complex128) for _ in range(3))
    nn, lmax, ltmax = np.zeros((nblk, S, F)), np.zeros(nblk), np.zeros(nblk)
    for j in range(nblk):
        _, _, w0, w1 = block_window(j, T, block_frames, context_frames)
        zr, zi, live = directions(Y, w0, w1)
        p = prior_weights(prior, S, w0, w1)
        old = admit(B[j])
        gamma, q, l = e_step(zr, zi, live, p, old)
        st = m_step(zr, zi, live, gamma, q, loading)
        gammas.append(gamma)
        qs.append(q)
        terms = np.abs(np.log(p)) + 2.0 * np.abs(old["sld"])[None] + C * np.abs(np.log(q))
        Bn[j], Bu[j], nn[j], lmax[j] = st["B"], st["Bu"], st["n"], np.max(np.abs(l))
        ltmax[j] = np.max(np.where(live[:, None, :], terms, 0.0))
        za = np.sqrt(zr * zr + zi * zi)
        with np.errstate(all="ignore"):
            w = np.where(live[:, None, :], gamma / q, 0.0)
            A[j] = C * np.einsum("tkf,tfa,tfb->kfab", w, za, za) / st["n"][:, :, None, None]
    return gammas, qs, Bn, dict(l_abs_max=lmax, l_terms_max=ltmax, n=nn, A=A, Bu=Bu)


def cacgmm_posteriors(Y, prior, B, S, block_frames, details=False):
    """The last pass alone: gamma (T, S*F) fp64 of every frame under its block's state B (nblk, S, F, C, C) or None; with
    details also l (T, S, F)."""
    Y, prior = _check_inputs(Y, prior, S)
    C, T = Y.shape[0], Y.shape[1]
    nblk = num_blocks(T, block_frames)
    B = _state(B, nblk, S, C)
    out, ls = np.zeros((T, S * F)), np.zeros((T, S, F))
    for j in range(nblk):
        b0, b1, _, _ = block_window(j, T, block_frames, 0)
        zr, zi, live = directions(Y, b0, b1)
        gamma, _, l = e_step(zr, zi, live, prior_weights(prior, S, b0, b1), admit(B[j]))
        out[b0:b1], ls[b0:b1] = gamma.reshape(b1 - b0, S * F), l
    return (out, ls) if details else out


def cacgmm_reference(Y, prior, S, iterations, block_frames, context_frames, loading, B_in=None):
    """Y (C, T, >= F) complex64, prior (>= T, >= S F) float32 -> (mask (T, S F) float32, B (nblk, S, F, C, C) complex128,
    details dict(states: the admitted state after B_in and after every iteration, iterations + 1 arrays like B; gamma (T, S F)
    fp64: the posteriors before their rounding))."""
    Y, prior = _check_inputs(Y, prior, S)
    C, T = Y.shape[0], Y.shape[1]
    check_arguments(C, S, T, iterations, block_frames, context_frames, loading)
    nblk = num_blocks(T, block_frames)
    B = np.stack([admit(Bj)["B"] for Bj in _state(B_in, nblk, S, C)])
    states = [B]
    for _ in range(iterations):
        B = cacgmm_step(Y, prior, B, S, block_frames, context_frames, loading)[2]
        states.append(B)
    gamma = cacgmm_posteriors(Y, prior, B, S, block_frames)
    return gamma.astype(np.float32), B, dict(states=states, gamma=gamma)
