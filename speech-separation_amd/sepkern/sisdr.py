"""SI-SDR (Le Roux et al. 2019), zero-mean, best speaker permutation.

The reference scores BSS-eval SDR with mir_eval (steps/evaluate_sources.py:57); SI-SDR is the
metric BASELINE.json's parity gate names, computed identically for both sides of a comparison.
"""
import itertools

import numpy as np


def si_sdr(est, ref):
    est = np.asarray(est, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    est = est - est.mean()
    ref = ref - ref.mean()
    alpha = np.dot(est, ref) / (np.dot(ref, ref) + 1e-30)
    target = alpha * ref
    noise = est - target
    return 10.0 * np.log10((np.dot(target, target) + 1e-30) / (np.dot(noise, noise) + 1e-30))


def si_sdr_best_perm(ests, refs):
    S = len(refs)
    return max(float(np.mean([si_sdr(ests[s], refs[p[s]]) for s in range(S)]))
               for p in itertools.permutations(range(S)))


# ------------------------------------------------------------------------------------------------ the training loss
# Host restatement (numpy fp64) of the SI-SDR uPIT loss the kernels compute (include/sepkern.h "SI-SDR uPIT loss",
# DESIGN section 13): the documentation of their arithmetic, and what tests/test_sisdr_loss.py pins against autograd.
EPS = 1e-30
KAPPA = 10.0 / np.log(10.0)


def _hann(n_fft):
    n = np.arange(n_fft, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / n_fft)).astype(np.float32).astype(np.float64)    # the library's float32 table


def _inner(e, r):
    """The plain sums -> zero-mean a = <e~,r~>, b = <r~,r~>, c = <e~,e~> and the two means."""
    n = float(e.shape[0])
    se, sr = e.sum(), r.sum()
    return np.dot(e, r) - se * sr / n, np.dot(r, r) - sr * sr / n, np.dot(e, e) - se * se / n, se / n, sr / n


def pit_si_sdr(ests, refs, count=1.0):
    """Utterance-level PIT on SI-SDR for ONE utterance: ests, refs = S waveforms each (equal lengths) ->
    dict(loss = -best score / count, pair (S,S) dB with pair[k][i] = SI-SDR(e_k, r_i), perm_score (S!) in
    itertools.permutations order, best_perm = arg-max (first maximum), coef (S,3): d loss / d e_k[n] = A e_k[n] + B r_i[n] + C
    with i the best permutation's reference for k).  A pair with b <= 0, a == 0 or c - a^2/b <= 0 (silent reference, exact
    copy) keeps its finite eps value in `pair` and gets zero coefficients."""
    S = len(refs)
    ests = [np.asarray(e, dtype=np.float64) for e in ests]
    refs = [np.asarray(r, dtype=np.float64) for r in refs]
    pair = np.zeros((S, S))
    for k in range(S):
        for i in range(S):
            a, b, c, _, _ = _inner(ests[k], refs[i])
            tt = (a / b) * a if b > 0.0 else 0.0
            pair[k, i] = 10.0 * np.log10((tt + EPS) / (max(c - tt, 0.0) + EPS))
    perms = list(itertools.permutations(range(S)))
    score = np.array([sum(pair[k, p[k]] for k in range(S)) / S for p in perms])
    best = int(np.argmax(score))                                  # first maximum
    coef = np.zeros((S, 3))
    m = -1.0 / (float(count) * S)
    for k in range(S):
        a, b, c, mue, mur = _inner(ests[k], refs[perms[best][k]])
        if b > 0.0 and a != 0.0:
            den = c - (a / b) * a
            if den > 0.0:
                P, Q = -2.0 * KAPPA / den, KAPPA * (2.0 / a + 2.0 * a / (b * den))
                coef[k] = m * P, m * Q, -m * (P * mue + Q * mur)
    return dict(loss=-score[best] / float(count), pair=pair, perm_score=score, best_perm=best, coef=coef)


def istft_adjoint_mask_grad(mix_spec, g, hop=128):
    """Adjoint of mask -> oracle.stft.istft(mix_spec * mask): mix_spec (F, T) complex, g (hop (T-1),) = d loss / d estimate ->
    d loss / d mask (F, T) real.  g is placed at offset n_fft/2 of a zero signal of length n_fft + hop (T-1), divided by the
    window-sum-square, framed WITHOUT reflection and transformed (windowed forward DFT) to U;
    dmask[f,t] = (c_f / n_fft) (Re X Re U + Im X Im U), c_f = 1 for the DC and Nyquist bins (whose imaginary parts the inverse
    real FFT ignores), 2 otherwise."""
    X = np.asarray(mix_spec, dtype=np.complex128)
    F, T = X.shape
    n_fft = 2 * (F - 1)
    win = _hann(n_fft)
    n = n_fft + hop * (T - 1)
    wss = np.zeros(n)
    for t in range(T):
        wss[t * hop:t * hop + n_fft] += win * win
    gp = np.zeros(n)
    gp[n_fft // 2:n - n_fft // 2] = np.asarray(g, dtype=np.float64)
    gp = np.where(wss > np.finfo(np.float32).tiny, gp / np.where(wss > 0, wss, 1.0), gp)
    idx = np.arange(n_fft)[None, :] + hop * np.arange(T)[:, None]
    U = np.fft.rfft(gp[idx] * win[None, :], axis=1).T              # (F, T)
    cf = np.full((F, 1), 2.0)
    cf[0, 0] = cf[F - 1, 0] = 1.0
    return cf / n_fft * (X.real * U.real + X.imag * U.imag)
