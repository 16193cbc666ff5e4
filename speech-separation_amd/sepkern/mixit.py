"""Mixture-invariant training loss (MixIT; Wisdom et al., "Unsupervised sound separation using mixtures of mixtures",
NeurIPS 2020), numpy fp64: the definition of loss=mixit (archs/uPIT.py) and of the arithmetic the kernels do
(include/sepkern.h "mixture-invariant loss", csrc/mixit.hip, sk_mixit_mask_grad in csrc/stft.hip).
tests/test_mixit_loss.py pins it against torch fp64 autograd of the direct definition.

One utterance: M estimates e_0 .. e_{M-1}, 2 <= M <= 4, and N = 2 references x_0, x_1 -- the two recordings whose sum the
network saw --, all of one length.  Plain sums, no mean removal:
    P_n = sum x_n^2,   c_nk = sum x_n e_k,   G_kl = sum e_k e_l.
An assignment is a code a in [0, 2^M): bit k of a names the reference that estimate k is added to.  Every code is legal, one
that leaves a group empty included.  With "k in n" for the estimates whose bit is n,
    err_n(a)   = max(P_n - 2 sum_{k in n} c_nk + sum_{k,l in n} G_kl, 0)            (= |x_n - sum_{k in n} e_k|^2)
    score_n(a) = 10 log10((P_n + eps) / (err_n(a) + tau P_n + eps)) dB,   eps = 1e-30,
    score(a)   = (score_0(a) + score_1(a)) / 2,
tau = 10^(-snr_max / 10) the paper's soft SNR threshold (conf key mixit_snr_max, default 30 dB): an estimate better than
snr_max earns next to nothing more.  best = the first maximum of score in code order; loss = -(1/count) sum_j score_j(best_j).
Gradient: with n = bit k of best and m_n = sum_{l in n} e_l,
    d loss / d e_k[t] = D_n (m_n[t] - x_n[t]),   D_n = kappa / (count (err_n + tau P_n + eps)),  kappa = 10 / ln 10,
and D_n = 0 where err_n + tau P_n <= 0 (a silent reference met exactly).  The signal is the same for every estimate of a group.
"""
import numpy as np

EPS = 1e-30
KAPPA = 10.0 / np.log(10.0)
SNR_MAX = 30.0          # dB: the default of the conf key mixit_snr_max
MIN_EST, MAX_EST = 2, 4  # M; the upper end is the library's SK_MAXS
NREF = 2


def tau_of(snr_max=SNR_MAX):
    return 10.0 ** (-float(snr_max) / 10.0)


def members(code, n, M):
    """The estimates of group n under the assignment `code`, ascending."""
    return [k for k in range(M) if ((code >> k) & 1) == n]


def sums(ests, refs):
    """-> P (2,), c (2, M), G (M, M)."""
    E = np.stack([np.asarray(e, dtype=np.float64) for e in ests])
    X = np.stack([np.asarray(x, dtype=np.float64) for x in refs])
    return (X * X).sum(axis=1), X @ E.T, E @ E.T


def errors(P, c, G, code):
    """err_n(code), n = 0, 1, from the sums: members ascending, G_kk then 2 G_kl for l > k (the kernel's order)."""
    M = G.shape[0]
    out = np.zeros(NREF)
    for n in range(NREF):
        ks = members(code, n, M)
        cs = gs = 0.0
        for i, k in enumerate(ks):
            cs += c[n, k]
            gs += G[k, k]
            for l in ks[i + 1:]:
                gs += 2.0 * G[k, l]
        out[n] = max((P[n] - 2.0 * cs) + gs, 0.0)
    return out


def mixit(ests, refs, count=1.0, snr_max=SNR_MAX):
    """MixIT for ONE utterance: ests = M waveforms, refs = 2 waveforms (equal lengths) ->
    dict(loss = -best score / count, score (2^M) dB in code order, best = arg-max (first maximum), err (2,) of the best code,
    coef (2,) = D_0, D_1, P, c, G)."""
    M = len(ests)
    if not MIN_EST <= M <= MAX_EST or len(refs) != NREF:
        raise ValueError("mixit: %d estimates against %d references (need %d..%d against %d)" % (M, len(refs), MIN_EST, MAX_EST, NREF))
    tau = tau_of(snr_max)
    P, c, G = sums(ests, refs)
    score = np.zeros(1 << M)
    for code in range(1 << M):
        err = errors(P, c, G, code)
        score[code] = 0.5 * sum(10.0 * np.log10((P[n] + EPS) / (err[n] + tau * P[n] + EPS)) for n in range(NREF))
    best = int(np.argmax(score))                                  # first maximum
    err = errors(P, c, G, best)
    coef = np.zeros(NREF)
    for n in range(NREF):
        den = err[n] + tau * P[n]
        if den > 0.0:
            coef[n] = KAPPA / (float(count) * (den + EPS))
    return dict(loss=-score[best] / float(count), score=score, best=best, err=err, coef=coef, P=P, c=c, G=G)


def gradient(ests, refs, best, coef):
    """d loss / d e_k, k < M, for the assignment `best` and the coefficients mixit() returned: D_n (m_n - x_n) with n = bit k."""
    M = len(ests)
    E = [np.asarray(e, dtype=np.float64) for e in ests]
    sig = []
    for n in range(NREF):
        ks = members(best, n, M)
        m = np.zeros_like(E[0])
        for l in ks:                                              # ascending
            m = m + E[l]
        sig.append(coef[n] * (m - np.asarray(refs[n], dtype=np.float64)))
    return [sig[(best >> k) & 1] for k in range(M)]
