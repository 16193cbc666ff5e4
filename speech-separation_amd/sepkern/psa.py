"""Phase-sensitive approximation (PSA) targets for utterance-level PIT (Kolbaek et al. 2017, "Multi-talker speech separation
with utterance-level permutation invariant training of deep recurrent neural networks", section III; Erdogan et al. 2015).

The network's masked mixture mask_s |Y| is resynthesised with the MIXTURE's phase, so the magnitude target |S_s| charges
nothing for a source whose phase differs from the mixture's.  PSA replaces it, per frame t and bin f, by the source's component
along the mixture:

    target_s = Re(S_s conj Y) / |Y|  =  |S_s| cos(theta_s - theta_Y)          (0 where the fp32 |Y|^2 < 2^-100)

with Y the mixture's STFT and S_s source s's, both as sk_stft defines them (oracle/stft.py).  The conf key `loss` of
archs/uPIT.py selects
    psa    the target as it is (it may be negative), and
    tpsa   the target held to [0, |Y|] -- the truncated form: the whole range mask_s |Y| reaches with a sigmoid mask.
The loss is the existing PIT-MSE with these targets in place of the source magnitudes, sum (mask_s |Y| - target_pi(s))^2 with
the same normalisation, arg-min over permutations and `norm`; the kernels of csrc/pit.hip serve it unchanged.

Below: the numpy fp64 restatement of what sk_stft_psa (csrc/stft.hip) computes from the spectra -- the documentation of its
arithmetic, and what tests/test_psa_loss.py and tests/test_gpu_psa.py pin the kernel to.
"""
import numpy as np

TINY = 2.0 ** -100           # |Y|^2 below this (in the kernel: the fp32 value) -> target 0


def _ymag(Y):
    Y = np.asarray(Y, dtype=np.complex128)
    y2 = Y.real * Y.real + Y.imag * Y.imag
    return Y, y2, np.sqrt(y2)


def psa_targets(Y, sources, clamp=False):
    """Y: the mixture's complex spectrum (any shape), sources: spectra [S_s] of that shape -> [target_s] float64.
    clamp: the truncated form, clip(target_s, 0, |Y|)."""
    Y, y2, mag = _ymag(Y)
    live = y2 >= TINY
    den = np.where(live, mag, 1.0)
    out = []
    for Ss in sources:
        Ss = np.asarray(Ss, dtype=np.complex128)
        t = np.where(live, (Ss.real * Y.real + Ss.imag * Y.imag) / den, 0.0)
        out.append(np.clip(t, 0.0, mag) if clamp else t)
    return out


def ideal_psm(Y, S):
    """The ideal phase-sensitive mask of one source, clip(Re(S conj Y) / |Y|^2, 0, 1): the oracle steps/evaluate_oracle.py --psm
    applies (0 where |Y|^2 < 2^-100)."""
    Y, y2, _ = _ymag(Y)
    S = np.asarray(S, dtype=np.complex128)
    live = y2 >= TINY
    return np.clip(np.where(live, (S.real * Y.real + S.imag * Y.imag) / np.where(live, y2, 1.0), 0.0), 0.0, 1.0)
