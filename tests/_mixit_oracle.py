"""Torch restatement (any dtype, autograd) of the mixture-invariant loss by its DIRECT definition, shared by
tests/test_mixit_loss.py and tests/test_gpu_mixit.py: the group sums m_n are formed, then |x_n - m_n|^2 -- no Gram matrix.
In float64 it is the oracle of sepkern/mixit.py and of the kernels' gradient; the same graph in float32 is the yardstick the
kernels' error is held against.  Inputs: noisy partitions with a known assignment."""
import numpy as np
import torch

import _sisdr_oracle as SO

EPS = 1e-30


def score_t(ests, refs, code, tau):
    """score(code) of one utterance: ests M tensors, refs 2 tensors."""
    total = 0.0
    for n in range(2):
        m = torch.zeros_like(refs[n])
        for k in range(len(ests)):                          # ascending
            if ((code >> k) & 1) == n:
                m = m + ests[k]
        P = torch.dot(refs[n], refs[n])
        d = refs[n] - m
        total = total + 10.0 * torch.log10((P + EPS) / (torch.dot(d, d) + tau * P + EPS))
    return 0.5 * total


def utterance_t(ests, refs, tau, force=None):
    """-> (scores (2^M) tensor, best code: first maximum, or `force`)."""
    score = torch.stack([score_t(ests, refs, a, tau) for a in range(1 << len(ests))])
    best = int(np.argmax(score.detach().double().numpy())) if force is None else int(force)
    return score, best


def loss_t(ests, refs, tau, count=None, force=None):
    """ests / refs: per utterance lists of tensors -> (loss = -(1/count) sum_j score_j(best_j), [scores], [best])."""
    total, scores, bests = 0.0, [], []
    for j, (es, xs) in enumerate(zip(ests, refs)):
        score, best = utterance_t(es, xs, tau, None if force is None else force[j])
        total = total + score[best]
        scores.append(score.detach())
        bests.append(best)
    count = float(len(ests)) if count is None else float(count)
    return -total / count, scores, bests


def loss_from_masks(specs, masks, refs, tau, dtype=torch.float64, count=None, force=None):
    """specs: per utterance (F, T_j) complex arrays; masks: per utterance (M, F, T_j) tensors (requires_grad for a gradient);
    refs: per utterance two waveforms (truncated to 128 (T_j - 1) samples).  The estimates are tests/_sisdr_oracle.py's iSTFT."""
    cdt = torch.complex128 if dtype == torch.float64 else torch.complex64
    ests, rts = [], []
    for X, m, xs in zip(specs, masks, refs):
        Xt = torch.as_tensor(np.asarray(X)).to(cdt)
        es = [SO.istft_t(Xt * m[k].to(dtype)) for k in range(m.shape[0])]
        ests.append(es)
        rts.append([torch.as_tensor(np.asarray(x, dtype=np.float64)[:es[0].shape[0]]).to(dtype) for x in xs])
    return loss_t(ests, rts, tau, count, force)


# ------------------------------------------------------------------------------------------------ inputs
def noisy_partition(L, M, seed, code=None, silent=None, noise=0.1):
    """M sources of L samples in disjoint bands (peak about 0.3 in sum); estimate k = source k + noise x white noise of the
    source's RMS; reference n = the sum of the sources whose bit of `code` (drawn when None) is n, rounded to int16 PCM.
    silent = n: the sources of group n are zero, so reference n is silent and its estimates are noise x a small white noise.
    -> dict(ests [float32 (L,)] * M, refs_pcm [int16 (L,)] * 2, code)."""
    rng = np.random.default_rng(seed)
    code = int(rng.integers(1, (1 << M) - 1)) if code is None else int(code)
    srcs = SO.band_sources(L, M, seed)
    ests, refs = [], [np.zeros(L), np.zeros(L)]
    for k, s in enumerate(srcs):
        n = (code >> k) & 1
        rms = np.sqrt(np.mean(s ** 2))
        if silent is not None and n == silent:
            s = np.zeros(L)
        refs[n] = refs[n] + s
        ests.append((s + noise * rms * rng.standard_normal(L)).astype(np.float32))
    return dict(ests=ests, refs_pcm=[SO.to_pcm(x) for x in refs], code=code)
