"""Torch restatement (any dtype, autograd) of the SI-SDR uPIT loss, shared by tests/test_sisdr_loss.py and
tests/test_gpu_sisdr.py: oracle/stft.py::istft as irfft x window, index_add overlap-add and a guarded window-sum-square
division, followed by sepkern/sisdr.py::si_sdr and the arg-max over itertools.permutations.  In float64 it is the oracle
of the kernels' gradient; the same graph in float32 is the yardstick their error is held against."""
import itertools

import numpy as np
import torch

from oracle import stft as OS

N_FFT, HOP, F = 512, 128, 257


def istft_t(spec):
    """spec (F, T) complex tensor -> (HOP (T-1),) real tensor; differentiable."""
    rdt = torch.float64 if spec.dtype == torch.complex128 else torch.float32
    T = spec.shape[1]
    win = torch.from_numpy(OS.hann_periodic(N_FFT)).to(rdt)
    frames = torch.fft.irfft(spec.transpose(0, 1), n=N_FFT, dim=1) * win            # (T, N)
    n = N_FFT + HOP * (T - 1)
    idx = (torch.arange(N_FFT)[None, :] + HOP * torch.arange(T)[:, None]).reshape(-1)
    y = torch.zeros(n, dtype=rdt).index_add(0, idx, frames.reshape(-1))
    wss = torch.zeros(n, dtype=rdt).index_add(0, idx, (win * win).repeat(T))
    # divide by 1 where wss is not above float32 tiny (the trimmed ends): autograd would return NaN from 0/0 there
    y = y / torch.where(wss > float(np.finfo(np.float32).tiny), wss, torch.ones_like(wss))
    return y[N_FFT // 2:n - N_FFT // 2]


def si_sdr_t(est, ref):
    est = est - est.mean()
    ref = ref - ref.mean()
    alpha = torch.dot(est, ref) / (torch.dot(ref, ref) + 1e-30)
    target = alpha * ref
    noise = est - target
    return 10.0 * torch.log10((torch.dot(target, target) + 1e-30) / (torch.dot(noise, noise) + 1e-30))


def utterance_scores(ests, refs):
    """-> (pair (S,S) tensor, perm scores (S!) tensor, best index: first maximum)."""
    S = len(refs)
    pair = torch.stack([torch.stack([si_sdr_t(ests[k], refs[i]) for i in range(S)]) for k in range(S)])
    perms = list(itertools.permutations(range(S)))
    score = torch.stack([sum(pair[k, p[k]] for k in range(S)) / S for p in perms])
    return pair, score, int(np.argmax(score.detach().numpy()))


def loss_from_masks(specs, masks, refs, dtype=torch.float64, count=None):
    """specs: list over utterances of (F, T_j) complex arrays; masks: list of (S, F, T_j) tensors (requires_grad for a
    gradient); refs: list of lists of S waveforms (at least HOP (T_j - 1) samples, truncated here).
    -> (loss = -(1/count) sum_j best score, dict(ests, pair, score, best, margin) per utterance lists)."""
    cdt = torch.complex128 if dtype == torch.float64 else torch.complex64
    info = dict(ests=[], pair=[], score=[], best=[], margin=[])
    total = 0.0
    for X, m, rs in zip(specs, masks, refs):
        Xt = torch.as_tensor(np.asarray(X)).to(cdt)
        S = m.shape[0]
        ests = [istft_t(Xt * m[s].to(dtype)) for s in range(S)]
        L = ests[0].shape[0]
        rts = [torch.as_tensor(np.asarray(r, dtype=np.float64)[:L]).to(dtype) for r in rs]
        pair, score, best = utterance_scores(ests, rts)
        total = total + score[best]
        sc = np.sort(score.detach().double().numpy())
        info["ests"].append([e.detach() for e in ests])
        info["pair"].append(pair.detach())
        info["score"].append(score.detach())
        info["best"].append(best)
        info["margin"].append(float(sc[-1] - sc[-2]) if len(sc) > 1 else float("inf"))
    count = float(len(specs)) if count is None else float(count)
    return -total / count, info


# ------------------------------------------------------------------------------------------------ inputs
def band_sources(n, S, seed):
    """S band-limited noise sources of n samples in disjoint bands (float64, peak about 0.3 in sum)."""
    rng = np.random.default_rng(seed)
    out = []
    nb = n // 2 + 1
    for s in range(S):
        spec = np.zeros(nb, dtype=np.complex128)
        lo, hi = int(nb * (0.05 + 0.9 * s / S)), int(nb * (0.05 + 0.9 * (s + 1) / S))
        spec[lo:hi] = rng.standard_normal(hi - lo) + 1j * rng.standard_normal(hi - lo)
        x = np.fft.irfft(spec, n=n)
        out.append(0.3 / S * x / np.abs(x).max())
    return out


def to_pcm(x):
    return np.clip(np.round(np.asarray(x) * 32768.0), -32768, 32767).astype(np.int16)


def ratio_mask_case(lengths, S, seed):
    """The construction of tests 5-7: per utterance S band-limited sources, their int16 PCM and the mixture's, the mixture's
    complex STFT (oracle), ratio masks |S_i| / sum |S| + N(0, 0.1^2) clipped to [0.02, 0.98], and a non-identity shuffle pi
    of the references: refs[i] = source pi[i], so the best permutation is not the identity.
    -> dict(specs [(F,T)], masks [(S,F,T) float32], refs_pcm [[int16]*S], shuffle)."""
    rng = np.random.default_rng(seed)
    shuffle = list(range(1, S)) + [0] if S > 1 else [0]
    specs, masks, refs = [], [], []
    for u, n in enumerate(lengths):
        srcs = [to_pcm(s) for s in band_sources(int(n), S, 1000 * seed + u)]
        mix = to_pcm(np.sum([s.astype(np.float64) for s in srcs], axis=0) / 32768.0)
        specs.append(OS.stft(OS.pcm16_to_float(mix)))
        mags = np.stack([np.abs(OS.stft(OS.pcm16_to_float(s))) for s in srcs]).astype(np.float64)
        m = mags / (mags.sum(axis=0, keepdims=True) + 1e-12) + 0.1 * rng.standard_normal(mags.shape)
        masks.append(np.clip(m, 0.02, 0.98).astype(np.float32))
        refs.append([srcs[shuffle[i]] for i in range(S)])
    return dict(specs=specs, masks=masks, refs_pcm=refs, shuffle=shuffle)
