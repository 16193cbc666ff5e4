"""BSS Eval (v3) SDR / SIR / SAR for a batch of utterances on the GPU: the numbers of sepkern/bsseval.py's
bss_eval_sources, computed by libsepkern's fp64 kernels (csrc/bsseval.hip; include/sepkern.h "BSS Eval").

The host function projects each estimate in the time domain; here every term is an energy.  With G the Gram matrix
of the delayed references (Cholesky factor L) and b_k the correlations of the references with estimate k,
y = L^-1 b_k gives |P_all e_k|^2 = |y|^2, likewise |P_j e_k|^2 from source j's own block, and
    target = |P_j e|^2, interference = |P_all e|^2 - |P_j e|^2, artifacts = |e|^2 - |P_all e|^2.
An utterance whose Gram matrix does not factor (rank-deficient references, e.g. a pure tone) is re-scored by the
host function, which falls back to least squares; the result says which utterances took that path.
"""
import itertools

import numpy as np
import torch

from . import _lib, bsseval, ops

MAX_WS_BYTES = 4 << 30       # device workspace per kernel call (Gram matrices of the chunk); larger batches are split
MAX_S = 4


class BatchResult(list):
    """A list of (sdr, sir, sar, perm) per utterance, in input order, plus `fallback`: the indices of the utterances
    that were re-scored by the host function because their Gram matrix did not factor on the device."""

    def __init__(self, items, fallback):
        super().__init__(items)
        self.fallback = list(fallback)

    @property
    def n_fallback(self):
        return len(self.fallback)


def _as_tensor(x):
    """(S, n) tensor on its own device, float32 / float64 / int16 as given."""
    if isinstance(x, torch.Tensor):
        t = x
    else:
        a = np.asarray(x)
        if a.dtype not in (np.float32, np.float64, np.int16):
            a = a.astype(np.float64)
        t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype not in (torch.float32, torch.float64, torch.int16):
        raise TypeError("bss_eval_sources_batch: inputs must be float32, float64 or int16, got %s" % t.dtype)
    return t.reshape(1, -1) if t.dim() == 1 else t


def _to_device_f64(t, device):
    """fp64 on the device; int16 PCM is scaled by 2^-15 (as the CLIs read wav files: exact)."""
    pcm = t.dtype == torch.int16
    t = t.to(device=device).to(torch.float64)
    return t * (1.0 / 32768.0) if pcm else t.contiguous()


def _check(refs, ests):
    """The host function's ValueErrors, before anything is copied: shapes first, then silent sources (host inputs
    checked on the host, device inputs in one batched device reduction)."""
    if len(refs) != len(ests):
        raise ValueError("got %d reference sets and %d estimate sets" % (len(refs), len(ests)))
    for r, e in zip(refs, ests):
        if r.shape != e.shape:
            raise ValueError("reference and estimated sources must have the same shape, got %s and %s"
                             % (tuple(r.shape), tuple(e.shape)))
        if r.dim() != 2:
            raise ValueError("sources must be (S, n) arrays, got shape %s" % (tuple(r.shape),))
    flags = []
    for r, e in zip(refs, ests):
        flags.append(torch.all(torch.any(r != 0, dim=1)))
        flags.append(torch.all(torch.any(e != 0, dim=1)))
    dev = [f for f in flags if f.is_cuda]
    dev_vals = iter(torch.stack(dev).cpu().tolist()) if dev else iter(())
    vals = [next(dev_vals) if f.is_cuda else bool(f) for f in flags]
    for u in range(len(refs)):
        if not vals[2 * u]:
            raise ValueError("all-zero reference source: BSS Eval metrics are undefined")
        if not vals[2 * u + 1]:
            raise ValueError("all-zero estimated source: BSS Eval metrics are undefined")


def _host(x):
    return x.detach().cpu().numpy()


def select(mat, compute_permutation):
    """(sdr, sir, sar, perm) from the (S, S, 3) dB matrix [k][j] (estimate k against source j), by the host function's
    rule: the permutation with the highest mean SIR, the first maximum in itertools.permutations order."""
    S = mat.shape[0]
    sdr, sir, sar = mat[..., 0], mat[..., 1], mat[..., 2]
    if not compute_permutation:
        idx = np.arange(S)
        return sdr[idx, idx].copy(), sir[idx, idx].copy(), sar[idx, idx].copy(), idx
    best, best_mean = None, None
    for perm in itertools.permutations(range(S)):                        # perm[j] = estimate given to source j
        mean_sir = np.mean([sir[perm[j], j] for j in range(S)])
        if best is None or mean_sir > best_mean:
            best, best_mean = perm, mean_sir
    rows, cols = np.array(best), np.arange(S)
    return sdr[rows, cols], sir[rows, cols], sar[rows, cols], rows


def pack(rows):
    """Packed fp64 rows of (S, n_u) device tensors: (flat tensor, offsets, lengths) as sk_bss_* take them."""
    S = rows[0].shape[0]
    lens = [int(x.shape[1]) for x in rows]
    offs = [0]
    for n in lens[:-1]:
        offs.append(offs[-1] + S * n)
    return torch.cat([x.reshape(-1) for x in rows]), offs, lens


def score_group(refs, ests, taps):
    """Device calls for utterances of one S: refs / ests lists of (S, n_u) fp64 device tensors.  Returns host arrays
    (out (U, S, S, 3), status (U,)); the batch is split into calls of at most MAX_WS_BYTES of workspace."""
    S = refs[0].shape[0]
    per = max(1, _lib.load().sk_bss_workspace_bytes(1, S, taps))
    chunk = max(1, int(MAX_WS_BYTES // per))
    outs, stats = [], []
    for c0 in range(0, len(refs), chunk):
        rcat, offs, lens = pack(refs[c0:c0 + chunk])
        ecat, _, _ = pack(ests[c0:c0 + chunk])
        out, status = ops.bss_eval(rcat, ecat, offs, lens, S, taps)
        outs.append(out)
        stats.append(status)
    return torch.cat(outs).cpu().numpy(), torch.cat(stats).cpu().numpy()


def bss_eval_sources_batch(refs, ests, compute_permutation=True, taps=bsseval.FILTER_TAPS):
    """bsseval.bss_eval_sources for every utterance of a batch: refs / ests are lists of (S, n_u) arrays or tensors
    (numpy or torch, host or device; float32, float64 or int16 PCM, which is scaled by 2^-15), 1 <= S <= 4 and n_u
    free per utterance.  Returns a BatchResult: one (sdr, sir, sar, perm) per utterance with the host function's
    shapes and conventions, and `.fallback`, the utterances re-scored by the host function."""
    refs = [_as_tensor(r) for r in refs]
    ests = [_as_tensor(e) for e in ests]
    _check(refs, ests)
    for r in refs:
        if r.shape[0] > MAX_S:
            raise _lib.SepkernError("bss_eval_sources_batch: %d sources; the kernels take at most %d" % (r.shape[0], MAX_S))
    if not 1 <= int(taps) <= 512:
        raise _lib.SepkernError("bss_eval_sources_batch: taps = %d; the kernels take 1..512" % taps)
    if not torch.cuda.is_available():
        raise _lib.SepkernError("bss_eval_sources_batch needs a GPU (the host function is sepkern.bsseval.bss_eval_sources)")
    dev = torch.device("cuda", torch.cuda.current_device())
    R = [_to_device_f64(r, dev) for r in refs]
    E = [_to_device_f64(e, dev) for e in ests]
    results, fallback = [None] * len(R), []
    groups = {}
    for u, r in enumerate(R):
        groups.setdefault(int(r.shape[0]), []).append(u)
    for S, idx in sorted(groups.items()):
        out, status = score_group([R[u] for u in idx], [E[u] for u in idx], int(taps))
        for i, u in enumerate(idx):
            if status[i] != 0:
                fallback.append(u)
                results[u] = bsseval.bss_eval_sources(_host(R[u]), _host(E[u]), compute_permutation, taps)
            else:
                results[u] = select(out[i], compute_permutation)
    return BatchResult(results, sorted(fallback))
