"""STOI / ESTOI for a batch of utterances on the GPU: the numbers of sepkern/stoi.py, computed by libsepkern's kernels
(csrc/stoi.hip, sk_stoi; include/sepkern.h "STOI").  Signals at another rate than 10 kHz go through sk_resample first."""
import numpy as np
import torch

from . import _lib, ops
from . import stoi as ST
from .bsseval_gpu import _as_tensor

MAX_WS_BYTES = 1 << 30       # device workspace per kernel call (the envelopes of the chunk); larger batches are split
MAX_S = 4


def _at_10k(rows, fs, device):
    """(S, n_u) tensors (float32 / float64 / int16 PCM, host or device) -> (flat fp32 device tensor at 10 kHz holding every
    row back to back, lengths per utterance at 10 kHz).  int16 is scaled by 2^-15, by sk_resample itself where it runs."""
    S = rows[0].shape[0]
    lens = [int(r.shape[1]) for r in rows]
    pcm = all(r.dtype == torch.int16 for r in rows)
    if int(fs) != ST.FS and pcm:
        flat = torch.cat([r.to(device).reshape(-1) for r in rows])
    else:
        flat = torch.cat([(r.to(device).to(torch.float32) * (1.0 / 32768.0) if r.dtype == torch.int16
                           else r.to(device).to(torch.float32)).reshape(-1) for r in rows])
    if int(fs) == ST.FS:
        return flat.contiguous(), lens
    out, outs = ops.resample_batch(flat.contiguous(), [n for n in lens for _ in range(S)], fs, ST.FS)
    return out, outs[::S]


def score_group(refs, ests, fs, device):
    """Device calls for utterances of one S.  Returns host arrays (out (U, S, S, 2), frames (U, S))."""
    S = refs[0].shape[0]
    lib = _lib.load()
    outs, frs = [], []
    c0 = 0
    while c0 < len(refs):
        c1, longest = c0, 0
        while c1 < len(refs):                  # the longest run whose workspace stays under MAX_WS_BYTES (always at least one)
            m = max(longest, -((-int(refs[c1].shape[1]) * ST.FS) // int(fs)))
            if c1 > c0 and lib.sk_stoi_workspace_bytes(c1 - c0 + 1, S, max(m, 1)) > MAX_WS_BYTES:
                break
            longest, c1 = m, c1 + 1
        rcat, lens = _at_10k(refs[c0:c1], fs, device)
        ecat, _ = _at_10k(ests[c0:c1], fs, device)
        offs = [0]
        for n in lens[:-1]:
            offs.append(offs[-1] + S * n)
        out, frames = ops.stoi(rcat, ecat, offs, lens, S)
        outs.append(out)
        frs.append(frames)
        c0 = c1
    return torch.cat(outs).cpu().numpy(), torch.cat(frs).cpu().numpy()


def stoi_batch(refs, ests, fs, compute_permutation=True):
    """stoi.stoi_sources for every utterance of a batch: refs / ests are lists of (S, n_u) arrays or tensors (numpy or torch,
    host or device; float32, float64 or int16 PCM, which is scaled by 2^-15) at fs Hz, 1 <= S <= 4 and n_u free per utterance.
    Returns one (stoi[S], estoi[S], perm, frames[S]) per utterance, in input order: perm[j] = the estimate given to source j,
    the assignment with the highest mean STOI (the first maximum in itertools.permutations order); ESTOI is reported under
    that same assignment; frames[j] < 30 marks the 1e-5 "not enough frames" value.  compute_permutation=False scores the
    diagonal."""
    refs = [_as_tensor(r) for r in refs]
    ests = [_as_tensor(e) for e in ests]
    if len(refs) != len(ests):
        raise ValueError("got %d reference sets and %d estimate sets" % (len(refs), len(ests)))
    for r, e in zip(refs, ests):
        if r.shape != e.shape or r.dim() != 2:
            raise ValueError("reference and estimated sources must be (S, n) arrays of one shape, got %s and %s"
                             % (tuple(r.shape), tuple(e.shape)))
        if not 1 <= r.shape[0] <= MAX_S or r.shape[1] < 1:
            raise _lib.SepkernError("stoi_batch: %d sources of %d samples; the kernels take 1..%d sources of at least one sample"
                                    % (r.shape[0], r.shape[1], MAX_S))
    if not torch.cuda.is_available():
        raise _lib.SepkernError("stoi_batch needs a GPU (the host function is sepkern.stoi.stoi_host)")
    dev = torch.device("cuda", torch.cuda.current_device())
    results = [None] * len(refs)
    groups = {}
    for u, r in enumerate(refs):
        groups.setdefault(int(r.shape[0]), []).append(u)
    for _, idx in sorted(groups.items()):
        out, frames = score_group([refs[u] for u in idx], [ests[u] for u in idx], fs, dev)
        for i, u in enumerate(idx):
            results[u] = ST.select(np.asarray(out[i]), frames[i], compute_permutation)
    return results
