"""Stitching the masks of overlapping windows into one recording: the definition, in numpy.

A recording too long for one pass of the network is separated window by window (continuous speech separation: Yoshioka et
al. 2018, the LibriCSS recipe of Chen et al. 2020): the network runs on overlapping windows of the training length, the
output order of neighbouring windows -- which utterance-level PIT fixes only inside one window -- is aligned on the frames
they share, and the windows are cross-faded.  This file states what sk_stitch (include/sepkern.h, csrc/stitch.hip) computes
and restates it in numpy; tests/test_gpu_stitch.py holds the kernels to it bit for bit.

Geometry.  T frames, windows of W frames every Hn frames, W/2 <= Hn < W: at most two windows cover a frame, the overlap is
O = W - Hn >= 1 frames.  K = 1 + ceil(max(T - W, 0) / Hn) windows; window k starts at frame k Hn and has
len_k = min(W, T - k Hn) frames: every window but the last is full, and for K >= 2 the last one has more than O frames, so
every boundary shares exactly O frames.  (For K = 1 the only window has the recording's T <= W frames.)

Boundary cost.  X (T, F) are the mixture's magnitude rows, m_k[t][s F + f] window k's mask (t local to the window, S outputs).
For k < K - 1, in fp64 with every operand widened first,

    cost_k[i][j] = sum_{o < O} sum_{f < F} ( X[(k+1) Hn + o][f] * ( m_k[Hn + o][i F + f] - m_{k+1}[o][j F + f] ) )^2

-- the PIT-MSE loss's magnitude-weighted distance, between two windows.  p_k is the permutation p, searched in
itertools.permutations order, that minimises sum_i cost_k[i][p(i)] (i ascending, fp64; the first minimum wins, as the PIT
kernels break ties: a silent overlap gives the identity).

Chain.  PI_0 = identity, PI_{k+1}(s) = p_k(PI_k(s)): stitched stream s is output PI_k(s) of window k.

Blend.  ramp[o], o < O, float32 in [0, 1]: the weight of the LATER window at overlap index o.  With a the earlier covering
window's value and b the later one's, each read at its permuted column, out = a + ramp[o] * (b - a): one fp32 subtraction, one
fp32 multiplication and one fp32 addition, each rounded (no fused multiply-add).  A frame one window covers is copied.
"""
import itertools

import numpy as np

F = 257
MAX_S = 4


def check_geometry(T, W, Hn):
    if T < 1:
        raise ValueError("stitch: T = %d frames, at least 1 expected" % T)
    if W < 2 or not (2 * Hn >= W and Hn < W):
        raise ValueError("stitch: hop Hn = %d outside [W/2, W) for windows of W = %d frames" % (Hn, W))


def window_starts(T, W, Hn):
    """The first frame of each of the K = 1 + ceil(max(T - W, 0) / Hn) windows."""
    check_geometry(T, W, Hn)
    K = 1 + -(-max(T - W, 0) // Hn)
    return [k * Hn for k in range(K)]


def window_lengths(T, W, Hn):
    return [min(W, T - st) for st in window_starts(T, W, Hn)]


def default_ramp(O):
    """The driver's cross-fade: float32(o + 1) / float32(O + 1), rounded once."""
    return (np.arange(1, O + 1, dtype=np.float32) / np.float32(O + 1)).astype(np.float32)


def boundary_cost(X, m_a, m_b, start_b, W, Hn, S):
    """cost[i][j] (S, S) float64 of the boundary between a window and its successor, whose first frame is start_b."""
    O = W - Hn
    x = X[start_b:start_b + O, :F].astype(np.float64)
    a = m_a[Hn:Hn + O, :S * F].astype(np.float64).reshape(O, S, F)
    b = m_b[:O, :S * F].astype(np.float64).reshape(O, S, F)
    cost = np.empty((S, S), dtype=np.float64)
    for i in range(S):
        for j in range(S):
            cost[i, j] = np.sum((x * (a[:, i] - b[:, j])) ** 2)
    return cost


def best_permutation(cost):
    """The first permutation in itertools.permutations order with the smallest sum_i cost[i][p(i)], and all the sums."""
    S = cost.shape[0]
    totals = []
    for p in itertools.permutations(range(S)):
        tot = np.float64(0.0)
        for i in range(S):
            tot = tot + cost[i, p[i]]
        totals.append(tot)
    best = 0
    for n, tot in enumerate(totals):
        if tot < totals[best]:
            best = n
    return list(itertools.permutations(range(S)))[best], totals


def stitch_reference(X, windows, W, Hn, ramp):
    """X (T, >= F) float32 magnitude rows, windows[k] (>= len_k, >= S F) float32 masks, ramp (W - Hn) float32 ->
    (out (T, S F) float32, perms (K, S) int32 = PI_k, cost (K - 1, S, S) float64)."""
    X = np.asarray(X)
    T = X.shape[0]
    starts = window_starts(T, W, Hn)
    K, O = len(starts), W - Hn
    if len(windows) != K:
        raise ValueError("stitch: %d windows given, T = %d, W = %d, Hn = %d make %d" % (len(windows), T, W, Hn, K))
    S = windows[0].shape[1] // F
    if not 1 <= S <= MAX_S:
        raise ValueError("stitch: S = %d outputs outside 1..%d" % (S, MAX_S))
    ramp = np.asarray(ramp, dtype=np.float32)
    if ramp.shape != (O,):
        raise ValueError("stitch: the ramp holds %s values, the overlap %d frames" % (ramp.shape, O))
    lens = [min(W, T - st) for st in starts]
    perms = np.zeros((K, S), dtype=np.int32)
    perms[0] = np.arange(S)
    cost = np.zeros((max(K - 1, 0), S, S), dtype=np.float64)
    for k in range(K - 1):
        cost[k] = boundary_cost(X, windows[k], windows[k + 1], starts[k + 1], W, Hn, S)
        p, _ = best_permutation(cost[k])
        perms[k + 1] = [p[perms[k][s]] for s in range(S)]
    out = np.empty((T, S * F), dtype=np.float32)
    for k in range(K):
        m = np.asarray(windows[k], dtype=np.float32)[:lens[k]]
        own = np.concatenate([m[:, perms[k][s] * F:(perms[k][s] + 1) * F] for s in range(S)], axis=1)
        if k == 0:
            out[:lens[0]] = own
            continue
        a = out[starts[k]:starts[k] + O]                       # what window k - 1 left there
        b = own[:O]
        d = (b - a).astype(np.float32)
        out[starts[k]:starts[k] + O] = (a + (ramp[:, None] * d).astype(np.float32)).astype(np.float32)
        out[starts[k] + O:starts[k] + lens[k]] = own[O:]
    return out, perms, cost


def memory_bytes(T, W, Hn, S):
    """Bytes of the window masks a recording keeps resident until it is stitched: K W S F 4."""
    return len(window_starts(T, W, Hn)) * W * S * F * 4
