"""Inputs shared by tests/test_stitch.py and tests/test_gpu_stitch.py: windows cut from one global mask."""
import numpy as np

from sepkern import stitch as st

F = st.F


def permuted_slices(T, W, Hn, S, seed, noise=0.0):
    """A float32 uniform(0, 1) global mask (T, S, F), X = |N(0, 1)| (T, F), and the windows cut from the mask: output j of
    window k holds global stream q_k[j] (q_k a random permutation), plus noise * uniform(-1, 1) when noise is given.
    -> (glob, X, windows [(len_k, S F) float32], qs)."""
    rng = np.random.default_rng(seed)
    glob = rng.uniform(0.0, 1.0, (T, S, F)).astype(np.float32)
    X = np.abs(rng.standard_normal((T, F))).astype(np.float32)
    starts, lens = st.window_starts(T, W, Hn), st.window_lengths(T, W, Hn)
    qs = [rng.permutation(S) for _ in starts]
    windows = []
    for s0, n, q in zip(starts, lens, qs):
        w = glob[s0:s0 + n][:, q, :].reshape(n, S * F).copy()
        if noise:
            w = (w + np.float32(noise) * rng.uniform(-1.0, 1.0, w.shape).astype(np.float32)).astype(np.float32)
        windows.append(w)
    return glob, X, windows, qs


def expected_perms(qs):
    """PI_k(s) = the output of window k that holds global stream q_0[s]."""
    S = len(qs[0])
    return np.array([[int(np.where(q == qs[0][s])[0][0]) for s in range(S)] for q in qs], dtype=np.int32)
