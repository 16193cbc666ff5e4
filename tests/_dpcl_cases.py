"""Cases, float32 error models and defect models of the deep-clustering tests.

tests/test_gpu_dpcl.py compares sk_dpcl_fwd / sk_dpcl_bwd / sk_dpcl_kmeans with sepkern/dpcl.py (numpy fp64) on the cases below;
tests/test_dpcl.py proves on any machine that the definition is what it says and that the cases can tell a wrong kernel from
a right one.

Gates (the rule of tests/test_gpu_sisdr.py): a compared quantity may be off by at most 4 x the error that the SAME formula
evaluated in float32 on the CPU leaves against fp64, measured per case; where that error happens to be below 2^-24 the gate
is 4 * 2^-24.
    loss       |L_j - L_j^fp64| / |C|_F^2 per utterance (|C|_F^2 is the largest of the three terms of L_j)
    dz         relative L2 error per utterance against the fp64 gradient.  At D = 1 every unit vector is [1] and the projection
               g - u (u . g) annihilates the gradient: the fp64 "gradient" is rounding noise of 1e-16 and no relative error
               against it means anything (with S = 1 even A u - Bm[:, y] cancels).  There the error is taken relative to
               the L2 norm over the points of 4 w_i (|A u_i| + |Bm[:, y_i]|) / |v_i| -- the size of the terms whose
               differences the gradient is -- for the kernel and the float32 model alike.
    centroids  largest absolute error (components of unit vectors' means: at most 1)
k-means labels are compared EXACTLY.  That is fair only where the reference's own decisions are not within rounding of a tie:
the builder keeps every arg-max of the initialisation at least 1e-4 and every assignment at least 1e-2 away from its
runner-up.  The worst fp32 error of a squared distance between unit vectors of D <= 40 components is of order D * 2^-23 ~ 5e-6.
"""
import functools

import numpy as np
import torch

from sepkern import dpcl

CH = 8                               # csrc/dpcl.hip: frames per chunk
FLOOR = 2.0 ** -24
FACTOR = 4.0
GAP_INIT, GAP_ASSIGN = 1e-4, 1e-2    # what the builder guarantees for the reference's decisions
GAP_POINT = 1e-4                     # overlapping case: points closer to a tie than this are not compared
MAX_TIED_SHARE = 0.005

BATCHES = {"ragged": [7, 5, 5, 1], "one_frame": [1], "uniform": [6, 6], "chunk-1": [CH - 1], "chunk": [CH], "chunk+1": [CH + 1]}
BINS = (5, 64, 65, 257)              # the tail wave branches at 64, 65 and 257
DS = ((1, 1), (3, 2), (20, 3), (40, 4))
WEIGHTS = ("mr", "vad")
DEFECTS = ("last_frame", "tail_bin", "last_plane", "wrong_utt", "unweighted")


def offsets(lens):
    """offs (T + 1) of a length-sorted batch: the packed-row table (sepkern/packing.py)."""
    lens = np.asarray(lens)
    n = np.array([(lens > t).sum() for t in range(int(lens[0]))])
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int32)


def gate(e32):
    return FACTOR * max(float(e32), FLOOR)


# ------------------------------------------------------------------------------------------------ loss cases
@functools.lru_cache(maxsize=None)
def loss_case(batch, F, D, S, pad=0, zero_utt=None):
    """Packed rows of a batch: z (R, F D + pad) float32 in (0, 1) (the padding columns hold a sentinel), mix and S sources (R, F)."""
    lens = BATCHES[batch]
    rng = np.random.default_rng([len(lens), lens[0], F, D, S])
    offs, R = offsets(lens), int(np.sum(lens))
    z = np.full((R, F * D + pad), 7.0, dtype=np.float32)
    z[:, :F * D] = 1.0 / (1.0 + np.exp(-rng.standard_normal((R, F * D)) * 1.5))
    srcs = [np.abs(rng.standard_normal((R, F))).astype(np.float32) * (1.0 + 0.3 * s) for s in range(S)]
    if S > 1:                                        # ties between sources: the lowest wins
        srcs[1][::3, ::4] = srcs[0][::3, ::4]
    mix = (np.abs(rng.standard_normal((R, F))) * rng.uniform(0.0, 1.0, (R, F)) ** 3).astype(np.float32)
    if zero_utt is not None:
        mix[dpcl.utterance_rows(lens, offs, zero_utt)] = 0.0
    return dict(lens=lens, offs=offs, R=R, F=F, D=D, S=S, z=z, mix=mix, srcs=srcs)


def loss_f32(c, j, kind, vad_db=dpcl.DEFAULT_VAD_DB):
    """L_j and dL_j/dz of utterance j by the definition's formulas in torch float32 on the CPU -> (L, dz (T, F D))."""
    F, D, S = c["F"], c["D"], c["S"]
    rows = dpcl.utterance_rows(c["lens"], c["offs"], j)
    z = torch.from_numpy(c["z"][rows][:, :F * D].copy())
    T = z.shape[0]
    v = z.view(T, D, F).permute(0, 2, 1).reshape(T * F, D)
    nrm = v.pow(2).sum(1).sqrt()
    u = v / nrm[:, None]
    m = torch.from_numpy(c["mix"][rows].reshape(-1).copy())
    wp = m if kind == "mr" else (m > float(dpcl.threshold(c["mix"][rows], vad_db))).float()
    tot = wp.sum()
    w = wp / tot if float(tot) > 0 else torch.zeros_like(wp)
    y = torch.from_numpy(dpcl.labels_of([s[rows] for s in c["srcs"]]))
    Y = torch.zeros(T * F, S)
    Y[torch.arange(T * F), y] = 1.0
    uw = u * w[:, None]
    A, Bm, C = uw.t() @ u, uw.t() @ Y, (Y * w[:, None]).sum(0)
    L = A.pow(2).sum() - 2.0 * Bm.pow(2).sum() + C.pow(2).sum()
    g = 4.0 * w[:, None] * (u @ A - Bm[:, y].t())
    dv = (g - u * (u * g).sum(1, keepdim=True)) / nrm[:, None]
    return float(L), dv.view(T, F, D).permute(0, 2, 1).reshape(T, D * F).double().numpy()


def loss_ref(c, j, kind, vad_db=dpcl.DEFAULT_VAD_DB):
    """fp64: (L_j, |C|_F^2, dL_j/dz (T, F D), the scale the gradient's error is relative to: None = its own norm)."""
    F, D = c["F"], c["D"]
    rows = dpcl.utterance_rows(c["lens"], c["offs"], j)
    args = (c["z"][rows], c["mix"][rows], [s[rows] for s in c["srcs"]], F, D, kind, vad_db)
    A, Bm, C, u, nrm, w, y = dpcl.moments(*args)
    scale = None
    if D == 1:                                       # (see the header: the projection annihilates the gradient)
        gun = 4.0 * w[:, None] * (np.abs(u @ A) + np.abs(Bm[:, y].T)) / nrm[:, None]
        scale = float(np.sqrt((gun * gun).sum()))
    return dpcl.loss_utt(*args), float((C * C).sum()), dpcl.grad_utt(*args), scale


def rel_l2(got, ref, scale=None):
    den = float(np.sqrt((np.asarray(ref, np.float64) ** 2).sum())) if scale is None else scale
    num = float(np.sqrt(((np.asarray(got, np.float64) - ref) ** 2).sum()))
    return num / den if den > 0 else (0.0 if num == 0 else float("inf"))


def defective(c, defect):
    """The case as a kernel with `defect` would see it: the definition evaluated on these inputs is what such a kernel returns."""
    lens, offs, F, D = c["lens"], c["offs"], c["F"], c["D"]
    d = dict(c, z=c["z"].copy(), mix=c["mix"].copy(), srcs=[s.copy() for s in c["srcs"]])
    if defect == "last_frame":                       # the last frame of every chunk is skipped
        for j, n in enumerate(lens):
            rows = dpcl.utterance_rows(lens, offs, j)
            last = sorted(set([min(t0 + CH, n) - 1 for t0 in range(0, n, CH)]))
            d["mix"][rows[last]] = 0.0
    elif defect == "tail_bin":                       # bin F - 1 (f = 256 of 257) is skipped
        d["mix"][:, F - 1] = 0.0
    elif defect == "last_plane":                     # plane D - 1 is not read
        d["z"][:, (D - 1) * F:D * F] = 0.0
    elif defect == "wrong_utt":                      # row of (t, j) taken as offs[t] + (j + 1) % n_t
        src = np.arange(c["R"])
        for t in range(lens[0]):
            n_t = int(offs[t + 1] - offs[t])
            src[offs[t]:offs[t + 1]] = offs[t] + (np.arange(n_t) + 1) % n_t
        d["z"] = d["z"][src]
    elif defect == "unweighted":                     # every point weighs the same
        d["mix"][:] = 1.0
    else:
        raise ValueError(defect)
    return d


def defect_applies(c, defect):
    if defect == "last_plane":
        return c["D"] > 1
    if defect == "wrong_utt":
        return len(c["lens"]) > 1
    return True


# ------------------------------------------------------------------------------------------------ k-means cases
KMEANS_CASES = (("ragged", 257, 4, 20), ("ragged", 257, 4, 40), ("ragged", 257, 2, 3), ("one_frame", 65, 3, 5), ("uniform", 64, 4, 4),
                ("chunk+1", 5, 2, 3), ("chunk+1", 257, 2, 20))


def _clustered(rng, n, F, D, S, hi, lo, noise):
    """(n, F D) rows whose points are drawn around S prototypes: cluster k has `hi` in dimensions k, k + S, ... and `lo` elsewhere."""
    proto = np.full((S, D), lo)
    for k in range(S):
        proto[k, k::S] = hi
    which = rng.integers(0, S, (n, F))
    v = np.clip(proto[which] + noise * rng.standard_normal((n, F, D)), 0.01, 0.99)            # (n, F, D)
    return v.transpose(0, 2, 1).reshape(n, D * F).astype(np.float32), proto


@functools.lru_cache(maxsize=None)
def kmeans_case(batch, F, S, D, iterations=20, pad=0):
    """The builder's recipe, the first seed whose reference decisions keep the gaps: well separated clusters, mix = 0.9 U^3 with
    one point at the utterance's level (1, 1/2, 1/4, ...: the utterances of a batch have different thresholds and active sets)."""
    lens = BATCHES[batch]
    offs, R = offsets(lens), int(np.sum(lens))
    for seed in range(200):
        rng = np.random.default_rng([seed, len(lens), lens[0], F, S, D])
        z = np.full((R, F * D + pad), 7.0, dtype=np.float32)
        z[:, :F * D], _ = _clustered(rng, R, F, D, S, 0.9, 0.1, 0.02)
        mix = (0.9 * rng.uniform(0.0, 1.0, (R, F)) ** 3).astype(np.float32)
        for j in range(len(lens)):
            rows = dpcl.utterance_rows(lens, offs, j)
            mix[rows] *= np.float32(0.5 ** j)
            mix[rows[int(rng.integers(len(rows)))], int(rng.integers(F))] = np.float32(0.5 ** j)
        ref = dpcl.kmeans_batch(z, mix, lens, offs, F, D, S, iterations)
        if ref["gap_init"] >= GAP_INIT and ref["gap_assign"] >= GAP_ASSIGN:
            return dict(lens=lens, offs=offs, R=R, F=F, D=D, S=S, z=z, mix=mix, ref=ref, seed=seed, iterations=iterations)
    raise AssertionError("no seed below 200 keeps the decision gaps for %r" % ((batch, F, S, D),))


@functools.lru_cache(maxsize=None)
def overlap_case():
    """Overlapping clusters, ONE Lloyd step from given centroids: some points lie within rounding of the boundary; labels are
    compared where the reference's gap is at least GAP_POINT, and the share of points below it is bounded."""
    lens, F, S, D = BATCHES["ragged"], 257, 3, 20
    offs, R = offsets(lens), int(np.sum(lens))
    rng = np.random.default_rng(20161)
    z, proto = _clustered(rng, R, F, D, S, 0.55, 0.45, 0.1)
    mix = (0.9 * rng.uniform(0.0, 1.0, (R, F)) ** 3).astype(np.float32)
    cin = proto / np.sqrt((proto * proto).sum(1, keepdims=True)) + 0.02 * rng.standard_normal((len(lens), S, D))
    cin = cin.astype(np.float32)
    ref = dpcl.kmeans_batch(z, mix, lens, offs, F, D, S, 1, centroids_in=cin)
    return dict(lens=lens, offs=offs, R=R, F=F, D=D, S=S, z=z, mix=mix, centroids_in=cin, ref=ref, iterations=1)


@functools.lru_cache(maxsize=None)
def few_active_case():
    """An utterance with fewer active points than clusters: two points above the threshold, S = 3 (centroid 2 copies centroid 0,
    and stays, having no active member of its own -- the tie between the two identical centroids is exact in any arithmetic)."""
    lens, F, S, D = BATCHES["uniform"], 65, 3, 5
    offs, R = offsets(lens), int(np.sum(lens))
    rng = np.random.default_rng(7)
    z, _ = _clustered(rng, R, F, D, S, 0.9, 0.1, 0.02)
    mix = (0.004 * rng.uniform(0.0, 1.0, (R, F))).astype(np.float32)          # below -40 dB of the maximum 1.0
    rows = dpcl.utterance_rows(lens, offs, 0)
    zu = z[rows].reshape(len(rows), D, F)
    zu[1, :, 3], zu[4, :, 60] = [0.9, 0.1, 0.1, 0.9, 0.1], [0.1, 0.9, 0.1, 0.1, 0.9]
    z[rows] = zu.reshape(len(rows), D * F)
    mix[rows[1], 3], mix[rows[4], 60] = 1.0, 0.8
    mix[dpcl.utterance_rows(lens, offs, 1)[2], 7] = 1.0                        # the second utterance: ONE active point
    ref = dpcl.kmeans_batch(z, mix, lens, offs, F, D, S, 3)
    return dict(lens=lens, offs=offs, R=R, F=F, D=D, S=S, z=z, mix=mix, ref=ref, iterations=3)


def centroid_error_model(c):
    """Largest centroid error of the float32 evaluation of the same algorithm against the fp64 reference."""
    r32 = dpcl.kmeans_batch(c["z"], c["mix"], c["lens"], c["offs"], c["F"], c["D"], c["S"], c["iterations"],
                            centroids_in=c.get("centroids_in"), dtype=np.float32)
    return float(np.abs(r32["centroids"].astype(np.float64) - c["ref"]["centroids"]).max()), r32
