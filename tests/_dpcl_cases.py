"""Cases, float32 error models and defect models of the deep-clustering tests.

tests/test_gpu_dpcl.py compares sk_dpcl_fwd / sk_dpcl_bwd / sk_dpcl_kmeans with sepkern/dpcl.py (numpy fp64) on the cases below;
tests/test_dpcl.py proves on any machine that the definition is what it says and that the cases can tell a wrong kernel from
a right one.  The second half of this file is the pin suite of csrc/dpcl.hip (tests/test_gpu_dpcl_cases.py runs it on the device,
tests/test_dpcl_cases.py proves its claims on any machine): the host code restated, a per-chunk fp64 Gram reference in the
kernel's column layout, cases on the tile, block and chunk edges with the boundary each claims, and defect models.

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
BINS = (5, 64, 65, 257)              # against the 64-point tile: below it, on it, one past it, a full chunk of 2056 points = 32 tiles + 8
                                     # (the tile edges proper, 64 and 256|257 points PER CHUNK, are EDGE_BINS' below: F = 8, 32, 33)
DS = ((1, 1), (3, 2), (20, 3), (40, 4))
WEIGHTS = ("mr", "vad")
DEFECTS = ("last_frame", "tail_bin", "last_plane", "wrong_utt", "unweighted")
# the pin suite's batches and bins (kept apart: tests/test_gpu_dpcl.py runs every batch of BATCHES at every bin of BINS)
EDGE_BATCHES = {"chunks_ragged": [19, 17, 9, 8, 3], "two_chunks": [2 * CH], "two_chunks+1": [2 * CH + 1]}
ALL_BATCHES = dict(BATCHES, **EDGE_BATCHES)
EDGE_BINS = (5, 8, 32, 33, 65)       # a full chunk of 8 frames is 40 | 64 | 256 | 264 | 520 points = 1 | 1 | 4 | 5 | 9 tiles of 64


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
    lens = ALL_BATCHES[batch]
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


def loss_f32(c, j, kind, vad_db=dpcl.DEFAULT_VAD_DB, moments=False):
    """L_j and dL_j/dz of utterance j by the definition's formulas in torch float32 on the CPU -> (L, dz (T, F D)); with
    moments=True also its A (D, D) and Bm (D, S), as fp64 arrays of the float32 values."""
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
    dz = dv.view(T, F, D).permute(0, 2, 1).reshape(T, D * F).double().numpy()
    return (float(L), dz, A.double().numpy(), Bm.double().numpy()) if moments else (float(L), dz)


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
    lens = ALL_BATCHES[batch]
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


# ================================================================================================ the pin suite of csrc/dpcl.hip
# ------------------------------------------------------------------------------------------------ its host code, restated
TP = 64                              # points per tile (one per lane)
DMAX = 40
MAXS = 4
AB = DMAX * DMAX + DMAX * MAXS       # floats of [A | Bm] per utterance at the fixed pitches (DMAX, MAXS)
WAVES = 4
ALIGN = 256


def tiles_of(D, S):
    """NT of dpcl_gram_kernel<NT, KM>, dpcl_loss_kernel<NT>, dpcl_cent_kernel<NT>."""
    return (D + S + 15) // 16


def npairs(NT, km):
    """Tile pairs a chunk's partial holds: the upper triangle (loss) or the last tile column (k-means)."""
    return NT if km else NT * (NT + 1) // 2


def chunks_of(T):
    return -(-T // CH)


def db_of(D):
    """DB of dpcl_bwd_kernel<DB>: the switch on (D + 7) / 8 with 40 as its default."""
    return {1: 8, 2: 16, 3: 24, 4: 32}.get((D + 7) // 8, 40)


def _align(n):
    return -(-n // ALIGN) * ALIGN


def layout_of(T, B, D, S, km):
    """The workspace: [chunk maxima | thresholds | pick values, indices, counts | centroids | Gram partials], byte offsets + total."""
    nc = B * chunks_of(T)
    lay, at = {}, 0
    for name, nbytes in (("cmax", nc * 4), ("thr", B * 4), ("pval", nc * 4 if km else 0), ("pidx", nc * 4 if km else 0),
                         ("pcnt", nc * 4 if km else 0), ("cent", B * MAXS * DMAX * 4 if km else 0),
                         ("partial", nc * npairs(tiles_of(D, S), km) * 256 * 8)):
        lay[name] = at
        at += _align(nbytes)
    lay["total"] = at + 256
    return lay


def chunk_table(n, F):
    """The chunks of an utterance of n frames: t0, frames, points, tiles of 64, trips of the four waves."""
    out = []
    for t0 in range(0, n, CH):
        nfr = min(CH, n - t0)
        npts = nfr * F
        ntiles = -(-npts // TP)
        out.append(dict(t0=t0, nfr=nfr, npts=npts, ntiles=ntiles, niter=-(-ntiles // WAVES)))
    return out


def instantiations(D, S, km):
    NT = tiles_of(D, S)
    if km:
        return {"gram<%d,true>" % NT, "cent<%d>" % NT}
    return {"gram<%d,false>" % NT, "loss<%d>" % NT, "bwd<%d>" % db_of(D)}


ALL_INSTANTIATIONS = ({"gram<%d,%s>" % (n, k) for n in (1, 2, 3) for k in ("false", "true")} | {"loss<%d>" % n for n in (1, 2, 3)} |
                      {"cent<%d>" % n for n in (1, 2, 3)} | {"bwd<%d>" % d for d in (8, 16, 24, 32, 40)})

# ------------------------------------------------------------------------------------------------ what a case may claim
PAIR_CLAIMS = {
    "nt1": lambda D, S: tiles_of(D, S) == 1, "nt2": lambda D, S: tiles_of(D, S) == 2, "nt3": lambda D, S: tiles_of(D, S) == 3,
    "abuts": lambda D, S: D + S == 16 * tiles_of(D, S),                  # no zero column: the one-hot block abuts the embedding
    "lone_block": lambda D, S: D + S == 16 * (tiles_of(D, S) - 1) + 1,   # the last tile holds one plane or one source, and zeros
    "d_on_tile": lambda D, S: D % 16 == 0,                               # the embedding ends on a tile edge
    "crosses": lambda D, S: tiles_of(D, S) > -(-D // 16),                # the block lies in a tile the embedding does not reach
    "seam16": lambda D, S: D >= 17, "seam32": lambda D, S: D >= 33,      # planes 15|16 (31|32) are both there
    "db8": lambda D, S: db_of(D) == 8, "db16": lambda D, S: db_of(D) == 16, "db24": lambda D, S: db_of(D) == 24,
    "db32": lambda D, S: db_of(D) == 32, "db40": lambda D, S: db_of(D) == 40,
    "db_full": lambda D, S: D == db_of(D), "db_low": lambda D, S: D == db_of(D) - 7,
    "a_one_trip": lambda D, S: D * D == 256, "a_two_trips": lambda D, S: 256 < D * D <= 512,
}
NT_EDGES = {(12, 4): ("nt1", "abuts"), (15, 1): ("nt1", "abuts"), (13, 4): ("nt2", "lone_block", "crosses"),
            (16, 1): ("nt2", "lone_block", "d_on_tile", "crosses", "a_one_trip", "db_full"), (28, 4): ("nt2", "abuts", "seam16"),
            (31, 1): ("nt2", "abuts", "seam16"), (29, 4): ("nt3", "lone_block", "crosses", "seam16"),
            (32, 1): ("nt3", "lone_block", "d_on_tile", "crosses", "db_full"), (40, 4): ("nt3", "db40", "db_full", "seam32")}
DB_EDGES = {(8, 2): ("db8", "db_full", "nt1"), (9, 2): ("db16", "db_low", "nt1"),
            (16, 2): ("db16", "db_full", "d_on_tile", "crosses", "a_one_trip", "nt2"),
            (17, 3): ("db24", "db_low", "a_two_trips", "seam16", "nt2"), (24, 2): ("db24", "db_full", "nt2"),
            (25, 2): ("db32", "db_low", "nt2"), (32, 2): ("db32", "db_full", "d_on_tile", "crosses", "nt3"),
            (33, 2): ("db40", "db_low", "seam32", "nt3")}
OLD_PAIRS = {(1, 1): ("db8", "db_low", "nt1")}                           # of DS: the one D = DB - 7 of dpcl_bwd_kernel<8>
LOSS_PAIRS = {**OLD_PAIRS, **NT_EDGES, **DB_EDGES}

GEOMETRY_CLAIMS = {
    "nchmax_gt_nch": lambda lens, F: any(chunks_of(n) < chunks_of(lens[0]) for n in lens),
    "multi_chunk_batch": lambda lens, F: len(lens) > 1 and chunks_of(lens[0]) > 1,
    "one_frame_last_chunk": lambda lens, F: any(n % CH == 1 and n > CH for n in lens),
    "three_frame_last_chunk": lambda lens, F: any(n % CH == 3 and n > CH for n in lens),
    "ends_on_chunk_edge": lambda lens, F: any(n % CH == 0 for n in lens),
    "one_full_tile": lambda lens, F: CH * F == TP and lens[0] >= CH,                     # npts = 64 from a full chunk
    "four_tiles": lambda lens, F: CH * F == 4 * TP and lens[0] >= CH,                    # every wave one full tile, niter = 1
    "five_tiles": lambda lens, F: 4 * TP < CH * F <= 5 * TP and lens[0] >= CH,           # niter = 2, waves 1..3 idle in the second trip
    "partial_tile": lambda lens, F: any(ch["npts"] % TP for n in lens for ch in chunk_table(n, F)),
}
_RAGGED = ("nchmax_gt_nch", "multi_chunk_batch", "one_frame_last_chunk", "three_frame_last_chunk", "ends_on_chunk_edge")
GEOMETRIES = {("chunks_ragged", 5): _RAGGED + ("partial_tile",), ("chunks_ragged", 65): _RAGGED + ("partial_tile",),
              ("chunks_ragged", 8): _RAGGED + ("one_full_tile",), ("chunks_ragged", 32): _RAGGED + ("four_tiles",),
              ("chunks_ragged", 33): _RAGGED + ("five_tiles", "partial_tile"),
              ("two_chunks", 8): ("one_full_tile", "ends_on_chunk_edge"), ("two_chunks", 32): ("four_tiles", "ends_on_chunk_edge"),
              ("two_chunks", 33): ("five_tiles", "partial_tile"),
              ("two_chunks+1", 8): ("one_full_tile", "one_frame_last_chunk", "partial_tile"),
              ("two_chunks+1", 32): ("four_tiles", "one_frame_last_chunk", "partial_tile"),
              ("two_chunks+1", 33): ("five_tiles", "one_frame_last_chunk", "partial_tile")}
TRIP_PAIRS = ((16, 1), (17, 3), (40, 4))         # the pairs that run on the wave-trip geometries (F = 8, 32, 33)


def _loss_cases():
    out = []
    for (batch, F) in GEOMETRIES:
        out += [(batch, F, D, S) for (D, S) in (LOSS_PAIRS if F in (5, 65) else TRIP_PAIRS)]
    return tuple(out)


LOSS_CASES = _loss_cases()                       # (batch, F, D, S): every pair on chunks_ragged at F = 5 and 65, TRIP_PAIRS on the rest
KMEANS_PAIRS = ((12, 4), (13, 4), (15, 2), (16, 2), (28, 4), (29, 4), (31, 2), (33, 3), (8, 2), (9, 2))
KMEANS_EDGE_CASES = tuple(("chunks_ragged", F, S, D) for F in (5, 65) for (D, S) in KMEANS_PAIRS)
KMEANS_ITERATION_CASES = (("chunks_ragged", 65, 4, 13), ("chunks_ragged", 5, 3, 33))     # also run at iterations 0 and 1


def check_claims():
    """Every case's predicates hold (run at import: a case that stops claiming what it says must not load)."""
    for (D, S), claims in LOSS_PAIRS.items():
        for name in claims:
            assert PAIR_CLAIMS[name](D, S), ("pair", D, S, name)
    for (batch, F), claims in GEOMETRIES.items():
        for name in claims:
            assert GEOMETRY_CLAIMS[name](ALL_BATCHES[batch], F), ("geometry", batch, F, name)
    assert [chunks_of(n) for n in EDGE_BATCHES["chunks_ragged"]] == [3, 3, 2, 1, 1]


check_claims()


# ------------------------------------------------------------------------------------------------ the per-chunk Gram reference
def edge_case(batch, F, D, S, pad=0):
    """loss_case with its key; the columns below F D do not depend on pad, so one reference serves both strides."""
    return dict(loss_case(batch, F, D, S, pad), batch=batch, key=(batch, F, D, S))


_POINTS = {}


def _points(c, j, kind):
    """Utterance j's points as the kernels see them: unit vectors, norms, labels and the weights BEFORE 1 / sum w."""
    at = (c["key"], j, kind)
    if at not in _POINTS:
        rows = dpcl.utterance_rows(c["lens"], c["offs"], j)
        v, nrm = dpcl.embed(c["z"][rows], c["F"], c["D"])
        m32 = c["mix"][rows].reshape(-1)
        wp = m32.astype(np.float64) if kind == "mr" else (m32 > dpcl.threshold(m32, dpcl.DEFAULT_VAD_DB)).astype(np.float64)
        _POINTS[at] = dict(rows=rows, u=dpcl.unit(v, nrm), nrm=nrm, y=dpcl.labels_of([s[rows] for s in c["srcs"]]), wp=wp, T=len(rows))
    return _POINTS[at]


def chunk_U(c, j, kind):
    """Per chunk of utterance j the (npts, P) matrix whose Gram matrix the chunk's partial is, in the kernel's column layout:
    sqrt(w) u in columns 0..D-1, zeros, sqrt(w) onehot(y) in the LAST S of the P = 16 NT columns."""
    p, F, D, S = _points(c, j, kind), c["F"], c["D"], c["S"]
    P, N = 16 * tiles_of(D, S), p["u"].shape[0]
    U = np.zeros((N, P))
    sw = np.sqrt(p["wp"])
    U[:, :D] = p["u"] * sw[:, None]
    U[np.arange(N), P - S + p["y"]] = sw
    return [U[ch["t0"] * F:ch["t0"] * F + ch["npts"]] for ch in chunk_table(c["lens"][j], F)]


def chunk_grams(c, j, kind):
    """The (P, P) fp64 matrices U^T U of the chunks of utterance j: what dpcl_gram_kernel<NT, false> stores per (j, chunk)."""
    return [U.T @ U for U in chunk_U(c, j, kind)]


def chunk_grams_f32(c, j, kind):
    """The same in float32 arithmetic throughout (as fp64 arrays): the error model of a chunk's partial."""
    p, F, D, S = _points(c, j, kind), c["F"], c["D"], c["S"]
    u = dpcl.unit(*dpcl.embed(c["z"][p["rows"]], F, D, np.float32))
    P, N = 16 * tiles_of(D, S), u.shape[0]
    U = np.zeros((N, P), dtype=np.float32)
    sw = np.sqrt(p["wp"].astype(np.float32))
    U[:, :D] = u * sw[:, None]
    U[np.arange(N), P - S + p["y"]] = sw
    assert U.dtype == np.float32
    return [(U[ch["t0"] * F:ch["t0"] * F + ch["npts"]].T @ U[ch["t0"] * F:ch["t0"] * F + ch["npts"]]).astype(np.float64)
            for ch in chunk_table(c["lens"][j], F)]


def gram_error(G, ref):
    """The largest error of a chunk's Gram matrix relative to sqrt(ref_aa ref_bb), the bound of its entry (a, b); an entry
    whose bound is zero -- a zero column -- must be exactly zero (inf otherwise)."""
    scale = np.sqrt(np.outer(np.diag(ref), np.diag(ref)))
    if np.any(G[scale == 0] != 0.0):
        return np.inf
    return float((np.abs(G - ref)[scale > 0] / scale[scale > 0]).max()) if np.any(scale > 0) else 0.0


def moments_of(G, D, S):
    """dpcl_loss_kernel on the chunks' sum G: (A, Bm, C the diagonal, 1 / sum w)."""
    P = G.shape[0]
    diag = np.diag(G)[P - S:]
    tr = float(diag.sum())
    sc = 1.0 / tr if tr > 0 else 0.0
    return G[:D, :D] * sc, G[:D, P - S:] * sc, diag * sc, sc


def loss_of(A, Bm, C):
    return float((A * A).sum() - 2.0 * (Bm * Bm).sum() + (C * C).sum())


def grad_of(c, j, kind, A, Bm, sc):
    """dpcl_bwd_kernel from the forward's A, Bm and 1 / sum w: (T, F D) fp64, count = 1."""
    p, F, D = _points(c, j, kind), c["F"], c["D"]
    g = 4.0 * (p["wp"] * sc)[:, None] * (p["u"] @ A - Bm[:, p["y"]].T)
    inv = np.where(p["nrm"] > 0, 1.0 / np.where(p["nrm"] > 0, p["nrm"], 1.0), 0.0)
    dv = (g - p["u"] * (p["u"] * g).sum(axis=1, keepdims=True)) * inv[:, None]
    return dv.reshape(p["T"], F, D).transpose(0, 2, 1).reshape(p["T"], D * F)


def ab_padding(D, S):
    """(AB,) bool: the entries of [A | Bm] beyond (D, S), which dpcl_loss_kernel must store as exact zeros."""
    pad = np.ones(AB, dtype=bool)
    pad[:DMAX * DMAX].reshape(DMAX, DMAX)[:D, :D] = False
    pad[DMAX * DMAX:].reshape(DMAX, MAXS)[:D, :S] = False
    return pad


def ab_of(A, Bm):
    """[A | Bm] at the fixed pitches (DMAX, MAXS), zero-padded: one utterance's AB floats as fp64."""
    out = np.zeros(AB)
    D, S = Bm.shape
    out[:DMAX * DMAX].reshape(DMAX, DMAX)[:D, :D] = A
    out[DMAX * DMAX:].reshape(DMAX, MAXS)[:D, :S] = Bm
    return out


@functools.lru_cache(maxsize=None)
def reference(key, j, kind):
    """fp64 of utterance j of edge_case(*key): L, |C|_F^2, dz (count = 1), the gradient's scale, ab (AB,), 1 / sum w, threshold."""
    c = edge_case(*key)
    L, c2, dz, scale = loss_ref(c, j, kind)
    rows = dpcl.utterance_rows(c["lens"], c["offs"], j)
    A, Bm = dpcl.moments(c["z"][rows], c["mix"][rows], [s[rows] for s in c["srcs"]], c["F"], c["D"], kind)[:2]
    p = _points(c, j, kind)
    tot = float(p["wp"].sum())
    thr = float(dpcl.threshold(c["mix"][rows], dpcl.DEFAULT_VAD_DB)) if kind == "vad" else 0.0
    return dict(L=L, c2=c2, dz=dz, scale=scale, ab=ab_of(A, Bm), sc=1.0 / tot if tot > 0 else 0.0, thr=thr)


@functools.lru_cache(maxsize=None)
def f32_errors(key, j, kind):
    """What the float32 CPU evaluation of the same formulas leaves against fp64: (loss / |C|_F^2, dz relative L2, ab largest
    absolute) -- the gates are FACTOR x these, floor FLOOR each."""
    c, r = edge_case(*key), reference(key, j, kind)
    L32, g32, A32, B32 = loss_f32(c, j, kind, moments=True)
    return abs(L32 - r["L"]) / r["c2"], rel_l2(g32, r["dz"], r["scale"]), float(np.abs(ab_of(A32, B32) - r["ab"]).max())


# 1 / sum w: every term of the trace is sqrtf(w)^2 -- two roundings of the root's, one of the product, at most three more where
# the matrix instruction adds its four points in float32 -- then exact fp64 sums and one rounding of the stored float: 7 * 2^-24
# relative in the worst case (vad weights are 0 / 1 and exact: one rounding).
SC_GATE = 8.0 * FLOOR


# ------------------------------------------------------------------------------------------------ defect models of the pin suite
# Each returns what a kernel with the defect would hand back for utterance j -- dict(L, dz, ab) -- from the restated layout
# or from the chunks' partials; DEFECT_CASES names the cases it must show on (all of them in LOSS_CASES).
EDGE_DEFECTS = ("chunk_pitch", "stale_chunk", "fourth_wave", "last_tile", "tile_seam", "onehot_overlap", "a_second_trip",
                "bwd_block_tail", "bwd_odd_row", "ab_padding")
_R5, _R65 = ("chunks_ragged", 5), ("chunks_ragged", 65)
DEFECT_CASES = {
    "chunk_pitch": [g + p for g in (_R5, _R65) for p in ((16, 2), (40, 4))],
    "stale_chunk": [g + p for g in (_R5, _R65) for p in ((16, 2), (40, 4))],
    "fourth_wave": [("two_chunks", 32, 16, 1), ("two_chunks+1", 33, 17, 3), ("chunks_ragged", 32, 40, 4), _R65 + (12, 4)],
    "last_tile": [("two_chunks+1", 33, 17, 3), ("two_chunks+1", 8, 16, 1), _R65 + (13, 4), _R5 + (8, 2)],
    "tile_seam": [_R65 + p for p in ((16, 1), (17, 3), (32, 1), (33, 2), (16, 2), (32, 2))],
    "onehot_overlap": [g + p for g in (_R5, _R65) for p in ((13, 4), (16, 1), (29, 4), (32, 1), (16, 2), (32, 2))],
    "a_second_trip": [_R65 + p for p in ((17, 3), (24, 2), (33, 2), (40, 4))] + [("two_chunks", 8, 17, 3)],
    "bwd_block_tail": [_R65 + p for p in ((8, 2), (9, 2), (16, 2), (17, 3), (24, 2), (25, 2), (32, 2), (33, 2), (40, 4))],
    "bwd_odd_row": [_R65 + p for p in ((8, 2), (16, 2), (24, 2), (32, 2), (40, 4))],
    "ab_padding": [_R65 + p for p in ((1, 1), (9, 2), (17, 3), (25, 2), (33, 2))],
}
SEAM_PLANES = (15, 16, 31, 32)


def defect_variants(key, defect):
    """tile_seam has one variant per seam plane the case has; every other defect has one."""
    return [p for p in SEAM_PLANES if p < key[2]] if defect == "tile_seam" else [None]


def _from_gram(c, j, kind, G, L=None, A_bwd=None):
    A, Bm, C, sc = moments_of(G, c["D"], c["S"])
    return dict(L=loss_of(A, Bm, C) if L is None else L, dz=grad_of(c, j, kind, A if A_bwd is None else A_bwd, Bm, sc), ab=ab_of(A, Bm))


def _drop_tiles(c, j, kind, dropped):
    """The utterance's Gram matrix without the tiles of every chunk that dropped(tile index, chunk) names."""
    G = 0.0
    for U, ch in zip(chunk_U(c, j, kind), chunk_table(c["lens"][j], c["F"])):
        keep = np.array([not dropped(q // TP, ch) for q in range(ch["npts"])])
        G = G + U[keep].T @ U[keep]
    return G


def defect_outputs(key, j, kind, defect, variant=None):
    c = edge_case(*key)
    lens, D, S = c["lens"], c["D"], c["S"]
    nch, nchmax = [chunks_of(n) for n in lens], chunks_of(lens[0])
    P = 16 * tiles_of(D, S)
    if defect in ("chunk_pitch", "stale_chunk"):
        store = {}                                   # what the gram kernel wrote, by slot; nobody wrote the others
        for jj in range(len(lens)):
            for ch, G in enumerate(chunk_grams(c, jj, kind)):
                store[jj * nchmax + ch] = G
        if defect == "chunk_pitch":                  # (j, ch) looked up at j * nch_j + ch; an unwritten slot counts as zeros
            slots = [j * nch[j] + ch for ch in range(nch[j])]
        else:                                        # nchmax chunks added: the extra slots hold utterance 0's, as a cached
            slots = [j * nchmax + ch for ch in range(nch[j])] + list(range(nch[j], nchmax))       # workspace may
        return _from_gram(c, j, kind, sum(store.get(s, np.zeros((P, P))) for s in slots))
    if defect == "fourth_wave":
        return _from_gram(c, j, kind, _drop_tiles(c, j, kind, lambda t, ch: t % WAVES == WAVES - 1))
    if defect == "last_tile":
        return _from_gram(c, j, kind, _drop_tiles(c, j, kind, lambda t, ch: ch["npts"] % TP != 0 and t == ch["ntiles"] - 1))
    if defect == "tile_seam":                        # a plane on the tile seam is not read: the kernel sees zeros there
        bad = dict(c, z=c["z"].copy())
        bad["z"][:, variant * c["F"]:(variant + 1) * c["F"]] = 0.0
        rows = dpcl.utterance_rows(lens, c["offs"], j)
        A, Bm = dpcl.moments(bad["z"][rows], c["mix"][rows], [s[rows] for s in c["srcs"]], c["F"], D, kind)[:2]
        L, _, dz, _ = loss_ref(bad, j, kind)
        return dict(L=L, dz=dz, ab=ab_of(A, Bm))
    if defect == "onehot_overlap":                   # the block written and read at D + s within tile ceil(D / 16) - 1: past
        t0 = -(-D // 16) - 1                         # the tile's end it wraps onto the embedding's own columns
        col = [t0 * 16 + (D + s - t0 * 16) % 16 for s in range(S)]
        G = 0.0
        for U in chunk_U(c, j, kind):
            V = np.zeros((U.shape[0], max(P, D + S)))
            V[:, :D] = U[:, :D]
            for s in range(S):
                V[:, col[s]] = U[:, P - S + s]
            W = np.zeros_like(U)
            W[:, :D] = V[:, :D]
            for s in range(S):
                W[:, P - S + s] = V[:, col[s]]
            G = G + W.T @ W
        return _from_gram(c, j, kind, G)
    G = sum(chunk_grams(c, j, kind))
    A, Bm, C, sc = moments_of(G, D, S)
    if defect == "a_second_trip":                    # |A|^2 without the entries e = a D + b >= 256
        return _from_gram(c, j, kind, G, L=loss_of(A, Bm, C) - float((A.reshape(-1)[256:] ** 2).sum()))
    if defect == "bwd_block_tail":                   # the last block of eight planes is not stored
        out = _from_gram(c, j, kind, G)
        out["dz"][:, 8 * ((D - 1) // 8) * c["F"]:] = 0.0
        return out
    if defect == "bwd_odd_row":                      # the last trip over two rows of A adds row b only: row DB - 1 is lost
        A_bwd = A.copy()
        if db_of(D) - 1 < D:
            A_bwd[db_of(D) - 1, :] = 0.0
        return _from_gram(c, j, kind, G, A_bwd=A_bwd)
    if defect == "ab_padding":
        # ab beyond (D, S) keeps what a D = 40, S = 4 utterance left there.  The backward multiplies a row b >= D by u_b = 0 and
        # never stores g_a for a >= D, so a FINITE stale value changes ab alone (compared exactly: any non-zero entry is caught);
        # a non-finite one (0 * NaN) reaches every dz of the utterance through the dot product.  Both are modelled: variant
        # None is the finite stale value, and dz is what the NaN gives.
        out = _from_gram(c, j, kind, G)
        out["ab"][ab_padding(D, S)] = 1.0 / DMAX
        if db_of(D) > D:
            out["dz"] = np.full_like(out["dz"], np.nan)
        return out
    raise ValueError(defect)


def defect_shows(key, kind, defect, variant=None, margin=10.0):
    """The largest ratio, over the utterances and the checked quantities (loss, dz, ab), of what the defect moves to margin x
    the quantity's gate; the padding of ab is compared exactly, so any change there counts as infinite."""
    c, worst = edge_case(*key), 0.0
    for j in range(len(c["lens"])):
        r, (e_l, e_g, e_ab) = reference(key, j, kind), f32_errors(key, j, kind)
        bad = defect_outputs(key, j, kind, defect, variant)
        dzerr = rel_l2(bad["dz"], r["dz"], r["scale"])
        moved = [abs(bad["L"] - r["L"]) / r["c2"] / gate(e_l), (np.inf if np.isnan(dzerr) else dzerr) / gate(e_g),
                 float(np.abs(bad["ab"] - r["ab"]).max()) / gate(e_ab)]
        if np.any(bad["ab"][ab_padding(c["D"], c["S"])] != 0.0):
            moved.append(np.inf)
        worst = max(worst, max(moved) / margin)
    return worst


# ------------------------------------------------------------------------------------------------ defects of the centroid update
# dpcl_gram_kernel<NT, true> leaves per (utterance, chunk) the weighted sums of the active members of every cluster and their
# weights; dpcl_cent_kernel<NT> adds an utterance's chunks and divides.  The builder's cases have converged long before their 20
# steps end, so the last update's members are the final labels': the update restated from the reference's labels must give the
# reference's centroids (asserted), and a defective update is then a function of the chunks' sums.
KMEANS_DEFECTS = ("chunk_pitch", "stale_chunk", "tile_seam")


def kmeans_chunk_sums(c, j):
    """Per chunk of utterance j: (sums (S, D), weights (S,)) of the active points by the reference's final labels, fp64."""
    F, D, S = c["F"], c["D"], c["S"]
    rows = dpcl.utterance_rows(c["lens"], c["offs"], j)
    u = dpcl.unit(*dpcl.embed(c["z"][rows], F, D))
    m32 = c["mix"][rows].reshape(-1)
    w = np.where(m32 > dpcl.threshold(m32, dpcl.DEFAULT_VAD_DB), m32.astype(np.float64), 0.0)
    lab = c["ref"]["labels"][rows].reshape(-1)
    out = []
    for ch in chunk_table(c["lens"][j], F):
        sel = slice(ch["t0"] * F, ch["t0"] * F + ch["npts"])
        onehot = (lab[sel][:, None] == np.arange(S)[None, :]) * w[sel][:, None]              # (npts, S)
        out.append((onehot.T @ u[sel], onehot.sum(axis=0)))
    return out


def kmeans_update(c, defect=None, variant=None):
    """The centroids (B, S, D) after the last update as dpcl_cent_kernel gives them, or as it would with the defect."""
    lens, S, D = c["lens"], c["S"], c["D"]
    nch, nchmax = [chunks_of(n) for n in lens], chunks_of(lens[0])
    store = {j * nchmax + ch: sw for j in range(len(lens)) for ch, sw in enumerate(kmeans_chunk_sums(c, j))}
    cent = c["ref"]["centroids"].copy()
    for j in range(len(lens)):
        slots = [j * nchmax + ch for ch in range(nch[j])]
        if defect == "chunk_pitch":
            slots = [j * nch[j] + ch for ch in range(nch[j])]
        elif defect == "stale_chunk":
            slots += list(range(nch[j], nchmax))
        s = sum(store[a][0] for a in slots if a in store)
        w = sum(store[a][1] for a in slots if a in store)
        if defect == "tile_seam":                    # plane `variant`'s sums are not read
            s = s.copy()
            s[:, variant] = 0.0
        for k in range(S):
            if w[k] > 0:
                cent[j][k] = s[k] / w[k]
    return cent


# ------------------------------------------------------------------------------------------------ the pick-tie case
TIE_LENS, TIE_F, TIE_S, TIE_D = [16, 16, 16], 65, 3, 6
# (lower, higher) point index of the two points that share the utterance's largest mix.  dpcl_pick_kernel: point q of a chunk
# of 520 is thread q % 256 on trip q // 256, wave (q % 256) / 64.
TIE_POINTS = ((50, 266),             # utterance 0: one chunk, one wave (threads 50 and 10 of wave 0): the lower index at the HIGHER lane
              (100, 300),            # utterance 1: one chunk, waves 1 (thread 100) and 0 (thread 44): the lower index in the HIGHER wave
              (300, 520 + 10))       # utterance 2: chunks 0 and 1


def _later_pick_gaps(z, mix, F, D, S):
    """The gaps of the farthest-first picks AFTER centroid 0 (whose own gap is the tie: zero by construction)."""
    cent = dpcl.kmeans(z, mix, F, D, S, 0)["centroids"]
    u = dpcl.unit(*dpcl.embed(z, F, D))
    m32 = np.asarray(mix, dtype=np.float32).reshape(-1)
    act = np.flatnonzero(m32 > dpcl.threshold(m32, dpcl.DEFAULT_VAD_DB))
    gap = np.inf
    for k in range(1, S):
        gap = min(gap, dpcl._gap_max(((u[act][:, None, :] - cent[None, :k, :]) ** 2).sum(axis=2).min(axis=1)))
    return gap


@functools.lru_cache(maxsize=None)
def tie_case(pad=0):
    """iterations = 0, no centroids_in: two points per utterance carry the same float32 maximum of mix and the prototypes of two
    different clusters.  The tie is exact in any arithmetic; the first seed whose LATER picks and assignments keep the gaps."""
    lens, F, S, D = TIE_LENS, TIE_F, TIE_S, TIE_D
    offs, R = offsets(lens), int(np.sum(lens))
    for seed in range(200):
        rng = np.random.default_rng([seed, 7243, F, S, D])
        z = np.full((R, F * D + pad), 7.0, dtype=np.float32)
        z[:, :F * D], proto = _clustered(rng, R, F, D, S, 0.9, 0.1, 0.02)
        mix = (0.9 * rng.uniform(0.0, 1.0, (R, F)) ** 3).astype(np.float32)
        for j in range(len(lens)):
            rows = dpcl.utterance_rows(lens, offs, j)
            mix[rows] *= np.float32(0.5 ** j)
            for q, k in zip(TIE_POINTS[j], (1, 2)):              # the lower point in cluster 1, the higher in cluster 2
                t, f = divmod(q, F)
                mix[rows[t], f] = np.float32(0.5 ** j)
                z[rows[t], f:F * D:F] = proto[k].astype(np.float32)
        ref = dpcl.kmeans_batch(z, mix, lens, offs, F, D, S, 0)
        later = min(_later_pick_gaps(z[dpcl.utterance_rows(lens, offs, j)], mix[dpcl.utterance_rows(lens, offs, j)], F, D, S)
                    for j in range(len(lens)))
        if later >= GAP_INIT and ref["gap_assign"] >= GAP_ASSIGN:
            return dict(lens=lens, offs=offs, R=R, F=F, D=D, S=S, z=z, mix=mix, ref=ref, seed=seed, iterations=0, later_gap=later)
    raise AssertionError("no seed below 200 keeps the gaps of the tie case")


def tie_unit_vectors(c, j):
    """(unit vector of the lower-indexed tied point, of the higher-indexed one) of utterance j, fp64."""
    rows = dpcl.utterance_rows(c["lens"], c["offs"], j)
    u = dpcl.unit(*dpcl.embed(c["z"][rows], c["F"], c["D"]))
    return u[TIE_POINTS[j][0]], u[TIE_POINTS[j][1]]


def pick_first_lane(c):
    """The tie case as a kernel would answer it that gives a tie to the lower lane (wave; the later chunk) instead of the lower
    index: the reference on a mixture whose higher-indexed point is one ulp louder."""
    mix = c["mix"].copy()
    for j in range(len(c["lens"])):
        rows = dpcl.utterance_rows(c["lens"], c["offs"], j)
        t, f = divmod(TIE_POINTS[j][1], c["F"])
        mix[rows[t], f] = np.nextafter(mix[rows[t], f], np.float32(np.inf))
    return dpcl.kmeans_batch(c["z"], mix, c["lens"], c["offs"], c["F"], c["D"], c["S"], 0)
