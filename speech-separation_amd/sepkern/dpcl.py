"""Deep clustering: the training objective on embeddings and the k-means that turns embeddings into masks; the definition, in numpy.

Deep clustering (Hershey et al. 2016) is the second standard method on WSJ0-2mix beside uPIT: the same network emits a
D-dimensional embedding for every time-frequency point, the objective pulls the embeddings of points dominated by the same
source together, and at inference k-means on the embeddings gives the masks -- for any number of clusters.  This file states
what sk_dpcl_fwd, sk_dpcl_bwd and sk_dpcl_kmeans (include/sepkern.h, csrc/dpcl.hip) compute: the low-rank form of the objective
(Isik et al. 2016), the sigmoid + unit-norm embedding and the magnitude-ratio weights of Wang et al. 2018 ("Alternative
objective functions for deep clustering"), and restates it in numpy fp64; tests/test_gpu_dpcl.py holds the kernels to it.

UNPINNED, the way sepkern/stoi.py, sepkern/wpe.py and sepkern/cacgmm.py are: no third-party implementation is installed to
compare against; the tests hold the definition to the N x N affinity form, to autograd and to its stated edge cases.  No
corpus is at hand either: nothing here says what score a model trained this way reaches.

Layout.  The network's output is z (R, ld >= F D) float32 packed rows (sepkern/packing.py: row of (t, j) = offs[t] + j) with
values in (0, 1) -- the sigmoid of the head.  Embedding dimension d of bin f is COLUMN d F + f: D planes of F columns, the shape
of the S mask planes of a uPIT model.  mix and the sources are (R, F) magnitudes.

Points.  A point is i = (row r, bin f); utterance j has N_j = lens[j] F points, numbered t F + f.

Embedding.  v_i = (z[r, d F + f])_d,  u_i = v_i / |v_i|.  A sigmoid output is positive, so the norm is never 0; a row of exact
zeros gives u = 0 and gradient 0, not NaN.

Labels.  y_i = the first s that attains max_s src_s[r, f] (ties to the lowest s); Y its one-hot matrix (N_j, S), 1 <= S <= 4.

Weights (conf key dpcl_weight).
    mr  (default; Wang 2018's magnitude ratio)  w_i = mix_i / sum_{k in j} mix_k
    vad (Hershey 2016)                          w_i = 1 / N_act where mix_i > thr_j, else 0
  thr_j = float32(10^(-dpcl_vad_db / 20)) * max_{k in j} mix_k, ONE float32 product (the comparison is between float32 values, so
  the kernel and this file agree on every point); dpcl_vad_db = 40 by default.  An utterance whose weights are all zero (an
  all-zero mixture) has w = 0, loss 0 and gradient 0.

Loss of an utterance.  With W = diag(w):
    A = U^T W U (D x D)     Bm = U^T W Y (D x S)     C = Y^T W Y (S x S, diagonal)
    L_j = |A|_F^2 - 2 |Bm|_F^2 + |C|_F^2      ( = | W^1/2 (U U^T - Y Y^T) W^1/2 |_F^2, the N x N form: loss_nxn below )
  The batch loss is (1 / count) sum_j L_j, count = B or the global utterance count of a data-parallel step, as the waveform
  losses take it.

Gradient.  g_i = 4 w_i (A u_i - Bm[:, y_i]);   dL / dv_i = (g_i - u_i (u_i . g_i)) / |v_i|;  scaled by gout / count.

k-means (inference).  Per utterance, on u with S clusters, 2 <= S <= 4.
    Active points: mix_i > thr_j (the vad rule).  An active point weighs mix_i, an inactive point 0.
    Initialisation, farthest-first and deterministic: centroid 0 = the active point of largest mix_i (ties: the lowest point
      index in (row, bin) order); centroid k = the active point that maximises its least squared distance to the centroids
      before k (ties the same way).  With at most k active points, centroid k copies centroid 0; without any active point every
      centroid is the zero vector.  A caller's centroids_in (S, D) skips the initialisation.
    `iterations` >= 0 Lloyd steps (default 20): every point, active or not, goes to the centroid of least squared Euclidean
      distance (ties to the lowest k); every centroid becomes the weighted mean of its active members; a cluster without active
      member keeps its centroid.
    After the last update, one final assignment: labels (T, F), mask (T, S F) with mask[t, k F + f] = 1.0 where the label is k and
      0.0 otherwise -- the uPIT mask layout --, and the centroids.
  kmeans() also reports the SMALLEST DECISION GAP it met, between the best and the second-best candidate of every arg-max
  (initialisation) and every arg-min (assignments): the tests ask the kernel for the reference's labels exactly, which is fair
  only where the reference's own decisions are not within rounding of a tie.

Out of the definition, on purpose: chimera networks (an embedding head beside a mask head), soft or spherical k-means, and any
tuning of D, the weights or the iteration count.
"""
import numpy as np

MAX_D = 40
MAX_S = 4
WEIGHTS = ("mr", "vad")
DEFAULT_VAD_DB = 40.0
DEFAULT_ITERATIONS = 20


def parse_weight(value):
    """The conf key dpcl_weight: 'mr' (default) or 'vad'."""
    value = str(value).strip().lower()
    if value not in WEIGHTS:
        raise ValueError("conf key dpcl_weight: %r is not one of %s" % (value, " / ".join(repr(v) for v in WEIGHTS)))
    return value


def parse_embed_dim(value):
    """The conf key embed_dim: an integer in 1..40."""
    try:
        D = int(value)
    except (TypeError, ValueError):
        raise ValueError("conf key embed_dim: %r is not an integer" % (value,))
    if not 1 <= D <= MAX_D:
        raise ValueError("conf key embed_dim: %d is outside 1..%d" % (D, MAX_D))
    return D


def vad_ratio(vad_db):
    """float32(10^(-vad_db / 20)): the factor of the activity threshold, as the kernels receive it."""
    r = np.float32(10.0 ** (-float(vad_db) / 20.0))
    if not (np.isfinite(r) and 0.0 <= r <= 1.0):
        raise ValueError("dpcl_vad_db = %r: a level of at least 0 dB expected" % (vad_db,))
    return r


def threshold(mix, vad_db):
    """thr_j of one utterance's float32 magnitudes: one float32 product."""
    mix = np.asarray(mix, dtype=np.float32)
    mx = np.float32(mix.max()) if mix.size else np.float32(0.0)
    return np.float32(vad_ratio(vad_db) * max(mx, np.float32(0.0)))


def embed(z, F, D, dtype=np.float64):
    """z (T, >= F D) rows of one utterance -> (v (N, D), |v| (N,)), N = T F points in (row, bin) order."""
    z = np.asarray(z)
    T = z.shape[0]
    v = z[:, :F * D].astype(dtype).reshape(T, D, F).transpose(0, 2, 1).reshape(T * F, D)
    return v, np.sqrt((v * v).sum(axis=1))


def unit(v, nrm):
    one = nrm.dtype.type(1.0)
    return v * np.where(nrm > 0, one / np.where(nrm > 0, nrm, one), nrm.dtype.type(0.0))[:, None]


def labels_of(srcs):
    """The dominant source of every point: srcs = S arrays (T, F) -> (N,) int, the first maximum."""
    return np.argmax(np.stack([np.asarray(s, dtype=np.float32).reshape(-1) for s in srcs]), axis=0)


def weights(mix, kind="mr", vad_db=DEFAULT_VAD_DB):
    """w (N,) fp64 of one utterance's magnitudes (T, F)."""
    m32 = np.asarray(mix, dtype=np.float32).reshape(-1)
    if kind == "mr":
        wp = m32.astype(np.float64)
    elif kind == "vad":
        wp = (m32 > threshold(m32, vad_db)).astype(np.float64)
    else:
        raise ValueError("dpcl weights: %r is neither 'mr' nor 'vad'" % (kind,))
    tot = wp.sum()
    return wp / tot if tot > 0 else np.zeros_like(wp)


def moments(z, mix, srcs, F, D, kind="mr", vad_db=DEFAULT_VAD_DB):
    """(A (D, D), Bm (D, S), C (S,) the diagonal, u, |v|, w, y) of one utterance."""
    v, nrm = embed(z, F, D)
    u = unit(v, nrm)
    y = labels_of(srcs)
    w = weights(mix, kind, vad_db)
    S = len(srcs)
    Y = np.zeros((u.shape[0], S))
    Y[np.arange(u.shape[0]), y] = 1.0
    uw = u * w[:, None]
    return uw.T @ u, uw.T @ Y, (Y * w[:, None]).sum(axis=0), u, nrm, w, y


def loss_utt(z, mix, srcs, F, D, kind="mr", vad_db=DEFAULT_VAD_DB):
    """L_j of one utterance (its rows z (T, >= F D), mix and srcs (T, F))."""
    A, Bm, C = moments(z, mix, srcs, F, D, kind, vad_db)[:3]
    return float((A * A).sum() - 2.0 * (Bm * Bm).sum() + (C * C).sum())


def loss_nxn(z, mix, srcs, F, D, kind="mr", vad_db=DEFAULT_VAD_DB):
    """The same loss in the N x N affinity form | W^1/2 (U U^T - Y Y^T) W^1/2 |_F^2 (small N only)."""
    _, _, _, u, _, w, y = moments(z, mix, srcs, F, D, kind, vad_db)
    Y = np.zeros((u.shape[0], len(srcs)))
    Y[np.arange(u.shape[0]), y] = 1.0
    sw = np.sqrt(w)
    M = (u @ u.T - Y @ Y.T) * sw[:, None] * sw[None, :]
    return float((M * M).sum())


def grad_utt(z, mix, srcs, F, D, kind="mr", vad_db=DEFAULT_VAD_DB):
    """dL_j / dz of one utterance, (T, F D) fp64 in z's column layout."""
    A, Bm, _, u, nrm, w, y = moments(z, mix, srcs, F, D, kind, vad_db)
    g = 4.0 * w[:, None] * (u @ A - Bm[:, y].T)
    inv = np.where(nrm > 0, 1.0 / np.where(nrm > 0, nrm, 1.0), 0.0)
    dv = (g - u * (u * g).sum(axis=1, keepdims=True)) * inv[:, None]
    T = np.asarray(z).shape[0]
    return dv.reshape(T, F, D).transpose(0, 2, 1).reshape(T, D * F)


def utterance_rows(lens, offs, j):
    """The packed rows of utterance j, frames ascending."""
    return np.asarray(offs)[:int(lens[j])] + j


def loss_batch(z, mix, srcs, lens, offs, F, D, kind="mr", vad_db=DEFAULT_VAD_DB, count=None):
    """Packed rows -> (loss, count, sum_j L_j, [L_j])."""
    Lj = []
    for j in range(len(lens)):
        rows = utterance_rows(lens, offs, j)
        Lj.append(loss_utt(np.asarray(z)[rows], np.asarray(mix)[rows], [np.asarray(s)[rows] for s in srcs], F, D, kind, vad_db))
    total = float(np.sum(np.array(Lj, dtype=np.float64)))
    count = float(len(lens) if count is None else count)
    return total / count, count, total, Lj


def grad_batch(z, mix, srcs, lens, offs, F, D, kind="mr", vad_db=DEFAULT_VAD_DB, count=None, gout=1.0):
    """d loss / dz on packed rows: (R, ld) fp64, zeros outside the batch's rows and the F D columns."""
    z = np.asarray(z)
    dz = np.zeros(z.shape, dtype=np.float64)
    count = float(len(lens) if count is None else count)
    for j in range(len(lens)):
        rows = utterance_rows(lens, offs, j)
        dz[rows, :F * D] = grad_utt(z[rows], np.asarray(mix)[rows], [np.asarray(s)[rows] for s in srcs], F, D, kind, vad_db) * (gout / count)
    return dz


def _gap_max(vals):
    """Best minus second best of an arg-max over vals (inf for a single candidate)."""
    if vals.size < 2:
        return np.inf
    top = np.partition(vals, -2)[-2:]
    return float(top[1] - top[0])


def kmeans(z, mix, F, D, S, iterations=DEFAULT_ITERATIONS, vad_db=DEFAULT_VAD_DB, centroids_in=None, dtype=np.float64):
    """One utterance: z (T, >= F D), mix (T, F) -> dict(labels (T, F) int32, mask (T, S F) float32, centroids (S, D) fp64,
    gap_init, gap_assign: the smallest decision gaps met (inf where no decision was taken), point_gap (T, F): every point's gap
    between its two nearest centroids in the final assignment).  dtype: the arithmetic; float64 is the definition, float32
    the error model the tests measure a kernel against."""
    if not 2 <= S <= MAX_S:
        raise ValueError("dpcl kmeans: S = %d clusters outside 2..%d" % (S, MAX_S))
    if iterations < 0:
        raise ValueError("dpcl kmeans: iterations = %d is negative" % iterations)
    v, nrm = embed(z, F, D, dtype)
    u = unit(v, nrm)
    T = np.asarray(z).shape[0]
    m32 = np.asarray(mix, dtype=np.float32).reshape(-1)
    active = m32 > threshold(m32, vad_db)
    w = np.where(active, m32.astype(dtype), dtype(0.0))
    act = np.flatnonzero(active)
    gap_init, gap_assign = np.inf, np.inf
    if centroids_in is not None:
        cent = np.array(centroids_in, dtype=dtype).reshape(S, D)
    else:
        cent = np.zeros((S, D), dtype=dtype)
        if act.size:
            vals = m32[act].astype(np.float64)
            cent[0] = u[act[int(np.argmax(vals))]]           # (argmax: the first maximum, act ascending)
            gap_init = min(gap_init, _gap_max(vals))
        for k in range(1, S):
            if act.size <= k:
                cent[k] = cent[0]
                continue
            d2 = ((u[act][:, None, :] - cent[None, :k, :]) ** 2).sum(axis=2).min(axis=1)
            cent[k] = u[act[int(np.argmax(d2))]]
            gap_init = min(gap_init, _gap_max(d2))

    def assign(c):
        d2 = ((u[:, None, :] - c[None, :, :]) ** 2).sum(axis=2)           # (N, S)
        srt = np.sort(d2, axis=1)
        return np.argmin(d2, axis=1), srt[:, 1] - srt[:, 0]                # (argmin: the first minimum)

    for _ in range(int(iterations)):
        lab, gaps = assign(cent)
        gap_assign = min(gap_assign, float(gaps.min()))
        for k in range(S):
            sel = (lab == k) & active
            tot = w[sel].sum()
            if tot > 0:
                cent[k] = (u[sel] * w[sel][:, None]).sum(axis=0) / tot
    lab, gaps = assign(cent)
    gap_assign = min(gap_assign, float(gaps.min()))
    labels = lab.reshape(T, F).astype(np.int32)
    mask = np.zeros((T, S * F), dtype=np.float32)
    for k in range(S):
        mask[:, k * F:(k + 1) * F] = labels == k
    return dict(labels=labels, mask=mask, centroids=cent, gap_init=gap_init, gap_assign=gap_assign, point_gap=gaps.reshape(T, F))


def kmeans_batch(z, mix, lens, offs, F, D, S, iterations=DEFAULT_ITERATIONS, vad_db=DEFAULT_VAD_DB, centroids_in=None, dtype=np.float64):
    """Packed rows -> dict(labels (R, F), mask (R, S F), centroids (B, S, D), gap_init, gap_assign, point_gap (R, F))."""
    z, mix = np.asarray(z), np.asarray(mix)
    R = int(np.sum(lens))
    out = dict(labels=np.zeros((R, F), dtype=np.int32), mask=np.zeros((R, S * F), dtype=np.float32),
               centroids=np.zeros((len(lens), S, D)), gap_init=np.inf, gap_assign=np.inf, point_gap=np.zeros((R, F)))
    for j in range(len(lens)):
        rows = utterance_rows(lens, offs, j)
        r = kmeans(z[rows], mix[rows], F, D, S, iterations, vad_db, None if centroids_in is None else np.asarray(centroids_in)[j], dtype)
        out["labels"][rows], out["mask"][rows], out["centroids"][j], out["point_gap"][rows] = r["labels"], r["mask"], r["centroids"], r["point_gap"]
        out["gap_init"], out["gap_assign"] = min(out["gap_init"], r["gap_init"]), min(out["gap_assign"], r["gap_assign"])
    return out
