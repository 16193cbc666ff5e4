"""The kernels of csrc/dpcl.hip on the MI355X at their tile, block and chunk edges (the pin suite; tests/test_gpu_dpcl.py holds the
kernels to the definition at the shapes of the feature, tests/test_gpu_dpcl_model.py runs them through the arch).

Cases, claims, gates and defect models: tests/_dpcl_cases.py; tests/test_dpcl_cases.py proves on any machine that the cases reach
all 17 instantiations and every listed edge and that they catch the defects.

sk_dpcl_fwd / sk_dpcl_bwd / sk_dpcl_kmeans are called through the C ABI on buffers this file owns:
    the workspace has exactly the queried size between two guard bands and is filled with 0xFF (NaN as float and as double),
        afresh before every launch: a kernel that reads a chunk nobody wrote finds NaN, not an earlier launch's numbers;
    lj, ab, stats, out, dz, mask, labels and centroids lie sentinel-filled between guard bands;
    the rows of z, mix and the sources past R and the columns of z past F D are NaN.
Compared against numpy fp64 (sepkern/dpcl.py), per utterance:
    loss, dz   the gates of tests/test_gpu_dpcl.py (4 x the float32 CPU evaluation's error, floor 4 * 2^-24; the D = 1 rule kept)
    ab         [A | Bm] entry by entry, absolute, 4 x the float32 evaluation's largest error of A / Bm (floor 4 * 2^-24); the padding
               beyond (D, S) exactly 0.0; A symmetric bit for bit
    stats      1 / sum w within 8 * 2^-24 relative (DC.SC_GATE says why), the threshold exactly
    k-means    labels and masks exactly, centroids within the 4 x rule
    partials   the workspace after sk_dpcl_fwd at the restated layout: every live (j, ch) slot against that chunk's fp64 Gram matrix
               (4 x the float32 evaluation's error), every other slot still 0xFF
Bit for bit: a second launch on a freshly poisoned workspace, ld = F D against F D + 8, every utterance of the ragged multi-chunk
batch alone against inside the batch.  Every figure is printed before it is asserted (profiles/dpcl_cases.txt records them).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _dpcl_cases as DC
from sepkern import dpcl

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
GUARD = 256                           # elements on either side of every output and of the workspace
EXTRA_ROWS = 2                        # rows past R in every row buffer
RATIO = float(dpcl.vad_ratio(dpcl.DEFAULT_VAD_DB))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib():
    from sepkern import _lib
    return _lib.load()


class Pool:
    """n elements of a device buffer between two guard bands, everything filled with `fill`."""

    def __init__(self, dev, n, dtype, fill):
        self.n, self.fill = int(n), fill
        self.whole = torch.full((self.n + 2 * GUARD,), fill, dtype=dtype, device=dev)
        self.data = self.whole[GUARD:GUARD + self.n]

    def ptr(self):
        return C.c_void_p(self.data.data_ptr())

    def numpy(self):
        return self.data.cpu().numpy()

    def guards_intact(self):
        w = self.whole.cpu()
        return bool((w[:GUARD] == self.fill).all()) and bool((w[GUARD + self.n:] == self.fill).all())


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _rows_in_nan(a, dev, ld=None):
    """The (R, n) array in a (R + EXTRA_ROWS, ld) device buffer whose other rows and columns are NaN."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.full((a.shape[0] + EXTRA_ROWS, a.shape[1] if ld is None else ld), float("nan"), device=dev)
    buf[:a.shape[0], :a.shape[1]] = torch.from_numpy(a).to(dev)
    return buf


def _operands(c, dev, pad):
    F, D = c["F"], c["D"]
    z = _rows_in_nan(c["z"][:, :F * D], dev, F * D + pad)
    mix = _rows_in_nan(c["mix"], dev)
    srcs = [_rows_in_nan(s, dev) for s in c.get("srcs", [])]
    lens = torch.tensor(list(c["lens"]), dtype=torch.int32, device=dev)
    offs = torch.from_numpy(np.asarray(c["offs"], dtype=np.int32)).to(dev)
    assert offs.numel() == c["lens"][0] + 1
    return z, mix, srcs, lens, offs


# ------------------------------------------------------------------------------------------------ loss and gradient
def _loss_launch(lib, dev, c, kind, ops, count, keep_ws=False):
    z, mix, srcs, lens, offs = ops
    F, D, S, B, T = c["F"], c["D"], c["S"], len(c["lens"]), c["lens"][0]
    nbytes = lib.sk_dpcl_workspace_bytes(T, B, F, D, S)
    assert nbytes == DC.layout_of(T, B, D, S, False)["total"]
    ws = Pool(dev, nbytes, torch.uint8, 0xFF)
    lj = Pool(dev, B, torch.float64, SENTINEL)
    ab, stats, out = Pool(dev, B * DC.AB, torch.float32, SENTINEL), Pool(dev, 2 * B, torch.float32, SENTINEL), Pool(dev, 3, torch.float32, SENTINEL)
    dz = Pool(dev, z.numel(), torch.float32, SENTINEL)
    sp = (C.c_void_p * 4)(*[srcs[s].data_ptr() if s < S else None for s in range(4)])
    wk = DC.WEIGHTS.index(kind)
    one = torch.ones(1, device=dev)
    cd = None if count is None else torch.full((1,), float(count), device=dev)
    rc = lib.sk_dpcl_fwd(_p(z), z.shape[1], _p(mix), sp, _p(lens), _p(offs), T, B, F, D, S, wk, RATIO, _p(cd), lj.ptr(), ab.ptr(),
                         stats.ptr(), out.ptr(), ws.ptr(), None)
    assert rc == 0, lib.sk_last_error()
    rc = lib.sk_dpcl_bwd(_p(z), z.shape[1], _p(mix), sp, _p(lens), _p(offs), T, B, F, D, S, wk, ab.ptr(), stats.ptr(), out.ptr(),
                         _p(one), dz.ptr(), None)
    assert rc == 0, lib.sk_last_error()
    torch.cuda.synchronize()
    for name, pool in (("ws", ws), ("lj", lj), ("ab", ab), ("stats", stats), ("out", out), ("dz", dz)):
        assert pool.guards_intact(), "%s: a guard band was written" % name
    res = dict(lj=lj.numpy(), ab=ab.numpy().reshape(B, DC.AB), stats=stats.numpy().reshape(B, 2), out=out.numpy(),
               dz=dz.numpy().reshape(z.shape))
    if keep_ws:
        res["ws"] = ws.numpy()
    return res


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _same_bits(a, b, keys):
    return all(a[k].shape == b[k].shape and _bits(a[k]) == _bits(b[k]) for k in keys)


def _loss_run(lib, dev, c, kind, pad, count=None):
    """Two launches, each on a freshly poisoned workspace and fresh outputs: the same bits, nothing outside the batch's rows and
    columns written, nothing NaN -> the first launch's results."""
    ops = _operands(c, dev, pad)
    a = _loss_launch(lib, dev, c, kind, ops, count)
    b = _loss_launch(lib, dev, c, kind, ops, count)
    assert _same_bits(a, b, ("lj", "ab", "stats", "out", "dz")), "a second launch gave other bits"
    R, FD = c["R"], c["F"] * c["D"]
    assert np.all(a["dz"][R:] == SENTINEL) and np.all(a["dz"][:, FD:] == SENTINEL)
    for k in ("lj", "ab", "stats", "out"):
        assert np.all(np.isfinite(a[k])), k
    assert np.all(np.isfinite(a["dz"][:R, :FD]))
    return a


def _check_loss(c, kind, res, worst, tag):
    key, F, D, S, B = c["key"], c["F"], c["D"], c["S"], len(c["lens"])
    pad_mask = DC.ab_padding(D, S)
    total, budget = 0.0, 0.0
    for j in range(B):
        r, (e_l, e_g, e_ab) = DC.reference(key, j, kind), DC.f32_errors(key, j, kind)
        rows = dpcl.utterance_rows(c["lens"], c["offs"], j)
        err = abs(res["lj"][j] - r["L"]) / r["c2"]
        gerr = DC.rel_l2(res["dz"][rows, :F * D].astype(np.float64) * B, r["dz"], r["scale"])   # (dz carries 1 / count)
        ab = res["ab"][j]
        aerr = float(np.abs(ab.astype(np.float64) - r["ab"]).max())
        serr = abs(float(res["stats"][j, 0]) - r["sc"]) / r["sc"]
        ratios = (err / max(e_l, DC.FLOOR), gerr / max(e_g, DC.FLOOR), aerr / max(e_ab, DC.FLOOR), serr / DC.FLOOR)
        print("dpcl_cases %-13s F=%2d D=%2d S=%d %-3s %s utt %d: loss %.3g (f32 %.3g, ratio %.2f)  dz %.3g (f32 %.3g, ratio %.2f)  "
              "ab %.3g (f32 %.3g, ratio %.2f)  1/sum w %.2f x 2^-24" % (key[0], F, D, S, kind, tag, j, err, e_l, ratios[0], gerr, e_g,
                                                                      ratios[1], aerr, e_ab, ratios[2], ratios[3]))
        for i in range(4):
            worst[i] = max(worst[i], ratios[i])
        assert err <= DC.gate(e_l), (j, err, e_l)
        assert gerr <= DC.gate(e_g), (j, gerr, e_g)
        assert aerr <= DC.gate(e_ab), (j, aerr, e_ab)
        assert serr <= DC.SC_GATE, (j, serr)
        assert np.float32(res["stats"][j, 1]) == np.float32(r["thr"]), (j, res["stats"][j, 1], r["thr"])
        assert np.all(ab[pad_mask] == 0.0), "ab of utterance %d is not zero beyond (D, S)" % j
        A = ab[:DC.DMAX * DC.DMAX].reshape(DC.DMAX, DC.DMAX)
        assert _bits(A) == _bits(A.T), "A of utterance %d is not symmetric bit for bit" % j
        total += r["L"]
        budget += (DC.gate(e_l) + 2.0 ** -23) * r["c2"]
    out = res["out"].astype(np.float64)
    assert out[1] == B and abs(out[2] - total) <= budget and abs(out[0] - total / B) <= budget / B


GEOMETRY_IDS = ["%s-F%d" % g for g in DC.GEOMETRIES]


@pytest.mark.parametrize("batch,F", list(DC.GEOMETRIES), ids=GEOMETRY_IDS)
def test_loss_gradient_ab_and_stats_at_the_edges(lib, dev, batch, F):
    """Every loss case of the geometry, both weightings, ld = F D and F D + 8 (the same bits)."""
    worst = [0.0, 0.0, 0.0, 0.0]
    for key in [k for k in DC.LOSS_CASES if k[:2] == (batch, F)]:
        for kind in DC.WEIGHTS:
            res = _loss_run(lib, dev, DC.edge_case(*key), kind, 0)
            _check_loss(DC.edge_case(*key), kind, res, worst, "ld=FD  ")
            resp = _loss_run(lib, dev, DC.edge_case(*key), kind, 8)
            _check_loss(DC.edge_case(*key), kind, resp, worst, "ld=FD+8")
            FD = key[1] * key[2]
            assert _same_bits(res, resp, ("lj", "ab", "stats", "out")) and _bits(res["dz"][:, :FD]) == _bits(resp["dz"][:, :FD])
    print("dpcl_cases %s F=%d: worst ratio to the float32 model: loss %.2f, dz %.2f, ab %.2f (gate %.0f); 1/sum w %.2f x 2^-24 (gate 8)"
          % (batch, F, worst[0], worst[1], worst[2], DC.FACTOR, worst[3]))


ALONE_KEYS = (("chunks_ragged", 65, 13, 4), ("chunks_ragged", 65, 33, 2), ("chunks_ragged", 5, 16, 2))


@pytest.mark.parametrize("key", ALONE_KEYS, ids=["%s-F%d-D%d-S%d" % k for k in ALONE_KEYS])
def test_an_utterance_of_the_ragged_batch_alone_gives_the_batchs_bits(lib, dev, key):
    """lens = [19, 17, 9, 8, 3]: nch = 3, 3, 2, 1, 1 against nchmax = 3.  Alone, every utterance is the whole grid and its partials
    have another pitch; B = 5 is no power of two, so the lone run takes a count_dev of 5 and dz is compared exactly."""
    c = DC.edge_case(*key)
    B = len(c["lens"])
    for kind in DC.WEIGHTS:
        res = _loss_run(lib, dev, c, kind, 0)
        for j in range(B):
            rows = dpcl.utterance_rows(c["lens"], c["offs"], j)
            alone = dict(c, lens=[c["lens"][j]], offs=DC.offsets([c["lens"][j]]), R=len(rows), z=c["z"][rows], mix=c["mix"][rows],
                         srcs=[s[rows] for s in c["srcs"]])
            ra = _loss_run(lib, dev, alone, kind, 0, count=B)
            assert ra["out"][1] == B
            for k in ("lj", "ab", "stats"):
                assert _bits(ra[k][0]) == _bits(res[k][j]), (k, kind, j)
            assert _bits(ra["dz"][:len(rows)]) == _bits(res["dz"][rows]), (kind, j)


PARTIAL_KEYS = (("chunks_ragged", 65, 13, 4), ("chunks_ragged", 5, 40, 4), ("chunks_ragged", 33, 16, 1))


@pytest.mark.parametrize("key", PARTIAL_KEYS, ids=["%s-F%d-D%d-S%d" % k for k in PARTIAL_KEYS])
def test_partials_are_the_chunks_gram_matrices_and_unwritten_slots_stay_poisoned(lib, dev, key):
    """The workspace after sk_dpcl_fwd, read at the restated layout: the partial of (j, ch) is the fp64 Gram matrix of that chunk
    within 4 x the float32 evaluation's error (relative to sqrt(G_aa G_bb); floor 4 * 2^-24), zero columns exactly zero; the
    slots of chunks past an utterance's own -- partials and chunk maxima -- still hold 0xFF; the thresholds are the definition's."""
    c = DC.edge_case(*key)
    F, D, S, B, T = c["F"], c["D"], c["S"], len(c["lens"]), c["lens"][0]
    NT, nchmax, lay = DC.tiles_of(D, S), DC.chunks_of(T), DC.layout_of(T, B, D, S, False)
    NP, worst = DC.npairs(NT, False), 0.0
    for kind in DC.WEIGHTS:
        ws = _loss_launch(lib, dev, c, kind, _operands(c, dev, 0), None, keep_ws=True)["ws"]
        raw = ws[lay["partial"]:lay["partial"] + B * nchmax * NP * 256 * 8].reshape(B, nchmax, NP * 256 * 8)
        cmax = ws[lay["cmax"]:lay["cmax"] + B * nchmax * 4].reshape(B, nchmax, 4)
        for j, n in enumerate(c["lens"]):
            grams, grams32 = DC.chunk_grams(c, j, kind), DC.chunk_grams_f32(c, j, kind)
            rows = dpcl.utterance_rows(c["lens"], c["offs"], j)
            for ch in range(nchmax):
                if ch >= DC.chunks_of(n):
                    assert np.all(raw[j, ch] == 0xFF), "partial of (%d, %d) was written" % (j, ch)
                    assert kind == "mr" or np.all(cmax[j, ch] == 0xFF), "chunk maximum of (%d, %d) was written" % (j, ch)
                    continue
                tiles = raw[j, ch].copy().view(np.float64).reshape(NP, 16, 16)
                G, p = np.zeros((16 * NT, 16 * NT)), 0
                for ti in range(NT):
                    for tj in range(ti, NT):
                        G[ti * 16:(ti + 1) * 16, tj * 16:(tj + 1) * 16] = tiles[p]
                        G[tj * 16:(tj + 1) * 16, ti * 16:(ti + 1) * 16] = tiles[p].T
                        p += 1
                err, e32 = DC.gram_error(G, grams[ch]), DC.gram_error(grams32[ch], grams[ch])
                worst = max(worst, err / max(e32, DC.FLOOR))
                assert err <= DC.gate(e32), (kind, j, ch, err, e32)
                if kind == "vad":
                    frames = rows[ch * DC.CH:(ch + 1) * DC.CH]
                    assert cmax[j, ch].copy().view(np.float32)[0] == c["mix"][frames].max(), (j, ch)
            if kind == "vad":
                thr = ws[lay["thr"] + 4 * j:lay["thr"] + 4 * j + 4].copy().view(np.float32)[0]
                assert thr == dpcl.threshold(c["mix"][rows], dpcl.DEFAULT_VAD_DB), j
            else:                                    # mr launches neither threshold kernel: both blocks keep the poison
                assert np.all(ws[lay["cmax"]:lay["partial"]] == 0xFF)
    print("dpcl_cases partials %s F=%d D=%d S=%d: worst ratio to the float32 model %.2f (gate %.0f)" % (key + (worst, DC.FACTOR)))


# ------------------------------------------------------------------------------------------------ k-means
def _kmeans_launch(lib, dev, c, ops, iterations, mask_pad):
    z, mix, _, lens, offs = ops
    F, D, S, B, T, R = c["F"], c["D"], c["S"], len(c["lens"]), c["lens"][0], c["R"]
    nbytes = lib.sk_dpcl_kmeans_workspace_bytes(T, B, F, D, S)
    assert nbytes == DC.layout_of(T, B, D, S, True)["total"]
    ws = Pool(dev, nbytes, torch.uint8, 0xFF)
    ld_mask = S * F + mask_pad
    mask = Pool(dev, (R + EXTRA_ROWS) * ld_mask, torch.float32, SENTINEL)
    labels = Pool(dev, R * F, torch.int32, -7)
    cent = Pool(dev, B * S * D, torch.float32, SENTINEL)
    rc = lib.sk_dpcl_kmeans(_p(z), z.shape[1], _p(mix), _p(lens), _p(offs), T, B, F, D, S, iterations, RATIO, None, mask.ptr(), ld_mask,
                            labels.ptr(), cent.ptr(), ws.ptr(), None)
    assert rc == 0, lib.sk_last_error()
    torch.cuda.synchronize()
    for name, pool in (("ws", ws), ("mask", mask), ("labels", labels), ("centroids", cent)):
        assert pool.guards_intact(), "%s: a guard band was written" % name
    return dict(mask=mask.numpy().reshape(R + EXTRA_ROWS, ld_mask), labels=labels.numpy().reshape(R, F), cent=cent.numpy().reshape(B, S, D))


def _kmeans_run(lib, dev, c, pad=0, mask_pad=5):
    ops = _operands(c, dev, pad)
    a = _kmeans_launch(lib, dev, c, ops, c["iterations"], mask_pad)
    b = _kmeans_launch(lib, dev, c, ops, c["iterations"], mask_pad)
    assert _same_bits(a, b, ("mask", "labels", "cent")), "a second launch gave other bits"
    R, SF = c["R"], c["S"] * c["F"]
    assert np.all(a["mask"][R:] == SENTINEL) and np.all(a["mask"][:, SF:] == SENTINEL)      # rows past R, columns past S F
    assert np.all(np.isfinite(a["cent"]))
    return a


def _check_kmeans(name, c, res):
    ref, R, SF = c["ref"], c["R"], c["S"] * c["F"]
    np.testing.assert_array_equal(res["labels"], ref["labels"])
    np.testing.assert_array_equal(res["mask"][:R, :SF], ref["mask"])
    e32, _ = DC.centroid_error_model(c)
    err = float(np.abs(res["cent"].astype(np.float64) - ref["centroids"]).max())
    print("dpcl_cases kmeans %s: centroid err %.3g (f32 %.3g, ratio %.2f of %.0f)" % (name, err, e32, err / max(e32, DC.FLOOR), DC.FACTOR))
    assert err <= DC.gate(e32), (err, e32)


@pytest.mark.parametrize("batch,F,S,D", DC.KMEANS_EDGE_CASES)
def test_kmeans_on_the_ragged_batch_at_the_tile_edges(lib, dev, batch, F, S, D):
    c = DC.kmeans_case(batch, F, S, D)
    assert c["ref"]["gap_init"] >= DC.GAP_INIT and c["ref"]["gap_assign"] >= DC.GAP_ASSIGN
    res = _kmeans_run(lib, dev, c, pad=8 if D % 2 else 0)
    _check_kmeans("%s F=%d S=%d D=%d" % (batch, F, S, D), c, res)


@pytest.mark.parametrize("iterations", (0, 1, 20))
@pytest.mark.parametrize("batch,F,S,D", DC.KMEANS_ITERATION_CASES)
def test_kmeans_iteration_counts(lib, dev, batch, F, S, D, iterations):
    c = DC.kmeans_case(batch, F, S, D, iterations)
    assert c["ref"]["gap_init"] >= DC.GAP_INIT and c["ref"]["gap_assign"] >= DC.GAP_ASSIGN
    _check_kmeans("%s F=%d S=%d D=%d iterations=%d" % (batch, F, S, D, iterations), c, _kmeans_run(lib, dev, c))


@pytest.mark.parametrize("batch,F,S,D", DC.KMEANS_ITERATION_CASES)
def test_kmeans_utterance_alone_gives_the_batchs_bits(lib, dev, batch, F, S, D):
    c = DC.kmeans_case(batch, F, S, D)
    res = _kmeans_run(lib, dev, c)
    for j in range(len(c["lens"])):
        rows = dpcl.utterance_rows(c["lens"], c["offs"], j)
        alone = dict(c, lens=[c["lens"][j]], offs=DC.offsets([c["lens"][j]]), R=len(rows), z=c["z"][rows], mix=c["mix"][rows])
        ra = _kmeans_run(lib, dev, alone)
        n = len(rows)
        assert _bits(ra["mask"][:n]) == _bits(res["mask"][rows]) and _bits(ra["labels"]) == _bits(res["labels"][rows]), j
        assert _bits(ra["cent"][0]) == _bits(res["cent"][j]), j


def test_pick_ties_go_to_the_lowest_point_index(lib, dev):
    """Two points per utterance share the largest mix: across the lanes of a wave, across waves, across chunks (iterations = 0:
    the centroids are the initialisation)."""
    c = DC.tie_case()
    assert c["later_gap"] >= DC.GAP_INIT and c["ref"]["gap_assign"] >= DC.GAP_ASSIGN
    res = _kmeans_run(lib, dev, c)
    e32, _ = DC.centroid_error_model(c)
    for j in range(len(c["lens"])):
        lo, hi = DC.tie_unit_vectors(c, j)
        got = res["cent"][j][0].astype(np.float64)
        print("dpcl_cases tie utt %d: centroid 0 is %.3g from the lower point's unit vector, %.3g from the higher's (gate %.3g)"
              % (j, np.abs(got - lo).max(), np.abs(got - hi).max(), DC.gate(e32)))
        assert np.abs(got - lo).max() <= DC.gate(e32) and np.abs(got - hi).max() >= 1e-2
    _check_kmeans("tie", c, res)
