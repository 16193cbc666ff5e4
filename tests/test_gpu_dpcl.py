"""sk_dpcl_fwd / sk_dpcl_bwd / sk_dpcl_kmeans on the MI355X against sepkern/dpcl.py's numpy fp64 definition.

Cases and gates: tests/_dpcl_cases.py (tests/test_dpcl.py shows on any machine that they catch a wrong kernel).
    loss       |L_j - L_j^fp64| / |C|_F^2 <= 4 x the error of the float32 CPU evaluation of the same formula (floor 4 * 2^-24)
    dz         relative L2 per utterance against the fp64 gradient <= 4 x the float32 CPU evaluation's
    k-means    labels and masks EXACTLY the reference's (its decision gaps are asserted wide), centroids within the 4 x rule
Every figure is printed before it is asserted (pytest -s shows them; profiles/dpcl.txt records them).
Shapes: the batches around a chunk boundary (CH = 8 frames), F in {5, 64, 65, 257} (the tail of a row against the 64-point
tile), (D, S) up to (40, 4) = the largest padded tile, ld = F D and F D + 8, both weightings.
The kernels' own edges -- the Gram-tile and backward-block edges of (D, S), multi-chunk ragged batches, the wave trips of a chunk,
the pick ties, ab and stats against the definition -- are pinned in tests/test_gpu_dpcl_cases.py (claims and defect models:
tests/test_dpcl_cases.py).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _dpcl_cases as DC
from sepkern import dpcl

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch.device("cuda", 0)


def _pk(lens, dev):
    from sepkern.packing import Packing
    return Packing(np.asarray(lens, dtype=np.int32), dev)


def _up(c, dev):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t(c["z"]), t(c["mix"]), [t(s) for s in c.get("srcs", [])]


def _loss_run(c, dev, kind, alloc_rows=0):
    """-> (res of ops.dpcl_fwd, dz (R + alloc_rows, ld) written into a sentinel-filled buffer) for the case c."""
    from sepkern import ops
    z, mix, srcs = _up(c, dev)
    pk = _pk(c["lens"], dev)
    if alloc_rows:                                   # a row buffer longer than the batch: the tail rows are not the kernels'
        z = torch.cat([z, torch.full((alloc_rows, z.shape[1]), SENTINEL, device=dev)])
        mix = torch.cat([mix, torch.full((alloc_rows, mix.shape[1]), SENTINEL, device=dev)])
        srcs = [torch.cat([s, torch.full((alloc_rows, s.shape[1]), SENTINEL, device=dev)]) for s in srcs]
    res = ops.dpcl_fwd(z, mix, srcs, pk, c["D"], kind)
    dz = torch.full_like(z, SENTINEL)
    ops.dpcl_bwd(z, mix, srcs, pk, c["D"], res, torch.ones(1, device=dev), kind, out=dz)
    return res, dz


def _check_loss_case(c, dev, kind, pad, worst):
    F, D, B, R = c["F"], c["D"], len(c["lens"]), c["R"]
    res, dz = _loss_run(c, dev, kind, alloc_rows=3 if pad else 0)
    lj, out, dz = res["lj"].cpu().numpy(), res["out"].cpu().numpy().astype(np.float64), dz.cpu().numpy()
    # padded rows and columns stay untouched
    assert np.all(dz[R:] == SENTINEL) and np.all(dz[:, F * D:] == SENTINEL)
    refs = [DC.loss_ref(c, j, kind) for j in range(B)]
    total, budget = float(np.sum([r[0] for r in refs])), 0.0
    for j in range(B):
        L, c2, g, gs = refs[j]
        L32, g32 = DC.loss_f32(c, j, kind)
        rows = dpcl.utterance_rows(c["lens"], c["offs"], j)
        err, e32 = abs(lj[j] - L) / c2, abs(L32 - L) / c2
        gerr, ge32 = DC.rel_l2(dz[rows, :F * D] * B, g, gs), DC.rel_l2(g32, g, gs)           # (dz carries 1 / count)
        print("dpcl %-9s F=%3d D=%2d S=%d %-3s pad=%d utt %d: loss err %.3g (f32 %.3g, ratio %.2f)  dz err %.3g (f32 %.3g, ratio %.2f)"
              % (c["batch"], F, D, c["S"], kind, pad, j, err, e32, err / DC.gate(e32) * DC.FACTOR, gerr, ge32, gerr / DC.gate(ge32) * DC.FACTOR))
        worst[0], worst[1] = max(worst[0], err / max(e32, DC.FLOOR)), max(worst[1], gerr / max(ge32, DC.FLOOR))
        assert err <= DC.gate(e32), (j, err, e32)
        assert gerr <= DC.gate(ge32), (j, gerr, ge32)
        budget += (DC.gate(e32) + 2.0 ** -23) * c2
    # the batch output: the utterances' sum (each within its gate; one float32 rounding of the stored value), its mean, the count
    assert out[1] == B and abs(out[2] - total) <= budget and abs(out[0] - total / B) <= budget / B


@pytest.mark.parametrize("F", DC.BINS)
@pytest.mark.parametrize("batch", list(DC.BATCHES))
def test_loss_and_gradient_match_the_definition(dev, batch, F):
    """Every (D, S), both weightings; ld = F D and F D + 8 alternate over the weightings and back."""
    worst = [0.0, 0.0]
    for i, (D, S) in enumerate(DC.DS):
        for k, kind in enumerate(DC.WEIGHTS):
            for pad in (0, 8):
                c = dict(DC.loss_case(batch, F, D, S, pad), batch=batch)
                _check_loss_case(c, dev, kind, pad, worst)
    print("dpcl %s F=%d: worst ratio to the float32 model: loss %.2f, dz %.2f (gate %.0f)" % (batch, F, worst[0], worst[1], DC.FACTOR))


@pytest.mark.parametrize("kind", DC.WEIGHTS)
def test_all_zero_utterance_inside_a_batch(dev, kind):
    c = dict(DC.loss_case("ragged", 65, 20, 3, 0, 2), batch="ragged")
    res, dz = _loss_run(c, dev, kind)
    lj, dz = res["lj"].cpu().numpy(), dz.cpu().numpy()
    rows = dpcl.utterance_rows(c["lens"], c["offs"], 2)
    assert lj[2] == 0.0 and np.all(dz[rows] == 0.0) and np.all(np.isfinite(dz)) and np.all(np.isfinite(lj))
    for j in (0, 1, 3):                              # the others are what they are without it
        L, c2 = DC.loss_ref(c, j, kind)[:2]
        assert abs(lj[j] - L) / c2 <= DC.gate(abs(DC.loss_f32(c, j, kind)[0] - L) / c2)


@pytest.mark.parametrize("kind", DC.WEIGHTS)
def test_loss_bits_do_not_depend_on_the_launch_the_batch_or_ld(dev, kind):
    from sepkern import ops
    F, D, S = 257, 40, 4
    c = dict(DC.loss_case("ragged", F, D, S), batch="ragged")
    res, dz = _loss_run(c, dev, kind)
    res2, dz2 = _loss_run(c, dev, kind)
    for k in ("lj", "ab", "stats", "out"):
        assert torch.equal(res[k], res2[k]), k
    assert torch.equal(dz, dz2)
    # ld padded against unpadded
    cp = dict(DC.loss_case("ragged", F, D, S, 8), batch="ragged")
    np.testing.assert_array_equal(cp["z"][:, :F * D], c["z"])
    resp, dzp = _loss_run(cp, dev, kind)
    assert torch.equal(resp["lj"], res["lj"]) and torch.equal(resp["ab"], res["ab"]) and torch.equal(dzp[:, :F * D], dz)
    # an utterance alone against the same utterance inside the batch (dz carries 1 / count: 4 against 1, a power of two)
    for j in (0, 1, 3):
        rows = dpcl.utterance_rows(c["lens"], c["offs"], j)
        alone = dict(lens=[c["lens"][j]], z=c["z"][rows], mix=c["mix"][rows], srcs=[s[rows] for s in c["srcs"]], D=D)
        ra, dza = _loss_run(alone, dev, kind)
        assert torch.equal(ra["lj"][0], res["lj"][j]) and torch.equal(ra["ab"][0], res["ab"][j]) and torch.equal(ra["stats"][0], res["stats"][j])
        assert torch.equal(dza * 0.25, dz[torch.from_numpy(rows).to(dev).long()])


def test_loss_count_and_gscale(dev):
    from sepkern import ops
    c = DC.loss_case("uniform", 64, 3, 2)
    z, mix, srcs = _up(c, dev)
    pk = _pk(c["lens"], dev)
    res = ops.dpcl_fwd(z, mix, srcs, pk, 3, count_dev=torch.full((1,), 8.0, device=dev))
    base = ops.dpcl_fwd(z, mix, srcs, pk, 3)
    assert float(res["out"][1]) == 8.0 and float(base["out"][1]) == 2.0 and torch.equal(res["out"][2], base["out"][2])
    assert abs(float(res["out"][0]) * 4 - float(base["out"][0])) <= 1e-7 * float(base["out"][0])
    g1 = ops.dpcl_bwd(z, mix, srcs, pk, 3, base, torch.ones(1, device=dev))
    g2 = ops.dpcl_bwd(z, mix, srcs, pk, 3, res, torch.full((1,), 4.0, device=dev))
    assert torch.equal(g1, g2)                        # 4 / 8 = 1 / 2: powers of two


# ------------------------------------------------------------------------------------------------ k-means
def _kmeans_run(c, dev, iterations=None, alloc_rows=0, mask_pad=0):
    from sepkern import ops
    z, mix, _ = _up(c, dev)
    pk = _pk(c["lens"], dev)
    S, F, R = c["S"], c["F"], c["R"]
    out = torch.full((R + alloc_rows, S * F + mask_pad), SENTINEL, device=dev)
    cin = None if c.get("centroids_in") is None else torch.from_numpy(c["centroids_in"]).to(dev)
    mask, labels, cent = ops.dpcl_kmeans(z, mix, pk, S, c["iterations"] if iterations is None else iterations, centroids_in=cin,
                                         out=out, D=c["D"])
    return out.cpu().numpy(), labels.cpu().numpy(), cent.cpu().numpy().astype(np.float64)


def _check_centroids(name, c, cent):
    e32, _ = DC.centroid_error_model(c)
    err = float(np.abs(cent - c["ref"]["centroids"]).max())
    print("dpcl kmeans %s: centroid err %.3g (f32 %.3g, ratio %.2f of %.0f)" % (name, err, e32, err / max(e32, DC.FLOOR), DC.FACTOR))
    assert err <= DC.gate(e32), (err, e32)


@pytest.mark.parametrize("batch,F,S,D", DC.KMEANS_CASES)
def test_kmeans_labels_are_exactly_the_reference(dev, batch, F, S, D):
    pad = 8 if D == 20 else 0
    c = DC.kmeans_case(batch, F, S, D, 20, pad)
    ref = c["ref"]
    assert ref["gap_init"] >= DC.GAP_INIT and ref["gap_assign"] >= DC.GAP_ASSIGN
    out, labels, cent = _kmeans_run(c, dev, alloc_rows=2, mask_pad=5)
    R = c["R"]
    np.testing.assert_array_equal(labels, ref["labels"])
    np.testing.assert_array_equal(out[:R, :S * F], ref["mask"])
    assert np.all(out[R:] == SENTINEL) and np.all(out[:, S * F:] == SENTINEL)
    _check_centroids("%s F=%d S=%d D=%d" % (batch, F, S, D), c, cent)
    # a second launch: the same bits
    out2, labels2, cent2 = _kmeans_run(c, dev, alloc_rows=2, mask_pad=5)
    assert np.array_equal(out, out2) and np.array_equal(labels, labels2) and np.array_equal(cent, cent2)


def test_kmeans_iterations_zero(dev):
    c = DC.kmeans_case("ragged", 257, 4, 20, 0)
    out, labels, cent = _kmeans_run(c, dev)
    np.testing.assert_array_equal(labels, c["ref"]["labels"])
    np.testing.assert_array_equal(out[:, :4 * 257], c["ref"]["mask"])
    _check_centroids("iterations=0", c, cent)


def test_kmeans_utterance_alone_and_in_a_batch_agree_bit_for_bit(dev):
    c = DC.kmeans_case("ragged", 257, 4, 40)
    out, labels, cent = _kmeans_run(c, dev)
    for j in (0, 2, 3):
        rows = dpcl.utterance_rows(c["lens"], c["offs"], j)
        alone = dict(c, lens=[c["lens"][j]], R=len(rows), z=c["z"][rows], mix=c["mix"][rows])
        o, l, ce = _kmeans_run(alone, dev)
        assert np.array_equal(o, out[rows]) and np.array_equal(l, labels[rows]) and np.array_equal(ce[0], cent[j])


def test_kmeans_one_step_on_overlapping_clusters(dev):
    c = DC.overlap_case()
    ref = c["ref"]
    sure = ref["point_gap"] >= DC.GAP_POINT
    assert 1.0 - sure.mean() <= DC.MAX_TIED_SHARE
    out, labels, cent = _kmeans_run(c, dev)
    print("dpcl kmeans overlap: %d of %d points under the gap, %d labels differ among them" %
          ((~sure).sum(), sure.size, (labels != ref["labels"])[~sure].sum()))
    np.testing.assert_array_equal(labels[sure], ref["labels"][sure])
    S, F = c["S"], c["F"]
    lab_from_mask = out[:, :S * F].reshape(-1, S, F).argmax(1)
    np.testing.assert_array_equal(lab_from_mask, labels)          # the mask is the labels', also where they may differ
    np.testing.assert_array_equal(out[:, :S * F].reshape(-1, S, F).sum(1), 1.0)
    _check_centroids("overlap", c, cent)


def test_kmeans_fewer_active_points_than_clusters(dev):
    c = DC.few_active_case()
    out, labels, cent = _kmeans_run(c, dev)
    np.testing.assert_array_equal(labels, c["ref"]["labels"])
    np.testing.assert_array_equal(out[:, :c["S"] * c["F"]], c["ref"]["mask"])
    assert np.array_equal(cent[0][2], cent[0][0]) and np.array_equal(cent[1][1], cent[1][0]) and np.array_equal(cent[1][2], cent[1][0])
    _check_centroids("few active", c, cent)
    # no active point at all: zero centroids, label 0
    from sepkern import ops
    z, _, _ = _up(c, dev)
    _, lab0, cen0 = ops.dpcl_kmeans(z, torch.zeros(c["R"], c["F"], device=dev), _pk(c["lens"], dev), 2, 3, D=c["D"])
    assert not bool(lab0.any()) and not bool(cen0.any())


# ------------------------------------------------------------------------------------------------ argument errors
def test_bad_arguments_are_sk_einval(dev):
    from sepkern import _lib
    lib = _lib.load()
    F, R = 5, 4
    buf, dzb, maskb = (torch.zeros(R, 64 * F, device=dev) for _ in range(3))
    mix = torch.zeros(R, F, device=dev)
    lens = torch.tensor([4], dtype=torch.int32, device=dev)
    offs = torch.arange(5, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    sp = (C.c_void_p * 4)(*[mix.data_ptr()] * 4)
    lj, ab, stats, out = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(1, 1760, device=dev), torch.zeros(1, 2, device=dev), torch.zeros(3, device=dev)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)

    def fwd(D, S, ld):
        return lib.sk_dpcl_fwd(p(buf), ld, p(mix), sp, p(lens), p(offs), 4, 1, F, D, S, 0, 0.01, None, p(lj), p(ab), p(stats), p(out), p(ws), None)

    def bwd(D, S, ld):
        return lib.sk_dpcl_bwd(p(buf), ld, p(mix), sp, p(lens), p(offs), 4, 1, F, D, S, 0, p(ab), p(stats), p(out), p(out), p(dzb), None)

    labels, cent = torch.zeros(R, F, dtype=torch.int32, device=dev), torch.zeros(1, 4, 40, device=dev)

    def km(D, S, ld, ld_mask=64 * F, iters=1):
        return lib.sk_dpcl_kmeans(p(buf), ld, p(mix), p(lens), p(offs), 4, 1, F, D, S, iters, 0.01, None, p(maskb), ld_mask, p(labels), p(cent), p(ws), None)

    for fn in (fwd, bwd, km):
        assert fn(41, 2, 64 * F) == -1 and b"D = 41" in lib.sk_last_error()
        assert fn(3, 5, 64 * F) == -1 and b"S = 5" in lib.sk_last_error()
        assert fn(3, 2, 3 * F - 1) == -1 and b"ld = 14" in lib.sk_last_error()
        assert fn(0, 2, 64 * F) == -1
    assert km(3, 1, 64 * F) == -1 and b"S = 1" in lib.sk_last_error()
    assert km(3, 2, 64 * F, ld_mask=2 * F - 1) == -1 and km(3, 2, 64 * F, iters=-1) == -1
    assert lib.sk_dpcl_workspace_bytes(4, 1, F, 41, 2) == 0 and lib.sk_dpcl_kmeans_workspace_bytes(4, 1, F, 3, 1) == 0
    assert lib.sk_dpcl_workspace_bytes(4, 1, F, 40, 4) > 0 and lib.sk_dpcl_kmeans_workspace_bytes(4, 1, F, 40, 4) > 0
    assert fwd(3, 2, 3 * F) == 0 and bwd(3, 2, 3 * F) == 0 and km(3, 2, 3 * F) == 0 and fwd(1, 1, F) == 0
    torch.cuda.synchronize()
