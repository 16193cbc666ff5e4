"""Deep clustering on any machine: sepkern/dpcl.py is what it says, and the cases of tests/test_gpu_dpcl.py can catch a wrong kernel.

1. The low-rank loss equals the N x N affinity form; the closed-form gradient equals torch fp64 autograd of the definition.
2. The stated edge cases: an all-zero mixture, ties between sources, a zero embedding.
3. The k-means reference: empty clusters, fewer active points than clusters, centroids_in, iterations = 0.
4. The conf keys.
5. The builder's cases keep the reference's decision gaps wide; the overlapping case has few points near a tie.
6. Five defect models of a kernel leave at least 10 x what the GPU test tolerates, on the GPU test's own cases.
"""
import os
import sys

import numpy as np
import pytest
import torch

import _dpcl_cases as DC
from conftest import PKG
from sepkern import dpcl

sys.path.insert(0, os.path.join(PKG, "archs"))


def _small(S, seed=0, T=3, F=4, D=3):
    rng = np.random.default_rng([seed, S])
    z = (1.0 / (1.0 + np.exp(-rng.standard_normal((T, F * D))))).astype(np.float32)
    mix = np.abs(rng.standard_normal((T, F))).astype(np.float32)
    srcs = [np.abs(rng.standard_normal((T, F))).astype(np.float32) for _ in range(S)]
    return z, mix, srcs, F, D


# ------------------------------------------------------------------------------------------------ 1: the two forms, the gradient
@pytest.mark.parametrize("kind", dpcl.WEIGHTS)
@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_low_rank_loss_is_the_affinity_form(S, kind):
    z, mix, srcs, F, D = _small(S)
    a, b = dpcl.loss_utt(z, mix, srcs, F, D, kind, 6.0), dpcl.loss_nxn(z, mix, srcs, F, D, kind, 6.0)
    assert abs(a - b) <= 1e-14 * max(1.0, abs(b)), (a, b)
    assert a > 0


def _torch_loss(z, mix, srcs, F, D, kind, vad_db):
    """The definition written with torch operations on an fp64 leaf (autograd's view of it)."""
    T = z.shape[0]
    v = z[:, :F * D].view(T, D, F).permute(0, 2, 1).reshape(T * F, D)
    u = v / v.pow(2).sum(1, keepdim=True).sqrt()
    w = torch.from_numpy(dpcl.weights(mix, kind, vad_db))
    y = torch.from_numpy(dpcl.labels_of(srcs))
    Y = torch.zeros(T * F, len(srcs), dtype=torch.float64)
    Y[torch.arange(T * F), y] = 1.0
    sw = w.sqrt()
    M = (u @ u.t() - Y @ Y.t()) * sw[:, None] * sw[None, :]
    return M.pow(2).sum()


@pytest.mark.parametrize("kind", dpcl.WEIGHTS)
@pytest.mark.parametrize("S", [1, 2, 4])
def test_closed_form_gradient_is_autograd_of_the_definition(S, kind):
    z, mix, srcs, F, D = _small(S, seed=3)
    zt = torch.from_numpy(z.astype(np.float64)).requires_grad_(True)
    _torch_loss(zt, mix, srcs, F, D, kind, 6.0).backward()
    got = dpcl.grad_utt(z, mix, srcs, F, D, kind, 6.0)
    assert np.abs(got - zt.grad.numpy()).max() <= 1e-14 * max(1.0, np.abs(got).max())
    assert np.abs(got).max() > 1e-4


def test_batch_loss_and_gradient_follow_the_packed_rows_and_the_count():
    c = DC.loss_case("ragged", 5, 3, 2)
    loss, count, total, Lj = dpcl.loss_batch(c["z"], c["mix"], c["srcs"], c["lens"], c["offs"], 5, 3)
    assert count == 4 and abs(loss - total / 4) < 1e-18 and len(Lj) == 4
    rows = dpcl.utterance_rows(c["lens"], c["offs"], 1)
    assert rows.tolist() == [1, 5, 8, 11, 14]
    assert Lj[1] == dpcl.loss_utt(c["z"][rows], c["mix"][rows], [s[rows] for s in c["srcs"]], 5, 3)
    dz = dpcl.grad_batch(c["z"], c["mix"], c["srcs"], c["lens"], c["offs"], 5, 3, count=8, gout=2.0)
    np.testing.assert_array_equal(dz[rows, :15], dpcl.grad_utt(c["z"][rows], c["mix"][rows], [s[rows] for s in c["srcs"]], 5, 3) * 0.25)
    assert dpcl.loss_batch(c["z"], c["mix"], c["srcs"], c["lens"], c["offs"], 5, 3, count=8)[0] == total / 8


# ------------------------------------------------------------------------------------------------ 2: stated edge cases
@pytest.mark.parametrize("kind", dpcl.WEIGHTS)
def test_all_zero_mixture_gives_zero_loss_and_gradient(kind):
    z, mix, srcs, F, D = _small(2)
    mix[:] = 0.0
    assert dpcl.loss_utt(z, mix, srcs, F, D, kind) == 0.0
    g = dpcl.grad_utt(z, mix, srcs, F, D, kind)
    assert np.all(g == 0.0)


def test_ties_between_sources_go_to_the_lowest():
    a = np.array([[1.0, 2.0, 3.0]], dtype=np.float32)
    assert dpcl.labels_of([a, a, a]).tolist() == [0, 0, 0]
    b = np.array([[1.0, 3.0, 3.0]], dtype=np.float32)
    assert dpcl.labels_of([b, a, a * 2]).tolist() == [2, 2, 2]
    assert dpcl.labels_of([a, b]).tolist() == [0, 1, 0]


def test_zero_embedding_gives_zero_gradient_not_nan():
    z, mix, srcs, F, D = _small(2)
    z[1, 2::F] = 0.0                                  # every dimension of point (row 1, bin 2)
    L, g = dpcl.loss_utt(z, mix, srcs, F, D), dpcl.grad_utt(z, mix, srcs, F, D)
    assert np.isfinite(L) and np.all(np.isfinite(g)) and np.all(g[1, 2::F] == 0.0) and np.abs(g).max() > 0


def test_vad_threshold_is_one_float32_product():
    mix = np.array([[0.3, 0.0031, 0.0029, 0.003]], dtype=np.float32)
    thr = dpcl.threshold(mix, 40.0)
    assert thr.dtype == np.float32 and thr == np.float32(np.float32(0.01) * np.float32(0.3))
    w = dpcl.weights(mix, "vad", 40.0)
    active = mix.reshape(-1) > thr                    # a float32 comparison: 0.003 against fl32(fl32(0.01) * fl32(0.3))
    assert active[:2].all() and not active[2] and (w > 0).tolist() == active.tolist()
    np.testing.assert_array_equal(w[active], 1.0 / active.sum())


# ------------------------------------------------------------------------------------------------ 3: the k-means reference
def _two_blobs(n=40, F=4, D=2):
    rng = np.random.default_rng(5)
    which = rng.integers(0, 2, (n, F))
    proto = np.array([[0.9, 0.1], [0.1, 0.9]])
    v = np.clip(proto[which] + 0.02 * rng.standard_normal((n, F, D)), 0.01, 0.99)
    mix = (0.2 + rng.uniform(0, 0.7, (n, F))).astype(np.float32)
    mix[0, 0] = 1.0
    return v.transpose(0, 2, 1).reshape(n, D * F).astype(np.float32), mix, which, F, D


def test_kmeans_finds_the_blobs_and_writes_upit_masks():
    z, mix, which, F, D = _two_blobs()
    r = dpcl.kmeans(z, mix, F, D, 2)
    lab = r["labels"]
    assert np.array_equal(lab, which) or np.array_equal(lab, 1 - which)
    assert r["mask"].shape == (40, 2 * F) and set(np.unique(r["mask"])) == {0.0, 1.0}
    np.testing.assert_array_equal(r["mask"][:, :F] + r["mask"][:, F:], 1.0)
    np.testing.assert_array_equal(r["mask"][:, F:], lab == 1)
    assert r["gap_init"] >= 1e-4 and r["gap_assign"] >= 1e-2
    # centroid 0 is the unit vector of the loudest active point
    v0 = z[0, 0::F].astype(np.float64)
    np.testing.assert_allclose(dpcl.kmeans(z, mix, F, D, 2, iterations=0)["centroids"][0], v0 / np.linalg.norm(v0), rtol=1e-15)


def test_kmeans_iterations_zero_is_the_initialisation_and_one_assignment():
    z, mix, _, F, D = _two_blobs()
    r0 = dpcl.kmeans(z, mix, F, D, 2, iterations=0)
    u = dpcl.unit(*dpcl.embed(z, F, D))
    d2 = ((u[:, None, :] - r0["centroids"][None]) ** 2).sum(2)
    np.testing.assert_array_equal(r0["labels"].reshape(-1), d2.argmin(1))
    # the centroids are points of the data: farthest-first picks the second from the other blob
    for c in r0["centroids"]:
        assert (np.abs(u - c).sum(1) == 0).any()
    assert abs(r0["centroids"][0] @ r0["centroids"][1]) < 0.5


def test_kmeans_centroids_in_skip_the_initialisation():
    z, mix, which, F, D = _two_blobs()
    cin = np.array([[0.0, 1.0], [1.0, 0.0]])          # the other order: labels follow the caller's centroids
    r = dpcl.kmeans(z, mix, F, D, 2, iterations=2, centroids_in=cin)
    np.testing.assert_array_equal(r["labels"], 1 - which)
    assert r["gap_init"] == np.inf
    r0 = dpcl.kmeans(z, mix, F, D, 2, iterations=0, centroids_in=cin)
    np.testing.assert_array_equal(r0["centroids"], cin)


def test_kmeans_empty_cluster_keeps_its_centroid():
    z, mix, which, F, D = _two_blobs()
    far = np.array([-1.0, -1.0]) / np.sqrt(2.0)       # nearer to no point than the other two
    cin = np.array([[0.99, 0.1], [0.1, 0.99], far])
    r = dpcl.kmeans(z, mix, F, D, 3, iterations=3, centroids_in=cin)
    np.testing.assert_array_equal(r["centroids"][2], far)
    assert not (r["labels"] == 2).any() and np.abs(r["centroids"][0] - cin[0]).max() > 1e-3


def test_kmeans_fewer_active_points_than_clusters():
    c = DC.few_active_case()
    ref, lens, offs = c["ref"], c["lens"], c["offs"]
    cen = ref["centroids"]
    # utterance 0: two active points -> centroids 0 and 1 are those points (the louder first), centroid 2 copies centroid 0
    # at the initialisation and, without an active member of its own, never moves; the exact tie goes to cluster 0
    np.testing.assert_array_equal(dpcl.kmeans_batch(c["z"], c["mix"], lens, offs, c["F"], c["D"], c["S"], 0)["centroids"][0][2],
                                  dpcl.kmeans_batch(c["z"], c["mix"], lens, offs, c["F"], c["D"], c["S"], 0)["centroids"][0][0])
    rows0 = dpcl.utterance_rows(lens, offs, 0)
    assert not (ref["labels"][rows0] == 2).any() and (ref["labels"][rows0] == 1).any()
    # utterance 1: one active point -> all three centroids are that point, every label is 0
    np.testing.assert_array_equal(cen[1][1], cen[1][0])
    np.testing.assert_array_equal(cen[1][2], cen[1][0])
    assert not ref["labels"][dpcl.utterance_rows(lens, offs, 1)].any()
    # no active point at all: zero centroids, label 0 everywhere
    r = dpcl.kmeans(c["z"][:2], np.zeros((2, c["F"]), np.float32), c["F"], c["D"], 2)
    assert not r["centroids"].any() and not r["labels"].any()


def test_kmeans_argument_errors():
    z, mix, _, F, D = _two_blobs()
    for bad in (dict(S=1), dict(S=5), dict(S=2, iterations=-1)):
        with pytest.raises(ValueError):
            dpcl.kmeans(z, mix, F, D, **bad)


# ------------------------------------------------------------------------------------------------ 4: conf keys
def test_conf_keys():
    import uPIT
    assert uPIT.parse_loss("dpcl") == "dpcl" and uPIT.parse_loss(" DPCL\n") == "dpcl" and uPIT.DPCL_LOSSES == ("dpcl",)
    for old in uPIT.LOSSES + uPIT.MIXIT_LOSSES:
        assert uPIT.parse_loss(old) == old
    with pytest.raises(ValueError) as e:
        uPIT.parse_loss("dc")
    assert "'mixit' / 'dpcl'" in str(e.value)
    assert "dpcl" not in uPIT.WAVE_LOSSES and "dpcl" not in uPIT.PSA_LOSSES           # it trains on what loss=mse trains on
    assert dpcl.parse_embed_dim("20") == 20 and dpcl.parse_embed_dim(40) == 40 and dpcl.parse_weight(" VAD") == "vad"
    for bad in ("0", "41", "-3", "x", None, "2.5"):
        with pytest.raises(ValueError):
            dpcl.parse_embed_dim(bad)
    with pytest.raises(ValueError):
        dpcl.parse_weight("irm")
    with pytest.raises(ValueError):
        dpcl.vad_ratio(-3.0)


class _Built(Exception):
    pass


def test_model_conf_sets_out_dim_and_refuses_bad_values(monkeypatch):
    """SepDNN.__init__ reads the conf keys before anything touches a GPU: out_dim = feat_dim * embed_dim for loss=dpcl, feat_dim *
    num_spk otherwise (the engine's _build is stood in for: this machine has no GPU to build on)."""
    import uPIT
    seen = {}

    def fake_build(self, gpuid, in_dim, out_dim, hidden_dim, num_layers, precision="fp32", sync_bn=False):
        seen.update(in_dim=in_dim, out_dim=out_dim, precision=precision)
        raise _Built()

    monkeypatch.setattr(uPIT.SepDNN, "_build", fake_build)
    with pytest.raises(_Built):
        uPIT.SepDNN(0, loss="dpcl", feat_dim="17", embed_dim="4", num_spk="3", dtype="bf16")
    assert seen == dict(in_dim=17, out_dim=68, precision="bf16")
    with pytest.raises(_Built):
        uPIT.SepDNN(0, loss="dpcl")
    assert seen["out_dim"] == 257 * 20
    with pytest.raises(_Built):
        uPIT.SepDNN(0, loss="mse", embed_dim="4", num_spk="3")
    assert seen["out_dim"] == 257 * 3
    for bad in (dict(embed_dim="41"), dict(embed_dim="0"), dict(dpcl_weight="irm"), dict(num_spk="5"), dict(num_spk="0"),
                dict(dpcl_kmeans_iters="-1"), dict(dpcl_vad_db="-1")):
        with pytest.raises(ValueError):
            uPIT.SepDNN(0, loss="dpcl", **bad)


# ------------------------------------------------------------------------------------------------ 5: the cases' decision gaps
@pytest.mark.parametrize("batch,F,S,D", DC.KMEANS_CASES)
def test_builder_cases_keep_the_decision_gaps_wide(batch, F, S, D):
    c = DC.kmeans_case(batch, F, S, D)
    ref = c["ref"]
    assert ref["gap_init"] >= DC.GAP_INIT and ref["gap_assign"] >= DC.GAP_ASSIGN, (ref["gap_init"], ref["gap_assign"], c["seed"])
    assert len(np.unique(ref["labels"])) == S                       # every cluster is populated
    # the utterances of a batch have different active sets and thresholds
    thr = [float(dpcl.threshold(c["mix"][dpcl.utterance_rows(c["lens"], c["offs"], j)], 40.0)) for j in range(len(c["lens"]))]
    assert len(set(thr)) == len(thr) and 0.05 < float((c["mix"] <= max(thr)).mean()) < 0.6
    # the float32 evaluation of the same algorithm takes the same decisions
    e32, r32 = DC.centroid_error_model(c)
    np.testing.assert_array_equal(r32["labels"], ref["labels"])
    assert e32 < 1e-5
    # iterations = 0 keeps the gaps too (the GPU test runs it on the first case)
    c0 = DC.kmeans_case(batch, F, S, D, iterations=0)
    assert c0["ref"]["gap_assign"] >= DC.GAP_ASSIGN


def test_overlapping_case_has_few_points_near_a_tie():
    c = DC.overlap_case()
    share = float((c["ref"]["point_gap"] < DC.GAP_POINT).mean())
    assert share <= DC.MAX_TIED_SHARE, share
    # it IS an overlapping case: the step moves labels across the boundary and some gaps are small
    assert float((c["ref"]["point_gap"] < 1e-2).mean()) > 0.005
    start = dpcl.kmeans_batch(c["z"], c["mix"], c["lens"], c["offs"], c["F"], c["D"], c["S"], 0, centroids_in=c["centroids_in"])
    assert (start["labels"] != c["ref"]["labels"]).any()


# ------------------------------------------------------------------------------------------------ 6: the cases catch defects
MARGIN = 10.0


# (the vad weights of the active points ARE equal: "unweighted" is a defect of the mr weights)
@pytest.mark.parametrize("defect,kind", [(d, k) for d in DC.DEFECTS for k in DC.WEIGHTS if (d, k) != ("unweighted", "vad")])
def test_gpu_cases_catch_the_defect(defect, kind):
    """A kernel with the defect returns the definition's value on the defective inputs: on the GPU test's cases that is at least
    10 x the gate away from the reference, in the loss or in the gradient, on every batch the defect can show on."""
    shown = 0
    for batch in DC.BATCHES:
        D, S = (20, 3)
        for F in (65, 257):
            c = DC.loss_case(batch, F, D, S)
            if not DC.defect_applies(c, defect):
                continue
            bad = DC.defective(c, defect)
            caught = False
            for j in range(len(c["lens"])):
                L, c2, g = DC.loss_ref(c, j, kind)[:3]
                Lb, _, gb = DC.loss_ref(bad, j, kind)[:3]
                L32, g32 = DC.loss_f32(c, j, kind)
                caught |= abs(Lb - L) / c2 >= MARGIN * DC.gate(abs(L32 - L) / c2)
                caught |= DC.rel_l2(gb, g) >= MARGIN * DC.gate(DC.rel_l2(g32, g))
            assert caught, "%s on %s F=%d leaves nothing the gates would see" % (defect, batch, F)
            shown += 1
    assert shown >= 4
