"""The pin suite of csrc/dpcl.hip on any machine: what tests/test_gpu_dpcl_cases.py runs on the device reaches what it claims.

1. The restated host code (tests/_dpcl_cases.py) is dpcl.hip's: the workspace layout against the library's two size queries
   (where the library loads) and against the documented formula, tiles_of and the DB choice against the switch tables of the source.
2. Every case's predicates hold; the table reaches all 17 instantiations, every listed NT, DB, seam and wave-trip edge, a
   multi-chunk ragged batch with nchmax > nch_j; the per-chunk Gram reference sums to the definition.
3. Every defect model moves a checked quantity (loss, dz, ab; centroids and labels for the pick tie) by at least 10 x its gate on
   every case that names it, and every defect is named by at least one case.
4. The new k-means cases keep the builder's decision gaps; the tie case's conditions hold.
"""
import os
import re

import numpy as np
import pytest

import _dpcl_cases as DC
from conftest import PKG
from sepkern import dpcl

MARGIN = 10.0


# ------------------------------------------------------------------------------------------------ 1: the restatement
def _documented_total(T, B, D, S, km):
    """The workspace as the comment on dpcl.hip's Layout states it -- [chunk maxima | thresholds | pick values, indices, counts
    | centroids | Gram partials] -- written out once more: every block rounded up to 256 bytes, 256 bytes of slack at the end."""
    up = lambda n: (n + 255) // 256 * 256
    nc = B * ((T + 7) // 8)
    NT = (D + S + 15) // 16
    pairs = NT if km else NT * (NT + 1) // 2
    pick = 3 * up(4 * nc) + up(4 * B * 4 * 40) if km else 0
    return up(4 * nc) + up(4 * B) + pick + up(8 * 256 * pairs * nc) + 256


SHAPES = [(T, B, D, S) for T in (1, 8, 9, 19, 400) for B in (1, 5, 64, 65) for (D, S) in ((1, 1), (12, 4), (13, 4), (16, 2), (29, 4), (40, 4))]


def test_the_restated_workspace_is_the_librarys():
    from sepkern import _lib
    try:
        lib = _lib.load()
    except _lib.SepkernError:
        lib = None
    for T, B, D, S in SHAPES:
        for km in (False, True):
            lay = DC.layout_of(T, B, D, S, km)
            names = ("cmax", "thr", "pval", "pidx", "pcnt", "cent", "partial", "total")
            assert all(lay[k] % 256 == 0 for k in names) and [lay[k] for k in names] == sorted(lay[k] for k in names)
            assert lay["total"] == _documented_total(T, B, D, S, km), (T, B, D, S, km)
            if not km:
                assert lay["pval"] == lay["pidx"] == lay["pcnt"] == lay["cent"] == lay["partial"]
            if lib is not None and (S >= 2 or not km):
                fn = lib.sk_dpcl_kmeans_workspace_bytes if km else lib.sk_dpcl_workspace_bytes
                assert fn(T, B, 65, D, S) == lay["total"], (T, B, D, S, km)
    assert DC.AB == 1760 and DC.DMAX == dpcl.MAX_D and DC.MAXS == dpcl.MAX_S


def test_the_restated_constants_and_switch_tables_are_the_sources():
    src = open(os.path.join(PKG, "csrc", "dpcl.hip")).read()
    const = dict(re.findall(r"constexpr int (\w+) = (\d+);", src))
    assert (int(const["DMAX"]), int(const["CH"]), int(const["TP"])) == (DC.DMAX, DC.CH, DC.TP)
    assert "inline int tiles_of(int D, int S) { return (D + S + 15) / 16; }" in src
    assert "constexpr int npairs(int NT, bool KM) { return KM ? NT : NT * (NT + 1) / 2; }" in src
    # dpcl_bwd_kernel: switch ((D + 7) / 8) { case n: DB ... default: 40 }
    assert "switch ((D + 7) / 8)" in src
    table = {int(n): int(db) for n, db in re.findall(r"case (\d+): SK_DPCL_BWD\((\d+)\)", src)}
    default = int(re.search(r"default: SK_DPCL_BWD\((\d+)\)", src).group(1))
    for D in range(1, DC.DMAX + 1):
        assert DC.db_of(D) == table.get((D + 7) // 8, default) == 8 * ((D + 7) // 8), D
    # gram / loss / cent: switch on tiles_of with NT = 1, 2 and 3 as the default, in both entry points
    for km, second in (("false", "dpcl_loss_kernel"), ("true", "dpcl_cent_kernel")):
        cases = re.findall(r"(case (\d)|default):\s*hipLaunchKernelGGL\(\(dpcl_gram_kernel<(\d), %s>\).*?\n\s*hipLaunchKernelGGL\(%s<(\d)>" % (km, second), src)
        assert [(c[1], c[2], c[3]) for c in cases] == [("1", "1", "1"), ("2", "2", "2"), ("", "3", "3")], cases
    for D in range(1, DC.DMAX + 1):
        for S in range(1, DC.MAXS + 1):
            assert 1 <= DC.tiles_of(D, S) <= 3 and 16 * (DC.tiles_of(D, S) - 1) < D + S <= 16 * DC.tiles_of(D, S)


def test_chunk_table_is_the_kernels_partition():
    assert [(c["nfr"], c["npts"], c["ntiles"], c["niter"]) for c in DC.chunk_table(19, 33)] == [(8, 264, 5, 2), (8, 264, 5, 2), (3, 99, 2, 1)]
    assert [(c["npts"], c["ntiles"], c["niter"]) for c in DC.chunk_table(17, 8)] == [(64, 1, 1), (64, 1, 1), (8, 1, 1)]
    assert [(c["npts"], c["ntiles"], c["niter"]) for c in DC.chunk_table(16, 32)] == [(256, 4, 1), (256, 4, 1)]
    assert [(c["t0"], c["ntiles"], c["niter"]) for c in DC.chunk_table(8, 65)] == [(0, 9, 3)]


# ------------------------------------------------------------------------------------------------ 2: the cases' claims
def test_every_claim_holds_and_every_listed_edge_is_reached():
    DC.check_claims()
    pairs = set((D, S) for (_, _, D, S) in DC.LOSS_CASES)
    assert pairs == set(DC.LOSS_PAIRS) and set(DC.NT_EDGES) | set(DC.DB_EDGES) <= pairs
    claimed = lambda name: {p for p, cl in DC.LOSS_PAIRS.items() if name in cl}
    # all five dpcl_bwd_kernel instantiations with D = DB and D = DB - 7
    for db in (8, 16, 24, 32, 40):
        here = {p for p in pairs if DC.db_of(p[0]) == db}
        assert here & claimed("db_full") and here & claimed("db_low"), db
        assert {D for D, _ in here} >= {db, db - 7}
    for lo, hi in ((8, 9), (16, 17), (24, 25), (32, 33)):              # both sides of every DB edge
        assert {lo, hi} <= {D for D, _ in pairs}
    # all three NT at D + S = 16 NT; NT = 2, 3 at 16 (NT - 1) + 1; D = 16 and 32
    # (NT = 3 cannot be filled: test_nt3_has_no_pair_with_d_plus_s_48)
    assert {DC.tiles_of(*p) for p in claimed("abuts")} == {1, 2} and {DC.tiles_of(*p) for p in claimed("lone_block")} == {2, 3}
    assert len(claimed("nt1") & claimed("abuts")) >= 2 and len(claimed("nt2") & claimed("abuts")) >= 2
    assert {D for D, _ in claimed("d_on_tile")} == {16, 32}
    assert claimed("a_one_trip") and claimed("a_two_trips") and claimed("seam16") and claimed("seam32")
    # the wave-trip geometries and the multi-chunk ragged batch, each with a loss case on it
    geo = set((b, F) for (b, F, _, _) in DC.LOSS_CASES)
    for name in DC.GEOMETRY_CLAIMS:
        assert any(name in cl for g, cl in DC.GEOMETRIES.items() if g in geo), name
    assert {F for _, F in geo} == set(DC.EDGE_BINS)
    lens = DC.EDGE_BATCHES["chunks_ragged"]
    assert [DC.chunks_of(n) for n in lens] == [3, 3, 2, 1, 1] and sorted(lens, reverse=True) == lens


def test_nt3_has_no_pair_with_d_plus_s_48():
    """D <= 40 and S <= 4 leave D + S <= 44: dpcl_gram_kernel<3, *> cannot be filled to its last column.  (40, 4) is the
    largest: four zero columns between the embedding and the block."""
    assert DC.DMAX + DC.MAXS == 44 and DC.tiles_of(40, 4) == 3 and (40, 4) in DC.LOSS_PAIRS
    assert not any(DC.PAIR_CLAIMS["nt3"](D, S) and DC.PAIR_CLAIMS["abuts"](D, S) for D in range(1, 41) for S in range(1, 5))


def test_the_table_reaches_every_instantiation():
    seen = set()
    for (_, _, D, S) in DC.LOSS_CASES:
        seen |= DC.instantiations(D, S, False)
    for (_, _, S, D) in DC.KMEANS_EDGE_CASES:
        seen |= DC.instantiations(D, S, True)
    assert seen == DC.ALL_INSTANTIATIONS and len(seen) == 17
    # the k-means pairs: both sides of the NT edges, planes 15|16 and 31|32 of dpcl_cent_kernel's tile index in one case
    assert {DC.tiles_of(D, S) for D, S in DC.KMEANS_PAIRS} == {1, 2, 3}
    assert any(D >= 17 for D, _ in DC.KMEANS_PAIRS) and any(D >= 33 for D, _ in DC.KMEANS_PAIRS)
    assert set(DC.KMEANS_ITERATION_CASES) <= set(DC.KMEANS_EDGE_CASES)


@pytest.mark.parametrize("kind", DC.WEIGHTS)
@pytest.mark.parametrize("key", [("chunks_ragged", 65, 13, 4), ("chunks_ragged", 5, 16, 2), ("two_chunks+1", 33, 17, 3),
                                 ("chunks_ragged", 8, 40, 4), ("chunks_ragged", 65, 1, 1)])
def test_chunk_grams_sum_to_the_definition(key, kind):
    c = DC.edge_case(*key)
    F, D, S = c["F"], c["D"], c["S"]
    P = 16 * DC.tiles_of(D, S)
    for j, n in enumerate(c["lens"]):
        grams = DC.chunk_grams(c, j, kind)
        assert len(grams) == DC.chunks_of(n) and all(G.shape == (P, P) for G in grams)
        # the float32 model of a partial is close, and another chunk's partial in its place is far outside the gate
        e32 = [DC.gram_error(G32, G) for G32, G in zip(DC.chunk_grams_f32(c, j, kind), grams)]
        assert all(e < 1e-5 for e in e32) and (D == 1 or all(e > 0 for e in e32))
        if len(grams) > 1:
            assert DC.gram_error(grams[1], grams[0]) >= MARGIN * DC.gate(e32[0])
        G = sum(grams)
        assert not G[D:P - S].any() and not G[:, D:P - S].any()                      # the columns in between are zero
        A, Bm, C, sc = DC.moments_of(G, D, S)
        rows = dpcl.utterance_rows(c["lens"], c["offs"], j)
        args = (c["z"][rows], c["mix"][rows], [s[rows] for s in c["srcs"]], F, D, kind)
        A0, B0, C0 = dpcl.moments(*args)[:3]
        assert np.abs(A - A0).max() <= 1e-12 and np.abs(Bm - B0).max() <= 1e-12 and np.abs(C - C0).max() <= 1e-12
        assert abs(DC.loss_of(A, Bm, C) - dpcl.loss_utt(*args)) <= 1e-12
        r = DC.reference(key, j, kind)
        assert DC.rel_l2(DC.grad_of(c, j, kind, A, Bm, sc), r["dz"], r["scale"]) <= 1e-12
        assert np.abs(DC.ab_of(A, Bm) - r["ab"]).max() <= 1e-12 and abs(sc - r["sc"]) <= 1e-12 * r["sc"]
        assert not r["ab"][DC.ab_padding(D, S)].any() and r["ab"][~DC.ab_padding(D, S)].all()


# ------------------------------------------------------------------------------------------------ 3: the defects
def test_every_defect_is_named_by_a_case_the_gpu_test_runs():
    assert set(DC.DEFECT_CASES) == set(DC.EDGE_DEFECTS)
    for defect, keys in DC.DEFECT_CASES.items():
        assert keys and all(k in DC.LOSS_CASES for k in keys), defect
        assert all(DC.defect_variants(k, defect) for k in keys), defect
    # what each defect needs of its cases
    need = {"chunk_pitch": "nchmax_gt_nch", "stale_chunk": "nchmax_gt_nch", "last_tile": "partial_tile"}
    for defect, claim in need.items():
        assert all(claim in DC.GEOMETRIES[k[:2]] for k in DC.DEFECT_CASES[defect])
    assert all(max(ch["ntiles"] for n in DC.ALL_BATCHES[k[0]] for ch in DC.chunk_table(n, k[1])) >= 4 for k in DC.DEFECT_CASES["fourth_wave"])
    assert all("crosses" in DC.LOSS_PAIRS[k[2:]] for k in DC.DEFECT_CASES["onehot_overlap"])
    assert all(k[2] * k[2] > 256 for k in DC.DEFECT_CASES["a_second_trip"])
    assert all("db_full" in DC.LOSS_PAIRS[k[2:]] for k in DC.DEFECT_CASES["bwd_odd_row"])
    assert all(DC.db_of(k[2]) > k[2] for k in DC.DEFECT_CASES["ab_padding"])
    assert {DC.db_of(k[2]) for k in DC.DEFECT_CASES["bwd_block_tail"]} == {8, 16, 24, 32, 40}


@pytest.mark.parametrize("defect", DC.EDGE_DEFECTS)
def test_edge_cases_catch_the_defect(defect):
    """What a kernel with the defect returns is at least 10 x the gate away from the reference, in the loss, the gradient or ab,
    on EVERY case that names the defect, under both weightings and for every variant."""
    least = np.inf
    for key in DC.DEFECT_CASES[defect]:
        for kind in DC.WEIGHTS:
            for variant in DC.defect_variants(key, defect):
                shown = DC.defect_shows(key, kind, defect, variant, MARGIN)
                least = min(least, shown)
                assert shown >= 1.0, "%s (%r) on %r %s moves %.3g of 10 x the gate" % (defect, variant, key, kind, shown)
    print("dpcl defect %-15s: at least %.3g x (10 x the gate) over %d cases" % (defect, least, len(DC.DEFECT_CASES[defect])))


def test_onehot_overlap_is_wrong_exactly_where_the_block_crosses_a_tile_edge():
    for (D, S), claims in DC.LOSS_PAIRS.items():
        if D == 1:
            continue
        key = ("chunks_ragged", 5, D, S)
        bad, ref = DC.defect_outputs(key, 0, "mr", "onehot_overlap"), DC.reference(key, 0, "mr")
        moved = abs(bad["L"] - ref["L"]) / ref["c2"]
        assert (moved > 1e-3) == ("crosses" in claims) and (moved < 1e-12 or "crosses" in claims), (D, S, moved)


def test_finite_stale_padding_of_ab_does_not_reach_the_gradient():
    """What the restated backward says of ab's padding: rows b >= D meet u_b = 0 and g_a for a >= D is never stored, so only a
    non-finite stale value (0 * NaN) changes dz.  The exact-zero check on ab is therefore the only guard against a finite one."""
    key = ("chunks_ragged", 65, 9, 2)
    c, r = DC.edge_case(*key), DC.reference(key, 1, "mr")
    G = sum(DC.chunk_grams(c, 1, "mr"))
    A, Bm, _, sc = DC.moments_of(G, 9, 2)
    assert DC.rel_l2(DC.grad_of(c, 1, "mr", A, Bm, sc), r["dz"]) <= 1e-12
    assert np.isnan(DC.defect_outputs(key, 1, "mr", "ab_padding")["dz"]).all()


# ------------------------------------------------------------------------------------------------ 4: the k-means cases
@pytest.mark.parametrize("batch,F,S,D", DC.KMEANS_EDGE_CASES)
def test_new_builder_cases_keep_the_decision_gaps_wide(batch, F, S, D):
    """The assertions of test_dpcl.py's test_builder_cases_keep_the_decision_gaps_wide on the pin suite's cases."""
    c = DC.kmeans_case(batch, F, S, D)
    ref = c["ref"]
    assert ref["gap_init"] >= DC.GAP_INIT and ref["gap_assign"] >= DC.GAP_ASSIGN, (ref["gap_init"], ref["gap_assign"], c["seed"])
    assert len(np.unique(ref["labels"])) == S
    for j in range(len(c["lens"])):                                  # every utterance populates every cluster
        assert len(np.unique(ref["labels"][dpcl.utterance_rows(c["lens"], c["offs"], j)])) == S
    thr = [float(dpcl.threshold(c["mix"][dpcl.utterance_rows(c["lens"], c["offs"], j)], 40.0)) for j in range(len(c["lens"]))]
    assert len(set(thr)) == len(thr) and 0.05 < float((c["mix"] <= max(thr)).mean()) < 0.6
    e32, r32 = DC.centroid_error_model(c)
    np.testing.assert_array_equal(r32["labels"], ref["labels"])
    assert e32 < 1e-5
    print("dpcl kmeans edge %s F=%d S=%d D=%d: seed %d, gap_init %.3g, gap_assign %.3g, float32 centroid error %.3g"
          % (batch, F, S, D, c["seed"], ref["gap_init"], ref["gap_assign"], e32))
    c0 = DC.kmeans_case(batch, F, S, D, iterations=0)
    assert c0["ref"]["gap_assign"] >= DC.GAP_ASSIGN
    if (batch, F, S, D) in DC.KMEANS_ITERATION_CASES:
        c1 = DC.kmeans_case(batch, F, S, D, iterations=1)
        assert c1["ref"]["gap_assign"] >= DC.GAP_ASSIGN and c1["ref"]["gap_init"] >= DC.GAP_INIT
        np.testing.assert_array_equal(DC.centroid_error_model(c1)[1]["labels"], c1["ref"]["labels"])
        np.testing.assert_array_equal(DC.centroid_error_model(c0)[1]["labels"], c0["ref"]["labels"])


@pytest.mark.parametrize("F", (5, 65))
def test_kmeans_edge_cases_catch_a_defective_centroid_update(F):
    """The update restated from the chunks' sums is the reference's; with a wrong chunk pitch, a stale chunk or an unread seam
    plane the centroids move by at least 10 x their gate on every case that can show it."""
    shown = {d: 0 for d in DC.KMEANS_DEFECTS}
    for (batch, _, S, D) in [k for k in DC.KMEANS_EDGE_CASES if k[1] == F]:
        c = DC.kmeans_case(batch, F, S, D)
        ref = c["ref"]["centroids"]
        assert np.abs(DC.kmeans_update(c) - ref).max() <= 1e-12
        tol = MARGIN * DC.gate(DC.centroid_error_model(c)[0])
        for defect in ("chunk_pitch", "stale_chunk"):
            bad = DC.kmeans_update(c, defect)
            assert np.abs(bad[:2] - ref[:2]).max() <= 1e-12                                  # nch_j = nchmax: nothing to get wrong
            assert all(np.abs(bad[j] - ref[j]).max() >= tol for j in (2, 3, 4)), (defect, S, D)
            shown[defect] += 1
        for plane in [p for p in DC.SEAM_PLANES if p < D]:
            assert np.abs(DC.kmeans_update(c, "tile_seam", plane) - ref)[:, :, plane].min() >= tol, (plane, S, D)
            shown["tile_seam"] += 1
    assert all(n >= 4 for n in shown.values()), shown


def test_the_tie_case_is_a_tie_and_nothing_else_is_close():
    c = DC.tie_case()
    F, ref = c["F"], c["ref"]
    assert ref["gap_init"] == 0.0 and c["later_gap"] >= DC.GAP_INIT and ref["gap_assign"] >= DC.GAP_ASSIGN
    where = []
    for j in range(len(c["lens"])):
        rows = dpcl.utterance_rows(c["lens"], c["offs"], j)
        m = c["mix"][rows].reshape(-1)
        lo, hi = DC.TIE_POINTS[j]
        assert lo < hi and m[lo] == m[hi] == m.max() and (m == m.max()).sum() == 2          # the same float32, the only two
        ulo, uhi = DC.tie_unit_vectors(c, j)
        np.testing.assert_array_equal(ref["centroids"][j][0], ulo)                       # the reference takes the lower index
        assert np.abs(ulo - uhi).max() >= 1e-2
        npts = DC.CH * F
        where.append(tuple((q // npts, (q % npts) % 256 // 64, (q % npts) % 64) for q in (lo, hi)))   # (chunk, wave, lane)
    (a0, b0), (a1, b1), (a2, b2) = where
    assert a0[:2] == b0[:2] and a0[2] > b0[2]        # one chunk, one wave, the lower index at the higher lane
    assert a1[0] == b1[0] and a1[1] > b1[1]          # one chunk, the lower index in the higher wave
    assert a2[0] < b2[0]                             # two chunks
    # the float32 evaluation takes the same decisions; a kernel that gives the tie away is far outside the centroids' gate
    e32, r32 = DC.centroid_error_model(c)
    np.testing.assert_array_equal(r32["labels"], ref["labels"])
    bad = DC.pick_first_lane(c)
    for j in range(len(c["lens"])):
        assert np.abs(bad["centroids"][j][0] - ref["centroids"][j][0]).max() >= MARGIN * DC.gate(e32)
        np.testing.assert_array_equal(bad["centroids"][j][0], DC.tie_unit_vectors(c, j)[1])
    assert (bad["labels"] != ref["labels"]).any()
