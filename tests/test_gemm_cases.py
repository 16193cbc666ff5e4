"""The GEMM case table (tests/_gemm_cases.py) can tell a wrong kernel from a right one -- shown on any machine.

Every case's claims hold over the restatement of gemm.hip's host code and loop bounds; every defect model changes at least one
checked element (sentinels included) of every case that names it, sigmoid cases by at least 10 x the gate; every case is the
witness of a defect or of a chooser threshold; the restated chooser reproduces the kernel ids recorded on the MI355X in
tests/test_gpu_gemm_choice.py.
"""
import numpy as np
import pytest

import _gemm_cases as G
import test_gpu_gemm_choice as GC


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.name)
def test_claims_hold(case):
    assert G.claims_hold(case) == []
    assert case.defects or any(cl[0] == "thr" for cl in case.claims), "a case must be the witness of a defect or a threshold"
    assert set(case.defects) <= set(G.DEFECTS)
    g = G.geometry(case)
    if not g["persistent"]:      # the tile-order map visits every tile exactly once
        seen = [G.tile_of_block(b, g["tilesM"], g["tilesN"], g["group"]) for b in range(g["tiles"])]
        assert sorted(seen) == [(r, c) for r in range(g["tilesM"]) for c in range(g["tilesN"])]


def test_table_covers_the_boundaries_it_promises():
    by_kid = {}
    for c in G.CASES:
        by_kid.setdefault(c.kid, []).append(c)
    assert set(by_kid) == set(G.KERNELS)
    for kid, ks in G.KERNELS.items():
        if ks["persistent"]:
            continue
        steps = {G._steps(G.geometry(c)) for c in by_kid[kid] if c.K % ks["bk"] == 0 and c.splitk == 1}
        assert {1, 2, 3, ks["ring"] + 1} <= steps, (ks["name"], steps)
        claimed = {cl for c in by_kid[kid] for cl in c.claims}
        assert {("tiles_mod8", 1), ("tiles_mod8", 7), ("tilesM", 1), ("tilesM", 2)} <= claimed, ks["name"]
        if ks.get("any_k"):
            assert {("K", w) for w in ("1", "BK-1", "BK", "BK+1", "2BK-1", "2BK+1")} <= claimed, ks["name"]
    for name in G.THRESHOLDS:
        sides = {cl[2] for c in G.CASES for cl in c.claims if cl[:2] == ("thr", name)}
        assert sides == {True, False}, name
    # ... and every threshold case is DECISIVE: with that one condition of the restated chooser forced to its other side (all
    # else as the case has it) another kernel takes the launch -- a chooser that dropped the condition could not pass both sides
    for c in G.CASES:
        for cl in c.claims:
            if cl[0] == "thr":
                other = G.geometry(c, False, G.P_MI355X, (cl[1], not cl[2]))["kid"]
                assert other != c.kid, (c.name, cl, "the kernel does not depend on this threshold here")
    for K, s in ((1792, 5), (1536, 8)):
        assert {c.kid for c in G.CASES if (c.K, c.splitk) == (K, s) and c.kind == "exact"} == {G.K_SPLIT, G.K_PL3}
    for K in (752, 768, 784, 1520, 1536):
        got = {(c.kid, c.form) for c in G.CASES if c.K == K and c.splitk == 1 and c.family == "sign"}
        assert {(G.K_PLANES, f) for f in ((0, 0), (0, 1), (1, 0))} <= got and {G.K_SPLIT, G.K_PL3} <= {k for k, _ in got}, K


def test_every_kernel_walks_an_uneven_tile_list_and_a_ragged_last_group():
    """The tile-order map is one function for all kernels, the persistent ones included: per kernel id the table holds a case
    whose XCD runs are of two lengths (nt > 8, nt % 8 != 0) and one whose last group of tile rows is smaller than the others
    and more than one tile column wide."""
    for kid, ks in G.KERNELS.items():
        geoms = [G.geometry(c) for c in G.CASES if c.kid == kid]
        assert any(G.xcd_remainder(g) for g in geoms), ks["name"]
        assert any(G.ragged_group(g) for g in geoms), ks["name"]
    for kid in (G.K_STREAMK, G.K_BF2_STREAMK):      # ... and a cut behind at least one whole round of tiles
        assert any(G.geometry(c)["cut"][1] >= 1 for c in G.CASES if c.kid == kid), G.KERNELS[kid]["name"]


def test_every_defect_model_is_named_by_a_case():
    for defect in G.DEFECTS:
        assert any(defect in c.defects for c in G.CASES), defect


@pytest.mark.parametrize("family", G.FAMILIES)
def test_every_defect_model_changes_a_checked_element(family):
    """Every case, the large ones included, witnesses every defect it names (embed cases: the model is shown on integer
    operands of the case's shape)."""
    for c in (c for c in G.CASES if c.family == family and c.defects):
        ops = G.int_operands(c)
        ref = G.reference(c, ops)
        atol = 10 * G.SIGMOID_ATOL if c.kind == "sigmoid" else 0.0
        for defect in c.defects:
            assert int(G.differs(ref, G.reference(c, ops, defect), atol).sum()) > 0, (c.name, defect)


def test_reference_is_the_plain_product():
    c = next(c for c in G.CASES if c.name.startswith("f32_v1_NT_130x131x100"))
    ia, ib, ibias, ic0 = G.int_operands(c)
    ref = G.reference(c)
    want = (np.einsum("zmk,zkn->zmn", ia.astype(np.int64), ib.astype(np.int64)) + ibias.astype(np.int64)[:, None, :]
            + ic0.astype(np.int64)) / 32.0
    assert np.array_equal(ref[:, :c.M, :c.N], want)
    assert np.isnan(ref[:, c.M:]).all() and np.isnan(ref[:, :, c.N:]).all()


def _f32_geom(shape, form, launch):
    M, N, K, pad = shape
    tA, tB = form
    splitk, batch, streamk_ws = launch
    lda, ldb = (M if tA else K) + pad, (K if tB else N)
    sA, sB = (K if tA else M) * lda, (N if tB else K) * ldb
    return G.vec_ok(0, lda, sA), G.vec_ok(0, ldb, sB), splitk > 1 or streamk_ws


def test_restated_chooser_reproduces_the_recorded_ids():
    got = {}
    for name, shape in GC.F32_SHAPES.items():
        M, N, K, _ = shape
        got[name] = {}
        for v in GC.F32_VARIANTS:
            groups = []
            for form in GC.FORMS:
                ids = ""
                for launch in GC.LAUNCHES:
                    vecA, vecB, ws = _f32_geom(shape, form, launch)
                    splitk, kchunk = G.slice_k(K, launch[0], 16)
                    ids += "%x" % G.choose_kernel(M, N, K, splitk, kchunk, vecA, vecB, False, v, form[0], form[1], launch[1], ws)[0]
                groups.append(ids)
            got[name][v] = " ".join(groups)
    assert got == GC.F32_EXPECTED
    for case, want in GC.BF16MM_EXPECTED.items():
        M, N, K, splitk, batch, streamk_ws = case
        s, _ = G.slice_k(K, splitk, 64)
        assert "%x" % G.choose_bf16_mm(M, N, K, s, batch, splitk > 1 or streamk_ws)[0] == want[0] and len(set(want)) == 1
    assert set("".join(GC.BF16_EXPECTED.values()).replace(" ", "")) == {"%x" % G.K_BF16}
    assert set(GC.PL3_EXPECTED.values()) == {"%x" % G.K_PL3}


def test_restated_older_shapes_are_those_of_test_gpu_kernels():
    """_gemm_cases.OLDER_SHAPES (behind the 'first run of ... at' report) is a copy of parametrize lists: it must not drift."""
    import test_gpu_kernels as TK
    for name, shapes in G.OLDER_SHAPES.items():
        marks = [m for m in getattr(TK, name).pytestmark if m.name == "parametrize" and m.args[0] == G.OLDER_SHAPE_ARGS[name]]
        assert len(marks) == 1, name
        assert [tuple(x) for x in marks[0].args[1]] == shapes, name
    gemm_tests = {n for n in dir(TK) if n.startswith("test_gemm") and any(
        m.name == "parametrize" and m.args[0].startswith("M,N,K") for m in getattr(getattr(TK, n), "pytestmark", []))}
    assert gemm_tests == set(G.OLDER_SHAPES), gemm_tests ^ set(G.OLDER_SHAPES)


def test_every_kernel_family_reaches_boundaries_the_older_tests_do_not():
    """first_time_claims() restates the GEMM shapes of tests/test_gpu_kernels.py; per kernel the table must add something."""
    first = G.first_time_claims()
    for kid, ks in G.KERNELS.items():
        new = {cl for c in G.CASES if c.kid == kid for cl in first[c.name]}
        assert new, ks["name"]
