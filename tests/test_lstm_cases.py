"""The recurrence case table (tests/_lstm_cases.py) can tell a wrong kernel from a right one -- shown on any machine.

The restated host code reproduces every launch recorded on the MI355X in tests/test_gpu_lstm_choice.py; decode_block is a
bijection for every plan of the table; the table reaches all 24 forward and 17 backward instantiations and, per KS x precision,
the boundaries listed in test_table_covers_the_boundaries_it_promises; every claim holds; every defect model moves a checked
output of every case that names it by at least 10 x that case's gate; the fp64 reference is oracle.upit.blstm_padded.
"""
import numpy as np
import pytest
import torch

import _lstm_cases as L
import test_gpu_lstm_choice as LC


def _mode_word(case):
    """test_gpu_lstm_choice.mode_word without the package (the same fields from the restated constants)."""
    d, H, B, kind, gmin, flavour, packed, exclusive, d0 = case
    m = kind | (gmin << L.GMIN_SHIFT) | (1 << L.MAP_SHIFT) | (L.POLL1 if d == "fwd" else 0)
    m |= L.SPLIT3 if "s3" in flavour else 0
    m |= L.TAGGED if "tagged" in flavour else 0
    m |= L.XL8 if "xl8" in flavour else 0
    m |= L.BF16 if "bf16" in flavour else 0
    m |= L.BWD_EXCLUSIVE if exclusive or flavour == "bit17" else 0
    if flavour == "kind3":
        m = (m & ~0xff) | 3
    if flavour == "gmin9":
        m |= 9 << L.GMIN_SHIFT
    return m


def test_restatement_reproduces_every_recorded_launch():
    assert set(LC.EXPECTED) == set(LC.CASES)
    got = {c: L.predict(c[0], LC.T, c[2], c[1], _mode_word(c), c[6], c[8]) for c in LC.CASES}
    wrong = {c: (got[c], e) for c, e in LC.EXPECTED.items() if got[c] != e}
    assert not wrong, wrong
    assert sum(e == -1 for e in LC.EXPECTED.values()) == 7


def test_mode_word_is_the_packages():
    for c in LC.CASES:
        assert _mode_word(c) == LC.mode_word(c), c


def test_spot_checks_of_the_plan():
    f = lambda B, H, kind=0: L.predict("fwd", 3, B, H, kind, False)
    assert f(33, 1024)[7:] == (256, 2) and f(100, 1024)[8] == 4
    assert f(272, 1024) == (3, 1, 64, 0, 0, 0, 0, 2176, 1) and f(272, 1024, 1) == -1
    assert f(769, 8) == (3, 1, 20, 0, 0, 0, 0, 1960, 1) and f(768, 8)[7:] == (240, 8)
    assert L.bwd_cfg(64, False)["cnt"] == [4] * 8 and L.bwd_cfg(38, False)["cnt"] == [3, 3, 3, 3, 3, 3, 1, 0]
    assert L.bwd_cfg(40, True)["cnt"] == [3, 3, 3, 1] and L.bwd_cfg(56, True)["cnt"] == [4, 4, 4, 2]


def test_decode_block_is_a_bijection():
    plans = {(c.plan(d, k)["KS"], c.plan(d, k)["nby"]) for c in L.CASES for d in ("fwd", "bwd") for _, k in c.runs() if not c.plan(d, k)["xl8"]}
    plans |= {(ks, nby) for ks in (20, 38, 40, 56, 64) for nby in range(1, 9) if ks * nby * 2 <= L.CUS}
    for NUG, nby in sorted(plans):
        for map_ in range(4):
            seen = sorted(L.decode_block(i, NUG, nby, map_) for i in range(NUG * nby * 2))
            assert seen == sorted((u, by, d) for u in range(NUG) for by in range(nby) for d in range(2)), (NUG, nby, map_)


@pytest.mark.parametrize("case", L.CASES, ids=lambda c: c.name)
def test_claims_hold(case):
    assert L.claims_hold(case) == []
    assert case.claims and case.defects and set(case.defects) <= set(L.DEFECTS)
    assert list(case.lens) == sorted(case.lens, reverse=True) and case.lens[0] == case.T and case.lens[-1] >= 1 and case.T <= 4
    for lay, kind in case.runs():
        for d in ("fwd", "bwd") if case.backward else ("fwd",):
            assert L.predict(d, case.T, case.B, case.H, case.mode(d, kind), lay == "packed") != -1


def _classes():
    """(precision, KS) -> the cases that run it."""
    out = {}
    for c in L.CASES:
        out.setdefault(("bf16" if c.bf else c.flavour if c.flavour == "s3" and "s3_family" in c.claims else "f32", c.plan()["KS"]), []).append(c)
    return out


def test_table_covers_the_boundaries_it_promises():
    """Every instantiation runs in at least one value case.  Per KS x precision (fp32, bf16, split3): HP exactly full, the lowest
    H of the class, H = 4 mod 8 and H = 4 mod 16, G in {1, 2, 8}, G > NBG, both launch kinds and both layouts; where the class has
    a backward, GM in {1, 8}."""
    reached = set()
    for c in L.CASES:
        for lay, kind in c.runs():
            for d in ("fwd", "bwd") if c.backward else ("fwd",):
                reached.add(L.instantiation(d, L.predict(d, c.T, c.B, c.H, c.mode(d, kind), lay == "packed")))
    assert L.ALL_INSTANTIATIONS - reached == set() and reached <= L.ALL_INSTANTIATIONS
    classes = _classes()
    assert set(classes) == {(p, ks) for p in ("f32", "bf16", "s3") for ks in (20, 40 if p != "f32" else 38, 56, 64) if (p, ks) != ("s3", 64)}
    missing = []
    for (prec, ks), cs in sorted(classes.items()):
        claimed = {n for c in cs for n in c.claims}
        want = {"hp_full", "lowest_h", "h4mod8", "h4mod16", "g1", "g2", "g8", "g_gt_nbg"} | ({"gm1", "gm8"} if prec != "s3" else set())
        have = claimed | {"g%d" % c.plan()["G"] for c in cs} | {"gm%d" % c.plan("bwd")["gm"] for c in cs if c.backward}
        missing += [(prec, ks, n) for n in sorted(want - have)]
        persistent = {c.plan("fwd", k)["persistent"] for c in cs for _, k in c.runs()}
        layouts = {lay for c in cs for lay, _ in c.runs()}
        missing += [(prec, ks, "launch kinds")] if persistent != {True, False} else []
        missing += [(prec, ks, "layouts")] if layouts != {"padded", "packed"} else []
    assert not missing, missing
    # the XCD-local form: both layouts, a group of one row, a single group, a full grid of eight streams
    xl = [c for c in L.CASES if c.flavour == "xl8"]
    assert {(c.B, c.H) for c in xl} == {(9, 644), (25, 644), (1, 896), (32, 892)} and all(c.layouts == ("padded", "packed") for c in xl)
    # the minimal shapes run forward AND backward
    assert all(c.backward for c in L.CASES if {"t1", "t2", "second_stream_one_step"} & set(c.claims))


def test_every_defect_model_is_named_by_a_case():
    for defect in L.DEFECTS:
        assert any(defect in c.defects for c in L.CASES), defect
    # the short sub-blocks the ring can have: fp32 KS 38 (cnt 1), bf16 KS 40 (1), bf16 KS 56 (2)
    short = {(c.bf, c.plan("bwd")["KS"]) for c in L.CASES if "short_subblock" in c.defects}
    assert short == {(False, 38), (True, 40), (True, 56)}


@pytest.mark.parametrize("case", L.CASES, ids=lambda c: c.name)
def test_every_defect_model_moves_a_checked_output(case):
    """... by at least 10 x the case's gate (a NaN where a number belongs counts as moved)."""
    for defect in case.defects:
        assert L.defect_moves(case, defect) >= 10.0, (case.name, defect, L.defect_moves(case, defect))


def test_clean_reference_scores_zero_and_a_perturbation_at_the_gate_is_seen():
    c = next(c for c in L.CASES if c.name == "f32_T2_B16_H16")
    ref = L.clean_reference(c)
    assert max(L.score(c, ref, ref).values()) == 0.0
    bad = dict(ref, y=ref["y"] + 3e-6)
    assert 1.0 < L.score(c, bad, ref)["y"] < 1.5 + 1e-9


@pytest.mark.parametrize("T,B,H,lens", [(4, 5, 8, [4, 3, 3, 1, 1]), (3, 18, 12, [3] * 7 + [2] * 6 + [1] * 5), (1, 1, 4, [1])])
def test_reference_agrees_with_the_oracle(T, B, H, lens):
    """fp64 forward and closed-form backward against oracle.upit.blstm_padded in float64 with autograd (the input projection is
    made the identity, so that x IS gx and x.grad IS dgx)."""
    from oracle import upit as OU
    r = np.random.RandomState(T * 100 + H)
    whh = r.rand(2, 4 * H, H) * 2 - 1
    gx_gm = r.randn(T, B, 2, 4 * H)                          # gate-major
    valid = np.arange(T)[:, None] < np.asarray(lens)[None, :]
    h0, c0, dy, dhn, dcn = r.randn(2, B, H), r.randn(2, B, H), r.randn(T, B, 2 * H), r.randn(2, B, H), r.randn(2, B, H)
    inp = dict(gx=L.to_interleaved(gx_gm, H), whh=whh, h0=h0, c0=c0, dy=dy, dhn=dhn, dcn=dcn, lens=lens)
    fwd = L.ref_forward(inp)
    bwd = L.ref_backward(inp, fwd)
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    x = t(gx_gm.reshape(T, B, 8 * H)).requires_grad_(True)
    eye = torch.eye(8 * H, dtype=torch.float64)
    ws = [[(eye[d * 4 * H:(d + 1) * 4 * H].clone(), t(whh[d]).requires_grad_(True), torch.zeros(4 * H, dtype=torch.float64, requires_grad=True),
            torch.zeros(4 * H, dtype=torch.float64)) for d in range(2)]]
    h0t, c0t = t(h0).requires_grad_(True), t(c0).requires_grad_(True)
    y, hn, cn = OU.blstm_padded(x, lens, ws, h0t, c0t)
    ((y * t(dy)).sum() + (hn * t(dhn)).sum() + (cn * t(dcn)).sum()).backward()
    tol = dict(rtol=0, atol=1e-12)
    np.testing.assert_allclose(fwd["y"], y.detach().numpy(), **tol)
    np.testing.assert_allclose(fwd["hn"], hn.detach().numpy(), **tol)
    np.testing.assert_allclose(fwd["cn"], cn.detach().numpy(), **tol)
    assert np.isnan(fwd["gates"][~valid]).all() and np.isnan(fwd["c"][~valid]).all() and not np.isnan(fwd["gates"][valid]).any()
    np.testing.assert_allclose(L.to_gate_major(bwd["dgx"], H).reshape(T, B, 8 * H), x.grad.numpy(), **tol)
    np.testing.assert_allclose(bwd["dh0"], h0t.grad.numpy(), **tol)
    np.testing.assert_allclose(bwd["dc0"], c0t.grad.numpy(), **tol)
    for d in range(2):
        np.testing.assert_allclose(bwd["dwhh"][d], ws[0][d][1].grad.numpy(), **tol)
        np.testing.assert_allclose(bwd["dbias"][:, d].sum(0), ws[0][d][2].grad.numpy(), **tol)
    np.testing.assert_allclose(L.dwhh_from(bwd["dgx"], fwd["y"], h0, lens), bwd["dwhh"], **tol)


def test_bf16_twin_rounds_the_product_operands_only():
    """The twin against oracle/upit_bf16.py (fp32 arithmetic around bf16-rounded product operands): same rounding rule bit for
    bit, results within fp32's own error of each other; with operands that ARE bf16 values the twin is the fp64 reference."""
    from oracle import upit_bf16 as OB
    x = np.random.RandomState(3).randn(4096).astype(np.float32) * np.float32(3.7)
    assert np.array_equal(L.rne_bf16(x), OB.rnd(torch.from_numpy(x)).double().numpy())
    T, B, H, lens = 3, 5, 8, [3, 3, 2, 1, 1]
    r = np.random.RandomState(7)
    f = lambda a: a.astype(np.float32).astype(np.float64)
    whh, gx_gm = f(r.rand(2, 4 * H, H) * 2 - 1), f(r.randn(T, B, 2, 4 * H))
    h0, c0 = f(r.randn(2, B, H)), f(r.randn(2, B, H))
    inp = dict(gx=L.to_interleaved(gx_gm, H), whh=whh, h0=h0, c0=c0, lens=lens)
    twin = L.ref_forward(inp, bf=True)
    t = lambda a: torch.tensor(a, dtype=torch.float32)
    eye = torch.eye(8 * H)
    ws = [[(eye[d * 4 * H:(d + 1) * 4 * H].clone(), t(whh[d]), torch.zeros(4 * H), torch.zeros(4 * H)) for d in range(2)]]
    # (the oracle rounds the projection's operands too: give it bf16-exact gx so that only the recurrent product differs)
    gxr = L.rne_bf16(gx_gm)
    y, hn, cn = OB.blstm_padded(t(gxr.reshape(T, B, 8 * H)), lens, ws, t(h0), t(c0))
    twin_r = L.ref_forward(dict(inp, gx=L.to_interleaved(gxr, H)), bf=True)
    np.testing.assert_allclose(twin_r["y"], y.double().numpy(), rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(twin_r["cn"], cn.double().numpy(), rtol=2e-3, atol=2e-4)
    assert np.abs(twin["y"] - L.ref_forward(inp)["y"]).max() > 1e-4          # the rounding is visible ...
    exact = dict(inp, whh=L.rne_bf16(whh), h0=L.rne_bf16(h0), lens=[1] * B)
    exact["gx"] = exact["gx"][:1]
    np.testing.assert_array_equal(L.ref_forward(exact, bf=True)["y"], L.ref_forward(exact)["y"])    # ... and is of the operands only


@pytest.mark.parametrize("bf", [False, True])
def test_probe_algebra_is_the_reference_and_sees_a_piece_in_the_wrong_slot(bf):
    """The one-hot probes' closed forms, fed the fp64 reference's own first-step outputs, give the reference's second step; an
    image read one chunk, one half-octet or one k off, or a dropped term, moves the expected gates by far more than the probe
    gate at EVERY probed k."""
    H, B, T, KS = 44, 32, L.PROBE_T, 20
    rows = np.arange(B)
    for kof in L.probe_assignment(H, B, L.probe_ks(H, KS, bf)):
        whh, gx = L.probe_weights(H), L.probe_fwd_inputs(H, B, kof)
        inp = dict(gx=gx.astype(np.float64), whh=whh, h0=np.zeros((2, B, H)), c0=np.zeros((2, B, H)), lens=[T] * B)
        f = L.ref_forward(inp, bf)
        first = np.stack([f["y"][0, :, :H], f["y"][1, :, H:]])
        yf = first[np.arange(2)[:, None], rows[None, :], kof]
        assert abs(yf - L.PROBE_H1).max() < 1e-15 and np.sort(np.abs(first), axis=2)[:, :, -2].max() < 1e-17
        want = L.probe_fwd_expected(whh, gx, kof, yf, bf)
        second = np.stack([f["gates"][1, :, 0], f["gates"][0, :, 1]], 1)
        assert np.abs(second - want).max() < 1e-7 * (1 if not bf else 1e-6) + 1e-8          # (fp64 h1 against its fp32 copy)
        for shift in (1, 4, 16, 32):
            moved = np.abs(want - L.probe_fwd_expected(whh, gx, kof, yf, bf, shift=shift)).reshape(B, 2, -1).max(2)
            assert moved.min() >= 10 * L.PROBE_ATOL, (shift, moved.min())
        gates, cs, c0, dy = L.probe_bwd_inputs(H, B, kof)
        binp = dict(dy=dy.astype(np.float64), whh=whh, c0=c0.astype(np.float64), h0=np.zeros((2, B, H)), dhn=None, dcn=None, lens=[T] * B)
        b = L.ref_backward(binp, dict(gates=gates.astype(np.float64), c=cs.astype(np.float64), y=np.zeros((T, B, 2 * H))), bf)
        dfirst = np.stack([b["dgx"][T - 1, :, 0], b["dgx"][0, :, 1]], 1).reshape(B, 2, H, 4)
        open_ = dfirst[rows[:, None], np.arange(2)[None, :], kof.T]
        gsecond = np.stack([b["dgx"][0, :, 0], b["dgx"][T - 1, :, 1]], 1)
        d2, dh0, dc0 = L.probe_bwd_expected(whh, gates, cs, c0, kof, open_, bf, dgx_second=gsecond)
        for got, ref in ((d2, gsecond), (dh0, b["dh0"]), (dc0, b["dc0"])):
            assert np.abs(got - ref).max() < 1e-12
        wrong = L.probe_bwd_expected(whh, gates, cs, c0, (kof + 4) % H, open_, bf, dgx_second=gsecond)[0]
        assert L.ratio(wrong, d2, *L.TOL_F32["dgx"]) >= 10


def test_probe_sets_visit_what_they_promise():
    for p in L.PROBES:
        plan = p.case().plan("fwd", p.kind)
        seen = set(np.concatenate([k.ravel() for k in p.kofs()]).tolist())
        if p.kind == 2:
            assert plan["persistent"] is False and all(sorted(k[d].tolist()) == list(range(p.H)) for k in p.kofs() for d in range(2))
            assert not np.array_equal(p.kofs()[0][0], p.kofs()[0][1])
        else:
            assert plan["persistent"] and seen == set(L.probe_ks(p.H, plan["KS"], plan["b16"]))
            assert {0, 3, 4, 7, 8, 15, 16, 31, 32, 8 * plan["KS"] - 1, 8 * plan["KS"], p.H - 5, p.H - 4, p.H - 1} & set(range(p.H)) <= seen
    assert {p.H for p in L.PROBES if p.kind == 2} == {324, 612, 644, 900, 1024}
    ks = {(p.flavour, p.case().plan("fwd", 1)["KS"]) for p in L.PROBES if p.kind == 1}
    assert ks == {("f32", 20), ("f32", 38), ("f32", 56), ("f32", 64), ("bf16", 20), ("bf16", 40), ("bf16", 56), ("bf16", 64),
                  ("s3", 20), ("s3", 40), ("s3", 56), ("xl8", 56)}
