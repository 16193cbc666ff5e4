"""The cases of tests/test_gpu_stoi_kernels.py can catch what they are meant to catch (runs on any machine).

The cases' claims -- F, nkept, T, the boundary each sits on, no frame within 1 dB of the keep threshold -- are asserted from
the host definition (sepkern/stoi.py) alone; the models of the three kernels in tests/_stoi_cases.py equal that definition;
and every defect model -- a scan that loses or doubles the carry between its trips or drops a wave's count, a kept row
written with the wrong stride, a neighbour frame taken from the wrong place, a missing tile, T or J off by one, a score tile
loaded short, bands shifted, the estimate index or the output matrix mixed up -- moves a quantity the GPU test checks by at
least 10 x its tolerance (exact quantities: at all) on the case named with it.
"""
import numpy as np
import pytest

import _stoi_cases as SC
from sepkern import stoi as ST

MARGIN = 10.0


def test_the_cases_sit_on_the_boundaries_they_claim():
    worst = SC.check_claims()
    print("smallest |keep margin| over the cases: %.1f dB" % worst)
    assert all(c.n < 80000 for c in SC.CASES)


def test_constants_are_within_their_caps():
    assert isinstance(SC.K_ENV, int) and 1 <= SC.K_ENV <= 12          # twice the measured 5.663, rounded up, at the most
    assert 0.0 < SC.SCORE_GATE <= 1e-9


def test_the_restated_workspace_is_the_librarys():
    from sepkern import _lib
    try:
        lib = _lib.load()
    except _lib.SepkernError:
        lib = None
    for U, S, n in ((1, 1, 1), (1, 1, 257), (3, 2, 33025), (30, 1, 77056), (2, 4, 16896), (7, 3, 4000), (5, 4, 79999)):
        lay = SC.workspace(U, S, n)
        Fm = lay["Fm"]
        assert Fm == max(1, ST.frame_starts(n).size)
        assert all(lay[k] % 256 == 0 for k in ("offs", "lens", "nkept", "kept", "energy", "env", "bytes"))
        assert lay["offs"] == 0 and lay["lens"] >= 8 * U and lay["nkept"] - lay["lens"] >= 4 * U
        assert lay["kept"] - lay["nkept"] >= 4 * U * S and lay["energy"] - lay["kept"] >= 4 * U * S * Fm
        assert lay["env"] - lay["energy"] >= 8 * U * S * Fm and lay["bytes"] - lay["env"] >= 4 * U * S * (S + 1) * 15 * Fm
        if lib is not None:
            assert lib.sk_stoi_workspace_bytes(U, S, n) == lay["bytes"], (U, S, n)
    assert SC.env_row(3, 2, 1, 4) == (3 * 3 + 1) * 15 + 4


@pytest.mark.parametrize("name", [c.name for c in SC.CASES])
def test_the_host_definition_reads_no_poisoned_sample(name):
    """NaN where sk_stoi must not read leaves every host result as it was: those samples are outside the definition."""
    c = SC.BY_NAME[name]
    h = c.host()
    refs, ests = c.poisoned()
    assert np.isnan(refs[:, c.n - 1]).all() and np.isnan(ests[:, c.n - 1]).all()
    if c.F == 0:
        assert np.isnan(refs).all() and np.isnan(ests).all()
    else:
        assert not np.isnan(refs[:, :SC.last_read(c.n)]).any()
        assert all(np.isnan(ests).any(axis=1)) and np.isnan(ests).sum() >= c.S * (c.n - SC.last_read(c.n))
    m, fr = ST.stoi_matrix(list(refs), list(ests))
    assert np.array_equal(m, h["m64"]) and fr.tolist() == h["frames"].tolist()
    for j in range(c.S):
        assert ST.kept_frames(refs[j]).tolist() == h["kept"][j].tolist()


@pytest.mark.parametrize("name", [c.name for c in SC.CASES])
def test_the_models_are_the_host_definition(name):
    c = SC.BY_NAME[name]
    h = c.host()
    refs, ests = c.signals()
    for j in range(c.S):
        row, nk = SC.scan(SC.keep_flags(refs[j]))
        assert nk == len(h["kept"][j]) and row[:nk].tolist() == h["kept"][j].tolist() and (row[nk:] == -1).all()
        assert (h["energy"][j] > 0).all() or c.runs[j] is None
        assert (h["etol"][j] <= 1e-12 * h["energy"][j]).all()
        rows = SC.envelope_rows(c, j)
        for q, e in enumerate(rows):
            ref = h["env"][j][q]
            assert e.shape == ref.shape == (15, h["T"][j])
            if e.size:
                assert np.abs(e - ref).max() <= 1e-13 * np.abs(ref).max()
                assert (h["e_ref"][j][q] > 0).all()
                # single precision: a few 2^-24 of the frame's largest envelope
                assert (h["e_ref"][j][q] <= 8 * 2.0 ** -24 * np.abs(ref).max(axis=0)).all()
        for k in range(c.S):
            want = ST.scores(h["env"][j][0], h["env"][j][1 + k])
            got = SC.score_model(rows[0], rows[1 + k])
            assert np.abs(np.array(got) - np.array(want)).max() <= 1e-12
            assert np.abs(np.array(want) - h["m64"][k, j]).max() == 0.0
    m, fr = SC.matrix_model(c)
    assert fr.tolist() == h["frames"].tolist() and np.abs(m - h["m64"]).max() <= 1e-12
    short = h["frames"] < 30
    assert np.all(m[:, short] == 1e-5)


def test_the_gate_of_the_end_to_end_check_is_far_below_a_definitional_slip():
    g = 4.0 * max(float(np.abs(c.host()["m64"] - c.host()["m32"]).max()) for c in SC.CASES)
    print("end-to-end gate g = %.3g" % g)
    assert 0.0 < g < 1e-5


# ------------------------------------------------------------------------------------------------ defects
def _kept_differs(name, defect):
    c = SC.BY_NAME[name]
    refs, _ = c.signals()
    good, bad = SC.scan(SC.keep_flags(refs[0])), SC.scan(SC.keep_flags(refs[0]), defect)
    return good[1] != bad[1] or good[0][:good[1]].tolist() != bad[0][:good[1]].tolist()


@pytest.mark.parametrize("defect,caught,missed", [
    ("carry_lost", ("all257", "all512", "all513", "across_255_256", "across_511_512", "trips_0_2", "waves"), ("all255", "all256")),
    ("carry_twice", ("all257", "all513", "trip1_only", "trips_0_2"), ("nkept0", "n256")),
    ("wave_dropped", ("all255", "all256", "all513", "waves"), ("T31",)),
])
def test_scan_defects_change_the_kept_list(defect, caught, missed):
    """Exact quantities: nkept or kept[:nkept] differs.  The cases named `missed` cannot see the defect, by construction."""
    for name in caught:
        assert _kept_differs(name, defect), (defect, name)
    for name in missed:
        assert not _kept_differs(name, defect), (defect, name)


def test_a_kept_row_written_with_stride_F_shows_in_the_mixed_batch():
    for S in (1, 2, 3, 4):
        cases = SC.group(S)
        good, bad = SC.kept_rows(cases), SC.kept_rows(cases, "kept_stride_F")
        assert good.shape == bad.shape
        wrong = [sig for sig in range(good.shape[0]) if not np.array_equal(good[sig], bad[sig])]
        assert wrong, S
        # alone every utterance's F is the stride: the defect shows only in the batch
        for c in cases:
            assert np.array_equal(SC.kept_rows([c]), SC.kept_rows([c], "kept_stride_F"))


def _env_hits(c, defect):
    """Largest err / tolerance over the signals and frames of case c under the defect, with the float32 model sane on the frame."""
    h, worst = c.host(), 0.0
    for j in range(c.S):
        for q, bad in enumerate(SC.envelope_rows(c, j, defect)):
            ref, e_ref = h["env"][j][q], h["e_ref"][j][q]
            if not ref.size:
                continue
            ratio = SC.frame_err(bad, ref) / SC.env_tolerance(ref, e_ref)
            t = int(np.argmax(ratio))
            assert e_ref[t] <= 1e-5 * np.abs(ref[:, t]).max()
            worst = max(worst, float(ratio[t]))
    return worst


@pytest.mark.parametrize("defect,caught,missed", [
    ("nxt_adjacent", ("T17_far", "T32_far", "T33_far", "trips_0_2", "waves"), ("T16", "all513", "s3_b")),
    ("no_prv_at_tile", ("T17_far", "T31", "T33_far", "all257", "s4_a"), ("T15", "T16")),
    ("tail_tile_dropped", ("T15", "T17_far", "T31", "T33_far", "T1", "s2_a"), ("T16", "T32_far")),
    ("bands_shifted", ("T1", "T16", "all513", "s4_b"), ()),
    ("est_index", ("s2_a", "s2_b", "s3_a", "s4_a"), ("T31",)),
])
def test_envelope_defects_miss_the_tolerance_by_ten(defect, caught, missed):
    for name in caught:
        r = _env_hits(SC.BY_NAME[name], defect)
        print("%s on %s: %.3g x the tolerance" % (defect, name, r))
        assert r >= MARGIN, (defect, name, r)
    for name in missed:
        assert _env_hits(SC.BY_NAME[name], defect) <= 1.0, (defect, name)


@pytest.mark.parametrize("defect,caught,missed", [
    ("drop_m64", ("T94", "T157", "T158", "all257", "s4_a"), ("T93", "T46")),
    ("tile_short", ("T94", "T158", "all513", "s4_a"), ("T93",)),
    ("J_less_one", ("T30", "T31", "T46", "T94", "s2_a"), ("T29",)),
    ("transposed", ("s2_a", "s2_b", "s3_a", "s3_b", "s4_a", "s4_b"), ("T94",)),
])
def test_score_defects_miss_the_gate_by_ten(defect, caught, missed):
    """The score kernel is checked against scores() in float64 on its own envelopes within SCORE_GATE."""
    for name in caught + missed:
        c = SC.BY_NAME[name]
        good, _ = SC.matrix_model(c)
        bad, _ = SC.matrix_model(c, defect)
        d = float(np.abs(good - bad).max())
        print("%s on %s: moves a score by %.3g (gate %.3g)" % (defect, name, d, SC.SCORE_GATE))
        if name in caught:
            assert d >= MARGIN * SC.SCORE_GATE, (defect, name, d)
        else:
            assert d == 0.0, (defect, name, d)


def test_T_taken_as_nkept_changes_frames():
    for c in SC.CASES:
        _, fr = SC.matrix_model(c, "T_is_nkept")
        differs = fr.tolist() != c.host()["frames"].tolist()
        assert differs == any(n > 0 for n in c.nkept()), c.name


def test_every_defect_model_is_exercised():
    import inspect
    src = inspect.getsource(inspect.getmodule(test_every_defect_model_is_exercised))
    for d in SC.KEEP_DEFECTS + SC.ENV_DEFECTS + SC.SCORE_DEFECTS + SC.OTHER_DEFECTS:
        assert '"%s"' % d in src, d
    assert len(SC.KEEP_DEFECTS + SC.ENV_DEFECTS + SC.SCORE_DEFECTS + SC.OTHER_DEFECTS) == 14
