"""The cases of tests/test_gpu_stft_family.py can catch what they are meant to catch (runs on any machine).

Every forward and inverse case is run through the defect models of tests/_stft_cases.py -- a kernel that pads symmetrically
or with zeros, reads the next utterance, transforms a stale tile, swaps mirrored bins, drops bin 128; that loses a
workgroup's three prelude frames, leaves a ring slot unrefilled, normalises the edge hops with the full window-sum-square,
skips the tail tile, takes the next source's mask or swaps two bins of a slot -- and on at least one frame (forward) or hop
(inverse) the error each leaves against the float64 reference must be at least 10 x the tolerance the GPU test asserts
there, with the final K of its family.  The float64 references are checked against oracle/stft.py.
"""
import numpy as np
import pytest

import _stft_cases as SC
from oracle import stft as OS

MARGIN = 10.0


def _caught(family, ref, e_ref, norms, bad, what):
    """The defect shows on at least one frame / hop by MARGIN x its tolerance; on the frames it shows the float32 model is sane."""
    err, tol = SC.unit_err(bad, ref), SC.tolerance(family, ref, e_ref)
    hit = err >= MARGIN * tol
    assert hit.any(), "%s: the defect leaves at most %.3g x the tolerance" % (what, float((err / tol).max()))
    assert (e_ref[hit] <= 1e-5 * norms[hit]).all(), (what, float((e_ref[hit] / norms[hit]).max()))
    return float((err / tol).max())


def test_every_family_factor_is_within_the_cap():
    assert set(SC.K) == {"stft_complex", "stft_mag", "istft", "istft_rows"}
    assert all(isinstance(k, int) and 1 <= k <= 8 for k in SC.K.values()), SC.K


def test_the_cases_sit_on_the_boundaries_they_claim():
    SC.check_forward_claims()
    SC.check_inverse_claims()
    SC.check_tpb4_claims()
    SC.check_rows_claims()


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("fmt", ["float32", "int16"])
def test_forward_reference_is_the_oracle_and_its_float32_model_is_single_precision(fmt):
    c = SC.fwd_case(fmt)
    for N, y, ref, e_c, e_m, norms in zip(SC.FWD_LENGTHS, c["y"], c["ref"], c["e_c"], c["e_m"], c["norms"]):
        assert np.array_equal(SC.padded(y), np.pad(y, 256, mode="reflect"))
        assert ref.dtype == np.complex128 and ref.shape == (SC.num_frames(N), SC.NBIN)
        assert np.array_equal(ref.T.astype(np.complex64), OS.stft(y))                    # exactly, after rounding
        assert (e_c > 0).all() and (e_m > 0).all()
        # single precision: a few 2^-24 of the windowed frame's norm per frame
        assert (e_c <= 8 * 2.0 ** -24 * norms).all() and (e_m <= 8 * 2.0 ** -24 * norms).all()
    if fmt == "int16":
        assert all(p.dtype == np.int16 and np.abs(p.astype(np.int32)).max() <= 20000 for p in c["raw"])


@pytest.mark.parametrize("fmt", ["float32", "int16"])
@pytest.mark.parametrize("i", range(len(SC.FWD_LENGTHS)), ids=["N%d" % n for n in SC.FWD_LENGTHS])
def test_forward_cases_catch_every_defect(i, fmt):
    c = SC.fwd_case(fmt)
    y, ref, norms = c["y"][i], c["ref"][i], c["norms"][i]
    defects = SC.fwd_defects(SC.FWD_LENGTHS[i])
    assert ("raw_next" in defects) == (SC.FWD_FRAMES[i] > SC.FPB)
    for d in defects:
        bad = SC.stft_eval(y, defect=d, nxt=SC.fwd_next(c, i))
        what = "stft N=%d %s %s" % (SC.FWD_LENGTHS[i], fmt, d)
        _caught("stft_complex", ref, c["e_c"][i], norms, bad, what)
        _caught("stft_mag", np.abs(ref), c["e_m"][i], norms, np.abs(bad), what + " (magnitudes)")


# ------------------------------------------------------------------------------------------------ inverse
def test_inverse_transform_ignores_the_imaginary_parts_of_dc_and_nyquist():
    X = SC.inv_spec(17, 1)
    assert np.abs(X[:, 0].imag).min() > 0 and np.abs(X[:, 256].imag).min() > 0
    Z = X.copy()
    Z[:, 0] = Z[:, 0].real
    Z[:, 256] = Z[:, 256].real
    for dt in (SC.F64, SC.F32):
        assert np.array_equal(SC.istft_eval(X, dt), SC.istft_eval(Z, dt))


@pytest.mark.parametrize("S", SC.INV_SPEAKERS)
def test_inverse_reference_is_the_oracle(S):
    c = SC.inv_case(S)
    for u, T in enumerate(c["T"]):
        for s in range(S):
            X = SC.masked(c["specs"][u], None if S == 1 else c["masks"][u][s])
            ref, e = c["ref"][u][s], c["e"][u][s]
            assert ref.shape == (T - 1, SC.HOP) and (e > 0).all()
            if S > 1:
                orc, _ = OS.reconstruct(c["specs"][u].T, c["masks"][u][s].T)
            else:
                orc = OS.istft(X.T)
            # the oracle accumulates in float32: four rounded products, three additions, the window sum and a division
            assert np.abs(orc.astype(np.float64) - ref.reshape(-1)).max() <= 16 * float(SC.ulp32(np.abs(ref).max()))


def _inverse_defects(T, S, tpb, spec, masks, ref, e_ref, norms, family, tag):
    defects = SC.inv_defects(T, S, tpb)
    for s in range(S):
        X = SC.masked(spec, None if masks is None else masks[s])
        for d in defects:
            if d == "next_mask":
                bad = SC.istft_eval(SC.masked(spec, masks[(s + 1) % S]))
            else:
                bad = SC.istft_eval(X, defect=d, tpb=tpb)
            _caught(family, ref[s], e_ref[s], norms[s], bad, "%s T=%d S=%d source %d %s" % (tag, T, S, s, d))
    return defects


@pytest.mark.parametrize("S", SC.INV_SPEAKERS)
@pytest.mark.parametrize("u", range(len(SC.INV_FRAMES)), ids=["T%d" % t for t in SC.INV_FRAMES])
def test_inverse_cases_catch_every_defect(u, S):
    c = SC.inv_case(S)
    T = c["T"][u]
    for family in ("istft", "istft_rows"):
        d = _inverse_defects(T, S, 2, c["specs"][u], c["masks"][u], c["ref"][u], c["e"][u], c["norms"][u], family, family)
    assert ("no_prelude" in d) == (T >= 32) and ("stale_slot" in d) == (T > 19) and ("next_mask" in d) == (S > 1)


@pytest.mark.parametrize("T", SC.TPB4_FRAMES)
def test_four_tiles_per_workgroup_cases_catch_every_defect(T):
    u = SC.tpb4_frames().index(T)
    spec, masks = SC.tpb4_utt(u)
    refs = [SC.inv_ref(SC.masked(spec, masks[s])) for s in range(SC.TPB4_S)]
    d = _inverse_defects(T, SC.TPB4_S, 4, spec, masks, [r[0] for r in refs], [r[1] for r in refs], [r[2] for r in refs],
                         "istft", "tpb4")
    assert ("no_prelude" in d) == (T > 64)
    # the workgroups of the alone run (two tiles each) start elsewhere: a lost prelude there shows on other hops
    if T > 64:
        a = SC.unit_err(SC.istft_eval(SC.masked(spec, masks[0]), defect="no_prelude", tpb=4), refs[0][0]) > 1e-4
        b = SC.unit_err(SC.istft_eval(SC.masked(spec, masks[0]), defect="no_prelude", tpb=2), refs[0][0]) > 1e-4
        assert a.sum() == 3 * (len(SC.istft_workgroups(T, 4)) - 1) and b.sum() > a.sum() and (b & ~a).any()


@pytest.mark.parametrize("S", SC.ROWS_SPEAKERS)
def test_packed_row_cases_catch_every_defect(S):
    c = SC.rows_case(S)
    for u, T in enumerate(c["T"]):
        norms = [np.sqrt((r ** 2).sum(axis=1)) for r in c["ref"][u]]
        _inverse_defects(T, S, 2, c["specs"][u], c["masks"][u], c["ref"][u], c["e"][u], norms, "istft_rows", "rows")
