"""sepkern/cacgmm.py, the numpy definition of sk_cacgmm, against closed forms and invariances, a refinement check, and the
gates of tests/test_gpu_cacgmm.py turned on mutants of the definition (the manner of tests/test_streaming_cases.py): every
mutant -- a mistake a kernel could make -- fails a gate on a case of the GPU test's list, and the definition passes them all."""
import functools

import numpy as np
import pytest

from sepkern import cacgmm as cg
import _cacgmm_cases as cc
from _cacgmm_cases import F, LOADING, cond_bound, inputs

T0 = 120


def checked_reference(Y, prior, S, I, Lb, Lc, loading=LOADING, B_in=None):
    """cacgmm_reference, with the conditioning of every state of every iteration asserted: every case goes through here."""
    mask, B, d = cg.cacgmm_reference(Y, prior, S, I, Lb, Lc, loading, B_in=B_in)
    assert len(d["states"]) == I + 1
    for st in d["states"]:
        assert float(np.max(np.linalg.cond(st))) <= cond_bound(Y.shape[0], loading)
    return mask, B, d


@functools.lru_cache(maxsize=None)
def reference(C, S, T, I, Lb, Lc):
    Y, prior, _ = inputs(C, S, T)
    return checked_reference(Y, prior, S, I, Lb, Lc)


@pytest.mark.parametrize("C,S", [(2, 2), (5, 4)])
def test_no_iterations_give_the_prior(C, S):
    Y, prior, _ = inputs(C, S, 33)
    mask, B, _ = checked_reference(Y, prior, S, 0, 16, 5, LOADING)
    p = cg.prior_weights(prior, S, 0, 33).reshape(33, S * F)
    assert mask.dtype == np.float32 and mask.tobytes() == p.astype(np.float32).tobytes()
    assert np.array_equal(B, np.broadcast_to(np.eye(C), B.shape))
    assert np.allclose(p.reshape(33, S, F).sum(axis=1), 1.0, atol=1e-15) and p.min() > 0.0


@pytest.mark.parametrize("C,S", [(2, 2), (4, 2), (8, 4)])
def test_one_step_from_the_identity_is_the_closed_form(C, S):
    T, Lb, Lc = 33, 16, 5
    Y, prior, _ = inputs(C, S, T)
    gammas, qs, Bn, d = cg.cacgmm_step(Y, prior, None, S, Lb, Lc, LOADING)
    for j in range(cg.num_blocks(T, Lb)):
        _, _, w0, w1 = cg.block_window(j, T, Lb, Lc)
        p = cg.prior_weights(prior, S, w0, w1)
        assert np.array_equal(gammas[j], p) and np.all(qs[j] == 1.0)
        y = np.transpose(Y[:, w0:w1], (1, 2, 0)).astype(np.complex128)
        z = y / np.linalg.norm(y, axis=-1, keepdims=True)
        want = C * np.einsum("tkf,tfa,tfb->kfab", p, z, np.conj(z)) / p.sum(axis=0)[:, :, None, None]
        tr = np.trace(want, axis1=-2, axis2=-1).real
        want = want + (LOADING * tr / C)[:, :, None, None] * np.eye(C)
        assert np.max(np.abs(Bn[j] - want)) <= 1e-12 * np.max(np.abs(want))
    assert np.array_equal(Bn, np.conj(np.swapaxes(Bn, -1, -2)))
    _, B1, _ = checked_reference(Y, prior, S, 1, Lb, Lc, LOADING)           # the same step through the reference: every state's conditioning
    assert B1.tobytes() == Bn.tobytes()


def test_a_power_of_two_on_every_frame_changes_no_bit():
    C, S, T = 4, 3, 40
    Y, prior, _ = inputs(C, S, T)
    scale = 2.0 ** np.random.default_rng(3).integers(-20, 21, T)
    Y2 = (Y * scale[None, :, None]).astype(np.complex64)
    a = checked_reference(Y, prior, S, 2, 16, 4, LOADING)
    b = checked_reference(Y2, prior, S, 2, 16, 4, LOADING)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_the_scale_of_B_and_a_phase_on_y_are_not_seen():
    C, S, T = 3, 2, 33
    Y, prior, _ = inputs(C, S, T)
    _, B, _ = reference(C, S, T, 2, 16, 5)
    g = cg.cacgmm_posteriors(Y, prior, B, S, 16)
    assert np.max(np.abs(cg.cacgmm_posteriors(Y, prior, 7.3 * B, S, 16) - g)) <= 1e-12
    phase = np.exp(1j * np.random.default_rng(5).uniform(0, 6.28, (1, T, F))) * 1.7
    Yp = (Y * phase).astype(np.complex64)
    assert np.max(np.abs(cg.cacgmm_posteriors(Yp, prior, B, S, 16) - g)) <= 1e-5          # complex64 rounds Y * phase


def test_permuting_the_priors_columns_permutes_the_outputs():
    C, S, T = 4, 3, 33
    Y, prior, _ = inputs(C, S, T)
    perm = [2, 0, 1]
    pp = np.ascontiguousarray(prior.reshape(T, S, F)[:, perm]).reshape(T, S * F)
    mask, B, d = reference(C, S, T, 3, 16, 5)
    mask_p, B_p, d_p = checked_reference(Y, pp, S, 3, 16, 5, LOADING)
    # the fp64 posteriors and the states, absolutely (gamma <= 1; the entries of B are O(C))
    assert np.max(np.abs(d_p["gamma"].reshape(T, S, F) - d["gamma"].reshape(T, S, F)[:, perm])) <= 1e-12
    assert np.max(np.abs(B_p - B[:, perm])) <= 1e-12
    assert np.max(np.abs(mask_p.reshape(T, S, F) - mask.reshape(T, S, F)[:, perm])) <= 2.0 ** -23    # the float32 outputs: one rounding apart at most


def test_dead_frames_get_the_prior_and_change_no_sum():
    C, S, T, Lb, Lc = 3, 2, 40, 16, 4
    Y, prior, _ = inputs(C, S, T)
    dead = [3, 17, 18, 39]
    Yd = np.array(Y)
    Yd[:, dead] = 0.0
    Yd[1, 17, 5] = -0.0
    mask, B, _ = checked_reference(Yd, prior, S, 2, Lb, Lc, LOADING)
    p = cg.prior_weights(prior, S, 0, T).reshape(T, S * F).astype(np.float32)
    assert mask[dead].tobytes() == p[dead].tobytes()
    # the same recording with the dead frames cut out (one window, so that no block edge moves)
    keep = [t for t in range(T) if t not in dead]
    m1, B1, _ = checked_reference(Yd, prior, S, 2, T, 0, LOADING)
    m2, B2, _ = checked_reference(np.ascontiguousarray(Yd[:, keep]), np.ascontiguousarray(prior[keep]), S, 2, T, 0, LOADING)
    assert B1.tobytes() == B2.tobytes() and m1[keep].tobytes() == m2.tobytes()


def test_an_all_dead_window_gives_the_prior_and_the_identity():
    C, S, T, Lb = 3, 2, 24, 8
    Y, prior, _ = inputs(C, S, T)
    Yd = np.array(Y)
    Yd[:, 8:16] = 0.0
    mask, B, _ = checked_reference(Yd, prior, S, 3, Lb, 0, LOADING)
    p = cg.prior_weights(prior, S, 0, T).reshape(T, S * F).astype(np.float32)
    assert mask[8:16].tobytes() == p[8:16].tobytes() and np.array_equal(B[1], np.broadcast_to(np.eye(C), B[1].shape))
    assert not np.array_equal(B[0], B[1]) and mask[:8].tobytes() != p[:8].tobytes()


def test_a_state_that_is_not_positive_definite_is_reset():
    C, S, T = 2, 2, 9
    Y, prior, _ = inputs(C, S, T)
    B_in = np.broadcast_to(np.eye(C, dtype=np.complex128), (1, S, F, C, C)).copy()
    B_in[0, 1, 7] = [[1.0, 2.0], [2.0, 1.0]]
    B_in[0, 0, 9] = np.nan
    mask, B, _ = checked_reference(Y, prior, S, 0, 16, 0, LOADING, B_in=B_in)
    p = cg.prior_weights(prior, S, 0, T).reshape(T, S * F).astype(np.float32)
    assert np.array_equal(B, np.broadcast_to(np.eye(C), B.shape)) and mask.tobytes() == p.tobytes()


@pytest.mark.parametrize("C,S", [(2, 2), (4, 2), (8, 2), (3, 3)])
def test_the_refinement_helps(C, S):
    """Mean |gamma - dominant| below the prior's, dominant = 1 for the source with the strongest image."""
    Y, prior, dom = inputs(C, S, T0)
    base = float(np.mean(np.abs(cg.prior_weights(prior, S, 0, T0) - dom)))
    for I in (1, 3, 5):
        _, _, d = reference(C, S, T0, I, T0, 0)
        ratio = float(np.mean(np.abs(d["gamma"].reshape(T0, S, F) - dom))) / base
        print("  C=%d S=%d I=%d: mean |gamma - dominant| is %.3f of the prior's" % (C, S, I, ratio))
        assert ratio < 1.0


# ---- the GPU gates on mutants of the definition
def mutant(name):
    """The definition with one mistake, as an implementation the gates take."""
    def impl(Y, prior, S, iterations, Lb, Lc, loading, B_in):
        C, T = Y.shape[0], Y.shape[1]
        nblk = cg.num_blocks(T, Lb)
        B = np.stack([cg.admit(Bj)["B"] for Bj in cg._state(B_in, nblk, S, C)])
        admit = lambda Bj: dict(cg.admit(Bj), sld=np.zeros((S, F))) if name == "no log det" else cg.admit(Bj)
        for _ in range(iterations):
            Bn = np.zeros_like(B)
            for j in range(nblk):
                b0, _, w0, w1 = cg.block_window(j, T, Lb, Lc)
                if name == "window clipped at the block" and j * Lb - Lc < 0:
                    w0 = b0
                if name == "context frame dropped" and w0 < b0:
                    w0 += 1
                zr, zi, live = cg.directions(Y, w0, w1)
                p = cg.prior_weights(prior, S, w0, w1)
                gamma, q, _ = cg.e_step(zr, zi, live, p, admit(B[j]))
                summed = live.copy()
                if name == "last frame of a chunk dropped":
                    summed[63::64] = False
                if name == "q of the new B":
                    q = cg.e_step(zr, zi, live, p, cg.m_step(zr, zi, summed, gamma, q, loading))[1]
                st = cg.m_step(zr, zi, summed, gamma, q, 0.0 if name == "no loading" else loading)
                Bn[j] = np.where(st["reset"][..., None, None], st["B"], st["B"] / C) if name == "factor C missing" else st["B"]
            B = Bn
        mask = np.zeros((T, S * F), dtype=np.float32)
        for j in range(nblk):
            b0, b1, _, _ = cg.block_window(j, T, Lb, 0)
            zr, zi, live = cg.directions(Y, b0, b1)
            mask[b0:b1] = cg.e_step(zr, zi, live, cg.prior_weights(prior, S, b0, b1), admit(B[j]))[0].reshape(b1 - b0, S * F)
        return mask, B
    return impl


def failed_gates(impl, C, S, gi):
    out = []
    for I in (0, 1, 3):
        if not cc.gate_posteriors(impl, C, S, gi, I)[0]:
            out.append("posteriors I=%d" % I)
    for from_identity in (True, False):
        if not cc.gate_one_step(impl, C, S, gi, from_identity)[0]:
            out.append("one step from %s" % ("the identity" if from_identity else "two iterations"))
    if not cc.gate_chaining(impl, C, S, gi):
        out.append("chaining")
    return out


# the case of the GPU test's list (tests/_cacgmm_cases.py: CS x GEOMETRIES) on which each mutant is looked at
MUTANTS = [("last frame of a chunk dropped", (2, 2), 6), ("context frame dropped", (2, 2), 3), ("q of the new B", (3, 3), 0),
           ("factor C missing", (2, 2), 0), ("no log det", (3, 3), 2), ("no loading", (4, 2), 1),
           ("window clipped at the block", (2, 2), 4)]


@pytest.mark.parametrize("name,cs,gi", MUTANTS)
def test_every_mutant_fails_a_gate(name, cs, gi):
    assert cs in cc.CS and 0 <= gi < len(cc.GEOMETRIES)
    failed = failed_gates(mutant(name), cs[0], cs[1], gi)
    print("  %s: fails %s" % (name, ", ".join(failed) or "nothing"))
    assert failed


@pytest.mark.parametrize("cs,gi", sorted(set((cs, gi) for _, cs, gi in MUTANTS)))
def test_the_definition_passes_every_gate(cs, gi):
    def definition(Y, prior, S, iterations, Lb, Lc, loading, B_in):        # cc.definition, every state's conditioning asserted
        mask, B, _ = checked_reference(Y, prior, S, iterations, Lb, Lc, loading, B_in=B_in)
        return mask, B

    assert failed_gates(definition, cs[0], cs[1], gi) == []
    assert failed_gates(mutant("none"), cs[0], cs[1], gi) == []            # the mutants' scaffold is the definition


def test_the_definition_passes_every_gate_on_blocks_and_windows_of_several_chunks():
    """The geometry the GPU test has for output walks and windows of more than two chunks of 64 frames."""
    gi = len(cc.GEOMETRIES) - 1
    T, Lb, Lc = cc.GEOMETRIES[gi]
    windows = [cg.block_window(j, T, Lb, Lc) for j in range(cg.num_blocks(T, Lb))]
    assert max(b1 - b0 for b0, b1, _, _ in windows) > 2 * 64 and max(w1 - w0 for _, _, w0, w1 in windows) > 2 * 64
    assert failed_gates(cc.definition, 2, 2, gi) == []
    assert "one step from the identity" in failed_gates(mutant("last frame of a chunk dropped"), 2, 2, gi)


BAD = [dict(C=1), dict(C=9), dict(S=1), dict(S=5), dict(T=0), dict(iterations=-1), dict(iterations=17), dict(block_frames=0),
       dict(context_frames=-1), dict(block_frames=4000, context_frames=49), dict(loading=-1e-3), dict(loading=float("nan")),
       dict(ld_prior=2 * F - 1), dict(ld_out=2 * F - 1), dict(y_row_stride=256), dict(have_Y=False), dict(have_prior=False),
       dict(have_mask_out=False)]


@pytest.mark.parametrize("bad", BAD)
def test_check_arguments_refuses_what_the_kernel_refuses(bad):
    good = dict(C=3, S=2, T=20, iterations=2, block_frames=8, context_frames=1, loading=LOADING, ld_prior=2 * F, ld_out=2 * F,
                y_row_stride=F)
    cg.check_arguments(**good)
    cg.check_arguments(**dict(good, iterations=0, block_frames=4096, context_frames=0, loading=0.0))
    with pytest.raises(ValueError, match="cacgmm: "):
        cg.check_arguments(**dict(good, **bad))
    assert cg.workspace_bytes(20, 3, 2, 8, 1) == 0
