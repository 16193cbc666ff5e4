"""sepkern/mvdr.py, the numpy definition sk_mvdr is held to: the properties an MVDR beamformer must have, on the CPU."""
import numpy as np
import pytest

from sepkern import mvdr as mv
from _mvdr_cases import LOADING, array_case, cond_bound, noise_condition, steering

F = mv.F


def binary_rank_one_case(C, S, T, seed):
    """Disjoint binary masks, exactly rank-1 sources, no noise: every (t, f) cell belongs to one source."""
    rng = np.random.default_rng(seed)
    a = steering(C, S, rng)
    owner = rng.integers(0, S, (T, F))
    X = (rng.standard_normal((S, T, F)) + 1j * rng.standard_normal((S, T, F))) * (owner[None] == np.arange(S)[:, None, None])
    Y = np.einsum("sfc,stf->ctf", a, X).astype(np.complex64)
    mask = np.ascontiguousarray(np.transpose((owner[None] == np.arange(S)[:, None, None]).astype(np.float32), (1, 0, 2)).reshape(T, S * F))
    return Y, mask, a


@pytest.mark.parametrize("C,S,ref", [(2, 2, 0), (4, 3, 2), (8, 4, 7)])
def test_distortionless_towards_a_rank_one_source(C, S, ref):
    Y, mask, a = binary_rank_one_case(C, S, 64, seed=C * 10 + S)
    _, W, _ = mv.mvdr_reference(Y, mask, S, 64, 0, ref, LOADING)
    resp = np.einsum("sfc,sfc->sf", np.conj(W[0].astype(np.complex128)), a)          # W^H a_s
    err = np.max(np.abs(resp - a[:, :, ref]))
    print("C=%d S=%d: max |W^H a - a[ref]| = %.3g" % (C, S, err))
    assert err <= 1e-6


def test_a_context_of_the_whole_recording_gives_one_beamformer():
    c = array_case(3, 2, 50, seed=1)
    for R in (4, 9):                                            # nblk = 5
        _, W, _ = mv.mvdr_reference(c["Y"], c["mask"], 2, 10, R, 0, LOADING)
        assert W.shape == (5, 2, F, 3)
        for j in range(1, 5):
            assert np.array_equal(W[j].view(np.uint32), W[0].view(np.uint32))
    _, W, _ = mv.mvdr_reference(c["Y"], c["mask"], 2, 10, 1, 0, LOADING)
    assert not np.array_equal(W[0], W[4])


def test_permuting_sources_or_channels_permutes_the_weights():
    C, S, T = 4, 3, 40
    c = array_case(C, S, T, seed=2)
    _, W, Z = mv.mvdr_reference(c["Y"], c["mask"], S, 16, 1, 1, LOADING)
    scale = np.max(np.abs(W), axis=-1, keepdims=True)
    sp = np.array([2, 0, 1])
    mask_p = c["mask"].reshape(T, S, F)[:, sp].reshape(T, S * F)
    _, Ws, _ = mv.mvdr_reference(c["Y"], mask_p, S, 16, 1, 1, LOADING)
    assert np.all(np.abs(Ws - W[:, sp]) <= 2.0 ** -20 * scale[:, sp])
    cp = np.array([3, 1, 0, 2])                                 # new channel i is old channel cp[i]: old 1 is new 1 ... ref follows
    ref_new = int(np.where(cp == 1)[0][0])
    _, Wc, Zc = mv.mvdr_reference(c["Y"][cp], c["mask"], S, 16, 1, ref_new, LOADING)
    assert np.all(np.abs(Wc - W[..., cp]) <= 2.0 ** -20 * scale)
    assert np.allclose(Zc, Z, rtol=0, atol=1e-4 * np.max(np.abs(Z)))


@pytest.mark.parametrize("k", [-9, 7])
def test_scaling_the_spectra_by_a_power_of_two_leaves_the_weights_bits(k):
    c = array_case(4, 2, 30, seed=3)
    _, W, Z = mv.mvdr_reference(c["Y"], c["mask"], 2, 8, 1, 0, LOADING)
    _, Wk, Zk = mv.mvdr_reference(c["Y"] * np.float32(2.0 ** k), c["mask"], 2, 8, 1, 0, LOADING)
    assert np.array_equal(W.view(np.uint32), Wk.view(np.uint32))
    assert np.array_equal((Z * np.float32(2.0 ** k)).view(np.uint32), Zk.view(np.uint32))


def test_a_source_silent_over_a_context_passes_the_reference_channel_through():
    C, S, T, Lb, ref = 3, 3, 40, 10, 2
    c = array_case(C, S, T, seed=4)
    mask = c["mask"].copy()
    mask[10:30, F:2 * F] = 0.0                                  # stream 1 over blocks 1 and 2
    e_ref = np.zeros(C, dtype=np.complex64)
    e_ref[ref] = 1.0
    _, W, Z = mv.mvdr_reference(c["Y"], mask, S, Lb, 0, ref, LOADING)
    for j in range(4):
        assert np.all(W[j, 1] == e_ref) == (j in (1, 2))
    assert np.array_equal(Z[1, 10:30], c["Y"][ref, 10:30])
    assert not np.any(np.all(W[:, 0] == e_ref, axis=-1)) and not np.any(np.all(W[:, 2] == e_ref, axis=-1))
    _, W1, _ = mv.mvdr_reference(c["Y"], mask, S, Lb, 1, ref, LOADING)     # a context that reaches an active block: no fallback
    assert not np.any(np.all(W1[:, 1] == e_ref, axis=-1))
    # all other streams silent: N_s == 0
    mask2 = np.zeros_like(mask)
    mask2[:, :F] = c["mask"][:, :F]
    _, W2, _ = mv.mvdr_reference(c["Y"], mask2, S, Lb, 0, ref, LOADING)
    assert np.all(W2 == e_ref)


@pytest.mark.parametrize("T", [1, 6, 7, 8, 22])              # Lb = 7: 1, Lb - 1, Lb, Lb + 1, 3 Lb + 1
def test_block_geometry(T):
    Lb, C, S = 7, 2, 2
    c = array_case(C, S, T, seed=10 + T)
    scm, W, Z = mv.mvdr_reference(c["Y"], c["mask"], S, Lb, 0, 0, LOADING)
    nblk = -(-T // Lb)
    assert scm.shape == (nblk, S, F, C, C) and W.shape == (nblk, S, F, C) and Z.shape == (S, T, F)
    assert W.dtype == np.complex64 and Z.dtype == np.complex64 and scm.dtype == np.complex128
    for j in range(nblk):                                       # a block on its own gives the same matrices and weights
        t0, t1 = j * Lb, min(T, (j + 1) * Lb)
        scm_j, W_j, Z_j = mv.mvdr_reference(c["Y"][:, t0:t1], c["mask"][t0:t1], S, Lb, 0, 0, LOADING)
        assert np.array_equal(scm_j[0], scm[j]) and np.array_equal(W_j[0], W[j]) and np.array_equal(Z_j, Z[:, t0:t1])
    assert np.array_equal(scm, np.conj(np.swapaxes(scm, -1, -2))) and np.all(scm[..., np.arange(C), np.arange(C)].imag == 0.0)
    assert mv.workspace_bytes(T, C, S, Lb) == nblk * S * 3 * 2 * F * 8


def test_the_loading_bounds_the_condition_number_of_every_block():
    """cond(N_s) <= C / delta + 1, down to one-frame blocks, whose N_s has rank S - 1 < C."""
    C, S, T = 8, 2, 6
    c = array_case(C, S, T, seed=5)
    scm, _, _ = mv.mvdr_reference(c["Y"], c["mask"], S, 1, 0, 0, LOADING)
    worst = float(np.max(noise_condition(scm, LOADING)))
    print("delta = 1e-3: worst cond %.6g, bound %.6g" % (worst, C / LOADING + 1))
    assert worst <= cond_bound(C, LOADING)
    assert float(np.max(noise_condition(scm, 1e-6))) > 1e6


@pytest.mark.parametrize("C,floor_db", [(4, 1.0), (2, 1.0)])
def test_beamforming_beats_masking_the_reference_channel(C, floor_db):
    S, T, Lb, ref = 2, 200, 200, 0
    c = array_case(C, S, T, seed=6)
    _, _, Z = mv.mvdr_reference(c["Y"], c["mask"], S, Lb, 0, ref, LOADING)
    target = c["a"][:, None, :, ref] * c["X"]                                    # (S, T, F)
    masked = np.transpose(c["mask"].reshape(T, S, F), (1, 0, 2)) * c["Y"][ref][None]
    e_bf, e_mask = np.sum(np.abs(Z - target) ** 2), np.sum(np.abs(masked - target) ** 2)
    gain = 10.0 * np.log10(e_mask / e_bf)
    print("C=%d: masked reference channel %.2f dB, beamformed %.2f dB below the target: gain %.2f dB"
          % (C, -10 * np.log10(e_mask / np.sum(np.abs(target) ** 2)), -10 * np.log10(e_bf / np.sum(np.abs(target) ** 2)), gain))
    assert gain >= floor_db


def test_arguments_out_of_range_are_refused():
    c = array_case(2, 2, 8, seed=7)
    for bad in (dict(S=1), dict(S=5), dict(Lb=0), dict(R=-1), dict(ref=2), dict(ref=-1), dict(loading=-1.0), dict(loading=float("nan"))):
        a = dict(S=2, Lb=4, R=0, ref=0, loading=LOADING)
        a.update(bad)
        with pytest.raises(ValueError, match="mvdr"):
            mv.mvdr_reference(c["Y"], c["mask"][:, :max(a["S"], 2) * F] if a["S"] <= 2 else np.zeros((8, a["S"] * F), np.float32),
                              a["S"], a["Lb"], a["R"], a["ref"], a["loading"])
    with pytest.raises(ValueError, match="channels"):
        mv.mvdr_reference(c["Y"][:1], c["mask"], 2, 4, 0, 0, LOADING)
