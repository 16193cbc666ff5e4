"""sepkern/wpd.py, the numpy definition sk_wpd is held to: closed forms, invariances, locality, conditioning, chaining, and that
it separates and dereverberates -- on the CPU."""
import functools

import numpy as np
import pytest

from sepkern import mvdr as mv
from sepkern import wpd as wd
from sepkern import wpe as wp
from _wpd_cases import FLOOR, LOADING, apply_filter, cond_bound, condition, w_gate, wpd_case

F = wd.F
GATE_DB = 0.89                                                   # test_it_separates_and_dereverberates: half of the measured 1.79 dB


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype in (np.complex64, np.float32) else np.uint64)


@functools.lru_cache(maxsize=None)
def case(C, T, S, seed, ref=0):
    c = wpd_case(C, T, S, seed, ref)
    for a in c.values():
        a.setflags(write=False)
    return c


def test_no_taps_floor_one_one_iteration_is_the_mpdr_closed_form():
    """K = 0, phi = 1, I = 1: every weight is the same number, which w does not see: w = solve(sum y y^H + load, PHI)[:, ref] / tr
    with numpy.linalg, to the solve's forward error carried through d and the division (_wpd_cases.w_gate)."""
    C, T, S, ref = 4, 40, 2, 1
    c = case(C, T, S, 1, ref)
    _, W, det = wd.wpd_reference(c["Y"], c["mask"], S, 0, 1, 1, T, 0, LOADING, 1.0, ref=ref, details=True)
    assert W.shape == (1, S, F, C) and not det["fallback"].any()
    y = np.transpose(c["Y"], (1, 2, 0)).astype(np.complex128)                              # (T, F, C)
    R = np.einsum("tfa,tfb->fab", y, np.conj(y))
    R = R + LOADING * np.trace(R, axis1=1, axis2=2).real[:, None, None] / C * np.eye(C)
    gate, _ = w_gate(det, C, ref)
    for s in range(S):
        m = c["mask"][:, s * F:(s + 1) * F].astype(np.float64)
        Phi = np.einsum("tf,tfa,tfb->fab", m, y, np.conj(y))
        G = np.linalg.solve(R, Phi)
        want = G[:, :, ref] / np.trace(G, axis1=1, axis2=2).real[:, None]
        err = np.max(np.abs(W[0, s] - want), axis=-1)
        print("stream %d: W off by %.3g of its gate" % (s, np.max(err / gate[0, s])))
        assert np.all(err <= gate[0, s])


@pytest.mark.parametrize("taps", [0, 3])
def test_a_single_instantaneous_source_passes_with_its_gain_at_the_reference(taps):
    """y = a s(t) exactly (a's entries are powers of two times 1, i, -1 or -i, so complex64 holds the products), mask 1 for
    stream 0 and 0 for stream 1: PHI is rank one, so w^H [a; 0] = a_ref whatever R (Souden's form), to the W gate times sum |a|.
    Without taps that makes z_0(t) = a_ref s(t) = Y[ref]; with taps the past may still lower the output's power on a finite
    window, so only the constraint is checked.  Stream 1 has Re tr PHI == 0 and passes Y[ref]'s bits through."""
    C, T, S, ref = 3, 50, 2, 2
    rng = np.random.default_rng(2)
    a = (2.0 ** rng.integers(-2, 3, (C, 1, F))) * (1j ** rng.integers(0, 4, (C, 1, F)))
    env = 0.2 + np.abs(np.sin(np.arange(T)[:, None] * rng.uniform(0.2, 0.6, (1, F))))
    src = (env * (rng.standard_normal((T, F)) + 1j * rng.standard_normal((T, F)))).astype(np.complex64)
    Y = (a * src[None]).astype(np.complex64)
    assert np.array_equal(Y.astype(np.complex128), a * src[None].astype(np.complex128))
    mask = np.zeros((T, S * F), dtype=np.float32)
    mask[:, :F] = 1.0
    Z, W, det = wd.wpd_reference(Y, mask, S, taps, 2, 2, T, 0, LOADING, FLOOR, ref=ref, details=True)
    assert not det["fallback"][:, 0].any() and det["fallback"][:, 1].all()
    assert np.array_equal(bits(Z[1]), bits(Y[ref]))
    e = np.zeros(C * (taps + 1))
    e[ref] = 1.0
    assert np.all(W[:, 1] == e)
    gate, _ = w_gate(det, C, ref)                                                          # (1, S, F)
    got = np.einsum("fc,cf->f", np.conj(W[0, 0, :, :C]), a[:, 0])
    assert np.all(np.abs(got - a[ref, 0]) <= gate[0, 0] * np.sum(np.abs(a[:, 0]), axis=0))
    assert np.all(np.abs(W[0, 0, :, ref] - 1.0) > 1e-3)                                    # not e_ref: it spreads over the channels
    if taps == 0:
        bound = gate[0, 0][None] * np.sum(np.abs(Y), axis=0) + 2.0 ** -23 * np.abs(Y[ref])  # W's error, and complex64's rounding
        assert np.all(np.abs(Z[0].astype(np.complex128) - Y[ref].astype(np.complex128)) <= bound)


@pytest.mark.parametrize("k", [-9, 7])
def test_scaling_the_spectra_by_a_power_of_two_leaves_w_and_scales_z(k):
    c = case(3, 40, 2, 3)
    Z, W = wd.wpd_reference(c["Y"], c["mask"], 2, 2, 2, 3, 16, 4, LOADING, FLOOR)
    Zs, Ws = wd.wpd_reference(c["Y"] * np.float32(2.0 ** k), c["mask"], 2, 2, 2, 3, 16, 4, LOADING, FLOOR)
    assert np.array_equal(bits(Ws), bits(W)) and np.array_equal(bits(Zs), bits(Z * np.float32(2.0 ** k)))


def test_permuting_the_channels_with_the_reference_following_permutes_w():
    """One iteration, so that both runs solve the same system in exact arithmetic: the channels' order enters through the
    order of lambda's sum over c (a relative C 2^-52 of the weights, so of R: at most cond C 2^-52 max|G| of G, below gG as
    C <= D) and through the order of R's rows in the factorisation, which is the solve's own forward error.  Each W is
    therefore within its own w_gate of the exact filter (cond(R) is the same on both sides) and the two differ by at most the
    sum of the gates; Z by that times sum |y_|, plus the two roundings to complex64, 2^-23 sum |w| |y_|."""
    C, K, S, ref, delay, Lb, Lc = 3, 2, 2, 1, 2, 16, 4
    c = case(C, 40, S, 4, ref)
    Y = c["Y"]
    Z, W, det = wd.wpd_reference(Y, c["mask"], S, K, delay, 1, Lb, Lc, LOADING, FLOOR, ref=ref, details=True)
    cp = np.array([2, 0, 1])                                                               # new channel i is old channel cp[i]
    refp = int(np.where(cp == ref)[0][0])
    Zp, Wp, detp = wd.wpd_reference(Y[cp], c["mask"], S, K, delay, 1, Lb, Lc, LOADING, FLOOR, ref=refp, details=True)
    assert not det["fallback"].any() and not detp["fallback"].any()
    gate = w_gate(det, C, ref)[0] + w_gate(detp, C, refp)[0]                                # (nblk, S, F)
    idx = np.concatenate([b * C + cp for b in range(K + 1)])
    werr = np.max(np.abs(Wp - W[..., idx]), axis=-1)
    print("permuted W off by %.3g of the two gates" % np.max(werr / gate))
    assert np.all(werr <= gate)
    _, bound = apply_filter(Y, W, K, delay, Lb)                                             # sum |w| |y_|, (S, T, F)
    ysum = np.sum(np.abs(wd.stacked(Y, 0, Y.shape[1], K, delay)), axis=2)                   # (T, F)
    gt = np.transpose(gate[np.arange(Y.shape[1]) // Lb], (1, 0, 2))                         # (S, T, F)
    assert np.all(np.abs(Zp.astype(np.complex128) - Z) <= gt * ysum[None] + 2.0 ** -23 * bound)


def test_a_block_depends_on_its_window_the_past_before_it_and_its_own_mask_columns_only():
    T, Lb, Lc, K, delay, j, S, C = 60, 10, 5, 3, 2, 3, 3, 2
    c = case(C, T, S, 5)
    Y, mask = c["Y"], c["mask"]
    Z, W = wd.wpd_reference(Y, mask, S, K, delay, 2, Lb, Lc, LOADING, FLOOR)
    b0, b1, w0, w1 = wd.block_window(j, T, Lb, Lc)
    lo = w0 - delay - K + 1                                      # the earliest frame a stacked vector of the window reaches
    nan = np.complex64(complex(np.nan, np.nan))
    for s in range(S):
        Y2, m2 = Y.copy(), np.full_like(mask, np.nan)
        Y2[:, :lo] = nan
        Y2[:, w1:] = nan
        m2[w0:w1, s * F:(s + 1) * F] = mask[w0:w1, s * F:(s + 1) * F]
        r = wd.wpd_block(Y2, m2, j, s, K, delay, 2, Lb, Lc, 0, LOADING, FLOOR)
        assert np.array_equal(bits(r["Z"]), bits(Z[s, b0:b1])) and np.array_equal(bits(r["W"]), bits(W[j, s]))
    Y2 = Y.copy()
    Y2[0, lo, :] += np.complex64(1.0)                            # ... and that frame does count
    r = wd.wpd_block(Y2, mask, j, 0, K, delay, 2, Lb, Lc, 0, LOADING, FLOOR)
    assert not np.array_equal(bits(r["Z"]), bits(Z[0, b0:b1]))


@pytest.mark.parametrize("T", [1, 7, 8, 9, 25])
def test_every_block_geometry_and_truncation_after_a_window_changes_nothing(T):
    """T < Lb, T = Lb, a last block of one frame, and contexts that reach beyond the recording on both sides."""
    Lb, Lc, S = 8, 3, 2
    c = case(2, 25, S, 7)
    Y, mask = c["Y"][:, :T], c["mask"][:T]
    Z, W, det = wd.wpd_reference(Y, mask, S, 2, 1, 2, Lb, Lc, LOADING, FLOOR, details=True)
    nblk = wd.num_blocks(T, Lb)
    assert nblk == -(-T // Lb) and Z.shape == (S, T, F) and W.shape == (nblk, S, F, 6)
    assert Z.dtype == np.complex64 and W.dtype == np.complex128
    assert np.isfinite(Z.view(np.float32)).all() and np.isfinite(W.view(np.float64)).all() and not det["fallback"].any()
    for j in range(nblk):
        b0, b1, _, w1 = wd.block_window(j, T, Lb, Lc)
        Zc, Wc = wd.wpd_reference(Y[:, :w1], mask[:w1], S, 2, 1, 2, Lb, Lc, LOADING, FLOOR)
        assert np.array_equal(bits(Zc[:, b0:b1]), bits(Z[:, b0:b1])) and np.array_equal(bits(Wc[j]), bits(W[j]))


def test_the_loading_bounds_the_condition_number_on_windows_shorter_than_d():
    C, K = 4, 5                                                  # D = 24 on windows of 3 to 9 frames
    c = case(C, 20, 2, 8)
    _, _, det = wd.wpd_reference(c["Y"], c["mask"], 2, K, 1, 1, 3, 3, LOADING, FLOOR, details=True)
    cond = condition(det["R"], det["fallback"])
    print("largest cond(R) %.6g, bound %.6g" % (cond.max(), C * (K + 1) / LOADING + 1.0))
    assert not det["fallback"].any() and cond.max() <= cond_bound(C * (K + 1), LOADING) and cond.max() > 1e3


@pytest.mark.parametrize("floor", [FLOOR, 1.0])
def test_iterations_in_one_call_are_one_iteration_calls_chained_through_w(floor):
    c = case(3, 33, 2, 9)
    Z, W, det = wd.wpd_reference(c["Y"], c["mask"], 2, 2, 3, 3, 16, 5, LOADING, floor, ref=1, details=True)
    assert not det["fallback"].any()
    Wc = None
    for _ in range(3):
        Zc, Wc = wd.wpd_reference(c["Y"], c["mask"], 2, 2, 3, 1, 16, 5, LOADING, floor, ref=1, W_in=Wc)
    assert np.array_equal(bits(Wc), bits(W)) and np.array_equal(bits(Zc), bits(Z))


def test_silent_windows_and_silent_masks_fall_back_and_a_delay_beyond_the_recording_does_not():
    C, K, T, Lb, Lc, S = 2, 3, 40, 8, 2, 2
    c = case(C, T, S, 10)
    Y, mask = c["Y"].copy(), c["mask"].copy()
    Y[:, :14] = 0.0                                              # block 0's window [0, 10) and beyond
    Y[1, 2, 9] = -0.0
    mask[14:28, F:] = 0.0                                        # stream 1 over block 2's window [14, 26)
    Z, W, det = wd.wpd_reference(Y, mask, S, K, 1, 2, Lb, Lc, LOADING, FLOOR, ref=1, details=True)
    fb = det["fallback"]
    assert fb[0].all() and fb[2, 1].all() and not fb[2, 0].any() and not fb[3:].any()
    assert np.array_equal(bits(Z[:, :8]), bits(np.stack([Y[1, :8]] * 2))) and np.array_equal(bits(Z[1, 16:24]), bits(Y[1, 16:24]))
    e = np.zeros(C * (K + 1))
    e[1] = 1.0
    assert np.all(W[0] == e) and np.all(W[2, 1] == e)
    # a delay beyond the recording: the past rows are zero, the loading keeps R definite, the present frame beamforms
    _, W, det = wd.wpd_reference(c["Y"], c["mask"], S, K, T, 2, Lb, Lc, LOADING, FLOOR, details=True)
    assert not det["fallback"].any() and np.all(W[..., C:] == 0.0) and np.all(np.abs(W[..., :C]).sum(axis=-1) > 0.0)


@pytest.mark.parametrize("bad", [dict(C=1), dict(C=9), dict(S=1), dict(S=5), dict(taps=-1), dict(delay=0), dict(C=8, taps=10),
                                 dict(iterations=0), dict(iterations=9), dict(T=0), dict(block_frames=0), dict(context_frames=-1),
                                 dict(block_frames=4000, context_frames=49), dict(ref=2), dict(ref=-1), dict(loading=-1e-3),
                                 dict(loading=float("nan")), dict(floor=0.0), dict(floor=1.5), dict(floor=float("nan"))])
def test_arguments_out_of_range_are_refused(bad):
    a = dict(C=2, S=2, T=10, taps=3, delay=2, iterations=2, block_frames=5, context_frames=1, ref=0, loading=LOADING, floor=FLOOR)
    wd.check_arguments(**a)
    a.update(bad)
    with pytest.raises(ValueError, match="wpd"):
        wd.check_arguments(**a)
    assert wd.workspace_bytes(10, 2, 2, 3, 5, 1) == 0


def test_wrong_shapes_are_refused():
    c = case(2, 25, 2, 7)
    with pytest.raises(ValueError, match="Y must be"):
        wd.wpd_reference(c["Y"].astype(np.complex128), c["mask"], 2, 1, 1, 1, 8, 0, LOADING, FLOOR)
    with pytest.raises(ValueError, match="mask must be"):
        wd.wpd_reference(c["Y"], c["mask"][:, :2 * F - 1], 2, 1, 1, 1, 8, 0, LOADING, FLOOR)
    with pytest.raises(ValueError, match="W_in must be"):
        wd.wpd_reference(c["Y"], c["mask"], 2, 1, 1, 1, 8, 0, LOADING, FLOOR, W_in=np.zeros((4, 2, F, 3), dtype=np.complex128))


def sdr_db(est, target):
    return 10.0 * np.log10(np.sum(np.abs(target) ** 2) / np.sum(np.abs(est - target) ** 2))


def test_it_separates_and_dereverberates():
    """Two sources, C = 4, 250 frames (4 s), the ideal masks, the defaults (K = 5, delay 3, I = 2, floor 1e-6, loading 1e-3), one
    window.  Every output is scored in dB against the DIRECT image of its source at the reference channel, and the gate is the
    improvement on the masked reference channel, mask_s Y[ref].  Measured on the CPU (profiles/wpd.txt):
        source 0: masked reference channel 0.45 dB, WPD 2.24 dB (+1.79)
        source 1: masked reference channel 0.14 dB, WPD 2.15 dB (+2.02)
    The gate is half the smaller improvement in dB.  Recorded, not gated: wpe_reference (K = 5, delay 3, I = 2) -> mvdr_reference
    (one block, the same masks) on the same scene: 2.74 dB (+2.30) and 2.66 dB (+2.52).  The scene's filters decay by 0.7 per frame
    and no filter touches the first two frames after the direct one (the delay is 3), so every score stays low; on this scene
    the cascade scores half a dB above WPD."""
    C, T, S, ref = 4, 250, 2, 0
    c = wpd_case(C, T, S, seed=12, ref=ref)
    Y, mask = c["Y"], c["mask"]
    Z, _, det = wd.wpd_reference(Y, mask, S, 5, 3, 2, T, 0, LOADING, FLOOR, ref=ref, details=True)
    assert not det["fallback"].any()
    X, _, _ = wp.wpe_reference(Y, 5, 3, 2, T, 0, LOADING, ref=ref)
    _, _, Zc = mv.mvdr_reference(X, mask, S, T, 0, ref, LOADING)
    gains = []
    for s in range(S):
        masked = mask[:, s * F:(s + 1) * F] * Y[ref]
        base, got, casc = sdr_db(masked, c["direct"][s]), sdr_db(Z[s], c["direct"][s]), sdr_db(Zc[s], c["direct"][s])
        print("source %d: masked reference channel %.2f dB, WPD %.2f dB (+%.2f), WPE -> MVDR %.2f dB (+%.2f)"
              % (s, base, got, got - base, casc, casc - base))
        gains.append(got - base)
    assert min(gains) >= GATE_DB
