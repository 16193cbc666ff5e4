"""sepkern/wpe.py, the numpy definition sk_wpe is held to: closed forms, invariances, locality, conditioning, and that it
dereverberates -- on the CPU."""
import numpy as np
import pytest

from oracle import stft as OS
from sepkern import wpe as wp
from _wpe_cases import LOADING, cond_bound, condition, reverb_case

F = wp.F


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype in (np.complex64, np.float32) else np.uint64)


def test_one_channel_one_tap_one_iteration_is_the_closed_form():
    T, delay, delta = 30, 2, 1e-3
    Y = reverb_case(1, T, seed=1)
    _, _, G = wp.wpe_reference(Y, 1, delay, 1, T, 0, delta)
    y = Y[0].astype(np.complex128)
    lam = np.abs(y) ** 2
    lam = np.maximum(lam, 1e-10 * lam.max(axis=0))
    past = np.zeros_like(y)
    past[delay:] = y[:-delay]
    want = (past * np.conj(y) / lam).sum(axis=0) / ((1.0 + delta) * (np.abs(past) ** 2 / lam).sum(axis=0))
    assert G.shape == (1, F, 1, 1)
    assert np.all(np.abs(G[0, :, 0, 0] - want) <= 1e-12 * np.abs(want))


@pytest.mark.parametrize("k", [-9, 7])
def test_scaling_the_spectra_by_a_power_of_two_leaves_g_and_scales_x(k):
    Y = reverb_case(2, 40, seed=2)
    X, mag, G = wp.wpe_reference(Y, 3, 2, 3, 16, 4, LOADING)
    Xs, mags, Gs = wp.wpe_reference(Y * np.float32(2.0 ** k), 3, 2, 3, 16, 4, LOADING)
    assert np.array_equal(bits(Gs), bits(G))
    assert np.array_equal(bits(Xs), bits(X * np.float32(2.0 ** k))) and np.array_equal(bits(mags), bits(mag * np.float32(2.0 ** k)))


def test_a_delay_beyond_the_window_and_an_all_zero_window_pass_y_through():
    Y = reverb_case(2, 20, seed=3)
    X, mag, G, d = wp.wpe_reference(Y, 2, 20, 2, 8, 2, LOADING, ref=1, details=True)        # t - delay < 0 for every frame
    assert d["passed"].all() and np.array_equal(bits(X), bits(Y)) and np.all(G == 0.0)
    assert np.array_equal(bits(mag), bits(np.abs(Y[1])))
    Y = Y.copy()
    Y[:, :13] = 0.0                                              # block 0's window [0, 10) and its past are zero
    Y[0, 3, 5] = -0.0
    X, _, G, d = wp.wpe_reference(Y, 2, 1, 2, 8, 2, LOADING, details=True)
    assert d["passed"][0].all() and not d["passed"][2].any()
    assert np.array_equal(bits(X[:, :8]), bits(Y[:, :8])) and np.all(G[0] == 0.0) and np.any(G[2] != 0.0)
    assert not np.array_equal(bits(X[:, 16:]), bits(Y[:, 16:]))


def test_a_context_of_the_whole_recording_gives_one_filter():
    Y = reverb_case(2, 50, seed=4)
    _, _, G = wp.wpe_reference(Y, 2, 1, 2, 10, 50, LOADING)
    assert G.shape == (5, F, 4, 2)
    for j in range(1, 5):
        assert np.array_equal(bits(G[j]), bits(G[0]))
    _, _, G = wp.wpe_reference(Y, 2, 1, 2, 10, 10, LOADING)
    assert not np.array_equal(G[0], G[4])


def test_a_block_depends_on_its_window_and_the_taps_before_it_only():
    T, Lb, Lc, K, delay, j = 60, 10, 5, 3, 2, 3
    Y = reverb_case(2, T, seed=5)
    X, _, G = wp.wpe_reference(Y, K, delay, 2, Lb, Lc, LOADING)
    b0, b1, w0, w1 = wp.block_window(j, T, Lb, Lc)
    lo = w0 - delay - K + 1                                      # the earliest frame a stacked past of the window reaches
    rng = np.random.default_rng(0)
    Y2 = Y.copy()
    Y2[:, :lo] = (rng.standard_normal((2, lo, F)) + 1j * rng.standard_normal((2, lo, F))).astype(np.complex64)
    Y2[:, w1:] = 7.0
    X2, _, G2 = wp.wpe_reference(Y2, K, delay, 2, Lb, Lc, LOADING)
    assert np.array_equal(bits(X2[:, b0:b1]), bits(X[:, b0:b1])) and np.array_equal(bits(G2[j]), bits(G[j]))
    Y2 = Y.copy()
    Y2[0, lo, :] += np.complex64(1.0)                            # ... and that frame does count
    X3, _, _ = wp.wpe_reference(Y2, K, delay, 2, Lb, Lc, LOADING)
    assert not np.array_equal(bits(X3[:, b0:b1]), bits(X[:, b0:b1]))


def test_permuting_the_channels_permutes_x():
    """The channels' order enters through the order of lambda's sum (a relative C 2^-52) and the order of R's rows in the
    factorisation (cond D 2^-52 <= 1e-10 of the prediction): both far below complex64's 2^-24, so the two results are the same
    or neighbouring complex64 values."""
    Y = reverb_case(3, 40, seed=6)
    X, _, _ = wp.wpe_reference(Y, 3, 2, 3, 16, 4, LOADING)
    cp = np.array([2, 0, 1])
    Xp, _, _ = wp.wpe_reference(Y[cp], 3, 2, 3, 16, 4, LOADING)
    scale = np.max(np.abs(Y))
    assert np.all(np.abs(Xp.astype(np.complex128) - X[cp]) <= 2.0 ** -22 * np.abs(X[cp]) + 1e-9 * scale)


@pytest.mark.parametrize("T", [1, 7, 8, 9, 25])
def test_every_block_geometry_and_truncation_after_a_window_changes_nothing(T):
    Lb, Lc = 8, 3
    Y = reverb_case(2, 25, seed=7)[:, :T]
    X, mag, G, d = wp.wpe_reference(Y, 2, 1, 2, Lb, Lc, LOADING, details=True)
    nblk = wp.num_blocks(T, Lb)
    assert nblk == -(-T // Lb) and X.shape == (2, T, F) and mag.shape == (T, F) and G.shape == (nblk, F, 4, 2)
    assert X.dtype == np.complex64 and mag.dtype == np.float32 and G.dtype == np.complex128
    assert np.isfinite(X.view(np.float32)).all() and np.isfinite(G.view(np.float64)).all()
    assert d["passed"].all() == (T == 1)                         # one frame has no past
    for j in range(nblk):
        b0, b1, _, w1 = wp.block_window(j, T, Lb, Lc)
        Xc, _, Gc = wp.wpe_reference(Y[:, :w1], 2, 1, 2, Lb, Lc, LOADING)
        assert np.array_equal(bits(Xc[:, b0:b1]), bits(X[:, b0:b1])) and np.array_equal(bits(Gc[j]), bits(G[j]))


def test_the_loading_bounds_the_condition_number_on_windows_shorter_than_d():
    C, K = 4, 6                                                  # D = 24 on windows of 3 to 9 frames
    Y = reverb_case(C, 20, seed=8)
    _, _, _, d = wp.wpe_reference(Y, K, 1, 1, 3, 3, LOADING, details=True)
    cond = condition(d["R"], d["passed"])
    print("largest cond(R) %.6g, bound %.6g" % (cond.max(), C * K / LOADING + 1.0))
    assert not d["passed"].any() and cond.max() <= cond_bound(C * K, LOADING) and cond.max() > 1e3


@pytest.mark.parametrize("bad", [dict(C=0), dict(C=9), dict(taps=0), dict(delay=0), dict(C=8, taps=11), dict(iterations=0),
                                 dict(iterations=9), dict(T=0), dict(block_frames=0), dict(context_frames=-1),
                                 dict(block_frames=4000, context_frames=49), dict(ref=2), dict(ref=-1), dict(loading=-1e-3),
                                 dict(loading=float("nan"))])
def test_arguments_out_of_range_are_refused(bad):
    a = dict(C=2, T=10, taps=3, delay=2, iterations=2, block_frames=5, context_frames=1, ref=0, loading=LOADING)
    wp.check_arguments(**a)
    a.update(bad)
    with pytest.raises(ValueError, match="wpe"):
        wp.check_arguments(**a)
    assert wp.workspace_bytes(10, 2, 3, 5, 1) == 0


def reverberant_source(seed, seconds=4.0, rate=8000, rt=0.5, early=0.05, C=2):
    """Envelope-modulated noise through C exponentially decaying impulse responses of rt seconds (-60 dB at their end):
    -> (Y (C, T, F), Y_early (C, T, F)), the STFTs of the source through the whole responses and through their first `early`
    seconds."""
    rng = np.random.default_rng(seed)
    n = int(seconds * rate)
    t = np.arange(n) / rate
    env = np.clip(np.sin(2.0 * np.pi * 3.0 * t + rng.uniform(0.0, 6.0)) + 0.3 * np.sin(2.0 * np.pi * 7.1 * t), 0.0, None) ** 2
    s = env * rng.standard_normal(n)
    L, Le = int(rt * rate), int(early * rate)
    Y, E = [], []
    for c in range(C):
        h = rng.standard_normal(L) * 10.0 ** (-3.0 * np.arange(L) / L)
        h[0] = 1.0
        Y.append(OS.stft(np.convolve(s, h)[:n].astype(np.float32)).T)
        E.append(OS.stft(np.convolve(s, h[:Le])[:n].astype(np.float32)).T)
    return np.stack(Y).astype(np.complex64), np.stack(E).astype(np.complex64)


def test_it_dereverberates():
    """4 s of envelope-modulated noise, two channels, 0.5 s exponentially decaying responses, K = 10, delay = 3, I = 3,
    delta = 1e-3, one window.  || X - Y_early ||^2 against || Y - Y_early ||^2, Y_early being the source through the first
    50 ms of each response.  Measured on the CPU: the first is 3.56 dB below the
    second over seven bins, 4.70 dB over all 257.  The gate is 1 dB, as the
    beamforming check of tests/test_mvdr.py gates a gain it measures at several dB."""
    Y, E = reverberant_source(seed=11)
    T = Y.shape[1]
    X, _, _, d = wp.wpe_reference(Y, 10, 3, 3, T, 0, LOADING, details=True)
    assert not d["passed"].any()
    seven = np.array([16, 48, 80, 112, 144, 176, 208])
    def gain(sel):
        return 10.0 * np.log10(np.sum(np.abs(Y[:, :, sel] - E[:, :, sel]) ** 2) / np.sum(np.abs(X[:, :, sel] - E[:, :, sel]) ** 2))
    g7, gall = gain(seven), gain(np.arange(F))
    print("late reverberation reduced by %.2f dB over seven bins, %.2f dB over all bins" % (g7, gall))
    assert g7 >= 1.0 and gall >= 1.0
