"""sepkern/stitch.py, the numpy definition of window stitching (no GPU): geometry, the known answer on permuted slices of
one global mask, and the blend's end points."""
import itertools

import numpy as np
import pytest

from sepkern import stitch as st
from _stitch_cases import expected_perms, permuted_slices

F = st.F


def legal_hops(W):
    return [Hn for Hn in range(1, W) if 2 * Hn >= W]


@pytest.mark.parametrize("W", [4, 7, 8, 9, 400])
def test_windows_cover_the_recording_and_every_boundary_shares_the_overlap(W):
    """For every legal Hn and T = 1 .. 4W: window k starts at k Hn, the windows cover [0, T) without a gap, every window but
    the last is full, and the last length lies in (O, W] -- so every boundary shares exactly O frames.  (With ONE window there
    is no boundary and its length is the recording's T <= W, which may be O or less: the interval is asserted wherever a second
    window exists, and T in [1, W] where not.)"""
    for Hn in legal_hops(W):
        O = W - Hn
        for T in range(1, 4 * W + 1):
            starts, lens = st.window_starts(T, W, Hn), st.window_lengths(T, W, Hn)
            K = len(starts)
            assert K == 1 + -(-max(T - W, 0) // Hn)
            assert starts == [k * Hn for k in range(K)]
            assert lens == [min(W, T - s0) for s0 in starts]
            assert all(n == W for n in lens[:-1])
            assert starts[-1] + lens[-1] == T                                  # the last window ends the recording
            assert all(starts[k + 1] <= starts[k] + lens[k] for k in range(K - 1))      # no gap
            if K >= 2:
                assert O < lens[-1] <= W
                for k in range(K - 1):                                         # exactly O shared frames, all inside window k + 1
                    assert starts[k] + lens[k] - starts[k + 1] == O and lens[k + 1] > O
                for k in range(K - 2):                                         # and no frame under three windows
                    assert starts[k] + lens[k] <= starts[k + 2]
            else:
                assert 1 <= lens[0] == T <= W


@pytest.mark.parametrize("args", [(0, 8, 4), (10, 8, 3), (10, 8, 8), (10, 9, 4), (10, 1, 1)])
def test_bad_geometry_is_refused(args):
    with pytest.raises(ValueError):
        st.window_starts(*args)


@pytest.mark.parametrize("S", [1, 2, 3, 4])
@pytest.mark.parametrize("W,Hn,T", [(8, 4, 13), (8, 4, 16), (9, 5, 24), (7, 6, 20), (4, 2, 41), (8, 4, 8), (8, 4, 5)])
def test_permuted_slices_of_one_mask_come_back_exactly(S, W, Hn, T):
    glob, X, windows, qs = permuted_slices(T, W, Hn, S, seed=100 * S + T)
    out, perms, cost = st.stitch_reference(X, windows, W, Hn, st.default_ramp(W - Hn))
    # stream s is output s of window 0 = global stream q_0[s], bit for bit (a == b in every overlap)
    assert out.dtype == np.float32 and np.array_equal(out, glob[:, qs[0], :].reshape(T, S * F))
    # PI_k(s) = the output of window k that holds global stream q_0[s]: the composition of the q_k
    assert perms.dtype == np.int32 and np.array_equal(perms, expected_perms(qs))
    assert cost.shape == (len(windows) - 1, S, S) and cost.dtype == np.float64
    for k in range(len(windows) - 1):               # the matching pairs cost exactly nothing, every other pair something
        for i in range(S):
            for j in range(S):
                assert (cost[k, i, j] == 0.0) == (qs[k][i] == qs[k + 1][j])


def test_one_window_is_a_copy():
    rng = np.random.default_rng(3)
    w = rng.uniform(0, 1, (5, 2 * F + 3)).astype(np.float32)          # padding columns are not part of the window
    out, perms, cost = st.stitch_reference(np.ones((5, F), np.float32), [w], 8, 4, st.default_ramp(4))
    assert np.array_equal(out, w[:, :2 * F]) and perms.tolist() == [[0, 1]] and cost.shape == (0, 2, 2)


def test_a_silent_overlap_gives_the_identity():
    """X = 0 on the shared frames: every cost is 0, the first permutation -- the identity -- wins, as the PIT kernels break ties."""
    S, W, Hn, T = 3, 8, 4, 20
    _, X, windows, _ = permuted_slices(T, W, Hn, S, seed=5)
    X[:] = 0.0
    _, perms, cost = st.stitch_reference(X, windows, W, Hn, st.default_ramp(W - Hn))
    assert not cost.any() and np.array_equal(perms, np.tile(np.arange(S, dtype=np.int32), (len(windows), 1)))


def test_best_permutation_takes_the_first_minimum_in_itertools_order():
    cost = np.array([[1.0, 1.0, 5.0], [1.0, 1.0, 5.0], [5.0, 5.0, 0.0]])
    p, totals = st.best_permutation(cost)
    assert p == (0, 1, 2) and len(totals) == 6 and totals[0] == totals[2] == 2.0       # (0,1,2) and (1,0,2) tie
    assert list(itertools.permutations(range(3)))[2] == (1, 0, 2)


@pytest.mark.parametrize("value", [0.0, 1.0])
def test_ramp_end_points_reproduce_the_earlier_and_the_later_window(value):
    """ramp = 0: a + 0 (b - a) = a, exactly.  ramp = 1: a + fl(b - a), which IS b wherever the difference is exact (Sterbenz:
    b/2 <= a <= 2b) and else within the two roundings, |out - b| <= 2^-24 (|b - a| + |b|) (1 + 2^-20)."""
    S, W, Hn, T = 2, 8, 5, 19
    _, X, windows, _ = permuted_slices(T, W, Hn, S, seed=9, noise=0.05)
    O = W - Hn
    out, perms, _ = st.stitch_reference(X, windows, W, Hn, np.full(O, value, np.float32))
    starts = st.window_starts(T, W, Hn)
    for k in range(1, len(windows)):
        src, row0 = (windows[k], 0) if value == 1.0 else (windows[k - 1], Hn)
        pk = perms[k] if value == 1.0 else perms[k - 1]
        want = np.concatenate([src[row0:row0 + O, p * F:(p + 1) * F] for p in pk], axis=1)
        got = out[starts[k]:starts[k] + O]
        if value == 0.0:
            assert np.array_equal(got, want)
            continue
        a = np.concatenate([windows[k - 1][Hn:Hn + O, p * F:(p + 1) * F] for p in perms[k - 1]], axis=1)
        exact = (a > 0) & (want > 0) & (want <= 2 * a) & (a <= 2 * want)
        assert exact.sum() > exact.size // 2 and np.array_equal(got[exact], want[exact])
        a64, b64 = a.astype(np.float64), want.astype(np.float64)
        assert np.all(np.abs(got.astype(np.float64) - b64) <= 2.0 ** -24 * (np.abs(b64 - a64) + np.abs(b64)) * (1 + 2.0 ** -20))


def test_the_blend_is_a_rounded_product_and_a_rounded_sum():
    """out = a + fl(ramp fl(b - a)) in float32: the value a fused multiply-add would give differs on these operands."""
    a, b, r = np.float32(0.016527635976672173), np.float32(0.8132702112197876), np.float32(0.91275554895401)
    X = np.ones((5, F), np.float32)
    w0 = np.full((4, F), a, np.float32)
    w1 = np.full((3, F), b, np.float32)
    out, _, _ = st.stitch_reference(X, [w0, w1], 4, 2, np.array([r, r], np.float32))
    want = np.float32(a + np.float32(r * np.float32(b - a)))
    assert out[2, 0] == want and out[3, 7] == want
    fused = np.float32(np.float64(a) + np.float64(r) * np.float64(np.float32(b - a)))
    assert fused != want, "choose operands on which the fused form rounds differently"


def test_memory_of_an_hour_at_two_speakers():
    """K W S 257 4 bytes stay resident: 1 124 windows of 400 frames for an hour (225 000 frames), 0.92 GB at S = 2."""
    assert len(st.window_starts(225000, 400, 200)) == 1124
    assert st.memory_bytes(225000, 400, 200, 2) == 1124 * 400 * 2 * 257 * 4 == 924377600
