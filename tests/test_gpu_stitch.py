"""sk_stitch on the MI355X against sepkern/stitch.py's numpy definition: perms equal, cost within 1e-10 relative, the stitched
mask bit for bit -- in two descriptor layouts, with NaN in everything the call must not read and a sentinel in everything it
must not write.

Inputs (tests/_stitch_cases.py): a float32 uniform(0, 1) global mask, a random output permutation per window, additive
0.05 uniform(-1, 1) noise, X = |N(0, 1)|.  The permutation choice is only comparable where the reference's own margin is wide:
each case asserts, on the REFERENCE's costs, that the second-best permutation's total is at least 10 times the best at every
boundary -- the GPU's fp64 summation order then cannot change the choice.
cost: the terms are non-negative and fewer than 2^17, so two fp64 summation orders differ by at most n 2^-53 ~ 1.5e-11 relative:
the gate is 1e-10."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from sepkern import stitch as st
from _stitch_cases import expected_perms, permuted_slices

pytestmark = pytest.mark.gpu

F = 257
CCH = 16          # mirrors csrc/stitch.hip's CCH: overlap frames per workgroup of the cost launch
FCH = 256         # mirrors csrc/stitch.hip's FCH: boundaries per round of the finish launch
SENTINEL = 12345.0

# (W, Hn, T)
SHAPES = [(8, 4, 8),            # K = 1, T = W
          (8, 4, 5),            # K = 1, T < W
          (8, 4, 13),           # last window O + 1 frames, the shortest possible
          (8, 4, 16),           # last window full, 2 Hn = W
          (9, 5, 24),
          (7, 6, 20),           # O = 1
          (4, 2, 132),          # K = 65: a chain longer than one wave
          (40, 20, 101),
          # overlaps of c - 1, c, c + 1 and 2c + 1 frames (c = CCH), three windows each, the last one short
          (2 * (CCH - 1), CCH - 1, 4 * (CCH - 1) - 4), (2 * CCH, CCH, 4 * CCH - 5), (2 * (CCH + 1), CCH + 1, 4 * (CCH + 1) - 6),
          (2 * (2 * CCH + 1), 2 * CCH + 1, 4 * (2 * CCH + 1) - 7),
          (4, 2, 2 * (FCH + 43) + 1)]       # K = 299: more boundaries than one round of the finish launch


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def case(S, W, Hn, T, noise=0.05):
    """Inputs and the numpy reference, computed once and shared (read-only)."""
    glob, X, windows, qs = permuted_slices(T, W, Hn, S, seed=1000 * S + 7 * T + W, noise=noise)
    ramp = st.default_ramp(W - Hn)
    out, perms, cost = st.stitch_reference(X, windows, W, Hn, ramp)
    for a in (glob, X, ramp, out, perms, cost) + tuple(windows):
        a.setflags(write=False)
    return dict(glob=glob, X=X, windows=windows, qs=qs, ramp=ramp, out=out, perms=perms, cost=cost)


def margin(cost):
    """second-best / best total over the S! permutations, the smallest over the boundaries (inf without a choice to make)."""
    worst = np.inf
    for c in cost:
        totals = sorted(st.best_permutation(c)[1])
        if len(totals) > 1:
            worst = min(worst, totals[1] / totals[0] if totals[0] > 0 else np.inf)
    return worst


def nan_mag(X, dev, pad=3):
    m = torch.full((X.shape[0], F + pad), float("nan"), device=dev)
    m[:, :F] = torch.from_numpy(X).to(dev)
    return m


def dense_layout(windows, dev):
    """Window-major dense: the windows' len_k x S F elements back to back in one buffer."""
    flat = torch.from_numpy(np.concatenate([w.reshape(-1) for w in windows])).to(dev)
    desc, at = [], 0
    for w in windows:
        desc.append((flat, at, w.shape[1]))
        at += w.size
    return desc


def packed_layout(windows, W, dev, pad=7, gap=5):
    """Uniform packed batches as the network writes them: batch rows (t, j) at t * B + j, leading dimension ld > S F, batches of
    different B, the last window in a batch of its own.  The batches lie in one pool in DESCENDING order, `gap` floats apart,
    so every batch after the first sits below the base pointer: its offsets are negative.  Padding columns, the rows past a
    short window's end and the gaps between the batches hold NaN."""
    SF = windows[0].shape[1]
    ld = SF + pad
    groups, k, sizes = [], 0, [3, 1, 2, 5]
    while k < len(windows) - 1:
        B = min(sizes[len(groups) % len(sizes)], len(windows) - 1 - k)
        groups.append(list(range(k, k + B)))
        k += B
    groups.append([len(windows) - 1])
    pool = torch.full((sum(W * len(ks) * ld + gap for ks in groups),), float("nan"), device=dev)
    desc, at = [None] * len(windows), pool.numel()
    for ks in groups:
        B = len(ks)
        at -= W * B * ld + gap
        buf = pool[at:at + W * B * ld].view(W * B, ld)
        for j, kk in enumerate(ks):
            w = torch.from_numpy(np.array(windows[kk])).to(dev)
            buf[j:j + B * w.shape[0]:B, :SF] = w
            desc[kk] = (buf, j * ld, B * ld)
    return desc


def run(c, desc, S, W, Hn, T, dev):
    from sepkern import ops
    out = torch.full((T + 3, S * F + 5), SENTINEL, device=dev)
    got, perms, cost = ops.stitch(nan_mag(c["X"], dev), desc, T, W, Hn, S, torch.from_numpy(c["ramp"]).to(dev), out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy(), perms.cpu().numpy(), cost.cpu().numpy()


@pytest.mark.parametrize("S", [1, 2, 3, 4])
@pytest.mark.parametrize("W,Hn,T", SHAPES)
def test_stitch_matches_the_definition_in_both_layouts(dev, S, W, Hn, T):
    c = case(S, W, Hn, T)
    K = len(c["windows"])
    m = margin(c["cost"])
    print("S=%d W=%d Hn=%d T=%d K=%d: second-best / best >= %.1f" % (S, W, Hn, T, K, m))
    assert m >= 10.0, "the reference's own margin is too narrow to compare permutation choices"
    assert np.array_equal(c["perms"], expected_perms(c["qs"]))       # (the noise does not change the reference's choice)
    results = [run(c, layout, S, W, Hn, T, dev) for layout in (dense_layout(c["windows"], dev), packed_layout(c["windows"], W, dev))]
    for out, perms, cost in results:
        assert perms.dtype == np.int32 and np.array_equal(perms, c["perms"])
        assert cost.shape == c["cost"].shape and cost.dtype == np.float64
        if K > 1:
            rel = np.max(np.abs(cost - c["cost"]) / c["cost"])
            print("  cost: max relative difference %.3g" % rel)
            assert rel <= 1e-10
        assert np.array_equal(out[:T, :S * F].view(np.uint32), c["out"].view(np.uint32))      # bit for bit; no NaN was read
        assert np.all(out[T:] == SENTINEL) and np.all(out[:, S * F:] == SENTINEL)              # nothing else was written
    for a, b in zip(results[0], results[1]):                                                    # the layout changes no bit
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("S", [1, 2, 3, 4])
@pytest.mark.parametrize("W,Hn,T", [(9, 5, 24), (4, 2, 132), (2 * CCH + 2, CCH + 1, 4 * CCH)])
def test_noise_free_slices_return_the_global_mask(dev, S, W, Hn, T):
    c = case(S, W, Hn, T, noise=0.0)
    out, perms, cost = run(c, packed_layout(c["windows"], W, dev), S, W, Hn, T, dev)
    want = c["glob"][:, c["qs"][0], :].reshape(T, S * F)
    assert np.array_equal(out[:T, :S * F].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(perms, expected_perms(c["qs"]))
    qs = c["qs"]
    for k in range(len(c["windows"]) - 1):           # matching outputs cost exactly nothing, every other pair something
        for i in range(S):
            for j in range(S):
                assert (cost[k, i, j] == 0.0) == (qs[k][i] == qs[k + 1][j])


def test_two_calls_give_the_same_bits(dev):
    S, W, Hn, T = 3, 40, 20, 101
    c = case(S, W, Hn, T)
    desc = packed_layout(c["windows"], W, dev)
    a, b = run(c, desc, S, W, Hn, T, dev), run(c, desc, S, W, Hn, T, dev)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_repeat_enqueues_the_same_result(dev):
    from sepkern import ops
    S, W, Hn, T = 2, 8, 4, 13
    c = case(S, W, Hn, T)
    out, perms, _ = ops.stitch(nan_mag(c["X"], dev), dense_layout(c["windows"], dev), T, W, Hn, S,
                               torch.from_numpy(c["ramp"]).to(dev), repeat=3)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), c["out"].view(np.uint32)) and np.array_equal(perms.cpu().numpy(), c["perms"])


@pytest.mark.parametrize("bad,name", [(dict(S=0), "S = 0"), (dict(S=5), "S = 5"), (dict(T=0), "T = 0"), (dict(Hn=8), "Hn = 8"),
                                      (dict(W=9, Hn=4), "Hn = 4"), (dict(ws=None), "ws is NULL")])
def test_bad_arguments_are_refused_before_any_launch(dev, bad, name):
    """SK_EINVAL and a message that names the argument; `out` keeps its sentinel: nothing ran."""
    from sepkern import _lib
    lib = _lib.load()
    S, W, Hn, T = 2, 8, 4, 13
    c = case(S, W, Hn, T)
    desc = dense_layout(c["windows"], dev)
    a = dict(S=S, W=W, Hn=Hn, T=T, ws=torch.zeros(lib.sk_stitch_workspace_bytes(T, W, Hn, S), dtype=torch.uint8, device=dev))
    a.update(bad)
    mag, ramp = nan_mag(c["X"], dev), torch.from_numpy(c["ramp"]).to(dev)
    d = torch.tensor([o for _, o, _ in desc] + [s for _, _, s in desc], dtype=torch.int64, device=dev)
    out = torch.full((T, S * F), SENTINEL, device=dev)
    perms = torch.full((len(desc), 4), -7, dtype=torch.int32, device=dev)
    cost = torch.zeros(len(desc), 4, 4, dtype=torch.float64, device=dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = lib.sk_stitch(p(mag), mag.stride(0), p(desc[0][0]), p(d), p(d[len(desc):]), a["T"], a["W"], a["Hn"], a["S"], p(ramp), p(out),
                       out.stride(0), p(perms), p(cost), p(a["ws"]), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -1                                                   # SK_EINVAL
    msg = lib.sk_last_error().decode()
    assert msg.startswith("sk_stitch: ") and name in msg, msg
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((perms == -7).all())
    if "ws" not in bad:
        assert lib.sk_stitch_workspace_bytes(a["T"], a["W"], a["Hn"], a["S"]) == 0


def test_the_wrapper_refuses_a_short_workspace_and_a_wrong_window_count(dev):
    from sepkern import ops, _lib
    S, W, Hn, T = 2, 8, 4, 13
    c = case(S, W, Hn, T)
    desc, mag, ramp = dense_layout(c["windows"], dev), nan_mag(c["X"], dev), torch.from_numpy(c["ramp"]).to(dev)
    with pytest.raises(_lib.SepkernError, match="workspace"):
        ops.stitch(mag, desc, T, W, Hn, S, ramp, ws=torch.zeros(8, dtype=torch.uint8, device=dev))
    with pytest.raises(_lib.SepkernError, match="windows"):
        ops.stitch(mag, desc[:-1], T, W, Hn, S, ramp)
