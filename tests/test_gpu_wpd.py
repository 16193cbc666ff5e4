"""sk_wpd on the MI355X against sepkern/wpd.py's numpy definition, in two layouts of Y and mask, with NaN in everything the
call must not read and a sentinel around everything it writes.

Inputs (tests/_wpd_cases.py): S reverberant sources per bin and their ideal ratio masks, loading 1e-3, floor 1e-6 (1 in a few
cases).  Each case first asserts, on the REFERENCE, that every (block, stream, bin) falls back or has cond(R) <= D / delta + 1.
W_out, one iteration at a time -- iteration 1 without W_in, iteration 2 with the kernel's own W_out of iteration 1 as W_in on
both sides: with gG = D 2^-52 cond(R) max|G| (G, d and cond the reference's) |W - W_ref| <= (gG / d) (1 + C max|G[:, ref]| / d),
the forward error of an fp64 Cholesky solve of a D x D system carried through d and the division (_wpd_cases.w_gate).
Z: within 2^-23 sum_d |w_d| |y__d| per element of the fp64 apply of the RETURNED W_out: the rounding to complex64 (2^-24 per
component) and an fp64 sum far below it.  Cells that fall back: exactly Y[ref]'s bits and W = e_ref.
Both layouts and two calls give the same bits; one call of I iterations gives the bits of I chained calls."""
import ctypes as C_
import functools

import numpy as np
import pytest
import torch

from sepkern import wpd as wd
from _wpd_cases import FLOOR, LOADING, apply_filter, cond_bound, w_gate, wpd_case

pytestmark = pytest.mark.gpu

F = 257
SENTINEL = 12345.0
GUARD = 64

# (C, K): D = 2; D = 3, 4, 5 around the tile width (at C = 5 PHI has a second tile row); a full tile of PHI over two tile rows
# of R; C not a multiple of 4, with past; several tiles in one wave (22 of them)
SMALL = [(2, 0), (3, 0), (2, 1), (5, 0), (4, 1), (5, 1), (3, 7)]
# D = 70 and D = 80, four waves
LARGE = [(7, 9), (8, 9)]
# (T, Lb, Lc): T < Lb; T = Lb; a last block of one frame; with a context; a context beyond the recording on either side;
# one-frame blocks; windows of more than two chunks of 64 frames
GEOMETRIES = [(9, 16, 0), (16, 16, 0), (33, 16, 0), (33, 16, 5), (40, 7, 100), (5, 1, 2), (150, 64, 40)]
LARGE_GEOMETRIES = [0, 1, 3]                                       # the D >= 70 cases: the numpy definition takes seconds there
SWITCH = (6, 6)                                                    # D = 42: 70 tiles, the smallest D with four waves
# (C, K, T, Lb, Lc) for the chunk lengths the geometries above stay inside: a second chunk at 256 frames (C <= 2), and 128
# frames plus one (C <= 4) with a last block of one frame
PINS = [(2, 1, 300, 300, 0), (4, 1, 130, 129, 0)]
DELAYS = [1, 3]
RATIOS = {}                                                        # label -> largest |W - W_ref| / gate, for the report at the end


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def inputs(C, T, S, ref):
    c = wpd_case(C, T, S, seed=1000 * S + 100 * C + T, ref=ref)
    for a in c.values():
        a.setflags(write=False)
    return c["Y"], c["mask"]


def dense_layout(Y, mask, dev):
    return torch.from_numpy(np.array(Y)).to(dev), torch.from_numpy(np.array(mask)).to(dev)


def padded_layout(Y, mask, dev, base=11, row_pad=6, chan_pad=13, mbase=7, mpad=5):
    """Y and mask as views into NaN pools: base pointers above the allocation starts, rows of 257 + row_pad (S 257 + mpad),
    channels chan_pad elements apart beyond their rows."""
    Y, mask = torch.from_numpy(np.array(Y)).to(dev), torch.from_numpy(np.array(mask)).to(dev)
    Cn, T = Y.shape[0], Y.shape[1]
    rs = F + row_pad
    cs = T * rs + chan_pad
    pool = torch.full((base + Cn * cs,), complex(float("nan"), float("nan")), dtype=torch.complex64, device=dev)
    view = torch.as_strided(pool, (Cn, T, F), (cs, rs, 1), base)
    view.copy_(Y)
    ld = mask.shape[1] + mpad
    mpool = torch.full((mbase + T * ld,), float("nan"), dtype=torch.float32, device=dev)
    mview = torch.as_strided(mpool, (T, mask.shape[1]), (ld, 1), mbase)
    mview.copy_(mask)
    return view, mview


def run(Y, mask, S, K, delay, I, Lb, Lc, ref, floor, W_in, dev, want_W=True):
    """The raw call on device tensors -> (Z, W) as numpy arrays; W_in a numpy array or None."""
    from sepkern import _lib
    lib = _lib.load()
    Cn, T = int(Y.shape[0]), int(Y.shape[1])
    nblk, D = -(-T // Lb), Cn * (K + 1)
    zpool = torch.full((GUARD + S * T * F + GUARD,), complex(SENTINEL, SENTINEL), dtype=torch.complex64, device=dev)
    Z = zpool[GUARD:GUARD + S * T * F].view(S, T, F)
    wpool = torch.full((GUARD + nblk * S * F * D + GUARD,), complex(SENTINEL, SENTINEL), dtype=torch.complex128, device=dev)
    W = wpool[GUARD:GUARD + nblk * S * F * D].view(nblk, S, F, D)
    Win = None if W_in is None else torch.from_numpy(np.ascontiguousarray(W_in)).to(dev)
    assert lib.sk_wpd_workspace_bytes(T, Cn, S, K, Lb, Lc) == wd.workspace_bytes(T, Cn, S, K, Lb, Lc) == 0
    p = lambda t: None if t is None else C_.c_void_p(t.data_ptr())
    _lib.call("sk_wpd", p(Y), int(Y.stride(0)), int(Y.stride(1)), p(mask), int(mask.stride(0)), T, Cn, S, K, delay, I, Lb, Lc, ref,
              LOADING, floor, p(Win), p(Z), p(W) if want_W else None, None, C_.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    # nothing but Z and W_out was written
    for pool in (zpool, wpool):
        g = torch.cat([pool[:GUARD], pool[-GUARD:]])
        assert bool((g.real == SENTINEL).all()) and bool((g.imag == SENTINEL).all())
    if not want_W:
        assert bool((W.real == SENTINEL).all())
    return Z.cpu().numpy(), W.cpu().numpy()


def check(Y, mask, got, S, K, delay, Lb, Lc, ref, floor, W_in, label):
    """One iteration of the kernel against one iteration of the definition from the same W_in."""
    Z, W = got
    Cn, T = Y.shape[0], Y.shape[1]
    D = Cn * (K + 1)
    Zr, Wr, det = wd.wpd_reference(Y, mask, S, K, delay, 1, Lb, Lc, LOADING, floor, ref=ref, W_in=W_in, details=True)
    fb = det["fallback"]
    gate, cond = w_gate(det, Cn, ref)
    # the reference's own conditioning, before anything is compared
    assert float(np.max(cond)) <= cond_bound(D, LOADING), label
    e = np.zeros(D)
    e[ref] = 1.0
    assert np.all(Wr[fb] == e)
    # W_out
    assert W.shape == Wr.shape and W.dtype == np.complex128 and np.isfinite(W.view(np.float64)).all()
    assert np.all(W[fb] == e), label
    werr = np.max(np.abs(W - Wr), axis=-1)
    ratio = float(np.max(np.where(gate > 0, werr / np.where(gate > 0, gate, 1.0), 0.0)))
    exact = np.array_equal(W.view(np.uint64), Wr.view(np.uint64))
    print("  %s: W off by %.3g of its gate%s (largest cond %.3g), %d cells fell back"
          % (label, ratio, " (bit for bit)" if exact else "", float(np.max(cond)), int(fb.sum())))
    RATIOS[label] = ratio
    assert np.all(werr <= gate), "%s: W off by %.3g of the gate" % (label, ratio)
    # Z: the fp64 apply of the returned W
    want, bound = apply_filter(Y, W, K, delay, Lb)
    ft = np.transpose(fb[np.arange(T) // Lb], (1, 0, 2))                        # (S, T, F)
    assert Z.shape == (S, T, F) and Z.dtype == np.complex64
    yref = np.broadcast_to(Y[ref, :, :F], (S, T, F))
    assert np.array_equal(np.ascontiguousarray(Z[ft]).view(np.uint32), np.ascontiguousarray(yref[ft]).view(np.uint32)), label
    zerr = np.abs(Z.astype(np.complex128) - want)
    zrel = float(np.max(zerr / np.maximum(bound, 1e-300)))
    assert np.all(zerr <= 2.0 ** -23 * bound), "%s: Z off by %.3g of sum |w| |y_|" % (label, zrel)
    return fb


def both_layouts(C, K, gi, delay, S, floor, dev):
    T, Lb, Lc = GEOMETRIES[gi]
    layouts_at(C, K, T, Lb, Lc, (gi + K) % C, delay, S, floor, dev)


def layouts_at(C, K, T, Lb, Lc, ref, delay, S, floor, dev):
    Y, mask = inputs(C, T, S, ref)
    label = "C=%d K=%d S=%d T=%d Lb=%d Lc=%d delay=%d ref=%d floor=%g" % (C, K, S, T, Lb, Lc, delay, ref, floor)
    W_in = None
    for it in (1, 2):
        dense = run(*dense_layout(Y, mask, dev), S, K, delay, 1, Lb, Lc, ref, floor, W_in, dev)
        padded = run(*padded_layout(Y, mask, dev), S, K, delay, 1, Lb, Lc, ref, floor, W_in, dev)
        check(Y, mask, dense, S, K, delay, Lb, Lc, ref, floor, W_in, "%s iteration %d" % (label, it))
        for a, b in zip(dense, padded):                                          # the layout changes no bit
            assert a.tobytes() == b.tobytes()
        again = run(*padded_layout(Y, mask, dev), S, K, delay, 1, Lb, Lc, ref, floor, W_in, dev)   # nor does a second call
        assert all(a.tobytes() == b.tobytes() for a, b in zip(padded, again))
        W_in = dense[1]
    both = run(*dense_layout(Y, mask, dev), S, K, delay, 2, Lb, Lc, ref, floor, None, dev)         # one call of two iterations
    assert all(a.tobytes() == b.tobytes() for a, b in zip(both, dense))


@pytest.mark.parametrize("delay", DELAYS)
@pytest.mark.parametrize("gi", range(len(GEOMETRIES)))
@pytest.mark.parametrize("C,K", SMALL)
def test_wpd_matches_the_definition_in_both_layouts(dev, C, K, gi, delay):
    both_layouts(C, K, gi, delay, 2, FLOOR, dev)


@pytest.mark.parametrize("delay", DELAYS)
@pytest.mark.parametrize("gi", range(len(GEOMETRIES)))
def test_wpd_matches_the_definition_with_four_waves(dev, gi, delay):
    both_layouts(SWITCH[0], SWITCH[1], gi, delay, 2, FLOOR, dev)


@pytest.mark.parametrize("delay", DELAYS)
@pytest.mark.parametrize("gi", LARGE_GEOMETRIES)
@pytest.mark.parametrize("C,K", LARGE)
def test_wpd_matches_the_definition_at_seventy_and_eighty_unknowns(dev, C, K, gi, delay):
    both_layouts(C, K, gi, delay, 2, FLOOR, dev)


@pytest.mark.parametrize("delay", DELAYS)
@pytest.mark.parametrize("C,K,T,Lb,Lc", PINS)
def test_wpd_matches_the_definition_at_its_longer_chunks(dev, C, K, T, Lb, Lc, delay):
    layouts_at(C, K, T, Lb, Lc, (T + K) % C, delay, 2, FLOOR, dev)


@pytest.mark.parametrize("C,K,gi,S,floor", [(2, 1, 3, 4, FLOOR), (4, 1, 2, 4, FLOOR), (3, 0, 3, 3, 1.0), (5, 1, 4, 2, 1.0)])
def test_wpd_matches_the_definition_with_more_streams_and_a_floor_of_one(dev, C, K, gi, S, floor):
    both_layouts(C, K, gi, 3, S, floor, dev)


@pytest.mark.parametrize("I", [2, 3])
@pytest.mark.parametrize("C,K,gi", [(3, 7, 6), (5, 1, 3), (6, 6, 3)])
def test_iterations_in_one_call_are_one_iteration_calls_chained_bit_for_bit(dev, C, K, gi, I):
    T, Lb, Lc = GEOMETRIES[gi]
    Y, mask = inputs(C, T, 2, 0)
    Yd, md = dense_layout(Y, mask, dev)
    one = run(Yd, md, 2, K, 3, I, Lb, Lc, 0, FLOOR, None, dev)
    W = None
    for _ in range(I):
        chained = run(Yd, md, 2, K, 3, 1, Lb, Lc, 0, FLOOR, W, dev)
        W = chained[1]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, chained))
    Z, _ = run(Yd, md, 2, K, 3, I, Lb, Lc, 0, FLOOR, None, dev, want_W=False)   # W_out may be NULL
    assert Z.tobytes() == one[0].tobytes()


def test_silent_windows_and_silent_masks_fall_back_and_a_delay_beyond_the_recording_does_not(dev):
    C, K, T, Lb, Lc, S = 2, 3, 40, 8, 2, 2
    Y, mask = (np.array(a) for a in inputs(C, T, S, 1))
    Y[:, :14] = 0.0                                                              # block 0's window [0, 10) and beyond
    Y[1, 2, 9] = -0.0
    mask[14:28, F:] = 0.0                                                        # stream 1 over block 2's window [14, 26)
    for delay in (1, 40):
        W_in = None
        for it in (1, 2):
            got = run(*dense_layout(Y, mask, dev), S, K, delay, 1, Lb, Lc, 1, FLOOR, W_in, dev)
            fb = check(Y, mask, got, S, K, delay, Lb, Lc, 1, FLOOR, W_in, "fallbacks delay=%d iteration %d" % (delay, it))
            # what the reference says: the silent cells fall back, a delay beyond the recording alone does not
            assert fb[0].all() and fb[2, 1].all() and not fb[2, 0].any() and not fb[3:].any()
            assert np.array_equal(got[0][:, :8].view(np.uint32), np.stack([Y[1, :8]] * 2).view(np.uint32))
            if delay == 40:
                assert np.all(got[1][..., C:] == 0.0)                            # the past rows are zero: the present frame beamforms
            W_in = got[1]


BAD = [(dict(C=1), "C = 1"), (dict(C=9), "C = 9"), (dict(S=1), "S = 1"), (dict(S=5), "S = 5"), (dict(K=-1), "taps = -1"),
       (dict(delay=0), "delay = 0"), (dict(K=26), "C * (taps + 1) = 81"), (dict(I=0), "iterations = 0"), (dict(I=9), "iterations = 9"),
       (dict(T=0), "T = 0"), (dict(Lb=0), "block_frames = 0"), (dict(Lc=-1), "context_frames = -1"), (dict(Lb=4000, Lc=49), "4098"),
       (dict(ref=-1), "ref = -1"), (dict(ref=3), "ref = 3"), (dict(loading=-1e-3), "loading"), (dict(loading=float("nan")), "loading"),
       (dict(floor=0.0), "floor"), (dict(floor=1.5), "floor"), (dict(floor=float("nan")), "floor"), (dict(ldm=2 * F - 1), "ld_mask"),
       (dict(yrs=256), "y_row_stride"), (dict(Y=None), "null pointer"), (dict(mask=None), "null pointer"), (dict(Z=None), "null pointer")]


@pytest.mark.parametrize("bad,name", BAD)
def test_bad_arguments_are_refused_before_any_launch(dev, bad, name):
    """SK_EINVAL and a message that names the argument; the outputs keep their sentinel: nothing ran."""
    from sepkern import _lib
    lib = _lib.load()
    C, K, T, S = 3, 2, 20, 2
    Y, mask = dense_layout(*inputs(C, T, S, 0), dev)
    Z = torch.full((5, T, F), complex(SENTINEL, SENTINEL), dtype=torch.complex64, device=dev)       # large enough for any bad shape
    W = torch.full((T, 5, F, 81), complex(SENTINEL, 0.0), dtype=torch.complex128, device=dev)
    a = dict(C=C, S=S, K=K, T=T, delay=2, I=2, Lb=8, Lc=1, ref=0, loading=LOADING, floor=FLOOR, yrs=F, ldm=S * F, Y=Y, mask=mask, Z=Z)
    a.update(bad)
    p = lambda t: None if t is None else C_.c_void_p(t.data_ptr())
    rc = lib.sk_wpd(p(a["Y"]), T * F, a["yrs"], p(a["mask"]), a["ldm"], a["T"], a["C"], a["S"], a["K"], a["delay"], a["I"], a["Lb"], a["Lc"],
                    a["ref"], a["loading"], a["floor"], None, p(a["Z"]), p(W), None, C_.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -1                                                   # SK_EINVAL
    msg = lib.sk_last_error().decode()
    assert msg.startswith("sk_wpd: ") and name in msg, msg
    torch.cuda.synchronize()
    assert bool((Z.real == SENTINEL).all()) and bool((W.real == SENTINEL).all())


def test_the_wrapper_returns_what_the_call_writes_honours_buffers_and_refuses_wrong_shapes(dev):
    from sepkern import ops, _lib
    C, K, T, Lb, Lc, S = 3, 2, 33, 16, 5, 2
    Y, mask = dense_layout(*inputs(C, T, S, 2), dev)
    Z, W = ops.wpd(Y, mask, S, K, 3, 2, Lb, Lc, LOADING, FLOOR, ref=2, want_W=True)
    torch.cuda.synchronize()
    want = run(Y, mask, S, K, 3, 2, Lb, Lc, 2, FLOOR, None, dev)
    for a, b in zip((Z, W), want):
        assert a.cpu().numpy().tobytes() == b.tobytes()
    buf = torch.zeros(S, T, F, dtype=torch.complex64, device=dev)
    Z2, W2 = ops.wpd(Y, mask, S, K, 3, 2, Lb, Lc, LOADING, FLOOR, ref=2, Z=buf)
    assert W2 is None and Z2.data_ptr() == buf.data_ptr() and torch.equal(torch.view_as_real(buf), torch.view_as_real(Z))
    # a W of an earlier call continues it: one more iteration on both sides
    Z3, W3 = ops.wpd(Y, mask, S, K, 3, 1, Lb, Lc, LOADING, FLOOR, ref=2, W_in=W, want_W=True)
    want3 = run(Y, mask, S, K, 3, 3, Lb, Lc, 2, FLOOR, None, dev)
    assert Z3.cpu().numpy().tobytes() == want3[0].tobytes() and W3.cpu().numpy().tobytes() == want3[1].tobytes()
    with pytest.raises(_lib.SepkernError, match="Y must be"):
        ops.wpd(Y.transpose(1, 2), mask, S, K, 3, 2, Lb, Lc, LOADING, FLOOR)
    with pytest.raises(_lib.SepkernError, match="mask must be"):
        ops.wpd(Y, mask[:, :2 * F - 1], S, K, 3, 2, Lb, Lc, LOADING, FLOOR)
    with pytest.raises(_lib.SepkernError, match="Z must be"):
        ops.wpd(Y, mask, S, K, 3, 2, Lb, Lc, LOADING, FLOOR, Z=torch.zeros(S, T + 1, F, dtype=torch.complex64, device=dev))
    with pytest.raises(_lib.SepkernError, match="W_in must be"):
        ops.wpd(Y, mask, S, K, 3, 2, Lb, Lc, LOADING, FLOOR, W_in=W[:, :, :, :-1].contiguous())
    with pytest.raises(_lib.SepkernError, match="sk_wpd: iterations"):
        ops.wpd(Y, mask, S, K, 3, 9, Lb, Lc, LOADING, FLOOR)


def test_report_the_largest_ratio_of_this_run():
    """A reporter, not a check: check() has asserted the gate per case.  With -s it prints the largest |W - W_ref| / gate of the
    cases that ran before it in this process in one line (profiles/wpd.txt records it); run alone it has nothing to print."""
    if RATIOS:
        worst = max(RATIOS, key=RATIOS.get)
        print("  largest |W - W_ref| / gate over %d checks: %.3g (%s)" % (len(RATIOS), RATIOS[worst], worst))
