"""sk_wpe on the MI355X against sepkern/wpe.py's numpy definition, in two layouts of Y and X, with NaN in everything the call
must not read and a sentinel around everything it writes.

Inputs (tests/_wpe_cases.py): reverberant spectra per bin, loading 1e-3.  Each case first asserts, on the REFERENCE, that every
(block, bin) is an exact pass-through or has cond(R) <= D / delta + 1.
G_out: within I D 2^-52 cond_ref max|G| of the reference's G of that (block, bin): the forward error of an fp64 Cholesky
solve of a D x D system, once per iteration.  (At D = 1 that is one unit in the last place per iteration: the kernel performs
the definition's operations in the definition's order.)
X: within 2^-23 (|y| + sum_d |G[d][c]| |y~[d]|) per element of the fp64 apply of the RETURNED G_out: the rounding to complex64
(2^-24 per component) and an fp64 sum far below it.
Pass-through cells: exactly Y's bits and G = 0.  mag_out: within 2^-22 relative of |X[ref]| from the returned X.
Both layouts and two calls give the same bits."""
import ctypes as C_
import functools

import numpy as np
import pytest
import torch

from sepkern import wpe as wp
from _wpe_cases import LOADING, apply_filter, cond_bound, condition, reverb_case

pytestmark = pytest.mark.gpu

F = 257
SENTINEL = 12345.0
GUARD = 64

# (C, K): D = 1; one channel, the literature's taps; a 2 x 2 tile; D = 3, 4, 5 around the tile width; several tiles and a
# wave per workgroup; D = 70 and D = 80 on four waves
SMALL = [(1, 1), (1, 10), (2, 2), (3, 1), (1, 4), (1, 5), (3, 7)]
LARGE = [(7, 10), (8, 10)]
# (T, Lb, Lc): T < Lb; T = Lb; a last block of one frame; with a context; a context beyond the recording on either side;
# one-frame blocks; windows of more than two chunks of 64 frames
GEOMETRIES = [(9, 16, 0), (16, 16, 0), (33, 16, 0), (33, 16, 5), (40, 7, 100), (5, 1, 2), (150, 64, 40)]
LARGE_GEOMETRIES = [0, 1, 3]                                       # the D >= 70 cases: the numpy definition takes seconds there
DELAYS = [1, 3]
ITERATIONS = [1, 3]
# (C, K, T, Lb, Lc) where the kernel's loops branch.  The chunk is 256 frames at C <= 2, 128 at C <= 4, else 64: a second chunk
# of 44 frames at 256, in the window walk and the output walk; a second chunk of one frame and a last block of one frame;
# windows of 390 and 520 frames whose delayed past reaches across chunk boundaries; 128 frames plus one; exactly one chunk of
# 64; one chunk of 64 plus 6 frames; windows of 97 and 130 frames in chunks of 64 with a context; 54 tiles, the most one wave
# takes at C = 1, and 65 tiles, the fewest on four waves
PINS = [(1, 2, 300, 300, 0), (2, 2, 258, 257, 0), (2, 1, 520, 260, 130), (3, 2, 129, 129, 0), (6, 1, 64, 64, 0), (5, 1, 70, 70, 0),
        (5, 2, 130, 65, 32), (1, 36, 100, 80, 10), (1, 37, 100, 80, 10)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def inputs(C, T):
    Y = reverb_case(C, T, seed=100 * C + T)
    Y.setflags(write=False)
    return Y


@functools.lru_cache(maxsize=8)
def reference(C, K, T, Lb, Lc, delay, I, ref):
    """The numpy definition, computed once and shared (read-only)."""
    X, mag, G, d = wp.wpe_reference(inputs(C, T), K, delay, I, Lb, Lc, LOADING, ref=ref, details=True)
    cond = condition(d["R"], d["passed"])
    for a in (X, mag, G, cond, d["passed"]):
        a.setflags(write=False)
    return dict(X=X, mag=mag, G=G, passed=d["passed"], cond=cond)


def dense_layout(Y, dev):
    return torch.from_numpy(np.array(Y)).to(dev)


def padded_layout(Y, dev, base=11, row_pad=6, chan_pad=13):
    """Y as a view into a NaN pool: a base pointer above the allocation start, rows of 257 + row_pad, channels chan_pad
    elements apart beyond their rows."""
    Y = torch.from_numpy(np.array(Y)).to(dev)
    Cn, T = Y.shape[0], Y.shape[1]
    rs = F + row_pad
    cs = T * rs + chan_pad
    pool = torch.full((base + Cn * cs,), complex(float("nan"), float("nan")), dtype=torch.complex64, device=dev)
    view = torch.as_strided(pool, (Cn, T, F), (cs, rs, 1), base)
    view.copy_(Y)
    return view


def x_buffer(Cn, T, padded, dev):
    """-> (pool, view (C, T, 257), mask of the pool's elements the view covers)."""
    rs, pad, base = (F + 3, 7, GUARD + 5) if padded else (F, 0, GUARD)
    cs = T * rs + pad
    pool = torch.full((base + Cn * cs + GUARD,), complex(SENTINEL, SENTINEL), dtype=torch.complex64, device=dev)
    view = torch.as_strided(pool, (Cn, T, F), (cs, rs, 1), base)
    own = torch.zeros(pool.shape, dtype=torch.bool, device=dev)
    torch.as_strided(own, (Cn, T, F), (cs, rs, 1), base).fill_(True)
    return pool, view, own


def run(Y, K, delay, I, Lb, Lc, ref, padded, dev):
    from sepkern import _lib
    lib = _lib.load()
    Cn, T = int(Y.shape[0]), int(Y.shape[1])
    nblk, D = -(-T // Lb), Cn * K
    xpool, X, own = x_buffer(Cn, T, padded, dev)
    ldm = F + (9 if padded else 0)
    mpool = torch.full((GUARD + T * ldm + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    mag = torch.as_strided(mpool, (T, F), (ldm, 1), GUARD)
    mown = torch.zeros(mpool.shape, dtype=torch.bool, device=dev)
    torch.as_strided(mown, (T, F), (ldm, 1), GUARD).fill_(True)
    gpool = torch.full((GUARD + nblk * F * D * Cn + GUARD,), complex(SENTINEL, SENTINEL), dtype=torch.complex128, device=dev)
    G = gpool[GUARD:GUARD + nblk * F * D * Cn].view(nblk, F, D, Cn)
    assert lib.sk_wpe_workspace_bytes(T, Cn, K, Lb, Lc) == wp.workspace_bytes(T, Cn, K, Lb, Lc) == 0
    p = lambda t: C_.c_void_p(t.data_ptr())
    _lib.call("sk_wpe", p(Y), int(Y.stride(0)), int(Y.stride(1)), T, Cn, K, delay, I, Lb, Lc, ref, LOADING, p(X), int(X.stride(0)),
              int(X.stride(1)), p(mag), ldm, p(G), None, C_.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    # nothing but X, mag_out and G_out was written
    assert bool((xpool[~own].real == SENTINEL).all()) and bool((xpool[~own].imag == SENTINEL).all())
    assert bool((mpool[~mown] == SENTINEL).all())
    g = torch.cat([gpool[:GUARD], gpool[-GUARD:]])
    assert bool((g.real == SENTINEL).all()) and bool((g.imag == SENTINEL).all())
    return X.cpu().numpy(), mag.cpu().numpy(), G.cpu().numpy()


def check(Y, r, got, Cn, K, delay, I, Lb, ref, label):
    X, mag, G = got
    D, T = Cn * K, Y.shape[1]
    passed = r["passed"]
    # the reference's own conditioning, before anything is compared
    assert float(np.max(r["cond"])) <= cond_bound(D, LOADING), label
    assert np.all(r["G"][passed] == 0.0)
    # G_out
    assert G.shape == r["G"].shape and G.dtype == np.complex128 and np.isfinite(G.view(np.float64)).all()
    assert np.all(G[passed] == 0.0), label
    gmax = np.max(np.abs(r["G"]), axis=(-2, -1))
    gerr = np.max(np.abs(G - r["G"]), axis=(-2, -1))
    gate = I * D * 2.0 ** -52 * r["cond"] * gmax
    ratio = float(np.max(np.where(gate > 0, gerr / np.where(gate > 0, gate, 1.0), 0.0)))
    print("  %s: G off by %.3g of its gate (largest cond %.3g), %d cells passed through" % (label, ratio, float(np.max(r["cond"])), int(passed.sum())))
    assert np.all(gerr <= gate), "%s: G off by %.3g of the gate I D 2^-52 cond max|G|" % (label, ratio)
    # X: the fp64 apply of the returned G
    want, bound = apply_filter(Y, G, K, delay, Lb)
    blk = np.arange(T) // Lb
    pt = passed[blk]                                                            # (T, F)
    assert X.shape == (Cn, T, F) and X.dtype == np.complex64
    assert np.array_equal(np.ascontiguousarray(X[:, pt]).view(np.uint32), np.ascontiguousarray(Y[:, :, :F][:, pt]).view(np.uint32)), label
    xerr = np.abs(X.astype(np.complex128) - want)
    xrel = float(np.max(xerr / np.maximum(bound, 1e-300)))
    assert np.all(xerr <= 2.0 ** -23 * bound), "%s: X off by %.3g of |y| + sum |G| |y~|" % (label, xrel)
    # mag_out
    m64 = np.abs(X[ref].astype(np.complex128))
    assert mag.dtype == np.float32 and np.all(np.abs(mag - m64) <= 2.0 ** -22 * m64), label
    return ratio


def both_layouts(C, K, gi, delay, I, dev):
    T, Lb, Lc = GEOMETRIES[gi]
    layouts_at(C, K, T, Lb, Lc, (gi + K) % C, delay, I, dev)


def layouts_at(C, K, T, Lb, Lc, ref, delay, I, dev):
    Y = inputs(C, T)
    r = reference(C, K, T, Lb, Lc, delay, I, ref)
    label = "C=%d K=%d T=%d Lb=%d Lc=%d delay=%d I=%d ref=%d" % (C, K, T, Lb, Lc, delay, I, ref)
    dense = run(dense_layout(Y, dev), K, delay, I, Lb, Lc, ref, False, dev)
    padded = run(padded_layout(Y, dev), K, delay, I, Lb, Lc, ref, True, dev)
    check(Y, r, dense, C, K, delay, I, Lb, ref, label + " dense")
    check(Y, r, padded, C, K, delay, I, Lb, ref, label + " padded")
    for a, b in zip(dense, padded):                                             # the layout changes no bit
        assert a.tobytes() == b.tobytes()
    again = run(padded_layout(Y, dev), K, delay, I, Lb, Lc, ref, True, dev)     # nor does a second call
    assert all(a.tobytes() == b.tobytes() for a, b in zip(padded, again))


@pytest.mark.parametrize("I", ITERATIONS)
@pytest.mark.parametrize("delay", DELAYS)
@pytest.mark.parametrize("gi", range(len(GEOMETRIES)))
@pytest.mark.parametrize("C,K", SMALL)
def test_wpe_matches_the_definition_in_both_layouts(dev, C, K, gi, delay, I):
    both_layouts(C, K, gi, delay, I, dev)


@pytest.mark.parametrize("I", ITERATIONS)
@pytest.mark.parametrize("delay", DELAYS)
@pytest.mark.parametrize("gi", LARGE_GEOMETRIES)
@pytest.mark.parametrize("C,K", LARGE)
def test_wpe_matches_the_definition_at_seventy_and_eighty_unknowns(dev, C, K, gi, delay, I):
    both_layouts(C, K, gi, delay, I, dev)


@pytest.mark.parametrize("delay,I", [(1, 1), (3, 3)])
@pytest.mark.parametrize("C,K,T,Lb,Lc", PINS)
def test_wpe_matches_the_definition_at_its_chunk_and_thread_count_edges(dev, C, K, T, Lb, Lc, delay, I):
    layouts_at(C, K, T, Lb, Lc, (T + K) % C, delay, I, dev)


def test_silent_windows_and_a_delay_beyond_the_recording_pass_y_through(dev):
    C, K, T, Lb, Lc = 2, 3, 40, 8, 2
    Y = np.array(inputs(C, T))
    Y[:, :14] = 0.0                                                              # block 0's window [0, 10) and its past
    Y[1, 2, 9] = -0.0
    for delay, everywhere in ((1, False), (40, True)):
        Xr, magr, Gr, d = wp.wpe_reference(Y, K, delay, 2, Lb, Lc, LOADING, ref=1, details=True)
        assert d["passed"][0].all() and d["passed"].all() == everywhere
        X, mag, G = run(dense_layout(Y, dev), K, delay, 2, Lb, Lc, 1, False, dev)
        r = dict(X=Xr, mag=magr, G=Gr, passed=d["passed"], cond=condition(d["R"], d["passed"]))
        check(Y, r, (X, mag, G), C, K, delay, 2, Lb, 1, "pass-through delay=%d" % delay)
        assert np.array_equal(X[:, :8].view(np.uint32), Y[:, :8].view(np.uint32)) and np.all(G[0] == 0.0)
        assert np.array_equal(mag[:8].view(np.uint32), np.abs(Y[1, :8]).view(np.uint32))


BAD = [(dict(C=0), "C = 0"), (dict(C=9), "C = 9"), (dict(K=0), "taps = 0"), (dict(delay=0), "delay = 0"), (dict(K=27), "C * taps = 81"),
       (dict(I=0), "iterations = 0"), (dict(I=9), "iterations = 9"), (dict(T=0), "T = 0"), (dict(Lb=0), "block_frames = 0"),
       (dict(Lc=-1), "context_frames = -1"), (dict(Lb=4000, Lc=49), "4098"), (dict(ref=-1), "ref = -1"), (dict(ref=3), "ref = 3"),
       (dict(loading=-1e-3), "loading"), (dict(loading=float("nan")), "loading"), (dict(yrs=256), "y_row_stride"),
       (dict(xrs=256), "x_row_stride"), (dict(ldm=256), "ld_mag"), (dict(Y=None), "null pointer"), (dict(X=None), "null pointer")]


@pytest.mark.parametrize("bad,name", BAD)
def test_bad_arguments_are_refused_before_any_launch(dev, bad, name):
    """SK_EINVAL and a message that names the argument; the outputs keep their sentinel: nothing ran."""
    from sepkern import _lib
    lib = _lib.load()
    C, K, T = 3, 2, 20
    Y = dense_layout(inputs(C, T), dev)
    X = torch.full((9, T, F), complex(SENTINEL, SENTINEL), dtype=torch.complex64, device=dev)       # large enough for any bad shape
    mag = torch.full((T, F), SENTINEL, dtype=torch.float32, device=dev)
    G = torch.full((T, F, 81, 9), complex(SENTINEL, 0.0), dtype=torch.complex128, device=dev)
    a = dict(C=C, K=K, T=T, delay=2, I=2, Lb=8, Lc=1, ref=0, loading=LOADING, yrs=F, xrs=F, ldm=F, Y=Y, X=X)
    a.update(bad)
    p = lambda t: None if t is None else C_.c_void_p(t.data_ptr())
    rc = lib.sk_wpe(p(a["Y"]), T * F, a["yrs"], a["T"], a["C"], a["K"], a["delay"], a["I"], a["Lb"], a["Lc"], a["ref"], a["loading"],
                    p(a["X"]), T * F, a["xrs"], p(mag), a["ldm"], p(G), None, C_.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -1                                                   # SK_EINVAL
    msg = lib.sk_last_error().decode()
    assert msg.startswith("sk_wpe: ") and name in msg, msg
    torch.cuda.synchronize()
    assert bool((X.real == SENTINEL).all()) and bool((mag == SENTINEL).all()) and bool((G.real == SENTINEL).all())


def test_the_wrapper_returns_what_the_call_writes_and_refuses_wrong_shapes(dev):
    from sepkern import ops, _lib
    C, K, T, Lb, Lc = 3, 2, 33, 16, 5
    Y = dense_layout(inputs(C, T), dev)
    X, mag, G = ops.wpe(Y, K, 3, 3, Lb, Lc, LOADING, ref=2, want_mag=True, want_G=True)
    torch.cuda.synchronize()
    want = run(Y, K, 3, 3, Lb, Lc, 2, False, dev)
    for a, b in zip((X, mag, G), want):
        assert a.cpu().numpy().tobytes() == b.tobytes()
    X2, mag2, G2 = ops.wpe(Y, K, 3, 3, Lb, Lc, LOADING, ref=2)
    assert mag2 is None and G2 is None and torch.equal(torch.view_as_real(X2), torch.view_as_real(X))
    with pytest.raises(_lib.SepkernError, match="Y must be"):
        ops.wpe(Y.transpose(1, 2), K, 3, 3, Lb, Lc, LOADING)
    with pytest.raises(_lib.SepkernError, match="X must be"):
        ops.wpe(Y, K, 3, 3, Lb, Lc, LOADING, X=torch.zeros(C, T + 1, F, dtype=torch.complex64, device=dev))
    with pytest.raises(_lib.SepkernError, match="sk_wpe: iterations"):
        ops.wpe(Y, K, 3, 9, Lb, Lc, LOADING)
