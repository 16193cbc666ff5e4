"""sk_mvdr on the MI355X against sepkern/mvdr.py's numpy definition, launch by launch: the context-summed covariance matrices
(scm_out) within 1e-10 of their trace, the weights within 2^-22 of the largest weight of their (block, s, f), Z within the
forward bound of a C-term complex fp32 dot product of the definition's apply step on the RETURNED weights -- in two layouts of
Y and the mask, with NaN in everything the call must not read and a sentinel around everything it writes.

Inputs (tests/_mvdr_cases.py): a synthetic array, ratio masks with noise, loading 1e-3.
scm: the terms of a diagonal entry are non-negative and a block has at most 4 096 frames here, so two fp64 summation orders
differ by at most L 2^-52 ~ 1e-12 of the trace; an off-diagonal entry is bounded by the trace.  The gate is 1e-10.
weights: the comparison means something only where the reference's own solve is well conditioned: each case first asserts, on
the REFERENCE, that every d is an exact fallback or greater than 1e-6 and that every cond(N_s) <= C / delta + 1; the fp64 solves
then differ by about cond C 2^-52 <= 1.5e-11, and both results are rounded to complex64 (2^-24 per component).
Z: |sum_c conj(W_c) Y_c - Z| <= (C + 3) 2^-23 sum_c |W_c| |Y_c|."""
import ctypes as C_
import functools

import numpy as np
import pytest
import torch

from sepkern import mvdr as mv
from _mvdr_cases import LOADING, array_case, cond_bound, noise_condition

pytestmark = pytest.mark.gpu

F = 257
SENTINEL = 12345.0
GUARD = 64        # complex64 elements of sentinel before and after each output

# (T, Lb): T < Lb; T = Lb; a last block of one frame; Lb a multiple of nothing inside the kernels (the apply launch walks 64
# frames per workgroup, bin 256 of the statistics launch takes frames 64 apart); one-frame blocks; blocks of more than two 64s
GEOMETRIES = [(9, 16), (16, 16), (33, 16), (130, 37), (5, 1), (200, 135)]
CHANNELS = [2, 3, 4, 7, 8]
STREAMS = [2, 3, 4]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def inputs(C, S, T, zero=None):
    c = array_case(C, S, T, seed=100 * C + 10 * S + T)
    if zero is not None:                                        # (stream, first frame, last frame + 1): a mask column block exactly zero
        s, t0, t1 = zero
        c["mask"] = c["mask"].copy()
        c["mask"][t0:t1, s * F:(s + 1) * F] = 0.0
    for a in c.values():
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def block_stats(C, S, T, Lb, zero=None):
    c = inputs(C, S, T, zero)
    A = mv.block_statistics(c["Y"], c["mask"], S, Lb)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def reference(C, S, T, Lb, R, ref, zero=None):
    """The numpy definition, computed once and shared (read-only): scm, weights, d (NaN = fallback), cond(N_s)."""
    scm = mv.context_sum(block_stats(C, S, T, Lb, zero), R)
    W, d = mv.mvdr_weights(scm, ref, LOADING)
    cond = noise_condition(scm, LOADING)
    for a in (scm, W, d, cond):
        a.setflags(write=False)
    return dict(scm=scm, W=W, d=d, cond=cond)


def dense_layout(c, dev):
    return torch.from_numpy(np.array(c["Y"])).to(dev), torch.from_numpy(np.array(c["mask"])).to(dev)


def padded_layout(c, S, dev, base=11, row_pad=6, chan_pad=13, mask_base=5, mask_pad=9):
    """Y as a view into a NaN pool: a base pointer above the allocation start, rows of 257 + row_pad, channels chan_pad elements
    apart beyond their rows; the mask likewise with ld = S F + mask_pad."""
    Y = torch.from_numpy(np.array(c["Y"])).to(dev)
    Cn, T = Y.shape[0], Y.shape[1]
    rs = F + row_pad
    cs = T * rs + chan_pad
    pool = torch.full((base + Cn * cs,), complex(float("nan"), float("nan")), dtype=torch.complex64, device=dev)
    view = torch.as_strided(pool, (Cn, T, F), (cs, rs, 1), base)
    view.copy_(Y)
    ld = S * F + mask_pad
    mpool = torch.full((mask_base + T * ld,), float("nan"), device=dev)
    mview = torch.as_strided(mpool, (T, S * F), (ld, 1), mask_base)
    mview.copy_(torch.from_numpy(np.array(c["mask"])).to(dev))
    return view, mview


def guarded(shape, dev):
    n = int(np.prod(shape))
    pool = torch.full((n + 2 * GUARD,), complex(SENTINEL, SENTINEL), dtype=torch.complex64, device=dev)
    return pool, pool[GUARD:GUARD + n].view(*shape)


def guards_intact(pool):
    g = torch.cat([pool[:GUARD], pool[-GUARD:]])
    return bool((g.real == SENTINEL).all()) and bool((g.imag == SENTINEL).all())


def run(Y, mask, S, Lb, R, ref, dev, loading=LOADING):
    from sepkern import ops, _lib
    Cn, T = int(Y.shape[0]), int(Y.shape[1])
    nblk = -(-T // Lb)
    wpool, w = guarded((nblk, S, F, Cn), dev)
    zpool, z = guarded((S, T, F), dev)
    nbytes = _lib.load().sk_mvdr_workspace_bytes(T, Cn, S, Lb)
    assert nbytes >= mv.workspace_bytes(T, Cn, S, Lb) > 0
    ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device=dev)
    _, _, scm = ops.mvdr(Y, mask, S, Lb, R, ref, loading, want_scm=True, weights=w, Z=z, ws=ws[:nbytes])
    torch.cuda.synchronize()
    assert guards_intact(wpool) and guards_intact(zpool) and bool((ws[nbytes:] == 0xA5).all())     # nothing else was written
    return scm.cpu().numpy(), w.cpu().numpy(), z.cpu().numpy()


def check(c, r, got, Cn, S, T, Lb, ref, label):
    scm, W, Z = got
    e_ref = np.zeros(Cn, dtype=np.complex64)
    e_ref[ref] = 1.0
    # the reference's own conditioning, before anything is compared
    d, fb = r["d"], np.isnan(r["d"])
    assert np.all(d[~fb] > 1e-6) and float(np.max(r["cond"])) <= cond_bound(Cn, LOADING)
    assert np.all(r["W"][fb] == e_ref)
    # launch 1 (and the context sum)
    tr = np.real(np.trace(r["scm"], axis1=-2, axis2=-1))
    assert scm.shape == r["scm"].shape and scm.dtype == np.complex128
    err = np.max(np.abs(scm - r["scm"]), axis=(-2, -1))
    rel = float(np.max(np.where(tr > 0, err / np.where(tr > 0, tr, 1.0), 0.0)))
    assert np.all(err <= 1e-10 * tr), "%s: scm off by %.3g of the trace" % (label, rel)
    # launch 2
    assert W.shape == r["W"].shape and W.dtype == np.complex64
    assert np.all(W[fb] == e_ref), label                                           # fallback cells exactly
    scale = np.max(np.abs(r["W"]), axis=-1)
    werr = np.max(np.abs(W.astype(np.complex128) - r["W"].astype(np.complex128)), axis=-1)
    wrel = float(np.max(werr / scale))
    assert np.all(werr <= 2.0 ** -22 * scale), "%s: weights off by %.3g of the largest" % (label, wrel)
    # launch 3, on the returned weights
    blk = np.arange(T) // Lb
    Y64, W64 = c["Y"].astype(np.complex128), W.astype(np.complex128)
    want = np.zeros((S, T, F), dtype=np.complex128)
    bound = np.zeros((S, T, F))
    for s in range(S):
        for ch in range(Cn):
            want[s] += np.conj(W64[blk, s, :, ch]) * Y64[ch]
            bound[s] += np.abs(W64[blk, s, :, ch]) * np.abs(Y64[ch])
    zerr = np.abs(Z.astype(np.complex128) - want)
    assert Z.shape == (S, T, F) and not np.isnan(Z.view(np.float32)).any()
    zrel = float(np.max(zerr / np.maximum(bound, 1e-300)))
    assert np.all(zerr <= (Cn + 3) * 2.0 ** -23 * bound), "%s: Z off by %.3g of sum |W| |Y|" % (label, zrel)
    print("  %s: scm %.2g of the trace, weights %.2g of the largest (2^-22 = 2.4e-7), Z %.2g of sum |W||Y| (bound %.2g), "
          "%d fallback cells" % (label, rel, wrel, zrel, (Cn + 3) * 2.0 ** -23, int(fb.sum())))


def contexts(C, S, T, Lb, gi):
    """(R, ref): every context -- none, one block, more than the recording holds -- with the reference channel alternating."""
    nblk = -(-T // Lb)
    refs = [0, C - 1]
    return [(0, refs[gi % 2]), (1, refs[(gi + 1) % 2]), (nblk + 5, refs[(gi + S) % 2])]


@pytest.mark.parametrize("S", STREAMS)
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("gi", range(len(GEOMETRIES)))
def test_mvdr_matches_the_definition_in_both_layouts(dev, gi, C, S):
    T, Lb = GEOMETRIES[gi]
    c = inputs(C, S, T)
    layouts = [dense_layout(c, dev), padded_layout(c, S, dev)]
    for R, ref in contexts(C, S, T, Lb, gi):
        r = reference(C, S, T, Lb, R, ref)
        results = [run(Y, m, S, Lb, R, ref, dev) for Y, m in layouts]
        for name, got in zip(("dense", "padded"), results):
            check(c, r, got, C, S, T, Lb, ref, "C=%d S=%d T=%d Lb=%d R=%d ref=%d %s" % (C, S, T, Lb, R, ref, name))
        for a, b in zip(results[0], results[1]):                                # the layout changes no bit
            assert a.tobytes() == b.tobytes()
        again = run(*layouts[1], S, Lb, R, ref, dev)                            # nor does a second call
        assert all(a.tobytes() == b.tobytes() for a, b in zip(results[1], again))


@pytest.mark.parametrize("R,silent_blocks", [(0, {1}), (1, set())])
def test_a_stream_silent_over_a_context_gets_the_reference_channel(dev, R, silent_blocks):
    C, S, T, Lb, ref = 4, 3, 40, 16, 3
    zero = (1, 16, 32)                                          # stream 1 exactly zero over block 1
    c = inputs(C, S, T, zero)
    r = reference(C, S, T, Lb, R, ref, zero)
    fb = np.isnan(r["d"])
    assert {j for j in range(3) if fb[j, 1].all()} == silent_blocks and not fb[:, 0].any() and not fb[:, 2].any()
    for name, (Y, m) in (("dense", dense_layout(c, dev)), ("padded", padded_layout(c, S, dev))):
        got = run(Y, m, S, Lb, R, ref, dev)
        check(c, r, got, C, S, T, Lb, ref, "fallback R=%d %s" % (R, name))
        if R == 0:                                              # the reference channel passed through, bit for bit
            assert np.array_equal(got[2][1, 16:32].view(np.uint32), c["Y"][ref, 16:32].view(np.uint32))
            assert np.all(got[0][1, 1] == 0.0)


def test_everything_silent_but_one_stream_is_a_fallback_everywhere(dev):
    """N_s == 0 for the one active stream, PHI_s == 0 for the others."""
    C, S, T, Lb = 3, 2, 20, 8
    c = inputs(C, S, T, (1, 0, T))
    r = reference(C, S, T, Lb, 1, 1, (1, 0, T))
    assert np.isnan(r["d"]).all()
    got = run(*dense_layout(c, dev), S, Lb, 1, 1, dev)
    check(c, r, got, C, S, T, Lb, 1, "all fallback")
    assert np.array_equal(got[2][0].view(np.uint32), c["Y"][1].view(np.uint32))


BAD = [(dict(C=1), "C = 1"), (dict(C=9), "C = 9"), (dict(S=1), "S = 1"), (dict(S=5), "S = 5"), (dict(T=0), "T = 0"),
       (dict(Lb=0), "block_frames = 0"), (dict(R=-1), "context_blocks = -1"), (dict(ref=-1), "ref = -1"), (dict(ref=3), "ref = 3"),
       (dict(loading=-1e-3), "loading"), (dict(loading=float("nan")), "loading"), (dict(ld=2 * F - 1), "ld_mask"),
       (dict(ws=None), "ws is NULL")]


@pytest.mark.parametrize("bad,name", BAD)
def test_bad_arguments_are_refused_before_any_launch(dev, bad, name):
    """SK_EINVAL and a message that names the argument; the outputs keep their sentinel: nothing ran."""
    from sepkern import _lib
    lib = _lib.load()
    C, S, T, Lb = 3, 2, 20, 8
    c = inputs(C, S, T)
    Y, mask = dense_layout(c, dev)
    a = dict(C=C, S=S, T=T, Lb=Lb, R=1, ref=0, loading=LOADING, ld=S * F,
             ws=torch.zeros(lib.sk_mvdr_workspace_bytes(T, C, S, Lb), dtype=torch.uint8, device=dev))
    a.update(bad)
    wpool, w = guarded((3, 4, F, 9), dev)                       # large enough for whatever the bad shape would make
    zpool, z = guarded((4, T, F), dev)
    scm = torch.full((3, 4, F, 9, 9), complex(SENTINEL, 0.0), dtype=torch.complex128, device=dev)
    p = lambda t: None if t is None else C_.c_void_p(t.data_ptr())
    rc = lib.sk_mvdr(p(Y), Y.stride(0), Y.stride(1), p(mask), a["ld"], a["T"], a["C"], a["S"], a["Lb"], a["R"], a["ref"], a["loading"],
                     p(w), p(z), p(scm), p(a["ws"]), C_.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -1                                                   # SK_EINVAL
    msg = lib.sk_last_error().decode()
    assert msg.startswith("sk_mvdr: ") and name in msg, msg
    torch.cuda.synchronize()
    assert bool((wpool.real == SENTINEL).all()) and bool((zpool.real == SENTINEL).all()) and bool((scm.real == SENTINEL).all())
    if set(bad) & {"C", "S", "T", "Lb"}:
        assert lib.sk_mvdr_workspace_bytes(a["T"], a["C"], a["S"], a["Lb"]) == 0


def test_the_wrapper_refuses_a_short_workspace_and_wrong_shapes(dev):
    from sepkern import ops, _lib
    C, S, T, Lb = 3, 2, 20, 8
    Y, mask = dense_layout(inputs(C, S, T), dev)
    with pytest.raises(_lib.SepkernError, match="workspace"):
        ops.mvdr(Y, mask, S, Lb, 1, 0, LOADING, ws=torch.zeros(8, dtype=torch.uint8, device=dev))
    with pytest.raises(_lib.SepkernError, match="mask must be"):
        ops.mvdr(Y, mask[:T - 1], S, Lb, 1, 0, LOADING)
    with pytest.raises(_lib.SepkernError, match="Y must be"):
        ops.mvdr(Y.transpose(1, 2), mask, S, Lb, 1, 0, LOADING)
    with pytest.raises(_lib.SepkernError, match="weights must be"):
        ops.mvdr(Y, mask, S, Lb, 1, 0, LOADING, Z=torch.zeros(S, T + 1, F, dtype=torch.complex64, device=dev))


def test_mask_istft_streams_is_mask_istft_per_stream(dev):
    """Descriptors only: stream s of ops.mask_istft_streams is ops.mask_istft_frames of spectrum s with mask block s."""
    from sepkern import ops
    S, T = 3, 21
    c = inputs(3, S, T)
    Z = torch.from_numpy(np.array(c["Y"])).to(dev)                              # any S spectra
    mask = torch.from_numpy(np.array(c["mask"])).to(dev)
    for m in (None, mask):
        wav, pcm = ops.mask_istft_streams(Z, m, S, want_pcm=True, want_float=True)
        assert tuple(wav.shape) == tuple(pcm.shape) == (S, 128 * (T - 1))
        for s in range(S):
            ms = None if m is None else m[:, s * F:(s + 1) * F].contiguous()
            rw, rp = ops.mask_istft_frames(Z[s].contiguous(), ms, 1, want_pcm=True, want_float=True)
            assert torch.equal(wav[s].view(torch.int32), rw[0].view(torch.int32)) and torch.equal(pcm[s], rp[0])
