"""sk_cacgmm on the MI355X against sepkern/cacgmm.py's numpy definition, in two layouts of Y, prior and mask_out, with NaN in
everything the call must not read and a sentinel around everything it writes.

The gates are tests/_cacgmm_cases.py's (their derivation is in that file's docstring; tests/test_cacgmm.py turns them on mutants
of the definition):
posteriors   mask_out within 2^-23 gamma + 2^-149 of cacgmm_posteriors in numpy on the RETURNED B_out (on B_in for I = 0)
one step     with I = 1, from the identity and from the state the reference reaches in two iterations, B_out within
             2^-52 (Lw + 132 C^2 cond(B_in) + 40 max|l|) A of cacgmm_step on the same state
chaining     I = 3 in one call is bit for bit three calls of I = 1 chained through B_out -> B_in, and I = 0 on that B_out
             reproduces mask_out
Both layouts and two calls give the same bits; dead frames get float32(p), an all-dead window B_out = I exactly.
Measured on the MI355X (profiles/cacgmm.txt): from the identity B_out had the definition's bits in all 48 cases (the closed-form
pass: no substitution, log or exp is evaluated there -- the cases from two iterations hold that path); from two iterations it
was off by at most 1.3e-3 of its gate (C = 2; 6e-8 .. 1.5e-4 of it at C >= 4) -- a few units in the last place, from the device
library's log and exp -- and mask_out by at most 0.5 of its gate, the rounding to float32.  The last geometry, (230, 150, 40),
is the one with more than two of the kernel's 64-frame chunks in a window (190 frames) and in a block's output walk (150)."""
import ctypes as C_

import numpy as np
import pytest
import torch

from sepkern import cacgmm as cg
import _cacgmm_cases as cc
from _cacgmm_cases import CS, F, GEOMETRIES, ITERATIONS, LOADING, inputs

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch.device("cuda", 0)


def y_layout(Y, padded, dev, base=11, row_pad=6, chan_pad=13):
    """Y dense, or as a view into a NaN pool: a base pointer above the allocation start, rows of 257 + row_pad, channels
    chan_pad elements apart beyond their rows."""
    Y = torch.from_numpy(np.array(Y)).to(dev)
    if not padded:
        return Y
    Cn, T = Y.shape[0], Y.shape[1]
    rs = F + row_pad
    cs = T * rs + chan_pad
    pool = torch.full((base + Cn * cs,), complex(float("nan"), float("nan")), dtype=torch.complex64, device=dev)
    view = torch.as_strided(pool, (Cn, T, F), (cs, rs, 1), base)
    view.copy_(Y)
    return view


def prior_layout(prior, S, padded, dev):
    prior = torch.from_numpy(np.array(prior)).to(dev)
    if not padded:
        return prior
    T, ld = prior.shape[0], S * F + 5
    pool = torch.full((7 + T * ld,), float("nan"), dtype=torch.float32, device=dev)
    view = torch.as_strided(pool, (T, S * F), (ld, 1), 7)
    view.copy_(prior)
    return view


def run(Y, prior, S, I, Lb, Lc, loading, B_in, padded, dev):
    """The raw call in one layout; asserts that nothing but mask_out and B_out was written.  -> (mask, B) in numpy."""
    from sepkern import _lib
    lib = _lib.load()
    Cn, T = int(Y.shape[0]), int(Y.shape[1])
    nblk = -(-T // Lb)
    Yd, pd = y_layout(Y, padded, dev), prior_layout(prior, S, padded, dev)
    ldo = S * F + (9 if padded else 0)
    mpool = torch.full((GUARD + T * ldo + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    mask = torch.as_strided(mpool, (T, S * F), (ldo, 1), GUARD)
    mown = torch.zeros(mpool.shape, dtype=torch.bool, device=dev)
    torch.as_strided(mown, (T, S * F), (ldo, 1), GUARD).fill_(True)
    nB = nblk * S * F * Cn * Cn
    bpool = torch.full((GUARD + nB + GUARD,), complex(SENTINEL, SENTINEL), dtype=torch.complex128, device=dev)
    B = bpool[GUARD:GUARD + nB].view(nblk, S, F, Cn, Cn)
    Bi = None if B_in is None else torch.from_numpy(np.array(B_in)).to(dev)
    assert lib.sk_cacgmm_workspace_bytes(T, Cn, S, Lb, Lc) == cg.workspace_bytes(T, Cn, S, Lb, Lc) == 0
    p = lambda t: None if t is None else C_.c_void_p(t.data_ptr())
    _lib.call("sk_cacgmm", p(Yd), int(Yd.stride(0)), int(Yd.stride(1)), p(pd), int(pd.stride(0)), T, Cn, S, I, Lb, Lc, loading, p(Bi),
              p(mask), ldo, p(B), None, C_.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((mpool[~mown] == SENTINEL).all())
    g = torch.cat([bpool[:GUARD], bpool[-GUARD:]])
    assert bool((g.real == SENTINEL).all()) and bool((g.imag == SENTINEL).all())
    return mask.cpu().numpy(), B.cpu().numpy()


def kernel(dev, padded=False):
    return lambda Y, prior, S, I, Lb, Lc, loading, B_in: run(Y, prior, S, I, Lb, Lc, loading, B_in, padded, dev)


@pytest.mark.parametrize("I", ITERATIONS)
@pytest.mark.parametrize("gi", range(len(GEOMETRIES)))
@pytest.mark.parametrize("C,S", CS)
def test_posteriors_in_both_layouts(dev, C, S, gi, I):
    ok, ratio, mask, B = cc.gate_posteriors(kernel(dev), C, S, gi, I)
    print("  C=%d S=%d %s I=%d: mask_out off by %.3g of 2^-23 gamma + 2^-149" % (C, S, GEOMETRIES[gi], I, ratio))
    assert ok
    assert np.array_equal(B, np.conj(np.swapaxes(B, -1, -2)))                            # full Hermitian matrices
    T, Lb, Lc = GEOMETRIES[gi]
    Y, prior, _ = inputs(C, S, T)
    if I == 0:
        p = cg.prior_weights(prior, S, 0, T).reshape(T, S * F).astype(np.float32)
        assert mask.tobytes() == p.tobytes() and np.array_equal(B, np.broadcast_to(np.eye(C), B.shape))
    else:
        assert float(np.max(np.linalg.cond(B))) <= cc.cond_bound(C, LOADING)
    for _ in range(2):                                                                    # the layout changes no bit, nor does a second call
        mask2, B2 = run(Y, prior, S, I, Lb, Lc, LOADING, None, True, dev)
        assert mask2.tobytes() == mask.tobytes() and B2.tobytes() == B.tobytes()


@pytest.mark.parametrize("from_identity", [True, False])
@pytest.mark.parametrize("gi", range(len(GEOMETRIES)))
@pytest.mark.parametrize("C,S", CS)
def test_one_step_is_the_definitions(dev, C, S, gi, from_identity):
    """c1 = 132 and c2 = 40 are derived in tests/_cacgmm_cases.py."""
    ok, ratio = cc.gate_one_step(kernel(dev, padded=bool(gi % 2)), C, S, gi, from_identity)
    print("  C=%d S=%d %s from %s: B_out off by %.3g of 2^-52 (Lw + 132 C^2 cond + 40 max|l|) A"
          % (C, S, GEOMETRIES[gi], "the identity" if from_identity else "two iterations", ratio))
    assert ok
    if not from_identity:                                                                 # I = 0 is evaluated on B_in
        T, Lb, Lc = GEOMETRIES[gi]
        B_in = cc.two_iterations(C, S, T, Lb, Lc)
        ok, ratio, _, B = cc.gate_posteriors(kernel(dev), C, S, gi, 0, B_in=B_in)
        assert ok and B.tobytes() == cg.hermitian(np.array(B_in)).tobytes()


@pytest.mark.parametrize("gi", range(len(GEOMETRIES)))
@pytest.mark.parametrize("C,S", CS)
def test_three_iterations_are_three_chained_calls(dev, C, S, gi):
    assert cc.gate_chaining(kernel(dev, padded=bool(gi % 2)), C, S, gi)


def test_dead_frames_and_dead_windows(dev):
    C, S, T, Lb, Lc = 3, 2, 40, 8, 2
    Y, prior, _ = inputs(C, S, T)
    Yd = np.array(Y)
    dead = [3, 39] + list(range(12, 30))                      # block 2's window [14, 26) is all dead; blocks 1 and 3 see dead frames
    Yd[:, dead] = 0.0
    p = cg.prior_weights(prior, S, 0, T).reshape(T, S * F).astype(np.float32)
    got = None
    for neg in (False, True):
        if neg:
            Yd[1, 20, 5] = -0.0
            Yd[0, 3, 9] = complex(0.0, -0.0)
        mask, B = run(Yd, prior, S, 2, Lb, Lc, LOADING, None, neg, dev)
        assert mask[dead].tobytes() == p[dead].tobytes()
        assert np.array_equal(B[2], np.broadcast_to(np.eye(C), B[2].shape)) and not np.array_equal(B[0], B[2])
        gamma = cg.cacgmm_posteriors(Yd, prior, B, S, Lb)
        assert np.all(np.abs(mask - gamma) <= 2.0 ** -23 * gamma + 2.0 ** -149)
        mask_r, B_r, _ = cg.cacgmm_reference(Yd, prior, S, 2, Lb, Lc, LOADING)
        assert np.max(np.abs(B - B_r)) <= 1e-9 * np.max(np.abs(B_r))
        if got is not None:                                   # a -0.0 among the zeros changes nothing
            assert got[0].tobytes() == mask.tobytes() and got[1].tobytes() == B.tobytes()
        got = (mask, B)


BAD = [(dict(C=1), "C = 1"), (dict(C=9), "C = 9"), (dict(S=1), "S = 1"), (dict(S=5), "S = 5"), (dict(T=0), "T = 0"),
       (dict(I=-1), "iterations = -1"), (dict(I=17), "iterations = 17"), (dict(Lb=0), "block_frames = 0"),
       (dict(Lc=-1), "context_frames = -1"), (dict(Lb=4000, Lc=49), "4098"), (dict(loading=-1e-3), "loading"),
       (dict(loading=float("nan")), "loading"), (dict(ldp=2 * F - 1), "ld_prior"), (dict(ldo=2 * F - 1), "ld_out"),
       (dict(yrs=256), "y_row_stride"), (dict(Y=None), "null pointer"), (dict(prior=None), "null pointer"),
       (dict(mask=None), "null pointer")]


@pytest.mark.parametrize("bad,name", BAD)
def test_bad_arguments_are_refused_before_any_launch(dev, bad, name):
    """SK_EINVAL and a message that names the argument; the outputs keep their sentinel: nothing ran."""
    from sepkern import _lib
    lib = _lib.load()
    C, S, T = 3, 2, 20
    Y, prior, _ = inputs(C, S, T)
    Yd = torch.zeros(9, T, F, dtype=torch.complex64, device=dev)                                   # large enough for any bad shape
    Yd[:C] = torch.from_numpy(np.array(Y)).to(dev)
    pd = torch.full((T, 5 * F), 0.5, dtype=torch.float32, device=dev)
    mask = torch.full((T, 5 * F), SENTINEL, dtype=torch.float32, device=dev)
    B = torch.full((T, 5, F, 9, 9), complex(SENTINEL, 0.0), dtype=torch.complex128, device=dev)
    a = dict(C=C, S=S, T=T, I=2, Lb=8, Lc=1, loading=LOADING, yrs=F, ldp=5 * F, ldo=5 * F, Y=Yd, prior=pd, mask=mask)
    a.update(bad)
    p = lambda t: None if t is None else C_.c_void_p(t.data_ptr())
    rc = lib.sk_cacgmm(p(a["Y"]), T * F, a["yrs"], p(a["prior"]), a["ldp"], a["T"], a["C"], a["S"], a["I"], a["Lb"], a["Lc"],
                       a["loading"], None, p(a["mask"]), a["ldo"], p(B), None, C_.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -1                                                   # SK_EINVAL
    msg = lib.sk_last_error().decode()
    assert msg.startswith("sk_cacgmm: ") and name in msg, msg
    torch.cuda.synchronize()
    assert bool((mask == SENTINEL).all()) and bool((B.real == SENTINEL).all())


def test_the_wrapper_returns_what_the_call_writes_and_refuses_wrong_shapes(dev):
    from sepkern import ops, _lib
    C, S, (T, Lb, Lc) = 3, 3, GEOMETRIES[3]
    Y, prior, _ = inputs(C, S, T)
    Yd, pd = y_layout(Y, True, dev), prior_layout(prior, S, True, dev)
    B_in = cc.two_iterations(C, S, T, Lb, Lc)
    Bi = torch.from_numpy(np.array(B_in)).to(dev)
    mask, B = ops.cacgmm(Yd, pd, S, 2, Lb, Lc, LOADING, B_in=Bi, want_B=True)
    torch.cuda.synchronize()
    want = run(Y, prior, S, 2, Lb, Lc, LOADING, B_in, False, dev)
    assert mask.cpu().numpy().tobytes() == want[0].tobytes() and B.cpu().numpy().tobytes() == want[1].tobytes()
    out = torch.full((T + 2, S * F + 3), SENTINEL, dtype=torch.float32, device=dev)
    mask2, B2 = ops.cacgmm(Yd, pd, S, 2, Lb, Lc, LOADING, B_in=Bi, out=out)
    assert B2 is None and mask2.data_ptr() == out.data_ptr() and torch.equal(mask2, mask)
    assert bool((out[T:] == SENTINEL).all()) and bool((out[:, S * F:] == SENTINEL).all())
    with pytest.raises(_lib.SepkernError, match="Y must be"):
        ops.cacgmm(Yd.transpose(1, 2), pd, S, 2, Lb, Lc, LOADING)
    with pytest.raises(_lib.SepkernError, match="prior must be"):
        ops.cacgmm(Yd, pd[:, :S * F - 1], S, 2, Lb, Lc, LOADING)
    with pytest.raises(_lib.SepkernError, match="expected dtype"):
        ops.cacgmm(Yd, pd.double(), S, 2, Lb, Lc, LOADING)
    with pytest.raises(_lib.SepkernError, match="B_in must be"):
        ops.cacgmm(Yd, pd, S, 2, Lb, Lc, LOADING, B_in=Bi[:, :2])
    with pytest.raises(_lib.SepkernError, match="out must be"):
        ops.cacgmm(Yd, pd, S, 2, Lb, Lc, LOADING, out=out[:T - 1])
    with pytest.raises(_lib.SepkernError, match="cacgmm: iterations"):
        ops.cacgmm(Yd, pd, S, 17, Lb, Lc, LOADING)
    with pytest.raises(_lib.SepkernError, match="cacgmm: C = 9"):                      # refused before B is sized by it
        ops.cacgmm(torch.zeros(9, T, F, dtype=torch.complex64, device=dev), pd, S, 2, Lb, Lc, LOADING, want_B=True)
    with pytest.raises(_lib.SepkernError, match="cacgmm: block_frames"):
        ops.cacgmm(Yd, pd, S, 2, 0, Lc, LOADING)
