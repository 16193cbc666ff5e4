"""sk_sisdr_pit_fwd, sk_mixit_fwd and sk_dynamic_mix on the MI355X at their loop edges (the pin suite of csrc/wave_loss.h, sisdr.hip,
mixit.hip and mix.hip; tests/test_gpu_sisdr.py, test_gpu_mixit.py and test_gpu_dynamic_mix.py hold the features).

Cases, claims, gates and defect models: tests/_wave_cases.py; tests/test_wave_cases.py proves on any machine that the cases reach
all 15 instantiations and every listed edge and that they catch the defects.

Every case goes through the C ABI (_lib.call) on buffers this file owns:
    the workspace of the two losses has exactly the queried size, holds 0xFF bytes (NaN as double) afresh before every launch --
        a finalize kernel that reads a chunk nobody wrote finds NaN, not an earlier call's sums -- and lies between two bands of
        0xA5 bytes that must be intact afterwards; the chunk slots past an utterance's own must still hold 0xFF;
    every output lies sentinel-filled between guard bands, and every element of it must have been written; the dynamic mix
        writes its signals in another order than the dense layout's with sentinels before, between and after them;
    the estimates are float32 buffers with NaN between the signals (sk_mask_istft_rows is not involved), at odd offsets.
Compared with the numpy fp64 definitions of the package at the gates in the header of tests/_wave_cases.py; every figure is
printed before it is asserted (profiles/wave_cases.txt records them).  Bit for bit: a second call, the float32 copy of an int16
reference, an utterance (a mixture) alone against inside its batch.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _wave_cases as WC
from sepkern import mixing

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
GUARD = 256                           # elements on either side of every output, bytes on either side of the workspace
GAP = 5                               # sentinels between two signals the dynamic mix writes


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib():
    from sepkern import _lib
    return _lib.load()


class Pool:
    """n elements of a device buffer between two guard bands, everything filled with `fill`."""

    def __init__(self, dev, n, dtype, fill):
        self.n, self.fill = int(n), fill
        self.whole = torch.full((self.n + 2 * GUARD,), fill, dtype=dtype, device=dev)
        self.data = self.whole[GUARD:GUARD + self.n]

    def ptr(self):
        return C.c_void_p(self.data.data_ptr())

    def numpy(self):
        return self.data.cpu().numpy()

    def guards_intact(self):
        w = self.whole.cpu()
        return bool((w[:GUARD] == self.fill).all()) and bool((w[GUARD + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.whole == self.fill).all())


class Workspace:
    """nbytes of 0xFF between two bands of 0xA5."""

    def __init__(self, dev, nbytes):
        self.n = int(nbytes)
        self.whole = torch.full((self.n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.whole[GUARD:GUARD + self.n] = 0xFF

    def ptr(self):
        return C.c_void_p(self.whole.data_ptr() + GUARD)

    def guards_intact(self):
        w = self.whole.cpu()
        return bool((w[:GUARD] == 0xA5).all()) and bool((w[GUARD + self.n:] == 0xA5).all())


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _nperm(S):
    return int(np.prod(np.arange(1, S + 1)))


# ------------------------------------------------------------------------------------------------ the two losses
def _loss_operands(c, dev, fmt):
    est = torch.from_numpy(c["est"]).to(dev)
    ref = torch.from_numpy(c["pcm"] if fmt == "int16" else c["ref32"]).to(dev)
    return est, ref


def _loss_buffers(c, dev, B):
    S = c["S"]
    if c["kind"] == "sisdr":
        return dict(pair=Pool(dev, B * S * S, torch.float32, SENTINEL), score=Pool(dev, _nperm(S) * B, torch.float32, SENTINEL),
                    best=Pool(dev, B, torch.int32, -7), out=Pool(dev, 3, torch.float32, SENTINEL), coef=Pool(dev, B * S * 3, torch.float32, SENTINEL))
    return dict(score=Pool(dev, (1 << S) * B, torch.float32, SENTINEL), best=Pool(dev, B, torch.int32, -7),
                out=Pool(dev, 3, torch.float32, SENTINEL), coef=Pool(dev, B * WC.NREF, torch.float32, SENTINEL))


def _loss_call(lib, c, ops, bufs, sel, count, ws, B=None, S=None, max_samples=None, tau=None, null=None):
    """The raw call on the utterances `sel`; B, S, max_samples, tau and null (the name of a pointer passed as NULL) override what
    the case says -- the bad-argument test's."""
    from sepkern import _lib
    est, ref = ops
    dev = est.device
    eo = torch.from_numpy(np.ascontiguousarray(c["est_offs"][sel]).reshape(-1)).to(dev)
    ro = torch.from_numpy(np.ascontiguousarray(c["ref_offs"][sel]).reshape(-1)).to(dev)
    ns = torch.from_numpy(np.ascontiguousarray(c["nsamp"][sel])).to(dev)
    cd = None if count is None else torch.full((1,), float(count), device=dev)
    a = dict(est=_p(est), est_offs=_p(eo), ref=_p(ref), ref_offs=_p(ro), nsamp=_p(ns), count_dev=_p(cd), ws=ws.ptr() if ws is not None else None,
             **{k: b.ptr() for k, b in bufs.items()})
    if null is not None:
        a[null] = None
    B = len(sel) if B is None else B
    S = c["S"] if S is None else S
    ms = c["max_samples"] if max_samples is None else max_samples
    pcm16 = int(ref.dtype == torch.int16)
    if c["kind"] == "sisdr":
        _lib.call("sk_sisdr_pit_fwd", a["est"], a["est_offs"], a["ref"], pcm16, a["ref_offs"], a["nsamp"], B, S, ms, a["count_dev"], a["pair"],
                  a["score"], a["best"], a["out"], a["coef"], a["ws"], None)
    else:
        _lib.call("sk_mixit_fwd", a["est"], a["est_offs"], a["ref"], pcm16, a["ref_offs"], a["nsamp"], B, S, ms, a["count_dev"],
                  float(c["tau"] if tau is None else tau), a["score"], a["best"], a["out"], a["coef"], a["ws"], None)
    torch.cuda.synchronize()


def _loss_run(lib, dev, c, ops, sel=None, count="case", want_partial=False):
    """One call on exactly sized, poisoned, guarded buffers -> the outputs as numpy arrays (float32 / int32 as stored); with
    want_partial also the head of the workspace, partial (B, nch, NQ) fp64, as the call left it."""
    sel = list(range(c["B"])) if sel is None else sel
    B, S = len(sel), c["S"]
    count = c["count"] if count == "case" else count
    query = lib.sk_sisdr_workspace_bytes if c["kind"] == "sisdr" else lib.sk_mixit_workspace_bytes
    nbytes = query(B, S, c["max_samples"])
    assert nbytes == WC.workspace_bytes(c["kind"], B, S, c["max_samples"]) > 0
    ws, bufs = Workspace(dev, nbytes), _loss_buffers(c, dev, B)
    _loss_call(lib, c, ops, bufs, sel, count, ws)
    assert ws.guards_intact(), "the call wrote outside the %d bytes the size query returned" % nbytes
    raw = {}
    for k, b in bufs.items():
        assert b.guards_intact(), k
        raw[k] = b.numpy()
        assert not (raw[k] == b.fill).any(), "%s: an element was not written" % k
    if want_partial:
        NQ = WC.nq_of(c["kind"], S)
        part = ws.whole[GUARD:GUARD + B * c["nch"] * NQ * 8].cpu().numpy().view(np.float64).reshape(B, c["nch"], NQ)
        return raw, part
    return raw


def _loss_got(c, raw, B):
    """The raw outputs in the shape WC.loss_ratios takes."""
    S = c["S"]
    score = raw["score"].astype(np.float64).reshape(-1, B)
    if c["kind"] == "sisdr":
        pair, coef = raw["pair"].astype(np.float64).reshape(B, S, S), raw["coef"].astype(np.float64).reshape(B, S, 3)
        utts = [dict(pair=pair[j], score=score[:, j], best=int(raw["best"][j]), coef=coef[j]) for j in range(B)]
    else:
        coef = raw["coef"].astype(np.float64).reshape(B, WC.NREF)
        utts = [dict(score=score[:, j], best=int(raw["best"][j]), coef=coef[j]) for j in range(B)]
    return dict(utts=utts, out=raw["out"].astype(np.float64))


def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in a)


def _solo_bits(c, raw, solo, j):
    """Utterance j's slice of the batch's outputs against the outputs of the call that held it alone."""
    B, S = c["B"], c["S"]
    v = lambda x: x.view(np.int32)                                                   # noqa: E731
    ok = np.array_equal(v(raw["score"]).reshape(-1, B)[:, j], v(solo["score"])) and raw["best"][j] == solo["best"][0]
    per = S * 3 if c["kind"] == "sisdr" else WC.NREF
    ok = ok and np.array_equal(v(raw["coef"]).reshape(B, per)[j], v(solo["coef"]))
    if c["kind"] == "sisdr":
        ok = ok and np.array_equal(v(raw["pair"]).reshape(B, S * S)[j], v(solo["pair"]))
    return bool(ok)


@pytest.mark.parametrize("name", WC.LOSS_CASES)
def test_loss_case_against_fp64(name, dev, lib):
    c, ref = WC.loss_case(name), WC.loss_reference(name)
    B = c["B"]
    ops16 = _loss_operands(c, dev, "int16")
    raw, part = _loss_run(lib, dev, c, ops16, want_partial=True)
    assert all(np.isfinite(raw[k]).all() for k in raw if k != "best")
    # the sums kernel wrote the chunks below ceil(L / CHUNK) of every utterance and no others: those still hold 0xFF
    for j in range(B):
        mych = WC.chunks_of(int(c["nsamp"][j]))
        assert mych < c["nch"] and np.isfinite(part[j, :mych]).all(), j
        assert (np.ascontiguousarray(part[j, mych:]).view(np.uint8) == 0xFF).all(), "utterance %d: a chunk past its own was written" % j
    ratios = WC.loss_ratios(name, _loss_got(c, raw, B))
    print("wave_cases %-24s B=%3d items=%5d: of the gate -- pair %s  score %.3f  coef %.3f  out %.3f; decisions %s; least margin %.2f dB"
          % (name, B, B * WC.nq_of(c["kind"], c["S"]), "%.3f" % ratios["pair"] if c["kind"] == "sisdr" else "  -  ", ratios["score"], ratios["coef"], ratios["out"],
             "all equal" if ratios["decisions"] == 0 else "DIFFER", min([w["gap"] for w in ref["utts"] if w["gap"] > 0] + [np.inf])))
    assert ratios["decisions"] == 0.0
    for j in range(B):                                                               # a tie goes to the first maximum
        tie = WC.expected_tie(c, j)
        if tie is not None:
            assert int(raw["best"][j]) == tie[0], (j, tie, int(raw["best"][j]))
            s = raw["score"].reshape(-1, B)[:, j]
            assert s[tie[0]] == s[tie[1]]
    assert max(ratios.values()) <= 1.0, ratios
    assert raw["out"][1] == np.float32(WC.count_of(c))
    # zero coefficients are exact zeros (their gate is 0 already; said once more where the branch is the case's point)
    for j, w in enumerate(ref["utts"]):
        zero = np.asarray(w["coef"]) == 0.0
        per = raw["coef"].reshape(B, -1)[j].reshape(zero.shape)
        assert not per[zero].any(), (j, per)
    # a second call on a freshly poisoned workspace, and the float32 copy of the references: the same bits
    assert _same_bits(raw, _loss_run(lib, dev, c, ops16)), "two calls differ"
    assert _same_bits(raw, _loss_run(lib, dev, c, _loss_operands(c, dev, "float32"))), "int16 and float32 references differ"
    # an utterance alone, with the batch's count: the bits it has inside the batch
    for j in sorted({0, int(np.argmax(c["nsamp"])), B - 1}):
        solo = _loss_run(lib, dev, c, ops16, sel=[j], count=WC.count_of(c))
        assert _solo_bits(c, raw, solo, j), "utterance %d alone differs from inside the batch of %d" % (j, B)


# ------------------------------------------------------------------------------------------------ the dynamic mix
def _mix_run(dev, c, dtype, quantize, which=None, gains=True):
    """The raw call on the mixtures `which`: signals written (mixture-major, sources last to first) with GAP sentinels around
    each -> ([(mixture, [sources], G)] as stored, float32)."""
    from sepkern import _lib
    which = list(range(c["B"])) if which is None else which
    B, S = len(which), c["S"]
    ns = [int(c["nsamp"][u]) for u in which]
    order = [(q, b) for b in range(B) for q in range(S, -1, -1)]
    out_offs, at = {}, GAP
    for q, b in order:
        out_offs[(q, b)] = at
        at += ns[b] + GAP
    buf = Pool(dev, at, torch.float32, SENTINEL)
    g = Pool(dev, S * B, torch.float32, SENTINEL)
    flat = torch.from_numpy(WC.mix_flat(c, dtype)).to(dev)
    d_in = torch.tensor([int(c["in_offs"][s, u]) for s in range(S) for u in which], dtype=torch.int64, device=dev)
    d_out = torch.tensor([out_offs[(q, b)] for q in range(S + 1) for b in range(B)], dtype=torch.int64, device=dev)
    d_ns = torch.tensor(ns, dtype=torch.int32, device=dev)
    d_amp = torch.tensor([float(c["amp"][s, u]) for s in range(S) for u in which], dtype=torch.float32, device=dev)
    d_peak = torch.tensor([float(c["peak"][u]) for u in which], dtype=torch.float32, device=dev)
    _lib.call("sk_dynamic_mix", _p(flat), int(dtype == "int16"), _p(d_in), _p(d_ns), B, S, _p(d_amp), _p(d_peak), int(quantize), buf.ptr(),
              _p(d_out), g.ptr() if gains else None, None)
    torch.cuda.synchronize()
    assert buf.guards_intact() and g.guards_intact()
    data, written = buf.numpy(), np.zeros(at, dtype=bool)
    for (q, b), o in out_offs.items():
        written[o:o + ns[b]] = True
    assert (data[~written] == np.float32(SENTINEL)).all(), "a sample outside the stated ranges was written"
    assert not (data[written] == np.float32(SENTINEL)).any() and (gains and not (g.numpy() == np.float32(SENTINEL)).any() or g.untouched())
    G = g.numpy().reshape(S, B)
    return [(data[out_offs[(0, b)]:out_offs[(0, b)] + ns[b]], [data[out_offs[(1 + s, b)]:out_offs[(1 + s, b)] + ns[b]] for s in range(S)], G[:, b])
            for b in range(B)]


def _mix_same(a, b):
    v = lambda x: np.ascontiguousarray(x).view(np.int32)                             # noqa: E731
    return all(np.array_equal(v(x[0]), v(y[0])) and all(np.array_equal(v(p), v(q)) for p, q in zip(x[1], y[1])) and np.array_equal(v(x[2]), v(y[2]))
               for x, y in zip(a, b))


@pytest.mark.parametrize("name", WC.MIX_CASES)
def test_mix_case_against_fp64(name, dev, lib):
    c = WC.mix_case(name)
    B, S = c["B"], c["S"]
    got = _mix_run(dev, c, c["dtype"], False)
    assert all(np.isfinite(m).all() and np.isfinite(G).all() and all(np.isfinite(s).all() for s in srcs) for m, srcs, G in got)
    as64 = [(m.astype(np.float64), [s.astype(np.float64) for s in srcs], G.astype(np.float64)) for m, srcs, G in got]
    ratios = WC.mix_ratios(name, as64)
    print("wave_cases %-24s %-32s B=%2d: of the gate -- gains %.3f  sources %.3f  mixture %.3f"
          % (name, WC.mix_instantiation(c), B, ratios["gains"], ratios["sources"], ratios["mixture"]))
    assert max(ratios.values()) <= 1.0, ratios
    for u, (m, srcs, G) in enumerate(got):                                           # the largest magnitude is the peak, or all is +0
        top = max(float(np.abs(x).max()) for x in [m] + srcs)
        if WC.mix_reference(name)[u][2].any():
            assert abs(top / float(c["peak"][u]) - 1.0) <= (S + 6) * WC.EPS24
        else:
            assert not G.any() and not any(x.any() or np.signbit(x).any() for x in [m] + srcs), "mixture %d: not +0 everywhere" % u
    # a second call, the other sample format, a call without gains: the same bits; a mixture alone: the bits it has in the batch
    assert _mix_same(got, _mix_run(dev, c, c["dtype"], False))
    assert _mix_same([(m, s, G * 0) for m, s, G in got], [(m, s, G * 0) for m, s, G in _mix_run(dev, c, c["dtype"], False, gains=False)])
    if c["flat"].dtype == np.int16:
        assert _mix_same(got, _mix_run(dev, c, "float32" if c["dtype"] == "int16" else "int16", False))
    for u in sorted({0, B - 1, int(np.argmax(c["nsamp"]))}):
        assert _mix_same([got[u]], _mix_run(dev, c, c["dtype"], False, which=[u])), u
    # quantize: mixing.quantize of the kernel's own unquantized result of the same arguments, bit for bit, gains unchanged
    quant = _mix_run(dev, c, c["dtype"], True)
    for (m, srcs, G), (qm, qs, qG) in zip(got, quant):
        for plain, q in zip([m] + srcs, [qm] + qs):
            want = mixing.quantize(plain)
            assert np.array_equal(q.astype(np.float64), want) and np.array_equal(np.signbit(q), np.signbit(want))
        assert np.array_equal(G.view(np.int32), qG.view(np.int32))
    if "clips_positive" in c["edges"]:                                               # +1 clips to 32767 / 32768, -1 is kept
        assert quant[0][0][700] == np.float32(32767.0 / 32768.0) and quant[1][0][700] == np.float32(-1.0)
        assert max(float(q.max()) for q in [quant[0][0]] + quant[0][1]) == 32767.0 / 32768.0
        assert min(float(q.min()) for q in [quant[1][0]] + quant[1][1]) == -1.0


# ------------------------------------------------------------------------------------------------ refused arguments
def _refused(lib, fn, what):
    from sepkern import _lib
    with pytest.raises(_lib.SepkernError) as e:
        fn()
    msg = str(e.value)
    assert "code %d" % WC.SK_EINVAL in msg and what in msg, (what, msg)
    return msg


@pytest.mark.parametrize("kind", ["sisdr", "mixit"])
def test_the_losses_refuse_bad_arguments_and_write_nothing(kind, dev, lib):
    c = WC.loss_case("%s_wrap_2_B%d" % (kind, WC.wrap_batch(kind, 2) - 1))
    ops = _loss_operands(c, dev, "int16")
    sel = list(range(c["B"]))
    who = "sk_sisdr_pit_fwd" if kind == "sisdr" else "sk_mixit_fwd"
    nbytes = WC.workspace_bytes(kind, c["B"], c["S"], c["max_samples"])

    def attempt(what, **kw):
        ws, bufs = Workspace(dev, nbytes), _loss_buffers(c, dev, c["B"])
        msg = _refused(lib, lambda: _loss_call(lib, c, ops, bufs, sel, None, ws, **kw), what)
        assert who in msg
        torch.cuda.synchronize()
        assert all(b.untouched() for b in bufs.values()) and ws.guards_intact() and bool((ws.whole[GUARD:GUARD + nbytes] == 0xFF).all())
    for S in ((0, 5, -1) if kind == "sisdr" else (1, 5, 0)):
        attempt("num_spk %d" % S if kind == "sisdr" else "%d estimates" % S, S=S)
    attempt("B = 0", B=0)
    attempt("B = 65536", B=65536)
    attempt("max_samples = 0", max_samples=0)
    for null in ("est", "est_offs", "ref", "ref_offs", "nsamp", "score", "best", "out", "coef", "ws") + (("pair",) if kind == "sisdr" else ()):
        attempt("null pointer", null=null)
    if kind == "mixit":
        for tau, text in ((-1e-9, "tau -1e-09"), (1.0 + 1e-9, "tau 1"), (float("nan"), "nan outside 0..1")):
            attempt(text, tau=tau)


def test_the_dynamic_mix_refuses_bad_arguments_and_writes_nothing(dev, lib):
    from sepkern import _lib
    c = WC.mix_case("mix_clip")
    B, S = c["B"], c["S"]
    flat = torch.from_numpy(c["flat"]).to(dev)
    d_in = torch.from_numpy(c["in_offs"].reshape(-1).copy()).to(dev)
    d_ns = torch.from_numpy(c["nsamp"]).to(dev)
    d_amp, d_peak = torch.from_numpy(c["amp"].reshape(-1).copy()).to(dev), torch.from_numpy(c["peak"]).to(dev)
    n = int(c["nsamp"].max())
    d_out = torch.tensor([(q * B + b) * n for q in range(S + 1) for b in range(B)], dtype=torch.int64, device=dev)

    def attempt(what, B=B, S=S, null=None):
        buf, g = Pool(dev, 3 * 2 * n, torch.float32, SENTINEL), Pool(dev, 16, torch.float32, SENTINEL)
        a = dict(flat=_p(flat), d_in=_p(d_in), d_ns=_p(d_ns), d_amp=_p(d_amp), d_peak=_p(d_peak), out=buf.ptr(), d_out=_p(d_out))
        if null:
            a[null] = None
        msg = _refused(lib, lambda: _lib.call("sk_dynamic_mix", a["flat"], 1, a["d_in"], a["d_ns"], B, S, a["d_amp"], a["d_peak"], 0, a["out"],
                                              a["d_out"], g.ptr(), None), what)
        assert "sk_dynamic_mix" in msg
        torch.cuda.synchronize()
        assert buf.untouched() and g.untouched()
    attempt("S = 0", S=0)
    attempt("S = 5", S=5)
    attempt("B = 0", B=0)
    attempt("B = 65536", B=65536)
    for null in ("flat", "d_in", "d_ns", "d_amp", "d_peak", "out", "d_out"):
        attempt("null pointer", null=null)


def test_the_size_queries_return_zero_for_what_they_refuse(lib):
    """(sk_dynamic_mix takes no workspace: these two are the family's size queries.)"""
    for fn, lo in ((lib.sk_sisdr_workspace_bytes, 1), (lib.sk_mixit_workspace_bytes, 2)):
        for bad in ((0, 2, 4096), (-3, 2, 4096), (8, lo - 1, 4096), (8, 5, 4096), (8, 2, 0), (8, 2, -1)):
            assert fn(*bad) == 0, bad
        assert fn(8, lo, 1) > 0 and fn(65535, 4, 1) > 0
    assert lib.sk_mixit_workspace_bytes(8, 1, 4096) == 0 < lib.sk_sisdr_workspace_bytes(8, 1, 4096)
