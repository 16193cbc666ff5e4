"""The recurrence kernels of csrc/lstm.hip at their unit-group, batch-group and K edges (cases and reference: tests/_lstm_cases.py).

Every call: the cached workspace is overwritten with 0xFF from byte 4 on (the library zeroes its control block itself; nothing
else may be relied on); every output is a view into a pool of sentinels (a NaN with a payload) with guard rows on both sides.
Asserted per call: sk_lstm_status is clean and sk_lstm_last_launch() is what the restated host code predicts (the case ran the
instantiation it claims); outputs are finite where defined, still the sentinel where they are nobody's to write (guards, gates /
c at padded positions, the bf16 twin's columns past 8H), zero at the padded positions of y and dgx; values meet the project's
gates against the fp64 reference (bf16: its bf16 twin).  The one-hot probes address the exchange image one k at a time.

Every run prints a line "lstm_cases: ..." with max err / (atol + rtol |ref|) per output (bf16 gradients: relative norm / 3e-3).
"""
import dataclasses
import time

import numpy as np
import pytest
import torch

import _lstm_cases as L

pytestmark = pytest.mark.gpu

SENT32, SENT16 = 0x7FC12345, 0x7FC1
FRONT, TAIL = 64, 256      # guard elements on both sides of every pool (FRONT keeps the 16-byte alignment the kernels ask for)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    from sepkern import ops as o
    if o.device_info()[0] != L.CUS:
        pytest.skip("the restated launch plans assume 256 CUs")
    return o


def report(*a):
    print("lstm_cases:", *a)


class Pool:
    """n elements between two guards, everything the sentinel."""

    def __init__(self, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        self.whole = torch.empty(FRONT + n + TAIL, dtype=dtype, device="cuda")
        self.ibits = self.whole.view(torch.int32 if dtype == torch.float32 else torch.int16)
        self.sent = SENT32 if dtype == torch.float32 else SENT16
        self.ibits.fill_(self.sent)
        self.t = self.whole[FRONT:FRONT + n].view(*shape)
        self.n = n

    def guards_ok(self):
        return bool((self.ibits[:FRONT] == self.sent).all()) and bool((self.ibits[FRONT + self.n:] == self.sent).all())

    def is_sentinel(self):
        return (self.ibits[FRONT:FRONT + self.n] == self.sent).view(*self.t.shape).cpu().numpy()


def filled(a):
    p = Pool(a.shape)
    p.t.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
    return p


class Lay:
    """Rows of the sequence tensors: zero-padded (T, B) or packed (row of (t, b) = offs[t] + b for t < lens[b])."""

    def __init__(self, lens, T, B, packed):
        lens = np.asarray(lens)
        self.T, self.B, self.packed = T, B, packed
        self.valid = np.arange(T)[:, None] < lens[None, :]
        if packed:
            offs = np.concatenate([[0], np.cumsum(self.valid.sum(1))]).astype(np.int32)
            self.rows, self.R = offs[:-1, None] + np.arange(B)[None, :], int(offs[-1])
            self.offs = torch.from_numpy(offs).cuda()
            self.exists = self.valid
        else:
            self.rows, self.R, self.offs = np.arange(T)[:, None] * B + np.arange(B)[None, :], T * B, None
            self.exists = np.ones((T, B), dtype=bool)
        self.lens = torch.from_numpy(lens.astype(np.int32)).cuda()

    def put(self, a):
        a = np.asarray(a, dtype=np.float32).reshape(self.T, self.B, -1)
        m = np.zeros((self.R, a.shape[2]), dtype=np.float32)
        m[self.rows[self.exists]] = a[self.exists]
        return filled(m)

    def take(self, what, pool, zero_padded, bad):
        """(T, B, C) float32 of an output pool; NaN where the output is undefined.  Appends to `bad` what breaks the rules."""
        m, s = pool.t.cpu().numpy(), pool.is_sentinel()
        if not pool.guards_ok():
            bad.append(what + ": guard rows written")
        out = np.full((self.T, self.B, m.shape[1]), np.nan, dtype=np.float32)
        out[self.valid] = m[self.rows[self.valid]]
        if not np.isfinite(out[self.valid]).all():
            bad.append(what + ": not finite where defined")
        if not self.packed and (~self.valid).any():
            pad = self.rows[~self.valid]
            if zero_padded and not (m[pad] == 0).all():
                bad.append(what + ": padded positions are not zero")
            if not zero_padded and not s[pad].all():
                bad.append(what + ": padded positions written")
        if zero_padded:
            out[~self.valid] = 0
        return out


def fresh_ws(ops, T, B, H):
    ws = ops.lstm_ws(T, B, H)
    ws[4:].fill_(0xFF)
    return ws


def after_call(ops, ws, want):
    ops.lstm_status(ws)
    n, q = ops.lstm_last_launch()
    assert (n,) + tuple(q) == want, ((n,) + tuple(q), want)


def run_forward(ops, case, lay, kind, inp, bad, want_gates=True, want_hn=True, want_cn=True):
    """One sk_lstm_fwd call; returns the pools and the outputs in the padded layout."""
    T, B, H = case.T, case.B, case.H
    gx, whh, h0, c0 = lay.put(inp["gx"].reshape(T, B, 8 * H)), filled(inp["whh"]), filled(inp["h0"]), filled(inp["c0"])
    y, gates, cs = Pool((lay.R, 2 * H)), Pool((lay.R, 8 * H)), Pool((lay.R, 2 * H))
    hn, cn = Pool((2, B, H)), Pool((2, B, H))
    ws = fresh_ws(ops, T, B, H)
    mode = case.mode("fwd", kind)
    ops.lstm_fwd(gx.t, whh.t, h0.t, c0.t, lay.lens, y.t, gates.t if want_gates else None, cs.t if want_gates else None,
                 hn.t if want_hn else None, cn.t if want_cn else None, T, B, H, mode, offs=lay.offs)
    after_call(ops, ws, L.predict("fwd", T, B, H, mode, lay.packed))
    out = dict(y=lay.take("y", y, True, bad))
    if want_gates:
        out["gates"] = lay.take("gates", gates, False, bad).reshape(T, B, 2, 4 * H)
        out["c"] = lay.take("c", cs, False, bad).reshape(T, B, 2, H)
    else:
        assert gates.is_sentinel().all() and cs.is_sentinel().all()
    for k, p, w in (("hn", hn, want_hn), ("cn", cn, want_cn)):
        if not p.guards_ok():
            bad.append(k + ": guards written")
        if w:
            out[k] = p.t.cpu().numpy()
            if not np.isfinite(out[k]).all():
                bad.append(k + ": not finite")
        else:
            assert p.is_sentinel().all()
    for k, p in (("gx", gx), ("whh", whh), ("h0", h0), ("c0", c0)):
        if not p.guards_ok():
            bad.append(k + ": guards of an input written")
    return dict(y=y, gates=gates, cs=cs), out


def run_backward(ops, case, lay, kind, inp, saved, bad, want_dh0=True, want_dc0=True, want_dbias=True, twin=True):
    """One sk_lstm_bwd call on the forward call's own gates / c."""
    T, B, H = case.T, case.B, case.H
    nbg = (B + 15) // 16
    dy, whh, c0 = lay.put(inp["dy"]), filled(inp["whh"]), filled(inp["c0"])
    dhn, dcn = filled(inp["dhn"]), filled(inp["dcn"])
    dgx, dh0, dc0, dbias = Pool((lay.R, 8 * H)), Pool((2, B, H)), Pool((2, B, H)), Pool((nbg, 2, 4 * H))
    ld = 8 * H + 8
    tw = Pool((lay.R, ld), torch.bfloat16) if twin else None
    ws = fresh_ws(ops, T, B, H)
    mode = case.mode("bwd", kind)
    ops.lstm_bwd(dy.t, whh.t, saved["gates"].t, saved["cs"].t, c0.t, lay.lens, dgx.t, dh0.t if want_dh0 else None,
                 dc0.t if want_dc0 else None, T, B, H, mode, dhn=dhn.t, dcn=dcn.t, dbias=dbias.t if want_dbias else None,
                 dgx_bf16=tw.t if twin else None, offs=lay.offs)
    after_call(ops, ws, L.predict("bwd", T, B, H, mode, lay.packed, want_dh0 or want_dc0))
    out = dict(dgx=lay.take("dgx", dgx, True, bad).reshape(T, B, 2, 4 * H))
    for k, p, w in (("dh0", dh0, want_dh0), ("dc0", dc0, want_dc0), ("dbias", dbias, want_dbias)):
        if not p.guards_ok():
            bad.append(k + ": guards written")
        if w:
            out[k] = p.t.cpu().numpy()
            if not np.isfinite(out[k]).all():
                bad.append(k + ": not finite")
        else:
            assert p.is_sentinel().all()
    if twin:
        s = tw.is_sentinel()
        if not tw.guards_ok() or not s[:, 8 * H:].all():
            bad.append("bf16 twin: columns past 8H or guards written")
        ex = np.unique(lay.rows[lay.exists])
        same = torch.equal(tw.t[:, :8 * H][torch.from_numpy(ex).cuda()], dgx.t[torch.from_numpy(ex).cuda()].bfloat16())
        if not same:
            bad.append("bf16 twin is not dgx rounded to bf16")
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    """Equal bit for bit where defined (NaN = undefined on both sides)."""
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(a)[~np.isnan(a)], bits(b)[~np.isnan(b)])


def run_case(ops, case, layout, kind):
    """Forward and (where the flavour has one) backward of one case; returns the outputs and the {output: measured / gate}."""
    inp = L.inputs(case)
    lay = Lay(case.lens, case.T, case.B, layout == "packed")
    bad = []
    saved, got = run_forward(ops, case, lay, kind, inp, bad)
    if case.backward:
        got.update(run_backward(ops, case, lay, kind, inp, saved, bad))
        got["dwhh"] = L.dwhh_from(got["dgx"], got["y"], inp["h0"], case.lens)
    assert not bad, bad
    ref = L.clean_reference(case, case.plan("fwd", kind)["persistent"])
    return got, L.score(case, got, ref)


RUNS = [(c, lay, k) for c in L.CASES for lay, k in c.runs()]


@pytest.mark.parametrize("case,layout,kind", RUNS, ids=["%s-%s-kind%d" % (c.name, lay, k) for c, lay, k in RUNS])
def test_value_cases(ops, case, layout, kind):
    t0 = time.time()
    got, s = run_case(ops, case, layout, kind)
    if case.flavour == "xl8":      # the XCD-local form: bit for bit the ordinary bf16 form
        plain, sp = run_case(ops, dataclasses.replace(case, flavour="bf16", name=case.name), layout, kind)
        assert L.predict("fwd", case.T, case.B, case.H, dataclasses.replace(case, flavour="bf16").mode("fwd", kind), False)[1] == L.K_FWD
        diff = [k for k in got if not same_bits(got[k], plain[k])]
        assert not diff, diff
    report("case %-24s %-6s kind %d  %s  %.2f s" % (case.name, layout, kind, " ".join("%s %.3f" % kv for kv in sorted(s.items())), time.time() - t0))
    over = {k: v for k, v in s.items() if not v <= 1.0}
    assert not over, over


OPT = L.Case("f32_T4_B20_H324_optional_pointers", "f32", 4, 20, 324, tuple(L.ragged(4, 20)))


@pytest.mark.parametrize("layout", ["padded", "packed"])
@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_optional_pointers(ops, direction, kind, layout):
    """Every reduced call's remaining outputs equal the full call's bit for bit."""
    inp = L.inputs(OPT)
    lay = Lay(OPT.lens, OPT.T, OPT.B, layout == "packed")
    bad = []
    saved, full = run_forward(ops, OPT, lay, kind, inp, bad)
    if direction == "fwd":
        for gates, hn, cn in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
            _, red = run_forward(ops, OPT, lay, kind, inp, bad, gates, hn, cn)
            diff = [k for k in red if not same_bits(red[k], full[k])]
            assert not diff, (gates, hn, cn, diff)
    else:
        fullb = run_backward(ops, OPT, lay, kind, inp, saved, bad)
        for dh0, dc0, dbias, twin in ((True, False, True, True), (False, True, True, False), (False, False, True, True), (True, True, False, False),
                                      (False, False, False, False)):
            red = run_backward(ops, OPT, lay, kind, inp, saved, bad, dh0, dc0, dbias, twin)
            diff = [k for k in red if not same_bits(red[k], fullb[k])]
            assert not diff, (dh0, dc0, dbias, diff)
    assert not bad, bad


# ------------------------------------------------------------------------------------ one-hot probes
@pytest.mark.parametrize("probe", L.PROBES, ids=lambda p: p.name)
def test_one_hot_probes(ops, probe):
    """Forward: the second step's stored gates are act(gx + h1[k] W_hh[:, k]) with h1[k] the kernel's own first-step output.
    Backward (no split3 form): the second step's dgx, dh0 and dc0 from the kernel's own first-step dgx -- four-term sums."""
    t0 = time.time()
    case, H, B, T = probe.case(), probe.H, probe.B, L.PROBE_T
    whh = L.probe_weights(H)
    lay = Lay(case.lens, T, B, False)
    worst = {}
    for kof in probe.kofs():
        bad = []
        rows = np.arange(B)
        gx = L.probe_fwd_inputs(H, B, kof)
        inp = dict(gx=gx, whh=whh, h0=np.zeros((2, B, H)), c0=np.zeros((2, B, H)))
        _, got = run_forward(ops, case, lay, probe.kind, inp, bad)
        first = np.stack([got["y"][0, :, :H], got["y"][1, :, H:]])                      # (2, B, H): y of the first processed step
        want_first = np.full((2, B, H), L.PROBE_H1 / (1.0 + np.exp(40.0)) * (1.0 + np.exp(-40.0)))
        want_first[np.arange(2)[:, None], rows[None, :], kof] = L.PROBE_H1
        worst["y1"] = max(worst.get("y1", 0), L.ratio(first, want_first, *L.TOL_F32["y"]))
        y_first = first[np.arange(2)[:, None], rows[None, :], kof]
        want = L.probe_fwd_expected(whh, gx, kof, y_first, probe.bf)
        second = np.stack([got["gates"][1, :, 0], got["gates"][0, :, 1]], 1)            # (B, 2, 4H)
        worst["gates2"] = max(worst.get("gates2", 0), L.ratio(second, want, 0.0, L.PROBE_ATOL))
        if case.backward:
            gates, cs, c0, dy = L.probe_bwd_inputs(H, B, kof)
            binp = dict(dy=dy, whh=whh, c0=c0, dhn=np.zeros((2, B, H)), dcn=np.zeros((2, B, H)))
            saved = dict(gates=lay.put(gates.reshape(T, B, 8 * H)), cs=lay.put(cs.reshape(T, B, 2 * H)))
            gb = run_backward(ops, case, lay, probe.kind, binp, saved, bad, twin=False)
            dfirst = np.stack([gb["dgx"][T - 1, :, 0], gb["dgx"][0, :, 1]], 1).reshape(B, 2, H, 4)
            open_ = dfirst[rows[:, None], np.arange(2)[None, :], kof.T]                # (B, 2, 4)
            others = dfirst.copy()
            others[rows[:, None], np.arange(2)[None, :], kof.T] = 0
            assert not others.any(), "the first step's dgx is non-zero away from the open unit"
            gsecond = np.stack([gb["dgx"][0, :, 0], gb["dgx"][T - 1, :, 1]], 1)
            d2, dh0, dc0 = L.probe_bwd_expected(whh, gates, cs, c0, kof, open_, probe.bf, dgx_second=gsecond)
            for k, g, w in (("dgx2", gsecond, d2), ("dh0", gb["dh0"], dh0), ("dc0", gb["dc0"], dc0)):
                worst[k] = max(worst.get(k, 0), L.ratio(g, w, *L.TOL_F32["dh0"]))
        assert not bad, bad
    report("probe %-24s %d runs  %s  %.2f s" % (probe.name, len(probe.kofs()), " ".join("%s %.3f" % kv for kv in sorted(worst.items())), time.time() - t0))
    over = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not over, over


@pytest.mark.parametrize("flavour,H", [("f32", 900), ("bf16", 324)])
def test_backward_probe_with_one_step(ops, flavour, H):
    """T = 1: the product for dh0 has no step before it -- dh0 is the four-term sum itself."""
    B, T = 32, 1
    case = L.Case("probe_T1", flavour, T, B, H, (1,) * B)
    p = case.plan("bwd", 1)
    kof = L.probe_assignment(H, B, L.probe_ks(H, p["KS"], case.bf))[0]
    whh = L.probe_weights(H)
    lay = Lay(case.lens, T, B, False)
    gates, cs, c0, dy = L.probe_bwd_inputs(H, B, kof, T)
    bad = []
    saved = dict(gates=lay.put(gates.reshape(T, B, 8 * H)), cs=lay.put(cs.reshape(T, B, 2 * H)))
    gb = run_backward(ops, case, lay, 1, dict(dy=dy, whh=whh, c0=c0, dhn=np.zeros((2, B, H)), dcn=np.zeros((2, B, H))), saved, bad, twin=False)
    rows = np.arange(B)
    open_ = gb["dgx"][0].reshape(B, 2, H, 4)[rows[:, None], np.arange(2)[None, :], kof.T]
    _, dh0, dc0 = L.probe_bwd_expected(whh, gates, cs, c0, kof, open_, case.bf, T)
    s = dict(dh0=L.ratio(gb["dh0"], dh0, *L.TOL_F32["dh0"]), dc0=L.ratio(gb["dc0"], dc0, *L.TOL_F32["dc0"]))
    report("probe T1 %s H%d  dh0 %.3f dc0 %.3f" % (flavour, H, s["dh0"], s["dc0"]))
    assert not bad and max(s.values()) <= 1.0, (bad, s)
