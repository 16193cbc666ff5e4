"""stoi_keep_kernel, stoi_env_kernel and stoi_score_kernel (csrc/stoi.hip) at the lengths their loops branch on, looked at
through sk_stoi's workspace: the kept lists and frame energies, the envelopes of every signal under every keep list, and
the scores, against sepkern/stoi.py in float64.

Cases, references, the envelope tolerance  err(t) <= K * E_ref(t) + ulp(t)  and the layout of the workspace are
tests/_stoi_cases.py's; the CPU file tests/test_stoi_cases.py proves that a scan that loses its carry, a neighbour frame taken
from the wrong place, a missing tile, a T or J off by one ... misses these checks by 10 x.  Everything that needs no tolerance is
exact: nkept and the kept lists; the workspace, `out` and `frames` lie in pools of 0xFF bytes / NaN / a sentinel with guard
bands (nothing but the owned elements changes, every owned element is written); every input sample the call must not read
holds NaN; a case alone, inside the mixed batch, in the batch in another order and in a second call must agree bit for bit,
and so must a pair of an S >= 2 utterance with an S = 1 call on that pair.

Branches that no test reached before and that run here: the scan's second and third trips (F = 257 .. 600) with a carry, a
trip that keeps nothing between two that do, S = 1 and S = 4 (20 signals per keep list), the score kernel's second and third
LDS tiles on a tile of exactly 30 frames, utterances whose row stride Fm is another utterance's F at F > 256.

Every figure is printed before it is asserted (pytest -s shows them); with SEPKERN_STOI_REPORT=<file> the measured ratios
are written there -- profiles/stoi_kernels.txt is such a file.
"""
import ctypes as C
import functools
import os
import time

import numpy as np
import pytest
import torch

import _stoi_cases as SC
from sepkern import stoi as ST

pytestmark = pytest.mark.gpu

T0 = time.time()
GUARD = 4096                 # bytes (workspace) / elements (out, frames) of fill in front of and behind every pool
GAP = 7                      # NaN samples in front of, between and behind the utterances of the packed inputs
FRAMES_FILL = -12345
ENV, ENERGY, SCORE, E2E = [], [], [], []      # the worst figure of every check: (what, ...)
BRANCHES = set()


def _report():
    lines = ["tests/test_gpu_stoi_kernels.py on the MI355X: the three kernels of csrc/stoi.hip through sk_stoi's workspace"]
    if ENV:
        w = max(ENV, key=lambda r: r[4])
        lines += ["envelopes     %5d checks   max (err - ulp) / E_ref %.3f   asserted K %d   (worst: %s, err %.3e, E_ref %.3e, ulp %.3e)"
                  % (len(ENV), w[4], SC.K_ENV, w[0], w[1], w[2], w[3])]
    if ENERGY:
        w = max(ENERGY, key=lambda r: r[1])
        lines += ["energies      %5d checks   max err / tolerance %.3g   (worst: %s)" % (len(ENERGY), w[1], w[0])]
    if SCORE:
        w = max(SCORE, key=lambda r: r[1])
        lines += ["score kernel  %5d checks   max |out - scores(float64) on its own envelopes| %.3e   16 x that %.3e   asserted gate %.3e   (worst: %s)"
                  % (len(SCORE), w[1], 16 * w[1], SC.SCORE_GATE, w[0])]
    if E2E:
        w = max(E2E, key=lambda r: r[1])
        lines += ["end to end    %5d checks   max |out - stoi_matrix(float64)| %.3e   gate g = 4 x the float32 error of the reference %.3e   (worst: %s)"
                  % (len(E2E), w[1], w[2], w[0])]
    lines += ["branches that ran: " + "; ".join(sorted(BRANCHES))]
    lines += ["wall time of the module: %.1f s" % (time.time() - T0)]
    print("\n" + "\n".join(lines))
    path = os.environ.get("SEPKERN_STOI_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n\nenvelopes, every check (its worst frame):\n")
            for r in ENV:
                f.write("%-44s err %.3e  E_ref %.3e  ulp %.3e  k %.3f\n" % r)
            f.write("\nscore kernel, every check:\n")
            for r in SCORE:
                f.write("%-44s %.3e\n" % r)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    from sepkern import _lib
    yield _lib
    _report()


@functools.lru_cache(maxsize=None)
def gate():
    """g = 4 x the float32 error of the reference over the case set (tests/test_gpu_stoi.py's rule)."""
    return 4.0 * max(float(np.abs(c.host()["m64"] - c.host()["m32"]).max()) for c in SC.CASES)


def p(t):
    return C.c_void_p(t.data_ptr())


class Pair(object):
    """Reference j and estimate k of a case as an S = 1 utterance (the poisoned signals, as they are)."""

    def __init__(self, case, k, j):
        self.S, self.n, self.F = 1, case.n, case.F
        refs, ests = case.poisoned()
        self._sig = (refs[j:j + 1], ests[k:k + 1])

    def poisoned(self):
        return self._sig


def run(lib, items):
    """One sk_stoi call on utterances of one S.  -> the workspace's bytes, out (U, S, S, 2), frames (U, S) on the host; the
    guard bands of the three pools are checked here."""
    S, U = items[0].S, len(items)
    lens = [c.n for c in items]
    offs, acc = [], GAP
    for n in lens:
        offs.append(acc)
        acc += S * n + GAP
    rbuf, ebuf = np.full(acc, np.nan, np.float32), np.full(acc, np.nan, np.float32)
    for c, o in zip(items, offs):
        refs, ests = c.poisoned()
        rbuf[o:o + S * c.n], ebuf[o:o + S * c.n] = refs.reshape(-1), ests.reshape(-1)
    lay = SC.workspace(U, S, max(lens))
    assert lib.load().sk_stoi_workspace_bytes(U, S, max(lens)) == lay["bytes"]
    wpool = torch.full((lay["bytes"] + 2 * GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    opool = torch.full((U * S * S * 2 + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    fpool = torch.full((U * S + 2 * GUARD,), FRAMES_FILL, dtype=torch.int32, device="cuda")
    d_ref, d_est = torch.from_numpy(rbuf).cuda(), torch.from_numpy(ebuf).cuda()
    h_offs, h_lens = (C.c_int64 * U)(*offs), (C.c_int32 * U)(*lens)
    lib.call("sk_stoi", p(d_ref), p(d_est), h_offs, h_lens, U, S, p(wpool[GUARD:]), p(opool[GUARD:]), p(fpool[GUARD:]),
             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    w, o, f = wpool.cpu().numpy(), opool.cpu().numpy(), fpool.cpu().numpy()
    assert (w[:GUARD] == 0xFF).all() and (w[GUARD + lay["bytes"]:] == 0xFF).all(), "a guard band of the workspace was written"
    assert np.isnan(o[:GUARD]).all() and np.isnan(o[-GUARD:]).all(), "a guard band of out was written"
    assert (f[:GUARD] == FRAMES_FILL).all() and (f[-GUARD:] == FRAMES_FILL).all(), "a guard band of frames was written"
    BRANCHES.add("S = %d" % S)
    return dict(S=S, U=U, lay=lay, offs=offs, lens=lens, ws=w[GUARD:GUARD + lay["bytes"]].copy(),
                out=o[GUARD:-GUARD].reshape(U, S, S, 2).copy(), frames=f[GUARD:-GUARD].reshape(U, S).copy())


def regions(res):
    """The workspace's parts as arrays over its bytes (views)."""
    lay, U, S, w = res["lay"], res["U"], res["S"], res["ws"]
    Fm, sigs = lay["Fm"], res["U"] * res["S"]
    part = lambda name, dt, count: w[lay[name]:lay[name] + count * np.dtype(dt).itemsize].view(dt)     # noqa: E731
    return dict(offs=part("offs", np.int64, U), lens=part("lens", np.int32, U), nkept=part("nkept", np.int32, sigs),
                kept=part("kept", np.int32, sigs * Fm).reshape(sigs, Fm), energy=part("energy", np.float64, sigs * Fm).reshape(sigs, Fm),
                env=part("env", np.float32, sigs * (S + 1) * SC.BANDS * Fm).reshape(sigs * (S + 1) * SC.BANDS, Fm))


def utterance(res, u, F):
    """Everything sk_stoi owns of utterance u, by the kernel's own nkept: a list of arrays to compare bit for bit."""
    S, r = res["S"], regions(res)
    bits = [res["out"][u], res["frames"][u], r["nkept"][u * S:(u + 1) * S]]
    for j in range(S):
        sig = u * S + j
        nk = int(r["nkept"][sig])
        assert 0 <= nk <= F, (u, j, nk, F)
        bits += [r["kept"][sig, :nk], r["energy"][sig, :F]]
        rows = [SC.env_row(sig, S, q, b) for q in range(S + 1) for b in range(SC.BANDS)]
        bits.append(r["env"][rows, :max(nk - 1, 0)])
    return bits


def same_bits(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def verify(cases, res, tag):
    """Assertions 1 to 6 of the module's docstring on one call."""
    S, U, lay = res["S"], res["U"], res["lay"]
    Fm, r, g = lay["Fm"], regions(res), gate()
    assert Fm == max(1, max(c.F for c in cases))
    assert r["offs"].tolist() == res["offs"] and r["lens"].tolist() == res["lens"]
    own = np.zeros(res["ws"].size, bool)                              # bytes of the workspace the call owns

    def mark(name, itemsize, first, count):
        own[lay[name] + first * itemsize:lay[name] + (first + count) * itemsize] = True
    mark("offs", 8, 0, U)
    mark("lens", 4, 0, U)
    mark("nkept", 4, 0, U * S)
    for u, c in enumerate(cases):
        h = c.host()
        what = "%s %s" % (tag, c.name)
        if c.F > SC.KEEP:
            BRANCHES.add("scan of %d trips" % (-(-c.F // SC.KEEP)))
            if Fm > c.F:
                BRANCHES.add("row stride Fm > F > 256")
        for j in range(S):
            sig, kept, T = u * S + j, h["kept"][j], h["T"][j]
            # 1. nkept and the kept list, exactly
            nk = int(r["nkept"][sig])
            print("%-44s reference %d: nkept %d (host %d), T %d" % (what, j, nk, len(kept), T))
            assert nk == len(kept) and r["kept"][sig, :nk].tolist() == kept.tolist(), (what, j)
            assert int(res["frames"][u, j]) == T == int(h["frames"][j])
            mark("kept", 4, sig * Fm, nk)
            mark("energy", 8, sig * Fm, c.F)
            if nk and int(kept[-1]) >= SC.KEEP:
                BRANCHES.add("kept frames past the first scan trip")
            # 2. the frame energies
            if c.F:
                err = np.abs(r["energy"][sig, :c.F] - h["energy"][j])
                err = np.where(np.isfinite(err), err, np.inf)
                with np.errstate(divide="ignore", invalid="ignore"):
                    ratio = np.where(err > 0, err / h["etol"][j], 0.0)
                ENERGY.append((what + " ref %d" % j, float(ratio.max())))
                print("%-44s reference %d: energy err / tolerance %.3g" % (what, j, ratio.max()))
                assert (err <= h["etol"][j]).all(), (what, j, float(ratio.max()))
            # 3. the envelopes of the S + 1 signals under this keep list
            envs = []
            for q in range(S + 1):
                rows = [SC.env_row(sig, S, q, b) for b in range(SC.BANDS)]
                for row in rows:
                    mark("env", 4, row * Fm, T)
                got = r["env"][rows, :T].astype(np.float64)
                envs.append(got)
                if T:
                    ref, e_ref = h["env"][j][q], h["e_ref"][j][q]
                    err, need = SC.frame_err(got, ref), SC.needed_k(SC.frame_err(got, ref), ref, e_ref)
                    t = int(np.argmax(need))
                    ENV.append(("%s ref %d signal %d" % (what, j, q), float(err[t]), float(e_ref[t]), float(SC.ulp32(np.abs(ref[:, t]).max())),
                                float(need[t])))
                    print("%-44s err %.3e  E_ref %.3e  ulp %.3e  k %.3f" % ENV[-1])
                    bad = np.nonzero(err > SC.env_tolerance(ref, e_ref))[0]
                    assert bad.size == 0, "%s: frames %s miss %d x E_ref + ulp (worst needs k = %.2f)" % (ENV[-1][0], bad[:8].tolist(), SC.K_ENV, need[t])
            if T > SC.STILE + SC.SSEG - 1:
                BRANCHES.add("score kernel walks %d LDS tiles" % (-(-(T - SC.SSEG + 1) // SC.STILE)))
            for k in range(S):
                got = res["out"][u, k, j]
                # 4. the score kernel alone: float64 scores of its own envelopes
                want = np.array(ST.scores(envs[0], envs[1 + k]))
                d = float(np.abs(got - want).max()) if np.isfinite(got).all() else np.inf
                SCORE.append(("%s out[%d][%d]" % (what, k, j), d))
                # 5. end to end
                e = float(np.abs(got - h["m64"][k, j]).max()) if np.isfinite(got).all() else np.inf
                E2E.append(("%s out[%d][%d]" % (what, k, j), e, g))
                print("%-44s out[%d][%d] = (%.9f, %.9f): score kernel %.3e (gate %.3e), end to end %.3e (gate %.3e)"
                      % (what, k, j, got[0], got[1], d, SC.SCORE_GATE, e, g))
                if T < SC.SSEG:
                    assert got[0] == SC.SHORT and got[1] == SC.SHORT, (what, k, j, got)
                assert d <= SC.SCORE_GATE and e <= g, (what, k, j, d, e)
    # 6. ownership inside the workspace; out and frames are owned whole
    w = res["ws"]
    assert (w[~own] == 0xFF).all(), "%s: %d bytes of the workspace outside the owned elements changed" % (tag, int((w[~own] != 0xFF).sum()))
    rk, mask4 = regions(res), own.view(np.uint8)
    for name, dt, unwritten in (("nkept", np.int32, lambda a: a == -1), ("kept", np.int32, lambda a: a == -1),
                                ("energy", np.float64, np.isnan), ("env", np.float32, np.isnan)):
        a = rk[name].reshape(-1)
        size = np.dtype(dt).itemsize
        o = mask4[lay[name]:lay[name] + a.size * size].reshape(-1, size)[:, 0].astype(bool)
        assert not unwritten(a[o]).any(), "%s: an owned element of %s was not written" % (tag, name)
    assert np.isfinite(res["out"]).all() and (res["frames"] >= 0).all(), "%s: an element of out / frames was not written" % tag
    assert g < 1e-5


@functools.lru_cache(maxsize=None)
def alone(name):
    from sepkern import _lib
    c = SC.BY_NAME[name]
    res = run(_lib, [c])
    verify([c], res, "alone")
    return utterance(res, 0, c.F)


def test_the_gate_is_far_below_a_definitional_slip(lib):
    print("end-to-end gate g = %.3g" % gate())
    assert 0.0 < gate() < 1e-5


@pytest.mark.parametrize("name", [c.name for c in SC.CASES])
def test_case_alone(lib, name):
    alone(name)


@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_mixed_batch_in_two_orders_and_twice(lib, S):
    cases = SC.group(S)
    first = run(lib, cases)
    verify(cases, first, "batch")
    again = run(lib, cases)
    assert first["ws"].tobytes() == again["ws"].tobytes() and first["out"].tobytes() == again["out"].tobytes(), "a second call gives other bits"
    assert first["frames"].tobytes() == again["frames"].tobytes()
    order = SC.other_order(cases)
    shuffled = [cases[i] for i in order]
    other = run(lib, shuffled)
    verify(shuffled, other, "reordered")
    for pos, i in enumerate(order):
        c = cases[i]
        a, b = utterance(first, i, c.F), utterance(other, pos, c.F)
        assert same_bits(a, b), "%s: the batch in another order gives other bits" % c.name
        assert same_bits(a, alone(c.name)), "%s: alone gives other bits than inside the mixed batch" % c.name


@pytest.mark.parametrize("S", [2, 3, 4])
def test_a_pair_has_the_bits_of_a_single_source_call(lib, S):
    for c in SC.group(S):
        full = run(lib, [c])
        pairs = [(k, j) for k in range(S) for j in range(S)]
        single = run(lib, [Pair(c, k, j) for k, j in pairs])
        for i, (k, j) in enumerate(pairs):
            print("%s out[%d][%d] = %r, S = 1 call: %r" % (c.name, k, j, full["out"][0, k, j].tolist(), single["out"][i, 0, 0].tolist()))
            assert full["out"][0, k, j].tobytes() == single["out"][i, 0, 0].tobytes(), (c.name, k, j)
            assert int(full["frames"][0, j]) == int(single["frames"][i, 0])
