"""stft_kernel, istft_kernel, istft_rows_kernel and stft_psa_kernel (csrc/stft.hip) at the lengths their tile loops branch
on, against float64 references of the same formulas.

Cases, references and the tolerance rule  err(q) <= K * E_ref(q) + ulp(q)  per frame / per hop are tests/_stft_cases.py's;
the CPU file tests/test_stft_cases.py proves that a kernel with a wrong padding, a stale tile, a lost prelude, an
unrefilled ring slot ... misses these tolerances by 10 x.  Everything that needs no tolerance is exact: every output
lands in a NaN-filled pool with guard bands and padded rows (nothing but the owned elements changes, every owned element
is written), every input element the call must not read holds NaN, and layouts, sample formats, routes, batch
compositions and repeated calls must agree bit for bit.

Branches that no test reached before and that run here: stft_kernel<BINMAJOR>'s st != 1 store (a launch that mixes
layouts), the pcm16 fast path with complex and bin-major output, istft_load with mst == 1 (a (257, T) spectrum with a
(T, S * 257) mask), the inverse at T = 2 .. 5 and 31 .. 49 with two tiles per workgroup (a second workgroup whose only tile
holds no frame, its prelude), istft_rows_kernel below two tiles and with ld > S * 257, stft_psa_kernel's copy of the
loader on both sides of the fast-path condition.

Every figure is printed before it is asserted (pytest -s shows them); with SEPKERN_STFT_REPORT=<file> the per-family
ratios are written there -- profiles/stft_family.txt is such a file.
"""
import ctypes as C
import functools
import os
import time

import numpy as np
import pytest
import torch

import _stft_cases as SC
from oracle import stft as OS

pytestmark = pytest.mark.gpu

RATIOS = []          # (family, what, err, E_ref, ulp, smallest k that would pass) of the worst frame / hop of a check
T0 = time.time()
GUARD = 512          # elements of NaN in front of and behind every pool
NAN = float("nan")
PCM_FILL = 0x5A5A    # int16 pools cannot hold NaN: owned samples are checked value by value instead
NBIN, HOP = SC.NBIN, SC.HOP


def _report():
    lines = ["family        checks   max (err - ulp) / E_ref   asserted k"]
    for fam in SC.K:
        rs = [r for r in RATIOS if r[0] == fam]
        if rs:
            worst = max(rs, key=lambda r: r[5])
            lines.append("%-12s %7d   %-25.3f %d     (worst: %s, err %.3e, E_ref %.3e, ulp %.3e)"
                         % (fam, len(rs), worst[5], SC.K[fam], worst[1], worst[2], worst[3], worst[4]))
    lines.append("wall time of the module: %.1f s" % (time.time() - T0))
    print("\n" + "\n".join(lines))
    path = os.environ.get("SEPKERN_STFT_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n\nevery check (its worst frame / hop):\n")
            for r in RATIOS:
                f.write("%-12s %-60s err %.3e  E_ref %.3e  ulp %.3e  k %.3f\n" % r)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    from sepkern import ops as _ops
    yield _ops
    _report()


def close(family, what, got, ref, e_ref):
    """Per frame / hop: err <= K[family] * E_ref + ulp, K from profiles/stft_family.txt (tests/_stft_cases.py K)."""
    err, tol = SC.unit_err(got, ref), SC.tolerance(family, ref, e_ref)
    need = SC.needed_k(err, ref, e_ref)
    i = int(np.argmax(need))
    RATIOS.append((family, what, float(err[i]), float(e_ref[i]), float(SC.ulp32(np.abs(ref[i]).max())), float(need[i])))
    print("%-12s %-60s err %.3e  E_ref %.3e  ulp %.3e  k %.3f" % RATIOS[-1])
    bad = np.nonzero(err > tol)[0]
    assert bad.size == 0, "%s: frames / hops %s miss %d x E_ref + ulp (worst needs k = %.2f)" % (what, bad[:8].tolist(), SC.K[family], need[i])
    return float(need[i])


def bits(t):
    t = t.contiguous()
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a.cpu()), bits(b.cpu()))


def nan_pool(n, dtype=torch.float32):
    """(pool, view): n elements between two guard bands, everything NaN."""
    pool = torch.full((n + 2 * GUARD,), complex(NAN, NAN) if dtype.is_complex else NAN, dtype=dtype, device="cuda")
    return pool, pool[GUARD:GUARD + n]


def check_owned(pool, owned):
    """owned: bool numpy array over the view.  Nothing outside the owned elements changed, every owned element was written."""
    own = np.zeros(pool.numel(), bool)
    own[GUARD:GUARD + owned.size] = owned
    own = torch.from_numpy(own).cuda()
    nan = torch.isnan(torch.view_as_real(pool)) if pool.is_complex() else torch.isnan(pool)[:, None]
    assert bool(nan[~own].all()), "an element outside the owned ones was written"
    assert not bool(nan[own].any()), "an owned element was not written (or is NaN)"


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def i64(v):
    return torch.tensor(list(v), dtype=torch.int64, device="cuda")


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ forward
# TF: frame-major rows of 260; FT: bin-major rows of T + 3; TBF: the padded time-major batch (T, B, 260); MIX / XIM: TF and FT
# utterances alternating in one launch (XIM: FT first) -- the bin-major kernel, whose frame-major utterances take its
# st != 1 store branch: between the two every length takes it once
LAYOUTS = ("TF", "FT", "TBF", "MIX", "XIM")
LD = 260


def fwd_layout(layout, Ts):
    offs, st, sf, acc = [], [], [], 0
    B, Tm = len(Ts), max(Ts)
    for b, T in enumerate(Ts):
        kind = ("TF", "FT")[(b + (layout == "XIM")) % 2] if layout in ("MIX", "XIM") else layout
        if kind == "TF":
            offs, st, sf, acc = offs + [acc], st + [LD], sf + [1], acc + T * LD + 5
        elif kind == "FT":
            offs, st, sf, acc = offs + [acc], st + [1], sf + [T + 3], acc + NBIN * (T + 3) + 5
        else:
            offs, st, sf, acc = offs + [b * LD], st + [B * LD], sf + [1], Tm * B * LD
    return acc, offs, st, sf


@functools.lru_cache(maxsize=None)
def fwd_input(fmt):
    """fmt 'float32', 'int16' or 'pcmfloat' (float32 holding exactly pcm / 32768): the launch's utterances back to back in
    its shuffled order, NaN (int16: -32768) behind the last one."""
    c = SC.fwd_case("float32" if fmt == "float32" else "int16")
    raw = [c["raw"][u] for u in c["order"]]
    if fmt == "pcmfloat":
        raw = [OS.pcm16_to_float(r) for r in raw]
    ns = [len(r) for r in raw]
    total = sum(ns)
    buf = np.full(total + GUARD, -32768 if fmt == "int16" else NAN, np.int16 if fmt == "int16" else np.float32)
    buf[:total] = np.concatenate(raw)
    return c, torch.from_numpy(buf).cuda(), total, ns


@functools.lru_cache(maxsize=None)
def fwd_run(fmt, cplx, layout):
    """One launch of the mixed lengths, twice: per utterance (case order) its (T, 257) result on the host."""
    from sepkern import ops
    c, buf, total, ns = fwd_input(fmt)
    Ts = [SC.num_frames(n) for n in ns]
    assert max(Ts) == max(SC.FWD_FRAMES)
    size, offs, st, sf = fwd_layout(layout, Ts)
    if layout in ("MIX", "XIM"):
        assert 1 in sf and any(v != 1 for v in sf)           # not every stride_f is 1: the bin-major kernel, both store branches
    idx = [o + np.arange(T)[:, None] * a + np.arange(NBIN)[None, :] * b for o, T, a, b in zip(offs, Ts, st, sf)]
    owned = np.zeros(size, bool)
    for i in idx:
        assert i.min() >= 0 and i.max() < size and not owned[i].any()
        owned[i] = True
    pools = []
    for _ in range(2):
        pool, view = nan_pool(size, torch.complex64 if cplx else torch.float32)
        ops.stft_batch(buf[:total], want_complex=cplx, out=view, out_offs=offs, stride_t=st, stride_f=sf, lengths=ns)
        torch.cuda.synchronize()
        pools.append(pool)
    assert same_bits(pools[0], pools[1]), "a second call gives other bits"
    check_owned(pools[0], owned)
    view = pools[0][GUARD:GUARD + size].cpu()
    res = [None] * len(ns)
    for pos, u in enumerate(c["order"]):
        res[u] = view[torch.from_numpy(idx[pos])]
    return res


@pytest.mark.parametrize("cplx", [True, False], ids=["complex", "magnitude"])
@pytest.mark.parametrize("fmt", ["float32", "int16"])
def test_stft_mixed_lengths_against_float64_in_every_layout(ops, fmt, cplx):
    c = SC.fwd_case(fmt)
    base = fwd_run(fmt, cplx, "TF")
    for layout in LAYOUTS[1:]:
        other = fwd_run(fmt, cplx, layout)
        for u, N in enumerate(SC.FWD_LENGTHS):
            assert same_bits(base[u], other[u]), "N = %d: layout %s gives other bits than TF" % (N, layout)
    family = "stft_complex" if cplx else "stft_mag"
    worst = 0.0
    for u, N in enumerate(SC.FWD_LENGTHS):
        ref = c["ref"][u] if cplx else np.abs(c["ref"][u])
        worst = max(worst, close(family, "stft %s %s N %d" % (fmt, "complex" if cplx else "magnitude", N), base[u].numpy(), ref,
                                 c["e_c"][u] if cplx else c["e_m"][u]))
    print("stft %s %s: largest (err - ulp) / E_ref %.3f (asserted %d)" % (fmt, family, worst, SC.K[family]))


@pytest.mark.parametrize("cplx", [True, False], ids=["complex", "magnitude"])
def test_stft_int16_input_gives_the_bits_of_its_float32_image(ops, cplx):
    for layout in LAYOUTS:
        a, b = fwd_run("int16", cplx, layout), fwd_run("pcmfloat", cplx, layout)
        for u, N in enumerate(SC.FWD_LENGTHS):
            assert same_bits(a[u], b[u]), (layout, N)


@pytest.mark.parametrize("fmt", ["float32", "int16"])
def test_stft_utterance_alone_gives_the_bits_it_has_in_the_mixed_launch(ops, fmt):
    c = SC.fwd_case(fmt)
    for cplx in (True, False):
        base = fwd_run(fmt, cplx, "MIX")
        for u, N in enumerate(SC.FWD_LENGTHS):
            w = torch.from_numpy(c["raw"][u]).cuda()
            tf = ops.stft_batch([w], want_complex=cplx, layout="TF")[0]
            ft = ops.stft_batch([w], want_complex=cplx, layout="FT")[0]
            assert same_bits(tf, base[u]), ("TF", cplx, N)
            assert same_bits(ft.t(), base[u]), ("FT", cplx, N)


# ------------------------------------------------------------------------------------------------ inverse, through the C ABI
ROUTES = ("FT", "TF", "FT/TF")       # (257, T) spectrum and mask; (T, 257) rows; (257, T) spectrum with a (T, S * 257) mask
PADT = 2                             # frames >= T of every spectrum and mask hold NaN


def istft_abi(Ts, specs, masks, S, route, want_pcm=True):
    """sk_mask_istft on one launch: specs[u] (T, 257) complex64, masks[u] (S, T, 257) float32 or None.  Outputs go into NaN /
    PCM_FILL pools with 7 elements between signals.  -> ([u][s] float32 host tensors, [u][s] int16 or None, wav pool)."""
    from sepkern import _lib
    bm_spec, bm_mask = route != "TF", route == "FT"
    parts, moffs, mst, msf, acc = [], [], [], [], 0
    for T, X in zip(Ts, specs):
        assert X.shape == (T, NBIN) and X.dtype == np.complex64
        if bm_spec:
            a = np.full((NBIN, T + PADT), complex(NAN, NAN), np.complex64)
            a[:, :T] = X.T
            st, sf = 1, T + PADT
        else:
            a = np.full((T + PADT, NBIN), complex(NAN, NAN), np.complex64)
            a[:T] = X
            st, sf = NBIN, 1
        moffs, mst, msf, acc = moffs + [acc], mst + [st], msf + [sf], acc + a.size
        parts.append(a.ravel())
    spec = torch.from_numpy(np.concatenate(parts)).cuda()
    mask, koffs, kst, ksf = None, [], [], []
    if masks is not None:
        parts, acc = [], 0
        for T, m in zip(Ts, masks):
            assert m.shape == (S, T, NBIN) and m.dtype == np.float32
            if bm_mask:
                a = np.full((S, NBIN, T + PADT), NAN, np.float32)
                a[:, :, :T] = m.transpose(0, 2, 1)
                koffs += [acc + s * NBIN * (T + PADT) for s in range(S)]
                st, sf = 1, T + PADT
            else:
                ld = S * NBIN + 3                              # padded rows, NaN in the padding columns
                a = np.full((T + PADT, ld), NAN, np.float32)
                for s in range(S):
                    a[:T, s * NBIN:(s + 1) * NBIN] = m[s]
                koffs += [acc + s * NBIN for s in range(S)]
                st, sf = ld, 1
            kst, ksf, acc = kst + [st], ksf + [sf], acc + a.size
            parts.append(a.ravel())
        mask = torch.from_numpy(np.concatenate(parts)).cuda()
    else:
        assert S == 1 and route != "FT/TF"
    ooffs, acc = [], 0
    for T in Ts:
        for _ in range(S):
            ooffs.append(acc)
            acc += HOP * (T - 1) + 7
    owned = np.zeros(acc, bool)
    for us, o in enumerate(ooffs):
        owned[o:o + HOP * (Ts[us // S] - 1)] = True
    wpool, wav = nan_pool(acc)
    ppool = torch.full((acc + 2 * GUARD,), PCM_FILL, dtype=torch.int16, device="cuda") if want_pcm else None
    pcm = ppool[GUARD:GUARD + acc] if want_pcm else None
    d = [i64(moffs), i64(mst), i64(msf), i64(koffs) if masks is not None else None, i64(kst) if masks is not None else None,
         i64(ksf) if masks is not None else None, torch.tensor(list(Ts), dtype=torch.int32, device="cuda"), i64(ooffs)]
    _lib.call("sk_mask_istft", p(spec), p(d[0]), p(d[1]), p(d[2]), p(mask), p(d[3]), p(d[4]), p(d[5]), p(d[6]), len(Ts), S, 512, 128,
              p(wav), p(pcm), p(d[7]), max(Ts), stream())
    torch.cuda.synchronize()
    check_owned(wpool, owned)
    hw = wav.cpu()
    wavs = [[hw[ooffs[u * S + s]:ooffs[u * S + s] + HOP * (T - 1)] for s in range(S)] for u, T in enumerate(Ts)]
    pcms = None
    if want_pcm:
        hp = ppool.cpu().numpy()
        own = np.zeros(hp.size, bool)
        own[GUARD:GUARD + acc] = owned
        assert (hp[~own] == PCM_FILL).all(), "an int16 sample outside the owned ones was written"
        # int16 = the device's own float output x 32767, truncated toward zero, wrapped: every sample, exactly
        want = np.full(hp.size, PCM_FILL, np.int16)
        want[GUARD:GUARD + acc][owned] = OS.to_int16_wav(hw.numpy()[owned])
        assert np.array_equal(hp, want), "%d int16 samples are not the truncation of the float output" % int((hp != want).sum())
        hp = torch.from_numpy(hp[GUARD:GUARD + acc])
        pcms = [[hp[ooffs[u * S + s]:ooffs[u * S + s] + HOP * (T - 1)] for s in range(S)] for u, T in enumerate(Ts)]
    return wavs, pcms, wpool


@pytest.mark.parametrize("S", SC.INV_SPEAKERS)
def test_istft_unequal_frames_against_float64_on_every_route(ops, S):
    c = SC.inv_case(S)
    order = c["order"]
    Ts = [c["T"][u] for u in order]
    specs = [c["specs"][u] for u in order]
    masks = [c["masks"][u] for u in order] if S > 1 else None
    routes = ROUTES if S > 1 else ROUTES[:2]
    res = {r: istft_abi(Ts, specs, masks, S, r) for r in routes}
    again = istft_abi(Ts, specs, masks, S, "FT")
    assert same_bits(res["FT"][2], again[2]), "a second call gives other bits"
    wav, pcm = res["FT"][0], res["FT"][1]
    for r in routes[1:]:
        for pos, T in enumerate(Ts):
            for s in range(S):
                assert same_bits(wav[pos][s], res[r][0][pos][s]), "T = %d source %d: route %s gives other bits than FT" % (T, s, r)
                assert torch.equal(pcm[pos][s], res[r][1][pos][s])
    worst = 0.0
    for pos, u in enumerate(order):
        for s in range(S):
            worst = max(worst, close("istft", "istft S %d T %d source %d" % (S, Ts[pos], s), wav[pos][s].numpy().reshape(-1, HOP),
                                     c["ref"][u][s], c["e"][u][s]))
    print("istft S %d: largest (err - ulp) / E_ref %.3f (asserted %d)" % (S, worst, SC.K["istft"]))
    # the project's own entry points on the same data: the whole launch, and every utterance alone (bin-major and frame-major)
    d_specs = [torch.from_numpy(np.ascontiguousarray(X.T)).cuda() for X in specs]
    d_masks = [[torch.from_numpy(np.ascontiguousarray(m[s].T)).cuda() for s in range(S)] for m in masks] if S > 1 else None
    w2, p2 = ops.mask_istft(d_specs, d_masks)
    for pos, T in enumerate(Ts):
        one_w, one_p = ops.mask_istft([d_specs[pos]], [d_masks[pos]] if S > 1 else None)
        rows = torch.from_numpy(specs[pos]).cuda()
        mrows = torch.from_numpy(np.ascontiguousarray(np.concatenate(list(masks[pos]), axis=1))).cuda() if S > 1 else None
        fw, fp = ops.mask_istft_frames(rows, mrows, S)
        for s in range(S):
            for what, w, q in (("mask_istft", w2[pos][s], p2[pos][s]), ("alone", one_w[0][s], one_p[0][s]), ("mask_istft_frames", fw[s], fp[s])):
                assert same_bits(wav[pos][s], w), "T = %d source %d: %s gives other bits" % (T, s, what)
                assert torch.equal(pcm[pos][s], q.cpu()), (T, s, what)


def test_istft_int16_wraps_exactly(ops):
    X = (SC.inv_spec(17, 77) * np.float32(12.0)).astype(np.complex64)
    wav, pcm, _ = istft_abi([17], [X], None, 1, "FT")                  # the exact int16 check is istft_abi's
    w = wav[0][0].numpy()
    assert np.abs(w).max() * 32767.0 > 65536.0 and int(pcm[0][0].abs().max()) > 30000


def test_istft_four_tiles_per_workgroup(ops):
    SC.check_tpb4_claims()
    Ts = SC.tpb4_frames()
    utts = [SC.tpb4_utt(u) for u in range(SC.TPB4_NUTT)]
    S = SC.TPB4_S
    wav, _, _ = istft_abi(Ts, [x for x, _ in utts], [m for _, m in utts], S, "FT", want_pcm=False)
    worst = 0.0
    for u in SC.tpb4_sample():
        X, m = utts[u]
        alone, _, _ = istft_abi([Ts[u]], [X], [m], S, "FT", want_pcm=False)        # two tiles per workgroup
        for s in range(S):
            ref, e, _ = SC.inv_ref(SC.masked(X, m[s]))
            worst = max(worst, close("istft", "istft tpb 4 utterance %d T %d source %d" % (u, Ts[u], s),
                                     wav[u][s].numpy().reshape(-1, HOP), ref, e))
            assert same_bits(wav[u][s], alone[0][s]), "utterance %d (T = %d) source %d: alone (tpb 2) gives other bits than inside the tpb 4 launch" % (u, Ts[u], s)
    print("istft tpb 4: largest (err - ulp) / E_ref %.3f (asserted %d)" % (worst, SC.K["istft"]))


# ------------------------------------------------------------------------------------------------ inverse on packed rows
@pytest.mark.parametrize("S", SC.ROWS_SPEAKERS)
def test_istft_rows_against_float64(ops, S):
    from sepkern import _lib
    from sepkern.packing import Packing
    c = SC.rows_case(S)
    Ts, B = c["T"], len(c["T"])
    pk = Packing(Ts, "cuda")
    ld = S * NBIN + SC.ROWS_PAD
    assert ld > S * NBIN and pk.R == sum(Ts) and pk.T == max(Ts)
    mixc = np.full((pk.R + 2, NBIN), complex(NAN, NAN), np.complex64)           # two rows nobody owns
    mask = np.full((pk.R + 2, ld), NAN, np.float32)
    for j, T in enumerate(Ts):
        rows = pk.offs_host[:T].astype(np.int64) + j
        mixc[rows] = c["specs"][j]
        for s in range(S):
            mask[rows, s * NBIN:(s + 1) * NBIN] = c["masks"][j][s]
    assert not np.isnan(mixc[:pk.R].real).any() and np.isnan(mask[:pk.R, S * NBIN:]).all()
    d_mixc, d_mask = torch.from_numpy(mixc).cuda(), torch.from_numpy(mask).cuda()
    ooffs, acc = [], 0
    for T in Ts:
        for _ in range(S):
            ooffs.append(acc)
            acc += HOP * (T - 1) + 7
    owned = np.zeros(acc, bool)
    for us, o in enumerate(ooffs):
        owned[o:o + HOP * (Ts[us // S] - 1)] = True
    d_ooffs = i64(ooffs)
    pools = []
    for _ in range(2):
        pool, wav = nan_pool(acc)
        _lib.call("sk_mask_istft_rows", p(d_mixc), p(d_mask), ld, p(pk.offs), p(pk.lens), B, S, 512, 128, p(wav), p(d_ooffs), pk.T, stream())
        torch.cuda.synchronize()
        pools.append(pool)
    assert same_bits(pools[0], pools[1]), "a second call gives other bits"
    check_owned(pools[0], owned)
    hw = pools[0][GUARD:GUARD + acc].cpu()
    est, _, eo = ops.mask_istft_rows(d_mixc, d_mask, pk, S)
    est = est.cpu()
    # the (257, T) route on the same data: reported, not required
    flat_w, _ = ops.mask_istft([torch.from_numpy(np.ascontiguousarray(X.T)).cuda() for X in c["specs"]],
                               [[torch.from_numpy(np.ascontiguousarray(m[s].T)).cuda() for s in range(S)] for m in c["masks"]], want_pcm=False)
    worst, agree = 0.0, 0
    for j, T in enumerate(Ts):
        for s in range(S):
            got = hw[ooffs[j * S + s]:ooffs[j * S + s] + HOP * (T - 1)]
            assert same_bits(got, est[eo[j * S + s]:eo[j * S + s] + HOP * (T - 1)]), (T, s)
            worst = max(worst, close("istft_rows", "istft_rows S %d T %d source %d" % (S, T, s), got.numpy().reshape(-1, HOP),
                                     c["ref"][j][s], c["e"][j][s]))
            agree += same_bits(got, flat_w[j][s])
    print("istft_rows S %d: largest (err - ulp) / E_ref %.3f (asserted %d); %d of %d signals agree bit for bit with ops.mask_istft"
          % (S, worst, SC.K["istft_rows"], agree, B * S))


# ------------------------------------------------------------------------------------------------ sk_stft_psa's copy of the loader
PSA_LENGTHS = [4224, 4223, 2175, 383, 257]      # tile 1 on both sides of the fast-path condition, a tile plus one, N mod 128 = 127


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_stft_psa_on_both_sides_of_the_fast_path(ops, dtype):
    """sk_stft_psa compared the way tests/test_gpu_psa.py does: its mixture rows are features_from_pcm's bit for bit, its
    targets are the formula on sk_stft's complex spectra within that test's bound."""
    import test_gpu_psa as P
    from sepkern import psa
    from sepkern.data import features_from_pcm
    S, dev = 2, torch.device("cuda", 0)
    assert SC.fast_tile(PSA_LENGTHS[0], 1) and not SC.fast_tile(PSA_LENGTHS[1], 1)
    sigs = P._signals(PSA_LENGTHS, S, seed=41)
    flat, _, lens = P._flat(sigs, dtype, dev)
    ref_mix, _, ref_pk = features_from_pcm({"flat": flat, "keys": ["mix", "source1", "source2"], "lens": lens}, dev)
    mix, tg, pk = P._run(sigs, dtype, dev)
    assert pk.R == ref_pk.R == sum(SC.num_frames(n) for n in PSA_LENGTHS) and mix.shape == ref_mix.shape
    assert torch.equal(mix, ref_mix)
    other = P._run(sigs, "float32" if dtype == "int16" else "int16", dev)
    assert torch.equal(other[0], mix) and all(torch.equal(a, b) for a, b in zip(other[1], tg))
    spectra = [o.cpu().numpy().astype(np.complex128) for o in
               ops.stft_batch([torch.from_numpy(x).cuda() for utt in sigs for x in utt], want_complex=True, layout="TF")]
    worst = 0.0
    for j in range(len(sigs)):
        Y, srcs = spectra[j * (S + 1)], spectra[j * (S + 1) + 1:(j + 1) * (S + 1)]
        ref = psa.psa_targets(Y, srcs)
        amag = np.sqrt(Y.real ** 2 + Y.imag ** 2)
        assert amag.min() > 0.0
        for s in range(S):
            bound = 8.0 * 2.0 ** -24 * (np.abs(srcs[s].real * Y.real) + np.abs(srcs[s].imag * Y.imag)) / amag + 2.0 ** -140
            err = np.abs(P._utt(tg[s], pk, j).cpu().numpy().astype(np.float64) - ref[s])
            worst = max(worst, float((err / bound).max()))
    print("stft_psa %s: worst |target - formula on sk_stft's spectra| / bound = %.3f (gate 1)" % (dtype, worst))
    assert worst <= 1.0
