"""The GEMM kernels of csrc/gemm.hip at their tile, K-step and slice boundaries, through the C ABI (cases: tests/_gemm_cases.py).

Every case: operands in NaN pools (base pointer above the allocation's start, lda / ldb padded), C a view into a pool of
sentinels (ldc > N, guard rows on both sides; the sentinel is a NaN with a payload, also C's prefill when not accumulating),
the split-K / stream-K workspace with its counters zeroed by sk_gemm_workspace_init and its slabs filled with the sentinel.
Asserted per case: sk_gemm_last_kernel() is the claimed id; exact cases equal the integer reference with ZERO difference,
sigmoid cases meet the project's gate against the fp64 sigmoid of the exact sum; every sentinel of C, of the workspace's tail
and every counter is as before; a second call and the dense layout give the same bits.  Embed cases: the ragged product is bit
for bit the [:M, :N] block of the zero-padded one.  Cases whose kernel depends on the stream-K cut run on 256-CU devices.

sk_cast_bf16_rows and sk_split_rows are pinned here too at R, C in {1, 7, 8, 9}.
"""
import ctypes as C
import dataclasses
import math

import pytest
import torch

import _gemm_cases as G

pytestmark = pytest.mark.gpu

SENT32 = 0x7FC12345      # the sentinel: a quiet NaN with a payload
SENT16 = 0x7FC1          # ... as bf16
TAIL = 64


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    from sepkern import _lib, ops
    return dict(L=_lib, lib=_lib.load(), ncu=ops.device_info()[0])


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _pool(n, dtype):
    """n elements of sentinel on the device (torch's allocations are 256-byte aligned: asserted, the alignment rules count on it)."""
    t = torch.empty(int(n), dtype=dtype, device="cuda")
    assert t.data_ptr() % 256 == 0
    if dtype == torch.float32:
        t.view(torch.int32).fill_(SENT32)
    else:
        t.view(torch.int16).fill_(SENT16)
    return t


def _split3(x):
    """The three bf16 pieces of an fp32 tensor by round-to-nearest-even (split3() of gemm.hip)."""
    hi = x.bfloat16()
    r = x - hi.float()
    mid = r.bfloat16()
    lo = (r - mid.float()).bfloat16()
    return hi, mid, lo


def _place(pool, off, ld, rows, block):
    """block (rows, cols) into the pool at element offset off with row stride ld."""
    pool.as_strided((rows, block.shape[1]), (ld, 1), off).copy_(block)


def float_operands(c):
    """(A (batch, M, K), B (batch, K, N), bias (batch, N) | None, C0 (batch, M, N) | None) as float32 CPU tensors."""
    if c.kind == "embed":
        A, B, bias = G.embed_operands(c)
        return torch.from_numpy(A), torch.from_numpy(B), None if bias is None else torch.from_numpy(bias), None
    ia, ib, ibias, ic0 = G.int_operands(c)
    ea, eb, eu = G.SCALES[c.kind]
    f = lambda x, e: None if x is None else torch.from_numpy(x * 2.0 ** -e).float()
    return f(ia, ea), f(ib, eb), f(ibias, eu), f(ic0, eu)


def launch(env, c, fops, dense=False):
    """Run case c on the float operands fops; returns (kernel id, the image of C (batch, M + GUARD_ROWS, ldc) as int32 bits,
    problems: a list of broken sentinels / counters)."""
    g = G.geometry(c, dense)
    A, B, bias, C0 = fops
    half = g["half"]
    dt = torch.bfloat16 if half else torch.float32
    nplanes = 3 if c.entry == "pl3" else 1
    planeA, planeB = g["a_rows"] * g["lda"] + 64, g["b_rows"] * g["ldb"] + 64      # (pl3: the planes' own padding)
    apool = _pool(g["a_off"] + (nplanes - 1) * planeA + g["a_elems"] + TAIL, dt)
    bpool = _pool(g["b_off"] + (nplanes - 1) * planeB + g["b_elems"] + TAIL, dt)
    for pool, X, kmaj, off, ld, st, rows, plane in ((apool, A.cuda(), c.a_kmajor, g["a_off"], g["lda"], g["sA"], g["a_rows"], planeA),
                                                    (bpool, B.cuda().transpose(1, 2), c.b_kmajor, g["b_off"], g["ldb"], g["sB"], g["b_rows"], planeB)):
        # X: (batch, dim, K); stored [K][dim] when k-major, else [dim][K]
        pieces = _split3(X) if c.entry == "pl3" else (X.to(dt),)
        for pi, piece in enumerate(pieces):
            for z in range(c.batch):
                blk = piece[z].t() if kmaj else piece[z]
                _place(pool, off + pi * plane + z * st, ld, rows, blk.contiguous())
    ldc, sC, M, N = g["ldc"], g["sC"], c.M, c.N
    front = G.GUARD_ROWS * ldc
    cpool = _pool(front + c.batch * sC + TAIL, torch.float32)
    cview = cpool[front:front + c.batch * sC].view(c.batch, M + G.GUARD_ROWS, ldc)
    if c.acc:
        cview[:, :M, :N] = C0.cuda()
    bpl = None
    if bias is not None:
        bpl = _pool(64 + c.batch * N + TAIL, torch.float32)
        bpl[64:64 + c.batch * N] = bias.cuda().reshape(-1)
    ws = None
    lib = env["lib"]
    if c.splitk > 1 or c.ws:
        nbytes = lib.sk_gemm_workspace_bytes(M, N, c.batch, c.splitk) if c.splitk > 1 else lib.sk_gemm_streamk_workspace_bytes()
        assert nbytes % 4 == 0 and nbytes >= G.COUNTER_BYTES
        ws = _pool(nbytes // 4 + TAIL, torch.float32)
        env["L"].call("sk_gemm_workspace_init", _p(ws), _stream())
    pa, pb, pc = C.c_void_p(apool.data_ptr() + g["a_off"] * apool.element_size()), \
        C.c_void_p(bpool.data_ptr() + g["b_off"] * bpool.element_size()), C.c_void_p(cview.data_ptr())
    pbias = None if bpl is None else C.c_void_p(bpl.data_ptr() + 256)
    common = (M, N, c.K, g["lda"], g["ldb"], ldc)
    tail = (c.batch, g["sA"], g["sB"], sC, N if bpl is not None else 0, c.splitk, _p(ws))
    if c.entry == "f32":
        env["L"].call("sk_gemm_f32_splitk", pa, pb, pc, pbias, *common, c.form[0], c.form[1], int(c.acc), c.act, *tail, c.variant, _stream())
    elif c.entry == "bf16":
        env["L"].call("sk_gemm_bf16_splitk", pa, pb, pc, pbias, *common, c.form[0], c.form[1], int(c.acc), c.act, *tail, _stream())
    elif c.entry == "mm":
        env["L"].call("sk_gemm_bf16_mm", pa, pb, pc, pbias, *common, c.form[0], c.form[1], int(c.acc), c.act, *tail, _stream())
    else:
        env["L"].call("sk_gemm_pl3_tn", pa, pb, pc, *common, planeA, planeB, int(c.acc), c.batch, g["sA"], g["sB"], sC, c.splitk,
                      _p(ws), _stream())
    kid = lib.sk_gemm_last_kernel()
    torch.cuda.synchronize()
    bad = []
    ci = cpool.view(torch.int32)
    if not bool((ci[:front] == SENT32).all()):
        bad.append("C front guard")
    if not bool((ci[front + c.batch * sC:] == SENT32).all()):
        bad.append("C tail guard")
    if ws is not None:
        wi = ws.view(torch.int32)
        if not bool((wi[:G.COUNTER_BYTES // 4] == 0).all()):
            bad.append("counters not back at zero: %d" % int((wi[:G.COUNTER_BYTES // 4] != 0).sum()))
        if not bool((wi[-TAIL:] == SENT32).all()):
            bad.append("workspace tail")
    if bpl is not None and not bool((bpl.view(torch.int32)[:64] == SENT32).all()):
        bad.append("bias guard")
    return kid, cview.view(torch.int32).clone(), bad


def expected_image(c, fops):
    """The reference image on the device (float64; NaN = the sentinel must stand there)."""
    if G.cheap(c):
        return torch.from_numpy(G.reference(c)).cuda()
    # the same as G.reference(c) without a defect, formed on the device for the large cases (integers: exact in float64)
    A, B, bias, C0 = (None if x is None else x.cuda().double() for x in fops)
    g = G.geometry(c)
    val = torch.bmm(A, B)
    if bias is not None:
        val += bias[:, None, :]
    if C0 is not None:
        val += C0
    if c.act == 1:
        val = torch.sigmoid(val)
    img = torch.full((c.batch, c.M + G.GUARD_ROWS, g["ldc"]), float("nan"), dtype=torch.float64, device="cuda")
    img[:, :c.M, :c.N] = val
    return img


def check_image(c, bits, want):
    """bits: int32 image of C; want: float64 image with NaN where the sentinel must stand.  Returns (wrong sentinels, largest
    difference, number of differing elements)."""
    keep = torch.isnan(want)
    sent_bad = int((bits[keep] != SENT32).sum())
    got = bits.view(torch.float32).double()[~keep]
    d = (got - want[~keep]).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
    tol = G.SIGMOID_ATOL if c.kind == "sigmoid" else 0.0
    return sent_bad, (float(d.max()) if d.numel() else 0.0), int((d > tol).sum())


def run_exact(env, c):
    fops = float_operands(c)
    want = expected_image(c, fops)
    kid, bits, bad = launch(env, c, fops)
    assert kid == c.kid, (c.name, kid)
    assert not bad, (c.name, bad)
    sent_bad, dmax, nbad = check_image(c, bits, want)
    print("%-44s %-30s max diff %.3g" % (c.name, G.KERNELS[kid]["name"], dmax))
    assert sent_bad == 0, (c.name, "sentinels overwritten", sent_bad)
    assert nbad == 0, (c.name, "elements off", nbad, "max diff", dmax)
    kid2, bits2, bad2 = launch(env, c, fops)
    assert kid2 == kid and not bad2 and torch.equal(bits, bits2), (c.name, "second call", bad2)
    if G.KERNELS[kid]["persistent"]:
        # a last ticket taken one arrival early shows only when the true last contributor is late enough to find the counter
        # reset (it leaves it at 1) or its slab unread: a matter of timing, so the stream-K launches are repeated
        for _ in range(6):
            kidn, bitsn, badn = launch(env, c, fops)
            assert kidn == kid and not badn and torch.equal(bits, bitsn), (c.name, "repeated call", badn)
    gd = G.geometry(c, dense=True)
    kid3, bits3, bad3 = launch(env, c, fops, dense=True)
    assert kid3 == gd["kid"] and not bad3, (c.name, "dense layout", kid3, bad3)
    if c.kind == "exact" or kid3 == kid:
        assert torch.equal(bits, bits3), (c.name, "dense layout: other bits")
    else:
        assert check_image(c, bits3, want)[2] == 0, (c.name, "dense layout")


def _run_family(env, cases, what):
    for c in cases:
        run_exact(env, c)
    first = G.first_time_claims()
    fmt = lambda cl: "%s%s" % (cl[0], list(cl[1:]) if len(cl) > 1 else "")
    kernels = sorted({G.KERNELS[c.kid]["name"] for c in cases})
    print("family %s: %d cases on %s" % (what, len(cases), ", ".join(kernels)))
    for kid in sorted({c.kid for c in cases}):
        new = sorted({fmt(cl) for c in cases if c.kid == kid for cl in first[c.name]})
        print("  first run of %s at: %s" % (G.KERNELS[kid]["name"], " ".join(new) or "-"))


def _family_cases(fam, cut):
    """The non-embed cases of a family; cut: those whose kernel depends on the stream-K cut (a 256-CU device), or the others."""
    return [c for c in G.CASES if c.family == fam and c.kind != "embed" and G.needs_256_cus(c) == cut]


@pytest.mark.parametrize("family", [f for f in G.FAMILIES if _family_cases(f, False)])
def test_family(env, family):
    _run_family(env, _family_cases(family, False), family)


@pytest.mark.parametrize("family", [f for f in G.FAMILIES if _family_cases(f, True)])
def test_family_cases_that_pass_a_stream_k_workspace(env, family):
    if env["ncu"] != G.P_MI355X:
        pytest.skip("the claimed kernels depend on the stream-K cut of a 256-CU device")
    _run_family(env, _family_cases(family, True), family + " (stream-K workspace)")


# ------------------------------------------------------------------------------------------------ bf16-pipe exactness probes
PROBES = [G.Case("f32", 2, (0, 1), 256, 256, K, G.K_SPLIT, bias=False) for K in (256, 2048)] + \
         [G.Case("f32", 9, (0, 1), 256, 256, K, G.K_PLANES, bias=False) for K in (256, 2048)] + \
         [G.Case("pl3", 0, (1, 0), 256, 256, K, G.K_PL3, bias=False) for K in (256, 2048)] + \
         [G.Case("bf16", 0, (0, 1), 256, 256, K, G.K_BF16, bias=False) for K in (256, 2048)] + \
         [G.Case("mm", 0, (0, 0), 256, 256, K, G.K_BF2, bias=False) for K in (256, 2048)] + \
         [G.Case("mm", 0, (0, 0), 256, 256, K, G.K_BF2_WIDE, bias=False, batch=512) for K in (256, 2048)] + \
         [G.Case("mm", 0, (0, 0), 2048, 1024, K, G.K_BF2_STREAMK, bias=False, ws=True) for K in (512, 2048)]


@pytest.mark.parametrize("case", PROBES, ids=lambda c: c.name)
def test_bf16_pipe_sums_integers_exactly(env, case):
    """Interior products (whole tiles, no edges) of integer operands |a|, |b| <= 8 on every kernel of the bf16 matrix pipe: the
    MFMA truncates the alignment of its addends, so exactness of sums below 2^22 units is measured here, not presumed."""
    c = case
    if G.needs_256_cus(c) and env["ncu"] != G.P_MI355X:
        pytest.skip("the stream-K cut of a 256-CU device")
    fops = float_operands(c)
    kid, bits, bad = launch(env, c, fops)
    sent_bad, dmax, nbad = check_image(c, bits, expected_image(c, fops))
    print("probe %-40s %-32s operand range +-%d: %d of %d elements differ, max diff %.3g" % (
        c.name, G.KERNELS[kid]["name"], G.operand_range(c.K), nbad, c.batch * c.M * c.N, dmax))
    assert kid == c.kid and not bad and sent_bad == 0 and nbad == 0


# ------------------------------------------------------------------------------------------------ embedding
EMBED = [c for c in G.CASES if c.kind == "embed"]


def _embed_run(env, c):
    A, B, bias, _ = float_operands(c)
    kid, bits, bad = launch(env, c, (A, B, bias, None))
    assert kid == c.kid and not bad, (c.name, kid, bad)
    return (A, B, bias), bits


@pytest.mark.parametrize("case", EMBED, ids=lambda c: c.name)
def test_ragged_product_is_the_block_of_the_padded_one(env, case):
    c = case
    (A, B, bias), bits = _embed_run(env, c)
    Mp, Np = G.padded_shape(c)
    cp = dataclasses.replace(c, M=Mp, N=Np, claims=(), defects=())
    gp, g = G.geometry(cp), G.geometry(c)
    assert (gp["kid"], gp["splitk"], gp["kchunk"], gp["flip_q"]) == (g["kid"], g["splitk"], g["kchunk"], g["flip_q"])
    Ap, Bp = torch.zeros(c.batch, Mp, c.K), torch.zeros(c.batch, c.K, Np)
    Ap[:, :c.M], Bp[:, :, :c.N] = A, B
    biasp = None
    if bias is not None:
        biasp = torch.zeros(c.batch, Np)
        biasp[:, :c.N] = bias
    kidp, bitsp, badp = launch(env, cp, (Ap, Bp, biasp, None))
    assert kidp == c.kid and not badp, (kidp, badp)
    assert bool((bits[:, c.M:] == SENT32).all()) and bool((bits[:, :, c.N:] == SENT32).all()), "sentinels overwritten"
    same = bits[:, :c.M, :c.N] == bitsp[:, :c.M, :c.N]
    assert bool(same.all()), (c.name, "elements with other bits than the padded product", int((~same).sum()))
    # the split product's own gate against fp64 (test_gemm_exact_bf16_split_is_an_fp32_product)
    Ad, Bd = A.cuda().double(), B.cuda().double()
    ref = torch.bmm(Ad, Bd) + (0 if bias is None else bias.cuda().double()[:, None, :])
    mag = torch.bmm(Ad.abs(), Bd.abs()).clamp_min(1e-30)
    err = float(((bits[:, :c.M, :c.N].view(torch.float32).double() - ref).abs() / mag).max())
    print("%-44s rel err of sum|a||b| %.3g (gate %.3g)" % (c.name, err, 2.0 ** -23 * 4 * math.sqrt(c.K)))
    assert err <= 2.0 ** -23 * 4 * math.sqrt(c.K), err
    # the dense layout and a second call: the same bits
    assert torch.equal(launch(env, c, (A, B, bias, None))[1], bits)
    kd, bitsd, badd = launch(env, c, (A, B, bias, None), dense=True)
    assert kd == c.kid and not badd and torch.equal(bitsd, bits)


@pytest.mark.parametrize("K,splitk", [(784, 1), (1792, 5), (1536, 8)])
def test_pl3_equals_split3_bit_for_bit(env, K, splitk):
    """gemm_f32_kernel_pl3 forms the same pieces, products, K order and sign phases as gemm_f32_kernel_split3's T/N form: on
    operands whose pieces round, a sign phase counted from a slice's own first step instead of the global one shows here."""
    a = next(c for c in EMBED if c.kid == G.K_SPLIT and (c.K, c.splitk) == (K, splitk) and c.form == (1, 0))
    b = next(c for c in EMBED if c.kid == G.K_PL3 and (c.K, c.splitk) == (K, splitk))
    (A, B, _), bits_a = _embed_run(env, a)
    (A2, B2, _), bits_b = _embed_run(env, b)
    assert torch.equal(A, A2) and torch.equal(B, B2)
    same = bits_a[:, :a.M, :a.N] == bits_b[:, :a.M, :a.N]
    assert bool(same.all()), ("elements that differ", int((~same).sum()))


SLICED_SIGN = [c for c in G.CASES if c.family == "sign" and c.splitk > 1]


@pytest.mark.parametrize("case", SLICED_SIGN, ids=lambda c: c.name)
def test_sliced_split_product_is_the_sum_of_its_slices_formed_unsplit(env, case):
    """Pins, per kernel and form, that the slices of a split-K product continue ONE sign pattern counted in global K steps -- on
    operands whose pieces round, where the direction in which the bf16 MFMA truncates shows in the bits.  The reference comes
    from the same kernel launched UNSPLIT (its phase starts at step 0 by construction) on the operands with every K outside
    slice s set to zero: zero products leave an accumulator as it is and a negation is exact, so that launch yields exactly the
    slab of slice s under the global pattern.  The sliced launch must equal the fp32 sum of those slabs in slice order
    (finish_splitk).  A phase counted from each slice's own first step gives other bits in every later slice."""
    c = dataclasses.replace(case, kind="embed", bias=False, claims=(), defects=())
    g = G.geometry(c)
    assert g["kid"] == case.kid and g["inkernel"] and g["flip_q"] > 0
    A, B, _, _ = float_operands(c)
    kid, bits, bad = launch(env, c, (A, B, None, None))
    assert kid == case.kid and not bad, (kid, bad)
    unsplit = dataclasses.replace(c, splitk=1)
    assert G.geometry(unsplit)["kid"] == case.kid and G.geometry(unsplit)["flip_q"] == g["flip_q"]
    total = None
    for kb, ke in g["slices"]:
        As, Bs = torch.zeros_like(A), torch.zeros_like(B)
        As[:, :, kb:ke], Bs[:, kb:ke, :] = A[:, :, kb:ke], B[:, kb:ke, :]
        kidu, slab, badu = launch(env, unsplit, (As, Bs, None, None))
        assert kidu == case.kid and not badu
        slab = slab[:, :c.M, :c.N].view(torch.float32)
        total = slab.clone() if total is None else total + slab      # fp32, slice order
    got = bits[:, :c.M, :c.N].view(torch.float32)
    assert bool(torch.isfinite(got).all())
    same = got == total
    assert bool(same.all()), (case.name, "elements that differ from the sum of the slices", int((~same).sum()))


# ------------------------------------------------------------------------------------------------ the row converters
RC = (1, 7, 8, 9)


def _rows_input(R, Cc, ld, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, Cc, generator=g) * torch.exp2(torch.randint(-20, 21, (R, Cc), generator=g).float())
    x.view(-1)[0] = 0.0
    pool = _pool(1 + R * ld + TAIL, torch.float32)       # the source starts 4 bytes past a 16-byte boundary
    _place(pool, 1, ld, R, x.cuda())
    return x, pool


@pytest.mark.parametrize("R", RC)
@pytest.mark.parametrize("Cc", RC)
def test_cast_bf16_rows(env, R, Cc):
    for ld_src, off in ((Cc + 3, 1), (G.pad8(Cc) + 4, 0)):
        x, pool = _rows_input(R, Cc, ld_src, R * 16 + Cc)
        if off == 0:
            pool = _pool(R * ld_src + TAIL, torch.float32)
            _place(pool, 0, ld_src, R, x.cuda())
        R_pad, ld = R + 3, G.pad8(Cc) + 8
        out = _pool(64 + R_pad * ld + TAIL, torch.bfloat16)
        env["L"].call("sk_cast_bf16_rows", C.c_void_p(pool.data_ptr() + 4 * off), R, Cc, ld_src, C.c_void_p(out.data_ptr() + 128), ld, R_pad,
                      _stream())
        torch.cuda.synchronize()
        body = out[64:64 + R_pad * ld].view(R_pad, ld).view(torch.int16).cpu()
        want = torch.zeros(R_pad, ld, dtype=torch.bfloat16)
        want[:R, :Cc] = x.bfloat16()
        assert torch.equal(body, want.view(torch.int16)), (R, Cc, ld_src)      # values RNE, pad rows and columns +0 exactly
        oi = out.view(torch.int16)
        assert bool((oi[:64] == SENT16).all()) and bool((oi[64 + R_pad * ld:] == SENT16).all())


@pytest.mark.parametrize("R", RC)
@pytest.mark.parametrize("Cc", RC)
def test_split_rows(env, R, Cc):
    for ld_src, off in ((Cc + 3, 1), (G.pad8(Cc) + 4, 0)):
        x, pool = _rows_input(R, Cc, ld_src, R * 16 + Cc + 100)
        if off == 0:
            pool = _pool(R * ld_src + TAIL, torch.float32)
            _place(pool, 0, ld_src, R, x.cuda())
        R_pad, ld = R + 3, G.pad8(Cc) + 8
        plane = R_pad * ld + 16
        out = _pool(64 + 3 * plane + TAIL, torch.bfloat16)
        env["L"].call("sk_split_rows", C.c_void_p(pool.data_ptr() + 4 * off), R, Cc, ld_src, C.c_void_p(out.data_ptr() + 128), ld, R_pad,
                      plane, _stream())
        torch.cuda.synchronize()
        oi = out.view(torch.int16).cpu()
        planes = [out[64 + p * plane:64 + p * plane + R_pad * ld].view(R_pad, ld).cpu() for p in range(3)]
        hi, mid, lo = planes
        want = [torch.zeros(R_pad, ld, dtype=torch.bfloat16) for _ in range(3)]
        for w, piece in zip(want, _split3(x)):
            w[:R, :Cc] = piece
        for p in range(3):
            assert torch.equal(planes[p].view(torch.int16), want[p].view(torch.int16)), (R, Cc, p)   # pads +0 exactly
        assert torch.equal(hi[:R, :Cc], x.bfloat16())
        total = hi[:R, :Cc].double() + mid[:R, :Cc].double() + lo[:R, :Cc].double()
        assert torch.equal(total, x.double()), "the three planes must sum to the input exactly"
        assert bool((oi[:64] == SENT16).all()) and bool((oi[64 + 2 * plane + R_pad * ld:] == SENT16).all())
        for p in range(2):      # the gap between planes is nobody's
            assert bool((oi[64 + p * plane + R_pad * ld:64 + (p + 1) * plane] == SENT16).all())
