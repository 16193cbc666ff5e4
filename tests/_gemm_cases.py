"""Cases, exact references and defect models of the GEMM kernel tests (csrc/gemm.hip).  Imports no GPU.

tests/test_gpu_gemm_cases.py runs every case below through the C ABI on operands in NaN pools and compares with the
references here; tests/test_gemm_cases.py proves on any machine that every case reaches the boundary it claims (the
claims are predicates over the RESTATEMENT of gemm.hip's host code and loop bounds in this file) and that every defect
model changes a checked element of a case that names it.

Operands of the EXACT cases are integers times a power of two (a = ia 2^-3, b = ib 2^-2, bias and C0 integers times 2^-5), so
every partial sum is a multiple of 2^-5 below 2^22 units and exactly representable whatever the summation order, the K
partition or the piece a product is formed from: the reference is the integer product and the comparison is equality.
SIGMOID cases use a = ia 2^-3, b = ib 2^-3 (pre-activations in units of 2^-6, spread over about +-6) and the project's gate on
sk_sigmoid (atol 2e-6).  EMBED cases use Gaussian operands scaled element-wise by 2^(-20 .. 20) (every split piece carries
weight): the ragged product must equal bit for bit the [:M, :N] block of the same operands zero-padded to whole 256 x 256
tiles, and meet 2^-23 * 4 sqrt(K) of sum |a||b| against fp64.

Out of scope: a product of more than 16384 tiles x batch entries (reduce_in_kernel's limit, the only way the fp32 entries
reach splitk_reduce_kernel) needs about a gigabyte of C; the reduce kernel is reached through the bf16 entries instead,
which always use it.
"""
import functools
from dataclasses import dataclass

import numpy as np

# ------------------------------------------------------------------------------------------------ restatement of gemm.hip
# kernel ids (the enum behind sk_gemm_last_kernel)
K_F32, K_SPLIT, K_DMA, K_WIDE, K_STREAMK, K_BF16, K_PLANES = 1, 2, 3, 4, 6, 9, 10
K_BF2, K_BF2_WIDE, K_BF2_STREAMK, K_PL3 = 11, 12, 13, 14
COUNTER_BYTES = 65536            # head of a workspace: 16384 ticket counters
GROUP_M = 8
P_MI355X = 256                   # streamk_wgs() on 256 CUs

# kernel_shape() + each kernel's K step, LDS ring depth (K steps in flight; the planes kernel: two LDS stages + two register
# sets, its main loop runs while kt + 4 < nk) and tile rows per group of the tile-order map
KERNELS = {
    K_F32: dict(name="gemm_f32_kernel", tile=(128, 128), bk=16, ring=2, threads=256, persistent=False, group=GROUP_M, any_k=True),
    K_SPLIT: dict(name="gemm_f32_kernel_split3", tile=(128, 128), bk=16, ring=2, threads=256, persistent=False, group=GROUP_M),
    K_DMA: dict(name="gemm_f32_kernel_dma<128>", tile=(128, 128), bk=16, ring=2, threads=256, persistent=False, group=GROUP_M),
    K_WIDE: dict(name="gemm_f32_kernel_dma<256>", tile=(256, 128), bk=16, ring=2, threads=512, persistent=False, group=GROUP_M // 2),
    K_STREAMK: dict(name="gemm_f32_kernel_streamk", tile=(256, 256), bk=16, ring=3, threads=512, persistent=True, group=GROUP_M // 2),
    K_BF16: dict(name="bf::gemm_bf16_kernel", tile=(128, 128), bk=32, ring=2, threads=256, persistent=False, group=GROUP_M, any_k=True),
    K_PLANES: dict(name="gemm_f32_kernel_planes", tile=(256, 128), bk=16, ring=4, threads=512, persistent=False, group=GROUP_M // 2),
    K_BF2: dict(name="bf2::gemm_bf16_nt_kernel<128>", tile=(256, 128), bk=64, ring=2, threads=512, persistent=False, group=GROUP_M),
    K_BF2_WIDE: dict(name="bf2::gemm_bf16_nt_kernel<256>", tile=(256, 256), bk=64, ring=2, threads=512, persistent=False, group=GROUP_M),
    K_BF2_STREAMK: dict(name="bf2::gemm_bf16_streamk_kernel", tile=(256, 256), bk=64, ring=2, threads=512, persistent=True, group=GROUP_M),
    K_PL3: dict(name="gemm_f32_kernel_pl3", tile=(128, 128), bk=16, ring=2, threads=256, persistent=False, group=GROUP_M),
}
SIGNED = (K_SPLIT, K_PLANES, K_PL3)          # the kernels with sign phases
BF16_PIPE = (K_SPLIT, K_PLANES, K_PL3, K_BF16, K_BF2, K_BF2_WIDE, K_BF2_STREAMK)


def cdiv(a, b):
    return -(-a // b)


def slice_k(K, splitk, bk):
    """slice_k(): (g.splitk, g.kchunk) -- only slices that hold work are counted."""
    kchunk = cdiv(cdiv(K, splitk), bk) * bk
    return cdiv(K, kchunk), kchunk


def reduce_in_kernel(splitk, tiles, batch):
    return splitk > 1 and tiles * batch * 4 <= COUNTER_BYTES


def flip_quarter(K, bk=16):
    nks = K // bk
    if nks < 48:
        return 0
    periods = (nks + 32) // 64
    return (nks + 4 * periods - 1) // (4 * periods)


def sign_of_step(q, kstep):
    """SignPhase: -1 where the stretch of global K step kstep is negative (signs + - - + ...), else +1."""
    if q <= 0:
        return 1
    return -1 if ((kstep // q + 1) & 2) else 1


def _thr(force, name, value):
    """A named threshold of the choosers: its value, or the one `force` = (name, value) puts in its place -- what
    test_gemm_cases.py uses to show that a threshold case is DECISIVE (the other side of that one condition is another kernel)."""
    return force[1] if force and force[0] == name else bool(value)


def streamk_cut(nt, nk, P=P_MI355X, force=None):
    """streamk_cut(): (sk_tiles, sk_full) or None when the cut is refused."""
    if P < 8 or nt >= (1 << 24) or not _thr(force, "nk>=8", nk >= 8):
        return None
    full = nt // P
    rem = nt - full * P
    if (rem > 0 and not _thr(force, "rem*nk>=P", rem * nk >= P)) or rem > 16384:
        return None
    return nt, full


def streamk_ranges(nt, nk, full, P=P_MI355X):
    """Per workgroup b of the stream-K kernels: (beg, end, t0, nseg) of its share of the last partial round (nseg without the
    `full` data-parallel segments)."""
    R = (nt - full * P) * nk
    out = []
    for b in range(P):
        beg, end = b * R // P, (b + 1) * R // P
        t0 = beg // nk if nk else 0
        out.append((beg, end, t0, ((end - 1) // nk - t0 + 1) if end > beg else 0))
    return out


def streamk_fixup(t, nk, R, P=P_MI355X):
    """The fix-up of stream-K tile t: (w0, w1, second) -- first and last contributing workgroup and whether the first
    contributor's piece of this tile is its second one."""
    w0 = ((t * nk + 1) * P - 1) // R
    w1 = ((t + 1) * nk * P - 1) // R
    return w0, w1, 1 if w0 * R // P < t * nk else 0


def xcd_map(b, nt):
    """blockIdx.x -> position in the tile list: blocks b and b + 8 share an XCD, each XCD walks its own run of the list."""
    q, rem, x, j = nt >> 3, nt & 7, b & 7, b >> 3
    return (x * (q + 1) if x < rem else rem * (q + 1) + (x - rem) * q) + j


def group_map(tile, tilesM, tilesN, group):
    """Position in the tile list -> (tile row, tile column): groups of `group` tile rows walked column by column."""
    per = group * tilesN
    grp = tile // per
    rem2 = tile - grp * per
    first = grp * group
    gsz = min(group, tilesM - first)
    return first + rem2 % gsz, rem2 // gsz


def tile_of_block(b, tilesM, tilesN, group, defect=None):
    nt = tilesM * tilesN
    if defect == "tile_order_xcd":      # the remainder runs forgotten: every XCD's run taken as nt / 8 long
        tile = (b & 7) * (nt >> 3) + (b >> 3)
    else:
        tile = xcd_map(b, nt)
    if defect == "tile_order_group":    # the last, smaller group walked as a full one
        per = group * tilesN
        grp = tile // per
        rem2 = tile - grp * per
        return grp * group + rem2 % group, rem2 // group
    return group_map(tile, tilesM, tilesN, group)


def vec_ok(off_bytes, ld, stride):
    """g.vecA / g.vecB: 16-byte aligned pointer, rows and batch stride whole float4s."""
    return off_bytes % 16 == 0 and ld % 4 == 0 and stride % 4 == 0


def dma_ok(vecA, vecB, M, N, K, kchunk, tA, tB, choose=False, force=None):
    if not vecA or not vecB or (tA and tB):
        return False
    if K % 16 or kchunk % 16:
        return False
    if tA and (not _thr(force, "M%4==0", M % 4 == 0) or M < 4):
        return False
    if not tB and (not _thr(force, "N%4==0", N % 4 == 0) or N < 4):
        return False
    if choose and not tA and tB and M >= 1024 and N >= 1024:
        return False
    return True


def choose_kernel(M, N, K, splitk, kchunk, vecA, vecB, bf16, variant, tA, tB, batch, ws, P=P_MI355X, force=None):
    """choose_kernel() with SEPKERN_GEMM_SPLIT unset: (kernel id, stream-K cut or None); splitk, kchunk as slice_k() left them."""
    if bf16:
        return K_BF16, None
    dma = dma_ok(vecA, vecB, M, N, K, kchunk, tA, tB, force=force)
    m256 = _thr(force, "M>=256", M >= 256)
    unsplit, large = splitk == 1, _thr(force, "large", (not tA) and M >= 4096 and N >= 1024)
    if variant in (0, 2, 9) and dma:
        planes = unsplit and batch == 1 and m256 and _thr(force, "N>=128", N >= 128) and \
            (variant == 9 or (variant == 0 and _thr(force, "tiles256x128>=192", cdiv(M, 256) * cdiv(N, 128) >= 192)))
        return (K_PLANES if planes else K_SPLIT), None
    mfma_choose = variant in (8, 0)
    if dma and ws and batch == 1 and m256 and N >= 256 and unsplit and (variant == 6 or (mfma_choose and large)):
        cut = streamk_cut(cdiv(M, 256) * cdiv(N, 256), K // 16, P, force)
        if cut:
            return K_STREAMK, cut
    if dma and m256 and (variant in (4, 6) or (mfma_choose and large and unsplit)):
        return K_WIDE, None
    return (K_DMA if variant != 1 and dma_ok(vecA, vecB, M, N, K, kchunk, tA, tB, mfma_choose, force) else K_F32), None


def choose_bf16_mm(M, N, K, splitk, batch, ws, P=P_MI355X, force=None):
    """The choice in sk_gemm_bf16_mm (splitk as slice_k() left it)."""
    cols256 = _thr(force, "cols256", N % 256 == 0 or N > 1024)
    cut = None
    if splitk == 1 and ws and batch == 1 and M >= 256 and cols256:
        cut = streamk_cut(cdiv(M, 256) * cdiv(N, 256), K // 64, P, force)
    wide = cut is not None or (cols256 and _thr(force, "tiles>=512", cdiv(M, 256) * cdiv(N, 256) * splitk * batch >= 2 * 256))
    return (K_BF2_STREAMK if cut else K_BF2_WIDE if wide else K_BF2), cut


# ------------------------------------------------------------------------------------------------ cases
GUARD_ROWS = 3       # sentinel rows behind row M - 1 of every batch entry of C (and the row gap in front of entry 0)
BASE_OFF = 64        # elements between an operand pool's start and the operand


@dataclass(frozen=True)
class Case:
    """One launch.  entry: f32 (sk_gemm_f32_splitk), bf16 (sk_gemm_bf16_splitk), mm (sk_gemm_bf16_mm), pl3 (sk_gemm_pl3_tn).
    form: (transA, transB) of the fp32-operand entries, (a_kmajor, b_kmajor) of mm; pl3 is T/N.  Layout: pad = elements added to
    lda / ldb (None: 4 floats / 8 bf16; 1 = the dword kernel; a pair: one each), a_off / b_off = extra elements in front of the operand (1 float: a
    pointer that is 4 mod 16 bytes), ldc = N + ldc_pad, ws = the stream-K workspace passed with splitk = 1, inter = both batch
    entries of the k-major operands side by side in one allocation (the dW_hh layout).  kid: the kernel id the case claims;
    claims: (predicate, args...) tuples over the restatement; defects: the defect models this case is a witness of."""
    entry: str
    variant: int
    form: tuple
    M: int
    N: int
    K: int
    kid: int
    splitk: int = 1
    batch: int = 1
    kind: str = "exact"
    bias: bool = True
    acc: bool = False
    act: int = 0
    pad: object = None
    a_off: int = 0
    b_off: int = 0
    ldc_pad: int = 5
    ws: bool = False
    inter: bool = False
    claims: tuple = ()
    defects: tuple = ()
    family: str = ""

    @property
    def name(self):
        f = "NT"[self.form[0]] + "NT"[self.form[1]] if self.entry in ("f32", "bf16") else \
            ("km" if self.form[0] else "rm") + ("km" if self.form[1] else "rm")
        s = "%s_v%d_%s_%dx%dx%d" % (self.entry, self.variant, f, self.M, self.N, self.K)
        if self.splitk > 1:
            s += "_s%d" % self.splitk
        if self.batch > 1:
            s += "_b%d%s" % (self.batch, "i" if self.inter else "")
        if self.kind != "exact":
            s += "_" + self.kind
        for flag, tag in ((self.acc, "acc"), (self.act, "sig"), (self.ws, "ws"), (self.a_off, "aoff%d" % self.a_off),
                          (self.b_off, "boff%d" % self.b_off), (self.pad is not None, "pad%s" % ("-".join(map(str, self.pad)) if isinstance(self.pad, tuple) else self.pad)),
                          (self.ldc_pad != 5, "ldc%d" % self.ldc_pad), (not self.bias and self.entry != "pl3", "nobias")):
            if flag:
                s += "_" + tag
        return s

    @property
    def a_kmajor(self):
        return True if self.entry == "pl3" else bool(self.form[0])

    @property
    def b_kmajor(self):
        if self.entry == "pl3":
            return True
        return bool(self.form[1]) if self.entry == "mm" else not self.form[1]


def pad8(n):
    return (n + 7) // 8 * 8


@functools.lru_cache(maxsize=None)
def geometry(c, dense=False, P=P_MI355X, force=None):
    """Everything the launch of case c is made of: leading dimensions, strides, offsets (elements), alignment, the sliced K, the
    kernel the restated chooser takes, its tiles.  dense: operands with no row padding and no extra offset.  force: (threshold
    name, value) put in place of that one condition of the chooser (_thr)."""
    half = c.entry in ("mm", "pl3")                      # bf16 elements in memory
    pad = 0 if dense else (c.pad if c.pad is not None else (8 if half else 4))
    pad_a, pad_b = pad if isinstance(pad, tuple) else (pad, pad)
    a_off, b_off = (0, 0) if dense else (c.a_off, c.b_off)
    a_rows, a_cols = (c.K, c.M) if c.a_kmajor else (c.M, c.K)
    b_rows, b_cols = (c.K, c.N) if c.b_kmajor else (c.N, c.K)
    if half and c.a_kmajor:
        a_cols = pad8(a_cols)                              # a k row's padded width
    if half and c.b_kmajor:
        b_cols = pad8(b_cols)
    if c.inter:
        assert c.a_kmajor and c.b_kmajor and c.batch == 2
        lda, ldb = (c.batch - 1) * c.M + a_cols + pad_a, (c.batch - 1) * c.N + b_cols + pad_b
        sA, sB = c.M, c.N
        a_elems, b_elems = a_rows * lda, b_rows * ldb
    else:
        lda, ldb = a_cols + pad_a, b_cols + pad_b
        sA, sB = a_rows * lda, b_rows * ldb
        a_elems, b_elems = c.batch * sA, c.batch * sB
    ldc = c.N + c.ldc_pad
    sC = (c.M + GUARD_ROWS) * ldc
    esz = 2 if half else 4
    vecA = vec_ok((BASE_OFF + a_off) * esz, lda, sA)
    vecB = vec_ok((BASE_OFF + b_off) * esz, ldb, sB)
    bk = 16
    if c.entry == "f32":
        splitk, kchunk = slice_k(c.K, c.splitk, 16)
        kid, cut = choose_kernel(c.M, c.N, c.K, splitk, kchunk, vecA, vecB, False, c.variant, c.form[0], c.form[1], c.batch,
                                 c.ws or c.splitk > 1, P, force)
    elif c.entry == "bf16":
        splitk, kchunk = slice_k(c.K, c.splitk, 32)
        kid, cut = K_BF16, None
    elif c.entry == "mm":
        splitk, kchunk = slice_k(c.K, c.splitk, 64)
        kid, cut = choose_bf16_mm(c.M, c.N, c.K, splitk, c.batch, c.ws or c.splitk > 1, P, force)
    else:
        splitk, kchunk = slice_k(c.K, c.splitk, 16)
        kid, cut = K_PL3, None
    ks = KERNELS[kid]
    bk = ks["bk"]
    tm, tn = ks["tile"]
    tilesM, tilesN = cdiv(c.M, tm), cdiv(c.N, tn)
    slices = [(s * kchunk, min(c.K, (s + 1) * kchunk)) for s in range(splitk)]
    inkernel = c.entry in ("f32", "pl3") and reduce_in_kernel(splitk, tilesM * tilesN, c.batch)
    flip_q = flip_quarter(c.K) if kid in SIGNED else 0
    return dict(lda=lda, ldb=ldb, ldc=ldc, sA=sA, sB=sB, sC=sC, a_off=BASE_OFF + a_off, b_off=BASE_OFF + b_off, a_elems=a_elems,
                b_elems=b_elems, a_rows=a_rows, b_rows=b_rows, vecA=vecA, vecB=vecB, splitk=splitk, kchunk=kchunk, kid=kid, cut=cut,
                bk=bk, tile=(tm, tn), tilesM=tilesM, tilesN=tilesN, tiles=tilesM * tilesN, slices=slices, inkernel=inkernel,
                flip_q=flip_q, group=ks["group"], ring=ks["ring"], persistent=ks["persistent"], half=half)


# ---- claims: named predicates over (case, geometry)
def _steps(g, s=0):
    kb, ke = g["slices"][s]
    return cdiv(ke - kb, g["bk"])


def _sk(c, g):
    nt, full = g["cut"]
    nk = c.K // g["bk"]
    R = (nt - full * P_MI355X) * nk
    return nt, full, nk, R, streamk_ranges(nt, nk, full)


def _dim(c, g, which, what):
    v, t = (c.M, g["tile"][0]) if which == "M" else (c.N, g["tile"][1])
    return v == {"1": 1, "4": 4, "tile-1": t - 1, "tile": t, "tile+1": t + 1, "tile+4": t + 4}.get(what, -1) or \
        (what.isdigit() and v == int(what))


def xcd_remainder(g):
    """The XCD runs of the tile list are of two lengths and more than one tile long: nt > 8 and nt % 8 != 0."""
    return g["tiles"] > 8 and g["tiles"] % 8 != 0


def ragged_group(g):
    """The last group of tile rows is smaller than the others and is walked over more than one tile column."""
    return g["tilesM"] > g["group"] and g["tilesM"] % g["group"] != 0 and g["tilesN"] > 1


def _slice_signs(g, s):
    kb, ke = g["slices"][s]
    return [sign_of_step(g["flip_q"], k) for k in range(kb // 16, cdiv(ke, 16))]


THRESHOLDS = {
    "M>=256": lambda c, g: c.M >= 256,
    "N>=128": lambda c, g: c.N >= 128,
    "tiles256x128>=192": lambda c, g: cdiv(c.M, 256) * cdiv(c.N, 128) >= 192,
    "large": lambda c, g: (not c.form[0]) and c.M >= 4096 and c.N >= 1024,
    "M%4==0": lambda c, g: c.M % 4 == 0,
    "N%4==0": lambda c, g: c.N % 4 == 0,
    "cols256": lambda c, g: c.N % 256 == 0 or c.N > 1024,
    "tiles>=512": lambda c, g: cdiv(c.M, 256) * cdiv(c.N, 256) * g["splitk"] * c.batch >= 512,
    "nk>=8": lambda c, g: c.K // (64 if c.entry == "mm" else 16) >= 8,
    "rem*nk>=P": lambda c, g: (lambda nt, nk: (nt % P_MI355X) * nk >= P_MI355X)(cdiv(c.M, 256) * cdiv(c.N, 256),
                                                                                  c.K // (64 if c.entry == "mm" else 16)),
}

PREDICATES = {
    "nk": lambda c, g, n: _steps(g) == n and c.K % g["bk"] == 0,
    "nk_ring+1": lambda c, g: _steps(g) == g["ring"] + 1,
    "K": lambda c, g, what: c.K == {"1": 1, "BK-1": g["bk"] - 1, "BK": g["bk"], "BK+1": g["bk"] + 1, "2BK-1": 2 * g["bk"] - 1,
                                    "2BK+1": 2 * g["bk"] + 1}[what],
    "ragged_k": lambda c, g: c.K % g["bk"] != 0,
    "M": lambda c, g, what: _dim(c, g, "M", what),
    "N": lambda c, g, what: _dim(c, g, "N", what),
    "a_kmajor": lambda c, g: c.a_kmajor,
    "b_kmajor": lambda c, g: c.b_kmajor,
    "tt": lambda c, g: c.entry in ("f32", "bf16") and c.form == (1, 1),
    "vec_mismatch": lambda c, g: g["vecA"] != g["vecB"],
    "dword": lambda c, g: g["kid"] == K_F32 and not (g["vecA"] and g["vecB"]),
    "ptr_4mod16": lambda c, g: (g["a_off"] * 4) % 16 == 4 or (g["b_off"] * 4) % 16 == 4,
    "tiles_mod8": lambda c, g, r: g["tiles"] % 8 == r and not g["persistent"],
    "tilesM": lambda c, g, k: g["tilesM"] == k * g["group"] + 1,
    "last_slice_short": lambda c, g: g["splitk"] > 1 and g["slices"][-1][1] - g["slices"][-1][0] < g["kchunk"],
    "last_slice_ragged": lambda c, g: g["splitk"] > 1 and (g["slices"][-1][1] - g["slices"][-1][0]) % g["bk"] != 0,
    "splitk_recomputed": lambda c, g, n: c.splitk != g["splitk"] and g["splitk"] == n,
    "inkernel_reduce": lambda c, g: g["inkernel"],
    "reduce_kernel": lambda c, g: g["splitk"] > 1 and not g["inkernel"],
    "scalar_reduce": lambda c, g: g["splitk"] > 1 and not g["inkernel"] and c.N % 4 != 0 and c.ldc_pad == 3,
    "batch_inter": lambda c, g: c.batch == 2 and c.inter and g["sA"] == c.M and g["lda"] >= 2 * c.M,
    "batch": lambda c, g: c.batch == 2,
    "flip_q": lambda c, g, q: g["flip_q"] == q,
    "nks": lambda c, g, n: c.K // 16 == n and c.K % 16 == 0,      # K steps of the whole product (what flip_quarter() sees)
    "slice_midstretch": lambda c, g: any((kb // 16) % g["flip_q"] != 0 for kb, _ in g["slices"][1:]),
    "slice_all_negative": lambda c, g: any(all(s < 0 for s in _slice_signs(g, i)) for i in range(g["splitk"])),
    "ends_negative": lambda c, g: any(_slice_signs(g, i)[-1] < 0 for i in range(g["splitk"])),
    "sigmoid": lambda c, g: c.act == 1,
    "accumulate": lambda c, g: c.acc,
    "sk_one_step_each": lambda c, g: (lambda nt, full, nk, R, rg: nt == 1 and nk == P_MI355X and all(e - b == 1 for b, e, _, _ in rg)
                                      and streamk_fixup(0, nk, R)[:2] == (0, P_MI355X - 1))(*_sk(c, g)),
    "sk_ranges_1_2": lambda c, g: (lambda nt, full, nk, R, rg: {e - b for b, e, _, _ in rg} == {1, 2})(*_sk(c, g)),
    "sk_two_tiles": lambda c, g: (lambda nt, full, nk, R, rg: any(n == 2 for _, _, _, n in rg))(*_sk(c, g)),
    "sk_first_piece_second": lambda c, g: (lambda nt, full, nk, R, rg: any(streamk_fixup(t, nk, R)[2] for t in range(nt - full * P_MI355X)))(*_sk(c, g)),
    "sk_refused": lambda c, g, nk: g["cut"] is None and c.ws and c.K // (64 if c.entry == "mm" else 16) == nk,
    "sk_cut": lambda c, g, nt, full: g["cut"] == (nt, full),      # the accepted partition: tiles, whole rounds in front of the cut
    "xcd_remainder": lambda c, g: xcd_remainder(g),
    "ragged_group": lambda c, g: ragged_group(g),
    "ragged_m": lambda c, g: c.M % g["tile"][0] != 0,
    "thr": lambda c, g, name, side: bool(THRESHOLDS[name](c, g)) == side,
}


def check_streamk_partition(c, g):
    """The stream-K kernel's own range arithmetic is consistent: every K step of the cut belongs to exactly one workgroup,
    workgroups w0 .. w1 of a tile are exactly those whose range meets it, each piece lies in the slab the fix-up reads."""
    nt, full, nk, R, rg = _sk(c, g)
    P = P_MI355X
    rem = nt - full * P
    assert rg[0][0] == 0 and rg[-1][1] == R and all(rg[b][1] == rg[b + 1][0] for b in range(P - 1))
    assert all(n in (0, 1, 2) for _, _, _, n in rg)
    for t in range(rem):
        w0, w1, second = streamk_fixup(t, nk, R)
        meets = [b for b, (beg, end, _, _) in enumerate(rg) if max(beg, t * nk) < min(end, (t + 1) * nk)]
        assert meets == list(range(w0, w1 + 1)), (t, w0, w1, meets)
        for w in meets:
            assert t - rg[w][2] == (second if w == w0 else 0), (t, w)      # slab 2 w + (t - t0)


# ---- the table
def _mk():
    cases = []

    def add(family, entry, variant, form, M, N, K, kid, claims=(), defects=(), **kw):
        cases.append(Case(entry, variant, form, M, N, K, kid, claims=tuple(claims), defects=tuple(defects), family=family, **kw))

    NN, NT, TN, TT = (0, 0), (0, 1), (1, 0), (1, 1)

    # ---------------- gemm_f32_kernel (register-staged; any K, any alignment; the only fp32 kernel with a T/T form)
    f = "f32_reg"
    for K, what in ((1, "1"), (15, "BK-1"), (16, "BK"), (17, "BK+1"), (31, "2BK-1"), (33, "2BK+1")):
        add(f, "f32", 1, NT, 129, 127, K, K_F32, [("K", what), ("M", "tile+1"), ("N", "tile-1")],
            ["ragged_k_dropped"] if K % 16 else ["partial_col_tile", "rows_past_m"])
    add(f, "f32", 1, NN, 128, 132, 32, K_F32, [("nk", 2), ("M", "tile"), ("N", "tile+4"), ("b_kmajor",)], ["partial_col_tile"])
    add(f, "f32", 1, TN, 4, 4, 48, K_F32, [("nk", 3), ("M", "4"), ("N", "4"), ("a_kmajor",)], ["rows_past_m"])
    add(f, "f32", 1, TT, 1, 129, 33, K_F32, [("tt",), ("M", "1"), ("N", "tile+1")], ["ragged_k_dropped", "rows_past_m"])
    add(f, "f32", 1, TT, 127, 1, 16, K_F32, [("tt",), ("M", "tile-1"), ("N", "1")], ["rows_past_m"])
    add(f, "f32", 0, NT, 130, 126, 40, K_F32, [("vec_mismatch",), ("ptr_4mod16",), ("dword",)], ["ragged_k_dropped"], a_off=1)
    add(f, "f32", 0, NN, 126, 130, 24, K_F32, [("vec_mismatch",), ("ptr_4mod16",), ("dword",)], ["ragged_k_dropped"], b_off=1)
    add(f, "f32", 0, TN, 131, 125, 19, K_F32, [("dword",), ("a_kmajor",)], ["ragged_k_dropped"], pad=1)
    add(f, "f32", 1, NT, 1152 - 3, 7 * 128 - 5, 16, K_F32, [("tiles_mod8", 7), ("tilesM", 1)], ["tile_order_xcd", "tile_order_group"])
    add(f, "f32", 1, NN, 17 * 128 - 4, 9 * 128 - 4, 16, K_F32, [("tiles_mod8", 1), ("tilesM", 2)], ["tile_order_xcd", "tile_order_group"])
    add(f, "f32", 1, NT, 130, 131, 100, K_F32, [("last_slice_short",), ("last_slice_ragged",), ("inkernel_reduce",)],
        ["ragged_k_dropped", "slice_plus", "slice_minus", "last_slice_full", "reduce_omits_last", "bias_per_slice",
         "acc_per_slice"], splitk=3, acc=True)
    add(f, "f32", 1, TT, 5, 7, 48, K_F32, [("splitk_recomputed", 3), ("tt",)], ["reduce_omits_last", "slice_plus"], splitk=64)
    add(f, "f32", 1, NT, 9, 130, 64, K_F32, [("batch",), ("inkernel_reduce",)], ["batch_slabs0", "batch_operand0"], splitk=2, batch=2)
    add(f, "f32", 1, NT, 40, 36, 16, K_F32, [("sigmoid",), ("accumulate",)], ["sigmoid_before_acc", "bias_per_slice"], kind="sigmoid",
        act=1, acc=True)
    add(f, "f32", 1, NN, 33, 40, 64, K_F32, [("sigmoid",), ("inkernel_reduce",)], ["sigmoid_before_acc", "acc_per_slice"], kind="sigmoid",
        act=1, acc=True, splitk=2)

    # ---------------- the 128 x 128 LDS-DMA kernels: gemm_f32_kernel_dma<128> (variant 3), _split3 (variant 2), and _pl3
    for f, v, kid in (("f32_dma", 3, K_DMA), ("f32_split3", 2, K_SPLIT)):
        for n in (1, 2, 3):
            add(f, "f32", v, (NT, NN, TN)[n - 1], 132, 124, 16 * n, kid, [("nk", n), ("nk_ring+1",)] if n == 3 else [("nk", n)],
                ["slice_minus"] if n > 1 else ["partial_col_tile"], splitk=1)
        add(f, "f32", v, NT, 1, 129, 16, kid, [("M", "1"), ("N", "tile+1")], ["rows_past_m", "partial_col_tile"])
        add(f, "f32", v, NT, 127, 1, 32, kid, [("M", "tile-1"), ("N", "1")], ["rows_past_m"])
        add(f, "f32", v, TN, 4, 132, 16, kid, [("M", "4"), ("N", "tile+4"), ("a_kmajor",)], ["kmajor_clamp", "rows_past_m"])
        add(f, "f32", v, TN, 132, 4, 32, kid, [("M", "tile+4"), ("N", "4"), ("a_kmajor",), ("b_kmajor",)], ["kmajor_clamp"])
        add(f, "f32", v, NN, 129, 132, 16, kid, [("N", "tile+4"), ("M", "tile+1"), ("b_kmajor",)], ["kmajor_clamp", "partial_col_tile"])
        add(f, "f32", v, NN, 128, 128, 16, kid, [("M", "tile"), ("N", "tile")], ["rows_past_m"])
        add(f, "f32", v, TN, 1152 - 4, 7 * 128 - 4, 16, kid, [("tiles_mod8", 7), ("tilesM", 1)], ["tile_order_xcd", "tile_order_group"])
        add(f, "f32", v, NT, 17 * 128 - 3, 9 * 128 - 1, 16, kid, [("tiles_mod8", 1), ("tilesM", 2)], ["tile_order_xcd", "tile_order_group"])
        add(f, "f32", v, NT, 130, 131, 112, kid, [("last_slice_short",), ("inkernel_reduce",)],
            ["slice_plus", "slice_minus", "last_slice_full", "reduce_omits_last", "bias_per_slice", "acc_per_slice"], splitk=3, acc=True)
        add(f, "f32", v, NN, 20, 132, 48, kid, [("splitk_recomputed", 3)], ["reduce_omits_last"], splitk=64)
        add(f, "f32", v, TN, 132, 260, 64, kid, [("batch_inter",), ("inkernel_reduce",)], ["batch_slabs0", "batch_operand0"],
            splitk=2, batch=2, inter=True, bias=False)
        add(f, "f32", v, NT, 40, 36, 16, kid, [("sigmoid",), ("accumulate",)], ["sigmoid_before_acc"], kind="sigmoid", act=1, acc=True)
    f = "pl3"
    for n in (1, 2, 3):
        add(f, "pl3", 0, TN, 132, 124, 16 * n, K_PL3, [("nk", n)], ["slice_minus"] if n > 1 else ["partial_col_tile"])
    add(f, "pl3", 0, TN, 1, 129, 16, K_PL3, [("M", "1"), ("N", "tile+1")], ["rows_past_m", "partial_col_tile"])
    add(f, "pl3", 0, TN, 4, 1, 32, K_PL3, [("M", "4"), ("N", "1")], ["rows_past_m"])
    add(f, "pl3", 0, TN, 132, 127, 16, K_PL3, [("M", "tile+4"), ("N", "tile-1")], ["partial_col_tile"])
    add(f, "pl3", 0, TN, 128, 128, 16, K_PL3, [("M", "tile"), ("N", "tile")], ["rows_past_m"])
    add(f, "pl3", 0, TN, 1152 - 3, 7 * 128 - 5, 16, K_PL3, [("tiles_mod8", 7), ("tilesM", 1)], ["tile_order_xcd", "tile_order_group"])
    add(f, "pl3", 0, TN, 17 * 128 - 1, 9 * 128 - 2, 16, K_PL3, [("tiles_mod8", 1), ("tilesM", 2)], ["tile_order_xcd", "tile_order_group"])
    add(f, "pl3", 0, TN, 130, 131, 112, K_PL3, [("last_slice_short",), ("inkernel_reduce",)],
        ["slice_plus", "slice_minus", "last_slice_full", "reduce_omits_last", "acc_per_slice"], splitk=3, acc=True)
    add(f, "pl3", 0, TN, 20, 132, 48, K_PL3, [("splitk_recomputed", 3)], ["reduce_omits_last"], splitk=64)
    add(f, "pl3", 0, TN, 136, 264, 64, K_PL3, [("batch_inter",), ("inkernel_reduce",)], ["batch_slabs0", "batch_operand0"],
        splitk=2, batch=2, inter=True)

    # ---------------- sign phases: _split3 and _pl3 (unsplit and sliced), _planes in its three forms (unsplit only)
    f = "sign"
    for K, q in ((752, 0), (768, 12), (784, 13), (1520, 24), (1536, 12)):
        cl = [("flip_q", q), ("nks", K // 16)]
        add(f, "f32", 2, (NT, NN, TN, NT, NN)[(K // 16) % 5], 132, 124, K, K_SPLIT, cl, ["slice_minus"])
        add(f, "pl3", 0, TN, 132, 124, K, K_PL3, cl, ["slice_minus"])
        for form in (NT, NN, TN):
            add(f, "f32", 9, form, 260, 132, K, K_PLANES, cl, ["slice_minus"])
    for K, s, cl in ((1792, 5, [("flip_q", 14), ("slice_midstretch",), ("ends_negative",)]),
                     (1536, 8, [("flip_q", 12), ("slice_all_negative",), ("ends_negative",)])):
        for form in (NT, NN, TN):
            add(f, "f32", 2, form, 132, 124, K, K_SPLIT, cl + [("inkernel_reduce",)], ["phase_operand_local", "final_not_negated"], splitk=s)
        add(f, "pl3", 0, TN, 132, 124, K, K_PL3, cl + [("inkernel_reduce",)], ["phase_operand_local", "final_not_negated"], splitk=s)
    # the same products on operands whose mid / low pieces carry weight: ragged == zero-padded bit for bit, pl3 == split3 T/N
    for K, s in ((784, 1), (1792, 5), (1536, 8)):
        d = ["phase_operand_local"] if s > 1 else ["slice_minus"]
        add("embed", "f32", 2, TN, 132, 124, K, K_SPLIT, [("flip_q", flip_quarter(K))], d, kind="embed", splitk=s, bias=False)
        add("embed", "pl3", 0, TN, 132, 124, K, K_PL3, [("flip_q", flip_quarter(K))], d, kind="embed", splitk=s)
    for form in (NT, NN):
        add("embed", "f32", 2, form, 129, 132, 784, K_SPLIT, [("flip_q", 13)], ["kmajor_clamp" if form == NN else "partial_col_tile"],
            kind="embed")
    for form in (NT, NN, TN):
        add("embed", "f32", 9, form, 260, 132, 784, K_PLANES, [("flip_q", 13), ("M", "260")], ["kmajor_clamp" if form != NT else "rows_past_m"],
            kind="embed")
    add("embed", "f32", 3, NN, 129, 132, 80, K_DMA, [("b_kmajor",)], ["kmajor_clamp"], kind="embed")
    add("embed", "f32", 4, TN, 260, 132, 80, K_WIDE, [("a_kmajor",)], ["kmajor_clamp"], kind="embed")
    add("embed", "mm", 0, (1, 1), 260, 132, 192, K_BF2, [("a_kmajor",)], ["partial_col_tile"], kind="embed", bias=False)

    # ---------------- the 256-row kernels: gemm_f32_kernel_dma<256> (variant 4) and gemm_f32_kernel_planes (variant 9)
    for f, v, kid in (("f32_wide", 4, K_WIDE), ("f32_planes", 9, K_PLANES)):
        is_wide = kid == K_WIDE
        for n in (1, 2, 3, 4, 5):
            add(f, "f32", v, (NT, NN, TN)[n % 3], 260, 132, 16 * n, kid, [("nk", n)] + ([("nk_ring+1",)] if n == KERNELS[kid]["ring"] + 1 else []),
                ["slice_minus"] if n > 1 else ["partial_col_tile"])
        add(f, "f32", v, NT, 256, 128, 16, kid, [("M", "256"), ("N", "tile")], ["rows_past_m"])
        add(f, "f32", v, TN, 260, 132, 64, kid, [("M", "260"), ("a_kmajor",), ("N", "tile+4")], ["kmajor_clamp", "partial_col_tile"])
        add(f, "f32", v, NN, 516, 132, 32, kid, [("M", "516"), ("b_kmajor",), ("N", "tile+4")], ["kmajor_clamp", "rows_past_m"])
        if is_wide:      # (the planes kernel takes N >= 128 only)
            add(f, "f32", v, NT, 257, 1, 16, kid, [("M", "tile+1"), ("N", "1")], ["rows_past_m"])
            add(f, "f32", v, TN, 256, 4, 16, kid, [("N", "4"), ("b_kmajor",)], ["kmajor_clamp"])
        else:
            add(f, "f32", v, NT, 257, 129, 16, kid, [("M", "tile+1"), ("N", "tile+1")], ["rows_past_m", "partial_col_tile"])
        add(f, "f32", v, TN, 5 * 256 - 4, 3 * 128 - 4, 16, kid, [("tiles_mod8", 7), ("tilesM", 1)], ["tile_order_xcd", "tile_order_group"])
        add(f, "f32", v, NT, 9 * 256 - 3, 9 * 128 - 1, 16, kid, [("tiles_mod8", 1), ("tilesM", 2)], ["tile_order_xcd", "tile_order_group"])
        add(f, "f32", v, NT, 300, 136, 16, kid, [("sigmoid",), ("accumulate",)], ["sigmoid_before_acc"], kind="sigmoid", act=1, acc=True)
    f = "f32_wide"
    add(f, "f32", 4, NT, 258, 131, 112, K_WIDE, [("last_slice_short",), ("inkernel_reduce",)],
        ["slice_plus", "slice_minus", "last_slice_full", "reduce_omits_last", "bias_per_slice", "acc_per_slice"], splitk=3, acc=True)
    add(f, "f32", 4, NN, 256, 132, 48, K_WIDE, [("splitk_recomputed", 3)], ["reduce_omits_last"], splitk=64)
    add(f, "f32", 4, TN, 260, 132, 64, K_WIDE, [("batch_inter",), ("inkernel_reduce",)], ["batch_slabs0", "batch_operand0"],
        splitk=2, batch=2, inter=True, bias=False)

    # ---------------- bf::gemm_bf16_kernel (fp32 operands rounded on their way into LDS; any K; always splitk_reduce_kernel)
    f = "bf16_reg"
    for K, what in ((1, "1"), (31, "BK-1"), (32, "BK"), (33, "BK+1"), (63, "2BK-1"), (65, "2BK+1")):
        add(f, "bf16", 0, (NT, TN, NN, TT, NT, NN)[K % 6], 129, 127 if K % 2 else 128, K, K_BF16, [("K", what), ("M", "tile+1")],
            ["ragged_k_dropped"] if K % 32 else ["rows_past_m"])
    add(f, "bf16", 0, TN, 4, 132, 96, K_BF16, [("nk", 3), ("nk_ring+1",), ("M", "4"), ("N", "tile+4")], ["partial_col_tile"])
    add(f, "bf16", 0, TT, 1, 1, 64, K_BF16, [("nk", 2), ("tt",), ("M", "1"), ("N", "1")], ["rows_past_m"])
    add(f, "bf16", 0, NT, 1152 - 3, 7 * 128 - 5, 32, K_BF16, [("tiles_mod8", 7), ("tilesM", 1)], ["tile_order_xcd", "tile_order_group"])
    add(f, "bf16", 0, NN, 17 * 128 - 4, 9 * 128 - 4, 32, K_BF16, [("tiles_mod8", 1), ("tilesM", 2)], ["tile_order_xcd", "tile_order_group"])
    add(f, "bf16", 0, NT, 130, 131, 200, K_BF16, [("last_slice_short",), ("last_slice_ragged",), ("scalar_reduce",)],
        ["ragged_k_dropped", "slice_plus", "slice_minus", "last_slice_full", "reduce_omits_last", "bias_per_slice", "acc_per_slice"],
        splitk=3, acc=True, ldc_pad=3)
    add(f, "bf16", 0, TT, 5, 8, 96, K_BF16, [("splitk_recomputed", 3), ("reduce_kernel",)], ["reduce_omits_last"], splitk=64)
    add(f, "bf16", 0, NT, 9, 130, 128, K_BF16, [("batch",), ("reduce_kernel",)], ["batch_slabs0", "batch_operand0"], splitk=2, batch=2)
    add(f, "bf16", 0, NT, 40, 36, 32, K_BF16, [("sigmoid",), ("accumulate",)], ["sigmoid_before_acc"], kind="sigmoid", act=1, acc=True,
        splitk=1)
    add(f, "bf16", 0, NN, 40, 37, 64, K_BF16, [("sigmoid",), ("scalar_reduce",)], ["sigmoid_before_acc", "acc_per_slice"], kind="sigmoid",
        act=1, acc=True, splitk=2, ldc_pad=3)

    # ---------------- bf2::gemm_bf16_nt_kernel<128 | 256> (bf16 operands in memory; always splitk_reduce_kernel)
    f = "bf2"
    RR, RK, KR, KK = (0, 0), (0, 1), (1, 0), (1, 1)
    for n in (1, 2, 3):
        add(f, "mm", 0, (RR, RK, KR)[n - 1], 260, 132, 64 * n, K_BF2, [("nk", n)] + ([("nk_ring+1",)] if n == 3 else []),
            ["slice_minus"] if n > 1 else ["partial_col_tile"])
    add(f, "mm", 0, RR, 1, 129, 64, K_BF2, [("M", "1"), ("N", "tile+1")], ["rows_past_m", "partial_col_tile"])
    add(f, "mm", 0, KK, 4, 4, 64, K_BF2, [("M", "4"), ("N", "4"), ("a_kmajor",), ("b_kmajor",)], ["rows_past_m"])
    add(f, "mm", 0, KK, 260, 132, 128, K_BF2, [("M", "tile+4"), ("N", "tile+4"), ("a_kmajor",), ("b_kmajor",)], ["partial_col_tile"])
    add(f, "mm", 0, KR, 255, 127, 64, K_BF2, [("M", "tile-1"), ("N", "tile-1")], ["rows_past_m"])
    add(f, "mm", 0, RK, 256, 128, 64, K_BF2, [("M", "tile"), ("N", "tile")], ["rows_past_m"])
    add(f, "mm", 0, RR, 9 * 256 - 3, 7 * 128 - 5, 64, K_BF2, [("tiles_mod8", 7), ("tilesM", 1)], ["tile_order_xcd", "tile_order_group"])
    add(f, "mm", 0, KK, 17 * 256 - 4, 9 * 128 - 4, 64, K_BF2, [("tiles_mod8", 1), ("tilesM", 2)], ["tile_order_xcd", "tile_order_group"])
    add(f, "mm", 0, RR, 258, 131, 448, K_BF2, [("last_slice_short",), ("scalar_reduce",)],
        ["slice_plus", "slice_minus", "last_slice_full", "reduce_omits_last", "bias_per_slice", "acc_per_slice"], splitk=3, acc=True, ldc_pad=3)
    add(f, "mm", 0, KK, 20, 132, 192, K_BF2, [("splitk_recomputed", 3), ("reduce_kernel",)], ["reduce_omits_last"], splitk=64)
    add(f, "mm", 0, KK, 264, 136, 128, K_BF2, [("batch_inter",), ("reduce_kernel",)], ["batch_slabs0", "batch_operand0"],
        splitk=2, batch=2, inter=True, bias=False)
    add(f, "mm", 0, RR, 40, 36, 64, K_BF2, [("sigmoid",), ("accumulate",)], ["sigmoid_before_acc"], kind="sigmoid", act=1, acc=True)

    # the 256-wide instantiation takes a launch of >= 512 tiles x slices x batch entries only: small tile counts times a batch
    # (and two K slices where that keeps C small)
    f = "bf2_wide"
    for n in (1, 2, 3):
        add(f, "mm", 0, (RR, RK, KR)[n - 1], 260, 1028, 64 * n, K_BF2_WIDE, [("nk", n)] + ([("nk_ring+1",)] if n == 3 else []),
            ["slice_minus"] if n > 1 else ["partial_col_tile"], batch=52)
    add(f, "mm", 0, KK, 256, 256, 128, K_BF2_WIDE, [("M", "tile"), ("N", "tile")], ["rows_past_m", "batch_operand0"], batch=256, splitk=2, bias=False)
    add(f, "mm", 0, KK, 1, 1028, 64, K_BF2_WIDE, [("M", "1"), ("a_kmajor",)], ["rows_past_m", "partial_col_tile"], batch=103)
    add(f, "mm", 0, KK, 4, 1025, 64, K_BF2_WIDE, [("M", "4"), ("a_kmajor",), ("b_kmajor",)], ["rows_past_m", "partial_col_tile"], batch=103)
    add(f, "mm", 0, RR, 255, 1279, 128, K_BF2_WIDE, [("M", "tile-1")], ["rows_past_m", "partial_col_tile"], batch=52, splitk=2)
    add(f, "mm", 0, KR, 257, 1281, 64, K_BF2_WIDE, [("M", "tile+1")], ["rows_past_m", "partial_col_tile"], batch=43)
    add(f, "mm", 0, KK, 260, 1284, 128, K_BF2_WIDE, [("M", "tile+4"), ("a_kmajor",), ("b_kmajor",)], ["partial_col_tile"], batch=43)
    add(f, "mm", 0, RK, 9 * 256 - 3, 7 * 256 - 5, 128, K_BF2_WIDE, [("tiles_mod8", 7), ("tilesM", 1)], ["tile_order_xcd", "tile_order_group"],
        batch=5, splitk=2, bias=False)
    add(f, "mm", 0, KK, 17 * 256 - 4, 9 * 256 - 4, 128, K_BF2_WIDE, [("tiles_mod8", 1), ("tilesM", 2)], ["tile_order_xcd", "tile_order_group"],
        batch=2, splitk=2, bias=False)
    add(f, "mm", 0, RR, 258, 1027, 448, K_BF2_WIDE, [("last_slice_short",), ("scalar_reduce",)],
        ["slice_plus", "slice_minus", "last_slice_full", "reduce_omits_last", "bias_per_slice", "acc_per_slice", "batch_slabs0"],
        splitk=3, acc=True, ldc_pad=3, batch=18)
    add(f, "mm", 0, KK, 20, 1028, 192, K_BF2_WIDE, [("splitk_recomputed", 3), ("reduce_kernel",)], ["reduce_omits_last"], splitk=64, batch=35)
    add(f, "mm", 0, RR, 40, 1028, 64, K_BF2_WIDE, [("sigmoid",), ("accumulate",)], ["sigmoid_before_acc"], kind="sigmoid", act=1, acc=True,
        batch=103)

    # ---------------- chooser thresholds (each side; every case also goes through the data check)
    f = "chooser"
    for M, side in ((256, True), (252, False)):      # planes needs M >= 256
        add(f, "f32", 9, TN, M, 128, 16, K_PLANES if side else K_SPLIT, [("thr", "M>=256", side)])
        add(f, "f32", 4, NN, M, 128, 16, K_WIDE if side else K_DMA, [("thr", "M>=256", side)])
    for N, side in ((128, True), (124, False)):
        add(f, "f32", 9, NN, 256, N, 16, K_PLANES if side else K_SPLIT, [("thr", "N>=128", side)])
    for N, side in ((192 * 128, True), (191 * 128, False)):
        add(f, "f32", 0, NT, 256, N, 16, K_PLANES if side else K_SPLIT, [("thr", "tiles256x128>=192", side)])
    for (M, N), side in (((4096, 1024), True), ((4092, 1024), False), ((4096, 1020), False)):
        add(f, "f32", 8, NN, M, N, 16, K_WIDE if side else K_DMA, [("thr", "large", side)])
    add(f, "f32", 8, NT, 4096, 1024, 16, K_WIDE, [("thr", "large", True)])
    add(f, "f32", 8, NT, 4092, 1024, 16, K_F32, [("thr", "large", False)])      # large N/T products run register-staged
    # (rows stay 16-byte aligned on the false side too -- lda = 132 -- so that only the tile dimension decides)
    for M, side in ((132, True), (130, False)):
        add(f, "f32", 0, TN, M, 128, 16, K_SPLIT if side else K_F32, [("thr", "M%4==0", side), ("a_kmajor",)], pad=(4 if side else 2, 4))
    for N, side in ((132, True), (130, False)):
        add(f, "f32", 3, NN, 128, N, 16, K_DMA if side else K_F32, [("thr", "N%4==0", side), ("b_kmajor",)], pad=(4, 4 if side else 2))
    for N, side in ((8192, True), (7936, False)):
        add(f, "mm", 0, RR, 4096, N, 64, K_BF2_WIDE if side else K_BF2, [("thr", "tiles>=512", side)], bias=False)
    add(f, "mm", 0, RK, 4096, 8196, 64, K_BF2_WIDE, [("thr", "cols256", True), ("thr", "tiles>=512", True)], bias=False)
    add(f, "mm", 0, RK, 256 * 128, 1020, 64, K_BF2, [("thr", "cols256", False)], bias=False)
    add(f, "mm", 0, RR, 2048, 1020, 512, K_BF2, [("thr", "cols256", False)], ws=True)      # ... of the stream-K use
    # (40 tiles: 7 K steps each would still give every workgroup one, so that nk >= 8 alone refuses the cut)
    add(f, "f32", 6, NT, 10240, 256, 128, K_STREAMK, [("thr", "nk>=8", True), ("thr", "rem*nk>=P", True)], ws=True)
    add(f, "f32", 6, NT, 10240, 256, 112, K_WIDE, [("thr", "nk>=8", False), ("sk_refused", 7)], ws=True)
    add(f, "f32", 6, NN, 256 * 31, 256, 128, K_WIDE, [("thr", "rem*nk>=P", False), ("sk_refused", 8)], ws=True)
    add(f, "mm", 0, RR, 10240, 256, 512, K_BF2_STREAMK, [("thr", "nk>=8", True), ("thr", "rem*nk>=P", True)], ws=True)
    add(f, "mm", 0, RR, 10240, 256, 448, K_BF2, [("thr", "nk>=8", False), ("sk_refused", 7)], ws=True)
    add(f, "mm", 0, KK, 256 * 31, 256, 512, K_BF2, [("thr", "rem*nk>=P", False), ("sk_refused", 8)], ws=True)

    # ---------------- stream-K at P = 256 workgroups (256-CU devices only): the smallest cuts the chooser allows
    for f, entry, v, kid, bk, forms, refused in (("streamk_f32", "f32", 6, K_STREAMK, 16, (NT, NN, TN), K_WIDE),
                                                 ("streamk_bf16", "mm", 0, K_BF2_STREAMK, 64, (RR, RK, KK), K_BF2)):
        add(f, entry, v, forms[0], 256, 256, 256 * bk, kid, [("sk_one_step_each",)], ["sk_ticket", "sk_first_piece"], ws=True, acc=True)
        add(f, entry, v, forms[1], 256, 256, 257 * bk, kid, [("sk_ranges_1_2",)], ["sk_ticket"], ws=True)
        add(f, entry, v, forms[2], 256, 256, 255 * bk, refused, [("sk_refused", 255)], ["slice_minus"], ws=True)
        add(f, entry, v, forms[0], 1280, 256, 64 * bk, kid, [("sk_two_tiles",), ("sk_first_piece_second",)], ["sk_first_piece", "sk_ticket"],
            ws=True)
        add(f, entry, v, forms[2], 256, 1028, 64 * bk, kid, [("sk_two_tiles",), ("sk_first_piece_second",), ("a_kmajor",), ("b_kmajor",)],
            ["sk_first_piece", "rows_past_m", "partial_col_tile"], ws=True, acc=True)
        # the tile-order map under a cut (the cases above are a single row or column of tiles).  A small grid, all of it cut:
        # 5 x 3 tiles of nk = 20 (fp32), 9 x 2 of nk = 16 (bf16) -- XCD runs of two lengths, a last group of one tile row walked
        # over several tile columns, a ragged M
        Mg, Ng, nkg = (1280 - 4, 768 - 4, 20) if kid == K_STREAMK else (2304 - 4, 512, 16)
        add(f, entry, v, forms[2 if kid == K_STREAMK else 1], Mg, Ng, nkg * bk, kid,
            [("sk_cut", cdiv(Mg, 256) * cdiv(Ng, 256), 0), ("nk", nkg), ("xcd_remainder",), ("ragged_group",), ("tilesM", 1), ("ragged_m",),
             ("b_kmajor",)], ["tile_order_xcd", "tile_order_group", "sk_ticket"], ws=True)
        # ... and one whole data-parallel round in front of the cut: 19 x 15 = 285 tiles of nk = 10, 29 of them cut (290 K steps
        # over 256 workgroups).  (The GPU test forms the reference of a product this size as a float64 product on the device:
        # exact for these operand ranges -- expected_image.)
        add(f, entry, v, forms[0 if kid == K_STREAMK else 2], 4864 - 4, 3840 - 4, 10 * bk, kid,
            [("sk_cut", 285, 1), ("nk", 10), ("xcd_remainder",), ("ragged_group",), ("ragged_m",), ("sk_two_tiles",)],
            ["tile_order_xcd", "tile_order_group", "sk_ticket"], ws=True)
    return tuple(cases)


CASES = _mk()
FAMILIES = tuple(dict.fromkeys(c.family for c in CASES))
STREAMK_FAMILIES = ("streamk_f32", "streamk_bf16")


def needs_256_cus(c):
    """The claimed id depends on the stream-K cut (P = 256): the case runs only on a 256-CU device."""
    return c.ws


def claims_hold(c):
    """[] or the list of claims of case c that fail (the claimed kernel id first)."""
    g = geometry(c)
    bad = []
    if g["kid"] != c.kid:
        bad.append(("kid", g["kid"]))
    for cl in c.claims:
        if not PREDICATES[cl[0]](c, g, *cl[1:]):
            bad.append(cl)
    if g["cut"] is not None:
        check_streamk_partition(c, g)
    return bad


for _c in CASES:       # asserted at import: a case that does not reach what it claims is a mistake in this table
    assert not claims_hold(_c), (_c.name, claims_hold(_c))
assert len({c.name for c in CASES}) == len(CASES), [c.name for c in CASES if [d.name for d in CASES].count(c.name) > 1]


# ------------------------------------------------------------------------------------------------ operands
SCALES = {"exact": (3, 2, 5), "sigmoid": (3, 3, 6)}     # a = ia 2^-ea, b = ib 2^-eb, bias / C0 / results in units of 2^-(ea + eb)
UNIT_LIMIT = 1 << 22


def operand_range(K):
    return 8 if K <= 4096 else 4


def seed_of(c):
    return (c.M * 131 + c.N * 17 + c.K * 7 + c.splitk * 3 + c.batch + KERNELS[c.kid]["bk"]) & 0x7fffffff


def int_operands(c):
    """(ia (batch, M, K), ib (batch, K, N), ibias (batch, N) or None, ic0 (batch, M, N) or None) as float64 integers, and the
    asserted bound sum |a||b| + |bias| + |C0| <= 2^22 units."""
    rng = np.random.default_rng(seed_of(c))
    r = operand_range(c.K)
    ia = rng.integers(-r, r + 1, (c.batch, c.M, c.K)).astype(np.float64)
    ib = rng.integers(-r, r + 1, (c.batch, c.K, c.N)).astype(np.float64)
    sig = c.kind == "sigmoid"
    ibias = rng.integers(-40, 41, (c.batch, c.N)).astype(np.float64) if (c.bias and c.entry != "pl3") else None
    ic0 = rng.integers(-60 if sig else -1000, 61 if sig else 1001, (c.batch, c.M, c.N)).astype(np.float64) if c.acc else None
    bound = r * r * c.K + (40 if ibias is not None else 0) + (1000 if ic0 is not None else 0)
    assert bound <= UNIT_LIMIT, (c.name, bound)
    return ia, ib, ibias, ic0


def embed_operands(c):
    """Gaussian operands scaled element-wise by 2^(-20 .. 20), float32 (A (batch, M, K), B (batch, K, N), bias or None)."""
    rng = np.random.default_rng(seed_of(c) + 1)
    sc = lambda shape: np.exp2(rng.integers(-20, 21, shape).astype(np.float64))
    A = (rng.standard_normal((c.batch, c.M, c.K)) * sc((c.batch, c.M, c.K))).astype(np.float32)
    B = (rng.standard_normal((c.batch, c.K, c.N)) * sc((c.batch, c.K, c.N))).astype(np.float32)
    if c.entry == "mm":      # bf16 operands in memory: representable values
        A = (A.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
        B = (B.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    bias = rng.standard_normal((c.batch, c.N)).astype(np.float32) if (c.bias and c.entry != "pl3") else None
    return A, B, bias


def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-x))


SIGMOID_ATOL = 2e-6          # the project's gate on sk_sigmoid (tests/test_gpu_kernels.py)

DEFECTS = ("ragged_k_dropped", "slice_plus", "slice_minus", "last_slice_full", "partial_col_tile", "rows_past_m", "kmajor_clamp",
           "tile_order_xcd", "tile_order_group", "reduce_omits_last", "batch_slabs0", "bias_per_slice", "acc_per_slice",
           "sigmoid_before_acc", "phase_operand_local", "final_not_negated", "sk_first_piece", "sk_ticket", "batch_operand0")


def reference(c, ops=None, defect=None):
    """The image of C the launch must leave: (batch, M + GUARD_ROWS, ldc) float64, NaN where the sentinel (or, without
    accumulate, the NaN prefill) must survive.  Exact cases: the integer product times 2^-5; sigmoid cases: the fp64 sigmoid of the
    exact pre-activation.  defect: the same computed by a kernel or host code with the named defect (DEFECTS) -- a model of the
    mistake's effect on the result at the granularity of K steps, slices, tiles, pieces and batch entries."""
    g = geometry(c)
    ia, ib, ibias, ic0 = ops if ops is not None else int_operands(c)
    ea, eb, eu = SCALES[c.kind if c.kind in SCALES else "exact"]
    unit = 2.0 ** -eu
    M, N, K, bk = c.M, c.N, c.K, g["bk"]
    tm, tn = g["tile"]
    img = np.full((c.batch, M + GUARD_ROWS, g["ldc"]), np.nan)
    slices = list(g["slices"])
    nsl = len(slices)
    if defect == "ragged_k_dropped":
        slices[-1] = (slices[-1][0], slices[-1][1] // bk * bk)
    elif defect == "slice_plus":          # every later slice starts one K step late
        slices = [(kb + (bk if s else 0), ke) for s, (kb, ke) in enumerate(slices)]
        if nsl == 1:
            slices = [(0, max(0, K - bk))]
    elif defect == "slice_minus":         # ... one K step early (the step is added twice); unsplit: the last step twice
        slices = [(kb - (bk if s else 0), ke) for s, (kb, ke) in enumerate(slices)]
        if nsl == 1:
            slices = [(0, K), (max(0, (K - 1) // bk * bk), K)]
    elif defect == "last_slice_full":     # the last slice runs kchunk long: it reads past K (modelled: the rows wrap)
        slices[-1] = (slices[-1][0], slices[-1][0] + g["kchunk"])
    parts = np.zeros((c.batch, len(slices), M, N))
    for z in range(c.batch):
        A, B = ia[0 if (defect == "batch_operand0" and z) else z], ib[z]
        if defect == "kmajor_clamp":      # the last four dims of a k-major operand come from the four in front of them
            if c.a_kmajor:
                A = A.copy()
                A[M - 4:] = A[M - 8:M - 4] if M >= 8 else np.nan
            if c.b_kmajor:
                B = B.copy()
                B[:, N - 4:] = B[:, N - 8:N - 4] if N >= 8 else np.nan
        for s, (kb, ke) in enumerate(slices):
            idx = np.arange(kb, ke) % K
            As, Bs = A[:, idx], B[idx, :]
            if defect in ("phase_operand_local", "final_not_negated") and g["flip_q"]:
                steps = np.arange(kb, ke) // 16
                glob = np.array([sign_of_step(g["flip_q"], k) for k in steps], np.float64)
                if defect == "phase_operand_local":
                    # the two uses of the phase disagree: the B operand's sign follows the slice's local step, the accumulators'
                    # sign the global one.  (A phase that is local in BOTH uses -- one SignPhase started at step 0 in every slice --
                    # is the same sum in exact arithmetic and no model on integers can show it: it moves only the direction in
                    # which the bf16 MFMA truncates.  test_gpu_gemm_cases.py sees it per kernel and form on operands whose pieces
                    # round: test_sliced_split_product_is_the_sum_of_its_slices_formed_unsplit, and test_pl3_equals_split3_bit_for_bit.)
                    loc = np.array([sign_of_step(g["flip_q"], k - kb // 16) for k in steps], np.float64)
                    Bs = Bs * (glob * loc)[:, None]
                    parts[z, s] = As @ Bs
                else:
                    parts[z, s] = (As @ Bs) * glob[-1]
            else:
                parts[z, s] = As @ Bs
    # stream-K: the tile's pieces through the slabs
    lost = np.zeros((M, N), bool)          # elements whose tile is never stored
    if g["cut"] is not None and defect in ("sk_first_piece", "sk_ticket"):
        nt, full, nk, R, rg = _sk(c, g)
        for t in range(nt - full * P_MI355X):
            w0, w1, second = streamk_fixup(t, nk, R)
            v = xcd_map(full * P_MI355X + t, nt)
            tr, tc = group_map(v, g["tilesM"], g["tilesN"], g["group"])
            rs, cs = slice(tr * tm, min(M, (tr + 1) * tm)), slice(tc * tn, min(N, (tc + 1) * tn))
            if defect == "sk_ticket":       # the ticket before the last one taken for the last: a lone contributor never stores,
                lost[rs, cs] = True         # several: the fix-up reads a slab whose piece has not been written (NaN-filled)
            else:                           # slab 2 w0 + (1 - second): the other tile's piece, or a slab never written
                if rg[w0][3] == 2:
                    beg, end = rg[w0][0], rg[w0][1]
                    other = t - 1 if second else t + 1
                    kb, ke = max(beg, other * nk) - other * nk, min(end, (other + 1) * nk) - other * nk
                    mb, me = max(beg, t * nk) - t * nk, min(end, (t + 1) * nk) - t * nk
                    vo = xcd_map(full * P_MI355X + other, nt)
                    otr, otc = group_map(vo, g["tilesM"], g["tilesN"], g["group"])
                    A, B = ia[0], ib[0]
                    Ao = np.zeros((tm, K))
                    Bo = np.zeros((K, tn))
                    ra, cb = A[otr * tm:(otr + 1) * tm], B[:, otc * tn:(otc + 1) * tn]
                    Ao[:ra.shape[0]], Bo[:, :cb.shape[1]] = ra, cb
                    wrong = Ao[:, kb * bk:ke * bk] @ Bo[kb * bk:ke * bk, :]
                    right = A[rs, mb * bk:me * bk] @ B[mb * bk:me * bk, cs]
                    parts[0, 0, rs, cs] += wrong[:rs.stop - rs.start, :cs.stop - cs.start] - right
                else:
                    parts[0, 0, rs, cs] = np.nan
    for z in range(c.batch):
        sl = parts[0 if (defect == "batch_slabs0" and z) else z]
        if defect == "reduce_omits_last" and sl.shape[0] > 1:
            sl = sl[:-1]
        tot = sl.sum(axis=0)
        nrep = nsl if nsl > 1 else 2       # an unsplit launch: the defect's effect shown as a second application
        if ibias is not None:
            tot = tot + ibias[z][None, :] * (nrep if defect == "bias_per_slice" else 1)
        val = tot * unit
        if c.act == 1 and defect == "sigmoid_before_acc":
            val = sigmoid64(val)
        if ic0 is not None:
            val = val + ic0[z] * unit * (nrep if defect == "acc_per_slice" else 1)
        if c.act == 1 and defect != "sigmoid_before_acc":
            val = sigmoid64(val)
        if ic0 is not None:
            img[z, :M, :N] = ic0[z] * unit          # what the launch finds there
        stored = np.ones((M, N), bool) & ~lost
        if defect in ("tile_order_xcd", "tile_order_group"):
            seen = set()
            for b in range(g["tiles"]):
                seen.add(tile_of_block(b, g["tilesM"], g["tilesN"], g["group"], defect))
            stored[:] = False
            for tr, tc in seen:
                if tr < g["tilesM"] and tc < g["tilesN"]:
                    stored[tr * tm:(tr + 1) * tm, tc * tn:(tc + 1) * tn] = True
        if defect == "partial_col_tile" and N % tn:
            stored[:, N // tn * tn:] = False
        img[z, :M, :N] = np.where(stored, val, img[z, :M, :N])
        if defect == "rows_past_m":        # the clamped edge row stored once more behind the matrix
            img[z, M, :N] = val[M - 1]
    return img


def differs(a, b, atol=0.0):
    """Elements at which two images differ (NaN equals NaN)."""
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b) > atol
    return (d | (np.isnan(a) != np.isnan(b))) & ~both_nan


def cheap(c):
    """Small enough for the numpy reference (the GPU test forms the larger ones on the device)."""
    return c.batch * c.M * c.N * c.K <= (1 << 29)


def padded_shape(c):
    """The embedding of a ragged product: the same operands zero-padded to whole 256 x 256 tiles."""
    return cdiv(c.M, 256) * 256, cdiv(c.N, 256) * 256


# ------------------------------------------------------------------------------------------------ what the older tests reach
# the GEMM parametrize lists of tests/test_gpu_kernels.py, by test function (test_gemm_cases.py checks them against that file's
# marks, so that the report cannot drift from it)
_F, _T = False, True
OLDER_SHAPES = {
    "test_gemm_matches_fp64": [
        (300, 200, 257, _F, _T), (256, 256, 64, _F, _F), (256, 256, 64, _T, _F), (256, 256, 64, _F, _T), (256, 256, 64, _T, _T),
        (130, 514, 96, _F, _T), (1000, 72, 1, _F, _F), (129, 131, 300, _T, _F), (64, 1792, 514, _F, _F), (300, 260, 512, _F, _T),
        (300, 260, 528, _F, _F), (132, 516, 1024, _T, _F), (1000, 772, 1792, _F, _T), (517, 1792, 3584, _F, _F),
        (1028, 132, 2048, _T, _F), (1, 4, 16, _F, _T), (4, 4, 16, _T, _F)],
    "test_gemm_exact_bf16_split_is_an_fp32_product": [
        (300, 260, 512, _F, _T), (300, 260, 528, _F, _F), (132, 516, 1024, _T, _F), (1000, 772, 1792, _F, _T),
        (517, 1792, 3584, _F, _F), (1028, 132, 2048, _T, _F), (4, 4, 16, _T, _F)],
    "test_gemm_bf16_equals_fp32_product_of_rounded_operands": [
        (300, 200, 257, _F, _T), (256, 256, 64, _F, _F), (256, 256, 64, _T, _F), (256, 256, 64, _F, _T), (256, 256, 64, _T, _T),
        (130, 514, 96, _F, _T), (1000, 72, 1, _F, _F), (129, 131, 300, _T, _F), (64, 1792, 514, _F, _F), (257, 384, 1000, _T, _F)],
    "test_gemm_splitk_is_deterministic_and_matches_fp64": [
        (300, 260, 5000, 5), (140, 257, 3000, 3), (129, 64, 4096, 0), (132, 64, 4096, 0), (300, 260, 4096, 4), (140, 260, 3008, 1)],
    "test_gemm_dma_kernels_forced": [
        (300, 260, 512, _F, _T, 1), (700, 260, 528, _F, _F, 1), (516, 132, 1024, _T, _F, 1), (1000, 772, 1792, _F, _T, 1),
        (517, 1792, 3584, _F, _F, 2), (1028, 132, 4096, _T, _F, 4), (256, 128, 16, _F, _T, 1), (1030, 1796, 528, _F, _F, 1),
        (772, 516, 1040, _T, _F, 1), (256, 256, 32, _F, _T, 1)],
    "test_gemm_stream_k_kernel": [
        (1000, 772, 1792, _F, _T), (4352, 4096, 256, _F, _T), (5000, 3800, 528, _F, _F), (3800, 5000, 528, _T, _F),
        (4096, 4096, 64, _F, _T), (300, 260, 64, _F, _T)],
    "test_gemm_split_kernels_of_the_large_products": [
        (1400, 1300, 1792, _F, _T), (1030, 772, 3584, _F, _F), (1028, 516, 2048, _T, _F), (256, 128, 16, _F, _T),
        (4352, 4096, 256, _F, _F), (300, 260, 64, _T, _F), (260, 132, 80, _F, _F), (260, 132, 112, _T, _F), (516, 260, 96, _F, _T)],
    "test_gemm_bf16_nt_equals_fp64_product_of_rounded_operands": [
        (256, 256, 64), (300, 200, 257), (1000, 771, 1792), (513, 1300, 320), (50, 7168, 128)],
    "test_gemm_bf16_k_major_operands_equal_fp64_product_of_rounded_operands": [
        (512, 512, 256, 1, 1), (771, 1792, 1280, 1, 0), (7168, 257, 1024, 1, 4), (300, 130, 192, 2, 1), (3584, 896, 640, 2, 2),
        (1000, 1800, 128, 1, 1)],
    "test_gemm_bf16_stream_k_kernel": [(1000, 772 + 512, 1792), (4352, 4096, 512), (5000, 3800, 1088), (4096, 4096, 512)],
    "test_gemm_on_operands_that_arrive_split_is_bit_for_bit_the_split_kernel": [
        (512, 272, 1280, 1, 1), (514, 384, 2048, 1, 3), (256, 128, 1024, 2, 2), (300, 260, 64, 1, 1), (1024, 512, 12800, 1, 5),
        (3584, 896, 1600, 2, 0)],
}
OLDER_SHAPE_ARGS = {      # the argnames of the shape list of each test (its other parametrize marks are variants / forms)
    "test_gemm_matches_fp64": "M,N,K,tA,tB", "test_gemm_exact_bf16_split_is_an_fp32_product": "M,N,K,tA,tB",
    "test_gemm_bf16_equals_fp32_product_of_rounded_operands": "M,N,K,tA,tB",
    "test_gemm_splitk_is_deterministic_and_matches_fp64": "M,N,K,S", "test_gemm_dma_kernels_forced": "M,N,K,tA,tB,S",
    "test_gemm_stream_k_kernel": "M,N,K,tA,tB", "test_gemm_split_kernels_of_the_large_products": "M,N,K,tA,tB",
    "test_gemm_bf16_nt_equals_fp64_product_of_rounded_operands": "M,N,K",
    "test_gemm_bf16_k_major_operands_equal_fp64_product_of_rounded_operands": "M,N,K,batch,splitk",
    "test_gemm_bf16_stream_k_kernel": "M,N,K", "test_gemm_on_operands_that_arrive_split_is_bit_for_bit_the_split_kernel": "M,N,K,batch,splitk",
}


def _older_suite():
    """The GEMM launches of tests/test_gpu_kernels.py as Cases (dense operands; a split count chosen at run time is counted at 1,
    2, 4 and 8), to tell which (kernel, boundary) pairs of the table above run for the first time."""
    out = []
    S = OLDER_SHAPES

    def add(entry, variant, form, M, N, K, splitk=1, batch=1, **kw):
        for s in ((1, 2, 4, 8) if splitk == 0 else (splitk,)):
            out.append(Case(entry, variant, (int(form[0]), int(form[1])), M, N, K, 0, splitk=s, batch=batch, **kw))

    for M, N, K, a, b in S["test_gemm_matches_fp64"]:
        add("f32", 0, (a, b), M, N, K)
    for M, N, K, a, b in S["test_gemm_bf16_equals_fp32_product_of_rounded_operands"]:
        add("bf16", 0, (a, b), M, N, K)
    for M, N, K, a, b in S["test_gemm_exact_bf16_split_is_an_fp32_product"]:
        for v in (2, 0):
            add("f32", v, (a, b), M, N, K)
    for M, N, K, s in S["test_gemm_splitk_is_deterministic_and_matches_fp64"]:      # both entries, T/N, the dW_hh layout
        add("f32", 0, (1, 0), M, N, K, s, 2, inter=True, acc=True)
        add("bf16", 0, (1, 0), M, N, K, s, 2, inter=True, acc=True)
    for v in (3, 4):
        for M, N, K, a, b, s in S["test_gemm_dma_kernels_forced"]:
            add("f32", v, (a, b), M, N, K, s)
    for M, N, K, a, b in S["test_gemm_stream_k_kernel"]:
        add("f32", 6, (a, b), M, N, K, ws=True)
    for v in (2, 9):
        for M, N, K, a, b in S["test_gemm_split_kernels_of_the_large_products"]:
            add("f32", v, (a, b), M, N, K)
    for M, N, K in S["test_gemm_bf16_nt_equals_fp64_product_of_rounded_operands"]:      # (K padded to the K step with zeros)
        add("mm", 0, (0, 0), M, N, cdiv(K, 64) * 64, act=1)
    for form in ((0, 1), (1, 0), (1, 1)):
        for M, N, K, batch, s in S["test_gemm_bf16_k_major_operands_equal_fp64_product_of_rounded_operands"]:
            add("mm", 0, form, M, N, K, s, batch)
    for form in ((0, 0), (0, 1), (1, 0), (1, 1)):
        for M, N, K in S["test_gemm_bf16_stream_k_kernel"]:
            add("mm", 0, form, M, N, K, ws=True)
    for M, N, K, batch, s in S["test_gemm_on_operands_that_arrive_split_is_bit_for_bit_the_split_kernel"]:
        add("pl3", 0, (1, 0), M, N, K, s, batch, inter=batch == 2)
        add("f32", 2, (1, 0), M, N, K, s, batch, inter=batch == 2)
    return out


@functools.lru_cache(maxsize=None)
def first_time_claims():
    """{case name: the claims of the case that no launch of the older suite satisfies on the same kernel}."""
    claims = {cl for c in CASES for cl in c.claims}
    reached = set()
    for o in _older_suite():
        g = geometry(o, dense=True)
        for cl in claims:
            try:
                if PREDICATES[cl[0]](o, g, *cl[1:]):
                    reached.add((g["kid"], cl))
            except (TypeError, ZeroDivisionError):      # a stream-K claim asked of a launch without a cut
                pass
    return {c.name: tuple(cl for cl in c.claims if (c.kid, cl) not in reached) for c in CASES}
