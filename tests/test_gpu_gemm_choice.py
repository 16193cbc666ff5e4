"""Which kernel each GEMM entry point launches (sk_gemm_last_kernel(), ids as include/sepkern.h lists them), pinned case by case.

The expected ids were recorded on an MI355X from the library as it was before the GEMM host code was unified: the launch
decisions (variant, form, alignment, K step, split-K, batch, stream-K workspace and its cut) must come out the same.  The
stream-K cut depends on the CU count, so the test runs only on a device with 256 CUs.  Every case has valid arguments and a
small K; only the kernel id is checked (the results are the business of test_gpu_kernels.py).
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

# name -> (M, N, K, pad): pad = 1 gives A rows one float longer than the operand (not 16-byte aligned)
F32_SHAPES = {"small": (256, 256, 256, 0), "large": (4096, 1536, 256, 0), "unaligned": (256, 256, 256, 1),
              "k264": (256, 256, 264, 0)}
F32_VARIANTS = (0, 1, 2, 3, 4, 6, 8, 9)
FORMS = ((0, 0), (0, 1), (1, 0), (1, 1))            # (transA, transB) or (a_kmajor, b_kmajor)
# (splitk, batch, stream-K workspace): splitk 4 always carries its split-K workspace
LAUNCHES = ((1, 1, False), (1, 1, True), (1, 2, False), (1, 2, True), (4, 1, False), (4, 2, False))

# shape -> variant -> one group per form (N/N N/T T/N T/T) of one hex digit per launch of LAUNCHES
F32_EXPECTED = {
    "small": {0: "222222 222222 222222 111111", 1: "111111 111111 111111 111111", 2: "222222 222222 222222 111111",
              3: "333333 333333 333333 111111", 4: "444444 444444 444444 111111", 6: "444444 444444 444444 111111",
              8: "333333 333333 333333 111111", 9: "aa2222 aa2222 aa2222 111111"},
    "large": {0: "aa2222 aa2222 aa2222 111111", 1: "111111 111111 111111 111111", 2: "222222 222222 222222 111111",
              3: "333333 333333 333333 111111", 4: "444444 444444 444444 111111", 6: "464444 464444 464444 111111",
              8: "464433 464411 333333 111111", 9: "aa2222 aa2222 aa2222 111111"},
    "unaligned": {v: "111111 111111 111111 111111" for v in F32_VARIANTS},
    "k264": {v: "111111 111111 111111 111111" for v in F32_VARIANTS},
}
# shape -> the same groups for sk_gemm_bf16_splitk
BF16_EXPECTED = {"small": "999999 999999 999999 999999", "large": "999999 999999 999999 999999"}
# sk_gemm_bf16_mm: (M, N, K, splitk, batch, stream-K workspace) -> one hex digit per form of FORMS
BF16MM_EXPECTED = {(512, 640, 128, 1, 1, False): "bbbb", (512, 512, 256, 4, 1, False): "bbbb",
                   (4096, 8192, 64, 1, 1, True): "cccc",        # the cut refused (1 K step): 256-wide tiles
                   (4096, 1536, 512, 1, 1, True): "dddd", (4096, 1536, 512, 1, 1, False): "bbbb"}
BF16MM_CASES = tuple(BF16MM_EXPECTED)
# sk_gemm_pl3_tn: (M, N, K, splitk, batch) -> id
PL3_EXPECTED = {(256, 512, 256, 1, 1): "e", (256, 512, 256, 4, 1): "e", (256, 512, 256, 1, 2): "e"}
PL3_CASES = tuple(PL3_EXPECTED)


def _lib():
    from sepkern import _lib as L
    return L


class _Bufs:
    """Zero-filled device buffers, one per role, grown on demand (the cases share them)."""

    def __init__(self):
        self.t = {}

    def get(self, role, nbytes, dtype=torch.float32):
        t = self.t.get(role)
        if t is None or t.numel() * t.element_size() < nbytes:
            esz = torch.empty(0, dtype=dtype).element_size()
            t = torch.zeros(-(-int(nbytes) // esz) + 64, dtype=dtype, device="cuda")
            self.t[role] = t
        return t

    def ws(self, lib, M, N, batch, splitk, streamk_ws):
        if splitk > 1:
            return self.get("ws_split", lib.sk_gemm_workspace_bytes(M, N, batch, splitk), torch.uint8)
        return self.get("ws_streamk", lib.sk_gemm_streamk_workspace_bytes(), torch.uint8) if streamk_ws else None


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32_launch(lib, bufs, entry, shape, form, launch, variant):
    M, N, K, pad = shape
    tA, tB = form
    splitk, batch, streamk_ws = launch
    lda, ldb = (M if tA else K) + pad, (K if tB else N)
    sA, sB, sC = (K if tA else M) * lda, (N if tB else K) * ldb, M * N
    A, B, Cm = bufs.get("A", 4 * batch * sA), bufs.get("B", 4 * batch * sB), bufs.get("C", 4 * batch * sC)
    ws = bufs.ws(lib, M, N, batch, splitk, streamk_ws)
    args = [_p(A), _p(B), _p(Cm), None, M, N, K, lda, ldb, N, tA, tB, 0, 0, batch, sA, sB, sC, 0, splitk, _p(ws)]
    _lib().call(entry, *(args + ([] if variant is None else [variant])), _stream())
    return lib.sk_gemm_last_kernel()


def f32_ids(bufs, entry="sk_gemm_f32_splitk", variants=F32_VARIANTS, shapes=F32_SHAPES):
    """{shape: {variant: "g g g g"}} for sk_gemm_f32_splitk; {shape: "g g g g"} for sk_gemm_bf16_splitk (variants=(None,))."""
    lib = _lib().load()
    out = {}
    for name, shape in shapes.items():
        row = {v: " ".join("".join("%x" % _f32_launch(lib, bufs, entry, shape, f, la, v) for la in LAUNCHES) for f in FORMS)
               for v in variants}
        out[name] = row[None] if variants == (None,) else row
    torch.cuda.synchronize()
    return out


def bf16mm_ids(bufs):
    lib = _lib().load()
    out = {}
    for case in BF16MM_CASES:
        M, N, K, splitk, batch, streamk_ws = case
        ids = ""
        for akm, bkm in FORMS:
            lda, ldb = ((M + 7) // 8 * 8 if akm else K), ((N + 7) // 8 * 8 if bkm else K)
            sA, sB = (K if akm else M) * lda, (K if bkm else N) * ldb
            A = bufs.get("A16", 2 * (batch * sA + lda), torch.bfloat16)
            B = bufs.get("B16", 2 * (batch * sB + ldb), torch.bfloat16)
            Cm = bufs.get("C", 4 * batch * M * N)
            ws = bufs.ws(lib, M, N, batch, splitk, streamk_ws)
            _lib().call("sk_gemm_bf16_mm", _p(A), _p(B), _p(Cm), None, M, N, K, lda, ldb, N, akm, bkm, 0, 0, batch, sA, sB,
                        M * N, 0, splitk, _p(ws), _stream())
            ids += "%x" % lib.sk_gemm_last_kernel()
        out[case] = ids
    torch.cuda.synchronize()
    return out


def pl3_ids(bufs):
    from sepkern import ops
    lib = _lib().load()
    out = {}
    for case in PL3_CASES:
        M, N, K, splitk, batch = case
        Apl = ops.split_rows(torch.zeros(K, batch * M, device="cuda"))
        Bpl = ops.split_rows(torch.zeros(K, batch * N, device="cuda"))
        Cm = bufs.get("C", 4 * batch * M * N)[:batch * M * N].view(batch * M, N)
        ops.gemm_pl3_tn(Apl, Bpl, Cm, M, N, K, batch=batch, sA=M, sB=N, sC=M * N, splitk=splitk, ws_tag="gemm_choice")
        out[case] = "%x" % lib.sk_gemm_last_kernel()
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def bufs():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    from sepkern import ops
    if ops.device_info()[0] != 256:
        pytest.skip("the recorded stream-K choices assume 256 CUs")
    return _Bufs()


def test_f32_splitk_kernel_choice(bufs):
    assert f32_ids(bufs) == F32_EXPECTED


def test_bf16_splitk_kernel_choice(bufs):
    assert f32_ids(bufs, "sk_gemm_bf16_splitk", (None,), {k: F32_SHAPES[k] for k in ("small", "large")}) == BF16_EXPECTED


def test_bf16_mm_kernel_choice(bufs):
    assert bf16mm_ids(bufs) == BF16MM_EXPECTED


def test_pl3_tn_kernel_choice(bufs):
    assert pl3_ids(bufs) == PL3_EXPECTED
