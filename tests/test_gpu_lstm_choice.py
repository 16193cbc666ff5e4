"""Which kernel, grid and launch count every sk_lstm_fwd / sk_lstm_bwd call takes (sk_lstm_last_launch(), include/sepkern.h),
pinned case by case.

The expected values were recorded on an MI355X from the library of commit 740d4f8, which had no such query: the case list below
ran against that build under a kernel trace, and each launch's demangled kernel name (it carries the template arguments), grid
and workgroup size were converted to the table once (G, which no trace shows, follows from the grid: the smallest allowed
number of batch groups per workgroup that gives it; the SK_EINVAL cases are the calls that returned -1 there and launched
nothing).  The same trace of the library with the query lists the same kernels with the same grids in the same order.  The
decisions -- mode decode, groups per workgroup, persistent or per step, the XCD-local form, the instantiation -- must come out
the same.  They depend on the CU count, so the test runs only on a device with 256 CUs.  T is 3 and the data is zero: only the
launch is checked (results are the business of test_gpu_kernels.py), and after every case the workspace's status word must be
clean.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

T = 3
HS = (256, 300, 600, 608, 612, 896, 900, 1024)
BS = (8, 16, 17, 32, 33, 100, 128)


def _cases():
    """(direction, H, B, launch kind, gmin, flavour, packed, exclusive, dh0 / dc0 wanted); flavour: f32, s3 (split3), tagged,
    s3+tagged, bf16, bf16+xl8, or an argument error: bit17 (forward), kind3, gmin9."""
    c = []
    for H in HS:                                            # every hidden size x batch size, the library's choice of launch
        for B in BS:
            c.append(("fwd", H, B, 0, 0, "f32", False, False, False))
            c.append(("bwd", H, B, 0, 0, "f32", False, False, True))
    for H, B in ((300, 8), (896, 32), (600, 100)):          # launch kinds 1 and 2, packed and padded
        for kind in (1, 2):
            c.append(("fwd", H, B, kind, 0, "f32", kind == 1, False, False))
            c.append(("bwd", H, B, kind, 0, "f32", kind == 1, False, True))
    c.append(("bwd", 896, 32, 2, 0, "f32", False, False, False))           # per step without the launch for dh0 / dc0
    for H, B in ((896, 32), (600, 100), (256, 128)):        # gmin 2
        c.append(("fwd", H, B, 0, 2, "f32", True, False, False))
        c.append(("bwd", H, B, 0, 2, "f32", True, False, True))
    c.append(("fwd", 600, 100, 2, 2, "f32", False, False, False))
    for H in HS:                                            # split3: H > 896 has no such instantiation and runs the plain product
        c.append(("fwd", H, 32, 0, 0, "s3", True, False, False))
    c.append(("fwd", 896, 32, 1, 0, "s3", False, False, False))
    c.append(("fwd", 600, 100, 2, 0, "s3", False, False, False))
    for H in (300, 896, 1024):                              # tagged; with split3 the split wins where it exists
        c.append(("fwd", H, 32, 0, 0, "tagged", True, False, False))
        c.append(("fwd", H, 32, 0, 0, "s3+tagged", False, False, False))
    c.append(("fwd", 1024, 32, 2, 0, "tagged", False, False, False))
    for H in (256, 600, 608, 612, 896, 900, 1024):          # bf16, ordinary form
        c.append(("fwd", H, 32, 0, 0, "bf16", True, False, False))
        c.append(("bwd", H, 32, 0, 0, "bf16", True, False, True))
    for H in (608, 612, 896, 900):                          # bf16 with the XCD-local form asked for: taken for 640 < H <= 896, B <= 32
        for B in (8, 32, 33):
            c.append(("fwd", H, B, 0, 0, "bf16+xl8", B != 8, False, False))
            c.append(("bwd", H, B, 0, 0, "bf16+xl8", B != 8, False, True))
    for kind, gmin in ((1, 0), (2, 0), (0, 2)):             # ... persistent launches with gmin <= 1 only
        c.append(("fwd", 896, 32, kind, gmin, "bf16+xl8", False, False, False))
        c.append(("bwd", 896, 32, kind, gmin, "bf16+xl8", False, False, True))
    c.append(("fwd", 896, 32, 0, 0, "f32+xl8", False, False, False))       # (the bit without bf16 changes nothing)
    for H, B, fl in ((896, 32, "f32"), (600, 100, "f32"), (300, 16, "f32"), (896, 32, "bf16"), (896, 32, "bf16+xl8")):
        c.append(("bwd", H, B, 0, 0, fl, True, True, True))                # backward, exclusive
    for d in ("fwd", "bwd"):                                # a grid that is not co-resident: per step, or SK_EINVAL when kind 1 insists
        c.append((d, 1024, 272, 0, 0, "f32", False, False, d == "bwd"))
        c.append((d, 1024, 272, 1, 0, "f32", False, False, d == "bwd"))
    c.append(("fwd", 896, 32, 0, 0, "bit17", False, False, False))         # argument errors: nothing is launched
    for d in ("fwd", "bwd"):
        c.append((d, 896, 32, 0, 0, "kind3", False, False, False))
        c.append((d, 896, 32, 0, 0, "gmin9", False, False, False))
    return tuple(c)


CASES = _cases()


def mode_word(case):
    from sepkern import ops
    d, H, B, kind, gmin, flavour, packed, exclusive, d0 = case
    # the engine's protocol fields ride along (map 1; forward: single poller), as in every product call
    m = kind | ops.lstm_gmin(gmin) | ops.lstm_variant_bits(False, 1, d == "fwd", split3="s3" in flavour, tagged="tagged" in flavour,
                                                           xl8="xl8" in flavour)
    m |= ops.LSTM_BF16 if "bf16" in flavour else 0
    m |= ops.LSTM_BWD_EXCLUSIVE if exclusive or flavour == "bit17" else 0
    if flavour == "kind3":
        m = (m & ~0xff) | 3
    if flavour == "gmin9":
        m |= ops.lstm_gmin(9)
    return m


class _Bufs:
    """Zero-filled device buffers, one per role, grown on demand (the cases share them)."""

    def __init__(self):
        self.t = {}

    def get(self, role, n, dtype=torch.float32):
        t = self.t.get(role)
        if t is None or t.numel() < n:
            t = torch.zeros(int(n) + 64, dtype=dtype, device="cuda")
            self.t[role] = t
        return C.c_void_p(t.data_ptr())


def launch(lib, bufs, case, mode):
    """One sk_lstm_fwd / sk_lstm_bwd call on zero data (uniform lengths T); returns (return code, workspace tensor)."""
    d, H, B, packed, d0 = case[0], case[1], case[2], case[6], case[8]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = bufs.get
    nws = lib.sk_lstm_workspace_bytes(T, B, H)
    f("ws", nws, torch.uint8)
    lens = bufs.t.get(("lens", B))
    if lens is None:
        lens = bufs.t[("lens", B)] = torch.full((B,), T, dtype=torch.int32, device="cuda")
        bufs.t[("offs", B)] = torch.arange(T + 1, dtype=torch.int32, device="cuda") * B
    lens_p = C.c_void_p(lens.data_ptr())
    offs_p = C.c_void_p(bufs.t[("offs", B)].data_ptr()) if packed else None
    TB, BH = T * B, 2 * B * H
    if d == "fwd":
        rc = lib.sk_lstm_fwd(f("gx", TB * 8 * H), f("whh", 8 * H * H), f("h0", BH), f("c0", BH), lens_p, offs_p, f("y", TB * 2 * H),
                             f("gates", TB * 8 * H), f("cs", TB * 2 * H), f("hn", BH), f("cn", BH), f("ws", nws, torch.uint8),
                             T, B, H, mode, st)
    else:
        rc = lib.sk_lstm_bwd(f("y", TB * 2 * H), None, None, f("whh", 8 * H * H), f("gates", TB * 8 * H), f("cs", TB * 2 * H),
                             f("c0", BH), lens_p, offs_p, f("gx", TB * 8 * H), f("hn", BH) if d0 else None, f("cn", BH) if d0 else None,
                             f("dbias", (B + 15) // 16 * 8 * H), None, 0, 0, f("ws", nws, torch.uint8), T, B, H, mode, st)
    return rc, bufs.t["ws"]


# case -> (launches, family, KS, bf16, packed, GM, exclusive, blocks, G), or -1 (SK_EINVAL, nothing launched)
EXPECTED = {
    ('fwd', 256, 8, 0, 0, 'f32', False, False, False): (1, 1, 20, 0, 0, 0, 0, 40, 1),
    ('bwd', 256, 8, 0, 0, 'f32', False, False, True): (1, 4, 20, 0, 0, 1, 0, 40, 1),
    ('fwd', 256, 16, 0, 0, 'f32', False, False, False): (1, 1, 20, 0, 0, 0, 0, 40, 1),
    ('bwd', 256, 16, 0, 0, 'f32', False, False, True): (1, 4, 20, 0, 0, 1, 0, 40, 1),
    ('fwd', 256, 17, 0, 0, 'f32', False, False, False): (1, 1, 20, 0, 0, 0, 0, 80, 1),
    ('bwd', 256, 17, 0, 0, 'f32', False, False, True): (1, 4, 20, 0, 0, 1, 0, 80, 1),
    ('fwd', 256, 32, 0, 0, 'f32', False, False, False): (1, 1, 20, 0, 0, 0, 0, 80, 1),
    ('bwd', 256, 32, 0, 0, 'f32', False, False, True): (1, 4, 20, 0, 0, 1, 0, 80, 1),
    ('fwd', 256, 33, 0, 0, 'f32', False, False, False): (1, 1, 20, 0, 0, 0, 0, 120, 1),
    ('bwd', 256, 33, 0, 0, 'f32', False, False, True): (1, 4, 20, 0, 0, 1, 0, 120, 1),
    ('fwd', 256, 100, 0, 0, 'f32', False, False, False): (1, 1, 20, 0, 0, 0, 0, 160, 2),
    ('bwd', 256, 100, 0, 0, 'f32', False, False, True): (1, 4, 20, 0, 0, 8, 0, 160, 2),
    ('fwd', 256, 128, 0, 0, 'f32', False, False, False): (1, 1, 20, 0, 0, 0, 0, 160, 2),
    ('bwd', 256, 128, 0, 0, 'f32', False, False, True): (1, 4, 20, 0, 0, 8, 0, 160, 2),
    ('fwd', 300, 8, 0, 0, 'f32', False, False, False): (1, 1, 20, 0, 0, 0, 0, 40, 1),
    ('bwd', 300, 8, 0, 0, 'f32', False, False, True): (1, 4, 20, 0, 0, 1, 0, 40, 1),
    ('fwd', 300, 16, 0, 0, 'f32', False, False, False): (1, 1, 20, 0, 0, 0, 0, 40, 1),
    ('bwd', 300, 16, 0, 0, 'f32', False, False, True): (1, 4, 20, 0, 0, 1, 0, 40, 1),
    ('fwd', 300, 17, 0, 0, 'f32', False, False, False): (1, 1, 20, 0, 0, 0, 0, 80, 1),
    ('bwd', 300, 17, 0, 0, 'f32', False, False, True): (1, 4, 20, 0, 0, 1, 0, 80, 1),
    ('fwd', 300, 32, 0, 0, 'f32', False, False, False): (1, 1, 20, 0, 0, 0, 0, 80, 1),
    ('bwd', 300, 32, 0, 0, 'f32', False, False, True): (1, 4, 20, 0, 0, 1, 0, 80, 1),
    ('fwd', 300, 33, 0, 0, 'f32', False, False, False): (1, 1, 20, 0, 0, 0, 0, 120, 1),
    ('bwd', 300, 33, 0, 0, 'f32', False, False, True): (1, 4, 20, 0, 0, 1, 0, 120, 1),
    ('fwd', 300, 100, 0, 0, 'f32', False, False, False): (1, 1, 20, 0, 0, 0, 0, 160, 2),
    ('bwd', 300, 100, 0, 0, 'f32', False, False, True): (1, 4, 20, 0, 0, 8, 0, 160, 2),
    ('fwd', 300, 128, 0, 0, 'f32', False, False, False): (1, 1, 20, 0, 0, 0, 0, 160, 2),
    ('bwd', 300, 128, 0, 0, 'f32', False, False, True): (1, 4, 20, 0, 0, 8, 0, 160, 2),
    ('fwd', 600, 8, 0, 0, 'f32', False, False, False): (1, 1, 38, 0, 0, 0, 0, 76, 1),
    ('bwd', 600, 8, 0, 0, 'f32', False, False, True): (1, 4, 38, 0, 0, 1, 0, 76, 1),
    ('fwd', 600, 16, 0, 0, 'f32', False, False, False): (1, 1, 38, 0, 0, 0, 0, 76, 1),
    ('bwd', 600, 16, 0, 0, 'f32', False, False, True): (1, 4, 38, 0, 0, 1, 0, 76, 1),
    ('fwd', 600, 17, 0, 0, 'f32', False, False, False): (1, 1, 38, 0, 0, 0, 0, 152, 1),
    ('bwd', 600, 17, 0, 0, 'f32', False, False, True): (1, 4, 38, 0, 0, 1, 0, 152, 1),
    ('fwd', 600, 32, 0, 0, 'f32', False, False, False): (1, 1, 38, 0, 0, 0, 0, 152, 1),
    ('bwd', 600, 32, 0, 0, 'f32', False, False, True): (1, 4, 38, 0, 0, 1, 0, 152, 1),
    ('fwd', 600, 33, 0, 0, 'f32', False, False, False): (1, 1, 38, 0, 0, 0, 0, 228, 1),
    ('bwd', 600, 33, 0, 0, 'f32', False, False, True): (1, 4, 38, 0, 0, 1, 0, 228, 1),
    ('fwd', 600, 100, 0, 0, 'f32', False, False, False): (1, 1, 38, 0, 0, 0, 0, 228, 3),
    ('bwd', 600, 100, 0, 0, 'f32', False, False, True): (1, 4, 38, 0, 0, 8, 0, 228, 3),
    ('fwd', 600, 128, 0, 0, 'f32', False, False, False): (1, 1, 38, 0, 0, 0, 0, 228, 3),
    ('bwd', 600, 128, 0, 0, 'f32', False, False, True): (1, 4, 38, 0, 0, 8, 0, 228, 3),
    ('fwd', 608, 8, 0, 0, 'f32', False, False, False): (1, 1, 38, 0, 0, 0, 0, 76, 1),
    ('bwd', 608, 8, 0, 0, 'f32', False, False, True): (1, 4, 38, 0, 0, 1, 0, 76, 1),
    ('fwd', 608, 16, 0, 0, 'f32', False, False, False): (1, 1, 38, 0, 0, 0, 0, 76, 1),
    ('bwd', 608, 16, 0, 0, 'f32', False, False, True): (1, 4, 38, 0, 0, 1, 0, 76, 1),
    ('fwd', 608, 17, 0, 0, 'f32', False, False, False): (1, 1, 38, 0, 0, 0, 0, 152, 1),
    ('bwd', 608, 17, 0, 0, 'f32', False, False, True): (1, 4, 38, 0, 0, 1, 0, 152, 1),
    ('fwd', 608, 32, 0, 0, 'f32', False, False, False): (1, 1, 38, 0, 0, 0, 0, 152, 1),
    ('bwd', 608, 32, 0, 0, 'f32', False, False, True): (1, 4, 38, 0, 0, 1, 0, 152, 1),
    ('fwd', 608, 33, 0, 0, 'f32', False, False, False): (1, 1, 38, 0, 0, 0, 0, 228, 1),
    ('bwd', 608, 33, 0, 0, 'f32', False, False, True): (1, 4, 38, 0, 0, 1, 0, 228, 1),
    ('fwd', 608, 100, 0, 0, 'f32', False, False, False): (1, 1, 38, 0, 0, 0, 0, 228, 3),
    ('bwd', 608, 100, 0, 0, 'f32', False, False, True): (1, 4, 38, 0, 0, 8, 0, 228, 3),
    ('fwd', 608, 128, 0, 0, 'f32', False, False, False): (1, 1, 38, 0, 0, 0, 0, 228, 3),
    ('bwd', 608, 128, 0, 0, 'f32', False, False, True): (1, 4, 38, 0, 0, 8, 0, 228, 3),
    ('fwd', 612, 8, 0, 0, 'f32', False, False, False): (1, 1, 56, 0, 0, 0, 0, 112, 1),
    ('bwd', 612, 8, 0, 0, 'f32', False, False, True): (1, 4, 56, 0, 0, 1, 0, 112, 1),
    ('fwd', 612, 16, 0, 0, 'f32', False, False, False): (1, 1, 56, 0, 0, 0, 0, 112, 1),
    ('bwd', 612, 16, 0, 0, 'f32', False, False, True): (1, 4, 56, 0, 0, 1, 0, 112, 1),
    ('fwd', 612, 17, 0, 0, 'f32', False, False, False): (1, 1, 56, 0, 0, 0, 0, 224, 1),
    ('bwd', 612, 17, 0, 0, 'f32', False, False, True): (1, 4, 56, 0, 0, 1, 0, 224, 1),
    ('fwd', 612, 32, 0, 0, 'f32', False, False, False): (1, 1, 56, 0, 0, 0, 0, 224, 1),
    ('bwd', 612, 32, 0, 0, 'f32', False, False, True): (1, 4, 56, 0, 0, 1, 0, 224, 1),
    ('fwd', 612, 33, 0, 0, 'f32', False, False, False): (1, 1, 56, 0, 0, 0, 0, 224, 2),
    ('bwd', 612, 33, 0, 0, 'f32', False, False, True): (1, 4, 56, 0, 0, 8, 0, 224, 2),
    ('fwd', 612, 100, 0, 0, 'f32', False, False, False): (1, 1, 56, 0, 0, 0, 0, 224, 4),
    ('bwd', 612, 100, 0, 0, 'f32', False, False, True): (1, 4, 56, 0, 0, 8, 0, 224, 4),
    ('fwd', 612, 128, 0, 0, 'f32', False, False, False): (1, 1, 56, 0, 0, 0, 0, 224, 4),
    ('bwd', 612, 128, 0, 0, 'f32', False, False, True): (1, 4, 56, 0, 0, 8, 0, 224, 4),
    ('fwd', 896, 8, 0, 0, 'f32', False, False, False): (1, 1, 56, 0, 0, 0, 0, 112, 1),
    ('bwd', 896, 8, 0, 0, 'f32', False, False, True): (1, 4, 56, 0, 0, 1, 0, 112, 1),
    ('fwd', 896, 16, 0, 0, 'f32', False, False, False): (1, 1, 56, 0, 0, 0, 0, 112, 1),
    ('bwd', 896, 16, 0, 0, 'f32', False, False, True): (1, 4, 56, 0, 0, 1, 0, 112, 1),
    ('fwd', 896, 17, 0, 0, 'f32', False, False, False): (1, 1, 56, 0, 0, 0, 0, 224, 1),
    ('bwd', 896, 17, 0, 0, 'f32', False, False, True): (1, 4, 56, 0, 0, 1, 0, 224, 1),
    ('fwd', 896, 32, 0, 0, 'f32', False, False, False): (1, 1, 56, 0, 0, 0, 0, 224, 1),
    ('bwd', 896, 32, 0, 0, 'f32', False, False, True): (1, 4, 56, 0, 0, 1, 0, 224, 1),
    ('fwd', 896, 33, 0, 0, 'f32', False, False, False): (1, 1, 56, 0, 0, 0, 0, 224, 2),
    ('bwd', 896, 33, 0, 0, 'f32', False, False, True): (1, 4, 56, 0, 0, 8, 0, 224, 2),
    ('fwd', 896, 100, 0, 0, 'f32', False, False, False): (1, 1, 56, 0, 0, 0, 0, 224, 4),
    ('bwd', 896, 100, 0, 0, 'f32', False, False, True): (1, 4, 56, 0, 0, 8, 0, 224, 4),
    ('fwd', 896, 128, 0, 0, 'f32', False, False, False): (1, 1, 56, 0, 0, 0, 0, 224, 4),
    ('bwd', 896, 128, 0, 0, 'f32', False, False, True): (1, 4, 56, 0, 0, 8, 0, 224, 4),
    ('fwd', 900, 8, 0, 0, 'f32', False, False, False): (1, 1, 64, 0, 0, 0, 0, 128, 1),
    ('bwd', 900, 8, 0, 0, 'f32', False, False, True): (1, 4, 64, 0, 0, 1, 0, 128, 1),
    ('fwd', 900, 16, 0, 0, 'f32', False, False, False): (1, 1, 64, 0, 0, 0, 0, 128, 1),
    ('bwd', 900, 16, 0, 0, 'f32', False, False, True): (1, 4, 64, 0, 0, 1, 0, 128, 1),
    ('fwd', 900, 17, 0, 0, 'f32', False, False, False): (1, 1, 64, 0, 0, 0, 0, 256, 1),
    ('bwd', 900, 17, 0, 0, 'f32', False, False, True): (1, 4, 64, 0, 0, 1, 0, 256, 1),
    ('fwd', 900, 32, 0, 0, 'f32', False, False, False): (1, 1, 64, 0, 0, 0, 0, 256, 1),
    ('bwd', 900, 32, 0, 0, 'f32', False, False, True): (1, 4, 64, 0, 0, 1, 0, 256, 1),
    ('fwd', 900, 33, 0, 0, 'f32', False, False, False): (1, 1, 64, 0, 0, 0, 0, 256, 2),
    ('bwd', 900, 33, 0, 0, 'f32', False, False, True): (1, 4, 64, 0, 0, 8, 0, 256, 2),
    ('fwd', 900, 100, 0, 0, 'f32', False, False, False): (1, 1, 64, 0, 0, 0, 0, 256, 4),
    ('bwd', 900, 100, 0, 0, 'f32', False, False, True): (1, 4, 64, 0, 0, 8, 0, 256, 4),
    ('fwd', 900, 128, 0, 0, 'f32', False, False, False): (1, 1, 64, 0, 0, 0, 0, 256, 4),
    ('bwd', 900, 128, 0, 0, 'f32', False, False, True): (1, 4, 64, 0, 0, 8, 0, 256, 4),
    ('fwd', 1024, 8, 0, 0, 'f32', False, False, False): (1, 1, 64, 0, 0, 0, 0, 128, 1),
    ('bwd', 1024, 8, 0, 0, 'f32', False, False, True): (1, 4, 64, 0, 0, 1, 0, 128, 1),
    ('fwd', 1024, 16, 0, 0, 'f32', False, False, False): (1, 1, 64, 0, 0, 0, 0, 128, 1),
    ('bwd', 1024, 16, 0, 0, 'f32', False, False, True): (1, 4, 64, 0, 0, 1, 0, 128, 1),
    ('fwd', 1024, 17, 0, 0, 'f32', False, False, False): (1, 1, 64, 0, 0, 0, 0, 256, 1),
    ('bwd', 1024, 17, 0, 0, 'f32', False, False, True): (1, 4, 64, 0, 0, 1, 0, 256, 1),
    ('fwd', 1024, 32, 0, 0, 'f32', False, False, False): (1, 1, 64, 0, 0, 0, 0, 256, 1),
    ('bwd', 1024, 32, 0, 0, 'f32', False, False, True): (1, 4, 64, 0, 0, 1, 0, 256, 1),
    ('fwd', 1024, 33, 0, 0, 'f32', False, False, False): (1, 1, 64, 0, 0, 0, 0, 256, 2),
    ('bwd', 1024, 33, 0, 0, 'f32', False, False, True): (1, 4, 64, 0, 0, 8, 0, 256, 2),
    ('fwd', 1024, 100, 0, 0, 'f32', False, False, False): (1, 1, 64, 0, 0, 0, 0, 256, 4),
    ('bwd', 1024, 100, 0, 0, 'f32', False, False, True): (1, 4, 64, 0, 0, 8, 0, 256, 4),
    ('fwd', 1024, 128, 0, 0, 'f32', False, False, False): (1, 1, 64, 0, 0, 0, 0, 256, 4),
    ('bwd', 1024, 128, 0, 0, 'f32', False, False, True): (1, 4, 64, 0, 0, 8, 0, 256, 4),
    ('fwd', 300, 8, 1, 0, 'f32', True, False, False): (1, 1, 20, 0, 1, 0, 0, 40, 1),
    ('bwd', 300, 8, 1, 0, 'f32', True, False, True): (1, 4, 20, 0, 1, 1, 0, 40, 1),
    ('fwd', 300, 8, 2, 0, 'f32', False, False, False): (3, 1, 20, 0, 0, 0, 0, 40, 1),
    ('bwd', 300, 8, 2, 0, 'f32', False, False, True): (4, 4, 20, 0, 0, 1, 0, 40, 1),
    ('fwd', 896, 32, 1, 0, 'f32', True, False, False): (1, 1, 56, 0, 1, 0, 0, 224, 1),
    ('bwd', 896, 32, 1, 0, 'f32', True, False, True): (1, 4, 56, 0, 1, 1, 0, 224, 1),
    ('fwd', 896, 32, 2, 0, 'f32', False, False, False): (3, 1, 56, 0, 0, 0, 0, 224, 1),
    ('bwd', 896, 32, 2, 0, 'f32', False, False, True): (4, 4, 56, 0, 0, 1, 0, 224, 1),
    ('fwd', 600, 100, 1, 0, 'f32', True, False, False): (1, 1, 38, 0, 1, 0, 0, 228, 3),
    ('bwd', 600, 100, 1, 0, 'f32', True, False, True): (1, 4, 38, 0, 1, 8, 0, 228, 3),
    ('fwd', 600, 100, 2, 0, 'f32', False, False, False): (3, 1, 38, 0, 0, 0, 0, 228, 3),
    ('bwd', 600, 100, 2, 0, 'f32', False, False, True): (4, 4, 38, 0, 0, 8, 0, 228, 3),
    ('bwd', 896, 32, 2, 0, 'f32', False, False, False): (3, 4, 56, 0, 0, 1, 0, 224, 1),
    ('fwd', 896, 32, 0, 2, 'f32', True, False, False): (1, 1, 56, 0, 1, 0, 0, 112, 2),
    ('bwd', 896, 32, 0, 2, 'f32', True, False, True): (1, 4, 56, 0, 1, 8, 0, 112, 2),
    ('fwd', 600, 100, 0, 2, 'f32', True, False, False): (1, 1, 38, 0, 1, 0, 0, 228, 3),
    ('bwd', 600, 100, 0, 2, 'f32', True, False, True): (1, 4, 38, 0, 1, 8, 0, 228, 3),
    ('fwd', 256, 128, 0, 2, 'f32', True, False, False): (1, 1, 20, 0, 1, 0, 0, 160, 2),
    ('bwd', 256, 128, 0, 2, 'f32', True, False, True): (1, 4, 20, 0, 1, 8, 0, 160, 2),
    ('fwd', 600, 100, 2, 2, 'f32', False, False, False): (3, 1, 38, 0, 0, 0, 0, 228, 3),
    ('fwd', 256, 32, 0, 0, 's3', True, False, False): (1, 2, 20, 0, 1, 0, 0, 80, 1),
    ('fwd', 300, 32, 0, 0, 's3', True, False, False): (1, 2, 20, 0, 1, 0, 0, 80, 1),
    ('fwd', 600, 32, 0, 0, 's3', True, False, False): (1, 2, 40, 0, 1, 0, 0, 160, 1),
    ('fwd', 608, 32, 0, 0, 's3', True, False, False): (1, 2, 40, 0, 1, 0, 0, 160, 1),
    ('fwd', 612, 32, 0, 0, 's3', True, False, False): (1, 2, 40, 0, 1, 0, 0, 160, 1),
    ('fwd', 896, 32, 0, 0, 's3', True, False, False): (1, 2, 56, 0, 1, 0, 0, 224, 1),
    ('fwd', 900, 32, 0, 0, 's3', True, False, False): (1, 1, 64, 0, 1, 0, 0, 256, 1),
    ('fwd', 1024, 32, 0, 0, 's3', True, False, False): (1, 1, 64, 0, 1, 0, 0, 256, 1),
    ('fwd', 896, 32, 1, 0, 's3', False, False, False): (1, 2, 56, 0, 0, 0, 0, 224, 1),
    ('fwd', 600, 100, 2, 0, 's3', False, False, False): (3, 2, 40, 0, 0, 0, 0, 240, 3),
    ('fwd', 300, 32, 0, 0, 'tagged', True, False, False): (1, 1, 20, 0, 1, 0, 0, 80, 1),
    ('fwd', 300, 32, 0, 0, 's3+tagged', False, False, False): (1, 2, 20, 0, 0, 0, 0, 80, 1),
    ('fwd', 896, 32, 0, 0, 'tagged', True, False, False): (1, 1, 56, 0, 1, 0, 0, 224, 1),
    ('fwd', 896, 32, 0, 0, 's3+tagged', False, False, False): (1, 2, 56, 0, 0, 0, 0, 224, 1),
    ('fwd', 1024, 32, 0, 0, 'tagged', True, False, False): (1, 1, 64, 0, 1, 0, 0, 256, 1),
    ('fwd', 1024, 32, 0, 0, 's3+tagged', False, False, False): (1, 1, 64, 0, 0, 0, 0, 256, 1),
    ('fwd', 1024, 32, 2, 0, 'tagged', False, False, False): (3, 1, 64, 0, 0, 0, 0, 256, 1),
    ('fwd', 256, 32, 0, 0, 'bf16', True, False, False): (1, 1, 20, 1, 1, 0, 0, 80, 1),
    ('bwd', 256, 32, 0, 0, 'bf16', True, False, True): (1, 4, 20, 1, 1, 1, 0, 80, 1),
    ('fwd', 600, 32, 0, 0, 'bf16', True, False, False): (1, 1, 40, 1, 1, 0, 0, 160, 1),
    ('bwd', 600, 32, 0, 0, 'bf16', True, False, True): (1, 4, 40, 1, 1, 1, 0, 160, 1),
    ('fwd', 608, 32, 0, 0, 'bf16', True, False, False): (1, 1, 40, 1, 1, 0, 0, 160, 1),
    ('bwd', 608, 32, 0, 0, 'bf16', True, False, True): (1, 4, 40, 1, 1, 1, 0, 160, 1),
    ('fwd', 612, 32, 0, 0, 'bf16', True, False, False): (1, 1, 40, 1, 1, 0, 0, 160, 1),
    ('bwd', 612, 32, 0, 0, 'bf16', True, False, True): (1, 4, 40, 1, 1, 1, 0, 160, 1),
    ('fwd', 896, 32, 0, 0, 'bf16', True, False, False): (1, 1, 56, 1, 1, 0, 0, 224, 1),
    ('bwd', 896, 32, 0, 0, 'bf16', True, False, True): (1, 4, 56, 1, 1, 1, 0, 224, 1),
    ('fwd', 900, 32, 0, 0, 'bf16', True, False, False): (1, 1, 64, 1, 1, 0, 0, 256, 1),
    ('bwd', 900, 32, 0, 0, 'bf16', True, False, True): (1, 4, 64, 1, 1, 1, 0, 256, 1),
    ('fwd', 1024, 32, 0, 0, 'bf16', True, False, False): (1, 1, 64, 1, 1, 0, 0, 256, 1),
    ('bwd', 1024, 32, 0, 0, 'bf16', True, False, True): (1, 4, 64, 1, 1, 1, 0, 256, 1),
    ('fwd', 608, 8, 0, 0, 'bf16+xl8', False, False, False): (1, 1, 40, 1, 0, 0, 0, 80, 1),
    ('bwd', 608, 8, 0, 0, 'bf16+xl8', False, False, True): (1, 4, 40, 1, 0, 1, 0, 80, 1),
    ('fwd', 608, 32, 0, 0, 'bf16+xl8', True, False, False): (1, 1, 40, 1, 1, 0, 0, 160, 1),
    ('bwd', 608, 32, 0, 0, 'bf16+xl8', True, False, True): (1, 4, 40, 1, 1, 1, 0, 160, 1),
    ('fwd', 608, 33, 0, 0, 'bf16+xl8', True, False, False): (1, 1, 40, 1, 1, 0, 0, 240, 1),
    ('bwd', 608, 33, 0, 0, 'bf16+xl8', True, False, True): (1, 4, 40, 1, 1, 1, 0, 240, 1),
    ('fwd', 612, 8, 0, 0, 'bf16+xl8', False, False, False): (1, 1, 40, 1, 0, 0, 0, 80, 1),
    ('bwd', 612, 8, 0, 0, 'bf16+xl8', False, False, True): (1, 4, 40, 1, 0, 1, 0, 80, 1),
    ('fwd', 612, 32, 0, 0, 'bf16+xl8', True, False, False): (1, 1, 40, 1, 1, 0, 0, 160, 1),
    ('bwd', 612, 32, 0, 0, 'bf16+xl8', True, False, True): (1, 4, 40, 1, 1, 1, 0, 160, 1),
    ('fwd', 612, 33, 0, 0, 'bf16+xl8', True, False, False): (1, 1, 40, 1, 1, 0, 0, 240, 1),
    ('bwd', 612, 33, 0, 0, 'bf16+xl8', True, False, True): (1, 4, 40, 1, 1, 1, 0, 240, 1),
    ('fwd', 896, 8, 0, 0, 'bf16+xl8', False, False, False): (1, 3, 56, 1, 0, 0, 0, 256, 1),
    ('bwd', 896, 8, 0, 0, 'bf16+xl8', False, False, True): (1, 5, 56, 1, 0, 0, 0, 256, 1),
    ('fwd', 896, 32, 0, 0, 'bf16+xl8', True, False, False): (1, 3, 56, 1, 1, 0, 0, 256, 1),
    ('bwd', 896, 32, 0, 0, 'bf16+xl8', True, False, True): (1, 5, 56, 1, 1, 0, 0, 256, 1),
    ('fwd', 896, 33, 0, 0, 'bf16+xl8', True, False, False): (1, 1, 56, 1, 1, 0, 0, 224, 2),
    ('bwd', 896, 33, 0, 0, 'bf16+xl8', True, False, True): (1, 4, 56, 1, 1, 8, 0, 224, 2),
    ('fwd', 900, 8, 0, 0, 'bf16+xl8', False, False, False): (1, 1, 64, 1, 0, 0, 0, 128, 1),
    ('bwd', 900, 8, 0, 0, 'bf16+xl8', False, False, True): (1, 4, 64, 1, 0, 1, 0, 128, 1),
    ('fwd', 900, 32, 0, 0, 'bf16+xl8', True, False, False): (1, 1, 64, 1, 1, 0, 0, 256, 1),
    ('bwd', 900, 32, 0, 0, 'bf16+xl8', True, False, True): (1, 4, 64, 1, 1, 1, 0, 256, 1),
    ('fwd', 900, 33, 0, 0, 'bf16+xl8', True, False, False): (1, 1, 64, 1, 1, 0, 0, 256, 2),
    ('bwd', 900, 33, 0, 0, 'bf16+xl8', True, False, True): (1, 4, 64, 1, 1, 8, 0, 256, 2),
    ('fwd', 896, 32, 1, 0, 'bf16+xl8', False, False, False): (1, 3, 56, 1, 0, 0, 0, 256, 1),
    ('bwd', 896, 32, 1, 0, 'bf16+xl8', False, False, True): (1, 5, 56, 1, 0, 0, 0, 256, 1),
    ('fwd', 896, 32, 2, 0, 'bf16+xl8', False, False, False): (3, 1, 56, 1, 0, 0, 0, 224, 1),
    ('bwd', 896, 32, 2, 0, 'bf16+xl8', False, False, True): (4, 4, 56, 1, 0, 1, 0, 224, 1),
    ('fwd', 896, 32, 0, 2, 'bf16+xl8', False, False, False): (1, 1, 56, 1, 0, 0, 0, 112, 2),
    ('bwd', 896, 32, 0, 2, 'bf16+xl8', False, False, True): (1, 4, 56, 1, 0, 8, 0, 112, 2),
    ('fwd', 896, 32, 0, 0, 'f32+xl8', False, False, False): (1, 1, 56, 0, 0, 0, 0, 224, 1),
    ('bwd', 896, 32, 0, 0, 'f32', True, True, True): (1, 4, 56, 0, 1, 8, 1, 224, 1),
    ('bwd', 600, 100, 0, 0, 'f32', True, True, True): (1, 4, 38, 0, 1, 8, 1, 228, 3),
    ('bwd', 300, 16, 0, 0, 'f32', True, True, True): (1, 4, 20, 0, 1, 8, 1, 40, 1),
    ('bwd', 896, 32, 0, 0, 'bf16', True, True, True): (1, 4, 56, 1, 1, 8, 1, 224, 1),
    ('bwd', 896, 32, 0, 0, 'bf16+xl8', True, True, True): (1, 5, 56, 1, 1, 0, 1, 256, 1),
    ('fwd', 1024, 272, 0, 0, 'f32', False, False, False): (3, 1, 64, 0, 0, 0, 0, 2176, 1),
    ('fwd', 1024, 272, 1, 0, 'f32', False, False, False): -1,
    ('bwd', 1024, 272, 0, 0, 'f32', False, False, True): (4, 4, 64, 0, 0, 1, 0, 2176, 1),
    ('bwd', 1024, 272, 1, 0, 'f32', False, False, True): -1,
    ('fwd', 896, 32, 0, 0, 'bit17', False, False, False): -1,
    ('fwd', 896, 32, 0, 0, 'kind3', False, False, False): -1,
    ('fwd', 896, 32, 0, 0, 'gmin9', False, False, False): -1,
    ('bwd', 896, 32, 0, 0, 'kind3', False, False, False): -1,
    ('bwd', 896, 32, 0, 0, 'gmin9', False, False, False): -1,
}


@pytest.fixture(scope="module")
def bufs():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    from sepkern import ops
    if ops.device_info()[0] != 256:
        pytest.skip("the recorded launch plans assume 256 CUs")
    return _Bufs()


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_recurrence_launch_choice(bufs, direction):
    from sepkern import _lib, ops
    lib = _lib.load()
    got = {}
    for case in CASES:
        if case[0] != direction:
            continue
        rc, ws = launch(lib, bufs, case, mode_word(case))
        n, q = ops.lstm_last_launch()
        if rc != 0:
            assert n == 0 and not any(q), (case, n, q)
            assert b"sk_lstm_" + direction.encode() in lib.sk_last_error(), (case, lib.sk_last_error())
        got[case] = (n,) + tuple(q) if rc == 0 else rc
        ops.lstm_status(ws)                                 # raises if a launch of this case timed out
    print(got)
    assert got == {c: e for c, e in EXPECTED.items() if c[0] == direction}
