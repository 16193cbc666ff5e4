"""The recurrence kernels of csrc/lstm.hip at their unit-group, batch-group and K edges: restated host code, an fp64 reference
with defect hooks, and the case table (tests/test_lstm_cases.py shows on any machine that the table can tell a wrong kernel
from a right one; tests/test_gpu_lstm_cases.py runs it on the device).  numpy only.

Restated from lstm.hip: pick_ks, groups_per_wg (256 CUs), decode_mode's rules for split3 / tagged / xl8, plan_launch, bwd_gm, the
launch count (with the backward's extra launch for dh0 / dc0 under step launches), BwdCfg::cnt and decode_block.  predict() gives
the 9-tuple (launches, family, KS, bf16, packed, GM, exclusive, blocks, G) that sk_lstm_last_launch() reports, or -1 (SK_EINVAL).

Layouts as the kernels take them: gx / gates / dgx (T, B, 2, 4H) gate-INTERLEAVED (4u + g), whh (2, 4H, H) and dbias
(rows, 2, 4H) gate-major (g H + u), y (T, B, 2H), c (T, B, 2, H), states (2, B, H).
"""
import dataclasses
import functools

import numpy as np

CUS, GMAX = 256, 8
# the mode word (include/sepkern.h, SK_LSTM_*)
AUTO, PERSISTENT, PER_STEP = 0, 1, 2
GMIN_SHIFT, BF16, BWD_EXCLUSIVE, MAP_SHIFT, POLL1, SPLIT3, TAGGED, XL8 = 8, 1 << 16, 1 << 17, 18, 1 << 20, 1 << 28, 1 << 29, 1 << 30
K_FWD, K_FWD_SPLIT3, K_FWD_XL8, K_BWD, K_BWD_XL8 = 1, 2, 3, 4, 5
F32_NSB, BF_NSB = 8, 4            # BwdCfg::NSB


# ------------------------------------------------------------------------------------ host code, restated
def pick_ks(H, bf=False):
    need = (H + 15) // 16
    for ks in (20, 40 if bf else 38, 56, 64):
        if ks >= need:
            return ks
    return 0


def decode_mode(backward, mode, H):
    """Mode of lstm.hip as a dict, or None where decode_mode returns SK_EINVAL."""
    kind, gmin = mode & 0xff, (mode >> GMIN_SHIFT) & 0xff
    if kind > PER_STEP or gmin > GMAX or (mode >> 31) != 0:
        return None
    bf, exclusive = bool(mode & BF16), bool(mode & BWD_EXCLUSIVE)
    if exclusive and not backward:
        return None
    s3 = (not backward) and bool(mode & SPLIT3) and not bf and pick_ks(H, True) != 64
    tagged = (not backward) and bool(mode & TAGGED) and not bf and not s3
    return dict(kind=kind, gmin=gmin, bf=bf, exclusive=exclusive, map=(mode >> MAP_SHIFT) & 3, s3=s3, tagged=tagged, xl8=bool(mode & XL8))


def groups_per_wg(NUG, NBG, gmin, cus=CUS):
    for g in range(max(1, gmin), GMAX + 1):
        if NUG * ((NBG + g - 1) // g) * 2 <= cus:
            return g
    return 0


def plan_launch(m, B, H, cus=CUS):
    KS = pick_ks(H, m["bf"] or m["s3"])
    NBG16 = (B + 15) // 16
    g = groups_per_wg(KS, NBG16, m["gmin"], cus)
    fits = g > 0
    persistent = m["kind"] == PERSISTENT or (m["kind"] == AUTO and fits)
    xl8 = m["xl8"] and m["bf"] and KS == 56 and B <= 32 and m["gmin"] <= 1 and cus >= 256 and persistent
    NBG = (B + 7) // 8 if xl8 else NBG16
    G = g if fits and not xl8 else 1
    nby = (NBG + G - 1) // G
    return dict(KS=KS, NBG=NBG, NBG16=NBG16, G=G, nby=nby, blocks=256 if xl8 else KS * nby * 2, fits=fits, persistent=persistent, xl8=xl8)


def bwd_gm(p, m):
    return 0 if p["xl8"] else 1 if p["G"] == 1 and not m["exclusive"] else GMAX


def predict(direction, T, B, H, mode, packed, want_d0=True):
    """What sk_lstm_last_launch() reports after the call: (launches, family, KS, bf16, packed, GM, exclusive, blocks, G); -1: SK_EINVAL."""
    backward = direction == "bwd"
    if not (T > 0 and B > 0 and H > 0 and H % 4 == 0 and H <= 1024):
        return -1
    m = decode_mode(backward, mode, H)
    if m is None:
        return -1
    p = plan_launch(m, B, H)
    if m["kind"] == PERSISTENT and not p["fits"]:
        return -1
    if backward:
        family, gm = (K_BWD_XL8 if p["xl8"] else K_BWD), bwd_gm(p, m)
        launches = 1 if p["persistent"] else T + int(bool(want_d0))
    else:
        family, gm = (K_FWD_XL8 if p["xl8"] else K_FWD_SPLIT3 if m["s3"] else K_FWD), 0
        launches = 1 if p["persistent"] else T
    return (launches, family, p["KS"], int(m["bf"]), int(bool(packed)), gm, int(m["exclusive"]), p["blocks"], p["G"])


def instantiation(direction, q):
    """The template instantiation a reported 9-tuple names."""
    _, family, KS, bf, packed, gm = q[:6]
    if family in (K_FWD, K_FWD_SPLIT3):
        return ("fwd", KS, bool(bf), family == K_FWD_SPLIT3, bool(packed))
    if family == K_FWD_XL8:
        return ("fwd_xl8", 56, bool(packed))
    return ("bwd", KS, bool(bf), gm) if family == K_BWD else ("bwd_xl8", 56)


ALL_INSTANTIATIONS = (
    {("fwd", ks, bf, False, pk) for bf in (False, True) for ks in (20, 40 if bf else 38, 56, 64) for pk in (False, True)}
    | {("fwd", ks, False, True, pk) for ks in (20, 40, 56) for pk in (False, True)}
    | {("fwd_xl8", 56, pk) for pk in (False, True)}
    | {("bwd", ks, bf, gm) for bf in (False, True) for ks in (20, 40 if bf else 38, 56, 64) for gm in (1, GMAX)} | {("bwd_xl8", 56)})
assert sum(i[0].startswith("fwd") for i in ALL_INSTANTIATIONS) == 24 and sum(i[0].startswith("bwd") for i in ALL_INSTANTIATIONS) == 17


def decode_block(L, NUG, nby, map_):
    """(unit group, workgroup row, direction) of linear block id L."""
    map_ &= 3
    S = nby * 2
    total = NUG * S
    x, j, per_xcd = L & 7, L >> 3, total >> 3
    if map_ == 1 and total % 8 == 0 and 8 % S == 0 and NUG % (8 // S) == 0:
        g = 8 // S
        stream, u = x // g, j * g + x % g
    elif (map_ == 2 and total % 8 == 0 and S % 2 == 0 and 8 % (S // 2) == 0 and (2 * NUG) % (8 // (S // 2)) == 0 and per_xcd % 2 == 0):
        g, half = 8 // (S // 2), per_xcd >> 1
        stream, u = 2 * (x // g) + (1 if j >= half else 0), (j % half) * g + x % g
    else:
        stream = L // NUG
        u = L - stream * NUG
    return u, stream % nby, stream // nby


def bwd_cfg(KS, bf):
    """BwdCfg<KS, BF>: chunks per wave, chunks per sub-block, cnt(sb) per sub-block, hidden units per chunk."""
    NQ = KS // 4 if bf else KS // 2
    NSB = BF_NSB if bf else F32_NSB
    SB = (NQ + NSB - 1) // NSB
    cnt = [0 if sb * SB >= NQ else SB if (sb + 1) * SB <= NQ else NQ - sb * SB for sb in range(NSB)]
    return dict(NQ=NQ, NSB=NSB, SB=SB, cnt=cnt, units=8 if bf else 4)


def fwd_chunk(bf16_image):
    return 32 if bf16_image else 16      # k per 1 KB chunk of the h image


# ------------------------------------------------------------------------------------ arithmetic
def rne_bf16(x):
    """fp64 -> fp32 -> bf16 (round to nearest even) -> fp64."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def to_gate_major(a, H):
    """(..., 4H) gate-interleaved -> gate-major."""
    return np.ascontiguousarray(np.swapaxes(a.reshape(a.shape[:-1] + (H, 4)), -1, -2)).reshape(a.shape)


def to_interleaved(a, H):
    return np.ascontiguousarray(np.swapaxes(a.reshape(a.shape[:-1] + (4, H)), -1, -2)).reshape(a.shape)


def _fwd_k_mask(H, KS, b16, defect):
    """Which k of the forward product a defect model leaves out (None: no K defect)."""
    keep = np.ones(H, dtype=bool)
    ch = fwd_chunk(b16)
    if defect == "drop_chunk":                       # the last chunk that holds a k < H is not multiplied
        c = (H - 1) // ch
        keep[c * ch:(c + 1) * ch] = False
    elif defect == "khalf_shift":                    # K half 1 starts one chunk late: its first chunk is left out
        k0 = 8 * KS
        keep[k0:k0 + ch] = False
    elif defect == "half_octet":                     # bf16 images: the second half-octet of the last whole octet read as zero
        k0 = H - 4 if H % 8 == 0 else H - 8
        keep[k0:k0 + 4] = False
    else:
        return None
    return keep


def _bwd_unit_mask(H, KS, bf, defect):
    """Which hidden units' dG (all four gates) the backward product leaves out under a defect model."""
    cfg = bwd_cfg(KS, bf)
    keep = np.ones(16 * KS, dtype=bool)
    per_wave, u = 2 * KS, cfg["units"]
    if defect == "drop_chunk":
        c = (H - 1) // u
        keep[c * u:(c + 1) * u] = False
    elif defect == "khalf_shift":                    # wave 1's eighth starts one chunk late
        keep[per_wave:per_wave + u] = False
    elif defect == "short_subblock":                 # every wave: the short last sub-block is not consumed
        sb = max(i for i, n in enumerate(cfg["cnt"]) if n > 0)
        for w in range(8):
            k0 = w * per_wave + sb * cfg["SB"] * u
            keep[k0:k0 + cfg["cnt"][sb] * u] = False
    else:
        return None
    return keep[:H]


def ref_forward(inp, bf=False, defect=None, plan=None):
    """The masked bidirectional recurrence in fp64; bf: the two product operands rounded to bf16.  Returns y, gates, c, hn, cn
    (padded layout; gates / c are NaN where no step ran, y is 0 there).  defect: see DEFECTS."""
    gx, whh, h0, c0, lens = inp["gx"], inp["whh"], inp["h0"], inp["c0"], np.asarray(inp["lens"])
    T, B, H = gx.shape[0], gx.shape[1], whh.shape[2]
    y = np.zeros((T, B, 2 * H))
    gates = np.full((T, B, 2, 4 * H), np.nan)
    cs = np.full((T, B, 2, H), np.nan)
    hn, cn = np.zeros((2, B, H)), np.zeros((2, B, H))
    KS = plan["KS"] if plan else pick_ks(H, bf)
    keep = _fwd_k_mask(H, KS, bool(plan and plan.get("b16")) or bf, defect)
    for d in range(2):
        W = rne_bf16(whh[d]) if bf else whh[d].astype(np.float64)
        if keep is not None:
            W = W * keep[None, :]
        h, c = h0[d].astype(np.float64).copy(), c0[d].astype(np.float64).copy()
        first = True
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            v = t < lens
            hop = rne_bf16(h) if bf else h
            if defect == "stale_empty_ug" and not first and 16 * ((H + 15) // 16) < 16 * KS:
                # an empty unit group publishes the previous image instead of zeros: k >= H of the image holds whatever the
                # workspace held (the device test fills it with 0xFF = NaN); only W's zero columns stand between it and the sum
                hop = hop + np.nan
            pre = to_interleaved(hop @ W.T, H) + gx[t, :, d]
            a = pre.reshape(B, H, 4)
            i, f, g, o = _sig(a[..., 0]), _sig(a[..., 1]), np.tanh(a[..., 2]), _sig(a[..., 3])
            cnew = f * c + i * g
            hnew = o * np.tanh(cnew)
            vv = v[:, None]
            gates[t, v, d] = np.stack([i, f, g, o], -1).reshape(B, 4 * H)[v]
            cs[t, v, d] = cnew[v]
            y[t, :, d * H:(d + 1) * H] = np.where(vv, hnew, 0.0)
            c, h = np.where(vv, cnew, c), np.where(vv, hnew, h)
            first = first and not v.any()
        hn[d], cn[d] = h, c
    out = dict(y=y, gates=gates, c=cs, hn=hn, cn=cn)
    if defect == "skip_bg_slot" and plan and plan["G"] > 1 and plan["NBG"] > 1:   # slot 1 of every workgroup never runs
        rows = np.zeros(B, dtype=bool)
        for bg in range(plan["NBG"]):
            if bg % plan["G"] == 1:
                rows[bg * 16:(bg + 1) * 16] = True
        for k in ("y", "gates", "c"):
            out[k][:, rows] = np.nan
        out["hn"][:, rows] = np.nan
        out["cn"][:, rows] = np.nan
    return out


def ref_backward(inp, fwd, bf=False, defect=None, plan=None, per_step=False):
    """Closed-form backward of ref_forward from its stored gates / c: dgx (0 at padded positions), dh0, dc0, dbias (one row per
    workgroup row `by` of the plan: the sum over its G batch groups; gate-major), dwhh = sum dG^T h_prev (gate-major)."""
    whh, h0, c0, lens = inp["whh"], inp["h0"], inp["c0"], np.asarray(inp["lens"])
    dy, dhn, dcn = inp["dy"], inp["dhn"], inp["dcn"]
    gates, cs, y = fwd["gates"], fwd["c"], fwd["y"]
    T, B, H = dy.shape[0], dy.shape[1], whh.shape[2]
    KS = plan["KS"] if plan else pick_ks(H, bf)
    G, NBG = (plan["G"], plan["NBG16"]) if plan else (1, (B + 15) // 16)
    keep = _bwd_unit_mask(H, KS, bf, defect)
    dgx = np.zeros((T, B, 2, 4 * H))
    dh0, dc0 = np.zeros((2, B, H)), np.zeros((2, B, H))
    dbias = np.zeros((NBG, 2, 4 * H))
    dwhh = np.zeros((2, 4 * H, H))
    by_of_row = (np.arange(B) // 16) // G
    for d in range(2):
        W = rne_bf16(whh[d]) if bf else whh[d].astype(np.float64)           # (4H gate-major, H)
        dh = (np.zeros((B, H)) if dhn is None else dhn[d].astype(np.float64).copy())
        dc = (np.zeros((B, H)) if dcn is None else dcn[d].astype(np.float64).copy())
        order = list(range(T - 1, -1, -1) if d == 0 else range(T))
        prev_rec = None
        for n, t in enumerate(order):
            v = t < lens
            vv = v[:, None]
            g4 = np.where(vv[..., None], np.nan_to_num(gates[t, :, d]).reshape(B, H, 4), 0.0)
            i, f, g, o = g4[..., 0], g4[..., 1], g4[..., 2], g4[..., 3]
            ct = np.nan_to_num(cs[t, :, d])
            tp = t - 1 if d == 0 else t + 1
            has_prev = np.full(B, tp >= 0) if d == 0 else (tp < lens)
            cprev = np.where(has_prev[:, None], np.nan_to_num(cs[min(max(tp, 0), T - 1), :, d]), c0[d])
            hprev = np.where(has_prev[:, None], y[min(max(tp, 0), T - 1), :, d * H:(d + 1) * H], h0[d])
            dht = dy[t, :, d * H:(d + 1) * H] + dh
            tc = np.tanh(ct)
            dct = dc + dht * o * (1 - tc * tc)
            dpre = np.stack([dct * g * i * (1 - i), dct * cprev * f * (1 - f), dct * i * (1 - g * g), dht * tc * o * (1 - o)], -1)
            dpre = np.where(vv[..., None], dpre, 0.0)                      # (B, H, 4)
            dgx[t, :, d] = dpre.reshape(B, 4 * H)
            dgm = to_gate_major(dpre.reshape(B, 4 * H), H)                 # (B, 4H) gate-major
            contrib = np.zeros((NBG, 4 * H))
            np.add.at(contrib, by_of_row, dgm)
            if defect == "dbias_last_step" and per_step:                    # step launches that do not ADD: the last one wins
                dbias[:, d] = contrib
            else:
                dbias[:, d] += contrib
            dwhh[d] += dgm.T @ hprev
            op = rne_bf16(dgm) if bf else dgm
            if keep is not None:
                op = (op.reshape(B, 4, H) * keep[None, None, :]).reshape(B, 4 * H)
            rec = op @ W
            if defect == "final_parity" and n == len(order) - 1:            # dh0's product reads the other parity slot
                rec = prev_rec if prev_rec is not None else np.full((B, H), np.nan)
            prev_rec = op @ W
            carry = np.zeros((B, H)) if defect == "carry_lost" else dh
            dh = np.where(vv, rec, carry)
            dc = np.where(vv, dct * f, dc)
        dh0[d], dc0[d] = dh, dc
    return dict(dgx=dgx, dh0=dh0, dc0=dc0, dbias=dbias, dwhh=dwhh)


def dwhh_from(dgx, y, h0, lens):
    """sum over (t, b) of dG^T h_prev from a run's own dgx and y (padded layout, fp64): (2, 4H, H) gate-major."""
    T, B, H = dgx.shape[0], dgx.shape[1], h0.shape[2]
    lens = np.asarray(lens)
    out = np.zeros((2, 4 * H, H))
    for d in range(2):
        for t in range(T):
            tp = t - 1 if d == 0 else t + 1
            has_prev = (np.full(B, tp >= 0)) if d == 0 else (tp < lens)
            hprev = np.where(has_prev[:, None], y[min(max(tp, 0), T - 1), :, d * H:(d + 1) * H], h0[d]).astype(np.float64)
            out[d] += to_gate_major(dgx[t, :, d].astype(np.float64), H).T @ hprev
    return out


# ------------------------------------------------------------------------------------ tolerances (the project's gates)
TOL_F32 = dict(y=(2e-5, 2e-6), hn=(2e-5, 2e-6), cn=(2e-5, 2e-6), gates=(2e-5, 2e-6), c=(2e-5, 2e-6),
               dgx=(1e-4, 2e-6), dh0=(1e-4, 2e-6), dc0=(1e-4, 2e-6), dbias=(1e-4, 2e-5), dwhh=(1e-4, 2e-5))
TOL_BF16_FWD = (2e-3, 2e-4)
BF16_GRAD_RELNORM = 3e-3
PROBE_ATOL = 2e-6


def ratio(got, ref, rtol, atol):
    """max of |got - ref| / (atol + rtol |ref|) over the elements where ref is defined (NaN in got counts as infinite)."""
    ref = np.asarray(ref, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    m = ~np.isnan(ref)
    if not m.any():
        return 0.0
    r = np.abs(got[m] - ref[m]) / (atol + rtol * np.abs(ref[m]))
    return float("inf") if np.isnan(r).any() else float(r.max())


def relnorm(got, ref):
    ref = np.nan_to_num(np.asarray(ref, dtype=np.float64))
    got = np.asarray(got, dtype=np.float64)
    if np.isnan(got).any():
        return float("inf")
    return float(np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-30))


def score(case, got, ref):
    """{output: measured / allowed}: a value above 1 fails the project's gate for that output."""
    out = {}
    for k, g in got.items():
        if case.bf:
            if k in ("y", "hn", "cn", "gates", "c"):
                out[k] = ratio(g, ref[k], *TOL_BF16_FWD)
            else:
                out[k] = relnorm(g, ref[k]) / BF16_GRAD_RELNORM
        else:
            out[k] = ratio(g, ref[k], *TOL_F32[k])
    return out


# ------------------------------------------------------------------------------------ cases
DEFECTS = {
    "drop_chunk": "one 1 KB chunk of the exchange image is not multiplied",
    "khalf_shift": "a wave's K range starts one chunk late",
    "short_subblock": "backward: the short last sub-block of the ring is not consumed",
    "half_octet": "bf16 images: the second half of an octet of W_hh read as zero",
    "stale_empty_ug": "an empty unit group leaves the old image where its zeros belong",
    "skip_bg_slot": "a workgroup skips one of its batch-group slots",
    "carry_lost": "backward: the gradient carried across a frozen step is lost",
    "final_parity": "backward: the product for dh0 reads the wrong parity slot",
    "dbias_last_step": "backward: dbias is not accumulated across step launches",
}
FWD_DEFECTS = ("drop_chunk", "khalf_shift", "half_octet", "stale_empty_ug", "skip_bg_slot")


def ragged(T, B):
    """Descending lengths T .. 1 over the batch."""
    return [T - (b * T) // B for b in range(B)]


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    flavour: str                  # f32, bf16, s3 (forward only), tagged (fp32 forward, "the data is the flag"), xl8
    T: int
    B: int
    H: int
    lens: tuple
    gmin: int = 0
    exclusive: bool = False
    kinds: tuple = (1, 2)
    layouts: tuple = ("padded", "packed")
    claims: tuple = ()            # names of CLAIMS
    defects: tuple = ()

    @property
    def bf(self):
        return self.flavour in ("bf16", "xl8")

    @property
    def backward(self):
        return self.flavour not in ("s3", "tagged")

    def mode(self, direction, kind):
        m = kind | (self.gmin << GMIN_SHIFT) | (1 << MAP_SHIFT) | (POLL1 if direction == "fwd" else 0)
        m |= BF16 if self.bf else 0
        m |= XL8 if self.flavour == "xl8" else 0
        m |= SPLIT3 if self.flavour == "s3" else 0
        m |= TAGGED if self.flavour == "tagged" else 0
        m |= BWD_EXCLUSIVE if self.exclusive and direction == "bwd" else 0
        return m

    def plan(self, direction="fwd", kind=1):
        m = decode_mode(direction == "bwd", self.mode(direction, kind), self.H)
        p = plan_launch(m, self.B, self.H)
        p["b16"] = m["bf"] or m["s3"]
        p["gm"] = bwd_gm(p, m) if direction == "bwd" else 0
        return p

    def runs(self):
        return [(lay, k) for lay in self.layouts for k in self.kinds]


def _empty_ugs(c):
    return c.plan()["KS"] - (c.H + 15) // 16


CLAIMS = {
    "ks20": lambda c: c.plan()["KS"] == 20, "ks38": lambda c: c.plan()["KS"] == 38, "ks40": lambda c: c.plan()["KS"] == 40,
    "ks56": lambda c: c.plan()["KS"] == 56, "ks64": lambda c: c.plan()["KS"] == 64,
    "hp_full": lambda c: c.H == 16 * c.plan()["KS"],
    "lowest_h": lambda c: c.H <= 4 or pick_ks(c.H - 4, c.plan()["b16"]) != c.plan()["KS"],
    "h4mod8": lambda c: c.H % 8 == 4, "h4mod16": lambda c: c.H % 16 == 4,
    "empty7": lambda c: _empty_ugs(c) == 7, "empty17": lambda c: _empty_ugs(c) == 17, "empty_ugs": lambda c: _empty_ugs(c) > 0,
    "g1": lambda c: c.plan()["G"] == 1, "g2": lambda c: c.plan()["G"] == 2, "g8": lambda c: c.plan()["G"] == 8,
    "g_gt_nbg": lambda c: c.plan()["G"] > c.plan()["NBG"],
    "nby2": lambda c: c.plan()["nby"] == 2, "nby3": lambda c: c.plan()["nby"] == 3, "nby6": lambda c: c.plan()["nby"] == 6,
    "gm1": lambda c: c.plan("bwd")["gm"] == 1, "gm8": lambda c: c.plan("bwd")["gm"] == 8,
    "last_row_one_group": lambda c: c.plan()["NBG"] % c.plan()["G"] == 1 and c.plan()["G"] > 1,
    "bg_of_one_row": lambda c: c.B % 16 == 1,
    "step_launches": lambda c: not c.plan(kind=0)["fits"] and c.plan(kind=0)["blocks"] == 1960,
    "exclusive_g1": lambda c: c.exclusive and c.plan()["G"] == 1 and c.plan("bwd")["gm"] == 8,
    "bwd_no_ring": lambda c: c.plan()["KS"] == 64 and not c.bf and all(n == 4 for n in bwd_cfg(64, False)["cnt"]),
    "short_sb": lambda c: min(n for n in bwd_cfg(c.plan("bwd")["KS"], c.bf)["cnt"] if n) < bwd_cfg(c.plan("bwd")["KS"], c.bf)["SB"],
    "t1": lambda c: c.T == 1, "t2": lambda c: c.T == 2, "b1": lambda c: c.B == 1,
    "second_stream_one_step": lambda c: c.B > 16 and c.lens[16] == 1 and c.lens[0] > 1,
    "tagged": lambda c: decode_mode(False, c.mode("fwd", 1), c.H)["tagged"] and predict("fwd", c.T, c.B, c.H, c.mode("fwd", 1), False)[1] == K_FWD,
    "s3_family": lambda c: predict("fwd", c.T, c.B, c.H, c.mode("fwd", 1), False)[1] == K_FWD_SPLIT3,
    "s3_falls_back": lambda c: c.flavour == "s3" and predict("fwd", c.T, c.B, c.H, c.mode("fwd", 1), False)[1] == K_FWD,
    "xl8_family": lambda c: predict("fwd", c.T, c.B, c.H, c.mode("fwd", 1), False)[1] == K_FWD_XL8
    and predict("bwd", c.T, c.B, c.H, c.mode("bwd", 1), False)[1] == K_BWD_XL8,
    "xl8_group_of_one_row": lambda c: c.B % 8 == 1, "xl8_odd_groups": lambda c: ((c.B + 7) // 8) % 2 == 1,
    "xl8_four_groups": lambda c: (c.B + 7) // 8 == 4,
    "fp32_ks56_where_bf16_ks40": lambda c: pick_ks(c.H) == 56 and pick_ks(c.H, True) == 40,
}


def _c(name, flavour, T, B, H, claims, defects=(), lens=None, **kw):
    return Case(name, flavour, T, B, H, tuple(ragged(T, B) if lens is None else lens), claims=tuple(claims), defects=tuple(defects), **kw)


_KD = ("drop_chunk", "khalf_shift")
CASES = (
    # ---- fp32
    _c("f32_T3_B17_H1024", "f32", 3, 17, 1024, ("ks64", "hp_full", "bg_of_one_row", "bwd_no_ring", "g1", "gm1"), _KD + ("carry_lost", "final_parity")),
    _c("f32_T3_B40_H900", "f32", 3, 40, 900, ("ks64", "g2", "nby2", "gm8", "last_row_one_group", "h4mod16", "h4mod8", "empty7", "lowest_h"),
       _KD + ("stale_empty_ug", "skip_bg_slot")),
    _c("f32_T3_B17_H612", "f32", 3, 17, 612, ("ks56", "fp32_ks56_where_bf16_ks40", "lowest_h", "h4mod8", "h4mod16", "empty_ugs"), _KD + ("stale_empty_ug",)),
    _c("f32_T3_B17_H640", "f32", 3, 17, 640, ("ks56", "fp32_ks56_where_bf16_ks40", "g1", "gm1"), _KD),
    _c("f32_T3_B33_H896", "f32", 3, 33, 896, ("ks56", "hp_full", "g2", "gm8"), _KD + ("skip_bg_slot", "dbias_last_step")),
    _c("f32_T4_B33_H324", "f32", 4, 33, 324, ("ks38", "empty17", "nby3", "lowest_h", "h4mod8", "h4mod16", "g1", "gm1", "short_sb"),
       _KD + ("short_subblock", "stale_empty_ug", "carry_lost", "dbias_last_step")),
    _c("f32_T3_B33_H320", "f32", 3, 33, 320, ("ks20", "hp_full", "g1", "gm1"), _KD + ("final_parity",)),
    _c("f32_T3_B20_H608", "f32", 3, 20, 608, ("ks38", "hp_full", "short_sb"), _KD + ("short_subblock",)),
    _c("f32_gmin8_B40_H64", "f32", 3, 40, 64, ("ks20", "g8", "g_gt_nbg", "gm8"), ("skip_bg_slot", "drop_chunk"), gmin=8),
    _c("f32_gmin8_B20_H324", "f32", 3, 20, 324, ("ks38", "g8", "g_gt_nbg", "gm8"), ("skip_bg_slot", "short_subblock"), gmin=8),
    _c("f32_gmin2_B40_H900", "f32", 3, 40, 900, ("ks64", "g2", "gm8"), ("skip_bg_slot",), gmin=2),
    _c("f32_gmin8_B20_H640", "f32", 3, 20, 640, ("ks56", "g8", "g_gt_nbg", "gm8"), ("skip_bg_slot",), gmin=8),
    _c("f32_gmin8_B20_H1024", "f32", 3, 20, 1024, ("ks64", "g8", "g_gt_nbg", "gm8"), ("skip_bg_slot",), gmin=8),
    _c("f32_T3_B768_H8", "f32", 3, 768, 8, ("ks20", "g8", "nby6", "gm8"), ("skip_bg_slot",)),
    _c("f32_T3_B769_H8_auto", "f32", 3, 769, 8, ("step_launches",), ("dbias_last_step",), kinds=(0,)),
    _c("f32_excl_B17_H1024", "f32", 3, 17, 1024, ("exclusive_g1", "ks64"), ("final_parity",), exclusive=True),
    _c("f32_excl_B17_H324", "f32", 3, 17, 324, ("exclusive_g1", "ks38"), ("short_subblock",), exclusive=True),
    _c("f32_T1_B1_H4", "f32", 1, 1, 4, ("t1", "b1", "ks20", "h4mod8", "h4mod16", "lowest_h"), ("final_parity",)),
    _c("f32_T2_B16_H16", "f32", 2, 16, 16, ("t2", "ks20"), ("final_parity", "drop_chunk"), lens=[2] * 8 + [1] * 8),
    _c("f32_T3_3_then_ones", "f32", 3, 17, 16, ("second_stream_one_step", "bg_of_one_row"), ("final_parity",), lens=[3] + [1] * 16),
    # ---- bf16 against the bf16 twin
    _c("bf16_B17_H320", "bf16", 3, 17, 320, ("ks20", "hp_full", "gm1"), _KD + ("half_octet",)),
    _c("bf16_B17_H324", "bf16", 3, 17, 324, ("ks40", "lowest_h", "h4mod8", "h4mod16", "short_sb"), _KD + ("half_octet", "short_subblock", "stale_empty_ug")),
    _c("bf16_B17_H612", "bf16", 3, 17, 612, ("ks40", "h4mod8", "gm1"), _KD + ("half_octet",)),
    _c("bf16_B17_H640", "bf16", 3, 17, 640, ("ks40", "hp_full"), _KD + ("half_octet", "short_subblock")),
    _c("bf16_B17_H644", "bf16", 3, 17, 644, ("ks56", "lowest_h", "h4mod8", "h4mod16", "short_sb"), _KD + ("half_octet", "short_subblock")),
    _c("bf16_B17_H896", "bf16", 3, 17, 896, ("ks56", "hp_full", "gm1"), _KD),
    _c("bf16_B17_H900", "bf16", 3, 17, 900, ("ks64", "lowest_h", "h4mod8", "h4mod16", "gm1"), _KD + ("half_octet",)),
    _c("bf16_B40_H900", "bf16", 3, 40, 900, ("ks64", "g2", "gm8", "last_row_one_group"), ("skip_bg_slot", "half_octet")),
    _c("bf16_B17_H1020", "bf16", 3, 17, 1020, ("ks64", "h4mod8"), _KD + ("half_octet",)),
    _c("bf16_B17_H1024", "bf16", 3, 17, 1024, ("ks64", "hp_full"), _KD),
    _c("bf16_gmin2_B17_H320", "bf16", 3, 17, 320, ("ks20", "g2", "gm8"), ("skip_bg_slot",), gmin=2),
    _c("bf16_gmin8_B17_H612", "bf16", 3, 17, 612, ("ks40", "g8", "g_gt_nbg", "gm8"), ("skip_bg_slot",), gmin=8),
    _c("bf16_gmin8_B17_H644", "bf16", 3, 17, 644, ("ks56", "g8", "g_gt_nbg", "gm8"), ("skip_bg_slot",), gmin=8),
    _c("bf16_gmin8_B17_H4", "bf16", 3, 17, 4, ("ks20", "lowest_h", "h4mod8", "h4mod16", "g8", "g_gt_nbg"), ("skip_bg_slot",), gmin=8),
    # ---- split3 forward
    _c("s3_B17_H320", "s3", 3, 17, 320, ("s3_family", "ks20", "hp_full"), _KD + ("half_octet",)),
    _c("s3_B17_H324", "s3", 3, 17, 324, ("s3_family", "ks40", "lowest_h", "h4mod8", "h4mod16"), _KD + ("half_octet", "stale_empty_ug")),
    _c("s3_B17_H612", "s3", 3, 17, 612, ("s3_family", "ks40", "h4mod8"), _KD + ("half_octet",)),
    _c("s3_B40_H640", "s3", 3, 40, 640, ("s3_family", "ks40", "hp_full", "g2"), ("skip_bg_slot",), gmin=2),
    _c("s3_B17_H644", "s3", 3, 17, 644, ("s3_family", "ks56", "lowest_h", "h4mod8", "h4mod16"), _KD + ("half_octet",)),
    _c("s3_B17_H896", "s3", 3, 17, 896, ("s3_family", "ks56", "hp_full"), _KD),
    _c("s3_B17_H900", "s3", 3, 17, 900, ("s3_falls_back", "ks64"), _KD),
    _c("s3_B17_H4", "s3", 3, 17, 4, ("s3_family", "ks20", "lowest_h", "h4mod8", "h4mod16"), ("drop_chunk",)),
    # ---- the tagged hand-off (fp32 forward; the engine's choice where split3 has no instantiation, H > 896)
    _c("tagged_B17_H1024", "tagged", 3, 17, 1024, ("tagged", "ks64", "hp_full"), _KD),
    _c("tagged_B40_H900", "tagged", 3, 40, 900, ("tagged", "ks64", "g2", "empty7", "h4mod16"), _KD + ("skip_bg_slot", "stale_empty_ug")),
    _c("tagged_B33_H324", "tagged", 4, 33, 324, ("tagged", "ks38", "empty17", "nby3"), _KD),
    # ---- geometry the lists above leave out, per KS x precision: G = 2, G = 8 > NBG
    _c("f32_gmin2_B33_H16", "f32", 3, 33, 16, ("ks20", "g2", "gm8"), ("skip_bg_slot",), gmin=2),
    _c("f32_gmin2_B33_H324", "f32", 3, 33, 324, ("ks38", "g2", "gm8"), ("skip_bg_slot",), gmin=2),
    _c("bf16_gmin2_B17_H612", "bf16", 3, 17, 612, ("ks40", "g2", "gm8"), ("skip_bg_slot",), gmin=2),
    _c("bf16_gmin2_B17_H644", "bf16", 3, 17, 644, ("ks56", "g2", "gm8"), ("skip_bg_slot",), gmin=2),
    _c("bf16_gmin8_B17_H900", "bf16", 3, 17, 900, ("ks64", "g8", "g_gt_nbg", "gm8"), ("skip_bg_slot",), gmin=8),
    _c("s3_gmin2_B17_H320", "s3", 3, 17, 320, ("s3_family", "ks20", "g2"), ("skip_bg_slot",), gmin=2),
    _c("s3_gmin8_B17_H4", "s3", 3, 17, 4, ("s3_family", "ks20", "g8", "g_gt_nbg"), ("skip_bg_slot",), gmin=8),
    _c("s3_gmin8_B17_H324", "s3", 3, 17, 324, ("s3_family", "ks40", "g8", "g_gt_nbg"), ("skip_bg_slot",), gmin=8),
    _c("s3_gmin2_B17_H644", "s3", 3, 17, 644, ("s3_family", "ks56", "g2"), ("skip_bg_slot",), gmin=2),
    _c("s3_gmin8_B17_H644", "s3", 3, 17, 644, ("s3_family", "ks56", "g8", "g_gt_nbg"), ("skip_bg_slot",), gmin=8),
    # ---- bf16, XCD-local streams of eight rows (persistent only)
    _c("xl8_B9_H644", "xl8", 3, 9, 644, ("xl8_family", "lowest_h", "h4mod8", "xl8_group_of_one_row"), _KD + ("half_octet",), kinds=(1,)),
    _c("xl8_B25_H644", "xl8", 3, 25, 644, ("xl8_family", "xl8_group_of_one_row", "xl8_four_groups"), _KD, kinds=(1,)),
    _c("xl8_B1_H896", "xl8", 3, 1, 896, ("xl8_family", "b1", "hp_full", "xl8_odd_groups"), _KD, kinds=(1,)),
    _c("xl8_B32_H892", "xl8", 3, 32, 892, ("xl8_family", "h4mod8"), _KD + ("half_octet",), kinds=(1,)),
)
assert len({c.name for c in CASES}) == len(CASES)
OPTIONAL_POINTER_CASE = next(c for c in CASES if c.name == "f32_T4_B33_H324")


def claims_hold(case):
    return [n for n in case.claims if not CLAIMS[n](case)]


def case_seed(case):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case.name)) % (2 ** 31)


@functools.lru_cache(maxsize=8)
def inputs(case):
    """Dense operands (|w| <= 1 / sqrt(H)), all exactly representable in fp32; gx has the spread of a projection plus biases."""
    r = np.random.RandomState(case_seed(case))
    T, B, H = case.T, case.B, case.H
    f = lambda a: a.astype(np.float32).astype(np.float64)
    d = dict(whh=f((r.rand(2, 4 * H, H) * 2 - 1) / np.sqrt(H)), gx=f(r.randn(T, B, 2, 4 * H) * 0.7),
             h0=f(r.randn(2, B, H)), c0=f(r.randn(2, B, H)), dy=f(r.randn(T, B, 2 * H)), dhn=f(r.randn(2, B, H)),
             dcn=f(r.randn(2, B, H)), lens=tuple(case.lens))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def reference(case, kind=1, defect=None):
    """fp64 outputs of the case (bf16 cases: the bf16 twin), forward and, for cases that have one, backward."""
    inp = inputs(case)
    pf, pb = case.plan("fwd", kind), case.plan("bwd", kind)
    fwd = ref_forward(inp, case.bf, defect if defect in FWD_DEFECTS else None, pf)
    out = dict(fwd)
    if case.backward:
        clean = fwd if defect not in FWD_DEFECTS else ref_forward(inp, case.bf, None, pf)
        skip = defect == "skip_bg_slot"
        bw = ref_backward(inp, clean, case.bf, None if skip else defect, pb, per_step=not pb["persistent"])
        if skip and pb["G"] > 1 and pb["NBG16"] > 1:
            rows = np.array([(b // 16) % pb["G"] == 1 for b in range(case.B)])
            bw["dgx"][:, rows] = np.nan
            bw["dh0"][:, rows] = np.nan
            bw["dc0"][:, rows] = np.nan
        out.update(bw)
    return out


@functools.lru_cache(maxsize=4)
def clean_reference(case, persistent=True):
    return reference(case, 1 if persistent else 2)


def defect_moves(case, defect):
    """max over the checked outputs of (defective - clean) / tolerance, over the case's runs' launch kinds."""
    best = 0.0
    kinds = sorted({k for _, k in case.runs()})
    if defect != "dbias_last_step":          # (the only model whose effect depends on the launch kind)
        kinds = kinds[:1]
    for kind in kinds:
        persistent = case.plan("fwd", kind)["persistent"]
        ref, bad = clean_reference(case, persistent), reference(case, kind, defect)
        s = score(case, {k: bad[k] for k in ref}, ref)
        best = max(best, max(s.values()))
    return best


# ------------------------------------------------------------------------------------ one-hot probes
# A dense product hides a piece of the exchange image that sits in the wrong LDS slot, or a K range that starts a chunk off,
# in a diffuse error.  The probes address the image one k at a time: after the first processed step exactly ONE unit per
# (direction, row) is non-zero, so the second step's product is one term (forward) or four (backward: the four gates of
# one unit) and can be stated exactly from the kernel's own first-step output.
PROBE_T = 2


def probe_ks(H, KS, bf):
    """The k the persistent sweep visits: octet and chunk edges at the start, the forward K halves' edge, the first and last
    unit of every backward wave's eighth and of every sub-block of the ring, and the end of H."""
    ks = {0, 3, 4, 7, 8, 15, 16, 31, 32, 8 * KS - 1, 8 * KS, H - 5, H - 4, H - 1}
    cfg = bwd_cfg(KS, bf)
    for w in range(8):
        for sb in range(cfg["NSB"]):
            if cfg["cnt"][sb]:
                u0 = w * 2 * KS + sb * cfg["SB"] * cfg["units"]
                ks |= {u0, u0 + cfg["cnt"][sb] * cfg["units"] - 1}
    return sorted(k for k in ks if 0 <= k < H)


def probe_assignment(H, B, ks=None):
    """List of (2, B) arrays: the open unit of every (direction, row).  Step-launch sweep (ks None, B = H): one array, the two
    directions two different permutations of all k.  Else the list `ks` dealt 2 B at a time over as many runs as it takes
    (the last run wraps round to the list's start)."""
    if ks is None:
        assert B == H
        return [np.stack([np.arange(H), (11 * np.arange(H) + 3) % H])]
    ks = np.asarray(ks)
    return [ks[(r * 2 * B + np.arange(2 * B)) % len(ks)].reshape(2, B) for r in range((len(ks) + 2 * B - 1) // (2 * B))]


def probe_weights(H, seed=5):
    return ((np.random.RandomState(seed).rand(2, 4 * H, H) - 0.5).astype(np.float32)).astype(np.float64)


def _pattern(B, n, salt):
    b, j, d = np.arange(B)[:, None, None], np.arange(n)[None, None, :], np.arange(2)[None, :, None]
    return (((b * 131 + j * 17 + d * 7 + salt) % 61) - 30).astype(np.float32) / np.float32(24)


def probe_fwd_inputs(H, B, kof):
    """gx (2, B, 2, 4H) fp32: the first processed step (t = 0 forward, t = 1 reverse) opens the output gate (+40) at unit
    kof[d, b] and shuts it (-40) everywhere else, with i = sigmoid(2), g = tanh(1) and c0 = h0 = 0; the second carries a pattern."""
    gx = np.empty((PROBE_T, B, 2, 4 * H), dtype=np.float32)
    drive = np.tile(np.array([2.0, 0.0, 1.0, -40.0], dtype=np.float32), H)
    second = _pattern(B, 4 * H, 0)
    for d in range(2):
        first_t = 0 if d == 0 else PROBE_T - 1
        gx[first_t, :, d] = drive
        gx[first_t, np.arange(B), d, 4 * kof[d] + 3] = 40.0
        gx[1 - first_t, :, d] = second[:, d]
    return gx


PROBE_H1 = 1.0 / (1.0 + np.exp(-40.0)) * np.tanh(1.0 / (1.0 + np.exp(-2.0)) * np.tanh(1.0))


def probe_fwd_expected(whh, gx, kof, y_first, bf, shift=0):
    """The second step's stored gates (B, 2, 4H) from the kernel's own y of the first (y_first (2, B): its value at the open
    unit): act(gx + h1 W_hh[:, k]) -- one product per gate row.  shift: a defect model, the image read `shift` k off."""
    B, H = gx.shape[1], whh.shape[2]
    out = np.empty((B, 2, 4 * H))
    for d in range(2):
        h1 = rne_bf16(y_first[d]) if bf else y_first[d].astype(np.float64)
        W = rne_bf16(whh[d]) if bf else whh[d]
        col = W[:, (kof[d] + shift) % H].T                                   # (B, 4H) gate-major
        pre = (to_interleaved(h1[:, None] * col, H) + gx[0 if d else 1, :, d].astype(np.float64)).reshape(B, H, 4)
        out[:, d] = np.stack([_sig(pre[..., 0]), _sig(pre[..., 1]), np.tanh(pre[..., 2]), _sig(pre[..., 3])], -1).reshape(B, 4 * H)
    return out


def probe_bwd_inputs(H, B, kof, T=PROBE_T):
    """Saved activations of a forward pass that never ran (any values in range do): gates (T, B, 2, 4H), c and c0, and dy one-hot
    at the first processed step (t = T - 1 forward direction, t = 0 reverse), unit kof[d, b]."""
    gates = np.empty((T, B, 2, 4 * H), dtype=np.float32)
    for t in range(T):
        p = _pattern(B, 4 * H, 3 + 5 * t).reshape(B, 2, H, 4)
        gates[t] = np.stack([0.5 + 0.3 * p[..., 0], 0.5 + 0.3 * p[..., 1], 0.7 * p[..., 2], 0.5 + 0.3 * p[..., 3]], -1).reshape(B, 2, 4 * H)
    cs = np.stack([_pattern(B, H, 11 + t) for t in range(T)]).astype(np.float32)          # (T, B, 2, H)
    c0 = np.ascontiguousarray(_pattern(B, H, 29).transpose(1, 0, 2))                       # (2, B, H)
    dy = np.zeros((T, B, 2 * H), dtype=np.float32)
    for d in range(2):
        dy[T - 1 if d == 0 else 0, np.arange(B), d * H + kof[d]] = 1.0
    return gates, cs, c0, dy


def probe_bwd_expected(whh, gates, cs, c0, kof, dgx_first, bf, T=PROBE_T, dgx_second=None):
    """From the kernel's own dgx of the first processed step (dgx_first (B, 2, 4): the four gates of the open unit): the
    recurrent gradient sum_g dG[g] W_hh[g H + k, :] (four terms), and with it the second step's dgx (B, 2, 4H) (T = 2) or dh0
    (T = 1), and dc0.  dh0 of T = 2 is the product of the kernel's own second-step dgx (dgx_second (B, 2, 4H); a bf16 rounding
    of it must not depend on the last bit of this reference).  Returns (dgx of the second step or None, dh0, dc0)."""
    B, H = gates.shape[1], whh.shape[2]
    g64, c64 = gates.astype(np.float64), cs.astype(np.float64)
    dgx2 = np.zeros((B, 2, 4 * H)) if T == 2 else None
    dh0, dc0 = np.zeros((2, B, H)), np.zeros((2, B, H))
    rows = np.arange(B)
    for d in range(2):
        t0 = T - 1 if d == 0 else 0
        W = (rne_bf16(whh[d]) if bf else whh[d]).reshape(4, H, H)              # [g][unit][k]
        dG = rne_bf16(dgx_first[:, d]) if bf else dgx_first[:, d].astype(np.float64)      # (B, 4)
        rec = np.einsum("bg,gbk->bk", dG, W[:, kof[d], :])                     # (B, H)
        k = kof[d]
        o0, f0 = g64[t0, rows, d, 4 * k + 3], g64[t0, rows, d, 4 * k + 1]
        tc0 = np.tanh(c64[t0, rows, d, k])
        dc = np.zeros((B, H))
        dc[rows, k] = o0 * (1 - tc0 * tc0) * f0                                # dh = 1 at the open unit
        if T == 2:
            t1 = 1 - t0
            g4 = g64[t1, :, d].reshape(B, H, 4)
            i, f, g, o = g4[..., 0], g4[..., 1], g4[..., 2], g4[..., 3]
            tc = np.tanh(c64[t1, :, d])
            dct = dc + rec * o * (1 - tc * tc)
            dgx2[:, d] = np.stack([dct * g * i * (1 - i), dct * c0[d].astype(np.float64) * f * (1 - f), dct * i * (1 - g * g),
                                   rec * tc * o * (1 - o)], -1).reshape(B, 4 * H)
            dG2 = to_gate_major(dgx2[:, d] if dgx_second is None else dgx_second[:, d].astype(np.float64), H)
            dG2 = rne_bf16(dG2) if bf else dG2
            dh0[d] = dG2 @ (rne_bf16(whh[d]) if bf else whh[d])
            dc0[d] = dct * f
        else:
            dh0[d], dc0[d] = rec, dc
    return dgx2, dh0, dc0


@dataclasses.dataclass(frozen=True)
class Probe:
    name: str
    flavour: str          # f32, bf16, s3, xl8
    B: int
    H: int
    kind: int             # 1: persistent, B = 32, the k of probe_ks; 2: step launches, B = H, every k

    @property
    def bf(self):
        return self.flavour in ("bf16", "xl8")

    def case(self):
        return Case(self.name, self.flavour, PROBE_T, self.B, self.H, (PROBE_T,) * self.B)

    def kofs(self):
        p = self.case().plan("fwd", self.kind)
        return probe_assignment(self.H, self.B, None if self.kind == 2 else probe_ks(self.H, p["KS"], p["b16"]))


PROBE_H = {"f32": (320, 324, 612, 900), "bf16": (320, 324, 644, 900), "s3": (320, 324, 644), "xl8": (644, 892)}   # one H per KS class
PROBES = tuple(Probe("probe_%s_B32_H%d" % (fl, H), fl, 32, H, 1) for fl, hs in PROBE_H.items() for H in hs) + \
    tuple(Probe("probe_%s_B%d_steps" % (fl, H), fl, H, H, 2) for fl in ("f32", "bf16") for H in (324, 612, 644, 900, 1024))
