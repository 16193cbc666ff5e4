"""Cases, float64 references, float32 error models and defect models of the streaming-kernel tests.

tests/test_gpu_streaming.py compares the kernels of csrc/bn_optim.hip, pit.hip, rsh.hip, packed.hip and the two row
converters of gemm.hip with the float64 references below; tests/test_streaming_cases.py proves on any machine that the
cases can tell a wrong kernel from a right one.

Tolerance of a compared quantity q:  err <= K[family] * E_ref(q) + eps(q)
  E_ref  the largest error against float64 of a float32 evaluation of the same formula on the CPU (reductions: the worse
         of a strictly serial np.cumsum order and np.sum's pairwise order; elementwise formulas: torch float32),
  eps    one float32 ulp of the largest compared value (E_ref can happen to be 0),
  K      twice the largest ratio (err - eps) / E_ref measured per family on the MI355X, rounded up (cap 8):
         profiles/streaming_kernels.txt.
"""
import itertools
import math

import numpy as np
import torch

F32, F64 = np.float32, np.float64

# loop bounds of the kernels (the constants the shapes are chosen against)
STREAM_TRIP = 4096 * 256        # bn_optim.hip stream_blocks(), rsh.hip rsh_blocks(): elements of one grid-stride trip
NORM_TRIP = 1024 * 256          # bn_optim.hip NORM_BLOCKS x 256
RCH = 256                       # bn_optim.hip: rows per block of the column reductions
PIT_TCH, RSH_TCH = 16, 8        # pit.hip TCH, rsh.hip RTCH: frames per block

EPS = float(F32(1e-5))          # what the kernels get: the float arguments of the C ABI
LR, BETA1, BETA2, ADAM_EPS, CLIP_EPS = (float(F32(v)) for v in (1e-3, 0.9, 0.999, 1e-8, 1e-6))
MAX_NORM = 0.25

# k per family: twice the largest measured ratio, rounded up (profiles/streaming_kernels.txt)
# measured maxima: colred 0.76, bn_chain 1.00, elementwise 1.00, grad_norm 0 (within eps), adam_skip 0.51, pit 0.30, rsh 0.43
K = {"colred": 2, "bn_chain": 2, "elementwise": 2, "grad_norm": 1, "adam_skip": 2, "pit": 1, "rsh": 1}

DEFECTS = ("last_row", "last_chunk", "last_col", "row_shift", "second_trip", "count_R", "next_perm")


# ------------------------------------------------------------------------------------------------ error measures
def ulp32(ref):
    ref = np.asarray(ref, F64)
    ref = ref[np.isfinite(ref)]
    return float(np.spacing(F32(np.max(np.abs(ref))))) if ref.size else 0.0


def maxerr(got, ref):
    """Largest absolute difference; positions where the reference is infinite must be the same infinity."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    fin = np.isfinite(ref)
    if not np.array_equal(got[~fin], ref[~fin]):
        return float("inf")
    return float(np.max(np.abs(got[fin] - ref[fin]))) if fin.any() else 0.0


def tolerance(family, ref, e_ref):
    return K[family] * e_ref + ulp32(ref)


def needed_k(err, ref, e_ref):
    """The smallest k with err <= k * E_ref + eps (inf: no k does)."""
    over = err - ulp32(ref)
    if over <= 0:
        return 0.0
    return over / e_ref if e_ref > 0 else float("inf")


def _sum(t, dt, order):
    if order == "serial":
        return np.cumsum(t, axis=0, dtype=dt)[-1] if t.shape[0] else np.zeros(t.shape[1:], dt)
    return np.sum(t, axis=0, dtype=dt)


def _ref_and_eref(fn):
    """fn(dtype, order) -> value: (float64 reference, E_ref over both float32 summation orders)."""
    ref = np.asarray(fn(F64, "pair"), F64)
    return ref, max(maxerr(fn(F32, o), ref) for o in ("serial", "pair"))


def _rows(R, defect, chunk):
    r = np.arange(R)
    if defect == "last_row":
        return r[:-1]
    if defect == "last_chunk":
        return r[:(-(-R // chunk) - 1) * chunk]
    if defect == "row_shift":
        return np.minimum(r + 1, R - 1)
    return r


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64 if dt is F64 else torch.float32) if isinstance(a, np.ndarray) else a


def ew_ref(fn, *args):
    """Elementwise formula fn over torch tensors: (float64 reference, E_ref of its torch float32 evaluation); numpy
    float32 arrays are the tensors, everything else is passed through."""
    ref = fn(*[_t(a, F64) for a in args])
    got = fn(*[_t(a, F32) for a in args])
    if isinstance(ref, tuple):
        refs = [r.numpy() for r in ref]
        return refs, [maxerr(g.numpy(), r) for g, r in zip(got, refs)]
    ref = ref.numpy()
    return ref, maxerr(got.numpy(), ref)


# ------------------------------------------------------------------------------------------------ column reductions
# colred_kernel: 64 columns x 256-row chunks (RCH), 4 row lanes; colfin: 256 columns per block
COL_SHAPES = [(2, 1), (3, 63), (255, 64), (256, 65), (257, 257), (513, 600), (1000, 200)]
COL_KINDS = ("mean", "var", "dbeta", "dgamma", "colsum")


def col_count(R):
    return R + R // 3 + 2


def col_cases():
    """(name, R, C, count, tight): every shape with count = R and count > R; one two-pass-variance case."""
    out = []
    for R, C in COL_SHAPES:
        out.append(("%dx%d" % (R, C), R, C, R, False))
        out.append(("%dx%d_count%d" % (R, C, col_count(R)), R, C, col_count(R), False))
    out.append(("513x600_mean30_std0.01", 513, 600, 513, True))
    return out


def col_inputs(R, C, tight=False, seed=0):
    g = np.random.default_rng(1000 * R + C + seed)
    if tight:
        x = (30.0 + 0.01 * g.standard_normal((R, C))).astype(F32)     # cancellation: only a two-pass variance survives
    else:
        x = (0.3 + 0.5 * g.standard_normal((R, C))).astype(F32)
    dy = g.standard_normal((R, C)).astype(F32)
    gamma = g.uniform(0.5, 1.5, C).astype(F32)
    beta = g.standard_normal(C).astype(F32)
    return dict(x=x, dy=dy, gamma=gamma, beta=beta)


def col_eval(kind, x, dt=F64, order="pair", defect=None, dy=None, mean=None, var=None, count=None, base=None):
    """One column reduction as the kernels define it, in dtype dt and summation order `order`, optionally with a defect."""
    R, C = x.shape
    count = R if count is None or defect == "count_R" else count
    idx = _rows(R, defect, RCH)
    xs = x[idx].astype(dt)
    if kind in ("mean", "colsum"):
        t = xs
    elif kind == "var":
        d = xs - mean.astype(dt)
        t = d * d
    elif kind == "dbeta":
        t = dy[idx].astype(dt)
    elif kind == "dgamma":
        rs = dt(1) / np.sqrt(var.astype(dt) + dt(EPS))
        t = dy[idx].astype(dt) * ((xs - mean.astype(dt)) * rs)
    else:
        raise ValueError(kind)
    s = np.array(_sum(t, dt, order), dt).reshape(C)
    if defect == "last_col":
        s[-1] = 0
    if kind == "mean":
        s = s * dt(1.0 / count)
    elif kind == "var":
        mu = mean.astype(dt)
        s = (s + dt(count - R) * mu * mu) * dt(1.0 / count)
    elif kind == "colsum" and base is not None:
        s = base.astype(dt) + s
    return s


def col_ref(kind, x, **kw):
    return _ref_and_eref(lambda dt, order: col_eval(kind, x, dt, order, **kw))


def col_defects(kind, R, count, tight=False):
    """The defect models that apply to one reduction of one case."""
    # (two rows lie symmetric about their mean: reading row 1 twice leaves their variance as it was -- row_shift needs three)
    d = ["last_row", "last_chunk", "last_col"] + (["row_shift"] if R >= 3 else [])
    if tight and kind in ("mean", "colsum"):
        d.remove("row_shift")         # sums of values of 30 +- 0.01: rows differ by less than float32 resolves; the case is the variance's
    if count > R and kind in ("mean", "var"):
        d.append("count_R")
    return d


# ------------------------------------------------------------------------------------------------ elementwise formulas
def ew_bn_apply(x, mean, var, gamma, beta):
    rs = 1.0 / torch.sqrt(var + EPS)
    return (x - mean) * rs * gamma + beta


def ew_bn_bwd_apply(dy, x, mean, var, gamma, dgamma, dbeta, count):
    rs = 1.0 / torch.sqrt(var + EPS)
    xh = (x - mean) * rs
    return gamma * rs * (dy - (1.0 / count) * (dbeta + xh * dgamma))


def ew_sigmoid_bwd(dm, m):
    return dm * m * (1.0 - m)


def ew_unfold_grad(G, dzsum, s, t, dW0):
    v = G * s + dzsum[:, None] * t
    return v if dW0 is None else dW0 + v


def ew_running(mean, var, rmean, rvar, count, momentum):
    if mean.dtype == torch.float32:
        unb = F32(count) / F32(count - 1)
        momentum = F32(momentum)
        keep = F32(1) - momentum
    else:
        unb = count / (count - 1.0)
        momentum = float(F32(momentum))
        keep = 1.0 - momentum
    return float(keep) * rmean + float(momentum) * mean, float(keep) * rvar + float(momentum) * (var * float(unb))


def bn_chain(x, dy, gamma, beta, count, dt, order):
    """Training-mode BatchNorm1d forward and backward over the zero-padded (count, C) grid of which x holds the first R
    rows (dy is zero on the others): every stage in dtype dt on the previous stage's result."""
    mean = col_eval("mean", x, dt, order, count=count)
    var = col_eval("var", x, dt, order, mean=mean, count=count)
    dbeta = col_eval("dbeta", x, dt, order, dy=dy)
    dgamma = col_eval("dgamma", x, dt, order, dy=dy, mean=mean, var=var)
    a = [_t(np.asarray(v, dt), dt) for v in (x.astype(dt), dy.astype(dt), mean, var, gamma.astype(dt), beta.astype(dt), dgamma, dbeta)]
    X, DY, M, V, G, Bt, DG, DB = a
    y = ew_bn_apply(X, M, V, G, Bt).numpy()
    dx = ew_bn_bwd_apply(DY, X, M, V, G, DG, DB, count).numpy()
    rm, rv = ew_running(M, V, torch.zeros_like(M), torch.ones_like(V), count, 0.1)
    return dict(mean=mean, var=var, y=y, dx=dx, dgamma=dgamma, dbeta=dbeta, running_mean=rm.numpy(), running_var=rv.numpy())


def bn_chain_torch64(x, dy, gamma, beta, count, momentum=float(F32(0.1))):
    """The same through torch.nn.BatchNorm1d and autograd in float64 on the padded grid (running statistics included)."""
    R, C = x.shape
    bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=momentum).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma).double())
        bn.bias.copy_(torch.from_numpy(beta).double())
    xp = torch.zeros(count, C, dtype=torch.float64)
    xp[:R] = torch.from_numpy(x).double()
    dyp = torch.zeros(count, C, dtype=torch.float64)
    dyp[:R] = torch.from_numpy(dy).double()
    xp.requires_grad_(True)
    y = bn(xp)
    y.backward(dyp)
    return dict(mean=xp.detach().mean(0).numpy(), var=xp.detach().var(0, unbiased=False).numpy(), y=y.detach()[:R].numpy(),
                dx=xp.grad[:R].numpy(), dgamma=bn.weight.grad.numpy(), dbeta=bn.bias.grad.numpy(),
                running_mean=bn.running_mean.numpy(), running_var=bn.running_var.numpy())


def bn_chain_eref(x, dy, gamma, beta, count, ref):
    """E_ref of every quantity of the chain: the worse of the two float32 orders against the float64 reference `ref`."""
    e = {}
    for order in ("serial", "pair"):
        c = bn_chain(x, dy, gamma, beta, count, F32, order)
        for k, v in c.items():
            e[k] = max(e.get(k, 0.0), maxerr(v, ref[k]))
    return e


# (R, count, C) of the packed backward; the last: R*C > STREAM_TRIP (bn_bwd_apply's second trip), 17 row chunks
PACKED_BN_SHAPES = [(3, 5, 7), (700, 1000, 200), (4100, 4200, 257)]


# ------------------------------------------------------------------------------------------------ grid-stride totals
STREAM_TOTALS = [1, 255, 257, STREAM_TRIP + 257]


def factor_rc(total):
    """(R, C) with R*C == total and C no divisor of the trip: the column phase changes between the trips."""
    return {1: (1, 1), 255: (5, 51), 257: (1, 257), STREAM_TRIP + 257: (116537, 9)}[total]


def att_rf(total):
    """att_update covers rows * 2F elements, an even number: the nearest even totals on the same side of every bound."""
    return {1: (1, 1), 255: (1, 127), 257: (3, 43), STREAM_TRIP + 257: (174806, 3)}[total]


def pad_shape(total):
    """(R, R_pad, C, ld_src, ld_dst) with R_pad * ld_dst == total (1: nothing to pad)."""
    return {1: (1, 1, 1, 1, 1), 255: (4, 5, 50, 53, 51), 257: (1, 1, 255, 256, 257), STREAM_TRIP + 257: (116530, 116537, 7, 8, 9)}[total]


# ------------------------------------------------------------------------------------------------ grad norm / Adam
NORM_SIZES = [1, 255, 256, 257, NORM_TRIP, NORM_TRIP + 1, STREAM_TRIP + 3]      # sumsq_kernel: NORM_BLOCKS x 256 per trip


def norm_inputs(n, clips):
    """A gradient of norm 2 (clipped at 0.25) or 0.05 (not) whose LAST element carries a quarter of the squared norm, so
    that an element lost at the end of the range shows."""
    g = np.random.default_rng(n).standard_normal(n)
    if n > 1:
        g[-1] = np.sign(g[-1]) * math.sqrt(np.sum(g[:-1] ** 2) / 3.0)
    g *= (2.0 if clips else 0.05) / math.sqrt(np.sum(g ** 2))
    return g.astype(F32)


def norm_eval(g, dt=F64, order="pair", defect=None):
    """[norm, clip coefficient] as sumsq_kernel / norm_fin_kernel define them."""
    n = g.shape[0]
    idx = np.arange(min(n, NORM_TRIP)) if defect == "second_trip" else _rows(n, defect, 256)
    v = g[idx].astype(dt)
    norm = np.sqrt(dt(_sum(v * v, dt, order)))
    coef = dt(MAX_NORM) / (norm + dt(CLIP_EPS))
    return np.array([norm, min(coef, dt(1))], dt)


def norm_ref(g):
    return _ref_and_eref(lambda dt, order: norm_eval(g, dt, order))


def norm_defects(n):
    return ["last_row", "last_chunk"] + (["row_shift"] if n >= 2 else []) + (["second_trip"] if n > NORM_TRIP else [])


def ew_adam(p, g, m, v, coef, step, lr=LR, beta1=BETA1, beta2=BETA2, eps=ADAM_EPS):
    """One clip_adam_kernel update (torch tensors): the bias corrections in double, rounded to float where the kernel
    rounds them. -> (p, m, v)"""
    bc1, bc2_sqrt = 1.0 - beta1 ** step, math.sqrt(1.0 - beta2 ** step)
    if p.dtype == torch.float32:
        bc1, bc2_sqrt = float(F32(bc1)), float(F32(bc2_sqrt))
    g = g * coef
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    return p - (lr / bc1) * (m / (torch.sqrt(v) / bc2_sqrt + eps)), m, v


def adam_restated(p0, grads, dtype=torch.float64, lr=LR, beta1=BETA1, beta2=BETA2, eps=ADAM_EPS, max_norm=MAX_NORM, clip_eps=CLIP_EPS):
    """clip_grad_norm_(max_norm) + Adam.step() for the gradients `grads` (steps 1, 2, ...) as the kernels state them:
    returns (p, m, v)."""
    p = p0.to(dtype).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step, g in enumerate(grads, 1):
        g = g.to(dtype)
        coef = torch.clamp(max_norm / (torch.sqrt((g * g).sum()) + clip_eps), max=1.0)
        p, m, v = ew_adam(p, g, m, v, coef, step, lr, beta1, beta2, eps)
    return p, m, v


def adam_inputs(n=1000, calls=6, seed=5):
    """Parameters and one gradient per call; calls 1, 3 and 6 clip (norm 3.2), the others do not."""
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (0.1 if c in (0, 2, 5) else 1e-3) for c in range(calls)]
    return p0, grads


# ------------------------------------------------------------------------------------------------ PIT-MSE
# pit_pair_kernel: TCH = 16 frames per block, whole 256-bin sweeps + tail; pit_finalize: b += 256; S <= SK_MAXS = 4
PIT_SPEAKERS = [1, 2, 3, 4]
PIT_SHAPES = [(1, 1, 1), (15, 3, 255), (16, 3, 256), (17, 5, 257), (33, 2, 513), (3, 257, 5)]


def ragged_lens(T, B):
    """Descending lengths, the longest T; with T > 16 one utterance ends inside the first 16-frame chunk and has an empty
    last chunk."""
    if B == 1:
        return np.array([T], np.int32)
    lens = T - (np.arange(B) * (T - 1)) // (B - 1)
    if B > 2:
        lens[1] = T                       # two utterances of full length: a frame's packed rows are more than one row
    return lens.astype(np.int32)


def perms(S):
    return list(itertools.permutations(range(S)))


def pit_inputs(S, T, B, F):
    """mask (T, B, S*F), mix (T, B, F), srcs S x (T, B, F) zero past every utterance's end; utterance b's sources are its
    masked mixture in the order of permutation want[b] plus noise, so that want[b] wins by a clear margin; want cycles
    through the last, the first and the following permutation indices (23 wins at S = 4)."""
    g = np.random.default_rng(S * 100003 + T * 1009 + B * 31 + F)
    lens = ragged_lens(T, B)
    valid = (np.arange(T)[:, None] < lens[None, :]).astype(F32)[:, :, None]
    mask = g.uniform(0.05, 1.0, (T, B, S * F)).astype(F32)
    mix = (g.uniform(0.2, 1.0, (T, B, F)).astype(F32)) * valid
    pl = perms(S)
    want = np.array([(len(pl) - 1 + b) % len(pl) for b in range(B)], np.int32)
    srcs = [np.zeros((T, B, F), F32) for _ in range(S)]
    for b in range(B):
        for s in range(S):
            est = mask[:, b, s * F:(s + 1) * F] * mix[:, b]
            srcs[pl[want[b]][s]][:, b] = (est + 0.05 * g.standard_normal((T, F))).astype(F32) * valid[:, b]
    return dict(S=S, T=T, B=B, F=F, lens=lens, mask=mask, mix=mix, srcs=srcs, want=want)


def pit_pair(c, dt=F64, order="pair", defect=None):
    """pair[b][s][r] = sum over the utterance's frames and bins of (mask_s * mix - src_r)^2, summed frame-major."""
    S, T, B, F, lens = c["S"], c["T"], c["B"], c["F"], c["lens"]
    tt = np.minimum(np.arange(T) + 1, T - 1) if defect == "row_shift" else np.arange(T)
    m = c["mask"][tt].astype(dt).reshape(T, B, S, 1, F)
    mx = c["mix"][tt].astype(dt).reshape(T, B, 1, 1, F)
    sv = np.stack([s[tt] for s in c["srcs"]], 2).astype(dt).reshape(T, B, 1, S, F)
    d = m * mx - sv
    t = d * d                                                                      # (T, B, S, S, F)
    keep = np.arange(T)[:, None] < lens[None, :]
    if defect == "last_row":
        keep &= np.arange(T)[:, None] < (lens - 1)[None, :]
    if defect == "last_chunk":
        keep &= np.arange(T)[:, None] < ((-(-lens // PIT_TCH) - 1) * PIT_TCH)[None, :]
    t = t * keep.astype(dt)[:, :, None, None, None]
    if defect == "last_col":
        t = t[..., :F - 1]
    t = np.ascontiguousarray(np.moveaxis(t, 4, 1)).reshape(-1, B, S, S)            # (T*F, B, S, S): frame-major, bins inside
    return np.array(_sum(t, dt, order), dt).reshape(B, S, S)


def pit_perm_loss(pair, dt=F64):
    """(S!, B) in itertools.permutations order, the S terms added in order."""
    pair = np.asarray(pair).astype(dt)
    S = pair.shape[1]
    out = []
    for p in perms(S):
        l = np.zeros(pair.shape[0], dt)
        for s in range(S):
            l = l + pair[:, s, p[s]]
        out.append(l)
    return np.stack(out)


def pit_out(best_vals, lens, F, S, norm_dev=None, dt=F64, order="pair", defect=None):
    """out[0..2] = [loss, norm, sum of the best permutation sums / S]."""
    b = np.asarray(best_vals).astype(dt)
    if defect == "second_trip":
        b = b[:256]
    lsum = dt(_sum(b, dt, order)) / dt(S)
    norm = dt(norm_dev) if norm_dev is not None else dt(np.sum(lens)) * dt(F)
    return np.array([lsum / norm, norm, lsum], dt)


def pit_dmask(mask, mix, srcs, best, norm, gscale, S, F):
    """dmask = gscale * 2 / (S * norm) * (mask_s * mix - src_perm[s]) * mix (torch tensors; the elementwise formula)."""
    k = gscale * 2.0 / (S * norm)
    if mask.dtype == torch.float32:
        k = float(F32(F32(gscale) * F32(2) / (F32(S) * F32(norm))))
    pl = perms(S)
    out = torch.empty_like(mask)
    for b in range(mix.shape[1]):
        for s in range(S):
            sv = srcs[pl[int(best[b])][s]][:, b]
            out[:, b, s * F:(s + 1) * F] = k * (mask[:, b, s * F:(s + 1) * F] * mix[:, b] - sv) * mix[:, b]
    return out


def argmin_gap(vals):
    """(arg-min, relative gap between the smallest and the second smallest finite value) per column of vals (n, B)."""
    v = np.asarray(vals, F64)
    idx = np.argmin(v, 0)
    gap = np.full(v.shape[1], np.inf)
    if v.shape[0] > 1:
        srt = np.sort(v, 0)
        ok = np.isfinite(srt[1])
        gap[ok] = (srt[1][ok] - srt[0][ok]) / np.abs(srt[1][ok])
    return idx, gap


# ------------------------------------------------------------------------------------------------ RSH loss
# rsh_sse_kernel<S>: S <= RMAXS = 8, RTCH = 8 frames per block; rsh_select: b += 256
RSH_SPEAKERS = [1, 4, 5, 8]
RSH_SHAPES = [(1, 1, 1), (8, 3, 256), (9, 5, 257), (17, 2, 513), (3, 257, 5)]


def rsh_inputs(S, T, B, F):
    """mask (T, B, F), x (T, B, 2F) = [mixture | attention], srcs S x (T, B, F), used (S, B): column b has 0, 1 or S - 1
    sources taken (b % 3).  Source r of utterance b is its masked mixture scaled by a factor of its own, so that the sums
    of squared errors of one utterance are well apart."""
    g = np.random.default_rng(S * 100019 + T * 1013 + B * 37 + F)
    lens = ragged_lens(T, B)
    valid = (np.arange(T)[:, None] < lens[None, :]).astype(F32)[:, :, None]
    mask = g.uniform(0.05, 1.0, (T, B, F)).astype(F32)
    x = np.concatenate([g.uniform(0.2, 1.0, (T, B, F)).astype(F32) * valid, g.uniform(0.0, 1.0, (T, B, F)).astype(F32) * valid], 2)
    srcs = []
    for r in range(S):
        amp = (1.0 + 0.25 * ((r * 3 + np.arange(B)) % S + 1)).astype(F32)[None, :, None]
        srcs.append((mask * x[:, :, :F] * amp + 0.02 * g.standard_normal((T, B, F)).astype(F32)) * valid)
    used = np.zeros((S, B), np.int32)
    for b in range(B):
        if b % 3 == 1:
            used[b % S, b] = 1
        elif b % 3 == 2:
            used[:, b] = 1
            used[b % S, b] = 0
    return dict(S=S, T=T, B=B, F=F, lens=lens, mask=mask, x=np.ascontiguousarray(x), srcs=[np.ascontiguousarray(s) for s in srcs], used=used)


def rsh_sse(c, dt=F64, order="pair", defect=None):
    """sse[r][b] = sum over all frames and bins of (mask * mix - src_r)^2 (zero rows past an utterance's end add nothing)."""
    S, T, B, F = c["S"], c["T"], c["B"], c["F"]
    tt = np.arange(T)
    if defect == "row_shift":
        tt = np.minimum(tt + 1, T - 1)
    elif defect == "last_row":
        tt = tt[:-1]
    elif defect == "last_chunk":
        tt = tt[:(-(-T // RSH_TCH) - 1) * RSH_TCH]
    mm = c["mask"][tt].astype(dt) * c["x"][tt][:, :, :F].astype(dt)
    out = []
    for r in range(S):
        d = mm - c["srcs"][r][tt].astype(dt)
        t = d * d
        if defect == "last_col":
            t = t[..., :F - 1]
        t = np.ascontiguousarray(np.moveaxis(t, 2, 1)).reshape(-1, B)
        out.append(np.array(_sum(t, dt, order), dt).reshape(B))
    return np.stack(out)


def rsh_select(sse, used):
    """The greedy rule (archs/RSH.py:229-244): sources already taken count as +inf, the first smallest wins and is marked.
    -> (sel (B), used after the pass, the winning values (B))."""
    v = np.where(used != 0, np.inf, np.asarray(sse, F64))
    sel = np.argmin(v, 0).astype(np.int32)
    cols = np.arange(v.shape[1])
    new = used.copy()
    new[sel, cols] = 1
    return sel, new, v[sel, cols]


def rsh_out(best_vals, lens, F, S, dt=F64, order="pair", defect=None):
    b = np.asarray(best_vals).astype(dt)
    if defect == "second_trip":
        b = b[:256]
    with np.errstate(invalid="ignore"):
        tot = dt(_sum(b, dt, order))
    return np.array([tot / dt(S), dt(np.sum(lens)) * dt(F)], dt)


def rsh_dmask(mask, mx, srcs, sel, gscale, S):
    k = gscale * 2.0 / S
    if mask.dtype == torch.float32:
        k = float(F32(F32(gscale) * F32(2) / F32(S)))
    out = torch.empty_like(mask)
    for b in range(mask.shape[1]):
        out[:, b] = k * (mask[:, b] * mx[:, b] - srcs[int(sel[b])][:, b]) * mx[:, b]
    return out


# ------------------------------------------------------------------------------------------------ row converters
CONVERT_SHAPES = [(1, 1), (5, 7), (64, 257), (130, 260), (2050, 4100)]    # the last: past cast's 4096- and split's 8192-block caps


def convert_input(R, C, seed=0):
    """Values spread over 2^-20 .. 2^20 with exact zeros among them."""
    g = torch.Generator().manual_seed(R * 7919 + C + seed)
    x = torch.randn(R, C, generator=g) * torch.exp2(torch.rand(R, C, generator=g) * 40.0 - 20.0)
    x[torch.rand(R, C, generator=g) < 0.05] = 0.0
    return x


def split3(x):
    """The three bf16 pieces of fp32 values, round to nearest even: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid)."""
    hi = x.bfloat16()
    r1 = x - hi.float()
    mid = r1.bfloat16()
    lo = (r1 - mid.float()).bfloat16()
    return hi, mid, lo
