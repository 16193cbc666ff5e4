"""The streaming kernels (csrc/bn_optim.hip, pit.hip, rsh.hip, packed.hip, the row converters of gemm.hip) at the shapes
their loops branch on, against float64 references of the same formulas.

Cases, references and the tolerance rule  err <= k * E_ref + eps  are tests/_streaming_cases.py's; the CPU file
tests/test_streaming_cases.py proves that a kernel with a dropped row, chunk, column or stride-loop trip misses these
tolerances by 10 x.  A multi-stage operation is checked stage by stage on the kernel's own output of the stage before, and
once as a whole against torch.nn.BatchNorm1d in float64.  Copies and selections are bit-exact.

Every figure is printed before it is asserted (pytest -s shows them); with SEPKERN_STREAMING_REPORT=<file> the
per-family ratios are written there -- profiles/streaming_kernels.txt is such a file.
"""
import os
import time

import numpy as np
import pytest
import torch

import _streaming_cases as SC
from _streaming_cases import F32, F64

pytestmark = pytest.mark.gpu

RATIOS = []          # (family, what, err, E_ref, eps, smallest k that would pass)
T0 = time.time()


def _report():
    lines = ["family        checks   max (err - eps) / E_ref   asserted k"]
    for fam in SC.K:
        rs = [r for r in RATIOS if r[0] == fam]
        if rs:
            worst = max(rs, key=lambda r: r[5])
            lines.append("%-12s %7d   %-25.3f %d     (worst: %s, err %.3e, E_ref %.3e, eps %.3e)"
                         % (fam, len(rs), worst[5], SC.K[fam], worst[1], worst[2], worst[3], worst[4]))
    lines.append("wall time of the module: %.1f s" % (time.time() - T0))
    print("\n" + "\n".join(lines))
    path = os.environ.get("SEPKERN_STREAMING_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n\nevery check:\n")
            for r in RATIOS:
                f.write("%-12s %-64s err %.3e  E_ref %.3e  eps %.3e  k %.3f\n" % r)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    from sepkern import ops as _ops
    yield _ops
    _report()


def dev(a):
    return (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a).cuda()


def host(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def close(family, what, got, ref, e_ref):
    """err <= K[family] * E_ref + eps, k from profiles/streaming_kernels.txt (tests/_streaming_cases.py K)."""
    got, ref = host(got), np.asarray(ref, F64)
    err, tol = SC.maxerr(got, ref), SC.tolerance(family, ref, e_ref)
    need = SC.needed_k(err, ref, e_ref)
    RATIOS.append((family, what, err, e_ref, SC.ulp32(ref), need))
    print("%-12s %-64s err %.3e  E_ref %.3e  eps %.3e  k %.3f" % RATIOS[-1])
    assert err <= tol, "%s: error %.3e > %d x %.3e + %.3e (needs k = %.2f)" % (what, err, SC.K[family], e_ref, SC.ulp32(ref), need)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


def all_nan(t):
    return bool(torch.isnan(t.float()).all())


# ------------------------------------------------------------------------------------ column reductions
# colred_kernel: 64 columns x RCH = 256-row chunks x 4 row lanes; colfin kernels: 256 columns per block
@pytest.mark.parametrize("name,R,C,count,tight", SC.col_cases(), ids=[c[0] for c in SC.col_cases()])
def test_column_reductions(ops, name, R, C, count, tight):
    c = SC.col_inputs(R, C, tight)
    x, dy = c["x"], c["dy"]
    xg, dyg = dev(x), dev(dy)
    mean, var = torch.empty(C).cuda(), torch.empty(C).cuda()
    ops.bn_stats(xg, mean, var, count=count)
    ref, e = SC.col_ref("mean", x, count=count)
    close("colred", "%s mean" % name, mean, ref, e)
    mean_k = host(mean)
    ref, e = SC.col_ref("var", x, mean=mean_k, count=count)
    close("colred", "%s var" % name, var, ref, e)
    var_k = host(var)
    dg, db = torch.empty(C).cuda(), torch.empty(C).cuda()
    ops.bn_bwd_sums(dyg, xg, mean, var, dg, db, SC.EPS)
    ref, e = SC.col_ref("dbeta", x, dy=dy)
    close("colred", "%s dbeta" % name, db, ref, e)
    ref, e = SC.col_ref("dgamma", x, dy=dy, mean=mean_k, var=var_k)
    close("colred", "%s dgamma" % name, dg, ref, e)
    out = torch.full((C,), float("nan")).cuda()
    ops.colsum(xg, R, C, C, out)
    ref, e = SC.col_ref("colsum", x)
    close("colred", "%s colsum" % name, out, ref, e)


@pytest.mark.parametrize("R,C", SC.COL_SHAPES)
def test_colsum_of_columns_inside_a_wider_matrix_accumulates(ops, R, C):
    g = np.random.default_rng(R + C)
    wide = (0.3 + 0.5 * g.standard_normal((R, C + 13))).astype(F32)
    base = g.standard_normal(C).astype(F32)
    out = dev(base)
    ops.colsum(dev(wide)[:, 5:], R, C, C + 13, out, accumulate=True)              # ld > C, a column offset, accumulate
    ref, e = SC.col_ref("colsum", np.ascontiguousarray(wide[:, 5:5 + C]), base=base)
    close("colred", "%dx%d colsum ld+13 off 5 accumulate" % (R, C), out, ref, e)


# ------------------------------------------------------------------------------------ BatchNorm chain, packed backward
# PACKED_BN_SHAPES: count > R (the engine's only path); (4100, 4200, 257): R*C > 4096 x 256, bn_bwd_apply's second trip
@pytest.mark.parametrize("R,count,C", SC.PACKED_BN_SHAPES + [(R, R, C) for R, C in SC.COL_SHAPES])
def test_bn_forward_backward_on_packed_rows_matches_batchnorm1d(ops, R, count, C):
    c = SC.col_inputs(R, C)
    x, dy, gamma, beta = c["x"], c["dy"], c["gamma"], c["beta"]
    ref = SC.bn_chain_torch64(x, dy, gamma, beta, count)                           # float64 autograd on the padded grid
    e = SC.bn_chain_eref(x, dy, gamma, beta, count, ref)
    tag = "bn (%d, %d, %d)" % (R, count, C)
    xg, dyg, gg, bg = dev(x), dev(dy), dev(gamma), dev(beta)
    mean, var = torch.empty(C).cuda(), torch.empty(C).cuda()
    ops.bn_stats(xg, mean, var, count=count)
    # running statistics: guard NULL, zero, non-zero
    for guard in (None, torch.zeros(1, dtype=torch.int32).cuda()):
        rm, rv = torch.zeros(C).cuda(), torch.ones(C).cuda()
        ops.bn_update_running(mean, var, rm, rv, count, 0.1, guard=guard)
        close("bn_chain", "%s running_mean guard %s" % (tag, "NULL" if guard is None else "0"), rm, ref["running_mean"], e["running_mean"])
        close("bn_chain", "%s running_var guard %s" % (tag, "NULL" if guard is None else "0"), rv, ref["running_var"], e["running_var"])
    (r_rm, r_rv), (e_rm, e_rv) = SC.ew_ref(SC.ew_running, host(mean), host(var), np.zeros(C, F32), np.ones(C, F32), count, 0.1)
    close("elementwise", "%s bn_running mean" % tag, rm, r_rm, e_rm)
    close("elementwise", "%s bn_running var" % tag, rv, r_rv, e_rv)
    before = (rm.clone(), rv.clone())
    ops.bn_update_running(mean, var, rm, rv, count, 0.1, guard=torch.full((1,), 7, dtype=torch.int32).cuda())
    assert same_bits(rm, before[0]) and same_bits(rv, before[1])                   # a raised guard word: left alone
    y = torch.empty(R, C).cuda()
    ops.bn_apply(xg, mean, var, gg, bg, y, SC.EPS)
    dg, db, dx = torch.empty(C).cuda(), torch.empty(C).cuda(), torch.empty(R, C).cuda()
    ops.bn_bwd_sums(dyg, xg, mean, var, dg, db, SC.EPS)
    ops.bn_bwd_apply(dyg, xg, mean, var, gg, dg, db, dx, count, SC.EPS)
    for k, got in (("mean", mean), ("var", var), ("y", y), ("dgamma", dg), ("dbeta", db), ("dx", dx)):
        close("bn_chain", "%s %s" % (tag, k), got, ref[k], e[k])
    # each elementwise kernel on its own, from the kernels' statistics and sums
    r, er = SC.ew_ref(SC.ew_bn_apply, x, host(mean), host(var), gamma, beta)
    close("elementwise", "%s bn_apply" % tag, y, r, er)
    r, er = SC.ew_ref(SC.ew_bn_bwd_apply, dy, x, host(mean), host(var), gamma, host(dg), host(db), count)
    close("elementwise", "%s bn_bwd_apply" % tag, dx, r, er)
    if count == R:                                                                 # the one-call form is the same two kernels
        dg2, db2, dx2 = torch.empty(C).cuda(), torch.empty(C).cuda(), torch.empty(R, C).cuda()
        ops.bn_bwd(dyg, xg, mean, var, gg, dx2, dg2, db2, SC.EPS)
        assert same_bits(dx2, dx) and same_bits(dg2, dg) and same_bits(db2, db)


# ------------------------------------------------------------------------------------ grid-stride kernels
# stream_blocks() / rsh_blocks(): at most 4096 blocks x 256 threads = 1 048 576 elements per trip of the stride loop
@pytest.mark.parametrize("total", SC.STREAM_TOTALS)
def test_stride_loop_bn_apply_and_backward(ops, total):
    R, C = SC.factor_rc(total)
    g = np.random.default_rng(total)
    x, dy = (0.3 + 0.5 * g.standard_normal((R, C))).astype(F32), g.standard_normal((R, C)).astype(F32)
    mean, var = (0.3 + 0.1 * g.standard_normal(C)).astype(F32), g.uniform(0.1, 0.5, C).astype(F32)
    gamma, beta = g.uniform(0.5, 1.5, C).astype(F32), g.standard_normal(C).astype(F32)
    dgam, dbet = (g.standard_normal(C) * 30).astype(F32), (g.standard_normal(C) * 30).astype(F32)
    out = torch.full((R * C + 64,), float("nan")).cuda()
    ops.bn_apply(dev(x), dev(mean), dev(var), dev(gamma), dev(beta), out[:R * C].view(R, C), SC.EPS)
    r, e = SC.ew_ref(SC.ew_bn_apply, x, mean, var, gamma, beta)
    close("elementwise", "bn_apply total %d" % total, out[:R * C].view(R, C), r, e)
    assert all_nan(out[R * C:])
    out.fill_(float("nan"))
    count = R + 3
    ops.bn_bwd_apply(dev(dy), dev(x), dev(mean), dev(var), dev(gamma), dev(dgam), dev(dbet), out[:R * C].view(R, C), count, SC.EPS)
    r, e = SC.ew_ref(SC.ew_bn_bwd_apply, dy, x, mean, var, gamma, dgam, dbet, count)
    close("elementwise", "bn_bwd_apply total %d" % total, out[:R * C].view(R, C), r, e)
    assert all_nan(out[R * C:])


@pytest.mark.parametrize("total", SC.STREAM_TOTALS)
def test_stride_loop_sigmoid_bwd_unfold_grad_clip_adam(ops, total):
    g = np.random.default_rng(total + 1)
    m, dm = g.uniform(0, 1, total).astype(F32), g.standard_normal(total).astype(F32)
    out = torch.full((total + 64,), float("nan")).cuda()
    ops.sigmoid_bwd(dev(dm), dev(m), out[:total])
    r, e = SC.ew_ref(SC.ew_sigmoid_bwd, dm, m)
    close("elementwise", "sigmoid_bwd n %d" % total, out[:total], r, e)
    assert all_nan(out[total:])
    # bn_unfold_grad: dW (O, C) from G (O, ldg > C)
    O, C = SC.factor_rc(total)
    G = g.standard_normal((O, C + 3)).astype(F32)
    dz, s, t, dW0 = (g.standard_normal(n).astype(F32) for n in (O, C, C, O * C))
    for acc in (False, True):
        dW = torch.full((total + 64,), float("nan")).cuda()
        dW[:total] = dev(dW0)
        ops.bn_unfold_grad(dev(G), dev(dz), dev(s), dev(t), dW[:total].view(O, C), accumulate=acc)
        r, e = SC.ew_ref(SC.ew_unfold_grad, np.ascontiguousarray(G[:, :C]), dz, s, t, dW0.reshape(O, C) if acc else None)
        close("elementwise", "bn_unfold_grad total %d accumulate %d" % (total, acc), dW[:total].view(O, C), r, e)
        assert all_nan(dW[total:])
    # clip_adam: one update, third step, a clip coefficient of 0.5
    p, gr, m1 = (g.standard_normal(total).astype(F32) for _ in range(3))
    gr *= F32(0.01)
    m1 *= F32(0.01)
    v1 = (g.uniform(0, 1e-4, total)).astype(F32)
    buf = torch.full((3, total + 64), float("nan")).cuda()
    for i, a in enumerate((p, m1, v1)):
        buf[i, :total] = dev(a)
    scal = torch.tensor([1.0, 0.5, 0.0, 0.0]).cuda()
    ops.clip_adam(buf[0, :total], dev(gr), buf[1, :total], buf[2, :total], scal, SC.LR, SC.BETA1, SC.BETA2, SC.ADAM_EPS, 3)
    refs, es = SC.ew_ref(lambda *a: SC.ew_adam(*a, 0.5, 3), p, gr, m1, v1)
    for i, name in enumerate("pmv"):
        close("elementwise", "clip_adam n %d %s" % (total, name), buf[i, :total], refs[i], es[i])
    assert all_nan(buf[:, total:])
    scal[2] = 1.0                                                                  # a step marked to be skipped touches nothing
    before = buf.clone()
    ops.clip_adam(buf[0, :total], dev(gr), buf[1, :total], buf[2, :total], scal, SC.LR, SC.BETA1, SC.BETA2, SC.ADAM_EPS, 4)
    assert same_bits(buf[:, :total], before[:, :total])


@pytest.mark.parametrize("total", SC.STREAM_TOTALS)
def test_stride_loop_attention_update_is_exact(ops, total):
    rows, F = SC.att_rf(total)                                                    # rows * 2F elements: the even neighbour of total
    g = torch.Generator().manual_seed(total)
    x, mk = torch.rand(rows, 2 * F, generator=g), torch.rand(rows, F, generator=g)
    dout = torch.randn(rows, 2 * F, generator=g)
    for relu in (True, False):
        want = x - torch.cat((torch.zeros_like(mk), mk), 1)
        gate = (want > 0).float() if relu else torch.ones_like(want)
        want = torch.relu(want) if relu else want
        out = ops.att_update(dev(x), dev(mk), relu)
        assert torch.equal(out.cpu(), want)
        dx, dmk = ops.att_update_bwd(dev(dout), out, F, relu)
        assert torch.equal(dx.cpu(), dout * gate) and torch.equal(dmk.cpu(), -(dout * gate)[:, F:])


@pytest.mark.parametrize("total", SC.STREAM_TOTALS)
def test_stride_loop_pad_rows_inside_a_sentinel_buffer(ops, total):
    from sepkern import _lib
    R, R_pad, C, ld_src, ld_dst = SC.pad_shape(total)                             # ld_src > C, ld_dst > C, R_pad > R (total > 1)
    g = torch.Generator().manual_seed(total)
    src = torch.randn(R, ld_src, generator=g)
    big = torch.full((total + 128,), float("nan")).cuda()
    dst = big[64:64 + total]
    srcg = dev(src)
    _lib.call("sk_pad_rows", ops._ptr(srcg), R, C, ld_src, ops._ptr(dst), ld_dst, R_pad, ops._stream())
    want = torch.zeros(R_pad, ld_dst)
    want[:R, :C] = src[:, :C]
    assert same_bits(dst.view(R_pad, ld_dst), want)
    assert all_nan(big[:64]) and all_nan(big[64 + total:])
    if total > 1:
        assert same_bits(ops.pad_rows(srcg[:, :C], ld_dst, R_pad), want)           # the wrapper, a strided view as its source


# ------------------------------------------------------------------------------------ grad norm / clip + Adam
# sumsq_kernel: NORM_BLOCKS = 1024 blocks x 256 threads = 262 144 elements per trip; n < 256: one partial block
@pytest.mark.parametrize("clips", [True, False])
@pytest.mark.parametrize("n", SC.NORM_SIZES)
def test_grad_norm(ops, n, clips):
    g = SC.norm_inputs(n, clips)
    scal = torch.tensor([float("nan"), float("nan"), float("nan"), 3.0]).cuda()
    ops.grad_norm(dev(g), SC.MAX_NORM, scal)
    ref, e = SC.norm_ref(g)
    close("grad_norm", "grad_norm n %d %s" % (n, "clips" if clips else "no clip"), scal[:2], ref, e)
    s = scal.cpu()
    assert (float(s[1]) < 1.0) == clips and float(s[2]) == 0.0 and float(s[3]) == 3.0


def test_clip_adam_after_skipped_steps_is_adam_on_the_applied_gradients(ops):
    """Six calls, the guard word raised on calls 2 and 5: the weights and moments are those of an Adam that saw the four
    applied gradients as its steps 1..4 (the bias correction uses step - scal[3])."""
    p0, grads = SC.adam_inputs(1000, 6)
    n = p0.numel()
    p, m, v, scal = dev(p0.clone()), torch.zeros(n).cuda(), torch.zeros(n).cuda(), torch.zeros(4).cuda()
    applied, skipped = [], 0
    for call in range(1, 7):
        skip = call in (2, 5)
        g = dev(grads[call - 1])
        before = (p.clone(), m.clone(), v.clone())
        ops.grad_norm(g, SC.MAX_NORM, scal, guard=torch.full((1,), 1.0 if skip else 0.0).cuda())
        ops.clip_adam(p, g, m, v, scal, SC.LR, SC.BETA1, SC.BETA2, SC.ADAM_EPS, call)
        skipped += skip
        s = scal.cpu()
        assert float(s[2]) == float(skip) and float(s[3]) == skipped
        if skip:
            assert all(same_bits(a, b) for a, b in zip((p, m, v), before))
        else:
            applied.append(grads[call - 1])
            assert not torch.equal(p, before[0])
    ref = SC.adam_restated(p0, applied)
    got32 = SC.adam_restated(p0, applied, dtype=torch.float32)
    for name, got, r, g32 in zip("pmv", (p, m, v), ref, got32):
        close("adam_skip", "clip_adam 6 calls, 2 skipped: %s" % name, got, r.numpy(), SC.maxerr(g32.numpy(), r.numpy()))


# ------------------------------------------------------------------------------------ PIT-MSE
# pit_pair_kernel<S>: S <= SK_MAXS = 4 (4 is the switch's default:), TCH = 16 frames per block, 256-bin sweeps + tail;
# pit_finalize_kernel: b += 256; pit_bwd_kernel: RB = 4 rows per block
@pytest.mark.parametrize("T,B,F", SC.PIT_SHAPES)
@pytest.mark.parametrize("S", SC.PIT_SPEAKERS)
def test_pit_mse_forward_backward(ops, S, T, B, F):
    from sepkern.packing import Packing
    c = SC.pit_inputs(S, T, B, F)
    lens = c["lens"]
    tag = "pit S%d (%d, %d, %d)" % (S, T, B, F)
    pair_ref, e_pair = SC._ref_and_eref(lambda dt, order: SC.pit_pair(c, dt, order))
    best_ref = np.argmin(SC.pit_perm_loss(pair_ref), 0)
    mask, mix, srcs = dev(c["mask"]), dev(c["mix"]), [dev(s) for s in c["srcs"]]
    gscale = 0.75
    pk = Packing.from_lens(lens, "cuda")
    assert pk.perm is None and pk.Rp > pk.R
    packed = (pk.pack(mask), pk.pack(mix), [pk.pack(s) for s in srcs])
    odd = (S + T) % 2 == 1                                                        # norm_dev: on the padded or on the packed run
    for layout, (km, kx, ks) in (("padded", (mask, mix, srcs)), ("packed", packed)):
        nd = float(F32(1234.5)) if odd == (layout == "padded") else None
        res = ops.pit_mse_fwd(km, kx, ks, dev(lens) if layout == "padded" else None, norm_dev=None if nd is None else torch.tensor([nd]).cuda(),
                              packing=pk if layout == "packed" else None)
        what = "%s %s%s" % (tag, layout, " norm_dev" if nd else "")
        close("pit", what + " pair", res["pair"], pair_ref, e_pair)
        pair_k = host(res["pair"])
        pl_ref = SC.pit_perm_loss(pair_k)                                          # all S! columns, itertools.permutations order
        close("pit", what + " perm_loss", res["perm_loss"], pl_ref, SC.maxerr(SC.pit_perm_loss(pair_k, F32), pl_ref))
        assert host(res["best_perm"]).tolist() == best_ref.tolist()
        bv = host(res["perm_loss"]).min(0)
        out_ref, e_out = SC._ref_and_eref(lambda dt, order: SC.pit_out(bv, lens, F, S, nd, dt, order))
        close("pit", what + " out", res["out"], out_ref, e_out)
        norm_k = float(host(res["out"])[1])
        dm = ops.pit_mse_bwd(km, kx, ks, res["best_perm"], res["out"], torch.tensor([gscale]).cuda(), packing=pk if layout == "packed" else None)
        if layout == "packed":
            assert dm.shape[0] == pk.Rp and float(dm[pk.R:].abs().sum()) == 0      # tail rows of the (Rp, .) buffer stay zero
            dm = pk.unpack(dm)
        tm, tx, ts = torch.from_numpy(c["mask"]), torch.from_numpy(c["mix"]), [torch.from_numpy(s) for s in c["srcs"]]
        dm_ref = SC.pit_dmask(tm.double(), tx.double(), [s.double() for s in ts], best_ref, norm_k, gscale, S, F).numpy()
        e_dm = SC.maxerr(SC.pit_dmask(tm, tx, ts, best_ref, norm_k, gscale, S, F).numpy(), dm_ref)
        close("pit", what + " dmask", dm, dm_ref, e_dm)


# ------------------------------------------------------------------------------------ RSH loss
# rsh_sse_kernel<S>: S <= RMAXS = 8 (one instantiation each), RTCH = 8 frames per block; rsh_select_kernel: b += 256
@pytest.mark.parametrize("T,B,F", SC.RSH_SHAPES)
@pytest.mark.parametrize("S", SC.RSH_SPEAKERS)
def test_rsh_loss_three_passes(ops, S, T, B, F):
    c = SC.rsh_inputs(S, T, B, F)
    tag = "rsh S%d (%d, %d, %d)" % (S, T, B, F)
    sse_ref, e_sse = SC._ref_and_eref(lambda dt, order: SC.rsh_sse(c, dt, order))
    mask, x, srcs, lens = dev(c["mask"]), dev(c["x"]), [dev(s) for s in c["srcs"]], dev(c["lens"])
    tm, tx, ts = torch.from_numpy(c["mask"]), torch.from_numpy(c["x"][:, :, :F].copy()), [torch.from_numpy(s) for s in c["srcs"]]
    used_ref = c["used"].copy()
    used = dev(c["used"].copy())
    for p in range(3):
        res = ops.rsh_loss_fwd(mask, x, srcs, lens, used)
        what = "%s pass %d" % (tag, p + 1)
        close("rsh", what + " sse", res["sse"], sse_ref, e_sse)
        sel64, _, _ = SC.rsh_select(sse_ref, used_ref)                            # the greedy rule on the float64 sums ...
        sel, used_ref, best = SC.rsh_select(host(res["sse"]), used_ref)           # ... and on the kernel's own
        assert sel.tolist() == sel64.tolist() == host(res["sel"]).tolist()
        assert np.array_equal(host(used), used_ref)
        out_ref, e_out = SC._ref_and_eref(lambda dt, order: SC.rsh_out(best, c["lens"], F, S, dt, order))
        close("rsh", what + " out", res["out"], out_ref, e_out)
        dm = ops.rsh_loss_bwd(mask, x, srcs, res["sel"], torch.tensor([0.75]).cuda())
        dm_ref = SC.rsh_dmask(tm.double(), tx.double(), [s.double() for s in ts], sel, 0.75, S).numpy()
        close("rsh", what + " dmask", dm, dm_ref, SC.maxerr(SC.rsh_dmask(tm, tx, ts, sel, 0.75, S).numpy(), dm_ref))


# ------------------------------------------------------------------------------------ packed-row movers
# pack_rows_kernel: ROWS = 8 sorted positions per block, column loop c += 256
@pytest.mark.parametrize("C,B,pad,shuffle", [(1, 1, 0, False), (1, 7, 12, True), (256, 8, 0, True), (256, 9, 12, False), (257, 7, 12, True),
                                             (257, 41, 0, True), (600, 9, 12, True), (600, 8, 0, False), (257, 1, 12, False), (600, 41, 12, True)])
def test_pack_unpack_rows_in_sentinel_buffers(ops, C, B, pad, shuffle):
    from torch.nn.utils.rnn import pack_padded_sequence
    from sepkern.packing import Packing
    g = np.random.default_rng(C * 100 + B)
    T = 6
    lens = np.sort(g.integers(1, T + 1, B))[::-1].copy()
    lens[0] = T
    if shuffle:
        lens = g.permutation(lens)
    x = torch.from_numpy(g.standard_normal((T, B, C)).astype(F32))
    for b, n in enumerate(lens):
        x[n:, b] = 0
    pk = Packing.from_lens(lens, "cuda")
    order = np.argsort(-lens, kind="stable")
    assert (pk.perm is not None) == bool(np.any(lens[1:] > lens[:-1]))
    if pk.perm is not None:
        assert np.array_equal(pk.perm_host, order)
    ref = pack_padded_sequence(x[:, torch.from_numpy(order)], torch.from_numpy(lens[order].copy()), enforce_sorted=True).data
    ld = C + pad
    rows = torch.full((pk.R + 3, ld), float("nan")).cuda()
    ops.pack_rows(dev(x), pk, rows)
    assert same_bits(rows[:pk.R, :C], ref)
    assert all_nan(rows[pk.R:]) and all_nan(rows[:, C:])                           # padding rows and columns keep their sentinel
    fill = torch.from_numpy(g.standard_normal(C).astype(F32))
    for f in (None, fill):
        big = torch.full((T + 1, B, C), float("nan")).cuda()
        ops.unpack_rows(rows, pk, big[:T], None if f is None else dev(f))
        want = x.clone()
        if f is not None:
            for b, n in enumerate(lens):
                want[n:, b] = f
        assert same_bits(big[:T], want) and all_nan(big[T])


# hprev_rows_kernel: i < 2 (H / 4) float4 per row, step 256 (H > 512: a second trip); ROWS = 8 positions per block
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("H,lens", [(4, [6] + [1] * 40), (128, [9, 7, 7, 3]), (516, [5, 3, 3, 1, 1, 1, 1, 1, 1]), (896, [4, 4, 2, 1]), (516, [6] + [1] * 40)])
def test_hprev_rows_in_a_sentinel_buffer(ops, H, lens, bf16):
    from sepkern.packing import Packing
    g = torch.Generator().manual_seed(H + len(lens))
    T, B = max(lens), len(lens)
    y = torch.randn(T, B, 2 * H, generator=g)
    h0 = torch.randn(2, B, H, generator=g)
    want = torch.zeros(T, B, 2 * H)
    for b, n in enumerate(lens):
        for t in range(n):
            want[t, b, :H] = y[t - 1, b, :H] if t > 0 else h0[0, b]
            want[t, b, H:] = y[t + 1, b, H:] if t + 1 < n else h0[1, b]
    pk = Packing.from_lens(lens, "cuda")
    yp = pk.pack(dev(y))
    dt = torch.bfloat16 if bf16 else torch.float32
    out = torch.full((pk.R + 2, 2 * H + 8), float("nan"), dtype=dt).cuda()          # ld_out > 2H
    ops.hprev_rows(yp, dev(h0), pk, H, out)
    wp = pk.pack(dev(want))[:pk.R].cpu()
    assert same_bits(out[:pk.R, :2 * H], wp.to(dt))
    assert all_nan(out[pk.R:]) and all_nan(out[:, 2 * H:])


# ------------------------------------------------------------------------------------ row converters (gemm.hip)
# cast_kernel: at most 4096 blocks x 256 threads x 8 columns; split_rows_kernel: 8192 x 256 x 4; both: a vector path for
# aligned rows, a scalar path otherwise
def _view(x, kind):
    R, C = x.shape
    if kind == "dense":
        return x.cuda()
    if kind == "odd_ld":                                                          # row stride not a multiple of 4 floats
        ld = C + 1 + ((C + 1) % 4 == 0)
        base = torch.full((R, ld), float("nan")).cuda()
        base[:, :C] = x.cuda()
        return base[:, :C]
    ld = (C + 3) // 4 * 4                                                         # "offset": 4 bytes past a 16-byte boundary
    base = torch.full((R * ld + 8,), float("nan")).cuda()
    assert base.data_ptr() % 16 == 0
    v = base[1:1 + R * ld].view(R, ld)[:, :C]
    v.copy_(x.cuda())
    return v


@pytest.mark.parametrize("R,C,kind", [(R, C, k) for R, C in SC.CONVERT_SHAPES[:-1] for k in ("dense", "odd_ld", "offset")] +
                         [(2050, 4100, "dense"), (2050, 4100, "offset")])
def test_cast_and_split_rows_are_exact(ops, R, C, kind):
    x = SC.convert_input(R, C)
    xv = _view(x, kind)
    assert same_bits(xv, x) and xv.data_ptr() % 16 == (4 if kind == "offset" else 0)
    assert kind != "odd_ld" or xv.stride(0) % 4 != 0
    rows = R + 3                                                                   # rows > R
    out = ops.cast_bf16(xv, rows=rows)
    ld = out.shape[1]
    assert out.shape == (rows, (C + 63) // 64 * 64)
    assert same_bits(out[:R, :C], x.bfloat16())
    assert not bits(out[R:].cpu()).any() and not bits(out[:, C:].cpu()).any()     # padding rows and columns: zero bits
    pl = ops.split_rows(xv)
    assert pl.rows == (R + 63) // 64 * 64 and pl.ld == (C + 7) // 8 * 8 and pl.t.shape == (3, pl.rows, pl.ld)
    planes = pl.t.cpu()
    for got, want in zip(planes, SC.split3(x)):
        assert same_bits(got[:R, :C], want)
    assert torch.equal(planes[:, :R, :C].double().sum(0), x.double())              # hi + mid + lo == x exactly
    assert not bits(planes[:, R:]).any() and not bits(planes[:, :, C:]).any()


# ------------------------------------------------------------------------------------ refusals by the host code
def test_host_rejects_bad_arguments_before_any_launch(ops):
    from sepkern._lib import SepkernError
    T, B, F = 2, 2, 3
    z = lambda *s: torch.zeros(*s).cuda()
    lens = torch.tensor([2, 2], dtype=torch.int32).cuda()
    with pytest.raises(SepkernError, match="outside 1..4"):                        # SK_MAXS
        ops.pit_mse_fwd(z(T, B, 5 * F), z(T, B, F), [z(T, B, F) for _ in range(5)], lens)
    with pytest.raises(SepkernError, match="outside 1..4"):
        ops.pit_mse_bwd(z(T, B, 5 * F), z(T, B, F), [z(T, B, F) for _ in range(5)], torch.zeros(B, dtype=torch.int32).cuda(), z(3), z(1))
    with pytest.raises(SepkernError, match="outside 1..8"):                        # RMAXS
        ops.rsh_loss_fwd(z(T, B, F), z(T, B, 2 * F), [z(T, B, F) for _ in range(9)], lens, torch.zeros(9, B, dtype=torch.int32).cuda())
    with pytest.raises(SepkernError, match="sk_colsum"):                           # ld < C
        ops.colsum(z(4, 6), 4, 6, 5, z(6))
    with pytest.raises(SepkernError, match="sk_pad_rows"):
        ops.pad_rows(z(4, 6), 5)
    with pytest.raises(SepkernError, match="sk_bn_stats"):                         # count < R
        ops.bn_stats(z(4, 6), z(6), z(6), count=3)
    with pytest.raises(SepkernError, match="sk_bn_bwd_apply"):
        ops.bn_bwd_apply(z(4, 6), z(4, 6), z(6), z(6), z(6), z(6), z(6), z(4, 6), 0, 1e-5)
    with pytest.raises(SepkernError, match="sk_clip_adam"):                        # step = 0
        ops.clip_adam(z(8), z(8), z(8), z(8), z(4), 1e-3, 0.9, 0.999, 1e-8, 0)


def test_bn_wrappers_refuse_views_whose_row_stride_is_not_their_width(ops):
    """They pass shape[1] as the row stride: a column-sliced view would be read wrong, so it is refused."""
    from sepkern._lib import SepkernError
    R, C = 6, 5
    wide = torch.randn(R, C + 3).cuda()
    xv, full = wide[:, :C], torch.randn(R, C).cuda()
    assert not xv.is_contiguous() and wide[:4].is_contiguous()
    v = lambda: torch.ones(C).cuda()
    calls = [lambda a: ops.bn_stats(a, v(), v()),
             lambda a: ops.bn_apply(a, v(), v(), v(), v(), torch.empty(R, C).cuda(), 1e-5),
             lambda a: ops.bn_apply(full, v(), v(), v(), v(), a, 1e-5),
             lambda a: ops.bn_bwd(a, full, v(), v(), v(), torch.empty(R, C).cuda(), v(), v(), 1e-5),
             lambda a: ops.bn_bwd_sums(full, a, v(), v(), v(), v(), 1e-5),
             lambda a: ops.bn_bwd_apply(full, a, v(), v(), v(), v(), v(), torch.empty(R, C).cuda(), R, 1e-5),
             lambda a: ops.sigmoid_bwd(a, full, torch.empty(R, C).cuda())]
    for call in calls:
        with pytest.raises(SepkernError, match="contiguous"):
            call(xv)
    mean, var = torch.empty(C + 3).cuda(), torch.empty(C + 3).cuda()
    ops.bn_stats(wide[:4], mean, var)                                             # a row slice of a dense buffer is fine
    ref, e = SC.col_ref("mean", host(wide[:4]))
    close("colred", "row slice mean", mean, ref, e)
