"""The cases of tests/test_gpu_streaming.py can catch what they are meant to catch (runs on any machine).

Every reduction case is run through the defect models of tests/_streaming_cases.py -- a kernel that drops its last row,
its last chunk or its last column, reads the next row, skips the second trip of its stride loop, ignores `count` or takes
the next permutation -- and the error each leaves against the float64 reference must be at least 10 x the tolerance the
GPU test asserts for that case (with the final k of its family).  The arg-min cases have clear winners, and the float64
restatements of Adam and of the three-way bf16 split are checked against torch.
"""
import numpy as np
import pytest
import torch

import _streaming_cases as SC

MARGIN = 10.0


def _caught(family, ref, e_ref, bad, what):
    err, tol = SC.maxerr(bad, ref), SC.tolerance(family, ref, e_ref)
    assert err >= MARGIN * tol, "%s: the defect leaves %.3g, the test tolerates %.3g" % (what, err, tol)


def test_every_family_factor_is_within_the_cap():
    assert all(isinstance(k, int) and 1 <= k <= 8 for k in SC.K.values()), SC.K


@pytest.mark.parametrize("name,R,C,count,tight", SC.col_cases(), ids=[c[0] for c in SC.col_cases()])
def test_column_reduction_cases_catch_every_defect(name, R, C, count, tight):
    c = SC.col_inputs(R, C, tight)
    x, dy = c["x"], c["dy"]
    mean = SC.col_eval("mean", x, count=count).astype(SC.F32)                 # the stage before, as a kernel would hand it on
    var = SC.col_eval("var", x, mean=mean, count=count).astype(SC.F32)
    kws = dict(mean=dict(count=count), var=dict(mean=mean, count=count), dbeta=dict(dy=dy), dgamma=dict(dy=dy, mean=mean, var=var),
               colsum=dict(base=c["beta"]))
    if count > R:                                                             # the reference IS the zero-padded (count, C) grid
        grid = np.zeros((count, C))
        grid[:R] = x
        mean64 = SC.col_eval("mean", x, count=count)
        np.testing.assert_allclose(mean64, grid.mean(0), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(SC.col_eval("var", x, mean=mean64, count=count), grid.var(0), rtol=1e-10)
    for kind in SC.COL_KINDS:
        ref, e_ref = SC.col_ref(kind, x, **kws[kind])
        assert e_ref <= 1e-3 * max(np.abs(ref).max(), 1e-30) or tight, (kind, e_ref)     # the float32 model itself is sane
        for d in SC.col_defects(kind, R, count, tight):
            _caught("colred", ref, e_ref, SC.col_eval(kind, x, defect=d, **kws[kind]), "%s %s %s" % (name, kind, d))


@pytest.mark.parametrize("R,count,C", SC.PACKED_BN_SHAPES + [(R, R, C) for R, C in SC.COL_SHAPES])
def test_bn_chain_restatement_is_batchnorm1d(R, count, C):
    """The numpy chain whose float32 evaluation gives the chain's E_ref is nn.BatchNorm1d + autograd in float64, and using
    count = R where count > R was given shows in dx."""
    c = SC.col_inputs(R, C)
    ref = SC.bn_chain_torch64(c["x"], c["dy"], c["gamma"], c["beta"], count)
    mine = SC.bn_chain(c["x"], c["dy"], c["gamma"], c["beta"], count, SC.F64, "pair")
    for k, v in mine.items():
        np.testing.assert_allclose(v, ref[k], rtol=1e-9, atol=1e-11 * max(1.0, np.abs(ref[k]).max()), err_msg=k)
    if count > R:
        e = SC.bn_chain_eref(c["x"], c["dy"], c["gamma"], c["beta"], count, ref)
        bad = SC.bn_chain(c["x"], c["dy"], c["gamma"], c["beta"], R, SC.F64, "pair")
        for k in ("mean", "var", "y", "dx", "running_var"):
            _caught("bn_chain", ref[k], e[k], bad[k], "bn chain (%d, %d, %d) %s count_R" % (R, count, C, k))


@pytest.mark.parametrize("clips", [True, False])
@pytest.mark.parametrize("n", SC.NORM_SIZES)
def test_grad_norm_cases_catch_every_defect(n, clips):
    g = SC.norm_inputs(n, clips)
    ref, e_ref = SC.norm_ref(g)
    assert (ref[1] < 1.0) == clips
    for d in SC.norm_defects(n):
        _caught("grad_norm", ref, e_ref, SC.norm_eval(g, defect=d), "grad_norm n=%d %s" % (n, d))


@pytest.mark.parametrize("T,B,F", SC.PIT_SHAPES)
@pytest.mark.parametrize("S", SC.PIT_SPEAKERS)
def test_pit_cases_have_clear_winners_and_catch_every_defect(S, T, B, F):
    c = SC.pit_inputs(S, T, B, F)
    pair, e_pair = SC._ref_and_eref(lambda dt, order: SC.pit_pair(c, dt, order))
    pl = SC.pit_perm_loss(pair)
    best, gap = SC.argmin_gap(pl)
    nperm = pl.shape[0]
    assert gap.min() >= 1e-3, gap.min()
    assert len(set(best.tolist())) >= min(3, nperm, B)
    assert S < 4 or 23 in best.tolist()
    for d in ["last_row", "last_chunk", "last_col"] + (["row_shift"] if T >= 2 else []):
        _caught("pit", pair, e_pair, SC.pit_pair(c, defect=d), "pit pair S=%d %s %s" % (S, (T, B, F), d))
    pair32 = pair.astype(SC.F32)
    ref_pl = SC.pit_perm_loss(pair32)
    e_pl = SC.maxerr(SC.pit_perm_loss(pair32, SC.F32), ref_pl)
    bv = ref_pl.min(0).astype(SC.F32)
    ref_out, e_out = SC._ref_and_eref(lambda dt, order: SC.pit_out(bv, c["lens"], F, S, None, dt, order))
    if nperm > 1:                                                             # permutation index p + 1
        nxt = (best + 1) % nperm
        _caught("pit", ref_pl, e_pl, np.roll(ref_pl, -1, axis=0), "pit perm_loss S=%d %s next_perm" % (S, (T, B, F)))
        _caught("pit", ref_out, e_out, SC.pit_out(ref_pl[nxt, np.arange(B)], c["lens"], F, S), "pit out S=%d %s next_perm" % (S, (T, B, F)))
    if B > 256:                                                               # pit_finalize's b += 256
        _caught("pit", ref_out, e_out, SC.pit_out(bv, c["lens"], F, S, defect="second_trip"), "pit out S=%d second_trip" % S)
    # dmask with the next permutation, elementwise
    m, mx, sv = torch.from_numpy(c["mask"]), torch.from_numpy(c["mix"]), [torch.from_numpy(s) for s in c["srcs"]]
    norm = float(ref_out[1])
    ref_dm = SC.pit_dmask(m.double(), mx.double(), [s.double() for s in sv], best, norm, 1.0, S, F).numpy()
    e_dm = SC.maxerr(SC.pit_dmask(m, mx, sv, best, norm, 1.0, S, F).numpy(), ref_dm)
    if nperm > 1:
        bad = SC.pit_dmask(m.double(), mx.double(), [s.double() for s in sv], (best + 1) % nperm, norm, 1.0, S, F).numpy()
        _caught("pit", ref_dm, e_dm, bad, "pit dmask S=%d %s next_perm" % (S, (T, B, F)))


@pytest.mark.parametrize("T,B,F", SC.RSH_SHAPES)
@pytest.mark.parametrize("S", SC.RSH_SPEAKERS)
def test_rsh_cases_have_clear_winners_and_catch_every_defect(S, T, B, F):
    c = SC.rsh_inputs(S, T, B, F)
    sse, e_sse = SC._ref_and_eref(lambda dt, order: SC.rsh_sse(c, dt, order))
    taken = c["used"].sum(0)
    assert set(taken.tolist()) == ({0, 1, S - 1} if B >= 3 else set(taken.tolist()))
    for d in ["last_row", "last_chunk", "last_col"] + (["row_shift"] if T >= 2 else []):
        _caught("rsh", sse, e_sse, SC.rsh_sse(c, defect=d), "rsh sse S=%d %s %s" % (S, (T, B, F), d))
    used, full = c["used"], False
    for _ in range(3):                                                        # the three passes of the GPU test
        v = np.where(used != 0, np.inf, sse)
        _, gap = SC.argmin_gap(v)
        assert gap.min() >= 1e-3, gap.min()
        full = full or bool((used.sum(0) == S).any())
        sel, used, best = SC.rsh_select(sse.astype(SC.F32), used)
        if B > 256 and np.isfinite(best).all():
            ref_out, e_out = SC._ref_and_eref(lambda dt, order: SC.rsh_out(best, c["lens"], F, S, dt, order))
            _caught("rsh", ref_out, e_out, SC.rsh_out(best, c["lens"], F, S, defect="second_trip"), "rsh out S=%d second_trip" % S)
    assert full or B < 3                                                     # a column with every source used was selected from


def test_adam_restatement_is_torch_adam_with_clipping():
    p0, grads = SC.adam_inputs()
    grads = grads[:4]
    pt = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([pt], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    clipped = 0
    for g in grads:
        pt.grad = g.double().clone()
        clipped += float(torch.nn.utils.clip_grad_norm_([pt], SC.MAX_NORM)) > SC.MAX_NORM
        opt.step()
    assert 0 < clipped < 4                                                   # both branches of the clip coefficient
    p, m, v = SC.adam_restated(p0, grads, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, clip_eps=1e-6)
    st = opt.state[pt]
    np.testing.assert_allclose(p.numpy(), pt.detach().numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(m.numpy(), st["exp_avg"].numpy(), rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(v.numpy(), st["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-22)
    # a skipped step that moved the bias correction on (steps 1, 3, 4, 6 instead of 1..4) would show
    p32, _, _ = SC.adam_restated(p0, grads, dtype=torch.float32)
    ref, _, _ = SC.adam_restated(p0, grads)
    e_ref = SC.maxerr(p32.numpy(), ref.numpy())
    bad, _, _ = SC.adam_restated(p0, [grads[0], torch.zeros_like(p0), grads[1]])
    good, _, _ = SC.adam_restated(p0, grads[:2])
    _caught("adam_skip", good.numpy(), e_ref, bad.numpy(), "adam: a skipped call applied as a zero gradient")


@pytest.mark.parametrize("R,C", SC.CONVERT_SHAPES[:-1] + [(300, 500)])
def test_bf16_three_way_split_restatement_reassembles_exactly(R, C):
    x = SC.convert_input(R, C)
    assert bool((x == 0).any()) or R * C < 20
    nz = x[x != 0].abs()
    assert nz.numel() == 0 or (float(nz.max()) < 2.0 ** 23 and float(nz.min()) > 0)
    hi, mid, lo = SC.split3(x)
    assert torch.equal(hi.double() + mid.double() + lo.double(), x.double())
    assert torch.equal(hi, x.bfloat16())
    # a split that truncates instead of rounding, or loses the third piece, does not reassemble
    assert R * C < 20 or not torch.equal(hi.double() + mid.double(), x.double())


def test_stride_loop_totals_cross_their_bounds():
    """The shapes the GPU tests derive from the totals multiply out, and the large ones take the loops' second trip."""
    for total in SC.STREAM_TOTALS:
        R, C = SC.factor_rc(total)
        assert R * C == total and (total < SC.STREAM_TRIP or SC.STREAM_TRIP % C != 0)
        rows, F = SC.att_rf(total)
        assert abs(rows * 2 * F - total) <= 3 and (rows * 2 * F > SC.STREAM_TRIP) == (total > SC.STREAM_TRIP)
        R, R_pad, Cc, ld_src, ld_dst = SC.pad_shape(total)
        assert R_pad * ld_dst == total and R <= R_pad and Cc <= ld_src and Cc <= ld_dst
    assert total % 256 != 0
    assert max(SC.NORM_SIZES) > SC.NORM_TRIP and 4100 * 257 > SC.STREAM_TRIP
    R, C = SC.CONVERT_SHAPES[-1]
    assert -(-R // 64) * 64 * (-(-C // 8) * 8 // 4) > 8192 * 256 and R * (-(-C // 64) * 64 // 8) > 4096 * 256
