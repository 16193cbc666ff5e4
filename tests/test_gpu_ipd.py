"""Inter-channel phase features on the MI355X: sk_stft_ipd against the existing STFT kernel, against sk_ipd_rows, against the
numpy restatement (sepkern/ipd.py) and the CPU oracle (oracle/stft.py); and an IPD model through the arch end to end against
an fp64 reference built from oracle.upit.blstm_padded and pit_mse.

One ragged batch of eight-microphone utterances, longest first: frame counts 165, 81, 80, 17, 16, 3 -- several workgroups (a
workgroup walks 5 tiles of 16 frames = 80), a workgroup plus one frame, exactly a workgroup, a tile plus one, exactly a tile,
and an utterance below one tile.  P = 1, 2 and 7 listed channels, int16 and float32 samples.  Run with -s for the figures."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

import _ipd_cases as cases
from _ipd_cases import CHANNELS, F, FRAMES, LENGTHS, PS
from conftest import PKG
from oracle import upit as OU

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(PKG, "archs"))

CASES = [(P, dt) for P in PS for dt in ("int16", "float32")]
REF = 0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def arch(dev):
    import uPIT
    return uPIT


def _flat(sigs, chans, dtype, dev):
    """Key-major flat tensor (every utterance's channel chans[0], then chans[1], ...) and the offset lists."""
    lens = [m.shape[1] for m in sigs]
    flat = np.concatenate([m[c] for c in chans for m in sigs])
    starts, total = np.concatenate([[0], np.cumsum(lens)[:-1]]), sum(lens)
    t = torch.from_numpy(flat.astype(np.float32) / np.float32(32768.0) if dtype == "float32" else flat).to(dev)
    return t, [[int(q * total + st) for st in starts] for q in range(len(chans))], lens


def _run(sigs, listed, dtype, dev, packed=True, ref=REF, **kw):
    from sepkern import ops
    from sepkern.packing import Packing
    flat, offs, lens = _flat(sigs, [ref] + list(listed), dtype, dev)
    pk = Packing([1 + n // 128 for n in lens], dev) if packed else None
    rows, mix = ops.stft_ipd(flat, offs, lens, pk=pk, **kw)
    return rows, mix, pk


@functools.lru_cache(maxsize=None)
def _batch(P, dtype):
    return _run(cases.case()["sigs"], CHANNELS[P], dtype, torch.device("cuda", 0))


def _utt(rows, pk, j):
    """Rows of utterance j of a packed (Rp, .) tensor -> (T_j, .)."""
    T = int(pk.lens_host[j])
    return rows[torch.from_numpy(pk.offs_host[:T].astype(np.int64) + j).to(rows.device)]


@functools.lru_cache(maxsize=None)
def _sk_stft():
    """The existing kernel's complex spectra of every microphone: [utterance] (8, T, 257) complex64 on the device."""
    from sepkern import ops
    sigs = cases.case()["sigs"]
    out = ops.stft_batch([torch.from_numpy(np.ascontiguousarray(x)).cuda() for m in sigs for x in m], want_complex=True, layout="TF")
    return [torch.stack(out[u * cases.NCHAN:(u + 1) * cases.NCHAN]) for u in range(len(sigs))]


def _blocks(rows, P):
    """(rows, ld) -> [(cos, sin) per listed channel], views."""
    from sepkern import ipd
    return [(rows[:, c0:c1], rows[:, s0:s1]) for (c0, c1), (s0, s1) in (ipd.columns(p) for p in range(P))]


# ------------------------------------------------------------------------------------------------ 1: the magnitude columns
@pytest.mark.parametrize("P,dtype", CASES)
def test_magnitude_columns_and_mix_rows_are_features_from_pcms_rows(dev, P, dtype):
    from sepkern import ipd
    from sepkern.data import features_from_pcm
    flat, _, lens = _flat(cases.case()["sigs"], [REF], dtype, dev)
    ref_mix, none, ref_pk = features_from_pcm({"flat": flat, "keys": ["mix"], "lens": lens}, dev)
    rows, mix, pk = _batch(P, dtype)
    assert none == [] and pk.R == ref_pk.R == sum(FRAMES) and pk.Rp > pk.R
    assert rows.shape == (pk.Rp, ipd.padded_dim(P)) and mix.shape == ref_mix.shape == (pk.Rp, F) and mix.is_contiguous()
    assert torch.equal(mix, ref_mix) and torch.equal(rows[:, :F], ref_mix)
    assert not rows[pk.R:].any() and not rows[:, ipd.in_dim(P):].any() and bool(torch.isfinite(rows).all())
    for c, s in _blocks(rows[:pk.R], P):       # unit modulus wherever the kernel did not declare silence
        m2 = c * c + s * s
        assert float((m2 - 1.0).abs().max()) < 1e-5 and bool((c < 0).any()) and bool((s < 0).any())


# ------------------------------------------------------------------------------------------------ 2: the same bits as sk_ipd_rows
@pytest.mark.parametrize("P,dtype", CASES)
def test_rows_are_sk_ipd_rows_on_the_existing_kernels_spectra(dev, P, dtype):
    """Whole rows, bit for bit: the magnitude columns (copied from what the caller holds), cos and sin of every listed channel,
    and the zero columns up to the next multiple of 16."""
    from sepkern import ops
    rows, mix, pk = _batch(P, dtype)
    for j, Y in enumerate(_sk_stft()):
        mag = ops.stft_batch([torch.from_numpy(cases.case()["sigs"][j][REF].copy()).to(dev)], want_complex=False)[0]
        got = ops.ipd_rows(Y, REF, CHANNELS[P], mag)
        assert got.shape == (FRAMES[j], rows.shape[1])
        assert torch.equal(got.view(torch.int32), _utt(rows, pk, j).view(torch.int32)), j
    # a strided view of the spectra and a wider magnitude buffer give the same rows
    Y = _sk_stft()[3]
    wide = torch.zeros(Y.shape[0], Y.shape[1], F + 5, dtype=torch.complex64, device=dev)
    wide[:, :, :F] = Y
    magw = torch.full((Y.shape[1], F + 3), 9.0, device=dev)
    magw[:, :F] = _utt(mix, pk, 3)
    assert torch.equal(ops.ipd_rows(wide[:, :, :F], REF, CHANNELS[P], magw[:, :F]), _utt(rows, pk, 3))


# ------------------------------------------------------------------------------------------------ 3: the formula in fp64
@pytest.mark.parametrize("P,dtype", CASES)
def test_features_are_the_formula_on_the_existing_kernels_spectra(dev, P, dtype):
    """|feature - r| <= 20 x 2^-24 (|a| + |b|) / (|Y_c| |Y_r|) + 2^-140, r = sepkern/ipd.py's fp64 formula on
    sk_stft(want_complex=True)'s spectra, a and b the two products of the numerator.  The roundings of ipd_feature: one
    product and one fused multiply-add in the numerator (2 half-ulps), two squared magnitudes of two roundings each, halved by
    the root (1 + 1), two reciprocal square roots at one ulp (2 + 2), two products (2): ten half-ulps, doubled."""
    from sepkern import ipd
    rows, _, pk = _batch(P, dtype)
    worst = 0.0
    for j, Yd in enumerate(_sk_stft()):
        Y = Yd.cpu().numpy().astype(np.complex128)
        got = _utt(rows, pk, j).cpu().numpy().astype(np.float64)
        yr = Y[REF]
        for p, ch in enumerate(CHANNELS[P]):
            yc = Y[ch]
            den = np.abs(yc) * np.abs(yr)
            assert den.min() > 0.0
            rc, rs = ipd.ipd(yc, yr)
            (c0, c1), (s0, s1) = ipd.columns(p)
            bc = 20.0 * 2.0 ** -24 * (np.abs(yc.real * yr.real) + np.abs(yc.imag * yr.imag)) / den + 2.0 ** -140
            bs = 20.0 * 2.0 ** -24 * (np.abs(yc.imag * yr.real) + np.abs(yc.real * yr.imag)) / den + 2.0 ** -140
            worst = max(worst, float((np.abs(got[:, c0:c1] - rc) / bc).max()), float((np.abs(got[:, s0:s1] - rs) / bs).max()))
    print("P=%d %s: worst |feature - formula on sk_stft's spectra| / bound = %.3f (gate 1)" % (P, dtype, worst))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ 4: end to end against the oracle
@functools.lru_cache(maxsize=None)
def _oracle_yardstick():
    """e: the largest absolute error of sk_stft's complex output against oracle/stft.py over every microphone of this batch."""
    return max(float(np.abs(Y.cpu().numpy().astype(np.complex128) - sp).max()) for Y, sp in zip(_sk_stft(), cases.case()["spec"]))


@pytest.mark.parametrize("P,dtype", CASES)
def test_features_against_the_oracle_stft(dev, P, dtype):
    """Reference: sepkern/ipd.py on oracle.stft.stft of the same samples.  Tolerance per element 4 e (1/|Y_c| + 1/|Y_r|), e the
    existing sk_stft's own worst error against that oracle on these signals (test_gpu_psa.py's yardstick: a relative error e / |Y|
    of either spectrum turns the unit phasor by as much; factor 4 as there).  It exceeds 0.1 on fewer than 1 % of the elements."""
    from sepkern import ipd
    e = _oracle_yardstick()
    share = cases.tolerance_share(e)
    assert share < cases.MAX_SHARE, share
    rows, _, pk = _batch(P, dtype)
    worst_abs = worst_rel = 0.0
    for j, sp in enumerate(cases.case()["spec"]):
        got = _utt(rows, pk, j).cpu().numpy().astype(np.float64)
        for p, ch in enumerate(CHANNELS[P]):
            rc, rs = ipd.ipd(sp[ch], sp[REF])
            tol = 4.0 * e * (1.0 / np.abs(sp[ch]) + 1.0 / np.abs(sp[REF]))
            (c0, c1), (s0, s1) = ipd.columns(p)
            for g, r in ((got[:, c0:c1], rc), (got[:, s0:s1], rs)):
                err = np.abs(g - r)
                worst_abs, worst_rel = max(worst_abs, float(err.max())), max(worst_rel, float((err / tol).max()))
    print("P=%d %s: sk_stft vs oracle e %.3g; tolerance > 0.1 on %.3g of the elements; worst feature error %.3g, %.3f of its "
          "tolerance (gate 1)" % (P, dtype, e, share, worst_abs, worst_rel))
    assert worst_rel <= 1.0


# ------------------------------------------------------------------------------------------------ 5: determinism, permutations
@pytest.mark.parametrize("P", PS)
def test_bits_do_not_depend_on_the_batch_the_sample_format_or_the_run(dev, P):
    sigs = cases.case()["sigs"]
    rows, mix, pk = _batch(P, "int16")
    for other in (_batch(P, "float32"), _run(sigs, CHANNELS[P], "int16", dev)):
        assert torch.equal(other[0].view(torch.int32), rows.view(torch.int32)) and torch.equal(other[1], mix)
    for j in range(len(sigs)):
        r1, m1, pk1 = _run([sigs[j]], CHANNELS[P], "int16", dev)
        assert torch.equal(r1[:pk1.R].view(torch.int32), _utt(rows, pk, j).view(torch.int32)), j
        assert torch.equal(m1[:pk1.R], _utt(mix, pk, j))


def test_permuting_the_channels_permutes_the_column_blocks(dev):
    sigs = cases.case()["sigs"]
    rows, _, pk = _batch(7, "int16")
    order = (6, 2, 7, 1)
    got, _, _ = _run(sigs, order, "int16", dev)
    assert torch.equal(got[:, :F], rows[:, :F])
    full = _blocks(rows, 7)
    for (c, s), ch in zip(_blocks(got, 4), order):
        rc, rs = full[CHANNELS[7].index(ch)]
        assert torch.equal(c.view(torch.int32), rc.view(torch.int32)) and torch.equal(s.view(torch.int32), rs.view(torch.int32))
    # another reference channel: cos is symmetric, sin antisymmetric -- up to the last bit, the products being formed the other way round
    swapped, _, _ = _run(sigs, (0,), "int16", dev, ref=3)
    (c, s), (c0, s0) = _blocks(swapped, 1)[0], full[CHANNELS[7].index(3)]
    assert float((c - c0)[:pk.R].abs().max()) < 1e-5 and float((s + s0)[:pk.R].abs().max()) < 1e-5


# ------------------------------------------------------------------------------------------------ 6: what is written, and where
@pytest.mark.parametrize("P,dtype", CASES)
def test_only_the_promised_elements_are_written(dev, P, dtype):
    from sepkern import ipd
    sigs = cases.case()["sigs"]
    rows, mix, pk = _batch(P, dtype)
    width, wp = ipd.in_dim(P), ipd.padded_dim(P)
    nan = float("nan")
    for ld in (wp + 9, width + min(5, wp - width)):          # beyond the padded width; and (P < 7) short of it
        pool = torch.full((pk.Rp + 3, ld), nan, device=dev)
        mpool = torch.full((pk.Rp + 3, F), nan, device=dev)
        ws = torch.empty(pk.R * F * 2, device=dev)
        ws.view(torch.int32).fill_(-1)                      # 0xFF bytes: NaN wherever it were read before it is written
        _run(sigs, CHANNELS[P], dtype, dev, out=(pool, mpool), ws=ws)
        zend = min(ld, wp)
        assert torch.equal(pool[:pk.R, :width].view(torch.int32), rows[:pk.R, :width].view(torch.int32))
        assert not pool[:pk.R, width:zend].any() and bool(torch.isnan(pool[:pk.R, zend:]).all())
        assert bool(torch.isnan(pool[pk.R:]).all())
        assert torch.equal(mpool[:pk.R], mix[:pk.R]) and bool(torch.isnan(mpool[pk.R:]).all())
    # per-utterance blocks hold the packed rows; rows of frames that do not exist stay as they were
    total = sum(FRAMES)
    pool, mpool = torch.full((total + 2, wp + 9), nan, device=dev), torch.full((total + 2, F), nan, device=dev)
    _, _, none = _run(sigs, CHANNELS[P], dtype, dev, packed=False, out=(pool, mpool))
    assert none is None
    at = 0
    for j, T in enumerate(FRAMES):
        assert torch.equal(pool[at:at + T, :wp].view(torch.int32), _utt(rows, pk, j).view(torch.int32))
        assert torch.equal(mpool[at:at + T], _utt(mix, pk, j))
        at += T
    assert bool(torch.isnan(pool[total:]).all()) and bool(torch.isnan(pool[:, wp:]).all()) and bool(torch.isnan(mpool[total:]).all())
    blocks, bmix, _ = _run(sigs, CHANNELS[P], dtype, dev, packed=False, want_mix=False)
    assert bmix is None and blocks.shape == (total, wp) and torch.equal(blocks.view(torch.int32), pool[:total, :wp].view(torch.int32))


# ------------------------------------------------------------------------------------------------ 7: silence
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_silence_gives_zero_features(dev, dtype):
    from sepkern import ops
    sigs = [m.copy() for m in cases.case()["sigs"][1:4]]
    sigs[0][2] = 0                              # a dead microphone
    sigs[1][0, 2048:2048 + 1536] = 0            # digital silence in the reference: frames 18 .. 26 see nothing but zeros
    sigs[2][5, :1024] = 0                       # ... and at the start of a listed channel, through the reflect padding: frames 0 .. 6
    rows, mix, pk = _run(sigs, CHANNELS[7], dtype, dev)
    assert bool(torch.isfinite(rows).all())
    blocks = [_blocks(_utt(rows, pk, j), 7) for j in range(3)]
    dead = CHANNELS[7].index(2)
    assert not blocks[0][dead][0].any() and not blocks[0][dead][1].any()
    assert all(float((c * c + s * s - 1.0).abs().max()) < 1e-5 for p, (c, s) in enumerate(blocks[0]) if p != dead)
    quiet = slice(18, 27)
    assert not _utt(mix, pk, 1)[quiet].any() and not _utt(rows, pk, 1)[quiet].any()
    assert bool(_utt(mix, pk, 1)[17].all()) and bool(_utt(mix, pk, 1)[27].all())
    late = CHANNELS[7].index(5)
    assert not blocks[2][late][0][:7].any() and not blocks[2][late][1][:7].any() and bool(blocks[2][late][0][7].any())
    assert bool(_utt(rows, pk, 2)[:7, :F].all())
    # the streaming kernel agrees on the same spectra
    Y = torch.stack(ops.stft_batch([torch.from_numpy(x.copy()).to(dev) for x in sigs[1]], want_complex=True, layout="TF"))
    got = ops.ipd_rows(Y, REF, CHANNELS[7], _utt(mix, pk, 1).contiguous())
    assert torch.equal(got.view(torch.int32), _utt(rows, pk, 1).view(torch.int32))


# ------------------------------------------------------------------------------------------------ 8: argument errors
def test_argument_errors_of_the_fused_kernel(dev):
    from sepkern import _lib, ipd
    from sepkern.packing import Packing
    sigs = cases.case()["sigs"][3:]
    flat, offs, lens = _flat(sigs, [0, 1, 2], "int16", dev)
    pk = Packing([1 + n // 128 for n in lens], dev)
    d64 = torch.tensor([o for row in offs for o in row] + [0, 17, 33], dtype=torch.int64, device=dev)
    d_ns = torch.tensor(lens, dtype=torch.int32, device=dev)
    rows = torch.full((pk.Rp, ipd.padded_dim(2)), 7.0, device=dev)
    ws = torch.empty(pk.R * F * 2, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731

    def call(B=3, C=3, n_fft=512, hop=128, offs_p=p(pk.offs), base_p=None, ld=rows.shape[1], min_samples=min(lens)):
        _lib.call("sk_stft_ipd", p(flat), 1, p(d64), p(d_ns), B, C, n_fft, hop, offs_p, base_p, p(rows), ld, None, p(ws), min_samples,
                  max(FRAMES[3:]), None)

    for kw, text in ((dict(C=1), r"C = 1 signals per utterance outside 2\.\.8"), (dict(C=9), r"C = 9 signals per utterance outside 2\.\.8"),
                     (dict(ld=1284), r"ld = 1284.*fewer than 257 \(1 \+ 2P\) = 1285"), (dict(n_fft=256, hop=64), r"only n_fft=512, hop=128"),
                     (dict(min_samples=256), r"256 samples.*reflect"), (dict(B=65536), r"B = 65536, at most 65535"),
                     (dict(base_p=p(d64[9:])), "one of them"), (dict(offs_p=None), "one of them")):
        with pytest.raises(_lib.SepkernError, match=r"code -1.*" + text):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((rows == 7.0).all())
    call()                                           # the same arguments, none of them off: it runs
    torch.cuda.synchronize()
    assert bool((rows[:pk.R, :ipd.in_dim(2)] != 7.0).any())


def test_argument_errors_of_the_streaming_kernel(dev):
    from sepkern import _lib, ops
    Y = _sk_stft()[4][:4].contiguous()               # (4, 16, 257)
    mag = Y[0].abs()
    out = torch.full((16, 784), 7.0, device=dev)
    for kw, text in ((dict(ref=4), r"ref = 4 outside \[0, 4\)"), (dict(ref=-1), r"ref = -1 outside"), (dict(channels=[4]), r"channel 4 outside \[0, 4\)"),
                     (dict(channels=[-1]), r"channel -1 outside"), (dict(channels=[0]), "channel 0 is the reference"),
                     (dict(channels=[1, 1], out=torch.full((16, 1296), 7.0, device=dev)), "channel 1 is repeated"),
                     (dict(channels=[]), "P = 0 listed channels"), (dict(out=torch.full((16, 770), 7.0, device=dev)), r"ld = 770.*= 771")):
        args = dict(dict(ref=0, channels=[1], out=out), **kw)
        with pytest.raises(_lib.SepkernError, match=r"code -1.*" + text):
            ops.ipd_rows(Y, args["ref"], args["channels"], mag, out=args["out"])
        torch.cuda.synchronize()
        assert bool((args["out"] == 7.0).all())
    with pytest.raises(_lib.SepkernError, match=r"C = 1 channels outside 2\.\.8"):
        ops.ipd_rows(Y[:1], 0, [1], mag, out=out)
    with pytest.raises(_lib.SepkernError, match="mag must be"):
        ops.ipd_rows(Y, 0, [1], mag[:, :256], out=out)


# ------------------------------------------------------------------------------------------------ 9: through the arch
ARCH_CHANS = (1, 2)
ARCH_LENGTHS = LENGTHS[2:]            # the four shortest: 80, 17, 16, 3 frames
ARCH_FRAMES = FRAMES[2:]


def _items(with_channels=True, chans=ARCH_CHANS):
    c = cases.case()
    items = []
    for m, srcs in zip(c["sigs"][2:], c["srcs"][2:]):
        d = {"mix": m[REF].copy(), "source1": srcs[0], "source2": srcs[1]}
        if with_channels:
            d.update(("chan%d" % ch, m[ch].copy()) for ch in chans)
        items.append(d)
    return items


def _model(arch, kind="mse", ipd=True, seed=8, H=64, L=2, chans=ARCH_CHANS):
    torch.manual_seed(seed)
    conf = dict(num_spk="2", hidden_dim=str(H), num_layers=str(L), loss=kind)
    if ipd:
        conf.update(ipd_channels=",".join(str(c) for c in chans), ipd_ref=str(REF))
    model = arch.SepDNN(0, **conf)
    model.cuda()
    model.train()
    return model


def _step(arch, model, batch, h0, c0):
    model.next_hidden = (h0.cuda(), c0.cuda())
    loss, norm = arch.compute_loss(model, 0, batch)
    loss.backward()
    return loss.detach().clone(), norm.clone(), {k: p.grad.clone() for k, p in model.named_parameters()}


def _fp64_reference(model, wide, mix, sources, pk, h0, c0, S=2):
    """Loss, permutations and parameter gradients in fp64 from the kernel's own feature rows: oracle.upit.blstm_padded, then
    BatchNorm1d over the zero-padded (B, 2H, T) grid in training mode, Linear, sigmoid (archs/uPIT.py:135-144 of the reference)
    and oracle.upit.pit_mse."""
    params = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.named_parameters()}
    weights = [[tuple(params["blstm.%s_l%d%s" % (n, l, sfx)] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
                for sfx in ("", "_reverse")] for l in range(model.num_layers)]
    lens = torch.tensor(ARCH_FRAMES)
    pad = lambda rows, C: pk.unpack(rows[:, :C].contiguous()).cpu().double()        # noqa: E731  (T, B, C), zeros behind an utterance's end
    y, _, _ = OU.blstm_padded(pad(wide, model.in_dim), lens, weights, h0.double(), c0.double())
    flat = y.reshape(-1, y.shape[2])                      # every (t, b) position of the padded grid enters the statistics
    mean, var = flat.mean(0), flat.var(0, unbiased=False)
    xbn = (y - mean) / torch.sqrt(var + 1e-5) * params["bn.weight"] + params["bn.bias"]
    bf = lambda x: x.permute(1, 0, 2).contiguous()                                  # noqa: E731  batch-first, as pit_mse views it
    mask = bf(torch.sigmoid(xbn @ params["lin.weight"].t() + params["lin.bias"]))
    lo, no, losses, idx = OU.pit_mse(mask, bf(pad(mix, F)), [bf(pad(s, F)) for s in sources], lens, S, F)
    lo.backward()
    return lo.detach(), no, losses.detach(), idx, {k: v.grad for k, v in params.items()}


@pytest.mark.parametrize("chans", [ARCH_CHANS, (1,)])
def test_arch_loss_matches_an_fp64_reference_on_the_kernels_rows(arch, dev, chans):
    """ipd_channels=1,2 is in_dim 257 (1 + 2 x 2) = 1285; ipd_channels=1 is the in_dim 771 of the measurements (tools/ipd_bench.py)."""
    from sepkern import ipd
    from sepkern.data import Prefetcher, features_from_pcm, ipd_rows_from_pcm
    S, H, L, B = 2, 64, 2, len(ARCH_LENGTHS)
    model = _model(arch, chans=chans)
    keys = ["chan%d" % c for c in chans]
    assert model.in_dim == ipd.in_dim(len(chans)) == {2: 1285, 1: 771}[len(chans)] and model.out_dim == 514
    batch = arch.WavCollator()(_items(chans=chans))
    assert batch["pcm"]["lens"] == ARCH_LENGTHS and batch["pcm"]["keys"] == ["mix", "source1", "source2"] + keys
    h0, c0 = torch.randn(2 * L, B, H), torch.randn(2 * L, B, H)
    (mix, sources, pk), wide = ipd_rows_from_pcm(batch["pcm"], dev, features_from_pcm)
    assert wide.shape == (pk.Rp, ipd.padded_dim(len(chans))) and torch.equal(wide[:, :F], mix)
    lo, no, losses, idx, og = _fp64_reference(model, wide, mix, sources, pk, h0, c0)
    two = torch.sort(losses, 0).values
    assert float((two[1] / two[0]).min()) > 1.0 + 1e-4          # no permutation is tied within ten times the loss gate

    loss, norm, grads = _step(arch, model, batch, h0, c0)
    lv, lo_v = float(loss), float(lo)
    print("IPD arch, loss=mse: loss %.8g (fp64 reference %.8g), norm %d" % (lv, lo_v, int(norm)))
    assert float(norm) == float(no) == sum(ARCH_FRAMES) * F
    assert model.last_best_perm.cpu().tolist() == idx.tolist()
    assert abs(lv - lo_v) <= 1e-5 * abs(lo_v)
    worst = 0.0
    assert set(grads) == set(og)
    for k, g in grads.items():
        err = float((g.cpu().double() - og[k]).norm() / (og[k].norm() + 1e-30))
        worst = max(worst, err)
        assert err < 2e-4, (k, err)
    print("IPD arch, loss=mse: worst parameter-gradient relative L2 %.3g (gate 2e-4)" % worst)
    assert float(grads["blstm.weight_ih_l0"][:, F:].abs().max()) > 0.0      # the phase columns reach the weights

    # the same batch staged by the prefetcher: the wide rows travel with it
    staged = list(Prefetcher([batch], dev))
    assert len(staged) == 1 and "pcm" not in staged[0] and staged[0]["ipd_keys"] == keys
    assert torch.equal(staged[0]["ipd"], wide) and torch.equal(staged[0]["packed"][0], mix)
    got = _step(arch, model, staged[0], h0, c0)
    assert torch.equal(got[0], loss) and torch.equal(got[1], norm) and all(torch.equal(g, grads[k]) for k, g in got[2].items())

    # a mono batch to this model, an array batch to a mono model, the channels in another order: refused
    if len(chans) < 2:
        return
    mono_batch = arch.WavCollator()(_items(False))
    with pytest.raises(ValueError, match="the batch holds one channel"):
        arch.compute_loss(model, 0, mono_batch)
    with pytest.raises(ValueError, match="the batch holds one channel"):
        arch.compute_loss(model, 0, list(Prefetcher([mono_batch], dev))[0])
    with pytest.raises(ValueError, match="the model sees one channel"):
        arch.compute_loss(_model(arch, ipd=False), 0, batch)
    with pytest.raises(ValueError, match="the model sees one channel"):
        arch.compute_loss(_model(arch, ipd=False), 0, staged[0])
    with pytest.raises(ValueError, match="in that order"):
        arch.compute_loss(model, 0, dict(staged[0], ipd_keys=["chan2", "chan1"]))
    # evaluation mode / no_grad (the CV pass) goes the same way
    model.eval()
    with torch.no_grad():
        model.next_hidden = (h0.cuda(), c0.cuda())
        cv, cvn = arch.compute_cv_loss(model, 0, batch)
    assert np.isfinite(float(cv)) and float(cvn) == float(norm)


def test_the_front_ends_give_the_mono_batchs_targets_for_the_array_batch(arch, dev):
    from sepkern.data import Prefetcher, features_from_pcm, psa_features_from_pcm, wave_features_from_pcm
    arr, mono = arch.WavCollator()(_items())["pcm"], arch.WavCollator()(_items(False))["pcm"]
    B = len(ARCH_LENGTHS)
    h0, c0 = torch.randn(4, B, 64), torch.randn(4, B, 64)
    for front, kw in ((features_from_pcm, {}), (psa_features_from_pcm, dict(clamp=False)), (psa_features_from_pcm, dict(clamp=True)),
                      (wave_features_from_pcm, {}), (wave_features_from_pcm, dict(source_mags=False))):
        a, m = front(arr, dev, **kw), front(mono, dev, **kw)
        assert torch.equal(a[0], m[0]) and len(a[1]) == len(m[1]) and all(torch.equal(x, y) for x, y in zip(a[1], m[1]))
        assert a[2].lens_host.tolist() == m[2].lens_host.tolist()
        if front is wave_features_from_pcm:
            assert torch.equal(torch.view_as_real(a[3]["mixc"]), torch.view_as_real(m[3]["mixc"])) and a[3]["nsamp"] == m[3]["nsamp"]
            assert {k: a[3]["sig_offs"][k] for k in m[3]["sig_offs"]} == m[3]["sig_offs"]
    # every supported loss takes the array batch, raw and staged, to the same bits
    for kind in ("psa", "tpsa", "dpcl", "sisdr"):
        model = _model(arch, kind)
        batch = {"pcm": arr}
        loss, norm, grads = _step(arch, model, batch, h0, c0)
        assert np.isfinite(float(loss)) and all(bool(torch.isfinite(g).all()) for g in grads.values()), kind
        assert float(grads["blstm.weight_ih_l0"][:, F:].abs().max()) > 0.0, kind
        staged = list(Prefetcher([batch], dev, keep_wave=kind == "sisdr", targets=kind if kind in ("psa", "tpsa") else None))[0]
        got = _step(arch, model, staged, h0, c0)
        assert torch.equal(got[0], loss) and all(torch.equal(g, grads[k]) for k, g in got[2].items()), kind


def test_a_mono_model_never_reaches_the_new_entry_points(arch, dev, monkeypatch):
    from sepkern import _lib
    calls = []
    real = _lib.call

    def spy(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    mono, arr = arch.WavCollator()(_items(False)), arch.WavCollator()(_items())
    h0, c0 = torch.randn(4, len(ARCH_LENGTHS), 64), torch.randn(4, len(ARCH_LENGTHS), 64)
    for kind in ("mse", "psa", "sisdr", "dpcl"):
        del calls[:]
        _step(arch, _model(arch, kind, ipd=False), mono, h0, c0)
        assert "sk_stft_ipd" not in calls and "sk_ipd_rows" not in calls and "sk_lstm_fwd" in calls, kind
    del calls[:]
    _step(arch, _model(arch, "mse"), arr, h0, c0)
    assert calls.count("sk_stft_ipd") == 1 and "sk_ipd_rows" not in calls


# ------------------------------------------------------------------------------------------------ 10: it descends
def test_twenty_steps_descend(arch, dev):
    """Twenty fused clip + Adam steps of an IPD model (loss=mse) on one fixed batch with fixed (h0, c0): the mean of the last five
    losses is below the mean of the first five (-s prints the curve)."""
    from sepkern.optim import ClipAdam
    batch = arch.WavCollator()(_items())
    model = _model(arch, "mse", seed=11)
    opt = ClipAdam(model, lr=1e-3, max_norm=0.25)
    B = len(ARCH_LENGTHS)
    h0, c0 = torch.randn(4, B, 64, device=dev), torch.randn(4, B, 64, device=dev)
    curve = []
    for _ in range(20):
        model.next_hidden = (h0, c0)
        loss, _ = arch.compute_loss(model, 0, batch)
        loss.backward()
        opt.step()
        curve.append(float(loss.detach()))
    print("twenty steps, IPD model, loss=mse: " + " ".join("%.6f" % v for v in curve))
    assert all(np.isfinite(curve)) and int(opt.scal[3]) == 0
    assert np.mean(curve[-5:]) < np.mean(curve[:5])
