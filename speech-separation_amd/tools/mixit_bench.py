#!/usr/bin/env python3
"""Timings of the mixture-invariant loss (profiles/mixit_loss.txt): everything in one process on one device, HIP events around
synchronised work, warmed up, variants alternating.

  kernels   sk_mask_istft_rows / sk_mixit_fwd / sk_mixit_mask_grad stand-alone at 32 utterances of U(24 k, 64 k) samples,
            M = 2 and 4: time, algorithmic bytes, share of the 8 TB/s HBM peak
  loss      loss forward + backward (mask in -> dmask out) against the same loss composed from PyTorch-ROCm's own ops
            (irfft, fold, fp64 Gram sums, the 2^M assignments as one einsum, autograd) on the same inputs
  step      the whole 3 x 896, 32-utterance ragged training step with loss=mixit (M = 4 masks, 2 references) beside the same
            step with loss=sisdr (S = 4 masks, 4 references)

    python tools/mixit_bench.py [--reps 50] [--steps 10] [--skip-step]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
for p in (PKG, os.path.join(PKG, "archs"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from sepkern import mixit, ops  # noqa: E402
from sepkern.data import wave_features_from_pcm  # noqa: E402
from sisdr_bench import F, HBM_PEAK, TorchLoss, pcm_of, timed  # noqa: E402

TAU = mixit.tau_of()


def loss_inputs(M, dev, batch=32):
    """Mixtures of two recordings (the references) and M random masks."""
    pcm = pcm_of(batch, 2)["pcm"]
    mix, _, pk, wave = wave_features_from_pcm(pcm, dev, source_mags=False)
    torch.manual_seed(M)
    mask = torch.rand(pk.Rp, M * F, device=dev) * 0.96 + 0.02
    return pk, wave, mask, ops.mixit_descriptors(pk, wave["sig_offs"], M)


def hip_loss(pk, wave, mask, desc, M, gscale, repeat=1):
    est, est_offs, _ = ops.mask_istft_rows(wave["mixc"], mask, pk, M, est_offs=desc["est_offs"], repeat=repeat)
    res = ops.mixit_fwd(est, est_offs, wave["flat"], desc["ref_offs"], desc["nsamp"], M, 128 * (pk.T - 1), TAU, repeat=repeat)
    dm = ops.mixit_mask_grad(est, est_offs, wave["flat"], desc["ref_offs"], res["best_code"], res["coef"], gscale, wave["mixc"], pk, M,
                             repeat=repeat)
    return res["out"], dm


def bench_kernels(dev, reps):
    out = {}
    for M in (2, 4):
        pk, wave, mask, desc = loss_inputs(M, dev)
        gscale = torch.ones(1, device=dev)
        hip_loss(pk, wave, mask, desc, M, gscale, repeat=2)
        torch.cuda.synchronize()
        ops.PROF = {}
        hip_loss(pk, wave, mask, desc, M, gscale, repeat=reps)
        torch.cuda.synchronize()
        prof, ops.PROF = ops.prof_summary(), None
        for cls, (_, ms, by) in prof.items():
            us = 1e3 * ms / reps
            out["M=%d %s" % (M, cls)] = {"us_per_launch": round(us, 2), "MB_algorithmic_per_launch": round(by / reps / 1e6, 2),
                                         "GBs_algorithmic": round(by / reps / us / 1e3, 1),
                                         "frac_of_hbm_peak": round(by / reps / (us * 1e-6) / HBM_PEAK, 3)}
        out["M=%d shape" % M] = {"utterances": pk.B, "frames": pk.R, "samples_per_estimate": int(128 * (pk.R - pk.B))}
    return out


class TorchMixit(TorchLoss):
    """sisdr_bench.TorchLoss's iSTFT (index_copy, complex product, irfft x window, fold, window-sum-square) followed by the
    mixture-invariant loss from the fp64 sums P, c, G: every assignment's two errors by one einsum, the thresholded scores,
    arg-max; autograd back."""

    def __init__(self, pk, wave, M, dev):
        super().__init__(pk, wave, 2, dev)              # two references
        self.S = M
        codes = torch.arange(1 << M, device=dev)
        bits = (codes[:, None] >> torch.arange(M, device=dev)[None, :]) & 1
        self.A = torch.stack([(bits == 0), (bits == 1)], dim=1).double()                     # (2^M, 2, M)

    def __call__(self, mask_rows, R):
        B, T, M = self.B, self.T, self.S
        padded = mask_rows.new_zeros(T * B, M * F).index_copy(0, self.idx, mask_rows[:R])
        m = padded.view(T, B, M, F).permute(1, 2, 0, 3)                                       # (B, M, T, F)
        frames = torch.fft.irfft(self.mix * m, n=512, dim=3) * self.win                       # (B, M, T, 512)
        cols = frames.reshape(B * M, T, 512).transpose(1, 2)
        y = torch.nn.functional.fold(cols, (1, self.n), (1, 512), stride=(1, 128)).view(B, M, self.n)
        e = (y[:, :, 256:self.n - 256] * self.inv[:, None, :] * self.keep[:, None, :]).double()
        x = self.refs
        P = (x * x).sum(-1)                                                                    # (B, 2)
        c = torch.einsum("bnt,bkt->bnk", x, e)
        G = torch.einsum("bkt,blt->bkl", e, e)
        err = P[:, None, :] - 2.0 * torch.einsum("ank,bnk->ban", self.A, c) + torch.einsum("ank,bkl,anl->ban", self.A, G, self.A)
        Pa = P[:, None, :]
        score = (10.0 * torch.log10((Pa + 1e-30) / (err.clamp_min(0.0) + TAU * Pa + 1e-30))).mean(-1)      # (B, 2^M)
        return -score.max(dim=1).values.mean()


def bench_loss(dev, reps):
    out = {}
    for M in (2, 4):
        pk, wave, mask, desc = loss_inputs(M, dev)
        gscale = torch.ones(1, device=dev)
        tl = TorchMixit(pk, wave, M, dev)
        mreq = mask.clone().requires_grad_(True)

        def run_hip():
            return hip_loss(pk, wave, mask, desc, M, gscale)

        def run_torch():
            mreq.grad = None
            loss = tl(mreq, pk.R)
            loss.backward()
            return loss

        lo_h, dm = run_hip()
        lo_t = run_torch()
        torch.cuda.synchronize()
        rel = float((dm[:pk.R] - mreq.grad[:pk.R]).norm() / mreq.grad[:pk.R].norm())
        ms_h, ms_t = [], []
        for _ in range(5):                      # alternating
            ms_h.append(timed(run_hip, reps))
            ms_t.append(timed(run_torch, max(1, reps // 5)))
        out["M=%d" % M] = {"hip_ms": round(float(np.median(ms_h)), 4), "torch_ms": round(float(np.median(ms_t)), 4),
                           "torch_over_hip": round(float(np.median(ms_t) / np.median(ms_h)), 2),
                           "loss_hip_dB": round(float(lo_h[0]), 5), "loss_torch_dB": round(float(lo_t), 5),
                           "dmask_rel_l2_hip_vs_torch": rel, "hip_ms_all": [round(v, 4) for v in ms_h],
                           "torch_ms_all": [round(v, 4) for v in ms_t]}
    return out


def bench_step(dev, steps, warmup=3):
    import uPIT
    from sepkern.optim import ClipAdam
    # the same 32 lengths for both (pcm_of draws them from the seed alone): two recordings for mixit, four sources for sisdr
    batches = {"mixit": pcm_of(32, 2, seed=1), "sisdr": pcm_of(32, 4, seed=1)}
    assert batches["mixit"]["pcm"]["lens"] == batches["sisdr"]["pcm"]["lens"]
    models = {}
    for kind in ("sisdr", "mixit"):
        torch.manual_seed(0)
        m = uPIT.SepDNN(0, hidden_dim="896", num_layers="3", num_spk="4", loss=kind)
        m.cuda()
        m.train()
        models[kind] = (m, ClipAdam(m, lr=1e-4, max_norm=0.25))

    def step(kind):
        m, opt = models[kind]
        loss, _ = uPIT.compute_loss(m, 0, batches[kind])
        loss.backward()
        opt.step()

    for kind in models:
        for _ in range(warmup):
            step(kind)
    ms = {"sisdr": [], "mixit": []}
    for _ in range(steps):                      # alternating
        for kind in ms:
            ms[kind].append(timed(lambda: step(kind), 1))
    out = {k: {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)} for k, v in ms.items()}
    out["mixit_minus_sisdr_ms"] = round(out["mixit"]["median_ms"] - out["sisdr"]["median_ms"], 3)
    out["frames"] = int(sum(1 + n // 128 for n in batches["mixit"]["pcm"]["lens"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"kernels": bench_kernels(dev, a.reps), "loss_fwd_bwd": bench_loss(dev, a.reps)}
    if not a.skip_step:
        res["training_step_3x896_b32_ragged_num_spk4"] = bench_step(dev, a.steps)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
