#!/usr/bin/env python3
"""Timings of the SI-SDR uPIT loss (profiles/sisdr_loss.txt): everything in one process on one device, HIP events around
synchronised work, warmed up, variants alternating.

  kernels   sk_mask_istft_rows / sk_sisdr_pit_fwd / sk_sisdr_mask_grad stand-alone at 32 utterances of U(24 k, 64 k) samples,
            S = 2 and 3: time, algorithmic bytes, share of the 8 TB/s HBM peak (as bench.py's aux block names STFT / iSTFT)
  loss      loss forward + backward (mask in -> dmask out) against the same loss composed from PyTorch-ROCm's own ops
            (irfft, fold, fp64 sums, autograd) on the same inputs
  step      the whole 3 x 896, 32-utterance ragged training step with loss=sisdr beside the same step with loss=mse

    python tools/sisdr_bench.py [--reps 50] [--steps 10] [--skip-step]
"""
import argparse
import itertools
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
for p in (PKG, os.path.join(PKG, "archs")):
    if p not in sys.path:
        sys.path.insert(0, p)

from sepkern import ops, synth  # noqa: E402
from sepkern.data import wave_features_from_pcm  # noqa: E402

HBM_PEAK = 8.0e12
F = 257


def pcm_of(batch, S, seed=0):
    """A WavCollator-shaped batch of `batch` synthetic utterances of U(24 k, 64 k) samples."""
    import uPIT
    rng = np.random.default_rng(seed)
    lengths = rng.integers(24000, 64001, batch)
    samples = []
    for sig in synth.pcm_batch(batch, num_spk=S, lengths=lengths):
        d = {"mix": sig[0]}
        for i in range(S):
            d["source%d" % (i + 1)] = sig[1 + i]
        samples.append(d)
    return uPIT.WavCollator()(samples)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def loss_inputs(S, dev, batch=32):
    pcm = pcm_of(batch, S)["pcm"]
    mix, _, pk, wave = wave_features_from_pcm(pcm, dev, source_mags=False)
    torch.manual_seed(S)
    mask = torch.rand(pk.Rp, S * F, device=dev) * 0.96 + 0.02
    return pk, wave, mask, ops.sisdr_descriptors(pk, wave["sig_offs"], S)


def hip_loss(pk, wave, mask, desc, S, gscale, repeat=1):
    est, est_offs, _ = ops.mask_istft_rows(wave["mixc"], mask, pk, S, est_offs=desc["est_offs"], repeat=repeat)
    res = ops.sisdr_pit_fwd(est, est_offs, wave["flat"], desc["ref_offs"], desc["nsamp"], S, 128 * (pk.T - 1), repeat=repeat)
    dm = ops.sisdr_mask_grad(est, est_offs, wave["flat"], desc["ref_offs"], res["best_perm"], res["coef"], gscale, wave["mixc"], pk, S,
                             repeat=repeat)
    return res["out"], dm


def bench_kernels(dev, reps):
    out = {}
    for S in (2, 3):
        pk, wave, mask, desc = loss_inputs(S, dev)
        gscale = torch.ones(1, device=dev)
        hip_loss(pk, wave, mask, desc, S, gscale, repeat=2)
        torch.cuda.synchronize()
        ops.PROF = {}
        hip_loss(pk, wave, mask, desc, S, gscale, repeat=reps)
        torch.cuda.synchronize()
        prof, ops.PROF = ops.prof_summary(), None
        for cls, (_, ms, by) in prof.items():
            us = 1e3 * ms / reps
            out["S=%d %s" % (S, cls)] = {"us_per_launch": round(us, 2), "MB_algorithmic_per_launch": round(by / reps / 1e6, 2),
                                         "GBs_algorithmic": round(by / reps / us / 1e3, 1),
                                         "frac_of_hbm_peak": round(by / reps / (us * 1e-6) / HBM_PEAK, 3)}
        out["S=%d shape" % S] = {"utterances": pk.B, "frames": pk.R, "samples_per_source": int(128 * (pk.R - pk.B))}
    return out


class TorchLoss:
    """The same loss from PyTorch-ROCm's own ops: packed mask rows -> padded grid (index_copy), complex product, irfft x window,
    fold (overlap-add), per-utterance window-sum-square, fp64 sums over the valid samples, SI-SDR, PIT arg-max; autograd back."""

    def __init__(self, pk, wave, S, dev):
        B, T = pk.B, pk.T
        self.B, self.T, self.S = B, T, S
        lens = torch.as_tensor(pk.lens_host.astype(np.int64))
        tt, jj = torch.meshgrid(torch.arange(T), torch.arange(B), indexing="ij")
        valid = tt < lens[None, :]
        self.idx = (tt * B + jj)[valid].to(dev)                     # packed row r -> padded row t B + j (time-major order)
        mixp = torch.zeros(T * B, F, dtype=torch.complex64, device=dev).index_copy(0, self.idx, wave["mixc"][:pk.R])
        self.mix = mixp.view(T, B, 1, F).permute(1, 2, 0, 3).contiguous()                    # (B, 1, T, F)
        self.win = torch.hann_window(512, periodic=True, device=dev)
        n = 512 + 128 * (T - 1)
        self.n = n
        frames_valid = valid.t().to(dev).float()                                              # (B, T)
        wsq = (self.win * self.win)[None, :, None] * frames_valid[:, None, :]                 # (B, 512, T)
        wss = torch.nn.functional.fold(wsq, (1, n), (1, 512), stride=(1, 128)).view(B, n)
        self.inv = torch.where(wss > 1e-30, 1.0 / wss.clamp_min(1e-30), torch.zeros_like(wss))[:, 256:n - 256]
        L = (lens - 1) * 128
        Lmax = int(L.max())
        self.keep = (torch.arange(Lmax)[None, :] < L[:, None]).to(dev)                        # (B, Lmax)
        self.nval = L.to(dev).double()
        flat = wave["flat"]
        refs = torch.zeros(B, S, Lmax, device=dev)
        for j in range(B):
            for i in range(S):
                o = wave["sig_offs"]["source%d" % (i + 1)][j]
                refs[j, i, :int(L[j])] = flat[o:o + int(L[j])].float() / 32768.0
        self.refs = refs.double()
        self.perms = torch.tensor(list(itertools.permutations(range(S))), device=dev)         # (P, S)

    def __call__(self, mask_rows, R):
        B, T, S = self.B, self.T, self.S
        padded = mask_rows.new_zeros(T * B, S * F).index_copy(0, self.idx, mask_rows[:R])
        m = padded.view(T, B, S, F).permute(1, 2, 0, 3)                                       # (B, S, T, F)
        frames = torch.fft.irfft(self.mix * m, n=512, dim=3) * self.win                       # (B, S, T, 512)
        cols = frames.reshape(B * S, T, 512).transpose(1, 2)
        y = torch.nn.functional.fold(cols, (1, self.n), (1, 512), stride=(1, 128)).view(B, S, self.n)
        e = (y[:, :, 256:self.n - 256] * self.inv[:, None, :] * self.keep[:, None, :]).double()
        r = self.refs
        nv = self.nval[:, None]
        se, sr = e.sum(-1), r.sum(-1)
        a = torch.einsum("bkn,bin->bki", e, r) - se[:, :, None] * sr[:, None, :] / nv[:, :, None]
        b = ((r * r).sum(-1) - sr * sr / nv)[:, None, :]
        c = ((e * e).sum(-1) - se * se / nv)[:, :, None]
        tt = a * a / b
        pair = 10.0 * torch.log10((tt + 1e-30) / (c - tt + 1e-30))                            # (B, S, S)
        score = pair[:, torch.arange(S, device=pair.device)[None, :], self.perms].mean(-1)    # (B, P)
        return -score.max(dim=1).values.mean()


def bench_loss(dev, reps):
    out = {}
    for S in (2, 3):
        pk, wave, mask, desc = loss_inputs(S, dev)
        gscale = torch.ones(1, device=dev)
        tl = TorchLoss(pk, wave, S, dev)
        mreq = mask.clone().requires_grad_(True)

        def run_hip():
            return hip_loss(pk, wave, mask, desc, S, gscale)

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
        out["S=%d" % S] = {"hip_ms": round(float(np.median(ms_h)), 4), "torch_ms": round(float(np.median(ms_t)), 4),
                           "torch_over_hip": round(float(np.median(ms_t) / np.median(ms_h)), 2),
                           "loss_hip_dB": round(float(lo_h[0]), 5), "loss_torch_dB": round(float(lo_t), 5),
                           "dmask_rel_l2_hip_vs_torch": rel, "hip_ms_all": [round(v, 4) for v in ms_h],
                           "torch_ms_all": [round(v, 4) for v in ms_t]}
    return out


def bench_step(dev, steps, warmup=3):
    import uPIT
    from sepkern.optim import ClipAdam
    batch = pcm_of(32, 2, seed=1)
    models = {}
    for kind in ("mse", "sisdr"):
        torch.manual_seed(0)
        m = uPIT.SepDNN(0, hidden_dim="896", num_layers="3", loss=kind)
        m.cuda()
        m.train()
        models[kind] = (m, ClipAdam(m, lr=1e-4, max_norm=0.25))

    def step(kind):
        m, opt = models[kind]
        loss, _ = uPIT.compute_loss(m, 0, batch)
        loss.backward()
        opt.step()

    for kind in models:
        for _ in range(warmup):
            step(kind)
    ms = {"mse": [], "sisdr": []}
    for _ in range(steps):                      # alternating
        for kind in ms:
            ms[kind].append(timed(lambda: step(kind), 1))
    out = {k: {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)} for k, v in ms.items()}
    out["sisdr_minus_mse_ms"] = round(out["sisdr"]["median_ms"] - out["mse"]["median_ms"], 3)
    out["frames"] = int(sum(1 + n // 128 for n in batch["pcm"]["lens"]))
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
        res["training_step_3x896_b32_ragged"] = bench_step(dev, a.steps)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
