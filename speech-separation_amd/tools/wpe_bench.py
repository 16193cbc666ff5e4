#!/usr/bin/env python3
"""Timings of WPE dereverberation (profiles/wpe.txt): everything in one process on one device, HIP events around synchronised
work, warmed up, variants alternating.

  kernel    sk_wpe at the one-hour shape (T = 225 000 frames, blocks of 600 frames, no context, 10 taps, a delay of 3,
            3 iterations, loading 1e-3; C = 7, the LibriCSS array, and C = 1; synthetic reverberant spectra): the whole call by
            HIP events against a COUNT of its fp64 operations -- per (t, f) and iteration 8 (D (D + 1) / 2 + D C) for the sums
            of R and P, 8 D C for the residual (iterations 2.., and once more for the output) -- at the 78.6 TFLOP/s fp64
            vector peak.  The count takes a multiply and an add as the two halves of a fused multiply-add; the kernel issues
            them separately (sepkern/wpe.py's arithmetic has one rounding per operation), so its own floor is twice the count's.
  torch     for comparison only: the same result composed from PyTorch-ROCm's own ops on the same tensors in the same call
            (complex128 matrix products and torch.linalg.solve per block); X compared

    python tools/wpe_bench.py [--reps 3] [--frames 225000]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
for p in (PKG, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from sepkern import ops, wpe as wp  # noqa: E402

FP64_PEAK = 78.6e12          # vector fp64, 256 CUs x 4 SIMDs x 16 lanes x 2 (FMA) x 2.4 GHz
F = 257
K, DELAY, ITERS, LB, LOADING = 10, 3, 3, 600, 1e-3


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def reverberant_inputs(C, T, dev, taps=8, decay=0.7):
    """tests/_wpe_cases.py's construction with torch's generator: Y (C, T, F) complex64."""
    g = torch.Generator(device=dev)
    g.manual_seed(10 * C + 1)
    gauss = lambda *sh: torch.complex(torch.randn(*sh, device=dev, generator=g), torch.randn(*sh, device=dev, generator=g)) * (0.5 ** 0.5)
    env = 0.2 + torch.sin(torch.arange(T, device=dev)[:, None] * (0.2 + 0.4 * torch.rand(1, F, device=dev, generator=g))).abs()
    S = gauss(T, F) * env
    Y = torch.zeros(C, T, F, dtype=torch.complex64, device=dev)
    for u in range(taps):
        h = gauss(C, 1, F) * decay ** u if u else torch.ones(C, 1, F, dtype=torch.complex64, device=dev)
        Y[:, u:] += h * S[None, :T - u]
    Y += 0.03 * float(Y.abs().pow(2).mean().sqrt()) * gauss(C, T, F)
    return Y


def torch_wpe(Y):
    """The definition with torch ops (T a multiple of the block length, no context, no pass-through cells).  -> X."""
    C, T, _ = Y.shape
    D, pad = C * K, DELAY + K - 1
    Yp = torch.cat([torch.zeros(C, pad, F, dtype=torch.complex128, device=Y.device), Y.to(torch.complex128)], 1)
    eye = torch.eye(D, dtype=torch.complex128, device=Y.device)
    X = torch.empty_like(Y)
    for j in range(T // LB):
        t0 = pad + j * LB
        y = Yp[:, t0:t0 + LB].permute(2, 0, 1)                                                # (F, C, Lb)
        yt = torch.cat([Yp[:, t0 - DELAY - k:t0 - DELAY - k + LB] for k in range(K)], 0).permute(2, 0, 1).contiguous()
        yh, yth = y.conj().transpose(1, 2), yt.conj().transpose(1, 2)
        x = y
        for _ in range(ITERS):
            lam = x.abs().pow(2).mean(1)
            lam = torch.maximum(lam, 1e-10 * lam.amax(1, keepdim=True))
            yw = yt / lam[:, None, :]
            R, P = yw @ yth, yw @ yh
            tr = torch.diagonal(R, dim1=-2, dim2=-1).real.sum(-1)
            G = torch.linalg.solve(R + (LOADING * tr / D)[:, None, None] * eye, P)
            x = y - G.conj().transpose(1, 2) @ yt
        X[:, j * LB:(j + 1) * LB] = x.permute(1, 2, 0).to(torch.complex64)
    return X


def fp64_count(C, T):
    D = C * K
    sums = 8.0 * (D * (D + 1) // 2 + D * C) * ITERS
    resid = 8.0 * D * C * ITERS                      # iterations 2.. over the window, and the output
    return float(T) * F * sums, float(T) * F * resid


def bench(dev, T, reps):
    res = {}
    for C in (7, 1):
        Y = reverberant_inputs(C, T, dev)
        X = torch.empty_like(Y)

        def run_hip():
            return ops.wpe(Y, K, DELAY, ITERS, LB, 0, LOADING, ref=0, want_mag=True, X=X)

        run_hip()
        tX = torch_wpe(Y)
        torch.cuda.synchronize()
        x_err = float((X - tX).abs().max() / tX.abs().max())
        gain = float((Y.abs().pow(2).sum() / X.abs().pow(2).sum()).log10() * 10.0)
        del tX
        ms_h, ms_t = [], []
        for _ in range(3):                      # alternating
            ms_h.append(timed(run_hip, reps))
            ms_t.append(timed(lambda: torch_wpe(Y), 1))
        sums, resid = fp64_count(C, T)
        ms = float(np.median(ms_h))
        res["C=%d" % C] = {
            "frames": T, "blocks": wp.num_blocks(T, LB), "D": C * K, "workgroups": wp.num_blocks(T, LB) * F,
            "hip_ms": round(ms, 3), "hip_ms_all": [round(v, 3) for v in ms_h],
            "fp64_Gop_sums": round(sums / 1e9, 1), "fp64_Gop_residual": round(resid / 1e9, 1),
            "ms_at_fp64_peak_sums_only": round(sums / FP64_PEAK * 1e3, 2),
            "ms_at_fp64_peak_all": round((sums + resid) / FP64_PEAK * 1e3, 2),
            "frac_of_fp64_peak_all": round((sums + resid) / (ms * 1e-3) / FP64_PEAK, 3),
            "MB_read_and_written": round(float(T) * F * C * 8 * (2 * ITERS + 2) / 1e6, 1),
            "torch_ms": round(float(np.median(ms_t)), 1), "torch_ms_all": [round(v, 1) for v in ms_t],
            "torch_over_hip": round(float(np.median(ms_t)) / ms, 1),
            "X_max_diff_vs_torch_rel_to_largest": x_err, "energy_removed_dB": round(gain, 2)}
        del Y, X
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=225000, help="a multiple of 600")
    a = ap.parse_args()
    if a.frames % LB:
        ap.error("--frames must be a multiple of %d" % LB)
    print(json.dumps({"one_hour": bench(torch.device("cuda", 0), a.frames, a.reps)}, indent=1))


if __name__ == "__main__":
    main()
