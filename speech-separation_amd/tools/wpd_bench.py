#!/usr/bin/env python3
"""Timings of WPD convolutional beamforming (profiles/wpd.txt): everything in one process on one device, HIP events around
synchronised work, warmed up, variants alternating.

  wpd       sk_wpd on a 10-minute recording of 7 channels (T = 37 500 frames, blocks of 600 frames, no context, a delay of 3,
            2 iterations, loading 1e-3, floor 1e-6, W_out written; synthetic reverberant sources and their ideal ratio masks,
            tests/_wpd_cases.py's construction with torch's generator) at the defaults (5 taps, D = 42) and at the most taps
            7 channels admit (10 taps, D = 77 of at most 80), for S = 2 and S = 3 streams: the whole call by HIP events against
            a COUNT of its fp64 operations -- per (t, f), stream and iteration 8 (D (D + 1) / 2 + C C) for the sums of R and
            PHI, 8 D for the power (from the second iteration on, and once more for the output) -- at the 78.6 TFLOP/s fp64
            vector peak.  The count takes a multiply and an add as the two halves of a fused multiply-add; the kernel issues
            them separately (sepkern/wpd.py's arithmetic has one rounding per operation), so its own floor is twice the count's.
  cascade   what sk_wpd takes the place of, in the same process and call, alternating with it: sk_wpe (10 taps, a delay of 3,
            3 iterations, blocks of 600 frames) and then sk_mvdr on its output (blocks of 200 frames, a context of one block),
            the defaults of steps/separate_wav.py, with the same masks.  The two do not compute the same thing; the figure
            stands beside sk_wpd's for scale only.

    python tools/wpd_bench.py [--reps 3] [--frames 37500]
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

from sepkern import ops, wpd as wd  # noqa: E402

FP64_PEAK = 78.6e12          # vector fp64, 256 CUs x 4 SIMDs x 16 lanes x 2 (FMA) x 2.4 GHz
F = 257
C = 7
DELAY, ITERS, LB, LOADING, FLOOR = 3, 2, 600, 1e-3, 1e-6
WPE = (10, 3, 3, 600, 0, 1e-3)
MVDR = (200, 1, 0, 1e-3)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def scene(S, T, dev, taps=12, decay=0.7):
    """tests/_wpd_cases.py's construction with torch's generator: Y (C, T, F) complex64, mask (T, S F) float32 for channel 0."""
    g = torch.Generator(device=dev)
    g.manual_seed(10 * S + 1)
    gauss = lambda *sh: torch.complex(torch.randn(*sh, device=dev, generator=g), torch.randn(*sh, device=dev, generator=g)) * (0.5 ** 0.5)
    Y = torch.zeros(C, T, F, dtype=torch.complex64, device=dev)
    power = torch.empty(S, T, F, device=dev)
    for s in range(S):
        env = 0.2 + torch.sin(torch.arange(T, device=dev)[:, None] * (0.2 + 0.4 * torch.rand(1, F, device=dev, generator=g))
                              + 6.0 * torch.rand(1, F, device=dev, generator=g)).abs()
        src = gauss(T, F) * env
        X = torch.zeros(C, T, F, dtype=torch.complex64, device=dev)
        for u in range(taps):
            X[:, u:] += gauss(C, 1, F) * decay ** u * src[None, :T - u]
        power[s] = X[0].abs().pow(2)
        Y += X
    Y += 0.03 * float(Y.abs().pow(2).mean().sqrt()) * gauss(C, T, F)
    mask = (power / power.sum(0, keepdim=True)).permute(1, 0, 2).reshape(T, S * F).contiguous()
    return Y, mask


def fp64_count(S, K, T):
    D = C * (K + 1)
    sums = 8.0 * (D * (D + 1) // 2 + C * C) * ITERS
    power = 8.0 * D * ITERS                          # iterations 2.. over the window, and the output
    return float(T) * F * S * sums, float(T) * F * S * power


def bench(dev, T, reps):
    res = {}
    for S in (2, 3):
        Y, mask = scene(S, T, dev)
        Z = torch.empty(S, T, F, dtype=torch.complex64, device=dev)
        X = torch.empty_like(Y)

        def cascade():
            ops.wpe(Y, *WPE, ref=0, X=X)
            return ops.mvdr(X, mask, S, *MVDR)

        for K in (5, 10):
            def run_wpd():
                return ops.wpd(Y, mask, S, K, DELAY, ITERS, LB, 0, LOADING, FLOOR, ref=0, want_W=True, Z=Z)

            _, Wd = run_wpd()
            cascade()
            torch.cuda.synchronize()
            e = torch.zeros(C * (K + 1), dtype=torch.complex128, device=dev)
            e[0] = 1.0
            fell_back = int((Wd == e).all(-1).sum())
            finite = bool(torch.isfinite(torch.view_as_real(Z)).all())
            ms_w, ms_c = [], []
            for _ in range(3):                      # alternating
                ms_w.append(timed(run_wpd, reps))
                ms_c.append(timed(cascade, reps))
            sums, power = fp64_count(S, K, T)
            ms = float(np.median(ms_w))
            nblk = wd.num_blocks(T, LB)
            res["S=%d K=%d" % (S, K)] = {
                "frames": T, "channels": C, "blocks": nblk, "D": C * (K + 1), "workgroups": nblk * F * S,
                "cells_that_fell_back": fell_back, "Z_finite": finite,
                "wpd_ms": round(ms, 3), "wpd_ms_all": [round(v, 3) for v in ms_w],
                "fp64_Gop_sums": round(sums / 1e9, 1), "fp64_Gop_power": round(power / 1e9, 1),
                "ms_at_fp64_peak_all": round((sums + power) / FP64_PEAK * 1e3, 2),
                "frac_of_fp64_peak_all": round((sums + power) / (ms * 1e-3) / FP64_PEAK, 3),
                "cascade_wpe_mvdr_ms": round(float(np.median(ms_c)), 3), "cascade_ms_all": [round(v, 3) for v in ms_c],
                "wpd_over_cascade": round(ms / float(np.median(ms_c)), 2)}
        del Y, mask, Z, X
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=37500)
    a = ap.parse_args()
    print(json.dumps({"ten_minutes_seven_channels": bench(torch.device("cuda", 0), a.frames, a.reps)}, indent=1))


if __name__ == "__main__":
    main()
