#!/usr/bin/env python3
"""Timings of the mask-guided cACGMM (profiles/cacgmm.txt): everything in one process on one device, HIP events around
synchronised work, warmed up, variants alternating.  There is no parent figure and no target: sk_mvdr and sk_wpe at their
defaults on the same recording are there for scale.

  kernel    sk_cacgmm on a 60 s recording of 7 channels and 2 streams (T = 3 751 frames; blocks of 200 frames with 200 frames of
            context on either side, loading 1e-3 -- separate_recording's defaults; synthetic spectra of tests/_cacgmm_cases.py's
            construction) at 1, 5 and 10 iterations: the whole call by HIP events against a COUNT of its fp64 operations, a
            multiply and an add as two.  Per frame of a window and iteration, K classes, C channels:
              directions      5 C                        (|y|^2 summed, 2 C divisions)
              substitutions   K (8 C (C - 1) / 2 + 5 C)  (a complex multiply-add is 8; the scaling by 1 / U[a][a], |x|^2)
              sums            K (8 C (C + 1) / 2 + 2 C)  (w z_a once per (class, a); the kernel forms it once per entry)
            and once more per frame of the recording the first two for the output pass; log, exp and the softmax are not
            counted (3 K logs and K exps per frame).  Peak: 78.6 TFLOP/s fp64 vector, which assumes fused multiply-adds; the
            kernel issues multiplies and adds separately (sepkern/cacgmm.py's arithmetic has one rounding per operation).
  scale     ops.mvdr (blocks of 200 frames, one block of context) and ops.wpe (10 taps, delay 3, 3 iterations, blocks of 600
            frames) on the same spectra in the same process.

    python tools/cacgmm_bench.py [--reps 5] [--seconds 60]
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

from sepkern import ops, cacgmm as cg  # noqa: E402

FP64_PEAK = 78.6e12          # vector fp64, 256 CUs x 4 SIMDs x 16 lanes x 2 (FMA) x 2.4 GHz
F = 257
C, S = 7, 2
LB, LC, LOADING = 200, 200, 1e-3
ITERATIONS = (1, 5, 10)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def spatial_inputs(T, dev):
    """tests/_cacgmm_cases.py's construction with torch's generator: Y (C, T, F) complex64, prior (T, S F) float32."""
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    gauss = lambda *sh: torch.complex(torch.randn(*sh, device=dev, generator=g), torch.randn(*sh, device=dev, generator=g)) * (0.5 ** 0.5)
    t = torch.arange(T, device=dev)[None, :, None]
    env = 0.05 + torch.sin(t * (0.05 + 0.35 * torch.rand(S, 1, F, device=dev, generator=g)) + 6.0 * torch.rand(S, 1, F, device=dev, generator=g)) ** 2
    src = gauss(S, T, F) * env
    h = gauss(S, C, 1, F)
    img = h * src[:, None]                                                               # (S, C, T, F)
    Y = img.sum(0)
    Y = Y + 0.316 * float(Y.abs().pow(2).mean().sqrt()) * gauss(C, T, F)
    power = img.abs().pow(2).mean(1)                                                      # (S, T, F)
    irm = power / power.sum(0)
    m = (irm + 0.35 * (0.5 - irm) + 0.1 * torch.randn(S, T, F, device=dev, generator=g)).clamp(0.0, 1.0)
    dominant = (power == power.amax(0)).float()
    return Y.contiguous(), m.permute(1, 0, 2).reshape(T, S * F).contiguous(), dominant.permute(1, 0, 2).reshape(T, S * F)


def fp64_count(T, iterations):
    windows = sum(w1 - w0 for _, _, w0, w1 in (cg.block_window(j, T, LB, LC) for j in range(cg.num_blocks(T, LB))))
    a = 5 * C + S * (8 * C * (C - 1) // 2 + 5 * C)
    b = S * (8 * C * (C + 1) // 2 + 2 * C)
    return float(F) * (windows * iterations * (a + b) + T * a), a, b, windows


def bench(dev, T, reps):
    Y, prior, dominant = spatial_inputs(T, dev)
    out = torch.empty(T, S * F, dtype=torch.float32, device=dev)
    runs = {"cacgmm I=%d" % I: (lambda I=I: ops.cacgmm(Y, prior, S, I, LB, LC, LOADING, out=out)) for I in ITERATIONS}
    runs["mvdr"] = lambda: ops.mvdr(Y, prior, S, 200, 1, 0, 1e-3)
    runs["wpe"] = lambda: ops.wpe(Y, 10, 3, 3, 600, 0, 1e-3)
    res = {"frames": T, "channels": C, "streams": S, "blocks": cg.num_blocks(T, LB), "workgroups": cg.num_blocks(T, LB) * F}
    base = float((prior - dominant).abs().mean())
    for name, fn in runs.items():
        fn()
    ms = {name: [] for name in runs}
    for _ in range(3):                      # alternating
        for name, fn in runs.items():
            ms[name].append(timed(fn, reps))
    for I in ITERATIONS:
        name = "cacgmm I=%d" % I
        mask, _ = runs[name]()
        torch.cuda.synchronize()
        ops_n, a, b, windows = fp64_count(T, I)
        m = float(np.median(ms[name]))
        res[name] = {"ms": round(m, 3), "ms_all": [round(v, 3) for v in ms[name]], "fp64_Gop": round(ops_n / 1e9, 2),
                     "ops_per_window_frame_and_iteration": a + b, "ops_per_output_frame": a, "window_frames": windows,
                     "ms_at_fp64_peak": round(ops_n / FP64_PEAK * 1e3, 4), "frac_of_fp64_peak": round(ops_n / (m * 1e-3) / FP64_PEAK, 4),
                     "TFLOPs_fp64": round(ops_n / (m * 1e-3) / 1e12, 3),
                     "mean_abs_mask_minus_dominant_over_priors": round(float((mask - dominant).abs().mean()) / base, 3)}
    for name in ("mvdr", "wpe"):
        res[name] = {"ms": round(float(np.median(ms[name])), 3), "ms_all": [round(v, 3) for v in ms[name]]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=60.0, help="length of the recording at 8 kHz")
    a = ap.parse_args()
    T = 1 + int(a.seconds * 8000) // 128
    print(json.dumps({"sixty_seconds": bench(torch.device("cuda", 0), T, a.reps)}, indent=1))


if __name__ == "__main__":
    main()
