#!/usr/bin/env python3
"""Timings of mask-based MVDR beamforming (profiles/mvdr.txt): everything in one process on one device, HIP events around
synchronised work, warmed up, variants alternating.

  kernels   sk_mvdr's three launches at the one-hour shape (T = 225 000 frames, blocks of 200 frames, a context of one block;
            C = 7, S = 2, the LibriCSS array, and C = 4, S = 4, one CHiME-5 array; a synthetic array: steering vectors times
            sparse Gaussian sources plus noise, noisy ratio masks): time per launch (torch.profiler's device times, summed per
            kernel name), algorithmic bytes against the 8 TB/s HBM peak, and for launches 1 and 2 the fp64 operations (a fused
            multiply-add counts two) against the 78.6 TFLOP/s fp64 vector peak; the whole call by HIP events
  torch     for comparison only: the same result composed from PyTorch-ROCm's own ops on the same tensors in the same call
            (complex128 matrix products per block, torch.linalg.solve); weights and Z compared

    python tools/mvdr_bench.py [--reps 10] [--frames 225000]
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

from sepkern import mvdr as mv, ops  # noqa: E402

HBM_PEAK = 8.0e12
FP64_PEAK = 78.6e12          # vector fp64, 256 CUs x 4 SIMDs x 16 lanes x 2 (FMA) x 2.4 GHz
F = 257
LB, R, LOADING = 200, 1, 1e-3
KERNELS = ("mvdr_stats_kernel", "mvdr_weights_kernel", "mvdr_apply_kernel")


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def array_inputs(C, S, T, dev):
    """tests/_mvdr_cases.py's construction with torch's generator: (Y (C, T, F) complex64, mask (T, S F) float32)."""
    g = torch.Generator(device=dev)
    g.manual_seed(10 * C + S)
    rnd = lambda *sh: torch.rand(*sh, device=dev, generator=g)
    gauss = lambda *sh: torch.complex(torch.randn(*sh, device=dev, generator=g), torch.randn(*sh, device=dev, generator=g)) * (0.5 ** 0.5)
    a = torch.polar(0.5 + rnd(S, 1, F, C), 2.0 * np.pi * rnd(S, 1, F, C))
    X = gauss(S, T, F) * (rnd(S, T, F) < 0.6)
    Y = torch.zeros(C, T, F, dtype=torch.complex64, device=dev)
    for s in range(S):
        Y += (a[s] * X[s][:, :, None]).permute(2, 0, 1)
    sigma = float(Y.abs().pow(2).mean().sqrt()) * 0.1
    Y += sigma * gauss(C, T, F)
    p = X.abs().pow(2)
    ratio = p / p.sum(0).clamp_min(1e-30)
    mask = (ratio + 0.05 * (2.0 * rnd(S, T, F) - 1.0)).clamp_(0.0, 1.0).permute(1, 0, 2).reshape(T, S * F).contiguous()
    return Y, mask


def torch_mvdr(Y, mask, S, ref):
    """The definition with torch ops (T a multiple of the block length; no fallback cells).  -> (weights, Z)."""
    C, T, _ = Y.shape
    nblk = T // LB
    y = Y.to(torch.complex128).view(C, nblk, LB, F).permute(1, 3, 0, 2)                  # (nblk, F, C, Lb)
    m = mask.to(torch.float64).view(nblk, LB, S, F).permute(2, 0, 3, 1)                     # (S, nblk, F, Lb)
    yh = y.conj().transpose(-1, -2).contiguous()
    A = torch.stack([torch.matmul(y * m[s][:, :, None, :], yh) for s in range(S)])          # (S, nblk, F, C, C)
    pad = torch.zeros_like(A[:, :R])
    Ap = torch.cat([pad, A, pad], 1)
    phi = sum(Ap[:, k:k + nblk] for k in range(2 * R + 1))
    W = []
    for s in range(S):
        N = sum(phi[o] for o in range(S) if o != s)
        tr = torch.diagonal(N, dim1=-2, dim2=-1).real.sum(-1)
        N = N + (LOADING * tr / C)[..., None, None] * torch.eye(C, dtype=torch.complex128, device=Y.device)
        G = torch.linalg.solve(N, phi[s])
        d = torch.diagonal(G, dim1=-2, dim2=-1).real.sum(-1)
        W.append((G[..., ref] / d[..., None]).to(torch.complex64))                         # (nblk, F, C)
    W = torch.stack(W, 1)                                                                   # (nblk, S, F, C)
    Z = torch.einsum("jsfc,cjtf->sjtf", W.conj(), Y.view(C, nblk, LB, F)).reshape(S, T, F)
    return W, Z


def fp64_ops(C, S, T, nblk):
    """fp64 operations of launches 1 and 2 as the kernels do them, a fused multiply-add counted as two."""
    off = C * (C - 1) // 2
    stats = float(T) * F * (off * 6 + C * 3 + (2 * off + C) * S * 2)
    chol = sum(4 * a + 2 + (C - 1 - a) * (8 * a + 2) for a in range(C))
    fwd = sum(8 * a + 2 for a in range(C))
    back = lambda k: sum(8 * (C - 1 - a) + 2 for a in range(k, C))
    solves = C * fwd + sum(back(k) for k in range(C)) + (back(0) - back(C // 2))          # column ref runs down to row 0
    ctx = (min(2 * R + 1, nblk) + (S - 1)) * (2 * off + C)
    weights = float(nblk) * S * F * (ctx + chol + solves + 4 * C)
    return {"mvdr_stats_kernel": stats, "mvdr_weights_kernel": weights}


def launch_times(fn, reps):
    """Device time per kernel name over `reps` calls (torch.profiler), in us per call; {} with the reason when unavailable."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            for name in KERNELS:
                if name in e.key:
                    tot = getattr(e, "device_time_total", None)
                    tot = getattr(e, "cuda_time_total", 0.0) if tot is None else tot
                    out[name] = round(out.get(name, 0.0) + float(tot) / reps, 2)
        return out
    except Exception as e:                                 # reported, not hidden
        return {"unavailable": repr(e)}


def bench(dev, T, reps):
    res = {}
    for C, S in ((7, 2), (4, 4)):
        Y, mask = array_inputs(C, S, T, dev)
        nblk, ref = mv.num_blocks(T, LB), 0
        weights = torch.empty(nblk, S, F, C, dtype=torch.complex64, device=dev)
        Z = torch.empty(S, T, F, dtype=torch.complex64, device=dev)

        def run_hip():
            return ops.mvdr(Y, mask, S, LB, R, ref, LOADING, weights=weights, Z=Z)

        def run_torch():
            return torch_mvdr(Y, mask, S, ref)

        run_hip()
        tW, tZ = run_torch()
        torch.cuda.synchronize()
        w_err = float(((weights - tW).abs().amax(-1) / tW.abs().amax(-1)).max())
        z_err = float((Z - tZ).abs().max() / tZ.abs().max())
        del tW, tZ
        ms_h, ms_t = [], []
        for _ in range(3):                      # alternating
            ms_h.append(timed(run_hip, reps))
            ms_t.append(timed(run_torch, 1))
        ws = float(mv.workspace_bytes(T, C, S, LB))
        algo = {"mvdr_stats_kernel": float(T) * F * (C * 8 + S * 4) + ws,
                "mvdr_weights_kernel": ws * min(2 * R + 1, nblk) + float(nblk) * S * F * C * 8,
                "mvdr_apply_kernel": float(T) * F * (C * 8 + S * 8) + float(nblk) * S * F * C * 8}
        flops = fp64_ops(C, S, T, nblk)
        per = launch_times(run_hip, reps)
        kern = {}
        for name, us in per.items():
            if name == "unavailable":
                kern[name] = us
                continue
            k = {"us_per_launch": us, "MB_algorithmic": round(algo[name] / 1e6, 1),
                 "frac_of_hbm_peak": round(algo[name] / (us * 1e-6) / HBM_PEAK, 3) if us else None}
            if name in flops:
                k["fp64_Gop"] = round(flops[name] / 1e9, 2)
                k["frac_of_fp64_peak"] = round(flops[name] / (us * 1e-6) / FP64_PEAK, 3) if us else None
                k["us_at_hbm_peak"] = round(algo[name] / HBM_PEAK * 1e6, 1)
                k["us_at_fp64_peak"] = round(flops[name] / FP64_PEAK * 1e6, 1)
            kern[name] = k
        res["C=%d S=%d" % (C, S)] = {
            "frames": T, "blocks": nblk, "workspace_bytes": int(ws), "launches": kern,
            "hip_ms_whole_call": round(float(np.median(ms_h)), 4), "torch_ms": round(float(np.median(ms_t)), 2),
            "torch_over_hip": round(float(np.median(ms_t) / np.median(ms_h)), 1),
            "whole_call_frac_of_hbm_peak": round(sum(algo.values()) / (np.median(ms_h) * 1e-3) / HBM_PEAK, 3),
            "weights_max_diff_vs_torch_rel_to_largest": w_err, "Z_max_diff_vs_torch_rel_to_largest": z_err,
            "hip_ms_all": [round(v, 4) for v in ms_h], "torch_ms_all": [round(v, 2) for v in ms_t]}
        del Y, mask, weights, Z
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=225000, help="a multiple of 200")
    a = ap.parse_args()
    if a.frames % LB:
        ap.error("--frames must be a multiple of %d" % LB)
    print(json.dumps({"one_hour": bench(torch.device("cuda", 0), a.frames, a.reps)}, indent=1))


if __name__ == "__main__":
    main()
