#!/usr/bin/env python3
"""Timings of window stitching and of the wav-to-wav path (profiles/stitch.txt): everything in one process on one device, HIP
events around synchronised work, warmed up, variants alternating.

  kernels   sk_stitch's three launches at the one-hour shape (T = 225 000 frames, W = 400, Hn = 200 -> 1 124 windows; S = 2 and 4;
            window-major dense masks: noisy permuted slices of one global mask): time per launch (torch.profiler's device
            times, summed per kernel name), algorithmic bytes, share of the 8 TB/s HBM peak; the whole call by HIP events
  torch     for comparison only: the same stitch composed from PyTorch-ROCm's own ops on the same tensors in the same call
            (fp64 costs per output pair, the S! totals by one gather, arg-min, the chain on the host, gathers and an
            unfused a + r (b - a)); results compared
  path      separate_recording on a synthetic recording (default 10 minutes of int16 noise at 8 kHz), hidden_dim 896, 3 layers,
            fp32 and bf16: frames/s and the real-time factor -- beside the resident-batch inference rate of one 32 x 400 batch
            through forward_packed without stitching, in the same call

    python tools/stitch_bench.py [--reps 20] [--minutes 10] [--skip-path]
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
for p in (PKG, os.path.join(PKG, "archs"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from sepkern import ops, stitch as st  # noqa: E402
from sepkern.packing import Packing  # noqa: E402
from sepkern.separate import separate_recording  # noqa: E402

HBM_PEAK = 8.0e12
F = 257
T_HOUR, W, HN = 225000, 400, 200


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def hour_inputs(S, dev):
    """(mag (T, F), buf (K, W, S, F): window k = frames k Hn .. of one global mask, outputs permuted, + 0.05 noise, ramp)."""
    g = torch.Generator(device=dev)
    g.manual_seed(S)
    K = len(st.window_starts(T_HOUR, W, HN))
    assert HN * (K - 1) + W == T_HOUR                     # every window full: one dense (K, W, S, F) buffer
    glob = torch.rand(T_HOUR, S, F, device=dev, generator=g)
    mag = torch.randn(T_HOUR, F, device=dev, generator=g).abs()
    rows = torch.arange(K, device=dev)[:, None] * HN + torch.arange(W, device=dev)[None, :]
    q = torch.stack([torch.randperm(S, device=dev, generator=g) for _ in range(K)])            # (K, S)
    buf = glob[rows][torch.arange(K, device=dev)[:, None], :, q].permute(0, 2, 1, 3).contiguous()
    buf += 0.05 * (2.0 * torch.rand(buf.shape, device=dev, generator=g) - 1.0)
    return mag, buf, torch.from_numpy(st.default_ramp(W - HN)).to(dev)


def torch_stitch(mag, buf, ramp):
    """The definition with torch ops (every window full).  -> (out (T, S F), perms (K, S))."""
    K, _, S, _ = buf.shape
    O, dev = W - HN, buf.device
    ov = (torch.arange(1, K, device=dev)[:, None] * HN + torch.arange(O, device=dev)[None, :])          # (K-1, O) frames
    x = mag[ov].double()
    a, b = buf[:-1, HN:].double(), buf[1:, :O].double()
    cost = torch.stack([torch.stack([((x * (a[:, :, i] - b[:, :, j])) ** 2).sum((1, 2)) for j in range(S)], 1) for i in range(S)], 1)
    plist = torch.tensor(list(itertools.permutations(range(S))), device=dev)                             # (S!, S)
    totals = cost[:, torch.arange(S, device=dev)[None, :], plist].sum(-1)                                # (K-1, S!)
    p = plist[totals.argmin(1)].cpu().numpy()
    perms = np.zeros((K, S), dtype=np.int64)
    perms[0] = np.arange(S)
    for k in range(K - 1):                                 # the chain, on the host
        perms[k + 1] = p[k][perms[k]]
    perms = torch.from_numpy(perms).to(dev)
    wp = torch.gather(buf, 2, perms[:, None, :, None].expand(K, W, S, F))
    out = torch.empty(K * HN + O, S, F, device=dev)
    out[:O] = wp[0, :O]
    late = (torch.arange(K, device=dev)[:, None] * HN + torch.arange(O, W, device=dev)[None, :]).reshape(-1)
    out[late] = wp[:, O:].reshape(-1, S, F)
    ea, lb = wp[:-1, HN:], wp[1:, :O]
    out[ov.reshape(-1)] = (ea + ramp[None, :, None, None] * (lb - ea)).reshape(-1, S, F)
    return out.view(-1, S * F), perms


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
            if "stitch_" in e.key:
                name = [n for n in ("stitch_cost_kernel", "stitch_finish_kernel", "stitch_blend_kernel") if n in e.key][0]
                tot = getattr(e, "device_time_total", None)
                tot = getattr(e, "cuda_time_total", 0.0) if tot is None else tot
                out[name] = round(out.get(name, 0.0) + float(tot) / reps, 2)
        return out
    except Exception as e:                                 # reported, not hidden
        return {"unavailable": repr(e)}


def bench_kernels(dev, reps):
    res = {}
    for S in (2, 4):
        mag, buf, ramp = hour_inputs(S, dev)
        K, O = buf.shape[0], W - HN
        flat = buf.view(-1)
        desc = [(flat, k * W * S * F, S * F) for k in range(K)]
        out = torch.empty(T_HOUR, S * F, device=dev)

        def run_hip():
            return ops.stitch(mag, desc, T_HOUR, W, HN, S, ramp, out=out)

        def run_torch():
            return torch_stitch(mag, buf, ramp)

        _, perms, _ = run_hip()
        t_out, t_perms = run_torch()
        torch.cuda.synchronize()
        same = bool(torch.equal(perms.long(), t_perms)) and bool(torch.equal(out.view(torch.int32), t_out.view(torch.int32)))
        ms_h, ms_t = [], []
        for _ in range(3):                      # alternating
            ms_h.append(timed(run_hip, reps))
            ms_t.append(timed(run_torch, max(1, reps // 10)))
        ov = (K - 1) * O
        algo = {"stitch_cost_kernel": 4.0 * F * ov * (2 * S + 1), "stitch_finish_kernel": 8.0 * (K - 1) * S * S * (-(-O // 16) + 1),
                "stitch_blend_kernel": 4.0 * F * S * ((T_HOUR + ov) + T_HOUR)}
        per = launch_times(run_hip, reps)
        kern = {}
        for name, us in per.items():
            kern[name] = us if name == "unavailable" else {
                "us_per_launch": us, "MB_algorithmic": round(algo[name] / 1e6, 2),
                "frac_of_hbm_peak": round(algo[name] / (us * 1e-6) / HBM_PEAK, 3) if us else None}
        res["S=%d" % S] = {"windows": K, "mask_bytes_resident": st.memory_bytes(T_HOUR, W, HN, S), "launches": kern,
                           "hip_ms_whole_call": round(float(np.median(ms_h)), 4), "torch_ms": round(float(np.median(ms_t)), 3),
                           "torch_over_hip": round(float(np.median(ms_t) / np.median(ms_h)), 1), "torch_gives_the_same_bits": same,
                           "whole_call_frac_of_hbm_peak": round(sum(algo.values()) / (np.median(ms_h) * 1e-3) / HBM_PEAK, 3),
                           "hip_ms_all": [round(v, 4) for v in ms_h], "torch_ms_all": [round(v, 3) for v in ms_t]}
        del mag, buf, out, t_out, desc, flat
        torch.cuda.empty_cache()
    return res


def bench_path(dev, minutes, reps=3):
    import uPIT
    n = int(minutes * 60 * 8000)
    pcm = torch.from_numpy((np.random.default_rng(0).standard_normal(n) * 3000.0).astype(np.int16)).to(dev)
    T = 1 + n // 128
    res = {"recording": {"minutes": minutes, "samples": n, "frames": T, "windows": len(st.window_starts(T, W, HN))}}
    for dtype in ("fp32", "bf16"):
        torch.manual_seed(0)
        model = uPIT.SepDNN(0, hidden_dim="896", num_layers="3", num_spk="2", dtype=dtype)
        model.cuda()
        model.eval()
        pk = Packing(np.full(32, W, dtype=np.int32), dev)
        x = torch.randn(pk.Rp, F, device=dev).abs()

        def resident():
            with torch.no_grad():
                model.hidden = model.init_hidden(32)
                model.forward_packed(x, pk)

        def path():
            separate_recording(model, pcm, 8000, W, HN, 32, want_float=False, want_pcm=True)

        resident()
        path()
        ms_r, ms_p = [], []
        for _ in range(reps):                   # alternating
            ms_r.append(timed(resident, 5))
            ms_p.append(timed(path, 1))
        model.check_status()
        r, p = float(np.median(ms_r)), float(np.median(ms_p))
        res[dtype] = {"path_ms": round(p, 2), "path_frames_per_s": round(T / (p * 1e-3)), "real_time_factor": round(p * 1e-3 / (n / 8000.0), 6),
                      "resident_batch_ms": round(r, 3), "resident_frames_per_s": round(32 * W / (r * 1e-3)),
                      # every frame runs through the network about W / Hn times; the rest is what stitching and the front / back end cost
                      "network_frames_per_recording_frame": round(len(st.window_starts(T, W, HN)) * W / T, 3),
                      "path_ms_all": [round(v, 2) for v in ms_p], "resident_ms_all": [round(v, 3) for v in ms_r]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--skip-path", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"kernels_one_hour": bench_kernels(dev, a.reps)}
    if not a.skip_path:
        res["wav_to_wav"] = bench_path(dev, a.minutes)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
