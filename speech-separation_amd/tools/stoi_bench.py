#!/usr/bin/env python3
"""Time of the STOI / ESTOI kernels (csrc/stoi.hip, sk_stoi) against the host function (sepkern/stoi.py).

For a batch of 256 two-speaker utterances of 4 s at 10 kHz (sepkern/synth.py sources, estimates = source + 0.2 other + noise):
  - us per batch of the device-resident call (ops.stoi on packed fp32 rows), HIP events around `reps` calls;
  - us per batch of each of its three kernels, from torch.profiler's kernel records of those calls;
  - the same batch through stoi.stoi_matrix on the host (on --cpu-utts utterances, scaled to the batch): the baseline is the
    host function, not an earlier version of the kernels;
  - the largest difference between the two on those utterances.
No speed-up is gated anywhere; profiles/stoi.txt keeps the output.

usage: stoi_bench.py [--utts 256] [--seconds 4] [--cpu-utts 8] [--reps 5]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from sepkern import ops, synth  # noqa: E402
from sepkern import stoi as ST  # noqa: E402

KERNELS = ("stoi_keep_kernel", "stoi_env_kernel", "stoi_score_kernel")


def batch(U, n, rng):
    refs, ests = [], []
    for u in range(U):
        r = np.stack([synth.speech_like(n, 7919 * u + s) for s in range(2)])
        e = r + 0.2 * r[::-1] + 0.05 * rng.standard_normal(r.shape)
        refs.append(r.astype(np.float32))
        ests.append(e.astype(np.float32))
    return refs, ests


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--cpu-utts", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    U, n, S = a.utts, int(a.seconds * ST.FS), 2
    refs, ests = batch(U, n, np.random.default_rng(0))
    rcat = torch.from_numpy(np.concatenate([r.reshape(-1) for r in refs])).cuda()
    ecat = torch.from_numpy(np.concatenate([e.reshape(-1) for e in ests])).cuda()
    offs, lens = [S * n * u for u in range(U)], [n] * U
    call = lambda: ops.stoi(rcat, ecat, offs, lens, S)      # noqa: E731
    out, frames = call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    us_call = e0.elapsed_time(e1) / a.reps * 1e3
    print("sk_stoi, %d utterances x %d sources x %d samples (%.1f s at 10 kHz), T = %d..%d frames: %.0f us per batch = %.0f utt/s"
          % (U, S, n, a.seconds, int(frames.min()), int(frames.max()), us_call, U / us_call * 1e6), flush=True)
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(a.reps):
            call()
        torch.cuda.synchronize()
    per = {k: [0.0, 0] for k in KERNELS}
    for ev in prof.events():
        for k in KERNELS:
            if k in ev.name:
                per[k][0] += float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0))
                per[k][1] += 1
    for k in KERNELS:
        if per[k][1]:
            print("  %-18s %8.1f us per batch (%d launches recorded)" % (k, per[k][0] / per[k][1], per[k][1]), flush=True)
        else:
            print("  %-18s no kernel record from the profiler" % k, flush=True)
    got = out.cpu().numpy()
    t0 = time.perf_counter()
    worst = 0.0
    for u in range(a.cpu_utts):
        want, fr = ST.stoi_matrix(list(refs[u]), list(ests[u]))
        assert fr.tolist() == frames[u].tolist()
        worst = max(worst, float(np.abs(got[u] - want).max()))
    cpu_s = (time.perf_counter() - t0) / a.cpu_utts
    print("host function stoi_matrix (fp64, %d torch threads): %.1f ms per utterance = %.0f us per batch of %d: %.0fx the kernels' time; "
          "largest |kernel - host| on %d utterances %.3g"
          % (torch.get_num_threads(), cpu_s * 1e3, cpu_s * U * 1e6, U, cpu_s * U * 1e6 / us_call, a.cpu_utts, worst), flush=True)


if __name__ == "__main__":
    main()
