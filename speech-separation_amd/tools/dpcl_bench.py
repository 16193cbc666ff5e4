#!/usr/bin/env python3
"""Timings of the deep-clustering kernels (profiles/dpcl.txt): everything in one process on one device, HIP events around
synchronised work, warmed up, variants alternating.  There is no parent figure and no target.

  kernels   sk_dpcl_fwd, sk_dpcl_bwd and sk_dpcl_kmeans (20 iterations, farthest-first initialisation, S = 2) on 32 utterances of
            400 frames, F = 257, at D = 20 and D = 40, both weightings: the whole call by HIP events against its ALGORITHMIC
            bytes at 8 TB/s (ops.dpcl_*'s own count: every operand read once per pass over the points, every result written
            once; z alone is 263 MB at D = 20 and 526 MB at D = 40).
  step      one training step (forward, loss, backward, clip + Adam) of the 3 x 896 network on 32 x 400 frames with loss=dpcl,
            D = 20, beside the same step with loss=mse, in the same process, alternating.

    python tools/dpcl_bench.py [--reps 5] [--no-step]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
for p in (PKG, HERE, os.path.join(PKG, "archs")):
    if p not in sys.path:
        sys.path.insert(0, p)

from sepkern import ops  # noqa: E402
from sepkern.packing import Packing  # noqa: E402

HBM_PEAK = 8.0e12
F, B, T, S = 257, 32, 400, 2


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(runs, reps, rounds=3):
    for fn in runs.values():
        fn()
    ms = {name: [] for name in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            ms[name].append(timed(fn, reps))
    return ms


def entry(ms, nbytes=None):
    m = float(np.median(ms))
    out = {"ms": round(m, 4), "ms_all": [round(v, 4) for v in ms]}
    if nbytes is not None:
        out.update(algorithmic_MB=round(nbytes / 1e6, 1), ms_at_8TBs=round(nbytes / HBM_PEAK * 1e3, 4),
                   frac_of_8TBs=round(nbytes / (m * 1e-3) / HBM_PEAK, 3))
    return out


def kernels(dev, reps):
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    pk = Packing(np.full(B, T, dtype=np.int32), dev)
    R = pk.R
    mix = torch.rand(R, F, device=dev, generator=g) ** 3
    srcs = [torch.rand(R, F, device=dev, generator=g) for _ in range(S)]
    one = torch.ones(1, device=dev)
    res = {"utterances": B, "frames": T, "points": R * F}
    for D in (20, 40):
        z = torch.sigmoid(torch.randn(R, F * D, device=dev, generator=g) * 1.5)
        dz = torch.empty_like(z)
        mask = torch.empty(R, S * F, device=dev)
        fwd = {w: ops.dpcl_fwd(z, mix, srcs, pk, D, w) for w in ("mr", "vad")}
        runs = {"fwd mr": lambda: ops.dpcl_fwd(z, mix, srcs, pk, D, "mr"), "fwd vad": lambda: ops.dpcl_fwd(z, mix, srcs, pk, D, "vad"),
                "bwd mr": lambda: ops.dpcl_bwd(z, mix, srcs, pk, D, fwd["mr"], one, "mr", out=dz),
                "bwd vad": lambda: ops.dpcl_bwd(z, mix, srcs, pk, D, fwd["vad"], one, "vad", out=dz),
                "kmeans 20": lambda: ops.dpcl_kmeans(z, mix, pk, S, 20, out=mask, D=D),
                "kmeans 0": lambda: ops.dpcl_kmeans(z, mix, pk, S, 0, out=mask, D=D)}
        ms = alternate(runs, reps)
        pts = float(R) * F * 4
        nbytes = {"fwd mr": pts * (D + 1 + S), "fwd vad": pts * (D + 2 + S), "bwd mr": pts * (2 * D + 1 + S), "bwd vad": pts * (2 * D + 1 + S),
                  "kmeans 20": pts * ((S - 1 + 21) * (D + 1) + 2 + S + 1), "kmeans 0": pts * ((S - 1 + 1) * (D + 1) + 2 + S + 1)}
        res["D=%d" % D] = {name: entry(ms[name], nbytes[name]) for name in runs}
        it = (float(np.median(ms["kmeans 20"])) - float(np.median(ms["kmeans 0"]))) / 20.0
        res["D=%d" % D]["kmeans per iteration"] = {"ms": round(it, 4), "algorithmic_MB": round(pts * (D + 1) / 1e6, 1),
                                                   "frac_of_8TBs": round(pts * (D + 1) / (it * 1e-3) / HBM_PEAK, 3)}
        del z, dz
    return res


def step(dev, reps):
    import uPIT
    from sepkern.optim import ClipAdam
    g = torch.Generator(device=dev)
    g.manual_seed(4)
    pk = Packing(np.full(B, T, dtype=np.int32), dev)
    mix = torch.rand(pk.Rp, F, device=dev, generator=g)
    srcs = [torch.rand(pk.Rp, F, device=dev, generator=g) * 0.6 for _ in range(S)]
    batch = {"packed": (mix, srcs, pk)}
    runs = {}
    for loss in ("mse", "dpcl"):
        torch.manual_seed(1)
        model = uPIT.SepDNN(0, hidden_dim="896", num_layers="3", num_spk=str(S), loss=loss, embed_dim="20")
        model.cuda()
        model.train()
        opt = ClipAdam(model, lr=1e-3, max_norm=0.25)

        def one(model=model, opt=opt):
            l, _ = uPIT.compute_loss(model, 0, batch)
            l.backward()
            opt.step()
        runs["step loss=%s" % loss] = one
    ms = alternate(runs, reps)
    return {name: entry(ms[name]) for name in runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"kernels": kernels(dev, a.reps)}
    if not a.no_step:
        out["training_step_3x896"] = step(dev, a.reps)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
