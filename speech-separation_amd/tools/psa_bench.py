#!/usr/bin/env python3
"""Timings of the phase-sensitive front end (profiles/psa_loss.txt): everything in one process on one device, HIP events
around synchronised work, warmed up, variants alternating.

  kernel    sk_stft_psa stand-alone on a ragged batch of 32 utterances of U(24 k, 64 k) int16 samples, S = 2 and S = 3: time per
            launch by the ops' own events, achieved GB/s and fraction of 8 TB/s in algorithmic bytes ((S+1) x 128 samples in,
            (S+1) x 257 floats out per frame)
  front     the whole front end of one batch as compute_loss calls it, fused (psa_features_from_pcm: one sk_stft_psa launch that
            writes packed rows) beside what it replaces (features_from_pcm: S+1 sk_stft launches into zero-filled (T,B,F) grids,
            each packed into rows), alternating, median; the ratio
  step      the 3 x 896, 32-utterance ragged --wav-input training step with loss=psa beside loss=mse from the same PCM batch,
            alternating, median of --steps each, with each arm's spread

    python tools/psa_bench.py [--reps 50] [--steps 10] [--skip-step] [--out profiles/psa_bench.json]
"""
import argparse
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
from sepkern.data import features_from_pcm, psa_features_from_pcm  # noqa: E402

HBM_GBS = 8000.0


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def profiled(fn, reps):
    """{class: (us per launch, algorithmic bytes per launch)} of fn(repeat=reps) by the ops' own events."""
    fn(2)
    torch.cuda.synchronize()
    ops.PROF = {}
    fn(reps)
    torch.cuda.synchronize()
    prof, ops.PROF = ops.prof_summary(), None
    return {cls: (1e3 * ms / reps, by / reps) for cls, (_, ms, by) in prof.items()}


def ragged_batch(S, seed=0, batch=32):
    """A WavCollator-shaped PCM batch on the host: {'flat' int16 key-major, 'keys', 'lens'}, longest first."""
    rng = np.random.default_rng(seed)
    lens = sorted((int(v) for v in rng.integers(24000, 64001, batch)), reverse=True)
    sigs = synth.pcm_batch(batch, num_spk=S, lengths=lens)
    keys = ["mix"] + ["source%d" % (s + 1) for s in range(S)]
    flat = np.concatenate([sig[q] for q in range(S + 1) for sig in sigs])
    return {"flat": torch.from_numpy(flat), "keys": keys, "lens": lens}


def bench_kernel(dev, reps, rounds=7):
    from sepkern.packing import Packing
    out = {}
    for S in (2, 3):
        pcm = ragged_batch(S)
        pcm = dict(pcm, flat=pcm["flat"].to(dev))
        ns, total = pcm["lens"], sum(pcm["lens"])
        starts = [sum(ns[:j]) for j in range(len(ns))]
        offs = [[q * total + st for st in starts] for q in range(S + 1)]
        pk = Packing([1 + n // 128 for n in ns], dev)
        res = profiled(lambda rep: ops.stft_psa(pcm["flat"], offs, ns, S, pk=pk, repeat=rep), reps)
        us, by = res["stft_psa_kernel"]
        r = {"frames": pk.R, "us_per_launch": round(us, 1), "MB_algorithmic": round(by / 1e6, 2),
             "GBs_algorithmic": round(by / us / 1e3, 1), "fraction_of_8TBs": round(by / us / 1e3 / HBM_GBS, 3)}
        # what the launch replaces, launch for launch: the S + 1 sk_stft launches alone (no zero-fill, no pack)
        grid = torch.zeros(pk.T, pk.B, 257, device=dev)
        gargs = dict(lengths=ns, out=grid, out_offs=[b * 257 for b in range(pk.B)], stride_t=[pk.B * 257] * pk.B, stride_f=[1] * pk.B)

        def stfts(rep):
            for q in range(S + 1):
                ops.stft_batch(pcm["flat"][q * total:(q + 1) * total], repeat=rep, **gargs)
        r["sk_stft_launches_alone_us"] = round(profiled(stfts, reps)["stft_kernel"][0], 1)
        # the whole front end as compute_loss calls it, alternating
        fused, unfused = [], []
        for f in (lambda: psa_features_from_pcm(pcm, dev), lambda: features_from_pcm(pcm, dev)):
            timed(f, 3)
        for _ in range(rounds):
            fused.append(timed(lambda: psa_features_from_pcm(pcm, dev), reps))
            unfused.append(timed(lambda: features_from_pcm(pcm, dev), reps))
        r["front_end_fused_us"] = round(1e3 * float(np.median(fused)), 1)
        r["front_end_sk_stft_zero_fill_pack_us"] = round(1e3 * float(np.median(unfused)), 1)
        r["front_end_spread_us"] = {"fused": [round(1e3 * min(fused), 1), round(1e3 * max(fused), 1)],
                                    "sk_stft_zero_fill_pack": [round(1e3 * min(unfused), 1), round(1e3 * max(unfused), 1)]}
        r["ratio_replaced_over_fused"] = round(float(np.median(unfused)) / float(np.median(fused)), 2)
        out["S=%d" % S] = r
    return out


def bench_step(dev, steps, warmup=3):
    import uPIT
    from sepkern.optim import ClipAdam
    batch = {"pcm": ragged_batch(2, seed=1)}
    models = {}
    for kind in ("mse", "psa"):
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
    ms = {k: [] for k in models}
    for _ in range(steps):                      # alternating
        for kind in models:
            ms[kind].append(timed(lambda: step(kind), 1))
    res = {"loss=" + k: {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
           for k, v in ms.items()}
    res["psa_minus_mse_ms"] = round(res["loss=psa"]["median_ms"] - res["loss=mse"]["median_ms"], 3)
    res["frames"] = int(sum(1 + n // 128 for n in batch["pcm"]["lens"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"kernel": bench_kernel(dev, a.reps)}
    if not a.skip_step:
        res["training_step_3x896_b32_wav_input"] = bench_step(dev, a.steps)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
