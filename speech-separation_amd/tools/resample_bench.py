#!/usr/bin/env python3
"""Timings of the resampling front end (profiles/resample.txt): everything in one process on one device, HIP events around
synchronised work, warmed up, variants alternating.

  kernel    sk_resample stand-alone, 16 k -> 8 k and 44.1 k -> 8 k, int16 in: a 32-utterance x 3-signal training batch of
            64 k-sample signals, and an extract_feats chunk of 256 files of 3 .. 8 s: time per launch and achieved GB/s in
            algorithmic bytes (input once, output once); beside it the two sk_stft launches (magnitude + complex) of the
            resampled mixtures that follow it in the loss=sisdr input path
  error     rms and largest error of the kernel against sepkern/resample.py's fp64 reference per rate pair (unit-scale noise)
  step      the 3 x 896, 32-utterance --wav-input training step fed a 16 kHz batch (resampled on the device inside the step)
            beside the same batch pre-resampled to 8 kHz int16 -- the same output lengths --, loss=mse and loss=sisdr

    python tools/resample_bench.py [--reps 50] [--steps 10] [--skip-step] [--out profiles/resample.txt]
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
from sepkern import resample as R  # noqa: E402

PAIRS = [(16000, 8000), (44100, 8000)]


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


def bench_kernel(dev, reps):
    out = {}
    rng = np.random.default_rng(0)
    shapes = {"train batch 32 x 3 x 64000": [64000] * 96,
              "extract_feats chunk 256 files": [int(v) for v in rng.uniform(3.0, 8.0, 256) * 16000]}
    for name, ns16 in shapes.items():
        for sr_in, sr_out in PAIRS:
            ns = [n * sr_in // 16000 for n in ns16]                       # the same durations at either rate
            flat = torch.from_numpy(rng.integers(-20000, 20000, sum(ns)).astype(np.int16)).to(dev)
            res = profiled(lambda rep: ops.resample_batch(flat, ns, sr_in, sr_out, repeat=rep), reps)
            us, by = res["resample_kernel"]
            pl = R.plan(sr_in, sr_out)
            key = "%s, %d -> %d" % (name, sr_in, sr_out)
            out[key] = {"us_per_launch": round(us, 1), "MB_algorithmic": round(by / 1e6, 2), "GBs_algorithmic": round(by / us / 1e3, 1),
                        "GFLOP": round(2e-9 * pl.ntaps * sum(pl.out_len(n) for n in ns), 2),
                        "TFLOPs": round(2e-6 * pl.ntaps * sum(pl.out_len(n) for n in ns) / us, 2)}
            if name.startswith("train"):                                     # the launches it precedes: the mixtures' two STFTs
                y, outs = ops.resample_batch(flat, ns, sr_in, sr_out)
                nmix = len(ns) // 3
                mix = y[:sum(outs[:nmix])]

                def stfts(rep):
                    ops.stft_batch(mix, lengths=outs[:nmix], repeat=rep)
                    ops.stft_batch(mix, lengths=outs[:nmix], want_complex=True, repeat=rep)
                s = profiled(stfts, reps)
                out[key]["two_stft_launches_us"] = round(s["stft_kernel"][0], 1)      # (the class's time per round: both launches)
    return out


def bench_error(dev):
    out = {}
    rng = np.random.default_rng(1)
    for sr_in, sr_out in [(16000, 8000), (48000, 8000), (44100, 8000), (11025, 8000), (8000, 16000)]:
        ns = [20000, 7777]
        x = (rng.standard_normal(sum(ns)) * 0.25).astype(np.float32)
        y, outs = ops.resample_batch(torch.from_numpy(x).to(dev), ns, sr_in, sr_out)
        y = y.cpu().numpy().astype(np.float64)
        ref = np.concatenate([R.resample_host(x[:ns[0]], sr_in, sr_out), R.resample_host(x[ns[0]:], sr_in, sr_out)])
        out["%d -> %d" % (sr_in, sr_out)] = {"ntaps": R.plan(sr_in, sr_out).ntaps, "rms_error": float(np.sqrt(np.mean((y - ref) ** 2))),
                                            "max_error": float(np.abs(y - ref).max()), "signal_rms": float(np.sqrt(np.mean(ref ** 2)))}
    return out


def bench_step(dev, steps, warmup=3):
    import uPIT
    from sepkern.optim import ClipAdam
    rng = np.random.default_rng(2)
    lens16 = sorted((int(v) for v in rng.integers(48000, 128001, 32)), reverse=True)       # 3 .. 8 s at 16 kHz
    samples = []
    for sig in synth.pcm_batch(32, num_spk=2, lengths=lens16):
        samples.append({"mix": sig[0], "source1": sig[1], "source2": sig[2], "rate": 16000})
    b16 = uPIT.WavCollator(8000)(samples)
    # the same tree pre-resampled to 8 kHz int16 (what a wav8k copy of it would hold): the same output lengths
    pcm = b16["pcm"]
    y, outs = ops.pcm_to_rate(pcm["flat"].to(dev), pcm["lens"] * 3, pcm["rate"] * 3, 8000)
    q = torch.clamp(torch.round(y * 32768.0), -32768, 32767).to(torch.int16).cpu()
    b8 = {"pcm": {"flat": q, "keys": list(pcm["keys"]), "lens": outs[:32]}}
    res = {}
    for kind in ("mse", "sisdr"):
        torch.manual_seed(0)
        m = uPIT.SepDNN(0, hidden_dim="896", num_layers="3", loss=kind)
        m.cuda()
        m.train()
        opt = ClipAdam(m, lr=1e-4, max_norm=0.25)

        def step(batch):
            loss, _ = uPIT.compute_loss(m, 0, batch)
            loss.backward()
            opt.step()

        for b in (b16, b8):
            for _ in range(warmup):
                step(b)
        ms = {"wav16k_resampled_in_step": [], "pre_resampled_8k": []}
        for _ in range(steps):                      # alternating
            ms["wav16k_resampled_in_step"].append(timed(lambda: step(b16), 1))
            ms["pre_resampled_8k"].append(timed(lambda: step(b8), 1))
        r = {k: {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)} for k, v in ms.items()}
        r["difference_ms"] = round(r["wav16k_resampled_in_step"]["median_ms"] - r["pre_resampled_8k"]["median_ms"], 3)
        res["loss=" + kind] = r
        del m, opt
    res["frames"] = int(sum(1 + n // 128 for n in outs[:32]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"kernel": bench_kernel(dev, a.reps), "error_vs_fp64": bench_error(dev)}
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
