#!/usr/bin/env python3
"""Timings of reverberant dynamic mixing (profiles/reverb_mix.txt): everything in one call on one device, HIP events around
synchronised work, warmed up, the driver's two arms alternating.

  kernel    sk_fir_convolve stand-alone on ragged batches of int16 sources of U(24 k, 64 k) samples, S = 2 signals per mixture:
            B = 32 and the reference's default batch B = 100, every signal with a synthetic RIR of its own of 800, 2 400 and 4 800
            taps (0.1, 0.3, 0.6 s at 8 kHz); time per call (both launches) by the ops' own events, GFLOP/s in transform and
            product flops, and the workspace the call took
  driver    steps/train_qsub.py --wav-input --dynamic-mix over a synthetic corpus (sepkern/synth.py) listed as single-speaker
            utterances, each run a fresh process: plain beside --mix-rir-synth LO,HI on the same sources, alternating, --rounds
            runs of each; frames/s of every epoch after the first and the SEPKERN_PREFETCH_TIMING=1 breakdown

    python tools/reverb_bench.py [--reps 20] [--skip-driver] [--utts 512] [--samples 40000] [--epochs 4] [--rounds 2] [--t60 0.2,0.6] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
for p in (PKG, os.path.join(PKG, "archs"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from sepkern import _lib, ops, reverb, synth  # noqa: E402
from dynmix_bench import profiled, write_corpora  # noqa: E402


def bench_kernel(dev, reps):
    out = {}
    for B in (32, 100):
        S = 2
        rng = np.random.default_rng(B + S)
        lens = sorted((int(v) for v in rng.integers(24000, 64001, B)), reverse=True)
        sigs = synth.pcm_batch(B, num_spk=S, lengths=lens)
        flat = torch.from_numpy(np.concatenate([sig[1 + s] for s in range(S) for sig in sigs])).to(dev)
        total, starts = sum(lens), [sum(lens[:j]) for j in range(B)]
        in_offs = [s * total + st for s in range(S) for st in starts]
        ns = lens * S
        for taps in (800, 2400, 4800):
            rirs = [reverb.synthetic_rir(rng, taps / 8000.0, 8000, 5.0) for _ in range(S * B)]
            assert all(len(h) == taps for h in rirs)
            rflat = torch.from_numpy(np.concatenate(rirs)).to(dev)
            roffs, tp, dl = [taps * j for j in range(S * B)], [taps] * (S * B), [0] * (S * B)
            us, flops = profiled(lambda rep: ops.fir_convolve(flat, in_offs, ns, rflat, roffs, tp, dl, repeat=rep), reps)["fir_convolve"]
            J = S * B
            ws = _lib.load().sk_fir_workspace_bytes((C.c_int32 * J)(*ns), (C.c_int32 * J)(*tp), (C.c_int32 * J)(*dl), J)
            out["B=%d S=%d taps=%d" % (B, S, taps)] = {
                "samples_per_source": total, "longest": lens[0], "us_per_call": round(us, 1), "GFLOP": round(flops / 1e9, 3),
                "GFLOPs": round(flops / us / 1e3, 1), "workspace_MB": round(ws / 1e6, 1),
                # every spectrum written once and, in launch two, read once per (block, partition) pair: what L2 serves
                "MB_read_by_launch_two": round(2.0 * 264 * 8 * sum(-(-taps // 256) * (-(-n // 256)) for n in ns) / 1e6, 1)}
    return out


def run_driver(data, out_dir, conf, epochs, t60, utts, timeout):
    cmd = [sys.executable, os.path.join(PKG, "steps", "train_qsub.py"), "uPIT", "0", data, out_dir, "--model-config", conf,
           "--wav-input", "--batch-size", "32", "--num-epochs", str(epochs), "--seed", "1", "--dynamic-mix", "--mixes-per-epoch", str(utts)]
    if t60:
        cmd += ["--mix-rir-synth", t60]
    env = dict(os.environ, SEPKERN_PREFETCH_TIMING="1")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout, cwd=PKG)
    if r.returncode != 0:
        raise RuntimeError("train_qsub.py failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    rates = [float(m.group(1)) for m in re.finditer(r"= (\d+) frames/s", r.stderr)]
    stage = [tuple(float(v) for v in m.groups()) for m in
             re.finditer(r"prefetch: per batch ([\d.]+) ms waiting for the loader, ([\d.]+) ms staging \(incl. the copies\), ([\d.]+) ms", r.stderr)]
    return {"frames_per_s_by_epoch": rates, "prefetch_ms_loader_stage_consumer_by_epoch": stage}


def bench_driver(utts, samples, epochs, rounds, t60, timeout):
    res = {"dynamic_mix": [], "reverberant": []}
    with tempfile.TemporaryDirectory() as root:
        _, single = write_corpora(root, utts, samples)
        conf = os.path.join(root, "conf")
        with open(conf, "w") as f:
            f.write("hidden_dim=896\nnum_layers=3\nnum_spk=2\n")
        for k in range(rounds):                      # alternating
            for name, arg in (("dynamic_mix", None), ("reverberant", t60)):
                res[name].append(run_driver(single, os.path.join(root, "exp_%s_%d" % (name, k)), conf, epochs, arg, utts, timeout))
                print("driver %s, round %d: %s" % (name, k, res[name][-1]["frames_per_s_by_epoch"]), file=sys.stderr, flush=True)
    for name in ("dynamic_mix", "reverberant"):
        warm = [v for run in res[name] for v in run["frames_per_s_by_epoch"][1:]]          # the first epoch starts the workers
        res[name + "_summary"] = {"median_frames_per_s": float(np.median(warm)), "min": min(warm), "max": max(warm), "epochs": len(warm)}
    res["reverberant_over_dynamic_mix"] = round(res["reverberant_summary"]["median_frames_per_s"] / res["dynamic_mix_summary"]["median_frames_per_s"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-driver", action="store_true")
    ap.add_argument("--utts", type=int, default=512, help="source pairs of the synthetic corpus = mixtures per epoch of both arms")
    ap.add_argument("--samples", type=int, default=40000, help="samples of every file of the corpus")
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--t60", default="0.2,0.6", help="--mix-rir-synth of the reverberant arm")
    ap.add_argument("--run-timeout", type=int, default=240, help="seconds a driver run may take")
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"kernel": bench_kernel(dev, a.reps)}
    if not a.skip_driver:
        res["driver_3x896_b32_wav_input_dynamic_mix"] = bench_driver(a.utts, a.samples, a.epochs, a.rounds, a.t60, a.run_timeout)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
