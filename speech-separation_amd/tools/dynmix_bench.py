#!/usr/bin/env python3
"""Timings of dynamic mixing (profiles/dynamic_mix.txt): everything in one call on one device, HIP events around synchronised
work, warmed up, the driver's two arms alternating.

  kernel    sk_dynamic_mix stand-alone on ragged batches of int16 sources of U(24 k, 64 k) samples: B = 32 with S = 2 and S = 3, and
            the reference's default batch B = 100 (S = 2); time per launch by the ops' own events, achieved GB/s and the fraction of
            8 TB/s in algorithmic bytes (every input sample once, every output sample once), with and without quantize
  driver    steps/train_qsub.py over a synthetic corpus (sepkern/synth.py), each run a fresh process: --wav-input on the
            pre-mixed files beside --wav-input --dynamic-mix on the same sources listed as single-speaker utterances, alternating,
            --rounds runs of each; frames/s of every epoch after the first and the SEPKERN_PREFETCH_TIMING=1 breakdown.  Every
            file holds --samples samples, so that both arms run steps of one shape: a dynamic mixture is as long as its shortest
            source, and with files of different lengths its batches would be shorter and more ragged than the pre-mixed ones --
            frames/s would then compare two length distributions, not two input paths

    python tools/dynmix_bench.py [--reps 50] [--skip-driver] [--utts 512] [--samples 40000] [--epochs 4] [--rounds 2] [--out profiles/dynmix_bench.json]
"""
import argparse
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
for p in (PKG, os.path.join(PKG, "archs")):
    if p not in sys.path:
        sys.path.insert(0, p)

from sepkern import ops, synth  # noqa: E402

HBM_GBS = 8000.0


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
    for B, S in ((32, 2), (32, 3), (100, 2)):
        rng = np.random.default_rng(B + S)
        lens = sorted((int(v) for v in rng.integers(24000, 64001, B)), reverse=True)
        sigs = synth.pcm_batch(B, num_spk=S, lengths=lens)
        flat = torch.from_numpy(np.concatenate([sig[1 + s] for s in range(S) for sig in sigs])).to(dev)
        total, starts = sum(lens), [sum(lens[:j]) for j in range(B)]
        offs = [[s * total + st for st in starts] for s in range(S)]
        amp = [[float(10.0 ** (v / 20.0)) for v in rng.uniform(-2.5, 2.5, B)] for _ in range(S)]
        buf = torch.empty((S + 1) * total, dtype=torch.float32, device=dev)
        r = {"samples_per_source": total, "longest": lens[0]}
        for name, q in (("plain", False), ("quantize", True)):
            us, by = profiled(lambda rep: ops.dynamic_mix(flat, offs, lens, amp, [0.9] * B, quantize=q, out=buf, repeat=rep),
                              reps)["dynamic_mix_kernel"]
            r[name] = {"us_per_launch": round(us, 1), "MB_algorithmic": round(by / 1e6, 2), "GBs_algorithmic": round(by / us / 1e3, 1),
                       "fraction_of_8TBs": round(by / us / 1e3 / HBM_GBS, 4)}
        out["B=%d S=%d" % (B, S)] = r
    return out


def write_corpora(root, utts, samples):
    """One synthetic wav tree, two data directories over it: `mixed` lists the pre-mixed files (WavTrainSet), `single` lists the
    same source files as single-speaker utterances with utt2spk (DynMixTrainSet)."""
    wavroot = os.path.join(root, "wav8k")
    ids = synth.write_wav_tree(wavroot, utts, num_spk=2, fixed_samples=samples)
    mixed, single = os.path.join(root, "data", "mixed"), os.path.join(root, "data", "single")
    synth.write_data_dir(mixed, wavroot, ids)
    os.makedirs(single, exist_ok=True)
    with open(os.path.join(single, "wav.scp"), "w") as scp, open(os.path.join(single, "utt2spk"), "w") as u2s:
        for k, i in enumerate(ids):
            for s in (1, 2):
                scp.write("%s_s%d %s/s%d/%s.wav\n" % (i, s, os.path.abspath(wavroot), s, i))
                u2s.write("%s_s%d spk%02d\n" % (i, s, (2 * k + s) % 40))          # 40 made-up speakers
    return mixed, single


def run_driver(data, out_dir, conf, epochs, dynamic, utts, timeout):
    cmd = [sys.executable, os.path.join(PKG, "steps", "train_qsub.py"), "uPIT", "0", data, out_dir, "--model-config", conf,
           "--wav-input", "--batch-size", "32", "--num-epochs", str(epochs), "--seed", "1"]
    if dynamic:
        cmd += ["--dynamic-mix", "--mixes-per-epoch", str(utts)]
    env = dict(os.environ, SEPKERN_PREFETCH_TIMING="1")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout, cwd=PKG)
    if r.returncode != 0:
        raise RuntimeError("train_qsub.py failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    rates = [float(m.group(1)) for m in re.finditer(r"= (\d+) frames/s", r.stderr)]
    stage = [tuple(float(v) for v in m.groups()) for m in
             re.finditer(r"prefetch: per batch ([\d.]+) ms waiting for the loader, ([\d.]+) ms staging \(incl. the copies\), ([\d.]+) ms", r.stderr)]
    return {"frames_per_s_by_epoch": rates, "prefetch_ms_loader_stage_consumer_by_epoch": stage}


def bench_driver(utts, samples, epochs, rounds, timeout):
    res = {"pre_mixed": [], "dynamic_mix": []}
    with tempfile.TemporaryDirectory() as root:
        mixed, single = write_corpora(root, utts, samples)
        conf = os.path.join(root, "conf")
        with open(conf, "w") as f:
            f.write("hidden_dim=896\nnum_layers=3\nnum_spk=2\n")
        for k in range(rounds):                      # alternating
            for name, data, dyn in (("pre_mixed", mixed, False), ("dynamic_mix", single, True)):
                res[name].append(run_driver(data, os.path.join(root, "exp_%s_%d" % (name, k)), conf, epochs, dyn, utts, timeout))
                print("driver %s, round %d: %s" % (name, k, res[name][-1]["frames_per_s_by_epoch"]), file=sys.stderr, flush=True)
    for name in ("pre_mixed", "dynamic_mix"):
        warm = [v for run in res[name] for v in run["frames_per_s_by_epoch"][1:]]          # the first epoch starts the workers
        res[name + "_summary"] = {"median_frames_per_s": float(np.median(warm)), "min": min(warm), "max": max(warm), "epochs": len(warm)}
    res["dynamic_over_pre_mixed"] = round(res["dynamic_mix_summary"]["median_frames_per_s"] / res["pre_mixed_summary"]["median_frames_per_s"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--skip-driver", action="store_true")
    ap.add_argument("--utts", type=int, default=512, help="utterances of the synthetic corpus = mixtures per epoch of both arms")
    ap.add_argument("--samples", type=int, default=40000, help="samples of every file of the corpus")
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--run-timeout", type=int, default=240, help="seconds a driver run may take")
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"kernel": bench_kernel(dev, a.reps)}
    if not a.skip_driver:
        res["driver_3x896_b32_wav_input"] = bench_driver(a.utts, a.samples, a.epochs, a.rounds, a.run_timeout)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
