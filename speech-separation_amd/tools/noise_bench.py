#!/usr/bin/env python3
"""Timings of noisy dynamic mixing (profiles/noise_mix.txt): every arm of a comparison in one call on one device, HIP events
around synchronised work, warmed up, the driver's arms alternating.

  kernel    sk_noise_factors, sk_diffuse_noise and sk_add_noise stand-alone at B = 32 mixtures of U(24 k, 64 k) samples, int16 noise,
            C = 1 (add_noise only), 4 and 8 channels; time per call by the ops' own events
  mixed     sepkern.data.mixed_pcm on a DynMixCollator batch of B = 32, S = 2: plain without and with noise; a 4-microphone
            simulated room without and with noise; wall time per call around a synchronise, median of --reps
  driver    steps/train_qsub.py --wav-input --dynamic-mix over a synthetic corpus, each run a fresh process: plain, + noise,
            rooms with an array (IPD model), rooms + noise -- alternating, --rounds runs of each; frames/s of every epoch after the first
  bench     bench.py --gpus 1 --steps 20 --warmup 3 of this tree and of --parent (a built checkout of the parent commit),
            alternating, three runs each

    python tools/noise_bench.py [--reps 20] [--skip-driver] [--parent DIR] [--utts 256] [--epochs 3] [--rounds 2] [--out FILE]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
ROOT = os.path.dirname(PKG)
for p in (PKG, os.path.join(PKG, "archs"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from sepkern import ops, synth  # noqa: E402
from dynmix_bench import profiled, write_corpora  # noqa: E402


def line(C, d=0.04):
    return np.array([[d * i, 0.0, 0.0] for i in range(C)]) + np.array([2.0, 2.0, 1.5])


def bench_kernel(dev, reps):
    out = {}
    B = 32
    rng = np.random.default_rng(B)
    lens = sorted((int(v) for v in rng.integers(24000, 64001, B)), reverse=True)
    total, starts = sum(lens), [sum(lens[:j]) for j in range(B)]
    amp = [float(10.0 ** (-v / 20.0)) for v in rng.uniform(-3.0, 6.0, B)]
    for C in (1, 4, 8):
        crops = torch.from_numpy(np.clip(np.rint(rng.standard_normal(C * total) * 3000.0), -32768, 32767).astype(np.int16)).to(dev)
        sig = torch.from_numpy((rng.standard_normal(C * total) * 0.1).astype(np.float32)).to(dev)
        offs = [[c * total + st for st in starts] for c in range(C)]
        r = {"samples_per_channel": total, "longest": lens[0]}
        noise = crops
        if C > 1:
            mics = np.stack([line(C)] * B)
            r["noise_factors_us"] = round(profiled(lambda rep: ops.noise_factors(mics, 8000, device=dev, repeat=rep), reps)["noise_factors_kernel"][0], 1)
            L = ops.noise_factors(mics, 8000, device=dev)
            us, flops = profiled(lambda rep: ops.diffuse_noise(crops, offs, lens, L, repeat=rep), reps)["diffuse_noise_kernel"]
            r["diffuse_noise_us"], r["diffuse_noise_GFLOPs"] = round(us, 1), round(flops / us / 1e3, 1)
            noise = ops.diffuse_noise(crops, offs, lens, L)
        us, by = profiled(lambda rep: ops.add_noise(sig, offs, noise, offs, lens, amp, repeat=rep), reps)["add_noise_kernel"]
        r["add_noise_us"], r["add_noise_GBs"] = round(us, 1), round(by / us / 1e3, 1)
        out["B=%d C=%d" % (B, C)] = r
    return out


def bench_mixed(dev, reps):
    import uPIT
    from sepkern.data import mixed_pcm
    out = {}
    with tempfile.TemporaryDirectory() as root:
        _, single = write_corpora(root, 64, 48000)
        scp = os.path.join(root, "noise.scp")
        synth_noise(root, scp)
        array = line(4) - line(4).mean(axis=0)
        arms = {"plain": {}, "plain + noise": dict(noise_scp=scp),
                "room, 4 microphones": dict(room_t60=(0.2, 0.4), array=array, ipd_channels=(1, 2, 3)),
                "room, 4 microphones + noise": dict(room_t60=(0.2, 0.4), array=array, ipd_channels=(1, 2, 3), noise_scp=scp)}
        batches = {}
        for name, kw in arms.items():
            ds = uPIT.DynMixTrainSet(single, 2, seed=1, max_samples=48000, **kw)
            batches[name] = ds.collator([ds[i] for i in range(32)])["pcm"]
        times = {name: [] for name in arms}
        for k in range(reps + 2):                        # alternating; the first two rounds warm up
            for name, pcm in batches.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                mixed_pcm(pcm, dev)
                torch.cuda.synchronize()
                if k >= 2:
                    times[name].append(1e3 * (time.perf_counter() - t0))
        for name, t in times.items():
            out[name] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}
    return out


def synth_noise(root, scp, rate=8000, files=8, samples=160000):
    import scipy.io.wavfile
    rng = np.random.default_rng(7)
    with open(scp, "w") as f:
        for k in range(files):
            path = os.path.join(root, "noise%d.wav" % k)
            scipy.io.wavfile.write(path, rate, np.clip(np.rint(rng.standard_normal(samples) * 2000.0), -32768, 32767).astype(np.int16))
            f.write("noise%d %s\n" % (k, path))


def run_driver(data, out_dir, conf, epochs, extra, utts, timeout):
    cmd = [sys.executable, os.path.join(PKG, "steps", "train_qsub.py"), "uPIT", "0", data, out_dir, "--model-config", conf,
           "--wav-input", "--batch-size", "32", "--num-epochs", str(epochs), "--seed", "1", "--dynamic-mix", "--mixes-per-epoch", str(utts)] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=PKG)
    if r.returncode != 0:
        raise RuntimeError("train_qsub.py failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    return [float(m.group(1)) for m in re.finditer(r"= (\d+) frames/s", r.stderr)]


def bench_driver(utts, samples, epochs, rounds, timeout):
    res = {}
    with tempfile.TemporaryDirectory() as root:
        _, single = write_corpora(root, utts, samples)
        scp, array = os.path.join(root, "noise.scp"), os.path.join(root, "array.txt")
        synth_noise(root, scp)
        open(array, "w").write("".join("%g 0 0\n" % (0.04 * i) for i in range(4)))
        mono, ipd = os.path.join(root, "mono"), os.path.join(root, "ipd")
        open(mono, "w").write("hidden_dim=896\nnum_layers=3\nnum_spk=2\n")
        open(ipd, "w").write("hidden_dim=896\nnum_layers=3\nnum_spk=2\nipd_channels=1,2,3\n")
        rooms = ["--mix-room-t60", "0.2,0.4", "--mix-array", array]
        arms = [("dynamic_mix", mono, []), ("dynamic_mix + noise", mono, ["--mix-noise-scp", scp]),
                ("rooms, 4 microphones", ipd, rooms), ("rooms, 4 microphones + noise", ipd, rooms + ["--mix-noise-scp", scp])]
        runs = {name: [] for name, _, _ in arms}
        for k in range(rounds):                          # alternating
            for name, conf, extra in arms:
                runs[name].append(run_driver(single, os.path.join(root, "exp%d_%d" % (len(runs[name]), abs(hash(name)))), conf, epochs, extra, utts, timeout))
                print("driver %s, round %d: %s" % (name, k, runs[name][-1]), file=sys.stderr, flush=True)
        for name, rr in runs.items():
            warm = [v for run in rr for v in run[1:]]    # the first epoch starts the workers
            res[name] = {"frames_per_s_by_epoch": rr, "median": float(np.median(warm)), "min": min(warm), "max": max(warm), "epochs": len(warm)}
    return res


def bench_trees(parent, timeout):
    res = {"this": [], "parent": []}
    for k in range(3):                                   # alternating
        for name, tree in (("this", ROOT), ("parent", parent)):
            r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3"],
                               capture_output=True, text=True, timeout=timeout, cwd=tree)
            lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not lines:
                raise RuntimeError("bench.py of %s failed (%d): %s" % (tree, r.returncode, r.stderr[-2000:]))
            res[name].append(json.loads(lines[-1]))
            print("bench %s, run %d: %s" % (name, k, lines[-1][:200]), file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-driver", action="store_true")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py of both trees, alternating")
    ap.add_argument("--utts", type=int, default=256, help="source pairs of the synthetic corpus = mixtures per epoch of every arm")
    ap.add_argument("--samples", type=int, default=40000, help="samples of every file of the corpus")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--run-timeout", type=int, default=240, help="seconds a driver or bench.py run may take")
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"kernel": bench_kernel(dev, a.reps), "mixed_pcm_B32_S2": bench_mixed(dev, a.reps)}
    if not a.skip_driver:
        res["driver_3x896_b32"] = bench_driver(a.utts, a.samples, a.epochs, a.rounds, a.run_timeout)
    if a.parent:
        res["bench_py_steps20_warmup3"] = bench_trees(os.path.abspath(a.parent), a.run_timeout)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
