#!/usr/bin/env python3
"""Timings of array dynamic mixing in simulated rooms (profiles/room_mix.txt): everything in one call on one device, HIP events
around synchronised work, warmed up, the driver's arms alternating.

  kernel    sk_room_rirs stand-alone: B = 32 mixtures x S = 2 sources x C in {1, 2, 4, 8} microphones (a ring of 5 cm radius),
            rooms drawn as DynMixTrainSet draws them (3 x 3 x 2.5 .. 8 x 6 x 4 m), nominal T60 in {0.2, 0.4, 0.6} s for every room
            of the batch (1 600 / 3 200 / 4 800 taps at 8 kHz); time per call by the ops' own events, the images of the batch
            (the sphere's volume over the room's: an estimate, beside the exact count of its first job) and images per second
  mixed     sepkern.data.mixed_pcm on one DynMixCollator batch of 32 mixtures of 40 000 samples: plain, --mix-rir-synth 0.2,0.6,
            rooms with one microphone, rooms with a 4-microphone array (three listed channels); wall time per call between
            synchronisations, the copy of the samples included
  driver    steps/train_qsub.py --wav-input --dynamic-mix over a synthetic corpus (sepkern/synth.py), each run a fresh process:
            plain, --mix-room-t60 LO,HI with the array given but a mono model, and the same with an IPD model (ipd_channels=1,2,3),
            alternating, --rounds runs of each; frames/s of every epoch after the first and the SEPKERN_PREFETCH_TIMING=1 breakdown

    python tools/room_bench.py [--reps 5] [--skip-driver] [--utts 512] [--samples 40000] [--epochs 3] [--rounds 2] [--t60 0.2,0.6] [--out FILE]
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
for p in (PKG, os.path.join(PKG, "archs"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from sepkern import ops, room  # noqa: E402
from dynmix_bench import profiled, write_corpora  # noqa: E402


def ring(C, radius=0.05):
    if C == 1:
        return np.zeros((1, 3))
    a = 2.0 * np.pi * np.arange(C) / C
    return np.stack([radius * np.cos(a), radius * np.sin(a), np.zeros(C)], axis=1)


def images_estimate(L, ntaps, rate=8000):
    """The sphere of radius c (ntaps + 32) / rate over the room's volume."""
    r = room.C_SOUND * (ntaps + 32.0) / rate
    return 4.0 / 3.0 * np.pi * r ** 3 / float(np.prod(L))


def bench_kernel(dev, reps):
    out, B, S = {}, 32, 2
    for C in (1, 2, 4, 8):
        for t60 in (0.2, 0.4, 0.6):
            rng = np.random.default_rng(7)
            ntaps = int(round(t60 * 8000))
            jobs = []
            for _ in range(B):
                r = room.draw_room(rng, (3, 3, 2.5), (8, 6, 4), (t60, t60), ring(C), S)
                jobs += [(r["L"], r["beta"], r["srcs"][s], r["mics"][c]) for s in range(S) for c in range(C)]
            args = ([j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs], [j[3] for j in jobs], [ntaps] * len(jobs), 8000)
            us, _ = profiled(lambda rep: ops.room_rirs(*args, device=dev, repeat=rep), reps)["room_rirs_kernel"]
            est = sum(images_estimate(j[0], ntaps) for j in jobs)
            out["C=%d t60=%.1f" % (C, t60)] = {
                "jobs": len(jobs), "taps": ntaps, "us_per_call": round(us, 1), "images_estimate": int(est),
                "images_of_job_0_exact_and_estimate": [room.count_images(*jobs[0], 8000, ntaps), int(images_estimate(jobs[0][0], ntaps))],
                "largest_job_images_estimate": int(max(images_estimate(j[0], ntaps) for j in jobs)),
                "Gimages_per_s": round(est / us / 1e3, 2)}
            print("kernel C=%d t60=%.1f: %s" % (C, t60, out["C=%d t60=%.1f" % (C, t60)]), file=sys.stderr, flush=True)
    return out


def bench_mixed(dev, reps, samples):
    import uPIT
    from sepkern.data import mixed_pcm
    out = {}
    with tempfile.TemporaryDirectory() as root:
        _, single = write_corpora(root, 64, samples)
        forms = {"plain": {}, "rir_synth_0.2_0.6": dict(rir_synth=(0.2, 0.6)), "room_0.2_0.6_mono": dict(room_t60=(0.2, 0.6)),
                 "room_0.2_0.6_4mics": dict(room_t60=(0.2, 0.6), array=ring(4), ipd_channels=(1, 2, 3)),
                 "room_0.2_0.2_4mics": dict(room_t60=(0.2, 0.2), array=ring(4), ipd_channels=(1, 2, 3))}
        for name, kw in forms.items():
            ds = uPIT.DynMixTrainSet(single, 2, seed=1, **kw)
            pcm = ds.collator([ds[i] for i in range(32)])["pcm"]
            pcm["flat"] = pcm["flat"].pin_memory()
            for _ in range(2):
                mixed_pcm(pcm, dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                mixed_pcm(pcm, dev)
            torch.cuda.synchronize()
            out[name] = {"ms_per_call": round(1e3 * (time.perf_counter() - t0) / reps, 3)}
            if "room" in pcm:
                out[name]["taps"] = [min(pcm["room"]["ntaps"]), max(pcm["room"]["ntaps"])]
                out[name]["images_estimate"] = int(sum(images_estimate(L, n) for L, n in zip(pcm["room"]["L"], pcm["room"]["ntaps"]))
                                                   * 2 * pcm["room"]["mics"].shape[1])
            print("mixed_pcm %s: %s" % (name, out[name]), file=sys.stderr, flush=True)
    return out


def run_driver(data, out_dir, conf, epochs, more, utts, timeout):
    cmd = [sys.executable, os.path.join(PKG, "steps", "train_qsub.py"), "uPIT", "0", data, out_dir, "--model-config", conf,
           "--wav-input", "--batch-size", "32", "--num-epochs", str(epochs), "--seed", "1", "--dynamic-mix", "--mixes-per-epoch", str(utts)]
    env = dict(os.environ, SEPKERN_PREFETCH_TIMING="1")
    r = subprocess.run(cmd + more, env=env, capture_output=True, text=True, timeout=timeout, cwd=PKG)
    if r.returncode != 0:
        raise RuntimeError("train_qsub.py failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    rates = [float(m.group(1)) for m in re.finditer(r"= (\d+) frames/s", r.stderr)]
    stage = [tuple(float(v) for v in m.groups()) for m in
             re.finditer(r"prefetch: per batch ([\d.]+) ms waiting for the loader, ([\d.]+) ms staging \(incl. the copies\), ([\d.]+) ms", r.stderr)]
    return {"frames_per_s_by_epoch": rates, "prefetch_ms_loader_stage_consumer_by_epoch": stage}


def bench_driver(utts, samples, epochs, rounds, t60, timeout):
    with tempfile.TemporaryDirectory() as root:
        _, single = write_corpora(root, utts, samples)
        mono, ipd, array = os.path.join(root, "conf"), os.path.join(root, "conf_ipd"), os.path.join(root, "array.txt")
        open(mono, "w").write("hidden_dim=896\nnum_layers=3\nnum_spk=2\n")
        open(ipd, "w").write("hidden_dim=896\nnum_layers=3\nnum_spk=2\nipd_channels=1,2,3\n")
        open(array, "w").write("".join("%.6f %.6f %.6f\n" % tuple(x) for x in ring(4)))
        arms = {"dynamic_mix": (mono, []), "rooms_mono_model": (mono, ["--mix-room-t60", t60, "--mix-array", array]),
                "rooms_ipd_model_4_mics": (ipd, ["--mix-room-t60", t60, "--mix-array", array])}
        res = {name: [] for name in arms}
        for k in range(rounds):                      # alternating
            for name, (conf, more) in arms.items():
                res[name].append(run_driver(single, os.path.join(root, "exp_%s_%d" % (name, k)), conf, epochs, more, utts, timeout))
                print("driver %s, round %d: %s" % (name, k, res[name][-1]), file=sys.stderr, flush=True)
    for name in list(arms):
        warm = [v for run in res[name] for v in run["frames_per_s_by_epoch"][1:]]          # the first epoch starts the workers
        res[name + "_summary"] = {"median_frames_per_s": float(np.median(warm)), "min": min(warm), "max": max(warm), "epochs": len(warm)}
    for name in list(arms)[1:]:
        res[name + "_over_dynamic_mix"] = round(res[name + "_summary"]["median_frames_per_s"] / res["dynamic_mix_summary"]["median_frames_per_s"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-mixed", action="store_true")
    ap.add_argument("--skip-driver", action="store_true")
    ap.add_argument("--utts", type=int, default=512, help="source pairs of the synthetic corpus = mixtures per epoch of every arm")
    ap.add_argument("--samples", type=int, default=40000, help="samples of every file of the corpus")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--t60", default="0.2,0.6", help="--mix-room-t60 of the room arms")
    ap.add_argument("--run-timeout", type=int, default=240, help="seconds a driver run may take")
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {}
    if not a.skip_kernel:
        res["kernel_B32_S2"] = bench_kernel(dev, a.reps)
    if not a.skip_mixed:
        res["mixed_pcm_B32_S2_%d_samples" % a.samples] = bench_mixed(dev, a.reps, a.samples)
    if not a.skip_driver:
        res["driver_3x896_b32_wav_input_dynamic_mix_t60_%s" % a.t60] = bench_driver(a.utts, a.samples, a.epochs, a.rounds, a.t60, a.run_timeout)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
