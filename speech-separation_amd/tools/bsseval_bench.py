#!/usr/bin/env python3
"""Throughput of the batched BSS Eval kernels (csrc/bsseval.hip) against the host function (sepkern/bsseval.py).

For 2- and 3-speaker batches with lengths U(24k, 64k) samples at 512 taps:
  - utterances/s of the device-resident batch call (ops.bss_eval on packed fp64 rows);
  - ms and fp64 GFLOP/s per phase: correlations (sk_bss_xcorr alone) and factorisation + solves (the rest of
    sk_bss_eval: assembly, Cholesky with the forward substitution folded in, energies), from the FLOP counts below;
  - the host function's utterances/s on a few of the same utterances;
  - end to end, steps/evaluate_sources.py with and without --gpu on a sepkern/synth.py wav tree.
The fp64 rates are quoted against the 78.6 TFLOP/s spec (matrix and vector alike on this chip); the project has
not measured its fp64 MFMA rate.

usage: bsseval_bench.py [--utts 512] [--cpu-utts 4] [--cli-utts 48] [--reps 3]
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import scipy.io.wavfile
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "steps"))
from sepkern import bsseval, ops, synth  # noqa: E402
from sepkern.bsseval_gpu import pack  # noqa: E402

SPEC_TF = 78.6
TAPS = 512


def flops(S, L, lens):
    """(correlation, factorisation + solves) fp64 FLOPs of a batch."""
    lags = S * (S + 1) // 2 * L + S * (S - 1) // 2 * (L - 1) + S * S * L + S
    corr = sum(2.0 * n * lags for n in lens)
    N = S * L
    fact = N ** 3 / 3.0 + S * N ** 2 + (S - 1) * (L ** 3 / 3.0 + S * L ** 2)
    return corr, fact * len(lens)


def batch(S, U, rng):
    lens = rng.integers(24000, 64001, size=U).tolist()
    refs, ests = [], []
    for u, n in enumerate(lens):
        r = np.stack([synth.speech_like(n, 7919 * u + s) for s in range(S)])
        e = r + 0.2 * r[::-1] + 0.05 * rng.standard_normal(r.shape)
        refs.append(r)
        ests.append(e)
    return refs, ests, lens


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def device_leg(S, U, cpu_utts, reps, rng):
    refs, ests, lens = batch(S, U, rng)
    R = [torch.from_numpy(r).cuda() for r in refs]
    E = [torch.from_numpy(e).cuda() for e in ests]
    rcat, offs, _ = pack(R)
    ecat, _, _ = pack(E)
    ms_all = timed(lambda: ops.bss_eval(rcat, ecat, offs, lens, S, TAPS), reps)
    ms_corr = timed(lambda: ops.bss_xcorr(rcat, ecat, offs, lens, S, TAPS), reps)
    out, status = ops.bss_eval(rcat, ecat, offs, lens, S, TAPS)
    fails = int((status != 0).sum())
    fc, ff = flops(S, TAPS, lens)
    ms_fact = ms_all - ms_corr
    t0 = time.perf_counter()
    for u in range(cpu_utts):
        bsseval.bss_eval_sources(refs[u], ests[u])
    cpu_s = (time.perf_counter() - t0) / cpu_utts
    print("S=%d U=%d mean n=%.0f: batch %.1f ms = %.0f utt/s (status != 0: %d) | correlations %.1f ms, %.0f GFLOP/s "
          "(%.2f%% of %.1f TF) | factor+solve %.1f ms, %.0f GFLOP/s (%.2f%%) | host function %.3f s/utt = %.2f utt/s"
          % (S, U, np.mean(lens), ms_all, U / ms_all * 1e3, fails, ms_corr, fc / ms_corr / 1e6, fc / ms_corr / 1e6 / SPEC_TF / 10,
             SPEC_TF, ms_fact, ff / ms_fact / 1e6, ff / ms_fact / 1e6 / SPEC_TF / 10, cpu_s, 1.0 / cpu_s), flush=True)


def cli_leg(n_utts):
    import evaluate_sources
    root = tempfile.mkdtemp(prefix="bss_cli_")
    try:
        wav = os.path.join(root, "wav")
        ids = synth.write_wav_tree(wav, n_utts, num_spk=2, min_s=3.0, max_s=8.0, seed=1)
        data = os.path.join(root, "data")
        synth.write_data_dir(data, wav, ids)
        with open(os.path.join(data, "utt2num_spk"), "w") as f:
            f.write("".join("%s 2\n" % i for i in ids))
        rng = np.random.default_rng(2)
        exp = os.path.join(root, "exp")
        for i in ids:
            srcs = [scipy.io.wavfile.read(os.path.join(wav, "s%d" % (s + 1), i + ".wav"))[1].astype(np.float64) for s in range(2)]
            for s in range(2):
                os.makedirs(os.path.join(exp, "wav", "s%d" % (s + 1)), exist_ok=True)
                est = srcs[s] + 0.2 * srcs[1 - s] + 300.0 * rng.standard_normal(len(srcs[s]))
                scipy.io.wavfile.write(os.path.join(exp, "wav", "s%d" % (s + 1), i + ".wav"), 8000,
                                       np.clip(np.round(est), -32768, 32767).astype(np.int16))
        evaluate_sources.main([data, exp, "--gpu"])            # warm: library load, kernels, allocator
        t0 = time.perf_counter()
        evaluate_sources.main([data, exp, "--gpu"])
        t_gpu = time.perf_counter() - t0
        t0 = time.perf_counter()
        evaluate_sources.main([data, exp])
        t_cpu = time.perf_counter() - t0
        print("evaluate_sources.py on %d utterances: default %.2f s, --gpu %.2f s: %.1fx" % (n_utts, t_cpu, t_gpu, t_cpu / t_gpu),
              flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=512)
    ap.add_argument("--cpu-utts", type=int, default=4)
    ap.add_argument("--cli-utts", type=int, default=48)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    print("torch threads %d" % torch.get_num_threads(), flush=True)
    device_leg(2, a.utts, a.cpu_utts, a.reps, rng)
    device_leg(3, a.utts // 2, a.cpu_utts, a.reps, rng)
    if a.cli_utts:
        cli_leg(a.cli_utts)


if __name__ == "__main__":
    main()
