#!/usr/bin/env python3
"""Timings of the inter-channel phase front end (profiles/ipd.txt): everything in one process on one device, HIP events around
synchronised work, warmed up, variants alternating.  The batch is 32 utterances of 400 frames (51100 int16 samples), C = 2, 4
and 8 microphones (P = C - 1 listed channels against microphone 0).

  fused     sk_stft_ipd: one launch from the PCM to the packed rows (+ the contiguous mixture rows); time per launch by the ops'
            own events, algorithmic bytes (C x 128 samples in, 257 (1 + 2P) + 257 floats out per frame) and the fraction of 8 TB/s
  unfused   the same rows on the kernels that were there before plus sk_ipd_rows: C sk_stft launches (complex) into a
            (C, T, B, 257) grid, one more for the reference's magnitudes, sk_ipd_rows over the grid's T x B rows.  A batch of
            equal lengths needs no pack: the grid's rows ARE the packed rows (a ragged batch adds an sk_pack_rows pass over the
            wide rows).  Per kernel class by the ops' events, and the whole route by wall events, alternating with the fused one
  step      the 3 x 896, 32 x 400 --wav-input training step (loss=mse) of an IPD model at in_dim 771 (ipd_channels=1) beside the
            mono model's on the reference channel of the same PCM, alternating, median of --steps each, with each arm's spread

    python tools/ipd_bench.py [--reps 30] [--steps 10] [--skip-step] [--out profiles/ipd_bench.json]
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

from sepkern import ipd, ops  # noqa: E402
from sepkern.packing import Packing  # noqa: E402

HBM_GBS = 8000.0
B, NSAMP, F = 32, 51100, 257


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
    """{class: (us per call of fn, algorithmic bytes per call)} of fn(repeat=reps) by the ops' own events."""
    fn(2)
    torch.cuda.synchronize()
    ops.PROF = {}
    fn(reps)
    torch.cuda.synchronize()
    prof, ops.PROF = ops.prof_summary(), None
    return {cls: (1e3 * ms / reps, by / reps) for cls, (_, ms, by) in prof.items()}


def array_pcm(C, seed=0):
    """int16 (C, B * NSAMP): channel-major, the utterances of a channel back to back -- WavCollator's layout with 'mix' = channel 0."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(-8000, 8000, size=(C, B * NSAMP), dtype=np.int16))


def bench_front(dev, reps, rounds=5):
    out = {}
    ns = [NSAMP] * B
    pk = Packing([1 + n // 128 for n in ns], dev)
    T = pk.T
    for C in (2, 4, 8):
        P = C - 1
        flat = array_pcm(C).to(dev).view(-1)
        total = B * NSAMP
        offs = [[q * total + j * NSAMP for j in range(B)] for q in range(C)]
        res = profiled(lambda rep: ops.stft_ipd(flat, offs, ns, pk=pk, repeat=rep), reps)
        us, by = res["stft_ipd_kernel"]
        r = {"frames": pk.R, "in_dim": ipd.in_dim(P),
             "fused": {"us_per_launch": round(us, 1), "MB_algorithmic": round(by / 1e6, 2), "GBs_algorithmic": round(by / us / 1e3, 1),
                       "fraction_of_8TBs": round(by / us / 1e3 / HBM_GBS, 3)}}
        # the unfused route: (C, T, B, 257) complex grid, the reference's magnitude grid, sk_ipd_rows over the T x B rows
        grid = torch.zeros(C, T * B, F, dtype=torch.complex64, device=dev)
        mag = torch.zeros(T * B, F, device=dev)
        gargs = dict(lengths=ns, out_offs=[b * F for b in range(B)], stride_t=[B * F] * B, stride_f=[1] * B)

        def stfts(rep=1):
            for q in range(C):
                ops.stft_batch(flat[q * total:(q + 1) * total], want_complex=True, out=grid[q].view(-1), repeat=rep, **gargs)
            ops.stft_batch(flat[:total], out=mag.view(-1), repeat=rep, **gargs)

        def unfused(rep=1):
            stfts(rep)
            return ops.ipd_rows(grid, 0, list(range(1, C)), mag, repeat=rep)

        parts = profiled(unfused, reps)
        r["unfused"] = {cls: {"us_per_batch": round(v[0], 1), "MB_algorithmic": round(v[1] / 1e6, 2)} for cls, v in parts.items()}
        r["unfused"]["kernels_total_us"] = round(sum(v[0] for v in parts.values()), 1)
        rows_f, _ = ops.stft_ipd(flat, offs, ns, pk=pk)
        rows_u = unfused()
        r["same_bits"] = bool(torch.equal(rows_f[:pk.R].view(torch.int32), rows_u.view(torch.int32)))
        fused_ms, unfused_ms = [], []
        for _ in range(rounds):               # wall events around the whole route (allocations and launches included), alternating
            fused_ms.append(timed(lambda: ops.stft_ipd(flat, offs, ns, pk=pk), reps))
            unfused_ms.append(timed(unfused, reps))
        r["route_wall_us"] = {"fused": round(1e3 * float(np.median(fused_ms)), 1), "unfused": round(1e3 * float(np.median(unfused_ms)), 1),
                              "fused_spread": [round(1e3 * min(fused_ms), 1), round(1e3 * max(fused_ms), 1)],
                              "unfused_spread": [round(1e3 * min(unfused_ms), 1), round(1e3 * max(unfused_ms), 1)]}
        r["ratio_unfused_over_fused"] = round(float(np.median(unfused_ms)) / float(np.median(fused_ms)), 2)
        out["C=%d" % C] = r
    return out


def bench_step(dev, steps, warmup=3):
    import uPIT
    from sepkern.optim import ClipAdam
    x = array_pcm(4, seed=1)                      # 'mix', two "sources" and the listed channel: key-major, as WavCollator ships them
    lens = [NSAMP] * B
    batches = {"mono": {"pcm": {"flat": x[:3].reshape(-1).clone(), "keys": ["mix", "source1", "source2"], "lens": lens}},
               "ipd": {"pcm": {"flat": x.reshape(-1).clone(), "keys": ["mix", "source1", "source2", "chan1"], "lens": lens}}}
    models = {}
    for kind, conf in (("mono", {}), ("ipd", {"ipd_channels": "1"})):
        torch.manual_seed(0)
        m = uPIT.SepDNN(0, hidden_dim="896", num_layers="3", **conf)
        m.cuda()
        m.train()
        models[kind] = (m, ClipAdam(m, lr=1e-4, max_norm=0.25))

    def step(kind):
        m, opt = models[kind]
        loss, _ = uPIT.compute_loss(m, 0, batches[kind])
        loss.backward()
        opt.step()

    for kind in models:
        for _ in range(warmup):
            step(kind)
    ms = {k: [] for k in models}
    for _ in range(steps):                      # alternating
        for kind in models:
            ms[kind].append(timed(lambda: step(kind), 1))
    res = {k: {"in_dim": models[k][0].in_dim, "median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3),
               "max_ms": round(max(v), 3)} for k, v in ms.items()}
    res["ipd_minus_mono_ms"] = round(res["ipd"]["median_ms"] - res["mono"]["median_ms"], 3)
    res["frames"] = B * (1 + NSAMP // 128)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"front_end_b32_t400": bench_front(dev, a.reps)}
    if not a.skip_step:
        res["training_step_3x896_b32_t400_wav_input"] = bench_step(dev, a.steps)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
