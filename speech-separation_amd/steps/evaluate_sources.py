#!/usr/bin/env python3
"""Scoring of reconstructed sources: the arguments, wav inputs and results/ files of the reference's
steps/evaluate_sources.py (:36-110), so that run_eval.sh:88-93 finds results/SDR_stats.txt and prints "mean SDR".

  results/{session,source}_{SDR,SIR,SAR}s.txt, results/{SDR,SIR,SAR}_stats.txt
      BSS Eval v3 SDR / SIR / SAR with the 512-tap allowed-distortion filter and the permutation search, as the
      reference gets them from mir_eval.separation.bss_eval_sources (steps/evaluate_sources.py:57); computed by
      sepkern/bsseval.py, a restatement of the published algorithm (mir_eval is not in this image).
  results/{session,source}_SISDRs.txt, {session,source}_SISDRis.txt, SISDR_stats.txt, SISDRi_stats.txt
      additionally: scale-invariant SDR (Le Roux et al. 2019) under its best permutation and its improvement over
      the unprocessed mixture -- the metric BASELINE.json's +-0.1 dB parity gate names.  Never mixed into the
      SDR files.
  results/{session,source}_{STOI,ESTOI}s.txt, results/{STOI,ESTOI}_stats.txt
      with --stoi: short-time objective intelligibility (Taal et al. 2011) and its extended form (Jensen & Taal 2016) under
      the assignment with the highest mean STOI (sepkern/stoi.py; with --gpu in the BSS Eval batches, sk_stoi).
Off the hot path: numpy on the host.  Reference and mixture wavs at another rate than the estimates' (--sample-rate) are
resampled to it first, on the GPU (sk_resample) -- the estimates were made from resampled mixtures.
"""
import argparse
import itertools
import os
import sys

import numpy as np
import scipy.io.wavfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))


def get_args(argv=None):
  parser = argparse.ArgumentParser(
    description="""This script computes BSS Eval SDR/SIR/SAR (and SI-SDR with its improvement over the mixture) for a
    set of estimated sources and ground truth sources.""")
  parser.add_argument("data_dir", metavar="data-dir", type=str, help="Test set data directory")
  parser.add_argument("exp_dir", metavar="exp-dir", type=str, help="Experiment directory")
  parser.add_argument("--gpu", action='store_true', default=False,
                      help="Score BSS Eval in batches on the GPU (sepkern/bsseval_gpu.py); SI-SDR stays on the host")
  parser.add_argument("--stoi", action='store_true', default=False,
                      help="Also write STOI and ESTOI (sepkern/stoi.py); with --gpu they are scored on the GPU in the same batches")
  parser.add_argument("--batch", type=int, default=256, help="Utterances per GPU batch (with --gpu)")
  parser.add_argument("--sample-rate", type=int, default=None,
                      help="Rate the estimates were written at (default: read from the first estimate's header); reference "
                           "and mixture wavs at another rate are resampled to it on the GPU before scoring (sk_resample)")
  return parser.parse_args(argv)


def read_pairs(path):
  """`<key> <value>` lines (wav.scp, utt2num_spk) in file order."""
  with open(path) as f:
    return [tuple(line.rstrip('\n').split(' ')[:2]) for line in f if line.strip()]


def load_wav(path, sample_rate=None):
  """A 16-bit wav as fp64 in [-1, 1).  With sample_rate, a file at another rate is resampled to it (on the GPU, sk_resample:
  the references the network was trained and run against, steps/extract_feats.py); the others are read as they always were."""
  fs, x = scipy.io.wavfile.read(path)
  if sample_rate is not None and fs != sample_rate:
    import torch
    from sepkern import ops
    if x.dtype != np.int16 or x.ndim != 1:
      raise ValueError("%s: only mono 16-bit PCM wav can be resampled" % path)
    y, _ = ops.resample_batch(torch.from_numpy(np.ascontiguousarray(x)).cuda(), [len(x)], fs, sample_rate)
    return y.cpu().numpy().astype(np.float64)
  return x.astype(np.float64) / 32768.0


def wav_rate(path):
  import wave
  with wave.open(path, "rb") as w:
    return w.getframerate()


class MetricFiles:
  """One metric's three files: session_<M>s.txt (`<id> <mean over sources>`), source_<M>s.txt (`<id> v1 v2 ...`)
  and <M>_stats.txt (Mean/Std/Max/Min over all sources of all utterances, tab-separated)."""

  def __init__(self, results_dir, metric):
    self.results_dir, self.metric, self.values = results_dir, metric, []
    self.session = open(os.path.join(results_dir, "session_%ss.txt" % metric), 'w')
    self.source = open(os.path.join(results_dir, "source_%ss.txt" % metric), 'w')

  def add(self, utt_id, per_source):
    per_source = [float(v) for v in per_source]
    self.session.write(utt_id + ' ' + str(sum(per_source) / len(per_source)) + '\n')
    self.source.write(utt_id + ''.join(' ' + str(v) for v in per_source) + '\n')
    self.values += per_source

  def close(self):
    self.session.close()
    self.source.close()
    v = np.array(self.values)
    with open(os.path.join(self.results_dir, "%s_stats.txt" % self.metric), 'w') as f:
      f.write("Mean:\t" + str(np.mean(v)) + '\n')
      f.write("Std:\t" + str(np.std(v)) + '\n')
      f.write("Max:\t" + str(np.amax(v)) + '\n')
      f.write("Min:\t" + str(np.amin(v)) + '\n')


def best_si_sdr(ests, refs):
  from sepkern.sisdr import si_sdr
  best = None
  for perm in itertools.permutations(range(len(refs))):
    v = [si_sdr(ests[perm[s]], refs[s]) for s in range(len(refs))]
    if best is None or sum(v) > sum(best):
      best = v
  return best


def main(argv=None):
  args = get_args(argv)
  from sepkern.bsseval import bss_eval_sources
  from sepkern.sisdr import si_sdr
  num_src = {k: int(v) for k, v in read_pairs(args.data_dir + "/utt2num_spk")}
  results = args.exp_dir + "/results"
  os.makedirs(results, exist_ok=True)
  out = {m: MetricFiles(results, m) for m in ("SDR", "SIR", "SAR", "SISDR", "SISDRi") + (("STOI", "ESTOI") if args.stoi else ())}
  rate = [args.sample_rate]                       # the estimates' rate: references and mixtures are brought to it

  def load(utt_id, mix_wav):
    S = num_src[utt_id]
    est_files = [args.exp_dir + "/wav/s" + str(s + 1) + "/" + utt_id + ".wav" for s in range(S)]
    if rate[0] is None:
      rate[0] = wav_rate(est_files[0])
    ests = [load_wav(f) for f in est_files]
    n = len(ests[0])                              # the first estimate sets the length (steps/evaluate_sources.py:51-55)
    ests = np.stack([e[:n] for e in ests])
    refs = np.stack([load_wav(mix_wav.replace("/mix/", "/s" + str(s + 1) + "/"), rate[0])[:n] for s in range(S)])
    return refs, ests, n

  def write(utt_id, mix_wav, refs, ests, n, sdr, sir, sar):
    out["SDR"].add(utt_id, sdr)
    out["SIR"].add(utt_id, sir)
    out["SAR"].add(utt_id, sar)
    si = best_si_sdr(ests, refs)
    mix = load_wav(mix_wav, rate[0])[:n]
    out["SISDR"].add(utt_id, si)
    out["SISDRi"].add(utt_id, [v - si_sdr(mix, refs[s]) for s, v in enumerate(si)])

  def write_stoi(utt_id, score):
    out["STOI"].add(utt_id, score[0])
    out["ESTOI"].add(utt_id, score[1])

  pairs = read_pairs(args.data_dir + "/wav.scp")
  if args.gpu:
    from sepkern.bsseval_gpu import bss_eval_sources_batch
    if args.batch < 1:
      raise ValueError("--batch must be >= 1")
    fallbacks = 0
    for b0 in range(0, len(pairs), args.batch):
      chunk = pairs[b0:b0 + args.batch]
      loaded = [load(utt_id, mix_wav) for utt_id, mix_wav in chunk]
      scores = bss_eval_sources_batch([l[0] for l in loaded], [l[1] for l in loaded])
      fallbacks += scores.n_fallback
      for (utt_id, mix_wav), (refs, ests, n), (sdr, sir, sar, _) in zip(chunk, loaded, scores):
        write(utt_id, mix_wav, refs, ests, n, sdr, sir, sar)
      if args.stoi:
        from sepkern.stoi_gpu import stoi_batch
        for (utt_id, _), score in zip(chunk, stoi_batch([l[0] for l in loaded], [l[1] for l in loaded], rate[0])):
          write_stoi(utt_id, score)
    if fallbacks:
      print("evaluate_sources.py: %d utterance(s) re-scored on the host (Gram matrix not factored on the GPU)" % fallbacks,
            file=sys.stderr)
  else:
    for utt_id, mix_wav in pairs:
      refs, ests, n = load(utt_id, mix_wav)
      sdr, sir, sar, _ = bss_eval_sources(refs, ests)
      write(utt_id, mix_wav, refs, ests, n, sdr, sir, sar)
      if args.stoi:
        from sepkern.stoi import stoi_sources
        write_stoi(utt_id, stoi_sources(refs, ests, rate[0]))
  for files in out.values():
    files.close()


if __name__ == '__main__':
  main()
