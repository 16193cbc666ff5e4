#!/usr/bin/env python3
"""Oracle-mask upper bound: counterpart of the reference's steps/evaluate_oracle.py (non-segment branch,
steps/evaluate_oracle.py:120-145; its segments branch does not run: `use_seg`/`rage`/`oracle_mask` NameErrors).

For every utterance of <data-dir>/wav.scp (wav files at another rate than --sample-rate are first resampled to it on the GPU,
sk_resample, as the reference's librosa.load(sr=) does): STFT of the mixture and of each source on the GPU (sk_stft), the
ideal ratio mask |S_i| / |M| (or the binary mask with --hard-mask, or with --psm the ideal phase-sensitive mask
clip(|S_i| cos(theta_i - theta_M) / |M|, 0, 1) of sepkern/psa.py, its numerator made by sk_stft_psa), mask-apply + iSTFT on the GPU
(sk_mask_istft), then the score: BSS Eval SDR / SIR / SAR without permutation search (the reference calls
mir_eval's bss_eval_sources with compute_permutation=False, steps/evaluate_oracle.py:118,143; here
sepkern/bsseval.py) into {session,source}_{SDR,SIR,SAR}s.txt + *_stats.txt under
<data-dir>/oracle_{soft,hard,psm}_mask_eval/, and SI-SDR under its own SISDR names.  With --stoi also STOI and ESTOI
(sepkern/stoi.py, without permutation search; with --gpu in the same batches, sk_stoi) under STOI / ESTOI names.
"""
import argparse
import glob
import os
import sys

import numpy as np
import scipy.io.wavfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))


def get_args(argv=None):
  parser = argparse.ArgumentParser(description="""Evaluates oracle (ideal) masks through the same STFT -> mask ->
  iSTFT path the separation models use""")
  parser.add_argument("data_dir", metavar="data-dir", type=str, help="Data directory with wav.scp")
  parser.add_argument("--hard-mask", action='store_true', help="Use hard mask", default=False)
  parser.add_argument("--psm", action='store_true', default=False,
                      help="Use the ideal phase-sensitive mask (the oracle of the loss=psa / tpsa targets)")
  parser.add_argument("--fft-dim", type=int, help="Dimension of FFT", default=512)
  parser.add_argument("--step-size", type=int, help="STFT step size", default=128)
  parser.add_argument("--sample-rate", type=int, help="Audio sample rate", default=8000)
  parser.add_argument("--gpu", action='store_true', default=False,
                      help="Score BSS Eval in batches on the GPU (sepkern/bsseval_gpu.py); SI-SDR stays on the host")
  parser.add_argument("--stoi", action='store_true', default=False,
                      help="Also write STOI and ESTOI (sepkern/stoi.py); with --gpu they are scored on the GPU in the same batches")
  parser.add_argument("--batch", type=int, default=256, help="Utterances per GPU batch (with --gpu)")
  return parser.parse_args(argv)


def main(argv=None):
  args = get_args(argv)
  if args.fft_dim != 512 or args.step_size != 128:
    raise ValueError("the HIP STFT kernels are built for --fft-dim 512 --step-size 128")
  if args.hard_mask and args.psm:
    raise ValueError("--hard-mask and --psm are two different oracles: give one of them")
  import torch
  from sepkern import ops
  from sepkern.bsseval import bss_eval_sources
  from sepkern.sisdr import si_sdr
  from evaluate_sources import MetricFiles
  dir_out = args.data_dir + ("/oracle_hard_mask_eval/" if args.hard_mask else "/oracle_psm_mask_eval/" if args.psm else "/oracle_soft_mask_eval/")
  os.makedirs(dir_out, exist_ok=True)
  out = {m: MetricFiles(dir_out, m) for m in ("SDR", "SIR", "SAR", "SISDR") + (("STOI", "ESTOI") if args.stoi else ())}
  pending = []                                    # --gpu: (id, device fp32 estimates, device references: int16 PCM, or float32 once resampled)

  def host_ref(t):
    """A device reference as fp64 on the host: int16 PCM scaled by 1/32768, resampled float32 as it is."""
    x = t.cpu().numpy().astype(np.float64)
    return x / 32768.0 if t.dtype == torch.int16 else x

  def write(reco_id, ests, refs, sdr, sir, sar, intel=None):
    if args.stoi:
      if intel is None:
        from sepkern.stoi import stoi_sources
        intel = stoi_sources(refs, ests, args.sample_rate, compute_permutation=False)
      out["STOI"].add(reco_id, intel[0])
      out["ESTOI"].add(reco_id, intel[1])
    out["SDR"].add(reco_id, sdr)
    out["SIR"].add(reco_id, sir)
    out["SAR"].add(reco_id, sar)
    out["SISDR"].add(reco_id, [si_sdr(ests[i], refs[i]) for i in range(len(refs))])

  def flush():
    if not pending:
      return
    from sepkern.bsseval_gpu import bss_eval_sources_batch
    ests = [torch.stack(e) for _, e, _ in pending]                       # fp32, resident on the device
    refs = [torch.stack([p[:e.shape[1]] for p in r]) for (_, _, r), e in zip(pending, ests)]   # int16 PCM (float32 once resampled)
    scores = bss_eval_sources_batch(refs, ests, compute_permutation=False)
    if scores.n_fallback:
      print("evaluate_oracle.py: %d utterance(s) re-scored on the host" % scores.n_fallback, file=sys.stderr)
    intel = [None] * len(pending)
    if args.stoi:
      from sepkern.stoi_gpu import stoi_batch
      intel = stoi_batch(refs, ests, args.sample_rate, compute_permutation=False)
    for (reco_id, _, _), e, r, (sdr, sir, sar, _), it in zip(pending, ests, refs, scores, intel):
      write(reco_id, e.cpu().numpy().astype(np.float64), host_ref(r), sdr, sir, sar, it)
    pending.clear()

  with open(args.data_dir + "/wav.scp", 'r') as listF:
    for line in listF:
      reco_id, filename = line.rstrip().split(' ')
      wav_files = sorted(glob.glob(filename.replace("/mix/", "/*/")))
      pcm, rates = [], []
      for f in wav_files:
        fs, x = scipy.io.wavfile.read(f)
        if x.dtype != np.int16 or x.ndim != 1:
          raise ValueError("%s: expected mono 16-bit PCM" % f)
        pcm.append(torch.from_numpy(np.ascontiguousarray(x)).cuda())
        rates.append(int(fs))
      if any(fs != args.sample_rate for fs in rates):
        # librosa.load(f, sr=args.sample_rate) (reference steps/evaluate_oracle.py:96,122): mixture and sources resampled on the
        # device (sk_resample); float32 signals from here on -- the resampled references are what the scores are taken against
        ns = [int(p.numel()) for p in pcm]
        flat, outs = ops.pcm_to_rate(torch.cat(pcm), ns, rates, args.sample_rate)
        pcm = list(torch.split(flat, outs))
      num_src = len(pcm) - 1
      mix_spec = ops.stft_batch([pcm[0]], want_complex=True, layout="FT")[0]           # (257, T) complex64
      if args.psm:
        n = int(pcm[0].numel())
        if num_src < 1 or any(int(p.numel()) != n for p in pcm):
          raise ValueError("%s: --psm needs sources of the mixture's length" % reco_id)
        # truncated targets clip(Re(S_i conj M) / |M|, 0, |M|) and |M| as (T, 257) blocks, one launch; the mask is their quotient
        mag, tg = ops.stft_psa(torch.cat(pcm), [[q * n] for q in range(num_src + 1)], [n], num_src, clamp=True)
        masks = (torch.stack(tg) / mag.clamp_min(1e-20)).transpose(1, 2)                # (S, 257, T)
      else:
        mags = torch.stack(ops.stft_batch(pcm[1:], want_complex=False, layout="FT"))      # (S, 257, T)
      if args.psm:
        pass
      elif args.hard_mask:
        masks = torch.nn.functional.one_hot(mags.argmax(0), num_src).permute(2, 0, 1).float()
      else:
        masks = mags / mix_spec.abs().clamp_min(1e-20)
      wav, _ = ops.mask_istft([mix_spec], [[masks[i].contiguous() for i in range(num_src)]], want_pcm=False)
      if args.gpu:
        pending.append((reco_id, [wav[0][i] for i in range(num_src)], pcm[1:]))
        if len(pending) >= args.batch:
          flush()
        continue
      ests = np.stack([wav[0][i].cpu().numpy().astype(np.float64) for i in range(num_src)])
      refs = np.stack([host_ref(pcm[i + 1])[:ests.shape[1]] for i in range(num_src)])
      sdr, sir, sar, _ = bss_eval_sources(refs, ests, compute_permutation=False)
      write(reco_id, ests, refs, sdr, sir, sar)
  flush()
  for files in out.values():
    files.close()


if __name__ == '__main__':
  main()
