#!/usr/bin/env python3
"""STFT feature extraction on the MI355X: drop-in for the reference's steps/extract_feats.py
(same positional arguments, options, input wav.scp/segments and output files).

  data-dir/wav.scp[.N]      `<id> <root>/mix/<id>.wav`; sources are found by globbing /mix/ -> /*/
  train: <feat-dir>/<id>.npz with mix, s1..sS = |STFT| float32 (257, T)
  test : <feat-dir>/<id>.npz with mix = complex64 STFT (257, T)
  data-dir/feats_<type>.scp[.N], data-dir/utt2num_spk[.N]

The reference calls librosa.load + librosa.stft per file on the CPU (steps/extract_feats.py:85-89,
104-105); here wav files are read as int16 PCM, batched, and transformed by sk_stft (PCM scaling,
reflect padding, periodic Hann, 512-point FFT and magnitude fused in one kernel) writing directly in
the on-disk (257, T) layout.  Only mono 16-bit PCM is supported.  A file at another rate than
--sample-rate is resampled to it on the GPU in front of the STFT (sk_resample: the band-limited sinc
interpolation librosa.load(sr=) delegates to resampy, sepkern/resample.py); files already at
--sample-rate (the reference's data is wav8k) go to the STFT as int16, untouched.

--psa-targets (train only): s1..sS hold the phase-sensitive targets |S_i| cos(theta_i - theta_mix) of sepkern/psa.py instead of
the magnitudes |S_i| (--psa-clamp: held to [0, |mix|]), made together with the mixture's magnitudes by one sk_stft_psa launch
per chunk; file names and keys stay, so the unchanged npz training path (loss=mse) then trains the phase-sensitive loss.

The stage is host-bound (the kernel transforms ~2 G frames/s; zlib compresses ~25 MB/s per core), so the host side is
organised around that: a chunk's wav files are read by a thread pool while the previous chunk is on the GPU, every
chunk crosses PCIe as ONE pinned copy each way, and np.savez_compressed (zlib releases the GIL) runs on --writers
threads while the next chunk is read and transformed.  Files, names and contents are the reference's.
"""
import argparse
import concurrent.futures
import glob
import os
import sys
import time

import numpy as np
import scipy.io.wavfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))


def get_args():
  parser = argparse.ArgumentParser(description="""Extracts and saves STFT-based features for source separation""")
  parser.add_argument("data_dir", metavar="data-dir", type=str, help="Data directory with wav.scp")
  parser.add_argument("data_type", metavar="data-type", type=str, choices=['train', 'test'],
                      help="""Dataset type. Train stores magnitude spectra for mixture and all sources.
                      Test stores just mix spectrum.""")
  parser.add_argument("feat_dir", metavar="feat-dir", type=str, help="Output directory for features")
  parser.add_argument("--fft-dim", type=int, help="Dimension of FFT", default=512)
  parser.add_argument("--step-size", type=int, help="STFT step size", default=128)
  parser.add_argument("--sample-rate", type=int, help="Audio sample rate", default=8000)
  parser.add_argument("--batch-files", type=int, help="utterances per kernel launch", default=256)
  parser.add_argument("--writers", type=int, default=8, help="threads that read wav files and compress / write the npz files")
  parser.add_argument("--psa-targets", action='store_true', default=False,
                      help="train only: store the sources' phase-sensitive targets (sepkern/psa.py) as s1..sS instead of their magnitudes")
  parser.add_argument("--psa-clamp", action='store_true', default=False,
                      help="with --psa-targets: the truncated form, targets held to [0, |mix|]")
  return parser.parse_args()


def read_pcm(path, offset=None, duration=None):
  """-> (int16 samples at the file's own rate, that rate)."""
  fs, x = scipy.io.wavfile.read(path)
  if x.dtype != np.int16:
    raise ValueError("%s: only 16-bit PCM wav is supported, got %s" % (path, x.dtype))
  if x.ndim > 1:
    raise ValueError("%s: only mono wav is supported" % path)
  if offset is not None:       # librosa.load(offset=, duration=): whole frames from int(offset*sr), cut at the file's rate
    start = int(offset * fs)
    x = x[start:start + int(duration * fs)]
  return np.ascontiguousarray(x), int(fs)


def main():
  args = get_args()
  if args.fft_dim != 512 or args.step_size != 128:
    raise ValueError("the HIP STFT kernel is built for --fft-dim 512 --step-size 128")
  if args.psa_clamp and not args.psa_targets:
    raise ValueError("--psa-clamp goes with --psa-targets")
  if args.psa_targets and args.data_type != "train":
    raise ValueError("--psa-targets: only the train features hold sources")
  import torch
  from sepkern import ops
  from sepkern.data import host_threads
  host_threads()

  job_suffix = ''
  if os.environ.get("SGE_TASK_ID", 'undefined') != 'undefined':
    job_suffix = '.' + os.environ["SGE_TASK_ID"]

  os.makedirs(args.feat_dir, exist_ok=True)
  featF = open(args.data_dir + "/feats_" + args.data_type + ".scp" + job_suffix, 'w')
  utt2num_spkF = open(args.data_dir + "/utt2num_spk" + job_suffix, 'w')

  seg_dict = None
  if os.path.isfile(args.data_dir + "/segments" + job_suffix):
    seg_dict = {}
    for line in open(args.data_dir + "/segments" + job_suffix):
      seg = line.rstrip().split()
      seg_dict.setdefault(seg[1], []).append((seg[0], float(seg[2]), float(seg[3])))

  # work list: (output id, [(npz key, wav path, offset, duration)], num_spk)
  work = []
  with open(args.data_dir + "/wav.scp" + job_suffix, 'r') as listF:
    for line in listF:
      reco_id, filename = line.rstrip().split(' ')
      wav_files = sorted(glob.glob(filename.replace("/mix/", "/*/")))
      num_spk = max(1, len(wav_files) - 1)
      if args.data_type == "train":
        keyed = [('mix' if i == 0 else 's' + str(i), f) for i, f in enumerate(wav_files)]
      else:
        keyed = [('mix', filename)]
      segs = seg_dict[reco_id] if seg_dict is not None else [(reco_id, None, None)]
      for seg_id, t0, t1 in segs:
        dur = None if t0 is None else t1 - t0
        work.append((seg_id, [(k, f, t0, dur) for k, f in keyed], num_spk))

  want_complex = args.data_type == "test"
  step = max(1, args.batch_files)
  chunks = [work[i0:i0 + step] for i0 in range(0, len(work), step)]
  t_start, n_frames = time.perf_counter(), 0
  F = 257

  def read_chunk(chunk):
    return [[read_pcm(f, t0, dur) for _, f, t0, dur in items] for _, items, _ in chunk]

  def write_npz(seg_id, file_dict):
    np.savez_compressed(os.path.join(args.feat_dir, seg_id), **file_dict)

  def write_npz_rows(seg_id, rows_dict):       # --psa-targets: (T, 257) blocks as the kernel wrote them -> the on-disk (257, T)
    write_npz(seg_id, {key: np.ascontiguousarray(a.T) for key, a in rows_dict.items()})

  def psa_chunk(dev_in, ns, entries):
    """The chunk's files as {seg_id: {'mix': (T,257), 's1': ...}} host arrays: one sk_stft_psa launch per source count."""
    starts = np.concatenate([[0], np.cumsum(ns)])
    out, copies = {}, []
    for S in sorted(set(len(keyed) - 1 for _, _, keyed in entries)):
      group = [e for e in entries if len(e[2]) - 1 == S]
      lens = [ns[keyed[0][1]] for _, _, keyed in group]
      for (seg_id, _, keyed), n in zip(group, lens):
        if any(ns[k] != n for _, k in keyed):
          raise ValueError("%s: a source's length differs from its mixture's" % seg_id)
      Ts = [1 + n // 128 for n in lens]
      if S == 0:                               # a mixture without sources: its magnitudes only
        mags = torch.cat(ops.stft_batch([dev_in[starts[keyed[0][1]]:starts[keyed[0][1]] + n] for (_, _, keyed), n in zip(group, lens)]))
        planes = [mags]
      else:
        sig_offs = [[int(starts[keyed[q][1]]) for _, _, keyed in group] for q in range(S + 1)]
        mix, tg = ops.stft_psa(dev_in, sig_offs, lens, S, clamp=args.psa_clamp)
        planes = [mix] + tg
      host = [torch.empty(p.shape, dtype=p.dtype).pin_memory() for p in planes]
      for h, p in zip(host, planes):
        h.copy_(p, non_blocking=True)
      copies.append((group, Ts, host))
    torch.cuda.synchronize()
    for group, Ts, host in copies:
      at = 0
      for (seg_id, _, keyed), T in zip(group, Ts):
        out[seg_id] = {key: h.numpy()[at:at + T] for (key, _), h in zip(keyed, host)}
        at += T
    return out

  with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, args.writers)) as pool:
    def submit_read(chunk):      # a chunk's files, split over the pool's threads (file reads release the GIL)
      parts = [chunk[k::max(1, args.writers)] for k in range(max(1, args.writers))]
      return [(part, pool.submit(read_chunk, part)) for part in parts if part]
    reading = submit_read(chunks[0]) if chunks else []
    writing = []
    for ci, chunk in enumerate(chunks):
      loaded = [(part, fut.result()) for part, fut in reading]
      reading = submit_read(chunks[ci + 1]) if ci + 1 < len(chunks) else []
      entries, pcms = [], []        # (seg_id, num_spk, [(key, index into pcms)])
      for part, sigs in loaded:
        for (seg_id, items, num_spk), arrs in zip(part, sigs):
          entries.append((seg_id, num_spk, [(key, len(pcms) + k) for k, (key, _, _, _) in enumerate(items)]))
          pcms.extend(arrs)
      order = {e[0]: n for n, e in enumerate(chunk)}
      entries.sort(key=lambda e: order[e[0]])          # the scp lines keep the order of wav.scp
      rates = [fs for _, fs in pcms]
      pcms = [x for x, _ in pcms]
      ns = [len(x) for x in pcms]
      host_in = torch.from_numpy(np.concatenate(pcms)).pin_memory()
      dev_in = host_in.to("cuda", non_blocking=True)                       # the chunk's samples: one copy
      if any(fs != args.sample_rate for fs in rates):                      # resampled on the device, grouped by rate; float32 from here
        dev_in, ns = ops.pcm_to_rate(dev_in, ns, rates, args.sample_rate)
      Ts = [1 + n // 128 for n in ns]                                      # (frame counts of the signals the STFT sees)
      if args.psa_targets:
        rows = psa_chunk(dev_in, ns, entries)
        for seg_id, num_spk, keyed in entries:
          writing.append(pool.submit(write_npz_rows, seg_id, rows[seg_id]))
          featF.write(seg_id + ' ' + os.path.join(args.feat_dir, seg_id) + '.npz\n')
          utt2num_spkF.write(seg_id + ' ' + str(num_spk) + '\n')
          n_frames += Ts[keyed[0][1]]
        writing = [w for w in writing if not (w.done() and w.result() is None)]
        continue
      out_offs, acc = [], 0
      for T in Ts:
        out_offs.append(acc)
        acc += T * F
      dev_out = torch.empty(acc, dtype=torch.complex64 if want_complex else torch.float32, device="cuda")
      ops.stft_batch(dev_in, want_complex=want_complex, lengths=ns, out=dev_out, out_offs=out_offs,
                     stride_t=[1] * len(Ts), stride_f=list(Ts))            # the reference's on-disk (257, T) layout
      host_out = torch.empty(acc, dtype=dev_out.dtype).pin_memory()
      host_out.copy_(dev_out, non_blocking=True)                           # ... and the chunk's spectra: one copy back
      torch.cuda.synchronize()
      spectra = host_out.numpy()
      for seg_id, num_spk, keyed in entries:
        file_dict = {key: spectra[out_offs[k]:out_offs[k] + Ts[k] * F].reshape(F, Ts[k]) for key, k in keyed}
        writing.append(pool.submit(write_npz, seg_id, file_dict))
        featF.write(seg_id + ' ' + os.path.join(args.feat_dir, seg_id) + '.npz\n')
        utt2num_spkF.write(seg_id + ' ' + str(num_spk) + '\n')
        n_frames += Ts[keyed[0][1]]
      writing = [w for w in writing if not (w.done() and w.result() is None)]   # (re-raises a writer's exception)
    for w in writing:
      w.result()
  dt = time.perf_counter() - t_start
  print("extract_feats: %d utterances, %d mixture frames in %.2f s = %.0f frames/s" % (len(work), n_frames, dt, n_frames / max(dt, 1e-9)),
        file=sys.stderr)

  featF.close()
  utt2num_spkF.close()


if __name__ == '__main__':
  main()
