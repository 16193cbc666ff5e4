#!/usr/bin/env python3
"""Separate recordings of any length: wav in, wav out.  No counterpart in the reference, whose test stage runs whole
utterances through the network (steps/eval_qsub.py) and reads its masks back from npz files (steps/reconstruct_sources.py).

For every line `<ID> <path>` of wav-scp (mono 16-bit PCM wav at any rate): resample to --sample-rate, one STFT of the whole
recording, the network on overlapping windows of --window-frames every --hop-frames as uniform batches of --batch-windows,
the windows' output orders aligned and cross-faded (sk_stitch), mask-apply + iSTFT -> <out-dir>/s<k>/<ID>.wav (int16, at --sample-rate;
the int16 conversion is reconstruct_sources.py's).  Everything between the PCM going in and the PCM coming out runs on the GPU
(sepkern/separate.py).  The arch file is given by path, as to steps/eval_qsub.py; it must be the uPIT arch (fp32 or bf16
models) -- an arch module whose SepDNN has no forward_packed (the RSH arch) is refused.  One recording per sk_stitch call,
one GPU.

--mvdr admits microphone-array recordings: a multi-channel wav file per ID, or one wav.scp per channel with the same IDs
(--mvdr-channel-scps, the way the CHiME-5 and Mixer-6 arrays lie on disk; wav-scp is then channel 0).  The network runs on
--ref-channel; its stitched masks steer one MVDR beamformer per stream over all channels (sk_mvdr, sepkern/mvdr.py), and the
beamformed streams are written.  The channels of an ID must share one rate and are cut to the shortest.

--wpe dereverberates the spectra first (sk_wpe, sepkern/wpe.py: weighted prediction error over all channels), with or without
--mvdr and on mono files too; without --mvdr a multi-channel recording is dereverberated with all its channels and the masks
are applied to --ref-channel.

--cacgmm (with --mvdr, multi-channel recordings only) re-estimates the stitched masks from all channels before they steer the
beamformers (sk_cacgmm, sepkern/cacgmm.py: a cACGMM spatial mixture model with the network's masks as its class prior).

--wpd (instead of --mvdr, multi-channel recordings only) beamforms with one WPD convolutional beamformer per stream (sk_wpd,
sepkern/wpd.py: dereverberation, separation and denoising in one filter over the present frame and the channels' past).  With
--wpe the network still sees the dereverberated reference channel, and the WPD beamformers the recording as it is.

A model trained with the conf key ipd_channels (sepkern/ipd.py) sees the array itself: besides the magnitudes of its reference
channel ipd_ref, the phase differences of the listed channels against it (sk_ipd_rows; after --wpe those of the dereverberated
spectra).  It takes multi-channel recordings with or without a beamformer -- without one the masks are applied to the
reference channel --, --ref-channel must be its ipd_ref, and a recording must have every listed channel.
"""
import argparse
import concurrent.futures
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.abspath(os.path.join(HERE, ".."))
os.environ.setdefault("SEPKERN_HOME", PKG)      # a frozen arch.py finds the sepkern package through it
for p in (PKG, HERE):
  if p not in sys.path:
    sys.path.append(p)

NO_FORWARD_PACKED = "separate_wav: the arch module %s has no SepDNN.forward_packed; windowed separation runs the uPIT arch only"


def get_args(argv=None):
  parser = argparse.ArgumentParser(description="""This separates wav recordings of any length into wav files""")
  parser.add_argument("arch_file", metavar="arch-file", type=str, help="DNN architecture file (uPIT)")
  parser.add_argument("gpu_id", metavar="gpu-id", type=int, help="GPU ID")
  parser.add_argument("model", type=str, help="Trained model to use")
  parser.add_argument("wav_scp", metavar="wav-scp", type=str, help="lines of `<ID> <path to a mono 16-bit wav file>` (with --mvdr, --wpd or --wpe: any number of channels)")
  parser.add_argument("out_dir", metavar="out-dir", type=str, help="Output directory: <out-dir>/s<k>/<ID>.wav")
  parser.add_argument("--model-config", type=str, help="Config file for DNN", default="")
  parser.add_argument("--window-frames", type=int, default=400, help="window length in frames (the training chunk length)")
  parser.add_argument("--hop-frames", type=int, default=200, help="window hop in frames, in [window/2, window)")
  parser.add_argument("--batch-windows", type=int, default=32, help="windows per pass of the network")
  parser.add_argument("--sample-rate", type=int, default=8000, help="rate the network works at: files at another rate are resampled to it on the GPU, the output is written at it")
  parser.add_argument("--seed", type=int, default=None, help="seed for the random h0/c0 of every window (archs/uPIT.py:121-127)")
  parser.add_argument("--mvdr", action="store_true", help="beamform multi-channel recordings with the masks (2..8 channels)")
  parser.add_argument("--mvdr-channel-scps", type=str, default="", help="F1[,F2,...]: further wav.scp files with the same IDs, one per extra channel; wav-scp is then channel 0")
  parser.add_argument("--ref-channel", type=int, default=0, help="the channel the network sees and the beamformers keep undistorted")
  parser.add_argument("--mvdr-block-frames", type=int, default=200, help="frames per block of beamformer weights")
  parser.add_argument("--mvdr-context-blocks", type=int, default=1, help="blocks on either side whose statistics a block's weights use")
  parser.add_argument("--mvdr-loading", type=float, default=1e-3, help="diagonal loading of the noise matrix, relative to its mean diagonal")
  parser.add_argument("--mvdr-postmask", action="store_true", help="multiply the beamformed spectra by the masks")
  parser.add_argument("--wpe", action="store_true", help="dereverberate the spectra by weighted prediction error first (1..8 channels)")
  parser.add_argument("--wpe-taps", type=int, default=10, help="frames of every channel's past the prediction uses (channels * taps <= 80)")
  parser.add_argument("--wpe-delay", type=int, default=3, help="frames between the present and the newest frame the prediction uses")
  parser.add_argument("--wpe-iterations", type=int, default=3, help="re-estimations of the weights (1..8)")
  parser.add_argument("--wpe-block-frames", type=int, default=600, help="frames per block of prediction filters")
  parser.add_argument("--wpe-context-frames", type=int, default=0, help="frames on either side of a block its filters are estimated on as well")
  parser.add_argument("--wpe-loading", type=float, default=1e-3, help="diagonal loading of the covariance matrix, relative to its mean diagonal")
  parser.add_argument("--cacgmm", action="store_true", help="re-estimate the masks from all channels by a mask-guided cACGMM before they steer the beamformers (needs --mvdr or --wpd)")
  parser.add_argument("--cacgmm-iterations", type=int, default=5, help="EM iterations of the spatial model (0..16)")
  parser.add_argument("--cacgmm-block-frames", type=int, default=200, help="frames per block of the spatial model")
  parser.add_argument("--cacgmm-context-frames", type=int, default=200, help="frames on either side of a block its model is fitted on as well")
  parser.add_argument("--cacgmm-loading", type=float, default=1e-3, help="diagonal loading of the classes' matrices, relative to their mean diagonal")
  parser.add_argument("--wpd", action="store_true", help="beamform multi-channel recordings with one WPD convolutional beamformer per stream instead of --mvdr (2..8 channels)")
  parser.add_argument("--wpd-taps", type=int, default=5, help="frames of every channel's past the beamformers use besides the present one (channels * (taps + 1) <= 80)")
  parser.add_argument("--wpd-delay", type=int, default=3, help="frames between the present and the newest past frame the beamformers use")
  parser.add_argument("--wpd-iterations", type=int, default=2, help="re-estimations of the streams' powers (1..8)")
  parser.add_argument("--wpd-block-frames", type=int, default=600, help="frames per block of beamformer filters")
  parser.add_argument("--wpd-context-frames", type=int, default=0, help="frames on either side of a block its filters are estimated on as well")
  parser.add_argument("--wpd-loading", type=float, default=1e-3, help="diagonal loading of the covariance matrix, relative to its mean diagonal")
  parser.add_argument("--wpd-floor", type=float, default=1e-6, help="floor of a stream's power, relative to its largest in the window, in (0, 1]")
  parser.add_argument("--wpd-postmask", action="store_true", help="multiply the beamformed spectra by the masks")
  parser.add_argument("--writers", type=int, default=8, help="threads that read the wav inputs and write the wav outputs")
  return parser.parse_args(argv)


def main(argv=None):
  args = get_args(argv)
  if args.wpd and args.mvdr:
    print("separate_wav: --wpd takes the place of --mvdr; give one of them", file=sys.stderr)
    return 1
  if args.mvdr_channel_scps and not (args.mvdr or args.wpe or args.wpd):
    print("separate_wav: --mvdr-channel-scps needs --mvdr", file=sys.stderr)
    return 1
  if args.cacgmm and not (args.mvdr or args.wpd):
    print("separate_wav: --cacgmm needs --mvdr or --wpd", file=sys.stderr)
    return 1
  import eval_qsub
  m = eval_qsub.load_arch(args.arch_file)
  if not hasattr(getattr(m, "SepDNN", None), "forward_packed"):
    print(NO_FORWARD_PACKED % os.path.basename(args.arch_file), file=sys.stderr)
    return 1
  import numpy as np
  import scipy.io.wavfile
  import torch
  from sepkern import stitch as st
  from sepkern.data import host_threads
  from sepkern.separate import separate_recording
  try:
    st.check_geometry(1, args.window_frames, args.hop_frames)
  except ValueError as e:
    print("separate_wav: %s" % e, file=sys.stderr)
    return 1
  torch.cuda.set_device(args.gpu_id)
  host_threads()
  model = eval_qsub.restore_model(m, args, args.gpu_id)
  ipd = bool(getattr(model, "ipd_channels", ()))
  if ipd and args.ref_channel != model.ipd_ref:
    print("separate_wav: --ref-channel %d, but the model was trained with ipd_ref = %d: its masks belong to that channel"
          % (args.ref_channel, model.ipd_ref), file=sys.stderr)
    return 1

  def read_scp(scp):
    out = []
    with open(scp) as f:
      for line in f:
        if line.strip():
          ID, path = line.rstrip('\n').split(' ', 1)
          out.append((ID, path))
    return out

  entries = [(ID, [path]) for ID, path in read_scp(args.wav_scp)]
  for scp in [f for f in args.mvdr_channel_scps.split(',') if f]:
    more = dict(read_scp(scp))
    missing = [ID for ID, _ in entries if ID not in more]
    if missing:
      print("separate_wav: %s lacks %d of wav-scp's IDs (%s ...)" % (scp, len(missing), missing[0]), file=sys.stderr)
      return 1
    for ID, paths in entries:
      paths.append(more[ID])

  def load(paths):
    """-> (rate, pinned int16 samples: (n,) for a mono recording, (C, n) for an array)"""
    rates, chans = [], []
    for path in paths:
      fs, x = scipy.io.wavfile.read(path)
      if x.dtype.name != 'int16' or x.ndim > 2 or (x.ndim == 2 and not (args.mvdr or args.wpe or args.wpd or ipd)):
        raise ValueError("%s: only mono 16-bit PCM wav is supported" % path)
      rates.append(int(fs))
      chans += [x] if x.ndim == 1 else [x[:, c] for c in range(x.shape[1])]
    if len(set(rates)) != 1:
      raise ValueError("%s: the channels' files have different rates %s" % (paths[0], sorted(set(rates))))
    if len(chans) == 1:
      return rates[0], torch.from_numpy(chans[0]).pin_memory()
    n = min(len(c) for c in chans)
    return rates[0], torch.from_numpy(np.stack([c[:n] for c in chans])).pin_memory()

  def write_wav(path, samples):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    scipy.io.wavfile.write(path, args.sample_rate, samples)

  t_start, n_frames, n_samples = time.perf_counter(), 0, 0
  with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, args.writers)) as pool:
    loading = pool.submit(load, entries[0][1]) if entries else None
    writing = []
    for i, (ID, _) in enumerate(entries):
      rate, pcm = loading.result()
      loading = pool.submit(load, entries[i + 1][1]) if i + 1 < len(entries) else None      # read under this recording's GPU work
      _, pcm16 = separate_recording(model, pcm, rate, args.window_frames, args.hop_frames, args.batch_windows,
                                    working_rate=args.sample_rate, want_float=False, want_pcm=True, ref_channel=args.ref_channel,
                                    mvdr_block_frames=args.mvdr_block_frames, mvdr_context_blocks=args.mvdr_context_blocks,
                                    mvdr_loading=args.mvdr_loading, mvdr_postmask=args.mvdr_postmask, mvdr=args.mvdr or not (args.wpe or args.wpd or ipd),
                                    wpe=args.wpe, wpe_taps=args.wpe_taps, wpe_delay=args.wpe_delay, wpe_iterations=args.wpe_iterations,
                                    wpe_block_frames=args.wpe_block_frames, wpe_context_frames=args.wpe_context_frames,
                                    wpe_loading=args.wpe_loading, cacgmm=args.cacgmm, cacgmm_iterations=args.cacgmm_iterations,
                                    cacgmm_block_frames=args.cacgmm_block_frames, cacgmm_context_frames=args.cacgmm_context_frames,
                                    cacgmm_loading=args.cacgmm_loading, wpd=args.wpd, wpd_taps=args.wpd_taps, wpd_delay=args.wpd_delay,
                                    wpd_iterations=args.wpd_iterations, wpd_block_frames=args.wpd_block_frames,
                                    wpd_context_frames=args.wpd_context_frames, wpd_loading=args.wpd_loading,
                                    wpd_floor=args.wpd_floor, wpd_postmask=args.wpd_postmask)
      out_h = torch.empty(pcm16.shape, dtype=torch.int16).pin_memory()
      out_h.copy_(pcm16, non_blocking=True)
      torch.cuda.synchronize()
      samples = out_h.numpy()
      n_frames += 1 + samples.shape[1] // 128
      n_samples += samples.shape[1]
      for s in range(samples.shape[0]):
        writing.append(pool.submit(write_wav, os.path.join(args.out_dir, "s%d" % (s + 1), ID + ".wav"), samples[s]))
    for w in writing:
      w.result()                                # re-raise a writer's exception
  model.check_status()
  dt = max(time.perf_counter() - t_start, 1e-9)
  print("separate_wav: %d recordings, %d frames in %.2f s = %.0f frames/s, real-time factor %.5f"
        % (len(entries), n_frames, dt, n_frames / dt, dt / max(n_samples / float(args.sample_rate), 1e-9)), file=sys.stderr)
  return 0


if __name__ == '__main__':
  sys.exit(main())
