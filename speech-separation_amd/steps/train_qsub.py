#!/usr/bin/env python3
"""Training driver with the command line, file names and line formats of the reference's steps/train_qsub.py
(:17-53 arguments; :73-76,105,138,144,150,155 files: intermediate_models/{init,NNN}.mdl, final.mdl,
train_stats/{train,cv}_loss.txt with lines "EEE <loss>", train_stats/plots/...), so steps/qsub_train.sh can call
it unchanged.  The step itself is the arch module's: compute_loss -> backward -> clip 0.25 -> Adam
(steps/train_qsub.py:116-122); an epoch's loss is sum(loss * norm) / sum(norm) (:118-119,143); every 5th epoch
runs the cross-validation set and writes a checkpoint (:124-152).

What is organised differently here, on the host side only:
  * the per-batch loss bookkeeping stays on the GPU: one host sync per epoch instead of two per step;
  * clip + Adam run fused over the model's flat parameter buffer (sepkern.optim.ClipAdam; --torch-optimizer
    restores the reference's torch calls on the same parameters);
  * under torch.distributed.run (one process per GPU) it trains data-parallel: replicas are made identical by a
    broadcast from rank 0, every epoch's utterances are dealt to the ranks in length-balanced global batches
    (sepkern.dist.EpochShards: same step count on every rank), gradients are summed over RCCL inside backward,
    the ranks' BatchNorm running statistics are averaged after every epoch (sepkern.dist.average_bn_buffers: the CV
    loss printed is the loss of the model saved), the cross-validation set is sharded too, rank 0 writes the files;
  * checkpoints also carry the optimizer state (NNN.opt), which the reference loses on resume (:107);
  * a recurrence launch that timed out never reaches the weights (the fused optimizer skips that step on the
    device) and is reported when the epoch ends;
  * batches are staged on the GPU AHEAD of the step that consumes them (sepkern.data.Prefetcher: loader workers inflate
    and pack in parallel, a thread copies through pinned memory on its own stream, --prefetch batches deep): the
    reference inflates, packs and copies each batch synchronously in front of its step (:113-117), which at 36 ms per
    step is the bound.  --prefetch 0 --num-workers 1 is the reference's loop.  Every epoch's wall time and frames/s go
    to stderr;
  * --dynamic-mix (with --wav-input): the training mixtures are not files.  Every epoch draws them afresh from single-speaker
    utterances and mixes them on the GPU (archs/uPIT.py DynMixTrainSet, sepkern.dist.MixDraws, sk_dynamic_mix).  With
    --mix-rir-scp or --mix-rir-synth every source is first convolved with a room impulse response, also on the GPU
    (sk_fir_convolve, sepkern/reverb.py): the mixtures are reverberant and the targets are the reverberant sources;
  * conf key loss=mixit (with --wav-input): mixture-invariant training on recordings without isolated sources
    (sepkern/mixit.py).  With --dynamic-mix every example is a mixture of TWO recordings, whatever num_spk (the number of
    masks, 2..4) is; fixed files mix / source1 / source2 with mix = source1 + source2 work too (the validation pass).
"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.abspath(os.path.join(HERE, ".."))
for p in (PKG, os.path.join(PKG, "tools"), os.path.join(PKG, "archs"), 'tools', 'archs'):
  if p not in sys.path:
    sys.path.append(p)

import torch
from torch.utils.data import DataLoader, Subset

CHECKPOINT_EVERY = 5          # steps/train_qsub.py:124,148: epoch % 5 == 4
CLIP_NORM = 0.25              # steps/train_qsub.py:121


def get_args(argv=None):
  parser = argparse.ArgumentParser(description="""This script trains a separation neural network""")
  parser.add_argument("arch_file", metavar="arch-file", type=str, help="DNN architecture file")
  parser.add_argument("gpu_id", metavar="gpu-id", type=int, help="GPU ID")
  parser.add_argument("data_dir", metavar="data-dir", type=str, help="Training data directory")
  parser.add_argument("dirout", type=str, help="Output directory")
  parser.add_argument("--cv-data-dir", type=str, help="Cross validation data directory", default="")
  parser.add_argument("--train-copy-location", type=str, help="Copy training data here for I/O purposes", default="")
  parser.add_argument("--model-config", type=str, help="Config file for DNN", default="")
  parser.add_argument("--batch-size", type=int, help="Batch size (per GPU)", default=100)
  parser.add_argument("--start-epoch", type=int, help="Epoch to start from", default=0)
  parser.add_argument("--num-epochs", type=int, help="Total number of training epochs", default=200)
  parser.add_argument("--learning-rate", type=float, help="Learning rate", default=0.001)
  parser.add_argument("--torch-optimizer", action="store_true",
                      help="use torch clip_grad_norm_ + optim.Adam instead of the fused kernel")
  parser.add_argument("--num-workers", type=int, default=None,
                      help="loader processes (default: up to 12 for npz features -- zlib inflate of ~1 MB per utterance is the "
                           "loader's cost: 8 feed a 35 ms step, the 13 ms bf16 step wants more --, 4 with --wav-input (reading 96 small wav files "
                           "per batch: ~15 ms per worker); capped by "
                           "the CPUs this process may use)")
  parser.add_argument("--prefetch", type=int, default=2,
                      help="batches staged on the GPU ahead of the step (pinned memory, own copy stream); 0: off")
  parser.add_argument("--wav-input", action="store_true",
                      help="read <data-dir>/wav.scp and compute the STFT features on the GPU inside the step "
                           "(arch must provide WavTrainSet) instead of loading feats_train.scp npz files")
  parser.add_argument("--sample-rate", type=int, default=None,
                      help="with --wav-input: the rate the network works at; wav files at another rate are resampled to it on "
                           "the GPU (sk_resample), as the reference's librosa.load(sr=) does.  Default: the files are taken as they are")
  parser.add_argument("--dynamic-mix", action="store_true",
                      help="with --wav-input: <data-dir> lists single-speaker utterances (wav.scp + utt2spk) and every training "
                           "mixture is drawn afresh each epoch -- partners, levels, crops -- and mixed on the GPU (sk_dynamic_mix; "
                           "arch must provide DynMixTrainSet).  The validation set stays the fixed one of --cv-data-dir")
  parser.add_argument("--mixes-per-epoch", type=int, default=None, help="with --dynamic-mix: mixtures per epoch (default: utterances / num_spk; utterances / 2 with loss=mixit)")
  parser.add_argument("--mix-snr-db", type=float, default=2.5,
                      help="with --dynamic-mix: every source's level is uniform in +-this many dB (2.5: WSJ0-2mix's [-5, 5] dB between two speakers)")
  parser.add_argument("--mix-peak", type=mix_peak, default=(0.9, 0.9), metavar="LO[,HI]",
                      help="with --dynamic-mix: the largest magnitude of a mixture and its sources, uniform in [LO, HI]")
  parser.add_argument("--mix-max-samples", type=int, default=0, help="with --dynamic-mix: crop mixtures to this many samples (0: whole utterances)")
  parser.add_argument("--mix-quantize", action="store_true",
                      help="with --dynamic-mix: round the mixed signals to the int16 grid, as a 16-bit wav file of them would hold them")
  parser.add_argument("--mix-rir-scp", type=str, default=None, metavar="FILE",
                      help="with --dynamic-mix: lines of `<rir-id> <path>`: room impulse responses (mono 16-bit wav at the working rate "
                           "-- --sample-rate, or the corpus's --, or 1-D float npy); every source is convolved with one of them on the "
                           "GPU (sk_fir_convolve) before the mixture is made")
  parser.add_argument("--mix-rir-synth", type=rir_synth, default=None, metavar="LO,HI",
                      help="with --dynamic-mix: synthetic room impulse responses in place of --mix-rir-scp, T60 uniform in [LO, HI] seconds")
  parser.add_argument("--mix-rir-prob", type=float, default=None, metavar="P",
                      help="with --mix-rir-scp / --mix-rir-synth: the probability that a source is reverberant (default 1.0)")
  parser.add_argument("--mix-room-t60", type=rir_synth, default=None, metavar="LO,HI",
                      help="with --dynamic-mix: every mixture is made in a simulated shoebox room of its own (image method, sk_room_rirs), "
                           "nominal T60 uniform in [LO, HI] seconds; in place of --mix-rir-scp / --mix-rir-synth")
  parser.add_argument("--mix-array", type=str, default=None, metavar="FILE",
                      help="with --mix-room-t60: the microphone array, one line `x y z` (metres from its centre) per microphone, at most 8; "
                           "an IPD model trains on its channels ipd_ref / ipd_channels.  Default: one microphone")
  parser.add_argument("--mix-room-dims", type=room_dims, default=None, metavar="x,y,z:x,y,z",
                      help="with --mix-room-t60: the smallest and the largest room in metres (default 3,3,2.5:8,6,4)")
  parser.add_argument("--mix-noise-scp", type=str, default=None, metavar="FILE",
                      help="with --dynamic-mix: lines of `<noise-id> <path>`: noise recordings (mono 16-bit wav at the working rate); a "
                           "crop of one is added to every mixture on the GPU (sk_add_noise), and an array mixture gets a diffuse "
                           "field made of one crop per microphone (sk_diffuse_noise; sepkern/noise.py)")
  parser.add_argument("--mix-noise-snr", type=noise_snr, default=None, metavar="LO,HI",
                      help="with --mix-noise-scp: the ratio of the mixture to the noise on the reference channel, uniform in [LO, HI] dB "
                           "(default -3,6)")
  parser.add_argument("--seed", type=int, default=None, help="seed for weights, shuffling, mixture draws and h0/c0")
  args = parser.parse_args(argv)
  dynamic_mixing(args)
  return args


def mix_peak(text):
  """--mix-peak LO[,HI] -> (lo, hi)."""
  parts = [float(v) for v in text.split(',')]
  if len(parts) not in (1, 2):
    raise argparse.ArgumentTypeError("LO or LO,HI expected")
  return (parts[0], parts[-1])


def rir_synth(text):
  """--mix-rir-synth LO,HI -> (lo, hi) seconds of T60."""
  parts = [float(v) for v in text.split(',')]
  if len(parts) != 2 or not 0.0 < parts[0] <= parts[1]:
    raise argparse.ArgumentTypeError("LO,HI with 0 < LO <= HI expected")
  return (parts[0], parts[1])


def noise_snr(text):
  """--mix-noise-snr LO,HI -> (lo, hi) dB."""
  try:
    parts = [float(v) for v in text.split(',')]
  except ValueError:
    parts = []
  if len(parts) != 2 or not parts[0] <= parts[1]:
    raise argparse.ArgumentTypeError("LO,HI with LO <= HI expected")
  return (parts[0], parts[1])


def room_dims(text):
  """--mix-room-dims x,y,z:x,y,z -> ((x, y, z), (x, y, z)), the smallest and the largest room."""
  try:
    lo, hi = [tuple(float(v) for v in part.split(',')) for part in text.split(':')]
  except ValueError:
    raise argparse.ArgumentTypeError("x,y,z:x,y,z expected")
  if len(lo) != 3 or len(hi) != 3 or not all(0.0 < a <= b for a, b in zip(lo, hi)):
    raise argparse.ArgumentTypeError("x,y,z:x,y,z with 0 < smallest <= largest expected")
  return (lo, hi)


NEEDS_WAV_INPUT = "`--dynamic-mix` needs `--wav-input`: the mixtures are made from waveforms on the GPU"
NEEDS_DYNAMIC_MIX = "`%s` needs `--dynamic-mix`: room impulse responses are applied to the sources of mixtures made on the GPU"
ROOM_NEEDS_DYNAMIC_MIX = "`%s` needs `--dynamic-mix`: the rooms are simulated for mixtures made on the GPU"
ROOM_OR_RIRS = "`--mix-room-t60` simulates the rooms; `%s` is another source of room impulse responses: give one of them"
ARRAY_NEEDS_ROOM = "`%s` needs `--mix-room-t60`: an array stands in a simulated room"
ONE_RIR_SOURCE = "`--mix-rir-scp` and `--mix-rir-synth` are two sources of room impulse responses: give one of them"


def reverb_options(args):
  """The --mix-rir-* options that were given, as DynMixTrainSet's keyword arguments ({} without any)."""
  given = {"rir_scp": getattr(args, "mix_rir_scp", None), "rir_synth": getattr(args, "mix_rir_synth", None),
           "rir_prob": getattr(args, "mix_rir_prob", None)}
  return {k: v for k, v in given.items() if v is not None}


def room_options(args):
  """The simulated-room options that were given, as DynMixTrainSet's keyword arguments ({} without any); the array file is read
  here (sepkern/room.py read_array)."""
  given = {"room_t60": getattr(args, "mix_room_t60", None), "array": getattr(args, "mix_array", None),
           "room_dims": getattr(args, "mix_room_dims", None)}
  given = {k: v for k, v in given.items() if v is not None}
  if isinstance(given.get("array"), str):
    from sepkern.room import read_array
    try:
      given["array"] = read_array(given["array"]) if os.path.exists(given["array"]) else None
    except ValueError as e:
      raise SystemExit("--mix-array: %s" % e)
    if given["array"] is None:
      raise SystemExit("--mix-array: there is no file %s" % args.mix_array)
  return given


ROOM_FLAGS = {"room_t60": "--mix-room-t60", "array": "--mix-array", "room_dims": "--mix-room-dims"}
NOISE_FLAGS = {"noise_scp": "--mix-noise-scp", "noise_snr_db": "--mix-noise-snr"}
NOISE_NEEDS_DYNAMIC_MIX = "`%s` needs `--dynamic-mix`: the noise is added to mixtures made on the GPU"
NOISE_NOT_WITH_MIXIT = ("`--mix-noise-scp` does not go with loss=mixit: with noise on it the mixture is no longer the sum of its "
                        "two references, which is what the mixture-invariant loss assumes")


def noise_options(args):
  """The --mix-noise-* options that were given, as DynMixTrainSet's keyword arguments ({} without any)."""
  given = {"noise_scp": getattr(args, "mix_noise_scp", None), "noise_snr_db": getattr(args, "mix_noise_snr", None)}
  return {k: v for k, v in given.items() if v is not None}


def noisy_mixing(m, args):
  """True with --mix-noise-scp.  With loss=mixit the run ends here, not at its first batch; a list that cannot be read or holds a
  file at another rate ends it when the set is built (dynamic_mix_batches), before any file of the corpus is mixed."""
  if "noise_scp" not in noise_options(args):
    return False
  conf = read_model_conf(args.model_config)
  if hasattr(m, "parse_loss") and m.parse_loss(conf.get('loss', 'mse')) in getattr(m, "MIXIT_LOSSES", ()):
    raise SystemExit(NOISE_NOT_WITH_MIXIT)
  return True


def dynamic_mixing(args):
  """True with --dynamic-mix.  The mixtures are made from waveforms: without --wav-input the run ends here, not at its first batch;
  so does a run with a --mix-rir-*, --mix-room-* or --mix-noise-* option and no --dynamic-mix, with two sources of RIRs, with an
  array and no simulated room, or with a noise level and no noise."""
  rir = reverb_options(args)
  room = [k for k in ("room_t60", "array", "room_dims") if getattr(args, "mix_" + k, None) is not None]
  noise = noise_options(args)
  if noise and not getattr(args, "dynamic_mix", False):
    raise SystemExit(NOISE_NEEDS_DYNAMIC_MIX % NOISE_FLAGS[sorted(noise)[0]])
  if "noise_snr_db" in noise and "noise_scp" not in noise:
    raise SystemExit("`--mix-noise-snr` needs `--mix-noise-scp`: there is no noise to set the level of")
  if not getattr(args, "dynamic_mix", False):
    if rir:
      raise SystemExit(NEEDS_DYNAMIC_MIX % ("--mix-" + sorted(rir)[0].replace("_", "-")))
    if room:
      raise SystemExit(ROOM_NEEDS_DYNAMIC_MIX % ROOM_FLAGS[room[0]])
    return False
  if not args.wav_input:
    raise SystemExit(NEEDS_WAV_INPUT)
  if room and "room_t60" not in room:
    raise SystemExit(ARRAY_NEEDS_ROOM % ROOM_FLAGS[room[0]])
  if room and rir:
    raise SystemExit(ROOM_OR_RIRS % ("--mix-" + sorted(rir)[0].replace("_", "-")))
  if "rir_scp" in rir and "rir_synth" in rir:
    raise SystemExit(ONE_RIR_SOURCE)
  if "rir_prob" in rir and len(rir) == 1:
    raise SystemExit("`--mix-rir-prob` needs `--mix-rir-scp` or `--mix-rir-synth`: there is no room impulse response to apply")
  if "rir_prob" in rir and not 0.0 <= rir["rir_prob"] <= 1.0:
    raise SystemExit("`--mix-rir-prob` is a probability: 0 <= P <= 1")
  return True


# ----------------------------------------------------------------------------------------------- files
class RunDir:
  """The files of one training run (layout of the reference, steps/train_qsub.py:73-76)."""

  def __init__(self, dirout, writer):
    self.models = dirout + '/intermediate_models/'
    self.plots = dirout + '/train_stats/plots/'
    self.final = dirout + '/final.mdl'
    self.writer = writer                      # only rank 0 touches the disk
    self.logs = {"train": LossLog(dirout + '/train_stats/train_loss.txt'),
                 "cv": LossLog(dirout + '/train_stats/cv_loss.txt')}
    if writer:
      os.makedirs(self.models, exist_ok=True)
      os.makedirs(self.plots, exist_ok=True)

  def epoch_tag(self, epoch_number):
    return str(epoch_number).zfill(3)

  def model_file(self, epoch_number):
    return self.models + self.epoch_tag(epoch_number) + '.mdl'

  def optimizer_file(self, epoch_number):
    return self.models + self.epoch_tag(epoch_number) + '.opt'


class LossLog:
  """train_loss.txt / cv_loss.txt: one line "EEE <loss>" per epoch (steps/train_qsub.py:138,144); the history is
  kept as the [[epochs], [losses]] pair tools/plot.py:plot_loss takes."""

  def __init__(self, path):
    self.path, self.history, self.handle = path, [[], []], None

  def reload(self):
    with open(self.path) as f:
      for line in f:
        fields = line.split()
        if len(fields) >= 2:
          self.history[0].append(int(fields[0]))
          self.history[1].append(float(fields[1]))      # the reference's np.float (:60) is gone from numpy

  def record(self, epoch_number, value, write):
    self.history[0].append(epoch_number)
    self.history[1].append(value)
    if write:
      if self.handle is None:
        self.handle = open(self.path, 'a')
      self.handle.write(str(epoch_number).zfill(3) + ' ' + str(value) + '\n')
      self.handle.flush()


def read_model_conf(path):
  """key=value per line; values stay strings, as SepDNN(**kwargs) expects (steps/train_qsub.py:87-91)."""
  conf = {}
  if path:
    with open(path) as f:
      for line in f:
        if '=' in line:
          key, value = line.rstrip().split('=', 1)
          conf[key] = value
  return conf


def waveform_loss(m, args):
  """True when the conf file selects a loss that works on waveforms (archs/uPIT.py: loss=sisdr, loss=mixit).  Such a loss
  cannot be computed from npz magnitude features: without --wav-input the run ends here, not at its first batch."""
  if not hasattr(m, "parse_loss"):
    return False
  kind = m.parse_loss(read_model_conf(args.model_config).get('loss', 'mse'))
  wave = kind in getattr(m, "WAVE_LOSSES", ('sisdr',))
  if wave and not args.wav_input:
    raise SystemExit(m.needs_waveforms(kind))
  return wave


def mixed_recordings(m, args):
  """How many recordings --dynamic-mix draws per training example: num_spk from the model conf -- except with loss=mixit, whose
  example is always a mixture of TWO recordings (the references), whatever number of masks num_spk asks the network for.  The
  "speaker" of utt2spk is then whatever must not be mixed with itself: a session, a room, a channel."""
  conf = read_model_conf(args.model_config)
  if hasattr(m, "parse_loss") and m.parse_loss(conf.get('loss', 'mse')) in getattr(m, "MIXIT_LOSSES", ()):
    return 2
  return int(conf.get('num_spk', 2))


def prefetch_targets(m, args):
  """'psa' / 'tpsa' when the conf file selects a loss whose targets are made from the waveforms (archs/uPIT.py: the
  phase-sensitive losses) -- the prefetcher then stages those targets where it would stage the source magnitudes -- else None.
  Like a waveform loss it cannot be computed from npz magnitude features: without --wav-input the run ends here."""
  if not hasattr(m, "parse_loss"):
    return None
  kind = m.parse_loss(read_model_conf(args.model_config).get('loss', 'mse'))
  if kind not in getattr(m, "PSA_LOSSES", ()):
    return None
  if not args.wav_input:
    raise SystemExit(m.needs_waveforms(kind))
  return kind


IPD_WANTS_ROOMS = " -- unless they are made in simulated rooms: give `--mix-room-t60` and `--mix-array`"


def ipd_model(m, args):
  """{'ipd_ref': r, 'ipd_channels': (c, ...)} when the conf file makes it an IPD model (archs/uPIT.py conf key ipd_channels,
  sepkern/ipd.py: the network also sees the phase differences between the channels of an array), else {}.  Such a model trains
  on multi-channel wav files, or on mixtures made in simulated rooms (--dynamic-mix --mix-room-t60 --mix-array): without
  --wav-input, with --dynamic-mix alone (its mixtures have one channel), with an array that lacks one of the model's microphones
  or with loss=mixit the run ends here, not at its first batch."""
  if not hasattr(m, "ipd_conf"):
    return {}
  conf = read_model_conf(args.model_config)
  try:
    ref, chans = m.ipd_conf(conf, m.parse_loss(conf.get('loss', 'mse')))
  except ValueError as e:
    raise SystemExit(str(e))
  if not chans:
    return {}
  if not args.wav_input:
    raise SystemExit(m.IPD_NEEDS_WAVEFORMS)
  if getattr(args, "dynamic_mix", False):
    # only in simulated rooms with an array that has the model's microphones (--mix-room-t60 with --mix-array)
    if getattr(args, "mix_room_t60", None) is None or getattr(args, "mix_array", None) is None:
      raise SystemExit(m.IPD_NO_DYNAMIC_MIX + IPD_WANTS_ROOMS)
    have = len(room_options(args)["array"])
    if max(chans + (ref,)) >= have:
      raise SystemExit("`--mix-array` %s has %d microphone(s): ipd_ref = %d with ipd_channels = %s needs %d"
                       % (args.mix_array, have, ref, ",".join(str(c) for c in chans), max(chans + (ref,)) + 1))
  return {"ipd_ref": ref, "ipd_channels": chans}


# ----------------------------------------------------------------------------------------------- data
def wav_train_set(m, args, data_dir):
  """The arch's WavTrainSet over data_dir; --sample-rate and an IPD model's channels (ipd_model) are handed on only when given
  (an arch without the arguments keeps working).  A set whose files do not fit the model -- mono files for an IPD model, array
  files for any other -- is refused by the arch here, when it is built."""
  extra = dict(getattr(args, "ipd", None) or {})
  if getattr(args, "sample_rate", None) is not None:
    extra["sample_rate"] = args.sample_rate
  try:
    return m.WavTrainSet(data_dir, **extra)
  except ValueError as e:
    if not extra.get("ipd_channels") and "ipd_channels" not in str(e):
      raise
    raise SystemExit(str(e))


def mixing_seed(args, rank, world):
  """The seed of --dynamic-mix's draws: --seed, or one drawn here -- once, by rank 0, for every rank -- and printed, so that the
  run's mixtures can be had again."""
  if args.seed is not None:
    return args.seed
  box = [int.from_bytes(os.urandom(4), "little") & 0x7fffffff]
  if world > 1:
    torch.distributed.broadcast_object_list(box, src=0)
  if rank == 0:
    print("dynamic mixing: the mixtures are drawn with seed %d" % box[0], flush=True)
  return box[0]


def dynamic_mix_batches(m, args, rank, world):
  """--dynamic-mix: the arch's DynMixTrainSet over the single-speaker utterances of data_dir, num_spk from the model conf (two
  recordings with loss=mixit: mixed_recordings), and MixDraws, whose batches are a function of the epoch alone (reseed_epoch
  calls its set_epoch)."""
  from sepkern import dist as skdist
  if not hasattr(m, "DynMixTrainSet"):
    raise SystemExit("--dynamic-mix: the arch %s provides no DynMixTrainSet" % getattr(m, "__name__", m))
  seed = mixing_seed(args, rank, world)
  try:
    dataset = m.DynMixTrainSet(args.data_dir, mixed_recordings(m, args),
                               mixes_per_epoch=args.mixes_per_epoch, snr_db=args.mix_snr_db, peak=args.mix_peak,
                               max_samples=args.mix_max_samples, seed=seed, sample_rate=getattr(args, "sample_rate", None),
                               quantize=args.mix_quantize, **reverb_options(args),      # (an arch without RIRs is given none)
                               **room_options(args), **noise_options(args), **(getattr(args, "ipd", None) or {}))
  except ValueError as e:
    if "noise" not in str(e) or not noise_options(args):
      raise
    raise SystemExit("--mix-noise-scp: %s" % e)
  draws = skdist.MixDraws(dataset.mixes_per_epoch, args.batch_size, rank, world, seed=seed)
  workers = loader_workers(args, world)
  extra = dict(persistent_workers=True, prefetch_factor=2) if workers > 0 else {}
  loader = DataLoader(dataset, batch_sampler=draws, collate_fn=dataset.collator, num_workers=workers, **extra)
  return staged(loader, args), draws


def training_batches(m, args, rank, world):
  """DataLoader over this rank's share of the training set, and the sampler to re-seed per epoch (or None).
  One process: the reference's shuffled loader (steps/train_qsub.py:80-81).  Several: EpochShards.  --dynamic-mix: MixDraws."""
  from sepkern import dist as skdist
  if dynamic_mixing(args):
    return dynamic_mix_batches(m, args, rank, world)
  dataset = wav_train_set(m, args, args.data_dir) if args.wav_input else m.TrainSet(args.data_dir, args.train_copy_location)
  seed = args.seed if args.seed is not None else 0
  workers = loader_workers(args, world)
  extra = dict(persistent_workers=True, prefetch_factor=2) if workers > 0 else {}      # workers live across epochs
  if world == 1 and args.seed is None:           # the reference's shuffled loader, order from the global RNG
    loader = DataLoader(dataset, batch_size=args.batch_size, shuffle=True, collate_fn=dataset.collator,
                        num_workers=workers, **extra)
    return staged(loader, args), None
  # with --seed (or several ranks) the order of an epoch is a function of (seed, epoch) alone -- EpochShards, whatever the
  # loader draws from its generator for itself (a persistent-worker loader draws a base seed on its first epoch only), so
  # that `--start-epoch N` continues exactly where an uninterrupted run would be
  counts = dataset.frame_counts() if (world > 1 and hasattr(dataset, "frame_counts")) else None
  shards = skdist.EpochShards(len(dataset), args.batch_size, rank, world, lengths=counts, seed=seed)
  loader = DataLoader(dataset, batch_sampler=shards, collate_fn=dataset.collator, num_workers=workers, **extra)
  return staged(loader, args), shards


def loader_workers(args, world):
  if args.num_workers is not None:
    return max(0, args.num_workers)
  try:
    cpus = len(os.sched_getaffinity(0))
  except AttributeError:
    cpus = os.cpu_count() or 1
  return max(1, min(4 if args.wav_input else 12, cpus // max(1, world) - 3))


def staged(loader, args):
  """The loader's batches staged on the GPU ahead of their step (--prefetch N > 0), or the loader as it is."""
  if args.prefetch <= 0:
    return loader
  from sepkern.data import Prefetcher
  return Prefetcher(loader, torch.device("cuda", torch.cuda.current_device()), depth=args.prefetch,
                    keep_wave=getattr(args, "keep_wave", False), targets=getattr(args, "prefetch_targets", None))


def validation_batches(m, args, rank, world):
  from sepkern import dist as skdist
  if not args.cv_data_dir:
    return None
  dataset = wav_train_set(m, args, args.cv_data_dir) if args.wav_input else m.TrainSet(args.cv_data_dir)
  part = dataset if world == 1 else Subset(dataset, skdist.shard_indices_contiguous(len(dataset), rank, world))
  if len(part) == 0:
    return []                                    # more ranks than utterances: this rank only joins the final sum
  return DataLoader(part, batch_size=args.batch_size, collate_fn=dataset.collator)


# ----------------------------------------------------------------------------------------------- model
def build_model(m, args, gpu, rank):
  """SepDNN from the conf file on the GPU, identical on every rank, with its optimizer."""
  from sepkern import dist as skdist
  from sepkern.optim import ClipAdam
  if args.seed is not None:
    torch.manual_seed(args.seed)
  model = m.SepDNN(gpu, **read_model_conf(args.model_config))
  model.cuda()
  if hasattr(model, "flat_parameters"):
    model.flat_parameters()                      # bind the flat buffers before anything is broadcast or optimised
  skdist.broadcast_model(model)                  # whatever RNG state each rank had
  if args.seed is not None:
    model.hidden_generator = torch.Generator(device="cuda")
    model.hidden_generator.manual_seed(args.seed + 7919 * rank)       # per-rank h0/c0 stream
  if args.torch_optimizer:
    optimizer = torch.optim.Adam(model.parameters(), lr=args.learning_rate)
  else:
    optimizer = ClipAdam(model, lr=args.learning_rate, max_norm=CLIP_NORM)
  return model, optimizer


def reseed_epoch(args, rank, epoch, order, model):
  """With --seed, everything random in an epoch (utterance order, the per-batch h0/c0 of archs/uPIT.py:121-127) is a
  function of (seed, rank, epoch) alone, so `--start-epoch N` continues exactly where an uninterrupted run would be."""
  if hasattr(order, "set_epoch"):
    order.set_epoch(epoch)                       # sepkern.dist.EpochShards
  elif isinstance(order, torch.Generator):
    order.manual_seed(args.seed * 1000003 + epoch)
  if args.seed is not None and getattr(model, "hidden_generator", None) is not None:
    model.hidden_generator.manual_seed(args.seed * 1000003 + 7919 * rank + 104729 * (epoch + 1))


def resume(model, optimizer, run, args):
  model.load_state_dict(torch.load(run.model_file(args.start_epoch), map_location=lambda storage, loc: storage.cuda()))
  if os.path.isfile(run.optimizer_file(args.start_epoch)):
    optimizer.load_state_dict(torch.load(run.optimizer_file(args.start_epoch),
                                         map_location=lambda storage, loc: storage.cuda()))
  run.logs["train"].reload()
  if args.cv_data_dir:
    run.logs["cv"].reload()


# ----------------------------------------------------------------------------------------------- passes
POLL_EVERY = 50      # steps between two reads of the optimizer's skipped-step counter (one small host sync each)


def rank_of():
  return torch.distributed.get_rank() if (torch.distributed.is_available() and torch.distributed.is_initialized()) else 0


def recover_from_timeout(model, optimizer, newly_skipped, epoch):
  """A persistent recurrence launch timed out (its bounded wait gave up: the grid was not co-resident).  The device
  already kept that step away from the weights on EVERY rank (the guard word is all-reduced with the gradients, so the
  skipped count is the same everywhere; train_epoch reads it at the same steps on every rank, so all ranks take this branch
  together).  Clear the sticky word, continue IN
  THIS PROCESS with one launch per step (never re-exec a process that holds the GPU), and say so."""
  try:
    model.check_status()                 # reads and clears the workspace's sticky word
  except Exception as e:                 # SepkernError(SK_ETIMEOUT): expected here
    print("train: %s" % e, file=sys.stderr)
  eng = getattr(model, "_engine", None)
  if eng is None or eng.lstm_mode == 2:
    raise RuntimeError("the recurrence failed in per-step launch mode too (%d steps skipped in epoch %d)"
                       % (newly_skipped, epoch + 1))
  eng.lstm_mode = 2
  print("train: epoch %d: %d step(s) skipped after a timed-out persistent recurrence launch; their loss terms are dropped, "
        "continuing with one launch per step (SEPKERN_LSTM_MODE=2)" % (epoch + 1, newly_skipped), file=sys.stderr)
  sys.stderr.flush()


def train_epoch(m, model, optimizer, batches, epoch, world, torch_clip):
  """One pass over this rank's batches.  Returns the device tensor [sum(loss * norm), sum(norm)] of the GLOBAL
  epoch (all-reduced), still un-synchronised.  Every POLL_EVERY steps (and at the end) the fused optimizer's
  skipped-step counter is read: the loss terms of a window that contains a skipped step (garbage or NaN forwards) are
  dropped instead of poisoning the epoch's sums, and the run continues in per-step launch mode."""
  dev = next(model.parameters()).device
  # [sum(loss * norm), sum(norm), frames] of the steps that reached the weights; `win` = the same for the open window
  acc = torch.zeros(3, device=dev, dtype=torch.float64)
  win = torch.zeros(3, device=dev, dtype=torch.float64)
  fused = hasattr(optimizer, "skipped")
  seen = optimizer.skipped() if fused else 0

  def close_window():
    nonlocal seen, win
    if fused:
      now = optimizer.skipped()
      if now > seen:
        recover_from_timeout(model, optimizer, now - seen, epoch)
        seen = now
        win = torch.zeros_like(win)
        return
    acc.add_(win)
    win = torch.zeros_like(win)

  t_epoch = time.perf_counter()
  steps = 0
  for batch in batches:
    steps += 1
    loss, norm = m.compute_loss(model, epoch, batch)
    win[0] += loss.detach().double() * norm.double()
    # under data parallelism `norm` is already the global frame count: every rank adds its 1/world share
    win[1] += norm.double() / world
    # (an arch whose norm is not frames x feat_dim -- uPIT with loss=sisdr counts utterances -- says how many frames the step had)
    frames = getattr(model, "step_frames", None)
    win[2] += norm.double() / world if frames is None else float(frames) * float(getattr(model, "feat_dim", 257))
    loss.backward()
    if torch_clip:
      # torch's optimizer knows nothing of the guard word: look at it here (one host sync per step on this
      # compatibility path; it is all-reduced with the gradients, so every rank decides alike)
      eng = getattr(model, "_engine", None)
      if eng is not None and float(eng.guard.item()) != 0.0:
        recover_from_timeout(model, optimizer, 1, epoch)
        win = torch.zeros_like(win)
        continue
      torch.nn.utils.clip_grad_norm_(model.parameters(), CLIP_NORM)
    optimizer.step()
    # One process: the counter's asynchronous host copy, one step behind -- after a timed-out launch the run switches to
    # per-step launches within a step or two instead of skipping every step up to the next poll.  Several ranks: WHEN that
    # copy lands differs from rank to rank, so only the poll at a fixed step -- whose count is the same everywhere, the
    # guard word being all-reduced with the gradients -- may close a window: all ranks then drop the same steps' loss
    # terms and switch the recurrence mode at the same step.
    if steps % POLL_EVERY == 0 or (fused and world == 1 and optimizer.skipped_nowait() > seen):
      close_window()
  close_window()
  if world > 1:
    torch.distributed.all_reduce(acc)
  # wall time and frames/s of the epoch as the user sees it (data loading included): stderr, the reference's stdout
  # lines stay as they are.  norm = frames x feat_dim (archs/uPIT.py:197); frames of windows that were dropped after a
  # timed-out launch are not counted.  (One host sync per epoch, here.)  An epoch without a batch (an empty shard, a
  # resume on a tiny set) reports zero steps.
  n_frames = float(acc[2].item()) / float(getattr(model, "feat_dim", 257))
  dt = time.perf_counter() - t_epoch
  if rank_of() == 0:
    print("train: epoch %d: %d steps, %.0f frames in %.2f s = %.0f frames/s"
          % (epoch + 1, steps, n_frames, dt, n_frames / dt if dt > 0 else 0.0), file=sys.stderr, flush=True)
  return acc[:2]


def validation_pass(m, model, batches, epoch, world, plot_dir):
  """Eval-mode pass over this rank's shard of the CV set; no collective inside (the arch keeps its local norm
  when not training).  Returns the global [sum(loss * norm), sum(norm)].  The recurrence's sticky status word rides
  with the sums, so that a timed-out launch on one rank is raised by ALL ranks together (a raise on one rank alone
  would leave the others waiting in this all-reduce)."""
  acc = torch.zeros(3, device=next(model.parameters()).device, dtype=torch.float64)
  model.eval()
  with torch.no_grad():
    for i, batch in enumerate(batches):
      where = plot_dir if (i == 0 and plot_dir) else ""
      loss, norm = m.compute_cv_loss(model, epoch, batch, where) if where else m.compute_cv_loss(model, epoch, batch)
      acc[0] += loss.detach().double() * norm.double()
      acc[1] += norm.double()
  model.train()
  eng = getattr(model, "_engine", None)
  if eng is not None:
    acc[2] = (eng.sticky() != 0).double().sum()
  if world > 1:
    torch.distributed.all_reduce(acc)
  if float(acc[2]) != 0.0:
    try:
      model.check_status()               # clears this rank's word
    except Exception:
      pass
    raise RuntimeError("validation pass of epoch %d: a persistent recurrence launch timed out on %d rank(s)"
                       % (epoch + 1, int(acc[2])))
  return acc[:2]


def report_failures(model, optimizer, world):
  """Epoch boundary: surface a timed-out recurrence launch that train_epoch's recovery did not absorb (host sync).  The
  verdict is all-reduced first: every rank raises, or none does."""
  bad = 0
  if hasattr(optimizer, "skipped") and getattr(model, "_engine", None) is not None:
    bad = int(model._engine.sticky().item() != 0)
  if world > 1:
    t = torch.tensor([float(bad)], device=next(model.parameters()).device)
    torch.distributed.all_reduce(t)
    bad = int(t.item() != 0)
  if bad:
    try:
      model.check_status()
    except Exception:
      pass
    raise RuntimeError("a persistent recurrence launch timed out after the fallback to per-step launches")


def write_checkpoint(model, optimizer, run, epoch_number):
  torch.save(model.state_dict(), run.model_file(epoch_number))
  torch.save(optimizer.state_dict(), run.optimizer_file(epoch_number))
  draw_losses(run, run.plots + 'epoch' + run.epoch_tag(epoch_number) + '/', epoch_number)


def draw_losses(run, where, last_epoch_number):
  try:
    import plot
  except ImportError:
    return
  train, cv = run.logs["train"].history, run.logs["cv"].history
  if not train[0]:
    return
  os.makedirs(where, exist_ok=True)
  plot.plot_loss(train, cv, where + 'Loss_' + run.epoch_tag(train[0][0]) + '-' + run.epoch_tag(last_epoch_number) + '.png')


# ----------------------------------------------------------------------------------------------- main
def main(argv=None):
  args = get_args(argv)
  from sepkern import dist as skdist
  rank, world, local = skdist.init_from_env()
  gpu = local if world > 1 else args.gpu_id
  chief = rank == 0
  if chief:
    print("Using " + args.arch_file + " DNN architecture")
    print("Using GPU", gpu, "of", world)
  m = __import__(args.arch_file)
  args.keep_wave = waveform_loss(m, args)        # (the prefetcher then carries the waveforms with the staged batch)
  args.prefetch_targets = prefetch_targets(m, args)     # (... or stages phase-sensitive targets in place of the source magnitudes)
  args.ipd = ipd_model(m, args)                  # (an IPD model's channels: the loader ships them, the prefetcher stages the wide rows)
  noisy_mixing(m, args)                          # (--mix-noise-scp with loss=mixit ends the run here)
  torch.cuda.set_device(gpu)
  from sepkern.data import host_threads
  host_threads()                                 # (the arithmetic is on the GPU; see sepkern.data.host_threads)

  run = RunDir(args.dirout, chief)
  train_batches, shards = training_batches(m, args, rank, world)
  cv_batches = validation_batches(m, args, rank, world)
  model, optimizer = build_model(m, args, gpu, rank)
  if chief:
    print("using lr=" + str(args.learning_rate))

  if args.start_epoch == 0:
    if chief:
      torch.save(model.state_dict(), run.models + 'init.mdl')
  else:
    resume(model, optimizer, run, args)

  for epoch in range(args.start_epoch, args.num_epochs):
    number = epoch + 1
    reseed_epoch(args, rank, epoch, shards, model)
    acc = train_epoch(m, model, optimizer, train_batches, epoch, world, args.torch_optimizer)
    # one set of BatchNorm running statistics on every rank before anything is scored or saved (the reference has one
    # model: what scores the CV set is what the checkpoint holds, steps/train_qsub.py:124-152)
    skdist.average_bn_buffers(model)
    checkpoint = epoch % CHECKPOINT_EVERY == CHECKPOINT_EVERY - 1
    if cv_batches is not None and checkpoint:
      cv = validation_pass(m, model, cv_batches, epoch, world,
                           run.plots + 'epoch' + run.epoch_tag(number) if chief else "")
      cv_value = float(cv[0] / cv[1])
      if chief:
        print("For epoch: " + run.epoch_tag(number) + " cv set loss is: " + str(cv_value))
      run.logs["cv"].record(number, cv_value, chief)
    value = float(acc[0] / acc[1])                  # the epoch's one host sync
    report_failures(model, optimizer, world)
    if chief:
      print("For epoch: " + run.epoch_tag(number) + " loss is: " + str(value))
    run.logs["train"].record(number, value, chief)
    if checkpoint and chief:
      print("Saving model for epoch " + run.epoch_tag(number))
      write_checkpoint(model, optimizer, run, number)
    sys.stdout.flush()

  if chief:
    torch.save(model.state_dict(), run.final)
    draw_losses(run, run.plots, args.num_epochs)
  if world > 1:
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == '__main__':
  main()
