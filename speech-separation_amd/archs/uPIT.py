#!/usr/bin/env python3
"""uPIT arch plug-in, MI355X-native: drop-in for the reference's archs/uPIT.py.

Same module-level protocol (looked up by name from steps/train_qsub.py:66,80-95,117-135 and
steps/eval_qsub.py:43-72 of the reference):

    TrainSet(datadir, location="")   .collator      reads <datadir>/feats_train.scp
    TestSet(datadir)                 .collator      reads <datadir>/feats_test.scp
    SepDNN(gpuid, **kwargs)          nn.Module; kwargs are strings from the conf file
    compute_loss(model, epoch, batch_sample, plotdir="")     -> (loss/norm, norm) 0-dim tensors
    compute_cv_loss(model, epoch, batch_sample, plotdir="")  -> same
    compute_masks(model, batch_sample, out_dir)              -> writes <out_dir>/<id>.npz

All numerics run in libsepkern.so (hand-written gfx950 kernels, see include/sepkern.h) through
sepkern.engine; there is NO CPU path -- SepDNN(-1) or a missing library raises.

Beyond the reference (all optional, defaults reproduce it):
  * conf keys hidden_dim (600) and num_layers (2): the reference hard-codes 2x600
    (archs/uPIT.py:115-119); BASELINE's 2x300 / 3x896 configurations need them.
  * model.hidden_generator: a torch.Generator for the randn h0/c0 the reference draws per batch
    (archs/uPIT.py:121-127); tests inject (h0, c0) by assigning model.next_hidden.
  * under torch.distributed (one process per GPU) gradients are all-reduced over RCCL inside
    backward and the loss is normalised by the GLOBAL frame count.
  * conf key loss: 'mse' (default, the reference's magnitude PIT-MSE) or 'sisdr': utterance-level PIT on the negative
    SI-SDR of the time-domain estimates istft(mask_s * STFT(mix)) against the source waveforms (include/sepkern.h
    "SI-SDR uPIT loss").  It needs waveforms: WavTrainSet batches (steps/train_qsub.py --wav-input).  compute_loss then
    returns (mean negative SI-SDR per utterance in dB, number of utterances).
    'psa' / 'tpsa': the phase-sensitive approximation of the uPIT paper (sepkern/psa.py): the PIT-MSE above with the targets
    |S_s| cos(theta_s - theta_mix) in place of |S_s| ('tpsa': held to [0, |mix|]), made from the waveforms by one kernel
    (sk_stft_psa).  It needs waveforms too -- or npz features written by steps/extract_feats.py --psa-targets, which train
    with the default loss=mse.  compute_loss returns what it returns for 'mse'.
    'mixit': mixture-invariant training (Wisdom et al. 2020; sepkern/mixit.py, include/sepkern.h "mixture-invariant loss"):
    the batch's mixture is the sum of TWO recordings, 'source1' and 'source2', the network emits num_spk = M masks, 2..4, and
    the best of the 2^M assignments of the M time-domain estimates to the two recordings is scored (SNR with the soft
    threshold of conf key mixit_snr_max, default 30 dB).  No isolated sources are needed.  It needs waveforms;
    compute_loss returns (mean negative score per utterance in dB, number of utterances).
    'dpcl': deep clustering (Hershey et al. 2016; sepkern/dpcl.py, include/sepkern.h "deep clustering"): the same network
    with out_dim = feat_dim * embed_dim (conf key embed_dim, default 20, at most 40) emits an embedding per time-frequency
    point, the loss (sk_dpcl_fwd / sk_dpcl_bwd) pulls the embeddings of points dominated by the same source together -- weights
    dpcl_weight = mr (magnitude ratio, default) or vad (points above -dpcl_vad_db dB, default 40) -- and at inference k-means
    (sk_dpcl_kmeans, dpcl_kmeans_iters Lloyd steps, default 20) turns the embeddings into num_spk binary masks in the uPIT
    mask layout: compute_masks, steps/reconstruct_sources.py and sepkern.separate run unchanged.  It trains on whatever
    loss=mse trains on (magnitudes of the mixture and the sources).  compute_loss returns (mean loss per utterance, number
    of utterances).
  * DynMixTrainSet / DynMixCollator (steps/train_qsub.py --dynamic-mix): training mixtures drawn afresh every epoch from
    single-speaker utterances and mixed on the GPU (sk_dynamic_mix); every loss above trains on them.  With rir_scp / rir_synth
    (--mix-rir-scp / --mix-rir-synth) every source is first convolved with a room impulse response, also on the GPU
    (sk_fir_convolve; sepkern/reverb.py): reverberant mixtures, reverberant sources as targets.  With room_t60
    (--mix-room-t60 [--mix-array FILE]) every mixture is made in a simulated shoebox room of its own: image-method RIRs from every
    source to every microphone of the array, made on the GPU (sk_room_rirs; sepkern/room.py), and the listed channels' mixtures
    at the reference channel's gains (sk_mix_channels) -- an array batch for an IPD model, or one microphone for any other.
    With noise_scp (--mix-noise-scp [--mix-noise-snr]) a noise recording is added to every mixture at a drawn SNR (sk_add_noise),
    and to an array mixture a diffuse field with the microphones' coherence (sk_noise_factors, sk_diffuse_noise; sepkern/noise.py).
  * conf keys ipd_channels (e.g. 1,2,3) and ipd_ref (0): an IPD model (sepkern/ipd.py).  The network's input is the magnitude
    of channel ipd_ref of an array recording followed by cos and sin of the phase difference of every listed channel against
    it, in_dim = 257 (1 + 2P); feat_dim, out_dim and the losses mse / psa / tpsa / dpcl / sisdr are what they are without.
    It trains on WavTrainSet(ipd_ref=, ipd_channels=) batches of multi-channel wav files (steps/train_qsub.py --wav-input hands
    the conf keys on): the mixture's listed channels travel as 'chan<c>' behind 'mix' and 'source<N>', and one sk_stft_ipd
    launch makes the wide rows.  With --dynamic-mix it trains only in simulated rooms (--mix-room-t60 with --mix-array).  Not with
    loss=mixit or npz features; steps/separate_wav.py separates with it.
"""
import collections
import itertools
import os
import sys

import numpy as np
import torch
import torch.nn as nn
from torch.utils.data import Dataset
from torch.utils.data.dataloader import default_collate

try:
    import sepkern  # noqa: F401
except ImportError:  # the frozen copy exp/<...>/arch.py is imported from another directory
    for cand in (os.environ.get("SEPKERN_HOME"), "speech-separation_amd",
                 os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")):
        if cand and os.path.isdir(os.path.join(cand, "sepkern")):
            sys.path.insert(0, os.path.abspath(cand))
            break
    import sepkern  # noqa: F401
from sepkern import dist as skdist
from sepkern import dpcl as _dpcl
from sepkern import ipd as _ipd
from sepkern import ops
from sepkern.data import features_from_pcm as _features_from_pcm, wave_features_from_pcm as _wave_features_from_pcm
from sepkern.data import psa_features_from_pcm as _psa_features_from_pcm, ipd_rows_from_pcm as _ipd_rows_from_pcm
from sepkern.data import batch_chan_keys as _batch_chan_keys
from sepkern.collate import collate_sorted, eval_magnitudes, read_scp, stage_copies, train_sample
from sepkern.model import SepDNNBase, UnpackFn, to_packed as _to_packed
from sepkern.packing import Packing
from sepkern._lib import SepkernError


class Collator():
  """Same contract as the reference Collator (archs/uPIT.py:23-48): dict samples are sorted by the length of `sort_key`
  (descending, via argsort()[::-1]) and every ndarray entry becomes a float32 PackedSequence; everything else goes
  through default_collate (sepkern.collate)."""

  def __init__(self, sort_key):
    self.key = sort_key
    if not sort_key:       # (the text a user of the reference sees)
      print("Warning: you have not provided a sort key.")
      print("  If you are using RNNs with variable-length input, you must")
      print("  provide the key for element in each sample that is the input")
      print("  of variable length.")

  def __call__(self, batch):
    return collate_sorted(batch, self.key) if self.key else default_collate(batch)


class TrainSet(Dataset):
  """feats_train.scp -> {'mix': (T,F), 'source1': (T,F), ...} (reference archs/uPIT.py:51-79)."""

  def __init__(self, datadir, location=""):
    self.list = read_scp(datadir + "/feats_train.scp")
    if location:
      self.list = stage_copies(self.list, location)
    self.collator = Collator('mix')

  def __len__(self):
    return len(self.list)

  def frame_counts(self):
    """Frames per utterance, from the npz headers only (length-balanced sharding across GPUs)."""
    from sepkern.data import npz_frames
    return [npz_frames(path) for path in self.list]

  def __getitem__(self, idx):
    return train_sample(self.list[idx])


class TestSet(Dataset):
  """feats_test.scp -> {'mix': |complex STFT| (T,F), 'name': '<id>.npz'} (reference archs/uPIT.py:81-94)."""

  def __init__(self, datadir):
    self.list = read_scp(datadir + "/feats_test.scp")
    self.collator = Collator('mix')

  def __len__(self):
    return len(self.list)

  def __getitem__(self, idx):
    mags, name = eval_magnitudes(self.list[idx])
    return {'mix': mags, 'name': name}


class WavTrainSet(Dataset):
  """On-GPU input pipeline: reads <datadir>/wav.scp and yields the int16 PCM of the mixture
  and its sources (found like steps/extract_feats.py:65 does, by globbing /mix/ -> /*/); the STFT that stage 1
  of the recipe would have stored as npz is computed on the GPU inside compute_loss (sk_stft straight into the
  padded (T,B,F) batch).  12x less host I/O than float32 spectrograms and no zlib in the loader."""

  def __init__(self, datadir, location="", sample_rate=None, ipd_ref=0, ipd_channels=()):
    import glob
    self.items = []
    for line in open(datadir + "/wav.scp"):
      reco_id, filename = line.rstrip('\n').split(' ')
      self.items.append(sorted(glob.glob(filename.replace("/mix/", "/*/"))))
    # ipd_channels (the model's conf keys, sepkern/ipd.py): the mixtures are array recordings.  'mix' is then channel ipd_ref
    # of the mixture file, its listed channels follow as 'chan<c>', and a source file with several channels gives its channel
    # ipd_ref.  Without them every file is mono, as before.
    self.ipd_ref = _ipd.parse_ref(ipd_ref)
    self.ipd_channels = _ipd.parse_channels(ipd_channels, self.ipd_ref)
    if self.items and self.items[0]:
      self._check_channels(self.items[0][0])
    # sample_rate (steps/train_qsub.py --sample-rate): the rate the network works at.  None: the files' own rate is never
    # looked at (the recipe's data is wav8k).  With a rate, the loader still ships the int16 PCM as it is on disk -- at the
    # file's rate, which it records -- and the batch is resampled on the GPU in front of the STFT (sk_resample), as the
    # reference's librosa.load(path, sr=) does on the host.
    self.sample_rate = None if sample_rate is None else int(sample_rate)
    self.collator = WavCollator(self.sample_rate)

  def __len__(self):
    return len(self.items)

  def frame_counts(self):
    from sepkern.data import wav_frames
    return [wav_frames(files[0], sample_rate=self.sample_rate) for files in self.items]

  def _check_channels(self, mix_file):
    """The mixture file against the model, from its header: raised when the set is built, not at the first batch."""
    import wave
    try:
      with wave.open(mix_file, "rb") as w:
        have = w.getnchannels()
    except wave.Error:          # (not 16-bit PCM: __getitem__ says so)
      return
    if not self.ipd_channels:
      if have != 1:
        raise ValueError("%s has %d channels and the model sees one: list the channels whose phase differences it is to see "
                         "in the conf key ipd_channels (only mono 16-bit PCM wav is supported without)" % (mix_file, have))
      return
    need = max(self.ipd_channels + (self.ipd_ref,)) + 1
    if have < need:
      raise ValueError("%s has %d channel(s): ipd_ref = %d with ipd_channels = %s needs %d -- a mono batch cannot feed an IPD model"
                       % (mix_file, have, self.ipd_ref, ",".join(str(c) for c in self.ipd_channels), need))

  def _read_array(self, idx):
    """__getitem__ with ipd_channels: {'mix': channel ipd_ref, 'source<N>': channel ipd_ref of each source file (a mono file as
    it is), 'chan<c>': the mixture's listed channels, in their listed order}."""
    import scipy.io.wavfile
    out, rate, extra = {}, None, {}
    for i, f in enumerate(self.items[idx]):
      fs, x = scipy.io.wavfile.read(f)
      if x.dtype != np.int16 or x.ndim not in (1, 2):
        raise ValueError("%s: only 16-bit PCM wav is supported" % f)
      if self.sample_rate is not None and rate is not None and fs != rate:
        raise ValueError("%s is sampled at %d Hz, its mixture at %d: the sources of a mixture must share its rate" % (f, fs, rate))
      rate = fs
      if i == 0:
        self._check_channels(f)
        for c in self.ipd_channels:
          extra[_ipd.chan_key(c)] = np.ascontiguousarray(x[:, c])
      elif x.ndim == 2 and x.shape[1] <= self.ipd_ref:
        raise ValueError("%s has %d channels, ipd_ref = %d" % (f, x.shape[1], self.ipd_ref))
      out['mix' if i == 0 else 'source' + str(i)] = np.ascontiguousarray(x[:, self.ipd_ref]) if x.ndim == 2 else x
    if len(out) == 1:
      out['source1'] = out['mix']
    out.update(extra)
    if self.sample_rate is not None:
      out['rate'] = int(rate)
    return out

  def __getitem__(self, idx):
    import scipy.io.wavfile
    if self.ipd_channels:
      return self._read_array(idx)
    out, rate = {}, None
    for i, f in enumerate(self.items[idx]):
      fs, x = scipy.io.wavfile.read(f)
      if x.dtype != np.int16 or x.ndim != 1:
        raise ValueError("%s: only mono 16-bit PCM wav is supported" % f)
      if self.sample_rate is not None and rate is not None and fs != rate:
        raise ValueError("%s is sampled at %d Hz, its mixture at %d: the sources of a mixture must share its rate" % (f, fs, rate))
      rate = fs
      out['mix' if i == 0 else 'source' + str(i)] = x
    if len(out) == 1:
      out['source1'] = out['mix']
    if self.sample_rate is not None:
      out['rate'] = int(rate)
    return out


class WavCollator():
  """Sorts by frame count (descending, as Collator does) and hands the batch over as ONE int16 tensor: the signals of all
  utterances, key-major ('mix', 'source1', ...), longest utterance first -- {'pcm': {'flat', 'keys', 'lens'}}.  With
  sample_rate (WavTrainSet(sample_rate=...)) the samples say at which 'rate' they were recorded, the frame counts are those at
  sample_rate, and the batch also carries {'rate': [per utterance], 'target_rate': sample_rate}.  One tensor
  crosses from the loader's worker process to the trainer instead of 32 x (S + 1) (each of which costs a shared-memory
  hand-over: measured 15-18 ms per batch whatever the worker count, more than a 14 ms bf16 step).
  An array item (WavTrainSet with ipd_channels) carries the mixture's listed channels as 'chan<c>': they follow the sources in
  'keys' and in the flat tensor, in the item's order; a batch without them is the batch it was."""

  def __init__(self, sample_rate=None):
    self.sample_rate = None if sample_rate is None else int(sample_rate)

  def __call__(self, batch):
    if self.sample_rate is None:
      rates = None
      frames = [1 + len(d['mix']) // 128 for d in batch]
    else:        # every sample carries 'rate', the rate of its files: the order is that of the frame counts AFTER resampling
      from sepkern.resample import out_len
      if any('rate' not in d for d in batch):
        raise ValueError("WavCollator(sample_rate=%d): a sample does not say at which rate it was recorded ('rate')" % self.sample_rate)
      rates = [int(d['rate']) for d in batch]
      batch = [{k: v for k, v in d.items() if k != 'rate'} for d in batch]
      frames = [1 + out_len(len(d['mix']), r, self.sample_rate) // 128 for d, r in zip(batch, rates)]
    order = np.argsort(np.array(frames))[::-1]
    chans = _ipd.chan_keys(batch[0])       # an array item's listed channels ('chan<c>', WavTrainSet with ipd_channels), in its order
    others = [k for k in batch[0] if k != 'mix' and k not in chans]
    bad = [k for k in others if not (k.startswith('source') and k[6:].isdigit())]
    if bad:
      raise ValueError("WavCollator: signals besides 'mix' must be named 'source<N>' (got %r)" % bad)
    keys = ['mix'] + sorted(others, key=lambda k: int(k[6:])) + chans
    # ONE list of sample counts ('lens', the mixture's) describes every key of the flat tensor: a source whose length differs
    # from its mixture's by a single sample would shift every later signal -- wrong targets, no error -- so it is one here
    for d in batch:
      for k in keys:
        if k not in d or len(d[k]) != len(d['mix']):
          raise ValueError("WavCollator: signal %r of an utterance has %s samples, its mixture %d -- the sources of a mixture "
                           "must have the mixture's length" % (k, len(d[k]) if k in d else "no", len(d['mix'])))
    flat = np.concatenate([batch[i][k] for k in keys for i in order])
    pcm = {'flat': torch.from_numpy(flat), 'keys': keys, 'lens': [int(len(batch[i]['mix'])) for i in order]}
    if rates is not None:      # 'lens' stay the sample counts on disk; sepkern.data resamples when a rate differs from the target
      pcm['rate'] = [rates[i] for i in order]
      pcm['target_rate'] = self.sample_rate
    return {'pcm': pcm}


class DynMixTrainSet(Dataset):
  """Dynamic mixing (steps/train_qsub.py --dynamic-mix): every training mixture is drawn afresh, every epoch, from
  single-speaker utterances -- random partners, levels, crops and peak -- and MIXED ON THE GPU (sk_dynamic_mix; sepkern/mixing.py
  states the rule).  datadir is Kaldi-style: wav.scp (`<utt-id> <path>` of mono 16-bit wav files, one speaker each) and utt2spk
  (`<utt-id> <speaker>`).  The loader ships only the int16 slices of the S sources: S files are read per mixture, not S + 1, and
  no float arithmetic runs on the host.

  The dataset index encodes the epoch: idx = epoch * mixes_per_epoch + i (sepkern.dist.MixDraws hands those out), and item idx is
  a function of (seed, idx) ALONE -- a numpy Generator seeded with that pair draws num_spk distinct speakers and one utterance of
  each, the common length n = min(len_s) (at most max_samples when that is > 0), a uniform crop start in every longer source,
  snr_s ~ U(-snr_db, +snr_db) dB independently per source (2.5: the level difference of two speakers lies in [-5, 5] dB, WSJ0-2mix's
  range) and a peak uniform in [peak[0], peak[1]].  Persistent loader workers therefore never need to be told the epoch, and a
  restarted run draws what the uninterrupted one would have.
  -> {'source1': int16[n], ..., 'amp': [10^(snr_s / 20)], 'peak': p} (+ 'rate' with sample_rate: the files' rate; the batch is
  resampled on the GPU in front of the mixing, and lengths, max_samples and the 257-sample limit count at sample_rate).

  Reverberation (rir_scp or rir_synth; sepkern/reverb.py): every source is convolved ON THE GPU (sk_fir_convolve) with a room
  impulse response before the levels are set, so an item also carries 'rir1' .. 'rir<S>' (float32 taps) and 'rir_delay' (the
  index of each direct path: the reverberant source stays aligned with the dry one).  Each source independently, with
  probability rir_prob: a RIR drawn uniformly from rir_scp (lines `<rir-id> <path>` of mono 16-bit wav or 1-D float npy files at
  the working rate, read once, here), or synthesised with t60 ~ U(rir_synth) seconds and a direct-to-reverberant ratio ~
  U(rir_drr_db) dB; otherwise the identity [1.0].  These draws come from a generator of their own, seeded (seed, idx, 1): draw(idx)
  and everything else an item carries are bit for bit what they are without reverberation.

  Simulated rooms (room_t60 = (lo, hi) seconds; sepkern/room.py): every mixture gets a shoebox room of its own -- dimensions uniform
  in room_dims = (lo, hi), a NOMINAL t60 uniform in room_t60 that sets the walls' reflection coefficients (Eyring), the microphone
  array `array` ((C, 3) offsets from its centre in metres; None: one microphone) somewhere in it at a random yaw, and the S
  sources -- and the image-method RIRs from every source to every microphone are made ON THE GPU (sk_room_rirs) in front of the
  convolution.  An item then carries 'room': the fp64 geometry {'L', 'beta', 'mics': the reference microphone ipd_ref followed
  by those of ipd_channels (only they travel), 'srcs', 'ntaps' = min(round(t60 rate), 8192) at the rate the convolution runs
  at, 'rate', 'chans'}.  With ipd_channels the mixed batch is an array batch ('chan<c>' behind the sources) for an IPD model.
  These draws come from a generator of their own, seeded (seed, idx, 2): draw(idx) and every other key are bit for bit what they
  are without a room.  Not together with rir_scp / rir_synth.

  Noise (noise_scp: lines `<noise-id> <path>` of mono 16-bit wav files at the working rate -- another rate is an error here, as
  for RIRs; the files are read lazily, with mmap; sepkern/noise.py): a noise recording is added ON THE GPU to every mixture
  (sk_add_noise) at a ratio of mixture to noise, on the reference channel, of snr ~ U(noise_snr_db) dB.  An item then carries
  'noise1' .. 'noise<C>' (int16, as long as the mixture at the working rate) -- one crop per microphone that travels, 1 without an
  array -- and 'noise_amp' = 10^(-snr / 20).  With an array the C crops are the independent inputs of a spherically isotropic
  field with the microphones' coherence (sk_noise_factors, sk_diffuse_noise).  Every crop is a (file, start) pair drawn on its
  own, and a file shorter than the mixture wraps around; crops that overlap -- a short list -- make the field less diffuse.
  These draws come from a generator of their own, seeded (seed, idx, 3): draw_noise(idx); every other key an item carries is bit
  for bit what it is without noise.  The sources stay clean: the targets of a noisy mixture are its noise-free sources."""

  def __init__(self, datadir, num_spk, mixes_per_epoch=None, snr_db=2.5, peak=(0.9, 0.9), max_samples=0, seed=0, sample_rate=None,
               quantize=False, rir_scp=None, rir_synth=None, rir_drr_db=(0.0, 15.0), rir_prob=1.0,
               room_t60=None, room_dims=((3, 3, 2.5), (8, 6, 4)), array=None, ipd_ref=0, ipd_channels=(),
               noise_scp=None, noise_snr_db=(-3.0, 6.0)):
    import wave
    self.num_spk, self.seed = int(num_spk), int(seed)
    self.snr_db, self.peak, self.max_samples = float(snr_db), (float(peak[0]), float(peak[1])), int(max_samples)
    self.sample_rate = None if sample_rate is None else int(sample_rate)
    if not 1 <= self.num_spk <= 4:
      raise ValueError("DynMixTrainSet: num_spk = %d outside 1..4" % self.num_spk)
    if self.snr_db < 0 or not 0 < self.peak[0] <= self.peak[1] <= 1.0 or self.max_samples < 0 or 0 < self.max_samples < 257:
      raise ValueError("DynMixTrainSet: snr_db >= 0, 0 < peak[0] <= peak[1] <= 1 and max_samples 0 or >= 257 expected")
    spk_of = dict(line.split()[:2] for line in open(datadir + "/utt2spk") if line.strip())
    by_spk, short, self.rate = {}, 0, None
    for line in open(datadir + "/wav.scp"):
      if not line.strip():
        continue
      utt, path = line.rstrip('\n').split(' ', 1)
      if utt not in spk_of:
        raise ValueError("DynMixTrainSet: utt2spk names no speaker for %r" % utt)
      with wave.open(path, "rb") as w:
        if w.getnchannels() != 1 or w.getsampwidth() != 2:
          raise ValueError("%s: only mono 16-bit PCM wav is supported" % path)
        n, fs = w.getnframes(), w.getframerate()
      if self.rate is not None and fs != self.rate:
        raise ValueError("%s is sampled at %d Hz, the files before it at %d: the utterances of a corpus must share one rate" % (path, fs, self.rate))
      self.rate = fs
      if self._at_rate(n) < 257:          # fewer samples than the STFT's reflect padding needs: cannot be framed
        short += 1
        continue
      by_spk.setdefault(spk_of[utt], []).append((path, n))
    if short:
      raise ValueError("DynMixTrainSet: %d utterance(s) of %s/wav.scp have fewer than 257 samples and cannot be framed; "
                       "take them out of the list" % (short, datadir))
    self.speakers = [by_spk[s] for s in sorted(by_spk)]
    if len(self.speakers) < self.num_spk:
      raise ValueError("DynMixTrainSet: %d speaker(s) in %s, a mixture needs %d different ones" % (len(self.speakers), datadir, self.num_spk))
    n_utts = sum(len(u) for u in self.speakers)
    self.mixes_per_epoch = int(mixes_per_epoch) if mixes_per_epoch else n_utts // self.num_spk
    if self.mixes_per_epoch < 1:
      raise ValueError("DynMixTrainSet: mixes_per_epoch must be at least 1")
    self.longest = max(n for u in self.speakers for _, n in u)
    self.collator = DynMixCollator(self.sample_rate, quantize)
    self._init_reverb(rir_scp, rir_synth, rir_drr_db, rir_prob)
    self._init_room(room_t60, room_dims, array, ipd_ref, ipd_channels)
    self._init_noise(noise_scp, noise_snr_db)

  def _init_noise(self, noise_scp, noise_snr_db):
    import wave
    self.noises = None
    self.noise_snr_db = (float(noise_snr_db[0]), float(noise_snr_db[1]))
    if not noise_scp:
      return
    if not self.noise_snr_db[0] <= self.noise_snr_db[1]:
      raise ValueError("DynMixTrainSet: noise_snr_db = (lo, hi) dB with lo <= hi expected")
    self.noises = []
    for line in open(noise_scp):
      if not line.strip():
        continue
      _, path = line.rstrip('\n').split(' ', 1)
      path = path.strip()
      with wave.open(path, "rb") as w:
        if w.getnchannels() != 1 or w.getsampwidth() != 2:
          raise ValueError("%s: only mono 16-bit PCM wav is supported for a noise recording" % path)
        if w.getframerate() != int(self.rir_rate):
          raise ValueError("noise recording %s is sampled at %d Hz, the run works at %d Hz: noise is not resampled"
                           % (path, w.getframerate(), int(self.rir_rate)))
        if w.getnframes() < 1:
          raise ValueError("%s: an empty noise recording" % path)
        self.noises.append((path, w.getnframes()))
    if not self.noises:
      raise ValueError("%s lists no noise recording" % noise_scp)

  def noise_channels(self):
    """Microphones that travel: the reference and, in a simulated room, those of ipd_channels."""
    return 1 + (len(self.ipd_channels) if self.room_t60 is not None else 0)

  def draw_noise(self, idx):
    """The noise of item idx, from a generator of its own: (snr dB, [(path, crop start, file length)] per microphone)."""
    rng = np.random.default_rng([self.seed, int(idx), 3])
    snr = float(rng.uniform(self.noise_snr_db[0], self.noise_snr_db[1]))
    crops = []
    for _ in range(self.noise_channels()):
      path, m = self.noises[int(rng.integers(len(self.noises)))]
      crops.append((path, int(rng.integers(m)), m))
    return snr, crops

  def _init_room(self, room_t60, room_dims, array, ipd_ref, ipd_channels):
    from sepkern import room as _room
    self.room_t60 = None
    self.ipd_ref = _ipd.parse_ref(ipd_ref)
    self.ipd_channels = _ipd.parse_channels(ipd_channels, self.ipd_ref)
    if room_t60 is None:
      if array is not None or self.ipd_channels:
        raise ValueError("DynMixTrainSet: an array and ipd_channels need simulated rooms (room_t60): the mixtures made on the GPU "
                         "have one channel without")
      return
    if self.reverb:
      raise ValueError("DynMixTrainSet: room_t60 simulates the rooms; rir_scp / rir_synth are another source of RIRs, give one of them")
    self.room_t60 = (float(room_t60[0]), float(room_t60[1]))
    self.room_dims = (tuple(float(v) for v in room_dims[0]), tuple(float(v) for v in room_dims[1]))
    self.array = np.zeros((1, 3)) if array is None else np.asarray(array, dtype=np.float64).reshape(-1, 3)
    if not 0.0 < self.room_t60[0] <= self.room_t60[1] or len(self.room_dims[0]) != 3 or len(self.room_dims[1]) != 3:
      raise ValueError("DynMixTrainSet: room_t60 = (lo, hi) seconds with 0 < lo <= hi and room_dims = ((x, y, z), (x, y, z)) expected")
    if not 1 <= len(self.array) <= _room.MAX_MICS:
      raise ValueError("DynMixTrainSet: an array of 1..%d microphones expected (got %d)" % (_room.MAX_MICS, len(self.array)))
    need = max(self.ipd_channels + (self.ipd_ref,)) + 1
    if need > len(self.array):
      raise ValueError("DynMixTrainSet: the array has %d microphone(s): ipd_ref = %d with ipd_channels = %s needs %d"
                       % (len(self.array), self.ipd_ref, ",".join(str(c) for c in self.ipd_channels), need))
    # the direct path must lie inside the shortest RIR (sk_fir_convolve: delay < ntaps), whatever the draw
    far = _room.direct_delay(self.room_dims[1], (0.0, 0.0, 0.0), self.rir_rate)
    if min(int(round(self.room_t60[0] * self.rir_rate)), _room.MAX_TAPS) <= far:
      raise ValueError("DynMixTrainSet: room_t60[0] = %g s is %d taps at %d Hz; the direct path across the largest room takes %d"
                       % (self.room_t60[0], int(round(self.room_t60[0] * self.rir_rate)), self.rir_rate, far))

  def draw_room(self, idx):
    """The room of item idx, from a generator of its own: the 'room' block an item carries."""
    from sepkern import room as _room
    rng = np.random.default_rng([self.seed, int(idx), 2])
    r = _room.draw_room(rng, self.room_dims[0], self.room_dims[1], self.room_t60, self.array, self.num_spk)
    picked = [self.ipd_ref] + list(self.ipd_channels)
    return {'L': r['L'], 'beta': r['beta'], 'mics': r['mics'][picked], 'srcs': r['srcs'],
            'ntaps': min(int(round(r['t60'] * self.rir_rate)), _room.MAX_TAPS), 'rate': int(self.rir_rate),
            'chans': [int(c) for c in self.ipd_channels]}

  def _init_reverb(self, rir_scp, rir_synth, rir_drr_db, rir_prob):
    self.rirs, self.rir_synth, self.rir_prob = None, None, float(rir_prob)
    self.rir_drr_db = (float(rir_drr_db[0]), float(rir_drr_db[1]))
    self.rir_rate = self.sample_rate if self.sample_rate is not None else self.rate      # the rate the convolution runs at
    if rir_scp and rir_synth:
      raise ValueError("DynMixTrainSet: rir_scp and rir_synth are two sources of RIRs; give one of them")
    if not 0.0 <= self.rir_prob <= 1.0 or self.rir_drr_db[0] > self.rir_drr_db[1]:
      raise ValueError("DynMixTrainSet: 0 <= rir_prob <= 1 and rir_drr_db[0] <= rir_drr_db[1] expected")
    if rir_scp:
      from sepkern.reverb import MAX_TAPS, read_rir_scp
      self.rirs, cut = read_rir_scp(rir_scp, self.rir_rate)
      if cut:
        print("DynMixTrainSet: %d of the %d RIRs of %s are longer than %d taps and were cut to that" % (cut, len(self.rirs), rir_scp, MAX_TAPS))
    elif rir_synth:
      self.rir_synth = (float(rir_synth[0]), float(rir_synth[1]))
      if not 0.0 < self.rir_synth[0] <= self.rir_synth[1] or int(round(self.rir_synth[0] * self.rir_rate)) < 1:
        raise ValueError("DynMixTrainSet: rir_synth = (lo, hi) seconds of T60 with 0 < lo <= hi, at least one tap long")
    self.reverb = self.rirs is not None or self.rir_synth is not None

  def draw_rirs(self, idx):
    """The RIRs of item idx, from a generator of their own: ([float32 taps per source], [delay per source])."""
    from sepkern.reverb import direct_delay, synthetic_rir
    rng = np.random.default_rng([self.seed, int(idx), 1])
    rirs, delays = [], []
    for _ in range(self.num_spk):
      if rng.random() >= self.rir_prob:
        rirs.append(np.ones(1, dtype=np.float32))
        delays.append(0)
        continue
      if self.rirs is not None:
        h = self.rirs[int(rng.integers(len(self.rirs)))]
      else:
        t60, drr = float(rng.uniform(*self.rir_synth)), float(rng.uniform(*self.rir_drr_db))
        h = synthetic_rir(rng, t60, self.rir_rate, drr)
      rirs.append(h)
      delays.append(direct_delay(h))
    return rirs, delays

  def _at_rate(self, n):
    """Samples once at sample_rate (sepkern/resample.py's length rule)."""
    if self.sample_rate is None or self.rate == self.sample_rate:
      return n
    from sepkern.resample import out_len
    return out_len(n, self.rate, self.sample_rate)

  def __len__(self):
    return self.mixes_per_epoch          # of ONE epoch; any idx >= 0 is an item (MixDraws adds epoch * mixes_per_epoch)

  def frame_counts(self):
    """An upper bound of every item's frame count (the draw decides the true one); only good for balancing ranks."""
    n = self._at_rate(self.longest)
    return [1 + (min(n, self.max_samples) if self.max_samples else n) // 128] * self.mixes_per_epoch

  def draw(self, idx):
    """What item idx is made of, without touching a file: [(path, crop start, file length)] per source, n, snr dB per source, peak."""
    rng = np.random.default_rng([self.seed, int(idx)])
    picks = [self.speakers[k][int(rng.integers(len(self.speakers[k])))] for k in rng.choice(len(self.speakers), self.num_spk, replace=False)]
    n = min(m for _, m in picks)
    if self.max_samples:      # (in file samples: at most max_samples once resampled)
      resampled = self.sample_rate is not None and self.rate != self.sample_rate
      n = min(n, self.max_samples * self.rate // self.sample_rate if resampled else self.max_samples)
    starts = [int(rng.integers(0, m - n + 1)) for _, m in picks]
    snr = [float(v) for v in rng.uniform(-self.snr_db, self.snr_db, self.num_spk)]
    return [(path, st, m) for (path, m), st in zip(picks, starts)], n, snr, float(rng.uniform(self.peak[0], self.peak[1]))

  def __getitem__(self, idx):
    import scipy.io.wavfile
    from sepkern.mixing import snr_to_amp
    if idx < 0:
      raise IndexError(idx)
    picks, n, snr, peak = self.draw(idx)
    out = {}
    for s, (path, st, m) in enumerate(picks):
      _, x = scipy.io.wavfile.read(path, mmap=True)
      if x.dtype != np.int16 or x.ndim != 1 or len(x) != m:
        raise ValueError("%s: changed since the set was built (mono 16-bit PCM of %d samples expected)" % (path, m))
      out['source' + str(s + 1)] = np.array(x[st:st + n])           # only the slice leaves the worker
    out['amp'] = [float(snr_to_amp(v)) for v in snr]
    out['peak'] = peak
    if self.sample_rate is not None:
      out['rate'] = int(self.rate)
    if self.reverb:
      rirs, out['rir_delay'] = self.draw_rirs(idx)
      for s, h in enumerate(rirs):
        out['rir' + str(s + 1)] = h
    if self.room_t60 is not None:
      out['room'] = self.draw_room(idx)
    if self.noises is not None:
      from sepkern.noise import snr_to_amp as noise_amp
      snr_n, crops = self.draw_noise(idx)
      nn = self._at_rate(n)                # the mixture's length at the working rate, where the noise is added
      for c, (path, st, m) in enumerate(crops):
        _, v = scipy.io.wavfile.read(path, mmap=True)
        if v.dtype != np.int16 or v.ndim != 1 or len(v) != m:
          raise ValueError("%s: changed since the set was built (mono 16-bit PCM of %d samples expected)" % (path, m))
        if st + nn <= m:
          out['noise' + str(c + 1)] = np.array(v[st:st + nn])
        else:                              # a file shorter than the mixture (or a crop near its end) wraps around
          out['noise' + str(c + 1)] = np.asarray(v).take(np.arange(st, st + nn) % m)
      out['noise_amp'] = float(noise_amp(snr_n))
    return out


class DynMixCollator():
  """WavCollator for DynMixTrainSet's items: sorted by frame count, longest first, the SOURCES' int16 samples as one tensor,
  key-major ('source1', ...), and what the GPU needs to mix them -- {'pcm': {'flat', 'keys': ['source1', ...], 'lens', 'mixing':
  {'amp': [S][B], 'peak': [B], 'quantize'}}} (+ 'rate' / 'target_rate' as WavCollator).  The batch holds no 'mix': sepkern.data's
  front ends make it (mixed_pcm) and go on as they do for a WavCollator batch.  Noisy items ('noise1' .. 'noise<C>', 'noise_amp')
  add 'noise' = {'flat': int16 tensor, channel-major in the batch's order, 'lens': samples per item, 'amp': [B]}; every item of a
  batch has noise or none does."""

  def __init__(self, sample_rate=None, quantize=False):
    self.sample_rate = None if sample_rate is None else int(sample_rate)
    self.quantize = bool(quantize)

  def __call__(self, batch):
    keys = sorted((k for k in batch[0] if k.startswith('source') and k[6:].isdigit()), key=lambda k: int(k[6:]))
    if not keys or keys != ['source' + str(s + 1) for s in range(len(keys))]:
      raise ValueError("DynMixCollator: an item holds the signals 'source1' .. 'source<S>' (got %r)" % sorted(batch[0]))
    # ONE list of sample counts describes every key of the flat tensor (see WavCollator): a source of another length is an error
    for d in batch:
      for k in keys:
        if k not in d or len(d[k]) != len(d[keys[0]]):
          raise ValueError("DynMixCollator: signal %r of a mixture has %s samples, its first source %d -- the sources of a mixture "
                           "must have one length" % (k, len(d[k]) if k in d else "no", len(d[keys[0]])))
      if len(d.get('amp', ())) != len(keys) or 'peak' not in d:
        raise ValueError("DynMixCollator: an item carries one 'amp' per source and a 'peak'")
    if self.sample_rate is None:
      rates = None
      frames = [1 + len(d[keys[0]]) // 128 for d in batch]
    else:
      from sepkern.resample import out_len
      if any('rate' not in d for d in batch):
        raise ValueError("DynMixCollator(sample_rate=%d): an item does not say at which rate it was recorded ('rate')" % self.sample_rate)
      rates = [int(d['rate']) for d in batch]
      frames = [1 + out_len(len(d[keys[0]]), r, self.sample_rate) // 128 for d, r in zip(batch, rates)]
    order = np.argsort(np.array(frames))[::-1]
    flat = np.concatenate([batch[i][k] for k in keys for i in order])
    pcm = {'flat': torch.from_numpy(flat), 'keys': keys, 'lens': [int(len(batch[i][keys[0]])) for i in order],
           'mixing': {'amp': [[float(batch[i]['amp'][s]) for i in order] for s in range(len(keys))],
                      'peak': [float(batch[i]['peak']) for i in order], 'quantize': self.quantize}}
    if rates is not None:
      pcm['rate'] = [rates[i] for i in order]
      pcm['target_rate'] = self.sample_rate
    if any('rir1' in d for d in batch):    # reverberant items: every source's RIR, source-major in the batch's order, as ONE tensor
      S = len(keys)
      if any(any('rir' + str(s + 1) not in d for s in range(S)) or len(d.get('rir_delay', ())) != S for d in batch):
        raise ValueError("DynMixCollator: a reverberant item carries 'rir1' .. 'rir<S>' and one 'rir_delay' per source, and so does every item of its batch")
      rirs = [[np.asarray(batch[i]['rir' + str(s + 1)], dtype=np.float32) for i in order] for s in range(S)]
      offs, at = [], 0
      for row in rirs:
        offs.append([])
        for h in row:
          offs[-1].append(at)
          at += len(h)
      pcm['reverb'] = {'flat': torch.from_numpy(np.concatenate([h for row in rirs for h in row])), 'offs': offs,
                       'taps': [[int(len(h)) for h in row] for row in rirs],
                       'delay': [[int(batch[i]['rir_delay'][s]) for i in order] for s in range(S)]}
    if any('room' in d for d in batch):    # simulated rooms: every item's geometry (fp64), in the batch's order
      rooms = [batch[i].get('room') for i in order]
      if any(r is None or r['chans'] != rooms[0]['chans'] or r['rate'] != rooms[0]['rate'] or len(r['srcs']) != len(keys) for r in rooms):
        raise ValueError("DynMixCollator: an item with a room carries S source positions, and every item of its batch has a room "
                         "with the same channels at the same rate")
      pcm['room'] = {'L': np.stack([r['L'] for r in rooms]), 'beta': np.stack([r['beta'] for r in rooms]),
                     'mics': np.stack([r['mics'] for r in rooms]), 'srcs': np.stack([r['srcs'] for r in rooms]),
                     'ntaps': [int(r['ntaps']) for r in rooms], 'rate': rooms[0]['rate'], 'chans': list(rooms[0]['chans'])}
    if any('noise1' in d for d in batch):  # noisy items: one crop per microphone, channel-major in the batch's order, as ONE tensor
      nk = sorted((k for k in batch[0] if k.startswith('noise') and k[5:].isdigit()), key=lambda k: int(k[5:]))
      if any('noise_amp' not in d or sorted(k for k in d if k.startswith('noise') and k[5:].isdigit()) != sorted(nk)
             or any(len(d[k]) != len(d[nk[0]]) for k in nk) for d in batch) or nk != ['noise' + str(c + 1) for c in range(len(nk))]:
        raise ValueError("DynMixCollator: a noisy item carries 'noise1' .. 'noise<C>' of one length and 'noise_amp', and so does "
                         "every item of its batch, with the same C")
      pcm['noise'] = {'flat': torch.from_numpy(np.concatenate([np.asarray(batch[i][k], dtype=np.int16) for k in nk for i in order])),
                      'lens': [int(len(batch[i][nk[0]])) for i in order], 'amp': [float(batch[i]['noise_amp']) for i in order]}
    return {'pcm': pcm}


class _DpclFn(torch.autograd.Function):
  """out = [mean_j L_j, count, sum_j L_j] of the deep-clustering loss (sepkern/dpcl.py) from the packed embedding rows."""

  @staticmethod
  def forward(ctx, z, mix, pk, count_dev, embed_dim, weight, vad_db, *srcs):
    res = ops.dpcl_fwd(z, mix, list(srcs), pk, embed_dim, weight, vad_db, count_dev)
    ctx.save_for_backward(z, mix, res["ab"], res["stats"], res["out"], *srcs)
    ctx.pk, ctx.conf = pk, (embed_dim, weight)
    return res["out"]

  @staticmethod
  def backward(ctx, gout):
    z, mix, ab, stats, out = ctx.saved_tensors[:5]
    srcs = list(ctx.saved_tensors[5:])
    # (columns >= F*D and rows >= R of a padded buffer: zero, as _WaveLossFn leaves dmask)
    dz = ops.dpcl_bwd(z, mix, srcs, ctx.pk, ctx.conf[0], dict(ab=ab, stats=stats, out=out), gout[0:1].contiguous(), ctx.conf[1])
    return (dz, None, None, None, None, None, None) + (None,) * len(srcs)


class _PitFn(torch.autograd.Function):
  """out = [loss/norm, norm, sum_b min_p L/S] (reference archs/uPIT.py:181-197,206)."""

  @staticmethod
  def forward(ctx, mask, mix, pk, norm_dev, *srcs):
    # mask (R, S*F), mix / srcs (R, F): packed rows of the batch pk (PackedSequence.data, archs/uPIT.py:160-167)
    res = ops.pit_mse_fwd(mask, mix, list(srcs), None, norm_dev, packing=pk)
    ctx.save_for_backward(mask, mix, res["best_perm"], res["out"], *srcs)
    ctx.pk = pk
    ctx.mark_non_differentiable(res["best_perm"])
    return res["out"], res["best_perm"]

  @staticmethod
  def backward(ctx, gout, _gperm):
    mask, mix, best, out = ctx.saved_tensors[:4]
    srcs = list(ctx.saved_tensors[4:])
    dmask = ops.pit_mse_bwd(mask, mix, srcs, best, out, gout[0:1].contiguous(), packing=ctx.pk)
    return (dmask, None, None, None) + (None,) * len(srcs)


LOSSES = ('mse', 'sisdr', 'psa', 'tpsa')
PSA_LOSSES = ('psa', 'tpsa')       # PIT-MSE on phase-sensitive targets (sepkern/psa.py); 'tpsa' holds them to [0, |mix|]
MIXIT_LOSSES = ('mixit',)          # mixture-invariant training (sepkern/mixit.py): num_spk masks against the TWO mixed recordings
WAVE_LOSSES = ('sisdr',) + MIXIT_LOSSES      # computed from the batch's waveforms (the driver keeps them with the staged batch)
DPCL_LOSSES = ('dpcl',)            # deep clustering (sepkern/dpcl.py): embeddings instead of masks, on loss=mse's inputs


def parse_loss(value):
  """The conf key `loss`: 'mse' (default), 'sisdr', 'psa', 'tpsa', 'mixit' or 'dpcl'."""
  value = str(value).strip().lower()
  known = LOSSES + MIXIT_LOSSES + DPCL_LOSSES
  if value not in known:
    raise ValueError("conf key loss: %r is not one of %s" % (value, " / ".join(repr(v) for v in known)))
  return value


IPD_NEEDS_WAVEFORMS = "`ipd_channels` needs waveforms: an IPD model trains on array recordings with `--wav-input`"
IPD_NO_MIXIT = "`ipd_channels` does not train with `loss=mixit`: its mixtures are sums of two recordings made on one channel"
IPD_NO_DYNAMIC_MIX = "`ipd_channels` does not train with `--dynamic-mix`: the mixtures made on the GPU have one channel"
IPD_NO_NPZ = ("`ipd_channels`: npz features hold one channel's magnitudes; an IPD model separates array recordings with "
              "steps/separate_wav.py")


def ipd_conf(conf, loss_kind=None):
  """(ipd_ref, ipd_channels) of a model conf (a dict of strings): (0, ()) for a model without ipd_channels.  With the
  conf's loss (parsed) an unsupported pairing is refused here, when the model -- or the driver -- reads its conf."""
  ref = _ipd.parse_ref(conf.get('ipd_ref', 0))
  chans = _ipd.parse_channels(conf.get('ipd_channels'), ref)
  if chans and loss_kind in MIXIT_LOSSES:
    raise ValueError(IPD_NO_MIXIT)
  return ref, chans


NEEDS_WAVEFORMS = "`loss=sisdr` needs waveforms: train with `--wav-input`"


def needs_waveforms(kind):
  """NEEDS_WAVEFORMS for another loss that is made from the waveforms."""
  return NEEDS_WAVEFORMS.replace("loss=sisdr", "loss=" + kind)


# A waveform loss as _WaveLossFn runs it: forward op (est, est_offs, ref, ref_offs, nsamp, n_est, max_samples, *extra, count),
# backward op (est, est_offs, ref, ref_offs, choice, coef, gscale, mixc, pk, n_est, out=dmask), the forward result's key of the
# per-utterance choice the backward needs.
_WaveLoss = collections.namedtuple('_WaveLoss', 'fwd bwd choice')
_SISDR = _WaveLoss(ops.sisdr_pit_fwd, ops.sisdr_mask_grad, 'best_perm')     # arg-max permutation; no extra arguments
_MIXIT = _WaveLoss(ops.mixit_fwd, ops.mixit_mask_grad, 'best_code')         # arg-max assignment code; extra = (tau,)


class _WaveLossFn(torch.autograd.Function):
  """out = [-mean_j best score, count, sum_j best score] from the packed mask rows: mask-apply + iSTFT of the n_est estimates,
  the loss's sums and its search (permutations / assignments) forward; the loss's gradient and the iSTFT's adjoint fused in
  one kernel backward."""

  @staticmethod
  def forward(ctx, mask, pk, wave, desc, count_dev, n_est, loss, extra):
    est, est_offs, _ = ops.mask_istft_rows(wave['mixc'], mask, pk, n_est, est_offs=desc['est_offs'])
    ref_offs = desc['ref_offs']
    res = loss.fwd(est, est_offs, wave['flat'], ref_offs, desc['nsamp'], n_est, 128 * (pk.T - 1), *extra, count_dev)
    best = res[loss.choice]
    ctx.save_for_backward(est, est_offs, ref_offs, best, res["coef"], wave['mixc'], wave['flat'])
    ctx.pk, ctx.n_est, ctx.loss, ctx.shape = pk, n_est, loss, tuple(mask.shape)
    ctx.mark_non_differentiable(best)
    return res["out"], best

  @staticmethod
  def backward(ctx, gout, _gbest):
    est, est_offs, ref_offs, best, coef, mixc, flat = ctx.saved_tensors
    dmask = torch.empty(ctx.shape, dtype=torch.float32, device=est.device)
    dmask[ctx.pk.R:].zero_()               # tail rows of an (Rp, .) buffer stay zero
    ctx.loss.bwd(est, est_offs, flat, ref_offs, best, coef, gout[0:1].contiguous(), mixc, ctx.pk, ctx.n_est, out=dmask)
    return dmask, None, None, None, None, None, None, None


class SepDNN(SepDNNBase):
  def __init__(self, gpuid, **kwargs):
    super(SepDNN, self).__init__()
    self.feat_dim = int(kwargs.get('feat_dim', 257))
    self.num_spk = int(kwargs.get('num_spk', 2))
    self.loss_kind = parse_loss(kwargs.get('loss', 'mse'))
    self.mixit_snr_max = float(kwargs.get('mixit_snr_max', 30.0))     # dB, read by loss=mixit only (sepkern/mixit.py: tau)
    if self.loss_kind in MIXIT_LOSSES and not 2 <= self.num_spk <= 4:
      raise ValueError("loss=mixit: num_spk = %d estimates per mixture is outside 2..4" % self.num_spk)
    # loss=dpcl (sepkern/dpcl.py): the head emits embed_dim planes of feat_dim columns; num_spk counts the label columns in
    # training and the clusters at inference
    self.embed_dim = _dpcl.parse_embed_dim(kwargs.get('embed_dim', 20))
    self.dpcl_weight = _dpcl.parse_weight(kwargs.get('dpcl_weight', 'mr'))
    self.dpcl_vad_db = float(kwargs.get('dpcl_vad_db', _dpcl.DEFAULT_VAD_DB))
    self.dpcl_kmeans_iters = int(kwargs.get('dpcl_kmeans_iters', _dpcl.DEFAULT_ITERATIONS))
    if self.loss_kind in DPCL_LOSSES:
      _dpcl.vad_ratio(self.dpcl_vad_db)
      if not 1 <= self.num_spk <= _dpcl.MAX_S:
        raise ValueError("loss=dpcl: num_spk = %d is outside 1..%d" % (self.num_spk, _dpcl.MAX_S))
      if self.dpcl_kmeans_iters < 0:
        raise ValueError("loss=dpcl: dpcl_kmeans_iters = %d is negative" % self.dpcl_kmeans_iters)
    out_dim = self.feat_dim * (self.embed_dim if self.loss_kind in DPCL_LOSSES else self.num_spk)
    # ipd_channels (sepkern/ipd.py): the network also sees the phase differences of the listed channels against ipd_ref --
    # in_dim = 257 (1 + 2P); feat_dim, out_dim and every loss stay as they are
    self.ipd_ref, self.ipd_channels = ipd_conf(kwargs, self.loss_kind)
    if self.ipd_channels and self.feat_dim != _ipd.F:
      raise ValueError("ipd_channels: the phase features are made for feat_dim = %d (got %d)" % (_ipd.F, self.feat_dim))
    in_dim = _ipd.in_dim(len(self.ipd_channels)) if self.ipd_channels else self.feat_dim
    for key in kwargs.keys():
      print('modelparam:', key, kwargs[key])
    # the reference hard-codes 2 x 600 (archs/uPIT.py:115-119); hidden_dim / num_layers widen it
    self._build(gpuid, in_dim, out_dim, int(kwargs.get('hidden_dim', 600)),
                int(kwargs.get('num_layers', 2)), str(kwargs.get('dtype', 'fp32')), kwargs.get('sync_bn', '0'))

  def forward_packed(self, x2d, pk):
    """x2d (R,F) packed rows of the batch pk (PackedSequence.data on the GPU) -> mask (R,F*S) packed."""
    if self.hidden is None:
      self.hidden = self.init_hidden(pk.B)
    h0, c0 = self.hidden
    return self.run_net_packed(x2d, pk, h0, c0)

  def masks_packed(self, x2d, pk):
    """x2d (R,F) packed rows -> the (rows, F*S) masks of the batch: the network's own output for a uPIT model (forward_packed's
    tensor itself); for a loss=dpcl model the k-means masks of its embeddings (sk_dpcl_kmeans: a fresh contiguous tensor of
    0.0 / 1.0 in the same layout, num_spk clusters)."""
    out = self.forward_packed(x2d, pk)
    if getattr(self, 'loss_kind', 'mse') not in DPCL_LOSSES:
      return out
    if not 2 <= self.num_spk <= _dpcl.MAX_S:
      raise ValueError("loss=dpcl: k-means masks need num_spk in 2..%d clusters (got %d)" % (_dpcl.MAX_S, self.num_spk))
    mags = x2d[:, :self.feat_dim].contiguous() if getattr(self, 'ipd_channels', ()) else x2d    # (an IPD model's rows start with them)
    return ops.dpcl_kmeans(out.detach(), mags, pk, self.num_spk, self.dpcl_kmeans_iters, self.dpcl_vad_db, D=self.embed_dim)[0]

  def forward_padded(self, x, lens):
    """x (T,B,F) time-major zero-padded CUDA tensor, lens int32 CUDA (B) -> mask (T,B,F*S)."""
    if self.hidden is None:
      self.hidden = self.init_hidden(x.shape[1])
    h0, c0 = self.hidden
    return self.run_net(x, lens, h0, c0)

  def forward(self, x):
    # x: packed sequence of dim feat_dim  ->  tensor of shape (batch, seq_length, feat_dim*num_spk)
    # RESTRICTION (variable-length batches, gradients): the values at zero-padded frames are filled in as the constant the
    # reference's network shows there, sigmoid(lin(bn(0))), and carry NO gradient back into lin / bn (UnpackFn).  A loss that
    # zeroes padded frames -- the reference's PIT-MSE does: mix = 0 there, archs/uPIT.py:181-197 -- gets the reference's parameter
    # gradients exactly; a loss that reads the padded frames of model(x) would miss their contribution to d lin / d bn.
    x2d, pk = _to_packed(x, self.lin.weight.device)
    mask = self.forward_packed(x2d, pk)
    # (padded frames: the constant the reference's BatchNorm / Linear / sigmoid produce there, archs/uPIT.py:135-144)
    fill = None if pk.uniform else self._engine.pad_row()
    if mask.requires_grad and not pk.uniform:       # (uniform: unpack is a view, differentiable as it is)
      padded = UnpackFn.apply(mask, pk, fill)
    else:
      padded = pk.unpack(mask, fill=fill)
    # batch-first AND contiguous, as the reference's Linear + sigmoid output is: its own loss code takes .view(batch, -1) of an
    # elementwise result of this tensor (archs/uPIT.py:192), which a permuted view would refuse
    return padded.permute(1, 0, 2).contiguous()


def compute_cv_loss(model, epoch, batch_sample, plotdir=""):
  if plotdir:
    loss, norm = compute_loss(model, epoch, batch_sample, plotdir)
  else:
    loss, norm = compute_loss(model, epoch, batch_sample)
  return loss, norm


def compute_loss_packed(model, mix, sources, pk, plotdir="", net_in=None):
  """compute_loss on inputs that are already resident on the GPU as PACKED rows: mix (R,F) and sources [(R,F)]*S
  float32 -- PackedSequence.data of the collator's batch -- and their Packing pk.  Same return as compute_loss.
  net_in (here and in the routes below): the network's input rows where they are not mix -- an IPD model's wide rows
  (sepkern.data.ipd_rows_from_pcm); the loss kernels read mix either way."""
  batch = pk.B
  model.zero_grad()
  model.hidden = model.init_hidden(batch)

  # data-parallel: divide by the GLOBAL frame count so that the summed gradients equal the
  # single-device gradient of the global batch (None = single process, kernel uses sum(lens)*F)
  # -- only while training: the CV pass runs the whole (unsharded) set on every rank, local norm.
  training_step = model.training and torch.is_grad_enabled()
  norm_override = skdist.global_norm(pk.lens, model.feat_dim) if training_step else None

  mask_out = model.forward_packed(mix if net_in is None else net_in, pk)
  # mask_out: tensor of shape (sum of lengths, feat_dim*num_spk)
  out, best = _PitFn.apply(mask_out, mix, pk, norm_override, *sources)
  loss, norm = out[0], out[1].detach()
  model.last_best_perm = best.detach()      # arg-min permutation per utterance (index into itertools.permutations)

  if plotdir:
    sys.path.append('tools')
    import plot
    os.system("mkdir -p " + plotdir)
    F = model.feat_dim
    rows0 = pk.offs[:int(pk.lens_host[0])].long()              # the rows of the batch's first (longest) utterance
    m0, x0 = mask_out.detach()[rows0], mix[rows0]
    masked = (m0.view(-1, model.num_spk, F) * x0.unsqueeze(1)).reshape(-1, model.num_spk * F)
    plot.plot_spec(x0.cpu().numpy(), plotdir + '/Mixture.png')
    plot.plot_spec(masked.cpu().numpy(), plotdir + '/Masked_Mixture.png')
    permutation = list(itertools.permutations(range(model.num_spk)))[int(best[0])]
    plot.plot_spec(torch.cat([sources[i][rows0] for i in permutation], dim=1).cpu().numpy(),
                   plotdir + '/Chosen_Permutation.png')

  return loss, norm


def compute_loss_dpcl(model, mix, sources, pk, net_in=None):
  """The loss=dpcl route on loss=mse's inputs: mix (R,F) and sources [(R,F)]*S packed magnitude rows and their Packing.
  Returns (mean deep-clustering loss per utterance, number of utterances)."""
  if len(sources) < model.num_spk:
    raise ValueError("loss=dpcl: the batch holds %d sources (num_spk = %d)" % (len(sources), model.num_spk))
  model.zero_grad()
  model.hidden = model.init_hidden(pk.B)
  # data-parallel: divide by the GLOBAL utterance count (None = single process: the kernel uses B), while training only
  training_step = model.training and torch.is_grad_enabled()
  count = skdist.global_norm(pk.lens.new_full((1,), pk.B), 1) if training_step else None
  z = model.forward_packed(mix if net_in is None else net_in, pk)      # (rows, feat_dim * embed_dim): plane d of a row = dimension d of its bins
  srcs = [s.contiguous() for s in sources[:model.num_spk]]
  out = _DpclFn.apply(z, mix.contiguous(), pk, count, model.embed_dim, model.dpcl_weight, model.dpcl_vad_db, *srcs)
  model.step_frames = pk.R                  # (the norm counts utterances: the driver's frames/s line reads this)
  return out[0], out[1].detach()


def _wave_loss(model, mix, pk, wave, loss, descriptors, extra=(), net_in=None):
  """The head the waveform losses share: a fresh state, the global count, the descriptors, the network, the loss ->
  (out = [loss, count, sum], the per-utterance choice)."""
  n_est = model.num_spk
  model.zero_grad()
  model.hidden = model.init_hidden(pk.B)
  # data-parallel: divide by the GLOBAL utterance count (None = single process: the kernel uses B), while training only
  training_step = model.training and torch.is_grad_enabled()
  count = skdist.global_norm(pk.lens.new_full((1,), pk.B), 1) if training_step else None
  desc = descriptors(pk, wave['sig_offs'], n_est)       # (uploaded before the network is enqueued, not behind it)
  mask_out = model.forward_packed(mix if net_in is None else net_in, pk)
  out, best = _WaveLossFn.apply(mask_out, pk, wave, desc, count, n_est, loss, extra)
  model.step_frames = pk.R                  # (the norm counts utterances: the driver's frames/s line reads this)
  return out, best.detach()


def compute_loss_wave(model, mix, pk, wave, net_in=None):
  """The loss=sisdr route: mix (R,F) packed magnitude rows (the network's input), wave as wave_features_from_pcm made it.
  Returns (mean negative SI-SDR per utterance in dB, number of utterances)."""
  S = model.num_spk
  missing = [k for k in ('source' + str(i + 1) for i in range(S)) if k not in wave['sig_offs']]
  if missing:
    raise ValueError("loss=sisdr: the batch holds no waveform %s (num_spk = %d)" % (", ".join(missing), S))
  out, model.last_best_perm = _wave_loss(model, mix, pk, wave, _SISDR, ops.sisdr_descriptors, net_in=net_in)
  # (last_best_perm: arg-max permutation per utterance, index into itertools.permutations)
  return out[0], out[1].detach()


def compute_loss_mixit(model, mix, pk, wave):
  """The loss=mixit route: mix (R,F) packed magnitude rows (the network's input), wave as wave_features_from_pcm made it, with
  exactly the two mixed recordings as 'source1' and 'source2'; the network's num_spk = M masks are the estimates.
  Returns (mean negative MixIT score per utterance in dB, number of utterances)."""
  M = model.num_spk
  if not 2 <= M <= 4:
    raise ValueError("loss=mixit: num_spk = %d estimates per mixture is outside 2..4" % M)
  have = sorted(k for k in wave['sig_offs'] if k != 'mix')
  missing = [k for k in ('source1', 'source2') if k not in have]
  if missing:
    raise ValueError("loss=mixit: the batch holds no waveform %s (the two mixed recordings are the references)" % ", ".join(missing))
  if have != ['source1', 'source2']:
    raise ValueError("loss=mixit: the batch holds the waveforms %s; the references are exactly source1 and source2 "
                     "(num_spk = %d counts the masks)" % (", ".join(have), M))
  tau = 10.0 ** (-float(getattr(model, 'mixit_snr_max', 30.0)) / 10.0)
  out, model.last_best_code = _wave_loss(model, mix, pk, wave, _MIXIT, ops.mixit_descriptors, (tau,))
  # (last_best_code: arg-max assignment per utterance, bit k = the reference estimate k is added to)
  return out[0], out[1].detach()


def compute_loss_padded(model, mix, sources, lens, plotdir=""):
  """compute_loss on zero-padded time-major inputs resident on the GPU: mix (T,B,F), sources [(T,B,F)]*S float32,
  lens int32 (B) in any order.  They are packed (sk_pack_rows; a view when all lengths are equal) and go the packed way."""
  pk = model.packing_of(lens)
  if pk.perm is not None:
    # not length-sorted (the collator's batches are): the rows are packed in sorted order, so the initial state drawn for
    # this batch follows, and the chosen permutations are handed back in the caller's order
    h, c = model.init_hidden(pk.B)
    pair = (pk.sort_batch(h, 1), pk.sort_batch(c, 1))
    rest = model.next_hidden
    model.next_hidden = pair if rest is None else [pair] + (rest if isinstance(rest, list) else [rest])
  out = compute_loss_packed(model, pk.pack(mix), [pk.pack(s) for s in sources], pk, plotdir)
  if pk.perm is not None:
    model.last_best_perm = pk.unsort_batch(model.last_best_perm, 0)
  return out


def _pcm_front(model, pcm, dev, front, **front_args):
  """A PCM batch through `front` (one of sepkern.data's front ends) -> (its result, net_in): for an IPD model net_in is the
  wide input rows, made with the front end's rows from one copy of the samples (sepkern.data.ipd_rows_from_pcm); for any other
  model None -- the call is the one it was."""
  _match_channels(model, _batch_chan_keys(pcm))
  if getattr(model, 'ipd_channels', ()):
    return _ipd_rows_from_pcm(pcm, dev, front, **front_args)
  return front(pcm, dev, **front_args), None


def _match_channels(model, have):
  """The 'chan<c>' signals of a batch against the model's ipd_channels: the same channels in the same order, or an error."""
  want = [_ipd.chan_key(c) for c in getattr(model, 'ipd_channels', ())]
  if list(have) == want:
    return
  if not want:
    raise ValueError("the batch carries the array channels %s and the model sees one channel: give it the conf key ipd_channels, "
                     "or build the WavTrainSet without" % ", ".join(have))
  if not have:
    raise ValueError("the model has ipd_channels = %s and the batch holds one channel: an IPD model trains on WavTrainSet(ipd_ref, "
                     "ipd_channels) batches (steps/train_qsub.py --wav-input)" % ",".join(str(c) for c in model.ipd_channels))
  raise ValueError("the batch carries the channels %s, the model's ipd_channels ask for %s in that order" % (", ".join(have), ", ".join(want)))


def _staged_net_in(model, batch_sample):
  """The wide rows a Prefetcher staged with the batch (None for a model without ipd_channels)."""
  _match_channels(model, batch_sample.get('ipd_keys', []) if 'ipd' in batch_sample else [])
  return batch_sample.get('ipd')


def compute_loss(model, epoch, batch_sample, plotdir=""):
  dev = model.lin.weight.device
  kind = getattr(model, 'loss_kind', 'mse')
  if kind in PSA_LOSSES:
    if 'pcm' in batch_sample:
      (mix, targets, pk), net_in = _pcm_front(model, batch_sample['pcm'], dev, _psa_features_from_pcm, clamp=kind == 'tpsa')
    elif 'packed' in batch_sample and 'targets' in batch_sample:  # staged by Prefetcher(targets=kind): the targets are in place
      if batch_sample['targets'] != kind:
        raise ValueError("loss=%s: the batch was staged with %r targets" % (kind, batch_sample['targets']))
      (mix, targets, pk), net_in = batch_sample['packed'], _staged_net_in(model, batch_sample)
    else:                                                         # npz feature batches hold magnitudes only
      raise ValueError(needs_waveforms(kind))
    if len(targets) < model.num_spk:
      raise ValueError("loss=%s: the batch holds %d source waveforms (num_spk = %d)" % (kind, len(targets), model.num_spk))
    return compute_loss_packed(model, mix, targets[:model.num_spk], pk, plotdir, net_in=net_in)
  if kind in WAVE_LOSSES:
    if 'pcm' in batch_sample:
      (mix, _, pk, wave), net_in = _pcm_front(model, batch_sample['pcm'], dev, _wave_features_from_pcm, source_mags=False)
    elif 'packed' in batch_sample and 'wave' in batch_sample:     # staged by Prefetcher(keep_wave=True)
      (mix, _, pk), wave, net_in = batch_sample['packed'], batch_sample['wave'], _staged_net_in(model, batch_sample)
    else:                                                         # npz feature batches hold magnitudes only
      raise ValueError(needs_waveforms(kind))
    if kind in MIXIT_LOSSES:       # (never an IPD model: SepDNN refuses the pairing)
      return compute_loss_mixit(model, mix, pk, wave)
    return compute_loss_wave(model, mix, pk, wave, net_in=net_in)
  if 'pcm' in batch_sample:        # WavTrainSet batches: features are computed on the GPU
    (mix, sources, pk), net_in = _pcm_front(model, batch_sample['pcm'], dev, _features_from_pcm)
  elif 'packed' in batch_sample:   # batches staged on the GPU ahead of the step (sepkern.data.Prefetcher)
    (mix, sources, pk), net_in = batch_sample['packed'], _staged_net_in(model, batch_sample)
  else:
    if getattr(model, 'ipd_channels', ()):
      raise ValueError(IPD_NO_NPZ)
    mix, pk = _to_packed(batch_sample['mix'], dev)
    sources = [_to_packed(batch_sample['source' + str(i + 1)], dev)[0] for i in range(model.num_spk)]
    net_in = None
  if kind in DPCL_LOSSES:          # the same front ends: magnitudes of the mixture and the sources
    return compute_loss_dpcl(model, mix, sources, pk, net_in=net_in)
  return compute_loss_packed(model, mix, sources[:model.num_spk], pk, plotdir, net_in=net_in)


def estimate_masks(model, batch_sample):
  """The arithmetic half of compute_masks: [(file name, {'s1': (257,T_i) float32, ...}), ...] for one batch, without
  touching the disk (steps/eval_qsub.py overlaps the zlib compression of one batch with the next batch's GPU work)."""
  if getattr(model, 'ipd_channels', ()):
    raise ValueError(IPD_NO_NPZ)
  dev = model.lin.weight.device
  mix, pk = _to_packed(batch_sample['mix'], dev)
  name = batch_sample['name']
  batch = pk.B

  model.zero_grad()
  model.hidden = model.init_hidden(batch)

  with torch.no_grad():
    mask_np = model.masks_packed(mix, pk).cpu().numpy()              # (sum of lengths, feat_dim*num_spk)
  lens, offs = pk.lens_host, pk.offs_host
  out = []
  for i in range(len(name)):
    mask = mask_np[offs[:lens[i]] + i].transpose()                  # rows (t, i), t < lens[i]  ->  (feat_dim*num_spk, T_i)
    file_dict = dict()
    for src in range(model.num_spk):
      file_dict['s' + str(src + 1)] = mask[src * model.feat_dim:(src + 1) * model.feat_dim]
    out.append((name[i], file_dict))
  return out


def compute_masks(model, batch_sample, out_dir):
  for name, file_dict in estimate_masks(model, batch_sample):
    np.savez_compressed(out_dir + '/' + name, **file_dict)
