"""Host-side helpers around the Kaldi-style data interface (scp files, per-utterance npz / wav): cheap frame
counts for length-balanced sharding, without decoding the payloads."""
import os
import sys
import time
import wave
import zipfile

from numpy.lib import format as npformat


def host_threads(limit=4):
  """Cap torch's CPU thread pool in a process whose arithmetic runs on the GPU.  torch sizes the pool by the HOST's core
  count (128 on the MI355X boxes) even when the process may use 16 of them; every host thread that touches a tensor (the
  staging thread's pinned copies, a writer pool) then spawns its own pool of spinning workers and starves the loader's
  processes -- measured: 95 ms instead of 8 ms to stage one batch (tools/loader_probe.py)."""
  import torch
  try:
    cpus = len(os.sched_getaffinity(0))
  except AttributeError:
    cpus = os.cpu_count() or 1
  torch.set_num_threads(max(1, min(limit, cpus)))


def npz_frames(path, key="mix"):
    """Frame count T of the (257, T) array `key` in a feats npz (steps/extract_feats.py:90 writes zlib-compressed
    npz): only the .npy header of the zip member is inflated."""
    with zipfile.ZipFile(path) as z:
        with z.open(key + ".npy") as f:
            version = npformat.read_magic(f)
            if version == (1, 0):
                shape, _, _ = npformat.read_array_header_1_0(f)
            else:
                shape, _, _ = npformat.read_array_header_2_0(f)
    return int(shape[1]) if len(shape) > 1 else int(shape[0])


def wav_frames(path, hop=128, sample_rate=None):
    """STFT frame count 1 + N // hop of a wav file, from its header; with sample_rate, N is the file's length once resampled
    to that rate (sepkern/resample.py's length rule)."""
    with wave.open(path, "rb") as w:
        n = w.getnframes()
        if sample_rate is not None and w.getframerate() != int(sample_rate):
            from .resample import out_len
            n = out_len(n, w.getframerate(), sample_rate)
        return 1 + n // hop


def _at_target_rate(pcm, flat):
  """A WavCollator batch that carries 'rate' (per utterance) and 'target_rate' (WavTrainSet(sample_rate=...)) with an utterance
  recorded at another rate: every signal of the batch resampled on the device (ops.pcm_to_rate: one sk_resample launch per
  rate) -> (float32 flat in the same key-major layout, samples per utterance at the target rate).  A batch without those keys,
  or wholly at the target rate, is returned as it came: (flat, pcm['lens']) -- the int16 path, untouched."""
  from . import ops
  ns = [int(n) for n in pcm['lens']]
  rates, target = pcm.get('rate'), pcm.get('target_rate')
  if rates is None or target is None or all(int(r) == int(target) for r in rates):
    return flat, ns
  nk = len(pcm['keys'])
  out, outs = ops.pcm_to_rate(flat, ns * nk, [int(r) for r in rates] * nk, target)
  return out, outs[:len(ns)]


def signal_keys(keys):
  """'mix' and 'source<N>' of a batch's keys: what the front ends below transform.  An array batch (WavTrainSet with
  ipd_channels) carries the mixture's other channels behind them as 'chan<c>'; the front ends' results for it are bit for bit
  those of the mono batch of the reference channel, and ipd_rows_from_pcm makes the network's wide input rows."""
  from .ipd import signal_keys as pick
  return pick(keys)


def batch_chan_keys(pcm):
  """The 'chan<c>' signals a PCM batch holds -- or, for a batch still to be mixed in simulated rooms (DynMixCollator with 'room'),
  will hold once mixed_pcm has made them --, in order."""
  from .ipd import chan_key, chan_keys
  if 'mixing' in pcm:
    return [chan_key(c) for c in (pcm.get('room') or {}).get('chans', ())]
  return chan_keys(pcm['keys'])


def _room_jobs(room, S, B):
  """The S C B jobs of a batch's 'room' block, source-major, then microphone (the reference first), then mixture -> (rooms, betas,
  srcs, mics, scales, ntaps, delays): every RIR scaled by 4 pi |src - mic_ref| so that the direct path at the reference is ~ 1,
  and every microphone of a source at the REFERENCE microphone's direct delay: the time differences between the channels survive."""
  import numpy as np
  from .room import FOUR_PI, direct_delay
  L, beta, mics, srcs = (np.asarray(room[k], dtype=np.float64) for k in ('L', 'beta', 'mics', 'srcs'))
  C = mics.shape[1]
  if L.shape != (B, 3) or beta.shape != (B, 6) or mics.shape != (B, C, 3) or srcs.shape != (B, S, 3) or len(room['ntaps']) != B \
      or C != 1 + len(room.get('chans', ())):
    raise ValueError("mixed_pcm: 'room' holds per mixture a room (3), reflection coefficients (6), the reference microphone and "
                     "one per listed channel (3 each), %d sources (3 each) and a tap count" % S)
  rooms, betas, ss, ms, scales, ntaps, delays = [], [], [], [], [], [], []
  for s in range(S):
    for c in range(C):
      for b in range(B):
        rooms.append(L[b]); betas.append(beta[b]); ss.append(srcs[b, s]); ms.append(mics[b, c])
        scales.append(FOUR_PI * float(np.sqrt(np.sum((srcs[b, s] - mics[b, 0]) ** 2))))
        ntaps.append(int(room['ntaps'][b]))
        delays.append(direct_delay(srcs[b, s], mics[b, 0], room['rate']))
  return rooms, betas, ss, ms, scales, ntaps, delays


def _to_device(t, dev):
  """A tensor on `dev`: as it came if it is there, else ONE pinned host-to-device copy, asynchronous on the current stream."""
  import torch
  if t.device == torch.device(dev):
    return t
  return (t if t.is_pinned() else t.pin_memory()).to(dev, non_blocking=True)


def key_offsets(ns, which):
  """The offsets of a key-major batch: the signal with index q among the batch's keys holds utterance j at
  q * sum(ns) + sum(ns[:j]) -> [[offset of utterance j] for q in which]: what the ops wrappers take as offsets [list][B]."""
  from .ops import prefix_sums
  starts, total = prefix_sums(ns)
  return [[q * total + st for st in starts] for q in which]


def _staged(pcm, dev):
  """The head the front ends below share: a batch still to be mixed is mixed (mixed_pcm), the samples cross to the device in one
  copy and signals at another rate are resampled (_at_target_rate) -> (pcm as the front end goes on with it, src, flat, ns):
  flat and ns are the working-rate samples and their counts, src the tensor that crossed -- flat itself unless a signal was
  resampled -- whose use on the current stream the caller records."""
  if 'mixing' in pcm:                                  # DynMixCollator: the mixture is made here, on the device
    pcm = mixed_pcm(pcm, dev)
  src = _to_device(pcm['flat'], dev)
  flat, ns = _at_target_rate(pcm, src)
  return pcm, src, flat, ns


def mixed_pcm(pcm, dev):
  """A DynMixCollator batch -- pcm carries 'mixing' = {'amp': [S][B], 'peak': [B], 'quantize'} and the int16 samples of the
  SOURCES only, keys 'source1' .. 'source<S>', no 'mix' -- mixed on the device -> an ordinary pcm dict ON the device: 'flat'
  float32 in WavCollator's layout, 'keys' = ['mix', 'source1', ..., 'chan<c>', ...], 'lens', no 'rate'.  One pinned H2D copy of
  the samples, then ONE pipeline whose stages a batch switches on by what it carries; a stage it does not carry costs no launch:
    1. 'rate' / 'target_rate' with an utterance at another rate: the sources resampled (ops.pcm_to_rate); a mixture is as long
       as its shortest resampled source;
    2. RIRs for S C B jobs, source-major, then microphone, then mixture: GIVEN with 'reverb' = {'flat': float32 tensor of all
       RIRs, 'offs' / 'taps' / 'delay': [S][B]} (C = 1; sepkern/reverb.py) or MADE with 'room' (per mixture the fp64 geometry of a
       simulated room and C = 1 + P microphones, the reference, then the listed 'chans': _room_jobs, then ONE ops.room_rirs;
       sepkern/room.py) -- not both;
    3. with RIRs, ONE ops.fir_convolve over the jobs (the channels of a source share its dry signal): the targets are the
       reverberant sources;
    4. ONE ops.dynamic_mix (sepkern/mixing.py states the rule) sets the levels on the reference channel, into a buffer of
       (S + 1 + P) sum(lens) samples;
    5. with P listed channels, ONE ops.mix_channels forms their mixtures at those gains behind it: levels and peak are
       defined on the reference channel, another channel may exceed the peak;
    6. with 'noise' (sepkern/noise.py), noise added in place to the mixture's channels, the sources stay clean: _with_noise.
  The front ends below start with this and go on as they do for a batch that came mixed from disk; enqueued on the CURRENT
  stream."""
  import torch
  from . import ops
  from .ipd import chan_key
  mixing, keys = pcm['mixing'], list(pcm['keys'])
  S, ns = len(keys), [int(n) for n in pcm['lens']]
  B = len(ns)
  if keys != ['source' + str(s + 1) for s in range(S)]:
    raise ValueError("mixed_pcm: a batch to be mixed holds the signals 'source1' .. 'source<S>' (got %r)" % keys)
  src = flat = _to_device(pcm['flat'], dev)
  offs = key_offsets(ns, range(S))
  rates, target = pcm.get('rate'), pcm.get('target_rate')
  if rates is not None and target is not None and any(int(r) != int(target) for r in rates):
    flat, outs = ops.pcm_to_rate(flat, ns * S, [int(r) for r in rates] * S, target)
    ends = ops.prefix_sums(outs)[0]
    offs = [ends[s * B:(s + 1) * B] for s in range(S)]
    ns = [min(outs[s * B + j] for s in range(S)) for j in range(B)]
  rv, room = pcm.get('reverb'), pcm.get('room')
  if room is not None and rv is not None:
    raise ValueError("mixed_pcm: a batch carries 'room' or 'reverb', not both")
  chans = list(room.get('chans', ())) if room is not None else []
  P = len(chans)
  C, held, rirs = 1 + P, [src, flat], None
  if room is not None:
    rooms, betas, ss, ms, scales, taps, delays = _room_jobs(room, S, B)
    rirs, roffs = ops.room_rirs(rooms, betas, ss, ms, taps, room['rate'], scales=scales, device=dev)
  elif rv is not None:
    rirs = _to_device(rv['flat'], dev)
    roffs, taps, delays = ([v for row in rv[k] for v in row] for k in ('offs', 'taps', 'delay'))
  if rirs is not None:      # ONE sk_fir_convolve launch pair over all S C B signals; the levels are set on its result
    flat, at = ops.fir_convolve(flat, [offs[s][b] for s in range(S) for _ in range(C) for b in range(B)], ns * (S * C), rirs, roffs, taps, delays)
    held += [rirs, flat]
    job = lambda s, c: at[(s * C + c) * B:(s * C + c + 1) * B]  # noqa: E731
    offs, chan_offs = [job(s, 0) for s in range(S)], [[job(s, 1 + p) for p in range(P)] for s in range(S)]
  total, quant = sum(ns), bool(mixing.get('quantize', False))
  out = torch.empty((S + 1 + P) * total, dtype=torch.float32, device=flat.device)
  _, gains = ops.dynamic_mix(flat, offs, ns, mixing['amp'], mixing['peak'], quantize=quant, out=out)
  if P:
    ops.mix_channels(flat, chan_offs, ns, gains, quantize=quant, out=out[(S + 1) * total:])
  cur = torch.cuda.current_stream(dev)
  for t in held:
    t.record_stream(cur)
  return _with_noise({'flat': out, 'keys': ['mix'] + keys + [chan_key(c) for c in chans], 'lens': ns}, pcm.get('noise'), mixing, room, dev)


def _with_noise(mixed, nz, mixing, room, dev):
  """mixed_pcm's last step: the batch as it came without 'noise' (nz is None), else noise added in place to 'mix' and the
  'chan<c>' signals of the mixed batch.  The crops are as long as the mixtures at the working rate, or longer: they are cut."""
  if nz is None:
    return mixed
  import torch
  from . import ops
  from .ipd import chan_keys
  keys, ns, out = mixed['keys'], mixed['lens'], mixed['flat']
  B = len(ns)
  chans = ['mix'] + chan_keys(keys)
  C = len(chans)
  nl = [int(v) for v in nz['lens']]
  crops = nz['flat']
  if len(nl) != B or len(nz['amp']) != B or crops.numel() != C * sum(nl) or any(a < b for a, b in zip(nl, ns)):
    raise ValueError("mixed_pcm: 'noise' holds one crop per channel (%d) and mixture (%d), each at least as long as its mixture, "
                     "and one amplitude per mixture" % (C, B))
  crops = _to_device(crops, dev)
  noffs, soffs = key_offsets(nl, range(C)), key_offsets(ns, [keys.index(k) for k in chans])
  quant = bool(mixing.get('quantize', False))
  cur = torch.cuda.current_stream(dev)
  if C == 1:
    ops.add_noise(out, soffs, crops, noffs, ns, nz['amp'], quantize=quant)
  else:
    L = ops.noise_factors(room['mics'], room['rate'], device=dev)
    field = ops.diffuse_noise(crops, noffs, ns, L)
    ops.add_noise(out, soffs, field, key_offsets(ns, range(C)), ns, nz['amp'], quantize=quant)
    L.record_stream(cur)
    field.record_stream(cur)
  crops.record_stream(cur)
  return mixed


def features_from_pcm(pcm, dev):
  """The on-GPU feature front end of a wav batch.  pcm = the arch's WavCollator batch: {'flat': int16 tensor
  holding every signal of the batch, key-major ('mix', 'source1', ...), longest utterance first; 'keys'; 'lens': samples per
  utterance; optionally 'rate' (Hz per utterance) and 'target_rate': signals at another rate are resampled on the device
  first, sk_resample} -> (mix (R,F), [source (R,F)...] packed rows, their Packing): STFT magnitudes by sk_stft into the (T,B,F) grid,
  then the valid rows.  One H2D copy for the whole batch; everything is enqueued on the CURRENT stream."""
  import torch
  from . import ops
  from .packing import Packing
  pcm, src, flat, ns = _staged(pcm, dev)                # (another tensor only when a signal had to be resampled)
  B, F = len(ns), 257
  pk = Packing.from_lens([1 + n // 128 for n in ns], dev)
  feats, at, total = [], 0, sum(ns)
  for _ in signal_keys(pcm['keys']):                   # ('chan<c>' keys of an array batch are the IPD front end's, below)
    out = torch.zeros(pk.T, B, F, device=dev)
    ops.stft_batch(flat[at:at + total], lengths=ns, out=out, out_offs=[b * F for b in range(B)],
                   stride_t=[B * F] * B, stride_f=[1] * B)
    at += total
    feats.append(pk.pack(out))
  src.record_stream(torch.cuda.current_stream(dev))
  return feats[0], feats[1:], pk


def wave_features_from_pcm(pcm, dev, source_mags=True):
  """features_from_pcm for a loss that works on waveforms (archs/uPIT.py, loss=sisdr): the same batch ->
  (mix (R,F), [source (R,F)...], Packing, wave), wave = {'mixc': the mixture's COMPLEX STFT as packed rows (Rp, F) complex64,
  'flat': the batch's int16 PCM on the device (key-major, as the collator laid it out), 'nsamp': samples per utterance,
  'sig_offs': {key: [offset of utterance j's signal in flat]}}.  A batch that carries 'rate' / 'target_rate' with a signal at
  another rate is resampled on the device first (sk_resample): 'flat' and 'nsamp' are then the float32 signals and their
  counts at the target rate, which is what the loss scores against.  The magnitudes are the same sk_stft launches as
  features_from_pcm's (bit-identical network input); source_mags=False skips the sources' (a waveform loss does not read
  them; the list is then empty)."""
  import torch
  from . import ops
  from .packing import Packing
  pcm, src, flat, ns = _staged(pcm, dev)                # resampled: float32 signals and their counts from here on
  B, F = len(ns), 257
  pk = Packing.from_lens([1 + n // 128 for n in ns], dev)
  if pk.perm is not None:
    raise ValueError("wave_features_from_pcm: the batch must be sorted by frame count, longest first (WavCollator does)")
  total = sum(ns)
  grid = dict(lengths=ns, out_offs=[b * F for b in range(B)], stride_t=[B * F] * B, stride_f=[1] * B)
  feats = []
  for q, _ in enumerate(signal_keys(pcm['keys']) if source_mags else pcm['keys'][:1]):
    out = torch.zeros(pk.T, B, F, device=dev)
    ops.stft_batch(flat[q * total:(q + 1) * total], out=out, **grid)
    feats.append(pk.pack(out))
  outc = torch.zeros(pk.T, B, F, dtype=torch.complex64, device=dev)
  ops.stft_batch(flat[:total], want_complex=True, out=outc, **grid)
  mixc = torch.view_as_complex(pk.pack(torch.view_as_real(outc).view(pk.T, B, 2 * F)).view(-1, F, 2))
  src.record_stream(torch.cuda.current_stream(dev))
  flat.record_stream(torch.cuda.current_stream(dev))
  wave = {'mixc': mixc, 'flat': flat, 'nsamp': ns,
          'sig_offs': dict(zip(pcm['keys'], key_offsets(ns, range(len(pcm['keys'])))))}
  return feats[0], feats[1:], pk, wave


PSA_TARGETS = ('psa', 'tpsa')        # Prefetcher(targets=...) / archs/uPIT.py's loss conf key: the target as it is / held to [0, |Y|]


def psa_features_from_pcm(pcm, dev, clamp=False):
  """features_from_pcm for the phase-sensitive losses (archs/uPIT.py, loss=psa / tpsa; sepkern/psa.py): the same batch ->
  (mix (Rp,F), [target (Rp,F)...], Packing), the mixture's magnitude rows (bit for bit features_from_pcm's: the network's input
  does not depend on the loss) and, where features_from_pcm returns the sources' magnitudes, their phase-sensitive targets
  Re(S_s conj Y) / |Y| (clamp: held to [0, |Y|]).  ONE launch, sk_stft_psa, writes the packed rows: no (T,B,F) grid, no pack, no
  source spectrum in memory.  A batch that carries 'rate' / 'target_rate' with a signal at another rate is resampled on the
  device first (sk_resample).  Everything is enqueued on the CURRENT stream."""
  import torch
  from . import ops
  from .packing import Packing
  pcm, src, flat, ns = _staged(pcm, dev)                # (another tensor only when a signal had to be resampled)
  nk = len(signal_keys(pcm['keys']))
  if nk < 2:
    raise ValueError("psa_features_from_pcm: the batch holds no source waveform")
  pk = Packing.from_lens([1 + n // 128 for n in ns], dev)
  if pk.perm is not None:
    raise ValueError("psa_features_from_pcm: the batch must be sorted by frame count, longest first (WavCollator does)")
  mix, targets = ops.stft_psa(flat, key_offsets(ns, range(nk)), ns, nk - 1, pk=pk, clamp=clamp)
  src.record_stream(torch.cuda.current_stream(dev))
  flat.record_stream(torch.cuda.current_stream(dev))
  return mix, targets, pk


def ipd_rows_from_pcm(pcm, dev, front=features_from_pcm, **front_args):
  """An array batch (WavTrainSet with ipd_channels: pcm['keys'] ends in 'chan<c>' keys, the mixture's listed channels) ->
  (what `front` -- one of the front ends above -- returns for it, wide): wide (Rp, ld) = the input rows of an IPD model,
  [ |Y_ref| | cos_1 | sin_1 | ... ] (sepkern/ipd.py) with the listed channels in the order of the batch's keys, made from
  the PCM by ONE sk_stft_ipd launch; ld = the width rounded up to 16, zero columns behind the features, rows R.. zero: the
  engine takes them as they are.  The samples cross to the device and are resampled (a batch with 'rate' / 'target_rate') once,
  for both.  `front` sees what it sees for the mono batch of the reference channel, so its mixture rows -- which the loss
  kernels read -- are bit for bit the magnitude columns of wide.  Everything is enqueued on the CURRENT stream."""
  import torch
  from . import ops
  from .ipd import chan_keys
  if 'mixing' in pcm:                    # simulated rooms with listed channels: mixed first (_staged), an array batch from there on
    if not batch_chan_keys(pcm):
      raise ValueError("ipd_rows_from_pcm: a batch mixed on the device (--dynamic-mix) has one channel")
  elif not chan_keys(pcm['keys']) or pcm['keys'][0] != 'mix':
    raise ValueError("ipd_rows_from_pcm: the batch holds no 'chan<c>' signals behind 'mix' (got %r)" % list(pcm['keys']))
  pcm, src, flat, ns = _staged(pcm, dev)
  keys = list(pcm['keys'])
  res = front({'flat': flat, 'keys': keys, 'lens': ns}, dev, **front_args)
  wide, _ = ops.stft_ipd(flat, key_offsets(ns, [keys.index(k) for k in ['mix'] + chan_keys(keys)]), ns, pk=res[2], want_mix=False)
  src.record_stream(torch.cuda.current_stream(dev))
  flat.record_stream(torch.cuda.current_stream(dev))
  return res, wide


# ----------------------------------------------------------------------------------------------- staging ahead of the step
class Prefetcher:
  """Iterates a DataLoader of the arch's batches and hands them over ALREADY ON THE GPU, as packed rows.

  The reference's loop (steps/train_qsub.py:113-122 over archs/uPIT.py:66-79,160-167) inflates the npz files, packs
  and copies every batch to the GPU synchronously in front of the step that consumes it.  At 36 ms per step that host
  work is the bound, so here a background thread takes the batches from the loader (whose workers inflate and pack in
  parallel), stages them through pinned memory and copies them on its own HIP stream, `depth` batches ahead:
    * PackedSequence batches (TrainSet): PackedSequence.data IS the engine's row layout -- one pinned copy + one
      asynchronous H2D per key, no padding anywhere; the batch arrives as {'packed': (mix, [sources], Packing)};
    * PCM batches (WavTrainSet, --wav-input): the int16 samples are copied and the STFT runs on the copy stream too
      (DynMixTrainSet, --dynamic-mix: the copy holds the sources only and the mixing runs there as well, mixed_pcm).
  The consumer's stream waits for the batch's event; nothing on the host blocks.  Everything else in a batch (names,
  ...) passes through untouched.
  keep_wave (PCM batches only): the staged batch also carries 'wave' -- the mixture's complex rows and the device PCM
  (wave_features_from_pcm) -- for a loss that works on waveforms; the sources' magnitudes are then not computed.
  targets ('psa' or 'tpsa'; PCM batches only): the staged 'packed' batch carries the sources' phase-sensitive targets
  (psa_features_from_pcm; 'tpsa': held to [0, |Y|]) where it would carry their magnitudes."""

  _END = object()

  def __init__(self, loader, device, depth=2, keep_wave=False, targets=None):
    import queue
    import threading
    self.loader, self.device, self.depth, self.keep_wave = loader, device, max(1, int(depth)), bool(keep_wave)
    self.targets = self._targets_kind(targets)
    if self.targets and self.keep_wave:
      raise ValueError("Prefetcher: keep_wave and targets belong to different losses; give one of them")
    self._queue_mod, self._threading = queue, threading
    self._stuck = None          # a staging thread that did not end when its consumer left early

  def __len__(self):
    return len(self.loader)

  def __iter__(self):
    import torch
    if self._stuck is not None:
      if self._stuck.is_alive():
        raise RuntimeError("Prefetcher: the staging thread of an earlier, abandoned pass is still inside the loader; "
                           "two threads must not share one loader iterator")
      self._stuck = None
    # The loader's iterator is made HERE, in the consumer's thread (with persistent workers: the worker processes are
    # started -- forked -- from this thread, not from a side thread of a process that holds the GPU, and a new pass
    # resets the same iterator only after the previous pass's thread is known to have left it).
    it = iter(self.loader)
    q = self._queue_mod.Queue(maxsize=self.depth)
    stop = self._threading.Event()
    dev = torch.device(self.device)
    stream = torch.cuda.Stream(device=dev)

    def put(item):
      while not stop.is_set():
        try:
          q.put(item, timeout=0.1)
          return True
        except self._queue_mod.Full:
          continue
      return False

    timing = os.environ.get("SEPKERN_PREFETCH_TIMING") == "1"      # diagnostic: where the staging thread's time goes
    acc = {"loader": 0.0, "stage": 0.0, "queue": 0.0, "n": 0}

    def work():
      try:
        torch.cuda.set_device(dev)
        with torch.cuda.stream(stream):
          while True:
            t0 = time.perf_counter()
            try:
              batch = next(it)
            except StopIteration:
              break
            t1 = time.perf_counter()
            staged = self.stage(batch, dev, self.keep_wave, self.targets)
            ev = torch.cuda.Event()
            ev.record(stream)
            if timing:
              ev.synchronize()
            t2 = time.perf_counter()
            if not put((staged, ev)):
              return
            t3 = time.perf_counter()
            acc["loader"] += t1 - t0; acc["stage"] += t2 - t1; acc["queue"] += t3 - t2; acc["n"] += 1
        put(self._END)
        if timing and acc["n"]:
          print("prefetch: per batch %.1f ms waiting for the loader, %.1f ms staging (incl. the copies), %.1f ms waiting for "
                "the consumer" % tuple(1e3 * acc[k] / acc["n"] for k in ("loader", "stage", "queue")), file=sys.stderr, flush=True)
      except BaseException as e:          # re-raised in the consumer
        put(e)

    th = self._threading.Thread(target=work, name="sepkern-prefetch", daemon=True)
    th.start()
    try:
      while True:
        item = q.get()
        if item is self._END:
          break
        if isinstance(item, BaseException):
          raise item
        staged, ev = item
        cur = torch.cuda.current_stream(dev)
        cur.wait_event(ev)
        for t in self._tensors(staged):
          t.record_stream(cur)             # allocated on the copy stream's pool, consumed on this one
        yield staged
    finally:
      # (normal end: the thread has put _END and is gone.  Early exit -- an exception in the step, a break: it may be
      # blocked in next(it); it returns as soon as the loader hands over that batch, finds `stop` set and leaves.)
      stop.set()
      th.join(timeout=60)
      if th.is_alive():
        self._stuck = th

  @staticmethod
  def _tensors(staged):
    p = staged.get('packed') if isinstance(staged, dict) else None      # (other batch types pass through as they came)
    if p is not None:
      yield p[0]
      for s in p[1]:
        yield s
      yield p[2].lens              # (lens / offs / perm are views of one staging tensor)
    w = staged.get('wave') if isinstance(staged, dict) else None
    if w is not None:
      yield w['mixc']
      yield w['flat']
    x = staged.get('ipd') if isinstance(staged, dict) else None
    if x is not None:
      yield x

  @staticmethod
  def _targets_kind(targets):
    if targets is not None and targets not in PSA_TARGETS:
      raise ValueError("Prefetcher(targets=%r): None, %s" % (targets, " or ".join(repr(t) for t in PSA_TARGETS)))
    return targets

  @staticmethod
  def stage(batch, dev, keep_wave=False, targets=None):
    """One batch -> {'packed': (mix (R,F), [source (R,F)...], Packing), <other keys unchanged>} on `dev`, enqueued on the
    CURRENT stream.  keep_wave: a PCM batch also gets 'wave' (wave_features_from_pcm; no source magnitudes); a batch that
    holds no PCM cannot, which is an error here rather than at the loss.  targets ('psa' / 'tpsa'): a PCM batch's 'packed' holds
    phase-sensitive targets in place of the source magnitudes (psa_features_from_pcm); a batch without PCM is again an error.
    An array batch (its PCM carries 'chan<c>' signals: WavTrainSet with ipd_channels) also gets 'ipd' -- the wide input rows of
    an IPD model (ipd_rows_from_pcm) -- and 'ipd_keys', the channels they were made of, in order."""
    import torch
    from torch.nn.utils.rnn import PackedSequence
    from .packing import Packing
    targets = Prefetcher._targets_kind(targets)
    if not isinstance(batch, dict):
      return batch
    if 'pcm' in batch:                   # WavCollator: {'pcm': {'flat': int16 tensor, 'keys', 'lens'}}: one pinned copy, STFT here
      pcm = batch['pcm']
      host = pcm['flat'] if pcm['flat'].is_pinned() else pcm['flat'].pin_memory()
      out = {k: v for k, v in batch.items() if k != 'pcm'}
      if keep_wave:
        front, front_args = wave_features_from_pcm, dict(source_mags=False)
      elif targets:
        front, front_args = psa_features_from_pcm, dict(clamp=targets == 'tpsa')
        out['targets'] = targets         # (says what 'packed' holds in place of the source magnitudes)
      else:
        front, front_args = features_from_pcm, {}
      if batch_chan_keys(pcm):           # an array batch: the IPD model's wide input rows are made here too
        res, out['ipd'] = ipd_rows_from_pcm(dict(pcm, flat=host), dev, front, **front_args)
        out['ipd_keys'] = batch_chan_keys(pcm)
      else:
        res = front(dict(pcm, flat=host), dev, **front_args)
      mix, sources, pk = res[:3]
      if keep_wave:
        out['wave'] = res[3]
      out['packed'] = (mix, sources, pk)
      out['_keepalive'] = host
      return out
    if keep_wave:
      raise ValueError("Prefetcher(keep_wave=True) needs PCM batches (WavTrainSet / --wav-input): this batch holds no waveforms")
    if targets:
      raise ValueError("Prefetcher(targets=%r) needs PCM batches (WavTrainSet / --wav-input): this batch holds no waveforms" % targets)
    seqs = {k: v for k, v in batch.items() if isinstance(v, PackedSequence)}
    if 'mix' not in seqs:
      return batch
    pk = Packing.from_batch_sizes(seqs['mix'].batch_sizes, dev)
    order = ['mix'] + sorted((k for k in seqs if k.startswith('source')), key=lambda k: int(k[6:]))
    hosts, devs = [], []
    for k in order:
      h = seqs[k].data.pin_memory()
      hosts.append(h)
      devs.append(h.to(dev, non_blocking=True))
    out = {k: v for k, v in batch.items() if k not in seqs}
    out['packed'] = (devs[0], devs[1:], pk)
    out['_keepalive'] = hosts               # pinned staging must outlive the asynchronous copies
    return out
