"""Cases, float64 references, float32 error models and defect models of the STFT / iSTFT kernel tests.

tests/test_gpu_stft_family.py compares stft_kernel, istft_kernel, istft_rows_kernel and stft_psa_kernel (csrc/stft.hip) with
the float64 references below at the lengths their tile loops branch on; tests/test_stft_cases.py proves on any machine
that the cases can tell a wrong kernel from a right one.

Tolerance of a compared frame (forward: its 257 bins) or hop (inverse: its 128 output samples) q:
    err(q) <= K[family] * E_ref(q) + ulp32(max |ref(q)|)
  E_ref  the largest error in q against float64 of the same formula evaluated in float32 on the CPU (np.fft on float32
         input computes in single precision; the result's dtype is asserted),
  K      twice the largest ratio (err - ulp) / E_ref measured per family on the MI355X, rounded up (cap 8):
         profiles/stft_family.txt.
"""
import functools

import numpy as np

from oracle import stft as OS

F32, F64, C64, C128 = np.float32, np.float64, np.complex64, np.complex128

# loop bounds of the kernels (the constants the shapes are chosen against)
NFFT, HOP, NBIN = 512, 128, 257
FPB = 16                        # fft512.h: frames (forward) / hops (inverse) per tile
TPB = 5                         # fft512.h: tiles one STFT workgroup walks
SPAN = NFFT + (FPB - 1) * HOP   # stft.hip: samples one forward tile loads
RING = FPB + 3                  # stft.hip: row slots of the iSTFT ring

# k per family: twice the largest measured ratio, rounded up (profiles/stft_family.txt)
# measured maxima: stft_complex 3.84, stft_mag 3.13 (the approximate square root), istft 1.66, istft_rows 1.56
K = {"stft_complex": 8, "stft_mag": 7, "istft": 4, "istft_rows": 4}

WIN = OS.hann_periodic(NFFT)                    # float32, as the kernels' table
WIN64 = WIN.astype(F64)

FWD_DEFECTS = ("sym_right", "sym_left", "zeros_right", "raw_next", "stale_tile", "swap_bins", "no_bin128")
INV_DEFECTS = ("no_prelude", "stale_slot", "full_wss_edge", "no_tail", "next_mask", "swap_pair")


# ------------------------------------------------------------------------------------------------ launch geometry
def num_frames(N):
    return 1 + N // HOP


def fast_tile(N, tile):
    """stft_kernel's fetch(): the whole span of `tile` lies inside the utterance (no reflect / clamp arithmetic)."""
    first = tile * FPB * HOP - NFFT // 2
    return first >= 0 and first + SPAN <= N


def stft_tiles(T):
    """Per workgroup of one utterance, the tiles it transforms."""
    nt = -(-T // FPB)
    return [list(range(t0, min(t0 + TPB, nt))) for t0 in range(0, nt, TPB)]


def istft_ntiles(T):
    return T // FPB + 1          # hops 0 .. T carry output samples


def istft_tpb(max_frames, nutt, S):
    """sk_mask_istft / sk_mask_istft_rows: tiles one workgroup walks."""
    ntiles = istft_ntiles(max_frames)
    return int(min(max(ntiles * nutt * S // 2048, 2), ntiles))


def istft_workgroups(T, tpb):
    """[tile0, tile1) of every workgroup that works on a signal of T frames."""
    nt = istft_ntiles(T)
    return [(t0, min(nt, t0 + tpb)) for t0 in range(0, nt, tpb)]


# ------------------------------------------------------------------------------------------------ error measures
def ulp32(v):
    return np.spacing(np.asarray(v, F64).astype(F32)).astype(F64)


def unit_err(got, ref):
    """Largest absolute difference per frame / hop (rows of a 2-D array); a non-finite result counts as infinite."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.ndim == 2, (got.shape, ref.shape)
    d = np.abs(got - ref)
    d = np.where(np.isfinite(d), d, np.inf)
    return d.max(axis=1)


def tolerance(family, ref, e_ref):
    """Per frame / hop: K * E_ref + one float32 ulp of its largest reference value."""
    return K[family] * np.asarray(e_ref, F64) + ulp32(np.abs(ref).max(axis=1))


def needed_k(err, ref, e_ref):
    """Per frame / hop the smallest k with err <= k * E_ref + ulp (inf: no k does)."""
    over = np.asarray(err, F64) - ulp32(np.abs(ref).max(axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(over <= 0, 0.0, np.where(np.asarray(e_ref) > 0, over / e_ref, np.inf))
    return k


# ------------------------------------------------------------------------------------------------ inputs
def noise(n, seed):
    return (np.random.default_rng(seed).standard_normal(n) * 0.2).astype(F32)


def pcm(n, seed):
    return np.random.default_rng(seed).integers(-20000, 20001, n).astype(np.int16)


# ------------------------------------------------------------------------------------------------ forward: samples -> frames
def padded(y, defect=None):
    """The centred signal: n_fft/2 reflected samples on both sides (oracle/stft.py: np.pad(mode='reflect'))."""
    y = np.asarray(y, F32)
    N = y.shape[0]
    left = y[0:256][::-1] if defect == "sym_left" else y[1:257][::-1]
    right = y[N - 257:N - 1][::-1]
    if defect == "sym_right":
        right = y[N - 256:N][::-1]
    elif defect == "zeros_right":
        right = np.zeros(256, F32)
    return np.concatenate([left, y, right])


def windowed_frames(y, defect=None, nxt=None):
    """(T, 512) float32: sample * window, the float32 product of oracle/stft.py.  Defects: see stft_eval."""
    y = np.asarray(y, F32)
    N, T = y.shape[0], num_frames(y.shape[0])
    ypad = padded(y, defect)
    idx = np.arange(NFFT)[None, :] + HOP * np.arange(T)[:, None]
    raw = ypad[idx]
    if defect == "raw_next":                    # tiles past the first read memory as it lies: the next utterance follows
        mem = np.concatenate([y, np.asarray(nxt, F32)[:NFFT]])
        for t in range(FPB, T):
            raw[t] = mem[t * HOP - NFFT // 2:t * HOP + NFFT // 2]
    elif defect == "stale_tile":                # a tile the workgroup prefetched and never stashed: the tile before it again
        for t in range(FPB, T):
            if (t // FPB) % TPB != 0:
                raw[t] = ypad[idx[t - FPB]]
    return raw * WIN[None, :]


def stft_eval(y, dt=F64, defect=None, nxt=None):
    """(T, 257) spectrum of y as oracle/stft.py defines it, the transform in dtype dt (complex128 / complex64).
    defect: right / left padding symmetric instead of reflected, zeros past N, raw memory past N (nxt: what follows), a
    tile transformed from the tile before, bins k and 256 - k swapped, bin 128 not written."""
    fr = windowed_frames(y, defect, nxt)
    if dt is F64:
        spec = np.fft.rfft(fr.astype(F64), axis=1)
    else:
        spec = np.fft.rfft(fr, axis=1)
        assert spec.dtype == C64, "np.fft.rfft of float32 frames is not single precision here: %s" % spec.dtype
    if defect == "swap_bins":
        spec = spec[:, ::-1].copy()
    elif defect == "no_bin128":
        spec = spec.copy()
        spec[:, 128] = 0
    return spec


def fwd_ref(y):
    """-> (ref (T, 257) complex128, per-frame E_ref of the complex bins, per-frame E_ref of the magnitudes, frame norms)."""
    ref = stft_eval(y, F64)
    s32 = stft_eval(y, F32)
    e_c = unit_err(s32.astype(C128), ref)
    e_m = unit_err(np.abs(s32).astype(F64), np.abs(ref))
    norms = np.sqrt((windowed_frames(y).astype(F64) ** 2).sum(axis=1))
    return ref, e_c, e_m, norms


def fwd_defects(N):
    T = num_frames(N)
    return [d for d in FWD_DEFECTS if T > FPB or d not in ("raw_next", "stale_tile")]


# N: the boundary it sits on
FWD_LENGTHS = [257,                      # shortest allowed, 3 frames
               383, 384, 385,            # N mod 128 = 127, 0, 1 at the right-hand reflection: 3 / 4 / 4 frames
               1920, 2047, 2048, 2175,   # 16 / 16 / 17 / 17 frames: the tile boundary
               4223, 4224,               # 33 / 34 frames: tile 1 takes the reflect path / the whole-tile fast path
               10112, 10240, 10367,      # 80 / 81 / 81 frames: the workgroup boundary
               12288]                    # 97 frames: the second workgroup takes two tiles, a prefetch inside it
FWD_FRAMES = [3, 3, 4, 4, 16, 16, 17, 17, 33, 34, 80, 81, 81, 97]
FWD_ORDER = [int(i) for i in np.random.default_rng(2024).permutation(len(FWD_LENGTHS))]     # positions in the launch


def check_forward_claims():
    """What the forward cases claim about the kernel's loop bounds; a constant that moved fails here."""
    assert SPAN == 2432 and FPB * TPB == 80
    assert [num_frames(n) for n in FWD_LENGTHS] == FWD_FRAMES
    assert [n % HOP for n in (383, 384, 385)] == [127, 0, 1]
    assert fast_tile(4224, 1) and not fast_tile(4223, 1) and not fast_tile(4224, 2) and not fast_tile(4224, 0)
    assert stft_tiles(16) == [[0]] and stft_tiles(17) == [[0, 1]]
    assert stft_tiles(80) == [[0, 1, 2, 3, 4]] and stft_tiles(81) == [[0, 1, 2, 3, 4], [5]]
    assert stft_tiles(97) == [[0, 1, 2, 3, 4], [5, 6]]
    # 12288: tiles 1 .. 4 are fast-path tiles, the second workgroup's 5 and 6 are not; 10367 is one sample short for tile 4
    assert all(fast_tile(12288, t) for t in (1, 2, 3, 4)) and not fast_tile(12288, 5) and not fast_tile(12288, 6)
    assert fast_tile(10367, 3) and not fast_tile(10367, 4) and fast_tile(10368, 4)
    assert FWD_ORDER != sorted(FWD_ORDER) and sorted(FWD_ORDER) == list(range(len(FWD_LENGTHS)))
    # the launch is sized by its longest utterance: two workgroups per utterance, the second leaves at once for most
    assert -(-max(FWD_FRAMES) // (FPB * TPB)) == 2


@functools.lru_cache(maxsize=None)
def fwd_case(fmt):
    """The forward launch: fmt 'float32' (white noise of std 0.2) or 'int16' (integers in +-20000).  -> dict: raw (what the
    kernel gets, per utterance), y (the float32 signals), order (launch position -> utterance), ref / e_c / e_m / norms per
    utterance.  Computed once, shared, never written to."""
    check_forward_claims()
    if fmt == "int16":
        raw = [pcm(n, 7000 + n) for n in FWD_LENGTHS]
        y = [OS.pcm16_to_float(p) for p in raw]
    else:
        raw = [noise(n, n) for n in FWD_LENGTHS]
        y = raw
    refs = [fwd_ref(v) for v in y]
    return dict(raw=raw, y=y, order=FWD_ORDER, ref=[r[0] for r in refs], e_c=[r[1] for r in refs], e_m=[r[2] for r in refs],
                norms=[r[3] for r in refs])


def fwd_next(case, u):
    """The samples that follow utterance u in the launch's buffer (after the last one: noise)."""
    pos = case["order"].index(u)
    return case["y"][case["order"][pos + 1]] if pos + 1 < len(case["order"]) else noise(NFFT, 99)


# ------------------------------------------------------------------------------------------------ inverse: frames -> samples
def masked(X, mask):
    """Mask product rounded to complex64, as oracle/stft.py's reconstruct (np.multiply of complex64 and float32)."""
    X = np.asarray(X, C64)
    return X if mask is None else np.multiply(X, np.asarray(mask, F32)).astype(C64)


def istft_eval(X, dt=F64, defect=None, tpb=2):
    """(T - 1, 128): the retained hops 2 .. T of librosa's istft of the (T, 257) complex64 spectrum X, every step after the
    mask product in dtype dt; a hop's four frames are added oldest first.
    defect: the three frames before a workgroup's first tile missing from its hops, the last frame replaced by the frame 19
    before it, the full window-sum-square on the edge hops, the tail tile's hops not written, bins 4 and 5 swapped."""
    X = np.asarray(X, C64)
    T = X.shape[0]
    if defect == "swap_pair":
        X = X.copy()
        X[:, [4, 5]] = X[:, [5, 4]]
    if dt is F64:
        fr = np.fft.irfft(X.astype(C128), n=NFFT, axis=1) * WIN64[None, :]
        wsq = WIN64 * WIN64
    else:
        x = np.fft.irfft(X, n=NFFT, axis=1)
        assert x.dtype == F32, "np.fft.irfft of a complex64 spectrum is not single precision here: %s" % x.dtype
        fr = x * WIN[None, :]
        wsq = WIN * WIN
    if defect == "stale_slot":
        fr = fr.copy()
        fr[T - 1] = fr[T - 1 - RING]
    H = T + 3
    Y, W = np.zeros((H, HOP), fr.dtype), np.zeros((H, HOP), fr.dtype)
    first_tile_of = np.zeros(H, np.int64)                      # first frame of the workgroup that writes the hop
    for t0, t1 in istft_workgroups(T, tpb):
        first_tile_of[t0 * FPB:min(H, t1 * FPB)] = t0 * FPB
    for q in range(3, -1, -1):                                 # hop h = frames h-3 (its last quarter) .. h (its first)
        add = fr[:, q * HOP:(q + 1) * HOP]
        if defect == "no_prelude":
            keep = (np.arange(T) >= first_tile_of[q:q + T])[:, None]
            add = add * keep
        Y[q:q + T] += add
        W[q:q + T] += wsq[None, q * HOP:(q + 1) * HOP]
    if defect == "full_wss_edge":
        full = ((wsq[3 * HOP:] + wsq[2 * HOP:3 * HOP]) + wsq[HOP:2 * HOP]) + wsq[:HOP]
        edge = (np.arange(H) < 3) | (np.arange(H) >= T)
        W[edge] = full[None, :]
    ok = W > np.finfo(F32).tiny
    out = np.where(ok, Y / np.where(ok, W, 1), Y)
    if defect == "no_tail":
        out[(T // FPB) * FPB:] = 0
    return out[2:T + 1]


def inv_ref(X):
    """-> (ref (T - 1, 128) float64, per-hop E_ref, per-hop norms)."""
    ref = istft_eval(X, F64)
    e = unit_err(istft_eval(X, F32).astype(F64), ref)
    return ref, e, np.sqrt((ref ** 2).sum(axis=1))


def inv_defects(T, S, tpb):
    d = ["full_wss_edge", "no_tail", "swap_pair"]
    if len(istft_workgroups(T, tpb)) > 1:
        d.append("no_prelude")
    if T > RING:
        d.append("stale_slot")
    if S > 1:
        d.append("next_mask")
    return d


def inv_spec(T, seed):
    """(T, 257) complex64: the first T frames of the STFT of white noise of std 0.2; the imaginary parts of the DC and the
    Nyquist bin, which an inverse real transform must ignore, hold noise too."""
    X = stft_eval(noise(HOP * (T + 2), seed), F64)[:T].astype(C64)
    g = np.random.default_rng(seed + 1)
    X[:, 0] += 1j * g.standard_normal(T).astype(F32)
    X[:, 256] += 1j * g.standard_normal(T).astype(F32)
    return X


def inv_masks(T, S, seed):
    """(S, T, 257) float32 uniform in (0, 1)."""
    return np.random.default_rng(seed).uniform(0.0, 1.0, (S, T, NBIN)).astype(F32)


INV_FRAMES = [2, 3, 4, 5,            # the first hops: one, two, three taps, then all four
              15, 16, 17,            # the tile boundary: 16 adds a tile that holds no frame
              31, 32, 33, 35,        # 32: a second workgroup whose only tile has no frames, its three-frame prelude
              48, 49]                # a second workgroup of two tiles / whose second tile has one frame
INV_ORDER = [int(i) for i in np.random.default_rng(2025).permutation(len(INV_FRAMES))]
INV_SPEAKERS = [1, 3]                # 1: no mask


def check_inverse_claims():
    assert RING == 19
    for S in INV_SPEAKERS:
        assert istft_tpb(max(INV_FRAMES), len(INV_FRAMES), S) == 2
    wg = lambda T: istft_workgroups(T, 2)    # noqa: E731
    assert wg(2) == wg(15) == [(0, 1)] and wg(16) == wg(17) == wg(31) == [(0, 2)]
    assert wg(32) == wg(33) == wg(35) == [(0, 2), (2, 3)] and wg(48) == wg(49) == [(0, 2), (2, 4)]
    assert INV_ORDER != sorted(INV_ORDER)


@functools.lru_cache(maxsize=None)
def inv_case(S):
    """The inverse launch of unequal T: specs[u] (T, 257) complex64, masks[u] (S, T, 257) or None (S = 1), ref[u][s], e[u][s]."""
    check_inverse_claims()
    specs = [inv_spec(T, 300 + T) for T in INV_FRAMES]
    masks = [inv_masks(T, S, 600 + T) if S > 1 else None for T in INV_FRAMES]
    refs = [[inv_ref(masked(X, None if m is None else m[s])) for s in range(S)] for X, m in zip(specs, masks)]
    return dict(T=INV_FRAMES, order=INV_ORDER, S=S, specs=specs, masks=masks, ref=[[r[0] for r in rs] for rs in refs],
                e=[[r[1] for r in rs] for rs in refs], norms=[[r[2] for r in rs] for rs in refs])


# one launch in which the host chooses four tiles per workgroup
TPB4_NUTT, TPB4_S, TPB4_FRAMES = 256, 4, (130, 97, 33)


@functools.lru_cache(maxsize=None)
def tpb4_frames():
    T = [int(v) for v in np.random.default_rng(4).choice(TPB4_FRAMES, TPB4_NUTT)]
    T[0] = 130                                                 # the launch's longest sizes its tiles
    return T


def tpb4_sample():
    """Six signals' utterances: the first, the last, one of each T in between, one more of the longest."""
    T = tpb4_frames()
    mid = [next(u for u in range(1, TPB4_NUTT - 1) if T[u] == t) for t in TPB4_FRAMES]
    more = max(u for u in range(1, TPB4_NUTT - 1) if T[u] == 130 and u not in mid)
    return [0] + mid + [more, TPB4_NUTT - 1]


def check_tpb4_claims():
    T = tpb4_frames()
    assert max(T) == 130 and istft_ntiles(130) == 9 and set(T) == set(TPB4_FRAMES)
    assert istft_tpb(130, TPB4_NUTT, TPB4_S) == 4
    assert istft_workgroups(130, 4) == [(0, 4), (4, 8), (8, 9)] and istft_workgroups(97, 4) == [(0, 4), (4, 7)]
    assert istft_workgroups(33, 4) == [(0, 3)]
    assert istft_tpb(130, 1, TPB4_S) == 2                      # ... and a signal of it run alone is walked two tiles at a time
    assert len(set(tpb4_sample())) == 6


def tpb4_utt(u):
    """(spec (T, 257), masks (4, T, 257)) of utterance u of the tpb == 4 launch."""
    T = tpb4_frames()[u]
    return inv_spec(T, 9000 + 2 * u), inv_masks(T, TPB4_S, 5000 + u)


# packed rows (sk_mask_istft_rows): frames per utterance, descending as Packing wants them
ROWS_FRAMES = [49, 33, 32, 17, 16, 4, 3, 2]
ROWS_SPEAKERS = [1, 4]
ROWS_PAD = 3                          # mask rows of ld = S * 257 + 3, the padding columns hold NaN


def check_rows_claims():
    for S in ROWS_SPEAKERS:
        assert istft_tpb(max(ROWS_FRAMES), len(ROWS_FRAMES), S) == 2
    assert ROWS_FRAMES == sorted(ROWS_FRAMES, reverse=True) and min(ROWS_FRAMES) == 2     # below two tiles too


@functools.lru_cache(maxsize=None)
def rows_case(S):
    check_rows_claims()
    specs = [inv_spec(T, 800 + T) for T in ROWS_FRAMES]
    masks = [inv_masks(T, S, 900 + T) for T in ROWS_FRAMES]
    refs = [[inv_ref(masked(X, m[s])) for s in range(S)] for X, m in zip(specs, masks)]
    return dict(T=ROWS_FRAMES, S=S, specs=specs, masks=masks, ref=[[r[0] for r in rs] for rs in refs],
                e=[[r[1] for r in rs] for rs in refs])
