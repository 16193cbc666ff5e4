"""Short-time objective intelligibility: STOI (Taal, Hendriks, Heusdens & Jensen 2011) and its extended form ESTOI
(Jensen & Taal 2016), defined once.  The kernels (csrc/stoi.hip, sk_stoi) and the scoring CLIs compute exactly this.

UNPINNED: neither pystoi nor any other implementation is installed where this project is built, and the reference project has
none, so everything below restates the two papers (and the authors' Matlab framing rule), not a package's output -- exactly as
sepkern/resample.py restates resampy and oracle/stft.py librosa.  What IS pinned (tests/test_stoi.py, tests/test_gpu_stoi.py):
the band table, identity, gain invariance, the short-utterance value, the silent-frame count against a direct computation,
the score of independent sources, and the kernels against this file.

All of it works on signals at FS = 10 kHz (other rates are resampled first, sepkern/resample.py).

    frame 256 samples, hop 128, FFT 512; 15 one-third-octave bands from 150 Hz; segments of N = 30 frames;
    beta = -15 dB (the clipping bound of STOI), 40 dB dynamic range (silent frames); EPS = float64 epsilon;
    w = np.hanning(258)[1:-1], i.e. w[i] = 0.5 (1 - cos(2 pi (i + 1) / 257)), i = 0..255

Framing.  A signal of n samples has frames at starts range(0, n - 256, 128): the end is EXCLUSIVE (the original Matlab
1:K:(length(x)-N)), so n <= 256 has no frame and n = 257 one.

Silent frames, decided by the reference alone, always in float64:  e_i = 20 log10(|w * frame_i|_2 + EPS); frame i is kept
iff e_i > max_i e_i - 40.  A reference without a frame, or one whose every frame is exactly zero, keeps NO frame (the rule
alone would keep all of an all-zero signal's).  The same frame indices are kept in the estimate.  Both signals are rebuilt by
overlap-add of the kept WINDOWED frames at hop 128: (n_kept - 1) 128 + 256 samples.

Band envelopes.  The rebuilt signals are framed again by the same rule -- T = n_kept - 1 frames (0 when nothing is kept) --
windowed again with w, zero-padded to 512; X[b][t] = sqrt(sum over bins [lo_b, hi_b) of |rFFT|^2), 15 x T.  With
f = linspace(0, 10000, 513)[:257], lo_b / hi_b is the bin nearest to 150 2^((2b-1)/6) / 150 2^((2b+1)/6): BAND_EDGES.

Segments.  J = T - 29 segments, frames [m, m + 30) of X (reference) and Y (estimate).
  STOI   per band row: c = |x| / (|y| + EPS), y' = min(c y, x (1 + 10^(15/20))); both rows minus their mean, divided by
         (their norm + EPS); d = sum x~ y~' / (15 J).
  ESTOI  rows normalised (mean, then norm + EPS), then columns the same way; d = sum x~ y~ / (30 J).
T < 30: both scores are SHORT = 1e-5, the customary "not enough frames" value; the T that is returned beside them tells.
"""
import itertools

import numpy as np

FS = 10000
N_FRAME = 256
HOP = 128
NFFT = 512
NUM_BANDS = 15
MIN_FREQ = 150.0
N_SEG = 30
BETA = -15.0
DYN_RANGE = 40.0
EPS = np.finfo(np.float64).eps
SHORT = 1e-5
WINDOW = np.hanning(N_FRAME + 2)[1:-1]


def band_edges():
    """[(lo_b, hi_b)]: band b sums rFFT bins lo_b .. hi_b - 1."""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    b = np.arange(NUM_BANDS, dtype=np.float64)
    lo = MIN_FREQ * 2.0 ** ((2 * b - 1) / 6)
    hi = MIN_FREQ * 2.0 ** ((2 * b + 1) / 6)
    near = lambda v: int(np.argmin(np.square(f - v)))    # noqa: E731
    return tuple((near(l), near(h)) for l, h in zip(lo, hi))


BAND_EDGES = band_edges()


def frame_starts(n):
    return np.arange(0, int(n) - N_FRAME, HOP, dtype=np.int64)


def _frames(x):
    """(F, 256) view-like array of the frames of x (F may be 0)."""
    s = frame_starts(len(x))
    return x[s[:, None] + np.arange(N_FRAME)[None, :]] if len(s) else np.zeros((0, N_FRAME), x.dtype)


def frame_energies_db(ref):
    """e_i of every frame of the reference, float64."""
    fr = _frames(np.asarray(ref, dtype=np.float64))
    return 20.0 * np.log10(np.linalg.norm(fr * WINDOW, axis=1) + EPS)


def kept_frames(ref):
    """Indices of the frames the silent-frame rule keeps (float64)."""
    fr = _frames(np.asarray(ref, dtype=np.float64))
    norms = np.linalg.norm(fr * WINDOW, axis=1)
    if len(norms) == 0 or not norms.max() > 0.0:
        return np.zeros(0, dtype=np.int64)
    e = 20.0 * np.log10(norms + EPS)
    return np.nonzero(e > e.max() - DYN_RANGE)[0]


def keep_margins(ref):
    """e_i - (max_i e_i - 40) of every frame, in dB: positive = kept.  A test asserts with it that none of its frames sits so
    close to the threshold that rounding could decide."""
    e = frame_energies_db(ref)
    return e - (e.max() - DYN_RANGE) if len(e) else e


def _rebuild(x, kept, w):
    """Overlap-add of the kept windowed frames of x at hop 128, in x's dtype."""
    out = np.zeros((len(kept) - 1) * HOP + N_FRAME if len(kept) else 0, dtype=x.dtype)
    for i, k in enumerate(kept):
        out[i * HOP:i * HOP + N_FRAME] += w * x[k * HOP:k * HOP + N_FRAME]
    return out


def _rfft(a):
    """rFFT along the last axis in a's own precision (numpy's pocketfft keeps float32; scipy's does too)."""
    return np.fft.rfft(a, n=NFFT, axis=-1)


def envelopes(x, kept, dtype=np.float64):
    """(15, T) band envelopes of x under the kept-frame list, everything in `dtype`."""
    x = np.asarray(x, dtype=dtype)
    w = WINDOW.astype(dtype)
    fr = _frames(_rebuild(x, kept, w)) * w
    spec = _rfft(fr)
    if spec.dtype != (np.complex64 if dtype == np.float32 else np.complex128):
        spec = spec.astype(np.complex64 if dtype == np.float32 else np.complex128)
    p = (spec.real * spec.real + spec.imag * spec.imag).astype(dtype)          # (T, 257)
    return np.stack([np.sqrt(p[:, lo:hi].sum(axis=1, dtype=dtype)) for lo, hi in BAND_EDGES]).astype(dtype)


def _segments(X):
    """(J, 15, 30): segment m = frames [m, m + 30)."""
    J = X.shape[1] - N_SEG + 1
    return np.stack([X[:, m:m + N_SEG] for m in range(J)])


def _norm_rows(a, eps):
    a = a - a.mean(axis=-1, keepdims=True)
    return a / (np.sqrt((a * a).sum(axis=-1, keepdims=True)) + eps)


def scores(X, Y):
    """(stoi, estoi) of two (15, T) envelope arrays, in their dtype; T < 30 -> (SHORT, SHORT)."""
    T = X.shape[1]
    if T < N_SEG:
        return SHORT, SHORT
    dt = X.dtype.type
    eps = dt(EPS)
    xs, ys = _segments(X), _segments(Y)
    J = xs.shape[0]
    # STOI
    c = np.sqrt((xs * xs).sum(axis=-1, keepdims=True)) / (np.sqrt((ys * ys).sum(axis=-1, keepdims=True)) + eps)
    yp = np.minimum(c * ys, xs * dt(1.0 + 10.0 ** (-BETA / 20.0)))
    d = float((_norm_rows(xs, eps) * _norm_rows(yp, eps)).sum(dtype=X.dtype) / dt(NUM_BANDS * J))
    # ESTOI
    xr, yr = _norm_rows(xs, eps), _norm_rows(ys, eps)
    xc = np.swapaxes(_norm_rows(np.swapaxes(xr, 1, 2), eps), 1, 2)
    yc = np.swapaxes(_norm_rows(np.swapaxes(yr, 1, 2), eps), 1, 2)
    e = float((xc * yc).sum(dtype=X.dtype) / dt(N_SEG * J))
    return d, e


def _at_10k(x, fs):
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError("stoi: one-dimensional signals only")
    if int(fs) == FS:
        return x
    from . import resample
    return resample.resample_host(x, fs, FS)


def stoi_pair(ref, est, fs=FS, dtype=np.float64):
    """(stoi, estoi, T) of one estimate against one reference.  The silent-frame decision is taken in float64; dtype=np.float32
    evaluates everything after it in float32 (the tests measure the float32 error of this very definition with it)."""
    ref, est = _at_10k(ref, fs), _at_10k(est, fs)
    if len(ref) != len(est):
        raise ValueError("stoi: reference and estimate differ in length (%d, %d)" % (len(ref), len(est)))
    kept = kept_frames(ref)
    X, Y = envelopes(ref, kept, dtype), envelopes(est, kept, dtype)
    d, e = scores(X, Y)
    return d, e, X.shape[1]


def stoi_host(ref, est, fs=FS, extended=False, dtype=np.float64):
    """STOI (extended=False) or ESTOI of `est` against `ref`, both at fs Hz (resampled to 10 kHz by resample.resample_host when
    fs != 10000).  1e-5 when the reference has fewer than 30 frames after silent-frame removal."""
    d, e, _ = stoi_pair(ref, est, fs, dtype)
    return e if extended else d


def stoi_matrix(refs, ests, fs=FS, dtype=np.float64):
    """(out (S, S, 2), frames (S,)): out[k][j] = (STOI, ESTOI) of estimate k against reference j -- sk_stoi's layout."""
    refs = [_at_10k(r, fs) for r in refs]
    ests = [_at_10k(e, fs) for e in ests]
    S = len(refs)
    out, frames = np.zeros((S, S, 2)), np.zeros(S, dtype=np.int32)
    for j in range(S):
        kept = kept_frames(refs[j])
        X = envelopes(refs[j], kept, dtype)
        frames[j] = X.shape[1]
        for k in range(S):
            out[k, j] = scores(X, envelopes(ests[k], kept, dtype))
    return out, frames


def select(mat, frames, compute_permutation=True):
    """(stoi[S], estoi[S], perm, frames[S]) from the (S, S, 2) matrix: the permutation with the highest mean STOI, the first
    maximum in itertools.permutations order (bsseval_gpu.select's convention: perm[j] = estimate given to source j); ESTOI is
    reported under that same assignment."""
    S = mat.shape[0]
    cols = np.arange(S)
    if not compute_permutation:
        return mat[cols, cols, 0].copy(), mat[cols, cols, 1].copy(), cols, np.asarray(frames).copy()
    best, best_mean = None, None
    for perm in itertools.permutations(range(S)):
        mean = np.mean([mat[perm[j], j, 0] for j in range(S)])
        if best is None or mean > best_mean:
            best, best_mean = perm, mean
    rows = np.array(best)
    return mat[rows, cols, 0], mat[rows, cols, 1], rows, np.asarray(frames).copy()


def stoi_sources(refs, ests, fs=FS, compute_permutation=True):
    """The host form of stoi_gpu.stoi_batch for one utterance: refs / ests (S, n) -> (stoi[S], estoi[S], perm, frames[S])."""
    mat, frames = stoi_matrix(list(refs), list(ests), fs)
    return select(mat, frames, compute_permutation)
