"""Band-limited sinc resampling: the arithmetic of the `sr=` half of librosa.core.load, defined once.

Every stage of the reference that opens a wav file does it with librosa.core.load(path, sr=args.sample_rate)
(steps/extract_feats.py:74,85,97,104, steps/evaluate_oracle.py:96,122), which resamples whatever is on disk.  librosa 0.6
delegates that to resampy's `kaiser_best` filter: a Kaiser-windowed sinc with

    num_zeros = 64,  rolloff = 0.9475937167399596,  Kaiser beta = 14.769656459379492

read from a table of 512 samples per zero crossing with linear interpolation between its entries.  Here the same filter is
evaluated EXACTLY at every tap instead of through that table.

UNPINNED: neither resampy nor librosa is installed where this project is built, so the three constants above, the length
rule below (librosa 0.6's resample(..., fix=True)) and the zero extension at both ends are restated from what the two
packages publish, not held to their output -- exactly as oracle/stft.py restates librosa's STFT.  What IS pinned
(tests/test_resample.py): this definition against scipy.signal.upfirdn with the same prototype filter, its DC gain, a tone
in the pass band and a tone above the new Nyquist.

For sr_in -> sr_out:  g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g, rho = L / M, scale = min(1, rho),

    w(t)  = rolloff sinc(rolloff t) I0(beta sqrt(1 - (t / num_zeros)^2)) / I0(beta)   for |t| < num_zeros, else 0
    y[n]  = scale sum_k x[k] w((n M / L - k) scale),   k over the samples that exist (zeros beyond both ends)
    n_out = ceil(n_in sr_out / sr_in)                  in exact integer arithmetic

Output n has phase p = (n M) mod L, so the filter is L rows of

    ntaps = floor(2 num_zeros / scale) + 1 = (2 num_zeros max(L, M)) // L + 1

taps (257 for 16 k -> 8 k, 706 for 44.1 k -> 8 k, 769 for 48 k -> 8 k, 129 for any up-sampling); row p, column i is the
weight -- `scale` included -- of input sample first(n) + i, where

    first(n) = floor((n M - num_zeros max(L, M)) / L) + 1

is the first input sample inside the filter's support (|n M / L - k| < num_zeros / scale): a closed form of n alone.
The kernel (csrc/resample.hip, sk_resample) computes y[n] = sum_i taps[p][i] x[first(n) + i] in fp32, i ascending.
"""
import math

import numpy as np

NUM_ZEROS = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492

_PLANS = {}


def ratio(sr_in, sr_out):
    """(L, M) = (sr_out, sr_in) / gcd."""
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in < 1 or sr_out < 1:
        raise ValueError("sample rates must be positive (got %d -> %d)" % (sr_in, sr_out))
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def out_len(n_in, sr_in, sr_out):
    """ceil(n_in * sr_out / sr_in), exactly."""
    return -((-int(n_in) * int(sr_out)) // int(sr_in))


def window(t):
    """w(t) of the module docstring (fp64), t in units of input samples times `scale`."""
    t = np.asarray(t, dtype=np.float64)
    inside = np.abs(t) < NUM_ZEROS
    arg = np.sqrt(np.clip(1.0 - (t / NUM_ZEROS) ** 2, 0.0, None))
    return np.where(inside, ROLLOFF * np.sinc(ROLLOFF * t) * np.i0(BETA * arg) / np.i0(BETA), 0.0)


class Plan:
    """The filter of one rate pair: L, M, scale, ntaps, half = num_zeros * max(L, M) and taps, the fp64 (L, ntaps) table by
    phase (`scale` included: every row sums to 1 within the filter's stop-band ripple)."""

    def __init__(self, sr_in, sr_out):
        self.sr_in, self.sr_out = int(sr_in), int(sr_out)
        self.L, self.M = ratio(sr_in, sr_out)
        if self.L == self.M:
            raise ValueError("resample plan: %d -> %d Hz is no rate change" % (sr_in, sr_out))
        self.half = NUM_ZEROS * max(self.L, self.M)
        self.ntaps = (2 * self.half) // self.L + 1
        self.scale = min(1.0, self.L / self.M)
        p = np.arange(self.L, dtype=np.int64)[:, None]
        j = self.first_of_phase(p) + np.arange(self.ntaps, dtype=np.int64)[None, :]
        self.taps = self._h(p - j * self.L)                       # h[m], m = p - j L: sample k = q + j of output n = (q L + p) / M
        self._device = {}

    def _h(self, m):
        """The prototype filter at integer m (units of 1 / L input samples): scale * w(m scale / L); zero for |m| >= half."""
        return self.scale * window(np.asarray(m, dtype=np.float64) * (self.scale / self.L))

    def prototype(self):
        """h[-half .. half] (2 half + 1 values): y[n] = sum_k x[k] h[n M - k L] -- what scipy.signal.upfirdn(h, x, up=L)
        evaluates at index n M + half."""
        return self._h(np.arange(-self.half, self.half + 1, dtype=np.int64))

    def first_of_phase(self, p):
        """first(n) - floor(n M / L) for an output of phase p."""
        return (np.asarray(p, dtype=np.int64) - self.half) // self.L + 1

    def first(self, n):
        """Index of the first input sample under the filter of output n (may be negative: zeros there)."""
        return (np.asarray(n, dtype=np.int64) * self.M - self.half) // self.L + 1

    def phase(self, n):
        return (np.asarray(n, dtype=np.int64) * self.M) % self.L

    def out_len(self, n_in):
        return out_len(n_in, self.sr_in, self.sr_out)

    def device_taps(self, device):
        """The fp32 device copy the kernel reads, (ntaps, L): element [i][c] is tap i of the outputs n with n mod L == c
        (phase (c M) mod L; L and M are coprime, so c <-> phase is one to one).  A wave's 64 consecutive outputs then read
        64 consecutive floats per tap (wrapping at L) instead of 64 rows."""
        import torch
        key = str(torch.device(device))
        t = self._device.get(key)
        if t is None:
            rows = self.taps[self.phase(np.arange(self.L))]         # (L, ntaps) by c = n mod L
            t = torch.from_numpy(np.ascontiguousarray(rows.T.astype(np.float32))).to(device)
            self._device[key] = t
        return t


def plan(sr_in, sr_out):
    """The cached Plan of a rate pair."""
    key = (int(sr_in), int(sr_out))
    pl = _PLANS.get(key)
    if pl is None:
        pl = _PLANS[key] = Plan(*key)
    return pl


def resample_host(x, sr_in, sr_out, chunk=4096):
    """The fp64 numpy reference of the definition above (tests; nothing on the hot path calls it)."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 1:
        raise ValueError("resample_host: one-dimensional signals only")
    if int(sr_in) == int(sr_out):
        return x.copy()
    pl = plan(sr_in, sr_out)
    n_out = pl.out_len(len(x))
    y = np.empty(n_out, dtype=np.float64)
    if n_out == 0:
        return y
    n = np.arange(n_out, dtype=np.int64)
    k0, ph = pl.first(n), pl.phase(n)
    left = max(0, -int(k0.min()))
    right = max(0, int(k0.max()) + pl.ntaps - len(x))
    xp = np.concatenate([np.zeros(left), x, np.zeros(right)])
    cols = np.arange(pl.ntaps, dtype=np.int64)[None, :]
    for a in range(0, n_out, chunk):
        b = min(n_out, a + chunk)
        y[a:b] = np.einsum("ij,ij->i", xp[k0[a:b, None] + left + cols], pl.taps[ph[a:b]])
    return y
