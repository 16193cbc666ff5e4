"""Shapes, signals and RIRs shared by tests/test_reverb.py and tests/test_gpu_reverb.py (not a test module)."""
import functools
import os

import numpy as np

EPS = 2.0 ** -24
P = 256


def case_list(lengths, taps):
    """(n, L, d) over the delays 0, 256, 300 and L - 1 that are legal for L taps."""
    return [(n, L, d) for n in lengths for L in taps for d in sorted({0, 256, 300, L - 1}) if 0 <= d < L]


@functools.lru_cache(maxsize=None)
def rir(L, seed=0):
    """A float32 RIR of L taps: a unit direct path in front of Gaussian noise that decays by 30 dB over the L taps, and every
    partition of 256 taps raised, where it has to be, to 2e-3 of the total energy (>= 1e-3 once the others have grown): a
    partition that is left out, or meets the wrong block, then changes the result by far more than rounding does."""
    rng = np.random.default_rng([77, L, seed])
    h = rng.standard_normal(L) * 0.2 * 10.0 ** (-1.5 * np.arange(L) / max(L, 2))
    h[0] = 1.0
    total = float(np.sum(h * h))
    for k in range(-(-L // P)):
        part = h[P * k:P * (k + 1)]
        e = float(np.sum(part * part))
        if e < 2e-3 * total:
            part *= np.sqrt(2e-3 * total / e)
    h = h.astype(np.float32)
    e = [float(np.sum(h[P * k:P * (k + 1)].astype(np.float64) ** 2)) for k in range(-(-L // P))]
    assert min(e) >= 1e-3 * sum(e)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def pool():
    """12 000 int16 samples of seeded Gaussian noise at level 0.1 under a slow envelope.  Shared, never written to."""
    rng = np.random.default_rng(2025)
    x = rng.standard_normal(12000) * 0.1 * (0.6 + 0.4 * np.sin(np.arange(12000) / 700.0))
    x = np.rint(x * 32768.0)
    assert np.abs(x).max() < 32768
    x = x.astype(np.int16)
    x.setflags(write=False)
    return x


def signal(n, at=0):
    return pool()[at:at + n]


def gate(x, h):
    """2^-24 ||h||_2 max|x|: one rounding of a result as large as the convolution gets on uncorrelated samples."""
    from sepkern import mixing
    return EPS * float(np.sqrt(np.sum(np.asarray(h, dtype=np.float64) ** 2))) * float(np.abs(mixing.as_float(x)).max())


def corpus(root, rate=8000, n_spk=4, n_utt=2, lengths=None):
    """A Kaldi-style directory of single-speaker files (wav.scp + utt2spk) of sepkern.synth's speech-like noise; lengths: samples
    per file, speaker-major."""
    import scipy.io.wavfile
    from sepkern import synth
    os.makedirs(os.path.join(root, "wav"), exist_ok=True)
    scp, u2s = [], []
    for p in range(n_spk):
        for k in range(n_utt):
            n = lengths[p * n_utt + k] if lengths else 600 + 97 * p + 211 * k
            x = np.rint(synth.speech_like(n, 100 * p + k) * (0.3 + 0.1 * k) * 32768.0).astype(np.int16)
            utt, path = "spk%d_%d" % (p, k), os.path.join(root, "wav", "spk%d_%d.wav" % (p, k))
            scipy.io.wavfile.write(path, rate, x)
            scp.append("%s %s\n" % (utt, path))
            u2s.append("%s spk%d\n" % (utt, p))
    open(os.path.join(root, "wav.scp"), "w").write("".join(scp))
    open(os.path.join(root, "utt2spk"), "w").write("".join(u2s))
    return root
