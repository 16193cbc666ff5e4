"""The array batch tests/test_ipd.py and tests/test_gpu_ipd.py share: six utterances at test_gpu_psa.py's lengths, eight
microphones each, as int16 PCM, with their oracle spectra (oracle/stft.py) -- computed once, never written to."""
import functools

import numpy as np

from oracle import stft as OS

F = 257
LENGTHS = [21000, 10240, 10112, 2048, 1920, 300]
FRAMES = [165, 81, 80, 17, 16, 3]
NCHAN = 8
PS = (1, 2, 7)
CHANNELS = {1: (1,), 2: (2, 5), 7: (1, 2, 3, 4, 5, 6, 7)}       # the listed channels of a case; the reference is channel 0
TOL_LIMIT, MAX_SHARE = 0.1, 0.01       # end to end: the tolerance 4 e (1/|Y_c| + 1/|Y_r|) exceeds 0.1 on fewer than 1 % of the elements


def array_signals(lengths, seed, nchan=NCHAN):
    """Per utterance (components, microphones): two white Gaussian sources (levels 0.1 and 0.15; white: no spectral nulls), source
    1 reaching microphone c with a delay of c samples and source 2 with 2 (nchan - 1 - c), plus independent sensor noise at 0.01;
    components = [source 1, source 2] as microphone 0 hears them.  Everything int16, nothing clips."""
    rng = np.random.default_rng(seed)
    out, lead = [], 2 * nchan
    for n in lengths:
        s1, s2 = (rng.standard_normal(n + lead) * a for a in (0.1, 0.15))
        mics = []
        for c in range(nchan):
            d1, d2 = c, 2 * (nchan - 1 - c)
            x = s1[lead - d1:lead - d1 + n] + s2[lead - d2:lead - d2 + n] + 0.01 * rng.standard_normal(n)
            mics.append(np.rint(x * 32768.0))
        comps = [np.rint(s1[lead:lead + n] * 32768.0), np.rint(s2[lead - 2 * (nchan - 1):lead - 2 * (nchan - 1) + n] * 32768.0)]
        assert max(np.abs(x).max() for x in mics + comps) < 32768
        out.append(([x.astype(np.int16) for x in comps], np.stack(mics).astype(np.int16)))
    return out


@functools.lru_cache(maxsize=None)
def case():
    """dict(sigs = [per utterance (NCHAN, n) int16], srcs = [per utterance [source 1, source 2] int16], spec = [per utterance
    (NCHAN, T, 257) complex128 oracle spectra])."""
    made = array_signals(LENGTHS, seed=91)
    assert [OS.num_frames(n) for n in LENGTHS] == FRAMES
    sigs = [m for _, m in made]
    spec = [np.stack([OS.stft(OS.pcm16_to_float(x)).T for x in m]).astype(np.complex128) for m in sigs]
    return dict(sigs=sigs, srcs=[c for c, _ in made], spec=spec)


def tolerance_share(e):
    """The share of (utterance, listed channel, frame, bin) elements of the case at which 4 e (1/|Y_c| + 1/|Y_r|) exceeds
    TOL_LIMIT, over all seven channels against the reference."""
    over = total = 0
    for sp in case()["spec"]:
        inv = 1.0 / np.maximum(np.abs(sp), 1e-300)
        tol = 4.0 * e * (inv[1:] + inv[:1])
        over += int((tol > TOL_LIMIT).sum())
        total += tol.size
    return over / total
