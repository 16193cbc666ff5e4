"""The pin suite of the waveform side of training: csrc/wave_loss.h, csrc/sisdr.hip (sk_sisdr_pit_fwd), csrc/mixit.hip
(sk_mixit_fwd) and csrc/mix.hip (sk_dynamic_mix).  tests/test_gpu_wave_cases.py runs the cases below on the device,
tests/test_wave_cases.py proves on any machine that they reach what they claim and that a wrong kernel would fail.

Here: the host code restated (CHUNK, the two nq_of, g_index, the workspace formulas, the dynamic mix's trip), the case tables
with the edges every case is there for, the references (always the package's numpy fp64 definitions: sisdr.pit_si_sdr,
mixit.mixit, mixing.mix, on the same float32 / int16 inputs), the gates, the kernels' chunked arithmetic restated in numpy, and
defect models: wrong variants of that restatement.

Gates
    MixIT    scores 2^-23 max(1, |v|) dB, coefficients 2^-22 relative (tests/test_gpu_mixit.py's).
    SI-SDR   pair, perm_score: 2^-23 max(1, |v|) dB + 4 x spread; coef: 2^-22 |v| + 4 x spread.  The spread is the difference of
             two evaluations of the REFERENCE: the plain-sums form in fp64 (pit_si_sdr) and the form with the means removed
             first in numpy longdouble.  It measures the inputs' conditioning, and in no case may 4 x spread exceed the
             rounding term (tests/test_wave_cases.py asserts it): a badly conditioned case cannot widen its own gate.
             Zero coefficients are exact zeros.
    both     best_perm / best_code equal in every utterance; out[1] exact, out[0] and out[2] within 2^-22 relative of the fp64
             sum of the reference's best scores.
    mix      (S + 5) 2^-24 relative on gains, (S + 6) 2^-24 peak on sources, S (2 S + 6) 2^-24 peak on the mixture
             (tests/test_gpu_dynamic_mix.py derives them); quantized output = mixing.quantize of the kernel's own unquantized
             result, bit for bit.
Decisions: every utterance that is not a tie is built so that the reference's best permutation or code leads the runner-up
by at least 1 dB.  A tie is exact in any arithmetic: two estimate offsets point at the same samples (or the utterance holds
exact numbers whose scores coincide term by term: one and two samples, an orthogonal pair at S = 2, two silent references), and
the expected answer is the first maximum.
Degenerate utterances hold zeros and signed powers of two over power-of-two lengths: every sum is exact in fp64, so the branch
taken cannot depend on the order of summation (asserted by summing in three orders).
"""
import functools
import itertools

import numpy as np

from sepkern import mixing, mixit, sisdr

# ------------------------------------------------------------------------------------------------ the host code, restated
CHUNK = 4096                          # wave_loss.h: samples per workgroup of a sums kernel
THREADS = 256                         # threads of a sums / finalize workgroup: the stride of gather_chunks and of the u loops
MAXS = 4                              # SK_MAXS
NREF = 2                              # mixit.hip
ALIGN = 256
MX_THREADS, MX_UNROLL = 1024, 4       # mix.hip
MX_TRIP = MX_THREADS * MX_UNROLL      # samples of a mixture one trip of dynamic_mix_kernel covers
SILENT = 2.0 ** -40                   # mix.hip MX_SILENT
EPS23, EPS22, EPS24 = 2.0 ** -23, 2.0 ** -22, 2.0 ** -24
MARGIN = 10.0
GAP_DB = 1.0
SK_EINVAL = -1                        # include/sepkern.h


def sisdr_nq(S):
    return 4 * S + S * S


def mixit_nq(M):
    return 2 + 2 * M + M * (M + 1) // 2


NQMAX = mixit_nq(MAXS)


def g_index(M, k, l):
    return 2 + 2 * M + k * M - k * (k - 1) // 2 + (l - k)


def nq_of(kind, S):
    return sisdr_nq(S) if kind == "sisdr" else mixit_nq(S)


def chunks_of(n):
    return -(-n // CHUNK)


def _align(n):
    return -(-n // ALIGN) * ALIGN


def partial_bytes(B, NQ, max_samples):
    return _align(B * chunks_of(max_samples) * NQ * 8)


def sisdr_workspace_bytes(B, S, max_samples):
    """[partial | best scores (B), fp64 pair matrix (B MAXS^2), sums (B x at most 2 MAXS^2)]; 0 for refused arguments."""
    if B <= 0 or not 1 <= S <= MAXS or max_samples <= 0:
        return 0
    return partial_bytes(B, sisdr_nq(S), max_samples) + _align(B * (1 + 3 * MAXS * MAXS) * 8)


def mixit_workspace_bytes(B, M, max_samples):
    """[partial | best scores (B), sums (B NQMAX)]; 0 for refused arguments."""
    if B <= 0 or not 2 <= M <= MAXS or max_samples <= 0:
        return 0
    return partial_bytes(B, mixit_nq(M), max_samples) + _align(B * (1 + NQMAX) * 8)


def workspace_bytes(kind, B, S, max_samples):
    return (sisdr_workspace_bytes if kind == "sisdr" else mixit_workspace_bytes)(B, S, max_samples)


def wrap_batch(kind, S):
    """The smallest B whose B * NQ items need a second trip of gather_chunks' stride loop."""
    return THREADS // nq_of(kind, S) + 1


def mix_trips(n):
    return -(-n // MX_TRIP)


# ------------------------------------------------------------------------------------------------ signals
LENGTHS = (1, 2, 255, 256, 257, 4095, 4096, 4097, 8192, 8193, 12289)
SNR_MAX = mixit.SNR_MAX               # 30 dB, the default: tau = 1e-3; the degenerate cases run at inf (tau = 0) and 0 dB (tau = 1)
DRAW_GAP_DB = 1.5                     # what a drawn utterance's decision must lead by to be kept (the test asserts GAP_DB = 1)
EST_PAD = np.float32(np.nan)          # between the estimates of the flat buffer: a sample read past an end is NaN
PCM_PAD = 12345                       # between the references


def _noise_pcm(rng, n, level, dc):
    x = np.rint((level * rng.standard_normal(n) + dc) * 32768.0)
    return np.clip(x, -32767, 32767).astype(np.int16)


def _dyadic(rng, n, kmin=2, kmax=6):
    """Signed powers of two 2^-kmin .. 2^-kmax and zeros: exactly representable as int16 PCM, every sum of products exact."""
    v = rng.choice([-1.0, 1.0], n) * 2.0 ** -rng.integers(kmin, kmax + 1, n)
    v[rng.random(n) < 0.2] = 0.0
    return v


def _pcm_of(v):
    x = np.asarray(v, dtype=np.float64) * 32768.0
    assert np.array_equal(x, np.rint(x)) and np.abs(x).max() <= 32768 and x.max() <= 32767
    return x.astype(np.int16)


def _sisdr_noisy(rng, n, S, minus_full_scale=False):
    """S references (int16, with a DC offset each) and S estimates = a drawn permutation of them at 8 .. 14 dB, with offsets of
    their own: the means matter, and the best permutation leads by far more than 1 dB."""
    refs = [_noise_pcm(rng, n, 0.08 + 0.02 * i, 0.02 * (i + 1) * (-1) ** i) for i in range(S)]
    if minus_full_scale:
        refs[0][n // 2] = -32768
    perm = list(rng.permutation(S))
    ests = []
    for k in range(S):
        r = refs[perm[k]].astype(np.float64) / 32768.0
        r0 = r - r.mean()
        noise = rng.standard_normal(n)
        noise *= np.sqrt(np.mean(r0 * r0)) * 10.0 ** (-rng.uniform(8.0, 14.0) / 20.0)
        ests.append(((0.5 + 0.25 * k) * (r0 + noise) + 0.03 * (k + 1)).astype(np.float32))
    return dict(est=ests, ref=refs, kind="noisy")


def _mixit_noisy(rng, n, M, minus_full_scale=False):
    """M sources, a drawn assignment with both groups populated, reference n = the sum of its group's sources (int16), every
    estimate its source plus noise at 8 .. 14 dB."""
    srcs = [_noise_pcm(rng, n, 0.03 + 0.01 * k, 0.0) for k in range(M)]
    code = int(rng.integers(1, (1 << M) - 1))
    refs = [np.sum([s.astype(np.int32) for k, s in enumerate(srcs) if ((code >> k) & 1) == g], axis=0) for g in range(NREF)]
    refs = [np.clip(x, -32767, 32767).astype(np.int16) for x in refs]
    if minus_full_scale:
        refs[1][n // 2] = -32768
    ests = []
    for s in srcs:
        v = s.astype(np.float64) / 32768.0
        noise = rng.standard_normal(n) * np.sqrt(np.mean(v * v) + 1e-12) * 10.0 ** (-rng.uniform(8.0, 14.0) / 20.0)
        ests.append((v + noise).astype(np.float32))
    return dict(est=ests, ref=refs, kind="noisy", code=code)


def _sisdr_tie(rng, n, S):
    """Estimates 0 and 1 are the SAME samples (one offset twice): rows 0 and 1 of pair hold the same bits, and the two
    permutations that exchange their references tie exactly.  x + y == y + x in any arithmetic."""
    u = _sisdr_noisy(rng, n, S)
    u["est"][1] = ("alias", 0)
    u["kind"] = "tie"
    return u


def _mixit_tie(rng, n, M):
    """x_0 = a + b, x_1 = a (+ c): estimates 0 and 1 are both a (one offset twice), so the codes that send 0 -> x_0, 1 -> x_1
    and 1 -> x_0, 0 -> x_1 tie exactly; the lower code wins."""
    a, b, c = (_noise_pcm(rng, n, 0.05, 0.0) for _ in range(3))
    x0 = a.astype(np.int32) + (b if M >= 3 else 0)
    x1 = a.astype(np.int32) + (c if M >= 4 else 0)
    f = lambda s: (s.astype(np.float64) / 32768.0 + 0.01 * rng.standard_normal(n)).astype(np.float32)   # noqa: E731
    ests = [f(a), ("alias", 0)] + ([f(b)] if M >= 3 else []) + ([f(c)] if M >= 4 else [])
    return dict(est=ests, ref=[x0.astype(np.int16), x1.astype(np.int16)], kind="tie")


def _sisdr_exact(rng, n, S, what):
    """Degenerate utterances on exact numbers (n a power of two, or 1):
    silent      reference 0 is zeros                      b == 0: projection 0, coefficients 0
    orthogonal  r = (+v, -v, ...), e = (+w, +w, -w, -w, ...) plus offsets    a == 0 exactly
    copy        every estimate is its reference bit for bit    den == 0
    one         a single sample: a == b == c == 0
    two         two samples: every zero-mean signal is a multiple of (1, -1), den == 0 for EVERY pair, all permutations tie"""
    assert n & (n - 1) == 0
    if what == "one" or what == "two":
        refs = [_pcm_of([2.0 ** -(2 + i), -(2.0 ** -(3 + i))][:n]) for i in range(S)]
        ests = [np.array([2.0 ** -(1 + k), -(2.0 ** -(4 + k))][:n], dtype=np.float32) for k in range(S)]
        if n == 2:                                   # differences that are powers of two: a / b is exact
            refs = [_pcm_of([2.0 ** -(2 + i), -(2.0 ** -(2 + i))]) for i in range(S)]
            ests = [np.array([2.0 ** -(1 + k) + 0.25, -(2.0 ** -(1 + k)) + 0.25], dtype=np.float32) for k in range(S)]
        return dict(est=ests, ref=refs, kind=what)
    refs = [_pcm_of(_dyadic(rng, n)) for _ in range(S)]
    ests = [_dyadic(rng, n).astype(np.float32) for _ in range(S)]
    if what == "silent":                             # (the other estimates: their references plus +-2^-8, so the decision is clear)
        refs[0] = np.zeros(n, dtype=np.int16)
        for i in range(1, S):
            ests[i] = (refs[i].astype(np.float64) / 32768.0 + rng.choice([-1.0, 1.0], n) * 2.0 ** -8).astype(np.float32)
    elif what == "orthogonal":
        for i in range(S):
            v, w = 2.0 ** -(2 + i), 2.0 ** -(3 + i)
            refs[i] = _pcm_of(np.tile([v, -v], n // 2) + 2.0 ** -5)
            ests[i] = (np.tile([w, w, -w, -w], n // 4) + 2.0 ** -4).astype(np.float32)
    elif what == "copy":
        ests = [(r.astype(np.float64) / 32768.0).astype(np.float32) for r in refs]
    else:
        raise ValueError(what)
    return dict(est=ests, ref=refs, kind=what)


def _mixit_exact(rng, n, M, what):
    """silent: both references zeros (P == 0: coefficient 0 where the error is 0 too; codes 0 and 2^M - 1 tie);
    partition: x_0 = e_0 + e_1, x_1 = the rest, exactly (den == 0 at tau == 0)."""
    assert n & (n - 1) == 0
    ests = [_dyadic(rng, n, 3, 6) for _ in range(M)]
    if what == "silent":
        refs = [np.zeros(n, dtype=np.int16)] * NREF
    elif what == "partition":
        refs = [_pcm_of(ests[0] + (ests[1] if M >= 3 else 0.0)), _pcm_of(np.sum(ests[2 if M >= 3 else 1:], axis=0))]
    else:
        raise ValueError(what)
    return dict(est=[e.astype(np.float32) for e in ests], ref=refs, kind=what)


def _gap_of(kind, u, snr_max):
    es = [u["est"][e[1]] if isinstance(e, tuple) else e for e in u["est"]]
    rs = [r.astype(np.float64) / 32768.0 for r in u["ref"]]
    score = sisdr.pit_si_sdr(es, rs)["perm_score"] if kind == "sisdr" else mixit.mixit(es, rs, snr_max=snr_max)["score"]
    top = np.sort(score)
    return np.inf if len(top) < 2 else float(top[-1] - top[-2])


def _drawn(build, kind, snr_max, rng, n, S, **kw):
    """The first draw whose reference decision leads the runner-up by DRAW_GAP_DB (short utterances can miss it by chance)."""
    for _ in range(200):
        u = build(rng, n, S, **kw)
        if _gap_of(kind, u, snr_max) >= DRAW_GAP_DB:
            return u
    raise AssertionError("no draw of %s n=%d S=%d keeps the decision gap" % (kind, n, S))


# ------------------------------------------------------------------------------------------------ the loss cases
def _short(j):
    """The lengths of a large batch's short utterances: a few hundred samples, odd and even, never the same twice in a row."""
    return 200 + 37 * (j % 7) + (j % 3)


def _large_batch(B):
    """B utterances: short ones and ONE multi-chunk utterance (4097 samples), not first."""
    lens = [_short(j) for j in range(B)]
    lens[min(3, B - 1)] = CHUNK + 1
    return lens


def _specs():
    """name -> dict(kind, S, lens or a builder list, max_samples, count, tau, edges)."""
    out = {}
    ragged = (4097, 1, 256, 255, 12289, 2, 257, 4095, 4096, 8192, 8193, 512)     # the longest is not first; 512: the tie
    for kind, counts in (("sisdr", (1, 2, 3, 4)), ("mixit", (2, 3, 4))):
        for S in counts:
            out["%s_lengths_%d" % (kind, S)] = dict(
                kind=kind, S=S, lens=ragged, max_samples=4 * CHUNK + 1, count=None, shared=(3, 2), tie=11 if S >= 2 else None,
                edges=("lengths", "ragged", "shared_ref", "minus_full_scale", "odd_offsets") + (("tie",) if S >= 2 else ()))
            B = wrap_batch(kind, S)
            for b, edge in ((B - 1, "below_wrap"), (B, "first_above_wrap")):
                out["%s_wrap_%d_B%d" % (kind, S, b)] = dict(kind=kind, S=S, lens=_large_batch(b), max_samples=2 * CHUNK + 1,
                                                            count=None if b == B else 2.0 * b,
                                                            edges=(edge, "ragged", "odd_offsets") + (("above_wrap",) if b == B else ()))
    for kind, S in (("sisdr", 2), ("mixit", 4)):                                 # the batch size training runs
        out["%s_train_%d_B32" % (kind, S)] = dict(kind=kind, S=S, lens=_large_batch(32), max_samples=2 * CHUNK + 1, count=64.0,
                                                  edges=("above_wrap", "training_batch", "ragged", "odd_offsets"))
    for kind, S in (("sisdr", 2), ("mixit", 2)):
        for b, edge in ((256, "u_below_wrap"), (257, "u_above_wrap")):
            out["%s_utts_%d_B%d" % (kind, S, b)] = dict(kind=kind, S=S, lens=_large_batch(b), max_samples=2 * CHUNK + 1,
                                                        count=None if b == 257 else 300.0, edges=(edge, "above_wrap", "ragged", "odd_offsets"))
    for S in (1, 2):
        out["sisdr_degenerate_%d" % S] = dict(kind="sisdr", S=S, max_samples=3 * CHUNK, count=None,
                                              exact=(("silent", 256), ("orthogonal", 2 * CHUNK), ("copy", CHUNK), ("one", 1), ("two", 2), ("copy", 256)),
                                              edges=("silent_ref", "orthogonal", "exact_copy", "one_sample", "two_samples", "ragged", "odd_offsets"))
    for snr_max, name in ((np.inf, "tau0"), (0.0, "tau1")):
        out["mixit_degenerate_%s" % name] = dict(kind="mixit", S=3, max_samples=3 * CHUNK, count=None, snr_max=snr_max,
                                                 exact=(("silent", 256), ("partition", 2 * CHUNK), ("noisy", 257), ("noisy", CHUNK + 1), ("partition", 256)),
                                                 edges=("both_silent", "exact_partition", name, "ragged", "odd_offsets"))
    return out


SPECS = _specs()
LOSS_CASES = tuple(SPECS)


def _layout(sizes, first=1):
    """Odd element offsets for signals of the given sizes, at least one pad element between two of them -> (offsets, total)."""
    offs, at = [], first
    for n in sizes:
        at += (at + 1) % 2
        offs.append(at)
        at += n + 1
    return offs, at + 1


@functools.lru_cache(maxsize=None)
def loss_case(name):
    """The flat buffers of a case: est (float32, NaN between the signals), pcm (int16) and its float32 copy ref32, the offset
    tables est_offs (B S) and ref_offs (B NR), nsamp (B) -- what the entry point takes -- and per utterance its kind."""
    sp = SPECS[name]
    kind, S = sp["kind"], sp["S"]
    NR = S if kind == "sisdr" else NREF
    rng = np.random.default_rng([len(name), S, sum(map(ord, name))])
    draw, tie, exact = (_sisdr_noisy, _sisdr_tie, _sisdr_exact) if kind == "sisdr" else (_mixit_noisy, _mixit_tie, _mixit_exact)
    noisy = functools.partial(_drawn, draw, kind, sp.get("snr_max", SNR_MAX))
    utts = []
    if "exact" in sp:
        for what, n in sp["exact"]:
            utts.append(noisy(rng, n, S) if what == "noisy" else exact(rng, n, S, what))
    else:
        for j, n in enumerate(sp["lens"]):
            if n <= 2:
                utts.append(exact(rng, n, S, "one" if n == 1 else "two") if kind == "sisdr" else noisy(rng, n, S))
            elif j == sp.get("tie"):
                utts.append(tie(rng, n, S))
            else:
                utts.append(noisy(rng, n, S, minus_full_scale=(j == 0)))
        if "shared" in sp:                            # utterance a reads the first samples of utterance b's references
            a, b = sp["shared"]
            na = len(utts[a]["ref"][0])
            shared = noisy(rng, len(utts[b]["ref"][0]), S)
            utts[b] = shared
            utts[a] = dict(est=[e[:na].copy() for e in shared["est"]], ref=[("share", b)] * NR, kind="noisy")
    nsamp = [len(u["est"][0]) for u in utts]
    own_e = [(j, k) for j, u in enumerate(utts) for k in range(S) if not isinstance(u["est"][k], tuple)]
    own_r = [(j, i) for j, u in enumerate(utts) for i in range(NR) if not isinstance(u["ref"][i], tuple)]
    eo, etot = _layout([nsamp[j] for j, _ in own_e])
    ro, rtot = _layout([nsamp[j] for j, _ in own_r], first=3)
    est, pcm = np.full(etot, EST_PAD, dtype=np.float32), np.full(rtot, PCM_PAD, dtype=np.int16)
    est_offs, ref_offs = np.zeros((len(utts), S), dtype=np.int64), np.zeros((len(utts), NR), dtype=np.int64)
    for (j, k), o in zip(own_e, eo):
        est[o:o + nsamp[j]] = utts[j]["est"][k]
        est_offs[j, k] = o
    for (j, i), o in zip(own_r, ro):
        pcm[o:o + nsamp[j]] = utts[j]["ref"][i]
        ref_offs[j, i] = o
    for j, u in enumerate(utts):
        for k in range(S):
            if isinstance(u["est"][k], tuple):
                est_offs[j, k] = est_offs[j, u["est"][k][1]]
        for i in range(NR):
            if isinstance(u["ref"][i], tuple):
                ref_offs[j, i] = ref_offs[u["ref"][i][1], i]
    pad = np.ones(rtot, dtype=bool)
    for (j, i), o in zip(own_r, ro):
        pad[o:o + nsamp[j]] = False
    ref32 = pcm.astype(np.float32) / np.float32(32768.0)
    ref32[pad] = np.nan                               # the float32 copy: NaN between the references
    B = len(utts)
    return dict(name=name, kind=kind, S=S, NR=NR, B=B, nsamp=np.array(nsamp, dtype=np.int32), max_samples=sp["max_samples"],
                nch=chunks_of(sp["max_samples"]), est=est, pcm=pcm, ref32=ref32, est_offs=est_offs, ref_offs=ref_offs,
                count=sp["count"], snr_max=sp.get("snr_max", SNR_MAX), tau=mixit.tau_of(sp.get("snr_max", SNR_MAX)), kinds=[u["kind"] for u in utts], edges=sp["edges"])


def signals(c, j, raw_pcm=False):
    """Utterance j as the kernel reads it: S float32 estimates and NR references in fp64 (int16 scaled by 2^-15)."""
    n = int(c["nsamp"][j])
    es = [c["est"][o:o + n] for o in c["est_offs"][j]]
    rs = [c["pcm"][o:o + n].astype(np.float64) * (1.0 if raw_pcm else 1.0 / 32768.0) for o in c["ref_offs"][j]]
    return es, rs


def count_of(c):
    return float(c["B"]) if c["count"] is None else float(c["count"])


# ------------------------------------------------------------------------------------------------ references and gates
def sisdr_longdouble(es, rs, count, best):
    """The second evaluation of the SI-SDR reference: the means removed first, numpy longdouble throughout -> pair (S, S),
    perm_score (S!), coef (S, 3) for the permutation `best`."""
    LD = np.longdouble
    S = len(rs)
    E = [np.asarray(e, dtype=LD) for e in es]
    R = [np.asarray(r, dtype=LD) for r in rs]
    mue, mur = [e.mean() for e in E], [r.mean() for r in R]
    E, R = [e - m for e, m in zip(E, mue)], [r - m for r, m in zip(R, mur)]
    eps, kappa = LD(sisdr.EPS), LD(10.0) / np.log(LD(10.0))
    abc = [[(np.dot(E[k], R[i]), np.dot(R[i], R[i]), np.dot(E[k], E[k])) for i in range(S)] for k in range(S)]
    pair = np.zeros((S, S), dtype=LD)
    for k in range(S):
        for i in range(S):
            a, b, c = abc[k][i]
            tt = (a / b) * a if b > 0 else LD(0)
            pair[k, i] = 10 * np.log10((tt + eps) / (max(c - tt, LD(0)) + eps))
    perms = list(itertools.permutations(range(S)))
    score = np.array([sum(pair[k, p[k]] for k in range(S)) / S for p in perms], dtype=LD)
    coef = np.zeros((S, 3), dtype=LD)
    m = LD(-1.0) / (LD(count) * S)
    for k in range(S):
        i = perms[best][k]
        a, b, c = abc[k][i]
        if b > 0 and a != 0:
            den = c - (a / b) * a
            if den > 0:
                P, Q = -2 * kappa / den, kappa * (2 / a + 2 * a / (b * den))
                coef[k] = m * P, m * Q, -m * (P * mue[k] + Q * mur[i])
    return pair, score, coef


def _runner_up_gap(score, best):
    rest = np.delete(np.asarray(score, dtype=np.float64), best)
    return float(score[best] - rest.max()) if rest.size else np.inf


@functools.lru_cache(maxsize=None)
def loss_reference(name):
    """Per utterance the package's fp64 definition on the case's own inputs, its gates, and (SI-SDR) the spreads.  Computed
    once per case, shared by every test, never written to."""
    c = loss_case(name)
    count, want = count_of(c), []
    for j in range(c["B"]):
        es, rs = signals(c, j)
        if c["kind"] == "sisdr":
            w = sisdr.pit_si_sdr(es, rs, count=count)
            score, best, coef = w["perm_score"], w["best_perm"], w["coef"]
            p_ld, s_ld, c_ld = sisdr_longdouble(es, rs, count, best)
            sp_pair = np.abs(w["pair"] - p_ld).astype(np.float64)
            sp_score, sp_coef = np.abs(score - s_ld).astype(np.float64), np.abs(coef - c_ld).astype(np.float64)
            g_pair = EPS23 * np.maximum(1.0, np.abs(w["pair"]))
            g_score, g_coef = EPS23 * np.maximum(1.0, np.abs(score)), EPS22 * np.abs(coef)
            want.append(dict(pair=w["pair"], score=score, best=best, coef=coef, spread=dict(pair=sp_pair, score=sp_score, coef=sp_coef),
                             round=dict(pair=g_pair, score=g_score, coef=g_coef),
                             gate=dict(pair=g_pair + 4.0 * sp_pair, score=g_score + 4.0 * sp_score, coef=g_coef + 4.0 * sp_coef)))
        else:
            w = mixit.mixit(es, rs, count=count, snr_max=c["snr_max"])
            want.append(dict(score=w["score"], best=w["best"], coef=w["coef"], P=w["P"], err=w["err"],
                             gate=dict(score=EPS23 * np.maximum(1.0, np.abs(w["score"])), coef=EPS22 * np.abs(w["coef"]))))
        want[-1]["gap"] = _runner_up_gap(want[-1]["score"], want[-1]["best"])
    tot = float(np.sum([w["score"][w["best"]] for w in want]))
    return dict(utts=want, out=np.array([-tot / count, count, tot]))


def expected_tie(c, j):
    """(first, last) index of the exact tie an utterance that was not drawn holds -- two estimates at one offset, or exact numbers
    whose scores coincide term by term -- or None.  The first is the expected decision."""
    if c["kinds"][j] == "noisy":
        return None
    score = loss_reference(c["name"])["utts"][j]["score"]
    top = np.flatnonzero(score == score.max())
    return (int(top[0]), int(top[-1])) if len(top) >= 2 else None


# ------------------------------------------------------------------------------------------------ the kernels' arithmetic, restated
def chunk_rows(c, j, drop_last=False, raw_pcm=False, chunk=CHUNK):
    """What the sums kernel stores for utterance j: one row of NQ fp64 sums per chunk below ceil(L / CHUNK), in the layouts the
    two .hip files state.  drop_last: every chunk loses its last sample."""
    es, rs = signals(c, j, raw_pcm)
    S, n, rows = c["S"], int(c["nsamp"][j]), []
    for n0 in range(0, n, chunk):
        n1 = min(n, n0 + chunk) - (1 if drop_last else 0)
        E = np.stack([e[n0:n1].astype(np.float64) for e in es])
        R = np.stack([r[n0:n1] for r in rs])
        if c["kind"] == "sisdr":                      # [sum e | sum r | sum e^2 | sum r^2 | sum e_k r_i, k-major]
            rows.append(np.concatenate([E.sum(1), R.sum(1), (E * E).sum(1), (R * R).sum(1), (E @ R.T).reshape(-1)]))
        else:                                         # [P_0 P_1 | c_0k | c_1k | G_kl, k <= l, row-major]
            row = np.zeros(mixit_nq(S))
            row[:2] = (R * R).sum(1)
            row[2:2 + 2 * S] = (R @ E.T).reshape(-1)
            G = E @ E.T
            for k in range(S):
                for l in range(k, S):
                    row[g_index(S, k, l)] = G[k, l]
            rows.append(row)
    return rows


def _argmax(score, last):
    score = np.asarray(score)
    return int(len(score) - 1 - np.argmax(score[::-1])) if last else int(np.argmax(score))


def sisdr_finalize(s, n, S, count, last_max=False, keep_mean=False, unguarded=False):
    """sisdr_finalize_kernel's per-utterance arithmetic on the gathered sums s (NQ,)."""
    n = float(n)

    def inner(k, i):
        se, sr = s[k], s[S + i]
        if keep_mean:
            return s[4 * S + k * S + i], s[3 * S + i], s[2 * S + k], 0.0, 0.0
        return s[4 * S + k * S + i] - se * sr / n, s[3 * S + i] - sr * sr / n, s[2 * S + k] - se * se / n, se / n, sr / n
    pair = np.zeros((S, S))
    with np.errstate(all="ignore"):
        for k in range(S):
            for i in range(S):
                a, b, c, _, _ = inner(k, i)
                tt = (a / b) * a if b > 0.0 else 0.0
                pair[k, i] = 10.0 * np.log10((tt + sisdr.EPS) / (max(c - tt, 0.0) + sisdr.EPS))
        perms = list(itertools.permutations(range(S)))
        score = np.array([sum(pair[k, p[k]] for k in range(S)) / S for p in perms])
        best = _argmax(score, last_max)
        coef = np.zeros((S, 3))
        m = -1.0 / (count * S)
        for k in range(S):
            a, b, c, mue, mur = inner(k, perms[best][k])
            if unguarded or (b > 0.0 and a != 0.0):
                den = c - np.float64(a) / np.float64(b) * a
                if unguarded or den > 0.0:
                    P, Q = -2.0 * sisdr.KAPPA / np.float64(den), sisdr.KAPPA * (2.0 / np.float64(a) + 2.0 * a / np.float64(b * den))
                    coef[k] = m * P, m * Q, -m * (P * mue + Q * mur)
    return dict(pair=pair, score=score, best=best, coef=coef)


def mixit_finalize(s, M, tau, count, last_max=False, unguarded=False):
    """mixit_finalize_kernel's per-utterance arithmetic on the gathered sums s (NQ,)."""
    P, cc = s[:2], s[2:2 + 2 * M].reshape(2, M)
    G = np.zeros((M, M))
    for k in range(M):
        for l in range(k, M):
            G[k, l] = G[l, k] = s[g_index(M, k, l)]
    with np.errstate(all="ignore"):
        score = np.zeros(1 << M)
        for code in range(1 << M):
            err = mixit.errors(P, cc, G, code)
            score[code] = 0.5 * sum(10.0 * np.log10((P[g] + mixit.EPS) / (err[g] + tau * P[g] + mixit.EPS)) for g in range(NREF))
        best = _argmax(score, last_max)
        den = mixit.errors(P, cc, G, best) + tau * P
        coef = np.where((den > 0.0) | unguarded, mixit.KAPPA / (count * (den + mixit.EPS)), 0.0)
    return dict(score=score, best=best, coef=coef)


LOSS_DEFECTS = ("gather_wrap", "gather_extra_chunk", "gather_short", "chunk_last_sample", "finalize_wrap", "tally_wrap", "last_maximum",
                "mean_kept", "pcm_unscaled", "unguarded_zero")


def loss_model(name, defect=None):
    """The whole call as the kernels compute it -- chunk rows, gather_chunks, the finalize step, tally_scores -- or as a kernel
    with `defect` would: per utterance dict(pair, score, best, coef) and out (3,).  An output nobody wrote is NaN."""
    c = loss_case(name)
    kind, S, B, count = c["kind"], c["S"], c["B"], count_of(c)
    NQ = nq_of(kind, S)
    rows = [chunk_rows(c, j, drop_last=(defect == "chunk_last_sample"), raw_pcm=(defect == "pcm_unscaled")) for j in range(B)]
    longest = int(np.argmax(c["nsamp"]))
    sums = np.zeros((B, NQ))
    for j in range(B):
        take = rows[j]
        if defect == "gather_short":
            take = take[:-1]
        elif defect == "gather_extra_chunk":          # slot (j, mych) holds what an earlier call's longer utterance left there
            take = take + [rows[longest][0]]
        sums[j] = np.sum(take, axis=0) if take else 0.0
    if defect == "gather_wrap":                       # the items idx = u NQ + q >= 256 are never gathered
        sums.reshape(-1)[THREADS:] = 0.0
    utts = []
    for j in range(B):
        kw = dict(last_max=(defect == "last_maximum"), unguarded=(defect == "unguarded_zero"))
        if kind == "sisdr":
            utts.append(sisdr_finalize(sums[j], c["nsamp"][j], S, count, keep_mean=(defect == "mean_kept"), **kw))
        else:
            utts.append(mixit_finalize(sums[j], S, c["tau"], count, **kw))
        if defect == "finalize_wrap" and j >= THREADS:
            utts[-1] = {k: (-1 if k == "best" else np.full_like(v, np.nan)) for k, v in utts[-1].items()}
    best = np.array([np.nan if u["best"] < 0 else u["score"][u["best"]] for u in utts])
    tot = float(best[:THREADS].sum()) if defect == "tally_wrap" else float(best.sum())
    return dict(utts=utts, out=np.array([-tot / count, count, tot]))


def _ratio(got, want, gate):
    """The largest |got - want| / gate; a zero gate asks for equality; a NaN anywhere is infinitely far."""
    got, want, gate = np.broadcast_arrays(np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(gate, np.float64))
    if got.size == 0:
        return 0.0
    d = np.abs(got - want)
    if np.isnan(d).any():
        return np.inf
    r = np.where(gate > 0, d / np.where(gate > 0, gate, 1.0), np.where(d > 0, np.inf, 0.0))
    return float(r.max())


def loss_ratios(name, got):
    """Every checked output of a call against the reference, as a fraction of its gate: dict(pair, score, coef, out, decisions);
    `decisions` is 0 where every best_perm / best_code is the reference's, inf otherwise."""
    ref = loss_reference(name)
    out = dict(pair=0.0, score=0.0, coef=0.0, decisions=0.0)
    for g, w in zip(got["utts"], ref["utts"]):
        for key in ("pair", "score", "coef"):
            if key in w["gate"]:
                out[key] = max(out[key], _ratio(g[key], w[key], w["gate"][key]))
        if int(g["best"]) != int(w["best"]):
            out["decisions"] = np.inf
    out["out"] = max(_ratio(got["out"][[0, 2]], ref["out"][[0, 2]], EPS22 * np.abs(ref["out"][[0, 2]])), _ratio(got["out"][1], ref["out"][1], 0.0))
    return out


def loss_defect_shows(name, defect):
    """The largest move of a checked output under the defect, in units of MARGIN x its gate."""
    return max(loss_ratios(name, loss_model(name, defect)).values()) / MARGIN


LOSS_DEFECT_CASES = {
    "gather_wrap": [n for n, sp in SPECS.items() if "above_wrap" in sp["edges"]],
    "gather_extra_chunk": [n for n in SPECS if "_lengths_" in n or "_train_" in n],
    "gather_short": [n for n in SPECS if "_lengths_" in n or "_train_" in n or "_degenerate_" in n],
    "chunk_last_sample": [n for n in SPECS if "_lengths_" in n or "_train_" in n],
    "finalize_wrap": [n for n, sp in SPECS.items() if "u_above_wrap" in sp["edges"]],
    "tally_wrap": [n for n, sp in SPECS.items() if "u_above_wrap" in sp["edges"]],
    "last_maximum": [n for n, sp in SPECS.items() if "tie" in sp["edges"]] + ["sisdr_degenerate_2", "mixit_degenerate_tau0"],
    "mean_kept": [n for n in SPECS if n.startswith("sisdr_lengths_") or n.startswith("sisdr_train_")],
    "pcm_unscaled": [n for n in SPECS if "_lengths_" in n or "_train_" in n],
    "unguarded_zero": ["sisdr_degenerate_1", "sisdr_degenerate_2", "mixit_degenerate_tau0"],
}

LOSS_EDGE_CLAIMS = {
    "lengths": lambda c: set(LENGTHS) <= set(c["nsamp"].tolist()),
    "ragged": lambda c: int(np.argmax(c["nsamp"])) != 0 and all(chunks_of(int(n)) < c["nch"] for n in c["nsamp"]),
    "shared_ref": lambda c: any((c["ref_offs"][a] == c["ref_offs"][b]).all() and c["nsamp"][a] != c["nsamp"][b]
                                for a in range(c["B"]) for b in range(a)),
    "minus_full_scale": lambda c: any((signals(c, j)[1][i] == -1.0).any() for j in range(c["B"]) for i in range(c["NR"])),
    "odd_offsets": lambda c: bool((c["est_offs"] % 2 == 1).all() and (c["ref_offs"] % 2 == 1).all()),
    "tie": lambda c: any(k == "tie" and c["est_offs"][j, 0] == c["est_offs"][j, 1] for j, k in enumerate(c["kinds"])),
    "below_wrap": lambda c: c["B"] * nq_of(c["kind"], c["S"]) <= THREADS < (c["B"] + 1) * nq_of(c["kind"], c["S"]),
    "above_wrap": lambda c: c["B"] * nq_of(c["kind"], c["S"]) > THREADS,
    "first_above_wrap": lambda c: (c["B"] - 1) * nq_of(c["kind"], c["S"]) <= THREADS < c["B"] * nq_of(c["kind"], c["S"]),
    "training_batch": lambda c: c["B"] == 32,
    "u_below_wrap": lambda c: c["B"] == THREADS,
    "u_above_wrap": lambda c: c["B"] == THREADS + 1,
    "silent_ref": lambda c: any(k == "silent" and not signals(c, j)[1][0].any() for j, k in enumerate(c["kinds"])),
    "orthogonal": lambda c: "orthogonal" in c["kinds"],
    "exact_copy": lambda c: any(k == "copy" and all(np.array_equal(e.astype(np.float64), r) for e, r in zip(*signals(c, j)))
                                for j, k in enumerate(c["kinds"])),
    "one_sample": lambda c: any(k == "one" and c["nsamp"][j] == 1 for j, k in enumerate(c["kinds"])),
    "two_samples": lambda c: any(k == "two" and c["nsamp"][j] == 2 for j, k in enumerate(c["kinds"])),
    "both_silent": lambda c: any(k == "silent" and not any(r.any() for r in signals(c, j)[1]) for j, k in enumerate(c["kinds"])),
    "exact_partition": lambda c: "partition" in c["kinds"],
    "tau0": lambda c: c["tau"] == 0.0,
    "tau1": lambda c: c["tau"] == 1.0,
}


def sums_in_three_orders(c, j):
    """The utterance's NQ sums added chunk by chunk, sample by sample forwards, and sample by sample backwards."""
    by_chunk = np.sum(chunk_rows(c, j), axis=0)
    terms = chunk_rows(c, j, chunk=1)                 # one sample per "chunk": the rows are the samples' own terms
    assert len(terms) == int(c["nsamp"][j])
    fwd, bwd = np.zeros_like(by_chunk), np.zeros_like(by_chunk)
    for t in terms:
        fwd = fwd + t
    for t in terms[::-1]:
        bwd = bwd + t
    return by_chunk, fwd, bwd


# ================================================================================================ dynamic mix
MIX_LENGTHS = (1, 63, 64, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193)
POOL = 16384


@functools.lru_cache(maxsize=None)
def _pool():
    """int16 noise through a 4-tap average with a slow envelope (tests/test_gpu_dynamic_mix.py's pool, shorter)."""
    rng = np.random.default_rng(4097)
    x = np.convolve(rng.standard_normal(POOL + 3), np.full(4, 0.25), mode="valid") * 0.1
    x *= 0.6 + 0.4 * np.sin(np.arange(POOL) / 900.0)
    return np.rint(x * 32768.0).astype(np.int16)


def _mix_specs():
    out = {}
    for S in (1, 2, 3, 4):
        for dtype in ("int16", "float32"):
            out["mix_lengths_%s_%d" % (dtype, S)] = dict(S=S, dtype=dtype, build="lengths", quantize=False, edges=("lengths", "overlap", "tail_trip"))
    out["mix_peaks"] = dict(S=2, dtype="int16", build="peaks", quantize=False,
                            edges=("peak_alone_in_second_trip", "peak_at_4095", "peak_in_mixture_only", "peak_in_one_source_only"))
    out["mix_silence"] = dict(S=2, dtype="float32", build="silence", quantize=False, edges=("on_threshold", "below_threshold", "all_silent"))
    out["mix_clip"] = dict(S=2, dtype="int16", build="clip", quantize=True, edges=("clips_positive", "minus_one_exact"))
    return out


MIX_SPECS = _mix_specs()
MIX_CASES = tuple(MIX_SPECS)


@functools.lru_cache(maxsize=None)
def mix_case(name):
    """flat (int16 or float32 samples), in_offs (S, B), nsamp (B), amp (S, B) float32, peak (B) float32, quantize."""
    sp = MIX_SPECS[name]
    S, build = sp["S"], sp["build"]
    rng = np.random.default_rng([S, len(name), sum(map(ord, name))])
    if build == "lengths":                           # overlapping stretches of one pool, odd offsets
        flat, nsamp = _pool(), list(MIX_LENGTHS)
        if sp["dtype"] == "float32":                 # float32 samples OFF the int16 grid (an int16 case runs its float32 copy anyway)
            flat = (flat.astype(np.float64) / 32768.0 * (1.0 + 0.01 * np.cos(np.arange(POOL) / 7.0))).astype(np.float32)
        offs = [[1 + 2 * (37 * u + 1201 * s) for u in range(len(nsamp))] for s in range(S)]
        amp = [[float(mixing.snr_to_amp(2.5 - s + 0.3 * u)) for u in range(len(nsamp))] for s in range(S)]
        peak = [float(np.float32(0.5 + 0.03 * u)) for u in range(len(nsamp))]
    elif build == "peaks":
        n = MX_TRIP + 1
        sig = []
        x0, x1 = _noise_pcm(rng, n, 0.05, 0.0), _noise_pcm(rng, n, 0.05, 0.0)
        x0[-1], x1[-1] = 20000, 18000                # 0: the maximum is the mixture's LAST sample, alone in the second trip
        sig += [x0, x1]
        x0, x1 = _noise_pcm(rng, n - 1, 0.05, 0.0), _noise_pcm(rng, n - 1, 0.05, 0.0)
        x0[MX_TRIP - 1], x1[MX_TRIP - 1] = -20000, -18000          # 1: at index 4095, the fourth load of the last thread
        sig += [x0, x1]
        x0 = _noise_pcm(rng, 1025, 0.05, 0.0)        # 2: in the mixture only -- equal sources: the mixture is twice either
        sig += [x0, x0.copy()]
        x0 = _noise_pcm(rng, 1023, 0.05, 0.0)        # 3: in one source only -- the other is its negative at half the amplitude
        sig += [x0, -x0]
        nsamp = [n, n - 1, 1025, 1023]
        lay, total = _layout([len(x) for x in sig])
        flat = np.full(total, PCM_PAD, dtype=np.int16)
        for x, o in zip(sig, lay):
            flat[o:o + len(x)] = x
        offs = [[lay[2 * u + s] for u in range(4)] for s in range(2)]
        amp, peak = [[1.0] * 4, [1.0, 1.0, 1.0, 0.5]], [0.9, 0.8, 0.7, 0.6]
    elif build == "silence":                         # float32: constant sources whose mean square is EXACTLY 2^-40 / 2^-42
        n = 1024
        live = (_noise_pcm(rng, n, 0.05, 0.0).astype(np.float32) / np.float32(32768.0))
        on, below, zero = np.full(n, 2.0 ** -20, np.float32), np.full(n, 2.0 ** -21, np.float32), np.zeros(n, np.float32)
        flat = np.concatenate([[np.float32(np.nan)], live, [np.float32(np.nan)], on, below, zero])
        o_live, o_on, o_below, o_zero = 1, n + 2, 2 * n + 2, 3 * n + 2
        offs = [[o_live, o_live, o_below, o_zero], [o_on, o_below, o_zero, o_below]]     # mixtures 2 and 3: everything silent
        nsamp = [n] * 4
        amp, peak = [[1.0] * 4, [0.5] * 4], [0.9] * 4
    elif build == "clip":
        n = 1025
        x0, x1 = _noise_pcm(rng, n, 0.05, 0.0), _noise_pcm(rng, n, 0.05, 0.0)
        x0[700], x1[700] = 20000, 18000
        flat = np.concatenate([[PCM_PAD], x0, [PCM_PAD], x1, [PCM_PAD], -x0, [PCM_PAD], -x1]).astype(np.int16)
        offs = [[1, 2 * n + 3], [n + 2, 3 * n + 4]]
        nsamp, amp, peak = [n, n], [[1.0, 1.0], [1.0, 1.0]], [1.0, 1.0]
    else:
        raise ValueError(build)
    B = len(nsamp)
    assert all(o % 2 == 1 or build == "silence" for row in offs for o in row)
    assert all(0 <= offs[s][u] and offs[s][u] + nsamp[u] <= len(flat) for s in range(S) for u in range(B))
    return dict(name=name, S=S, B=B, dtype=sp["dtype"], flat=flat, in_offs=np.array(offs, dtype=np.int64), nsamp=np.array(nsamp, dtype=np.int32),
                amp=np.array(amp, dtype=np.float32), peak=np.array(peak, dtype=np.float32), quantize=sp["quantize"], edges=sp["edges"])


def mix_flat(c, dtype):
    """The case's samples in the other format where they have one (int16 -> the same values as float32)."""
    if c["flat"].dtype == np.int16 and dtype == "float32":
        return c["flat"].astype(np.float32) / np.float32(32768.0)
    assert (c["flat"].dtype == np.int16) == (dtype == "int16")
    return c["flat"]


def mix_sources(c, u):
    n = int(c["nsamp"][u])
    return [c["flat"][o:o + n] for o in c["in_offs"][:, u]]


@functools.lru_cache(maxsize=None)
def mix_reference(name):
    """mixing.mix in fp64, unquantized, per mixture: [(mixture, [sources], G)] -- computed once, shared, never written to."""
    c = mix_case(name)
    return [mixing.mix(mix_sources(c, u), c["amp"][:, u], c["peak"][u]) for u in range(c["B"])]


MIX_DEFECTS = ("sums_tail", "max_tail", "threshold", "no_clip")


def mix_model(name, u, defect=None, quantized=False):
    """dynamic_mix_kernel's three passes restated for mixture u, or with a defect: the tail trip (the samples from the last
    multiple of 4096 below n on) left out of the sums or of the maximum, `>` for `>=` at the threshold, no clipping."""
    c = mix_case(name)
    xs = [mixing.as_float(x) for x in mix_sources(c, u)]
    n = len(xs[0])
    tail = MX_TRIP * ((n - 1) // MX_TRIP)
    head = slice(0, tail if (n > MX_TRIP) else n)
    g = []
    for x, a in zip(xs, c["amp"][:, u]):
        P = float(np.sum(x[head] ** 2) if defect == "sums_tail" else np.sum(x * x)) / n
        keep = P > SILENT if defect == "threshold" else P >= SILENT
        g.append(float(a) / np.sqrt(P) if keep else 0.0)
    sel = head if defect == "max_tail" else slice(0, n)
    m = max(float(np.abs(sum(gs * x[sel] for gs, x in zip(g, xs))).max()), max(float(np.abs(gs * x[sel]).max()) for gs, x in zip(g, xs)))
    cc = float(c["peak"][u]) / m if m > 0.0 else 0.0
    G = np.array([gs * cc for gs in g])
    outs = [Gs * x for Gs, x in zip(G, xs)]
    mixture = sum(outs)
    if quantized:
        q = (lambda v: np.rint(v * 32768.0) / 32768.0) if defect == "no_clip" else mixing.quantize
        mixture, outs = q(mixture), [q(o) for o in outs]
    return mixture, outs, G


def mix_gates(S, peak):
    return dict(gains=(S + 5) * EPS24, sources=(S + 6) * EPS24 * peak, mixture=S * (2 * S + 6) * EPS24 * peak)


def mix_ratios(name, got, quantized=False):
    """got[u] = (mixture, [sources], G) against the reference, as fractions of the gates; quantized results are compared exactly
    with mixing.quantize of the reference (the CPU side of the bit-for-bit rule)."""
    c = mix_case(name)
    out = dict(gains=0.0, sources=0.0, mixture=0.0)
    for u, ((mix, srcs, G), (rm, rs, rG)) in enumerate(zip(got, mix_reference(name))):
        gt = mix_gates(c["S"], float(c["peak"][u]))
        if quantized:
            rm, rs, gt = mixing.quantize(rm), [mixing.quantize(s) for s in rs], dict(gt, sources=0.0, mixture=0.0)
        live = rG != 0.0
        out["gains"] = max(out["gains"], _ratio(G[live] / rG[live], 1.0, gt["gains"]), _ratio(G[~live], 0.0, 0.0))
        out["sources"] = max([out["sources"]] + [_ratio(a, b, gt["sources"]) for a, b in zip(srcs, rs)])
        out["mixture"] = max(out["mixture"], _ratio(mix, rm, gt["mixture"]))
    return out


def mix_defect_shows(name, defect):
    c = mix_case(name)
    got = [mix_model(name, u, defect, quantized=c["quantize"]) for u in range(c["B"])]
    return max(mix_ratios(name, got, quantized=c["quantize"]).values()) / MARGIN


# (with ONE source the power cancels: G = peak / max |x| whatever P is -- the S = 1 cases cannot show a wrong sum, and do not claim to)
MIX_DEFECT_CASES = {"sums_tail": [n for n, sp in MIX_SPECS.items() if sp["build"] == "lengths" and sp["S"] >= 2] + ["mix_peaks"],
                    "max_tail": [n for n, sp in MIX_SPECS.items() if sp["build"] == "lengths" and sp["S"] == 1] + ["mix_peaks"],
                    "threshold": ["mix_silence"], "no_clip": ["mix_clip"]}


def _where_max(name, u):
    """(index, 'mixture' or source number) of the largest magnitude among the reference's mixture and sources, and the
    runner-up's share of it among the OTHER signals at any index."""
    mix, srcs, _ = mix_reference(name)[u]
    sig = [np.abs(mix)] + [np.abs(s) for s in srcs]
    tops = [float(s.max()) for s in sig]
    q = int(np.argmax(tops))
    return int(np.argmax(sig[q])), q, max(t for k, t in enumerate(tops) if k != q) / tops[q]


MIX_EDGE_CLAIMS = {
    "lengths": lambda c: tuple(c["nsamp"].tolist()) == MIX_LENGTHS,
    "overlap": lambda c: c["S"] == 1 or any(abs(int(c["in_offs"][0, u] - c["in_offs"][1, u])) < c["nsamp"][u] for u in range(c["B"])),
    "tail_trip": lambda c: {int(n) % MX_TRIP for n in c["nsamp"] if n > MX_TRIP} >= {1, MX_TRIP - 1, 0},
    "peak_alone_in_second_trip": lambda c: c["nsamp"][0] == MX_TRIP + 1 and _where_max(c["name"], 0)[:2] == (MX_TRIP, 0),
    "peak_at_4095": lambda c: c["nsamp"][1] == MX_TRIP and _where_max(c["name"], 1)[:2] == (MX_TRIP - 1, 0),
    "peak_in_mixture_only": lambda c: _where_max(c["name"], 2)[1] == 0 and _where_max(c["name"], 2)[2] <= 0.6,
    "peak_in_one_source_only": lambda c: _where_max(c["name"], 3)[1] == 1 and _where_max(c["name"], 3)[2] <= 0.6,
    "on_threshold": lambda c: float(np.mean(mix_sources(c, 0)[1].astype(np.float64) ** 2)) == SILENT and mix_reference(c["name"])[0][2][1] > 0,
    "below_threshold": lambda c: float(np.mean(mix_sources(c, 1)[1].astype(np.float64) ** 2)) == SILENT / 4 and mix_reference(c["name"])[1][2][1] == 0,
    "all_silent": lambda c: all(not mix_reference(c["name"])[u][2].any() and not mix_reference(c["name"])[u][0].any() for u in (2, 3)),
    "clips_positive": lambda c: c["quantize"] and c["peak"][0] == 1.0 and abs(mix_reference(c["name"])[0][0][700] - 1.0) < 1e-12,
    "minus_one_exact": lambda c: c["quantize"] and c["peak"][1] == 1.0 and abs(mix_reference(c["name"])[1][0][700] + 1.0) < 1e-12,
}


def mix_instantiation(c, dtype=None):
    return "dynamic_mix_kernel<%d, %s>" % (c["S"], "true" if (dtype or c["dtype"]) == "int16" else "false")


def loss_instantiation(c):
    return "%s_sums_kernel<%d>" % (c["kind"], c["S"])


ALL_INSTANTIATIONS = ({"sisdr_sums_kernel<%d>" % S for S in (1, 2, 3, 4)} | {"mixit_sums_kernel<%d>" % M for M in (2, 3, 4)} |
                      {"dynamic_mix_kernel<%d, %s>" % (S, p) for S in (1, 2, 3, 4) for p in ("true", "false")})
