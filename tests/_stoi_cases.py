"""Cases, float64 references and defect models of the STOI kernel tests.

tests/test_gpu_stoi_kernels.py compares stoi_keep_kernel, stoi_env_kernel and stoi_score_kernel (csrc/stoi.hip) with the
references below through sk_stoi's workspace -- kept lists, frame energies, envelopes, scores -- at the lengths their loops
branch on; tests/test_stoi_cases.py proves on any machine that the cases can tell a wrong kernel from a right one.

Signals.  float32 white noise of amplitude 1e-6 with loud runs of amplitude 0.1: a run (a, c) covers samples
[128 a, 128 (a + c - 1) + 256), i.e. frames a .. a + c - 1 whole and half of frames a - 1 and a + c, so the silent-frame rule
keeps exactly frames max(0, a - 1) .. min(F - 1, a + c): c + 2 well inside the signal, c + 1 at its start, and with c = 0
the two frames that share 128 loud samples (one, frame 0, for the run (0, 0)).

Tolerance of an envelope frame t (its 15 bands):  err(t) <= K * E_ref(t) + ulp32(max_band ref(t)), E_ref the error of
sepkern/stoi.py's envelopes(dtype=float32) on that frame, K twice the largest (err - ulp) / E_ref measured on the MI355X,
rounded up (profiles/stoi_kernels.txt) -- the rule of tests/_stft_cases.py.
"""
import functools

import numpy as np

from sepkern import stoi as ST

F32, F64 = np.float32, np.float64

# loop bounds of csrc/stoi.hip (the constants the cases are chosen against)
FRAME, HOP = 256, 128
KEEP = 256                      # stoi_keep_kernel: frames per trip of the scan (one per thread)
WAVE = 64                       # frames per wave of a trip: four ballots, four counts
FPB = 16                        # fft512.h: frames per tile of stoi_env_kernel
BANDS = 15
SSEG = 30                       # frames per segment
STILE = 64                      # segments per LDS tile of stoi_score_kernel
TILE_FRAMES = STILE + SSEG - 1  # frames such a tile loads: 93
GROUPS = 16                     # 16-lane groups of the score kernel: segment ms of a tile goes to group ms % 16
SHORT = 1e-5
BAND_LO = (7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219)   # g_stoi_lo

# measured on the MI355X (profiles/stoi_kernels.txt)
K_ENV = 12                      # envelopes: twice the largest (err - ulp) / E_ref (5.663), rounded up
SCORE_GATE = 16 * 2.0 ** -52    # stoi_score_kernel against scores() in float64 on its own envelopes: 16 x the worst difference
                                # (2.22e-16, one ulp of a score near 1); anything above 1e-9 would be a defect, not summation order

QUIET, LOUD = 1e-6, 0.1
MARGIN_DB = 1.0                 # no frame of a case sits closer to the keep threshold


# ------------------------------------------------------------------------------------------------ launch geometry
def num_frames(n):
    return -(-(n - FRAME) // HOP) if n > FRAME else 0


def length(F, tail=HOP):
    """The n with F >= 1 frames whose last `tail` samples (1 .. 128) no frame covers: n = 256 + 128 F at tail = 128, the
    shortest such n at tail = 1 -- one sample less has F - 1 frames."""
    assert F >= 1 and 1 <= tail <= HOP
    return HOP * (F - 1) + FRAME + tail


def last_read(n):
    """One past the last sample a frame covers."""
    F = num_frames(n)
    return HOP * (F - 1) + FRAME if F else 0


def align(o, a=256):
    return (o + a - 1) // a * a


def workspace(U, S, max_len):
    """stoi_carve: byte offsets of offs | lens | nkept | kept | energy | env, the row stride Fm, the size."""
    Fm = max(1, num_frames(max_len))
    sigs = U * S
    lay, o = {"Fm": Fm}, 0
    for name, nbytes in (("offs", U * 8), ("lens", U * 4), ("nkept", sigs * 4), ("kept", sigs * Fm * 4),
                         ("energy", sigs * Fm * 8), ("env", sigs * (S + 1) * BANDS * Fm * 4)):
        lay[name] = o
        o = align(o + nbytes)
    lay["bytes"] = o
    return lay


def env_row(rj, S, q, band):
    """Row (of Fm floats) of signal q (0: reference j, q >= 1: estimate q - 1) under the keep list of reference rj = u S + j."""
    return (rj * (S + 1) + q) * BANDS + band


# ------------------------------------------------------------------------------------------------ error measures
def ulp32(v):
    return np.spacing(np.asarray(v, F64).astype(F32)).astype(F64)


def frame_err(got, ref):
    """Largest absolute difference over the bands per frame of (15, T) arrays; a non-finite result counts as infinite."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape and got.ndim == 2, (got.shape, ref.shape)
    d = np.abs(got - ref)
    return np.where(np.isfinite(d), d, np.inf).max(axis=0) if d.shape[1] else np.zeros(0)


def env_tolerance(ref, e_ref, k=None):
    return (K_ENV if k is None else k) * np.asarray(e_ref, F64) + ulp32(np.abs(ref).max(axis=0))


def needed_k(err, ref, e_ref):
    """Per frame the smallest k with err <= k * E_ref + ulp (inf: no k does)."""
    over = np.asarray(err, F64) - ulp32(np.abs(ref).max(axis=0))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(over <= 0, 0.0, np.where(np.asarray(e_ref) > 0, over / e_ref, np.inf))


def energy_tolerance(x):
    """Per frame of the fp64 signal x: 1024 x 2^-53 x sum w x^2.  The kernel's window comes from the device's cos, numpy's from
    its own: two ulp of 1 each, i.e. 2^-52 absolute in w, so 2^-51 w x^2 per term of the energy; the rounded product, its
    square and the 256-term sum in any order add at most 260 x 2^-53 x sum w^2 x^2 <= 260 x 2^-53 x sum w x^2."""
    fr = ST._frames(np.asarray(x, F64))
    return 1024.0 * 2.0 ** -53 * (fr * fr * ST.WINDOW).sum(axis=1)


# ------------------------------------------------------------------------------------------------ signals
def expected_kept(F, runs):
    """Frames the rule keeps for loud runs (a, c) that neither touch nor overlap."""
    kept = []
    for a, c in runs:
        kept += list(range(max(0, a - 1), min(F - 1, a + c) + 1))
    assert kept == sorted(set(kept)), runs
    return np.array(kept, np.int64)


def build(n, runs, seed):
    """float32 signal of n samples: noise of amplitude QUIET, loud noise on the runs."""
    rng = np.random.default_rng(seed)
    x = QUIET * rng.standard_normal(n)
    for a, c in runs:
        lo, hi = HOP * a, min(n, HOP * (a + c - 1) + FRAME)
        x[lo:hi] = LOUD * rng.standard_normal(hi - lo)
    return x.astype(F32)


class Case(object):
    """One utterance: S references of one length with their own loud runs (None: an all-zero reference), S estimates.
    estimate k = sum_j MIX[k][j] reference j + GAIN[k] x loud noise, in float32: neither symmetric in (k, j) nor silent anywhere."""

    def __init__(self, name, F, runs, boundary, tail=HOP, n=None):
        self.name, self.F, self.runs, self.boundary = name, F, runs, boundary
        self.S = len(runs)
        self.n = length(F, tail) if n is None else n
        assert num_frames(self.n) == F and self.n < 80000
        self.seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name))

    @functools.lru_cache(maxsize=None)
    def signals(self):
        """(refs, ests): float32 (S, n), clean (no NaN).  Never written to."""
        S, n = self.S, self.n
        refs = np.stack([np.zeros(n, F32) if r is None else build(n, r, self.seed + 17 * j) for j, r in enumerate(self.runs)])
        ests = np.empty_like(refs)
        for k in range(S):
            other = build(n, [(0, self.F + 2)], self.seed + 1000 + k)
            acc = F32(GAIN[k]) * other
            for j in range(S):
                acc = acc + F32(MIX[k][j]) * refs[j]
            ests[k] = acc
        refs.setflags(write=False)
        ests.setflags(write=False)
        return refs, ests

    def claimed_kept(self):
        return [np.zeros(0, np.int64) if r is None else expected_kept(self.F, r) for r in self.runs]

    @functools.lru_cache(maxsize=None)
    def poisoned(self):
        """The signals as the kernels get them: NaN in every sample sk_stoi must not read -- both signals past the last frame
        (sample n - 1 always), the whole of a signal without a frame, an estimate outside the frames some reference keeps."""
        refs, ests = self.signals()
        refs, ests = refs.copy(), ests.copy()
        end = last_read(self.n)
        assert end < self.n
        read = np.zeros(self.n, bool)
        for kept in self.claimed_kept():
            for f in kept:
                read[HOP * f:HOP * f + FRAME] = True
        assert not read[end:].any()
        refs[:, end:] = np.nan
        ests[:, ~read] = np.nan
        return refs, ests

    @functools.lru_cache(maxsize=None)
    def host(self):
        """Everything the GPU test compares with, from sepkern/stoi.py on the clean signals, computed once:
        kept[j], energy[j] (F,), etol[j] (F,), T[j], env[j][q] (15, T) float64, e_ref[j][q] (T,), m64 / m32 (S, S, 2), frames."""
        refs, ests = self.signals()
        S = self.S
        h = dict(kept=[], energy=[], etol=[], T=[], env=[], e_ref=[])
        for j in range(S):
            kept = ST.kept_frames(refs[j])
            fr = ST._frames(refs[j].astype(F64)) * ST.WINDOW
            h["kept"].append(kept)
            h["energy"].append((fr * fr).sum(axis=1))
            h["etol"].append(energy_tolerance(refs[j]))
            h["T"].append(max(len(kept) - 1, 0))
            e64 = [ST.envelopes(x, kept) for x in [refs[j]] + list(ests)]
            e32 = [ST.envelopes(x, kept, F32) for x in [refs[j]] + list(ests)]
            assert all(e.dtype == F32 for e in e32)
            h["env"].append(e64)
            h["e_ref"].append([frame_err(a, b) for a, b in zip(e32, e64)])
        h["m64"], h["frames"] = ST.stoi_matrix(list(refs), list(ests))
        h["m32"], fr32 = ST.stoi_matrix(list(refs), list(ests), dtype=F32)
        assert fr32.tolist() == h["frames"].tolist() == h["T"]
        return h

    def check_claims(self):
        """From the host definition alone: the F, nkept and T the case claims, and no frame near the keep threshold."""
        refs, _ = self.signals()
        assert ST.frame_starts(self.n).size == self.F == num_frames(self.n)
        margins = []
        for j, want in enumerate(self.claimed_kept()):
            got = ST.kept_frames(refs[j])
            assert got.tolist() == want.tolist(), (self.name, j, got, want)
            if self.runs[j] is not None and self.F:
                margins.append(float(np.abs(ST.keep_margins(refs[j])).min()))
                assert margins[-1] > MARGIN_DB, (self.name, j, margins[-1])
        return margins

    def nkept(self):
        return [len(k) for k in self.claimed_kept()]

    def T(self):
        return [max(k - 1, 0) for k in self.nkept()]


GAIN = (0.5, 0.75, 1.0, 1.25)
MIX = ((1.0, 0.20, 0.30, 0.40),
       (0.35, 1.0, 0.15, 0.25),
       (0.10, 0.45, 1.0, 0.05),
       (0.30, 0.10, 0.20, 1.0))


def _one(name, F, runs, boundary, tail=HOP):
    return Case(name, F, [runs], boundary, tail)


def _cases():
    c = []
    # the scan of stoi_keep_kernel, every frame kept: one trip less a frame, one trip, a trip and a frame, two, two and a frame
    for F, tail in ((255, 128), (256, 1), (257, 128), (512, 1), (513, 64)):
        c.append(_one("all%d" % F, F, [(0, F)], "scan: F = %d, every frame kept, %d trips" % (F, -(-F // KEEP)), tail))
    # the scan, sparse
    c.append(_one("trip1_only", 400, [(300, 40)], "scan: kept frames in the second trip only (carry 0)"))
    c.append(_one("across_255_256", 300, [(250, 10)], "scan: a run across frames 255 | 256", 1))
    c.append(_one("across_511_512", 520, [(505, 12)], "scan: a run across frames 511 | 512"))
    c.append(_one("trips_0_2", 600, [(10, 35), (530, 20)], "scan: trips 0 and 2 keep frames, trip 1 none", 1))
    c.append(_one("waves", 500, [(60, 8), (188, 8), (316, 8), (444, 8)],
                  "scan: runs across the wave boundaries 63 | 64 and 191 | 192 of trips 0 and 1"))
    # tiles of stoi_env_kernel
    c.append(_one("T15", 40, [(0, 15)], "env: T = 15, a tile less a frame", 1))
    c.append(_one("T16", 40, [(0, 16)], "env: T = 16, one whole tile"))
    c.append(_one("T17_far", 140, [(0, 15), (101, 0)], "env: T = 17, prv of t = 16 is frame 15, cur frame 100"))
    c.append(_one("T31", 60, [(0, 31)], "env: T = 31; score: J = 2"))
    c.append(_one("T32_far", 140, [(0, 29), (101, 1)], "env: T = 32, two whole tiles, kept frames 29 | 100 inside a tile", 1))
    c.append(_one("T33_far", 230, [(0, 31), (201, 0)], "env: T = 33, prv of t = 32 is frame 31, cur frame 200"))
    c.append(_one("T1", 30, [(1, 0)], "env: T = 1 (nkept = 2)"))
    c.append(_one("nkept1", 30, [(0, 0)], "env: nkept = 1, T = 0", 1))
    c.append(_one("nkept0", 40, None, "env: an all-zero reference, nkept = 0"))
    # tiles of stoi_score_kernel
    c.append(_one("T29", 50, [(0, 29)], "score: T = 29, short"))
    c.append(_one("T30", 50, [(5, 29)], "score: T = 30, J = 1", 1))
    c.append(_one("T45", 70, [(0, 45)], "score: T = 45, J = 16: every group one segment"))
    c.append(_one("T46", 70, [(9, 45)], "score: T = 46, J = 17: group 0 takes a second segment"))
    c.append(_one("T93", 110, [(0, 93)], "score: T = 93, J = 64: one whole tile", 1))
    c.append(_one("T94", 110, [(5, 93)], "score: T = 94, J = 65: the second tile holds exactly 30 frames"))
    c.append(_one("T157", 170, [(0, 157)], "score: T = 157, J = 128: two whole tiles"))
    c.append(_one("T158", 170, [(3, 157)], "score: T = 158, J = 129: a third tile of 30 frames", 1))
    # degenerate lengths
    c.append(Case("n1", 0, [[(0, 1)]], "n = 1: no frame", n=1))
    c.append(Case("n256", 0, [[(0, 1)]], "n = 256: no frame", n=256))
    c.append(Case("n257", 1, [[(0, 1)]], "n = 257: one frame", n=257))
    # S >= 2: the references of an utterance keep different frames; one T below 30 and one above
    c.append(Case("s2_a", 120, [[(0, 20)], [(30, 39)]], "S = 2: T = 20, 40"))
    c.append(Case("s2_b", 60, [[(0, 35)], [(40, 10)]], "S = 2: T = 35, 11", 1))
    c.append(Case("s3_a", 100, [[(20, 9)], [(0, 33)], [(30, 63)]], "S = 3: T = 10, 33, 64", 1))
    c.append(Case("s3_b", 70, [[(0, 31)], [(50, 4)], [(10, 44)]], "S = 3: T = 31, 5, 45"))
    c.append(Case("s4_a", 130, [[(100, 11)], [(0, 30)], [(40, 46)], [(20, 93)]], "S = 4: T = 12, 30, 47, 94"))
    c.append(Case("s4_b", 50, [[(0, 29)], [(10, 34)], None, [(30, 15)]], "S = 4: T = 29, 35, 0 (all-zero), 16", 1))
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def group(S):
    """The cases of S sources in the order of their mixed batch."""
    return [c for c in CASES if c.S == S]


def other_order(cases):
    """The same batch in another order (fixed)."""
    idx = [int(i) for i in np.random.default_rng(len(cases)).permutation(len(cases))]
    if idx == list(range(len(cases))):
        idx = idx[::-1]
    return idx


def check_claims():
    """What the cases claim about the kernels' loop bounds; a constant that moved fails here.  -> the smallest keep margin."""
    assert (FRAME, HOP, KEEP, WAVE, FPB, SSEG, STILE, TILE_FRAMES) == (256, 128, 256, 64, 16, 30, 64, 93)
    assert BAND_LO == tuple([lo for lo, _ in ST.BAND_EDGES] + [ST.BAND_EDGES[-1][1]])
    assert [num_frames(n) for n in (1, 256, 257, 384, 385, 33024, 33025)] == [0, 0, 1, 1, 2, 256, 257]
    assert length(257, 1) == 33025 and num_frames(length(257, 1) - 1) == 256          # the second trip needs n >= 33025
    margins = []
    for c in CASES:
        margins += c.check_claims()
    trips = lambda name: sorted(set(int(f) // KEEP for f in BY_NAME[name].claimed_kept()[0]))     # noqa: E731
    waves = lambda name: sorted(set(int(f) // WAVE for f in BY_NAME[name].claimed_kept()[0]))     # noqa: E731
    for F in (255, 256, 257, 512, 513):
        assert BY_NAME["all%d" % F].claimed_kept()[0].tolist() == list(range(F))
    assert trips("all255") == trips("all256") == [0] and trips("all257") == trips("all512") == [0, 1] and trips("all513") == [0, 1, 2]
    assert trips("trip1_only") == [1] and trips("across_255_256") == [0, 1] and trips("across_511_512") == [1, 2]
    assert trips("trips_0_2") == [0, 2] and BY_NAME["trips_0_2"].F > 2 * KEEP
    assert waves("waves") == [0, 1, 2, 3, 4, 5, 6, 7]
    T1 = lambda name: BY_NAME[name].T()[0]                                                         # noqa: E731
    assert [T1(n) for n in ("T15", "T16", "T17_far", "T31", "T32_far", "T33_far", "T1", "nkept1", "nkept0")] == [15, 16, 17, 31, 32, 33, 1, 0, 0]
    assert [BY_NAME[n].nkept()[0] for n in ("T1", "nkept1", "nkept0")] == [2, 1, 0]
    for name, t, a, b in (("T17_far", 16, 15, 100), ("T33_far", 32, 31, 200)):     # prv of a tile's first frame lies far from cur
        kp = BY_NAME[name].claimed_kept()[0]
        assert t % FPB == 0 and kp[t - 1] == a and kp[t] == b
    kp = BY_NAME["T32_far"].claimed_kept()[0]
    assert kp[29] == 29 and kp[30] == 100
    assert [T1("T%d" % t) for t in (29, 30, 45, 46, 93, 94, 157, 158)] == [29, 30, 45, 46, 93, 94, 157, 158]
    J = lambda t: t - SSEG + 1                                                                     # noqa: E731
    assert J(29) == 0 and J(30) == 1 and J(45) == GROUPS and J(46) == GROUPS + 1 and J(93) == STILE and J(94) == STILE + 1
    assert min(TILE_FRAMES, 94 - STILE) == SSEG and J(157) == 2 * STILE and min(TILE_FRAMES, 158 - 2 * STILE) == SSEG
    assert [BY_NAME[n].F for n in ("n1", "n256", "n257")] == [0, 0, 1] and BY_NAME["n257"].nkept() == [1]
    assert sorted(set(c.S for c in CASES)) == [1, 2, 3, 4]
    for c in CASES:
        if c.S >= 2:
            T = c.T()
            assert min(T) < SSEG <= max(T) and len(set(T)) == c.S, (c.name, T)
            assert len(set(tuple(k) for k in c.claimed_kept())) == c.S
    for S in (1, 2, 3, 4):                       # in the mixed batch all but the longest get another utterance's F as row stride
        Fs = [c.F for c in group(S)]
        assert len(Fs) >= 2 and sum(F == max(Fs) for F in Fs) == 1
        assert other_order(group(S)) != list(range(len(Fs)))
    return min(margins)


# ------------------------------------------------------------------------------------------------ models of the three kernels
KEEP_DEFECTS = ("carry_lost", "carry_twice", "wave_dropped")
ENV_DEFECTS = ("nxt_adjacent", "no_prv_at_tile", "tail_tile_dropped", "bands_shifted", "est_index")
SCORE_DEFECTS = ("drop_m64", "tile_short", "J_less_one", "transposed")
OTHER_DEFECTS = ("kept_stride_F", "T_is_nkept")


def scan(flags, defect=None):
    """stoi_keep_kernel's scan of the keep flags, trip by trip and wave by wave -> (kept row of F entries, -1 where nothing
    was written, nkept).  defect: the carry between trips lost, added twice, wave 0's count dropped from the prefix."""
    flags = np.asarray(flags, bool)
    F = len(flags)
    kept, base = np.full(F, -1, np.int64), 0
    for c0 in range(0, F, KEEP):
        trip = flags[c0:c0 + KEEP]
        wcnt = [int(trip[w * WAVE:(w + 1) * WAVE].sum()) for w in range(KEEP // WAVE)]
        for i in np.nonzero(trip)[0]:
            wave, lane = divmod(int(i), WAVE)
            before = int(trip[wave * WAVE:wave * WAVE + lane].sum())
            first = 1 if defect == "wave_dropped" and wave >= 2 else 0
            pos = base + before + sum(wcnt[first:wave])
            if 0 <= pos < F:
                kept[pos] = c0 + i
        if defect == "carry_lost":
            base = sum(wcnt)
        elif defect == "carry_twice":
            base += 2 * sum(wcnt)
        else:
            base += sum(wcnt)
    return kept, base


def keep_flags(x):
    """The 40 dB rule on the fp64 energies, as the kernel evaluates it."""
    fr = ST._frames(np.asarray(x, F64)) * ST.WINDOW
    en = (fr * fr).sum(axis=1)
    if not len(en) or not en.max() > 0.0:
        return np.zeros(len(en), bool)
    db = 20.0 * np.log10(np.sqrt(en) + ST.EPS)
    return db > db.max() - 40.0


def kept_rows(cases, defect=None):
    """The kept region of the workspace for a batch, -1 where nothing is written: rows of Fm entries, the kernel's stride.
    defect kept_stride_F: every signal's row starts at sig * F of its own utterance."""
    S = cases[0].S
    Fm = max(1, max(c.F for c in cases))
    ws = np.full(len(cases) * S * Fm, -1, np.int64)
    for u, c in enumerate(cases):
        refs, _ = c.signals()
        for j in range(S):
            row, nk = scan(keep_flags(refs[j]))
            sig = u * S + j
            o = sig * (c.F if defect == "kept_stride_F" else Fm)
            ws[o:o + nk] = row[:nk]
    return ws.reshape(len(cases) * S, Fm)


def envelope_model(x, kept, defect=None):
    """(15, T) float64 envelopes the way stoi_env_kernel forms them: frame t of the rebuilt signal gathered from the kept
    frames k_{t-1}, k_t, k_{t+1}.  defect: nxt read from frame k_t + 1, prv missing at a tile's first frame, the last partial
    tile not written (NaN), band edges one bin up."""
    x = np.asarray(x, F64)
    kept = [int(k) for k in kept]
    T = max(len(kept) - 1, 0)
    w = ST.WINDOW
    fr = np.zeros((T, FRAME))
    for t in range(T):
        cur = w * x[HOP * kept[t]:HOP * kept[t] + FRAME]
        knext = kept[t] + 1 if defect == "nxt_adjacent" else kept[t + 1]
        nxt = w[:HOP] * x[HOP * knext:HOP * knext + HOP]
        fr[t, HOP:] = cur[HOP:] + nxt
        fr[t, :HOP] = cur[:HOP]
        if t > 0 and not (defect == "no_prv_at_tile" and t % FPB == 0):
            fr[t, :HOP] = w[HOP:] * x[HOP * kept[t - 1] + HOP:HOP * kept[t - 1] + FRAME] + cur[:HOP]
    spec = np.fft.rfft(fr * w, n=ST.NFFT, axis=-1)
    p = spec.real * spec.real + spec.imag * spec.imag
    sh = 1 if defect == "bands_shifted" else 0
    env = np.stack([np.sqrt(p[:, lo + sh:hi + sh].sum(axis=1)) for lo, hi in zip(BAND_LO[:-1], BAND_LO[1:])]).reshape(BANDS, T)
    if defect == "tail_tile_dropped" and T % FPB:
        env[:, T // FPB * FPB:] = np.nan
    return env


def envelope_rows(case, j, defect=None):
    """The S + 1 envelope arrays under reference j's keep list.  defect est_index: signal q >= 1 read from estimate q (the last
    one from estimate S - 1 again) instead of q - 1."""
    refs, ests = case.signals()
    kept = ST.kept_frames(refs[j])
    rows = [refs[j]] + [ests[min(q, case.S - 1) if defect == "est_index" else q - 1] for q in range(1, case.S + 1)]
    return [envelope_model(x, kept, None if defect == "est_index" else defect) for x in rows]


def segment_scores(X, Y):
    """(J, 2): STOI and ESTOI sums of every segment (before the division by 15 J / 30 J), float64."""
    eps = ST.EPS
    xs, ys = ST._segments(X), ST._segments(Y)
    c = np.sqrt((xs * xs).sum(axis=-1, keepdims=True)) / (np.sqrt((ys * ys).sum(axis=-1, keepdims=True)) + eps)
    yp = np.minimum(c * ys, xs * (1.0 + 10.0 ** (-ST.BETA / 20.0)))
    d = (ST._norm_rows(xs, eps) * ST._norm_rows(yp, eps)).sum(axis=(1, 2))
    xr, yr = ST._norm_rows(xs, eps), ST._norm_rows(ys, eps)
    xc = np.swapaxes(ST._norm_rows(np.swapaxes(xr, 1, 2), eps), 1, 2)
    yc = np.swapaxes(ST._norm_rows(np.swapaxes(yr, 1, 2), eps), 1, 2)
    return np.stack([d, (xc * yc).sum(axis=(1, 2))], axis=1)


def score_model(X, Y, defect=None):
    """(stoi, estoi) of (15, T) envelopes the way stoi_score_kernel walks them, float64.  defect: segments m >= 64 dropped, every
    tile after the first loaded one frame short (its last frame zero), one segment too few."""
    X, Y = np.asarray(X, F64), np.asarray(Y, F64)
    T = X.shape[1]
    if T < SSEG:
        return SHORT, SHORT
    J = T - SSEG + 1
    tot = np.zeros(2)
    for m0 in range(0, J, STILE):
        if defect == "drop_m64" and m0 > 0:
            break
        nt = min(TILE_FRAMES, T - m0)
        if defect == "tile_short" and m0 > 0:
            nt -= 1
        xs, ys = np.zeros((BANDS, TILE_FRAMES)), np.zeros((BANDS, TILE_FRAMES))
        xs[:, :nt], ys[:, :nt] = X[:, m0:m0 + nt], Y[:, m0:m0 + nt]
        ns = min(STILE, J - m0 - (1 if defect == "J_less_one" and m0 + STILE >= J else 0))
        if ns > 0:
            tot += segment_scores(xs[:, :ns + SSEG - 1], ys[:, :ns + SSEG - 1]).sum(axis=0)
    Jd = J - 1 if defect == "J_less_one" else J
    if Jd < 1:
        return SHORT, SHORT
    return tot[0] / (BANDS * Jd), tot[1] / (SSEG * Jd)


def matrix_model(case, defect=None):
    """(out (S, S, 2), frames (S,)) from the models above, sk_stoi's layout.  defect: any of SCORE_DEFECTS, T_is_nkept (frames)."""
    refs, ests = case.signals()
    S = case.S
    out, frames = np.zeros((S, S, 2)), np.zeros(S, np.int64)
    for j in range(S):
        kept = ST.kept_frames(refs[j])
        frames[j] = len(kept) if defect == "T_is_nkept" else max(len(kept) - 1, 0)
        rows = envelope_rows(case, j)
        for k in range(S):
            out[k, j] = score_model(rows[0], rows[1 + k], defect if defect in SCORE_DEFECTS else None)
    if defect == "transposed":
        out = np.swapaxes(out, 0, 1).copy()
    return out, frames
