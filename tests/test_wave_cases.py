"""The pin suite of the waveform losses and the dynamic mix on any machine: what tests/test_gpu_wave_cases.py runs on the device
reaches what it claims (cases, gates and defect models: tests/_wave_cases.py).

1. The restated host code is the sources': CHUNK, the two nq_of, g_index, the workspace formulas, MX_THREADS and MX_UNROLL against
   the text of wave_loss.h, sisdr.hip, mixit.hip and mix.hip and, where the library loads, against the two size queries.
2. Every case's edge predicates hold; the table reaches every instantiation (sisdr_sums_kernel<1..4>, mixit_sums_kernel<2..4>,
   dynamic_mix_kernel<1..4, int16 | float32>), every listed length, both sides of every 256 wrap, every degenerate branch and
   every tie -- and each case is the only one on some edge, so removing one fails a coverage assertion.  -s prints the report.
3. Conditioning: every drawn decision leads by 1 dB, every tie is exact, 4 x the reference's spread stays below the rounding
   term of every SI-SDR gate, the degenerate utterances' sums are the same bits in three orders of summation.
4. Every defect model moves a checked output by at least 10 x its gate (or flips a decision) on every case that names it, and
   every defect is named by a case.
"""
import os
import re

import numpy as np
import pytest

import _wave_cases as WC
from conftest import PKG
from sepkern import mixing, mixit


def _src(name):
    return open(os.path.join(PKG, "csrc", name)).read()


# ------------------------------------------------------------------------------------------------ 1: the restatement
def test_the_restated_constants_are_the_sources():
    wl, si, mi, mx = _src("wave_loss.h"), _src("sisdr.hip"), _src("mixit.hip"), _src("mix.hip")
    assert "constexpr int CHUNK = %d;" % WC.CHUNK in wl
    assert "for (int idx = threadIdx.x; idx < B * NQ; idx += %d)" % WC.THREADS in wl
    assert "(nsamp[u] + CHUNK - 1) / CHUNK" in wl
    assert "return sk_align((size_t)B * sk_cdiv(max_samples, CHUNK) * NQ * sizeof(double), %d);" % WC.ALIGN in wl
    assert "constexpr int nq_of(int S) { return 4 * S + S * S; }" in si
    assert "constexpr int nq_of(int M) { return 2 + 2 * M + M * (M + 1) / 2; }" in mi
    assert "constexpr int g_index(int M, int k, int l) { return 2 + 2 * M + k * M - k * (k - 1) / 2 + (l - k); }" in mi
    assert "constexpr int NREF = %d;" % WC.NREF in mi and "constexpr int NQMAX = 2 + 2 * MAXM + MAXM * (MAXM + 1) / 2;" in mi
    for text in (si, mi):
        assert len(re.findall(r"for \(int u = threadIdx\.x; u < B; u \+= %d\)" % WC.THREADS, text)) == 1
        assert "dim3(%d)" % WC.THREADS in text and "B > 0 && B <= 65535" in text
    assert "partial_bytes(B, nq_of(S), max_samples) + sk_align((size_t)B * (1 + 3 * MAXS * MAXS) * sizeof(double), 256)" in si
    assert "partial_bytes(B, nq_of(M), max_samples) + sk_align((size_t)B * (1 + NQMAX) * sizeof(double), 256)" in mi
    assert "if (B <= 0 || S < 1 || S > MAXS || max_samples <= 0) return 0;" in si
    assert "if (B <= 0 || M < 2 || M > MAXM || max_samples <= 0) return 0;" in mi
    assert "constexpr int MX_THREADS = %d;" % WC.MX_THREADS in mx and "constexpr int MX_UNROLL = %d;" % WC.MX_UNROLL in mx
    assert mx.count("i0 += MX_UNROLL * MX_THREADS") == 3 and "constexpr double MX_SILENT = 1.0 / 1099511627776.0;" in mx
    assert WC.SILENT == 1.0 / 1099511627776.0 == mixing.SILENT and WC.MAXS == mixing.MAX_SOURCES == mixit.MAX_EST
    assert "#define SK_MAXS %d" % WC.MAXS in _src("sk_common.h") and "constexpr int MAXS = SK_MAXS;" in si and "constexpr int MAXM = SK_MAXS;" in mi
    # g_index walks the row-major upper triangle behind P and c, and nq_of counts it
    for M in (2, 3, 4):
        assert [WC.g_index(M, k, l) for k in range(M) for l in range(k, M)] == list(range(2 + 2 * M, WC.mixit_nq(M)))
    assert [WC.sisdr_nq(S) for S in (1, 2, 3, 4)] == [5, 12, 21, 32] and [WC.mixit_nq(M) for M in (2, 3, 4)] == [9, 14, 20]
    assert WC.NQMAX == 20 and 2 * WC.MAXS ** 2 >= WC.sisdr_nq(WC.MAXS)


def _documented(kind, B, S, max_samples):
    """The workspace as include/sepkern.h and the two files' comments state it, written out once more."""
    up = lambda n: (n + 255) // 256 * 256                                          # noqa: E731
    nch = (max_samples + 4095) // 4096
    if kind == "sisdr":
        return up(8 * B * nch * (4 * S + S * S)) + up(8 * B * (1 + 16 + 32))
    return up(8 * B * nch * (2 + 2 * S + S * (S + 1) // 2)) + up(8 * B * (1 + 20))


def test_the_restated_workspaces_are_the_librarys():
    from sepkern import _lib
    try:
        lib = _lib.load()
    except _lib.SepkernError:
        lib = None
    for kind, fn in (("sisdr", "sk_sisdr_workspace_bytes"), ("mixit", "sk_mixit_workspace_bytes")):
        for B in (1, 9, 32, 256, 257, 65535):
            for S in (1, 2, 3, 4):
                for ms in (1, 4095, 4096, 4097, 64000):
                    want = WC.workspace_bytes(kind, B, S, ms)
                    assert want == (0 if kind == "mixit" and S == 1 else _documented(kind, B, S, ms)), (kind, B, S, ms)
                    if lib is not None:
                        assert getattr(lib, fn)(B, S, ms) == want, (kind, B, S, ms)
        for bad in ((0, 2, 100), (-1, 2, 100), (4, 0, 100), (4, 5, 100), (4, 2, 0), (4, 2, -5)):
            assert WC.workspace_bytes(kind, *bad) == 0 and (lib is None or getattr(lib, fn)(*bad) == 0), (kind, bad)
    for name in WC.LOSS_CASES:                                                       # the sums of every case fit their block
        c = WC.loss_case(name)
        assert WC.workspace_bytes(c["kind"], c["B"], c["S"], c["max_samples"]) > 0 and c["nsamp"].max() <= c["max_samples"]


# ------------------------------------------------------------------------------------------------ 2: claims and coverage
def test_every_claim_holds_and_the_table_reaches_every_edge():
    seen, edges, report = set(), {}, []
    for name in WC.LOSS_CASES:
        c = WC.loss_case(name)
        for e in c["edges"]:
            assert WC.LOSS_EDGE_CLAIMS[e](c), (name, e)
            edges.setdefault((c["kind"], c["S"], e), []).append(name)
        seen.add(WC.loss_instantiation(c))
        items = c["B"] * WC.nq_of(c["kind"], c["S"])
        report.append("%-24s %-22s B=%3d items=%5d (%s 256) chunks %s of %d  %s" % (
            name, WC.loss_instantiation(c), c["B"], items, ">" if items > 256 else "<=",
            sorted(set(WC.chunks_of(int(n)) for n in c["nsamp"])), c["nch"], " ".join(c["edges"])))
        assert c["nsamp"].min() >= 1 and c["nsamp"].max() <= c["max_samples"]        # the contract: never nsamp > max_samples
    for name in WC.MIX_CASES:
        c = WC.mix_case(name)
        for e in c["edges"]:
            assert WC.MIX_EDGE_CLAIMS[e](c), (name, e)
            edges.setdefault(("mix", c["S"], c["dtype"], e), []).append(name)
        seen.add(WC.mix_instantiation(c))
        if c["flat"].dtype == np.int16:                                              # an int16 case also runs as its float32 copy
            seen.add(WC.mix_instantiation(c, "float32"))
        report.append("%-24s %-32s B=%2d trips %s  %s" % (name, WC.mix_instantiation(c), c["B"], sorted(set(WC.mix_trips(int(n)) for n in c["nsamp"])),
                                                          " ".join(c["edges"])))
    print("\n".join("wave_cases coverage: " + r for r in report))
    assert seen == WC.ALL_INSTANTIATIONS and len(seen) == 15
    for kind, counts in (("sisdr", (1, 2, 3, 4)), ("mixit", (2, 3, 4))):
        for S in counts:                              # per instantiation: every length, both sides of the item wrap, a ragged grid
            for e in ("lengths", "below_wrap", "first_above_wrap", "above_wrap", "ragged", "shared_ref", "minus_full_scale", "odd_offsets"):
                assert edges.get((kind, S, e)), (kind, S, e)
            if S >= 2:
                assert edges.get((kind, S, "tie")), (kind, S)
            B = WC.wrap_batch(kind, S)
            assert (B - 1) * WC.nq_of(kind, S) <= 256 < B * WC.nq_of(kind, S)
            assert {"%s_wrap_%d_B%d" % (kind, S, B - 1), "%s_wrap_%d_B%d" % (kind, S, B)} <= set(WC.LOSS_CASES)
        assert any(e[0] == kind and e[2] == "u_below_wrap" for e in edges) and any(e[0] == kind and e[2] == "u_above_wrap" for e in edges)
    assert edges[("sisdr", 2, "training_batch")] and edges[("mixit", 4, "training_batch")]
    assert WC.loss_case("sisdr_train_2_B32")["B"] * WC.sisdr_nq(2) == 384 and WC.loss_case("mixit_train_4_B32")["B"] * WC.mixit_nq(4) == 640
    for e in ("silent_ref", "orthogonal", "exact_copy", "one_sample", "two_samples"):
        assert edges.get(("sisdr", 1, e)) and edges.get(("sisdr", 2, e)), e
    for e in ("both_silent", "exact_partition"):
        assert len(edges[("mixit", 3, e)]) == 2
    assert edges[("mixit", 3, "tau0")] and edges[("mixit", 3, "tau1")]
    counts = {True: 0, False: 0}
    for name in WC.LOSS_CASES:
        counts[WC.loss_case(name)["count"] is None] += 1
    assert counts[True] >= 7 and counts[False] >= 7                                  # the default count and a count_dev scalar
    for S in (1, 2, 3, 4):
        for dtype in ("int16", "float32"):
            assert edges.get(("mix", S, dtype, "lengths")) and edges.get(("mix", S, dtype, "tail_trip"))
    for e in WC.MIX_EDGE_CLAIMS:
        assert any(k[0] == "mix" and k[3] == e for k in edges), e
    # every case is the only one on some edge: the table has no case that could leave unnoticed
    for name in WC.LOSS_CASES + WC.MIX_CASES:
        assert any(v == [name] for v in edges.values()), name


def test_the_lengths_sit_on_the_loop_edges():
    assert WC.LENGTHS == (1, 2, 255, 256, 257, 4095, 4096, 4097, 8192, 8193, 12289)
    assert WC.MIX_LENGTHS == (1, 63, 64, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193)
    assert [WC.chunks_of(n) for n in WC.LENGTHS] == [1, 1, 1, 1, 1, 1, 1, 2, 2, 3, 4]
    assert [n % WC.CHUNK for n in (4097, 8193, 12289)] == [1, 1, 1] and 8192 % WC.CHUNK == 0
    assert [WC.mix_trips(n) for n in WC.MIX_LENGTHS] == [1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 3]
    for name in WC.LOSS_CASES:
        c = WC.loss_case(name)
        if "lengths" in c["edges"]:
            assert any(c["nch"] > WC.chunks_of(int(n)) and int(n) % WC.CHUNK == 1 for n in c["nsamp"])
            # the pads: NaN around every estimate, around every float32 reference
            for j in range(c["B"]):
                for o in c["est_offs"][j]:
                    assert np.isnan(c["est"][o - 1]) and np.isnan(c["est"][o + c["nsamp"][j]]) and not np.isnan(c["est"][o:o + c["nsamp"][j]]).any()
                for o in c["ref_offs"][j]:
                    assert np.isnan(c["ref32"][o - 1]) and not np.isnan(c["ref32"][o:o + c["nsamp"][j]]).any()
        assert np.array_equal(c["ref32"][~np.isnan(c["ref32"])].astype(np.float64) * 32768.0, c["pcm"][~np.isnan(c["ref32"])].astype(np.float64))


# ------------------------------------------------------------------------------------------------ 3: conditioning
@pytest.mark.parametrize("name", WC.LOSS_CASES)
def test_decisions_are_clear_or_exact_ties_and_the_spread_stays_below_the_rounding(name):
    c, ref = WC.loss_case(name), WC.loss_reference(name)
    model = WC.loss_model(name)
    worst = dict(pair=0.0, score=0.0, coef=0.0)
    ties, least = [], np.inf
    for j, w in enumerate(ref["utts"]):
        tie = WC.expected_tie(c, j)
        if c["kinds"][j] == "tie":
            assert tie is not None, (name, j)
        if tie is None:
            assert w["gap"] >= WC.GAP_DB, (name, j, w["gap"])
            least = min(least, w["gap"])
        else:                                         # exact in the reference AND in the kernel's restated arithmetic; the rest is far
            ties.append((j, tie))
            assert w["best"] == tie[0] and w["gap"] == 0.0
            m = model["utts"][j]["score"]
            assert m[tie[0]] == m[tie[1]] == m.max() and int(np.argmax(m)) == tie[0]
            below = m[m < m.max()]
            assert below.size == 0 or m.max() - below.max() >= WC.GAP_DB, (name, j)
        if c["kind"] == "sisdr":
            for key in worst:
                r = w["round"][key]
                assert np.all(4.0 * w["spread"][key] <= r), (name, j, key, float((4.0 * w["spread"][key] - r).max()))
                worst[key] = max(worst[key], float(np.max(np.where(r > 0, 4.0 * w["spread"][key] / np.where(r > 0, r, 1.0), 0.0))))
        if c["kinds"][j] not in ("noisy", "tie"):     # exact numbers: the same bits in three orders, zero spread
            a, b, d = WC.sums_in_three_orders(c, j)
            assert np.array_equal(a, b) and np.array_equal(a, d), (name, j)
            if c["kind"] == "sisdr":
                assert not any(w["spread"][key][np.asarray(w[key]) == 0.0].any() for key in ("coef",))
    # the restated arithmetic is the definition (so the defect models are variants of what the reference computes)
    ratios = WC.loss_ratios(name, model)
    assert max(ratios.values()) <= 1e-3, ratios
    spread = "4 x spread / rounding term: pair %.2g score %.2g coef %.2g" % (worst["pair"], worst["score"], worst["coef"])
    print("wave_cases cpu %-24s least decision margin %6.2f dB, ties (utterance, (first, last)) %s, %s"
          % (name, least, ties, spread if c["kind"] == "sisdr" else "no spread term in the MixIT gates"))


def test_the_degenerate_branches_are_taken():
    for S in (1, 2):
        c, ref = WC.loss_case("sisdr_degenerate_%d" % S), WC.loss_reference("sisdr_degenerate_%d" % S)
        for j, what in enumerate(c["kinds"]):
            w = ref["utts"][j]
            sums = np.sum(WC.chunk_rows(c, j), axis=0)
            n = float(c["nsamp"][j])
            abc = [[(sums[4 * S + k * S + i] - sums[k] * sums[S + i] / n, sums[3 * S + i] - sums[S + i] ** 2 / n, sums[2 * S + k] - sums[k] ** 2 / n)
                    for i in range(S)] for k in range(S)]
            if what == "silent":
                assert all(abc[k][0][1] == 0.0 for k in range(S)) and not w["coef"][[k for k in range(S) if _ref_of(S, w["best"], k) == 0]].any()
            elif what == "orthogonal":
                assert all(abc[k][i][0] == 0.0 and abc[k][i][1] > 0 and abc[k][i][2] > 0 for k in range(S) for i in range(S)) and not w["coef"].any()
            elif what in ("copy", "two"):
                for k in range(S):
                    a, b, cc = abc[k][_ref_of(S, w["best"], k)]
                    assert b > 0 and a != 0 and cc - (a / b) * a == 0.0
                assert not w["coef"].any()
            elif what == "one":
                assert all(v == 0.0 for row in abc for t in row for v in t) and not w["coef"].any() and not w["pair"].any()
            assert np.all(np.isfinite(w["pair"])) and np.all(np.isfinite(w["coef"]))
    for name in ("mixit_degenerate_tau0", "mixit_degenerate_tau1"):
        c, ref = WC.loss_case(name), WC.loss_reference(name)
        for j, what in enumerate(c["kinds"]):
            w = ref["utts"][j]
            if what == "silent":
                assert not w["P"].any() and w["best"] == 0 and w["coef"][1] == 0.0 and w["coef"][0] > 0
            elif what == "partition":
                assert not w["err"].any() and w["P"].all()
                assert (not w["coef"].any()) if c["tau"] == 0.0 else w["coef"].all()
            else:
                assert w["coef"].all()
            assert np.all(np.isfinite(w["score"])) and np.all(np.isfinite(w["coef"]))
    assert WC.loss_case("mixit_degenerate_tau0")["tau"] == 0.0 and WC.loss_case("mixit_degenerate_tau1")["tau"] == 1.0
    assert WC.loss_case("mixit_lengths_3")["tau"] == 1e-3


def _ref_of(S, best, k):
    import itertools
    return list(itertools.permutations(range(S)))[best][k]


# ------------------------------------------------------------------------------------------------ 4: the defects
def test_every_defect_is_named_by_a_case():
    assert set(WC.LOSS_DEFECT_CASES) == set(WC.LOSS_DEFECTS) and set(WC.MIX_DEFECT_CASES) == set(WC.MIX_DEFECTS)
    assert all(v and set(v) <= set(WC.LOSS_CASES) for v in WC.LOSS_DEFECT_CASES.values())
    assert all(v and set(v) <= set(WC.MIX_CASES) for v in WC.MIX_DEFECT_CASES.values())
    for kind in ("sisdr", "mixit"):                   # both losses, where the defect is in the shared skeleton
        for d in ("gather_wrap", "gather_extra_chunk", "gather_short", "chunk_last_sample", "finalize_wrap", "tally_wrap", "last_maximum",
                  "pcm_unscaled", "unguarded_zero"):
            assert any(n.startswith(kind) for n in WC.LOSS_DEFECT_CASES[d]), (kind, d)


@pytest.mark.parametrize("defect", WC.LOSS_DEFECTS)
def test_loss_cases_catch_the_defect(defect):
    least = np.inf
    for name in WC.LOSS_DEFECT_CASES[defect]:
        shown = WC.loss_defect_shows(name, defect)
        least = min(least, shown)
        assert shown >= 1.0, "%s on %s moves %.3g of 10 x the gate" % (defect, name, shown)
    print("wave_cases defect %-18s: at least %.3g x (10 x the gate) over %d cases" % (defect, least, len(WC.LOSS_DEFECT_CASES[defect])))


@pytest.mark.parametrize("defect", WC.MIX_DEFECTS)
def test_mix_cases_catch_the_defect(defect):
    least = np.inf
    for name in WC.MIX_DEFECT_CASES[defect]:
        shown = WC.mix_defect_shows(name, defect)
        least = min(least, shown)
        assert shown >= 1.0, "%s on %s moves %.3g of 10 x the gate" % (defect, name, shown)
    print("wave_cases defect %-18s: at least %.3g x (10 x the gate) over %d cases" % (defect, least, len(WC.MIX_DEFECT_CASES[defect])))


def test_the_mix_model_is_the_definition_and_the_wrap_defects_spare_the_small_batches():
    for name in WC.MIX_CASES:
        c = WC.mix_case(name)
        got = [WC.mix_model(name, u) for u in range(c["B"])]
        assert max(WC.mix_ratios(name, got).values()) <= 1e-6, name
    # a defect must not show where its edge is not reached: the other side of each wrap computes the reference
    for name in WC.LOSS_CASES:
        c = WC.loss_case(name)
        if "below_wrap" in c["edges"]:
            assert max(WC.loss_ratios(name, WC.loss_model(name, "gather_wrap")).values()) <= 1e-3, name
        if "u_below_wrap" in c["edges"]:
            for d in ("finalize_wrap", "tally_wrap"):
                assert max(WC.loss_ratios(name, WC.loss_model(name, d)).values()) <= 1e-3, (name, d)
    c = WC.mix_case("mix_clip")                       # what the clip case pins: +1 clips to 32767/32768, -1 is kept
    q0, q1 = mixing.quantize(WC.mix_reference("mix_clip")[0][0]), mixing.quantize(WC.mix_reference("mix_clip")[1][0])
    assert q0[700] == 32767.0 / 32768.0 and q1[700] == -1.0 and c["quantize"]
