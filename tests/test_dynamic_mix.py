"""Dynamic mixing without a GPU: the numpy statement of the rule (sepkern/mixing.py) against closed forms, the draws of
archs/uPIT.py's DynMixTrainSet, the batch sampler sepkern.dist.MixDraws, DynMixCollator's layout, the driver's options and the
entry point's argument checks."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import PKG

sys.path.insert(0, os.path.join(PKG, "archs"))
sys.path.insert(0, os.path.join(PKG, "steps"))


# ------------------------------------------------------------------------------------------------ 1: the rule, closed forms
def _sines(n=8000):
    t = np.arange(n)
    # whole numbers of periods: mean squares are exactly A^2 / 2 up to rounding
    return 0.3 * np.sin(2 * np.pi * 50 * t / n), 0.05 * np.sin(2 * np.pi * 130 * t / n + 0.4)


@pytest.mark.parametrize("snr", [(0.0, 0.0), (2.5, -2.5), (-1.25, 2.0)])
def test_power_ratio_is_the_drawn_snr_and_the_largest_signal_reaches_peak(snr):
    from sepkern import mixing
    a, b = _sines()
    amp = [mixing.snr_to_amp(v) for v in snr]
    mix, (ya, yb), G = mixing.mix([a, b], amp, 0.8)
    ratio = 10.0 * np.log10(np.mean(ya ** 2) / np.mean(yb ** 2))
    want = 20.0 * np.log10(float(amp[0]) / float(amp[1]))          # the amplitudes as float32 handed them over
    assert abs(ratio - want) < 1e-9 and abs(want - (snr[0] - snr[1])) < 1e-5
    assert abs(max(np.abs(mix).max(), np.abs(ya).max(), np.abs(yb).max()) - 0.8) < 1e-15
    np.testing.assert_allclose(mix, ya + yb, rtol=0, atol=1e-16)
    np.testing.assert_allclose(ya, G[0] * a, rtol=0, atol=0)
    # unit power times the amplitude times the common scale: G_s = amp_s c / sqrt(P_s)
    assert abs(G[0] * np.sqrt(np.mean(a ** 2)) / float(amp[0]) - G[1] * np.sqrt(np.mean(b ** 2)) / float(amp[1])) < 1e-12


def test_int16_samples_are_scaled_by_32768():
    from sepkern import mixing
    a, b = _sines()
    a16, b16 = np.rint(a * 32768).astype(np.int16), np.rint(b * 32768).astype(np.int16)
    m16, s16, g16 = mixing.mix([a16, b16], [1.0, 0.5], 0.9)
    mf, sf, gf = mixing.mix([a16 / 32768.0, b16 / 32768.0], [1.0, 0.5], 0.9)
    assert np.array_equal(m16, mf) and np.array_equal(g16, gf) and all(np.array_equal(x, y) for x, y in zip(s16, sf))


def test_a_silent_source_gets_gain_zero_and_the_rest_still_reach_peak():
    from sepkern import mixing
    a, b = _sines()
    for quiet in (np.zeros_like(a), np.full_like(a, 2.0 ** -21)):       # mean square 0 and 2^-42 < 2^-40
        mix, srcs, G = mixing.mix([a, quiet, b], [1.0, 1.0, 1.0], 0.7)
        assert G[1] == 0.0 and not srcs[1].any() and G[0] > 0 and G[2] > 0
        assert np.isfinite(mix).all() and abs(max(np.abs(mix).max(), np.abs(srcs[0]).max(), np.abs(srcs[2]).max()) - 0.7) < 1e-15
    # just above the limit it is a source like any other
    _, _, G = mixing.mix([a, np.full_like(a, 2.0 ** -19)], [1.0, 1.0], 0.7)
    assert G[1] > 0


def test_all_sources_silent_gives_zeros():
    from sepkern import mixing
    z = np.zeros(300)
    mix, srcs, G = mixing.mix([z, z], [1.0, 1.0], 0.9, quantized=True)
    assert not mix.any() and not srcs[0].any() and not srcs[1].any() and not G.any() and np.isfinite(G).all()


def test_quantize_is_idempotent_and_lands_on_the_int16_grid():
    from sepkern import mixing
    a, b = _sines()
    mix, srcs, _ = mixing.mix([a, b], [1.0, 0.8], 0.9, quantized=True)
    plain, _, _ = mixing.mix([a, b], [1.0, 0.8], 0.9)
    for v in [mix] + srcs:
        k = v * 32768.0
        assert np.array_equal(k, np.rint(k)) and k.min() >= -32768 and k.max() <= 32767
        assert np.array_equal(mixing.quantize(v), v)
    assert np.abs(mix - plain).max() <= 0.5 / 32768 and np.abs(mix - plain).max() > 0
    assert np.array_equal(mixing.quantize(np.array([1.0, -1.0, 2.0, -2.0, 0.5 / 32768, 1.5 / 32768])),
                          np.array([32767, -32768, 32767, -32768, 0, 2]) / 32768.0)       # clip, and ties go to even


def test_bad_arguments():
    from sepkern import mixing
    with pytest.raises(ValueError):
        mixing.mix([np.ones(4), np.ones(5)], [1, 1], 0.9)
    with pytest.raises(ValueError):
        mixing.mix([np.ones(4)] * 5, [1] * 5, 0.9)
    with pytest.raises(ValueError):
        mixing.mix([np.ones(4), np.ones(4)], [1], 0.9)


# ------------------------------------------------------------------------------------------------ 2: the draws
N_SPK, N_UTT = 6, 3


def _corpus(root, n_spk=N_SPK, n_utt=N_UTT, rate=8000, lengths=None):
    """<root>/wav/<spk>_<k>.wav, wav.scp and utt2spk: n_spk speakers x n_utt short files of different lengths; sample j of
    speaker p's k-th file is its own id (so a slice says where it came from)."""
    import scipy.io.wavfile
    os.makedirs(os.path.join(root, "wav"), exist_ok=True)
    scp, u2s = [], []
    for p in range(n_spk):
        for k in range(n_utt):
            n = lengths[p * n_utt + k] if lengths else 400 + 37 * p + 101 * k
            x = ((np.arange(n) * 7 + 1000 * p + 100 * k) % 30000 - 15000).astype(np.int16)
            utt, path = "spk%d_%d" % (p, k), os.path.join(root, "wav", "spk%d_%d.wav" % (p, k))
            scipy.io.wavfile.write(path, rate, x)
            scp.append("%s %s\n" % (utt, path))
            u2s.append("%s spk%d\n" % (utt, p))
    open(os.path.join(root, "wav.scp"), "w").write("".join(scp))
    open(os.path.join(root, "utt2spk"), "w").write("".join(u2s))
    return root


def _same_item(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)


def test_an_item_is_a_function_of_seed_and_index(tmp_path):
    import uPIT
    data = _corpus(str(tmp_path))
    ds = uPIT.DynMixTrainSet(data, 2, seed=5)
    assert ds.mixes_per_epoch == len(ds) == N_SPK * N_UTT // 2 and len(ds.frame_counts()) == len(ds)
    again = uPIT.DynMixTrainSet(data, 2, seed=5)
    other = uPIT.DynMixTrainSet(data, 2, seed=6)
    N = len(ds)
    items = [ds[i] for i in range(3 * N)]
    assert all(_same_item(x, again[i]) for i, x in enumerate(items))
    assert not all(_same_item(x, other[i]) for i, x in enumerate(items))
    # epoch e + 1 (indices N ..) is not epoch e
    assert not all(_same_item(items[i], items[N + i]) for i in range(N))
    for i, it in enumerate(items):
        picks, n, snr, peak = ds.draw(i)
        assert sorted(it) == ["amp", "peak", "source1", "source2"] and peak == it["peak"] == 0.9
        # distinct speakers, one length after cropping, the slice that was drawn, levels inside the range
        spk = [os.path.basename(p).split("_")[0] for p, _, _ in picks]
        assert len(set(spk)) == 2
        assert it["source1"].dtype == np.int16 and len(it["source1"]) == len(it["source2"]) == n == min(m for _, _, m in picks) >= 257
        for s, (path, st, m) in enumerate(picks):
            import scipy.io.wavfile
            assert 0 <= st <= m - n and np.array_equal(it["source%d" % (s + 1)], scipy.io.wavfile.read(path)[1][st:st + n])
        assert all(abs(v) <= 2.5 for v in snr) and np.allclose(it["amp"], [10 ** (v / 20) for v in snr], rtol=1e-6)
    assert max(f for f in ds.frame_counts()) >= max(1 + len(it["source1"]) // 128 for it in items)
    # crops really start anywhere, levels and partners vary
    assert len({ds.draw(i)[0][0][1] for i in range(3 * N)}) > 3 and len({tuple(p for p, _, _ in ds.draw(i)[0]) for i in range(3 * N)}) > 3


def test_loader_workers_see_the_same_items(tmp_path):
    import uPIT
    from sepkern.dist import MixDraws
    from torch.utils.data import DataLoader
    ds = uPIT.DynMixTrainSet(_corpus(str(tmp_path)), 3, seed=1, peak=(0.5, 0.9), snr_db=4.0, max_samples=300)
    got = []
    for workers in (0, 2):
        draws = MixDraws(ds.mixes_per_epoch, 2, 0, 1)
        draws.set_epoch(2)
        got.append(list(DataLoader(ds, batch_sampler=draws, collate_fn=ds.collator, num_workers=workers)))
    assert len(got[0]) == len(got[1]) == 3
    for a, b in zip(*got):
        assert torch.equal(a["pcm"]["flat"], b["pcm"]["flat"]) and a["pcm"]["lens"] == b["pcm"]["lens"] == [300, 300]
        assert a["pcm"]["mixing"] == b["pcm"]["mixing"] and a["pcm"]["keys"] == ["source1", "source2", "source3"]
        assert all(0.5 <= p <= 0.9 for p in a["pcm"]["mixing"]["peak"])
    assert len({p for a in got[0] for p in a["pcm"]["mixing"]["peak"]}) == 6


def test_a_corpus_that_cannot_be_mixed_is_refused(tmp_path):
    import uPIT
    two = _corpus(os.path.join(str(tmp_path), "two"), n_spk=2)
    uPIT.DynMixTrainSet(two, 2)
    with pytest.raises(ValueError, match="2 speaker.*needs 3"):
        uPIT.DynMixTrainSet(two, 3)
    short = _corpus(os.path.join(str(tmp_path), "short"), n_spk=3, n_utt=2, lengths=[400, 256, 500, 300, 100, 257])
    with pytest.raises(ValueError, match="2 utterance.*fewer than 257 samples"):
        uPIT.DynMixTrainSet(short, 2)
    with pytest.raises(ValueError, match="max_samples"):
        uPIT.DynMixTrainSet(two, 2, max_samples=100)


def test_a_sample_rate_is_recorded_and_lengths_count_at_it(tmp_path):
    import uPIT
    from sepkern.resample import out_len
    data = _corpus(str(tmp_path), n_spk=3, n_utt=2, rate=16000, lengths=[700, 900, 1100, 600, 800, 1000])
    ds = uPIT.DynMixTrainSet(data, 2, sample_rate=8000, max_samples=400)
    for i in range(6):
        it = ds[i]
        assert it["rate"] == 16000 and 257 <= out_len(len(it["source1"]), 16000, 8000) <= 400
    batch = ds.collator([ds[i] for i in range(3)])["pcm"]
    assert batch["rate"] == [16000] * 3 and batch["target_rate"] == 8000
    with pytest.raises(ValueError, match="cannot be framed"):       # 500 samples at 16 kHz are 250 at 8 kHz
        uPIT.DynMixTrainSet(_corpus(os.path.join(str(tmp_path), "b"), n_spk=2, n_utt=1, rate=16000, lengths=[500, 900]), 2, sample_rate=8000)


# ------------------------------------------------------------------------------------------------ 3: who draws what
@pytest.mark.parametrize("n,bs", [(23, 4), (32, 4), (5, 8), (9, 2), (64, 3)])
def test_mix_draws_partition_the_epoch(n, bs):
    from sepkern.dist import MixDraws
    for world in (1, 2, 4):
        for epoch in (0, 3):
            per_rank = []
            for r in range(world):
                d = MixDraws(n, bs, r, world, seed=9)
                d.set_epoch(epoch)
                per_rank.append(list(d))
                assert len(per_rank[-1]) == len(d) and all(0 < len(b) <= bs for b in per_rank[-1])
            assert len({len(b) for b in per_rank}) == 1                        # equal batch counts
            drawn = sorted(i for batches in per_rank for b in batches for i in b)
            assert drawn == list(range(epoch * n, (epoch + 1) * n))           # every index once, no two ranks the same
            # consecutive ranges, round-robin: rank r's k-th batch lies before rank r + 1's k-th
            for batches in per_rank:
                assert all(b == list(range(b[0], b[0] + len(b))) for b in batches)
            for k in range(len(per_rank[0])):
                firsts = [per_rank[r][k][0] for r in range(world)]
                assert firsts == sorted(firsts)


def test_set_epoch_on_a_fresh_sampler_is_the_running_samplers_epoch():
    from sepkern.dist import MixDraws
    running = MixDraws(10, 3, 1, 2, seed=4)
    history = []
    for e in range(4):
        running.set_epoch(e)
        history.append(list(running))
    fresh = MixDraws(10, 3, 1, 2, seed=4)
    fresh.set_epoch(3)
    assert list(fresh) == history[3] and history[3] != history[2]
    with pytest.raises(ValueError):
        MixDraws(0, 3, 0, 1)
    # fewer indices than ranks: nobody goes without a batch
    tiny = [list(MixDraws(2, 4, r, 4)) for r in range(4)]
    assert all(len(b) == 1 and len(b[0]) == 1 for b in tiny) and {b[0][0] for b in tiny} == {0, 1}


# ------------------------------------------------------------------------------------------------ 4: the collator
def test_collator_layout_order_and_length_check():
    import uPIT
    rng = np.random.default_rng(0)
    lens = [400, 1000, 257, 640]                                              # 4, 8, 3 and 6 frames
    items = [{"source1": rng.integers(-9, 9, n).astype(np.int16), "source2": rng.integers(-9, 9, n).astype(np.int16),
              "amp": [1.0 + j, 0.5], "peak": 0.1 * (j + 1)} for j, n in enumerate(lens)]
    pcm = uPIT.DynMixCollator(quantize=True)(items)["pcm"]
    order = [1, 3, 0, 2]                                                    # longest first
    assert pcm["keys"] == ["source1", "source2"] and pcm["lens"] == [lens[i] for i in order] and "mix" not in pcm["keys"]
    assert pcm["flat"].dtype == torch.int16
    assert np.array_equal(pcm["flat"].numpy(), np.concatenate([items[i][k] for k in ("source1", "source2") for i in order]))
    assert pcm["mixing"] == {"amp": [[1.0 + i for i in order], [0.5] * 4], "peak": [0.1 * (i + 1) for i in order], "quantize": True}
    assert "rate" not in pcm and uPIT.DynMixCollator()(items)["pcm"]["mixing"]["quantize"] is False
    bad = [dict(items[0], source2=items[0]["source2"][:-1])] + items[1:]
    with pytest.raises(ValueError, match="must have one length"):
        uPIT.DynMixCollator()(bad)
    with pytest.raises(ValueError, match="one 'amp' per source"):
        uPIT.DynMixCollator()([dict(items[0], amp=[1.0])])
    with pytest.raises(ValueError, match="'rate'"):
        uPIT.DynMixCollator(sample_rate=8000)(items)


# ------------------------------------------------------------------------------------------------ 5: the driver's options
def test_dynamic_mix_needs_wav_input(tmp_path):
    import train_qsub
    with pytest.raises(SystemExit, match="--dynamic-mix.*needs.*--wav-input"):
        train_qsub.get_args(["uPIT", "0", "data", "out", "--dynamic-mix"])
    args = train_qsub.get_args(["uPIT", "0", "data", "out", "--wav-input", "--dynamic-mix", "--mix-peak", "0.5,0.8",
                                "--mix-snr-db", "3", "--mixes-per-epoch", "7", "--mix-max-samples", "4000", "--mix-quantize"])
    assert args.mix_peak == (0.5, 0.8) and args.mix_snr_db == 3.0 and args.mixes_per_epoch == 7 and args.mix_quantize
    assert train_qsub.get_args(["uPIT", "0", "data", "out", "--wav-input", "--dynamic-mix", "--mix-peak", "0.7"]).mix_peak == (0.7, 0.7)
    plain = train_qsub.get_args(["uPIT", "0", "data", "out"])
    assert not plain.dynamic_mix and plain.mix_peak == (0.9, 0.9) and plain.mix_snr_db == 2.5
    # arguments built by hand reach the same check in training_batches, before any file is opened
    args.wav_input = False
    with pytest.raises(SystemExit, match="--dynamic-mix.*needs.*--wav-input"):
        train_qsub.training_batches(None, args, 0, 1)


def test_training_batches_builds_the_dynamic_set(tmp_path):
    import train_qsub
    import uPIT
    from sepkern.dist import MixDraws
    data = _corpus(str(tmp_path))
    conf = os.path.join(str(tmp_path), "conf")
    open(conf, "w").write("num_spk=3\nhidden_dim=64\n")
    args = train_qsub.get_args(["uPIT", "0", data, "out", "--wav-input", "--dynamic-mix", "--model-config", conf, "--batch-size", "4",
                                "--seed", "3", "--prefetch", "0", "--num-workers", "0", "--mixes-per-epoch", "10"])
    loader, draws = train_qsub.training_batches(uPIT, args, 1, 2)
    assert isinstance(draws, MixDraws) and (draws.n, draws.bs, draws.rank, draws.world) == (10, 4, 1, 2)
    ds = loader.dataset
    assert isinstance(ds, uPIT.DynMixTrainSet) and ds.num_spk == 3 and ds.seed == 3 and ds.mixes_per_epoch == 10
    draws.set_epoch(1)
    batches = list(loader)
    assert len(batches) == 2 and batches[0]["pcm"]["keys"] == ["source1", "source2", "source3"] and len(batches[0]["pcm"]["lens"]) == 4


# ------------------------------------------------------------------------------------------------ 6: the entry point's checks
def test_entry_point_refuses_bad_shapes_before_it_touches_a_device():
    from sepkern import _lib
    lib = _lib.load()
    for S, B, word in ((5, 3, b"S = 5"), (0, 3, b"S = 0"), (2, 0, b"B = 0"), (2, 65536, b"B = 65536")):
        rc = lib.sk_dynamic_mix(None, 1, None, None, B, S, None, None, 0, None, None, None, None)
        assert rc == -1 and word in lib.sk_last_error(), (S, B, lib.sk_last_error())
    assert lib.sk_dynamic_mix(None, 1, None, None, 3, 2, None, None, 0, None, None, None, None) == -1
    assert b"null pointer" in lib.sk_last_error()
