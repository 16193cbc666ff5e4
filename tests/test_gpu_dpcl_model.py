"""loss=dpcl through the arch on the MI355X: compute_loss against the definition and the CPU oracle network, a few training
steps, the waveform front end, the k-means masks compute_masks writes, windowed separation with a deep-clustering model -- and
the uPIT path of sepkern/separate.py, bit for bit what it was.

The oracle network is oracle/upit.py's OracleSepDNN (the network tests/_cpu_arch.py wraps): the same BLSTM -> BatchNorm -> Linear
-> sigmoid with feat_dim * embed_dim outputs, followed by the definition's loss in torch fp64.  Gates of the arch test of
tests/test_gpu_sisdr.py: the loss within 1e-5 relative, every parameter gradient within 2e-4 relative L2.
"""
import os
import sys

import numpy as np
import pytest
import torch

import _dpcl_cases as DC
from conftest import ROOT
from oracle import upit as OU
from sepkern import dpcl
from sepkern import stitch as st

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "speech-separation_amd", "archs"))

F17, D4, S2, H, LENS = 17, 4, 2, 32, [12, 10, 7, 7, 3]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def arch(dev):
    import uPIT
    return uPIT


def _samples(rng, lens, S, F):
    out = []
    for n in lens:
        d = {"mix": (np.abs(rng.standard_normal((n, F))) * rng.uniform(0, 1, (n, F)) ** 2).astype(np.float32)}
        for s in range(S):
            d["source%d" % (s + 1)] = np.abs(rng.standard_normal((n, F))).astype(np.float32) * 0.6
        out.append(d)
    return out


def _model(arch, seed=3, **conf):
    torch.manual_seed(seed)
    kw = dict(feat_dim=str(F17), embed_dim=str(D4), num_spk=str(S2), hidden_dim=str(H), num_layers="1", loss="dpcl")
    kw.update({k: str(v) for k, v in conf.items()})
    model = arch.SepDNN(0, **kw)
    model.cuda()
    model.train()
    return model


def _embeddings(model, mix, pk, hidden):
    """The model's own output rows for (mix, pk) from the given initial state, training-mode statistics, no gradient."""
    with torch.no_grad():
        model.hidden = hidden
        return model.forward_packed(mix, pk)[:pk.R].cpu().numpy()


def _torch_loss64(z, mix, srcs, F, D, kind):
    """L_j of one utterance in torch fp64 (differentiable in z (T, F D)); labels and weights are data."""
    T = z.shape[0]
    v = z.view(T, D, F).permute(0, 2, 1).reshape(T * F, D)
    u = v / v.pow(2).sum(1, keepdim=True).sqrt()
    w = torch.from_numpy(dpcl.weights(mix, kind))
    y = torch.from_numpy(dpcl.labels_of(srcs))
    Y = torch.zeros(T * F, len(srcs), dtype=torch.float64)
    Y[torch.arange(T * F), y] = 1.0
    uw = u * w[:, None]
    A, Bm, C = uw.t() @ u, uw.t() @ Y, (Y * w[:, None]).sum(0)
    return A.pow(2).sum() - 2.0 * Bm.pow(2).sum() + C.pow(2).sum()


# (the last case: the widest head, out_dim = 257 * 40 = 10280 columns, on a batch of a few rows -- BatchNorm fold, bias + sigmoid
# and the padded-row constant at a width no uPIT model has)
@pytest.mark.parametrize("kind,F17,D4,LENS", [("mr", 17, 4, LENS), ("vad", 17, 4, LENS), ("mr", 257, 40, [3, 2])],
                         ids=["mr", "vad", "widest-head"])
def test_compute_loss_is_the_definition_on_the_models_output_and_the_oracle_networks_gradient(arch, dev, kind, F17, D4, LENS):
    from sepkern.model import to_packed
    rng = np.random.default_rng(31)
    samples = _samples(rng, LENS, S2, F17)
    batch = arch.Collator("mix")(samples)
    model = _model(arch, dpcl_weight=kind, feat_dim=F17, embed_dim=D4)
    assert model.out_dim == F17 * D4 and model.loss_kind == "dpcl"
    B = len(LENS)
    h0, c0 = torch.randn(2, B, H), torch.randn(2, B, H)
    # the oracle network with the same weights: embed_dim planes of feat_dim columns are its "speakers"
    orc = OU.OracleSepDNN(feat_dim=F17, num_spk=D4, hidden_dim=H, num_layers=1)
    orc.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    orc.train()
    out, _ = orc(batch["mix"], (h0, c0))                                    # (B, T, F D), float32
    total = 0.0
    for j, n in enumerate(LENS):
        total = total + _torch_loss64(out[j, :n].double(), samples[j]["mix"], [samples[j]["source%d" % (s + 1)] for s in range(S2)], F17, D4, kind)
    lo = total / B
    lo.backward()
    # the model
    model.next_hidden = (h0.cuda(), c0.cuda())
    loss, count = arch.compute_loss(model, 0, batch)
    loss.backward()
    assert float(count) == B and model.step_frames == sum(LENS)
    lv = float(loss.detach())
    print("arch loss=dpcl %s: loss %.8f (oracle network + fp64 loss %.8f)" % (kind, lv, float(lo.detach())))
    assert abs(lv - float(lo.detach())) <= 1e-5 * abs(float(lo.detach()))
    og, worst = dict(orc.named_parameters()), 0.0
    for k, p in model.named_parameters():
        ref = og[k].grad.double()
        err = float((p.grad.cpu().double() - ref).norm() / (ref.norm() + 1e-30))
        worst = max(worst, err)
        assert err < 2e-4, (k, err)
    print("arch loss=dpcl %s: worst parameter-gradient relative L2 %.3g (gate 2e-4)" % (kind, worst))
    # the definition on the model's own output
    mix, pk = to_packed(batch["mix"], dev)
    srcs = [to_packed(batch["source%d" % (s + 1)], dev)[0].cpu().numpy() for s in range(S2)]
    z = _embeddings(model, mix, pk, (h0.cuda(), c0.cuda()))
    ref = dpcl.loss_batch(z, mix.cpu().numpy(), srcs, pk.lens_host, pk.offs_host, F17, D4, kind)[0]
    assert abs(lv - ref) <= 2e-6 * abs(ref), (lv, ref)
    # evaluation mode / no_grad (the CV pass) goes the same way
    model.eval()
    with torch.no_grad():
        cv, cvn = arch.compute_cv_loss(model, 0, batch)
    assert np.isfinite(float(cv)) and float(cvn) == B


def test_twenty_steps_descend_and_bf16_runs(arch, dev):
    from sepkern.optim import ClipAdam
    rng = np.random.default_rng(32)
    batch = arch.Collator("mix")(_samples(rng, LENS, S2, F17))
    B = len(LENS)
    h0, c0 = torch.randn(2, B, H, device=dev), torch.randn(2, B, H, device=dev)
    for dtype in ("fp32", "bf16"):
        model = _model(arch, seed=4, dtype=dtype)
        opt = ClipAdam(model, lr=1e-3, max_norm=0.25)
        curve = []
        for _ in range(21):
            model.next_hidden = (h0, c0)
            loss, _ = arch.compute_loss(model, 0, batch)
            loss.backward()
            opt.step()
            curve.append(float(loss.detach()))
        print("loss=dpcl %s, 20 steps: " % dtype + " ".join("%.5f" % v for v in curve))
        assert all(np.isfinite(curve)) and curve[-1] < curve[0]


def test_pcm_batches_take_the_same_route(arch, dev):
    """A WavCollator batch (F = 257, embed_dim = 3): the loss is the definition on the features the front end made."""
    from sepkern.data import features_from_pcm
    rng = np.random.default_rng(33)
    samples = []
    for n in (128 * 9 + 40, 128 * 6 + 3, 128 * 6):
        srcs = [(rng.standard_normal(n) * 2500.0 * (1 + s)).astype(np.int16) for s in range(2)]
        samples.append({"mix": (srcs[0].astype(np.int32) + srcs[1]).clip(-32768, 32767).astype(np.int16), "source1": srcs[0], "source2": srcs[1]})
    batch = arch.WavCollator()(samples)
    model = _model(arch, seed=5, feat_dim=257, embed_dim=3)
    B = 3
    h0, c0 = torch.randn(2, B, H, device=dev), torch.randn(2, B, H, device=dev)
    model.next_hidden = (h0, c0)
    loss, count = arch.compute_loss(model, 0, batch)
    loss.backward()
    assert float(count) == B and all(torch.isfinite(p.grad).all() for p in model.parameters())
    mix, sources, pk = features_from_pcm(batch["pcm"], dev)
    assert pk.lens_host.tolist() == [10, 7, 7] and mix.shape[1] == 257
    z = _embeddings(model, mix, pk, (h0, c0))
    ref = dpcl.loss_batch(z, mix[:pk.R].cpu().numpy(), [s[:pk.R].cpu().numpy() for s in sources[:2]], pk.lens_host, pk.offs_host, 257, 3)[0]
    print("loss=dpcl from PCM: %.8f (definition on the front end's features %.8f)" % (float(loss.detach()), ref))
    assert abs(float(loss.detach()) - ref) <= 2e-6 * abs(ref)


def test_compute_masks_writes_the_kmeans_masks(arch, dev, tmp_path):
    from sepkern.model import to_packed
    rng = np.random.default_rng(34)
    lens = [12, 10, 7]
    samples = _samples(rng, lens, S2, F17)
    for i, d in enumerate(samples):
        d["name"] = "utt%d.npz" % i
    batch = arch.Collator("mix")([{"mix": d["mix"], "name": d["name"]} for d in samples])
    from sepkern import ops
    model = _model(arch, seed=6, dpcl_kmeans_iters=3)
    with torch.no_grad():
        model.lin.weight.mul_(12.0)             # an untrained head's embeddings are all but equal: spread them
    model.eval()
    h0, c0 = torch.randn(2, 3, H, device=dev), torch.randn(2, 3, H, device=dev)
    model.next_hidden = (h0, c0)
    arch.compute_masks(model, batch, str(tmp_path))
    mix, pk = to_packed(batch["mix"], dev)
    z = _embeddings(model, mix, pk, (h0, c0))
    # the files hold sk_dpcl_kmeans of the model's embeddings, bit for bit (tests/test_gpu_dpcl.py holds the kernel to the definition)
    direct = ops.dpcl_kmeans(torch.from_numpy(z).to(dev), mix, pk, S2, 3, D=D4)[0].cpu().numpy()
    # ... and the definition's masks wherever the reference's own decision is not within rounding of a tie (the embeddings of
    # an untrained network are no builder's case: some points lie on the boundary)
    ref = dpcl.kmeans_batch(z, mix.cpu().numpy(), pk.lens_host, pk.offs_host, F17, D4, S2, 3)
    sure = ref["point_gap"] >= DC.GAP_POINT
    print("compute_masks: reference gaps init %.3g, assignments %.3g, %d of %d points under %.0e" %
          (ref["gap_init"], ref["gap_assign"], (~sure).sum(), sure.size, DC.GAP_POINT))
    assert ref["gap_init"] >= DC.GAP_INIT and sure.mean() >= 0.95 and len(np.unique(ref["labels"])) == S2
    for i, n in enumerate(lens):
        got = np.load(str(tmp_path / ("utt%d.npz" % i)))
        assert sorted(got.files) == ["s1", "s2"]
        s1, s2 = got["s1"], got["s2"]
        assert s1.shape == s2.shape == (F17, n) and s1.dtype == np.float32
        assert set(np.unique(s1)) <= {0.0, 1.0} and np.array_equal(s1 + s2, np.ones((F17, n), np.float32))
        rows = dpcl.utterance_rows(pk.lens_host, pk.offs_host, i)
        assert np.array_equal(np.concatenate([s1, s2]).T, direct[rows])
        want = ref["mask"][rows]                                               # (T_i, S F)
        ok = sure[rows].T
        assert np.array_equal(s1[ok], want[:, :F17].T[ok]) and np.array_equal(s2[ok], want[:, F17:].T[ok])


W, HN = 16, 8


def _pcm_of_frames(T, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy((rng.standard_normal(128 * (T - 1) + 17) * 3000.0).astype(np.int16))


def _window_arrays(desc, lens, S):
    return [torch.as_strided(t, (n, S * 257), (stride, 1), t.storage_offset() + off).cpu().numpy() for (t, off, stride), n in zip(desc, lens)]


def _seeded(model, seed=5):
    model.hidden_generator = torch.Generator(device="cuda")
    model.hidden_generator.manual_seed(seed)
    return model


def test_separate_recording_with_a_deep_clustering_model(arch, dev):
    from sepkern.separate import separate_recording
    model = _model(arch, seed=7, feat_dim=257, embed_dim=3, dpcl_kmeans_iters=4)
    model.eval()
    T = 2 * HN + W                                                             # three windows of 16 frames every 8
    wav, _, d = separate_recording(_seeded(model), _pcm_of_frames(T, 8), 8000, W, HN, batch_windows=2, return_details=True)
    torch.cuda.synchronize()
    lens = st.window_lengths(T, W, HN)
    assert lens == [W, W, W] and tuple(wav.shape) == (S2, 128 * (T - 1)) and bool(torch.isfinite(wav).all())
    windows = _window_arrays(d["masks"], lens, S2)
    for w in windows:                                                         # k-means masks: 0 / 1, one cluster per point
        assert set(np.unique(w)) <= {0.0, 1.0} and np.array_equal(w[:, :257] + w[:, 257:], np.ones((W, 257), np.float32))
    out, perms, cost = st.stitch_reference(d["mag"].cpu().numpy(), windows, W, HN, st.default_ramp(W - HN))
    assert np.array_equal(d["perms"].cpu().numpy(), perms)
    assert np.array_equal(d["stitched"].cpu().numpy().view(np.uint32), out.view(np.uint32))
    assert model.training is False
    # the windows ARE the k-means of the model's embeddings: window 2 (a batch of its own) from the same state
    from sepkern.packing import Packing
    _seeded(model)
    with torch.no_grad():
        model.init_hidden(2)                                                   # (the first batch's draw)
        pk = Packing(np.array([W], dtype=np.int32), dev)
        x = pk.rows(257)
        x[:W] = d["mag"][2 * HN:2 * HN + W]
        model.hidden = model.init_hidden(1)
        again = model.masks_packed(x, pk)
    assert np.array_equal(again[:W].cpu().numpy(), windows[2])


def test_upit_windows_are_forward_packed_bit_for_bit(arch, dev):
    """The unchanged path: with a uPIT model masks_packed hands on forward_packed's own tensor, and separate_recording's stitched
    masks are what the forward_packed-based window loop gave."""
    from sepkern import ops
    from sepkern.packing import Packing
    from sepkern.separate import separate_recording
    torch.manual_seed(13)
    model = arch.SepDNN(0, hidden_dim="32", num_layers="1", num_spk="2")
    model.cuda()
    model.eval()
    T = 2 * HN + W + 3                                                         # three full windows and a short one
    pcm = _pcm_of_frames(T, 9)
    _, _, d = separate_recording(_seeded(model), pcm, 8000, W, HN, batch_windows=2, return_details=True)
    mag = d["mag"]
    pk1 = Packing(np.array([5], dtype=np.int32), dev)
    with torch.no_grad():
        model.hidden = model.init_hidden(1)
        x = pk1.rows(257)
        x[:5] = mag[:5]
        a = model.masks_packed(x, pk1)
        b = model.forward_packed(x, pk1)
    assert torch.equal(a, b) and a.shape[1] == 2 * 257
    # the window loop as it was, on forward_packed
    starts = st.window_starts(T, W, HN)
    lens = [min(W, T - s0) for s0 in starts]
    assert lens == [W, W, W, W - HN + 3]
    _seeded(model)
    windows = [None] * len(starts)
    with torch.no_grad():
        for ks in ([0, 1], [2], [3]):
            B, n = len(ks), lens[ks[0]]
            pk = Packing(np.full(B, n, dtype=np.int32), dev)
            idx = (torch.arange(n, device=dev).unsqueeze(1) + torch.tensor([starts[k] for k in ks], device=dev).unsqueeze(0)).reshape(-1)
            x = pk.rows(257)
            torch.index_select(mag, 0, idx, out=x[:pk.R])
            model.hidden = model.init_hidden(B)
            mask = model.forward_packed(x, pk)
            ld = int(mask.stride(0))
            for j, k in enumerate(ks):
                windows[k] = (mask, j * ld, B * ld)
    ramp = torch.from_numpy(st.default_ramp(W - HN)).to(dev)
    stitched, perms, _ = ops.stitch(mag, windows, T, W, HN, 2, ramp)
    assert torch.equal(perms, d["perms"]) and torch.equal(stitched.view(torch.int32), d["stitched"].view(torch.int32))
