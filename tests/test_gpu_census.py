"""Kernel census: which `__global__` serves which launch of which BASELINE configuration.

One training step of every one-GPU BASELINE configuration (+ the reference's default model at its default batch size, + the
headline in the reference's literal fp32-MFMA arithmetic) runs with a spy on the ctypes boundary: every C entry point called, and
for the GEMMs and the recurrences the kernel the library chose (sk_gemm_last_kernel(), sk_lstm_last_launch()).  The table
generated from that is the one DESIGN.md section 4 carries between its census markers: this test regenerates it and compares,
so the document cannot go stale.
`python tests/test_gpu_census.py` prints the table (and writes gpurun_out/census.md).
It also writes census_order.txt beside census.md: per configuration the launches in the order they were enqueued -- what a
host-side change of the engine must leave as it is, stream by stream.
"""
import os
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "speech-separation_amd", "archs"))

GEMM_KERNELS = {
    1: "gemm_f32_kernel (fp32 MFMA, register-staged)", 2: "gemm_f32_kernel_split3 (split products, 128x128)",
    3: "gemm_f32_kernel_dma (fp32 MFMA, LDS-DMA 128x128)", 4: "gemm_f32_kernel_dma256 (fp32 MFMA, 256x128)",
    6: "gemm_f32_kernel_streamk (fp32 MFMA, 256x256 persistent)", 9: "bf::gemm_bf16_kernel (fp32 operands rounded on the way in)",
    10: "gemm_f32_kernel_planes (split products, split once while staging, 256x128)",
    11: "bf2::gemm_bf16_nt_kernel<128>", 12: "bf2::gemm_bf16_nt_kernel<256>", 13: "bf2::gemm_bf16_streamk_kernel",
    14: "gemm_f32_kernel_pl3 (split products on operands that arrive split, 128x128)",
}
# entry point -> the kernel(s) it launches when the choice does not depend on the arguments
FIXED = {
    "sk_stft": "stft_kernel", "sk_mask_istft": "istft_kernel", "sk_pit_mse_fwd": "pit_pair_kernel + pit_finalize_kernel",
    "sk_pit_mse_bwd": "pit_bwd_kernel", "sk_bn_stats": "colred_kernel + colfin_kernel + colfin_var_kernel", "sk_bn_fold": "bn_fold_kernel",
    "sk_bn_unfold_grad": "bn_unfold_grad_kernel", "sk_bn_update_running": "bn_running_kernel", "sk_bn_apply": "bn_apply_kernel",
    "sk_bn_bwd_sums": "colred_kernel + colfin_kernel", "sk_bn_bwd_apply": "bn_bwd_apply_kernel", "sk_colsum": "colred_kernel + colfin_kernel",
    "sk_sigmoid_bwd": "sigmoid_bwd_kernel", "sk_pad_rows": "pad_rows_kernel", "sk_gate_rows": "gate_rows_kernel",
    "sk_hprev_rows": "hprev_rows_kernel", "sk_pack_rows": "pack_rows_kernel", "sk_unpack_rows": "pack_rows_kernel (unpack form)",
    "sk_cast_bf16_rows": "bf2::cast_kernel", "sk_split_rows": "split_rows_kernel", "sk_grad_norm": "sumsq_kernel + norm_fin_kernel", "sk_clip_adam": "clip_adam_kernel",
    "sk_rsh_loss_fwd": "rsh_sse_kernel + rsh_select_kernel", "sk_rsh_loss_bwd": "rsh_bwd_kernel", "sk_att_update": "att_update_kernel",
    "sk_att_update_bwd": "att_update_bwd_kernel",
}


def _lstm_row(name, T, B, H):
    """Kernel instantiation and grid of the recurrence call that just returned, from sk_lstm_last_launch()."""
    from sepkern import ops
    _, q = ops.lstm_last_launch()
    tf = lambda i: "true" if q[i] else "false"      # noqa: E731
    if q[ops.LSTM_Q_FAMILY] in (ops.LSTM_K_FWD_XL8, ops.LSTM_K_BWD_XL8):           # XCD-local streams of 8 rows
        n8 = 2 * ((B + 7) // 8)
        k = "lstm_fwd_xl8_kernel<56, %s>" % tf(ops.LSTM_Q_PACKED) if name == "sk_lstm_fwd" else "lstm_bwd_xl8_kernel<56>"
        return k, "T=%d B=%d H=%d: %d streams of 28 workgroups x 32 units x 8 rows, one XCD each (%d CUs held)" % (T, B, H, n8, 28 * n8)
    if name == "sk_lstm_fwd":
        k = "lstm_fwd_kernel<%d, %s, 8, %s, %s>" % (q[ops.LSTM_Q_KS], tf(ops.LSTM_Q_BF16),
                                                    "true" if q[ops.LSTM_Q_FAMILY] == ops.LSTM_K_FWD_SPLIT3 else "false", tf(ops.LSTM_Q_PACKED))
    else:
        k = "lstm_bwd_kernel<%d, %s, %d>%s" % (q[ops.LSTM_Q_KS], tf(ops.LSTM_Q_BF16), q[ops.LSTM_Q_GM],
                                               " (exclusive)" if q[ops.LSTM_Q_EXCLUSIVE] else "")
    return k, "T=%d B=%d H=%d: %d persistent workgroups (one per CU), %d batch group(s) each" % (T, B, H, q[ops.LSTM_Q_BLOCKS], q[ops.LSTM_Q_G])


class Spy:
    def __init__(self):
        from sepkern import _lib
        self._lib, self.rows, self.seq, self.orig = _lib, {}, [], _lib.call

    def __enter__(self):
        lib = self._lib

        def call(name, *args):
            self.orig(name, *args)
            side = torch.cuda.current_stream() != torch.cuda.default_stream()
            val = lambda a: getattr(a, "value", a)      # noqa: E731
            if name in ("sk_gemm_f32_splitk", "sk_gemm_bf16_splitk", "sk_gemm_bf16_mm", "sk_gemm_bf16_nt", "sk_gemm_pl3_tn"):
                kid = lib.load().sk_gemm_last_kernel()
                M, N, K = (args[3], args[4], args[5]) if name == "sk_gemm_pl3_tn" else (args[4], args[5], args[6])
                if name == "sk_gemm_pl3_tn":
                    form, batch, splitk = "T/N", args[12], args[16]
                elif name == "sk_gemm_bf16_nt":
                    form, batch, splitk = "N/T", args[12], args[17]
                else:
                    form = ("T" if args[10] else "N") + "/" + (("N" if args[11] else "T") if name == "sk_gemm_bf16_mm" else ("T" if args[11] else "N"))
                    batch, splitk = args[14], args[19]
                shape = "%s %d x %d x %d%s%s" % (form, M, N, K, " x%d" % batch if batch > 1 else "", " in %d K slices" % splitk if splitk > 1 else "")
                key = (name, GEMM_KERNELS.get(kid, "kernel %d" % kid), shape, "side" if side else "main")
            elif name in ("sk_lstm_fwd", "sk_lstm_bwd"):
                k, shape = _lstm_row(name, *[val(a) for a in (args[12:15] if name == "sk_lstm_fwd" else args[17:20])])
                key = (name, k, shape, "side" if side else "main")
            elif name in FIXED:
                key = (name, FIXED[name], "", "side" if side else "main")
            else:
                return
            self.rows[key] = self.rows.get(key, 0) + 1
            self.seq.append(key)
        lib.call = call
        return self

    def __exit__(self, *exc):
        self._lib.call = self.orig
        return False


def _step(arch, H, L, S, B, T, dtype, env=None, ragged=False):
    """One training step of the given configuration on a uniform batch; returns the spy (rows: counts, seq: enqueue order)."""
    import uPIT
    from sepkern.optim import ClipAdam
    from sepkern.packing import Packing
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        torch.manual_seed(0)
        F = 257
        if arch == "rsh":
            import RSH
            model = RSH.SepDNN(0, hidden_dim=str(H), num_layers=str(L), dtype=dtype)
        else:
            model = uPIT.SepDNN(0, num_spk=str(S), hidden_dim=str(H), num_layers=str(L), dtype=dtype)
        model.cuda()
        model.train()
        opt = ClipAdam(model, lr=1e-3, max_norm=0.25)
        g = torch.Generator(device="cuda").manual_seed(1)
        pk = Packing.from_lens([T - (i * (T // 2)) // max(1, B - 1) for i in range(B)] if ragged else [T] * B, "cuda")
        mix = torch.rand(pk.Rp, F, device="cuda", generator=g)
        srcs = [torch.rand(pk.Rp, F, device="cuda", generator=g) * 0.6 for _ in range(S)]

        def step():
            if arch == "rsh":
                lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
                mp = mix.view(T, B, F)
                combos = torch.cat([mp, torch.ones_like(mp)], 2).contiguous()
                loss, _ = RSH.compute_loss_padded(model, [(S, combos, [s_.view(T, B, F) for s_ in srcs], lens)])
            else:
                loss, _ = uPIT.compute_loss_packed(model, mix, srcs, pk)
            loss.backward()
            opt.step()
        step()                                             # warm-up: lazily built engine, workspaces
        torch.cuda.synchronize()
        with Spy() as spy:
            step()
            torch.cuda.synchronize()
        model.check_status()
        return spy
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


CONFIGS = (
    ("BASELINE configs[1] (the headline): uPIT 3x896, 2-spk, 32 x 400, fp32", dict(arch="upit", H=896, L=3, S=2, B=32, T=400, dtype="fp32")),
    ("the same model on a RAGGED batch (the WSJ0-2mix-shaped set: 32 utterances of 200 .. 400 frames)",
     dict(arch="upit", H=896, L=3, S=2, B=32, T=400, dtype="fp32", ragged=True)),
    ("the same step in the reference's literal arithmetic (bench.py secondary.fp32_mfma: GEMM variants 8 / 1, plain forward product)",
     dict(arch="upit", H=896, L=3, S=2, B=32, T=400, dtype="fp32", env={"SEPKERN_GEMM_VARIANTS": "8,1", "SEPKERN_LSTM_FWD": "0,1,1,0,0,0,0,0"})),
    ("BASELINE configs[3]: uPIT 3x896, 3-spk, 32 x 400, bf16", dict(arch="upit", H=896, L=3, S=3, B=32, T=400, dtype="bf16")),
    ("BASELINE configs[0]'s model at the reference's batch size: uPIT 2x600, 2-spk, 100 x 400, fp32", dict(arch="upit", H=600, L=2, S=2, B=100, T=400, dtype="fp32")),
    ("BASELINE configs[4] (one GPU): RSH 2x600, 4-spk, 32 x 400, fp32", dict(arch="rsh", H=600, L=2, S=4, B=32, T=400, dtype="fp32")),
    ("BASELINE configs[0] (the plumbing case): uPIT 2x300, 2-spk, 8 x 100, fp32 -- a hidden size that is no multiple of 8: fp32 operands, the 128 x 128 split kernel",
     dict(arch="upit", H=300, L=2, S=2, B=8, T=100, dtype="fp32")),
)


def census_markdown(sequence=None):
    """The census tables; sequence (a list): receives, per configuration, one line per launch in enqueue order."""
    out = []
    for title, cfg in CONFIGS:
        spy = _step(**cfg)
        rows = spy.rows
        if sequence is not None:
            sequence += ["== " + title] + [" | ".join(k) for k in spy.seq]
        out.append("**%s** -- one training step:" % title)
        out.append("")
        out.append("| launches | entry point | kernel | shape / grid | stream |")
        out.append("|---|---|---|---|---|")
        order = sorted(rows.items(), key=lambda kv: (0 if "gemm" in kv[0][0] else 1 if "lstm" in kv[0][0] else 2, kv[0][0], kv[0][2], kv[0][3]))
        for (name, kern, shape, stream), n in order:
            out.append("| %d | `%s` | %s | %s | %s |" % (n, name, kern, shape, stream))
        out.append("")
    return "\n".join(out).rstrip() + "\n"


BEGIN, END = "<!-- census:begin (generated by tests/test_gpu_census.py; do not edit) -->", "<!-- census:end -->"


def test_design_md_carries_the_generated_census():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    md = census_markdown()
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "census.md"), "w") as f:
        f.write(md)
    doc = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert BEGIN in doc and END in doc, "DESIGN.md has no census block"
    have = doc[doc.index(BEGIN) + len(BEGIN):doc.index(END)].strip()
    assert have == md.strip(), "DESIGN.md's kernel census is stale: regenerate it (gpurun_out/census.md holds the current one)"
    # every fp32 GEMM kernel the library still carries serves a launch of some configuration above
    used = {r.split("|")[3].strip() for r in md.splitlines() if r.startswith("| ")}
    # (id 4, gemm_f32_kernel_dma256, is the one exception: it is what variants 8 / 6 fall back to for a large product when the caller
    # passes no stream-K workspace or the stream-K cut does not apply -- the engine always passes one, so no step launches it; its
    # parity is pinned in test_gpu_kernels.py under variant 4)
    for kid in (1, 2, 3, 6, 10, 11, 12, 13, 14):
        assert GEMM_KERNELS[kid] in used, "no configuration launches " + GEMM_KERNELS[kid]
    assert GEMM_KERNELS[4] not in used, "gemm_f32_kernel_dma256 is launched by a step now: list it above and drop this note"


if __name__ == "__main__":
    seq = []
    text = census_markdown(seq)
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "census.md"), "w") as fh:
        fh.write(text)
        with open(os.path.join(os.path.dirname(fh.name), "census_order.txt"), "w") as fo:      # beside census.md
            fo.write("\n".join(seq) + "\n")
    print(text)
