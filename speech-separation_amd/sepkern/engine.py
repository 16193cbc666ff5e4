"""The uPIT network (BLSTM -> BatchNorm1d -> Linear -> sigmoid) as a sequence of libsepkern calls.

Mirrors SepDNN.forward of the reference (archs/uPIT.py:129-147) and the backward torch's autograd
would run for it, on PACKED rows -- the layout of the PackedSequence the reference's collator builds
(archs/uPIT.py:46) and nn.LSTM consumes (:132): only the R = sum(lens) valid frames of a length-sorted
batch exist (sepkern.packing.Packing), so no product, statistic or store touches a padded frame.
All parameters live in ONE flat fp32 buffer (and all gradients in another):
  * the LSTM kernels want (2, 4H, *) blocks (both directions of a layer) contiguous,
  * data-parallel training all-reduces one buffer (RCCL, one collective per step),
  * clip_grad_norm_ + Adam run as one fused pass over it (sepkern.optim).
nn.Parameters with the reference's names are views into it, so state_dict() is unchanged.
"""
import math
import os
from collections import namedtuple

import torch

from . import dist as skdist
from . import ops
from ._lib import SepkernError


def _switches(bf16, hidden, env=os.environ):
    """Every environment switch of the engine -> {Engine attribute: value} (what was measured for each default:
    DESIGN.md 5 / 6 and DESIGN_HISTORY.md, "The engine's defaults").  On/off switches: "0" = off, any other value = on, unset =
    the default given here.  A malformed value is a SepkernError that names the variable and what it accepts.  The attributes stay
    plain: drivers and tests assign lstm_mode, overlap, var_main, var_side on a built engine, and every pass reads them anew."""

    def bad(name, accepted):
        return SepkernError("%s=%r: expected %s" % (name, env[name], accepted))

    def on(name, default):
        return env[name] != "0" if name in env else default

    def lstm_bits(name, **default):
        if name not in env:
            return ops.lstm_variant_bits(**default)
        try:
            return ops.lstm_variant_from_spec(env[name])
        except ValueError:
            raise bad(name, 'comma-separated integers "half,map,poll1,repflags,spread,delay,tagged,split3,xl8"') from None

    def ints(name, default, n, accepted):
        try:
            v = [int(x) for x in env.get(name, default).split(",")]
        except ValueError:
            v = []
        if len(v) != n:
            raise bad(name, accepted)
        return v

    lstm_mode, = ints("SEPKERN_LSTM_MODE", "0", 1, "an integer: 0 (auto), 1 (persistent) or 2 (one launch per time step)")
    var_main, var_side = ints("SEPKERN_GEMM_VARIANTS", "0,2", 2, 'two integers "main,side" (sk_gemm_f32_splitk variants)')
    bwd_exclusive = env.get("SEPKERN_BWD_EXCLUSIVE", "auto")
    if bwd_exclusive not in ("auto", "0", "1"):
        raise bad("SEPKERN_BWD_EXCLUSIVE", "auto, 0 or 1")
    fwd = (dict(blockmap=1, poll1=True, spread=True, xl8=True) if bf16 else    # a flag per 128-byte line; XCD-local streams of 8 rows where they fit
           dict(blockmap=1, poll1=True, split3=True) if hidden <= 896 else     # h W_hh^T by the exact three-way bf16 split, flags hand-off
           dict(blockmap=1, poll1=True, poll_delay=8, tagged=True))            # the split's register slice does not fit: "the data is the flag"
    fwd_bits = lstm_bits("SEPKERN_LSTM_FWD", **fwd)
    split3_fwd = bool(fwd_bits & ops.LSTM_SPLIT3) and not bf16 and hidden <= 896
    return dict(
        # launch kind of the recurrences (ops.LSTM_AUTO / _PERSISTENT / _PER_STEP); drivers fall back to 2 after a timed-out launch
        lstm_mode=lstm_mode,
        # hand-off geometry / protocol / arithmetic of the persistent recurrences (mode bits; speed only but for split3 / tagged)
        fwd_bits=fwd_bits,
        bwd_bits=lstm_bits("SEPKERN_LSTM_BWD", blockmap=1, poll_delay=ops.LSTM_DELAY_NONE, xl8=bf16),
        # which fp32 forward arithmetic those bits select at this size (bench.py's config.numerics reports it)
        split3_fwd=split3_fwd,
        tagged_fwd=bool(fwd_bits & ops.LSTM_TAGGED) and not bf16 and not split3_fwd,
        # products that nobody waits for run on a side stream, co-resident with a recurrence; off: one stream, same bits
        overlap=on("SEPKERN_OVERLAP", True),
        # BatchNorm folded into the Linear layer (fp32; the bf16 arithmetic is DEFINED with bn(y) and W rounded separately)
        bn_fold=on("SEPKERN_BN_FOLD", True) and not bf16,
        # fp32 GEMM variant on the main stream (0: the library chooses) / beside a recurrence (2: the 128 x 128 split kernel, which fits there)
        var_main=var_main, var_side=var_side,
        # fp32 weight gradients on operands that arrive split (planes; a second direction's columns start 16-byte aligned only if 8 | H)
        wgrad_planes=on("SEPKERN_WGRAD_PLANES", True) and not bf16 and hidden % 8 == 0,
        # backward recurrences keep their CUs to themselves while those products run: auto = on ragged batches; 0 / 1 = never / always
        bwd_exclusive=bwd_exclusive,
        # data-parallel runs: BatchNorm over the GLOBAL batch instead of per rank (sepkern/dist.py)
        sync_bn=on("SEPKERN_SYNC_BN", False),
    )


def _align(n, a=4):
    return (n + a - 1) // a * a


class ParamLayout:
    """Offsets (in floats) of every parameter block inside the flat buffer.

    Per layer: weight_ih (2,4H,I) | weight_hh (2,4H,H) | bias_ih (2,4H) | bias_hh (2,4H); then
    lin.weight (out_dim, 2H), lin.bias, bn.weight, bn.bias.  Every block starts 16-byte aligned.
    uPIT: in_dim = F, out_dim = S*F; RSH: in_dim = 2F (mixture | attention), out_dim = F.
    """

    def __init__(self, in_dim, out_dim, hidden, layers):
        self.I, self.O, self.H, self.L = in_dim, out_dim, hidden, layers
        self.blocks = {}
        off = 0
        H = hidden
        for l in range(layers):
            I = in_dim if l == 0 else 2 * H
            for name, shape in (("weight_ih", (2, 4 * H, I)), ("weight_hh", (2, 4 * H, H)),
                                ("bias_ih", (2, 4 * H)), ("bias_hh", (2, 4 * H))):
                self.blocks["%s_l%d" % (name, l)] = (off, shape)
                off = _align(off + math.prod(shape))
        for name, shape in (("lin.weight", (out_dim, 2 * H)), ("lin.bias", (out_dim,)),
                            ("bn.weight", (2 * H,)), ("bn.bias", (2 * H,))):
            self.blocks[name] = (off, shape)
            off = _align(off + math.prod(shape))
        self.total = off

    GUARD = 4      # floats in front of the gradients in Engine.grad_full (word 0: the recurrence's status, see Engine)

    def grad_chunks(self):
        """[(name, lo, hi)] over Engine.grad_full = [guard words | gradients], in the order in which the backward pass
        completes them: Linear + BatchNorm, then the LSTM layers from the top down; the bottom layer's chunk comes last
        and carries the guard words in front of it (they are written at the very end of the pass).  Contiguous, disjoint,
        covering the buffer: the data-parallel exchange may go chunk by chunk (sepkern.dist.GradReducer)."""
        G = self.GUARD
        start = [self.blocks["weight_ih_l%d" % l][0] for l in range(self.L)] + [self.blocks["lin.weight"][0]]
        out = [("lin+bn", G + start[self.L], G + self.total)]
        for l in range(self.L - 1, 0, -1):
            out.append(("layer%d" % l, G + start[l], G + start[l + 1]))
        out.append(("guard+layer0", 0, G + start[1]))
        return out

    def view(self, flat, name):
        off, shape = self.blocks[name]
        return flat[off:off + math.prod(shape)].view(shape)


# What a layer's forward keeps for its backward:
#   inp (Rp, I padded) the layer's input rows, zero tail | gates (Rp, 8H) projections -> saved gates -> dgx, in place |
#   cs (Rp, 2H) cell states | y (Rp, 2H) output rows | wih_gi: W_ih, rows gate-interleaved, columns padded like inp |
#   hprev: the recurrent inputs of the rows (_hprev: fp32 rows, bf16 rows or Planes) | hprev_ready: event behind the side block
#   that made hprev and the planes (None: made inline) | inp_planes: inp as Planes (operands that arrive split), else None
LayerSaved = namedtuple("LayerSaved", "inp gates cs y wih_gi hprev hprev_ready inp_planes")
# A saved forward, what backward() takes (opaque to callers; several may be alive at once): layers = [LayerSaved]; xbn = bn(y_top)
# where BatchNorm is not folded, fold = (s, t) where it is; ytop_planes: the top layer's output as Planes, else None; version =
# param_version() at the forward; cache: the forward's bf16 operand copies (_copy), else None
FwdCtx = namedtuple("FwdCtx", "layers mean var bn_count xbn fold ytop_planes mask pk h0 c0 training version cache")
# What the steps of one pass share; side None: co-scheduling off (Engine._side); cache: bf16 operand copies (_copy); forward:
# save for backward / cut the weight gradients' operands into planes; backward: accumulate into the gradient buffer
_Pass = namedtuple("_Pass", "pk main side cache save planes acc", defaults=(False, False, False))


class _Beside:
    """`with _Beside(main, side, reads=...) as blk:` runs the block on the side stream after everything `main` has enqueued so
    far, so that it executes beside what main enqueues next.  side None (co-scheduling off): the block runs inline on main.
    reads: tensors / Planes of main's that the block reads and that are not sure to outlive the pass -- its temporaries, and in a
    forward (which never joins the streams) everything; what a ctx holds lives until backward()'s join, what the block allocates
    itself is the side stream's own.  blk.back(...) names results that main reads later.  Both are kept alive by record_stream():
    the caching allocator hands such memory out again only when the other stream has passed the point of release.  That is the
    engine's ONE lifetime mechanism -- not lists kept until a join: a forward has no join (an inference pass not even a ctx),
    and joining there would serialise what the side stream overlaps.
    event=True: blk.ready is an event behind the block; main orders itself after the block with blk.wait() or, in a later
    pass, by handing the event to an inline block as `after` (blocks ON the side stream follow it by stream order)."""
    def __init__(self, main, side, reads=(), after=None, event=False):
        self.main, self.side, self.reads, self.after, self.event, self.ready = main, side, reads, after, event, None
        self.inline, self.stream = side is None, main if side is None else side

    def __enter__(self):
        if self.inline:
            if self.after is not None:
                self.main.wait_event(self.after)
            return self
        self.side.wait_stream(self.main)
        self._cm = torch.cuda.stream(self.side)
        self._cm.__enter__()
        return self

    def __exit__(self, *exc):
        if not self.inline:
            if self.event:
                self.ready = torch.cuda.Event()
                self.ready.record(self.side)
            self._cm.__exit__(*exc)
            for t in self.reads:
                if t is not None:
                    t.record_stream(self.side)

    def back(self, *results):
        for t in () if self.inline else results:
            if t is not None:
                t.record_stream(self.main)

    def wait(self):
        """main waits for the block (once)."""
        if self.ready is not None:
            self.main.wait_event(self.ready)
            self.ready = None


class Engine:
    """Forward / backward of the network on one device."""

    def __init__(self, in_dim, out_dim, hidden, layers, device, precision="fp32", sync_bn=False):
        if precision not in ("fp32", "bf16"):
            raise SepkernError("precision must be 'fp32' or 'bf16' (got %r)" % (precision,))
        # bf16: EVERY matrix product (input projections, Linear, the recurrence h W_hh^T, their data and weight
        # gradients) rounds both operands to bf16 on the way into the matrix cores and accumulates in fp32;
        # parameters, activations, cell state, gradients, BatchNorm, the loss and Adam stay fp32.
        self.precision, self.bf16 = precision, precision == "bf16"
        if hidden % 4 != 0 or hidden > 1024:
            raise SepkernError("hidden_dim must be a multiple of 4 and <= 1024 (got %d)" % hidden)
        # The three arithmetic arrangements of the products (_proj / _dgrad / _wgrad):
        #   nt (bf16, 8 | H): ROW-MAJOR bf16 copies of the operands (_copy; the backward recurrence writes the copy of dgx itself,
        #     sk_hprev_rows the recurrent inputs); a factor whose rows are the contraction index enters K-major (sk_gemm_bf16_mm);
        #   planes (fp32, 8 | H, split GEMM variants; _planes()): the weight gradients read operands their producers cut into
        #     the three bf16 pieces, bit for bit the products of the 128 x 128 split kernel on the fp32 operands;
        #   otherwise the kernels that read fp32 operands (bf16: rounded on the way into LDS -- same arithmetic, half the speed).
        self.nt = self.bf16 and hidden % 8 == 0
        vars(self).update(_switches(self.bf16, hidden))
        self.sync_bn = self.sync_bn or bool(sync_bn)
        self.I, self.O, self.H, self.L = in_dim, out_dim, hidden, layers
        self.layout = ParamLayout(in_dim, out_dim, hidden, layers)
        self._chunk = {name: (lo, hi) for name, lo, hi in self.layout.grad_chunks()}
        self.device = device
        self.flat = torch.zeros(self.layout.total, device=device)
        # [guard words | gradients]: the recurrence's sticky status (sepkern/ops.lstm_sticky) is copied into word 0 at the
        # end of every backward, so the data-parallel all-reduce of the buffer tells EVERY rank when any rank's
        # persistent launch timed out, and the fused clip+Adam skips that step on the device (no host sync per step).
        # In FRONT of the gradients: the bottom layer's gradients are the last to be complete, so in the chunked exchange
        # (ParamLayout.grad_chunks) the guard travels with the last chunk.
        G = ParamLayout.GUARD
        self.grad_full = torch.zeros(G + self.layout.total, device=device)
        self.grad, self.guard = self.grad_full[G:], self.grad_full[0:1]
        self.running_mean, self.running_var = torch.zeros(2 * hidden, device=device), torch.ones(2 * hidden, device=device)
        self.eps, self.momentum = 1e-5, 0.1
        self.side = None
        self.grads_fresh = True        # True: next backward may overwrite instead of accumulate
        self.version = 0               # bumped by whoever writes the parameters (ClipAdam, load_state_dict): see backward()

    def p(self, name):
        return self.layout.view(self.flat, name)

    def param_version(self):
        """Changes whenever the parameters were written: `version` is bumped by sepkern.optim.ClipAdam (its kernel writes
        through raw pointers), torch's own counter covers in-place torch ops on the flat buffer or its views."""
        return (self.version, self.flat._version)

    def g(self, name):
        return self.layout.view(self.grad, name)

    def zero_grad(self):
        """model.zero_grad(): the next backward overwrites every gradient element, so nothing is memset."""
        self.grads_fresh = True

    def check_status(self):
        """Host-side check (synchronises): raises SepkernError if a persistent recurrence launch timed out since the
        last check.  Training does not need it per step -- see `guard` -- drivers call it at epoch / checkpoint time."""
        ops.lstm_status(ops.workspace(0, "lstm"))

    def sticky(self):
        """The workspace's sticky status word as a device tensor (1 element, int32): non-zero after a timed-out launch."""
        return ops.lstm_sticky(ops.workspace(0, "lstm"))

    def pad_row(self):
        """(out_dim,) the mask the reference's network shows at a zero-padded frame with the statistics of the last forward:
        sigmoid(lin(bn(0))) (archs/uPIT.py:135-144 run BatchNorm / Linear / sigmoid over the padded (B, T_max) grid).  The
        engine never computes padded frames; callers that hand out padded masks (SepDNN.forward, run_net) fill them in."""
        mean, var = self._last_bn
        Wf, bf_, _, _ = ops.bn_fold(self.p("lin.weight"), self.p("lin.bias"), mean, var, self.p("bn.weight"), self.p("bn.bias"),
                                    self.eps)
        zero = torch.zeros(1, 2 * self.H, device=self.device)
        row = torch.empty(1, self.O, device=self.device)
        ops.gemm(zero, Wf, row, 1, self.O, 2 * self.H, 2 * self.H, 2 * self.H, self.O, transB=True, bias=bf_, act=1)
        return row.view(-1)

    def _side(self, main, create=True):
        """The side stream if this pass co-schedules (persistent recurrences to run beside, a second layer), else None -- asked at
        the start of every pass, so `overlap` and `lstm_mode` may be assigned between passes.  create=False (a forward that saves
        nothing: inference) works ahead on the side stream only if a training pass has made one; it never creates it."""
        if not (self.overlap and self.lstm_mode == 0 and self.L > 1):
            return None
        if self.side is None and create:
            self.side = torch.cuda.Stream(device=main.device)
        return self.side

    def _planes(self):
        """Whether a saving forward cuts the weight gradients' operands into planes: only under the split arithmetic -- with
        fp32-MFMA variants asked for (8 / 1, the reference's literal arithmetic) they stay fp32-MFMA products of fp32 operands."""
        return self.wgrad_planes and self.var_side in (0, 2) and self.var_main in (0, 2, 9)

    def _put(self, name, val, acc):
        """Small gradient vectors produced by non-accumulating kernels."""
        (self.g(name).add_ if acc else self.g(name).copy_)(val)

    def _hand_over(self, reducer, name, stream):
        """Data-parallel chunked exchange: the kernels that complete chunk `name` of grad_chunks() are enqueued on `stream`."""
        if reducer is not None:
            reducer.chunk(self.grad_full, *self._chunk[name], stream)

    # ------------------------------------------------------------------ the three kinds of product
    # All of them over packed rows: operands are (Rp, C) row buffers with zero tail rows; row-parallel products write the
    # R valid rows, contractions over rows run over all Rp (whole K steps).
    # fp32: the fp32 MFMA kernels on the fp32 tensors.  bf16: sk_gemm_bf16_nt / _mm on bf16 copies; `cache` (one dict per
    # step) holds the copies already made, keyed by (address, shape) of the fp32 tensor, and keeps them alive.
    @staticmethod
    def _cache_put(cache, t2d, copy):
        """`copy`, just enqueued on the current stream, is t2d's bf16 copy for the rest of the step.  The entry holds the fp32 SOURCE
        too: its address cannot be recycled for another tensor of the same shape while the copy is cached (sources are not
        written between their uses within a step)."""
        cur, ev = torch.cuda.current_stream(), torch.cuda.Event()
        ev.record(cur)
        cache[(t2d.data_ptr(), tuple(t2d.shape))] = ent = (copy, ev, cur, t2d)
        return ent

    @staticmethod
    def _copy(cache, t2d):
        """Row-major bf16 copy of t2d (whole K steps of zero rows behind it: it may serve as a K-major factor), made once per
        step.  A copy made on one stream and used on the other is ordered by ITS OWN event: the user waits for that cast, not
        for everything the maker's stream has queued behind it."""
        cur = torch.cuda.current_stream()
        ent = cache.get((t2d.data_ptr(), tuple(t2d.shape)))
        if ent is None:
            ent = Engine._cache_put(cache, t2d, ops.cast_bf16(t2d, rows=ops.pad_to(t2d.shape[0], 64) + 64))
        elif ent[2] != cur:
            cur.wait_event(ent[1])
            ent[0].record_stream(cur)
        return ent[0]

    @staticmethod
    def _bf16_rows(R, Rp, C, dev):
        """A bf16 row buffer that a kernel fills with R rows of C columns and that then serves as a K-major factor: leading
        dimension C rounded up to 64, whole K steps of zero rows behind the data (everything outside [:R, :C] is zero)."""
        rows, ld = ops.pad_to(Rp, 64) + 64, ops.pad_to(C, 64)
        if ld != C:
            return torch.zeros(rows, ld, dtype=torch.bfloat16, device=dev)
        buf = torch.empty(rows, ld, dtype=torch.bfloat16, device=dev)
        buf[R:].zero_()
        return buf

    def _proj(self, cache, inp2d, w, out2d, bias, R, act=0):
        """out[:R] (R, N) = act(inp[:R] (R, K) w (N, K)^T + bias)."""
        N, K = w.shape[0], inp2d.shape[1]
        if not self.nt:
            ops.gemm(inp2d, w, out2d, R, N, K, inp2d.stride(0), K, N, transB=True, bias=bias, act=act, bf16=self.bf16, variant=self.var_main)
            return
        a, b = self._copy(cache, inp2d), self._copy(cache, w)
        # (not the stream-K kernel: with 1400 tiles of 28 K steps its fix-up costs more than the sixth partial round it saves --
        # main-stream products 3.03 vs 3.11 ms per step; the data gradients' 350 tiles of 112 steps are where it pays)
        ops.gemm_bf16_nt(a, b, out2d, R, N, a.shape[1], a.shape[1], b.shape[1], N, bias=bias, act=act)

    def _dgrad(self, cache, dout2d, w, out2d, R, ws_tag):
        """out[:R] (R, K) = dout[:R] (R, N) w (N, K)."""
        N, K = dout2d.shape[1], w.shape[1]
        if not self.nt:
            # large data gradients unsplit (stream-K / 256 x 128 tiles: 125.5-134.6 TFLOP/s against 119-120 for two K slices)
            sk = 1 if (not self.bf16 and R >= 4096 and K >= 1024 and N % 16 == 0) else 0
            ops.gemm(dout2d, w, out2d, R, K, N, N, K, K, splitk=sk, ws_tag=ws_tag, bf16=self.bf16, variant=self.var_main)
            return
        # w (N, K) is the K-major B of the product as it lies (contraction over its rows, zero rows up to dout's padded width)
        a, b = self._copy(cache, dout2d), self._copy(cache, w)
        ops.gemm_bf16_mm(a, b, out2d, R, K, a.shape[1], a.shape[1], b.shape[1], K, b_kmajor=True, splitk=0, ws_tag=ws_tag, streamk=True)

    def _wgrad(self, cache, dout2d, inp2d, gw, acc, ws_tag, beside=False, batch=1, sA=0, sB=0, sC=0):
        """gw ([batch,] N, K) [+]= dout (Rp, >= N)^T inp (Rp, >= K), contraction over all Rp rows (zero tails).  batch = 2 with
        operand strides: the two directions of the recurrent weight gradient in one launch.  The operands are a layer's, in the
        arrangement its forward chose: both Planes, or fp32 / bf16 row buffers.  beside=True: the product runs co-resident with
        a recurrence (side stream): the GEMM variant that fits there (var_side)."""
        N, K = gw.shape[-2:]
        if isinstance(dout2d, ops.Planes):              # operands that arrive split (fp32): both factors as planes
            ops.gemm_pl3_tn(dout2d, inp2d, gw, N, K, dout2d.rows, accumulate=acc, batch=batch, sA=sA, sB=sB, sC=sC, splitk=0, ws_tag=ws_tag)
            return
        Rp = dout2d.shape[0]
        if not self.nt:
            ops.gemm(dout2d, inp2d, gw, N, K, Rp, dout2d.stride(0), inp2d.stride(0), K, transA=True, accumulate=acc, splitk=0,
                     batch=batch, sA=sA, sB=sB, sC=sC, ws_tag=ws_tag, bf16=self.bf16, variant=self.var_side if beside else self.var_main)
            return
        # both factors K-major as they lie (their rows are the contraction index)
        a = dout2d if dout2d.dtype == torch.bfloat16 else self._copy(cache, dout2d)
        b = inp2d if inp2d.dtype == torch.bfloat16 else self._copy(cache, inp2d)
        ops.gemm_bf16_mm(a, b, gw, N, K, ops.pad_to(Rp, 64), a.shape[1], b.shape[1], K, a_kmajor=True, b_kmajor=True,
                         accumulate=acc, batch=batch, sA=sA, sB=sB, sC=sC, splitk=0, ws_tag=ws_tag, streamk=not beside and batch == 1)

    def _hprev(self, y, h0l, pk):
        """The recurrent inputs of a layer's packed rows (sk_hprev_rows), as the operand its recurrent weight gradient reads."""
        hp = self._bf16_rows(pk.R, pk.Rp, 2 * self.H, y.device) if self.nt else pk.rows(2 * self.H)
        return ops.hprev_rows(y, h0l, pk, self.H, hp)

    # ------------------------------------------------------------------ forward
    def _layer_weights(self, l, ws_tag="bn"):
        """(W_ih of layer l with rows gate-interleaved and columns zero-padded, summed bias gate-interleaved)."""
        H = self.H
        I = self.I if l == 0 else 2 * H
        wih = self.p("weight_ih_l%d" % l)
        # b_ih + b_hh for both directions: the two bias blocks are adjacent rows of a (2, 8H) matrix
        off_ih, _ = self.layout.blocks["bias_ih_l%d" % l]
        bsum = torch.empty(8 * H, device=wih.device)
        ops.colsum(self.flat[off_ih:], 2, 8 * H, 8 * H, bsum, ws_tag=ws_tag)
        # the recurrence keeps i,f,g,o of a cell adjacent (one 16-byte access per cell and step instead of four H-strided ones):
        # reorder the rows of W_ih and of the bias once, the GEMM then writes gx in that order ... and in the same pass pad layer
        # 0's input width to a multiple of 16 with zero columns (F = 257 -> 272; RSH 514 -> 528): rows 16-byte aligned AND K whole
        # 16-deep K steps, what the split-product kernels ask for.  The layers above read y (2H columns, 4 | 2H) as it lies
        Ip = ops.pad_to(I, 16 if l == 0 else 4)
        wih_gi = ops.gate_rows(wih.view(8 * H, I), H, out=torch.empty(8 * H, Ip, device=wih.device), cols=I)
        return wih_gi, ops.gate_rows(bsum, H)

    def _layer_forward(self, ps, l, inp, inp_pl, weights, h0, c0, hn, cn):
        """Layer l on the rows `inp` (inp_pl: the same as Planes, where the layer below made them) -> (LayerSaved, y as Planes
        or None, the recurrence's workspace)."""
        pk, H = ps.pk, self.H
        R, Rp = pk.R, pk.Rp
        wih_gi, bsum = weights
        Ip = wih_gi.shape[1]
        # The weight gradients contract over all Rp rows of `inp` and rely on ZERO tail rows R..Rp.  The layers above
        # the first read y = pk.rows() (zero tail by construction); the caller's x2d is only known to hold R rows, so
        # it is taken as it is only when there is no tail (R == Rp) -- whatever lies behind row R of a larger buffer
        # (another batch, NaN) never enters a product.
        if Ip != inp.shape[1] or inp.shape[0] < Rp or not inp.is_contiguous() or (l == 0 and Rp > R):
            inp = ops.pad_rows(inp[:R], Ip, rows=Rp)   # one pass, no memset (F = 257 -> 272; tail rows zero)
        gx = pk.rows(8 * H)
        if ps.planes and l == 0:
            # the (padded) network input as planes, for layer 0's weight gradient: beside its projection
            with _Beside(ps.main, ps.side, reads=(inp,)) as blk:
                inp_pl = ops.split_rows(inp, R)
            blk.back(inp_pl)
        self._proj(ps.cache, inp, wih_gi, gx, bsum, R)
        y = pk.rows(2 * H)
        cs = torch.empty(Rp, 2 * H, device=y.device) if ps.save else None
        sl = slice(2 * l, 2 * l + 2)
        ws = ops.lstm_fwd(gx, self.p("weight_hh_l%d" % l), h0[sl], c0[sl], pk.lens, y, gx if ps.save else None, cs,
                          None if hn is None else hn[sl], None if cn is None else cn[sl], pk.T, pk.B, H,
                          self.lstm_mode | self.fwd_bits, bf16=self.bf16, offs=None if pk.uniform else pk.offs, rows=R)
        hp = hp_ready = y_pl = None
        if ps.save:
            # the recurrent inputs of the layer's rows, for its recurrent weight gradient: gathered HERE, beside the next
            # layer's projection, not in the backward pass where the side stream is the bound (planes: cut there too, and so
            # is y -- the next layer's input, or the Linear layer's: the other factor of their weight gradients)
            with _Beside(ps.main, ps.side, reads=(y,), event=True) as blk:
                hp = self._hprev(y, h0[sl], pk)
                if ps.planes:
                    hp, y_pl = ops.split_rows(hp, R), ops.split_rows(y, R)
            blk.back(hp, y_pl)
            hp_ready = blk.ready
        return LayerSaved(inp, gx, cs, y, wih_gi, hp, hp_ready, inp_pl), y_pl, ws

    def _head_forward(self, ps, y_top, training, ws):
        """BatchNorm1d + Linear + sigmoid on the top layer's rows -> (mask (Rp, out_dim), mean, var, bn_count, xbn, fold)."""
        pk, H = ps.pk, self.H
        R, dev = pk.R, y_top.device
        count = pk.B * pk.T           # BatchNorm1d sees the zero-padded (B, 2H, T_max) grid (archs/uPIT.py:135-138)
        if training:
            mean, var = torch.empty(2 * H, device=dev), torch.empty(2 * H, device=dev)
            ops.bn_stats(y_top, mean, var, rows=R, count=count)
            bn_count = float(count)
            if self.sync_bn:                             # statistics of the global batch (one all-gather)
                mean, var, bn_count = skdist.combine_bn_stats(mean, var, pk.B, pk.T)
            # (guarded: after a timed-out launch y is garbage and must not reach running statistics a checkpoint will hold)
            ops.bn_update_running(mean, var, self.running_mean, self.running_var, int(bn_count), self.momentum, guard=ops.lstm_sticky(ws))
        else:
            mean, var, bn_count = self.running_mean, self.running_var, float(count)
        self._last_bn = (mean, var)
        mask = torch.empty(pk.Rp, self.O, device=dev)
        xbn = fold = None
        if self.bn_fold:
            # BatchNorm folded into the Linear weights (sk_bn_fold): mask = sigmoid(y Wf^T + bf), the
            # normalised activations are never written (one 92 MB pass less, forward and backward)
            Wf, bf_, *fold = ops.bn_fold(self.p("lin.weight"), self.p("lin.bias"), mean, var, self.p("bn.weight"), self.p("bn.bias"), self.eps)
            self._proj(ps.cache, y_top, Wf, mask, bf_, R, act=1)
        else:
            xbn = pk.rows(2 * H)
            ops.bn_apply(y_top[:R], mean, var, self.p("bn.weight"), self.p("bn.bias"), xbn, self.eps)
            self._proj(ps.cache, xbn, self.p("lin.weight"), mask, self.p("lin.bias"), R, act=1)
        return mask, mean, var, bn_count, xbn, fold

    def forward(self, x2d, pk, h0, c0, training, save, want_state=False):
        """x2d (>= R, in_dim) packed rows of the batch `pk` (sepkern.packing.Packing), h0/c0 (2L,B,H) in sorted order ->
        (mask (R, out_dim) packed, hn, cn (2L,B,H) or None, ctx or None).  ctx feeds backward(); several may be alive
        (the RSH arch runs the network num_spk times per batch)."""
        # (also taken: rows already as wide as layer 0 reads them, in_dim rounded up to 16 with ZERO columns behind in_dim --
        # sk_stft_ipd / sk_ipd_rows write them so; with R == Rp layer 0 then skips its sk_pad_rows pass)
        if x2d.dim() != 2 or x2d.shape[1] not in (self.I, ops.pad_to(self.I, 16)) or x2d.shape[0] < pk.R:
            raise SepkernError("forward: input is %s, expected (>= %d, %d) packed rows" % (tuple(x2d.shape), pk.R, self.I))
        L, dev = self.L, x2d.device
        main = torch.cuda.current_stream(dev)
        ps = _Pass(pk, main, self._side(main, create=save), {}, save=save, planes=save and self._planes())
        hn = torch.empty(2 * L, pk.B, self.H, device=dev) if want_state else None
        cn = torch.empty(2 * L, pk.B, self.H, device=dev) if want_state else None
        # The gate-interleaved W_ih and summed biases of the layers above the first depend on the weights only: with a side stream
        # they are made there, beside layer 0's projection and recurrence, not in front of each layer's projection on main
        ahead = {}
        if ps.side is not None:
            with _Beside(main, ps.side, event=True) as pre:
                for l in range(1, L):
                    ahead[l] = self._layer_weights(l, ws_tag="bn_side")
            pre.back(*[t for w in ahead.values() for t in w])
        inp, inp_pl, layers, ws = x2d, None, [], None
        for l in range(L):
            if l in ahead:
                pre.wait()
            rec, inp_pl, ws = self._layer_forward(ps, l, inp, inp_pl, ahead[l] if l in ahead else self._layer_weights(l), h0, c0, hn, cn)
            layers.append(rec)
            inp = rec.y
        if not save and not skdist.is_parallel():
            # inference: the caller copies the masks to the host next, a sync costs nothing.  Under data parallelism a
            # raise on ONE rank would leave the others waiting in their next collective: there the sticky word stays set
            # and the driver reports it on every rank together (steps/train_qsub.py::validation_pass)
            ops.lstm_status(ws)
        mask, mean, var, bn_count, xbn, fold = self._head_forward(ps, inp, training, ws)
        # (cache: the backward pass multiplies the SAME bf16 copies of the weights and layer inputs, none is written in between)
        ctx = FwdCtx(layers, mean, var, bn_count, xbn, fold, inp_pl, mask, pk, h0, c0, training, self.param_version(),
                     ps.cache if self.nt else None) if save else None
        return mask[:pk.R], hn, cn, ctx

    # ------------------------------------------------------------------ backward
    def _head_backward(self, ps, ctx, dmask, dz, reducer):
        """sigmoid, Linear and BatchNorm backward -> dy (Rp, 2H), the gradient wrt the top layer's output."""
        pk, H, O, cache = ps.pk, self.H, self.O, ps.cache
        R, Rp, dev = pk.R, pk.Rp, dmask.device
        ops.sigmoid_bwd(dmask[:R], ctx.mask[:R], dz)
        dxbn = torch.empty(Rp, 2 * H, device=dev)
        # (folded or not, the data gradient contracts with the UNFOLDED weight: dxbn is the gradient wrt bn(y))
        self._dgrad(cache, dz, self.p("lin.weight"), dxbn, R, "gemm")
        y_top = ctx.layers[-1].y
        dy = torch.empty(Rp, 2 * H, device=dev)
        dgamma, dbeta = torch.empty(2 * H, device=dev), torch.empty(2 * H, device=dev)
        ops.bn_bwd_sums(dxbn[:R], y_top[:R], ctx.mean, ctx.var, dgamma, dbeta, self.eps)
        self._put("bn.weight", dgamma, ps.acc)           # local sums: the flat all-reduce adds the ranks up later
        self._put("bn.bias", dbeta, ps.acc)
        if self.sync_bn:                                 # dx needs the sums over the global batch (one all-reduce)
            dgamma, dbeta = skdist.allreduce_bn_sums(dgamma, dbeta)
        ops.bn_bwd_apply(dxbn[:R], y_top[:R], ctx.mean, ctx.var, self.p("bn.weight"), dgamma, dbeta, dy, ctx.bn_count, self.eps)
        del dxbn
        # the Linear layer's own gradients are needed by nobody before clip+Adam: beside the top layer's recurrence
        # (enqueued HERE, after the BatchNorm backward on the main stream: issued earlier they ran beside those short
        # critical-path kernels and slowed them)
        with _Beside(ps.main, ps.side) as blk:
            tag, beside = ("", False) if blk.inline else ("_side", True)
            if ctx.fold is not None:
                # dW = dz^T bn(y) = (dz^T y) diag(s) + colsum(dz) t^T  (sk_bn_unfold_grad): the product runs against y itself
                G, dzsum = torch.empty(O, 2 * H, device=dev), torch.empty(O, device=dev)
                if ctx.ytop_planes is not None:
                    self._wgrad(cache, ops.split_rows(dz, R), ctx.ytop_planes, G, False, "gemm" + tag, beside)   # (R x O: a tenth of a layer's dgx)
                else:
                    self._wgrad(cache, dz, y_top, G, False, "gemm" + tag, beside)
                ops.colsum(dz, R, O, O, dzsum, ws_tag="bn" + tag)
                ops.bn_unfold_grad(G, dzsum, ctx.fold[0], ctx.fold[1], self.g("lin.weight"), accumulate=ps.acc)
                self._put("lin.bias", dzsum, ps.acc)
            else:
                self._wgrad(cache, dz, ctx.xbn, self.g("lin.weight"), ps.acc, "gemm" + tag, beside)
                ops.colsum(dz, R, O, O, self.g("lin.bias"), accumulate=ps.acc, ws_tag="bn" + tag)
        self._hand_over(reducer, "lin+bn", blk.stream)   # (bn.weight / bn.bias were put before the side stream forked)
        return dy

    def _layer_backward(self, ps, l, rec, dy, dbias, c0, state, want_din, reducer):
        """Layer l from dy (Rp, 2H) and state = (dhn, dcn, dh0, dc0) of all layers; dbias: room for its bias-gradient partials ->
        (the gradient wrt its input -- the next dy, at layer 0 the caller's dx (R, in_dim) -- or None, the recurrence's workspace)."""
        pk, H, cache = ps.pk, self.H, ps.cache
        R, Rp, B, dev = pk.R, pk.Rp, pk.B, dy.device
        I = self.I if l == 0 else 2 * H
        Ip = rec.wih_gi.shape[1]
        planes = rec.inp_planes is not None
        mode = self.lstm_mode | self.bwd_bits
        if planes and (self.bwd_exclusive == "1" or (self.bwd_exclusive == "auto" and not pk.uniform and B > 16)):
            mode |= ops.LSTM_BWD_EXCLUSIVE           # its CUs to itself while the weight gradients run (why on ragged batches: DESIGN.md 6)
        sl = slice(2 * l, 2 * l + 2)
        dhn, dcn, dh0, dc0 = (None if t is None else t[sl] for t in state)      # the layer's (2, B, H) of each state gradient
        dgx = rec.gates                                  # overwritten in place, cell by cell
        # The recurrence writes dgx a second time in the form the layer's products read: its three bf16 planes for the two weight
        # gradients (fp32), or the bf16 operand copy of all three products instead of a cast pass over 4 x the bytes
        twin = ops.Planes.empty(R, 8 * H, dev) if planes else self._bf16_rows(R, Rp, 8 * H, dev) if self.nt else None
        ws = ops.lstm_bwd(dy, self.p("weight_hh_l%d" % l), dgx, rec.cs, c0[sl], pk.lens, dgx, dh0, dc0, pk.T, B, H,
                          mode, dhn=dhn, dcn=dcn, bf16=self.bf16, dbias=dbias, dgx_bf16=twin,
                          offs=None if pk.uniform else pk.offs, rows=R)
        if self.nt:
            self._cache_put(cache, dgx, twin)
        dgx_op, inp_op = (twin, rec.inp_planes) if planes else (dgx, rec.inp)       # the weight gradients' two operands
        din = None
        if want_din:                                     # the only product the next recurrence (or the caller) waits for
            din = torch.empty(Rp, Ip, device=dev)
            self._dgrad(cache, dgx, rec.wih_gi, din, R, "gemm_dgrad")
            if l == 0:
                din = din[:R] if Ip == I else din[:R, :I].contiguous()
        # The weight gradients of the layers above the first run beside the NEXT recurrence; layer 0's inline: they share nothing with
        # the side stream's but bf16 operand copies, which carry their own events (_copy), so they start as layer 0's recurrence ends
        with _Beside(ps.main, ps.side if l > 0 else None, reads=(twin,) if planes else (), after=rec.hprev_ready) as blk:
            tag, beside = ("main", False) if blk.inline else ("side", True)
            gw_hh = torch.empty(2, 4 * H, H, device=dev)     # rows gate-interleaved, like dgx (sk_gate_rows puts them back)
            gw_ih = torch.empty(8 * H, Ip, device=dev)       # (both allocated HERE: memory of the stream that uses it, no event at release)
            # dW_hh[d] = sum_rows dG[:, d]^T hprev[:, d-half]: both directions as one batched launch
            self._wgrad(cache, dgx_op, rec.hprev, gw_hh, False, "gemm_" + tag, beside, batch=2, sA=4 * H, sB=H, sC=4 * H * H)
            # dW_ih (both directions stacked as (8H, I)) = dgx^T x_in
            self._wgrad(cache, dgx_op, inp_op, gw_ih, False, "gemm_" + tag, beside)
            ops.gate_rows(gw_hh, H, back=True, out=self.g("weight_hh_l%d" % l), accumulate=ps.acc)
            ops.gate_rows(gw_ih, H, back=True, out=self.g("weight_ih_l%d" % l).view(8 * H, I), accumulate=ps.acc, cols=I)
            db = torch.empty(8 * H, device=dev)
            ops.colsum(dbias, dbias.shape[0], 8 * H, 8 * H, db, ws_tag="bn_" + tag)       # a few rows: the kernel did the sums
            self._put("bias_ih_l%d" % l, db.view(2, 4 * H), ps.acc)
            self._put("bias_hh_l%d" % l, db.view(2, 4 * H), ps.acc)
        if l > 0:
            self._hand_over(reducer, "layer%d" % l, blk.stream)
        return din, ws

    def backward(self, ctx, dmask, dhn=None, dcn=None, want_dx=False, want_dstate=False, reducer=None):
        """Parameter gradients (into the flat gradient buffer) from dmask (R, out_dim) packed and, optionally, the
        gradient wrt the final state (dhn, dcn (2L,B,H)).  Returns (dx (R, in_dim) packed or None, dh0, dc0 or None).
        reducer (sepkern.dist.GradReducer, data-parallel runs with SEPKERN_DP_OVERLAP=1, last backward of a step only):
        every chunk of ParamLayout.grad_chunks() is handed over as soon as the kernels that complete it are enqueued."""
        if ctx is None:
            raise SepkernError("backward called without a saved forward")
        if not ctx.training:
            raise SepkernError("backward through eval-mode BatchNorm is not built")
        pk, L, dev = ctx.pk, self.L, dmask.device
        main = torch.cuda.current_stream(dev)
        # bf16 operand copies (see _copy): the forward's, unless the parameters were written since (a backward of a ctx saved
        # before an optimizer step would otherwise multiply stale bf16 weight copies against the new fp32 weights)
        cache = ctx.cache if (ctx.cache is not None and ctx.version == self.param_version()) else {}
        ps = _Pass(pk, main, self._side(main), cache, acc=not self.grads_fresh)
        # dz and the bias-gradient partials, written on main and read on the side stream: allocated HERE, they outlive the join
        dz = pk.rows(self.O)
        dbias = torch.empty(L, (pk.B + 15) // 16, 8 * self.H, device=dev)
        dy = self._head_backward(ps, ctx, dmask.contiguous(), dz, reducer)
        dh0 = torch.empty(2 * L, pk.B, self.H, device=dev) if want_dstate else None
        dc0 = torch.empty(2 * L, pk.B, self.H, device=dev) if want_dstate else None
        for l in range(L - 1, -1, -1):
            dy, ws = self._layer_backward(ps, l, ctx.layers[l], dy, dbias[l], ctx.c0, (dhn, dcn, dh0, dc0), want_dx or l > 0, reducer)
        if ps.side is not None:
            main.wait_stream(ps.side)
        self.guard.copy_(ops.lstm_sticky(ws))      # int32 -> float: non-zero = this step's gradients are garbage
        self._hand_over(reducer, "guard+layer0", main)
        self.grads_fresh = False
        return dy, dh0, dc0        # (dy: layer 0's input gradient, the caller's dx)
