"""Tensor-level wrappers over the C ABI (include/sepkern.h).

PyTorch supplies device memory and the current HIP stream; all arithmetic is in libsepkern.so.
Every wrapper takes fp32 CUDA tensors and passes raw device pointers.
"""
import ctypes as C
import itertools

import torch

from . import _lib
from . import cacgmm as _cacgmm
from . import dpcl as _dpcl
from . import wpe as _wpe

_WS = {}

# Optional per-kernel-class timing with HIP events recorded on the launch stream (bench.py):
# PROF = {} enables it; each timed call appends (class, start_event, end_event, flops).
PROF = None


class _timed:
    def __init__(self, cls, flops=0.0):
        self.cls, self.flops = cls, flops

    def __enter__(self):
        if PROF is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if PROF is not None:
            self.e1.record()
            # launches on a side stream are co-scheduled with other kernels: their durations are kept apart
            side = torch.cuda.current_stream() != torch.cuda.default_stream()
            PROF.setdefault(self.cls + ("@side" if side else ""), []).append((self.e0, self.e1, self.flops))
        return False


def prof_summary():
    """{class: (launches, total_ms, total_flops)} -- call after torch.cuda.synchronize()."""
    out = {}
    for cls, recs in (PROF or {}).items():
        out[cls] = (len(recs), sum(a.elapsed_time(b) for a, b, _ in recs), sum(f for _, _, f in recs))
    return out


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t, dtype=torch.float32):
    if t is None:
        return
    if not t.is_cuda:
        raise _lib.SepkernError("sepkern ops need CUDA(HIP) tensors; got a CPU tensor (there is no CPU path)")
    if t.dtype != dtype:
        raise _lib.SepkernError("expected dtype %s, got %s" % (dtype, t.dtype))


def _dense(what, *ts):
    """The wrappers below pass shape[1] as the row stride: a view with any other stride would be read wrong."""
    for t in ts:
        _chk(t)
        if not t.is_contiguous():
            raise _lib.SepkernError("%s needs contiguous tensors (got strides %s for shape %s)" % (what, tuple(t.stride()), tuple(t.shape)))


def workspace(nbytes, tag="default"):
    """A cached per-(device, tag) scratch buffer of at least nbytes (owned by torch's allocator)."""
    key = (torch.cuda.current_device(), tag)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        # zeroed: the LSTM workspace starts with a sticky status word that no launch clears (include/sepkern.h) ...
        old, ws = ws, torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")
        if old is not None and tag == "lstm":
            ws[:4].copy_(old[:4])      # ... and a larger request must not lose it (RSH passes of different (T, B))
        _WS[key] = ws
    return ws


def device_info():
    ncu, lds = C.c_int(0), C.c_int(0)
    _lib.call("sk_device_info", C.byref(ncu), C.byref(lds))
    return ncu.value, lds.value


# ----------------------------------------------------------------------------- GEMM
_NUM_CUS = None


def _num_cus():
    """The device's CU count (queried once)."""
    global _NUM_CUS
    if _NUM_CUS is None:
        _NUM_CUS = device_info()[0]
    return _NUM_CUS


def pick_splitk(M, N, K, batch=1):
    """K slices for a product with few output tiles and a long K (weight gradients; the N = 2H data gradient):
    the matrix pipe of a CU is saturated by its resident 128x128 blocks, so time goes with the LARGEST number
    of blocks any CU gets, ceil(blocks / CUs); choose the slice count that minimises that quantisation loss
    plus the cost of writing and re-reading the partial slabs (measured: 1400 tiles on 256 CUs run at 91 %)."""
    cus = _num_cus()
    tiles = ((M + 127) // 128) * ((N + 127) // 128) * batch
    if tiles >= 16 * cus or K < 2048:
        return 1
    work = 2.0 * M * N * K * batch / 140e12                      # seconds at the kernel's un-quantised rate
    best, best_t = 1, None
    for s in range(1, 33):
        if K // s < 512:
            break
        per_cu = tiles * s / cus
        eff = per_cu / -(-(tiles * s) // cus) * min(1.0, 0.55 + 0.15 * min(per_cu, 3.0))   # <3 blocks/CU: poor overlap
        t = work / eff + (0 if s == 1 else 2.0 * s * M * N * batch * 4 / 4e12)
        if best_t is None or t < best_t * 0.995:
            best, best_t = s, t
    return best


def gemm(A, B, Cout, M, N, K, lda, ldb, ldc, transA=False, transB=False, bias=None, accumulate=False, act=0,
         batch=1, sA=0, sB=0, sC=0, sbias=0, splitk=1, ws_tag="gemm", bf16=False, variant=0):
    """Cout[M,N] = act(opA(A) opB(B) + bias (+ Cout)).  A/B/Cout are tensors whose data_ptr() is the
    first element of the operand (views are fine: leading dimensions are explicit).  splitk > 1 (or 0 =
    choose) splits K into deterministic partial slabs -- for weight gradients.  bf16=True rounds A and B to
    bf16 on the way into the matrix cores (fp32 accumulate; everything in memory stays fp32).  variant (fp32 only,
    sk_gemm_f32_splitk's `variant`): 0 choose -- the three-way bf16 split of both operands on the bf16 matrix pipe (six piece
    products per element pair: fp32 products in another summation order) wherever the operands are aligned, else the
    fp32-MFMA kernels; 1 the register-staged fp32-MFMA kernel; 2 / 9 the 128 x 128 / 256 x 128 split-once-while-staging split
    kernels; 3 / 4 / 6 the 128 x 128 / 256 x 128 / stream-K 256 x 256 fp32-MFMA LDS-DMA kernels; 8 choose among the fp32-MFMA
    kernels only (the reference's literal arithmetic; SEPKERN_GEMM_SPLIT=0 makes 0 mean this)."""
    for t in (A, B, Cout, bias):
        _chk(t)
    if splitk == 0:
        splitk = pick_splitk(M, N, K, batch)
    ws = None
    if splitk > 1:
        ws = workspace(_lib.load().sk_gemm_workspace_bytes(M, N, batch, splitk), ws_tag)
    elif not bf16 and batch == 1 and (variant == 6 or (M >= 4096 and N >= 1024 and
                                                       (variant == 0 or (variant == 8 and not transA)))):
        ws = _streamk_ws()                                                              # pieces of the stream-K cut
    with _timed("gemm_bf16_kernel" if bf16 else "gemm_f32_kernel", 2.0 * M * N * K * batch) as rec:
        args = (_ptr(A), _ptr(B), _ptr(Cout), _ptr(bias), M, N, K, lda, ldb, ldc, int(transA), int(transB), int(accumulate),
                int(act), batch, sA, sB, sC, sbias, int(splitk), _ptr(ws))
        if bf16:
            _lib.call("sk_gemm_bf16_splitk", *args, _stream())
        else:
            _lib.call("sk_gemm_f32_splitk", *args, int(variant), _stream())
            if PROF is not None and _lib.load().sk_gemm_last_kernel() in (2, 10):
                # the launch ran on the bf16 matrix pipe (split products): its own class -- another pipe, another peak
                rec.cls = "gemm_f32_split_kernel"


def _streamk_ws():
    """The stream-K kernels' workspace (ticket counters + piece slabs, 134 MB): ONE per stream -- launches on a stream run
    in order, so they can share it; two streams never do (their tickets and slabs would mix)."""
    return workspace(_lib.load().sk_gemm_streamk_workspace_bytes(), "streamk_%x" % torch.cuda.current_stream().cuda_stream)


def pad_to(n, m):
    return (n + m - 1) // m * m


def cast_bf16(x2d, ld=None, out=None, rows=None):
    """bf16 copy of an fp32 (R, C) matrix (row stride x2d.stride(0)), leading dimension ld >= C (default: C rounded
    up to 64), extra columns zero; rows >= R: that many rows are written, those past R zero (a copy that also serves as
    a K-major factor, gemm_bf16_mm).  Returns the (rows or R, ld) bfloat16 tensor."""
    _chk(x2d)
    R, Cc = x2d.shape
    ld = pad_to(Cc, 64) if ld is None else ld
    rows = R if rows is None else rows
    if out is None:
        out = torch.empty(rows, ld, dtype=torch.bfloat16, device=x2d.device)
    _lib.call("sk_cast_bf16_rows", _ptr(x2d), R, Cc, x2d.stride(0), _ptr(out), ld, rows, _stream())
    return out


class Planes:
    """The three bf16 planes (hi, mid, lo pieces: x = hi + mid + lo exactly) of an fp32 (R, C) matrix: t is a (3, rows, ld)
    bfloat16 tensor, ld = C rounded up to 8, rows >= R rounded up to 64 with zero tail rows ("operands that arrive split",
    include/sepkern.h).  Made by split_rows() or by lstm_bwd(dgx_bf16=Planes.empty(...))."""

    def __init__(self, t, R, C):
        self.t, self.R, self.C = t, R, C
        self.rows, self.ld = t.shape[1], t.shape[2]
        self.plane = t.stride(0)

    def record_stream(self, stream):
        self.t.record_stream(stream)

    @staticmethod
    def empty(R, C, device, zero_tail=True):
        rows, ld = pad_to(R, 64), pad_to(C, 8)
        t = torch.empty(3, rows + 1, ld, dtype=torch.bfloat16, device=device)[:, :rows]     # (+1 row: a clamped edge tile may read past the last row's end)
        if zero_tail and (rows > R or ld > C):
            t[:, R:].zero_()
            if ld > C:
                t[:, :, C:].zero_()
        return Planes(t, R, C)


def split_rows(x2d, R=None):
    """Planes of the first R rows of an fp32 (>= R, C) matrix (sk_split_rows: one pass, 4 bytes read and 6 written per element)."""
    _chk(x2d)
    R = x2d.shape[0] if R is None else R
    Cc = x2d.shape[1]
    pl = Planes.empty(R, Cc, x2d.device, zero_tail=False)
    with _timed("split_rows_kernel", 0.0):
        _lib.call("sk_split_rows", _ptr(x2d), R, Cc, x2d.stride(0), _ptr(pl.t), pl.ld, pl.rows, pl.plane, _stream())
    return pl


def gemm_pl3_tn(A, B, Cout, M, N, K, accumulate=False, batch=1, sA=0, sB=0, sC=0, splitk=1, ws_tag="gemm"):
    """Cout[M, N] (+)= A^T B with A, B Planes whose rows are the contraction index (K <= their row counts, K % 16 == 0): the weight
    gradients on operands that arrive split (sk_gemm_pl3_tn).  batch / strides (in columns) / splitk (0 = choose) as gemm()."""
    _chk(Cout)
    if splitk == 0:
        splitk = pick_splitk(M, N, K, batch)
    ws = workspace(_lib.load().sk_gemm_workspace_bytes(M, N, batch, splitk), ws_tag) if splitk > 1 else None
    with _timed("gemm_f32_split_kernel", 2.0 * M * N * K * batch):
        _lib.call("sk_gemm_pl3_tn", _ptr(A.t), _ptr(B.t), _ptr(Cout), M, N, K, A.ld, B.ld, Cout.stride(-2), A.plane, B.plane,
                  int(accumulate), batch, sA, sB, sC, int(splitk), _ptr(ws), _stream())


def gemm_bf16_nt(A, B, Cout, M, N, K, lda, ldb, ldc, bias=None, accumulate=False, act=0, batch=1, sA=0, sB=0, sC=0,
                 sbias=0, splitk=1, ws_tag="gemm", streamk=False):
    """Cout[M,N] = act(A[M,K] B[N,K]^T + bias (+ Cout)) with A, B bfloat16 tensors (K-contiguous, K % 64 == 0).
    streamk: as gemm_bf16_mm."""
    _gemm_bf16("sk_gemm_bf16_nt", (), A, B, Cout, M, N, K, lda, ldb, ldc, bias, accumulate, act, batch, sA, sB, sC, sbias,
               splitk, ws_tag, streamk)


def gemm_bf16_mm(A, B, Cout, M, N, K, lda, ldb, ldc, a_kmajor=False, b_kmajor=False, bias=None, accumulate=False, act=0, batch=1,
                 sA=0, sB=0, sC=0, sbias=0, splitk=1, ws_tag="gemm", streamk=False):
    """Cout[M,N] = act(opA opB + bias (+ Cout)) on bfloat16 operands in memory, either of them optionally K-MAJOR
    (a_kmajor: A stored [K][M] with lda elements between k rows; b_kmajor: B stored [K][N]) -- sk_gemm_bf16_mm.  Row-major
    operands: K-contiguous as in gemm_bf16_nt.  K % 64 == 0.  streamk=True (unbatched products that have the chip to
    themselves): the persistent stream-K kernel instead of K slices where it applies."""
    _gemm_bf16("sk_gemm_bf16_mm", (int(a_kmajor), int(b_kmajor)), A, B, Cout, M, N, K, lda, ldb, ldc, bias, accumulate, act,
               batch, sA, sB, sC, sbias, splitk, ws_tag, streamk)


def _gemm_bf16(entry, kmajor, A, B, Cout, M, N, K, lda, ldb, ldc, bias, accumulate, act, batch, sA, sB, sC, sbias, splitk,
               ws_tag, streamk):
    """gemm_bf16_nt / gemm_bf16_mm through their own entry points (kmajor: the (a_kmajor, b_kmajor) arguments of _mm)."""
    _chk(A, torch.bfloat16)
    _chk(B, torch.bfloat16)
    _chk(Cout)
    _chk(bias)
    ws = None
    if streamk and batch == 1 and splitk in (0, 1) and M >= 256 and (N % 256 == 0 or N > 1024) and K >= 512:
        splitk = 1
        ws = _streamk_ws()
    if splitk == 0:
        splitk = pick_splitk_bf16(M, N, K, batch)
    if splitk > 1:
        ws = workspace(_lib.load().sk_gemm_workspace_bytes(M, N, batch, splitk), ws_tag)
    with _timed("gemm_bf16_nt_kernel", 2.0 * M * N * K * batch):
        _lib.call(entry, _ptr(A), _ptr(B), _ptr(Cout), _ptr(bias), M, N, K, lda, ldb, ldc, *kmajor, int(accumulate), int(act),
                  batch, sA, sB, sC, sbias, int(splitk), _ptr(ws), _stream())


def pick_splitk_bf16(M, N, K, batch=1):
    """K slices for the 256 x 256-tile bf16 kernel (one block per CU): enough blocks to fill the chip about twice,
    slices of at least 1024."""
    cus = _num_cus()
    tiles = ((M + 255) // 256) * ((N + 255) // 256) * batch
    best, best_t = 1, None
    for s in range(1, 17):
        if K // s < 1024 and s > 1:
            break
        rounds = -(-(tiles * s) // cus)
        t = rounds / s + (0.0 if s == 1 else 0.02 * s)       # time ~ rounds x K/s, plus the slab round trip
        if best_t is None or t < best_t * 0.98:
            best, best_t = s, t
    return best


# ----------------------------------------------------------------------------- signal batches
# ONE flat 1-D tensor of samples, nested lists of offsets [list][B] into it and the samples per utterance: what every wrapper
# that takes such a batch checks and builds, stated once.  `who` is the wrapper's name, for the message.  The descriptor tensors
# must outlive the (asynchronous) launch call: a wrapper keeps its references until the call returns.
def _i64(vals, device):
    return torch.tensor(vals, dtype=torch.int64, device=device)


def _i32(vals, device):
    return torch.tensor(vals, dtype=torch.int32, device=device)


def _samples(who, t, what="samples", pcm=True):
    """t holds samples: on the device, 1-D, contiguous, float32 or (pcm) int16 PCM, which the kernels scale by 1/32768 -> pcm16."""
    pcm16 = pcm and t.dtype == torch.int16
    _chk(t, torch.int16 if pcm16 else torch.float32)
    if t.dim() != 1 or not t.is_contiguous():
        raise _lib.SepkernError("%s needs one contiguous 1-D tensor of %s (got strides %s for shape %s)" % (who, what, tuple(t.stride()), tuple(t.shape)))
    return pcm16


def prefix_sums(ns):
    """Lengths -> (where each begins when they lie back to back, their sum): one linear prefix sum."""
    starts = list(itertools.accumulate(ns, initial=0))
    total = starts.pop()
    return starts, total


def _lengths(who, nsamp, least=None, what="signal"):
    """nsamp -> (ns, starts, total); an empty batch is refused, and a length below `least` (None: the C side refuses short ones)."""
    ns = [int(n) for n in nsamp]
    if not ns or (least is not None and min(ns) < least):
        raise _lib.SepkernError("%s needs at least one %s%s" % (who, what, "" if least is None else ", each of at least %d samples" % least))
    return (ns,) + prefix_sums(ns)


def _offsets(who, offs, ns, numel, *counts):
    """Nested offset lists (any iterables) -> (the flat list in the order the kernels read them: the outermost list slowest, the
    B = len(ns) utterances fastest; then the number of lists found at every level).  counts: one (lo, hi, what) per level of
    lists above [B] -- none for a plain [B] list, one for [S][B], two for [S][P][B] --, the range their number must lie in and
    what they are, for the message; every list of a level is as long as the first.  Signal u of every innermost list is the
    ns[u] samples at its offset and must lie inside the buffer of numel elements (a negative length is refused here)."""
    rows, B, found = [offs], len(ns), []
    for lo, hi, what in counts:
        rows = [list(r) for r in rows]
        n = len(rows[0])
        if not lo <= n <= hi or any(len(r) != n for r in rows):
            raise _lib.SepkernError("%s needs %s lists of offsets, one per %s, each with one offset for each of the %d signals (got %d)"
                                    % (who, lo if lo == hi else "%d..%d" % (lo, hi), what, B, n))
        found.append(n)
        rows = [x for r in rows for x in r]
    rows = [[int(o) for o in r] for r in rows]
    if any(len(r) != B for r in rows):
        raise _lib.SepkernError("%s needs one offset per signal: lists of %d (got %s)" % (who, B, sorted({len(r) for r in rows})))
    if min(ns) < 0 or any(o < 0 or o + n > numel for r in rows for o, n in zip(r, ns)):
        raise _lib.SepkernError("%s: a signal runs past its buffer (or has a negative offset or length)" % who)
    return ([o for r in rows for o in r], *found)


def _out(who, out, size, like):
    """A flat float32 buffer of at least `size` elements on the device of `like`: a new one, or the caller's, checked."""
    if out is None:
        return torch.empty(size, dtype=torch.float32, device=like.device)
    _chk(out)
    if out.dim() != 1 or not out.is_contiguous() or out.numel() < size or out.device != like.device:
        raise _lib.SepkernError("%s: out must be a contiguous 1-D float32 tensor of at least %d samples on the samples' device" % (who, size))
    return out


def _row_layout(who, ns, pk):
    """Where the frames of signals of ns samples go as rows -> (Ts, rows, rows_p, bases).  With pk, the batch's Packing: its packed
    rows (bases None) -- it has no perm and its frame counts are the signals'; without: utterance u's T_u = 1 + ns[u] // 128 rows
    start at bases[u] = sum_{v<u} T_v."""
    Ts = [1 + n // 128 for n in ns]
    if pk is None:
        bases, rows = prefix_sums(Ts)
        return Ts, rows, rows, bases
    if pk.perm is not None:
        raise _lib.SepkernError("%s needs a length-sorted batch (Packing without perm)" % who)
    if pk.B != len(ns) or [int(t) for t in pk.lens_host] != Ts:
        raise _lib.SepkernError("%s: the Packing's frame counts are not those of the signals" % who)
    return Ts, pk.R, pk.Rp, None


# ----------------------------------------------------------------------------- STFT / iSTFT
def stft_batch(wavs, want_complex=False, layout="TF", out=None, out_offs=None, stride_t=None, stride_f=None, lengths=None, repeat=1):
    """STFT (n_fft 512, hop 128, reflect-centred, periodic Hann) of a list of 1-D waveforms.

    wavs: list of 1-D CUDA tensors, float32 in [-1,1) or int16 PCM (scaled by 1/32768 in-kernel) -- or, with
    `lengths` (samples per utterance), ONE 1-D CUDA tensor holding the utterances back to back (a batch that crossed
    PCIe as one copy).
    layout "TF": returns list of (T_u, 257) tensors; "FT": list of (257, T_u) (the reference's npz layout).
    With `out` given, writes element (t,f) of utterance u at out_offs[u] + t*stride_t[u] + f*stride_f[u].
    repeat (bench.py's aux leg): the launch is enqueued that many times back to back (same result) between the profile's events.
    """
    if lengths is not None:
        cat, dev = wavs, wavs.device
        pcm16 = _samples("stft", cat)
        ns, woffs, total = _lengths("stft", lengths, 257, "waveform longer than n_fft/2 samples")
        if total != cat.numel():
            raise _lib.SepkernError("stft needs lengths that add up to the tensor of samples")
    else:
        dev = wavs[0].device
        pcm16 = wavs[0].dtype == torch.int16
        for w in wavs:
            _chk(w, torch.int16 if pcm16 else torch.float32)
            if w.dim() != 1 or w.numel() <= 256:
                raise _lib.SepkernError("stft needs 1-D waveforms longer than n_fft/2 samples")
        ns = [int(w.numel()) for w in wavs]
        cat, woffs = torch.cat(wavs) if len(wavs) > 1 else wavs[0].contiguous(), prefix_sums(ns)[0]
    Ts = [1 + n // 128 for n in ns]
    F = 257
    ret = None
    if out is None:
        odt = torch.complex64 if want_complex else torch.float32
        out_offs, size = prefix_sums([T * F for T in Ts])
        out = torch.empty(size, dtype=odt, device=dev)
        stride_t = [F if layout == "TF" else 1 for T in Ts]
        stride_f = [1 if layout == "TF" else T for T in Ts]
        ret = [out[o:o + T * F].view((T, F) if layout == "TF" else (F, T)) for o, T in zip(out_offs, Ts)]
    d_woffs, d_ns = _i64(woffs, dev), _i32(ns, dev)
    d_ooffs, d_st, d_sf = _i64(out_offs, dev), _i64(stride_t, dev), _i64(stride_f, dev)
    frame_major = all(int(v) == 1 for v in stride_f)
    # algorithmic bytes: 128 new samples in, 257 bins out per frame
    with _timed("stft_kernel", repeat * float(sum(Ts)) * (128 * (2 if pcm16 else 4) + 257 * (8 if want_complex else 4))):
        for _ in range(repeat):
            _lib.call("sk_stft", _ptr(cat), int(pcm16), _ptr(d_woffs), _ptr(d_ns), len(ns), 512, 128, int(want_complex),
                      _ptr(out), _ptr(d_ooffs), _ptr(d_st), _ptr(d_sf), int(frame_major), max(Ts), _stream())
    return ret if ret is not None else out


def resample_into(src, in_offs, n_in, out, out_offs, n_out, sr_in, sr_out, repeat=1):
    """sk_resample on signals described by offsets: signal u = n_in[u] samples at src[in_offs[u]] (1-D CUDA tensor, float32 or
    int16 PCM scaled by 1/32768 in-kernel) at sr_in Hz -> its n_out[u] float32 samples at sr_out Hz at out[out_offs[u]]
    (sepkern/resample.py defines the arithmetic and holds the tap table).  Nothing else of `out` is written.  Any number of
    signals: the kernel takes 65535 per launch, more go in as many launches."""
    from . import resample as rs
    pcm16 = _samples("resample_into", src)
    _samples("resample_into", out, "output samples", pcm=False)
    n_in, n_out = _lengths("resample_into", n_in, 0)[0], _lengths("resample_into", n_out, 0)[0]
    nsig = len(n_in)
    if len(n_out) != nsig:
        raise _lib.SepkernError("resample_into: one length per signal, in and out")
    in_offs, = _offsets("resample_into", in_offs, n_in, src.numel())
    out_offs, = _offsets("resample_into", out_offs, n_out, out.numel())
    if max(n_out) == 0:
        return out
    pl = rs.plan(sr_in, sr_out)
    taps = pl.device_taps(src.device)
    d_offs, d_ns = _i64(in_offs + out_offs, src.device), _i32(n_in + n_out, src.device)
    # algorithmic bytes: every input sample once, every output sample once
    with _timed("resample_kernel", repeat * float(sum(n_in) * (2 if pcm16 else 4) + sum(n_out) * 4)):
        for _ in range(repeat):
            for a in range(0, nsig, 65535):          # sk_resample takes at most 65535 signals (the grid's y): one launch per chunk
                b = min(nsig, a + 65535)
                _lib.call("sk_resample", _ptr(src), int(pcm16), _ptr(d_offs[a:b]), _ptr(d_ns[a:b]), b - a, _ptr(taps), pl.L, pl.M,
                          pl.ntaps, _ptr(out), _ptr(d_offs[nsig + a:nsig + b]), _ptr(d_ns[nsig + a:nsig + b]), max(n_out[a:b]),
                          _stream())
    return out


def resample_batch(flat, lengths, sr_in, sr_out, repeat=1):
    """Resample a ragged batch: flat = ONE 1-D CUDA tensor holding the signals back to back (float32, or int16 PCM), lengths =
    samples per signal, all at sr_in Hz -> (out_flat float32: the signals at sr_out Hz back to back, out_lengths);
    out_lengths[u] = ceil(lengths[u] sr_out / sr_in).  Enqueued on the current stream."""
    from . import resample as rs
    _samples("resample_batch", flat)
    ns, in_offs, total = _lengths("resample_batch", lengths, 0)
    if total != flat.numel():
        raise _lib.SepkernError("resample_batch needs lengths that add up to the tensor of samples")
    outs = [rs.out_len(n, sr_in, sr_out) for n in ns]
    out_offs, size = prefix_sums(outs)
    out = _out("resample_batch", None, size, flat)
    resample_into(flat, in_offs, ns, out, out_offs, outs, sr_in, sr_out, repeat=repeat)
    return out, outs


def pcm_to_rate(flat, lengths, rates, target):
    """A batch of int16 PCM signals recorded at DIFFERENT rates -> float32 at `target` Hz: flat = the signals back to back on
    the device, lengths / rates per signal.  Signals are resampled grouped by rate (one sk_resample launch per rate); a signal
    already at `target` is only scaled by 1/32768 (exact: what sk_stft's pcm16 path does to it).
    Returns (out_flat float32, out_lengths)."""
    from . import resample as rs
    if not _samples("pcm_to_rate", flat):
        raise _lib.SepkernError("pcm_to_rate takes int16 PCM (got %s)" % flat.dtype)
    (ns, in_offs, total), rates, target = _lengths("pcm_to_rate", lengths, 0), [int(r) for r in rates], int(target)
    if total != flat.numel() or len(rates) != len(ns):
        raise _lib.SepkernError("pcm_to_rate needs lengths that add up to the tensor of samples and one rate per signal")
    outs = [rs.out_len(n, r, target) if r != target else n for n, r in zip(ns, rates)]
    out_offs, size = prefix_sums(outs)
    out = _out("pcm_to_rate", None, size, flat)
    for r in sorted(set(rates)):
        idx = [u for u, ru in enumerate(rates) if ru == r]
        if r != target:
            resample_into(flat, [in_offs[u] for u in idx], [ns[u] for u in idx], out, [out_offs[u] for u in idx],
                          [outs[u] for u in idx], r, target)
            continue
        k = 0
        while k < len(idx):                  # runs of neighbouring signals are converted in one go
            e = k
            while e + 1 < len(idx) and idx[e + 1] == idx[e] + 1:
                e += 1
            n = sum(ns[u] for u in idx[k:e + 1])
            a, b = in_offs[idx[k]], out_offs[idx[k]]
            torch.mul(flat[a:a + n], 1.0 / 32768.0, out=out[b:b + n])
            k = e + 1
    return out, outs


# ----------------------------------------------------------------------------- dynamic mixing
def dynamic_mix(flat, src_offs, nsamp, amp, peak, quantize=False, out=None, repeat=1):
    """Training mixtures made on the device from single-speaker signals in one launch (sk_dynamic_mix; sepkern/mixing.py defines
    the arithmetic).  flat: ONE 1-D CUDA tensor of samples, float32 or int16 PCM (scaled by 1/32768 in-kernel); src_offs: S lists
    (source 1 .. S) of B offsets into flat -- mixture u's source s is the nsamp[u] samples at src_offs[s][u], and signals may
    overlap; amp: S lists of B linear amplitudes; peak: B target peaks.
    -> (out_flat, gains): out_flat float32 in WavCollator's layout -- key-major ('mix', 'source1', ...), the utterances of every
    key back to back in the order given, (S + 1) sum(nsamp) samples -- and gains (S, B), the final gain of every source.
    quantize: every output sample lands on the int16 grid (clip(rint(32768 v)) / 32768).  out: a float32 buffer of that size to
    write into."""
    pcm16 = _samples("dynamic_mix", flat)
    ns, starts, total = _lengths("dynamic_mix", nsamp, 1, "mixture")
    B, dev = len(ns), flat.device
    offs, S = _offsets("dynamic_mix", src_offs, ns, flat.numel(), (1, 4, "source"))
    amp = [[float(a) for a in row] for row in amp]
    peak = [float(p) for p in peak]
    if len(amp) != S or any(len(row) != B for row in amp) or len(peak) != B:
        raise _lib.SepkernError("dynamic_mix needs one amplitude per source signal (%d x %d) and one peak per mixture" % (S, B))
    out = _out("dynamic_mix", out, (S + 1) * total, flat)
    d64, d_ns = _i64(offs + [q * total + st for q in range(S + 1) for st in starts], dev), _i32(ns, dev)
    d_f = torch.tensor([a for row in amp for a in row] + peak, dtype=torch.float32, device=dev)
    gains = torch.empty(S, B, dtype=torch.float32, device=dev)
    # algorithmic bytes: every input sample once, every output sample once
    with _timed("dynamic_mix_kernel", repeat * float(total) * (S * (2 if pcm16 else 4) + (S + 1) * 4)):
        for _ in range(repeat):
            _lib.call("sk_dynamic_mix", _ptr(flat), int(pcm16), _ptr(d64), _ptr(d_ns), B, S, _ptr(d_f), _ptr(d_f[S * B:]),
                      int(bool(quantize)), _ptr(out), _ptr(d64[S * B:]), _ptr(gains), _stream())
    return out[:(S + 1) * total], gains


# ----------------------------------------------------------------------------- room impulse responses
def fir_convolve(flat, in_offs, ns, rir_flat, rir_offs, taps, delay, repeat=1):
    """Signals convolved with room impulse responses in one call (sk_fir_convolve; sepkern/reverb.py defines the result).  flat:
    ONE 1-D CUDA tensor of samples, float32 or int16 PCM (scaled by 1/32768 in-kernel); job j: the ns[j] samples at in_offs[j]
    with the taps[j] float32 taps at rir_offs[j] of rir_flat (1-D CUDA float32), at delay[j] in [0, taps[j]) -- jobs may share a
    signal or a RIR.  -> (out, offsets): out float32, the jobs' ns[j] output samples back to back, job j's at offsets[j]."""
    pcm16 = _samples("fir_convolve", flat)
    _samples("fir_convolve", rir_flat, "RIR taps", pcm=False)
    ns, out_offs, at = _lengths("fir_convolve", ns, 1, "job")
    taps, delay = _lengths("fir_convolve", taps, 1, "RIR")[0], [int(d) for d in delay]
    J = len(ns)
    if not len(taps) == len(delay) == J:
        raise _lib.SepkernError("fir_convolve: one offset, length, RIR offset, tap count and delay per job")
    in_offs, = _offsets("fir_convolve", in_offs, ns, flat.numel())
    rir_offs, = _offsets("fir_convolve", rir_offs, taps, rir_flat.numel())
    h_in, h_rir, h_out = (C.c_int64 * J)(*in_offs), (C.c_int64 * J)(*rir_offs), (C.c_int64 * J)(*out_offs)
    h_ns, h_taps, h_delay = (C.c_int32 * J)(*ns), (C.c_int32 * J)(*taps), (C.c_int32 * J)(*delay)
    nbytes = _lib.load().sk_fir_workspace_bytes(h_ns, h_taps, h_delay, J)
    if nbytes == 0:
        raise _lib.SepkernError("fir_convolve: 1..65535 jobs of 1..8192 taps, 0 <= delay < taps and 1..2^30 samples (sk_fir_workspace_bytes refused the jobs)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=flat.device)
    out = _out("fir_convolve", None, at, flat)
    # 5 N log2 N per 512-point transform (N = 512) and 8 flops per bin and partition product
    nb = [(d + n - 1) // 256 - d // 256 + 1 for n, d in zip(ns, delay)]
    kk = [-(-t // 256) for t in taps]
    flops = sum(5.0 * 512 * 9 * (k + 2 * b) + 8.0 * 257 * k * b for k, b in zip(kk, nb))
    with _timed("fir_convolve", repeat * flops):
        for _ in range(repeat):
            _lib.call("sk_fir_convolve", _ptr(flat), int(pcm16), h_in, h_ns, _ptr(rir_flat), h_rir, h_taps, h_delay, J, _ptr(ws),
                      _ptr(out), h_out, _stream())
    return out, out_offs


# ----------------------------------------------------------------------------- simulated rooms
def room_rirs(rooms, betas, srcs, mics, ntaps, rate, scales=None, device=None, repeat=1):
    """Image-method room impulse responses made on the device in one launch (sk_room_rirs; sepkern/room.py defines the result).
    Job j: the room rooms[j] = (Lx, Ly, Lz), the reflection coefficients betas[j] (six), a source srcs[j] and a microphone
    mics[j] (three numbers each, metres), ntaps[j] taps at `rate` Hz, every image's amplitude times scales[j] (default 1).
    The geometry is HOST data (numpy float64).  -> (rirs, offsets): float32 on `device` (default: the current one), the jobs'
    taps back to back, job j's at offsets[j]."""
    import numpy as np
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise _lib.SepkernError("room_rirs makes its impulse responses on a CUDA(HIP) device (there is no CPU path)")
    ntaps = [int(t) for t in ntaps]
    J = len(ntaps)
    h_room, h_beta, h_src, h_mic = (np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(J, -1) if J else np.zeros((0, w)))
                                    for a, w in ((rooms, 3), (betas, 6), (srcs, 3), (mics, 3)))
    h_scale = np.ones(J, dtype=np.float64) if scales is None else np.ascontiguousarray(np.asarray(scales, dtype=np.float64).reshape(-1))
    if J == 0 or h_room.shape != (J, 3) or h_beta.shape != (J, 6) or h_src.shape != (J, 3) or h_mic.shape != (J, 3) or h_scale.shape != (J,):
        raise _lib.SepkernError("room_rirs: per job a room (3), reflection coefficients (6), a source (3), a microphone (3), a tap count and a scale")
    offs, at = [], 0
    for t in ntaps:
        offs.append(at)
        at += max(t, 0)
    h_taps, h_offs = (C.c_int32 * J)(*ntaps), (C.c_int64 * J)(*offs)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    nbytes = _lib.load().sk_room_workspace_bytes(hp(h_room), hp(h_beta), hp(h_src), hp(h_mic), hp(h_scale), h_taps, h_offs, J, float(rate))
    if nbytes == 0:
        raise _lib.SepkernError("room_rirs: 1..65535 jobs of 1..8192 taps at rate >= 1, rooms with positive dimensions, reflection "
                                "coefficients in [0, 1], sources and microphones strictly inside their room and at least 0.01 m apart "
                                "(sk_room_workspace_bytes refused the jobs)")
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty(at, dtype=torch.float32, device=dev)
        with _timed("room_rirs_kernel"):
            for _ in range(repeat):
                _lib.call("sk_room_rirs", hp(h_room), hp(h_beta), hp(h_src), hp(h_mic), hp(h_scale), h_taps, h_offs, J, float(rate), _ptr(ws),
                          _ptr(out), _stream())
    return out, offs


def mix_channels(flat, chan_offs, nsamp, gains, quantize=False, out=None, repeat=1):
    """The other channels of array mixtures at the gains dynamic_mix returned for the reference channel (sk_mix_channels;
    sepkern/mixing.py mix_channels states the rule).  flat: ONE 1-D CUDA float32 tensor; chan_offs[s][p][u]: the offset of source
    s on channel p of mixture u (nsamp[u] samples); gains: dynamic_mix's (S, B) tensor.
    -> out_flat float32, channel-major, the utterances of every channel back to back in the order given: P sum(nsamp) samples.
    Levels and the peak are defined on the reference channel: another channel may exceed the peak.  out: a float32 buffer of
    that size to write into."""
    _samples("mix_channels", flat, pcm=False)
    _chk(gains)
    ns, starts, total = _lengths("mix_channels", nsamp, 1, "mixture")
    B, dev = len(ns), flat.device
    offs, S, P = _offsets("mix_channels", chan_offs, ns, flat.numel(), (1, 4, "source"), (1, 7, "channel"))          # [S][P][B]
    if tuple(gains.shape) != (S, B) or not gains.is_contiguous() or gains.device != dev:
        raise _lib.SepkernError("mix_channels: gains is dynamic_mix's contiguous (S, B) = (%d, %d) tensor on the samples' device" % (S, B))
    out = _out("mix_channels", out, P * total, flat)
    d64, d_ns = _i64(offs + [p * total + st for p in range(P) for st in starts], dev), _i32(ns, dev)
    with _timed("mix_channels_kernel", repeat * float(total) * P * (S + 1) * 4):
        for _ in range(repeat):
            _lib.call("sk_mix_channels", _ptr(flat), _ptr(d64), _ptr(d_ns), B, S, P, _ptr(gains), int(bool(quantize)), _ptr(out),
                      _ptr(d64[S * P * B:]), _stream())
    return out[:P * total]


# ----------------------------------------------------------------------------- noisy dynamic mixing
def noise_factors(mics, rate, device=None, repeat=1):
    """The Cholesky factors of a diffuse field's coherence at B arrays (sk_noise_factors; sepkern/noise.py factors defines the
    result).  mics: HOST data (numpy float64) of shape (B, C, 3), metres, 2 <= C <= 8.  -> L float32 (B, 257, C (C + 1) / 2) on
    `device` (default: the current one), entry i (i + 1) / 2 + j = L_k[i, j], j <= i: what diffuse_noise takes."""
    import numpy as np
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise _lib.SepkernError("noise_factors makes its factors on a CUDA(HIP) device (there is no CPU path)")
    h = np.ascontiguousarray(np.asarray(mics, dtype=np.float64))
    if h.ndim != 3 or h.shape[2] != 3 or h.shape[0] < 1 or not 2 <= h.shape[1] <= 8:
        raise _lib.SepkernError("noise_factors: microphones (B, C, 3) with B >= 1 and 2 <= C <= 8 expected (got shape %s)" % (h.shape,))
    B, Cm = h.shape[:2]
    with torch.cuda.device(dev):
        L = torch.empty(B, 257, Cm * (Cm + 1) // 2, dtype=torch.float32, device=dev)
        with _timed("noise_factors_kernel"):
            for _ in range(repeat):
                _lib.call("sk_noise_factors", h.ctypes.data_as(C.c_void_p), B, Cm, float(rate), _ptr(L), _stream())
    return L


def diffuse_noise(flat, chan_offs, nsamp, L, out=None, repeat=1):
    """A diffuse noise field from C independent noise signals per mixture in one launch (sk_diffuse_noise; sepkern/noise.py
    diffuse defines the result).  flat: ONE 1-D CUDA tensor of samples, float32 or int16 PCM; chan_offs[c][u]: the offset of
    mixture u's signal c (nsamp[u] samples); L: noise_factors' (B, 257, C (C + 1) / 2) tensor.
    -> out_flat float32, channel-major, the mixtures of every channel back to back in the order given: C sum(nsamp) samples.
    out: a float32 buffer of that size to write into."""
    pcm16 = _samples("diffuse_noise", flat)
    _chk(L)
    ns, starts, total = _lengths("diffuse_noise", nsamp, 1, "mixture")
    B, dev = len(ns), flat.device
    offs, Cn = _offsets("diffuse_noise", chan_offs, ns, flat.numel(), (2, 8, "channel"))
    if tuple(L.shape) != (B, 257, Cn * (Cn + 1) // 2) or not L.is_contiguous() or L.device != dev:
        raise _lib.SepkernError("diffuse_noise: L is noise_factors' contiguous (B, 257, C (C + 1) / 2) = (%d, 257, %d) tensor on the samples' device"
                                % (B, Cn * (Cn + 1) // 2))
    out = _out("diffuse_noise", out, Cn * total, flat)
    d64, d_ns = _i64(offs + [c * total + st for c in range(Cn) for st in starts], dev), _i32(ns, dev)
    # 5 N log2 N per 512-point transform, 2 C per frame, and 4 flops per bin and factor entry
    frames = sum(-(-n // 128) + 3 for n in ns)
    with _timed("diffuse_noise_kernel", repeat * frames * (5.0 * 512 * 9 * 2 * Cn + 4.0 * 257 * Cn * (Cn + 1) / 2)):
        for _ in range(repeat):
            _lib.call("sk_diffuse_noise", _ptr(flat), int(pcm16), _ptr(d64), _ptr(d_ns), B, Cn, max(ns), _ptr(L), _ptr(out),
                      _ptr(d64[Cn * B:]), _stream())
    return out[:Cn * total]


def add_noise(sig, sig_offs, noise, noise_offs, nsamp, amp, quantize=False, repeat=1):
    """Noise added IN PLACE to the channels of B mixtures at the given amplitudes in one launch (sk_add_noise; sepkern/noise.py
    add_noise states the rule).  sig: ONE 1-D CUDA float32 tensor, sig_offs[c][u] the offset of channel c of mixture u (nsamp[u]
    samples), the reference channel first; noise / noise_offs: the same for the noise, float32 or int16 PCM; amp: B linear
    amplitudes, 10^(-snr / 20).  -> the B gains a (float32 tensor): a = amp sqrt(P_mix / P_noise) on the reference channel."""
    _samples("add_noise", sig, "signals", pcm=False)
    pcm16 = _samples("add_noise", noise, "noise")
    if noise.device != sig.device:
        raise _lib.SepkernError("add_noise needs the signals and the noise on one device")
    ns, _, total = _lengths("add_noise", nsamp, 1, "mixture")
    B, dev = len(ns), sig.device
    so, Cn = _offsets("add_noise", sig_offs, ns, sig.numel(), (1, 8, "channel"))
    no, Cv = _offsets("add_noise", noise_offs, ns, noise.numel(), (1, 8, "noise channel"))
    amp = [float(a) for a in amp]
    if Cv != Cn or len(amp) != B:
        raise _lib.SepkernError("add_noise needs one noise signal per channel (%d, got %d) and one amplitude per mixture" % (Cn, Cv))
    d64, d_ns = _i64(so + no, dev), _i32(ns, dev)
    d_amp = torch.tensor(amp, dtype=torch.float32, device=dev)
    gains = torch.empty(B, dtype=torch.float32, device=dev)
    with _timed("add_noise_kernel", repeat * float(total) * (8 + (2 if pcm16 else 4) + Cn * (8 + (2 if pcm16 else 4)))):
        for _ in range(repeat):
            _lib.call("sk_add_noise", _ptr(sig), _ptr(d64), _ptr(noise), int(pcm16), _ptr(d64[Cn * B:]), _ptr(d_ns), B, Cn, _ptr(d_amp),
                      int(bool(quantize)), _ptr(gains), _stream())
    return gains


def mask_istft_flat(mixcat, maskcat, Ts, S, want_pcm=True, want_float=True, repeat=1):
    """Mask-apply + iSTFT on buffers that crossed PCIe as ONE copy each: mixcat = the utterances' (257, T_u) complex64
    spectra back to back (flattened), maskcat = None or, per utterance and source (utterance-major), the (257, T_u) float32
    masks back to back.  Returns (wav float32 flat or None, pcm int16 flat or None, offsets): source s of utterance u is
    the 128 (T_u - 1) samples at offsets[u * S + s]."""
    dev = mixcat.device
    nutt, F = len(Ts), 257
    _chk(mixcat, torch.complex64)
    _chk(maskcat)
    if mixcat.numel() != F * sum(Ts) or (maskcat is not None and maskcat.numel() != F * S * sum(Ts)):
        raise _lib.SepkernError("mask_istft: buffer sizes do not match the frame counts")
    moffs, koffs, ooffs, am, ak, ao = [], [], [], 0, 0, 0
    for T in Ts:
        moffs.append(am)
        am += T * F
        for s in range(S):
            koffs.append(ak)
            ak += T * F
            ooffs.append(ao)
            ao += 128 * (T - 1)
    wav = torch.empty(ao, dtype=torch.float32, device=dev) if want_float else None
    pcm = torch.empty(ao, dtype=torch.int16, device=dev) if want_pcm else None
    d_moffs, d_mst, d_msf = _i64(moffs, dev), _i64([1] * nutt, dev), _i64(list(Ts), dev)
    d_koffs = d_kst = d_ksf = None
    if maskcat is not None:
        d_koffs, d_kst, d_ksf = _i64(koffs, dev), d_mst, d_msf
    d_T, d_ooffs = torch.tensor(list(Ts), dtype=torch.int32, device=dev), _i64(ooffs, dev)
    # algorithmic bytes per frame and source: the complex spectrum (read once per source), the mask, 128 samples out
    per = 257 * 8 + (257 * 4 if maskcat is not None else 0) + 128 * ((2 if want_pcm else 0) + (4 if want_float else 0))
    with _timed("istft_kernel", repeat * float(sum(Ts)) * S * per):
        for _ in range(repeat):
            _lib.call("sk_mask_istft", _ptr(mixcat), _ptr(d_moffs), _ptr(d_mst), _ptr(d_msf),
                      _ptr(maskcat), _ptr(d_koffs), _ptr(d_kst), _ptr(d_ksf),
                      _ptr(d_T), nutt, S, 512, 128, _ptr(wav), _ptr(pcm), _ptr(d_ooffs), max(Ts), _stream())
    return wav, pcm, ooffs


def mask_istft(mix_specs, masks=None, want_pcm=True, want_float=True, repeat=1):
    """Mask-apply + iSTFT.  mix_specs: list of (257, T_u) complex64 CUDA tensors (the reference's
    feats_test layout); masks: None or list (per utterance) of lists (per source) of (257, T_u) float32.
    Returns (list of lists of float32 waveforms or None, list of lists of int16 waveforms or None)."""
    nutt = len(mix_specs)
    S = len(masks[0]) if masks is not None else 1
    Ts = [int(m.shape[1]) for m in mix_specs]
    for m in mix_specs:
        _chk(m, torch.complex64)
        if m.shape[0] != 257:
            raise _lib.SepkernError("mask_istft expects (257, T) spectra")
    mixcat = torch.cat([m.contiguous().view(-1) for m in mix_specs])
    maskcat = None
    if masks is not None:
        for u in range(nutt):
            for s in range(S):
                _chk(masks[u][s])
        maskcat = torch.cat([masks[u][s].contiguous().view(-1) for u in range(nutt) for s in range(S)])
    wav, pcm, ooffs = mask_istft_flat(mixcat, maskcat, Ts, S, want_pcm, want_float, repeat=repeat)

    def split(buf):
        if buf is None:
            return None
        return [[buf[ooffs[u * S + s]:ooffs[u * S + s] + 128 * (Ts[u] - 1)] for s in range(S)] for u in range(nutt)]
    return split(wav), split(pcm)


def mask_istft_frames(mixc, mask, S, want_pcm=True, want_float=True, repeat=1):
    """Mask-apply + iSTFT of ONE recording held frame-major: mixc (T, 257) complex64 (sk_stft's rows), mask (T, ld >= S*257)
    float32 with source s in columns s*257 .. (unit column stride; None = all ones, S = 1) -- sk_mask_istft with row strides,
    nothing is transposed.  Returns (wav (S, 128 (T - 1)) float32 or None, pcm likewise int16 or None)."""
    _chk(mixc, torch.complex64)
    _chk(mask)
    T = int(mixc.shape[0])
    if mixc.dim() != 2 or mixc.shape[1] != 257 or not mixc.is_contiguous() or T < 2:
        raise _lib.SepkernError("mask_istft_frames: mixc must be (T >= 2, 257) contiguous complex64")
    if mask is not None and (mask.dim() != 2 or mask.stride(1) != 1 or mask.shape[0] < T or mask.shape[1] < S * 257):
        raise _lib.SepkernError("mask_istft_frames: mask must be (>= T, >= S*257) with unit column stride")
    dev, L = mixc.device, 128 * (T - 1)
    wav = torch.empty(S, L, dtype=torch.float32, device=dev) if want_float else None
    pcm = torch.empty(S, L, dtype=torch.int16, device=dev) if want_pcm else None
    ld = int(mask.stride(0)) if mask is not None else 0
    # [mix_offs | mix_st | mix_sf | mask_st | mask_sf | mask_offs (S) | out_offs (S)]; they must outlive the (asynchronous) launch call
    d = _i64([0, 257, 1, ld, 1] + [s * 257 for s in range(S)] + [s * L for s in range(S)], dev)
    d_T = torch.tensor([T], dtype=torch.int32, device=dev)
    per = 257 * 8 + (257 * 4 if mask is not None else 0) + 128 * ((2 if want_pcm else 0) + (4 if want_float else 0))
    with _timed("istft_kernel", repeat * float(T) * S * per):
        for _ in range(repeat):
            _lib.call("sk_mask_istft", _ptr(mixc), _ptr(d[0:1]), _ptr(d[1:2]), _ptr(d[2:3]),
                      _ptr(mask), _ptr(d[5:5 + S]) if mask is not None else None, _ptr(d[3:4]) if mask is not None else None,
                      _ptr(d[4:5]) if mask is not None else None, _ptr(d_T), 1, S, 512, 128, _ptr(wav), _ptr(pcm),
                      _ptr(d[5 + S:]), T, _stream())
    return wav, pcm


# ----------------------------------------------------------------------------- stitching windowed masks
def stitch(mag, windows, T, W, Hn, S, ramp, out=None, ws=None, repeat=1):
    """The masks of the overlapping windows of one recording aligned and cross-faded (sk_stitch; sepkern/stitch.py defines the
    result).  mag: (>= T, ld >= 257) float32 magnitude rows of the whole recording with unit column stride; windows: one
    (tensor, element offset, row stride) per window -- element (t, c) of window k is tensor.view(-1)[offset + t * stride + c];
    the tensors may be different allocations (the outputs of different batches: they stay where the network wrote them; the
    caller keeps them alive until the launches have run); ramp: (W - Hn) float32, the weight of the later window.
    out: a (>= T, >= S*257) float32 buffer with unit column stride to write into (rows < T, columns < S*257 only).
    ws: a uint8 workspace of the caller's instead of the cached one.
    -> (out (T, .), perms (K, S) int32, cost (K - 1, S, S) float64); nothing synchronises with the host."""
    lib = _lib.load()
    T, W, Hn, S = int(T), int(W), int(Hn), int(S)
    nbytes = lib.sk_stitch_workspace_bytes(T, W, Hn, S)
    K = 1 + -(-max(T - W, 0) // Hn) if Hn > 0 else 1
    if nbytes and len(windows) != K:
        raise _lib.SepkernError("stitch: %d windows given, T = %d, W = %d, Hn = %d make %d" % (len(windows), T, W, Hn, K))
    _chk(mag)
    _chk(ramp)
    if nbytes and K > 1 and (mag.dim() != 2 or mag.stride(1) != 1 or mag.shape[0] < T or mag.shape[1] < 257 or ramp.numel() != W - Hn
                             or not ramp.is_contiguous()):
        raise _lib.SepkernError("stitch: mag must be (>= T, >= 257) with unit column stride, ramp W - Hn contiguous floats")
    base = windows[0][0]
    dev = base.device
    offs = []
    for t, off, _ in windows:
        _chk(t)
        delta = t.data_ptr() - base.data_ptr()          # in bytes; float32 storage: a multiple of 4
        offs.append(delta // 4 + int(off))
    if out is None:
        out = torch.empty(max(T, 1), S * 257, dtype=torch.float32, device=dev)
    _chk(out)
    if out.dim() != 2 or out.stride(1) != 1 or out.shape[0] < T or out.shape[1] < S * 257:
        raise _lib.SepkernError("stitch: out must be (>= T, >= S*257) float32 with unit column stride")
    if ws is None:
        ws = workspace(nbytes, "stitch")
    elif nbytes and (ws.dtype != torch.uint8 or ws.numel() < nbytes):
        raise _lib.SepkernError("stitch: workspace of %d bytes, %d expected" % (ws.numel(), nbytes))
    perms = torch.empty(max(K, 1), max(S, 1), dtype=torch.int32, device=dev)
    cost = torch.empty(max(K - 1, 0), max(S, 1), max(S, 1), dtype=torch.float64, device=dev)
    # descriptor arrays must outlive the (asynchronous) launch call: keep references until it returns
    d = _i64(offs + [int(st) for _, _, st in windows], dev)
    # algorithmic bytes: the cost launch reads both windows' O overlap frames and the mixture's; the blend launch reads every
    # window element once and writes every output element once
    ov = max(K - 1, 0) * max(W - Hn, 0)
    with _timed("stitch", repeat * 4.0 * 257 * (ov * (2 * S + 1) + (T + ov) * S + T * S)):
        for _ in range(repeat):
            _lib.call("sk_stitch", _ptr(mag), int(mag.stride(0)) if mag is not None and mag.dim() == 2 else 0, _ptr(base), _ptr(d[:len(windows)]),
                      _ptr(d[len(windows):]), T, W, Hn, S, _ptr(ramp), _ptr(out), int(out.stride(0)), _ptr(perms), _ptr(cost),
                      _ptr(ws), _stream())
    return out[:T], perms, cost


# ----------------------------------------------------------------------------- the array kernels' shared argument checks
def _array_spectra(who, Y):
    """Y of mvdr, wpe, wpd and cacgmm: (C, T, >= 257) complex64, read where it lies -> (C, T)."""
    _chk(Y, torch.complex64)
    if Y.dim() != 3 or Y.shape[2] < 257 or Y.stride(2) != 1:
        raise _lib.SepkernError("%s: Y must be (C, T, >= 257) complex64 with unit bin stride" % who)
    return int(Y.shape[0]), int(Y.shape[1])


def _stream_columns(who, name, m, T, S):
    """A mask, prior or output of T frames with stream s in columns s*257 .. of a row."""
    _chk(m)
    if m.dim() != 2 or m.stride(1) != 1 or m.shape[0] < T or m.shape[1] < S * 257:
        raise _lib.SepkernError("%s: %s must be (>= T, >= S*257) float32 with unit column stride" % (who, name))


def _num_blocks(T, Lb):
    """Blocks of Lb frames; 1 where Lb is one the call itself will refuse, so that the buffers can still be sized."""
    return _wpe.num_blocks(T, Lb) if Lb > 0 else 1


# ----------------------------------------------------------------------------- mask-based MVDR beamforming
def mvdr(Y, mask, S, block_frames, context_blocks, ref, loading, want_scm=False, weights=None, Z=None, ws=None, repeat=1):
    """One MVDR beamformer per stream and block of frames, steered by the masks (sk_mvdr; sepkern/mvdr.py defines the result).
    Y: (C, T, >= 257) complex64 spectra with unit bin stride (any channel and row stride: a view is read where it lies);
    mask: (>= T, >= S*257) float32 with unit column stride, stream s in columns s*257 .. (ops.stitch's output).
    weights / Z: contiguous complex64 buffers of (nblk, S, 257, C) / (S, T, 257) to write into; ws: a uint8 workspace of the
    caller's instead of the cached one.
    -> (weights (nblk, S, 257, C) complex64, Z (S, T, 257) complex64, scm (nblk, S, 257, C, C) complex128 or None); nothing
    synchronises with the host."""
    lib = _lib.load()
    C, T = _array_spectra("mvdr", Y)
    S, Lb, R, ref = int(S), int(block_frames), int(context_blocks), int(ref)
    _stream_columns("mvdr", "mask", mask, T, S)
    nbytes = lib.sk_mvdr_workspace_bytes(T, C, S, Lb)
    nblk = _num_blocks(T, Lb)
    dev = Y.device
    if weights is None:
        weights = torch.empty(nblk, S, 257, C, dtype=torch.complex64, device=dev)
    if Z is None:
        Z = torch.empty(S, T, 257, dtype=torch.complex64, device=dev)
    _chk(weights, torch.complex64)
    _chk(Z, torch.complex64)
    if tuple(weights.shape) != (nblk, S, 257, C) or tuple(Z.shape) != (S, T, 257) or not weights.is_contiguous() or not Z.is_contiguous():
        raise _lib.SepkernError("mvdr: weights must be (nblk, S, 257, C) and Z (S, T, 257), contiguous complex64")
    scm = torch.empty(nblk, S, 257, C, C, dtype=torch.complex128, device=dev) if want_scm else None
    if ws is None:
        ws = workspace(nbytes, "mvdr")
    elif nbytes and (ws.dtype != torch.uint8 or ws.numel() < nbytes):
        raise _lib.SepkernError("mvdr: workspace of %d bytes, %d expected" % (ws.numel(), nbytes))
    # algorithmic bytes: Y and the mask read by the statistics launch, Y read again and Z written by the apply launch, the
    # block statistics written once and read 2 R + 1 times, the weights written and read
    stats = float(nbytes)
    per = float(T) * 257 * (2 * C * 8 + S * 4 + S * 8)
    with _timed("mvdr", repeat * (per + stats * (1 + min(2 * R + 1, nblk)) + 2.0 * nblk * S * 257 * C * 8)):
        for _ in range(repeat):
            _lib.call("sk_mvdr", _ptr(Y), int(Y.stride(0)), int(Y.stride(1)), _ptr(mask), int(mask.stride(0)), T, C, S, Lb, R, ref,
                      float(loading), _ptr(weights), _ptr(Z), _ptr(scm), _ptr(ws), _stream())
    return weights, Z, scm


def mask_istft_streams(Z, mask, S, want_pcm=True, want_float=True, repeat=1):
    """iSTFT of S spectra held frame-major, each with its own column block of one mask: Z (S, T, 257) contiguous complex64
    (ops.mvdr's output), mask None or (>= T, ld >= S*257) float32 with unit column stride, stream s in columns s*257 .. --
    sk_mask_istft over S one-source items, descriptors only.  Returns (wav (S, 128 (T - 1)) float32 or None, pcm likewise
    int16 or None)."""
    _chk(Z, torch.complex64)
    _chk(mask)
    S = int(S)
    if Z.dim() != 3 or Z.shape[0] != S or Z.shape[2] != 257 or not Z.is_contiguous() or Z.shape[1] < 2:
        raise _lib.SepkernError("mask_istft_streams: Z must be (S, T >= 2, 257) contiguous complex64")
    T = int(Z.shape[1])
    if mask is not None and (mask.dim() != 2 or mask.stride(1) != 1 or mask.shape[0] < T or mask.shape[1] < S * 257):
        raise _lib.SepkernError("mask_istft_streams: mask must be (>= T, >= S*257) with unit column stride")
    dev, L = Z.device, 128 * (T - 1)
    wav = torch.empty(S, L, dtype=torch.float32, device=dev) if want_float else None
    pcm = torch.empty(S, L, dtype=torch.int16, device=dev) if want_pcm else None
    ld = int(mask.stride(0)) if mask is not None else 0
    # [mix_offs | mix_st | mix_sf | mask_offs | mask_st | mask_sf | out_offs], S entries each; they must outlive the (asynchronous) launch call
    d = _i64([s * T * 257 for s in range(S)] + [257] * S + [1] * S + [s * 257 for s in range(S)] + [ld] * S + [1] * S
             + [s * L for s in range(S)], dev)
    d_T = torch.tensor([T] * S, dtype=torch.int32, device=dev)
    part = lambda k: _ptr(d[k * S:(k + 1) * S])
    has = mask is not None
    per = 257 * 8 + (257 * 4 if has else 0) + 128 * ((2 if want_pcm else 0) + (4 if want_float else 0))
    with _timed("istft_kernel", repeat * float(T) * S * per):
        for _ in range(repeat):
            _lib.call("sk_mask_istft", _ptr(Z), part(0), part(1), part(2), _ptr(mask), part(3) if has else None,
                      part(4) if has else None, part(5) if has else None, _ptr(d_T), S, 1, 512, 128, _ptr(wav), _ptr(pcm),
                      part(6), T, _stream())
    return wav, pcm


# ----------------------------------------------------------------------------- WPE dereverberation
def wpe(Y, taps, delay, iterations, block_frames, context_frames, loading, ref=0, want_mag=False, want_G=False, X=None, repeat=1):
    """Dereverberation by weighted prediction error, per block of frames and bin (sk_wpe; sepkern/wpe.py defines the result).
    Y: (C, T, >= 257) complex64 spectra with unit bin stride (any channel and row stride: a view is read where it lies), 1 <= C
    <= 8, C * taps <= 80.  X: a complex64 (C, T, >= 257) buffer with unit bin stride to write into (not overlapping Y).
    -> (X (C, T, 257) complex64, mag (T, 257) float32 = |X[ref]| or None, G (nblk, 257, C*taps, C) complex128 or None); nothing
    synchronises with the host."""
    _lib.load()
    C, T = _array_spectra("wpe", Y)
    K, dl, I, Lb, Lc, ref = int(taps), int(delay), int(iterations), int(block_frames), int(context_frames), int(ref)
    dev = Y.device
    if X is None:
        X = torch.empty(C, T, 257, dtype=torch.complex64, device=dev)
    _chk(X, torch.complex64)
    if X.dim() != 3 or tuple(X.shape[:2]) != (C, T) or X.shape[2] < 257 or X.stride(2) != 1:
        raise _lib.SepkernError("wpe: X must be (C, T, >= 257) complex64 with unit bin stride")
    nblk = _num_blocks(T, Lb)
    D = C * K
    mag = torch.empty(T, 257, dtype=torch.float32, device=dev) if want_mag else None
    G = torch.empty(nblk, 257, max(D, 0), C, dtype=torch.complex128, device=dev) if want_G else None
    # algorithmic bytes: every iteration reads its window twice (the weights, then the sums), the block is read once more and X
    # written; the windows overlap by the context
    win = float(min(T, Lb + 2 * max(Lc, 0))) * nblk if Lb > 0 else 0.0
    per = 257.0 * C * 8 * (2 * max(I, 0) * win + 2 * T) + (257.0 * 4 * T if want_mag else 0.0) + (257.0 * nblk * D * C * 16 if want_G else 0.0)
    with _timed("wpe", repeat * per):
        for _ in range(repeat):
            _lib.call("sk_wpe", _ptr(Y), int(Y.stride(0)), int(Y.stride(1)), T, C, K, dl, I, Lb, Lc, ref, float(loading), _ptr(X),
                      int(X.stride(0)), int(X.stride(1)), _ptr(mag), 257, _ptr(G), None, _stream())
    return X[:, :, :257], mag, G


# ----------------------------------------------------------------------------- mask-based WPD convolutional beamforming
def wpd(Y, mask, S, taps, delay, iterations, block_frames, context_frames, loading, floor, ref=0, W_in=None, want_W=False, Z=None,
        repeat=1):
    """One WPD convolutional beamformer per stream, block of frames and bin, steered by the masks (sk_wpd; sepkern/wpd.py
    defines the result).  Y: (C, T, >= 257) complex64 spectra with unit bin stride (any channel and row stride: a view is read
    where it lies), 2 <= C <= 8, C * (taps + 1) <= 80; mask: (>= T, >= S*257) float32 with unit column stride, stream s in
    columns s*257 .. (ops.stitch's or ops.cacgmm's output); W_in: None or the (nblk, S, 257, C*(taps+1)) contiguous complex128
    filters to start from (a W of an earlier call); Z: a contiguous complex64 (S, T, 257) buffer to write into.
    -> (Z (S, T, 257) complex64, W (nblk, S, 257, C*(taps+1)) complex128 or None); nothing synchronises with the host."""
    _lib.load()
    C, T = _array_spectra("wpd", Y)
    S, K, dl, I, Lb, Lc, ref = int(S), int(taps), int(delay), int(iterations), int(block_frames), int(context_frames), int(ref)
    _stream_columns("wpd", "mask", mask, T, S)
    dev = Y.device
    nblk = _num_blocks(T, Lb)
    D = max(C * (K + 1), 0)
    shape_W = (nblk, max(S, 0), 257, D)
    if W_in is not None:
        _chk(W_in, torch.complex128)
        if tuple(W_in.shape) != shape_W or not W_in.is_contiguous():
            raise _lib.SepkernError("wpd: W_in must be (nblk, S, 257, C*(taps+1)) contiguous complex128")
    if Z is None:
        Z = torch.empty(max(S, 0), T, 257, dtype=torch.complex64, device=dev)
    _chk(Z, torch.complex64)
    if tuple(Z.shape) != (S, T, 257) or not Z.is_contiguous():
        raise _lib.SepkernError("wpd: Z must be (S, T, 257) contiguous complex64")
    W = torch.empty(shape_W, dtype=torch.complex128, device=dev) if want_W else None
    # algorithmic bytes: every stream reads its window of Y twice per iteration (the weights, then the sums) and its masks
    # once, the block is read once more and Z written; the windows overlap by the context
    win = float(min(T, Lb + 2 * max(Lc, 0))) * nblk if Lb > 0 else 0.0
    per = 257.0 * S * ((C * 8 * 2 + 4) * max(I, 0) * win + (C * 8 + 8) * T)
    per += 257.0 * nblk * S * D * 16 * ((W_in is not None) + bool(want_W))
    with _timed("wpd", repeat * per):
        for _ in range(repeat):
            _lib.call("sk_wpd", _ptr(Y), int(Y.stride(0)), int(Y.stride(1)), _ptr(mask), int(mask.stride(0)), T, C, S, K, dl, I, Lb,
                      Lc, ref, float(loading), float(floor), _ptr(W_in), _ptr(Z), _ptr(W), None, _stream())
    return Z, W


# ----------------------------------------------------------------------------- mask-guided cACGMM spatial clustering
def cacgmm(Y, prior, S, iterations, block_frames, context_frames, loading, B_in=None, want_B=False, out=None, repeat=1):
    """The masks re-estimated from all channels by a cACGMM whose class prior they are, per block of frames and bin (sk_cacgmm;
    sepkern/cacgmm.py defines the result).  Y: (C, T, >= 257) complex64 spectra with unit bin stride (any channel and row
    stride: a view is read where it lies; ops.wpe's X will do), 2 <= C <= 8; prior: (>= T, >= S*257) float32 with unit column
    stride, stream s in columns s*257 .. (ops.stitch's output); B_in: None or the (nblk, S, 257, C, C) contiguous complex128
    state to start from (a B of an earlier call); out: a float32 (>= T, >= S*257) buffer with unit column stride to write into
    (not overlapping prior).
    -> (mask (T, S*257) float32, B (nblk, S, 257, C, C) complex128 or None); nothing synchronises with the host."""
    _lib.load()
    _chk(prior)
    C, T = _array_spectra("cacgmm", Y)
    S, I, Lb, Lc = int(S), int(iterations), int(block_frames), int(context_frames)
    try:                                    # the kernel's own limits, before anything is sized by them
        _cacgmm.check_arguments(C, S, T, I, Lb, Lc, float(loading), y_row_stride=int(Y.stride(1)))
    except ValueError as e:
        raise _lib.SepkernError(str(e))
    _stream_columns("cacgmm", "prior", prior, T, S)
    dev = Y.device
    nblk = _num_blocks(T, Lb)
    shape_B = (nblk, S, 257, C, C)
    if B_in is not None:
        _chk(B_in, torch.complex128)
        if tuple(B_in.shape) != shape_B or not B_in.is_contiguous():
            raise _lib.SepkernError("cacgmm: B_in must be (nblk, S, 257, C, C) contiguous complex128")
    if out is None:
        out = torch.empty(T, S * 257, dtype=torch.float32, device=dev)
    _stream_columns("cacgmm", "out", out, T, S)
    B = torch.empty(shape_B, dtype=torch.complex128, device=dev) if want_B else None
    # algorithmic bytes: every iteration reads its window of Y and of the prior once, the block is read once more and the
    # masks written; the windows overlap by the context
    win = float(min(T, Lb + 2 * Lc)) * nblk
    per = 257.0 * (C * 8 + S * 4) * (I * win + T) + 257.0 * S * 4 * T
    per += 257.0 * nblk * S * C * C * 16 * ((B_in is not None) + bool(want_B))
    with _timed("cacgmm", repeat * per):
        for _ in range(repeat):
            _lib.call("sk_cacgmm", _ptr(Y), int(Y.stride(0)), int(Y.stride(1)), _ptr(prior), int(prior.stride(0)), T, C, S, I, Lb, Lc,
                      float(loading), _ptr(B_in), _ptr(out), int(out.stride(0)), _ptr(B), None, _stream())
    return out[:T, :S * 257], B


# ----------------------------------------------------------------------------- deep clustering: loss and k-means masks
DPCL_AB = 40 * 40 + 40 * 4          # floats of [A | Bm] per utterance (include/sepkern.h)


def _dpcl_args(who, z, mix, pk, D, S, smin):
    """The checks the three deep-clustering wrappers share -> (F, D, S, ld)."""
    _chk(z)
    _chk(mix)
    D, S = int(D), int(S)
    if pk.perm is not None:
        raise _lib.SepkernError("%s needs a length-sorted batch (Packing without perm)" % who)
    if not 1 <= D <= _dpcl.MAX_D or not smin <= S <= _dpcl.MAX_S:
        raise _lib.SepkernError("%s: D = %d outside 1..%d or S = %d outside %d..%d" % (who, D, _dpcl.MAX_D, S, smin, _dpcl.MAX_S))
    if mix.dim() != 2 or not mix.is_contiguous() or mix.shape[0] < pk.R or mix.shape[1] < 1:
        raise _lib.SepkernError("%s: mix must be (>= R, F) contiguous float32 rows of the batch" % who)
    F = int(mix.shape[1])
    if z.dim() != 2 or z.stride(1) != 1 or z.shape[0] < pk.R or z.shape[1] < F * D:
        raise _lib.SepkernError("%s: z must be (>= R, >= F*D = %d) float32 with unit column stride (got %s)" % (who, F * D, tuple(z.shape)))
    return F, D, S, int(z.stride(0))


def _dpcl_srcs(who, srcs, mix):
    for s in srcs:
        _chk(s)
        if s.dim() != 2 or not s.is_contiguous() or s.shape[0] < mix.shape[0] or s.shape[1] != mix.shape[1]:
            raise _lib.SepkernError("%s: every source must be (>= R, F) contiguous float32 rows like mix" % who)
    return (C.c_void_p * len(srcs))(*[s.data_ptr() for s in srcs])


def _dpcl_weight(who, weight):
    try:
        return _dpcl.WEIGHTS.index(weight)
    except ValueError:
        raise _lib.SepkernError("%s: weight %r is neither 'mr' nor 'vad'" % (who, weight))


def dpcl_fwd(z, mix, srcs, pk, D, weight="mr", vad_db=40.0, count_dev=None, repeat=1):
    """The deep-clustering loss of a packed batch (sk_dpcl_fwd; sepkern/dpcl.py defines it).  z: (>= R, ld >= F*D) float32
    embedding rows with unit column stride, dimension d of bin f in column d*F + f; mix and the S = len(srcs) sources: (>= R, F)
    contiguous float32 magnitude rows of the batch pk; weight 'mr' or 'vad' (active above -vad_db dB of the utterance's maximum);
    count_dev: optional device scalar replacing B (the global utterance count under data parallelism).
    -> dict(out (3,) = [loss, count, sum_j L_j], lj (B,) float64, ab (B, 1760) = A and Bm per utterance, stats (B, 2)): what
    dpcl_bwd takes; nothing synchronises with the host."""
    lib = _lib.load()
    F, D, S, ld = _dpcl_args("dpcl_fwd", z, mix, pk, D, len(srcs), 1)
    sp = _dpcl_srcs("dpcl_fwd", srcs, mix)
    wk = _dpcl_weight("dpcl_fwd", weight)
    ratio = float(_dpcl.vad_ratio(vad_db))
    _chk(count_dev)
    dev = z.device
    lj = torch.empty(pk.B, dtype=torch.float64, device=dev)
    ab = torch.empty(pk.B, DPCL_AB, dtype=torch.float32, device=dev)
    stats = torch.empty(pk.B, 2, dtype=torch.float32, device=dev)
    out = torch.empty(3, dtype=torch.float32, device=dev)
    ws = workspace(lib.sk_dpcl_workspace_bytes(pk.T, pk.B, F, D, S), "dpcl")
    # algorithmic bytes: the embeddings, the mixture (twice with 'vad': the threshold pass) and the S sources, read once
    with _timed("dpcl_fwd", repeat * float(pk.R) * F * 4 * (D + 1 + wk + S)):
        for _ in range(repeat):
            _lib.call("sk_dpcl_fwd", _ptr(z), ld, _ptr(mix), sp, _ptr(pk.lens), _ptr(pk.offs), pk.T, pk.B, F, D, S, wk, ratio,
                      _ptr(count_dev), _ptr(lj), _ptr(ab), _ptr(stats), _ptr(out), _ptr(ws), _stream())
    return dict(out=out, lj=lj, ab=ab, stats=stats)


def dpcl_bwd(z, mix, srcs, pk, D, res, gscale, weight="mr", out=None, repeat=1):
    """dz = gscale[0] / count * d(sum_j L_j) / dz (sk_dpcl_bwd) from dpcl_fwd's result `res` on the same operands.  out: a float32
    buffer of z's shape and strides to write into; only the batch's rows and the columns < F*D are written -- a fresh buffer is
    allocated with everything else zero.  -> dz."""
    _lib.load()
    F, D, S, ld = _dpcl_args("dpcl_bwd", z, mix, pk, D, len(srcs), 1)
    sp = _dpcl_srcs("dpcl_bwd", srcs, mix)
    wk = _dpcl_weight("dpcl_bwd", weight)
    _chk(gscale)
    for t in (res["ab"], res["stats"], res["out"]):
        _chk(t)
    if out is None:
        out = torch.empty_like(z)
        if out.shape[0] > pk.R:
            out[pk.R:].zero_()
        if out.shape[1] > F * D:
            out[:, F * D:].zero_()
    _chk(out)
    if out.shape != z.shape or out.stride() != z.stride():
        raise _lib.SepkernError("dpcl_bwd: out must have z's shape and strides")
    # algorithmic bytes: the forward's operands read once, dz written once
    with _timed("dpcl_bwd", repeat * float(pk.R) * F * 4 * (2 * D + 1 + S)):
        for _ in range(repeat):
            _lib.call("sk_dpcl_bwd", _ptr(z), ld, _ptr(mix), sp, _ptr(pk.lens), _ptr(pk.offs), pk.T, pk.B, F, D, S, wk, _ptr(res["ab"]),
                      _ptr(res["stats"]), _ptr(res["out"]), _ptr(gscale), _ptr(out), _stream())
    return out


def dpcl_kmeans(z, mix, pk, S, iterations=20, vad_db=40.0, centroids_in=None, out=None, D=None, repeat=1):
    """k-means masks from the embeddings of a packed batch (sk_dpcl_kmeans; sepkern/dpcl.py defines the result).  z: (>= R, ld >=
    F*D) float32 embedding rows with unit column stride; mix: (>= R, F) contiguous float32 magnitude rows; D: the embedding
    dimension, default z.shape[1] // F (to be given when z carries padding columns); 2 <= S <= 4 clusters; iterations >= 0 Lloyd steps; points above -vad_db dB of their
    utterance's maximum are active; centroids_in: None (farthest-first initialisation) or (B, S, D) contiguous float32;
    out: a float32 (>= R, >= S*F) buffer with unit column stride to write the masks into (rows of the batch, columns < S*F only).
    -> (mask (rows of out, S*F) of 0.0 / 1.0 in the uPIT mask layout, labels (R, F) int32, centroids (B, S, D) float32); nothing
    synchronises with the host."""
    lib = _lib.load()
    F = int(mix.shape[1]) if mix.dim() == 2 and mix.shape[1] > 0 else 1
    F, D, S, ld = _dpcl_args("dpcl_kmeans", z, mix, pk, int(z.shape[1]) // F if D is None and z.dim() == 2 else D, S, 2)
    iterations = int(iterations)
    if iterations < 0:
        raise _lib.SepkernError("dpcl_kmeans: iterations = %d is negative" % iterations)
    ratio = float(_dpcl.vad_ratio(vad_db))
    dev = z.device
    if centroids_in is not None:
        _chk(centroids_in)
        if tuple(centroids_in.shape) != (pk.B, S, D) or not centroids_in.is_contiguous():
            raise _lib.SepkernError("dpcl_kmeans: centroids_in must be (B, S, D) contiguous float32")
    if out is None:
        out = torch.empty(z.shape[0], S * F, dtype=torch.float32, device=dev)
        if out.shape[0] > pk.R:
            out[pk.R:].zero_()
    _chk(out)
    if out.dim() != 2 or out.stride(1) != 1 or out.shape[0] < pk.R or out.shape[1] < S * F:
        raise _lib.SepkernError("dpcl_kmeans: out must be (>= R, >= S*F) float32 with unit column stride")
    labels = torch.empty(pk.R, F, dtype=torch.int32, device=dev)
    cent = torch.empty(pk.B, S, D, dtype=torch.float32, device=dev)
    ws = workspace(lib.sk_dpcl_kmeans_workspace_bytes(pk.T, pk.B, F, D, S), "dpcl")
    # algorithmic bytes: the embeddings once per initial centroid after the first, per iteration and for the assignment; the
    # mixture beside each pass and for the threshold; the masks and labels written
    passes = (0 if centroids_in is not None else S - 1) + iterations + 1
    with _timed("dpcl_kmeans", repeat * float(pk.R) * F * 4 * (passes * D + passes + 2 + S + 1)):
        for _ in range(repeat):
            _lib.call("sk_dpcl_kmeans", _ptr(z), ld, _ptr(mix), _ptr(pk.lens), _ptr(pk.offs), pk.T, pk.B, F, D, S, iterations, ratio,
                      _ptr(centroids_in), _ptr(out), int(out.stride(0)), _ptr(labels), _ptr(cent), _ptr(ws), _stream())
    return out[:, :S * F], labels, cent


# ----------------------------------------------------------------------------- PIT-MSE
def pit_mse_fwd(mask, mix, srcs, lens, norm_dev=None, packing=None, repeat=1):
    """mask (T,B,S*F), mix (T,B,F), srcs list of S (T,B,F), lens int32 (B), norm_dev: optional device
    scalar replacing sum(lens)*F (the global norm under data parallelism) ->
    dict(out (3,), pair (B,S,S), perm_loss (S!,B), best_perm (B)).
    packing (sepkern.packing.Packing): mask (>= R, S*F), mix and srcs (>= R, F) are PACKED rows (PackedSequence.data)."""
    if packing is not None:
        T, B, F = packing.T, packing.B, mix.shape[1]
        lens = packing.lens
    else:
        T, B, F = mix.shape
    S = len(srcs)
    for t in [mask, mix] + list(srcs):
        _chk(t)
        if not t.is_contiguous():
            raise _lib.SepkernError("pit_mse needs contiguous tensors")
    _chk(lens, torch.int32)
    nperm = 1
    for i in range(2, S + 1):
        nperm *= i
    dev = mix.device
    pair = torch.empty(B, S, S, device=dev)
    perm_loss = torch.empty(nperm, B, device=dev)
    best = torch.empty(B, dtype=torch.int32, device=dev)
    out = torch.empty(3, device=dev)
    ws = workspace(_lib.load().sk_pit_workspace_bytes(T, B, S), "pit")
    sp = (C.c_void_p * S)(*[s.data_ptr() for s in srcs])
    _chk(norm_dev)
    rows = packing.R if packing is not None else T * B
    with _timed("pit_fwd", repeat * float(rows) * (2 * S + 1) * F * 4):       # algorithmic bytes: mask, mixture, S sources
        for _ in range(repeat):
            _lib.call("sk_pit_mse_fwd", _ptr(mask), _ptr(mix), sp, _ptr(lens), _ptr(packing.offs) if packing is not None else None,
                      T, B, F, S, _ptr(norm_dev), _ptr(pair), _ptr(perm_loss), _ptr(best), _ptr(out), _ptr(ws), _stream())
    return dict(out=out, pair=pair, perm_loss=perm_loss, best_perm=best)


def pit_mse_bwd(mask, mix, srcs, best_perm, out, gscale, packing=None, repeat=1):
    S = len(srcs)
    dmask = torch.empty_like(mask)
    sp = (C.c_void_p * S)(*[s.data_ptr() for s in srcs])
    _chk(gscale)
    if packing is not None:
        T, B, F, R, offs = packing.T, packing.B, mix.shape[1], packing.R, packing.offs
        if mask.shape[0] > R:
            dmask[R:].zero_()            # tail rows of an (Rp, .) buffer stay zero
    else:
        (T, B, F), R, offs = mix.shape, 0, None
    rows = R if packing is not None else T * B
    with _timed("pit_bwd", repeat * float(rows) * (3 * S + 1) * F * 4):        # the forward's operands + dmask written
        for _ in range(repeat):
            _lib.call("sk_pit_mse_bwd", _ptr(mask), _ptr(mix), sp, _ptr(best_perm), _ptr(out), _ptr(gscale), _ptr(offs), R, T, B, F, S,
                      _ptr(dmask), _stream())
    return dmask


# ----------------------------------------------------------------------------- SI-SDR uPIT loss (waveform domain)
def _est_offsets(pk, S):
    """Offsets (host list, j * S + s) of the estimates of a packed batch in one flat buffer, and its length: utterance j has
    128 (T_j - 1) samples per source."""
    offs, acc = [], 0
    for T in pk.lens_host:
        for _ in range(S):
            offs.append(acc)
            acc += 128 * (int(T) - 1)
    return offs, acc


def mask_istft_rows(mixc, mask, pk, S, est_offs=None, repeat=1):
    """Mask-apply + iSTFT on PACKED rows: mixc (>= R, 257) complex64, mask (>= R, ld >= S*257) float32 rows of the batch pk
    -> (est: flat float32, est_offs: int64 device (B*S), offsets: the same as a host list).  Estimate s of utterance j is the
    128 (T_j - 1) samples at offsets[j * S + s] -- what sk_mask_istft computes from the same spectra in its own layout.
    est_offs: the device copy of the offsets when the caller made it ahead of time (the upload is a synchronous copy: made
    behind a network's forward pass it would hold the host until that pass has run)."""
    _chk(mixc, torch.complex64)
    _chk(mask)
    if pk.perm is not None:
        raise _lib.SepkernError("mask_istft_rows needs a length-sorted batch (Packing without perm)")
    if mixc.dim() != 2 or mixc.shape[1] != 257 or not mixc.is_contiguous() or mask.dim() != 2 or mask.stride(1) != 1:
        raise _lib.SepkernError("mask_istft_rows: mixc must be (R, 257) contiguous, mask (R, ld) with unit column stride")
    if mixc.shape[0] < pk.R or mask.shape[0] < pk.R or pk.lens_host[-1] < 2:
        raise _lib.SepkernError("mask_istft_rows: fewer rows than the batch has frames, or an utterance of one frame")
    offsets, total = _est_offsets(pk, S)
    est = torch.empty(total, dtype=torch.float32, device=mixc.device)
    d_offs = _i64(offsets, mixc.device) if est_offs is None else est_offs
    _chk(d_offs, torch.int64)
    # algorithmic bytes per frame and source: the complex spectrum, the mask, 128 samples out
    with _timed("istft_rows_kernel", repeat * float(pk.R) * S * (257 * 8 + 257 * 4 + 128 * 4)):
        for _ in range(repeat):
            _lib.call("sk_mask_istft_rows", _ptr(mixc), _ptr(mask), int(mask.stride(0)), _ptr(pk.offs), _ptr(pk.lens), pk.B, S, 512, 128,
                      _ptr(est), _ptr(d_offs), pk.T, _stream())
    return est, d_offs, offsets


# ----------------------------------------------------------------------------- waveform losses: SI-SDR uPIT and MixIT
MIXIT_NREF = 2


def _wave_descriptors(pk, sig_offs, n_est, n_ref):
    """The small device tables of one batch's waveform loss, uploaded in one go BEFORE the network runs: est_offs (B*n_est)
    int64 as mask_istft_rows lays the estimates out, ref_offs (B*n_ref) int64 from sig_offs = {'source<i>': [offset of utterance
    j]}, nsamp (B) int32 = 128 (T_j - 1)."""
    offsets, _ = _est_offsets(pk, n_est)
    refs = [int(sig_offs["source%d" % (i + 1)][j]) for j in range(pk.B) for i in range(n_ref)]
    both = _i64(offsets + refs, pk.device)
    return dict(est_offs=both[:pk.B * n_est], ref_offs=both[pk.B * n_est:], nsamp=(pk.lens - 1) * 128)


def sisdr_descriptors(pk, sig_offs, S):
    """_wave_descriptors of the SI-SDR loss: S estimates against the S references 'source1' .. 'source<S>'."""
    return _wave_descriptors(pk, sig_offs, S, S)


def mixit_descriptors(pk, sig_offs, M):
    """_wave_descriptors of the mixture-invariant loss: M estimates against the two mixed recordings 'source1' / 'source2'."""
    return _wave_descriptors(pk, sig_offs, M, MIXIT_NREF)


def _chk_flat_waves(who, est, est_offs, ref, ref_offs, nsamp, count_dev, n_est, n_ref, need):
    """The flat-waveform arguments of a loss forward -> (pcm16, B); `need` words what est_offs / ref_offs must hold."""
    _chk(est)
    pcm16 = ref.dtype == torch.int16
    _chk(ref, torch.int16 if pcm16 else torch.float32)
    _chk(est_offs, torch.int64)
    _chk(ref_offs, torch.int64)
    _chk(nsamp, torch.int32)
    _chk(count_dev)
    B = int(nsamp.numel())
    if est_offs.numel() != B * n_est or ref_offs.numel() != B * n_ref:
        raise _lib.SepkernError("%s: need %s" % (who, need))
    return pcm16, B


def _wave_mask_grad(who, entry, label, row_bytes, est, est_offs, ref, ref_offs, best, coef, gscale, mixc, pk, n_est, ld, out, repeat):
    """sk_sisdr_mask_grad / sk_mixit_mask_grad (one signature): make or check dmask -- the tail rows of a fresh buffer are
    zeroed (as pit_mse_bwd leaves them), `out` (>= R rows) is written in place and otherwise left alone --, time, call.
    row_bytes(pcm16): the algorithmic bytes per frame."""
    pcm16 = ref.dtype == torch.int16
    _chk(est)
    _chk(ref, torch.int16 if pcm16 else torch.float32)
    _chk(mixc, torch.complex64)
    _chk(gscale)
    _chk(coef)
    _chk(best, torch.int32)
    if out is None:
        ld = n_est * 257 if ld is None else int(ld)
        out = torch.empty(pk.Rp, ld, dtype=torch.float32, device=est.device)
        if pk.Rp > pk.R:
            out[pk.R:].zero_()
    _chk(out)
    if out.dim() != 2 or out.stride(1) != 1 or out.shape[0] < pk.R or mixc.shape[0] < pk.R or not mixc.is_contiguous():
        raise _lib.SepkernError("%s: dmask / mixture rows do not cover the batch" % who)
    with _timed(label, repeat * float(pk.R) * row_bytes(pcm16)):
        for _ in range(repeat):
            _lib.call(entry, _ptr(est), _ptr(est_offs), _ptr(ref), int(pcm16), _ptr(ref_offs), _ptr(pk.lens), _ptr(best),
                      _ptr(coef), _ptr(gscale), _ptr(mixc), _ptr(pk.offs), pk.B, n_est, 512, 128, pk.T, _ptr(out),
                      int(out.stride(0)), _stream())
    return out


def sisdr_pit_fwd(est, est_offs, ref, ref_offs, nsamp, S, max_samples, count_dev=None, repeat=1):
    """PIT on SI-SDR.  est: flat float32 estimates at est_offs (int64 device, B*S: j * S + k); ref: flat references, float32 or
    int16 PCM (scaled by 1/32768), reference i of utterance j at ref_offs[j * S + i]; nsamp int32 device (B): samples per
    utterance; count_dev: optional device scalar replacing B (the global utterance count under data parallelism) ->
    dict(out (3,) = [-mean best score, count, sum of best scores], pair (B,S,S) dB, perm_score (S!,B), best_perm (B),
    coef (B,S,3))."""
    pcm16, B = _chk_flat_waves("sisdr_pit_fwd", est, est_offs, ref, ref_offs, nsamp, count_dev, S, S,
                               "B*S estimate and reference offsets")
    nperm = 1
    for i in range(2, S + 1):
        nperm *= i
    dev = est.device
    pair = torch.empty(B, S, S, device=dev)
    perm_score = torch.empty(nperm, B, device=dev)
    best = torch.empty(B, dtype=torch.int32, device=dev)
    out = torch.empty(3, device=dev)
    coef = torch.empty(B, S, 3, device=dev)
    ws = workspace(_lib.load().sk_sisdr_workspace_bytes(B, S, int(max_samples)), "sisdr")
    # algorithmic bytes: every estimate and every reference sample once
    with _timed("sisdr_fwd", repeat * float(est.numel()) * (4 + (2 if pcm16 else 4))):
        for _ in range(repeat):
            _lib.call("sk_sisdr_pit_fwd", _ptr(est), _ptr(est_offs), _ptr(ref), int(pcm16), _ptr(ref_offs), _ptr(nsamp), B, S,
                      int(max_samples), _ptr(count_dev), _ptr(pair), _ptr(perm_score), _ptr(best), _ptr(out), _ptr(coef), _ptr(ws),
                      _stream())
    return dict(out=out, pair=pair, perm_score=perm_score, best_perm=best, coef=coef)


def sisdr_mask_grad(est, est_offs, ref, ref_offs, best_perm, coef, gscale, mixc, pk, S, ld=None, out=None, repeat=1):
    """dmask (Rp, ld) = gscale * d loss / d mask of the SI-SDR uPIT loss (sk_sisdr_mask_grad): the SI-SDR gradient and the
    adjoint of mask-apply + iSTFT in one kernel.  Rows of the batch's frames are written, columns < S*257; dmask as
    _wave_mask_grad makes or checks it."""
    # algorithmic bytes per frame and source: 2 x 128 new samples, the mixture's complex row, 257 gradients out
    return _wave_mask_grad("sisdr_mask_grad", "sk_sisdr_mask_grad", "sisdr_bwd",
                           lambda pcm16: S * (128 * (4 + (2 if pcm16 else 4)) + 257 * 8 + 257 * 4),
                           est, est_offs, ref, ref_offs, best_perm, coef, gscale, mixc, pk, S, ld, out, repeat)


def mixit_fwd(est, est_offs, ref, ref_offs, nsamp, M, max_samples, tau, count_dev=None, repeat=1):
    """The mixture-invariant loss (sk_mixit_fwd; sepkern/mixit.py defines it).  est: flat float32 estimates at est_offs (int64
    device, B*M: j * M + k); ref: flat references, float32 or int16 PCM (scaled by 1/32768), reference n of utterance j at
    ref_offs[j * 2 + n]; nsamp int32 device (B): samples per utterance; tau = 10^(-snr_max/10); count_dev: optional device
    scalar replacing B (the global utterance count under data parallelism) ->
    dict(out (3,) = [-mean best score, count, sum of best scores], assign_score (2^M,B) dB, best_code (B), coef (B,2))."""
    pcm16, B = _chk_flat_waves("mixit_fwd", est, est_offs, ref, ref_offs, nsamp, count_dev, M, MIXIT_NREF,
                               "B*M estimate offsets and B*2 reference offsets")
    dev = est.device
    score = torch.empty(1 << M, B, device=dev)
    best = torch.empty(B, dtype=torch.int32, device=dev)
    out = torch.empty(3, device=dev)
    coef = torch.empty(B, MIXIT_NREF, device=dev)
    ws = workspace(_lib.load().sk_mixit_workspace_bytes(B, M, int(max_samples)), "mixit")
    # algorithmic bytes: every estimate and both reference samples once
    nref = float(est.numel()) / M * MIXIT_NREF
    with _timed("mixit_fwd", repeat * (float(est.numel()) * 4 + nref * (2 if pcm16 else 4))):
        for _ in range(repeat):
            _lib.call("sk_mixit_fwd", _ptr(est), _ptr(est_offs), _ptr(ref), int(pcm16), _ptr(ref_offs), _ptr(nsamp), B, M,
                      int(max_samples), _ptr(count_dev), float(tau), _ptr(score), _ptr(best), _ptr(out), _ptr(coef), _ptr(ws),
                      _stream())
    return dict(out=out, assign_score=score, best_code=best, coef=coef)


def mixit_mask_grad(est, est_offs, ref, ref_offs, best_code, coef, gscale, mixc, pk, M, ld=None, out=None, repeat=1):
    """dmask (Rp, ld) = gscale * d loss / d mask of the mixture-invariant loss (sk_mixit_mask_grad): one transform per
    (utterance, reference) whose result lands in the column block of every estimate of that reference's group.  Rows of the
    batch's frames are written, columns < M*257; dmask as _wave_mask_grad makes or checks it."""
    _chk(est_offs, torch.int64)
    _chk(ref_offs, torch.int64)
    if est_offs.numel() != pk.B * M or ref_offs.numel() != pk.B * MIXIT_NREF or best_code.numel() != pk.B or coef.numel() != pk.B * MIXIT_NREF:
        raise _lib.SepkernError("mixit_mask_grad: need B*M estimate offsets, B*2 reference offsets and coefficients, B codes")
    # algorithmic bytes per frame: M + 1 x 128 new samples and the mixture's complex row per reference at most, M x 257 gradients out
    return _wave_mask_grad("mixit_mask_grad", "sk_mixit_mask_grad", "mixit_bwd",
                           lambda pcm16: 128 * (4 * M + MIXIT_NREF * (2 if pcm16 else 4)) + MIXIT_NREF * 257 * 8 + M * 257 * 4,
                           est, est_offs, ref, ref_offs, best_code, coef, gscale, mixc, pk, M, ld, out, repeat)


# ----------------------------------------------------------------------------- phase-sensitive targets (loss=psa / tpsa)
def stft_psa(flat, sig_offs, nsamp, S, pk=None, clamp=False, out=None, repeat=1):
    """The network's input and the phase-sensitive targets of a batch of waveforms in one launch (sk_stft_psa; sepkern/psa.py
    defines the arithmetic).  flat: ONE 1-D CUDA tensor holding every signal, float32 or int16 PCM (scaled by 1/32768
    in-kernel); sig_offs: S + 1 lists (the mixture's, then source 1 .. S) of B offsets into flat; nsamp: samples per utterance.
    -> (mix_rows, targets): the mixture's magnitudes |Y| and a list of S views of one buffer, target_s = Re(S_s conj Y) / |Y|
    (clamp: held to [0, |Y|]).
    With pk (the batch's Packing, length-sorted: no perm) both are packed rows (Rp, 257), rows R.. zero; without it, utterance u
    is the block of T_u = 1 + nsamp[u] // 128 rows that starts at row sum_{v<u} T_v (frame-major (T_u, 257)).
    out = (mix (>= rows, ld), targets (S, >= rows, ld)) float32 with unit column stride is written in place."""
    pcm16 = _samples("stft_psa", flat)
    ns = _lengths("stft_psa", nsamp, what="utterance")[0]
    B, F, dev = len(ns), 257, flat.device
    offs, _ = _offsets("stft_psa", sig_offs, ns, flat.numel(), (S + 1, S + 1, "signal (the mixture, then the S sources)"))
    Ts, rows, rows_p, bases = _row_layout("stft_psa", ns, pk)
    if out is None:
        mix = torch.empty(rows_p, F, dtype=torch.float32, device=dev)
        tgt = torch.empty(max(S, 1), rows_p, F, dtype=torch.float32, device=dev)
        if rows_p > rows:
            mix[rows:].zero_()
            tgt[:, rows:].zero_()
    else:
        mix, tgt = out
    _chk(mix)
    _chk(tgt)
    if mix.dim() != 2 or tgt.dim() != 3 or mix.stride(1) != 1 or tgt.stride(2) != 1 or tgt.stride(1) != mix.stride(0) or \
            mix.shape[0] < rows or tgt.shape[1] < rows or tgt.shape[0] < S or mix.shape[1] != tgt.shape[2]:
        raise _lib.SepkernError("stft_psa: out must be (mix (>= rows, ld), targets (S, >= rows, ld)) with one row stride")
    ld = int(mix.stride(0)) if mix.shape[0] > 1 else int(mix.shape[1])
    ws = torch.empty(rows * F, 2, dtype=torch.float32, device=dev)       # the mixture's complex bins on their way to the contractions
    d64, d_ns = _i64(offs + (bases or []), dev), _i32(ns, dev)
    # algorithmic bytes per frame: 128 new samples of each of the S + 1 signals in, their 257 values out
    with _timed("stft_psa_kernel", repeat * float(sum(Ts)) * (S + 1) * (128 * (2 if pcm16 else 4) + 257 * 4)):
        for _ in range(repeat):
            _lib.call("sk_stft_psa", _ptr(flat), int(pcm16), _ptr(d64), _ptr(d_ns), B, int(S), 512, 128, int(bool(clamp)),
                      _ptr(pk.offs) if pk is not None else None, _ptr(d64[(S + 1) * B:]) if pk is None else None,
                      _ptr(mix), _ptr(tgt), ld, int(tgt.stride(0)), _ptr(ws), min(ns), max(Ts), _stream())
    return mix, [tgt[s] for s in range(S)]


# ----------------------------------------------------------------------------- inter-channel phase features (ipd_channels)
def stft_ipd(flat, sig_offs, nsamp, pk=None, out=None, want_mix=True, ws=None, repeat=1):
    """The input rows of an IPD model from a batch of array waveforms in one launch (sk_stft_ipd; sepkern/ipd.py defines the
    arithmetic).  flat: ONE 1-D CUDA tensor holding every signal, float32 or int16 PCM (scaled by 1/32768 in-kernel); sig_offs:
    1 + P lists (the reference channel's, then listed channel 1 .. P) of B offsets into flat; nsamp: samples per utterance.
    -> (rows (>= R, ld), mix (>= R, 257) or None): rows = [ |Y_r| | cos_1 | sin_1 | ... ] of width 257 (1 + 2P) in a buffer whose
    row stride ld is that width rounded up to 16, the columns in between zero -- the engine takes it as it is; mix = a contiguous
    copy of the magnitude columns (want_mix), which the loss kernels read.
    With pk (the batch's Packing, length-sorted: no perm) both are packed rows (Rp, .), rows R.. zero; without it, utterance u is
    the block of T_u = 1 + nsamp[u] // 128 rows that starts at row sum_{v<u} T_v.
    out = (rows (>= R, ld >= width) float32 with unit column stride, mix (>= R, 257) contiguous or None) is written in place.
    ws: the work rows, a float32 tensor of at least R * 257 * 2 elements (default: allocated here)."""
    from . import ipd as _ipd
    pcm16 = _samples("stft_ipd", flat)
    ns = _lengths("stft_ipd", nsamp, what="utterance")[0]
    B, F, dev = len(ns), 257, flat.device
    offs, nsig = _offsets("stft_ipd", sig_offs, ns, flat.numel(), (2, 1 + _ipd.MAX_PAIRS, "channel (the reference first)"))
    P = nsig - 1
    Ts, nrows, rows_p, bases = _row_layout("stft_ipd", ns, pk)
    width = _ipd.in_dim(P)
    if out is None:
        rows = torch.empty(rows_p, _ipd.padded_dim(P), dtype=torch.float32, device=dev)
        mix = torch.empty(rows_p, F, dtype=torch.float32, device=dev) if want_mix else None
        if rows_p > nrows:
            rows[nrows:].zero_()
            if mix is not None:
                mix[nrows:].zero_()
    else:
        rows, mix = out
    _chk(rows)
    _chk(mix)
    if rows.dim() != 2 or rows.stride(1) != 1 or rows.shape[0] < nrows or rows.shape[1] < width:
        raise _lib.SepkernError("stft_ipd: rows must be (>= %d, >= %d) float32 with unit column stride" % (nrows, width))
    if mix is not None and (mix.dim() != 2 or tuple(mix.shape[1:]) != (F,) or mix.shape[0] < nrows or not mix.is_contiguous()):
        raise _lib.SepkernError("stft_ipd: mix must be a contiguous (>= %d, 257) float32 tensor" % nrows)
    ld = int(rows.stride(0)) if rows.shape[0] > 1 else int(rows.shape[1])
    if ws is None:
        ws = torch.empty(nrows * F, 2, dtype=torch.float32, device=dev)  # the reference's complex bins on their way to the contractions
    _chk(ws)
    if not ws.is_contiguous() or ws.numel() < nrows * F * 2:
        raise _lib.SepkernError("stft_ipd: ws must be a contiguous float32 tensor of at least %d elements" % (nrows * F * 2))
    d64, d_ns = _i64(offs + (bases or []), dev), _i32(ns, dev)
    # algorithmic bytes per frame: 128 new samples of each of the 1 + P signals in; 257 (1 + 2P) features (+ 257 of mix) out
    nbytes = (1 + P) * 128 * (2 if pcm16 else 4) + (width + (F if mix is not None else 0)) * 4
    with _timed("stft_ipd_kernel", repeat * float(sum(Ts)) * nbytes):
        for _ in range(repeat):
            _lib.call("sk_stft_ipd", _ptr(flat), int(pcm16), _ptr(d64), _ptr(d_ns), B, 1 + P, 512, 128,
                      _ptr(pk.offs) if pk is not None else None, _ptr(d64[(1 + P) * B:]) if pk is None else None,
                      _ptr(rows), ld, _ptr(mix), _ptr(ws), min(ns), max(Ts), _stream())
    return rows, mix


def ipd_rows(Y, ref, channels, mag, out=None, repeat=1):
    """The input rows of an IPD model from spectra in memory (sk_ipd_rows; sepkern/ipd.py).  Y (C, T, 257) complex64 with unit bin
    stride (any channel / row stride), ref: the reference channel, channels: the listed ones; mag (T, >= 257) float32: the
    reference channel's magnitude rows as the caller holds them, copied into columns 0..256 unchanged.
    -> rows (T, ld) float32, ld = 257 (1 + 2P) rounded up to 16, the columns behind the features zero.  out (T, >= width) with
    unit column stride is written in place."""
    from . import ipd as _ipd
    _chk(Y, torch.complex64)
    _chk(mag)
    channels = [int(c) for c in channels]
    if Y.dim() != 3 or Y.shape[2] != 257 or Y.stride(2) != 1:
        raise _lib.SepkernError("ipd_rows: Y must be (C, T, 257) complex64 with unit bin stride")
    nch, T, P = int(Y.shape[0]), int(Y.shape[1]), len(channels)
    if mag.dim() != 2 or mag.shape[0] != T or mag.shape[1] < 257 or mag.stride(1) != 1:
        raise _lib.SepkernError("ipd_rows: mag must be (T, >= 257) float32 rows of the %d frames" % T)
    if out is None:
        out = torch.empty(T, _ipd.padded_dim(P) if 1 <= P <= _ipd.MAX_PAIRS else 257, dtype=torch.float32, device=Y.device)
    _chk(out)
    if out.dim() != 2 or out.shape[0] != T or out.stride(1) != 1:
        raise _lib.SepkernError("ipd_rows: out must be (T, >= 257 (1 + 2P)) float32 with unit column stride")
    chans = (C.c_int32 * max(P, 1))(*channels)          # (host array: the entry point checks and copies it before it returns)
    ld = int(out.stride(0)) if T > 1 else int(out.shape[1])
    ld_mag = int(mag.stride(0)) if T > 1 else int(mag.shape[1])
    # algorithmic bytes per frame: the 1 + P channels' complex bins and the magnitude row in, the feature row out
    with _timed("ipd_rows_kernel", repeat * float(T) * 257 * ((1 + P) * 8 + 4 + (1 + 2 * P) * 4)):
        for _ in range(repeat):
            _lib.call("sk_ipd_rows", _ptr(Y), int(Y.stride(0)), int(Y.stride(1)) if T > 1 else 257, T, nch, int(ref), chans, P,
                      _ptr(mag), ld_mag, _ptr(out), ld, _stream())
    return out


# ----------------------------------------------------------------------------- RSH loss / attention
def rsh_loss_fwd(mask, x, srcs, lens, used):
    """One greedy-assignment pass.  mask (T,B,F), x (T,B,2F) [mixture | attention], srcs list of S (T,B,F),
    used (S,B) int32 (updated in place) -> dict(out (2,) = [loss term, norm term], sse (S,B), sel (B))."""
    T, B, F = mask.shape
    S = len(srcs)
    for t in [mask, x] + list(srcs):
        _chk(t)
        if not t.is_contiguous():
            raise _lib.SepkernError("rsh_loss needs contiguous tensors")
    _chk(lens, torch.int32)
    _chk(used, torch.int32)
    dev = mask.device
    sse = torch.empty(S, B, device=dev)
    sel = torch.empty(B, dtype=torch.int32, device=dev)
    out = torch.empty(2, device=dev)
    ws = workspace(_lib.load().sk_rsh_workspace_bytes(T, B, S), "rsh")
    sp = (C.c_void_p * S)(*[s.data_ptr() for s in srcs])
    _lib.call("sk_rsh_loss_fwd", _ptr(mask), _ptr(x), x.shape[2], sp, _ptr(lens), T, B, F, S, _ptr(used), _ptr(sse),
              _ptr(sel), _ptr(out), _ptr(ws), _stream())
    return dict(out=out, sse=sse, sel=sel)


def rsh_loss_bwd(mask, x, srcs, sel, gscale):
    T, B, F = mask.shape
    S = len(srcs)
    dmask = torch.empty_like(mask)
    sp = (C.c_void_p * S)(*[s.data_ptr() for s in srcs])
    _chk(gscale)
    _lib.call("sk_rsh_loss_bwd", _ptr(mask), _ptr(x), x.shape[2], sp, _ptr(sel), _ptr(gscale), T, B, F, S, _ptr(dmask),
              _stream())
    return dmask


def att_update(x, mask, relu):
    out = torch.empty_like(x)
    F = mask.shape[-1]
    _lib.call("sk_att_update", _ptr(x), _ptr(mask), _ptr(out), x.numel() // (2 * F), F, int(relu), _stream())
    return out


def att_update_bwd(dx_out, x_out, F, relu):
    dx_in = torch.empty_like(dx_out)
    dmask = torch.empty(dx_out.shape[:-1] + (F,), device=dx_out.device)
    _lib.call("sk_att_update_bwd", _ptr(dx_out), _ptr(x_out), _ptr(dx_in), _ptr(dmask), dx_out.numel() // (2 * F), F,
              int(relu), _stream())
    return dx_in, dmask


# ----------------------------------------------------------------------------- BN / column ops
def bn_ws(R, Ccols, tag="bn"):
    return workspace(_lib.load().sk_bn_workspace_bytes(R, Ccols), tag)


def bn_stats(x2d, mean, var, rows=None, count=None):
    """mean / biased variance per column over `count` rows of which the first `rows` of x2d are stored and the rest are
    zero rows that are not (packed sequences: count = B * T_max); defaults: all of x2d's rows, count = rows."""
    _dense("bn_stats", x2d, mean, var)
    R, Cc = x2d.shape
    R = R if rows is None else rows
    _lib.call("sk_bn_stats", _ptr(x2d), R, Cc, int(R if count is None else count), _ptr(mean), _ptr(var), _ptr(bn_ws(R, Cc)),
              _stream())


def bn_update_running(mean, var, rmean, rvar, count, momentum, guard=None):
    """guard: optional device word (the recurrence's sticky status, lstm_sticky): non-zero = leave the running statistics."""
    _lib.call("sk_bn_update_running", _ptr(mean), _ptr(var), _ptr(rmean), _ptr(rvar), int(count), mean.numel(), float(momentum),
              _ptr(guard), _stream())


def bn_apply(x2d, mean, var, gamma, beta, out, eps):
    _dense("bn_apply", x2d, mean, var, gamma, beta, out)
    R, Cc = x2d.shape
    _lib.call("sk_bn_apply", _ptr(x2d), _ptr(mean), _ptr(var), _ptr(gamma), _ptr(beta), _ptr(out), R, Cc, float(eps),
              _stream())


def bn_fold(W, b, mean, var, gamma, beta, eps, ld=None):
    """BatchNorm folded into the Linear layer behind it (sk_bn_fold): returns (Wf (O, ld), bf (O), s (C), t (C)) with
    lin(bn(x)) = x Wf[:, :C]^T + bf."""
    for t_ in (W, b, mean, var, gamma, beta):
        _chk(t_)
    O, Cc = W.shape
    ld = Cc if ld is None else ld
    Wf = torch.empty(O, ld, device=W.device)
    bf, s, t = torch.empty(O, device=W.device), torch.empty(Cc, device=W.device), torch.empty(Cc, device=W.device)
    _lib.call("sk_bn_fold", _ptr(W), _ptr(b), _ptr(mean), _ptr(var), _ptr(gamma), _ptr(beta), float(eps), O, Cc, _ptr(Wf), ld,
              _ptr(bf), _ptr(s), _ptr(t), _stream())
    return Wf, bf, s, t


def bn_unfold_grad(G, dzsum, s, t, dW, accumulate=False):
    """dW (O, C) (+)= G[:, :C] diag(s) + dzsum t^T (sk_bn_unfold_grad): the gradient of the unfolded Linear weight from
    G = dz^T x, the product against the raw (un-normalised) activations."""
    for t_ in (G, dzsum, s, t, dW):
        _chk(t_)
    O, Cc = dW.shape
    _lib.call("sk_bn_unfold_grad", _ptr(G), G.stride(0), _ptr(dzsum), _ptr(s), _ptr(t), _ptr(dW), O, Cc, int(accumulate), _stream())


def bn_bwd(dout, x2d, mean, var, gamma, dx, dgamma, dbeta, eps):
    _dense("bn_bwd", dout, x2d, mean, var, gamma, dx, dgamma, dbeta)
    R, Cc = x2d.shape
    _lib.call("sk_bn_bwd", _ptr(dout), _ptr(x2d), _ptr(mean), _ptr(var), _ptr(gamma), _ptr(dx), _ptr(dgamma),
              _ptr(dbeta), _ptr(bn_ws(R, Cc)), R, Cc, float(eps), _stream())


def bn_bwd_sums(dout, x2d, mean, var, dgamma, dbeta, eps):
    _dense("bn_bwd_sums", dout, x2d, mean, var, dgamma, dbeta)
    R, Cc = x2d.shape
    _lib.call("sk_bn_bwd_sums", _ptr(dout), _ptr(x2d), _ptr(mean), _ptr(var), _ptr(dgamma), _ptr(dbeta),
              _ptr(bn_ws(R, Cc)), R, Cc, float(eps), _stream())


def bn_bwd_apply(dout, x2d, mean, var, gamma, dgamma, dbeta, dx, count, eps):
    _dense("bn_bwd_apply", dout, x2d, mean, var, gamma, dgamma, dbeta, dx)
    R, Cc = x2d.shape
    _lib.call("sk_bn_bwd_apply", _ptr(dout), _ptr(x2d), _ptr(mean), _ptr(var), _ptr(gamma), _ptr(dgamma), _ptr(dbeta),
              _ptr(dx), R, Cc, float(count), float(eps), _stream())


def colsum(x, R, Ccols, ld, out, accumulate=False, ws_tag="bn"):
    _lib.call("sk_colsum", _ptr(x), R, Ccols, ld, _ptr(out), int(accumulate), _ptr(bn_ws(R, Ccols, ws_tag)), _stream())


def pad_rows(x2d, ld, rows=None):
    """(rows, ld) copy of an (R, C) matrix with zero columns C..ld-1 and zero rows R..rows-1, one pass (sk_pad_rows)."""
    _chk(x2d)
    R, Cc = x2d.shape
    rows = R if rows is None else rows
    out = torch.empty(rows, ld, device=x2d.device)
    _lib.call("sk_pad_rows", _ptr(x2d), R, Cc, x2d.stride(0), _ptr(out), ld, rows, _stream())
    return out


# ----------------------------------------------------------------------------- packed rows
def pack_rows(padded, pk, out):
    """(T, B, C) zero-padded (caller's utterance order) -> the first R rows of out (>= R, ld): packed rows."""
    _chk(padded)
    _chk(out)
    _, B, Cc = padded.shape                  # (frames past pk.T, if any, are padding)
    _lib.call("sk_pack_rows", _ptr(padded), _ptr(pk.offs), _ptr(pk.perm), pk.T, B, Cc, _ptr(out), out.stride(0), _stream())


def unpack_rows(packed, pk, out, fill=None):
    """The first R rows of packed (>= R, ld) -> out (T, B, C) in the caller's utterance order; padded positions get the row
    `fill` (C floats) or zeros."""
    _chk(packed)
    _chk(out)
    _chk(fill)
    T, B, Cc = out.shape
    _lib.call("sk_unpack_rows", _ptr(packed), packed.stride(0), _ptr(pk.offs), _ptr(pk.perm), T, B, Cc, _ptr(fill), _ptr(out),
              _stream())


def hprev_rows(y2d, h0, pk, H, out):
    """out[r] = [forward-direction output one frame earlier | reverse-direction output one frame later] of packed row r,
    h0 (2, B, H) where a row has no such neighbour (sk_hprev_rows); out fp32 or bfloat16, (>= R, ld >= 2H)."""
    _chk(y2d)
    _chk(h0)
    bf = out.dtype == torch.bfloat16
    _chk(out, torch.bfloat16 if bf else torch.float32)
    _lib.call("sk_hprev_rows", _ptr(y2d), y2d.stride(0), _ptr(h0), _ptr(pk.offs), pk.T, pk.B, H, _ptr(out), out.stride(0), int(bf),
              _stream())
    return out


def sigmoid_bwd(dmask, m, dz):
    _dense("sigmoid_bwd", dmask, m, dz)
    _lib.call("sk_sigmoid_bwd", _ptr(dmask), _ptr(m), _ptr(dz), dmask.numel(), _stream())


# ----------------------------------------------------------------------------- LSTM recurrence
def lstm_ws(T, B, H):
    n = _lib.load().sk_lstm_workspace_bytes(T, B, H)
    if n == 0:
        raise _lib.SepkernError("unsupported LSTM shape B=%d H=%d" % (B, H))
    return workspace(n, "lstm")


# Fields of sk_lstm_fwd's / sk_lstm_bwd's `mode` word: include/sepkern.h's SK_LSTM_* names (what each means and which direction
# reads it is written there).  The low byte is the launch kind.
LSTM_AUTO, LSTM_PERSISTENT, LSTM_PER_STEP = 0, 1, 2
LSTM_GMIN_SHIFT = 8                 # bits 8..15
LSTM_BF16 = 1 << 16
LSTM_BWD_EXCLUSIVE = 1 << 17        # backward; the forward's retired `half`
LSTM_MAP_SHIFT = 18                 # bits 18..19
LSTM_POLL1 = 1 << 20
LSTM_REPFLAGS = 1 << 21
LSTM_FLAG_PER_LINE = 1 << 22
LSTM_DELAY_SHIFT = 23               # bits 23..27
LSTM_DELAY_NONE = 31
LSTM_SPLIT3 = 1 << 28
LSTM_TAGGED = 1 << 29
LSTM_XL8 = 1 << 30
# sk_lstm_last_launch(): indices of its eight values, and the kernel families
LSTM_Q_FAMILY, LSTM_Q_KS, LSTM_Q_BF16, LSTM_Q_PACKED, LSTM_Q_GM, LSTM_Q_EXCLUSIVE, LSTM_Q_BLOCKS, LSTM_Q_G = range(8)
LSTM_K_FWD, LSTM_K_FWD_SPLIT3, LSTM_K_FWD_XL8, LSTM_K_BWD, LSTM_K_BWD_XL8 = 1, 2, 3, 4, 5


def lstm_gmin(g):
    return (int(g) & 0xff) << LSTM_GMIN_SHIFT


def lstm_map(m):
    return (int(m) & 3) << LSTM_MAP_SHIFT


def lstm_variant_bits(half=False, blockmap=0, poll1=False, repflags=False, spread=False, poll_delay=0, tagged=False, split3=False,
                      xl8=False):
    """Geometry / protocol variants of the persistent recurrence (speed only; include/sepkern.h, SK_LSTM_*);
    poll_delay: the forward kernel's polling wave holds its first poll of a step back (units of 0.1 us, 0 = the library's
    choice, 31 = none); tagged (forward, fp32): the exchanged h carries the step's epoch in its two low mantissa bits and
    nothing else is signalled (mode bit 29); split3 (forward, fp32): the product h W_hh^T by the exact three-way bf16 split
    of both operands on the bf16 matrix pipe (mode bit 28; flags hand-off, the tagged one does not combine with it); xl8 (forward,
    bf16, 640 < H <= 896, B <= 32, persistent launches; other shapes run the ordinary form): XCD-local streams of 8 rows x 28
    workgroups of 32 units with a plain-store hand-off (mode bit 30) -- the same arithmetic bit for bit."""
    if half:      # (the first field of SEPKERN_LSTM_FWD / _BWD keeps its place so that recorded switch strings stay readable)
        raise _lib.SepkernError("the 8-unit / 256-thread forward recurrence (field `half`, mode bit 17) was retired in r05: "
                                "measured slower at every shape (DESIGN_HISTORY.md)")
    return (lstm_map(blockmap) | (LSTM_POLL1 if poll1 else 0) | (LSTM_REPFLAGS if repflags else 0) |
            (LSTM_FLAG_PER_LINE if spread else 0) | ((int(poll_delay) & 31) << LSTM_DELAY_SHIFT) |
            (LSTM_TAGGED if tagged else 0) | (LSTM_SPLIT3 if split3 else 0) | (LSTM_XL8 if xl8 else 0))


def lstm_variant_from_spec(spec):
    """The mode bits of a SEPKERN_LSTM_FWD / _BWD string: up to nine comma-separated integers
    "half,map,poll1,repflags,spread,delay,tagged,split3,xl8" (lstm_variant_bits' arguments; missing fields are 0)."""
    v = [int(x) for x in spec.split(",")]
    v += [0] * (9 - len(v))
    return lstm_variant_bits(bool(v[0]), v[1], bool(v[2]), bool(v[3]), bool(v[4]), v[5], tagged=bool(v[6]), split3=bool(v[7]),
                             xl8=bool(v[8]))


def lstm_last_launch():
    """(launches, [family, KS, bf16, packed, GM, exclusive, blocks, G]) of this thread's last lstm_fwd / lstm_bwd call
    (sk_lstm_last_launch, include/sepkern.h; index the list with LSTM_Q_*)."""
    out = (C.c_int * 8)()
    n = _lib.load().sk_lstm_last_launch(out)
    return n, list(out)


def lstm_fwd(gx, whh, h0, c0, lens, y, gates, cs, hn, cn, T, B, H, mode=0, bf16=False, blockmap=0, offs=None, rows=None):
    """bf16=True: W_hh and h_{t-1} enter the matrix cores rounded to bf16 (fp32 accumulate, fp32 state).
    blockmap 0..2: which workgroups share an XCD / a CU (mode bits 18..19; speed only).  offs (int32, T+1): the sequence tensors are PACKED
    rows (lens sorted descending; `rows` of them: the launch's algorithmic work for the profile); None: zero-padded (T, B, .)."""
    ws = lstm_ws(T, B, H)
    mode = int(mode) | (LSTM_BF16 if bf16 else 0) | lstm_map(blockmap)
    _chk(offs, torch.int32)
    with _timed("lstm_fwd_kernel", 2.0 * (T * B if rows is None else rows) * 2 * 4 * H * H):
        _lib.call("sk_lstm_fwd", _ptr(gx), _ptr(whh), _ptr(h0), _ptr(c0), _ptr(lens), _ptr(offs), _ptr(y), _ptr(gates), _ptr(cs),
                  _ptr(hn), _ptr(cn), _ptr(ws), T, B, H, mode, _stream())
    return ws


def lstm_bwd(dy, whh, gates, cs, c0, lens, dgx, dh0, dc0, T, B, H, mode=0, dhn=None, dcn=None, bf16=False,
             dbias=None, dgx_bf16=None, offs=None, rows=None):
    """dbias ((B+15)//16, 2, 4H): optional by-product (include/sepkern.h), its column sum is the bias gradient.
    dgx_bf16: a (rows, ld >= 8H) bfloat16 tensor that receives dgx as bf16 as well -- or (fp32 configuration) a Planes object:
    dgx's three exact bf16 pieces, the operand gemm_pl3_tn reads.  offs: as lstm_fwd."""
    plane = 0
    if isinstance(dgx_bf16, Planes):
        if bf16:
            raise _lib.SepkernError("lstm_bwd: planes of dgx belong to the fp32 configuration")
        plane, dgx_bf16 = dgx_bf16.plane, dgx_bf16.t[0]
    ws = lstm_ws(T, B, H)
    mode = int(mode) | (LSTM_BF16 if bf16 else 0)
    _chk(dbias)
    _chk(offs, torch.int32)
    _chk(dgx_bf16, torch.bfloat16)
    if dgx_bf16 is not None and (dgx_bf16.dim() != 2 or dgx_bf16.stride(1) != 1):
        raise _lib.SepkernError("lstm_bwd: the bf16 twin must be a row-major (rows, ld) matrix")
    with _timed("lstm_bwd_kernel", 2.0 * (T * B if rows is None else rows) * 2 * 4 * H * H):
        _lib.call("sk_lstm_bwd", _ptr(dy), _ptr(dhn), _ptr(dcn), _ptr(whh), _ptr(gates), _ptr(cs), _ptr(c0),
                  _ptr(lens), _ptr(offs), _ptr(dgx), _ptr(dh0), _ptr(dc0), _ptr(dbias), _ptr(dgx_bf16),
                  0 if dgx_bf16 is None else dgx_bf16.stride(0), int(plane), _ptr(ws), T, B, H, mode, _stream())
    return ws


def gate_rows(src, H, back=False, out=None, accumulate=False, cols=None):
    """Reorder rows of a (nblk * 4H, C) fp32 matrix (or (nblk * 4H,) vector) between torch's gate-major order and the
    gate-interleaved order of gx / gates / dgx (include/sepkern.h, sk_gate_rows).  src / out may have leading dimensions
    larger than the `cols` logical columns (default: the narrower of the two)."""
    _chk(src)
    s2 = src.reshape(-1, 1) if src.dim() == 1 else src.reshape(-1, src.shape[-1])
    if s2.stride(-1) != 1:
        raise _lib.SepkernError("gate_rows needs unit-stride rows")
    nblk = s2.shape[0] // (4 * H)
    if out is None:
        out = torch.empty_like(src)
    o2 = out.reshape(-1, 1) if out.dim() == 1 else out.reshape(-1, out.shape[-1])
    C_ = min(s2.shape[1], o2.shape[1]) if cols is None else cols
    _lib.call("sk_gate_rows", _ptr(s2), _ptr(o2), nblk, H, C_, s2.stride(0), o2.stride(0), int(back), int(accumulate), _stream())
    return out


def gates_interleaved(t, H, back=False):
    """(..., 4H) gate-major <-> gate-interleaved along the LAST axis, by torch view/permute (tests and tools: the
    product path gets the interleaved order for free from reordered weight rows)."""
    shape = t.shape
    if back:
        return t.reshape(shape[:-1] + (H, 4)).transpose(-1, -2).reshape(shape).contiguous()
    return t.reshape(shape[:-1] + (4, H)).transpose(-1, -2).reshape(shape).contiguous()


def lstm_status(ws):
    """Raises SepkernError (SK_ETIMEOUT) if a persistent launch on this workspace timed out since the last call."""
    _lib.call("sk_lstm_status", _ptr(ws), _stream())


def lstm_sticky(ws):
    """The workspace's sticky status word as a 1-element int32 view (device side checks, no sync)."""
    return ws[:4].view(torch.int32)


# ----------------------------------------------------------------------------- optimizer
def grad_norm(g, max_norm, scal, guard=None):
    """scal (4,) <- [norm, clip coefficient, skip this step, skipped so far]; guard: optional 1-element float tensor,
    non-zero = do not apply this step (include/sepkern.h)."""
    ws = workspace(_lib.load().sk_optim_workspace_bytes(g.numel()), "optim")
    _lib.call("sk_grad_norm", _ptr(g), g.numel(), float(max_norm), _ptr(guard), _ptr(scal), _ptr(ws), _stream())


def clip_adam(p, g, m, v, scal, lr, beta1, beta2, eps, step):
    _lib.call("sk_clip_adam", _ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), _ptr(scal), float(lr), float(beta1),
              float(beta2), float(eps), int(step), _stream())


# ----------------------------------------------------------------------------- BSS Eval scoring (fp64)
def bss_xc_len(S, taps):
    """Doubles per utterance in sk_bss_xcorr's record (include/sepkern.h)."""
    return S * (S + 1) // 2 * (2 * taps - 1) + S * S * taps + S


def _bss_args(ref, est, offs, lens, S, taps):
    _chk(ref, torch.float64)
    _chk(est, torch.float64)
    if ref.shape != est.shape or ref.dim() != 1 or not ref.is_contiguous() or not est.is_contiguous():
        raise _lib.SepkernError("bss: ref and est must be contiguous 1-D fp64 tensors of one length (packed rows)")
    offs = [int(o) for o in offs]
    lens = [int(n) for n in lens]
    if len(offs) != len(lens) or any(o + S * n > ref.numel() for o, n in zip(offs, lens)):
        raise _lib.SepkernError("bss: offsets / lengths run past the packed rows")
    U = len(lens)
    h_offs = (C.c_int64 * U)(*offs)
    h_lens = (C.c_int32 * U)(*lens)
    nbytes = _lib.load().sk_bss_workspace_bytes(U, S, taps)
    # per call, not the cached workspace(): a batch's matrices take gigabytes that should go back to the allocator
    ws = torch.empty(nbytes, dtype=torch.uint8, device=ref.device) if nbytes else None
    return U, h_offs, h_lens, ws


def bss_xcorr(ref, est, offs, lens, S, taps):
    """Lag correlations of packed fp64 rows: utterance u's source / estimate i starts at offs[u] + i*lens[u] of ref /
    est.  Returns (U, bss_xc_len(S, taps)) fp64 (record layout in include/sepkern.h)."""
    U, h_offs, h_lens, ws = _bss_args(ref, est, offs, lens, S, taps)
    xc = torch.empty(U, bss_xc_len(S, taps), dtype=torch.float64, device=ref.device)
    _lib.call("sk_bss_xcorr", _ptr(ref), _ptr(est), h_offs, h_lens, U, S, taps, _ptr(ws), _ptr(xc), _stream())
    return xc


def bss_eval(ref, est, offs, lens, S, taps):
    """SDR / SIR / SAR of every (estimate k, source j) pair: returns (out (U, S, S, 3) fp64 dB, status (U) int32);
    status != 0 marks an utterance whose Gram matrix did not factor (include/sepkern.h)."""
    U, h_offs, h_lens, ws = _bss_args(ref, est, offs, lens, S, taps)
    out = torch.empty(U, S, S, 3, dtype=torch.float64, device=ref.device)
    status = torch.empty(U, dtype=torch.int32, device=ref.device)
    with _timed("bss_eval"):
        _lib.call("sk_bss_eval", _ptr(ref), _ptr(est), h_offs, h_lens, U, S, taps, _ptr(ws), _ptr(out), _ptr(status),
                  _stream())
    return out, status


# ----------------------------------------------------------------------------- STOI / ESTOI scoring
def stoi(ref, est, offs, lens, S):
    """STOI and ESTOI of every (estimate k, reference j) pair of packed fp32 rows at 10 kHz (sk_bss_eval's layout: utterance
    u's source / estimate i starts at offs[u] + i*lens[u]): returns (out (U, S, S, 2) fp64, frames (U, S) int32: the T of
    reference j; T < 30 -> 1e-5).  The definition is sepkern/stoi.py's (include/sepkern.h "STOI")."""
    _chk(ref)
    _chk(est)
    if ref.shape != est.shape or ref.dim() != 1 or not ref.is_contiguous() or not est.is_contiguous():
        raise _lib.SepkernError("stoi: ref and est must be contiguous 1-D fp32 tensors of one length (packed rows)")
    offs = [int(o) for o in offs]
    lens = [int(n) for n in lens]
    if len(offs) != len(lens) or not lens or any(o + S * n > ref.numel() for o, n in zip(offs, lens)):
        raise _lib.SepkernError("stoi: offsets / lengths run past the packed rows")
    U = len(lens)
    h_offs = (C.c_int64 * U)(*offs)
    h_lens = (C.c_int32 * U)(*lens)
    nbytes = _lib.load().sk_stoi_workspace_bytes(U, S, max(lens))
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=ref.device)
    out = torch.empty(U, max(S, 0), max(S, 0), 2, dtype=torch.float64, device=ref.device)
    frames = torch.empty(U, max(S, 0), dtype=torch.int32, device=ref.device)
    with _timed("stoi"):
        _lib.call("sk_stoi", _ptr(ref), _ptr(est), h_offs, h_lens, U, S, _ptr(ws), _ptr(out), _ptr(frames), _stream())
    return out, frames
