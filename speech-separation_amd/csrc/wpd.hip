// wpd.hip -- mask-based WPD convolutional beamforming of a multi-channel recording (sk_wpd).
//
// No counterpart in the reference, which works on one close-talk channel; sepkern/wpd.py states the definition (per block of
// frames, bin and stream, on a window around the block: the power of the stream weights the covariance R of the stacked vector
// y_ = [present frame; delayed past], the stream's mask weights the spatial covariance PHI of the present frame,
// G = R^-1 [PHI; 0] by an fp64 Cholesky solve, w = G[:, ref] / Re tr G[:C], z = w^H y_) and restates it in numpy.  One launch,
// one workgroup per (block, bin, stream), as in wpe.hip: the problems are independent, so there are no atomics, no hand-off
// between workgroups and no workspace, and every sum has one order whatever the strides.
//
// A workgroup keeps in LDS the upper triangle of R (packed by rows), the D x C buffer [PHI; 0] (which the solves turn into G in
// place), 1 / diag U, the filter w, the window's weights 1 / lambda(t), and a chunk of TC frames of its bin widened to fp64:
// the TC + K - 1 frames the chunk's stacked pasts are made of, the chunk's own frames and its masks.  An iteration walks the
// window's chunks twice, as wpe_kernel does:
//   pass A   lambda(t): m(t) (sum_c |y_c|^2) / C in the first iteration of a call without W_in, |w^H y_(t)|^2 otherwise
//            (a thread per frame, D complex multiply-adds); after the last chunk lambda_max, the floor, 1 / lambda in place
//   pass B   every thread owns one 4 x 4 tile of the upper triangle of R or of PHI (wpe_solve.h) and adds (omega y_a) conj(y_b),
//            or (m y_a) conj(y_b), frame by frame, t ascending
// then the tiles go to LDS, the traces and the loading follow, the solve is wpe.hip's (wpe_solve.h), and d, the division and
// the vote on w's components end the iteration.  A last walk over the block's own frames applies w and writes Z.
// What differs from wpe_kernel: the stacked vector begins with the present frame, so the first C rows and columns of R address
// the `cur` slab of the staged chunk; the right-hand side has (C / 4)^2 tiles, weighted by the mask, in the first C rows of a
// buffer that is otherwise zero; and pass A needs the filter alone, not a D x C matrix.  The operations and their order are
// sepkern/wpd.py's, one rounding each -- no multiply is fused into an add in this file.
#include "sk_common.h"
#include "wpe_solve.h"  // the tiles and the solve, shared with wpe.hip

// sepkern/wpd.py states every operation with a rounding of its own: no product is fused into a sum here
#pragma clang fp contract(off)

namespace {

constexpr int NBIN = 257;
constexpr int WPD_MINC = 2, WPD_MAXC = 8, WPD_MINS = 2, WPD_MAXS = 4, WPD_MAXD = 80, WPD_MAXIT = 8, WPD_MAXWIN = 4096;
constexpr int WPD_LDS_LIMIT = 159 * 1024;  // of a CU's 160 KB; the kernel has a few hundred bytes of static LDS besides

// frames per chunk (wpe.hip's): pass A and the apply walk have TC frames for the workgroup's threads.  A longer chunk saves
// barriers, a shorter one LDS: at the defaults (C = 7, K = 5, a window of 600) a workgroup takes 40 KB and three share a CU
constexpr int wpd_tc(int C) { return C <= 2 ? 256 : C <= 4 ? 128 : 64; }
// frames of the past slab: a chunk's stacked pasts reach K - 1 frames further back than its first frame's
constexpr int wpd_pf(int C, int K) { return K > 0 ? wpd_tc(C) + K - 1 : 0; }

// LDS of one workgroup, in bytes: [R triangle | PHI~/G | past | cur | w] complex128, [rinv | omega | m | red] fp64
inline size_t wpd_lds_bytes(int C, int K, int lw) {
  const size_t D = (size_t)C * (K + 1), TC = wpd_tc(C), PF = wpd_pf(C, K);
  return 16 * (D * (D + 1) / 2 + D * C + PF * C + TC * C + D) + 8 * (D + (size_t)lw + TC + 4);
}

template <int C, int NTHR>
__global__ __launch_bounds__(NTHR) void wpd_kernel(const float2* __restrict__ Y, int64_t ycs, int64_t yrs, const float* __restrict__ mask,
                                                   int ldm, int T, int S, int K, int delay, int iters, int Lb, int Lc, int ref,
                                                   double loading, double floor, int lw_max,
                                                   const double2* __restrict__ Win /* (nblk, S, NBIN, D) or NULL */,
                                                   float2* __restrict__ Z /* (S, T, NBIN) */, double2* __restrict__ Wout /* or NULL */) {
  extern __shared__ __align__(16) unsigned char wpd_lds[];
  constexpr int TC = wpd_tc(C), NCT = (C + 3) / 4;
  const int D = C * (K + 1), NP = D * (D + 1) / 2, NTR = (D + 3) / 4, PF = wpd_pf(C, K);
  double2* const Rt = (double2*)wpd_lds;
  double2* const PG = Rt + NP;
  double2* const past = PG + D * C;
  double2* const cur = past + PF * C;
  double2* const wv = cur + TC * C;
  double* const rinv = (double*)(wv + D);
  double* const lam = rinv + D;
  double* const mch = lam + lw_max;
  double* const red = mch + TC;

  const int tid = threadIdx.x, j = blockIdx.x, f = blockIdx.y, s = blockIdx.z;
  const int b0 = (int)min((int64_t)T, (int64_t)j * Lb), b1 = (int)min((int64_t)T, (int64_t)j * Lb + Lb);
  const int w0 = (int)max((int64_t)0, (int64_t)j * Lb - Lc), w1 = (int)min((int64_t)T, (int64_t)j * Lb + Lb + Lc);
  const float2* __restrict__ Yf = Y + f;
  const float* __restrict__ mf = mask + s * NBIN + f;
  const int64_t cell = (((int64_t)j * S + s) * NBIN + f) * D;  // of Win and Wout

  // this thread's tile: rows 4 ti .. 4 ti + 3 of y_ against columns 4 tj .. of y_ (R, tj >= ti), or of y against y (PHI)
  const SolveTile tile = solve_tile(tid, NTR, NCT, NCT);
  // offsets into [past | cur] of the tile's operands at the chunk's first frame; a frame further is C elements further.
  // y_(t)[c] lies at cur[(t - c0) C + c], y_(t)[C + k C + c] at past[(t - c0 + K - 1 - k) C + c].  Rows and columns past D
  // (or C) repeat the last one: their accumulators are never stored.
  auto off_of = [&](int d) { return d < C ? PF * C + d : (K - 1 - (d - C) / C) * C + (d - C) % C; };
  int offa[4], offb[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int lim = tile.is_p ? C - 1 : D - 1;
    offa[q] = off_of(min(4 * tile.ti + q, lim));
    offb[q] = off_of(min(4 * tile.tj + q, lim));
  }

  // the chunk [c0, c0 + nfr): its stacked pasts' frames (where the pass reads them) and its own, widened, and its masks
  auto stage = [&](int c0, int nfr, bool with_past) {
    if (with_past && K > 0) {
      const int64_t u0 = (int64_t)c0 - delay - K + 1;  // u0 + r <= c0 + nfr - 1 - delay < T
      for (int idx = tid; idx < (nfr + K - 1) * C; idx += NTHR) {
        const int r = idx / C, c = idx - r * C;
        const int64_t u = u0 + r;
        float2 v = make_float2(0.f, 0.f);
        if (u >= 0) v = Yf[c * ycs + u * yrs];
        past[idx] = make_double2((double)v.x, (double)v.y);
      }
    }
    for (int idx = tid; idx < nfr * C; idx += NTHR) {
      const int r = idx / C, c = idx - r * C;
      const float2 v = Yf[c * ycs + (int64_t)(c0 + r) * yrs];
      cur[idx] = make_double2((double)v.x, (double)v.y);
    }
    for (int r = tid; r < nfr; r += NTHR) mch[r] = (double)mf[(int64_t)(c0 + r) * ldm];
  };
  // z = w^H y_ of frame r of the staged chunk, d ascending
  auto dot = [&](int r) {
    double sr = 0.0, si = 0.0;
    const double2* __restrict__ yp = cur + r * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {  // conj(w) y
      const double2 w = wv[c], y = yp[c];
      sr += w.x * y.x + w.y * y.y;
      si += w.x * y.y - w.y * y.x;
    }
    for (int k = 0; k < K; ++k) {
      yp = past + (r + K - 1 - k) * C;
      const double2* __restrict__ wp = wv + C + k * C;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const double2 w = wp[c], y = yp[c];
        sr += w.x * y.x + w.y * y.y;
        si += w.x * y.y - w.y * y.x;
      }
    }
    return make_double2(sr, si);
  };

  if (Win)
    for (int d = tid; d < D; d += NTHR) wv[d] = Win[cell + d];

  bool fb = false;
  for (int it = 0; it < iters && !fb; ++it) {
    // ---- pass A: lambda(t) over the window
    const bool have_w = it > 0 || Win != nullptr;
    for (int c0 = w0; c0 < w1; c0 += TC) {
      const int nfr = min(TC, w1 - c0);
      __syncthreads();  // the chunk before is read; w is written
      stage(c0, nfr, have_w);  // without a filter lambda is the present frame's power
      __syncthreads();
      for (int r = tid; r < nfr; r += NTHR) {
        double l;
        if (have_w) {
          const double2 z = dot(r);
          l = z.x * z.x + z.y * z.y;
        } else {
          double p = 0.0;
#pragma unroll
          for (int c = 0; c < C; ++c) {
            const double2 y = cur[r * C + c];
            p += y.x * y.x + y.y * y.y;
          }
          l = mch[r] * (p / (double)C);
        }
        lam[c0 - w0 + r] = l;
      }
    }
    __syncthreads();
    double lmax = 0.0;
    for (int t = tid; t < w1 - w0; t += NTHR) lmax = fmax(lmax, lam[t]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lmax = fmax(lmax, __shfl_xor(lmax, o, 64));
    if ((tid & 63) == 0) red[tid >> 6] = lmax;
    __syncthreads();
    lmax = red[0];
#pragma unroll
    for (int w = 1; w < NTHR / 64; ++w) lmax = fmax(lmax, red[w]);
    if (lmax == 0.0) {  // uniform over the workgroup
      fb = true;
      break;
    }
    for (int t = tid; t < w1 - w0; t += NTHR) lam[t] = 1.0 / fmax(lam[t], floor * lmax);

    // ---- pass B: the tiles of R and PHI, t ascending
    double ar[4][4], ai[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) ar[p][q] = ai[p][q] = 0.0;
    for (int c0 = w0; c0 < w1; c0 += TC) {
      const int nfr = min(TC, w1 - c0);
      __syncthreads();  // the chunk before is read; lam is written
      stage(c0, nfr, true);
      __syncthreads();
      if (tile.has) {
        const double2* __restrict__ base = past;
        const double* __restrict__ wt = tile.is_p ? mch : lam + (c0 - w0);
        for (int r = 0; r < nfr; ++r, base += C) tile_frame(ar, ai, base, offa, offb, wt[r]);
      }
    }
    // PG held the previous G, which nothing reads any more: [PHI; 0]
    for (int idx = C * C + tid; idx < D * C; idx += NTHR) PG[idx] = make_double2(0.0, 0.0);
    tile_store(tile, ar, ai, Rt, PG, D, C, C);
    __syncthreads();
    double tr = 0.0, trp = 0.0;
    for (int a = 0; a < D; ++a) tr += Rt[tri_row(D, a)].x;
#pragma unroll
    for (int c = 0; c < C; ++c) trp += PG[c * C + c].x;
    if (tr == 0.0 || trp == 0.0) {  // uniform: every thread adds the same numbers in the same order
      fb = true;
      break;
    }
    __syncthreads();
    const double load = loading * tr / (double)D;
    for (int a = tid; a < D; a += NTHR) Rt[tri_row(D, a)].x += load;

    // ---- R = U^H U, U^H Z = PHI~, U G = Z
    cholesky_solve_lds<NTHR>(Rt, PG, rinv, D, C, tid);
    __syncthreads();
    // ---- d = Re tr G[:C], w = G[:, ref] / d
    double d = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) d += PG[c * C + c].x;
    int bad = !(d > 0.0);
    for (int a = tid; a < D; a += NTHR) {
      const double2 g = PG[a * C + ref];
      const double2 w = make_double2(g.x / d, g.y / d);
      wv[a] = w;
      bad |= !(isfinite(w.x) && isfinite(w.y));
    }
    if (__syncthreads_or(bad)) fb = true;
  }

  // ---- the block's own frames
  __syncthreads();
  float2* __restrict__ Zs = Z + (int64_t)s * T * NBIN + f;
  if (fb) {  // Y[ref]'s own bits, w = e_ref
    for (int r = tid; r < b1 - b0; r += NTHR) Zs[(int64_t)(b0 + r) * NBIN] = Yf[ref * ycs + (int64_t)(b0 + r) * yrs];
    if (Wout)
      for (int a = tid; a < D; a += NTHR) Wout[cell + a] = make_double2(a == ref ? 1.0 : 0.0, 0.0);
    return;
  }
  for (int c0 = b0; c0 < b1; c0 += TC) {
    const int nfr = min(TC, b1 - c0);
    __syncthreads();
    stage(c0, nfr, true);
    __syncthreads();
    for (int r = tid; r < nfr; r += NTHR) {
      const double2 z = dot(r);
      Zs[(int64_t)(c0 + r) * NBIN] = make_float2((float)z.x, (float)z.y);
    }
  }
  if (Wout)
    for (int a = tid; a < D; a += NTHR) Wout[cell + a] = wv[a];
}

inline int wpd_tiles(int C, int K) {
  const int ntr = (C * (K + 1) + 3) / 4, nct = (C + 3) / 4;
  return ntr * (ntr + 1) / 2 + nct * nct;
}

}  // namespace

// sk_wpd keeps everything between its passes in LDS
extern "C" size_t sk_wpd_workspace_bytes(int T, int C, int S, int taps, int block_frames, int context_frames) { return 0; }

extern "C" int sk_wpd(const void* Y_c64, int64_t y_chan_stride, int64_t y_row_stride, const float* mask, int ld_mask, int T, int C, int S,
                      int taps, int delay, int iterations, int block_frames, int context_frames, int ref, double loading, double floor,
                      const void* W_in_c128, void* Z_c64, void* W_out_c128, void* ws, sk_stream_t stream) {
  SK_CHECK_ARG(C >= WPD_MINC && C <= WPD_MAXC, "sk_wpd: C = %d channels outside %d..%d", C, WPD_MINC, WPD_MAXC);
  SK_CHECK_ARG(S >= WPD_MINS && S <= WPD_MAXS, "sk_wpd: S = %d streams outside %d..%d", S, WPD_MINS, WPD_MAXS);
  SK_CHECK_ARG(taps >= 0, "sk_wpd: taps = %d is negative", taps);
  SK_CHECK_ARG(delay >= 1, "sk_wpd: delay = %d, at least 1 expected", delay);
  SK_CHECK_ARG((int64_t)C * ((int64_t)taps + 1) <= WPD_MAXD, "sk_wpd: C * (taps + 1) = %lld above %d", (long long)C * ((long long)taps + 1),
               WPD_MAXD);
  SK_CHECK_ARG(iterations >= 1 && iterations <= WPD_MAXIT, "sk_wpd: iterations = %d outside 1..%d", iterations, WPD_MAXIT);
  SK_CHECK_FRAMES("sk_wpd", T);
  SK_CHECK_BLOCK_FRAMES("sk_wpd", block_frames);
  SK_CHECK_WINDOW("sk_wpd", block_frames, context_frames, WPD_MAXWIN);
  SK_CHECK_REF("sk_wpd", ref, C);
  SK_CHECK_LOADING("sk_wpd", loading);
  SK_CHECK_ARG(floor > 0.0 && floor <= 1.0, "sk_wpd: floor = %g outside (0, 1] or NaN", floor);
  SK_CHECK_LD_MASK("sk_wpd", ld_mask, S);
  SK_CHECK_Y_ROW_STRIDE("sk_wpd", y_row_stride);
  SK_CHECK_ARG(Y_c64 && mask && Z_c64, "sk_wpd: null pointer (Y, mask or Z)");
  const float2* Y = (const float2*)Y_c64;
  const double2* Win = (const double2*)W_in_c128;
  float2* Z = (float2*)Z_c64;
  double2* Wout = (double2*)W_out_c128;
  const int K = taps, Lb = block_frames, Lc = context_frames;
  const int nblk = (int)sk_cdiv(T, Lb), lw = (int)min((int64_t)T, (int64_t)Lb + 2 * (int64_t)Lc);
  return sk_dispatch_int<WPD_MINC, WPD_MAXC>(C, [&](auto c) {
    constexpr int Cc = decltype(c)::value;
    auto launch = [&](auto kernel, int nthr) {
      return sk_launch_lds("sk_wpd", "wpd_kernel", kernel, dim3((unsigned)nblk, NBIN, (unsigned)S), dim3(nthr), wpd_lds_bytes(Cc, K, lw),
                           WPD_LDS_LIMIT, (hipStream_t)stream, Y, y_chan_stride, y_row_stride, mask, ld_mask, T, S, K, delay, iterations, Lb,
                           Lc, ref, loading, floor, lw, Win, Z, Wout);
    };
    // a wave is enough while every tile has a thread in it
    return wpd_tiles(Cc, K) <= 64 ? launch(wpd_kernel<Cc, 64>, 64) : launch(wpd_kernel<Cc, 256>, 256);
  });
}
