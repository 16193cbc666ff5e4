// wpe.hip -- dereverberation of a multi-channel recording by weighted prediction error (sk_wpe).
//
// No counterpart in the reference, which works on one close-talk channel; sepkern/wpe.py states the definition (per block of
// frames and bin, on a window around the block: the power of the previous iteration's output weights the covariance R of the
// stacked past y~ and its cross-covariance P with the present, G = R^-1 P by an fp64 Cholesky solve, x = y - G^H y~) and
// restates it in numpy.  One launch, one workgroup per (block, bin): the problems are independent, so there are no atomics,
// no hand-off between workgroups and no workspace, and every sum has one order whatever the strides.
//
// A workgroup keeps in LDS the upper triangle of R (packed by rows), P (which the solves turn into G in place), 1 / diag U,
// the window's weights 1 / lambda(t), and a chunk of TC frames of its bin widened to fp64: the TC + K - 1 frames the chunk's
// stacked pasts are made of, the chunk's own frames, and the chunk's x.  An iteration walks the window's chunks twice:
//   pass A   x = y - G^H y~ with the previous G (threads over (frame, channel); skipped in the first iteration, where x = y),
//            then lambda(t); after the last chunk lambda_max, the floor, and w = 1 / lambda in place
//   pass B   every thread owns one 4 x 4 tile of the upper triangle of R or of P -- 16 complex accumulators on registers --
//            and adds (w y~_a) conj(b) frame by frame, t ascending: 8 complex LDS reads for 64 multiplies and 64 adds
// then the tiles go to LDS, the trace and the loading follow, and the factorisation and the two substitutions run
// right-looking over the workgroup, one barrier per pivot: the pivot row stays unscaled while its step reads it and all rows
// are scaled by 1 / diag U afterwards.  A last walk over the block's own frames applies G and writes X (and |X[ref]|).
// The operations and their order are sepkern/wpe.py's, one rounding each -- no multiply is fused into an add in this file --
// because the tests bound G by the forward error of the SOLVE, I D 2^-52 cond(R) max|G|, which at D = 1 is one unit in the last
// place per iteration and leaves no room for sums of hundreds of frames rounded another way; on the MI355X G has come out
// bit for bit the definition's.  The price is the fused rate: the sums of pass B take twice the fp64 issue slots.
// Pass A costs D C of the D (D + 1) / 2 + D C complex multiply-adds per frame that pass B needs, 16 % at D = 80, C = 8: the
// price of not keeping x for a window of up to 4096 frames.  With few unknowns most threads have no tile: at C = 1, K = 10
// nine of a wave's 64 lanes work in pass B (profiles/wpe.txt).
#include "sk_common.h"
#include "wpe_solve.h"  // the tiles and the solve, shared with wpd.hip

// sepkern/wpe.py states every operation with a rounding of its own: no product is fused into a sum here
#pragma clang fp contract(off)

namespace {

constexpr int NBIN = 257;
constexpr int WPE_MAXC = 8, WPE_MAXD = 80, WPE_MAXIT = 8, WPE_MAXWIN = 4096;
constexpr double WPE_FLOOR = 1e-10;
constexpr int WPE_LDS_LIMIT = 159 * 1024;  // of a CU's 160 KB; the kernel has a few hundred bytes of static LDS besides

// frames per chunk: pass A and the apply walk have TC * C items for the workgroup's threads
constexpr int wpe_tc(int C) { return C <= 2 ? 256 : C <= 4 ? 128 : 64; }

// LDS of one workgroup, in bytes: [R triangle | P/G | past | cur | x] complex128, [rinv | w | red] fp64
inline size_t wpe_lds_bytes(int C, int K, int lw) {
  const size_t D = (size_t)C * K, TC = wpe_tc(C);
  return 16 * (D * (D + 1) / 2 + D * C + (TC + K - 1) * C + 2 * TC * C) + 8 * (D + (size_t)lw + 4);
}

template <int C, int NTHR>
__global__ __launch_bounds__(NTHR) void wpe_kernel(const float2* __restrict__ Y, int64_t ycs, int64_t yrs, int T, int K, int delay,
                                                   int iters, int Lb, int Lc, int ref, double loading, int lw_max,
                                                   float2* __restrict__ X, int64_t xcs, int64_t xrs, float* __restrict__ mag,
                                                   int ldm, double2* __restrict__ Gout /* (nblk, NBIN, D, C) or NULL */) {
  extern __shared__ __align__(16) unsigned char wpe_lds[];
  constexpr int TC = wpe_tc(C), NCT = (C + 3) / 4;
  const int D = C * K, NP = D * (D + 1) / 2, NTR = (D + 3) / 4;
  double2* const Rt = (double2*)wpe_lds;
  double2* const PG = Rt + NP;
  double2* const past = PG + D * C;
  double2* const cur = past + (TC + K - 1) * C;
  double2* const xs = cur + TC * C;
  double* const rinv = (double*)(xs + TC * C);
  double* const lam = rinv + D;
  double* const red = lam + lw_max;

  const int tid = threadIdx.x, j = blockIdx.x, f = blockIdx.y;
  const int b0 = (int)min((int64_t)T, (int64_t)j * Lb), b1 = (int)min((int64_t)T, (int64_t)j * Lb + Lb);
  const int w0 = (int)max((int64_t)0, (int64_t)j * Lb - Lc), w1 = (int)min((int64_t)T, (int64_t)j * Lb + Lb + Lc);
  const float2* __restrict__ Yf = Y + f;

  // this thread's tile: rows 4 ti .. 4 ti + 3 of y~ against columns 4 tj .. of y~ (R, tj >= ti) or of y (P)
  const SolveTile tile = solve_tile(tid, NTR, NTR, NCT);
  const int ti = tile.ti, tj = tile.tj;
  const bool is_p = tile.is_p, has_tile = tile.has;
  // offsets into [past | cur] of the tile's operands at the chunk's first frame; a frame further is C elements further.
  // y~(t)[k C + c] lies at past[(t - c0 + K - 1 - k) C + c].  Rows and columns past D (or C) repeat the last one: their
  // accumulators are never stored.
  int offa[4], offb[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int da = min(4 * ti + q, D - 1);
    offa[q] = (K - 1 - da / C) * C + da % C;
    if (is_p) {
      offb[q] = (TC + K - 1) * C + min(4 * tj + q, C - 1);
    } else {
      const int db = min(4 * tj + q, D - 1);
      offb[q] = (K - 1 - db / C) * C + db % C;
    }
  }

  // the chunk [c0, c0 + nfr): its stacked pasts' frames and its own, widened
  auto stage = [&](int c0, int nfr) {
    const int64_t u0 = (int64_t)c0 - delay - K + 1;  // u0 + r <= c0 + nfr - 1 - delay < T
    for (int idx = tid; idx < (nfr + K - 1) * C; idx += NTHR) {
      const int r = idx / C, c = idx - r * C;
      const int64_t u = u0 + r;
      float2 v = make_float2(0.f, 0.f);
      if (u >= 0) v = Yf[c * ycs + u * yrs];
      past[idx] = make_double2((double)v.x, (double)v.y);
    }
    for (int idx = tid; idx < nfr * C; idx += NTHR) {
      const int r = idx / C, c = idx - r * C;
      const float2 v = Yf[c * ycs + (int64_t)(c0 + r) * yrs];
      cur[idx] = make_double2((double)v.x, (double)v.y);
    }
  };
  // x = y - G^H y~ of the staged chunk into xs (x = y with no G yet)
  auto residual = [&](int nfr, bool have_g) {
    for (int idx = tid; idx < nfr * C; idx += NTHR) {
      const int r = idx / C, c = idx - r * C;
      double sr = 0.0, si = 0.0;
      if (have_g) {
        for (int k = 0; k < K; ++k) {
          const double2* __restrict__ yp = past + (r + K - 1 - k) * C;
          const double2* __restrict__ gp = PG + k * C * C + c;
#pragma unroll
          for (int c2 = 0; c2 < C; ++c2) {  // conj(g) y
            const double2 g = gp[c2 * C], y = yp[c2];
            sr += g.x * y.x + g.y * y.y;
            si += g.x * y.y - g.y * y.x;
          }
        }
      }
      const double2 y = cur[idx];
      xs[idx] = make_double2(y.x - sr, y.y - si);
    }
  };

  bool pass = false;
  for (int it = 0; it < iters && !pass; ++it) {
    // ---- pass A: lambda(t) over the window
    for (int c0 = w0; c0 < w1; c0 += TC) {
      const int nfr = min(TC, w1 - c0);
      stage(c0, nfr);
      __syncthreads();
      residual(nfr, it > 0);
      __syncthreads();
      for (int r = tid; r < nfr; r += NTHR) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const double2 x = xs[r * C + c];
          s += x.x * x.x + x.y * x.y;
        }
        lam[c0 - w0 + r] = s / (double)C;
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
      pass = true;
      break;
    }
    for (int t = tid; t < w1 - w0; t += NTHR) lam[t] = 1.0 / fmax(lam[t], WPE_FLOOR * lmax);

    // ---- pass B: the tiles of R and P, t ascending
    double ar[4][4], ai[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) ar[p][q] = ai[p][q] = 0.0;
    for (int c0 = w0; c0 < w1; c0 += TC) {
      const int nfr = min(TC, w1 - c0);
      __syncthreads();  // the chunk before is read; lam is written
      stage(c0, nfr);
      __syncthreads();
      if (has_tile) {
        const double2* __restrict__ base = past;
        for (int r = 0; r < nfr; ++r, base += C) {
          tile_frame(ar, ai, base, offa, offb, lam[c0 - w0 + r]);
        }
      }
    }
    // PG held the previous G, which pass A has finished with
    tile_store(tile, ar, ai, Rt, PG, D, D, C);
    __syncthreads();
    double tr = 0.0;
    for (int a = 0; a < D; ++a) tr += Rt[tri_row(D, a)].x;
    if (tr == 0.0) {  // uniform: every thread adds the same numbers in the same order
      pass = true;
      break;
    }
    __syncthreads();
    const double load = loading * tr / (double)D;
    for (int a = tid; a < D; a += NTHR) Rt[tri_row(D, a)].x += load;

    // ---- R = U^H U, U^H Z = P, U G = Z
    const int bad = cholesky_solve_lds<NTHR>(Rt, PG, rinv, D, C, tid);
    if (__syncthreads_or(bad)) pass = true;
  }

  // ---- the block's own frames
  __syncthreads();
  if (pass) {  // Y's own bits, G = 0
    for (int idx = tid; idx < (b1 - b0) * C; idx += NTHR) {
      const int r = idx / C, c = idx - r * C;
      const float2 v = Yf[c * ycs + (int64_t)(b0 + r) * yrs];
      X[c * xcs + (int64_t)(b0 + r) * xrs + f] = v;
      if (mag && c == ref) mag[(int64_t)(b0 + r) * ldm + f] = (float)sqrt((double)v.x * v.x + (double)v.y * v.y);
    }
    if (Gout)
      for (int idx = tid; idx < D * C; idx += NTHR) Gout[((int64_t)j * NBIN + f) * D * C + idx] = make_double2(0.0, 0.0);
    return;
  }
  for (int c0 = b0; c0 < b1; c0 += TC) {
    const int nfr = min(TC, b1 - c0);
    __syncthreads();
    stage(c0, nfr);
    __syncthreads();
    residual(nfr, true);
    __syncthreads();
    for (int idx = tid; idx < nfr * C; idx += NTHR) {
      const int r = idx / C, c = idx - r * C;
      const float2 v = make_float2((float)xs[idx].x, (float)xs[idx].y);
      X[c * xcs + (int64_t)(c0 + r) * xrs + f] = v;
      if (mag && c == ref) mag[(int64_t)(c0 + r) * ldm + f] = (float)sqrt((double)v.x * v.x + (double)v.y * v.y);
    }
  }
  if (Gout)
    for (int idx = tid; idx < D * C; idx += NTHR) Gout[((int64_t)j * NBIN + f) * D * C + idx] = PG[idx];
}

inline int wpe_tiles(int C, int K) {
  const int ntr = (C * K + 3) / 4;
  return ntr * (ntr + 1) / 2 + ntr * ((C + 3) / 4);
}

}  // namespace

// sk_wpe keeps everything between its passes in LDS
extern "C" size_t sk_wpe_workspace_bytes(int T, int C, int taps, int block_frames, int context_frames) { return 0; }

extern "C" int sk_wpe(const void* Y_c64, int64_t y_chan_stride, int64_t y_row_stride, int T, int C, int taps, int delay, int iterations,
                      int block_frames, int context_frames, int ref, double loading, void* X_c64, int64_t x_chan_stride,
                      int64_t x_row_stride, float* mag_out, int ld_mag, void* G_out_c128, void* ws, sk_stream_t stream) {
  SK_CHECK_ARG(C >= 1 && C <= WPE_MAXC, "sk_wpe: C = %d channels outside 1..%d", C, WPE_MAXC);
  SK_CHECK_ARG(taps >= 1, "sk_wpe: taps = %d, at least 1 expected", taps);
  SK_CHECK_ARG(delay >= 1, "sk_wpe: delay = %d, at least 1 expected", delay);
  SK_CHECK_ARG((int64_t)C * taps <= WPE_MAXD, "sk_wpe: C * taps = %lld above %d", (long long)C * taps, WPE_MAXD);
  SK_CHECK_ARG(iterations >= 1 && iterations <= WPE_MAXIT, "sk_wpe: iterations = %d outside 1..%d", iterations, WPE_MAXIT);
  SK_CHECK_FRAMES("sk_wpe", T);
  SK_CHECK_BLOCK_FRAMES("sk_wpe", block_frames);
  SK_CHECK_WINDOW("sk_wpe", block_frames, context_frames, WPE_MAXWIN);
  SK_CHECK_REF("sk_wpe", ref, C);
  SK_CHECK_LOADING("sk_wpe", loading);
  SK_CHECK_Y_ROW_STRIDE("sk_wpe", y_row_stride);
  SK_CHECK_ARG(x_row_stride >= NBIN, "sk_wpe: x_row_stride = %lld below 257", (long long)x_row_stride);
  SK_CHECK_ARG(!mag_out || ld_mag >= NBIN, "sk_wpe: ld_mag = %d below 257", ld_mag);
  SK_CHECK_ARG(Y_c64 && X_c64, "sk_wpe: null pointer (Y or X)");
  const float2* Y = (const float2*)Y_c64;
  float2* X = (float2*)X_c64;
  double2* G = (double2*)G_out_c128;
  const int K = taps, Lb = block_frames, Lc = context_frames;
  const int nblk = (int)sk_cdiv(T, Lb), lw = (int)min((int64_t)T, (int64_t)Lb + 2 * (int64_t)Lc);
  return sk_dispatch_int<1, WPE_MAXC>(C, [&](auto c) {
    constexpr int Cc = decltype(c)::value;
    auto launch = [&](auto kernel, int nthr) {
      return sk_launch_lds("sk_wpe", "wpe_kernel", kernel, dim3((unsigned)nblk, NBIN), dim3(nthr), wpe_lds_bytes(Cc, K, lw), WPE_LDS_LIMIT,
                           (hipStream_t)stream, Y, y_chan_stride, y_row_stride, T, K, delay, iterations, Lb, Lc, ref, loading, lw, X,
                           x_chan_stride, x_row_stride, mag_out, ld_mag, G);
    };
    // a wave is enough while every tile has a thread in it
    return wpe_tiles(Cc, K) <= 64 ? launch(wpe_kernel<Cc, 64>, 64) : launch(wpe_kernel<Cc, 256>, 256);
  });
}
