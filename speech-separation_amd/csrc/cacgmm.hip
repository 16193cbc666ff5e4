// cacgmm.hip -- mask-guided spatial clustering of a multi-channel recording with a cACGMM (sk_cacgmm).
//
// No counterpart in the reference, which works on one close-talk channel; sepkern/cacgmm.py states the definition (per block of
// frames and bin, on a window around the block: the directions z = y / |y| of the frames are clustered into one complex angular
// central Gaussian per stream, with the network's masks as the class prior of every frame; q_k = z^H B_k^-1 z by an fp64
// Cholesky factor and a forward substitution, the posteriors gamma by a softmax, B_k' = C sum gamma_k / q_k z z^H / sum gamma_k)
// and restates it in numpy.  One launch, one workgroup per (block, bin), as in wpe.hip: the problems are independent, so there
// are no atomics, no hand-off between workgroups and no workspace, and every sum has one order whatever the strides.
//
// A workgroup keeps in LDS the state B_k and its factor U_k of every class (K C^2 complex128 each, at most 4 KB), 1 / diag U,
// sum log diag U, and a chunk of TC frames of its bin: the directions in fp64, the priors, and per (frame, class) l, q,
// gamma / q and gamma.  gamma and q of a window of up to 4096 frames do not fit, and they need not: the update takes q from the
// OLD state, so an iteration walks the window's chunks once, each chunk through
//   pass A   the frames' norms and directions (threads over frames), the K forward substitutions, q and l (threads over
//            (frame, class)), the softmax (threads over frames)
//   pass B   every thread owns one entry (k, a, b) of the upper triangles of the S_k, or one n_k, on registers and adds its
//            chunk frame by frame, t ascending
// then B' = S C / n, the trace and the loading follow, and the factorisation runs right-looking over the workgroup with one
// barrier per pivot (wpe.hip's scheme: the pivot row stays unscaled while its step reads it).  A last walk over the block's own
// frames is pass A alone and writes the posteriors.  The operations and their order are sepkern/cacgmm.py's, one rounding
// each -- no multiply is fused into an add in this file -- so that B comes out of a step within a few units in the last place
// of numpy's: what differs is the device library's log and exp.  With one entry per thread pass B reads three LDS words for
// eight operations and at C = 2, K = 2 eight of 256 threads have an entry; the kernel is small beside sk_wpe in the same
// chain (profiles/cacgmm.txt).
#include "sk_common.h"

// sepkern/cacgmm.py states every operation with a rounding of its own: no product is fused into a sum here
#pragma clang fp contract(off)

namespace {

constexpr int NBIN = 257;
constexpr int CG_MINC = 2, CG_MAXC = 8, CG_MINS = 2, CG_MAXS = 4, CG_MAXIT = 16, CG_MAXWIN = 4096;
constexpr int CG_TC = 64;     // frames per chunk
constexpr int CG_NTHR = 256;  // >= CG_MAXS * (CG_MAXC (CG_MAXC + 1) / 2 + 1) accumulators, >= CG_TC * CG_MAXS items of pass A
constexpr double CG_PRIOR_FLOOR = 1e-6;

template <int C>
__global__ __launch_bounds__(CG_NTHR) void cacgmm_kernel(const float2* __restrict__ Y, int64_t ycs, int64_t yrs,
                                                         const float* __restrict__ prior, int ldp, int T, int K, int iters, int Lb,
                                                         int Lc, double loading, const double2* __restrict__ Bin,
                                                         float* __restrict__ out, int ldo, double2* __restrict__ Bout) {
  constexpr int TC = CG_TC, KM = CG_MAXS, NT = C * (C + 1) / 2, CC = C * C;
  __shared__ double2 Bs[KM * CC];  // the state: upper triangles, real diagonals
  __shared__ double2 Us[KM * CC];  // its factor: strictly upper part, scaled
  __shared__ double2 zs[TC * C];
  __shared__ double rinv[KM * C], piv[KM * C], sld[KM], nk[KM];
  __shared__ double ps[TC * KM], ls[TC * KM], qs[TC * KM], gq[TC * KM], gm[TC * KM];
  __shared__ int live[TC], identk[KM];

  const int tid = threadIdx.x, j = blockIdx.x, f = blockIdx.y;
  const int b0 = (int)min((int64_t)T, (int64_t)j * Lb), b1 = (int)min((int64_t)T, (int64_t)j * Lb + Lb);
  const int w0 = (int)max((int64_t)0, (int64_t)j * Lb - Lc), w1 = (int)min((int64_t)T, (int64_t)j * Lb + Lb + Lc);
  const float2* __restrict__ Yf = Y + f;
  const float* __restrict__ pf = prior + f;

  // this thread's accumulator: entry (ea, eb) of class ek's upper triangle, or n of class ek
  int ek = 0, ea = 0, eb = 0;
  const bool has_s = tid < K * NT, has_n = !has_s && tid < K * NT + K;
  if (has_s) {
    ek = tid / NT;
    int e = tid - ek * NT;
    while (e >= C - ea) {
      e -= C - ea;
      ++ea;
    }
    eb = ea + e;
  } else if (has_n) {
    ek = tid - K * NT;
  }

  // ---- admission of the state in Bs: factorise, reset the classes that fail (or whose n is zero) to the identity
  bool ident = false;
  auto admit = [&](bool check_n) {
    for (int idx = tid; idx < K * CC; idx += CG_NTHR) Us[idx] = Bs[idx];
    for (int a = 0; a < C; ++a) {
      __syncthreads();
      const int m = C - 1 - a;
      for (int idx = tid; idx < K * m * m; idx += CG_NTHR) {
        const int k = idx / (m * m), rem = idx - k * m * m, ii = rem / m, bb = rem - ii * m;
        if (bb < ii) continue;
        const double2* __restrict__ rowa = Us + k * CC + a * C;  // U[a][b] = B[a][b] / U[a][a], formed where it is used
        const double ri = 1.0 / sqrt(rowa[a].x);
        const double uar = rowa[a + 1 + ii].x * ri, uai = rowa[a + 1 + ii].y * ri, ubr = rowa[a + 1 + bb].x * ri, ubi = rowa[a + 1 + bb].y * ri;
        double2* e = Us + k * CC + (a + 1 + ii) * C + (a + 1 + bb);
        double2 v = *e;
        v.x -= uar * ubr + uai * ubi;  // conj(ua) ub; on the diagonal |ua|^2, and the imaginary part is never read
        v.y -= uar * ubi - uai * ubr;
        *e = v;
      }
      if (tid < K) {  // row a is not written in its own step
        const double d = Us[tid * CC + a * C + a].x;
        piv[tid * C + a] = d;
        rinv[tid * C + a] = 1.0 / sqrt(d);
      }
    }
    __syncthreads();
    for (int idx = tid; idx < K * CC; idx += CG_NTHR) {
      const int k = idx / CC, rem = idx - k * CC, a = rem / C, b = rem - a * C;
      if (b > a) {
        const double ri = rinv[k * C + a];
        Us[idx] = make_double2(Us[idx].x * ri, Us[idx].y * ri);
      }
    }
    __syncthreads();
    if (tid < K) {
      const int k = tid;
      bool ok = true;
      double s = 0.0;
      for (int a = 0; a < C; ++a) {
        const double d = piv[k * C + a];
        ok = ok && d > 0.0 && isfinite(d);
        s = s + log(sqrt(d));
        for (int b = a + 1; b < C; ++b) ok = ok && isfinite(Us[k * CC + a * C + b].x) && isfinite(Us[k * CC + a * C + b].y);
      }
      if (!ok || (check_n && nk[k] == 0.0)) {
        for (int a = 0; a < C; ++a) {
          for (int b = 0; b < C; ++b) {
            Bs[k * CC + a * C + b] = make_double2(a == b ? 1.0 : 0.0, 0.0);
            Us[k * CC + a * C + b] = make_double2(0.0, 0.0);
          }
          rinv[k * C + a] = 1.0;
        }
        s = 0.0;
      }
      sld[k] = s;
      int id = 1;
      for (int a = 0; a < C; ++a)
        for (int b = a; b < C; ++b) {
          const double2 v = Bs[k * CC + a * C + b];
          id &= (v.x == (a == b ? 1.0 : 0.0)) && (b == a || v.y == 0.0);
        }
      identk[k] = id;
    }
    __syncthreads();
    ident = true;
    for (int k = 0; k < K; ++k) ident = ident && identk[k] != 0;
  };

  // ---- pass A of the chunk [c0, c0 + nfr): zs, live, and per (frame, class) ls = gamma, gq = gamma / q, gm = gamma, the last
  // two zero on dead frames
  auto pass_a = [&](int c0, int nfr) {
    for (int idx = tid; idx < nfr * C; idx += CG_NTHR) {
      const int r = idx / C, c = idx - r * C;
      const float2 v = Yf[c * ycs + (int64_t)(c0 + r) * yrs];
      zs[idx] = make_double2((double)v.x, (double)v.y);
    }
    for (int idx = tid; idx < nfr * K; idx += CG_NTHR) {
      const int r = idx / K, k = idx - r * K;
      ps[r * KM + k] = fmax((double)pf[(int64_t)(c0 + r) * ldp + k * NBIN], CG_PRIOR_FLOOR);
    }
    __syncthreads();
    if (tid < nfr) {
      const int r = tid;
      double n = 0.0;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const double2 y = zs[r * C + c];
        n = n + (y.x * y.x + y.y * y.y);
      }
      const bool lv = n != 0.0;
      const double s = sqrt(lv ? n : 1.0);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const double2 y = zs[r * C + c];
        zs[r * C + c] = lv ? make_double2(y.x / s, y.y / s) : make_double2(0.0, 0.0);
      }
      live[r] = lv;
      double tot = 0.0;
      for (int k = 0; k < K; ++k) tot = tot + ps[r * KM + k];
      for (int k = 0; k < K; ++k) ps[r * KM + k] = ps[r * KM + k] / tot;
    }
    __syncthreads();
    if (!ident) {
      for (int idx = tid; idx < nfr * K; idx += CG_NTHR) {
        const int r = idx / K, k = idx - r * K;
        if (!live[r]) continue;
        const double2* __restrict__ U = Us + k * CC;
        double xr[C], xi[C], q = 0.0;
#pragma unroll
        for (int a = 0; a < C; ++a) {
          double vr = zs[r * C + a].x, vi = zs[r * C + a].y;
#pragma unroll
          for (int i = 0; i < a; ++i) {  // - conj(U[i][a]) x[i]
            const double2 u = U[i * C + a];
            vr -= u.x * xr[i] + u.y * xi[i];
            vi -= u.x * xi[i] - u.y * xr[i];
          }
          const double ri = rinv[k * C + a];
          xr[a] = vr * ri;
          xi[a] = vi * ri;
          q = q + (xr[a] * xr[a] + xi[a] * xi[a]);
        }
        qs[r * KM + k] = q;
        ls[r * KM + k] = (log(ps[r * KM + k]) - 2.0 * sld[k]) - (double)C * log(q);
      }
    }
    __syncthreads();
    if (tid < nfr) {
      const int r = tid;
      const bool lv = live[r] != 0;
      if (!lv || ident) {  // gamma = p, q = 1
        for (int k = 0; k < K; ++k) {
          const double p = ps[r * KM + k];
          ls[r * KM + k] = p;
          gq[r * KM + k] = gm[r * KM + k] = lv ? p : 0.0;
        }
      } else {
        double lmax = ls[r * KM];
        for (int k = 1; k < K; ++k) lmax = fmax(lmax, ls[r * KM + k]);
        double tot = 0.0;
        for (int k = 0; k < K; ++k) {
          const double e = exp(ls[r * KM + k] - lmax);
          ls[r * KM + k] = e;
          tot = tot + e;
        }
        for (int k = 0; k < K; ++k) {
          const double g = ls[r * KM + k] / tot;
          ls[r * KM + k] = g;
          gm[r * KM + k] = g;
          gq[r * KM + k] = g / qs[r * KM + k];
        }
      }
    }
    __syncthreads();
  };

  // ---- the initial state
  for (int idx = tid; idx < K * CC; idx += CG_NTHR) {
    const int k = idx / CC, rem = idx - k * CC, a = rem / C, b = rem - a * C;
    double2 v = make_double2(a == b ? 1.0 : 0.0, 0.0);
    if (Bin && a <= b) {
      v = Bin[(((int64_t)j * K + k) * NBIN + f) * CC + rem];
      if (a == b) v.y = 0.0;
    }
    Bs[idx] = v;
  }
  __syncthreads();
  admit(false);

  for (int it = 0; it < iters; ++it) {
    double ar = 0.0, ai = 0.0;
    for (int c0 = w0; c0 < w1; c0 += TC) {
      const int nfr = min(TC, w1 - c0);
      pass_a(c0, nfr);
      // ---- pass B: t ascending; a dead frame adds zeros
      if (has_s) {
        for (int r = 0; r < nfr; ++r) {
          const double w = gq[r * KM + ek];
          const double2 a = zs[r * C + ea], b = zs[r * C + eb];
          const double pr = a.x * w, pi = a.y * w;
          ar += pr * b.x + pi * b.y;  // (w z_a) conj(z_b)
          ai += pi * b.x - pr * b.y;
        }
      } else if (has_n) {
        for (int r = 0; r < nfr; ++r) ar += gm[r * KM + ek];
      }
      __syncthreads();  // the chunk is read
    }
    if (has_n) nk[ek] = ar;
    __syncthreads();
    if (has_s) {
      const double cs = (double)C / nk[ek];
      Bs[ek * CC + ea * C + eb] = make_double2(ar * cs, ea == eb ? 0.0 : ai * cs);
    }
    __syncthreads();
    if (tid < K) {
      double tr = 0.0;
      for (int a = 0; a < C; ++a) tr = tr + Bs[tid * CC + a * C + a].x;
      const double load = loading * tr / (double)C;
      for (int a = 0; a < C; ++a) Bs[tid * CC + a * C + a].x = Bs[tid * CC + a * C + a].x + load;
    }
    __syncthreads();
    admit(true);
  }

  // ---- the block's own frames
  for (int c0 = b0; c0 < b1; c0 += TC) {
    const int nfr = min(TC, b1 - c0);
    pass_a(c0, nfr);
    for (int idx = tid; idx < nfr * K; idx += CG_NTHR) {
      const int r = idx / K, k = idx - r * K;
      out[(int64_t)(c0 + r) * ldo + k * NBIN + f] = (float)ls[r * KM + k];
    }
    __syncthreads();
  }
  if (Bout)
    for (int idx = tid; idx < K * CC; idx += CG_NTHR) {
      const int k = idx / CC, rem = idx - k * CC, a = rem / C, b = rem - a * C;
      double2 v = a <= b ? Bs[idx] : Bs[k * CC + b * C + a];
      if (a > b) v.y = -v.y;
      Bout[(((int64_t)j * K + k) * NBIN + f) * CC + rem] = v;
    }
}

}  // namespace

// sk_cacgmm keeps everything between its passes in LDS
extern "C" size_t sk_cacgmm_workspace_bytes(int T, int C, int S, int block_frames, int context_frames) { return 0; }

extern "C" int sk_cacgmm(const void* Y_c64, int64_t y_chan_stride, int64_t y_row_stride, const float* prior, int ld_prior, int T, int C,
                         int S, int iterations, int block_frames, int context_frames, double loading, const void* B_in_c128,
                         float* mask_out, int ld_out, void* B_out_c128, void* ws, sk_stream_t stream) {
  SK_CHECK_ARG(C >= CG_MINC && C <= CG_MAXC, "sk_cacgmm: C = %d channels outside %d..%d", C, CG_MINC, CG_MAXC);
  SK_CHECK_ARG(S >= CG_MINS && S <= CG_MAXS, "sk_cacgmm: S = %d streams outside %d..%d", S, CG_MINS, CG_MAXS);
  SK_CHECK_FRAMES("sk_cacgmm", T);
  SK_CHECK_ARG(iterations >= 0 && iterations <= CG_MAXIT, "sk_cacgmm: iterations = %d outside 0..%d", iterations, CG_MAXIT);
  SK_CHECK_BLOCK_FRAMES("sk_cacgmm", block_frames);
  SK_CHECK_WINDOW("sk_cacgmm", block_frames, context_frames, CG_MAXWIN);
  SK_CHECK_LOADING("sk_cacgmm", loading);
  SK_CHECK_ARG(ld_prior >= S * NBIN, "sk_cacgmm: ld_prior = %d below S*257 = %d", ld_prior, S * NBIN);
  SK_CHECK_ARG(ld_out >= S * NBIN, "sk_cacgmm: ld_out = %d below S*257 = %d", ld_out, S * NBIN);
  SK_CHECK_Y_ROW_STRIDE("sk_cacgmm", y_row_stride);
  SK_CHECK_ARG(Y_c64 && prior && mask_out, "sk_cacgmm: null pointer (Y, prior or mask_out)");
  const float2* Y = (const float2*)Y_c64;
  const double2* Bi = (const double2*)B_in_c128;
  double2* Bo = (double2*)B_out_c128;
  const int nblk = (int)sk_cdiv(T, block_frames);
  return sk_dispatch_int<CG_MINC, CG_MAXC>(C, [&](auto c) {
    hipLaunchKernelGGL((cacgmm_kernel<decltype(c)::value>), dim3((unsigned)nblk, NBIN), dim3(CG_NTHR), 0, (hipStream_t)stream, Y,
                       y_chan_stride, y_row_stride, prior, ld_prior, T, S, iterations, block_frames, context_frames, loading, Bi, mask_out,
                       ld_out, Bo);
    SK_CHECK_LAUNCH("cacgmm_kernel");
    return SK_OK;
  });
}
