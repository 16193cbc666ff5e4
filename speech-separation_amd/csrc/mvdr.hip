// mvdr.hip -- mask-based MVDR beamforming of a multi-channel recording (sk_mvdr).
//
// No counterpart in the reference, which works on one channel; sepkern/mvdr.py states the definition (mask-weighted spatial
// covariance matrices per block of frames, summed over a context of blocks; Souden's reference-channel MVDR weights from an
// fp64 Cholesky solve; the weights applied per frame) and restates it in numpy.  Three streaming launches on one stream, no
// atomics, no hand-off between workgroups, no host synchronisation:
//   mvdr_stats_kernel    block x group of 64 bins, one wave per PART of the upper triangle (rows p and C-1-p: C + 1 entries, the
//                        middle row of an odd C alone): the products y_a conj(y_b) of a (t, f) formed once in fp64 and weighted
//                        into the S accumulators, frames ascending; the triangle of (block, s, f) goes to the workspace, bins
//                        innermost.  Bin 256 has a wave of its own: its lanes take the block's frames 64 apart and are added
//                        by a fixed butterfly.
//   mvdr_weights_kernel  block x group of 64 bins, one wave per stream s: the context's partials added in ascending order (PHI_s,
//                        on registers), the other streams' rows through LDS (N_s, s' ascending), the loading, the Cholesky
//                        factorisation N = U^H U and the C solves, fully unrolled on registers; the fallback rule; complex64 out
//   mvdr_apply_kernel    64 frames of one block x group of 64 bins: a thread keeps the S x C weights of its bin on registers
//                        and walks its wave's frames; every element of Z is written once
// Bins are the coalesced dimension in all three: the rows of Y, of the mask and of Z are frame-major.
#include "sk_common.h"

namespace {

constexpr int NBIN = 257;
constexpr int NGRP = 5;        // groups of 64 bins: four full ones and bin 256
constexpr int MINC = 2, MAXC = 8, MINS = 2;
constexpr int AFR = 64;        // frames per workgroup of the apply launch
constexpr double D_MIN = 1e-12;

constexpr int tri_count(int C) { return C * (C + 1) / 2; }
// index of entry (a, b), a <= b, of the upper triangle stored row by row
constexpr int tri_index(int C, int a, int b) { return a * C - a * (a - 1) / 2 + (b - a); }
constexpr int stats_parts(int C) { return (C + 1) / 2; }

// One row of the triangle for one (t, f): the products y_a conj(y_b), b >= a, weighted into the S accumulators of the row.
// Accumulator layout of a row: [s][0] the (real) diagonal, [s][1 + 2 k], [s][2 + 2 k] the entry (a, a + 1 + k).
template <int C, int S, int A>
__device__ __forceinline__ void stats_row(const double (&yr)[C], const double (&yi)[C], const double (&m)[S],
                                          double (&acc)[S][2 * (C - A) - 1]) {
  const double dg = yr[A] * yr[A] + yi[A] * yi[A];
#pragma unroll
  for (int s = 0; s < S; ++s) acc[s][0] += m[s] * dg;
#pragma unroll
  for (int b = A + 1; b < C; ++b) {
    const double pr = yr[A] * yr[b] + yi[A] * yi[b];
    const double pi = yi[A] * yr[b] - yr[A] * yi[b];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      acc[s][1 + 2 * (b - A - 1)] += m[s] * pr;
      acc[s][2 + 2 * (b - A - 1)] += m[s] * pi;
    }
  }
}

template <int C, int S, int A>
__device__ __forceinline__ void stats_store_row(double (&acc)[S][2 * (C - A) - 1], bool spread, int f,
                                                double* __restrict__ dst /* (S, NP, 2, NBIN) of the block */) {
  constexpr int NP = tri_count(C);
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int q = 0; q < 2 * (C - A) - 1; ++q) {
      double v = acc[s][q];
      if (spread) {  // wave-uniform: the lanes hold frames 64 apart of ONE bin
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      }
      const int e = tri_index(C, A, A + (q + 1) / 2), ri = q == 0 ? 0 : 1 - (q & 1);
      if (!spread || (threadIdx.x & 63) == 0) dst[((int64_t)(s * NP + e) * 2 + ri) * NBIN + f] = v;
    }
}

template <int C, int S, int P>
__device__ __forceinline__ void stats_part(const float2* __restrict__ Y, int64_t ycs, int64_t yrs,
                                           const float* __restrict__ mask, int ld, int t0, int t1, int tstep, int f, bool spread,
                                           double* __restrict__ dst) {
  constexpr int A0 = P, A1 = C - 1 - P;  // A1 >= A0; equal for the middle row of an odd C
  double acc0[S][2 * (C - A0) - 1], acc1[S][2 * (C - A1) - 1];
#pragma unroll
  for (int s = 0; s < S; ++s) {
#pragma unroll
    for (int q = 0; q < 2 * (C - A0) - 1; ++q) acc0[s][q] = 0.0;
#pragma unroll
    for (int q = 0; q < 2 * (C - A1) - 1; ++q) acc1[s][q] = 0.0;
  }
#pragma unroll 2
  for (int t = t0; t < t1; t += tstep) {
    double yr[C], yi[C], m[S];
#pragma unroll
    for (int c = A0; c < C; ++c) {  // channels below A0 enter neither row
      const float2 v = Y[c * ycs + (int64_t)t * yrs + f];
      yr[c] = (double)v.x;
      yi[c] = (double)v.y;
    }
#pragma unroll
    for (int s = 0; s < S; ++s) m[s] = (double)mask[(int64_t)t * ld + s * NBIN + f];
    stats_row<C, S, A0>(yr, yi, m, acc0);
    if (A1 != A0) stats_row<C, S, A1>(yr, yi, m, acc1);
  }
  stats_store_row<C, S, A0>(acc0, spread, f, dst);
  if (A1 != A0) stats_store_row<C, S, A1>(acc1, spread, f, dst);
}

template <int C, int S>
__global__ __launch_bounds__(64 * stats_parts(C)) void mvdr_stats_kernel(const float2* __restrict__ Y, int64_t ycs, int64_t yrs,
                                                                        const float* __restrict__ mask, int ld, int T, int Lb,
                                                                        double* __restrict__ part /* (nblk, S, NP, 2, NBIN) */) {
  const int j = blockIdx.x, g = blockIdx.y, lane = threadIdx.x;
  const bool spread = g == NGRP - 1;
  const int b0 = (int)min((int64_t)T, (int64_t)j * Lb), b1 = (int)min((int64_t)T, (int64_t)j * Lb + Lb);
  const int f = spread ? NBIN - 1 : g * 64 + lane;
  const int t0 = spread ? b0 + lane : b0, tstep = spread ? 64 : 1;
  double* __restrict__ dst = part + (int64_t)j * S * tri_count(C) * 2 * NBIN;
  switch (threadIdx.y) {  // wave-uniform
    case 0: stats_part<C, S, 0>(Y, ycs, yrs, mask, ld, t0, b1, tstep, f, spread, dst); break;
    case 1: if constexpr (stats_parts(C) > 1) stats_part<C, S, 1>(Y, ycs, yrs, mask, ld, t0, b1, tstep, f, spread, dst); break;
    case 2: if constexpr (stats_parts(C) > 2) stats_part<C, S, 2>(Y, ycs, yrs, mask, ld, t0, b1, tstep, f, spread, dst); break;
    default: if constexpr (stats_parts(C) > 3) stats_part<C, S, 3>(Y, ycs, yrs, mask, ld, t0, b1, tstep, f, spread, dst); break;
  }
}

// The weights of one (block, s, f): thread (lane = bin, y = s).  Every loop below is unrolled and every index a constant, so the
// two triangles stay on registers.
template <int C, int S>
__global__ __launch_bounds__(64 * S) void mvdr_weights_kernel(const double* __restrict__ part, int nblk, int R, int ref,
                                                             double loading, float2* __restrict__ weights /* (nblk, S, NBIN, C) */,
                                                             double2* __restrict__ scm /* (nblk, S, NBIN, C, C) or NULL */) {
  constexpr int NP = tri_count(C);
  __shared__ double row[S][2 * C][64];  // one row of every stream's PHI
  const int j = blockIdx.x, lane = threadIdx.x, s = threadIdx.y;
  const int f = blockIdx.y * 64 + lane;
  const bool live = f < NBIN;
  const int fc = live ? f : NBIN - 1;  // idle lanes of the last group compute bin 256 again and store nothing
  const int lo = max(0, (int)max((int64_t)j - R, (int64_t)0)), hi = (int)min((int64_t)nblk - 1, (int64_t)j + R);

  double pr[NP], pi[NP];  // PHI_s, upper triangle
#pragma unroll
  for (int e = 0; e < NP; ++e) pr[e] = pi[e] = 0.0;
  for (int jj = lo; jj <= hi; ++jj) {
    const double* __restrict__ src = part + ((int64_t)jj * S + s) * NP * 2 * NBIN + fc;
#pragma unroll
    for (int a = 0; a < C; ++a)
#pragma unroll
      for (int b = a; b < C; ++b) {
        const int e = tri_index(C, a, b);
        pr[e] += src[(int64_t)(2 * e) * NBIN];
        if (b > a) pi[e] += src[(int64_t)(2 * e + 1) * NBIN];
      }
  }
  if (scm && live) {
    double2* __restrict__ o = scm + (((int64_t)j * S + s) * NBIN + f) * C * C;
#pragma unroll
    for (int a = 0; a < C; ++a)
#pragma unroll
      for (int b = 0; b < C; ++b) {
        const int e = a <= b ? tri_index(C, a, b) : tri_index(C, b, a);
        o[a * C + b] = make_double2(pr[e], a == b ? 0.0 : a < b ? pi[e] : -pi[e]);
      }
  }

  double nr[NP], ni[NP];  // N_s, then U
#pragma unroll
  for (int a = 0; a < C; ++a) {
    __syncthreads();
#pragma unroll
    for (int b = a; b < C; ++b) {
      row[s][2 * (b - a)][lane] = pr[tri_index(C, a, b)];
      row[s][2 * (b - a) + 1][lane] = pi[tri_index(C, a, b)];
    }
    __syncthreads();
#pragma unroll
    for (int b = a; b < C; ++b) {
      double vr = 0.0, vi = 0.0;
#pragma unroll
      for (int o = 0; o < S; ++o)
        if (o != s) {
          vr += row[o][2 * (b - a)][lane];
          vi += row[o][2 * (b - a) + 1][lane];
        }
      nr[tri_index(C, a, b)] = vr;
      ni[tri_index(C, a, b)] = vi;
    }
  }
  double trp = 0.0, trn = 0.0;
#pragma unroll
  for (int a = 0; a < C; ++a) {
    trp += pr[tri_index(C, a, a)];
    trn += nr[tri_index(C, a, a)];
  }
  const double load = loading * trn / C;
#pragma unroll
  for (int a = 0; a < C; ++a) nr[tri_index(C, a, a)] += load;

  // N = U^H U, U upper triangular, in place; rinv = 1 / diag U.  A matrix that is not positive definite gives NaN, which the
  // test on d below turns into the fallback.
  double rinv[C];
#pragma unroll
  for (int a = 0; a < C; ++a) {
    double dd = nr[tri_index(C, a, a)];
#pragma unroll
    for (int k = 0; k < a; ++k) {
      const int e = tri_index(C, k, a);
      dd -= nr[e] * nr[e] + ni[e] * ni[e];
    }
    rinv[a] = 1.0 / sqrt(dd);
#pragma unroll
    for (int b = a + 1; b < C; ++b) {
      double vr = nr[tri_index(C, a, b)], vi = ni[tri_index(C, a, b)];
#pragma unroll
      for (int k = 0; k < a; ++k) {  // - conj(U[k][a]) U[k][b]
        const int ea = tri_index(C, k, a), eb = tri_index(C, k, b);
        vr -= nr[ea] * nr[eb] + ni[ea] * ni[eb];
        vi -= nr[ea] * ni[eb] - ni[ea] * nr[eb];
      }
      nr[tri_index(C, a, b)] = vr * rinv[a];
      ni[tri_index(C, a, b)] = vi * rinv[a];
    }
  }

  // column k of G = N^-1 PHI: U^H z = PHI[:, k], then U g = z from the last row up -- to row k for the trace, to row 0 for k == ref
  double d = 0.0, wr[C], wi[C];
#pragma unroll
  for (int c = 0; c < C; ++c) wr[c] = wi[c] = 0.0;
#pragma unroll
  for (int k = 0; k < C; ++k) {
    double zr[C], zi[C], gr[C], gi[C];
#pragma unroll
    for (int a = 0; a < C; ++a) {
      double vr = a <= k ? pr[tri_index(C, a, k)] : pr[tri_index(C, k, a)];
      double vi = a == k ? 0.0 : a < k ? pi[tri_index(C, a, k)] : -pi[tri_index(C, k, a)];
#pragma unroll
      for (int i = 0; i < a; ++i) {  // - conj(U[i][a]) z[i]
        const int e = tri_index(C, i, a);
        vr -= nr[e] * zr[i] + ni[e] * zi[i];
        vi -= nr[e] * zi[i] - ni[e] * zr[i];
      }
      zr[a] = vr * rinv[a];
      zi[a] = vi * rinv[a];
    }
#pragma unroll
    for (int a = C - 1; a >= 0; --a) {
      if (a >= k || k == ref) {  // rows below k only for the reference column (uniform over the workgroup)
        double vr = zr[a], vi = zi[a];
#pragma unroll
        for (int i = a + 1; i < C; ++i) {  // - U[a][i] g[i]
          const int e = tri_index(C, a, i);
          vr -= nr[e] * gr[i] - ni[e] * gi[i];
          vi -= nr[e] * gi[i] + ni[e] * gr[i];
        }
        gr[a] = vr * rinv[a];
        gi[a] = vi * rinv[a];
      }
    }
    d += gr[k];
    if (k == ref) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        wr[c] = gr[c];
        wi[c] = gi[c];
      }
    }
  }

  const bool fallback = trp == 0.0 || trn == 0.0 || !(d > D_MIN);
  if (live) {
    float2* __restrict__ w = weights + (((int64_t)j * S + s) * NBIN + f) * C;
#pragma unroll
    for (int c = 0; c < C; ++c)
      w[c] = fallback ? make_float2(c == ref ? 1.f : 0.f, 0.f) : make_float2((float)(wr[c] / d), (float)(wi[c] / d));
  }
}

template <int C, int S>
__global__ __launch_bounds__(256) void mvdr_apply_kernel(const float2* __restrict__ Y, int64_t ycs, int64_t yrs,
                                                         const float2* __restrict__ weights, int T, int Lb, int chunks,
                                                         float2* __restrict__ Z /* (S, T, NBIN) */) {
  const int j = blockIdx.x / chunks, ch = blockIdx.x - j * chunks;
  const int f = blockIdx.y * 64 + (threadIdx.x & 63), wave = threadIdx.x >> 6;
  if (f >= NBIN) return;
  const int64_t b0 = (int64_t)j * Lb + (int64_t)ch * AFR;
  const int t0 = (int)min((int64_t)T, b0), t1 = (int)min(min((int64_t)T, b0 + AFR), (int64_t)j * Lb + Lb);
  float wr[S][C], wi[S][C];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const float2* __restrict__ w = weights + (((int64_t)j * S + s) * NBIN + f) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      wr[s][c] = w[c].x;
      wi[s][c] = w[c].y;
    }
  }
  for (int t = t0 + wave; t < t1; t += 4) {
    float yr[C], yi[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float2 v = Y[c * ycs + (int64_t)t * yrs + f];
      yr[c] = v.x;
      yi[c] = v.y;
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
      float zr = 0.f, zi = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {  // conj(w) y, c ascending
        zr = fmaf(wr[s][c], yr[c], zr);
        zr = fmaf(wi[s][c], yi[c], zr);
        zi = fmaf(wr[s][c], yi[c], zi);
        zi = fmaf(-wi[s][c], yr[c], zi);
      }
      Z[((int64_t)s * T + t) * NBIN + f] = make_float2(zr, zi);
    }
  }
}

inline bool mvdr_shape_ok(int T, int C, int S, int Lb) {
  return C >= MINC && C <= MAXC && S >= MINS && S <= SK_MAXS && T >= 1 && Lb >= 1 && sk_cdiv(Lb, AFR) * sk_cdiv(T, Lb) <= 2147483647;
}

template <int C, int S>
int mvdr_launch(const float2* Y, int64_t ycs, int64_t yrs, const float* mask, int ld, int T, int Lb, int R, int ref, double loading,
                float2* weights, float2* Z, double2* scm, double* part, hipStream_t st) {
  const int nblk = (int)sk_cdiv(T, Lb), chunks = (int)sk_cdiv(min(Lb, T), AFR);
  hipLaunchKernelGGL((mvdr_stats_kernel<C, S>), dim3((unsigned)nblk, NGRP), dim3(64, stats_parts(C)), 0, st, Y, ycs, yrs, mask, ld, T, Lb, part);
  SK_CHECK_LAUNCH("mvdr_stats_kernel");
  hipLaunchKernelGGL((mvdr_weights_kernel<C, S>), dim3((unsigned)nblk, NGRP), dim3(64, S), 0, st, (const double*)part, nblk, R, ref, loading,
                     weights, scm);
  SK_CHECK_LAUNCH("mvdr_weights_kernel");
  hipLaunchKernelGGL((mvdr_apply_kernel<C, S>), dim3((unsigned)(nblk * chunks), NGRP), dim3(256), 0, st, Y, ycs, yrs, (const float2*)weights, T, Lb,
                     chunks, Z);
  SK_CHECK_LAUNCH("mvdr_apply_kernel");
  return SK_OK;
}

}  // namespace

// [block statistics (nblk, S, C (C + 1) / 2, 2, 257) fp64]
extern "C" size_t sk_mvdr_workspace_bytes(int T, int C, int S, int block_frames) {
  if (!mvdr_shape_ok(T, C, S, block_frames)) return 0;
  return sk_align((size_t)sk_cdiv(T, block_frames) * S * tri_count(C) * 2 * NBIN * sizeof(double), 256);
}

extern "C" int sk_mvdr(const void* Y_c64, int64_t y_chan_stride, int64_t y_row_stride, const float* mask, int ld_mask, int T, int C,
                       int S, int block_frames, int context_blocks, int ref, double loading, void* weights_c64, void* Z_c64,
                       void* scm_out_c128, void* ws, sk_stream_t stream) {
  SK_CHECK_ARG(C >= MINC && C <= MAXC, "sk_mvdr: C = %d channels outside %d..%d", C, MINC, MAXC);
  SK_CHECK_ARG(S >= MINS && S <= SK_MAXS, "sk_mvdr: S = %d streams outside %d..%d", S, MINS, SK_MAXS);
  SK_CHECK_FRAMES("sk_mvdr", T);
  SK_CHECK_BLOCK_FRAMES("sk_mvdr", block_frames);
  SK_CHECK_ARG(context_blocks >= 0, "sk_mvdr: context_blocks = %d is negative", context_blocks);
  SK_CHECK_REF("sk_mvdr", ref, C);
  SK_CHECK_LOADING("sk_mvdr", loading);
  SK_CHECK_LD_MASK("sk_mvdr", ld_mask, S);
  SK_CHECK_Y_ROW_STRIDE("sk_mvdr", y_row_stride);
  SK_CHECK_ARG(mvdr_shape_ok(T, C, S, block_frames), "sk_mvdr: T = %d frames in blocks of %d make too many workgroups", T, block_frames);
  SK_CHECK_ARG(Y_c64 && mask && weights_c64 && Z_c64, "sk_mvdr: null pointer (Y, mask, weights or Z)");
  SK_CHECK_ARG(ws, "sk_mvdr: ws is NULL, %zu bytes of workspace expected", sk_mvdr_workspace_bytes(T, C, S, block_frames));
  const float2* Y = (const float2*)Y_c64;
  float2 *W = (float2*)weights_c64, *Z = (float2*)Z_c64;
  return sk_dispatch_int<MINC, MAXC>(C, [&](auto c) {
    return sk_dispatch_int<MINS, SK_MAXS>(S, [&](auto s) {
      return mvdr_launch<decltype(c)::value, decltype(s)::value>(Y, y_chan_stride, y_row_stride, mask, ld_mask, T, block_frames, context_blocks,
                                                                 ref, loading, W, Z, (double2*)scm_out_c128, (double*)ws, (hipStream_t)stream);
    });
  });
}
