// wpe_solve.h -- what wpe.hip and wpd.hip share: the 4 x 4 tiles of a weighted Hermitian sum, one per thread, and the fp64
// Cholesky solve of up to 80 x 80 in a workgroup's LDS.  The operations and their order are sepkern/wpe.py's (covariances,
// cholesky_solve), one rounding each: no multiply is fused into an add in this file or in a file that includes it.
#pragma once
#include "sk_common.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ int tri_row(int D, int a) { return a * D - a * (a - 1) / 2; }  // packed index of (a, a)

// A thread's tile: rows 4 ti .. 4 ti + 3 against columns 4 tj .. of the upper triangle of R (tj >= ti; NTR tile rows), or,
// for the threads after those, tile (ti, tj) of the right-hand side, NPR x NCT tiles
struct SolveTile {
  int ti, tj;
  bool is_p, has;
};

__device__ __forceinline__ SolveTile solve_tile(int tid, int NTR, int NPR, int NCT) {
  SolveTile t{0, 0, false, true};
  int r = tid;
  while (t.ti < NTR && r >= NTR - t.ti) {
    r -= NTR - t.ti;
    ++t.ti;
  }
  if (t.ti < NTR) {
    t.tj = t.ti + r;
  } else if (r < NPR * NCT) {
    t.is_p = true;
    t.ti = r / NCT;
    t.tj = r - t.ti * NCT;
  } else {
    t.has = false;
  }
  return t;
}

// one frame of a tile: acc += (w a_p) conj(b_q), the operands at base[offa[p]], base[offb[q]]
__device__ __forceinline__ void tile_frame(double (&ar)[4][4], double (&ai)[4][4], const double2* __restrict__ base, const int (&offa)[4],
                                           const int (&offb)[4], double w) {
  double pr[4], pi[4], qr[4], qi[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double2 a = base[offa[q]], b = base[offb[q]];
    pr[q] = a.x * w;
    pi[q] = a.y * w;
    qr[q] = b.x;
    qi[q] = b.y;
  }
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // a conj(b)
      ar[p][q] += pr[p] * qr[q] + pi[p] * qi[q];
      ai[p][q] += pi[p] * qr[q] - pr[p] * qi[q];
    }
}

// the tile to LDS: the packed upper triangle Rt of a D x D matrix (real diagonal), or the first PR rows of PG (rows of C)
__device__ __forceinline__ void tile_store(const SolveTile& t, const double (&ar)[4][4], const double (&ai)[4][4], double2* Rt, double2* PG,
                                           int D, int PR, int C) {
  if (!t.has) return;
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int a = 4 * t.ti + p, b = 4 * t.tj + q;
      if (t.is_p) {
        if (a < PR && b < C) PG[a * C + b] = make_double2(ar[p][q], ai[p][q]);
      } else if (a <= b && b < D) {
        Rt[tri_row(D, a) + (b - a)] = make_double2(ar[p][q], a == b ? 0.0 : ai[p][q]);
      }
    }
}

// PG (D x C) <- R^-1 PG for the loaded R in Rt, over the workgroup's NTHR threads; rinv: D doubles.  Right-looking, one barrier
// per pivot: step a takes row a's products out of the rows below it.  Row a stays unscaled in LDS while its step reads it;
// U[a][b] = R[a][b] / U[a][a] is formed where it is used, with the rounding the stored value will have.  Returns whether a
// component this thread wrote last is not finite; PG is complete after the caller's next barrier.
template <int NTHR>
__device__ __forceinline__ int cholesky_solve_lds(double2* Rt, double2* PG, double* rinv, int D, int C, int tid) {
  for (int a = 0; a < D; ++a) {
    __syncthreads();
    const double2* __restrict__ rowa = Rt + tri_row(D, a);  // (a, b) at rowa[b - a]
    const double ri = 1.0 / sqrt(rowa[0].x);
    if (tid == 0) rinv[a] = ri;
    const int m = D - 1 - a;
    for (int idx = tid; idx < m * m; idx += NTHR) {
      const int ii = idx / m, bb = idx - ii * m;
      if (bb < ii) continue;
      const double uar = rowa[1 + ii].x * ri, uai = rowa[1 + ii].y * ri, ubr = rowa[1 + bb].x * ri, ubi = rowa[1 + bb].y * ri;
      double2* e = Rt + tri_row(D, a + 1 + ii) + (bb - ii);
      double2 v = *e;
      v.x -= uar * ubr + uai * ubi;  // conj(ua) ub; on the diagonal |ua|^2, and the imaginary part is never read
      v.y -= uar * ubi - uai * ubr;
      *e = v;
    }
  }
  __syncthreads();
  for (int idx = tid; idx < D * D; idx += NTHR) {
    const int a = idx / D, b = idx - a * D;
    if (b > a) {
      double2* e = Rt + tri_row(D, a) + (b - a);
      const double ri = rinv[a];
      *e = make_double2(e->x * ri, e->y * ri);
    }
  }
  // ---- U^H Z = P
  for (int a = 0; a < D; ++a) {
    __syncthreads();
    const double2* __restrict__ rowa = Rt + tri_row(D, a);
    const double ri = rinv[a];
    const int m = D - 1 - a;
    for (int idx = tid; idx < m * C; idx += NTHR) {
      const int bb = idx / C, c = idx - bb * C;
      const double2 z0 = PG[a * C + c], u = rowa[1 + bb];
      const double zr = z0.x * ri, zi = z0.y * ri;
      double2* e = PG + (a + 1 + bb) * C + c;  // -= conj(u) z
      *e = make_double2(e->x - (u.x * zr + u.y * zi), e->y - (u.x * zi - u.y * zr));
    }
  }
  __syncthreads();
  for (int idx = tid; idx < D * C; idx += NTHR) {
    const double ri = rinv[idx / C];
    PG[idx] = make_double2(PG[idx].x * ri, PG[idx].y * ri);
  }
  // ---- U G = Z, from the last row up
  for (int a = D - 1; a >= 0; --a) {
    __syncthreads();
    const double ri = rinv[a];
    for (int idx = tid; idx < a * C; idx += NTHR) {
      const int r = idx / C, c = idx - r * C;
      const double2 g0 = PG[a * C + c], u = Rt[tri_row(D, r) + (a - r)];
      const double gr = g0.x * ri, gi = g0.y * ri;
      double2* e = PG + r * C + c;  // -= u g
      *e = make_double2(e->x - (u.x * gr - u.y * gi), e->y - (u.x * gi + u.y * gr));
    }
  }
  __syncthreads();
  int bad = 0;
  for (int idx = tid; idx < D * C; idx += NTHR) {
    const double ri = rinv[idx / C];
    const double2 g = make_double2(PG[idx].x * ri, PG[idx].y * ri);
    PG[idx] = g;
    bad |= !(isfinite(g.x) && isfinite(g.y));
  }
  return bad;
}

}  // namespace
