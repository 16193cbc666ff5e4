// bsseval.hip -- batched BSS Eval (v3) source scoring in fp64: lag correlations, block-Toeplitz Gram assembly,
// blocked Cholesky with an fp64-MFMA trailing update, forward substitution folded into the factorisation, and the
// SDR / SIR / SAR energies (include/sepkern.h "BSS Eval").
//
// One call scores U utterances of S sources with one filter length L (taps).  Per utterance:
//   xc   = [ c_ij[d], i <= j, -L < d < L  |  c_{r_i,e_k}[t], 0 <= t < L  |  |e_k|^2 ]     (xcorr record, fp64)
//   full = the (S*L) Gram matrix G of the delayed references, padded to Np = 16*ceil(S*L/16) with an identity,
//          followed by 16 rows whose first S hold b_k^T (b_k[a*L + t] = c_{r_a,e_k}[t]); factoring the whole
//          (Np + 16) x Np trapezoid turns those rows into y_k^T = (L^-1 b_k)^T, so |P_all e_k|^2 = |y_k|^2 and,
//          because the leading L x L block of the factor is G_00's, |P_0 e_k|^2 = |y_k[0:L)|^2
//   one  = for j >= 1 the same for G_jj (L square, padded to Lp) with rows b_{k,j}^T: |P_j e_k|^2 = |y|^2
// Every matrix is factored by ONE workgroup; nothing is reduced across workgroups, no float atomics: each value has
// one fixed order of operations, whatever else is in the batch.
#include "sk_common.h"

#include <math.h>

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxS = 4;
constexpr int kMaxTaps = 512;
constexpr int kCorrBlock = 256;   // lags per correlation workgroup; also samples per LDS chunk
constexpr int kCholThreads = 256;

struct Geom {
  int S, L, P;        // sources, taps, source pairs i <= j
  int64_t X;          // doubles per xcorr record
  int64_t rr, re, ee; // offsets of the three parts inside a record
  int Np, Lp;         // padded orders of the full and single-source systems (multiples of 16)
  int64_t full_sz, one_sz, mats;   // doubles per full / single matrix, per utterance's matrices
};

Geom geom(int S, int L) {
  Geom g;
  g.S = S;
  g.L = L;
  g.P = S * (S + 1) / 2;
  g.rr = 0;
  g.re = (int64_t)g.P * (2 * L - 1);
  g.ee = g.re + (int64_t)S * S * L;
  g.X = g.ee + S;
  g.Np = (int)sk_cdiv((int64_t)S * L, 16) * 16;
  g.Lp = (int)sk_cdiv(L, 16) * 16;
  g.full_sz = (int64_t)(g.Np + 16) * g.Np;
  g.one_sz = S > 1 ? (int64_t)(g.Lp + 16) * g.Lp : 0;
  g.mats = g.full_sz + (S - 1) * g.one_sz;
  return g;
}

// workspace layout (bytes, each part 256-aligned): offs (U int64) | lens (U int32) | xc (U*X) | mats (U*mats) |
// energies (U * (S + S*S) fp64: |P_all e_k|^2 then |P_j e_k|^2 at [j*S + k]) | task status (U*S int32)
struct Ws {
  int64_t* offs;
  int32_t* lens;
  double* xc;
  double* mats;
  double* energy;
  int32_t* tstat;
  size_t bytes;
};

Ws carve(void* base, int U, const Geom& g) {
  Ws w;
  size_t o = 0;
  char* b = (char*)base;
  w.offs = (int64_t*)(b + o); o = sk_align(o + (size_t)U * 8, 256);
  w.lens = (int32_t*)(b + o); o = sk_align(o + (size_t)U * 4, 256);
  w.xc = (double*)(b + o);    o = sk_align(o + (size_t)U * g.X * 8, 256);
  w.mats = (double*)(b + o);  o = sk_align(o + (size_t)U * g.mats * 8, 256);
  w.energy = (double*)(b + o); o = sk_align(o + (size_t)U * (g.S + g.S * g.S) * 8, 256);
  w.tstat = (int32_t*)(b + o); o = sk_align(o + (size_t)U * g.S * 4, 256);
  w.bytes = o;
  return w;
}

// ------------------------------------------------------------------------------------------ lag correlations
// Job list of one utterance (blockIdx.y): every job is c[d] = sum_m x[m] y[m + d] for 0 <= d < count, written to
// out[d * step] of the utterance's record.
//   pairs i <= j : (x = r_i, y = r_j) for d >= 0 -> rr[pair][L-1+d];  for i < j also (x = r_j, y = r_i), d >= 1 ->
//                  rr[pair][L-1-d] (c_ij[-d] = c_ji[d]); for i == j the negative lags are the mirror, copied after
//   cross (i, k) : (x = r_i, y = e_k), d < L -> re[(i*S + k)*L + d]
//   energy k     : (x = e_k, y = e_k), d = 0 -> ee[k]
struct Job {
  const double* x;
  const double* y;
  int count;       // number of lags
  int first;       // first lag
  int64_t out;     // record offset of lag `first`
  int step;        // +1 or -1 along the record
};

__device__ Job job_of(int jb, const double* ref, const double* est, int64_t off, int n, const Geom& g) {
  const int S = g.S, L = g.L;
  Job j;
  j.step = 1;
  j.first = 0;
  int p = 0;
  for (int a = 0; a < S; ++a)
    for (int b = a; b < S; ++b, ++p) {
      const int64_t base = g.rr + (int64_t)p * (2 * L - 1) + (L - 1);
      if (jb == 0) {
        j.x = ref + off + (int64_t)a * n; j.y = ref + off + (int64_t)b * n;
        j.count = L; j.out = base;
        return j;
      }
      --jb;
      if (a != b) {
        if (jb == 0) {
          j.x = ref + off + (int64_t)b * n; j.y = ref + off + (int64_t)a * n;
          j.first = 1; j.count = L - 1; j.out = base - 1; j.step = -1;
          return j;
        }
        --jb;
      }
    }
  if (jb < S * S) {
    const int a = jb / S, k = jb % S;
    j.x = ref + off + (int64_t)a * n; j.y = est + off + (int64_t)k * n;
    j.count = L; j.out = g.re + (int64_t)jb * L;
    return j;
  }
  jb -= S * S;
  j.x = est + off + (int64_t)jb * n; j.y = j.x;
  j.count = 1; j.out = g.ee + jb;
  return j;
}

int num_jobs(int S) { return S * (S + 1) / 2 + S * (S - 1) / 2 + S * S + S; }

// grid (lag blocks, jobs, U), 256 threads.  Thread t owns lag first + blockIdx.x*256 + t and walks the samples in
// chunks of 256 through LDS: x[m0 .. m0+256) and y[m0 + d0 .. m0 + d0 + 512) (zero outside [0, n)), one fma per
// sample in ascending m.  A job of one lag (the energies) spreads its samples over the 256 threads instead (m = t
// mod 256 in ascending order, then a fixed tree in LDS).
__global__ void __launch_bounds__(kCorrBlock) bss_xcorr_kernel(const double* __restrict__ ref, const double* __restrict__ est,
                                                               const int64_t* __restrict__ offs, const int32_t* __restrict__ lens,
                                                               Geom g, double* __restrict__ xc) {
  __shared__ double xs[kCorrBlock];
  __shared__ double ys[2 * kCorrBlock];
  const int u = blockIdx.z, t = threadIdx.x;
  const int n = lens[u];
  const Job j = job_of(blockIdx.y, ref, est, offs[u], n, g);
  double* rec = xc + (int64_t)u * g.X;
  if (j.count <= 1) {                                  // one lag (or none: taps = 1 has no negative lags)
    if (blockIdx.x != 0) return;
    double acc = 0.0;
    for (int m = t; m + j.first < n; m += kCorrBlock) acc = fma(j.x[m], j.y[m + j.first], acc);
    xs[t] = acc;
    __syncthreads();
    for (int h = kCorrBlock / 2; h > 0; h >>= 1) {
      if (t < h) xs[t] = xs[t] + xs[t + h];
      __syncthreads();
    }
    if (t == 0 && j.count == 1) rec[j.out] = xs[0];
    return;
  }
  const int d0 = j.first + blockIdx.x * kCorrBlock;     // lag of thread 0
  if (d0 >= j.first + j.count) return;                 // uniform per block
  const int d = d0 + t;
  double acc = 0.0;
  // only m < n - d contributes (y index < n); m < n bounds x
  const int mend = n - d0;                              // no thread of the block has a term at m >= n - d0
  for (int m0 = 0; m0 < mend; m0 += kCorrBlock) {
    const int mx = m0 + t;
    xs[t] = mx < n ? j.x[mx] : 0.0;
    const int64_t y0 = (int64_t)m0 + d0 + t;
    ys[t] = y0 < n ? j.y[y0] : 0.0;
    ys[t + kCorrBlock] = y0 + kCorrBlock < n ? j.y[y0 + kCorrBlock] : 0.0;
    __syncthreads();
#pragma unroll 8
    for (int mm = 0; mm < kCorrBlock; ++mm) acc = fma(xs[mm], ys[mm + t], acc);
    __syncthreads();
  }
  if (d < j.first + j.count) rec[j.out + (int64_t)(d - j.first) * j.step] = acc;
}

// c_ii[-d] = c_ii[d]
__global__ void bss_mirror_kernel(Geom g, double* __restrict__ xc) {
  const int u = blockIdx.y, i = blockIdx.x;
  double* rec = xc + (int64_t)u * g.X;
  int p = 0;
  for (int a = 0; a < i; ++a) p += g.S - a;            // pair index of (i, i)
  double* c = rec + g.rr + (int64_t)p * (2 * g.L - 1) + (g.L - 1);
  for (int d = 1 + threadIdx.x; d < g.L; d += blockDim.x) c[-d] = c[d];
}

// ------------------------------------------------------------------------------------------ Gram assembly
__device__ __forceinline__ double corr(const double* rec, const Geom& g, int a, int b, int d) {
  // c_ab[d] = sum_m r_a[m] r_b[m + d]; stored for a <= b, and c_ab[d] = c_ba[-d]
  if (a > b) {
    const int s = a; a = b; b = s; d = -d;
  }
  const int p = a * g.S - a * (a - 1) / 2 + (b - a);
  return rec[g.rr + (int64_t)p * (2 * g.L - 1) + (g.L - 1) + d];
}

// grid (row blocks of the largest matrix, matrices per utterance, U); thread per (row, col) with a grid-stride over
// columns.  Entry (a*L + t, b*L + t') = <r_a(. - t), r_b(. - t')> = c_ab[t - t'] (sepkern/bsseval.py _DelayedSpan).
__global__ void bss_assemble_kernel(Geom g, const double* __restrict__ xc, double* __restrict__ mats) {
  const int u = blockIdx.z, which = blockIdx.y;        // 0: full, j >= 1: single source j
  const int order = which == 0 ? g.Np : g.Lp;
  const int rows = order + 16;
  const int row = blockIdx.x;
  if (row >= rows) return;
  const double* rec = xc + (int64_t)u * g.X;
  double* A = mats + (int64_t)u * g.mats + (which == 0 ? 0 : g.full_sz + (int64_t)(which - 1) * g.one_sz);
  const int L = g.L, S = g.S;
  const int n = which == 0 ? S * L : L;                // true order
  for (int col = threadIdx.x; col < order; col += blockDim.x) {
    double v = 0.0;
    if (row < order) {
      if (row < n && col < n) {
        const int a = which == 0 ? row / L : which, t = row % L;
        const int b = which == 0 ? col / L : which, tt = col % L;
        v = corr(rec, g, a, b, t - tt);
      } else {
        v = row == col ? 1.0 : 0.0;
      }
    } else {
      const int k = row - order;                       // right-hand side k: b_k^T, or b_{k,j}^T
      if (k < S && col < n) {
        const int a = which == 0 ? col / L : which, t = col % L;
        v = rec[g.re + (int64_t)(a * S + k) * L + t];
      }
    }
    A[(int64_t)row * order + col] = v;
  }
}

// ------------------------------------------------------------------------------------------ Cholesky
// One workgroup (4 waves) per matrix: right-looking, panel width 16.  A is (order + 16) x order, row-major, lower
// part used; the last 16 rows are the right-hand sides.  Per panel p:
//   1. the 16 x 16 diagonal tile is factored in LDS, one entry per thread;
//   2. every row below it is solved against the tile's transpose, one row per thread;
//   3. the trailing tiles (I, J), p < J <= I, get C -= A_Ip A_Jp^T by four v_mfma_f64_16x16x4_f64, one tile per
//      wave at a time.  A/B operand of lane l: element (l & 15, 4q + (l >> 4)) of the panel rows; C/D element of
//      lane l, register r: (row, col) = ((l >> 4) + 4 r, l & 15)  (the f64 layout, unlike every other MFMA).
// A pivot that is not finite or not above 2^-40 times its original diagonal entry sets the task's bit in the status word
// (a plain store; the host re-scores such an utterance on the CPU).
__global__ void __launch_bounds__(kCholThreads) bss_chol_kernel(Geom g, double* __restrict__ mats, double* __restrict__ energy,
                                                                int32_t* __restrict__ tstat) {
  __shared__ double D[16][17];
  __shared__ double diag0[kMaxS * kMaxTaps];
  __shared__ int bad;
  const int u = blockIdx.y, which = blockIdx.x;
  const int order = which == 0 ? g.Np : g.Lp;
  const int n = which == 0 ? g.S * g.L : g.L;
  const int ld = order;
  const int nt = order / 16;
  double* A = mats + (int64_t)u * g.mats + (which == 0 ? 0 : g.full_sz + (int64_t)(which - 1) * g.one_sz);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t == 0) bad = 0;
  for (int c = t; c < order; c += kCholThreads) diag0[c] = A[(int64_t)c * ld + c];
  __syncthreads();
  const double tiny = 0x1p-40;
  for (int p = 0; p < nt; ++p) {
    const int c0 = 16 * p;
    // 1. diagonal tile
    const int r = t >> 4, c = t & 15;
    D[r][c] = A[(int64_t)(c0 + r) * ld + c0 + c];
    __syncthreads();
    for (int k = 0; k < 16; ++k) {
      const double piv = D[k][k];
      const double ds = sqrt(piv);
      if (t == 0 && !(piv > tiny * diag0[c0 + k] && piv < INFINITY)) bad = 1;
      __syncthreads();
      if (c == k && r > k) D[r][k] = D[r][k] / ds;
      if (t == 0) D[k][k] = ds;
      __syncthreads();
      if (r > k && c > k && c <= r) D[r][c] = fma(-D[r][k], D[c][k], D[r][c]);
      __syncthreads();
    }
    if (c <= r) A[(int64_t)(c0 + r) * ld + c0 + c] = D[r][c];
    // 2. panel rows below the tile (right-hand-side rows included)
    for (int i = c0 + 16 + t; i < order + 16; i += kCholThreads) {
      asm volatile("" ::: "memory");                   // keep the tile's 136 LDS reads inside the loop (registers)
      double* row = A + (int64_t)i * ld + c0;
      double x[16];
#pragma unroll
      for (int s = 0; s < 16; ++s) x[s] = row[s];
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        double v = x[s];
#pragma unroll
        for (int q = 0; q < s; ++q) v = fma(-x[q], D[s][q], v);
        x[s] = v / D[s][s];
      }
#pragma unroll
      for (int s = 0; s < 16; ++s) row[s] = x[s];
    }
    __syncthreads();
    // 3. trailing update: tiles (I, J), p < J <= min(I, nt - 1), p < I < mt, enumerated row by row
    const int lr = lane & 15, lk = lane >> 4;
    const int64_t ntiles_full = (int64_t)(nt - 1 - p) * (nt - p) / 2;   // I < nt
    const int64_t ntiles = ntiles_full + (nt - 1 - p);                   // + the right-hand-side row of tiles
    for (int64_t q = wave; q < ntiles; q += kCholThreads / 64) {
      int I, J;
      if (q < ntiles_full) {
        // q = (I' (I' + 1)) / 2 + J' with I' = I - p - 1, J' = J - p - 1 <= I'
        int Ip = (int)((sqrt(8.0 * (double)q + 1.0) - 1.0) * 0.5);
        while ((int64_t)(Ip + 1) * (Ip + 2) / 2 <= q) ++Ip;
        while ((int64_t)Ip * (Ip + 1) / 2 > q) --Ip;
        I = p + 1 + Ip;
        J = p + 1 + (int)(q - (int64_t)Ip * (Ip + 1) / 2);
      } else {
        I = nt;
        J = p + 1 + (int)(q - ntiles_full);
      }
      const double* Ai = A + (int64_t)(16 * I + lr) * ld + c0 + lk;
      const double* Bj = A + (int64_t)(16 * J + lr) * ld + c0 + lk;
      double* Cp = A + (int64_t)(16 * I + lk) * ld + 16 * J + lr;
      f64x4 acc;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = Cp[(int64_t)4 * e * ld];
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-Ai[4 * s], Bj[4 * s], acc, 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) Cp[(int64_t)4 * e * ld] = acc[e];
    }
    __syncthreads();
  }
  // energies of the solved right-hand sides: wave k sums y_k^2 over [0, L) and [0, n), lanes in ascending columns,
  // then a fixed butterfly
  const int S = g.S, L = g.L;
  if (wave < S) {
    const double* y = A + (int64_t)(order + wave) * ld;
    double head = 0.0, all = 0.0;
    for (int col = lane; col < n; col += 64) {
      const double v = y[col];
      if (col < L) head = fma(v, v, head);
      all = fma(v, v, all);
    }
    for (int h = 32; h > 0; h >>= 1) {
      head += __shfl_xor(head, h, 64);
      all += __shfl_xor(all, h, 64);
    }
    double* e = energy + (int64_t)u * (S + S * S);
    if (lane == 0) {
      if (which == 0) {
        e[wave] = all;                  // |P_all e_k|^2
        e[S + wave] = head;             // |P_0 e_k|^2 at [j = 0][k]
      } else {
        e[S + which * S + wave] = all;  // |P_j e_k|^2
      }
    }
  }
  if (t == 0) tstat[(int64_t)u * S + which] = bad ? (1 << which) : 0;
}

// ------------------------------------------------------------------------------------------ dB
__device__ __forceinline__ double db(double num, double den) {
  // a non-positive denominator is a zero one that rounding pushed below zero (the energies are differences)
  return den > 0.0 ? 10.0 * log10(num / den) : INFINITY;
}

// thread per (u, k, j): out[((u*S + k)*S + j)*3 + {0,1,2}] = SDR / SIR / SAR of estimate k against source j
__global__ void bss_db_kernel(Geom g, int U, const double* __restrict__ xc, const double* __restrict__ energy,
                              const int32_t* __restrict__ tstat, double* __restrict__ out, int32_t* __restrict__ status) {
  const int S = g.S;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)U * S * S) return;
  const int u = (int)(i / (S * S)), k = (int)(i / S % S), j = (int)(i % S);
  const double* e = energy + (int64_t)u * (S + S * S);
  const double ee = xc[(int64_t)u * g.X + g.ee + k];
  const double pall = e[k], pj = e[S + j * S + k];
  double* o = out + i * 3;
  o[0] = db(pj, ee - pj);
  o[1] = db(pj, pall - pj);
  o[2] = db(pall, ee - pall);
  if (k == 0 && j == 0) {
    int s = 0;
    for (int w = 0; w < S; ++w) s |= tstat[(int64_t)u * S + w];
    status[u] = s;
  }
}

int check_args(int U, int S, int taps, const int64_t* offs_host, const int32_t* lens_host) {
  SK_CHECK_ARG(U >= 1, "bss: U = %d, need >= 1", U);
  SK_CHECK_ARG(S >= 1 && S <= kMaxS, "bss: S = %d, need 1..%d", S, kMaxS);
  SK_CHECK_ARG(taps >= 1 && taps <= kMaxTaps, "bss: taps = %d, need 1..%d", taps, kMaxTaps);
  SK_CHECK_ARG(offs_host && lens_host, "bss: offs_host and lens_host are required");
  for (int u = 0; u < U; ++u) {
    SK_CHECK_ARG(lens_host[u] >= 1, "bss: utterance %d has length %d, need >= 1", u, lens_host[u]);
    SK_CHECK_ARG(offs_host[u] >= 0, "bss: utterance %d has offset %lld", u, (long long)offs_host[u]);
  }
  return SK_OK;
}

int run_xcorr(const double* ref, const double* est, const int64_t* offs_host, const int32_t* lens_host, int U,
              const Geom& g, const Ws& w, double* xc, hipStream_t st) {
  SK_CHECK_HIP(hipMemcpyAsync(w.offs, offs_host, (size_t)U * 8, hipMemcpyHostToDevice, st));
  SK_CHECK_HIP(hipMemcpyAsync(w.lens, lens_host, (size_t)U * 4, hipMemcpyHostToDevice, st));
  const int lagblocks = (int)sk_cdiv(g.L, kCorrBlock);
  hipLaunchKernelGGL(bss_xcorr_kernel, dim3(lagblocks, num_jobs(g.S), U), dim3(kCorrBlock), 0, st, ref, est, w.offs, w.lens,
                     g, xc);
  SK_CHECK_LAUNCH("bss_xcorr_kernel");
  hipLaunchKernelGGL(bss_mirror_kernel, dim3(g.S, U), dim3(256), 0, st, g, xc);
  SK_CHECK_LAUNCH("bss_mirror_kernel");
  return SK_OK;
}

}  // namespace

extern "C" size_t sk_bss_workspace_bytes(int U, int S, int taps) {
  if (U < 1 || S < 1 || S > kMaxS || taps < 1 || taps > kMaxTaps) return 0;
  return carve(nullptr, U, geom(S, taps)).bytes;
}

extern "C" int sk_bss_xcorr(const double* ref, const double* est, const int64_t* offs_host, const int32_t* lens_host, int U,
                            int S, int taps, void* ws, double* xc, sk_stream_t stream) {
  const int rc = check_args(U, S, taps, offs_host, lens_host);
  if (rc) return rc;
  SK_CHECK_ARG(ref && est && ws && xc, "bss_xcorr: null pointer");
  const Geom g = geom(S, taps);
  const Ws w = carve(ws, U, g);
  return run_xcorr(ref, est, offs_host, lens_host, U, g, w, xc, (hipStream_t)stream);
}

extern "C" int sk_bss_eval(const double* ref, const double* est, const int64_t* offs_host, const int32_t* lens_host, int U,
                           int S, int taps, void* ws, double* out, int32_t* status, sk_stream_t stream) {
  const int rc = check_args(U, S, taps, offs_host, lens_host);
  if (rc) return rc;
  SK_CHECK_ARG(ref && est && ws && out && status, "bss_eval: null pointer");
  const Geom g = geom(S, taps);
  const Ws w = carve(ws, U, g);
  hipStream_t st = (hipStream_t)stream;
  int e = run_xcorr(ref, est, offs_host, lens_host, U, g, w, w.xc, st);
  if (e) return e;
  hipLaunchKernelGGL(bss_assemble_kernel, dim3(g.Np + 16, S, U), dim3(256), 0, st, g, w.xc, w.mats);
  SK_CHECK_LAUNCH("bss_assemble_kernel");
  hipLaunchKernelGGL(bss_chol_kernel, dim3(S, U), dim3(kCholThreads), 0, st, g, w.mats, w.energy, w.tstat);
  SK_CHECK_LAUNCH("bss_chol_kernel");
  const int64_t nthr = (int64_t)U * S * S;
  hipLaunchKernelGGL(bss_db_kernel, dim3((unsigned)sk_cdiv(nthr, 256)), dim3(256), 0, st, g, U, w.xc, w.energy, w.tstat, out,
                     status);
  SK_CHECK_LAUNCH("bss_db_kernel");
  return SK_OK;
}
