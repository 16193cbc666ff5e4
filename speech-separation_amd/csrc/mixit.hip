// mixit.hip -- the mixture-invariant loss (MixIT) on time-domain estimates: the statistics and the finalize step
// (include/sepkern.h "mixture-invariant loss"; sepkern/mixit.py states the definition in numpy fp64).
// The estimates come from sk_mask_istft_rows, the gradient goes back through sk_mixit_mask_grad (both in stft.hip).
//
// One streaming pass reads every estimate and both reference samples once and forms, per utterance, the plain sums
//   P_n = sum x_n^2,  c_nk = sum x_n e_k,  G_kl = sum e_k e_l (k <= l)        (NQ = 2 + 2 M + M (M + 1) / 2 values)
// in fp64, exactly as sisdr.hip forms its sums: a thread adds its samples in index order, a workgroup (one chunk of CHUNK
// samples) adds its threads by a fixed shuffle tree, and the finalize kernel adds the chunks of an utterance in chunk order.
// No atomics; the chunk grid of an utterance depends on its own length only, so each value has one order of operations
// whatever else is in the batch.  The error of every one of the 2^M assignments follows from these sums alone.
#include "sk_common.h"

#include <math.h>

namespace {

constexpr int MAXM = SK_MAXS;
constexpr int NREF = 2;
constexpr int CHUNK = 4096;               // samples per workgroup: 16 per thread
constexpr int NQMAX = 2 + 2 * MAXM + MAXM * (MAXM + 1) / 2;

__host__ __device__ constexpr int nq_of(int M) { return 2 + 2 * M + M * (M + 1) / 2; }
// index of G_kl, k <= l, in the row-major upper triangle that follows P and c
__host__ __device__ constexpr int g_index(int M, int k, int l) { return 2 + 2 * M + k * M - k * (k - 1) / 2 + (l - k); }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// partial[(u * nch + ch) * NQ + q]: [P_0 P_1 | c_0k (M) | c_1k (M) | G_kl, k <= l, row-major]
template <int M>
__global__ __launch_bounds__(256) void mixit_sums_kernel(const float* __restrict__ est, const int64_t* __restrict__ est_offs,
                                                         const void* __restrict__ ref, int pcm16,
                                                         const int64_t* __restrict__ ref_offs,
                                                         const int32_t* __restrict__ nsamp, int nch,
                                                         double* __restrict__ partial) {
  constexpr int NQ = nq_of(M);
  __shared__ double red[4][NQ];
  const int u = blockIdx.y, ch = blockIdx.x;
  const int L = nsamp[u];
  const int n0 = ch * CHUNK;
  if (n0 >= L) return;  // (the finalize kernel reads the chunks below ceil(L / CHUNK) only)
  const int n1 = min(L, n0 + CHUNK);
  const float* ep[M];
  int64_t ro[NREF];
#pragma unroll
  for (int k = 0; k < M; ++k) ep[k] = est + est_offs[u * M + k];
#pragma unroll
  for (int n = 0; n < NREF; ++n) ro[n] = ref_offs[u * NREF + n];
  double acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
  for (int i = n0 + threadIdx.x; i < n1; i += 256) {
    double e[M], x[NREF];
#pragma unroll
    for (int k = 0; k < M; ++k) e[k] = (double)ep[k][i];
#pragma unroll
    for (int n = 0; n < NREF; ++n)  // int16 PCM scaled by 2^-15: exact in fp32 and in fp64
      x[n] = pcm16 ? (double)((const int16_t*)ref)[ro[n] + i] * (1.0 / 32768.0) : (double)((const float*)ref)[ro[n] + i];
#pragma unroll
    for (int n = 0; n < NREF; ++n) {
      acc[n] += x[n] * x[n];
#pragma unroll
      for (int k = 0; k < M; ++k) acc[2 + n * M + k] += x[n] * e[k];
    }
#pragma unroll
    for (int k = 0; k < M; ++k)
#pragma unroll
      for (int l = k; l < M; ++l) acc[g_index(M, k, l)] += e[k] * e[l];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const double v = wave_sum_f64(acc[q]);
    if (lane == 0) red[wave][q] = v;
  }
  __syncthreads();
  if (threadIdx.x < NQ) {
    const int q = threadIdx.x;
    partial[((int64_t)u * nch + ch) * NQ + q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
  }
}

// First one thread per (utterance, sum) adds that sum's chunks in chunk order; then one thread per utterance walks the 2^M
// assignment codes (bit k of a code = the reference estimate k is added to) in code order: the two errors from the sums, the
// two thresholded scores, their mean; the first maximum wins and leaves its two gradient coefficients.  Thread 0 finally adds
// the best scores in utterance order.  The utterance's sums are indexed at run time and live in the workspace.
__global__ __launch_bounds__(256) void mixit_finalize_kernel(const double* __restrict__ partial, int nch,
                                                             const int32_t* __restrict__ nsamp, int B, int M, double tau,
                                                             const float* __restrict__ count_dev, double* __restrict__ best_score,
                                                             double* __restrict__ sums, float* __restrict__ assign_score,
                                                             int32_t* __restrict__ best_code, float* __restrict__ out,
                                                             float* __restrict__ coef) {
  const int NQ = nq_of(M);
  const int ncode = 1 << M;
  const double count = count_dev ? (double)count_dev[0] : (double)B;
  const double eps = 1e-30, kappa = 10.0 / log(10.0);
  for (int idx = threadIdx.x; idx < B * NQ; idx += 256) {
    const int u = idx / NQ, q = idx - u * NQ;
    const int mych = (nsamp[u] + CHUNK - 1) / CHUNK;
    double a = 0.0;
    for (int c = 0; c < mych; ++c) a += partial[((int64_t)u * nch + c) * NQ + q];
    sums[idx] = a;
  }
  __syncthreads();
  for (int u = threadIdx.x; u < B; u += 256) {
    const double* const s = sums + (int64_t)u * NQ;
    // err_n(code) = max(P_n - 2 sum_{k in n} c_nk + sum_{k,l in n} G_kl, 0): members ascending, G_kk then 2 G_kl for l > k
    auto error = [&](int code, int n) {
      double cs = 0.0, gs = 0.0;
      for (int k = 0; k < M; ++k) {
        if (((code >> k) & 1) != n) continue;
        cs += s[2 + n * M + k];
        gs += s[g_index(M, k, k)];
        for (int l = k + 1; l < M; ++l)
          if (((code >> l) & 1) == n) gs += 2.0 * s[g_index(M, k, l)];
      }
      return fmax((s[n] - 2.0 * cs) + gs, 0.0);
    };
    double best = 0.0;
    int bc = 0;
    for (int code = 0; code < ncode; ++code) {
      double sc = 0.0;
      for (int n = 0; n < NREF; ++n) sc += 10.0 * log10((s[n] + eps) / (error(code, n) + tau * s[n] + eps));
      sc *= 0.5;
      assign_score[(int64_t)code * B + u] = (float)sc;
      if (code == 0 || sc > best) {
        best = sc;
        bc = code;
      }
    }
    best_code[u] = bc;
    best_score[u] = best;
    for (int n = 0; n < NREF; ++n) {
      const double den = error(bc, n) + tau * s[n];
      coef[u * NREF + n] = den > 0.0 ? (float)(kappa / (count * (den + eps))) : 0.0f;  // a silent reference met exactly: no gradient
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int u = 0; u < B; ++u) tot += best_score[u];
    out[0] = (float)(-tot / count);
    out[1] = (float)count;
    out[2] = (float)tot;
  }
}

size_t partial_bytes(int B, int M, int max_samples) {
  return sk_align((size_t)B * sk_cdiv(max_samples, CHUNK) * nq_of(M) * sizeof(double), 256);
}

}  // namespace

extern "C" size_t sk_mixit_workspace_bytes(int B, int M, int max_samples) {
  if (B <= 0 || M < 2 || M > MAXM || max_samples <= 0) return 0;
  return partial_bytes(B, M, max_samples) + sk_align((size_t)B * (1 + NQMAX) * sizeof(double), 256);  // + best scores, sums
}

extern "C" int sk_mixit_fwd(const float* est, const int64_t* est_offs, const void* ref, int pcm16, const int64_t* ref_offs,
                            const int32_t* nsamp, int B, int M, int max_samples, const float* count_dev, double tau,
                            float* assign_score, int32_t* best_code, float* out, float* coef, void* ws, sk_stream_t stream) {
  SK_CHECK_ARG(M >= 2 && M <= MAXM, "sk_mixit_fwd: %d estimates per utterance, outside 2..%d", M, MAXM);
  SK_CHECK_ARG(est && est_offs && ref && ref_offs && nsamp && assign_score && best_code && out && coef && ws,
               "sk_mixit_fwd: null pointer");
  SK_CHECK_ARG(B > 0 && B <= 65535 && max_samples > 0, "sk_mixit_fwd: bad sizes");
  SK_CHECK_ARG(tau >= 0.0 && tau <= 1.0, "sk_mixit_fwd: tau %g outside 0..1", tau);
  const int nch = (int)sk_cdiv(max_samples, CHUNK);
  double* partial = (double*)ws;
  double* best_score = (double*)((char*)ws + partial_bytes(B, M, max_samples));
  double* sums = best_score + B;  // B x NQ <= B x NQMAX
  dim3 grid((unsigned)nch, (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
#define SK_MIXIT_SUMS(NM) \
  hipLaunchKernelGGL(mixit_sums_kernel<NM>, grid, dim3(256), 0, st, est, est_offs, ref, pcm16, ref_offs, nsamp, nch, partial)
  switch (M) {
    case 2: SK_MIXIT_SUMS(2); break;
    case 3: SK_MIXIT_SUMS(3); break;
    default: SK_MIXIT_SUMS(4); break;
  }
#undef SK_MIXIT_SUMS
  SK_CHECK_LAUNCH("mixit_sums_kernel");
  hipLaunchKernelGGL(mixit_finalize_kernel, dim3(1), dim3(256), 0, st, partial, nch, nsamp, B, M, tau, count_dev, best_score,
                     sums, assign_score, best_code, out, coef);
  SK_CHECK_LAUNCH("mixit_finalize_kernel");
  return SK_OK;
}
