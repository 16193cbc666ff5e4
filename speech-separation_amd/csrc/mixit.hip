// mixit.hip -- the mixture-invariant loss (MixIT) on time-domain estimates: the statistics and the finalize step
// (include/sepkern.h "mixture-invariant loss"; sepkern/mixit.py states the definition in numpy fp64).
// The estimates come from sk_mask_istft_rows, the gradient goes back through sk_mixit_mask_grad (both in stft.hip).
//
// One streaming pass reads every estimate and both reference samples once and forms, per utterance, the plain sums
//   P_n = sum x_n^2,  c_nk = sum x_n e_k,  G_kl = sum e_k e_l (k <= l)        (NQ = 2 + 2 M + M (M + 1) / 2 values)
// in fp64, on the sums skeleton of wave_loss.h (which states the order of operations), as sisdr.hip forms its sums.  The
// error of every one of the 2^M assignments follows from these sums alone.
//
// Shape coverage: tests/test_gpu_wave_cases.py runs mixit_sums_kernel<2..4> and the finalize kernel at the lengths and batch
// sizes named under sisdr.hip, at tau = 0, 1e-3 and 1, with both references silent, an exact partition and exact ties, against fp64.
#include "wave_loss.h"

#include <math.h>

namespace {

constexpr int MAXM = SK_MAXS;
constexpr int NREF = 2;
constexpr int NQMAX = 2 + 2 * MAXM + MAXM * (MAXM + 1) / 2;

__host__ __device__ constexpr int nq_of(int M) { return 2 + 2 * M + M * (M + 1) / 2; }
// index of G_kl, k <= l, in the row-major upper triangle that follows P and c
__host__ __device__ constexpr int g_index(int M, int k, int l) { return 2 + 2 * M + k * M - k * (k - 1) / 2 + (l - k); }

// partial[(u * nch + ch) * NQ + q]: [P_0 P_1 | c_0k (M) | c_1k (M) | G_kl, k <= l, row-major]
template <int M>
__global__ __launch_bounds__(256) void mixit_sums_kernel(const float* __restrict__ est, const int64_t* __restrict__ est_offs,
                                                         const void* __restrict__ ref, int pcm16,
                                                         const int64_t* __restrict__ ref_offs,
                                                         const int32_t* __restrict__ nsamp, int nch,
                                                         double* __restrict__ partial) {
  constexpr int NQ = nq_of(M);
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
    for (int n = 0; n < NREF; ++n) x[n] = ref_f64(ref, pcm16, ro[n], i);
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
  chunk_store<NQ>(acc, partial + ((int64_t)u * nch + ch) * NQ);
}

// Between gather_chunks and tally_scores, one thread per utterance walks the 2^M assignment codes (bit k of a code = the
// reference estimate k is added to) in code order: the two errors from the sums, the two thresholded scores, their mean; the
// first maximum wins and leaves its two gradient coefficients.  The utterance's sums are indexed at run time and live in the workspace.
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
  gather_chunks(partial, nch, nsamp, B, NQ, sums);
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
  tally_scores(best_score, B, count, out);
}

}  // namespace

extern "C" size_t sk_mixit_workspace_bytes(int B, int M, int max_samples) {
  if (B <= 0 || M < 2 || M > MAXM || max_samples <= 0) return 0;
  return partial_bytes(B, nq_of(M), max_samples) + sk_align((size_t)B * (1 + NQMAX) * sizeof(double), 256);  // + best scores, sums
}

extern "C" int sk_mixit_fwd(const float* est, const int64_t* est_offs, const void* ref, int pcm16, const int64_t* ref_offs,
                            const int32_t* nsamp, int B, int M, int max_samples, const float* count_dev, double tau,
                            float* assign_score, int32_t* best_code, float* out, float* coef, void* ws, sk_stream_t stream) {
  SK_CHECK_ARG(M >= 2 && M <= MAXM, "sk_mixit_fwd: %d estimates per utterance, outside 2..%d", M, MAXM);
  SK_CHECK_ARG(est && est_offs && ref && ref_offs && nsamp && assign_score && best_code && out && coef && ws,
               "sk_mixit_fwd: null pointer");
  SK_CHECK_ARG(B > 0 && B <= 65535, "sk_mixit_fwd: B = %d utterances outside 1..65535", B);
  SK_CHECK_ARG(max_samples > 0, "sk_mixit_fwd: max_samples = %d, at least 1 expected", max_samples);
  SK_CHECK_ARG(tau >= 0.0 && tau <= 1.0, "sk_mixit_fwd: tau %g outside 0..1", tau);
  const int nch = (int)sk_cdiv(max_samples, CHUNK);
  double* partial = (double*)ws;
  double* best_score = (double*)((char*)ws + partial_bytes(B, nq_of(M), max_samples));
  double* sums = best_score + B;  // B x NQ <= B x NQMAX
  dim3 grid((unsigned)nch, (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  const sums_kernel_t sums_kernel[MAXM - 1] = {mixit_sums_kernel<2>, mixit_sums_kernel<3>, mixit_sums_kernel<4>};
  hipLaunchKernelGGL(sums_kernel[M - 2], grid, dim3(256), 0, st, est, est_offs, ref, pcm16, ref_offs, nsamp, nch, partial);
  SK_CHECK_LAUNCH("mixit_sums_kernel");
  hipLaunchKernelGGL(mixit_finalize_kernel, dim3(1), dim3(256), 0, st, partial, nch, nsamp, B, M, tau, count_dev, best_score,
                     sums, assign_score, best_code, out, coef);
  SK_CHECK_LAUNCH("mixit_finalize_kernel");
  return SK_OK;
}
