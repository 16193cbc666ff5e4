// sisdr.hip -- utterance-level PIT on the SI-SDR of time-domain estimates: the statistics and the finalize step
// (include/sepkern.h "SI-SDR uPIT loss").  The estimates come from sk_mask_istft_rows, the gradient
// goes back through sk_sisdr_mask_grad (both in stft.hip, on the FFT of fft512.h).
//
// One streaming pass reads every estimate and every reference sample once and forms, per utterance, the plain sums
//   sum e_k, sum r_i, sum e_k^2, sum r_i^2, sum e_k r_i        (4 S + S^2 values)
// in fp64, on the sums skeleton of wave_loss.h (which states the order of operations).
//
// Shape coverage: tests/test_gpu_wave_cases.py runs sisdr_sums_kernel<1..4> and the finalize kernel at 1, 2, 255 | 256 | 257,
// 4095 | 4096 | 4097, 8192 | 8193 and 12289 samples, at B * NQ and B either side of 256, and on every zero-coefficient branch and
// exact tie, against fp64 (tests/_wave_cases.py names the edge each case is there for).
#include "wave_loss.h"

#include <math.h>

namespace {

constexpr int MAXS = SK_MAXS;

__host__ __device__ constexpr int nq_of(int S) { return 4 * S + S * S; }

// partial[(u * nch + ch) * NQ + q], NQ = 4 S + S^2: [sum e (S) | sum r (S) | sum e^2 (S) | sum r^2 (S) | sum e_k r_i (k-major)]
template <int S>
__global__ __launch_bounds__(256) void sisdr_sums_kernel(const float* __restrict__ est, const int64_t* __restrict__ est_offs,
                                                         const void* __restrict__ ref, int pcm16,
                                                         const int64_t* __restrict__ ref_offs,
                                                         const int32_t* __restrict__ nsamp, int nch,
                                                         double* __restrict__ partial) {
  constexpr int NQ = nq_of(S);
  const int u = blockIdx.y, ch = blockIdx.x;
  const int L = nsamp[u];
  const int n0 = ch * CHUNK;
  if (n0 >= L) return;  // (the finalize kernel reads the chunks below ceil(L / CHUNK) only)
  const int n1 = min(L, n0 + CHUNK);
  const float* ep[S];
  int64_t ro[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    ep[s] = est + est_offs[u * S + s];
    ro[s] = ref_offs[u * S + s];
  }
  double acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
  for (int n = n0 + threadIdx.x; n < n1; n += 256) {
    double e[S], r[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      e[s] = (double)ep[s][n];
      r[s] = ref_f64(ref, pcm16, ro[s], n);
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
      acc[s] += e[s];
      acc[S + s] += r[s];
      acc[2 * S + s] += e[s] * e[s];
      acc[3 * S + s] += r[s] * r[s];
#pragma unroll
      for (int i = 0; i < S; ++i) acc[4 * S + s * S + i] += e[s] * r[i];
    }
  }
  chunk_store<NQ>(acc, partial + ((int64_t)u * nch + ch) * NQ);
}

// Between gather_chunks and tally_scores, one thread per utterance: zero-mean inner products -> pair (dB), permutation
// scores, arg-max, the gradient's three coefficients per estimate.  Values that are indexed at run time (the utterance's
// sums, the pair matrix in fp64, the best scores) live in the workspace, not in registers.
__global__ __launch_bounds__(256) void sisdr_finalize_kernel(const double* __restrict__ partial, int nch,
                                                             const int32_t* __restrict__ nsamp, int B, int S,
                                                             const float* __restrict__ count_dev, double* __restrict__ best_score,
                                                             double* __restrict__ pair64, double* __restrict__ sums, float* __restrict__ pair,
                                                             float* __restrict__ perm_score, int32_t* __restrict__ best_perm,
                                                             float* __restrict__ out, float* __restrict__ coef) {
  const int NQ = nq_of(S);
  int nperm = 1;
  for (int i = 2; i <= S; ++i) nperm *= i;
  const double count = count_dev ? (double)count_dev[0] : (double)B;
  const double eps = 1e-30, kappa = 10.0 / log(10.0);
  gather_chunks(partial, nch, nsamp, B, NQ, sums);
  for (int u = threadIdx.x; u < B; u += 256) {
    const double n = (double)nsamp[u];
    auto total = [&](int q) { return sums[u * NQ + q]; };
    // zero-mean a = <e~_k, r~_i>, b = <r~_i, r~_i>, c = <e~_k, e~_k> and the two means
    auto inner = [&](int k, int i, double& a, double& b, double& c, double& mue, double& mur) {
      const double se = total(k), sr = total(S + i);
      a = total(4 * S + k * S + i) - se * sr / n;
      b = total(3 * S + i) - sr * sr / n;
      c = total(2 * S + k) - se * se / n;
      mue = se / n;
      mur = sr / n;
    };
    double* const pr = pair64 + (int64_t)u * (MAXS * MAXS);
    for (int k = 0; k < S; ++k)
      for (int i = 0; i < S; ++i) {
        double a, b, c, mue, mur;
        inner(k, i, a, b, c, mue, mur);
        const double tt = b > 0.0 ? (a / b) * a : 0.0;  // |projection of e~ on r~|^2
        const double nn = fmax(c - tt, 0.0);
        const double v = 10.0 * log10((tt + eps) / (nn + eps));
        pr[k * S + i] = v;
        pair[((int64_t)u * S + k) * S + i] = (float)v;
      }
    double best = 0.0;
    int bi = 0;
    for (int p = 0; p < nperm; ++p) {
      const unsigned code = sk_nth_perm_code(p, S);
      double sc = 0.0;
      for (int k = 0; k < S; ++k) sc += pr[k * S + ((code >> (2 * k)) & 3u)];
      sc /= (double)S;
      perm_score[(int64_t)p * B + u] = (float)sc;
      if (p == 0 || sc > best) {
        best = sc;
        bi = p;
      }
    }
    best_perm[u] = bi;
    best_score[u] = best;
    const unsigned code = sk_nth_perm_code(bi, S);
    const double m = -1.0 / (count * (double)S);
    for (int k = 0; k < S; ++k) {
      double a, b, c, mue, mur;
      inner(k, (int)((code >> (2 * k)) & 3u), a, b, c, mue, mur);
      double cA = 0.0, cB = 0.0, cC = 0.0;
      if (b > 0.0 && a != 0.0) {
        const double den = c - (a / b) * a;
        if (den > 0.0) {
          const double P = -2.0 * kappa / den, Q = kappa * (2.0 / a + 2.0 * a / (b * den));
          cA = m * P;
          cB = m * Q;
          cC = -m * (P * mue + Q * mur);
        }
      }
      float* co = coef + ((int64_t)u * S + k) * 3;
      co[0] = (float)cA;
      co[1] = (float)cB;
      co[2] = (float)cC;
    }
  }
  tally_scores(best_score, B, count, out);
}

}  // namespace

extern "C" size_t sk_sisdr_workspace_bytes(int B, int S, int max_samples) {
  if (B <= 0 || S < 1 || S > MAXS || max_samples <= 0) return 0;
  return partial_bytes(B, nq_of(S), max_samples) + sk_align((size_t)B * (1 + 3 * MAXS * MAXS) * sizeof(double), 256);  // + best scores, fp64 pair matrix, sums
}

extern "C" int sk_sisdr_pit_fwd(const float* est, const int64_t* est_offs, const void* ref, int pcm16,
                                const int64_t* ref_offs, const int32_t* nsamp, int B, int S, int max_samples,
                                const float* count_dev, float* pair, float* perm_score, int32_t* best_perm, float* out,
                                float* coef, void* ws, sk_stream_t stream) {
  SK_CHECK_ARG(S >= 1 && S <= MAXS, "sk_sisdr_pit_fwd: num_spk %d outside 1..%d", S, MAXS);
  SK_CHECK_ARG(est && est_offs && ref && ref_offs && nsamp && pair && perm_score && best_perm && out && coef && ws,
               "sk_sisdr_pit_fwd: null pointer");
  SK_CHECK_ARG(B > 0 && B <= 65535, "sk_sisdr_pit_fwd: B = %d utterances outside 1..65535", B);
  SK_CHECK_ARG(max_samples > 0, "sk_sisdr_pit_fwd: max_samples = %d, at least 1 expected", max_samples);
  const int nch = (int)sk_cdiv(max_samples, CHUNK);
  double* partial = (double*)ws;
  double* best_score = (double*)((char*)ws + partial_bytes(B, nq_of(S), max_samples));
  double* pair64 = best_score + B;
  double* sums = pair64 + (size_t)B * MAXS * MAXS;  // B x (4 S + S^2) <= B x 2 MAXS^2
  dim3 grid((unsigned)nch, (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  const sums_kernel_t sums_kernel[MAXS] = {sisdr_sums_kernel<1>, sisdr_sums_kernel<2>, sisdr_sums_kernel<3>, sisdr_sums_kernel<4>};
  hipLaunchKernelGGL(sums_kernel[S - 1], grid, dim3(256), 0, st, est, est_offs, ref, pcm16, ref_offs, nsamp, nch, partial);
  SK_CHECK_LAUNCH("sisdr_sums_kernel");
  hipLaunchKernelGGL(sisdr_finalize_kernel, dim3(1), dim3(256), 0, st, partial, nch, nsamp, B, S, count_dev, best_score, pair64, sums, pair,
                     perm_score, best_perm, out, coef);
  SK_CHECK_LAUNCH("sisdr_finalize_kernel");
  return SK_OK;
}
