// wave_loss.h -- what the waveform losses (sisdr.hip, mixit.hip and their gradient kernels in stft.hip) share: the reference
// read and the fp64 sums skeleton.  A sums kernel gives one workgroup one chunk of CHUNK samples of one utterance: a thread
// adds its samples in index order (the loss's own statements), chunk_store adds the workgroup's threads by a fixed shuffle
// tree; the finalize kernel (one workgroup) adds an utterance's chunks in chunk order (gather_chunks), searches per utterance
// (the loss's own code), and adds the best scores in utterance order (tally_scores).  No atomics; the chunk grid of an
// utterance depends on its own length only, so each value has one order of operations whatever else is in the batch.
//
// Shape coverage: tests/test_gpu_wave_cases.py runs the skeleton through both losses -- a second trip of gather_chunks' stride
// loop (B * NQ > 256), of the finalize loops and a tally over B = 257, grids with more chunks than any utterance has over a
// workspace of exactly the queried size that holds NaN -- against fp64 (cases and the edges they claim: tests/_wave_cases.py).
#pragma once
#include "sk_common.h"

namespace {

constexpr int CHUNK = 4096;  // samples per workgroup of a sums kernel: 16 per thread

// Sample n of the reference that starts at `off`, as stored, float32 or int16 PCM; the 2^-15 of PCM is the caller's (folded
// into a coefficient, or ref_f64).  (off and n arrive apart and are added per branch: added at the call, the shared index
// changed the register allocation of mixit_sums_kernel<4> from 60 VGPRs to 72.)
__device__ __forceinline__ float ref_raw(const void* ref, int pcm16, int64_t off, int n) {
  return pcm16 ? (float)((const int16_t*)ref)[off + n] : ((const float*)ref)[off + n];
}

// The same sample in fp64; int16 PCM scaled by 2^-15: exact in fp32 and in fp64.
__device__ __forceinline__ double ref_f64(const void* ref, int pcm16, int64_t off, int n) {
  return pcm16 ? (double)((const int16_t*)ref)[off + n] * (1.0 / 32768.0) : (double)((const float*)ref)[off + n];
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Every sums kernel: grid (chunks of the longest utterance, B), 256 threads, partial[(u * nch + ch) * NQ + q].
typedef void (*sums_kernel_t)(const float* est, const int64_t* est_offs, const void* ref, int pcm16, const int64_t* ref_offs,
                              const int32_t* nsamp, int nch, double* partial);

// The tail of a sums kernel (256 threads): acc[q] over the workgroup -> row[q], the chunk's NQ values of `partial`.
template <int NQ>
__device__ __forceinline__ void chunk_store(const double (&acc)[NQ], double* __restrict__ row) {
  __shared__ double red[4][NQ];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const double v = wave_sum_f64(acc[q]);
    if (lane == 0) red[wave][q] = v;
  }
  __syncthreads();
  if (threadIdx.x < NQ) {
    const int q = threadIdx.x;
    row[q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
  }
}

// The head of a finalize kernel: one thread per (utterance, sum) adds that sum's chunks in chunk order (the chunks below
// ceil(L / CHUNK): the sums kernel wrote no others); sums[u * NQ + q] is complete for every thread on return.
__device__ __forceinline__ void gather_chunks(const double* __restrict__ partial, int nch, const int32_t* __restrict__ nsamp,
                                              int B, int NQ, double* __restrict__ sums) {
  for (int idx = threadIdx.x; idx < B * NQ; idx += 256) {
    const int u = idx / NQ, q = idx - u * NQ;
    const int mych = (nsamp[u] + CHUNK - 1) / CHUNK;
    double a = 0.0;
    for (int c = 0; c < mych; ++c) a += partial[((int64_t)u * nch + c) * NQ + q];
    sums[idx] = a;
  }
  __syncthreads();
}

// The end of a finalize kernel: thread 0 adds the best scores in utterance order -> out = [-mean, count, sum].
__device__ __forceinline__ void tally_scores(const double* __restrict__ best_score, int B, double count, float* __restrict__ out) {
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int u = 0; u < B; ++u) tot += best_score[u];
    out[0] = (float)(-tot / count);
    out[1] = (float)count;
    out[2] = (float)tot;
  }
}

// bytes of `partial`: B utterances x chunks of the longest x NQ sums
inline size_t partial_bytes(int B, int NQ, int max_samples) {
  return sk_align((size_t)B * sk_cdiv(max_samples, CHUNK) * NQ * sizeof(double), 256);
}

}  // namespace
