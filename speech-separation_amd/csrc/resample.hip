// resample.hip -- band-limited sinc resampling of a ragged batch of signals (sk_resample), gfx950.
//
// The `sr=` half of librosa.core.load (reference steps/extract_feats.py:74,85,97,104, steps/evaluate_oracle.py:96,122); the
// arithmetic is defined in sepkern/resample.py, which also makes the tap table.  For the rate ratio L / M (coprime) output n
// of a signal is
//     y[n] = sum_{i < ntaps} taps[i][n mod L] * x[first(n) + i],   first(n) = floor((n M - 64 max(L, M)) / L) + 1,
// x = 0 outside the signal, summed in fp32 with i ascending: a fixed order, so two launches agree bit for bit.
//
// One workgroup of 256 threads produces a tile of `tile` (1024 where it fits) consecutive outputs of one signal.  It stages
// the input span the tile reads -- first(n0) .. first(n0 + tile - 1) + ntaps, (tile - 1) M / L + 2 + ntaps samples: 2305 floats
// for 1024 outputs at 2:1 -- into LDS once, converting int16 PCM on the way in and writing zeros beyond the signal's ends, so
// that every input sample leaves HBM about once (instead of ntaps L / M times) and the inner loop carries no bounds check.
// Thread t takes outputs n0 + t, n0 + t + 256, ... (4, 2 or 1 of them, summed side by side): a wave's 64 lanes own 64 consecutive outputs, stored coalesced.  Their
// phases (n M) mod L step by M mod L, which is why the table is indexed by n mod L rather than by phase and kept tap-major:
// per tap the wave reads 64 consecutive floats (wrapping at L) -- two or three cache lines from L2 / L1, not 64 rows.  With
// L == 1 (integer decimation) every lane reads the same tap: the single row goes to LDS behind the samples and is read as a
// broadcast.  The lanes' sample reads are M / L floats apart: 2-way bank conflicts at 2:1 and 6:1 (ds_read_b32 is served per
// 32-lane half on 32 banks).  One LDS read per FMA is what bounds the kernel (108 us for 96 signals of 64 000 samples at 2:1,
// profiles/resample.txt); the job is small next to a training step and is left at that.
#include "sk_common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_NUM_ZEROS = 64;
constexpr int RS_LDS_BYTES = 60 * 1024;  // per workgroup: the tile shrinks (1024, 512, 256 outputs) until its span fits

__host__ __device__ __forceinline__ int64_t rs_floor_div(int64_t a, int64_t b) {  // b > 0
  int64_t q = a / b;
  return (a % b < 0) ? q - 1 : q;
}

// samples of LDS a tile of `tile` outputs stages: first(n0 + tile - 1) - first(n0) <= floor((tile - 1) M / L) + 1
__host__ __device__ __forceinline__ int64_t rs_span(int tile, int L, int M, int ntaps) {
  return (int64_t)(tile - 1) * M / L + 2 + ntaps;
}

// NPT = outputs per thread (tile = 256 NPT).  A thread's outputs n0 + t + 256 j are summed side by side, each in its own
// accumulator and each with i ascending -- the order above --, so NPT independent FMA chains are in flight, and with L == 1
// one tap read from LDS serves all NPT of them.
template <int NPT>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const void* __restrict__ in, int pcm16,
                                                              const int64_t* __restrict__ in_offs,
                                                              const int32_t* __restrict__ n_in, const float* __restrict__ taps,
                                                              int L, int M, int ntaps, int span, float* __restrict__ out,
                                                              const int64_t* __restrict__ out_offs,
                                                              const int32_t* __restrict__ n_out) {
  extern __shared__ float rs_lds[];  // `span` samples, then (L == 1) the ntaps taps
  constexpr int tile = NPT * RS_THREADS;
  const int sig = blockIdx.y;
  const int NO = n_out[sig];
  const int n0 = blockIdx.x * tile;
  if (n0 >= NO) return;  // block-uniform
  const int NI = n_in[sig];
  const int tid = threadIdx.x;
  const int64_t half = (int64_t)RS_NUM_ZEROS * max(L, M);
  const int64_t base = rs_floor_div((int64_t)n0 * M - half, L) + 1;  // first(n0)
  const int64_t ioff = in_offs[sig];
  if (pcm16) {
    const int16_t* x = (const int16_t*)in + ioff;
    for (int i = tid; i < span; i += RS_THREADS) {
      const int64_t k = base + i;
      rs_lds[i] = (k >= 0 && k < NI) ? (float)x[k] * (1.0f / 32768.0f) : 0.f;
    }
  } else {
    const float* x = (const float*)in + ioff;
    for (int i = tid; i < span; i += RS_THREADS) {
      const int64_t k = base + i;
      rs_lds[i] = (k >= 0 && k < NI) ? x[k] : 0.f;
    }
  }
  if (L == 1)
    for (int i = tid; i < ntaps; i += RS_THREADS) rs_lds[span + i] = taps[i];
  __syncthreads();

  const int nend = min(n0 + tile, NO);
  const float* xs[NPT];
  float acc[NPT];
#pragma unroll
  for (int j = 0; j < NPT; ++j) {
    const int n = n0 + tid + j * RS_THREADS;
    // first(n) - first(n0): inside [0, span - ntaps] by rs_span's bound; an output past the end reads the tile's first window
    xs[j] = rs_lds + (n < nend ? (int)(rs_floor_div((int64_t)n * M - half, L) + 1 - base) : 0);
    acc[j] = 0.f;
  }
  if (L == 1) {
    const float* tp = rs_lds + span;
#pragma unroll 4
    for (int i = 0; i < ntaps; ++i) {
      const float h = tp[i];
#pragma unroll
      for (int j = 0; j < NPT; ++j) acc[j] = fmaf(h, xs[j][i], acc[j]);
    }
  } else {
    const float* tp[NPT];
#pragma unroll
    for (int j = 0; j < NPT; ++j) tp[j] = taps + (n0 + tid + j * RS_THREADS) % L;  // row i at tp + i L: inside the table
#pragma unroll 4
    for (int i = 0; i < ntaps; ++i) {
#pragma unroll
      for (int j = 0; j < NPT; ++j) acc[j] = fmaf(tp[j][(int64_t)i * L], xs[j][i], acc[j]);
    }
  }
  float* const y = out + out_offs[sig];
#pragma unroll
  for (int j = 0; j < NPT; ++j) {
    const int n = n0 + tid + j * RS_THREADS;
    if (n < nend) y[n] = acc[j];
  }
}

int rs_gcd(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

}  // namespace

extern "C" int sk_resample(const void* in, int pcm16, const int64_t* in_offs, const int32_t* n_in, int nsig,
                           const float* taps, int L, int M, int ntaps, float* out, const int64_t* out_offs,
                           const int32_t* n_out, int max_out, sk_stream_t stream) {
  SK_CHECK_ARG(L >= 1 && M >= 1 && L <= 65536 && M <= 65536, "sk_resample: rate ratio L / M = %d / %d outside 1..65536", L, M);
  SK_CHECK_ARG(L != M, "sk_resample: L == M (%d) is no rate change", L);
  SK_CHECK_ARG(rs_gcd(L, M) == 1, "sk_resample: L / M = %d / %d is not in lowest terms", L, M);
  const int64_t want = (int64_t)2 * RS_NUM_ZEROS * std::max(L, M) / L + 1;
  SK_CHECK_ARG(ntaps == want, "sk_resample: ntaps %d does not match L / M = %d / %d (%lld taps per phase)", ntaps, L, M,
               (long long)want);
  SK_CHECK_ARG(in && in_offs && n_in && taps && out && out_offs && n_out, "sk_resample: null pointer");
  SK_CHECK_ARG(nsig > 0 && nsig <= 65535 && max_out > 0, "sk_resample: bad nsig/max_out");
  int tile = 1024;
  const int64_t row = (L == 1) ? ntaps : 0;
  while (tile > 256 && (rs_span(tile, L, M, ntaps) + row) * 4 > RS_LDS_BYTES) tile /= 2;
  const int64_t span = rs_span(tile, L, M, ntaps);
  SK_CHECK_ARG((span + row) * 4 <= RS_LDS_BYTES, "sk_resample: the ratio %d / %d needs %lld bytes of LDS per tile (limit %d)", L,
               M, (long long)((span + row) * 4), RS_LDS_BYTES);
  dim3 grid((unsigned)sk_cdiv(max_out, tile), (unsigned)nsig);
  auto kern = tile == 1024 ? resample_kernel<4> : tile == 512 ? resample_kernel<2> : resample_kernel<1>;
  hipLaunchKernelGGL(kern, grid, dim3(RS_THREADS), (size_t)((span + row) * 4), (hipStream_t)stream, in, pcm16, in_offs, n_in, taps,
                     L, M, ntaps, (int)span, out, out_offs, n_out);
  SK_CHECK_LAUNCH("sk_resample");
  return SK_OK;
}
