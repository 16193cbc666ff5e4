// mix.hip -- dynamic mixing: training mixtures made on the device from single-speaker signals (sk_dynamic_mix), and the other
// channels of an array mixture at the gains it found (sk_mix_channels, at the end), gfx950.
//
// The arithmetic is defined in sepkern/mixing.py (the WSJ0-2mix rule: plain mean-square power, one scale for the mixture and
// its sources, the largest of them at `peak`).  For mixture u with sources x_s of n samples, amplitudes amp_s and peak p:
//     P_s = (1/n) sum x_s^2                       fp64: every thread sums its samples in order, then a fixed tree
//     g_s = fp32(amp_s / sqrt(P_s)), 0 where P_s < 2^-40                               (formed in fp64, rounded once)
//     m   = max_n max(|chain_n(g)|, max_s |g_s x_s[n]|)                                 fp32; a maximum has no order
//     c   = fp32(p / m), 0 where m == 0;   G_s = g_s * c  (fp32)
//     source s = G_s x_s[n],   mixture = chain_n(G),   chain_n(a) = fmaf(a_{S-1}, x_{S-1}[n], ... fmaf(a_0, x_0[n], 0))
//     quantize: every output v -> clip(rint(32768 v), -32768, 32767) / 32768      (what a 16-bit wav file would hand back)
//
// ONE workgroup of 1024 threads per mixture, three passes over that mixture's samples (sums of squares, maximum, write): no
// workspace, no atomics, no hand-off between workgroups, so a mixture's numbers cannot depend on the batch around it and two
// launches agree bit for bit.  Thread t takes samples t, t + 1024, ...: a wave reads and writes 64 consecutive samples.  The
// second and third reads of the samples (at most a few hundred KB per mixture) come from L2.  A launch lasts as long as its
// longest mixture takes on one CU -- three dependent passes through that CU's memory pipeline --, not as long as HBM would need:
// 37 us for 32 two-source mixtures of up to 64 000 samples, 52 us for 100 (profiles/dynamic_mix.txt).
//
// Shape coverage: tests/test_gpu_wave_cases.py runs dynamic_mix_kernel<1..4, int16 | float32> at 1, 63 | 64, 1023 | 1024 | 1025,
// 4095 | 4096 | 4097 and 8191 | 8192 | 8193 samples, with the maximum alone in the last trip, on and below the silence threshold,
// all silent, and with a clipping quantize, against fp64 (tests/_wave_cases.py names the edge each case is there for).
#include "sk_common.h"

namespace {

constexpr int MX_THREADS = 1024;
constexpr int MX_WAVES = MX_THREADS / SK_WAVE;
constexpr int MX_UNROLL = 4;  // samples per source a thread loads before it uses the first
constexpr double MX_SILENT = 1.0 / 1099511627776.0;  // 2^-40: a source whose mean square is below this gets gain 0

// The samples i0, i0 + 1024, .. (MX_UNROLL of them) of every source, zero beyond the signal's end: all loads of a trip are issued
// before the first is used, so a thread has MX_UNROLL S loads in flight instead of one (a zero adds nothing to a sum or a maximum).
template <int S, bool PCM>
__device__ __forceinline__ void mx_load_trip(const void* const* x, unsigned i0, unsigned n, float (*v)[S]) {
#pragma unroll
  for (int k = 0; k < MX_UNROLL; ++k) {
    const unsigned i = i0 + (unsigned)k * MX_THREADS;
#pragma unroll
    for (int s = 0; s < S; ++s) v[k][s] = (i < n) ? sk_sample<PCM>(x[s], i) : 0.f;
  }
}

template <int S, bool PCM>
__global__ __launch_bounds__(MX_THREADS) void dynamic_mix_kernel(const void* __restrict__ in, const int64_t* __restrict__ in_offs,
                                                                 const int32_t* __restrict__ nsamp, int B,
                                                                 const float* __restrict__ amp, const float* __restrict__ peak,
                                                                 int quantize, float* __restrict__ out,
                                                                 const int64_t* __restrict__ out_offs, float* __restrict__ gains) {
  __shared__ double red_sum[S][MX_WAVES];
  __shared__ float red_max[MX_WAVES];
  const int u = blockIdx.x;
  const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const unsigned n = (unsigned)nsamp[u];
  const void* x[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int64_t o = in_offs[s * B + u];
    x[s] = PCM ? (const void*)((const int16_t*)in + o) : (const void*)((const float*)in + o);
  }

  // pass 1: sums of squares in fp64 -- per thread in sample order, lanes by a butterfly, waves in index order
  double sq[S];
#pragma unroll
  for (int s = 0; s < S; ++s) sq[s] = 0.0;
  float v[MX_UNROLL][S];
  for (unsigned i0 = tid; i0 < n; i0 += MX_UNROLL * MX_THREADS) {
    mx_load_trip<S, PCM>(x, i0, n, v);
#pragma unroll
    for (int k = 0; k < MX_UNROLL; ++k) {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const double d = (double)v[k][s];
        sq[s] += d * d;
      }
    }
  }
#pragma unroll
  for (int s = 0; s < S; ++s) {
    double t = sq[s];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if (lane == 0) red_sum[s][wave] = t;
  }
  __syncthreads();
  float g[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < MX_WAVES; ++w) t += red_sum[s][w];
    const double P = t / (double)n;
    g[s] = (P >= MX_SILENT) ? (float)((double)amp[s * B + u] / sqrt(P)) : 0.f;
  }

  // pass 2: the largest magnitude of the mixture and of every source at the gains g
  float m = 0.f;
  for (unsigned i0 = tid; i0 < n; i0 += MX_UNROLL * MX_THREADS) {
    mx_load_trip<S, PCM>(x, i0, n, v);
#pragma unroll
    for (int k = 0; k < MX_UNROLL; ++k) {
      float acc = 0.f;
#pragma unroll
      for (int s = 0; s < S; ++s) {
        m = fmaxf(m, fabsf(g[s] * v[k][s]));
        acc = fmaf(g[s], v[k][s], acc);
      }
      m = fmaxf(m, fabsf(acc));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (lane == 0) red_max[wave] = m;
  __syncthreads();
  m = red_max[0];
#pragma unroll
  for (int w = 1; w < MX_WAVES; ++w) m = fmaxf(m, red_max[w]);
  const float c = (m == 0.f) ? 0.f : (float)((double)peak[u] / (double)m);
  float G[S];
#pragma unroll
  for (int s = 0; s < S; ++s) G[s] = g[s] * c;
  if (gains != nullptr && tid == 0) {
#pragma unroll
    for (int s = 0; s < S; ++s) gains[s * B + u] = G[s];
  }

  // pass 3: write the mixture (signal 0) and the sources (signals 1 .. S)
  float* y[S + 1];
#pragma unroll
  for (int q = 0; q <= S; ++q) y[q] = out + out_offs[q * B + u];
  for (unsigned i0 = tid; i0 < n; i0 += MX_UNROLL * MX_THREADS) {
    mx_load_trip<S, PCM>(x, i0, n, v);
#pragma unroll
    for (int k = 0; k < MX_UNROLL; ++k) {
      const unsigned i = i0 + (unsigned)k * MX_THREADS;
      if (i >= n) break;
      float acc = 0.f;
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const float r = G[s] * v[k][s];
        acc = fmaf(G[s], v[k][s], acc);
        y[1 + s][i] = quantize ? sk_quant16(r) : r;
      }
      y[0][i] = quantize ? sk_quant16(acc) : acc;
    }
  }
}

// ---- the other channels of an array mixture (sk_mix_channels) ------------------------------------------------------------------
// out_{p,u}[n] = chain_n(G) over channel p's S signals, with the gains sk_dynamic_mix found on the reference channel.
// grid (B, P, MC_SPLIT), 256 threads: workgroup z of a signal takes samples z 256 + t, then every MC_SPLIT 256-th -- one writer
// per element, nothing shared.
constexpr int MC_THREADS = 256;
constexpr int MC_SPLIT = 16;
constexpr int MC_MAXP = 7;

template <int S>
__global__ __launch_bounds__(MC_THREADS) void mix_channels_kernel(const float* __restrict__ in, const int64_t* __restrict__ in_offs,
                                                                  const int32_t* __restrict__ nsamp, int B, int P,
                                                                  const float* __restrict__ gains, int quantize,
                                                                  float* __restrict__ out, const int64_t* __restrict__ out_offs) {
  const int u = blockIdx.x, p = blockIdx.y;
  const unsigned n = (unsigned)nsamp[u];
  const float* x[S];
  float G[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    x[s] = in + in_offs[((int64_t)s * P + p) * B + u];
    G[s] = gains[s * B + u];
  }
  float* const y = out + out_offs[(int64_t)p * B + u];
  for (unsigned i = blockIdx.z * MC_THREADS + threadIdx.x; i < n; i += MC_SPLIT * MC_THREADS) {
    float acc = 0.f;
#pragma unroll
    for (int s = 0; s < S; ++s) acc = fmaf(G[s], x[s][i], acc);
    y[i] = quantize ? sk_quant16(acc) : acc;
  }
}

}  // namespace

extern "C" int sk_mix_channels(const float* in, const int64_t* in_offs, const int32_t* nsamp, int B, int S, int P, const float* gains,
                               int quantize, float* out, const int64_t* out_offs, sk_stream_t stream) {
  SK_CHECK_ARG(S >= 1 && S <= SK_MAXS, "sk_mix_channels: S = %d sources outside 1..%d", S, SK_MAXS);
  SK_CHECK_ARG(P >= 1 && P <= MC_MAXP, "sk_mix_channels: P = %d channels outside 1..%d", P, MC_MAXP);
  SK_CHECK_ARG(B >= 1 && B <= 65535, "sk_mix_channels: B = %d mixtures outside 1..65535", B);
  SK_CHECK_ARG(in && in_offs && nsamp && gains && out && out_offs, "sk_mix_channels: null pointer");
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)B, (unsigned)P, MC_SPLIT);
  const int qz = quantize != 0;
  sk_dispatch_int<1, SK_MAXS>(S, [&](auto s) {
    hipLaunchKernelGGL((mix_channels_kernel<decltype(s)::value>), grid, dim3(MC_THREADS), 0, st, in, in_offs, nsamp, B, P, gains, qz, out,
                       out_offs);
    return 0;
  });
  SK_CHECK_LAUNCH("sk_mix_channels");
  return SK_OK;
}

extern "C" int sk_dynamic_mix(const void* in, int pcm16, const int64_t* in_offs, const int32_t* nsamp, int B, int S,
                              const float* amp, const float* peak, int quantize, float* out, const int64_t* out_offs,
                              float* gains, sk_stream_t stream) {
  SK_CHECK_ARG(S >= 1 && S <= SK_MAXS, "sk_dynamic_mix: S = %d sources outside 1..%d", S, SK_MAXS);
  SK_CHECK_ARG(B >= 1 && B <= 65535, "sk_dynamic_mix: B = %d mixtures outside 1..65535", B);
  SK_CHECK_ARG(in && in_offs && nsamp && amp && peak && out && out_offs, "sk_dynamic_mix: null pointer");
  const hipStream_t st = (hipStream_t)stream;
  const bool p = pcm16 != 0;
  const int qz = quantize != 0;
  sk_dispatch_int<1, SK_MAXS>(S, [&](auto s) {
    constexpr int SS = decltype(s)::value;
    if (p)
      hipLaunchKernelGGL((dynamic_mix_kernel<SS, true>), dim3((unsigned)B), dim3(MX_THREADS), 0, st, in, in_offs, nsamp, B, amp, peak, qz,
                         out, out_offs, gains);
    else
      hipLaunchKernelGGL((dynamic_mix_kernel<SS, false>), dim3((unsigned)B), dim3(MX_THREADS), 0, st, in, in_offs, nsamp, B, amp, peak, qz,
                         out, out_offs, gains);
    return 0;
  });
  SK_CHECK_LAUNCH("sk_dynamic_mix");
  return SK_OK;
}
