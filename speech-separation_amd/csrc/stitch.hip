// stitch.hip -- the masks of overlapping windows of one long recording put back together (sk_stitch).
//
// No counterpart in the reference, which separates whole test utterances in one pass (steps/eval_qsub.py); sepkern/stitch.py
// states the definition (continuous speech separation: windows of the training length, the output order of neighbouring
// windows aligned on the frames they share, a cross-fade) and restates it in numpy.  Three streaming launches on one stream,
// no atomics, no hand-off between workgroups, no host synchronisation:
//   stitch_cost_kernel    boundary x chunk of CCH overlap frames: the S x S magnitude-weighted squared distances between the
//                         outputs of the two windows, fp64, one partial per (boundary, chunk) in a fixed workspace slot
//   stitch_finish_kernel  one workgroup: per boundary the chunks added in ascending order, the S! permutation sums (on
//                         registers) and the first minimum; then the chain PI_{k+1} = p_k o PI_k, 256 boundaries at a time
//   stitch_blend_kernel   FR output frames per workgroup, lanes over the S * 257 columns: each output element is written
//                         once, from the one or two windows that cover its frame, each read at its permuted column
// Window k is addressed by a descriptor (offset, row stride), so the masks stay where the network wrote them.  The 257-column
// blocks of a permuted row put source and destination at different 16-byte phases: lanes move one dword each, 256 contiguous
// bytes per wave instruction, in all three kernels.
#include "sk_common.h"

namespace {

constexpr int MAXS = SK_MAXS;
constexpr int NBIN = 257;
constexpr int CCH = 16;   // overlap frames per workgroup of the cost launch
constexpr int FR = 4;     // output frames per workgroup of the blend launch
constexpr int FCH = 256;  // boundaries per round of the finish launch (= its workgroup size)

// Block-wide fp64 sum for blockDim.x == 256, one fixed order; result valid in every thread.
__device__ __forceinline__ double block_sum256_f64(double v, double* red /* >= 4 doubles of LDS */) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

template <int S>
__global__ __launch_bounds__(256) void stitch_cost_kernel(const float* __restrict__ mag, int ld_mag,
                                                          const float* __restrict__ mask,
                                                          const int64_t* __restrict__ win_offs,
                                                          const int64_t* __restrict__ win_st, int Hn, int O,
                                                          double* __restrict__ partial /* (K-1, nch, S*S) */) {
  __shared__ double red[4];
  const int k = blockIdx.x, ch = blockIdx.y, nch = gridDim.y;
  const int o0 = ch * CCH, nfr = min(CCH, O - o0);
  const float* __restrict__ xa = mag + ((int64_t)(k + 1) * Hn + o0) * ld_mag;
  const int64_t sta = win_st[k], stb = win_st[k + 1];
  const float* __restrict__ ma = mask + win_offs[k] + (int64_t)(Hn + o0) * sta;  // the earlier window's last O frames
  const float* __restrict__ mb = mask + win_offs[k + 1] + (int64_t)o0 * stb;    // the later window's first O frames
  double acc[S][S];
#pragma unroll
  for (int i = 0; i < S; ++i)
#pragma unroll
    for (int j = 0; j < S; ++j) acc[i][j] = 0.0;
  auto element = [&](int dt, int f) {
    const double x = (double)xa[(int64_t)dt * ld_mag + f];
    double b[S];
#pragma unroll
    for (int j = 0; j < S; ++j) b[j] = (double)mb[dt * stb + j * NBIN + f];
#pragma unroll
    for (int i = 0; i < S; ++i) {
      const double a = (double)ma[dt * sta + i * NBIN + f];
#pragma unroll
      for (int j = 0; j < S; ++j) {
        const double d = x * (a - b[j]);
        acc[i][j] += d * d;
      }
    }
  };
  // as pit_pair_kernel: the thread's bin fixed, the chunk's frames as the inner loop; bin 256 of frame tid goes to thread tid
#pragma unroll 4
  for (int dt = 0; dt < nfr; ++dt) element(dt, threadIdx.x);
  if ((int)threadIdx.x < nfr) element(threadIdx.x, 256);
#pragma unroll
  for (int i = 0; i < S; ++i)
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const double v = block_sum256_f64(acc[i][j], red);
      if (threadIdx.x == 0) partial[((int64_t)k * nch + ch) * (S * S) + i * S + j] = v;
    }
}

// PI' = p o PI on permutation codes (element i in bits 2i, 2i+1, as sk_nth_perm_code makes them)
__device__ __forceinline__ unsigned compose_code(unsigned p, unsigned pi, int S) {
  unsigned r = 0u;
  for (int s = 0; s < S; ++s) r |= ((p >> (2 * ((pi >> (2 * s)) & 3u))) & 3u) << (2 * s);
  return r;
}

template <int S>
__global__ __launch_bounds__(FCH) void stitch_finish_kernel(const double* __restrict__ partial, int nch, int K,
                                                            double* __restrict__ cost, int32_t* __restrict__ perms) {
  constexpr int SS = S * S, NPERM = S == 1 ? 1 : S == 2 ? 2 : S == 3 ? 6 : 24;
  __shared__ unsigned code[FCH];  // p_k of the round's boundaries, then PI_{k+1}
  __shared__ unsigned carry;      // PI of the round's first window
  const int tid = threadIdx.x;
  if (tid == 0) carry = 0xE4u;  // the identity
  if (tid < S) perms[tid] = tid;
  for (int k0 = 0; k0 < K - 1; k0 += FCH) {
    const int k = k0 + tid, n = min(FCH, K - 1 - k0);
    if (tid < n) {
      // the S x S sums stay in registers: every loop below is unrolled, every index a constant (no scratch); a chunk's S*S
      // partials are one contiguous run, and the chunks are added in ascending order
      const double* __restrict__ pk = partial + (int64_t)k * nch * SS;
      double pr[SS];
#pragma unroll
      for (int q = 0; q < SS; ++q) pr[q] = 0.0;
      for (int c = 0; c < nch; ++c) {
#pragma unroll
        for (int q = 0; q < SS; ++q) pr[q] += pk[c * SS + q];
      }
#pragma unroll
      for (int q = 0; q < SS; ++q) cost[(int64_t)k * SS + q] = pr[q];
      unsigned bestc = 0xE4u;
      double best = 0.0;
#pragma unroll
      for (int p = 0; p < NPERM; ++p) {
        const unsigned pc = sk_nth_perm_code(p, S);
        double l = 0.0;
#pragma unroll
        for (int i = 0; i < S; ++i) l += pr[i * S + ((pc >> (2 * i)) & 3u)];
        if (p == 0 || l < best) {
          best = l;
          bestc = pc;
        }
      }
      code[tid] = bestc;
    }
    __syncthreads();
    if (tid == 0) {  // the chain is sequential, on register-held codes
      unsigned pi = carry;
      for (int i = 0; i < n; ++i) {
        pi = compose_code(code[i], pi, S);
        code[i] = pi;
      }
      carry = pi;
    }
    __syncthreads();
    if (tid < n) {
#pragma unroll
      for (int s = 0; s < S; ++s) perms[(int64_t)(k + 1) * S + s] = (int32_t)((code[tid] >> (2 * s)) & 3u);
    }
    __syncthreads();
  }
}

template <int S>
__global__ __launch_bounds__(256) void stitch_blend_kernel(const float* __restrict__ mask,
                                                           const int64_t* __restrict__ win_offs,
                                                           const int64_t* __restrict__ win_st,
                                                           const int32_t* __restrict__ perms,
                                                           const float* __restrict__ ramp, int T, int Hn, int O, int K,
                                                           float* __restrict__ out, int ld_out) {
  constexpr int SF = S * NBIN;
  __shared__ int64_t src_late[FR][S], src_early[FR][S];  // element offset of (frame, output)'s 257 values (any sign)
  __shared__ float weight[FR];
  __shared__ int covered_twice[FR];
  const int t0 = blockIdx.x * FR, nrows = min(FR, T - t0);
  if ((int)threadIdx.x < nrows * S) {
    const int r = threadIdx.x / S, s = threadIdx.x - r * S, t = t0 + r;
    const int kl = min(t / Hn, K - 1), o = t - kl * Hn;  // the later (or only) window that covers t, and t inside it
    src_late[r][s] = win_offs[kl] + (int64_t)o * win_st[kl] + perms[(int64_t)kl * S + s] * NBIN;
    const bool two = kl > 0 && o < O;
    src_early[r][s] = two ? win_offs[kl - 1] + (int64_t)(o + Hn) * win_st[kl - 1] + perms[(int64_t)(kl - 1) * S + s] * NBIN : 0;
    if (s == 0) {
      weight[r] = two ? ramp[o] : 0.f;
      covered_twice[r] = two;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nrows * SF; i += 256) {
    const int r = i / SF, c = i - r * SF, s = c / NBIN, f = c - s * NBIN;
    float v = mask[src_late[r][s] + f];
    if (covered_twice[r]) {  // a + w (b - a): a subtraction, a multiplication and an addition, each rounded -- never a fused multiply-add
#pragma clang fp contract(off)
      const float a = mask[src_early[r][s] + f];
      const float p = weight[r] * (v - a);
      v = a + p;
    }
    out[(int64_t)(t0 + r) * ld_out + c] = v;
  }
}

inline int stitch_windows(int T, int W, int Hn) { return 1 + (int)sk_cdiv(T > W ? T - W : 0, Hn); }
inline bool stitch_shape_ok(int T, int W, int Hn, int S) {
  return S >= 1 && S <= MAXS && T >= 1 && W >= 2 && Hn < W && 2 * (int64_t)Hn >= W && sk_cdiv(W - Hn, CCH) <= 65535;
}

}  // namespace

// [partials (K-1, nch, S*S) fp64]
extern "C" size_t sk_stitch_workspace_bytes(int T, int W, int Hn, int S) {
  if (!stitch_shape_ok(T, W, Hn, S)) return 0;
  const int K = stitch_windows(T, W, Hn);
  return sk_align((size_t)(K - 1) * sk_cdiv(W - Hn, CCH) * S * S * sizeof(double), 256) + 256;
}

extern "C" int sk_stitch(const float* mag_rows, int ld_mag, const float* mask, const int64_t* win_offs,
                         const int64_t* win_st, int T, int W, int Hn, int S, const float* ramp, float* out, int ld_out,
                         int32_t* perms, double* cost, void* ws, sk_stream_t stream) {
  SK_CHECK_ARG(S >= 1 && S <= MAXS, "sk_stitch: S = %d outputs outside 1..%d", S, MAXS);
  SK_CHECK_ARG(T >= 1, "sk_stitch: T = %d frames, at least 1 expected", T);
  SK_CHECK_ARG(W >= 2 && Hn < W && 2 * (int64_t)Hn >= W, "sk_stitch: hop Hn = %d outside [W/2, W) for W = %d", Hn, W);
  SK_CHECK_ARG(stitch_shape_ok(T, W, Hn, S), "sk_stitch: overlap W - Hn = %d beyond %d frames", W - Hn, 65535 * CCH);
  SK_CHECK_ARG(mask && win_offs && win_st && out && perms, "sk_stitch: null pointer (mask, win_offs, win_st, out or perms)");
  SK_CHECK_ARG(ld_out >= S * NBIN, "sk_stitch: ld_out = %d below S * 257 = %d", ld_out, S * NBIN);
  const int K = stitch_windows(T, W, Hn), O = W - Hn;
  const int nch = (int)sk_cdiv(O, CCH);
  hipStream_t st = (hipStream_t)stream;
  if (K > 1) {
    SK_CHECK_ARG(ws, "sk_stitch: ws is NULL, %zu bytes of workspace expected", sk_stitch_workspace_bytes(T, W, Hn, S));
    SK_CHECK_ARG(mag_rows && ramp && cost, "sk_stitch: null pointer (mag_rows, ramp or cost) with %d windows", K);
    SK_CHECK_ARG(ld_mag >= NBIN, "sk_stitch: ld_mag = %d below 257", ld_mag);
    dim3 grid((unsigned)(K - 1), (unsigned)nch);
    double* partial = (double*)ws;
    switch (S) {
      case 1: hipLaunchKernelGGL(stitch_cost_kernel<1>, grid, dim3(256), 0, st, mag_rows, ld_mag, mask, win_offs, win_st, Hn, O, partial); break;
      case 2: hipLaunchKernelGGL(stitch_cost_kernel<2>, grid, dim3(256), 0, st, mag_rows, ld_mag, mask, win_offs, win_st, Hn, O, partial); break;
      case 3: hipLaunchKernelGGL(stitch_cost_kernel<3>, grid, dim3(256), 0, st, mag_rows, ld_mag, mask, win_offs, win_st, Hn, O, partial); break;
      default: hipLaunchKernelGGL(stitch_cost_kernel<4>, grid, dim3(256), 0, st, mag_rows, ld_mag, mask, win_offs, win_st, Hn, O, partial); break;
    }
    SK_CHECK_LAUNCH("stitch_cost_kernel");
  }
  switch (S) {
    case 1: hipLaunchKernelGGL(stitch_finish_kernel<1>, dim3(1), dim3(FCH), 0, st, (const double*)ws, nch, K, cost, perms); break;
    case 2: hipLaunchKernelGGL(stitch_finish_kernel<2>, dim3(1), dim3(FCH), 0, st, (const double*)ws, nch, K, cost, perms); break;
    case 3: hipLaunchKernelGGL(stitch_finish_kernel<3>, dim3(1), dim3(FCH), 0, st, (const double*)ws, nch, K, cost, perms); break;
    default: hipLaunchKernelGGL(stitch_finish_kernel<4>, dim3(1), dim3(FCH), 0, st, (const double*)ws, nch, K, cost, perms); break;
  }
  SK_CHECK_LAUNCH("stitch_finish_kernel");
  dim3 bgrid((unsigned)sk_cdiv(T, FR));
  switch (S) {
    case 1: hipLaunchKernelGGL(stitch_blend_kernel<1>, bgrid, dim3(256), 0, st, mask, win_offs, win_st, perms, ramp, T, Hn, O, K, out, ld_out); break;
    case 2: hipLaunchKernelGGL(stitch_blend_kernel<2>, bgrid, dim3(256), 0, st, mask, win_offs, win_st, perms, ramp, T, Hn, O, K, out, ld_out); break;
    case 3: hipLaunchKernelGGL(stitch_blend_kernel<3>, bgrid, dim3(256), 0, st, mask, win_offs, win_st, perms, ramp, T, Hn, O, K, out, ld_out); break;
    default: hipLaunchKernelGGL(stitch_blend_kernel<4>, bgrid, dim3(256), 0, st, mask, win_offs, win_st, perms, ramp, T, Hn, O, K, out, ld_out); break;
  }
  SK_CHECK_LAUNCH("stitch_blend_kernel");
  return SK_OK;
}
