// sk_common.h -- shared helpers for libsepkern (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <type_traits>

#include "../../include/sepkern.h"

#define SK_WAVE 64

// thread-local message for the last failing call (sk_last_error)
char* sk_errbuf();
int sk_fail(int code, const char* fmt, ...);
// build-option bits of the translation units that carry diagnostic switches (sk_build_flags)
unsigned sk_gemm_build_flags();
unsigned sk_lstm_build_flags();
// compute units of the current device, queried on first use and cached (0 while the query fails)
int sk_num_cus();

#define SK_CHECK_ARG(cond, ...)                          \
  do {                                                   \
    if (!(cond)) return sk_fail(SK_EINVAL, __VA_ARGS__); \
  } while (0)

#define SK_CHECK_LAUNCH(what)                                                       \
  do {                                                                              \
    hipError_t e__ = hipGetLastError();                                             \
    if (e__ != hipSuccess) return sk_fail(SK_ELAUNCH, "%s: %s", what, hipGetErrorString(e__)); \
  } while (0)

#define SK_CHECK_HIP(expr)                                                                   \
  do {                                                                                       \
    hipError_t e__ = (expr);                                                                 \
    if (e__ != hipSuccess) return sk_fail(SK_ELAUNCH, "%s: %s", #expr, hipGetErrorString(e__)); \
  } while (0)

static inline int64_t sk_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline size_t sk_align(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- what the array kernels (mvdr, wpe, wpd, cacgmm) share on the host ------------------------------------------------------
// A runtime n in LO..HI as a compile-time constant: f(std::integral_constant<int, n>{}).  The caller has checked the range; a
// value outside it takes HI.
template <int LO, int HI, class F>
inline int sk_dispatch_int(int n, F&& f) {
  if constexpr (LO == HI) {
    return f(std::integral_constant<int, HI>{});
  } else {
    return n == LO ? f(std::integral_constant<int, LO>{}) : sk_dispatch_int<LO + 1, HI>(n, f);
  }
}

// One launch with `lds` bytes of dynamic LDS, refused above `limit`.  A kernel's dynamic LDS above 64 KB has to be allowed
// first, on the device the launch goes to: asked for per call, as no cached answer holds for another device or is safe between
// host threads.  `entry` is the C entry point's name, for the message.
template <class... P, class... A>
inline int sk_launch_lds(const char* entry, const char* what, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, int limit,
                         hipStream_t st, A... args) {
  if (lds > (size_t)limit) return sk_fail(SK_EINVAL, "%s: %zu bytes of LDS per workgroup (limit %d)", entry, lds, limit);
  if (lds > 64 * 1024) SK_CHECK_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
  SK_CHECK_LAUNCH(what);
  return SK_OK;
}

// The checks of the block arguments, one line each so that an entry point keeps its own order; `who` is its name, a literal.
#define SK_CHECK_FRAMES(who, T) SK_CHECK_ARG((T) >= 1, who ": T = %d frames, at least 1 expected", T)
#define SK_CHECK_BLOCK_FRAMES(who, Lb) SK_CHECK_ARG((Lb) >= 1, who ": block_frames = %d, at least 1 expected", Lb)
#define SK_CHECK_WINDOW(who, Lb, Lc, maxwin)                                                                            \
  do {                                                                                                                  \
    SK_CHECK_ARG((Lc) >= 0, who ": context_frames = %d is negative", Lc);                                               \
    SK_CHECK_ARG((int64_t)(Lb) + 2 * (int64_t)(Lc) <= (maxwin),                                                         \
                 who ": a window of block_frames + 2 context_frames = %lld frames, at most %d", (long long)(Lb) + 2 * (long long)(Lc), maxwin); \
  } while (0)
#define SK_CHECK_REF(who, ref, C) SK_CHECK_ARG((ref) >= 0 && (ref) < (C), who ": ref = %d outside [0, %d)", ref, C)
#define SK_CHECK_LOADING(who, loading) SK_CHECK_ARG((loading) >= 0.0, who ": loading = %g is negative or NaN", loading)
#define SK_CHECK_Y_ROW_STRIDE(who, yrs) SK_CHECK_ARG((yrs) >= 257, who ": y_row_stride = %lld below 257", (long long)(yrs))
#define SK_CHECK_LD_MASK(who, ld, S) SK_CHECK_ARG((ld) >= (S) * 257, who ": ld_mask = %d below S * 257 = %d", ld, (S) * 257)

// ---- device helpers ------------------------------------------------------------------------
__device__ __forceinline__ float sk_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Block-wide sum for blockDim.x == 256 (4 waves); result valid in every thread.
__device__ __forceinline__ float sk_block_sum256(float v, float* red /* >= 4 floats of LDS */) {
  v = sk_wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- what the waveform-batch kernels (mix.hip, noise.hip) share ---------------------------------------------------------------
// sample i of a signal: float32 as it is, int16 PCM scaled by 1/32768 (exact)
template <bool PCM>
__device__ __forceinline__ float sk_sample(const void* base, unsigned i) {
  if (PCM) return (float)((const int16_t*)base)[i] * (1.0f / 32768.0f);
  return ((const float*)base)[i];
}

// v on the int16 grid: what a 16-bit wav file would hand back
__device__ __forceinline__ float sk_quant16(float v) { return fminf(fmaxf(rintf(v * 32768.0f), -32768.0f), 32767.0f) * (1.0f / 32768.0f); }

// Lexicographic permutation number `idx` of {0..S-1} (itertools.permutations order), S <= SK_MAXS: element i of the
// permutation in bits 2i, 2i+1 of the result (no arrays: nothing a kernel would keep in scratch).
#define SK_MAXS 4
__device__ __forceinline__ unsigned sk_nth_perm_code(int idx, int S) {
  unsigned avail = 0xE4u, code = 0u;  // the elements still free, in increasing order, two bits each
  int fact = 1;
  for (int i = 2; i < S; ++i) fact *= i;  // (S-1)!
  for (int i = 0; i < S; ++i) {
    const int q = idx / fact;
    idx -= q * fact;
    code |= ((avail >> (2 * q)) & 3u) << (2 * i);
    avail = (avail & ((1u << (2 * q)) - 1u)) | ((avail >> (2 * q + 2)) << (2 * q));
    if (S - 1 - i > 0) fact /= (S - 1 - i);
  }
  return code;
}
__device__ __forceinline__ void sk_nth_perm(int idx, int S, int* perm) {
  const unsigned code = sk_nth_perm_code(idx, S);
  for (int i = 0; i < S; ++i) perm[i] = (int)((code >> (2 * i)) & 3u);
}

__device__ __forceinline__ float sk_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
