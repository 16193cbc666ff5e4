// fft512.h -- the 256-point complex FFT behind every n_fft = 512 transform of the library, with its constants and tables:
// what the STFT-family kernels (stft.hip) and the STOI envelope kernel (stoi.hip) share.  Device code only, for inclusion by
// a .hip file: everything sits in an anonymous namespace, and every translation unit gets its own 6 KB copy of the tables.
//
// The 512 real samples of a frame are packed into 256 complex points; the 256-point FFT is computed by
// SIXTEEN lanes, each holding 16 points: two in-register 16-point FFTs (radix 4 x 4) with ONE transpose
// through LDS in between (256 = 16 x 16), then the real-FFT split, whose mirrored partner Z[256-k] lives
// in lane (16-j)%16 of the same group and is fetched with a cross-lane shuffle.  A wavefront therefore
// transforms 4 frames at once and a workgroup (4 waves) 16 consecutive frames of one utterance, whose
// 75 %-overlapping samples are read from HBM once, coalesced, into LDS.  Compared with one-frame-per-wave
// radix-4 stages (3 LDS exchanges) this is ~6x less LDS traffic and ~2x fewer twiddle multiplies.
#pragma once
#include "sk_common.h"
#include "tables512.inc"

namespace {

constexpr int NFFT = 512;
constexpr int NBIN = 257;
constexpr int HOP = 128;
constexpr int FPB = 16;       // frames per workgroup (STFT and iSTFT): 4 waves x 4 frames
constexpr int XLD = 17;       // padded row of the 16 x 16 transpose (conflict-free column reads)
constexpr int TPB = 5;        // consecutive 16-frame tiles per STFT workgroup (next tile's samples are prefetched)

// Complex numbers are 2-vectors so that additions, scalings and the two halves of a complex product map onto
// the packed fp32 VALU ops (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32, swizzles and signs in their modifiers).
typedef float v2f __attribute__((ext_vector_type(2)));

__device__ __forceinline__ v2f cmul(v2f a, v2f b) {  // (a.x b.x - a.y b.y, a.x b.y + a.y b.x)
  const v2f bs = {-b.y, b.x};
  return a.xx * b + a.yy * bs;
}
__device__ __forceinline__ v2f mul_mi(v2f a) { return (v2f){a.y, -a.x}; }  // a * (-i)
__device__ __forceinline__ v2f conj(v2f a) { return (v2f){a.x, -a.y}; }
__device__ __forceinline__ v2f ld2(const float2* p) { return *reinterpret_cast<const v2f*>(p); }
__device__ __forceinline__ void st2(float2* p, v2f v) { *reinterpret_cast<v2f*>(p) = v; }

// A wave's LDS instructions execute in order, so data exchanged between the lanes of ONE wave needs no
// hardware barrier -- only a compiler fence so that the ds_writes stay ahead of the ds_reads that follow.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// radix-4 DFT of (a, b, c, d) (forward, e^{-i...})
__device__ __forceinline__ void radix4(v2f& a, v2f& b, v2f& c, v2f& d) {
  const v2f s0 = a + c, s1 = a - c, s2 = b + d, s3 = mul_mi(b - d);
  a = s0 + s2;
  b = s1 + s3;
  c = s0 - s2;
  d = s1 - s3;
}

// In-register 16-point DFT, natural order in and out (16 = 4 x 4).
__device__ __forceinline__ void dft16(v2f (&x)[16]) {
  constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, R2 = 0.70710678118654752f;
  // step A: for n2 = 0..3 a radix-4 over n1 of x[4 n1 + n2]  ->  t[k1][n2] kept in x[4 k1 + n2]
#pragma unroll
  for (int n2 = 0; n2 < 4; ++n2) radix4(x[n2], x[4 + n2], x[8 + n2], x[12 + n2]);
  // twiddles W16^(n2 k1): (1,1)=W1 (1,2)=W2 (1,3)=W3 (2,1)=W2 (2,2)=W4 (2,3)=W6 (3,1)=W3 (3,2)=W6 (3,3)=W9
  x[4 + 1] = cmul(x[4 + 1], (v2f){C1, -S1});
  x[4 + 2] = cmul(x[4 + 2], (v2f){R2, -R2});
  x[4 + 3] = cmul(x[4 + 3], (v2f){S1, -C1});
  x[8 + 1] = cmul(x[8 + 1], (v2f){R2, -R2});
  x[8 + 2] = mul_mi(x[8 + 2]);
  x[8 + 3] = cmul(x[8 + 3], (v2f){-R2, -R2});
  x[12 + 1] = cmul(x[12 + 1], (v2f){S1, -C1});
  x[12 + 2] = cmul(x[12 + 2], (v2f){-R2, -R2});
  x[12 + 3] = cmul(x[12 + 3], (v2f){-C1, S1});
  // step B: for k1 = 0..3 a radix-4 over n2  ->  X[k1 + 4 k2] left in x[4 k1 + k2]
#pragma unroll
  for (int k1 = 0; k1 < 4; ++k1) radix4(x[4 * k1 + 0], x[4 * k1 + 1], x[4 * k1 + 2], x[4 * k1 + 3]);
  // transpose the 4 x 4 register tile so that x[k] = X[k]
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = a + 1; b < 4; ++b) {
      const v2f tmp = x[4 * a + b];
      x[4 * a + b] = x[4 * b + a];
      x[4 * b + a] = tmp;
    }
}

// 256-point forward FFT by the 16 lanes of one group (j = lane & 15).  On entry z[n1] = in[16 n1 + j];
// on exit z[k2] = Z[j + 16 k2].  xch: this GROUP's 16 x XLD float2 transpose area in LDS; tw = e^{-2 pi i m/512}.
// The transpose goes through a 16 x XLD FLOAT plane, real parts first, then imaginary parts: half the LDS of a
// complex plane (the STFT workgroup then fits four times per CU instead of three) for twice the LDS instructions.
// t256[16 k1 + j] = W256^(j k1): the inter-stage twiddles laid out so that the 16 lanes of a group read 128 contiguous
// bytes (read from the 512-entry table at (2 j k1) & 511 the even k1 are 2- to 8-way bank conflicts: r03).
__device__ __forceinline__ void fft256_g16(v2f (&z)[16], float* xch, const float2* t256, int j) {
  dft16(z);  // over n1: z[k1] = A[k1][n2 = j]
#pragma unroll
  for (int k1 = 1; k1 < 16; ++k1) z[k1] = cmul(z[k1], ld2(&t256[16 * k1 + j]));  // W256^(j k1)
#pragma unroll
  for (int k1 = 0; k1 < 16; ++k1) xch[k1 * XLD + j] = z[k1].x;
  wave_sync();
  float re[16];
#pragma unroll
  for (int n2 = 0; n2 < 16; ++n2) re[n2] = xch[j * XLD + n2];  // lane j now plays k1 = j
  wave_sync();
#pragma unroll
  for (int k1 = 0; k1 < 16; ++k1) xch[k1 * XLD + j] = z[k1].y;
  wave_sync();
#pragma unroll
  for (int n2 = 0; n2 < 16; ++n2) z[n2] = (v2f){re[n2], xch[j * XLD + n2]};
  wave_sync();
  dft16(z);  // over n2: z[k2] = Z[j + 16 k2]
}

// The two tables fft256_g16 and the real split read, into LDS by a workgroup of 256 threads.  No barrier: the caller's next one
// publishes them.
__device__ __forceinline__ void fft512_tables(float2* tw, float2* t256, int tid) {
  for (int i = tid; i < NFFT; i += 256) tw[i] = g_tw512[i];
  t256[tid] = g_tw512[(2 * (tid & 15) * (tid >> 4)) & 511];
}

}  // namespace
