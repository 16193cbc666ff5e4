// noise.hip -- noisy dynamic mixing, gfx950: the Cholesky factors of a diffuse field's coherence at an array's microphones
// (sk_noise_factors), the field itself from C independent noise signals (sk_diffuse_noise, the hot kernel), and noise added to a
// mixture's channels at a drawn SNR (sk_add_noise).  The definitions are sepkern/noise.py's (Habets, Cohen & Gannot 2008 on the
// library's own 512 / 128 transform); diffuse_f32 there restates the arithmetic of sk_diffuse_noise in numpy float32.
//
// sk_diffuse_noise -- grid (tiles, B), 4 waves = 16 sixteen-lane groups as in stft.hip.  A tile owns 13 hops (1664 samples) of one
// mixture and transforms the 16 frames t = 13 q .. 13 q + 15 that touch them, one frame per group (frame t covers samples
// 128 (t - 3) .. + 511, zero outside [0, n)).  Per group:
//   * the tile's 2 432 samples of one channel are staged in LDS once, coalesced; a group windows its frame and runs the 256-point
//     FFT of fft512.h and the real split: lane l holds bins l + 16 k2 and their mirrors 256 - (l + 16 k2), k2 < 8, and bin 128 --
//     17 per lane, as fir_output_kernel holds its accumulators;
//   * WHERE THE C SPECTRA LIVE: 34 C floats per lane, 272 at C = 8, beside the transform's own ~150 registers.  All in registers
//     the compiler spilled from C = 7 on; all in LDS they would be 16 C 2 KB = 263 KB at C = 8, more than a CU's 160 KB.  So the
//     first four or five channels stay in registers and the last C - 4 (at most three) -- the ones the fewest rows of the mix
//     read -- go to LDS, every thread's bins in slots of its own, which no barrier has to guard;
//   * channel i = C - 1 .. 0: X_i = L[i, 0] N_0, then fmaf(L[i, j], N_j, .) with j ascending; descending, so that N_i is dead once
//     X_i is formed.  X_i is inverted -- the forward transform of the conjugate, as in fir_output_kernel --, times 1/512 and the
//     window, to LDS (16 frames x 512 floats = 32 KB); after a barrier every sample of the tile is the sum of its four frames in
//     ascending frame order times fp32(2/3), and only i < n is stored.
// Row c of the mixture's factors, (c + 1) x 257 floats, is staged in LDS entry-major while channel c is mixed, so that the lanes
// of a group read consecutive words (all 37 KB of them at C = 8 would not fit beside the LDS-resident spectra).  No atomics, no
// workspace, one writer per element: a mixture's bits depend neither on the batch around it nor on the run, and int16 samples
// (scaled by 1/32768, exact) give the bits their float32 copies give.
//
// sk_add_noise -- one workgroup of 1024 threads per mixture, as dynamic_mix_kernel: the two fp64 sums on the reference channel
// (every thread in sample order, lanes by a butterfly, waves in index order), then out_c = fmaf(a, v_c, y_c) over all channels.
#include <cmath>

#include "fft512.h"

namespace {

constexpr int NZ_MINC = 2, NZ_MAXC = 8;
constexpr int NZ_TILE_HOPS = 13;
constexpr int NZ_TILE = NZ_TILE_HOPS * HOP;   // 1664 samples
constexpr int NZ_STAGE = 15 * HOP + NFFT;      // 2432: the samples the tile's 16 frames cover
constexpr int NZ_LROW = 260;                  // floats per staged entry of the factors: bins 0 .. 256, padded
constexpr int NZ_MAX_SAMPLES = 1 << 30;
constexpr int NZ_MAX_B = 65535;
constexpr double NZ_C = 343.0;
constexpr double NZ_EPS = 1.0 / 1048576.0;    // 2^-20
constexpr double NZ_MIN_DIST = 0.01;          // room.MIN_DIRECT
constexpr double NZ_SILENT = 1.0 / 1099511627776.0;  // 2^-40, mixing.SILENT
constexpr int NZ_FCHUNK = 16;                 // mixtures per launch of noise_factors_kernel (their microphones travel as arguments)

// ---- sk_noise_factors ------------------------------------------------------------------------------------------------------------
struct NzMics {
  double m[NZ_FCHUNK][NZ_MAXC][3];
};

// one thread per (mixture, bin): Gamma, the loading and the Cholesky factor in fp64 registers (every loop unrolled)
template <int C>
__global__ __launch_bounds__(256) void noise_factors_kernel(NzMics mics, int nb, double rate, float* __restrict__ L) {
  constexpr int TRI = C * (C + 1) / 2;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= nb * NBIN) return;
  const int u = idx / NBIN, k = idx - u * NBIN;
  const double f = (double)k * rate / (double)NFFT;
  double a[TRI];
#pragma unroll
  for (int i = 0; i < C; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double g = 1.0;
      if (j < i) {
        double d2 = 0.0;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const double t = mics.m[u][i][q] - mics.m[u][j][q];
          d2 += t * t;
        }
        const double x = 2.0 * f * sqrt(d2) / NZ_C;
        g = (x == 0.0) ? 1.0 : sinpi(x) / (M_PI * x);
      }
      a[i * (i + 1) / 2 + j] = (1.0 - NZ_EPS) * g + (i == j ? NZ_EPS : 0.0);
    }
  }
  // Cholesky-Banachiewicz, row by row, in place
#pragma unroll
  for (int i = 0; i < C; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double s = a[i * (i + 1) / 2 + j];
#pragma unroll
      for (int p = 0; p < j; ++p) s -= a[i * (i + 1) / 2 + p] * a[j * (j + 1) / 2 + p];
      a[i * (i + 1) / 2 + j] = (i == j) ? sqrt(s) : s / a[j * (j + 1) / 2 + j];
    }
  }
  float* const o = L + (int64_t)idx * TRI;
#pragma unroll
  for (int e = 0; e < TRI; ++e) o[e] = (float)a[e];
}

// ---- sk_diffuse_noise ------------------------------------------------------------------------------------------------------------
template <int C, bool PCM>
__global__ __launch_bounds__(256) void diffuse_noise_kernel(const void* __restrict__ in, const int64_t* __restrict__ in_offs,
                                                            const int32_t* __restrict__ nsamp, int B, int max_nsamp,
                                                            const float* __restrict__ L, float* __restrict__ out,
                                                            const int64_t* __restrict__ out_offs) {
  constexpr int TRI = C * (C + 1) / 2;
  __shared__ float2 tw[NFFT];
  __shared__ float2 t256[256];
  __shared__ float xch[16][16 * XLD];
  __shared__ float frames[16][NFFT];   // forward: the tile's NZ_STAGE samples of one channel; inverse: the 16 windowed frames
  __shared__ float Lrow[C * NZ_LROW];   // row c of the factors while channel c is mixed: entry j at Lrow[j * NZ_LROW + bin]
  // C >= 5: the last NL channels' spectra -- the ones the fewest rows of the mix read -- live in LDS, every thread's 16 paired
  // bins in slots of its own (no barrier guards them) and bin 128 once per group; four or five stay in registers
  constexpr int NL = (C >= 7) ? 3 : (C >= 5) ? C - 4 : 0, CR = C - NL;
  __shared__ float2 spl[NL ? NL * 16 * 256 : 1];
  __shared__ float2 spl128[NL ? NL * 16 : 1];
  const int u = blockIdx.y, q = blockIdx.x;
  const int n = min(nsamp[u], max_nsamp);
  const int i_lo = q * NZ_TILE;
  if (i_lo >= n) return;   // (the whole workgroup: no barrier has been met)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  fft512_tables(tw, t256, tid);   // (published by the barrier behind the first channel's samples)
  const float* const Lu = L + (int64_t)u * NBIN * TRI;
  const int l = lane & 15, g = lane >> 4, grp = 4 * wave + g;
  const int partner = (lane & 48) | ((16 - l) & 15);
  // the window at this lane's samples r, r + 1, r = 32 m + 2 l -- packed point 16 m + l --, for analysis and synthesis alike
  v2f wv[16];
#pragma unroll
  for (int m = 0; m < 16; ++m) wv[m] = (v2f){g_hann512[32 * m + 2 * l], g_hann512[32 * m + 2 * l + 1]};
  float* const stg = &frames[0][0];
  const int s_lo = i_lo - 3 * HOP;   // the first sample of the tile's first frame

  // forward: sp[c][k2] = N_c[l + 16 k2], sp[c][8 + k2] = N_c[256 - (l + 16 k2)] (lane 0, k2 = 0: bins 0 and 256), sp[c][16] = N_c[128]
  v2f sp[CR][17];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int64_t o = in_offs[c * B + u];
    const float* const xf = (const float*)in + o;
    const int16_t* const xi = (const int16_t*)in + o;
    if (c > 0) __syncthreads();   // the previous channel's samples have been read
    for (int i = tid; i < NZ_STAGE; i += 256) {   // samples s_lo .. s_lo + 2431, read once, coalesced; zero outside [0, n)
      const int s = s_lo + i;
      float v = 0.f;
      if (s >= 0 && s < n) v = PCM ? (float)xi[s] * (1.0f / 32768.0f) : xf[s];
      stg[i] = v;
    }
    __syncthreads();   // (c == 0: also the tables and the factors)
    v2f z[16];
    const float* const mine = stg + HOP * grp + 2 * l;
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1)   // packed point 16 n1 + l <-> samples r, r + 1 of the frame, r = 32 n1 + 2 l
      z[n1] = wv[n1] * *reinterpret_cast<const v2f*>(mine + 32 * n1);
    fft256_g16(z, xch[grp], t256, l);
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) {
      v2f zc;
      zc.x = __shfl(z[15 - k2].x, partner, 64);
      zc.y = __shfl(z[15 - k2].y, partner, 64);
      if (l == 0) zc = z[(16 - k2) & 15];
      const v2f zk = z[k2], cz = conj(zc);
      const v2f A = 0.5f * (zk + cz), Bt = cmul(ld2(&tw[l + 16 * k2]), 0.5f * mul_mi(zk - cz));
      if (c < CR) {
        sp[c < CR ? c : 0][k2] = A + Bt;
        sp[c < CR ? c : 0][8 + k2] = conj(A - Bt);
      } else {
        st2(&spl[((c - CR) * 16 + k2) * 256 + tid], A + Bt);
        st2(&spl[((c - CR) * 16 + 8 + k2) * 256 + tid], conj(A - Bt));
      }
    }
    // bin 128: lane 0's is the true one, and only lane 0's is used
    if (c < CR) sp[c < CR ? c : 0][16] = conj(z[8]);
    else if (l == 0) st2(&spl128[(c - CR) * 16 + grp], conj(z[8]));
  }

  // Channel i = C - 1 .. 0: X_i = sum_{j <= i} L[i, j] N_j with j ascending, inverted and written.  Descending, so that N_i is dead
  // once X_i is formed: the registers hold the C spectra and one X, never two sets.  (The factors come from LDS between the
  // barriers below, which keeps the compiler from forming a later row early and holding it.)
  float* const fr = frames[grp];
#pragma unroll
  for (int ci = 0; ci < C; ++ci) {
    const int c = C - 1 - ci;
    // (the last reads of Lrow lie behind the two barriers of the channel before)
    for (int i = tid; i < (c + 1) * NBIN; i += 256) {
      const int j = i / NBIN, k = i - j * NBIN;
      Lrow[j * NZ_LROW + k] = Lu[k * TRI + c * (c + 1) / 2 + j];
    }
    __syncthreads();
    v2f x[17];
#pragma unroll
    for (int b = 0; b < 17; ++b) {
      const int k = (b < 8) ? l + 16 * b : (b < 16) ? 256 - (l + 16 * (b - 8)) : 128;
      const float* const row = Lrow + k;
      v2f acc = row[0] * sp[0][b];
#pragma unroll
      for (int j = 1; j < C; ++j) {
        if (j <= c) {
          const float f = row[j * NZ_LROW];
          const v2f v = (j < CR) ? sp[j < CR ? j : 0][b]
                                 : ld2(b < 16 ? &spl[((j < CR ? 0 : j - CR) * 16 + (b & 15)) * 256 + tid] : &spl128[(j < CR ? 0 : j - CR) * 16 + grp]);
          acc.x = fmaf(f, v.x, acc.x);
          acc.y = fmaf(f, v.y, acc.y);
        }
      }
      x[b] = acc;
      asm volatile("" ::: "memory");   // bin by bin: with a row's loads all in flight at once the registers do not suffice
    }
    // X -> Z, the 256-point spectrum of y[2m] + i y[2m + 1] (twice it), as fir_output_kernel forms it
    v2f z[16], zb[8];
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) {
      const v2f yk = x[k2], ym = conj(x[8 + k2]);
      const v2f E = yk + ym, O = cmul(yk - ym, conj(ld2(&tw[l + 16 * k2])));
      z[k2] = E + (v2f){-O.y, O.x};
      zb[k2] = conj(E) + (v2f){O.y, O.x};
    }
#pragma unroll
    for (int k2 = 8; k2 < 16; ++k2) {
      v2f v;
      v.x = __shfl(zb[15 - k2].x, partner, 64);
      v.y = __shfl(zb[15 - k2].y, partner, 64);
      if (l == 0) v = (k2 == 8) ? 2.0f * conj(x[16]) : zb[(16 - k2) & 7];
      z[k2] = v;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = conj(z[i]);
    fft256_g16(z, xch[grp], t256, l);   // inverse = conj(forward(conj Z)) / 256
    __syncthreads();                     // the previous channel's frames (at first: the last channel's samples) have been read
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) {    // packed point l + 16 k2 <-> samples r, r + 1, r = 2 l + 32 k2
      const v2f v = {z[k2].x * (1.0f / 512.0f), -z[k2].y * (1.0f / 512.0f)};
      *reinterpret_cast<v2f*>(fr + 2 * l + 32 * k2) = v * wv[k2];
    }
    __syncthreads();
    // sample i_lo + m lies in the tile's hop m / 128, which frames m / 128 .. m / 128 + 3 cover, at r = m % 128 + 384 - 128 d
    float* const y = out + out_offs[c * B + u];
    for (int m = tid; m < NZ_TILE; m += 256) {
      const int i = i_lo + m;
      if (i >= n) break;
      const int h = m >> 7, r = (m & 127) + 3 * HOP;
      const float s = ((frames[h][r] + frames[h + 1][r - HOP]) + frames[h + 2][r - 2 * HOP]) + frames[h + 3][r - 3 * HOP];
      y[i] = s * (2.0f / 3.0f);
    }
  }
}

// ---- sk_add_noise ----------------------------------------------------------------------------------------------------------------
constexpr int AN_THREADS = 1024;
constexpr int AN_WAVES = AN_THREADS / SK_WAVE;

template <bool PCM>
__global__ __launch_bounds__(AN_THREADS) void add_noise_kernel(float* __restrict__ sig, const int64_t* __restrict__ sig_offs,
                                                               const void* __restrict__ noise, const int64_t* __restrict__ noise_offs,
                                                               const int32_t* __restrict__ nsamp, int B, int C,
                                                               const float* __restrict__ amp, int quantize, float* __restrict__ gains) {
  __shared__ double red[2][AN_WAVES];
  const int u = blockIdx.x;
  const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const unsigned n = (unsigned)nsamp[u];
  // pass 1: mean squares of the mixture and the noise on the reference channel, fp64
  {
    const float* const y = sig + sig_offs[u];
    const int64_t o = noise_offs[u];
    const void* const v = PCM ? (const void*)((const int16_t*)noise + o) : (const void*)((const float*)noise + o);
    double sy = 0.0, sv = 0.0;
    for (unsigned i = tid; i < n; i += AN_THREADS) {
      const double a = (double)y[i], b = (double)sk_sample<PCM>(v, i);
      sy += a * a;
      sv += b * b;
    }
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) {
      sy += __shfl_xor(sy, o2, 64);
      sv += __shfl_xor(sv, o2, 64);
    }
    if (lane == 0) {
      red[0][wave] = sy;
      red[1][wave] = sv;
    }
  }
  __syncthreads();   // (also: every thread has read the reference channel before any thread rewrites it)
  double ty = 0.0, tv = 0.0;
#pragma unroll
  for (int w = 0; w < AN_WAVES; ++w) {
    ty += red[0][w];
    tv += red[1][w];
  }
  const double Py = ty / (double)n, Pv = tv / (double)n;
  const float a = (Py >= NZ_SILENT && Pv >= NZ_SILENT) ? (float)((double)amp[u] * sqrt(Py / Pv)) : 0.f;
  if (gains != nullptr && tid == 0) gains[u] = a;
  // pass 2: every channel, in place
  for (int c = 0; c < C; ++c) {
    float* const y = sig + sig_offs[c * B + u];
    const int64_t o = noise_offs[c * B + u];
    const void* const v = PCM ? (const void*)((const int16_t*)noise + o) : (const void*)((const float*)noise + o);
    for (unsigned i = tid; i < n; i += AN_THREADS) {
      const float r = fmaf(a, sk_sample<PCM>(v, i), y[i]);
      y[i] = quantize ? sk_quant16(r) : r;
    }
  }
}

}  // namespace

extern "C" int sk_noise_factors(const double* mics_host, int B, int C, double rate, float* L, sk_stream_t stream) {
  SK_CHECK_ARG(C >= NZ_MINC && C <= NZ_MAXC, "sk_noise_factors: C = %d microphones outside %d..%d", C, NZ_MINC, NZ_MAXC);
  SK_CHECK_ARG(B >= 1 && B <= NZ_MAX_B, "sk_noise_factors: B = %d mixtures outside 1..%d", B, NZ_MAX_B);
  SK_CHECK_ARG(rate >= 1.0 && std::isfinite(rate), "sk_noise_factors: rate = %g below 1", rate);
  SK_CHECK_ARG(mics_host && L, "sk_noise_factors: null pointer");
  for (int u = 0; u < B; ++u)
    for (int i = 0; i < C; ++i)
      for (int j = 0; j < i; ++j) {
        double d2 = 0.0;
        for (int q = 0; q < 3; ++q) {
          const double t = mics_host[((int64_t)u * C + i) * 3 + q] - mics_host[((int64_t)u * C + j) * 3 + q];
          d2 += t * t;
        }
        SK_CHECK_ARG(std::sqrt(d2) >= NZ_MIN_DIST * (1.0 - 1e-9),   // (a 1 cm grid is 1 cm apart, whatever its roundings)
                     "sk_noise_factors: microphones %d and %d of mixture %d are less than %g m apart (or not finite)",
                     j, i, u, NZ_MIN_DIST);
      }
  const hipStream_t st = (hipStream_t)stream;
  const int64_t tri = (int64_t)C * (C + 1) / 2;
  for (int u0 = 0; u0 < B; u0 += NZ_FCHUNK) {
    const int nb = std::min(NZ_FCHUNK, B - u0);
    NzMics mics = {};
    for (int u = 0; u < nb; ++u)
      for (int i = 0; i < C; ++i)
        for (int q = 0; q < 3; ++q) mics.m[u][i][q] = mics_host[((int64_t)(u0 + u) * C + i) * 3 + q];
    float* const Lc = L + (int64_t)u0 * NBIN * tri;
    const dim3 grid((unsigned)sk_cdiv((int64_t)nb * NBIN, 256));
    sk_dispatch_int<NZ_MINC, NZ_MAXC>(C, [&](auto c) {
      hipLaunchKernelGGL((noise_factors_kernel<decltype(c)::value>), grid, dim3(256), 0, st, mics, nb, rate, Lc);
      return 0;
    });
    SK_CHECK_LAUNCH("noise_factors_kernel");
  }
  return SK_OK;
}

extern "C" int sk_diffuse_noise(const void* in, int pcm16, const int64_t* in_offs, const int32_t* nsamp, int B, int C, int max_nsamp,
                                const float* L, float* out, const int64_t* out_offs, sk_stream_t stream) {
  SK_CHECK_ARG(C >= NZ_MINC && C <= NZ_MAXC, "sk_diffuse_noise: C = %d channels outside %d..%d", C, NZ_MINC, NZ_MAXC);
  SK_CHECK_ARG(B >= 1 && B <= NZ_MAX_B, "sk_diffuse_noise: B = %d mixtures outside 1..%d", B, NZ_MAX_B);
  SK_CHECK_ARG(max_nsamp >= 1 && max_nsamp <= NZ_MAX_SAMPLES, "sk_diffuse_noise: max_nsamp = %d outside 1..2^30", max_nsamp);
  SK_CHECK_ARG(in && in_offs && nsamp && L && out && out_offs, "sk_diffuse_noise: null pointer");
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)sk_cdiv(max_nsamp, NZ_TILE), (unsigned)B);
  const bool p = pcm16 != 0;
  sk_dispatch_int<NZ_MINC, NZ_MAXC>(C, [&](auto c) {
    constexpr int CC = decltype(c)::value;
    if (p)
      hipLaunchKernelGGL((diffuse_noise_kernel<CC, true>), grid, dim3(256), 0, st, in, in_offs, nsamp, B, max_nsamp, L, out, out_offs);
    else
      hipLaunchKernelGGL((diffuse_noise_kernel<CC, false>), grid, dim3(256), 0, st, in, in_offs, nsamp, B, max_nsamp, L, out, out_offs);
    return 0;
  });
  SK_CHECK_LAUNCH("diffuse_noise_kernel");
  return SK_OK;
}

extern "C" int sk_add_noise(float* sig, const int64_t* sig_offs, const void* noise, int noise_pcm16, const int64_t* noise_offs,
                            const int32_t* nsamp, int B, int C, const float* amp, int quantize, float* gains_out, sk_stream_t stream) {
  SK_CHECK_ARG(C >= 1 && C <= NZ_MAXC, "sk_add_noise: C = %d channels outside 1..%d", C, NZ_MAXC);
  SK_CHECK_ARG(B >= 1 && B <= NZ_MAX_B, "sk_add_noise: B = %d mixtures outside 1..%d", B, NZ_MAX_B);
  SK_CHECK_ARG(sig && sig_offs && noise && noise_offs && nsamp && amp, "sk_add_noise: null pointer");
  const hipStream_t st = (hipStream_t)stream;
  const int qz = quantize != 0;
  if (noise_pcm16)
    hipLaunchKernelGGL(add_noise_kernel<true>, dim3((unsigned)B), dim3(AN_THREADS), 0, st, sig, sig_offs, noise, noise_offs, nsamp, B, C,
                       amp, qz, gains_out);
  else
    hipLaunchKernelGGL(add_noise_kernel<false>, dim3((unsigned)B), dim3(AN_THREADS), 0, st, sig, sig_offs, noise, noise_offs, nsamp, B, C,
                       amp, qz, gains_out);
  SK_CHECK_LAUNCH("add_noise_kernel");
  return SK_OK;
}
