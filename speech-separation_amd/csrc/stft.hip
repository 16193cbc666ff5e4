// stft.hip -- framed STFT / mask-apply + iSTFT for n_fft = 512, gfx950.
//
// The 256-point FFT by sixteen lanes, its constants and its tables are fft512.h's (which describes the plan); a wavefront
// transforms 4 frames at once and a workgroup (4 waves) 16 consecutive frames of one utterance.
// Both kernels are streaming kernels (HBM roofline):
//   STFT   reads 128 new samples and writes 257 bins per frame,
//   iSTFT  reads 257 complex bins (+257 mask values) and writes 128 samples per frame per source.
// The SI-SDR training loss (sisdr.hip) adds two kernels that share this FFT: istft_rows_kernel, the iSTFT reading the training
// engine's packed rows, and sisdr_grad_kernel, its adjoint fused with the SI-SDR gradient -- the STFT kernel with another
// sample loader and another epilogue (2 x 128 samples + 257 complex bins in, 257 gradients out per frame and source).
// The mixture-invariant loss (mixit.hip) adds mixit_grad_kernel, the same adjoint with one transform per (utterance, reference)
// whose result goes to the column block of every estimate assigned to that reference.  Both are grad_tiles, the one tile
// loop of the adjoint, called with the loss's own sample formula and store.
// The phase-sensitive loss adds stft_psa_kernel, the STFT kernel over the S + 1 signals of an utterance.  STOI scoring, which
// shares the FFT alone, is stoi.hip.
//
// Shape coverage: tests/test_gpu_stft_family.py runs stft_kernel, istft_kernel, istft_rows_kernel and stft_psa_kernel at the
// lengths their tile loops branch on, against fp64 (grad_tiles: EDGE_LENGTHS in tests/test_gpu_sisdr.py).
//
// Reference semantics restated: librosa.core.stft / istft as used at
// steps/extract_feats.py:85-89,104-105 and steps/reconstruct_sources.py:39-42 (see oracle/stft.py).
#include "fft512.h"
#include "wave_loss.h"

namespace {

// BINMAJOR == false: every utterance of the launch is written frame-major (stride_f == 1): lanes store their
// bins straight from registers.  BINMAJOR == true: arbitrary strides (the reference's on-disk (257, T)
// layout): results are staged in LDS and written with consecutive threads on consecutive frames.
template <bool BINMAJOR, bool CPLX>
__global__ __launch_bounds__(256, BINMAJOR ? 2 : 4) void stft_kernel(const void* __restrict__ wav, int pcm16,
                                                   const int64_t* __restrict__ wav_offs,
                                                   const int32_t* __restrict__ nsamp,
                                                   void* __restrict__ out, const int64_t* __restrict__ out_offs,
                                                   const int64_t* __restrict__ stride_t,
                                                   const int64_t* __restrict__ stride_f) {
  __shared__ __attribute__((aligned(16))) float smp[NFFT + (FPB - 1) * HOP];
  __shared__ __attribute__((aligned(16))) float win[NFFT];
  __shared__ float2 tw[NFFT];
  __shared__ float2 t256[256];
  __shared__ float xch[16][16 * XLD];  // one transpose plane per 16-lane group
  __shared__ float2 ost[BINMAJOR ? FPB : 1][BINMAJOR ? NBIN : 1];

  const int u = blockIdx.y;
  const int N = nsamp[u];
  const int T = 1 + N / HOP;
  const int tile0 = blockIdx.x * TPB;  // this block transforms tiles tile0 .. tile0+TPB-1 (FPB frames each)
  if (tile0 * FPB >= T) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t woff = wav_offs[u];
  const int64_t ooff = out_offs[u];
  const int64_t st = stride_t[u], sf = stride_f[u];
  constexpr int SPAN = NFFT + (FPB - 1) * HOP, SPT = (SPAN + 255) / 256;  // samples per tile / per thread

  // reflect-padded samples [t0*HOP, t0*HOP + SPAN) of the padded signal (zeros past the last frame of the
  // utterance).  Tiles whose whole span lies inside the utterance (all but the first and the last one or two)
  // take a block-uniform path without the reflect/clamp arithmetic.
  auto fetch = [&](int t0, float (&r)[SPT]) {
    const int nfr = min(FPB, T - t0);
    const int span = NFFT + (nfr - 1) * HOP;
    const int first = t0 * HOP - NFFT / 2;
    if (first >= 0 && first + SPAN <= N) {
      if (pcm16) {
        const int16_t* w = (const int16_t*)wav + woff + first;
#pragma unroll
        for (int q = 0; q < SPT; ++q) {
          const int i = tid + 256 * q;
          r[q] = (i < SPAN) ? (float)w[i] * (1.0f / 32768.0f) : 0.f;
        }
      } else {
        const float* w = (const float*)wav + woff + first;
#pragma unroll
        for (int q = 0; q < SPT; ++q) {
          const int i = tid + 256 * q;
          r[q] = (i < SPAN) ? w[i] : 0.f;
        }
      }
      return;
    }
#pragma unroll
    for (int q = 0; q < SPT; ++q) {
      const int i = tid + 256 * q;
      int src = first + i;
      if (src < 0) src = -src;
      if (src >= N) src = 2 * (N - 1) - src;
      src = max(0, min(src, N - 1));
      float v = pcm16 ? (float)((const int16_t*)wav)[woff + src] * (1.0f / 32768.0f) : ((const float*)wav)[woff + src];
      r[q] = (i < span) ? v : 0.f;
    }
  };
  auto stash = [&](const float (&r)[SPT]) {
#pragma unroll
    for (int q = 0; q < SPT; ++q) {
      const int i = tid + 256 * q;
      if (i < SPAN) smp[i] = r[q];
    }
  };

  for (int i = tid; i < NFFT; i += 256) {
    tw[i] = g_tw512[i];
    win[i] = g_hann512[i];
  }
  t256[tid] = g_tw512[(2 * (tid & 15) * (tid >> 4)) & 511];
  float pre[SPT];
  fetch(tile0 * FPB, pre);
  stash(pre);
  __syncthreads();

  const int j = lane & 15, g = lane >> 4;
  const int fr = 4 * wave + g;  // this group's frame within a tile
  const int partner = (lane & 48) | ((16 - j) & 15);
  for (int ti = 0; ti < TPB; ++ti) {
    const int t0 = (tile0 + ti) * FPB;
    if (t0 >= T) break;  // block-uniform
    const int nfr = min(FPB, T - t0);
    const bool more = ti + 1 < TPB && t0 + FPB < T;
    if (more) fetch(t0 + FPB, pre);  // next tile's samples travel while this tile is transformed
    const bool active = fr < nfr;
    v2f z[16];
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) {  // packed point n = 16 n1 + j  <->  samples 2n, 2n+1
      const v2f sm = *reinterpret_cast<const v2f*>(&smp[fr * HOP + 32 * n1 + 2 * j]);
      const v2f w = *reinterpret_cast<const v2f*>(&win[32 * n1 + 2 * j]);
      z[n1] = sm * w;
    }
    fft256_g16(z, xch[4 * wave + g], t256, j);

    // real-FFT split: X[k] = Xe + W^k Xo, Xe = (Z[k] + conj Z[256-k])/2, Xo = -i (Z[k] - conj Z[256-k])/2, k = j + 16 k2.
    // Z[256-k] is register 15-k2 of lane (16-j)%16 of this group (register (16-k2)%16 of lane 0 itself when j == 0).
    // r03: the bins k and 256-k of a pair are formed by ONE lane from shared terms -- Xe[256-k] = conj Xe[k],
    // Xo[256-k] = conj Xo[k], W^(256-k) = -conj W^k, so with A = Xe[k], Bt = W^k Xo[k]:  X[k] = A + Bt,  X[256-k] = conj(A - Bt).
    // Lane j takes k2 = 0..7 (its partner's k2 = 8..15 are the mirrors of lane 16-j's 0..7): 16 shuffles, 8 twiddles and 8
    // complex products per lane instead of 32 / 16 / 16; lane 0 adds the self-paired bin 128 (k2 = 0 gives bins 0 and 256).
    // frame-major output row of this group's frame: lane j writes bins j + 16 k2 and 256 - j - 16 k2 at constant offsets
    constexpr int CW = CPLX ? 2 : 1;
    float* const orow = (float*)out + CW * (ooff + (int64_t)(t0 + fr) * st) + CW * j;
    float* const orow2 = (float*)out + CW * (ooff + (int64_t)(t0 + fr) * st) + CW * (256 - j);
    auto emit = [&](v2f x, int k, float* dstp) {
      if (BINMAJOR)
        st2(&ost[fr][k], x);
      else if (CPLX)
        *reinterpret_cast<v2f*>(dstp) = x;
      else
        *dstp = __builtin_amdgcn_sqrtf(x.x * x.x + x.y * x.y);
    };
    if (active) {  // uniform over the 16-lane group, which is all the shuffles below reach
#pragma unroll
      for (int k2 = 0; k2 < 8; ++k2) {
        v2f zc;
        zc.x = __shfl(z[15 - k2].x, partner, 64);
        zc.y = __shfl(z[15 - k2].y, partner, 64);
        if (j == 0) zc = z[(16 - k2) & 15];
        const v2f zk = z[k2], cz = conj(zc);
        const int k = j + 16 * k2;
        const v2f A = 0.5f * (zk + cz), Bt = cmul(ld2(&tw[k]), 0.5f * mul_mi(zk - cz));
        emit(A + Bt, k, orow + CW * 16 * k2);
        emit(conj(A - Bt), 256 - k, orow2 - CW * 16 * k2);
      }
      if (j == 0) {  // bin 128 pairs with itself
        const v2f zk = z[8], cz = conj(zk);
        emit(0.5f * (zk + cz) + cmul(ld2(&tw[128]), 0.5f * mul_mi(zk - cz)), 128, orow + CW * 128);
      }
    }
    __syncthreads();  // every wave is done with smp (and ost is complete)
    if (BINMAJOR) {
      const int total = nfr * NBIN;
      for (int i = tid; i < total; i += 256) {
        int f2, k;
        if (st == 1) {  // bin-major (F,T): consecutive threads -> consecutive frames
          k = i / nfr;
          f2 = i - k * nfr;
        } else {  // frame-major: consecutive threads -> consecutive bins
          f2 = i / NBIN;
          k = i - f2 * NBIN;
        }
        const float2 x = ost[f2][k];
        const int64_t o = ooff + (int64_t)(t0 + f2) * st + (int64_t)k * sf;
        if (CPLX)
          ((float2*)out)[o] = x;
        else
          ((float*)out)[o] = __builtin_amdgcn_sqrtf(x.x * x.x + x.y * x.y);
      }
    }
    if (more) {
      stash(pre);
      __syncthreads();
    }
  }
}

constexpr int RING = FPB + 3;  // row slots of the iSTFT ring: one tile of frames + the 3 frames before it
// float2 per slot: a 257-bin spectrum, then the FFT's 16 x 17 float transpose plane, then 512 samples.  272 (r03; was 258):
// consecutive slots lie 544 dwords = 32 banks (mod 64) apart, so the two frames a 32-lane group of ds_read_b64 covers fall
// on opposite halves of the bank row; and bin k of frame t sits at index k ^ ((t + 3) & 15) -- a permutation inside each
// aligned group of 16 bins -- so that the 16 FRAMES x one bin a 16-lane group of the tile load writes (rows now a multiple
// of 32 banks apart) land on 16 different bank pairs.  Both were 2-way conflicts (35 % of the kernel's LDS cycles, r02 PMC).
constexpr int RLD = 272;

// Masked spectra of frames [tfirst, tfirst + COUNT) into their ring slots (zeros outside [0, T)).
template <int COUNT>
__device__ __forceinline__ void istft_load(float2 (*rows)[RLD], int tfirst, int T, const float2* __restrict__ mix,
                                           int64_t mo, int64_t mst, int64_t msf, const float* __restrict__ mask,
                                           int64_t ko, int64_t kst, int64_t ksf) {
  for (int i = threadIdx.x; i < COUNT * NBIN; i += 256) {
    int fr, k;
    if (mst == 1) {  // bin-major (257, T): consecutive threads -> consecutive frames
      k = i / COUNT;
      fr = i - k * COUNT;
    } else {
      fr = i / NBIN;
      k = i - fr * NBIN;
    }
    const int t = tfirst + fr;
    float2 x = make_float2(0.f, 0.f);
    if (t >= 0 && t < T) {
      x = mix[mo + (int64_t)t * mst + (int64_t)k * msf];
      if (mask) {
        const float m = mask[ko + (int64_t)t * kst + (int64_t)k * ksf];
        x.x *= m;
        x.y *= m;
      }
    }
    rows[(t + 3) % RING][k ^ ((t + 3) & 15)] = x;
  }
}

// Inverse real FFT of frame t by one 16-lane group; the windowed 512 samples replace the spectrum in the slot.
// key = (t + 3) & 15: the slot's bin permutation (RLD).
__device__ __forceinline__ void istft_frame(float2* row, const float2* tw, const float2* t256, const float* win, int j, int key) {
  v2f z[16];
#pragma unroll
  for (int n1 = 0; n1 < 16; ++n1) {
    const int k = 16 * n1 + j;
    v2f a = ld2(&row[k ^ key]);
    v2f b = ld2(&row[(256 - k) ^ key]);
    if (k == 0) {  // irfft ignores Im X[0] and Im X[256]
      a.y = 0.f;
      b.y = 0.f;
    }
    b = conj(b);  // conj(X[256-k])
    const v2f xe = 0.5f * (a + b), hd = 0.5f * (a - b);
    const v2f xo = cmul(hd, conj(ld2(&tw[k])));  // * conj(W^k)
    // Z = Xe + i Xo ; feed conj(Z) to the forward FFT
    z[n1] = (v2f){xe.x - xo.y, -(xe.y + xo.x)};
  }
  wave_sync();  // the spectrum is in registers: the slot now serves as the transpose area, then as the output
  // transpose plane: the odd one of the two groups that share a 32-lane half sits 16 banks further (slots are a multiple
  // of 32 banks apart), so the two groups' column writes / row reads never meet on a bank
  fft256_g16(z, reinterpret_cast<float*>(row) + 16 * ((threadIdx.x >> 4) & 1), t256, j);
  float* tf = reinterpret_cast<float*>(row);
#pragma unroll
  for (int k2 = 0; k2 < 16; ++k2) {  // z[k2] = Y[n], n = j + 16 k2; x[2n] = Re Y / 256, x[2n+1] = -Im Y / 256
    const int n = j + 16 * k2;
    const v2f w = *reinterpret_cast<const v2f*>(&win[2 * n]);
    *reinterpret_cast<v2f*>(&tf[2 * n]) = w * (z[k2] * (v2f){1.0f / 256.0f, -1.0f / 256.0f});
  }
}

// Bin-major fast path of the tile load (the reference's (257, T) layout: stride_t == 1 for spectrum and mask): thread
// (fr = tid & 15, k0 = tid >> 4) owns frame t0 + fr and bins k0, k0 + 16, ... -- 17 loads at a constant pointer
// stride, no per-element index arithmetic.  fetch() only issues the global loads (into registers: they travel while
// the current tile is transformed and overlap-added), stash() applies the mask and fills the ring slot.
struct TileRegs {
  float2 x[17];
  float m[17];
};

__device__ __forceinline__ void istft_fetch(TileRegs& r, int t0, int T, const float2* __restrict__ mix, int64_t mo, int64_t msf,
                                            const float* __restrict__ mask, int64_t ko, int64_t ksf) {
  const int fr = threadIdx.x & 15, k0 = threadIdx.x >> 4;
  const int t = t0 + fr;
  const bool ok = t >= 0 && t < T;
  const float2* pm = mix + mo + (ok ? t : 0) + (int64_t)k0 * msf;
  const float* pk = mask ? mask + ko + (ok ? t : 0) + (int64_t)k0 * ksf : nullptr;
#pragma unroll
  for (int q = 0; q < 17; ++q) {
    const bool live = ok && (q < 16 || k0 == 0);  // bin 256 = k0 0, q 16
    r.x[q] = live ? pm[(int64_t)q * 16 * msf] : make_float2(0.f, 0.f);
    r.m[q] = (live && pk) ? pk[(int64_t)q * 16 * ksf] : 1.f;
  }
}

__device__ __forceinline__ void istft_stash(const TileRegs& r, float2 (*rows)[RLD], int t0) {
  const int fr = threadIdx.x & 15, k0 = threadIdx.x >> 4;
  float2* row = rows[(t0 + fr + 3) % RING] + (k0 ^ ((t0 + fr + 3) & 15));
#pragma unroll
  for (int q = 0; q < 17; ++q)
    if (q < 16 || k0 == 0) row[16 * q] = make_float2(r.x[q].x * r.m[q], r.x[q].y * r.m[q]);
}

// Output samples of the 16 hops of tile t0 from the windowed frames in the ring: thread (m0 = tid & 127, hsel = tid >> 7)
// produces sample m0 of hops t0 + hsel + 2q, q = 0..7.  With all four taps inside [0, T) the window-sum-square is a
// constant of the thread (inv_full = its reciprocal).
__device__ __forceinline__ void istft_overlap_add(float2 (*rows)[RLD], const float* win, int t0, int T, int nout, int m0, int hsel,
                                                  float inv_full, float* __restrict__ wav_out, int16_t* __restrict__ pcm_out,
                                                  int64_t oo) {
  // overlap-add in increasing frame order, window-sum-square normalisation, trim, convert
  int slot = (t0 + hsel) % RING;  // ring slot of frame hp - 3 (frame t lives in slot (t + 3) % RING)
#pragma unroll
  for (int q = 0; q < FPB * HOP / 256; ++q) {
    const int hp = t0 + hsel + 2 * q;
    const int n = hp * HOP + m0 - NFFT / 2;
    const int s3 = slot, s2 = slot + 1 >= RING ? slot + 1 - RING : slot + 1, s1 = slot + 2 >= RING ? slot + 2 - RING : slot + 2,
              s0 = slot + 3 >= RING ? slot + 3 - RING : slot + 3;
    slot = slot + 2 >= RING ? slot + 2 - RING : slot + 2;
    if (n < 0 || n >= nout) continue;
    float acc;
    if (hp >= 3 && hp < T) {  // all four frames exist
      acc = reinterpret_cast<const float*>(rows[s3])[3 * HOP + m0];
      acc += reinterpret_cast<const float*>(rows[s2])[2 * HOP + m0];
      acc += reinterpret_cast<const float*>(rows[s1])[HOP + m0];
      acc += reinterpret_cast<const float*>(rows[s0])[m0];
      acc *= inv_full;
    } else {
      acc = 0.f;
      float wss = 0.f;
      const int sl[4] = {s0, s1, s2, s3};
#pragma unroll
      for (int qq = 3; qq >= 0; --qq) {
        const int t = hp - qq;
        if (t >= 0 && t < T) {
          const int m = qq * HOP + m0;
          acc += reinterpret_cast<const float*>(rows[sl[qq]])[m];
          const float w = win[m];
          wss += w * w;
        }
      }
      if (wss > 1.17549435e-38f) acc /= wss;
    }
    if (wav_out) wav_out[oo + n] = acc;
    if (pcm_out) {
      const float sv = acc * 32767.0f;
      pcm_out[oo + n] = (int16_t)(long long)sv;  // truncation toward zero, wrap on overflow
    }
  }
}

// One workgroup reconstructs `tpb` consecutive 16-hop tiles of one (utterance, source): every frame is read
// and transformed once; the 3 frames that overlap into the next tile stay in the LDS ring.
__global__ __launch_bounds__(256, 3) void istft_kernel(
    const float2* __restrict__ mix, const int64_t* __restrict__ mix_offs, const int64_t* __restrict__ mix_st,
    const int64_t* __restrict__ mix_sf, const float* __restrict__ mask, const int64_t* __restrict__ mask_offs,
    const int64_t* __restrict__ mask_st, const int64_t* __restrict__ mask_sf, const int32_t* __restrict__ nframes,
    int S, float* __restrict__ wav_out, int16_t* __restrict__ pcm_out, const int64_t* __restrict__ out_offs, int tpb) {
  // 48.4 KB: three workgroups per CU.  (Reading the 6 KB of tables through the vector L1 instead would fit four, but
  // the 64-bit gather addresses push the kernel over 128 VGPRs into scratch: measured 2.7 -> 4.9 ms.)
  __shared__ __attribute__((aligned(16))) float2 rows[RING][RLD];
  __shared__ __attribute__((aligned(16))) float win[NFFT];
  __shared__ float2 tw[NFFT];
  __shared__ float2 t256[256];

  const int us = blockIdx.y;
  const int u = us / S;
  const int T = nframes[u];
  const int nout = HOP * (T - 1);
  const int ntiles = T / FPB + 1;  // hops 0 .. T carry output samples
  const int tile0 = blockIdx.x * tpb;
  if (tile0 >= ntiles) return;
  const int tile1 = min(ntiles, tile0 + tpb);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, fr = 4 * __builtin_amdgcn_readfirstlane(wave) + (lane >> 4);
  const int64_t mo = mix_offs[u], mst = mix_st[u], msf = mix_sf[u];
  const int64_t ko = mask ? mask_offs[us] : 0, kst = mask ? mask_st[u] : 0, ksf = mask ? mask_sf[u] : 0;
  const int64_t oo = out_offs[us];
  const bool binmajor = mst == 1 && (!mask || kst == 1);  // block-uniform

  TileRegs pre;
  if (binmajor) istft_fetch(pre, tile0 * FPB, T, mix, mo, msf, mask, ko, ksf);
  for (int i = tid; i < NFFT; i += 256) {
    tw[i] = g_tw512[i];
    win[i] = g_hann512[i];
  }
  t256[tid] = g_tw512[(2 * (tid & 15) * (tid >> 4)) & 511];
  if (tile0 > 0) {  // the 3 frames before this block's first tile
    const int tf = tile0 * FPB - 3;
    istft_load<3>(rows, tf, T, mix, mo, mst, msf, mask, ko, kst, ksf);
    __syncthreads();
    if (fr < 3) istft_frame(rows[(tf + fr + 3) % RING], tw, t256, win, j, (tf + fr + 3) & 15);
  }
  // overlap-add roles: thread (m0 = tid & 127, hsel = tid >> 7) produces sample m0 of hops t0 + hsel + 2q, q = 0..7.
  // With all four taps inside [0, T) the window-sum-square is a constant of the thread.
  const int m0 = tid & (HOP - 1), hsel = __builtin_amdgcn_readfirstlane(tid >> 7);  // wave-uniform: the slot arithmetic stays scalar
  float wss_full = 0.f;
  __syncthreads();  // win is complete
#pragma unroll
  for (int q = 3; q >= 0; --q) {
    const float w = win[q * HOP + m0];
    wss_full += w * w;
  }
  const float inv_full = 1.0f / wss_full;

  for (int tile = tile0; tile < tile1; ++tile) {
    const int t0 = tile * FPB;
    __syncthreads();  // the previous tile's overlap-add is done with the slots about to be refilled
    if (binmajor)
      istft_stash(pre, rows, t0);
    else
      istft_load<FPB>(rows, t0, T, mix, mo, mst, msf, mask, ko, kst, ksf);
    __syncthreads();
    if (binmajor && tile + 1 < tile1) istft_fetch(pre, t0 + FPB, T, mix, mo, msf, mask, ko, ksf);  // travels under the FFTs
    istft_frame(rows[(t0 + fr + 3) % RING], tw, t256, win, j, (t0 + fr + 3) & 15);
    __syncthreads();
    istft_overlap_add(rows, win, t0, T, nout, m0, hsel, inv_full, wav_out, pcm_out, oo);
  }
}

// ---- packed rows (the training engine's layout): row of (t, j) = offs[t] + j, mixture (R, 257) complex64, mask (R, ld)
// with source s in columns s * 257 ...  A tile is read frame-major: thread tid owns bin tid of each of the 16 frames (one
// coalesced row sweep per frame, the row's base a scalar), threads 0..15 also bin 256 of frame tid.  fetch() only issues
// the loads, stash() applies the mask and fills the ring slots (RLD: the bin permutation keeps a frame's 256 stores conflict-free).
struct RowRegs {
  float2 x[17];
  float m[17];
};

__device__ __forceinline__ void istft_rows_fetch(RowRegs& r, int t0, int T, const float2* __restrict__ mix,
                                                 const float* __restrict__ mask, int ld, int col0,
                                                 const int32_t* __restrict__ offs, int u) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < 17; ++q) {
    const int t = q < FPB ? t0 + q : t0 + tid, k = q < FPB ? tid : 256;
    const bool live = t < T && (q < FPB || tid < FPB);
    const int64_t row = live ? (int64_t)offs[t] + u : 0;
    r.x[q] = live ? mix[row * NBIN + k] : make_float2(0.f, 0.f);
    r.m[q] = live ? mask[row * ld + col0 + k] : 0.f;
  }
}

__device__ __forceinline__ void istft_rows_stash(const RowRegs& r, float2 (*rows)[RLD], int t0) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < 17; ++q) {
    const int t = q < FPB ? t0 + q : t0 + tid, k = q < FPB ? tid : 256;
    if (q < FPB || tid < FPB) rows[(t + 3) % RING][k ^ ((t + 3) & 15)] = make_float2(r.x[q].x * r.m[q], r.x[q].y * r.m[q]);
  }
}

// istft_kernel on packed rows: blockIdx.y = j * S + s, float32 samples out.
__global__ __launch_bounds__(256, 3) void istft_rows_kernel(const float2* __restrict__ mix, const float* __restrict__ mask, int ld,
                                                            const int32_t* __restrict__ offs, const int32_t* __restrict__ nframes,
                                                            int S, float* __restrict__ wav_out,
                                                            const int64_t* __restrict__ out_offs, int tpb) {
  __shared__ __attribute__((aligned(16))) float2 rows[RING][RLD];
  __shared__ __attribute__((aligned(16))) float win[NFFT];
  __shared__ float2 tw[NFFT];
  __shared__ float2 t256[256];

  const int us = blockIdx.y;
  const int u = us / S, col0 = (us - u * S) * NBIN;
  const int T = nframes[u];
  const int nout = HOP * (T - 1);
  const int ntiles = T / FPB + 1;  // hops 0 .. T carry output samples
  const int tile0 = blockIdx.x * tpb;
  if (tile0 >= ntiles) return;
  const int tile1 = min(ntiles, tile0 + tpb);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, fr = 4 * __builtin_amdgcn_readfirstlane(wave) + (lane >> 4);
  const int64_t oo = out_offs[us];

  RowRegs pre;
  istft_rows_fetch(pre, tile0 * FPB, T, mix, mask, ld, col0, offs, u);
  for (int i = tid; i < NFFT; i += 256) {
    tw[i] = g_tw512[i];
    win[i] = g_hann512[i];
  }
  t256[tid] = g_tw512[(2 * (tid & 15) * (tid >> 4)) & 511];
  if (tile0 > 0) {  // the 3 frames before this block's first tile (all of them exist: tile0 * FPB - 3 >= 13, < T)
    const int tf = tile0 * FPB - 3;
    for (int i = tid; i < 3 * NBIN; i += 256) {
      const int f3 = i / NBIN, k = i - f3 * NBIN, t = tf + f3;
      float2 x = make_float2(0.f, 0.f);
      if (t < T) {
        const int64_t row = (int64_t)offs[t] + u;
        const float m = mask[row * ld + col0 + k];
        x = mix[row * NBIN + k];
        x.x *= m;
        x.y *= m;
      }
      rows[(t + 3) % RING][k ^ ((t + 3) & 15)] = x;
    }
    __syncthreads();
    if (fr < 3) istft_frame(rows[(tf + fr + 3) % RING], tw, t256, win, j, (tf + fr + 3) & 15);
  }
  const int m0 = tid & (HOP - 1), hsel = __builtin_amdgcn_readfirstlane(tid >> 7);
  float wss_full = 0.f;
  __syncthreads();  // win is complete
#pragma unroll
  for (int q = 3; q >= 0; --q) {
    const float w = win[q * HOP + m0];
    wss_full += w * w;
  }
  const float inv_full = 1.0f / wss_full;

  for (int tile = tile0; tile < tile1; ++tile) {
    const int t0 = tile * FPB;
    __syncthreads();  // the previous tile's overlap-add is done with the slots about to be refilled
    istft_rows_stash(pre, rows, t0);
    __syncthreads();
    if (tile + 1 < tile1) istft_rows_fetch(pre, t0 + FPB, T, mix, mask, ld, col0, offs, u);  // travels under the FFTs
    istft_frame(rows[(t0 + fr + 3) % RING], tw, t256, win, j, (t0 + fr + 3) & 15);
    __syncthreads();
    istft_overlap_add(rows, win, t0, T, nout, m0, hsel, inv_full, wav_out, nullptr, oo);
  }
}

// ---- adjoint of mask-apply + iSTFT, fused with a waveform loss's gradient: the tile loop of sisdr_grad_kernel and
// mixit_grad_kernel.  stft_kernel<frame-major> with another sample loader and another epilogue: the "signal" of utterance u is
//   g[p] = sample(n) / wss[p],  n = p - 256 in [0, L_u), 0 elsewhere   (sample: the loss's gradient at n, gscale included),
// framed WITHOUT reflection (frame t = g[tH .. tH + 512)); each bin U[t][f] of its windowed transform is contracted with the
// mixture's bin on the way out: put(at, (c_f / 512) (Re X Re U + Im X Im U)), c_f = 1 at f = 0, 256, else 2, where `at` is
// column f of dmask's row offs[t] + u; put adds the column block(s) of the estimate(s) the signal belongs to.
// A block transforms tiles tile0 .. tile0 + TPB - 1 (tile0 * FPB < T is the caller's check); all 256 threads arrive together.
template <class Sample, class Put>
__device__ __forceinline__ void grad_tiles(int u, int T, int tile0, const float2* __restrict__ mix, const int32_t* __restrict__ offs,
                                           float* __restrict__ dmask, int ld, Sample sample, Put put) {
  __shared__ __attribute__((aligned(16))) float smp[NFFT + (FPB - 1) * HOP];
  __shared__ __attribute__((aligned(16))) float win[NFFT];
  __shared__ float2 tw[NFFT];
  __shared__ float2 t256[256];
  __shared__ float xch[16][16 * XLD];

  const int L = HOP * (T - 1);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int SPAN = NFFT + (FPB - 1) * HOP, SPT = (SPAN + 255) / 256;

  // Every sample a thread loads has the same position m0 inside its hop (tiles start on hop boundaries, 256 = 2 hops).
  // The window-sum-square of a hop that four frames cover is ((w3^2 + w2^2) + w1^2) + w0^2 with w2^2 rounded and the three
  // other squares fused into their adds -- the contraction the compiler chose for this sum from the start (it may as well fuse
  // w2^2 and round w3^2: another last bit in every sample), written out here; edge hops add the rounded squares.  Nothing
  // in the loader is left to the file's contraction setting.
  const int m0 = tid & (HOP - 1);
  float wsq[4], inv_full;
  {
#pragma clang fp contract(off)
    float w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      w[q] = g_hann512[q * HOP + m0];
      wsq[q] = w[q] * w[q];
    }
    inv_full = 1.0f / __builtin_fmaf(w[0], w[0], __builtin_fmaf(w[1], w[1], __builtin_fmaf(w[3], w[3], wsq[2])));
  }

  auto fetch = [&](int t0, float (&r)[SPT]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int q = 0; q < SPT; ++q) {
      const int i = tid + 256 * q;
      const int p = t0 * HOP + i, n = p - NFFT / 2;
      float v = 0.f;
      if (i < SPAN && n >= 0 && n < L) {
        const float sv = sample(n);
        const int hp = p >> 7;  // frames hp - 3 .. hp cover p
        float inv = inv_full;
        if (hp < 3 || hp >= T) {
          float wss = 0.f;
#pragma unroll
          for (int qq = 3; qq >= 0; --qq)
            if (hp - qq >= 0 && hp - qq < T) wss += wsq[qq];
          inv = wss > 1.17549435e-38f ? 1.0f / wss : 1.0f;
        }
        v = sv * inv;
      }
      r[q] = v;
    }
  };
  auto stash = [&](const float (&r)[SPT]) {
#pragma unroll
    for (int q = 0; q < SPT; ++q) {
      const int i = tid + 256 * q;
      if (i < SPAN) smp[i] = r[q];
    }
  };

  for (int i = tid; i < NFFT; i += 256) {
    tw[i] = g_tw512[i];
    win[i] = g_hann512[i];
  }
  t256[tid] = g_tw512[(2 * (tid & 15) * (tid >> 4)) & 511];
  float pre[SPT];
  fetch(tile0 * FPB, pre);
  stash(pre);
  __syncthreads();

  const int j = lane & 15, g = lane >> 4;
  const int fr = 4 * wave + g;
  const int partner = (lane & 48) | ((16 - j) & 15);
  for (int ti = 0; ti < TPB; ++ti) {
    const int t0 = (tile0 + ti) * FPB;
    if (t0 >= T) break;  // block-uniform
    const int nfr = min(FPB, T - t0);
    const bool more = ti + 1 < TPB && t0 + FPB < T;
    if (more) fetch(t0 + FPB, pre);
    const bool active = fr < nfr;
    v2f z[16];
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) {
      const v2f sm = *reinterpret_cast<const v2f*>(&smp[fr * HOP + 32 * n1 + 2 * j]);
      const v2f w = *reinterpret_cast<const v2f*>(&win[32 * n1 + 2 * j]);
      z[n1] = sm * w;
    }
    fft256_g16(z, xch[4 * wave + g], t256, j);

    // real-FFT split as in stft_kernel; every bin is contracted with the mixture's and stored straight from registers
    const int64_t row = active ? (int64_t)offs[t0 + fr] + u : 0;
    const float2* const xlo = mix + row * NBIN + j;
    const float2* const xhi = mix + row * NBIN + (256 - j);
    float* const dlo = dmask + row * ld + j;
    float* const dhi = dmask + row * ld + (256 - j);
    if (active) {
#pragma unroll
      for (int k2 = 0; k2 < 8; ++k2) {
        v2f zc;
        zc.x = __shfl(z[15 - k2].x, partner, 64);
        zc.y = __shfl(z[15 - k2].y, partner, 64);
        if (j == 0) zc = z[(16 - k2) & 15];
        const v2f zk = z[k2], cz = conj(zc);
        const int k = j + 16 * k2;
        const v2f A = 0.5f * (zk + cz), Bt = cmul(ld2(&tw[k]), 0.5f * mul_mi(zk - cz));
        const v2f ua = A + Bt, ub = conj(A - Bt);  // U[k], U[256 - k]
        const v2f xa = ld2(xlo + 16 * k2), xb = ld2(xhi - 16 * k2);
        const float sa = (k == 0) ? 1.0f / 512.0f : 2.0f / 512.0f;  // bin 256 - k is the Nyquist bin exactly when k == 0
        put(dlo + 16 * k2, sa * (xa.x * ua.x + xa.y * ua.y));
        put(dhi - 16 * k2, sa * (xb.x * ub.x + xb.y * ub.y));
      }
      if (j == 0) {  // bin 128 pairs with itself
        const v2f zk = z[8], cz = conj(zk);
        const v2f ua = 0.5f * (zk + cz) + cmul(ld2(&tw[128]), 0.5f * mul_mi(zk - cz));
        const v2f xa = ld2(xlo + 128);
        put(dlo + 128, (2.0f / 512.0f) * (xa.x * ua.x + xa.y * ua.y));
      }
    }
    __syncthreads();  // every wave is done with smp
    if (more) {
      stash(pre);
      __syncthreads();
    }
  }
}

// SI-SDR (include/sepkern.h, sk_sisdr_mask_grad): blockIdx.y = (utterance j, estimate k); i = the best permutation's source,
//   sample(n) = (A e_k[n] + B r_i[n]) + C   with A, B, C = coef * gscale (B also carries int16 PCM's 2^-15),
// as two rounded products, their sum, plus C: no fused multiply-add, whatever the file's contraction setting.
__global__ __launch_bounds__(256, 4) void sisdr_grad_kernel(const float* __restrict__ est, const int64_t* __restrict__ est_offs,
                                                            const void* __restrict__ ref, int pcm16,
                                                            const int64_t* __restrict__ ref_offs,
                                                            const int32_t* __restrict__ nframes,
                                                            const int32_t* __restrict__ best_perm, const float* __restrict__ coef,
                                                            const float* __restrict__ gscale, const float2* __restrict__ mix,
                                                            const int32_t* __restrict__ offs, int S, float* __restrict__ dmask,
                                                            int ld) {
  const int us = blockIdx.y;
  const int u = us / S, ks = us - u * S;
  const int T = nframes[u];
  const int tile0 = blockIdx.x * TPB;
  if (tile0 * FPB >= T) return;
  int perm[SK_MAXS];
  sk_nth_perm(best_perm[u], S, perm);
  int src = perm[0];
#pragma unroll
  for (int q = 1; q < SK_MAXS; ++q) src = (q < S && ks == q) ? perm[q] : src;
  const float gs = gscale[0];
  const float cA = coef[3 * us] * gs, cB = coef[3 * us + 1] * gs * (pcm16 ? 1.0f / 32768.0f : 1.0f), cC = coef[3 * us + 2] * gs;
  const float* const ep = est + est_offs[us];
  const int64_t roff = ref_offs[u * S + src];
  grad_tiles(
      u, T, tile0, mix, offs, dmask, ld,
      [&](int n) {
#pragma clang fp contract(off)
        const float a = cA * ep[n], b = cB * ref_raw(ref, pcm16, roff, n);
        return (a + b) + cC;
      },
      [&](float* at, float v) { at[ks * NBIN] = v; });
}

// MixIT (include/sepkern.h, sk_mixit_mask_grad): blockIdx.y = j * 2 + n, ONE transform per (utterance j, reference n), whose
// gradient signal and contraction are the same for every estimate of n's group; put stores each bin into every member's
// column block.  With m = the members' estimates added in ascending order, D = coef * gscale and xs = int16 PCM's 2^-15 (or 1),
//   sample(t) = D * fma(-x_n[t], xs, m):   the adds, ONE fused multiply-add, one product.
// The members (bits of best_code[j] equal to n) and their sample streams are wavefront-uniform; an empty group leaves before
// the first barrier.  The groups partition the estimates, so every column < M * 257 of a row is written once, by one lane.
__global__ __launch_bounds__(256, 4) void mixit_grad_kernel(const float* __restrict__ est, const int64_t* __restrict__ est_offs,
                                                            const void* __restrict__ ref, int pcm16,
                                                            const int64_t* __restrict__ ref_offs,
                                                            const int32_t* __restrict__ nframes,
                                                            const int32_t* __restrict__ best_code, const float* __restrict__ coef,
                                                            const float* __restrict__ gscale, const float2* __restrict__ mix,
                                                            const int32_t* __restrict__ offs, int M, float* __restrict__ dmask,
                                                            int ld) {
  const int un = blockIdx.y;
  const int u = un >> 1, grp = un & 1;
  const int T = nframes[u];
  const int tile0 = blockIdx.x * TPB;
  if (tile0 * FPB >= T) return;
  // the group's members, ascending: their sample streams and their column blocks (slots >= nm repeat the first member)
  const int code = __builtin_amdgcn_readfirstlane(best_code[u]);
  int nm = 0, col[SK_MAXS];
  const float* ep[SK_MAXS];
#pragma unroll
  for (int q = 0; q < SK_MAXS; ++q) {
    col[q] = 0;
    ep[q] = est;
  }
#pragma unroll
  for (int k = SK_MAXS - 1; k >= 0; --k)  // descending, each member pushed to the front: slot 0 ends as the first member
    if (k < M && ((code >> k) & 1) == grp) {
#pragma unroll
      for (int q = SK_MAXS - 1; q > 0; --q) {
        col[q] = col[q - 1];
        ep[q] = ep[q - 1];
      }
      col[0] = k * NBIN;
      ep[0] = est + est_offs[u * M + k];
      ++nm;
    }
  if (nm == 0) return;  // block-uniform: nobody waits at a barrier
  const float cD = coef[un] * gscale[0];
  const float xs = pcm16 ? 1.0f / 32768.0f : 1.0f;
  const int64_t roff = ref_offs[un];
  grad_tiles(
      u, T, tile0, mix, offs, dmask, ld,
      [&](int n) {
#pragma clang fp contract(off)
        const float rv = ref_raw(ref, pcm16, roff, n);
        float m = ep[0][n];
        if (nm > 1) m += ep[1][n];
        if (nm > 2) m += ep[2][n];
        if (nm > 3) m += ep[3][n];
        return cD * __builtin_fmaf(-rv, xs, m);
      },
      [&](float* at, float v) {
        at[col[0]] = v;
        if (nm > 1) at[col[1]] = v;
        if (nm > 2) at[col[2]] = v;
        if (nm > 3) at[col[3]] = v;
      });
}

// ---- phase-sensitive targets (include/sepkern.h, sk_stft_psa; the definition is sepkern/psa.py's).
// stft_kernel<frame-major> with a loop over the S + 1 signals of a tile and another epilogue: the mixture (q = 0) leaves
// |Y| in its row and its 257 complex bins in the work rows; every source bin is contracted on its way out with the mixture's,
//   target = (Re S Re Y + Im S Im Y) / |Y|   (0 where |Y|^2 < 2^-100; with clamp, held to [0, |Y|]),
// and stored from registers at row offs[t] + u (packed) or row_base[u] + t.  A lane reads back exactly the bins it wrote itself
// (lane j of a frame's group: Y[j + 16 k2] and the mirrors Y[256 - j - 16 k2], k2 < 8, lane 0 also Y[128]) a few microseconds
// later: they come from L2.  Holding them in registers instead -- 17 complex values, 34 VGPRs on top of stft_kernel's 108 at
// four workgroups per CU -- compiled to 128 VGPRs with 8 of them spilled to scratch.  The next signal's
// samples of the same tile (or the next tile's mixture) travel while the current one is transformed.  Vector stores only.
__device__ __forceinline__ void pin(v2f& x) {  // the bin is final here: what is done with it must not reach back into how it is rounded
  asm volatile("" : "+v"(x.x), "+v"(x.y));
}

__global__ __launch_bounds__(256, 4) void stft_psa_kernel(const void* __restrict__ wav, int pcm16, const int64_t* __restrict__ sig_offs,
                                                          const int32_t* __restrict__ nsamp, int B, int S, int clamp,
                                                          const int32_t* __restrict__ offs, const int64_t* __restrict__ row_base,
                                                          float* mix_rows, float* __restrict__ targets, int ld,
                                                          int64_t plane, float2* ywork) {
  __shared__ __attribute__((aligned(16))) float smp[NFFT + (FPB - 1) * HOP];
  __shared__ __attribute__((aligned(16))) float win[NFFT];
  __shared__ float2 tw[NFFT];
  __shared__ float2 t256[256];
  __shared__ float xch[16][16 * XLD];

  const int u = blockIdx.y;
  const int N = nsamp[u];
  const int T = 1 + N / HOP;
  const int tile0 = blockIdx.x * TPB;
  if (tile0 * FPB >= T) return;
  const int tend = min(T, (tile0 + TPB) * FPB);  // this block's frames: [tile0 * FPB, tend)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int SPAN = NFFT + (FPB - 1) * HOP, SPT = (SPAN + 255) / 256;

  // stft_kernel's sample loader, the signal q of the utterance chosen per call
  auto fetch = [&](int t0, int q, float (&r)[SPT]) {
    const int64_t woff = sig_offs[(int64_t)q * B + u];
    const int nfr = min(FPB, T - t0);
    const int span = NFFT + (nfr - 1) * HOP;
    const int first = t0 * HOP - NFFT / 2;
    if (first >= 0 && first + SPAN <= N) {
      if (pcm16) {
        const int16_t* w = (const int16_t*)wav + woff + first;
#pragma unroll
        for (int i2 = 0; i2 < SPT; ++i2) {
          const int i = tid + 256 * i2;
          r[i2] = (i < SPAN) ? (float)w[i] * (1.0f / 32768.0f) : 0.f;
        }
      } else {
        const float* w = (const float*)wav + woff + first;
#pragma unroll
        for (int i2 = 0; i2 < SPT; ++i2) {
          const int i = tid + 256 * i2;
          r[i2] = (i < SPAN) ? w[i] : 0.f;
        }
      }
      return;
    }
#pragma unroll
    for (int i2 = 0; i2 < SPT; ++i2) {
      const int i = tid + 256 * i2;
      int src = first + i;
      if (src < 0) src = -src;
      if (src >= N) src = 2 * (N - 1) - src;
      src = max(0, min(src, N - 1));
      float v = pcm16 ? (float)((const int16_t*)wav)[woff + src] * (1.0f / 32768.0f) : ((const float*)wav)[woff + src];
      r[i2] = (i < span) ? v : 0.f;
    }
  };
  auto stash = [&](const float (&r)[SPT]) {
#pragma unroll
    for (int i2 = 0; i2 < SPT; ++i2) {
      const int i = tid + 256 * i2;
      if (i < SPAN) smp[i] = r[i2];
    }
  };

  for (int i = tid; i < NFFT; i += 256) {
    tw[i] = g_tw512[i];
    win[i] = g_hann512[i];
  }
  t256[tid] = g_tw512[(2 * (tid & 15) * (tid >> 4)) & 511];
  float pre[SPT];
  fetch(tile0 * FPB, 0, pre);
  stash(pre);
  __syncthreads();

  const int j = lane & 15, g = lane >> 4;
  const int fr = 4 * wave + g;
  const int partner = (lane & 48) | ((16 - j) & 15);
  // a source's bin s against the mixture's y: one fused product-sum, the reciprocal square root, one multiply.  The upper end
  // of the truncated form is the |Y| this lane STORED at q == 0, read back (mag): the stored bits, whichever way the compiler
  // contracts a second y.x * y.x + y.y * y.y.
  auto target = [&](v2f s, v2f y, const float* mag) {
    const float y2 = y.x * y.x + y.y * y.y;
    float v = (s.x * y.x + s.y * y.y) * __builtin_amdgcn_rsqf(y2);
    if (!(y2 >= 0x1p-100f)) v = 0.f;
    if (clamp) v = fminf(fmaxf(v, 0.f), *mag);
    return v;
  };

  int t0 = tile0 * FPB, q = 0;
  while (true) {  // (t0, q) in the order tiles outer, signals inner; every condition is block-uniform
    int nq = q + 1, nt0 = t0;
    if (nq > S) {
      nq = 0;
      nt0 = t0 + FPB;
    }
    const bool more = nt0 < tend;
    if (more) fetch(nt0, nq, pre);  // the next signal's samples travel while this one is transformed
    const bool active = fr < min(FPB, T - t0);
    v2f z[16];
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) {
      const v2f sm = *reinterpret_cast<const v2f*>(&smp[fr * HOP + 32 * n1 + 2 * j]);
      const v2f w = *reinterpret_cast<const v2f*>(&win[32 * n1 + 2 * j]);
      z[n1] = sm * w;
    }
    fft256_g16(z, xch[4 * wave + g], t256, j);

    if (active) {  // uniform over the 16-lane group, which is all the shuffles below reach
      const int64_t row = offs ? (int64_t)offs[t0 + fr] + u : row_base[u] + (t0 + fr);
      float* const base = (q == 0 ? mix_rows : targets + (int64_t)(q - 1) * plane) + row * ld;
      float* const olo = base + j;
      float* const ohi = base + (256 - j);
      const float* const mlo = mix_rows + row * ld + j;  // |Y| of this frame, as stored
      const float* const mhi = mix_rows + row * ld + (256 - j);
      float2* const ylo = ywork + row * NBIN + j;  // the mixture's bins of this frame, written at q == 0 by this very lane
      float2* const yhi = ywork + row * NBIN + (256 - j);
#pragma unroll
      for (int k2 = 0; k2 < 8; ++k2) {  // real-FFT split as in stft_kernel
        v2f zc;
        zc.x = __shfl(z[15 - k2].x, partner, 64);
        zc.y = __shfl(z[15 - k2].y, partner, 64);
        if (j == 0) zc = z[(16 - k2) & 15];
        const v2f zk = z[k2], cz = conj(zc);
        const int k = j + 16 * k2;
        const v2f A = 0.5f * (zk + cz), Bt = cmul(ld2(&tw[k]), 0.5f * mul_mi(zk - cz));
        v2f xa = A + Bt, xb = conj(A - Bt);  // X[k], X[256 - k]
        pin(xa);
        pin(xb);
        if (q == 0) {
          st2(ylo + 16 * k2, xa);
          st2(yhi - 16 * k2, xb);
          olo[16 * k2] = __builtin_amdgcn_sqrtf(xa.x * xa.x + xa.y * xa.y);
          ohi[-16 * k2] = __builtin_amdgcn_sqrtf(xb.x * xb.x + xb.y * xb.y);
        } else {
          olo[16 * k2] = target(xa, ld2(ylo + 16 * k2), mlo + 16 * k2);
          ohi[-16 * k2] = target(xb, ld2(yhi - 16 * k2), mhi - 16 * k2);
        }
      }
      if (j == 0) {  // bin 128 pairs with itself
        const v2f zk = z[8], cz = conj(zk);
        v2f xa = 0.5f * (zk + cz) + cmul(ld2(&tw[128]), 0.5f * mul_mi(zk - cz));
        pin(xa);
        if (q == 0) {
          st2(ylo + 128, xa);
          olo[128] = __builtin_amdgcn_sqrtf(xa.x * xa.x + xa.y * xa.y);
        } else {
          olo[128] = target(xa, ld2(ylo + 128), mlo + 128);
        }
      }
    }
    if (!more) break;
    __syncthreads();  // every wave is done with smp
    stash(pre);
    __syncthreads();
    t0 = nt0;
    q = nq;
  }
}

}  // namespace

extern "C" int sk_stft_psa(const void* wav, int pcm16, const int64_t* sig_offs, const int32_t* nsamp, int B, int S, int n_fft,
                           int hop, int clamp, const int32_t* offs, const int64_t* row_base, float* mix_rows, float* targets,
                           int ld, int64_t plane, void* ws, int min_samples, int max_frames, sk_stream_t stream) {
  SK_CHECK_ARG(n_fft == NFFT && hop == HOP, "sk_stft_psa: only n_fft=512, hop=128 are built (got %d, %d)", n_fft, hop);
  SK_CHECK_ARG(S >= 1 && S <= SK_MAXS, "sk_stft_psa: num_spk %d outside 1..%d", S, SK_MAXS);
  SK_CHECK_ARG(min_samples > NFFT / 2, "sk_stft_psa: an utterance of %d samples: reflect padding needs more than n_fft/2 = %d",
               min_samples, NFFT / 2);
  SK_CHECK_ARG(wav && sig_offs && nsamp && mix_rows && targets && ws, "sk_stft_psa: null pointer");
  SK_CHECK_ARG((offs != nullptr) != (row_base != nullptr), "sk_stft_psa: give the packed batch's offs or per-utterance row bases, one of them");
  SK_CHECK_ARG(ld >= NBIN, "sk_stft_psa: rows of %d floats hold fewer than F = %d", ld, NBIN);
  SK_CHECK_ARG(S == 1 || plane >= 0, "sk_stft_psa: negative plane stride");
  SK_CHECK_ARG(B > 0 && B <= 65535 && max_frames > 0, "sk_stft_psa: bad B/max_frames");
  dim3 grid((unsigned)sk_cdiv(max_frames, FPB * TPB), (unsigned)B);
  hipLaunchKernelGGL(stft_psa_kernel, grid, dim3(256), 0, (hipStream_t)stream, wav, pcm16, sig_offs, nsamp, B, S, clamp, offs,
                     row_base, mix_rows, targets, ld, plane, (float2*)ws);
  SK_CHECK_LAUNCH("sk_stft_psa");
  return SK_OK;
}

extern "C" int sk_stft(const void* wav, int pcm16, const int64_t* wav_offs, const int32_t* nsamp, int nutt, int n_fft,
                       int hop, int want_complex, void* out, const int64_t* out_offs, const int64_t* stride_t,
                       const int64_t* stride_f, int frame_major, int max_frames, sk_stream_t stream) {
  SK_CHECK_ARG(n_fft == NFFT && hop == HOP, "sk_stft: only n_fft=512, hop=128 are built (got %d, %d)", n_fft, hop);
  SK_CHECK_ARG(wav && wav_offs && nsamp && out && out_offs && stride_t && stride_f, "sk_stft: null pointer");
  SK_CHECK_ARG(nutt > 0 && nutt <= 65535 && max_frames > 0, "sk_stft: bad nutt/max_frames");
  dim3 grid((unsigned)sk_cdiv(max_frames, FPB * TPB), (unsigned)nutt);
#define SK_STFT_LAUNCH(BM, CX)                                                                                 \
  hipLaunchKernelGGL((stft_kernel<BM, CX>), grid, dim3(256), 0, (hipStream_t)stream, wav, pcm16, wav_offs, nsamp, \
                     out, out_offs, stride_t, stride_f)
  if (frame_major) {
    if (want_complex) SK_STFT_LAUNCH(false, true); else SK_STFT_LAUNCH(false, false);
  } else {
    if (want_complex) SK_STFT_LAUNCH(true, true); else SK_STFT_LAUNCH(true, false);
  }
#undef SK_STFT_LAUNCH
  SK_CHECK_LAUNCH("sk_stft");
  return SK_OK;
}

extern "C" int sk_mask_istft(const void* mix_c64, const int64_t* mix_offs, const int64_t* mix_st,
                             const int64_t* mix_sf, const float* mask, const int64_t* mask_offs,
                             const int64_t* mask_st, const int64_t* mask_sf, const int32_t* nframes, int nutt, int S,
                             int n_fft, int hop, float* wav_out, int16_t* pcm_out, const int64_t* out_offs,
                             int max_frames, sk_stream_t stream) {
  SK_CHECK_ARG(n_fft == NFFT && hop == HOP, "sk_mask_istft: only n_fft=512, hop=128 are built");
  SK_CHECK_ARG(mix_c64 && mix_offs && mix_st && mix_sf && nframes && out_offs, "sk_mask_istft: null pointer");
  SK_CHECK_ARG(!mask || (mask_offs && mask_st && mask_sf), "sk_mask_istft: mask given without its strides");
  SK_CHECK_ARG(wav_out || pcm_out, "sk_mask_istft: no output buffer");
  SK_CHECK_ARG(nutt > 0 && S > 0 && (int64_t)nutt * S <= 65535 && max_frames > 1, "sk_mask_istft: bad sizes");
  // tiles of 16 hops per (utterance, source); a workgroup walks `tpb` of them so that every frame is transformed
  // once, as long as that still leaves a few workgroups per CU
  const int ntiles = max_frames / FPB + 1;
  const int64_t total = (int64_t)ntiles * nutt * S;
  const int tpb = (int)std::min<int64_t>(std::max<int64_t>(total / 2048, 2), ntiles);
  dim3 grid((unsigned)sk_cdiv(ntiles, tpb), (unsigned)(nutt * S));
  hipLaunchKernelGGL(istft_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const float2*)mix_c64, mix_offs, mix_st,
                     mix_sf, mask, mask_offs, mask_st, mask_sf, nframes, S, wav_out, pcm_out, out_offs, tpb);
  SK_CHECK_LAUNCH("sk_mask_istft");
  return SK_OK;
}

extern "C" int sk_mask_istft_rows(const void* mix_rows_c64, const float* mask, int ld, const int32_t* offs,
                                  const int32_t* nframes, int B, int S, int n_fft, int hop, float* wav_out,
                                  const int64_t* out_offs, int max_frames, sk_stream_t stream) {
  SK_CHECK_ARG(n_fft == NFFT && hop == HOP, "sk_mask_istft_rows: only n_fft=512, hop=128 are built (got %d, %d)", n_fft, hop);
  SK_CHECK_ARG(S >= 1 && S <= SK_MAXS, "sk_mask_istft_rows: num_spk %d outside 1..%d", S, SK_MAXS);
  SK_CHECK_ARG(mix_rows_c64 && mask && offs && nframes && wav_out && out_offs, "sk_mask_istft_rows: null pointer");
  SK_CHECK_ARG(ld >= S * NBIN, "sk_mask_istft_rows: mask rows of %d floats hold fewer than S*F = %d", ld, S * NBIN);
  SK_CHECK_ARG(B > 0 && (int64_t)B * S <= 65535 && max_frames > 1, "sk_mask_istft_rows: bad sizes");
  const int ntiles = max_frames / FPB + 1;
  const int64_t total = (int64_t)ntiles * B * S;
  const int tpb = (int)std::min<int64_t>(std::max<int64_t>(total / 2048, 2), ntiles);
  dim3 grid((unsigned)sk_cdiv(ntiles, tpb), (unsigned)(B * S));
  hipLaunchKernelGGL(istft_rows_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const float2*)mix_rows_c64, mask, ld, offs,
                     nframes, S, wav_out, out_offs, tpb);
  SK_CHECK_LAUNCH("sk_mask_istft_rows");
  return SK_OK;
}

extern "C" int sk_sisdr_mask_grad(const float* est, const int64_t* est_offs, const void* ref, int pcm16,
                                  const int64_t* ref_offs, const int32_t* nframes, const int32_t* best_perm,
                                  const float* coef, const float* gscale, const void* mix_rows_c64, const int32_t* offs,
                                  int B, int S, int n_fft, int hop, int max_frames, float* dmask, int ld,
                                  sk_stream_t stream) {
  SK_CHECK_ARG(n_fft == NFFT && hop == HOP, "sk_sisdr_mask_grad: only n_fft=512, hop=128 are built (got %d, %d)", n_fft, hop);
  SK_CHECK_ARG(S >= 1 && S <= SK_MAXS, "sk_sisdr_mask_grad: num_spk %d outside 1..%d", S, SK_MAXS);
  SK_CHECK_ARG(est && est_offs && ref && ref_offs && nframes && best_perm && coef && gscale && mix_rows_c64 && offs && dmask,
               "sk_sisdr_mask_grad: null pointer");
  SK_CHECK_ARG(ld >= S * NBIN, "sk_sisdr_mask_grad: dmask rows of %d floats hold fewer than S*F = %d", ld, S * NBIN);
  SK_CHECK_ARG(B > 0 && (int64_t)B * S <= 65535 && max_frames > 1, "sk_sisdr_mask_grad: bad sizes");
  dim3 grid((unsigned)sk_cdiv(max_frames, FPB * TPB), (unsigned)(B * S));
  hipLaunchKernelGGL(sisdr_grad_kernel, grid, dim3(256), 0, (hipStream_t)stream, est, est_offs, ref, pcm16, ref_offs, nframes,
                     best_perm, coef, gscale, (const float2*)mix_rows_c64, offs, S, dmask, ld);
  SK_CHECK_LAUNCH("sk_sisdr_mask_grad");
  return SK_OK;
}

extern "C" int sk_mixit_mask_grad(const float* est, const int64_t* est_offs, const void* ref, int pcm16,
                                  const int64_t* ref_offs, const int32_t* nframes, const int32_t* best_code,
                                  const float* coef, const float* gscale, const void* mix_rows_c64, const int32_t* offs,
                                  int B, int M, int n_fft, int hop, int max_frames, float* dmask, int ld,
                                  sk_stream_t stream) {
  SK_CHECK_ARG(n_fft == NFFT && hop == HOP, "sk_mixit_mask_grad: only n_fft=512, hop=128 are built (got %d, %d)", n_fft, hop);
  SK_CHECK_ARG(M >= 2 && M <= SK_MAXS, "sk_mixit_mask_grad: %d estimates per utterance, outside 2..%d", M, SK_MAXS);
  SK_CHECK_ARG(est && est_offs && ref && ref_offs && nframes && best_code && coef && gscale && mix_rows_c64 && offs && dmask,
               "sk_mixit_mask_grad: null pointer");
  SK_CHECK_ARG(ld >= M * NBIN, "sk_mixit_mask_grad: dmask rows of %d floats hold fewer than M*F = %d", ld, M * NBIN);
  SK_CHECK_ARG(B > 0 && (int64_t)B * 2 <= 65535 && max_frames > 1, "sk_mixit_mask_grad: bad sizes");
  dim3 grid((unsigned)sk_cdiv(max_frames, FPB * TPB), (unsigned)(B * 2));
  hipLaunchKernelGGL(mixit_grad_kernel, grid, dim3(256), 0, (hipStream_t)stream, est, est_offs, ref, pcm16, ref_offs, nframes,
                     best_code, coef, gscale, (const float2*)mix_rows_c64, offs, M, dmask, ld);
  SK_CHECK_LAUNCH("sk_mixit_mask_grad");
  return SK_OK;
}
