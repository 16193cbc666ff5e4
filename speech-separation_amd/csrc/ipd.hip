// ipd.hip -- inter-channel phase features for a network that sees an array (include/sepkern.h, sk_stft_ipd / sk_ipd_rows; the
// definition is sepkern/ipd.py's).  A feature row is [ |Y_r| (257) | cos_1 | sin_1 | ... | cos_P | sin_P ], cos / sin of the phase
// of listed channel c against the reference channel r, 0 where either fp32 squared magnitude is below 2^-100.
//   stft_ipd_kernel  training: from the batch's PCM to the packed rows in one launch.  stft_psa_kernel's structure (stft.hip):
//                    tiles outer, the 1 + P signals of an utterance inner; the reference (q = 0) leaves |Y_r| in the row and its
//                    257 bins in the work rows, every later channel is contracted with them on its way out, by the lane that
//                    wrote them, and stored from registers.  Streaming: 128 new samples in, 257 (or 514) floats out per frame
//                    and signal; the reference's bins come back from L2.
//   ipd_rows_kernel  inference: the same features from spectra already in memory, a plain streaming kernel.
// Both call ipd_feature, which spells its roundings out, so the two agree bit for bit on the same spectra.
// Shape coverage: tests/test_gpu_ipd.py runs both at 165, 81, 80, 17, 16 and 3 frames -- several workgroups, either side of the
// 16-frame tile (and of stft_kernel's 80-frame workgroup), below one tile -- with 1, 2 and 7 listed channels, against fp64.
#include "fft512.h"

namespace {

// cos and sin of arg(yc conj yr).  Every rounding is written out -- one product and one fused multiply-add per numerator and per
// squared magnitude, two reciprocal square roots (never one of the product: 2^-100 x 2^-100 underflows), two products -- so
// that the file's contraction setting decides nothing: sk_stft_ipd and sk_ipd_rows must agree bit for bit.
__device__ __forceinline__ v2f ipd_feature(v2f yc, v2f yr) {
#pragma clang fp contract(off)
  const float c2 = __fmaf_rn(yc.x, yc.x, __fmul_rn(yc.y, yc.y));
  const float r2 = __fmaf_rn(yr.x, yr.x, __fmul_rn(yr.y, yr.y));
  const float re = __fmaf_rn(yc.x, yr.x, __fmul_rn(yc.y, yr.y));
  const float im = __fmaf_rn(yc.y, yr.x, -__fmul_rn(yc.x, yr.y));
  const float ic = __builtin_amdgcn_rsqf(c2), ir = __builtin_amdgcn_rsqf(r2);
  v2f v = {__fmul_rn(__fmul_rn(re, ic), ir), __fmul_rn(__fmul_rn(im, ic), ir)};
  if (!(c2 >= 0x1p-100f && r2 >= 0x1p-100f)) v = (v2f){0.f, 0.f};
  return v;
}

// |x| with the roundings of stft_kernel<frame-major, magnitude> (stft.hip) as it compiles: both squares rounded, their sum, the
// root -- written out, since this file's x.x * x.x + x.y * x.y was contracted to a fused multiply-add and missed sk_stft's last
// bit (tests/test_gpu_ipd.py holds the two kernels to each other).
__device__ __forceinline__ float magnitude(v2f x) {
#pragma clang fp contract(off)
  const float a = x.x * x.x, b = x.y * x.y;  // (plain operators: the pragma reaches them, not the body of an inlined __fadd_rn)
  return __builtin_amdgcn_sqrtf(a + b);
}

__device__ __forceinline__ void pin(v2f& x) {  // the bin is final here: what is done with it must not reach back into how it is rounded
  asm volatile("" : "+v"(x.x), "+v"(x.y));
}

constexpr int SPAN = NFFT + (FPB - 1) * HOP, SPT = (SPAN + 255) / 256;  // samples per tile / per thread
// Consecutive 16-frame tiles per workgroup of stft_ipd_kernel.  One: a tile is already 1 + P transforms whose samples are
// prefetched one behind the other, and a batch of 32 x 400 frames then gives 800 workgroups instead of stft_kernel's 160 (TPB = 5)
// on 256 CUs -- measured 31 / 58 / 132 us against 71 / 134 / 259 us at C = 2 / 4 / 8 (profiles/ipd.txt).  The tile loop below
// is written for any value.
constexpr int IPD_TPB = 1;

// stft_kernel's sample loader (stft.hip): the reflect-padded samples [t0*HOP, t0*HOP + SPAN) of the signal of N samples at
// wav + woff (zeros past the last frame), thread tid taking samples tid + 256 i.  Tiles whose whole span lies inside the signal
// take a block-uniform path without the reflect / clamp arithmetic.
__device__ __forceinline__ void fetch_samples(const void* __restrict__ wav, int pcm16, int64_t woff, int N, int T, int t0, int tid,
                                              float (&r)[SPT]) {
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
}

// blockIdx.y = utterance, blockIdx.x = group of IPD_TPB tiles.  Signal q of utterance u: sig_offs[q * B + u]; q = 0 is the reference.
// Row of frame t: offs[t] + u (packed) or row_base[u] + t.  Listed channel q >= 1 owns columns 257 (2q - 1) .. 257 (2q + 1) - 1.
// zpad = the columns behind the features that are stored as zeros (to the next multiple of 16, or to ld if that comes first).
__global__ __launch_bounds__(256, 4) void stft_ipd_kernel(const void* __restrict__ wav, int pcm16, const int64_t* __restrict__ sig_offs,
                                                          const int32_t* __restrict__ nsamp, int B, int P,
                                                          const int32_t* __restrict__ offs, const int64_t* __restrict__ row_base,
                                                          float* rows, int ld, int zpad, float* __restrict__ mix_rows, float2* ywork) {
  __shared__ __attribute__((aligned(16))) float smp[SPAN];
  __shared__ __attribute__((aligned(16))) float win[NFFT];
  __shared__ float2 tw[NFFT];
  __shared__ float2 t256[256];
  __shared__ float xch[16][16 * XLD];

  const int u = blockIdx.y;
  const int N = nsamp[u];
  const int T = 1 + N / HOP;
  const int tile0 = blockIdx.x * IPD_TPB;
  if (tile0 * FPB >= T) return;
  const int tend = min(T, (tile0 + IPD_TPB) * FPB);  // this block's frames: [tile0 * FPB, tend)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

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
  fetch_samples(wav, pcm16, sig_offs[u], N, T, tile0 * FPB, tid, pre);
  stash(pre);
  __syncthreads();

  const int j = lane & 15, g = lane >> 4;
  const int fr = 4 * wave + g;
  const int partner = (lane & 48) | ((16 - j) & 15);

  int t0 = tile0 * FPB, q = 0;
  while (true) {  // (t0, q) in the order tiles outer, signals inner; every condition is block-uniform
    int nq = q + 1, nt0 = t0;
    if (nq > P) {
      nq = 0;
      nt0 = t0 + FPB;
    }
    const bool more = nt0 < tend;
    if (more) fetch_samples(wav, pcm16, sig_offs[(int64_t)nq * B + u], N, T, nt0, tid, pre);  // travels while this signal is transformed
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
      // q == 0: the magnitude columns; q >= 1: the cos block of the channel, its sin block NBIN floats on
      // The lane's bins are j + 16 k2 and their mirrors 256 - j - 16 k2: two element indices and constant offsets from them, into
      // the output row (oi) and into the work rows and mix_rows alike (yi: both are (rows, 257)).  Indices, not five pointers:
      // with the pointers held across the loop the kernel compiled to 128 VGPRs with 4 of them spilled.
      const int64_t oi = row * ld + (q == 0 ? 0 : NBIN * (2 * q - 1)) + j;
      const int64_t yi = row * NBIN + j;  // the reference's bins of this frame, written at q == 0 by this very lane
      const int mir = 256 - 2 * j;        // bin 256 - j - 16 k2 lies mir - 16 k2 behind bin j
      auto put = [&](v2f x, int off) {
        if (q == 0) {
          st2(ywork + yi + off, x);
          const float m = magnitude(x);
          rows[oi + off] = m;
          if (mix_rows) mix_rows[yi + off] = m;
        } else {
          const v2f f = ipd_feature(x, ld2(ywork + yi + off));
          rows[oi + off] = f.x;
          rows[oi + off + NBIN] = f.y;
        }
      };
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
        put(xa, 16 * k2);
        put(xb, mir - 16 * k2);
      }
      if (j == 0) {  // bin 128 pairs with itself
        const v2f zk = z[8], cz = conj(zk);
        v2f xa = 0.5f * (zk + cz) + cmul(ld2(&tw[128]), 0.5f * mul_mi(zk - cz));
        pin(xa);
        put(xa, 128);
      }
      if (q == 0 && j < zpad) rows[row * ld + NBIN * (1 + 2 * P) + j] = 0.f;  // zpad <= 15
    }
    if (!more) break;
    __syncthreads();  // every wave is done with smp
    stash(pre);
    __syncthreads();
    t0 = nt0;
    q = nq;
  }
}

struct IpdChans {
  int c[7];
};

// One workgroup per frame: thread tid takes bins tid (and 256 for tid 0).  The magnitude columns are copied from mag, unchanged.
__global__ __launch_bounds__(256) void ipd_rows_kernel(const float2* __restrict__ Y, int64_t ycs, int64_t yrs, int ref, int P,
                                                       IpdChans ch, const float* __restrict__ mag, int ld_mag, float* __restrict__ rows,
                                                       int ld, int zpad) {
  const int64_t t = blockIdx.x;
  const int tid = threadIdx.x;
  float* const out = rows + t * ld;
  const float2* const yr = Y + ref * ycs + t * yrs;
  for (int k = tid; k < NBIN; k += 256) {
    out[k] = mag[t * ld_mag + k];
    const v2f r = ld2(yr + k);
#pragma unroll
    for (int p = 0; p < 7; ++p) {
      if (p < P) {
        const v2f f = ipd_feature(ld2(Y + ch.c[p] * ycs + t * yrs + k), r);
        out[NBIN * (1 + 2 * p) + k] = f.x;
        out[NBIN * (2 + 2 * p) + k] = f.y;
      }
    }
  }
  if (tid < zpad) out[NBIN * (1 + 2 * P) + tid] = 0.f;
}

// the columns behind a row's `width` features that are stored as zeros: up to the next multiple of 16, or to ld if that is nearer
int zero_columns(int width, int ld) { return (int)std::min<int64_t>(ld, sk_align(width, 16)) - width; }

}  // namespace

extern "C" int sk_stft_ipd(const void* wav, int pcm16, const int64_t* sig_offs, const int32_t* nsamp, int B, int C, int n_fft,
                           int hop, const int32_t* offs, const int64_t* row_base, float* rows, int ld, float* mix_rows, void* ws,
                           int min_samples, int max_frames, sk_stream_t stream) {
  SK_CHECK_ARG(n_fft == NFFT && hop == HOP, "sk_stft_ipd: only n_fft=512, hop=128 are built (got %d, %d)", n_fft, hop);
  SK_CHECK_ARG(C >= 2 && C <= 8, "sk_stft_ipd: C = %d signals per utterance outside 2..8 (the reference and 1..7 listed channels)", C);
  SK_CHECK_ARG(min_samples > NFFT / 2, "sk_stft_ipd: an utterance of %d samples: reflect padding needs more than n_fft/2 = %d",
               min_samples, NFFT / 2);
  SK_CHECK_ARG(wav && sig_offs && nsamp && rows && ws, "sk_stft_ipd: null pointer");
  SK_CHECK_ARG((offs != nullptr) != (row_base != nullptr), "sk_stft_ipd: give the packed batch's offs or per-utterance row bases, one of them");
  const int width = NBIN * (2 * C - 1);
  SK_CHECK_ARG(ld >= width, "sk_stft_ipd: ld = %d, rows hold fewer than 257 (1 + 2P) = %d floats", ld, width);
  SK_CHECK_ARG(B > 0 && B <= 65535 && max_frames > 0, "sk_stft_ipd: bad B/max_frames (B = %d, at most 65535)", B);
  dim3 grid((unsigned)sk_cdiv(max_frames, FPB * IPD_TPB), (unsigned)B);
  hipLaunchKernelGGL(stft_ipd_kernel, grid, dim3(256), 0, (hipStream_t)stream, wav, pcm16, sig_offs, nsamp, B, C - 1, offs, row_base,
                     rows, ld, zero_columns(width, ld), mix_rows, (float2*)ws);
  SK_CHECK_LAUNCH("sk_stft_ipd");
  return SK_OK;
}

extern "C" int sk_ipd_rows(const void* Y_c64, int64_t y_chan_stride, int64_t y_row_stride, int T, int C, int ref, const int32_t* chans_host,
                           int P, const float* mag, int ld_mag, float* rows, int ld, sk_stream_t stream) {
  SK_CHECK_FRAMES("sk_ipd_rows", T);
  SK_CHECK_ARG(C >= 2 && C <= 8, "sk_ipd_rows: C = %d channels outside 2..8", C);
  SK_CHECK_REF("sk_ipd_rows", ref, C);
  SK_CHECK_ARG(chans_host && P >= 1 && P <= 7, "sk_ipd_rows: P = %d listed channels outside 1..7 (or no list)", P);
  IpdChans ch = {};
  for (int p = 0; p < P; ++p) {
    const int c = chans_host[p];
    SK_CHECK_ARG(c >= 0 && c < C, "sk_ipd_rows: channel %d outside [0, %d)", c, C);
    SK_CHECK_ARG(c != ref, "sk_ipd_rows: channel %d is the reference (repeated)", c);
    for (int p2 = 0; p2 < p; ++p2) SK_CHECK_ARG(ch.c[p2] != c, "sk_ipd_rows: channel %d is repeated", c);
    ch.c[p] = c;
  }
  SK_CHECK_Y_ROW_STRIDE("sk_ipd_rows", y_row_stride);
  SK_CHECK_ARG(y_chan_stride >= 0, "sk_ipd_rows: negative y_chan_stride");
  const int width = NBIN * (1 + 2 * P);
  SK_CHECK_ARG(ld >= width, "sk_ipd_rows: ld = %d, rows hold fewer than 257 (1 + 2P) = %d floats", ld, width);
  SK_CHECK_ARG(ld_mag >= NBIN, "sk_ipd_rows: ld_mag = %d below 257", ld_mag);
  SK_CHECK_ARG(Y_c64 && mag && rows, "sk_ipd_rows: null pointer");
  hipLaunchKernelGGL(ipd_rows_kernel, dim3((unsigned)T), dim3(256), 0, (hipStream_t)stream, (const float2*)Y_c64, y_chan_stride,
                     y_row_stride, ref, P, ch, mag, ld_mag, rows, ld, zero_columns(width, ld));
  SK_CHECK_LAUNCH("sk_ipd_rows");
  return SK_OK;
}
