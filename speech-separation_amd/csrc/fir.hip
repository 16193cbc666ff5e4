// fir.hip -- convolution of signals with room impulse responses (sk_fir_convolve), gfx950: the stage in front of sk_dynamic_mix
// that makes dynamic mixtures reverberant.  The definition is sepkern/reverb.py's: y[i] = sum_k h[k] x[i + delay - k], 0 <= i < n,
// x zero outside [0, n); convolve_partitioned_f32 there restates the arithmetic below in numpy float32.
//
// Uniformly partitioned overlap-save on the 256-point complex FFT of fft512.h (a 512-point real transform per 16-lane group).
// For a job of n samples, L taps (K = ceil(L / 256) partitions) at delay d, with the block grid on the FULL convolution's index:
//     X_b = rfft512(x[256 (b - 1) .. 256 (b + 1))), zero outside the signal       b = 0 .. bx1 = min(b1, (n - 1) / 256 + 1)
//     H_k = rfft512(taps [256 k .. 256 k + 256) followed by 256 zeros)            k = 0 .. K - 1
//     Y_b = sum_k H_k X_{b-k},  k ascending over max(0, b - bx1) .. min(K - 1, b)  (the X beyond bx1 are transforms of zeros)
//     full[256 b .. 256 b + 256) = the last 256 samples of irfft512(Y_b)          b = b0 = d / 256 .. b1 = (d + n - 1) / 256
//     out[i] = full[d + i]
// (d < L <= 256 K, so b0 - K + 1 <= 0: the first output block always reaches back to X_0.)
//
// TWO launches, with the spectra in the caller's workspace between them:
//   fir_spectra_kernel   every job's H_k and X_b: one 16-lane group per transform, 16 per workgroup;
//   fir_output_kernel    one 16-lane group per output block: accumulates its own 257 bins over k (every lane its 17 bins, one
//                        fixed pair of fmas per bin and part), inverts -- the FORWARD transform of the conjugate -- and stores
//                        only the samples inside [d, d + n).
// The one-launch form would transform the K neighbouring blocks again in every output block: K times the forward FFTs (19 times
// at 4 800 taps) to save a round trip through L2 of spectra that are read K times anyway.
// No atomics, no hand-off between workgroups inside a launch, one summation order: a job's bits depend neither on the batch
// around it nor on the run, and int16 samples (scaled by 1/32768, exact) give the bits their float32 copies give.
#include <vector>

#include "fft512.h"

namespace {

constexpr int FIR_P = 256;            // taps per partition = output samples per block
constexpr int FIR_SPEC = 264;         // float2 per stored spectrum: bins 0 .. 256, padded to a multiple of 64 bytes
constexpr int FIR_MAX_TAPS = 8192;
constexpr int FIR_MAX_JOBS = 65535;
constexpr int FIR_MAX_SAMPLES = 1 << 30;

// One job as both kernels read it (built on the host, copied into the workspace).
struct FirJob {
  int64_t in_off, rir_off, out_off;  // elements
  int64_t ws_off;                    // first spectrum of the job: K of H, then bx1 + 1 of X
  int32_t n, L, d, K, b0, bx1;
  int32_t t_start;                   // index of the job's first transform among all of launch one
  int32_t o_start;                   // index of the job's first output block among all of launch two
};

struct FirPlan {
  int64_t transforms, blocks, spectra;
};

// Checks of the job arrays, shared by the size query and the call; 0 = fine, else the index of the message below.
const char* const kFirWhy[] = {"", "ntaps outside 1..8192", "delay outside [0, ntaps)", "nsamp outside 1..2^30",
                               "more than 2^31 - 1 transforms or output blocks in one call"};

int fir_plan(const int32_t* nsamp, const int32_t* ntaps, const int32_t* delay, int J, FirPlan* plan, int* bad_job, FirJob* jobs) {
  int64_t t = 0, o = 0, s = 0;
  for (int j = 0; j < J; ++j) {
    *bad_job = j;
    const int64_t n = nsamp[j], L = ntaps[j], d = delay[j];
    if (L < 1 || L > FIR_MAX_TAPS) return 1;
    if (d < 0 || d >= L) return 2;
    if (n < 1 || n > FIR_MAX_SAMPLES) return 3;
    const int64_t K = (L + FIR_P - 1) / FIR_P, b0 = d / FIR_P, b1 = (d + n - 1) / FIR_P;
    const int64_t bx1 = std::min(b1, (n - 1) / FIR_P + 1);
    if (jobs) {
      jobs[j].ws_off = s;
      jobs[j].n = (int32_t)n; jobs[j].L = (int32_t)L; jobs[j].d = (int32_t)d; jobs[j].K = (int32_t)K;
      jobs[j].b0 = (int32_t)b0; jobs[j].bx1 = (int32_t)bx1;
      jobs[j].t_start = (int32_t)t;
      jobs[j].o_start = (int32_t)o;
    }
    t += K + bx1 + 1;
    o += b1 - b0 + 1;
    s += K + bx1 + 1;
    if (t > INT32_MAX - 16 || o > INT32_MAX - 16) return 4;
  }
  plan->transforms = t;
  plan->blocks = o;
  plan->spectra = s;
  return 0;
}

size_t fir_jobs_bytes(int J) { return sk_align((size_t)J * sizeof(FirJob), 256); }

// The job that holds item `idx` of a launch: the last j with start(j) <= idx (starts ascend strictly; start(0) = 0).
template <bool OUT>
__device__ __forceinline__ int fir_find(const FirJob* __restrict__ jobs, int J, int idx) {
  int lo = 0, hi = J - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((OUT ? jobs[mid].o_start : jobs[mid].t_start) <= idx) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// acc += h * x, the same two fmas per part wherever it is formed
__device__ __forceinline__ v2f fir_cmac(v2f h, v2f x, v2f acc) {
  v2f r;
  r.x = fmaf(-h.y, x.y, fmaf(h.x, x.x, acc.x));
  r.y = fmaf(h.y, x.x, fmaf(h.x, x.y, acc.y));
  return r;
}

// launch one -- grid: ceil(total / 16) workgroups of 256; transform q of a job: q < K the partition H_q, else the block X_{q-K}
template <bool PCM>
__global__ __launch_bounds__(256) void fir_spectra_kernel(const void* __restrict__ in, const float* __restrict__ rir,
                                                          const FirJob* __restrict__ jobs, int J, int total,
                                                          float2* __restrict__ spec) {
  __shared__ float2 tw[NFFT];
  __shared__ float2 t256[256];
  __shared__ float xch[16][16 * XLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  fft512_tables(tw, t256, tid);
  __syncthreads();
  const int l = lane & 15, g = lane >> 4;
  const int t = blockIdx.x * 16 + 4 * wave + g;
  const bool active = t < total;
  const int tt = active ? t : total - 1;  // an idle group goes through the transform (the wave's LDS exchange) and stores nothing
  const FirJob jb = jobs[fir_find<false>(jobs, J, tt)];
  const int q = tt - jb.t_start;
  const bool isH = q < jb.K;
  // sample r of the transform's 512 = element s0 + r of its source where that lies in [0, lim) and r < rmax
  const int s0 = isH ? FIR_P * q : FIR_P * (q - jb.K - 1);
  const int lim = isH ? jb.L : jb.n;
  const int rmax = isH ? FIR_P : NFFT;
  const float* hp = rir + jb.rir_off;
  const float* xf = (const float*)in + jb.in_off;
  const int16_t* xi = (const int16_t*)in + jb.in_off;
  v2f z[16];
#pragma unroll
  for (int n1 = 0; n1 < 16; ++n1) {  // packed point 16 n1 + l <-> samples r, r + 1, r = 32 n1 + 2 l
    const int r = 32 * n1 + 2 * l;
    float v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int s = s0 + r + e;
      v[e] = 0.f;
      if (r + e < rmax && s >= 0 && s < lim) {
        if (isH) v[e] = hp[s];
        else v[e] = PCM ? (float)xi[s] * (1.0f / 32768.0f) : xf[s];
      }
    }
    z[n1] = (v2f){v[0], v[1]};
  }
  fft256_g16(z, xch[4 * wave + g], t256, l);

  // real-FFT split as in stft_kernel: lane l forms X[k], X[256 - k] for k = l + 16 k2, k2 < 8; lane 0 also X[128]
  const int partner = (lane & 48) | ((16 - l) & 15);
  float2* const sp = spec + (jb.ws_off + q) * FIR_SPEC;
#pragma unroll
  for (int k2 = 0; k2 < 8; ++k2) {
    v2f zc;
    zc.x = __shfl(z[15 - k2].x, partner, 64);
    zc.y = __shfl(z[15 - k2].y, partner, 64);
    if (l == 0) zc = z[(16 - k2) & 15];
    const v2f zk = z[k2], cz = conj(zc);
    const int k = l + 16 * k2;
    const v2f A = 0.5f * (zk + cz), Bt = cmul(ld2(&tw[k]), 0.5f * mul_mi(zk - cz));
    if (active) {
      st2(&sp[k], A + Bt);
      st2(&sp[256 - k], conj(A - Bt));
    }
  }
  if (active && l == 0) st2(&sp[128], conj(z[8]));
}

// launch two -- grid: ceil(total / 16) workgroups of 256; one 16-lane group per output block
__global__ __launch_bounds__(256) void fir_output_kernel(const FirJob* __restrict__ jobs, int J, int total,
                                                         const float2* __restrict__ spec, float* __restrict__ out) {
  __shared__ float2 tw[NFFT];
  __shared__ float2 t256[256];
  __shared__ float xch[16][16 * XLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  fft512_tables(tw, t256, tid);
  __syncthreads();
  const int l = lane & 15, g = lane >> 4;
  const int ob = blockIdx.x * 16 + 4 * wave + g;
  const bool active = ob < total;
  const int oo = active ? ob : total - 1;
  const FirJob jb = jobs[fir_find<true>(jobs, J, oo)];
  const int b = jb.b0 + (oo - jb.o_start);
  const int k_lo = max(0, b - jb.bx1), k_hi = min(jb.K - 1, b);  // never empty (see the header comment)
  const float2* const H = spec + jb.ws_off * FIR_SPEC;
  const float2* const X = H + (int64_t)jb.K * FIR_SPEC;

  // acc[k2] = Y[l + 16 k2], acc[8 + k2] = Y[256 - (l + 16 k2)] (lane 0, k2 = 0: Y[0] and Y[256]), acc[16] = Y[128] (used by lane 0)
  v2f acc[17];
#pragma unroll
  for (int i = 0; i < 17; ++i) acc[i] = (v2f){0.f, 0.f};
  for (int k = k_lo; k <= k_hi; ++k) {
    const float2* hp = H + (int64_t)k * FIR_SPEC;
    const float2* xp = X + (int64_t)(b - k) * FIR_SPEC;
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) {
      const int i = l + 16 * k2;
      acc[k2] = fir_cmac(ld2(&hp[i]), ld2(&xp[i]), acc[k2]);
      acc[8 + k2] = fir_cmac(ld2(&hp[256 - i]), ld2(&xp[256 - i]), acc[8 + k2]);
    }
    acc[16] = fir_cmac(ld2(&hp[128]), ld2(&xp[128]), acc[16]);
  }

  // Y -> Z, the 256-point spectrum of y[2m] + i y[2m + 1] (twice it: the halves are left to the final scale):
  //   E = Y[k] + conj Y[256 - k],  O = (Y[k] - conj Y[256 - k]) conj(W^k),  Z[k] = E + i O,  Z[256 - k] = conj E + i conj O
  v2f z[16], zb[8];
#pragma unroll
  for (int k2 = 0; k2 < 8; ++k2) {
    const v2f yk = acc[k2], ym = conj(acc[8 + k2]);
    const v2f E = yk + ym, O = cmul(yk - ym, conj(ld2(&tw[l + 16 * k2])));
    z[k2] = E + (v2f){-O.y, O.x};
    zb[k2] = conj(E) + (v2f){O.y, O.x};
  }
  // Z[l + 16 k2], k2 >= 8, is Z[256 - k] of lane (16 - l) % 16's k2' = 15 - k2; lane 0 holds its own, and Z[128] = 2 conj Y[128]
  const int partner = (lane & 48) | ((16 - l) & 15);
#pragma unroll
  for (int k2 = 8; k2 < 16; ++k2) {
    v2f v;
    v.x = __shfl(zb[15 - k2].x, partner, 64);
    v.y = __shfl(zb[15 - k2].y, partner, 64);
    if (l == 0) v = (k2 == 8) ? 2.0f * conj(acc[16]) : zb[(16 - k2) & 7];
    z[k2] = v;
  }
  // inverse = conj(forward(conj Z)) / 256
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = conj(z[i]);
  fft256_g16(z, xch[4 * wave + g], t256, l);

  if (!active) return;
  float* const y = out + jb.out_off;
  const int base = FIR_P * b - jb.d;  // out index of the block's first sample
#pragma unroll
  for (int k2 = 8; k2 < 16; ++k2) {  // packed point l + 16 k2 >= 128: the last 256 samples of the 512
    const int i = base + 2 * (l + 16 * k2) - FIR_P;
    if (i >= 0 && i < jb.n) y[i] = z[k2].x * (1.0f / 512.0f);
    if (i + 1 >= 0 && i + 1 < jb.n) y[i + 1] = -z[k2].y * (1.0f / 512.0f);
  }
}

}  // namespace

// workspace: the J jobs (256-aligned) | the spectra, FIR_SPEC float2 each
extern "C" size_t sk_fir_workspace_bytes(const int32_t* nsamp_host, const int32_t* ntaps_host, const int32_t* delay_host, int J) {
  if (J < 1 || J > FIR_MAX_JOBS || !nsamp_host || !ntaps_host || !delay_host) return 0;
  FirPlan plan;
  int bad = 0;
  if (fir_plan(nsamp_host, ntaps_host, delay_host, J, &plan, &bad, nullptr) != 0) return 0;
  return fir_jobs_bytes(J) + (size_t)plan.spectra * FIR_SPEC * sizeof(float2);
}

extern "C" int sk_fir_convolve(const void* in, int pcm16, const int64_t* in_offs_host, const int32_t* nsamp_host, const float* rir,
                               const int64_t* rir_offs_host, const int32_t* ntaps_host, const int32_t* delay_host, int J, void* ws,
                               float* out, const int64_t* out_offs_host, sk_stream_t stream) {
  SK_CHECK_ARG(J >= 1 && J <= FIR_MAX_JOBS, "sk_fir_convolve: J = %d jobs outside 1..%d", J, FIR_MAX_JOBS);
  SK_CHECK_ARG(in_offs_host && nsamp_host && rir_offs_host && ntaps_host && delay_host && out_offs_host,
               "sk_fir_convolve: the job arrays (host) are required");
  FirPlan plan;
  int bad = 0;
  const int why = fir_plan(nsamp_host, ntaps_host, delay_host, J, &plan, &bad, nullptr);
  SK_CHECK_ARG(why == 0, "sk_fir_convolve: job %d (nsamp %d, ntaps %d, delay %d): %s", bad, nsamp_host[bad], ntaps_host[bad],
               delay_host[bad], kFirWhy[why]);
  for (int j = 0; j < J; ++j)
    SK_CHECK_ARG(in_offs_host[j] >= 0 && rir_offs_host[j] >= 0 && out_offs_host[j] >= 0, "sk_fir_convolve: job %d has a negative offset", j);
  SK_CHECK_ARG(in && rir && ws && out, "sk_fir_convolve: null pointer");
  std::vector<FirJob> jobs((size_t)J);
  fir_plan(nsamp_host, ntaps_host, delay_host, J, &plan, &bad, jobs.data());
  for (int j = 0; j < J; ++j) {
    jobs[j].in_off = in_offs_host[j];
    jobs[j].rir_off = rir_offs_host[j];
    jobs[j].out_off = out_offs_host[j];
  }
  const hipStream_t st = (hipStream_t)stream;
  FirJob* const d_jobs = (FirJob*)ws;
  float2* const spec = (float2*)((char*)ws + fir_jobs_bytes(J));
  // (a copy from pageable memory is staged before the call returns, as for sk_stoi's arrays)
  SK_CHECK_HIP(hipMemcpyAsync(d_jobs, jobs.data(), (size_t)J * sizeof(FirJob), hipMemcpyHostToDevice, st));
  const unsigned g1 = (unsigned)sk_cdiv(plan.transforms, 16), g2 = (unsigned)sk_cdiv(plan.blocks, 16);
  if (pcm16)
    hipLaunchKernelGGL(fir_spectra_kernel<true>, dim3(g1), dim3(256), 0, st, in, rir, d_jobs, J, (int)plan.transforms, spec);
  else
    hipLaunchKernelGGL(fir_spectra_kernel<false>, dim3(g1), dim3(256), 0, st, in, rir, d_jobs, J, (int)plan.transforms, spec);
  SK_CHECK_LAUNCH("fir_spectra_kernel");
  hipLaunchKernelGGL(fir_output_kernel, dim3(g2), dim3(256), 0, st, d_jobs, J, (int)plan.blocks, spec, out);
  SK_CHECK_LAUNCH("fir_output_kernel");
  return SK_OK;
}
