// stoi.hip -- STOI / ESTOI scoring for gfx950 (include/sepkern.h "STOI"; the definition is sepkern/stoi.py's).
// stoi_env_kernel transforms with the 256-point FFT and the tables of fft512.h; its real-FFT split is stft_kernel's (stft.hip).
#include "fft512.h"

namespace {

// Signals at 10 kHz, frames of 256 samples at hop 128, w[i] = 0.5 (1 - cos(2 pi (i + 1) / 257)).  Three kernels, nothing
// reduced across workgroups, no atomics:
//   stoi_keep_kernel   one workgroup per reference: fp64 energy of every windowed frame (a wave per frame, lanes in a fixed
//                      order, a fixed butterfly), their maximum, the 40 dB rule, and an exclusive scan of the keep flags into
//                      the list of kept frame indices;
//   stoi_env_kernel    the S + 1 signals that share a reference's keep list: a 16-lane group per frame t of the REBUILT signal,
//                      whose sample 128 t + r is formed on the way in from the (at most two) kept windowed frames that cover
//                      it, windowed again, packed with 256 zeros into the 256-point complex FFT; |X|^2, 15 band sums in
//                      ascending bin order, sqrt -> env[signal][band][t] (fp32);
//   stoi_score_kernel  one workgroup per (utterance, estimate, reference): tiles of 64 segments of 30 frames staged in LDS, a
//                      16-lane group per segment (lane = band), fp64 accumulators, segments in a fixed order per group and the
//                      16 group sums added in a fixed order.
// A score's operations depend on its own utterance alone, so its bits depend neither on the batch nor on the run.
constexpr int SN = 256;         // STOI frame
constexpr int SBANDS = 15;
constexpr int SSEG = 30;        // frames per segment
constexpr int STILE = 64;       // segments per LDS tile of the score kernel
constexpr int SLD = 97;         // frames per band row of a tile (64 + 29 used), odd: the 15 rows start on different banks
constexpr int kStoiMaxLen = 1 << 24;
constexpr double kStoiEps = 2.220446049250313e-16;
constexpr double kStoiShort = 1e-5;
__constant__ int g_stoi_lo[SBANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};  // band b: bins [lo[b], lo[b+1])

__host__ __device__ inline int stoi_num_frames(int n) { return n > SN ? (n - SN + HOP - 1) / HOP : 0; }  // range(0, n - 256, 128)
__device__ __forceinline__ double stoi_window(int i) { return 0.5 * (1.0 - cos(6.283185307179586476925 * (double)(i + 1) / 257.0)); }

__device__ __forceinline__ double group_sum16(double v) {  // over the 16 lanes of a group, a fixed butterfly; every lane gets the sum
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// grid (U * S); signal sig = u * S + j: energy / kept rows of Fm entries each.
__global__ __launch_bounds__(256) void stoi_keep_kernel(const float* __restrict__ ref, const int64_t* __restrict__ offs,
                                                        const int32_t* __restrict__ lens, int S, int Fm, double* energy,
                                                        int32_t* __restrict__ kept, int32_t* __restrict__ nkept) {
  __shared__ double w[SN];
  __shared__ double wmax[4];
  __shared__ int wcnt[4];
  const int sig = blockIdx.x, u = sig / S, j = sig - u * S;
  const int n = lens[u];
  const int F = stoi_num_frames(n);
  const float* x = ref + offs[u] + (int64_t)j * n;
  double* en = energy + (int64_t)sig * Fm;
  int32_t* kp = kept + (int64_t)sig * Fm;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  w[tid] = stoi_window(tid);
  __syncthreads();
  double mx = 0.0;
  for (int f = wave; f < F; f += 4) {  // samples 128 f .. 128 f + 255 <= n - 2
    const float* p = x + (int64_t)f * HOP;
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double v = w[lane + 64 * q] * (double)p[lane + 64 * q];
      acc = fma(v, v, acc);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) en[f] = acc;
    mx = fmax(mx, acc);
  }
  if (lane == 0) wmax[wave] = mx;
  __syncthreads();  // also: every en[f] of this block is written
  mx = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
  // keep iff 20 log10(|frame| + EPS) > 20 log10(max |frame| + EPS) - 40, and nothing of an all-zero reference
  const double thr = 20.0 * log10(sqrt(mx) + kStoiEps) - 40.0;
  int base = 0;
  for (int c0 = 0; c0 < F; c0 += 256) {  // block-uniform
    const int f = c0 + tid;
    const bool flag = f < F && mx > 0.0 && 20.0 * log10(sqrt(en[f]) + kStoiEps) > thr;
    const unsigned long long b = __ballot(flag);
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[wave] = __popcll(b);
    __syncthreads();
    int pos = base + before;
    for (int q = 0; q < 4; ++q) {
      if (q < wave) pos += wcnt[q];
      base += wcnt[q];
    }
    if (flag) kp[pos] = f;  // pos < F <= Fm
    __syncthreads();
  }
  if (tid == 0) nkept[sig] = base;
}

// grid (U * S * (S + 1), tiles of FPB frames); signal index = (u * S + j) * (S + 1) + q: q = 0 reference j, q >= 1 estimate q - 1,
// all under reference j's keep list.  env row of (signal, band): Fm floats.  Two workgroups per SIMD set: at four (128 VGPRs) the
// 64-bit addresses of the three frames a sample is formed from do not fit and the kernel goes to scratch.
__global__ __launch_bounds__(256, 2) void stoi_env_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                          const int64_t* __restrict__ offs, const int32_t* __restrict__ lens, int S,
                                                          int Fm, const int32_t* __restrict__ kept,
                                                          const int32_t* __restrict__ nkept, float* __restrict__ env) {
  __shared__ __attribute__((aligned(16))) float win[SN];
  __shared__ float2 tw[NFFT];
  __shared__ float2 t256[256];
  __shared__ float xch[16][16 * XLD];  // per group: the FFT's transpose plane, then the frame's 257 powers (272 floats)

  const int sg = blockIdx.x;
  const int rj = sg / (S + 1), q = sg - rj * (S + 1);  // rj = u * S + j
  const int u = rj / S, j = rj - u * S;
  const int T = max(nkept[rj] - 1, 0);  // frames of the rebuilt signal
  const int t0 = blockIdx.y * FPB;
  if (t0 >= T) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lens[u];
  const float* x = (q == 0 ? ref + (int64_t)j * n : est + (int64_t)(q - 1) * n) + offs[u];
  const int32_t* kp = kept + (int64_t)rj * Fm;

  for (int i = tid; i < NFFT; i += 256) tw[i] = g_tw512[i];
  win[tid] = (float)stoi_window(tid);
  t256[tid] = g_tw512[(2 * (tid & 15) * (tid >> 4)) & 511];
  __syncthreads();

  const int l = lane & 15, g = lane >> 4;
  const int fr = 4 * wave + g;
  const int t = t0 + fr;
  const bool active = t < T;
  const int partner = (lane & 48) | ((16 - l) & 15);
  // rebuilt sample 128 t + r = w[r] x[128 k_t + r] + (r < 128 ? w[r + 128] x[128 k_{t-1} + 128 + r] (t > 0)
  //                                                          : w[r - 128] x[128 k_{t+1} + r - 128] (t + 1 <= T: always there))
  const float* cur = x;
  const float* prv = nullptr;
  const float* nxt = x;
  if (active) {  // every kept index is < F, so 128 k + 255 <= n - 2
    cur = x + (int64_t)kp[t] * HOP;
    nxt = x + (int64_t)kp[t + 1] * HOP;
    if (t > 0) prv = x + (int64_t)kp[t - 1] * HOP;
  }
  v2f z[16];
#pragma unroll
  for (int n1 = 0; n1 < 16; ++n1) {  // packed point 16 n1 + l <-> samples r, r + 1, r = 32 n1 + 2 l; points 128.. are the zero padding
    z[n1] = (v2f){0.f, 0.f};
    if (n1 < 8 && active) {
      const int r = 32 * n1 + 2 * l;
      const v2f w = *reinterpret_cast<const v2f*>(&win[r]);
      v2f s = w * (v2f){cur[r], cur[r + 1]};
      if (n1 < 4) {
        if (prv) s = *reinterpret_cast<const v2f*>(&win[r + HOP]) * (v2f){prv[r + HOP], prv[r + HOP + 1]} + s;
      } else {
        s = s + *reinterpret_cast<const v2f*>(&win[r - HOP]) * (v2f){nxt[r - HOP], nxt[r - HOP + 1]};
      }
      z[n1] = s * w;
    }
  }
  float* const pw = xch[4 * wave + g];
  fft256_g16(z, pw, t256, l);

  // real-FFT split as in stft_kernel; the 257 powers go to the group's LDS plane
  if (active) {
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) {
      v2f zc;
      zc.x = __shfl(z[15 - k2].x, partner, 64);
      zc.y = __shfl(z[15 - k2].y, partner, 64);
      if (l == 0) zc = z[(16 - k2) & 15];
      const v2f zk = z[k2], cz = conj(zc);
      const int k = l + 16 * k2;
      const v2f A = 0.5f * (zk + cz), Bt = cmul(ld2(&tw[k]), 0.5f * mul_mi(zk - cz));
      const v2f xa = A + Bt, xb = conj(A - Bt);  // X[k], X[256 - k]
      pw[k] = xa.x * xa.x + xa.y * xa.y;
      pw[256 - k] = xb.x * xb.x + xb.y * xb.y;
    }
    if (l == 0) {  // bin 128 pairs with itself
      const v2f zk = z[8], cz = conj(zk);
      const v2f xa = 0.5f * (zk + cz) + cmul(ld2(&tw[128]), 0.5f * mul_mi(zk - cz));
      pw[128] = xa.x * xa.x + xa.y * xa.y;
    }
  }
  wave_sync();
  if (active && l < SBANDS) {  // lane b: band b, bins in ascending order
    const int lo = g_stoi_lo[l], hi = g_stoi_lo[l + 1];
    float acc = 0.f;
    for (int k = lo; k < hi; ++k) acc += pw[k];
    env[((int64_t)sg * SBANDS + l) * Fm + t] = __builtin_amdgcn_sqrtf(acc);
  }
}

// grid (U * S * S): block = (u * S + k) * S + j scores estimate k against reference j.
__global__ __launch_bounds__(256) void stoi_score_kernel(int S, int Fm, const int32_t* __restrict__ nkept,
                                                         const float* __restrict__ env, double* __restrict__ out,
                                                         int32_t* __restrict__ frames) {
  __shared__ float Xs[SBANDS][SLD];
  __shared__ float Ys[SBANDS][SLD];
  __shared__ double part[2][16];
  const int blk = blockIdx.x;
  const int uk = blk / S, j = blk - uk * S;
  const int u = uk / S, k = uk - u * S;
  const int rj = u * S + j;
  const int T = max(nkept[rj] - 1, 0);
  const int tid = threadIdx.x;
  if (k == 0 && tid == 0) frames[rj] = T;
  if (T < SSEG) {  // block-uniform
    if (tid == 0) {
      out[2 * (int64_t)blk] = kStoiShort;
      out[2 * (int64_t)blk + 1] = kStoiShort;
    }
    return;
  }
  const int J = T - SSEG + 1;
  const float* ex = env + ((int64_t)rj * (S + 1)) * SBANDS * Fm;
  const float* ey = env + ((int64_t)rj * (S + 1) + 1 + k) * SBANDS * Fm;
  const int b = tid & 15, grp = tid >> 4;
  const bool live = b < SBANDS;
  const int br = live ? b : 0;
  const double clipk = 1.0 + 5.623413251903491;  // 1 + 10^(15/20)
  double dsum = 0.0, esum = 0.0;
  for (int m0 = 0; m0 < J; m0 += STILE) {  // block-uniform
    const int nt = min(STILE + SSEG - 1, T - m0);  // frames of this tile
    __syncthreads();
    for (int i = tid; i < SBANDS * (STILE + SSEG - 1); i += 256) {
      const int bb = i / (STILE + SSEG - 1), tt = i - bb * (STILE + SSEG - 1);
      Xs[bb][tt] = tt < nt ? ex[(int64_t)bb * Fm + m0 + tt] : 0.f;
      Ys[bb][tt] = tt < nt ? ey[(int64_t)bb * Fm + m0 + tt] : 0.f;
    }
    __syncthreads();
    for (int ms = grp; ms < STILE && m0 + ms < J; ms += 16) {  // uniform over the 16-lane group
      const float* xr = &Xs[br][ms];
      const float* yr = &Ys[br][ms];
      double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0;
      for (int t = 0; t < SSEG; ++t) {
        const double xv = live ? (double)xr[t] : 0.0, yv = live ? (double)yr[t] : 0.0;
        sx += xv;
        sy += yv;
        sxx = fma(xv, xv, sxx);
        syy = fma(yv, yv, syy);
      }
      const double c = sqrt(sxx) / (sqrt(syy) + kStoiEps);
      const double mx = sx / SSEG, my = sy / SSEG;
      double syp = 0.0, dxx = 0.0, dyy = 0.0;
      for (int t = 0; t < SSEG; ++t) {
        const double xv = live ? (double)xr[t] : 0.0, yv = live ? (double)yr[t] : 0.0;
        syp += fmin(c * yv, xv * clipk);
        const double dx = xv - mx, dy = yv - my;
        dxx = fma(dx, dx, dxx);
        dyy = fma(dy, dy, dyy);
      }
      const double myp = syp / SSEG;
      double dpp = 0.0, dxp = 0.0;
      for (int t = 0; t < SSEG; ++t) {
        const double xv = live ? (double)xr[t] : 0.0, yv = live ? (double)yr[t] : 0.0;
        const double dp = fmin(c * yv, xv * clipk) - myp;
        dpp = fma(dp, dp, dpp);
        dxp = fma(xv - mx, dp, dxp);
      }
      const double ix = 1.0 / (sqrt(dxx) + kStoiEps), iy = 1.0 / (sqrt(dyy) + kStoiEps);
      const double sb = live ? dxp * ix / (sqrt(dpp) + kStoiEps) : 0.0;
      dsum += group_sum16(sb);  // STOI of this segment: the 15 bands' correlations
      // ESTOI: the row-normalised values of column t over the 15 bands, normalised again, correlated
      double eseg = 0.0;
      for (int t = 0; t < SSEG; ++t) {
        const double xn = live ? ((double)xr[t] - mx) * ix : 0.0, yn = live ? ((double)yr[t] - my) * iy : 0.0;
        const double cmx = group_sum16(xn) / SBANDS, cmy = group_sum16(yn) / SBANDS;
        const double dx = live ? xn - cmx : 0.0, dy = live ? yn - cmy : 0.0;
        const double cxx = group_sum16(dx * dx), cyy = group_sum16(dy * dy), cxy = group_sum16(dx * dy);
        eseg += cxy / ((sqrt(cxx) + kStoiEps) * (sqrt(cyy) + kStoiEps));
      }
      esum += eseg;
    }
  }
  if (b == 0) {
    part[0][grp] = dsum;
    part[1][grp] = esum;
  }
  __syncthreads();
  if (tid == 0) {
    double d = 0.0, e = 0.0;
    for (int i = 0; i < 16; ++i) {
      d += part[0][i];
      e += part[1][i];
    }
    out[2 * (int64_t)blk] = d / ((double)SBANDS * J);
    out[2 * (int64_t)blk + 1] = e / ((double)SSEG * J);
  }
}

// workspace (each part 256-aligned): offs (U int64) | lens (U int32) | nkept (U*S int32) | kept (U*S*Fm int32) |
// energy (U*S*Fm fp64) | env (U*S*(S+1)*15*Fm fp32)
struct StoiWs {
  int64_t* offs;
  int32_t* lens;
  int32_t* nkept;
  int32_t* kept;
  double* energy;
  float* env;
  size_t bytes;
};

StoiWs stoi_carve(void* base, int U, int S, int Fm) {
  StoiWs w;
  size_t o = 0;
  char* b = (char*)base;
  const size_t sigs = (size_t)U * S;
  w.offs = (int64_t*)(b + o); o = sk_align(o + (size_t)U * 8, 256);
  w.lens = (int32_t*)(b + o); o = sk_align(o + (size_t)U * 4, 256);
  w.nkept = (int32_t*)(b + o); o = sk_align(o + sigs * 4, 256);
  w.kept = (int32_t*)(b + o); o = sk_align(o + sigs * Fm * 4, 256);
  w.energy = (double*)(b + o); o = sk_align(o + sigs * Fm * 8, 256);
  w.env = (float*)(b + o); o = sk_align(o + sigs * (S + 1) * SBANDS * Fm * 4, 256);
  w.bytes = o;
  return w;
}

bool stoi_sizes_ok(int U, int S, int max_len) {
  return U >= 1 && U <= (1 << 20) && S >= 1 && S <= SK_MAXS && max_len >= 1 && max_len <= kStoiMaxLen;
}

}  // namespace

extern "C" size_t sk_stoi_workspace_bytes(int U, int S, int max_len) {
  if (!stoi_sizes_ok(U, S, max_len)) return 0;
  return stoi_carve(nullptr, U, S, std::max(1, stoi_num_frames(max_len))).bytes;
}

extern "C" int sk_stoi(const float* ref, const float* est, const int64_t* offs_host, const int32_t* lens_host, int U, int S, void* ws,
                       double* out, int32_t* frames, sk_stream_t stream) {
  SK_CHECK_ARG(U >= 1 && U <= (1 << 20), "sk_stoi: U = %d, need 1..%d", U, 1 << 20);
  SK_CHECK_ARG(S >= 1 && S <= SK_MAXS, "sk_stoi: S = %d, need 1..%d", S, SK_MAXS);
  SK_CHECK_ARG(offs_host && lens_host, "sk_stoi: offs_host and lens_host are required");
  int max_len = 0;
  for (int u = 0; u < U; ++u) {
    SK_CHECK_ARG(lens_host[u] >= 1 && lens_host[u] <= kStoiMaxLen, "sk_stoi: utterance %d has length %d, need 1..%d", u,
                 lens_host[u], kStoiMaxLen);
    SK_CHECK_ARG(offs_host[u] >= 0, "sk_stoi: utterance %d has offset %lld", u, (long long)offs_host[u]);
    max_len = std::max(max_len, (int)lens_host[u]);
  }
  SK_CHECK_ARG(ref && est && ws && out && frames, "sk_stoi: null pointer");
  const int Fm = std::max(1, stoi_num_frames(max_len));
  const StoiWs w = stoi_carve(ws, U, S, Fm);
  hipStream_t st = (hipStream_t)stream;
  SK_CHECK_HIP(hipMemcpyAsync(w.offs, offs_host, (size_t)U * 8, hipMemcpyHostToDevice, st));
  SK_CHECK_HIP(hipMemcpyAsync(w.lens, lens_host, (size_t)U * 4, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(stoi_keep_kernel, dim3((unsigned)(U * S)), dim3(256), 0, st, ref, w.offs, w.lens, S, Fm, w.energy, w.kept,
                     w.nkept);
  SK_CHECK_LAUNCH("stoi_keep_kernel");
  hipLaunchKernelGGL(stoi_env_kernel, dim3((unsigned)(U * S * (S + 1)), (unsigned)sk_cdiv(Fm, FPB)), dim3(256), 0, st, ref, est,
                     w.offs, w.lens, S, Fm, w.kept, w.nkept, w.env);
  SK_CHECK_LAUNCH("stoi_env_kernel");
  hipLaunchKernelGGL(stoi_score_kernel, dim3((unsigned)(U * S * S)), dim3(256), 0, st, S, Fm, w.nkept, w.env, out, frames);
  SK_CHECK_LAUNCH("stoi_score_kernel");
  return SK_OK;
}
