// dpcl.hip -- deep clustering on packed rows: the training loss (sk_dpcl_fwd / sk_dpcl_bwd) and the k-means that turns the
// embeddings into masks (sk_dpcl_kmeans).
//
// No counterpart in the reference, whose only objective is the magnitude PIT-MSE; sepkern/dpcl.py states the definition
// (Hershey et al. 2016; the low-rank objective of Isik et al. 2016; the unit-norm sigmoid embedding and the magnitude-ratio
// weights of Wang et al. 2018) and restates the arithmetic in numpy fp64.
//
// The network's rows z (R, ld >= F*D): embedding dimension d of bin f is column d*F + f -- D planes of F columns, so plane d of
// a row is contiguous and a wave reads 64 consecutive points of one plane per load.  A point is (row, bin); utterance j has
// lens[j] * F points, numbered t * F + f.  Every kernel is partitioned by (utterance, chunk of CH frames of THAT utterance): chunk
// boundaries depend on the utterance's own length only, every sum has one fixed order, nothing is atomic -- two launches agree
// bit for bit, and an utterance's numbers do not depend on the batch around it.
//
//   dpcl_gram_kernel      (utterance, chunk): the points of the chunk in tiles of 64, four waves taking every fourth tile.  A lane
//                         owns one point: it loads the D planes' values into its own LDS column, normalises, scales by sqrt(w)
//                         and appends sqrt(w) * onehot(label) in the LAST S of the P = 16 NT columns (columns in between are
//                         zero).  The wave then forms the tile's Gram matrix U^T U with the exact-fp32 MFMA (16x16x4: the A and
//                         the B fragment of a column tile are the same LDS word, one read serves both).  Every MFMA starts from
//                         zero and sums FOUR points; its result is added to fp64 accumulators on the vector pipe.  (A running fp32
//                         accumulator rounds once per point: over the 64 points of a tile that random walk alone is 2e-7 of an
//                         entry, and the loss |A|^2 - 2 |Bm|^2 + |C|^2 amplifies an entry's error several times.)  The Gram
//                         matrix holds A = V^T W V, Bm = V^T W Y and C = Y^T W Y at once.  Points past the chunk's end are
//                         read from its last point and given weight zero: no branch around the MFMA.  The four waves' sums are
//                         added in wave order and stored as one partial per (utterance, chunk).
//                         Loss: label = dominant source, weight = mix (mr) or [mix > thr] (vad); the normaliser 1 / sum w is the
//                         trace of C and is applied after the chunks are added.  k-means: label = nearest centroid, weight =
//                         mix on active points; only the tiles that hold Bm and C (the weighted sums and the weights) are formed.
//   dpcl_loss_kernel      per utterance: the chunks' partials added in ascending order in fp64, L_j, A and Bm for the backward
//   dpcl_out_kernel       the batch output [loss, count, sum_j L_j], utterances added in ascending order in fp64
//   dpcl_bwd_kernel       one point per lane; A and Bm of the utterance are read at wave-uniform addresses (scalar loads, two
//                         rows of A per trip), the embedding and the gradient stay in registers (D rounded up to a multiple
//                         of 8 picks the instantiation) with a copy of the embedding in the lane's own LDS column
//   dpcl_chunkmax_kernel, dpcl_thr_kernel     max mix per utterance -> the activity threshold (vad weights, k-means)
//   dpcl_pick_kernel, dpcl_pick_finish_kernel farthest-first initialisation: two launches per centroid
//   dpcl_cent_kernel      per utterance: the chunks' weighted sums added in fp64 -> the new centroids
//   dpcl_assign_kernel    the final assignment: labels, the 0/1 mask rows, the centroids
#include "sk_common.h"

namespace {

constexpr int MAXS = SK_MAXS;
constexpr int DMAX = 40;            // embedding dimensions
constexpr int CH = 8;               // frames per chunk
constexpr int TP = 64;              // points per tile (one per lane)
constexpr int LDP = TP + 4;         // LDS column pitch: bank (c & 15) * 4 + (k & 3) for the MFMA fragment reads -- no conflicts
constexpr int AB = DMAX * DMAX + DMAX * MAXS;   // floats of [A | Bm] per utterance, zero-padded to fixed pitches (DMAX, MAXS)

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct SrcPtrs {
  const float* p[MAXS];
};

__device__ __forceinline__ double block_sum256_f64(double v, double* red /* >= 4 doubles of LDS */) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// the dominant source of a point: the first maximum
__device__ __forceinline__ int dominant(const SrcPtrs& src, int S, int64_t at) {
  int y = 0;
  float best = src.p[0][at];
#pragma unroll
  for (int s = 1; s < MAXS; ++s)
    if (s < S) {
      const float v = src.p[s][at];
      if (v > best) {
        best = v;
        y = s;
      }
    }
  return y;
}

// The D values of a point into the LDS column `col` (pitch `pitch`); returns 1 / |v| (0 for a zero vector).
__device__ __forceinline__ float load_point(const float* __restrict__ zp, int F, int D, float* col, int pitch) {
  float ss = 0.f;
#pragma unroll 4
  for (int d = 0; d < D; ++d) {
    const float v = zp[(int64_t)d * F];
    ss = fmaf(v, v, ss);
    col[d * pitch] = v;
  }
  return ss > 0.f ? 1.0f / sqrtf(ss) : 0.f;
}

constexpr int npairs(int NT, bool KM) { return KM ? NT : NT * (NT + 1) / 2; }

// ---------------------------------------------------------------------------------------------- the Gram matrix of a chunk
template <int NT, bool KM>
__global__ __launch_bounds__(256) void dpcl_gram_kernel(const float* __restrict__ z, int ld, const float* __restrict__ mix,
                                                        SrcPtrs src, const int32_t* __restrict__ offs,
                                                        const int32_t* __restrict__ lens, int F, int D, int S, int vad,
                                                        const float* __restrict__ thr, const float* __restrict__ cent,
                                                        double* __restrict__ partial, int nchmax) {
  constexpr int P = 16 * NT, NP = npairs(NT, KM);
  __shared__ float U[4 * P * LDP];
  __shared__ float cl[MAXS * DMAX];
  const int j = blockIdx.y, ch = blockIdx.x, len = lens[j], t0 = ch * CH;
  if (t0 >= len) return;  // (the whole workgroup: before any barrier)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nfr = min(CH, len - t0), npts = nfr * F, ntiles = (npts + TP - 1) / TP, niter = (ntiles + 3) / 4;
  float* __restrict__ Uw = U + wave * (P * LDP);
  float* __restrict__ col = Uw + lane;
  for (int c = D; c < P; ++c) col[c * LDP] = 0.f;  // the columns between the embedding and the one-hot block stay zero
  if (KM && tid < MAXS * DMAX) cl[tid] = cent[(int64_t)j * (MAXS * DMAX) + tid];
  const float th = (vad || KM) ? thr[j] : 0.f;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  double acc[NP][4];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[p][r] = 0.0;
  __syncthreads();
  for (int it = 0; it < niter; ++it) {
    const int q = (it * 4 + wave) * TP + lane;
    const bool valid = q < npts;
    const int qc = valid ? q : npts - 1;  // past the end: the chunk's last point, with weight zero
    const int fr = qc / F, f = qc - fr * F;
    const int64_t row = (int64_t)offs[t0 + fr] + j;
    const float m = mix[row * F + f];
    const float inv = load_point(z + row * ld + f, F, D, col, LDP);
    int y;
    float sw;
    if (KM) {
      sw = (valid && m > th) ? sqrtf(m) : 0.f;
      float dist[MAXS] = {0.f, 0.f, 0.f, 0.f};
      for (int d = 0; d < D; ++d) {
        const float vh = col[d * LDP] * inv;
#pragma unroll
        for (int k = 0; k < MAXS; ++k) {
          const float df = vh - cl[k * DMAX + d];
          dist[k] = fmaf(df, df, dist[k]);
        }
        col[d * LDP] = vh * sw;
      }
      y = 0;
      float best = dist[0];
#pragma unroll
      for (int k = 1; k < MAXS; ++k)
        if (k < S && dist[k] < best) {
          best = dist[k];
          y = k;
        }
    } else {
      y = dominant(src, S, row * F + f);
      const float w = vad ? (m > th ? 1.f : 0.f) : m;
      sw = valid ? sqrtf(w) : 0.f;
      const float sc = inv * sw;
      for (int d = 0; d < D; ++d) col[d * LDP] *= sc;
    }
#pragma unroll
    for (int s = 0; s < MAXS; ++s)
      if (s < S) col[(P - S + s) * LDP] = (y == s) ? sw : 0.f;
    __syncthreads();
    const float* __restrict__ fr0 = Uw + (lane & 15) * LDP + (lane >> 4);
#pragma unroll 2
    for (int k0 = 0; k0 < TP; k0 += 4) {
      float a[NT];
      f32x4 r[NP];
#pragma unroll
      for (int t = 0; t < NT; ++t) a[t] = fr0[t * 16 * LDP + k0];
      if (KM) {
#pragma unroll
        for (int t = 0; t < NT; ++t) r[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], a[NT - 1], zero, 0, 0, 0);
      } else {
        int p = 0;
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
          for (int tj = ti; tj < NT; ++tj, ++p) r[p] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ti], a[tj], zero, 0, 0, 0);
      }
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[p][i] += (double)r[p][i];
    }
    __syncthreads();
  }
  // the four waves' tiles added in wave order: element (row, col) of a 16 x 16 tile at row * 16 + col
  double* __restrict__ red = reinterpret_cast<double*>(U);  // 4 * NP * 256 doubles <= 4 * P * LDP floats
  static_assert(4 * NP * 256 * sizeof(double) <= 4 * P * LDP * sizeof(float), "the waves' sums must fit the tile buffer");
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[(wave * NP + p) * 256 + ((lane >> 4) * 4 + r) * 16 + (lane & 15)] = acc[p][r];
  __syncthreads();
  double* __restrict__ out = partial + ((int64_t)j * nchmax + ch) * (NP * 256);
#pragma unroll
  for (int p = 0; p < NP; ++p)
    out[p * 256 + tid] = ((red[(0 * NP + p) * 256 + tid] + red[(1 * NP + p) * 256 + tid]) + red[(2 * NP + p) * 256 + tid]) +
                         red[(3 * NP + p) * 256 + tid];
}

// ---------------------------------------------------------------------------------------------- the loss of an utterance
template <int NT>
__global__ __launch_bounds__(256) void dpcl_loss_kernel(const double* __restrict__ partial, int nchmax,
                                                        const int32_t* __restrict__ lens, int D, int S,
                                                        const float* __restrict__ thr, double* __restrict__ lj,
                                                        float* __restrict__ ab, float* __restrict__ stats) {
  constexpr int P = 16 * NT, NP = npairs(NT, false);
  __shared__ double G[P * P];
  __shared__ double red[4];
  const int j = blockIdx.x, tid = threadIdx.x, nch = (lens[j] + CH - 1) / CH;
  const double* __restrict__ pj = partial + (int64_t)j * nchmax * (NP * 256);
  int p = 0;
#pragma unroll
  for (int ti = 0; ti < NT; ++ti)
#pragma unroll
    for (int tj = ti; tj < NT; ++tj, ++p) {
      double s = 0.0;
      for (int c = 0; c < nch; ++c) s += pj[(int64_t)c * (NP * 256) + p * 256 + tid];
      const int a = ti * 16 + (tid >> 4), b = tj * 16 + (tid & 15);
      G[a * P + b] = s;
      if (ti != tj) G[b * P + a] = s;
    }
  __syncthreads();
  double tr = 0.0;
  for (int s = 0; s < S; ++s) tr += G[(P - S + s) * P + (P - S + s)];
  const double sc = tr > 0.0 ? 1.0 / tr : 0.0;  // 1 / sum of the weights: an all-zero mixture gives loss 0, gradient 0
  double part = 0.0;
  for (int e = tid; e < D * D; e += 256) {
    const int a = e / D, b = e - a * D;
    const double v = G[a * P + b] * sc;
    part += v * v;
  }
  for (int e = tid; e < D * S; e += 256) {
    const int a = e / S, s = e - a * S;
    const double v = G[a * P + P - S + s] * sc;
    part -= 2.0 * v * v;
  }
  if (tid < S) {
    const double v = G[(P - S + tid) * P + (P - S + tid)] * sc;
    part += v * v;
  }
  const double L = block_sum256_f64(part, red);
  if (tid == 0) {
    lj[j] = L;
    stats[2 * j] = (float)sc;
    stats[2 * j + 1] = thr ? thr[j] : 0.f;
  }
  float* __restrict__ abj = ab + (int64_t)j * AB;
  for (int e = tid; e < DMAX * DMAX; e += 256) {
    const int a = e / DMAX, b = e - a * DMAX;
    abj[e] = (a < D && b < D) ? (float)(G[a * P + b] * sc) : 0.f;
  }
  if (tid < DMAX * MAXS) {
    const int a = tid / MAXS, s = tid - a * MAXS;
    abj[DMAX * DMAX + tid] = (a < D && s < S) ? (float)(G[a * P + P - S + s] * sc) : 0.f;
  }
}

__global__ void dpcl_out_kernel(const double* __restrict__ lj, int B, const float* __restrict__ count_dev,
                                float* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = 0.0;
  for (int j = 0; j < B; ++j) s += lj[j];
  const double count = count_dev ? (double)count_dev[0] : (double)B;
  out[0] = (float)(s / count);
  out[1] = (float)count;
  out[2] = (float)s;
}

// ---------------------------------------------------------------------------------------------- the gradient
template <int DB>
__global__ __launch_bounds__(256) void dpcl_bwd_kernel(const float* __restrict__ z, int ld, const float* __restrict__ mix,
                                                       SrcPtrs src, const int32_t* __restrict__ offs,
                                                       const int32_t* __restrict__ lens, int F, int D, int S, int vad,
                                                       const float* __restrict__ ab, const float* __restrict__ stats,
                                                       const float* __restrict__ out, const float* __restrict__ gscale,
                                                       float* __restrict__ dz) {
  __shared__ float V[DB * 256];
  const int j = blockIdx.y;
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= (int64_t)lens[j] * F) return;
  const int t = (int)(q / F), f = (int)(q - (int64_t)t * F);
  const int64_t row = (int64_t)offs[t] + j;
  const float m = mix[row * F + f];
  const int y = dominant(src, S, row * F + f);
  const float sc = stats[2 * j], th = stats[2 * j + 1];
  const float w = vad ? (m > th ? sc : 0.f) : m * sc;
  const float* __restrict__ zp = z + row * ld + f;
  float* __restrict__ dp = dz + row * ld + f;
  float* col = V + threadIdx.x;  // the lane's own column: u_b at a loop-dependent b without indexing registers
  float u[DB], g[DB];
  float ss = 0.f;
#pragma unroll
  for (int d = 0; d < DB; ++d) {
    u[d] = d < D ? zp[(int64_t)d * F] : 0.f;
    ss = fmaf(u[d], u[d], ss);
  }
  const float inv = ss > 0.f ? 1.0f / sqrtf(ss) : 0.f;
#pragma unroll
  for (int d = 0; d < DB; ++d) {
    u[d] *= inv;
    col[d * 256] = u[d];
    g[d] = 0.f;
  }
  // A and Bm at wave-uniform addresses (the utterance is the workgroup's): two rows of A per trip live in scalar registers.
  // A is symmetric bit for bit, so row b serves as column b; g[a] adds its products with b ascending.
  const float* __restrict__ Aj = ab + (int64_t)j * AB;
  const float* __restrict__ Bj = Aj + DMAX * DMAX;
#pragma unroll 1
  for (int b = 0; b < DB; b += 2) {
    const float u0 = col[b * 256], u1 = col[(b + 1) * 256];
    const float* __restrict__ r = Aj + b * DMAX;
#pragma unroll
    for (int a = 0; a < DB; ++a) g[a] = fmaf(r[DMAX + a], u1, fmaf(r[a], u0, g[a]));
  }
  float dot = 0.f;
#pragma unroll
  for (int a = 0; a < DB; ++a) {
    const float b0 = Bj[a * MAXS], b1 = Bj[a * MAXS + 1], b2 = Bj[a * MAXS + 2], b3 = Bj[a * MAXS + 3];
    g[a] -= (y == 0 ? b0 : y == 1 ? b1 : y == 2 ? b2 : b3);
    dot = fmaf(u[a], g[a], dot);
  }
  const float fac = 4.0f * w * inv * (gscale[0] / out[1]);
#pragma unroll
  for (int a = 0; a < DB; ++a)
    if (a < D) dp[(int64_t)a * F] = fac * (g[a] - u[a] * dot);
}

// ---------------------------------------------------------------------------------------------- the activity threshold
__global__ __launch_bounds__(256) void dpcl_chunkmax_kernel(const float* __restrict__ mix, const int32_t* __restrict__ offs,
                                                            const int32_t* __restrict__ lens, int F,
                                                            float* __restrict__ cmax, int nchmax) {
  __shared__ float red[4];
  const int j = blockIdx.y, ch = blockIdx.x, len = lens[j], t0 = ch * CH;
  if (t0 >= len) return;
  const int npts = min(CH, len - t0) * F;
  float mx = 0.f;  // (magnitudes: nothing below zero counts)
  for (int q = threadIdx.x; q < npts; q += 256) {
    const int fr = q / F, f = q - fr * F;
    mx = fmaxf(mx, mix[((int64_t)offs[t0 + fr] + j) * F + f]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) cmax[(int64_t)j * nchmax + ch] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ void dpcl_thr_kernel(const float* __restrict__ cmax, int nchmax, const int32_t* __restrict__ lens, int B, float ratio,
                                float* __restrict__ thr) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= B) return;
  const int nch = (lens[j] + CH - 1) / CH;
  float mx = 0.f;
  for (int c = 0; c < nch; ++c) mx = fmaxf(mx, cmax[(int64_t)j * nchmax + c]);
  thr[j] = ratio * mx;  // one fp32 product, as the definition forms it
}

// The centroid state (B, MAXS, DMAX), fixed pitches: the caller's (B, S, D) centroids, or zeros before the initialisation.
__global__ __launch_bounds__(256) void dpcl_cent_in_kernel(const float* __restrict__ in, int D, int S, float* __restrict__ cent) {
  const int j = blockIdx.x, tid = threadIdx.x;
  if (tid >= MAXS * DMAX) return;
  const int k = tid / DMAX, d = tid - k * DMAX;
  cent[(int64_t)j * (MAXS * DMAX) + tid] = (in && k < S && d < D) ? in[((int64_t)j * S + k) * D + d] : 0.f;
}

// ---------------------------------------------------------------------------------------------- farthest-first initialisation
// The chunk's best active point for centroid k: the largest mix (k == 0) or the largest least squared distance to the centroids
// before k; ties to the lowest point index.  Also the number of active points.
__global__ __launch_bounds__(256) void dpcl_pick_kernel(const float* __restrict__ z, int ld, const float* __restrict__ mix,
                                                        const int32_t* __restrict__ offs, const int32_t* __restrict__ lens,
                                                        int F, int D, int k, const float* __restrict__ thr,
                                                        const float* __restrict__ cent, float* __restrict__ pval,
                                                        int32_t* __restrict__ pidx, int32_t* __restrict__ pcnt, int nchmax) {
  __shared__ float V[DMAX * 256];
  __shared__ float cl[MAXS * DMAX];
  __shared__ float rv[4];
  __shared__ int ri[4], rc[4];
  const int j = blockIdx.y, ch = blockIdx.x, len = lens[j], t0 = ch * CH;
  if (t0 >= len) return;
  const int tid = threadIdx.x, npts = min(CH, len - t0) * F;
  if (tid < MAXS * DMAX) cl[tid] = cent[(int64_t)j * (MAXS * DMAX) + tid];
  __syncthreads();
  const float th = thr[j];
  float* col = V + tid;
  float best = -1.f;
  int bi = 0x7fffffff, cnt = 0;
  for (int q = tid; q < npts; q += 256) {
    const int fr = q / F, f = q - fr * F;
    const int64_t row = (int64_t)offs[t0 + fr] + j;
    const float m = mix[row * F + f];
    if (!(m > th)) continue;
    ++cnt;
    float val = m;
    if (k > 0) {
      const float inv = load_point(z + row * ld + f, F, D, col, 256);
      val = 3.4e38f;
      for (int c = 0; c < k; ++c) {
        float dist = 0.f;
        for (int d = 0; d < D; ++d) {
          const float df = col[d * 256] * inv - cl[c * DMAX + d];
          dist = fmaf(df, df, dist);
        }
        val = fminf(val, dist);
      }
    }
    if (val > best) {  // (q ascends: the first of equal values stays)
      best = val;
      bi = (t0 + fr) * F + f;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    cnt += __shfl_xor(cnt, o, 64);
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
  if ((tid & 63) == 0) {
    rv[tid >> 6] = best;
    ri[tid >> 6] = bi;
    rc[tid >> 6] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) {
      if (rv[w] > best || (rv[w] == best && ri[w] < bi)) {
        best = rv[w];
        bi = ri[w];
      }
      cnt += rc[w];
    }
    const int64_t at = (int64_t)j * nchmax + ch;
    pval[at] = best;
    pidx[at] = bi;
    pcnt[at] = cnt;
  }
}

// One wave per utterance: the best chunk (ascending: the first of equal values), the point's unit vector into centroid k;
// with at most k active points centroid k copies centroid 0 (zeros when there is no active point at all).
__global__ __launch_bounds__(64) void dpcl_pick_finish_kernel(const float* __restrict__ z, int ld, const int32_t* __restrict__ offs,
                                                              const int32_t* __restrict__ lens, int F, int D, int k,
                                                              const float* __restrict__ pval, const int32_t* __restrict__ pidx,
                                                              const int32_t* __restrict__ pcnt, int nchmax,
                                                              float* __restrict__ cent) {
  const int j = blockIdx.x, lane = threadIdx.x, nch = (lens[j] + CH - 1) / CH;
  float best = -1.f;
  int bi = 0, nact = 0;
  for (int c = 0; c < nch; ++c) {
    const int64_t at = (int64_t)j * nchmax + c;
    nact += pcnt[at];
    if (pval[at] > best) {
      best = pval[at];
      bi = pidx[at];
    }
  }
  float* __restrict__ cj = cent + (int64_t)j * (MAXS * DMAX);
  if (nact <= k) {
    if (lane < D) cj[k * DMAX + lane] = k == 0 ? 0.f : cj[lane];
    return;
  }
  const int t = bi / F, f = bi - t * F;
  const float v = lane < D ? z[((int64_t)offs[t] + j) * ld + (int64_t)lane * F + f] : 0.f;
  const float ss = sk_wave_sum(v * v);
  if (lane < D) cj[k * DMAX + lane] = ss > 0.f ? v * (1.0f / sqrtf(ss)) : 0.f;
}

// ---------------------------------------------------------------------------------------------- the centroid update
template <int NT>
__global__ __launch_bounds__(256) void dpcl_cent_kernel(const double* __restrict__ partial, int nchmax,
                                                        const int32_t* __restrict__ lens, int D, int S,
                                                        float* __restrict__ cent) {
  constexpr int NP = npairs(NT, true);
  const int j = blockIdx.x, tid = threadIdx.x, nch = (lens[j] + CH - 1) / CH;
  if (tid >= D * S) return;
  const int d = tid / S, k = tid - d * S, cc = 16 - S + k;  // column P - S + k sits in the last column tile at cc
  const double* __restrict__ pj = partial + (int64_t)j * nchmax * (NP * 256);
  const int es = (d >> 4) * 256 + (d & 15) * 16 + cc, ew = (NT - 1) * 256 + cc * 16 + cc;
  double s = 0.0, w = 0.0;
  for (int c = 0; c < nch; ++c) {
    s += pj[(int64_t)c * (NP * 256) + es];
    w += pj[(int64_t)c * (NP * 256) + ew];
  }
  if (w > 0.0) cent[(int64_t)j * (MAXS * DMAX) + k * DMAX + d] = (float)(s / w);  // a cluster without active members keeps its centroid
}

// ---------------------------------------------------------------------------------------------- the final assignment
__global__ __launch_bounds__(256) void dpcl_assign_kernel(const float* __restrict__ z, int ld, const int32_t* __restrict__ offs,
                                                          const int32_t* __restrict__ lens, int F, int D, int S,
                                                          const float* __restrict__ cent, float* __restrict__ mask, int ld_mask,
                                                          int32_t* __restrict__ labels, float* __restrict__ cent_out) {
  __shared__ float V[DMAX * 256];
  __shared__ float cl[MAXS * DMAX];
  const int j = blockIdx.y, tid = threadIdx.x;
  if (tid < MAXS * DMAX) cl[tid] = cent[(int64_t)j * (MAXS * DMAX) + tid];
  __syncthreads();
  if (blockIdx.x == 0 && tid < S * D) {
    const int k = tid / D, d = tid - k * D;
    cent_out[((int64_t)j * S + k) * D + d] = cl[k * DMAX + d];
  }
  const int64_t q = (int64_t)blockIdx.x * 256 + tid;
  if (q >= (int64_t)lens[j] * F) return;
  const int t = (int)(q / F), f = (int)(q - (int64_t)t * F);
  const int64_t row = (int64_t)offs[t] + j;
  float* col = V + tid;
  const float inv = load_point(z + row * ld + f, F, D, col, 256);
  float dist[MAXS] = {0.f, 0.f, 0.f, 0.f};
  for (int d = 0; d < D; ++d) {
    const float vh = col[d * 256] * inv;
#pragma unroll
    for (int k = 0; k < MAXS; ++k) {
      const float df = vh - cl[k * DMAX + d];
      dist[k] = fmaf(df, df, dist[k]);
    }
  }
  int y = 0;
  float best = dist[0];
#pragma unroll
  for (int k = 1; k < MAXS; ++k)
    if (k < S && dist[k] < best) {
      best = dist[k];
      y = k;
    }
  labels[row * F + f] = y;
#pragma unroll
  for (int k = 0; k < MAXS; ++k)
    if (k < S) mask[row * ld_mask + (int64_t)k * F + f] = (y == k) ? 1.f : 0.f;
}

// ---------------------------------------------------------------------------------------------- host side
inline int tiles_of(int D, int S) { return (D + S + 15) / 16; }
inline int chunks_of(int T) { return (int)sk_cdiv(T, CH); }
inline bool shape_ok(int T, int B, int F, int D, int S, int smin) {
  return T >= 1 && B >= 1 && B <= 65535 && F >= 1 && D >= 1 && D <= DMAX && S >= smin && S <= MAXS &&
         (int64_t)T * F <= 0x7fffffff && sk_cdiv((int64_t)T * F, 256) <= 0x7fffffff;
}

struct Layout {  // workspace: [chunk maxima | thresholds | pick values, indices, counts | centroids | Gram partials]
  size_t cmax, thr, pval, pidx, pcnt, cent, partial, total;
};
inline Layout layout_of(int T, int B, int D, int S, bool km) {
  const size_t nc = (size_t)B * chunks_of(T);
  const int NT = tiles_of(D, S);
  Layout l;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t r = at;
    at += sk_align(bytes, 256);
    return r;
  };
  l.cmax = take(nc * sizeof(float));
  l.thr = take((size_t)B * sizeof(float));
  l.pval = take(km ? nc * sizeof(float) : 0);
  l.pidx = take(km ? nc * sizeof(int32_t) : 0);
  l.pcnt = take(km ? nc * sizeof(int32_t) : 0);
  l.cent = take(km ? (size_t)B * MAXS * DMAX * sizeof(float) : 0);
  l.partial = take(nc * npairs(NT, km) * 256 * sizeof(double));
  l.total = at + 256;
  return l;
}

int launch_threshold(const float* mix, const int32_t* offs, const int32_t* lens, int T, int B, int F, float ratio, char* ws,
                     const Layout& l, hipStream_t st) {
  const int nchmax = chunks_of(T);
  hipLaunchKernelGGL(dpcl_chunkmax_kernel, dim3(nchmax, B), dim3(256), 0, st, mix, offs, lens, F, (float*)(ws + l.cmax), nchmax);
  SK_CHECK_LAUNCH("dpcl_chunkmax_kernel");
  hipLaunchKernelGGL(dpcl_thr_kernel, dim3((unsigned)sk_cdiv(B, 64)), dim3(64), 0, st, (const float*)(ws + l.cmax), nchmax, lens, B,
                     ratio, (float*)(ws + l.thr));
  SK_CHECK_LAUNCH("dpcl_thr_kernel");
  return SK_OK;
}

int check_common(const char* who, const void* z, int ld, const void* mix, const void* lens, const void* offs, int T, int B, int F,
                 int D, int S, int smin) {
  SK_CHECK_ARG(D >= 1 && D <= DMAX, "%s: D = %d embedding dimensions outside 1..%d", who, D, DMAX);
  SK_CHECK_ARG(S >= smin && S <= MAXS, "%s: S = %d outside %d..%d", who, S, smin, MAXS);
  SK_CHECK_ARG(F >= 1 && T >= 1 && B >= 1 && B <= 65535, "%s: F = %d, T = %d, B = %d: F, T >= 1 and 1 <= B <= 65535 expected", who, F, T, B);
  SK_CHECK_ARG(shape_ok(T, B, F, D, S, smin), "%s: T * F = %lld points per utterance beyond 2^31 - 1", who, (long long)T * F);
  SK_CHECK_ARG((int64_t)ld >= (int64_t)F * D, "%s: ld = %d below F * D = %lld", who, ld, (long long)F * D);
  SK_CHECK_ARG(z && mix && lens && offs, "%s: null pointer (z, mix, lens or offs)", who);
  return SK_OK;
}

}  // namespace

extern "C" size_t sk_dpcl_workspace_bytes(int T, int B, int F, int D, int S) {
  if (!shape_ok(T, B, F, D, S, 1)) return 0;
  return layout_of(T, B, D, S, false).total;
}

extern "C" size_t sk_dpcl_kmeans_workspace_bytes(int T, int B, int F, int D, int S) {
  if (!shape_ok(T, B, F, D, S, 2)) return 0;
  return layout_of(T, B, D, S, true).total;
}

extern "C" int sk_dpcl_fwd(const float* z, int ld, const float* mix, const float* const* src_host, const int32_t* lens,
                           const int32_t* offs, int T, int B, int F, int D, int S, int weight, float vad_ratio,
                           const float* count_dev, double* lj, float* ab, float* stats, float* out, void* ws,
                           sk_stream_t stream) {
  if (int rc = check_common("sk_dpcl_fwd", z, ld, mix, lens, offs, T, B, F, D, S, 1)) return rc;
  SK_CHECK_ARG(weight == SK_DPCL_MR || weight == SK_DPCL_VAD, "sk_dpcl_fwd: weight = %d is neither SK_DPCL_MR nor SK_DPCL_VAD", weight);
  SK_CHECK_ARG(!(weight == SK_DPCL_VAD) || (vad_ratio >= 0.f && vad_ratio <= 1.f), "sk_dpcl_fwd: vad_ratio = %g outside [0, 1]", (double)vad_ratio);
  SK_CHECK_ARG(src_host && lj && ab && stats && out && ws, "sk_dpcl_fwd: null pointer (src_host, lj, ab, stats, out or ws)");
  SrcPtrs sp;
  for (int s = 0; s < MAXS; ++s) {
    sp.p[s] = s < S ? src_host[s] : nullptr;
    SK_CHECK_ARG(s >= S || sp.p[s], "sk_dpcl_fwd: source %d is a null pointer", s);
  }
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  const Layout l = layout_of(T, B, D, S, false);
  const int vad = weight == SK_DPCL_VAD, nchmax = chunks_of(T);
  if (vad)
    if (int rc = launch_threshold(mix, offs, lens, T, B, F, vad_ratio, w, l, st)) return rc;
  const float* thr = vad ? (const float*)(w + l.thr) : nullptr;
  double* partial = (double*)(w + l.partial);
  const dim3 grid(nchmax, B);
  switch (tiles_of(D, S)) {
    case 1:
      hipLaunchKernelGGL((dpcl_gram_kernel<1, false>), grid, dim3(256), 0, st, z, ld, mix, sp, offs, lens, F, D, S, vad, thr, nullptr, partial, nchmax);
      hipLaunchKernelGGL(dpcl_loss_kernel<1>, dim3(B), dim3(256), 0, st, (const double*)partial, nchmax, lens, D, S, thr, lj, ab, stats);
      break;
    case 2:
      hipLaunchKernelGGL((dpcl_gram_kernel<2, false>), grid, dim3(256), 0, st, z, ld, mix, sp, offs, lens, F, D, S, vad, thr, nullptr, partial, nchmax);
      hipLaunchKernelGGL(dpcl_loss_kernel<2>, dim3(B), dim3(256), 0, st, (const double*)partial, nchmax, lens, D, S, thr, lj, ab, stats);
      break;
    default:
      hipLaunchKernelGGL((dpcl_gram_kernel<3, false>), grid, dim3(256), 0, st, z, ld, mix, sp, offs, lens, F, D, S, vad, thr, nullptr, partial, nchmax);
      hipLaunchKernelGGL(dpcl_loss_kernel<3>, dim3(B), dim3(256), 0, st, (const double*)partial, nchmax, lens, D, S, thr, lj, ab, stats);
      break;
  }
  SK_CHECK_LAUNCH("dpcl_gram_kernel / dpcl_loss_kernel");
  hipLaunchKernelGGL(dpcl_out_kernel, dim3(1), dim3(64), 0, st, lj, B, count_dev, out);
  SK_CHECK_LAUNCH("dpcl_out_kernel");
  return SK_OK;
}

extern "C" int sk_dpcl_bwd(const float* z, int ld, const float* mix, const float* const* src_host, const int32_t* lens,
                           const int32_t* offs, int T, int B, int F, int D, int S, int weight, const float* ab,
                           const float* stats, const float* out, const float* gscale, float* dz, sk_stream_t stream) {
  if (int rc = check_common("sk_dpcl_bwd", z, ld, mix, lens, offs, T, B, F, D, S, 1)) return rc;
  SK_CHECK_ARG(weight == SK_DPCL_MR || weight == SK_DPCL_VAD, "sk_dpcl_bwd: weight = %d is neither SK_DPCL_MR nor SK_DPCL_VAD", weight);
  SK_CHECK_ARG(src_host && ab && stats && out && gscale && dz, "sk_dpcl_bwd: null pointer (src_host, ab, stats, out, gscale or dz)");
  SrcPtrs sp;
  for (int s = 0; s < MAXS; ++s) {
    sp.p[s] = s < S ? src_host[s] : nullptr;
    SK_CHECK_ARG(s >= S || sp.p[s], "sk_dpcl_bwd: source %d is a null pointer", s);
  }
  hipStream_t st = (hipStream_t)stream;
  const int vad = weight == SK_DPCL_VAD;
  const dim3 grid((unsigned)sk_cdiv((int64_t)T * F, 256), B);
#define SK_DPCL_BWD(DB) \
  hipLaunchKernelGGL(dpcl_bwd_kernel<DB>, grid, dim3(256), 0, st, z, ld, mix, sp, offs, lens, F, D, S, vad, ab, stats, out, gscale, dz)
  switch ((D + 7) / 8) {
    case 1: SK_DPCL_BWD(8); break;
    case 2: SK_DPCL_BWD(16); break;
    case 3: SK_DPCL_BWD(24); break;
    case 4: SK_DPCL_BWD(32); break;
    default: SK_DPCL_BWD(40); break;
  }
#undef SK_DPCL_BWD
  SK_CHECK_LAUNCH("dpcl_bwd_kernel");
  return SK_OK;
}

extern "C" int sk_dpcl_kmeans(const float* z, int ld, const float* mix, const int32_t* lens, const int32_t* offs, int T, int B,
                              int F, int D, int S, int iterations, float vad_ratio, const float* centroids_in, float* mask,
                              int ld_mask, int32_t* labels, float* centroids, void* ws, sk_stream_t stream) {
  if (int rc = check_common("sk_dpcl_kmeans", z, ld, mix, lens, offs, T, B, F, D, S, 2)) return rc;
  SK_CHECK_ARG(iterations >= 0, "sk_dpcl_kmeans: iterations = %d is negative", iterations);
  SK_CHECK_ARG(vad_ratio >= 0.f && vad_ratio <= 1.f, "sk_dpcl_kmeans: vad_ratio = %g outside [0, 1]", (double)vad_ratio);
  SK_CHECK_ARG(mask && labels && centroids && ws, "sk_dpcl_kmeans: null pointer (mask, labels, centroids or ws)");
  SK_CHECK_ARG((int64_t)ld_mask >= (int64_t)S * F, "sk_dpcl_kmeans: ld_mask = %d below S * F = %lld", ld_mask, (long long)S * F);
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  const Layout l = layout_of(T, B, D, S, true);
  const int nchmax = chunks_of(T), NT = tiles_of(D, S);
  if (int rc = launch_threshold(mix, offs, lens, T, B, F, vad_ratio, w, l, st)) return rc;
  const float* thr = (const float*)(w + l.thr);
  float* cent = (float*)(w + l.cent);
  float* pval = (float*)(w + l.pval);
  int32_t* pidx = (int32_t*)(w + l.pidx);
  int32_t* pcnt = (int32_t*)(w + l.pcnt);
  double* partial = (double*)(w + l.partial);
  const dim3 grid(nchmax, B);
  hipLaunchKernelGGL(dpcl_cent_in_kernel, dim3(B), dim3(256), 0, st, centroids_in, D, S, cent);
  SK_CHECK_LAUNCH("dpcl_cent_in_kernel");
  if (!centroids_in) {
    for (int k = 0; k < S; ++k) {
      hipLaunchKernelGGL(dpcl_pick_kernel, grid, dim3(256), 0, st, z, ld, mix, offs, lens, F, D, k, thr, (const float*)cent, pval, pidx, pcnt, nchmax);
      SK_CHECK_LAUNCH("dpcl_pick_kernel");
      hipLaunchKernelGGL(dpcl_pick_finish_kernel, dim3(B), dim3(64), 0, st, z, ld, offs, lens, F, D, k, (const float*)pval,
                         (const int32_t*)pidx, (const int32_t*)pcnt, nchmax, cent);
      SK_CHECK_LAUNCH("dpcl_pick_finish_kernel");
    }
  }
  SrcPtrs none;
  for (int s = 0; s < MAXS; ++s) none.p[s] = nullptr;
  for (int it = 0; it < iterations; ++it) {
    switch (NT) {
      case 1:
        hipLaunchKernelGGL((dpcl_gram_kernel<1, true>), grid, dim3(256), 0, st, z, ld, mix, none, offs, lens, F, D, S, 0, thr, (const float*)cent, partial, nchmax);
        hipLaunchKernelGGL(dpcl_cent_kernel<1>, dim3(B), dim3(256), 0, st, (const double*)partial, nchmax, lens, D, S, cent);
        break;
      case 2:
        hipLaunchKernelGGL((dpcl_gram_kernel<2, true>), grid, dim3(256), 0, st, z, ld, mix, none, offs, lens, F, D, S, 0, thr, (const float*)cent, partial, nchmax);
        hipLaunchKernelGGL(dpcl_cent_kernel<2>, dim3(B), dim3(256), 0, st, (const double*)partial, nchmax, lens, D, S, cent);
        break;
      default:
        hipLaunchKernelGGL((dpcl_gram_kernel<3, true>), grid, dim3(256), 0, st, z, ld, mix, none, offs, lens, F, D, S, 0, thr, (const float*)cent, partial, nchmax);
        hipLaunchKernelGGL(dpcl_cent_kernel<3>, dim3(B), dim3(256), 0, st, (const double*)partial, nchmax, lens, D, S, cent);
        break;
    }
    SK_CHECK_LAUNCH("dpcl_gram_kernel / dpcl_cent_kernel");
  }
  hipLaunchKernelGGL(dpcl_assign_kernel, dim3((unsigned)sk_cdiv((int64_t)T * F, 256), B), dim3(256), 0, st, z, ld, offs, lens, F, D, S,
                     (const float*)cent, mask, ld_mask, labels, centroids);
  SK_CHECK_LAUNCH("dpcl_assign_kernel");
  return SK_OK;
}
