// room.hip -- image-method room impulse responses made on the device (sk_room_rirs), gfx950: the stage in front of
// sk_fir_convolve that gives array dynamic mixing its rooms.  The definition is sepkern/room.py's (Allen & Berkley's images,
// Peterson's 64-tap Hann-windowed sinc per image); ism_rir_f32 there restates the arithmetic below in numpy.
//
// One workgroup of 16 waves per job and segment of 1024 taps; the segment under construction lives in LDS, one private copy
// per wave (16 x 4 KB).
//   * The images of a job are numbered i = 0 .. 8 (2 Mx + 1)(2 My + 1)(2 Mz + 1) - 1: parity p = i & 7, then m with m_z fastest.
//     Chunk c = i >> 6 belongs to wave c % 16.
//   * Scan: one image per lane, 64 at a time, in fp64 without contraction -- position, distance, tau = d (rate / c), and, where the
//     image's 64 taps meet the workgroup's segment, the amplitude with integer powers of the six reflection coefficients.
//     floor(tau) and the fraction f are split there; from f on everything is fp32: sinpi(f), cos and sin of pi f / 32, fp32(A).
//     At d = 200 m an fp32 tau would be off by 3e-4 samples.
//   * Deposit: the images that count are handed out one by one (readlane) in ascending order.  Lane j owns tap floor(tau) - 31 + j:
//     sin(pi (j - 31 - f)) = (-1)^j sin(pi f) and cos(pi (j - 31 - f) / 32) = cos a_j cos(pi f / 32) + sin a_j sin(pi f / 32), so a
//     lane needs one reciprocal and a few multiply-adds, and one image is one 256-byte row segment of the wave's own copy.
//   * h = copy0 + copy1 + ... + copy15 in that order, written with plain vector stores.
// A wave's deposits are one LDS round trip after the other (the next image may touch the same taps), so a workgroup's speed goes
// with its waves: private copies let every wave deposit whole images with all 64 lanes and without a barrier.  Cutting the time
// axis between WORKGROUPS keeps the copies small enough for 16 of them, and costs a scan of all images per segment (the
// amplitude is formed only for hits).  A tap's sum runs over the images that cover it, in ascending order per wave: the same
// bits whatever the segment length, so the cut is no part of the definition (DESIGN 28 has the measurements).  No atomics, no
// hand-off between workgroups: a job's bits depend neither on the batch around it nor on the run.
#include <cmath>
#include <vector>

#include "sk_common.h"

namespace {

constexpr int RM_WAVES = 16;
constexpr int RM_THREADS = RM_WAVES * SK_WAVE;
constexpr int RM_SEG = 1024;         // taps a workgroup builds
constexpr int RM_WIDTH = 64;          // taps per image
constexpr int RM_HALF = 31;           // an image's first tap is floor(tau) - RM_HALF
constexpr int RM_MAX_TAPS = 8192;
constexpr int RM_MAX_JOBS = 65535;
constexpr double RM_C = 343.0;        // m/s
constexpr double RM_MIN_DIRECT = 0.01;
constexpr int RM_LDS_LIMIT = 159 * 1024;
constexpr double RM_MAX_CANDIDATES = 134217728.0;  // 2^27 image positions scanned per job (8192 taps in 2 x 2 x 2 m need 4.5e7)

// One job as the kernel reads it (built on the host, copied into the workspace).
struct RoomJob {
  double L[3], beta[6], src[3], mic[3];
  double scale, rate_over_c;
  int64_t out_off;
  int32_t ntaps, total;   // total = 8 nx ny nz candidate images
  int32_t M[3], pad;
};

const char* const kRoomWhy[] = {"",
                                "ntaps outside 1..8192",
                                "a room dimension is not positive",
                                "a reflection coefficient outside [0, 1]",
                                "the source or the microphone does not lie strictly inside the room",
                                "source and microphone are less than 0.01 m apart",
                                "a negative output offset",
                                "scale is not finite",
                                "more than 2^27 candidate images (the room is too small for this many taps)"};

// Checks of the job arrays, shared by the size query and the call; 0 = fine, else the index of the message above.
int room_plan(const double* room, const double* beta, const double* src, const double* mic, const double* scale, const int32_t* ntaps,
              const int64_t* offs, int J, double rate, int* bad_job, RoomJob* jobs) {
  for (int j = 0; j < J; ++j) {
    *bad_job = j;
    const double *L = room + 3 * j, *b = beta + 6 * j, *s = src + 3 * j, *m = mic + 3 * j;
    if (ntaps[j] < 1 || ntaps[j] > RM_MAX_TAPS) return 1;
    for (int a = 0; a < 3; ++a)
      if (!(L[a] > 0.0) || !std::isfinite(L[a])) return 2;
    for (int a = 0; a < 6; ++a)
      if (!(b[a] >= 0.0 && b[a] <= 1.0)) return 3;
    double d2 = 0.0;
    for (int a = 0; a < 3; ++a) {
      if (!(s[a] > 0.0 && s[a] < L[a]) || !(m[a] > 0.0 && m[a] < L[a])) return 4;
      d2 += (s[a] - m[a]) * (s[a] - m[a]);
    }
    if (!(std::sqrt(d2) >= RM_MIN_DIRECT)) return 5;
    if (offs[j] < 0) return 6;
    if (!std::isfinite(scale[j])) return 7;
    // |m_a| <= M_a holds every image that counts (sepkern/room.py image_range forms the same numbers in the same order)
    double total = 8.0;
    int32_t M[3];
    for (int a = 0; a < 3; ++a) {
      const double r = std::ceil(((double)ntaps[j] + 32.0) * RM_C / (rate * 2.0 * L[a])) + 1.0;
      if (!(r < 1.0e8)) return 8;
      M[a] = (int32_t)r;
      total *= 2.0 * r + 1.0;
    }
    if (!(total <= RM_MAX_CANDIDATES)) return 8;
    if (jobs) {
      RoomJob& q = jobs[j];
      for (int a = 0; a < 3; ++a) { q.L[a] = L[a]; q.src[a] = s[a]; q.mic[a] = m[a]; q.M[a] = M[a]; }
      for (int a = 0; a < 6; ++a) q.beta[a] = b[a];
      q.scale = scale[j];
      q.rate_over_c = rate / RM_C;
      q.out_off = offs[j];
      q.ntaps = ntaps[j];
      q.total = (int32_t)total;
      q.pad = 0;
    }
  }
  return 0;
}

size_t room_jobs_bytes(int J) { return sk_align((size_t)J * sizeof(RoomJob), 256); }

bool room_args(const double* room, const double* beta, const double* src, const double* mic, const double* scale, const int32_t* ntaps,
               const int64_t* offs) {
  return room && beta && src && mic && scale && ntaps && offs;
}

// b^e, e >= 0, by binary exponentiation (0^0 = 1); room.py's _ipow multiplies in the same order
__device__ __forceinline__ double rm_ipow(double b, int e) {
#pragma clang fp contract(off)
  double r = 1.0;
  while (e > 0) {
    if (e & 1) r = r * b;
    e >>= 1;
    b = b * b;
  }
  return r;
}

__device__ __forceinline__ float rm_lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// grid (J, segments of the longest RIR), 1024 threads; dynamic LDS: RM_WAVES copies of RM_SEG floats.  Workgroup (j, y) builds taps
// [y RM_SEG, (y + 1) RM_SEG) of job j; one that lies beyond its job's taps leaves at once.
__global__ __launch_bounds__(RM_THREADS) void room_rirs_kernel(const RoomJob* __restrict__ jobs, float* __restrict__ rir) {
  extern __shared__ float rm_acc[];
  const RoomJob& jb = jobs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntaps = jb.ntaps, total = jb.total;
  const int t0 = (int)blockIdx.y * RM_SEG;
  if (t0 >= ntaps) return;
  const int width = min(ntaps - t0, RM_SEG);
  float* const acc = rm_acc + wave * RM_SEG;
  for (int n = lane; n < width; n += SK_WAVE) acc[n] = 0.f;   // the wave's own copy: its later accesses need no barrier

  // what lane j keeps for every image: j - 31, cos and sin of a_j = pi (j - 31) / 32 (rounded from fp64 once), (-1)^j
  const float tj = (float)(lane - RM_HALF);
  const float cj = (float)cospi((double)(lane - RM_HALF) * (1.0 / 32.0)), sj = (float)sinpi((double)(lane - RM_HALF) * (1.0 / 32.0));
  const float sgn = (lane & 1) ? -1.f : 1.f;

  const unsigned nz = 2u * (unsigned)jb.M[2] + 1u, ny = 2u * (unsigned)jb.M[1] + 1u;
  const double roc = jb.rate_over_c, scale = jb.scale;
  for (int c0 = wave * SK_WAVE; c0 < total; c0 += RM_WAVES * SK_WAVE) {
    // ---- scan: image c0 + lane, geometry in fp64, no contraction (ism_rir_f32 forms the same bits)
    const int i = c0 + lane;
    bool counts = false;
    int n0 = 0;
    float f = 0.f, A32 = 0.f;
    if (i < total) {
#pragma clang fp contract(off)
      const unsigned q = (unsigned)i >> 3, qz = q / nz;
      const int m[3] = {(int)(qz / ny) - jb.M[0], (int)(qz % ny) - jb.M[1], (int)(q % nz) - jb.M[2]};
      double d2 = 0.0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int p = (i >> a) & 1;
        const double R = (1.0 - 2.0 * (double)p) * jb.src[a] + 2.0 * (double)m[a] * jb.L[a] - jb.mic[a];
        d2 = (a == 0) ? R * R : d2 + R * R;
      }
      const double d = sqrt(d2);
      const double tau = d * roc;
      const double k = floor(tau);
      n0 = (int)fmin(k, 1.0e9) - RM_HALF;
      // the amplitude only where the 64 taps meet this workgroup's segment (which lies inside [0, ntaps): the image counts)
      if (n0 < t0 + width && n0 + RM_WIDTH > t0) {
        double g = 1.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const int p = (i >> a) & 1;
          g = (g * rm_ipow(jb.beta[2 * a], abs(m[a] - p))) * rm_ipow(jb.beta[2 * a + 1], abs(m[a]));
        }
        const double A = (scale * g) / ((4.0 * M_PI) * d);
        counts = A != 0.0;
        f = (float)(tau - k);
        A32 = (float)A;
      }
    }
    unsigned long long todo = __ballot(counts);
    if (todo == 0) continue;
    // the fp32 values every lane of the deposit needs, made 64 images at a time
    const float phi = f * (1.0f / 32.0f);
    const float cphi = cospif(phi), sphi = sinpif(phi);
    const float s = sinpif(f > 0.5f ? 1.0f - f : f);
    // ---- deposit: the images that count, ascending; lane j adds tap n0 + j
    while (todo) {
      const int l = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(todo));
      todo &= todo - 1;
      const int n = __builtin_amdgcn_readlane(n0, l) + lane - t0;
      const float fi = rm_lane_f(f, l), Ai = rm_lane_f(A32, l), si = rm_lane_f(s, l), ci = rm_lane_f(cphi, l), zi = rm_lane_f(sphi, l);
      const float t = tj - fi;
      const float w = 0.5f + 0.5f * (cj * ci + sj * zi);
      const float sinc = (t == 0.f) ? 1.0f : (sgn * si) * __builtin_amdgcn_rcpf(3.14159265358979323846f * t);
      const float v = (Ai * w) * sinc;
      if (n >= 0 && n < width) acc[n] += v;
    }
  }
  __syncthreads();
  float* const out = rir + jb.out_off + t0;
  for (int n = tid; n < width; n += RM_THREADS) {
    float h = rm_acc[n];
#pragma unroll
    for (int w = 1; w < RM_WAVES; ++w) h += rm_acc[w * RM_SEG + n];   // the waves' copies in index order
    out[n] = h;
  }
}

}  // namespace

// workspace: the J jobs (256-aligned)
extern "C" size_t sk_room_workspace_bytes(const double* room_host, const double* beta_host, const double* src_host, const double* mic_host,
                                          const double* scale_host, const int32_t* ntaps_host, const int64_t* rir_offs_host, int J,
                                          double rate) {
  if (J < 1 || J > RM_MAX_JOBS || !(rate >= 1.0) || !std::isfinite(rate)) return 0;
  if (!room_args(room_host, beta_host, src_host, mic_host, scale_host, ntaps_host, rir_offs_host)) return 0;
  int bad = 0;
  if (room_plan(room_host, beta_host, src_host, mic_host, scale_host, ntaps_host, rir_offs_host, J, rate, &bad, nullptr) != 0) return 0;
  return room_jobs_bytes(J);
}

extern "C" int sk_room_rirs(const double* room_host, const double* beta_host, const double* src_host, const double* mic_host,
                            const double* scale_host, const int32_t* ntaps_host, const int64_t* rir_offs_host, int J, double rate,
                            void* ws, float* rir, sk_stream_t stream) {
  SK_CHECK_ARG(J >= 1 && J <= RM_MAX_JOBS, "sk_room_rirs: J = %d jobs outside 1..%d", J, RM_MAX_JOBS);
  SK_CHECK_ARG(rate >= 1.0 && std::isfinite(rate), "sk_room_rirs: rate = %g below 1", rate);
  SK_CHECK_ARG(room_args(room_host, beta_host, src_host, mic_host, scale_host, ntaps_host, rir_offs_host),
               "sk_room_rirs: the job arrays (host) are required");
  int bad = 0;
  const int why = room_plan(room_host, beta_host, src_host, mic_host, scale_host, ntaps_host, rir_offs_host, J, rate, &bad, nullptr);
  SK_CHECK_ARG(why == 0, "sk_room_rirs: job %d (ntaps %d, room %g x %g x %g m): %s", bad, ntaps_host[bad], room_host[3 * bad],
               room_host[3 * bad + 1], room_host[3 * bad + 2], kRoomWhy[why]);
  SK_CHECK_ARG(ws && rir, "sk_room_rirs: null pointer");
  std::vector<RoomJob> jobs((size_t)J);
  room_plan(room_host, beta_host, src_host, mic_host, scale_host, ntaps_host, rir_offs_host, J, rate, &bad, jobs.data());
  int longest = 1;
  for (int j = 0; j < J; ++j) longest = std::max(longest, (int)ntaps_host[j]);
  const hipStream_t st = (hipStream_t)stream;
  RoomJob* const d_jobs = (RoomJob*)ws;
  // (a copy from pageable memory is staged before the call returns, as for sk_fir_convolve's jobs)
  SK_CHECK_HIP(hipMemcpyAsync(d_jobs, jobs.data(), (size_t)J * sizeof(RoomJob), hipMemcpyHostToDevice, st));
  return sk_launch_lds("sk_room_rirs", "room_rirs_kernel", room_rirs_kernel, dim3((unsigned)J, (unsigned)sk_cdiv(longest, RM_SEG)),
                       dim3(RM_THREADS), (size_t)RM_WAVES * RM_SEG * sizeof(float), RM_LDS_LIMIT, st, (const RoomJob*)d_jobs, rir);
}
