/* sepkern.h -- C ABI of libsepkern.so: the MI355X (gfx950) kernels under the uPIT hot path.
 *
 * The reference (mmaciej2/speech-separation) has no FFI: its hot path is library calls made
 * from Python (torch / librosa).  Each entry point below replaces the library call(s) cited
 * next to it and is what the host-side mirror of archs/uPIT.py, steps/extract_feats.py and
 * steps/reconstruct_sources.py binds through ctypes.
 *
 * Conventions
 *   - every function returns 0 on success, a negative SK_E* code otherwise; nothing throws
 *     across the boundary; sk_last_error() returns a thread-local message for the last failure
 *   - all pointers are DEVICE pointers unless the name ends in _host; the caller owns every
 *     buffer (the library allocates nothing); workspace sizes are queried
 *   - all work is enqueued asynchronously on `stream` (a hipStream_t passed as void*)
 *   - tensors are row-major contiguous fp32; sequence tensors are time-major, either zero-padded (T, B, C) or
 *     PACKED as torch's PackedSequence.data holds them (see "packed rows" below): every sequence entry point takes an
 *     offset table `offs` (NULL = padded)
 *   - LSTM weight layout is torch's per-parameter layout (gate rows i,f,g,o), so a
 *     reference state_dict round-trips unchanged
 */
#ifndef SEPKERN_H
#define SEPKERN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SK_VERSION 148

#define SK_OK 0
#define SK_EINVAL (-1)   /* bad argument / unsupported shape */
#define SK_ELAUNCH (-2)  /* HIP launch or runtime error      */
#define SK_ETIMEOUT (-3) /* a persistent kernel's bounded spin gave up (see sk_lstm_status) */

typedef void* sk_stream_t; /* hipStream_t */

int sk_version(void);
const char* sk_last_error(void);
/* Which numerics- or timing-changing build options this library was compiled with: 0 for the product build (plain `make`).
 * The kernel sources carry arithmetic / tuning / stamp switches for the measurement scripts under profiles/ (`make variant`,
 * `make gemm_variant` build them into libsepkern_<name>.so next to the product library); a library built with any of them
 * reports it here, and the ctypes loader refuses it unless SEPKERN_ALLOW_DIAGNOSTIC_LIB=1 (sepkern/_lib.py), bench.py unless
 * --diagnostic -- a headline can then not come from a wrong-numerics build by accident. */
#define SK_BUILD_TIMING_ONLY 0x1 /* results WRONG by construction (work skipped or faked to bound a kernel's time): reserved --
                                    no switch of the product sources sets it; an investigation kept under profiles/ may   */
#define SK_BUILD_ARITH 0x2       /* another arithmetic than documented (no sign phases, ...)                               */
#define SK_BUILD_TUNING 0x4      /* same results, other tuning constants (LDS stages, ring depths, poll cadence, ...)      */
#define SK_BUILD_STAMPS 0x8      /* per-phase clock stamps in the recurrence kernels                                       */
unsigned sk_build_flags(void);
/* number of CUs / LDS bytes per workgroup of the current device */
int sk_device_info(int* num_cu, int* lds_bytes);

/* ---------------------------------------------------------------- STFT front end
 * Replaces librosa.core.load's PCM scaling + librosa.core.stft(n_fft=512, hop=128) [+ np.abs]
 * (reference steps/extract_feats.py:85-89 train, :104-105 test).
 * Utterance u: samples wav[wav_offs[u] .. +nsamp[u]) (float32, or int16 PCM scaled by 1/32768
 * when pcm16 != 0); T_u = 1 + nsamp[u]/hop frames, reflect-padded by n_fft/2, periodic Hann.
 * Output element (t, f) of utterance u goes to out[out_offs[u] + t*stride_t[u] + f*stride_f[u]]
 * (units: elements; float32 magnitude when want_complex == 0, interleaved complex64 otherwise).
 * (stride_t = F, stride_f = 1) is the (T,F) training layout; (1, T_u) is the reference's
 * on-disk (F, T) layout.  frame_major != 0 promises stride_f[u] == 1 for every utterance (the strides live on
 * the device): frames are then stored straight from registers, coalesced, with no LDS staging.
 * max_frames >= max_u T_u sizes the grid.  n_fft must be 512. */
int sk_stft(const void* wav, int pcm16, const int64_t* wav_offs, const int32_t* nsamp, int nutt,
            int n_fft, int hop, int want_complex, void* out, const int64_t* out_offs,
            const int64_t* stride_t, const int64_t* stride_f, int frame_major, int max_frames, sk_stream_t stream);

/* ---------------------------------------------------------------- resampling front end
 * Replaces the `sr=` half of librosa.core.load (reference steps/extract_feats.py:74,85,97,104, steps/evaluate_oracle.py:96,122):
 * band-limited sinc interpolation with resampy's kaiser_best filter (64 zero crossings, Kaiser window), every tap evaluated
 * exactly; the arithmetic and the tap table are sepkern/resample.py's (unpinned: neither package is available to test against).
 * Rate ratio L / M = sr_out / sr_in in lowest terms, L != M.  Signal u: n_in[u] samples at in + in_offs[u] (float32, or int16
 * PCM scaled by 1/32768 when pcm16 != 0 -- sk_stft's convention); its n_out[u] float32 outputs go to out + out_offs[u]
 * (elements), nothing beyond them is written:
 *   y[n] = sum_{i < ntaps} taps[i * L + n % L] * x[first(n) + i],  first(n) = floor((n M - 64 max(L, M)) / L) + 1,
 * x = 0 outside [0, n_in[u]), fp32 accumulation with i ascending (bitwise reproducible; no atomics).
 * taps: ntaps x L float32, TAP-major, column c = the row of the outputs with n % L == c (phase (c M) % L), the factor
 * min(1, L / M) included; ntaps must equal 128 max(L, M) / L + 1 (integer division): 257 for 2:1, 706 for 441:80, 129 upwards.
 * The descriptor arrays live on the device; max_out >= max_u n_out[u] sizes the grid; 1 <= nsig <= 65535 (the grid's y).
 * A workgroup stages (tile - 1) M / L + 2 + ntaps samples, plus the ntaps taps when L == 1, in LDS, tile = 1024, 512 or 256
 * outputs, the largest that fits 60 KB.  A ratio whose 256-output tile does not fit is SK_EINVAL: M > 30 when L == 1
 * (511 M + 4 floats), M / L beyond 40.09 otherwise (383 M / L + 3 floats). */
int sk_resample(const void* in, int pcm16, const int64_t* in_offs, const int32_t* n_in, int nsig,
                const float* taps, int L, int M, int ntaps,
                float* out, const int64_t* out_offs, const int32_t* n_out, int max_out, sk_stream_t stream);

/* ---------------------------------------------------------------- dynamic mixing (training mixtures made on the device)
 * Mixes B training mixtures from single-speaker signals in ONE launch, by the WSJ0-2mix rule (sepkern/mixing.py states the
 * arithmetic and restates it in numpy fp64).  Source s of mixture u: nsamp[u] samples x_s at in + in_offs[s*B + u] (elements;
 * float32, or int16 PCM scaled by 1/32768 when pcm16 != 0); a crop is an offset, and two mixtures may read the same samples.
 *   P_s = mean x_s^2 (fp64);  g_s = fp32(amp[s*B + u] / sqrt(P_s)), 0 where P_s < 2^-40 (a silent source: no NaN, no huge gain)
 *   m = max_n max(|sum_s g_s x_s[n]|, max_s |g_s x_s[n]|) (fp32);  c = fp32(peak[u] / m), 0 where m == 0;  G_s = g_s * c (fp32)
 *   out + out_offs[(1+s)*B + u]: G_s x_s[n];   out + out_offs[u]: the mixture fmaf(G_s, x_s[n], acc), s ascending from acc = 0
 * (the sum inside m is that same chain with g).  amp are LINEAR amplitudes (the host computes 10^(snr/20)).  The mixture and its
 * sources share one scale, the largest magnitude among them is peak[u]; power is the plain mean square, not an active level.
 * quantize != 0: every output v becomes clip(rint(32768 v), -32768, 32767) / 32768, what a 16-bit wav file would hand back.
 * Only nsamp[u] floats at each of the (S + 1) B output offsets are written; gains (S*B floats, may be NULL) receives G.
 * One workgroup per mixture, no workspace, no atomics: bitwise reproducible, and a mixture's numbers do not depend on the batch
 * around it.  The descriptor arrays live on the device.  1 <= S <= 4, 1 <= B <= 65535, nsamp[u] >= 1. */
int sk_dynamic_mix(const void* in, int pcm16, const int64_t* in_offs, const int32_t* nsamp, int B, int S,
                   const float* amp, const float* peak, int quantize,
                   float* out, const int64_t* out_offs, float* gains, sk_stream_t stream);

/* ---------------------------------------------------------------- room impulse responses (reverberant dynamic mixing)
 * Convolves J signals with room impulse responses in one call; sepkern/reverb.py defines the result and restates the
 * arithmetic in numpy float32.  Job j: the nsamp[j] samples x at in + in_offs[j] (elements; float32, or int16 PCM scaled by
 * 1/32768 when pcm16 != 0, as sk_dynamic_mix takes them) and the ntaps[j] float32 taps h at rir + rir_offs[j]:
 *   out[out_offs[j] + i] = sum_{k < ntaps[j]} h[k] x[i + delay[j] - k],  0 <= i < nsamp[j],  x = 0 outside [0, nsamp[j])
 * i.e. np.convolve(x, h)[delay : delay + nsamp]: the output keeps the signal's length, and delay = the index of the direct path
 * keeps it aligned with the dry signal.  Exactly nsamp[j] floats are written per job.  Jobs may share a signal or a RIR.
 * Uniformly partitioned overlap-save, partitions of 256 taps, 512-point real transforms (the STFT front end's FFT), fp32: launch
 * one writes every job's partition and block spectra to ws, launch two accumulates each output block's spectrum over the
 * partitions in ascending order, inverts and stores.  No atomics, no hand-off between workgroups, one summation order: a
 * job's bits depend neither on the batch around it nor on the run, and int16 samples give the bits of their float32 copies.
 * The job arrays (names ending in _host) are HOST arrays, copied into the workspace on `stream`: the grids and the workspace
 * layout depend on them.  1 <= J <= 65535, 1 <= ntaps <= 8192, 0 <= delay < ntaps, 1 <= nsamp <= 2^30, offsets >= 0; at most
 * 2^31 - 1 transforms per call.  ws >= sk_fir_workspace_bytes(...) (0 for arguments out of range).  Bad arguments return
 * SK_EINVAL before anything is launched. */
size_t sk_fir_workspace_bytes(const int32_t* nsamp_host, const int32_t* ntaps_host, const int32_t* delay_host, int J);
int sk_fir_convolve(const void* in, int pcm16, const int64_t* in_offs_host, const int32_t* nsamp_host, const float* rir,
                    const int64_t* rir_offs_host, const int32_t* ntaps_host, const int32_t* delay_host, int J, void* ws,
                    float* out, const int64_t* out_offs_host, sk_stream_t stream);

/* ---------------------------------------------------------------- simulated rooms (array dynamic mixing)
 * Image-method room impulse responses made on the device, J per call; sepkern/room.py defines the result (ism_rir) and
 * restates the arithmetic in numpy (ism_rir_f32).  Job j: a rigid shoebox room[3j..] = (Lx, Ly, Lz) metres with the wall
 * reflection coefficients beta[6j..] = (x0, x1, y0, y1, z0, z1), a source src[3j..] and a microphone mic[3j..], c = 343 m/s.
 * Every image (p in {0,1}^3, m in Z^3) at R_a = (1 - 2 p_a) src_a + 2 m_a L_a - mic_a, d = |R|, tau = d rate / c adds
 *   A 0.5 (1 + cos(2 pi t / 64)) sinc(t),  t = n - tau,  to the taps n = floor(tau) - 31 .. floor(tau) + 32 inside [0, ntaps[j]),
 *   A = scale[j] prod_a beta_a0^|m_a - p_a| beta_a1^|m_a| / (4 pi d)                                               (0^0 = 1)
 * and exactly ntaps[j] floats are written at rir + rir_offs[j].  Geometry (position, d, tau, A) in fp64, the taps in fp32.
 * One workgroup per job builds the RIR in LDS, one private copy per wave, the images in an order fixed by the job's own
 * arguments: no atomics, no hand-off between workgroups, and a job's bits depend neither on the batch around it nor on the run.
 * The job arrays (names ending in _host) are HOST arrays, copied into the workspace on `stream`.  1 <= J <= 65535, 1 <= ntaps <=
 * 8192, room dimensions > 0, 0 <= beta <= 1, source and microphone strictly inside the room and at least 0.01 m apart, rate >= 1,
 * offsets >= 0, scale finite, at most 2^27 image positions to scan per job (8192 taps at 8 kHz in 2 x 2 x 2 m need 4.5e7).
 * ws >= sk_room_workspace_bytes(...) (0 for arguments out of range).  Bad arguments return SK_EINVAL before anything is launched. */
size_t sk_room_workspace_bytes(const double* room_host, const double* beta_host, const double* src_host, const double* mic_host,
                               const double* scale_host, const int32_t* ntaps_host, const int64_t* rir_offs_host, int J, double rate);
int sk_room_rirs(const double* room_host, const double* beta_host, const double* src_host, const double* mic_host,
                 const double* scale_host, const int32_t* ntaps_host, const int64_t* rir_offs_host, int J, double rate, void* ws,
                 float* rir, sk_stream_t stream);

/* The other channels of B array mixtures at the gains sk_dynamic_mix returned for the reference channel.  Channel p (0 <= p < P) of
 * mixture u: source s is the nsamp[u] float32 samples at in + in_offs[(s*P + p)*B + u], and
 *   out[out_offs[p*B + u] + n] = fmaf(G_s, x_{s,p,u}[n], acc), s ascending from acc = 0, G_s = gains[s*B + u]
 * -- sk_dynamic_mix's own chain: fed the reference channel's signals it reproduces that mixture bit for bit.  quantize != 0:
 * the same clip(rint(32768 v), -32768, 32767) / 32768.  Levels and the peak are DEFINED on the reference channel: another
 * channel may exceed `peak` (and, quantized, clip).  One writer per element; the descriptor arrays live on the device.
 * 1 <= S <= 4, 1 <= P <= 7, 1 <= B <= 65535, nsamp[u] >= 1. */
int sk_mix_channels(const float* in, const int64_t* in_offs, const int32_t* nsamp, int B, int S, int P, const float* gains,
                    int quantize, float* out, const int64_t* out_offs, sk_stream_t stream);

/* ---------------------------------------------------------------- noisy dynamic mixing (additive and diffuse array noise)
 * sepkern/noise.py defines the three results (Habets, Cohen & Gannot 2008 on the library's 512 / 128 transform) and restates
 * sk_diffuse_noise in numpy float32 (diffuse_f32).
 *
 * sk_noise_factors: for mixture u with C microphones at mics_host[(u*C + i)*3 ..] (HOST, fp64, metres) and bins k = 0 .. 256 at
 * f_k = k rate / 512: Gamma_k[i,j] = sinc(2 f_k d_ij / 343), and L_k = the lower-triangular Cholesky factor of
 * (1 - 2^-20) Gamma_k + 2^-20 I, all in fp64, one thread per (mixture, bin); L[(u*257 + k)*C(C+1)/2 + i(i+1)/2 + j] = fp32(L_k[i,j]),
 * j <= i.  The microphones travel as kernel arguments, 16 mixtures per launch.  2 <= C <= 8, 1 <= B <= 65535, rate >= 1,
 * microphones of a mixture at least 0.01 m apart.
 *
 * sk_diffuse_noise: channel c of mixture u: the nsamp[u] samples N_c at in + in_offs[c*B + u] (float32, or int16 PCM scaled by
 * 1/32768 when pcm16 != 0), C mutually independent noise signals, zero outside [0, nsamp[u]).  T = ceil(n / 128) + 3 frames,
 * frame t covering samples 128 (t - 3) .. + 511, periodic Hann for analysis and synthesis; per frame and bin
 *   X_i = L[i,0] N_0, then fmaf(L[i,j], N_j, .) with j ascending to i                (L: sk_noise_factors' layout)
 * and out[out_offs[c*B + u] + n] = fp32(2/3) times the sum of the four windowed inverse frames that cover sample n, in ascending
 * frame order.  Exactly nsamp[u] floats are written per signal.  A workgroup owns 13 hops of one mixture and transforms the 16
 * frames that touch them, the C spectra in registers; no atomics, no workspace, one writer per element: a mixture's bits depend
 * neither on the batch around it nor on the run, and int16 samples give the bits of their float32 copies.  The descriptor
 * arrays live on the device; max_nsamp >= max_u nsamp[u] sizes the grid (a longer signal is cut to it).  2 <= C <= 8,
 * 1 <= B <= 65535, 1 <= max_nsamp <= 2^30.
 *
 * sk_add_noise: IN PLACE on the C channels y_c of B mixtures (nsamp[u] float32 at sig + sig_offs[c*B + u], the reference channel
 * c = 0 first), with the noise v_c at noise + noise_offs[c*B + u] (float32, or int16 PCM when noise_pcm16 != 0):
 *   P_y = mean y_0^2, P_v = mean v_0^2 (fp64);  a = fp32(amp[u] sqrt(P_y / P_v)), 0 where either is below 2^-40
 *   y_c[n] = fmaf(a, v_c[n], y_c[n]);   quantize != 0: then clip(rint(32768 v), -32768, 32767) / 32768
 * amp is LINEAR (the host computes 10^(-snr/20)); one gain serves all channels, so a diffuse field keeps its coherence.  The
 * SNR is that of the whole mixture over the noise on the reference channel; the clean mixture's peak may be exceeded (and,
 * quantized, clipped).  gains_out (B floats, may be NULL) receives a.  One workgroup per mixture as sk_dynamic_mix: bitwise
 * reproducible, independent of the batch.  The descriptor arrays live on the device.  1 <= C <= 8, 1 <= B <= 65535, nsamp[u] >= 1.
 *
 * Bad arguments return SK_EINVAL before anything is launched. */
int sk_noise_factors(const double* mics_host, int B, int C, double rate, float* L, sk_stream_t stream);
int sk_diffuse_noise(const void* in, int pcm16, const int64_t* in_offs, const int32_t* nsamp, int B, int C, int max_nsamp,
                     const float* L, float* out, const int64_t* out_offs, sk_stream_t stream);
int sk_add_noise(float* sig, const int64_t* sig_offs, const void* noise, int noise_pcm16, const int64_t* noise_offs,
                 const int32_t* nsamp, int B, int C, const float* amp, int quantize, float* gains_out, sk_stream_t stream);

/* ---------------------------------------------------------------- mask-apply + iSTFT back end
 * Replaces np.multiply(mix_spec, mask) + librosa.core.istft(hop_length=128) + (*32767).astype(int16)
 * (reference steps/reconstruct_sources.py:39-42).  For utterance u and source s:
 *   spec (f,t) = mix[mix_offs[u] + f*mix_sf[u] + t*mix_st[u]] (complex64)
 *   mask (f,t) = mask[mask_offs[u*S+s] + f*mask_sf[u] + t*mask_st[u]] (float32; NULL mask = all ones)
 * Output 128*(T_u-1) samples at wav_out / pcm_out + out_offs[u*S+s] (either may be NULL).
 * int16 conversion truncates toward zero and WRAPS (no saturation), as the reference does. */
int sk_mask_istft(const void* mix_c64, const int64_t* mix_offs, const int64_t* mix_st, const int64_t* mix_sf,
                  const float* mask, const int64_t* mask_offs, const int64_t* mask_st, const int64_t* mask_sf,
                  const int32_t* nframes, int nutt, int S, int n_fft, int hop,
                  float* wav_out, int16_t* pcm_out, const int64_t* out_offs, int max_frames,
                  sk_stream_t stream);

/* ---------------------------------------------------------------- stitching windowed masks (long recordings)
 * A recording of T frames, too long for one pass of the network, is separated on overlapping windows of W frames every Hn
 * frames (W/2 <= Hn < W: at most two windows cover a frame, O = W - Hn >= 1 frames are shared); sk_stitch aligns the output
 * order of neighbouring windows on the frames they share and cross-fades them into one (T, S*257) mask.  No counterpart in the
 * reference; sepkern/stitch.py states the definition and restates the arithmetic below in numpy.
 * K = 1 + ceil(max(T - W, 0) / Hn) windows; window k starts at frame k Hn and has min(W, T - k Hn) frames (all but the last are
 * full; for K >= 2 the last has more than O).  Element (t, c) of window k, t local, c < S*257 with output s in columns
 * s*257 .. s*257+256, is mask[win_offs[k] + t*win_st[k] + c] (elements; the per-item offset / stride convention of sk_stft and
 * sk_mask_istft): the windows stay where the network wrote them -- window j of a uniform packed batch of B windows with
 * leading dimension ld has offset base + j*ld and stride B*ld, and windows of different batches mix freely (offsets are signed:
 * a batch allocated below `mask` has negative ones).
 * mag_rows (T, ld_mag >= 257): the magnitude rows of the WHOLE recording, as sk_stft writes them.
 *   cost (K-1, S, S) fp64: cost[k][i][j] = sum_{o < O, f < 257} (X[(k+1) Hn + o][f] (m_k[Hn + o][i*257 + f] - m_{k+1}[o][j*257 + f]))^2,
 *        every operand widened to fp64 first -- the PIT-MSE loss's magnitude-weighted distance, between two windows
 *   p_k = the first permutation p in itertools.permutations order that minimises sum_i cost[k][i][p(i)] (the PIT kernels' tie
 *        rule: a silent overlap gives the identity);  PI_0 = identity, PI_{k+1}(s) = p_k(PI_k(s));  perms (K, S) int32 = PI
 *   out (T, ld_out >= S*257): stream s of frame t = output PI_k(s) of the window(s) k that cover t.  One window: a copy.  Two:
 *        a + ramp[o] (b - a) with a the earlier and b the later window's value and o = t - (the later window's start); the
 *        subtraction, the product and the sum are fp32, each rounded (no fused multiply-add: numpy float32 gives the same
 *        bits), so a == b returns a.  ramp: O floats in [0, 1], the weight of the LATER window.
 * Three launches on `stream`, no host synchronisation: (1) boundaries x chunks of 16 overlap frames, fp64 partial sums into
 * fixed slots of ws; (2) one workgroup adds each boundary's chunks in ascending order, searches the S! permutations and
 * composes PI along the chain; (3) output frames x columns: every element of out in rows < T, columns < S*257 is written
 * exactly once, by one lane, and nothing else is; every mask element is read at most once per launch, and nothing outside the
 * windows' min(W, T - k Hn) x S*257 elements is read.  No atomics, no hand-off between workgroups: bitwise reproducible, and a
 * recording's bits do not depend on the descriptors' layout.  K = 1 is a copy (mag_rows, ramp, cost and ws may be NULL);
 * S = 1 skips the search.  All pointers are device pointers, the descriptors K entries each.
 * SK_EINVAL before anything is launched: S outside 1..4, T < 1, Hn outside [W/2, W), ws NULL where K > 1 (its size is the
 * caller's to honour: ws >= sk_stitch_workspace_bytes(T, W, Hn, S), which is 0 for arguments out of range). */
size_t sk_stitch_workspace_bytes(int T, int W, int Hn, int S);
int sk_stitch(const float* mag_rows, int ld_mag, const float* mask, const int64_t* win_offs, const int64_t* win_st,
              int T, int W, int Hn, int S, const float* ramp, float* out, int ld_out, int32_t* perms, double* cost,
              void* ws, sk_stream_t stream);

/* ---------------------------------------------------------------- mask-based MVDR beamforming (multi-channel recordings)
 * The stitched masks of one microphone steer one MVDR beamformer per separated stream over all C microphones (Souden et al.
 * 2010; Heymann et al. 2016; the CSS recipe of Yoshioka et al. 2018).  No counterpart in the reference; sepkern/mvdr.py states
 * the definition and restates the arithmetic below in numpy fp64.
 * Y: complex64 spectra, element (c, t, f) at Y[c*y_chan_stride + t*y_row_stride + f] (elements; unit bin stride, F = 257 bins,
 * y_row_stride >= 257); mask (T, ld_mask >= S*257) float32 with stream s in columns s*257 .. s*257+256 (sk_stitch's output).
 * nblk = ceil(T / block_frames) blocks; block j holds frames [j Lb, min(T, (j+1) Lb)), Lb = block_frames.
 *   A_j[s][f]   = sum_t mask[t][s*257 + f] y y^H, y = Y[:, t, f], t ascending over the block, every operand widened to fp64 first
 *                 (Hermitian: the upper triangle is computed, the diagonal is real)
 *   PHI_s[j][f] = sum of A_j'[s][f] over j' in [max(0, j - R), min(nblk - 1, j + R)], j' ascending, R = context_blocks
 *                 (R >= nblk - 1: one time-invariant beamformer)
 *   N_s         = sum_{s' != s} PHI_s', s' ascending (summed, not total minus own); then N_s += (loading * Re tr N_s / C) I
 *   G = N_s^-1 PHI_s (fp64 Cholesky factorisation and C solves), d = Re tr G, W_s[j][f] = G[:, ref] / d;
 *                 W_s[j][f] = e_ref (the reference channel passed through) where Re tr PHI_s == 0, Re tr N_s == 0 or not d > 1e-12
 *   weights (nblk, S, 257, C) complex64 = W;  scm_out (nblk, S, 257, C, C) complex128 = PHI_s before any loading (may be NULL)
 *   Z (S, T, 257) complex64: Z_s[t][f] = sum_c conj(W_s[t / Lb][f][c]) Y[c][t][f], fp32 fused multiply-adds, c ascending
 * (a post-mask is sk_mask_istft's mask argument).  Three launches on `stream`, no host synchronisation: (1) blocks x groups of
 * 64 bins, the upper triangle spread over the waves of a workgroup, into fixed slots of ws; (2) per (block, s, f) the context
 * sum, N_s, the factorisation and the solves on registers; (3) frames x bins: every element of Z and of weights is written
 * exactly once, nothing else is written, and nothing of Y outside its C x T x 257 elements or of mask outside its T x S*257 is
 * read.  No atomics, no hand-off between workgroups, every sum in one fixed order: bitwise reproducible, and the bits do not
 * depend on the strides.  The summation order inside a block is the definition's for bins 0..255; bin 256 adds 64 interleaved
 * partial sums.  Launch 2 reads (2 R + 1) blocks' statistics per block.  All pointers are device pointers.
 * SK_EINVAL before anything is launched: C outside 2..8, S outside 2..4, T < 1, block_frames < 1, context_blocks < 0, ref
 * outside [0, C), loading negative or NaN, ld_mask < S*257, y_row_stride < 257, a NULL Y, mask, weights, Z or ws (its size is
 * the caller's to honour: ws >= sk_mvdr_workspace_bytes(T, C, S, block_frames), which is 0 for arguments out of range). */
size_t sk_mvdr_workspace_bytes(int T, int C, int S, int block_frames);
int sk_mvdr(const void* Y_c64, int64_t y_chan_stride, int64_t y_row_stride, const float* mask, int ld_mask, int T, int C, int S,
            int block_frames, int context_blocks, int ref, double loading, void* weights_c64, void* Z_c64, void* scm_out_c128,
            void* ws, sk_stream_t stream);

/* ---------------------------------------------------------------- WPE dereverberation (multi-channel recordings)
 * Weighted prediction error (Nakatani et al. 2010; Yoshioka & Nakatani 2012): per bin, the late reverberation of every channel
 * is predicted from all channels' past, taps frames starting delay frames back, and subtracted.  No counterpart in the
 * reference; sepkern/wpe.py states the definition and restates the arithmetic below in numpy fp64.
 * Y: complex64 spectra, element (c, t, f) at Y[c*y_chan_stride + t*y_row_stride + f] (elements; unit bin stride, F = 257 bins,
 * y_row_stride >= 257); X likewise with strides of its own; X must not overlap Y.  D = C*taps <= 80.
 * nblk = ceil(T / Lb) blocks, Lb = block_frames; block j holds frames [j Lb, min(T, (j+1) Lb)), its window is
 * [max(0, j Lb - Lc), min(T, (j+1) Lb + Lc)), Lc = context_frames, Lb + 2 Lc <= 4096.  Per (block, bin), on the window, with
 * y~(t)[k C + c] = Y[c][t - delay - k][f] (0 before frame 0; the recording's frames before the window), x = y at first:
 *   lambda(t) = (sum_c |x_c(t)|^2) / C, c ascending, fp64; lambda(t) <- max(lambda(t), 1e-10 max_t lambda); w(t) = 1 / lambda(t)
 *   R = sum_t (w y~) y~^H (upper triangle, real diagonal), P = sum_t (w y~) y(t)^H, t ascending; R += (loading Re tr R / D) I
 *   G = R^-1 P: fp64 Cholesky factorisation R = U^H U and two triangular solves per column;   x(t) = y(t) - G^H y~(t)
 * `iterations` times.  The cell is passed through -- X = Y's own bits, G = 0 -- when in any iteration max lambda == 0,
 * Re tr R == 0 before the loading, or a component of G is not finite (a matrix that is not positive definite leaves NaN).
 *   X[c][t][f] = complex64(x_c(t)) for t in the block;  mag_out (T, ld_mag >= 257) float32 = |X[ref][t][f]| of the rounded value
 *   (may be NULL);  G_out (nblk, 257, D, C) complex128 = the last iteration's G (may be NULL).
 * One launch on `stream`, one workgroup per (block, bin) with R, P, G and the window's weights in LDS (up to 121 KB), no
 * host synchronisation, no atomics, no hand-off between workgroups, every sum in one fixed order: bitwise reproducible, and
 * the bits do not depend on the strides.  Every element of X (and of mag_out, G_out) is written exactly once, nothing else is
 * written, and nothing of Y outside its C x T x 257 elements is read.  All pointers are device pointers.
 * SK_EINVAL before anything is launched: C outside 1..8, taps < 1, delay < 1, C*taps > 80, iterations outside 1..8, T < 1,
 * block_frames < 1, context_frames < 0, block_frames + 2 context_frames > 4096, ref outside [0, C), loading negative or NaN,
 * y_row_stride or x_row_stride < 257, ld_mag < 257 with a mag_out, a NULL Y or X.  ws: sk_wpe keeps nothing in device memory
 * between its passes; sk_wpe_workspace_bytes is 0 and ws may be NULL. */
size_t sk_wpe_workspace_bytes(int T, int C, int taps, int block_frames, int context_frames);
int sk_wpe(const void* Y_c64, int64_t y_chan_stride, int64_t y_row_stride, int T, int C, int taps, int delay, int iterations,
           int block_frames, int context_frames, int ref, double loading, void* X_c64, int64_t x_chan_stride, int64_t x_row_stride,
           float* mag_out, int ld_mag, void* G_out_c128, void* ws, sk_stream_t stream);

/* ---------------------------------------------------------------- mask-based WPD convolutional beamforming (multi-channel recordings)
 * Weighted power minimisation distortionless response (Nakatani & Kinoshita 2019; Nakatani et al. 2020; the steering-vector-free
 * form of Zhang et al. 2020): dereverberation, separation and denoising solved jointly -- one filter per stream over the
 * present frame and the delayed past of all channels, fitted under that stream's own power and constrained to pass the
 * stream's direct image at the reference microphone.  It takes the place of sk_wpe + sk_mvdr.  No counterpart in the
 * reference; sepkern/wpd.py states the definition and restates the arithmetic below in numpy fp64.
 * Y: complex64 spectra, element (c, t, f) at Y[c*y_chan_stride + t*y_row_stride + f] (elements; unit bin stride, F = 257 bins,
 * y_row_stride >= 257); mask (T, ld_mask >= S*257) float32 with stream s in columns s*257 .. (sk_stitch's or sk_cacgmm's
 * output).  D = C*(taps + 1) <= 80; taps == 0 is a weighted MPDR beamformer.  Blocks and windows are sk_wpe's: block j holds
 * frames [j Lb, min(T, (j+1) Lb)), its window is [max(0, j Lb - Lc), min(T, (j+1) Lb + Lc)), Lb + 2 Lc <= 4096.
 * Per (block, bin, stream s), on the window, every operand widened to fp64 first, with m(t) = mask[t][s*257 + f],
 * y_(t)[c] = Y[c][t][f], y_(t)[C + k C + c] = Y[c][t - delay - k][f] (0 before frame 0; the recording's frames before the
 * window) and y(t) the first C entries of y_(t):
 *   lambda(t) = m(t) ((sum_c |y_c(t)|^2) / C), c ascending, in the first iteration of a call without W_in; otherwise
 *               |z(t)|^2 of z(t) = w^H y_(t), d ascending, with the previous iteration's w or W_in
 *   lambda(t) <- max(lambda(t), floor max_t lambda);  omega(t) = 1 / lambda(t)
 *   R = sum_t (omega y_) y_^H (upper triangle, real diagonal), t ascending;  R += (loading Re tr R / D) I
 *   PHI = sum_t (m y) y^H, C x C, every entry summed as it stands, t ascending;  PHI~ = [PHI; 0], D x C
 *   G = R^-1 PHI~: fp64 Cholesky factorisation R = U^H U and two triangular solves per column (sk_wpe's)
 *   d = sum_{c < C} Re G[c][c], c ascending;  w = G[:, ref] / d
 * `iterations` times.  The cell falls back to w = e_ref -- Z = Y[ref]'s own bits -- when in any iteration max lambda == 0,
 * Re tr R == 0 before the loading, Re tr PHI == 0, d is not > 0 or a component of w is not finite.
 *   Z (S, T, 257) complex64, contiguous: Z[s][t][f] = complex64(w^H y_(t)) for t in the block
 *   W_out (nblk, S, 257, D) complex128 = the last iteration's w (may be NULL);  W_in likewise, the filter to start from (may be
 *   NULL): one call of I iterations gives the bits of I calls of one chained through W_out -> W_in in every cell that does not
 *   fall back.  With loading > 0 cond(R) <= D / loading + 1 however short the window.
 * One launch on `stream`, grid (nblk, 257, S), one workgroup per (block, bin, stream) with R, PHI~, G, w and the window's
 * weights in LDS (up to 112 KB), no host synchronisation, no atomics, no hand-off between workgroups, every sum in one fixed
 * order: bitwise reproducible, and the bits do not depend on the strides.  Every element of Z and of W_out is written exactly
 * once, nothing else is written, and nothing of Y outside its C x T x 257 elements or of mask outside its T x S*257 is read.
 * All pointers are device pointers.
 * SK_EINVAL before anything is launched: C outside 2..8, S outside 2..4, taps < 0, delay < 1, C*(taps + 1) > 80, iterations
 * outside 1..8, T < 1, block_frames < 1, context_frames < 0, block_frames + 2 context_frames > 4096, ref outside [0, C),
 * loading negative or NaN, floor outside (0, 1] or NaN, ld_mask < S*257, y_row_stride < 257, a NULL Y, mask or Z.  ws: sk_wpd
 * keeps nothing in device memory between its passes; sk_wpd_workspace_bytes is 0 and ws may be NULL.  Not in it, on purpose: a
 * noise class, an eigenvector steering estimate, online estimation. */
size_t sk_wpd_workspace_bytes(int T, int C, int S, int taps, int block_frames, int context_frames);
int sk_wpd(const void* Y_c64, int64_t y_chan_stride, int64_t y_row_stride, const float* mask, int ld_mask, int T, int C, int S,
           int taps, int delay, int iterations, int block_frames, int context_frames, int ref, double loading, double floor,
           const void* W_in_c128, void* Z_c64, void* W_out_c128, void* ws, sk_stream_t stream);

/* ---------------------------------------------------------------- mask-guided cACGMM spatial clustering (multi-channel recordings)
 * Between the network and the beamformer: the masks of one microphone are re-estimated from all C channels by a complex
 * angular central Gaussian mixture model on the directions y / |y| (Ito et al. 2016), with the network's masks as the class
 * prior of every time-frequency point (Nakatani et al. 2017; guided source separation, Boeddeker et al. 2018).  No counterpart
 * in the reference; sepkern/cacgmm.py states the definition and restates the arithmetic below in numpy fp64.
 * Y: complex64 spectra, element (c, t, f) at Y[c*y_chan_stride + t*y_row_stride + f] (elements; unit bin stride, F = 257 bins,
 * y_row_stride >= 257; this may be sk_wpe's X); prior (T, ld_prior >= S*257) float32 with stream k in columns k*257 ..
 * (sk_stitch's output); mask_out (T, ld_out >= S*257) float32 likewise, not overlapping prior (neighbouring windows read it).
 * Blocks and windows are sk_wpe's: block j holds frames [j Lb, min(T, (j+1) Lb)), its window is [max(0, j Lb - Lc),
 * min(T, (j+1) Lb + Lc)), Lb + 2 Lc <= 4096.  Per (block, bin), on the window, every operand widened to fp64 first:
 *   n(t) = sum_c |y_c(t)|^2, c ascending; a frame with n(t) == 0 is dead, otherwise z(t) = y(t) / sqrt(n(t))
 *   p_k(t) = max(m_k, 1e-6) / sum_k' max(m_k', 1e-6), k' ascending, m_k = prior[t][k*257 + f]: fixed over the iterations
 *   state: one Hermitian B_k per class, I at the start or B_in (nblk, S, 257, C, C) complex128, of which the upper triangle and
 *          the real part of the diagonal are read.  A state is admitted before it is used: B_k = U^H U by an fp64 Cholesky
 *          factorisation; class k is reset to I where a pivot is not > 0 or not finite or an entry of U is not finite
 *   pass:  q_k(t) = ||U_k^-H z(t)||^2 by forward substitution;  l_k(t) = (log p_k(t) - 2 sum_a log U_k[a][a]) - C log q_k(t);
 *          gamma_k(t) = exp(l_k - max l) / sum_k' exp(l_k' - max l), k' ascending.  Dead frames get gamma_k = p_k and take part
 *          in no sum; while every class of the cell is the identity the pass is q = 1, gamma = p
 *   update (q of the old B): n_k = sum_t gamma_k(t), S_k = sum_t (gamma_k(t) / q_k(t)) z z^H, t ascending over the window (upper
 *          triangle, real diagonal);  B_k' = S_k (C / n_k);  B_k' += (loading Re tr B_k' / C) I;  admitted as above, and reset
 *          where n_k == 0
 * `iterations` (0..16) passes with update, then one pass without over the block's own frames:
 *   mask_out[t][k*257 + f] = float32(gamma_k(t));  B_out (nblk, S, 257, C, C) complex128 = the last state, full Hermitian
 *   matrices (may be NULL).  With iterations == 0 and no B_in mask_out is float32(p).  The model does not see the scale of B
 *   or a complex scalar on y(t); with loading > 0 every updated B_k has a condition number of at most C / loading + 1.
 * One launch on `stream`, one workgroup per (block, bin) with the states, their factors and a chunk of 64 frames in LDS, no
 * host synchronisation, no atomics, no hand-off between workgroups, every sum in one fixed order: bitwise reproducible, and
 * the bits do not depend on the strides or on the call count (one call of I iterations = I calls of one chained through
 * B_out -> B_in).  Every element of mask_out (T x S*257) and of B_out is written exactly once, nothing else is written, and
 * nothing of Y outside its C x T x 257 elements or of prior outside its T x S*257 is read.  All pointers are device pointers.
 * SK_EINVAL before anything is launched: C outside 2..8, S outside 2..4, T < 1, iterations outside 0..16, block_frames < 1,
 * context_frames < 0, block_frames + 2 context_frames > 4096, loading negative or NaN, ld_prior or ld_out < S*257,
 * y_row_stride < 257, a NULL Y, prior or mask_out.  ws: sk_cacgmm keeps nothing in device memory between its passes;
 * sk_cacgmm_workspace_bytes is 0 and ws may be NULL.  Not in it, on purpose: a noise class, learned mixture weights,
 * permutation alignment across bins, S = 1. */
size_t sk_cacgmm_workspace_bytes(int T, int C, int S, int block_frames, int context_frames);
int sk_cacgmm(const void* Y_c64, int64_t y_chan_stride, int64_t y_row_stride, const float* prior, int ld_prior, int T, int C, int S,
              int iterations, int block_frames, int context_frames, double loading, const void* B_in_c128, float* mask_out,
              int ld_out, void* B_out_c128, void* ws, sk_stream_t stream);

/* ---------------------------------------------------------------- fp32 GEMM (matrix cores)
 * C[M,N] (ldc) = act( opA(A) * opB(B) + bias[n] + (accumulate ? C : 0) ).
 * transA == 0: A is M x K row-major (lda); transA != 0: A is stored K x M row-major (lda).
 * transB == 0: B is K x N row-major (ldb); transB != 0: B is stored N x K row-major (ldb).
 * act: 0 none, 1 sigmoid.  bias may be NULL.  batch > 1 runs `batch` independent problems with
 * pointer strides sA/sB/sC/sbias (elements).  Replaces the matrix products inside nn.LSTM's input
 * projection, nn.Linear and their backward passes (reference archs/uPIT.py:132,141). */
int sk_gemm_f32(const float* A, const float* B, float* C, const float* bias, int M, int N, int K,
                int lda, int ldb, int ldc, int transA, int transB, int accumulate, int act,
                int batch, int64_t sA, int64_t sB, int64_t sC, int64_t sbias, sk_stream_t stream);
/* Same product with K split into `splitk` slices (for weight gradients: few output tiles, K = T*B rows):
 * slices write dense partial slabs into ws (>= sk_gemm_workspace_bytes); the block that finishes a tile's LAST slice
 * (a ticket counter per tile at the head of ws) adds the slabs in fixed slice order and applies bias / accumulate /
 * act -- deterministic, no floating-point atomics, no second launch (the bf16 kernels use a second kernel for the same
 * sums).  ws must be ZERO-FILLED before its first use; every launch leaves its head (the counters) zeroed again.
 * variant (which kernel; results agree to fp32 summation order -- every variant is an fp32 product with fp32 accumulation):
 *   0  choose (the default everywhere).  Products whose operands allow LDS-DMA staging (every operand row 16-byte aligned, K a
 *      multiple of 16, not the T/T form) run on the BF16 MATRIX PIPE by the three-way split of both fp32 operands: x = hi + mid + lo
 *      EXACTLY, three bf16 pieces made by rounding to nearest (bf16 has 8 significand bits: |x - hi| <= 2^-8 |x|, so |mid| <= 2^-8 |x|
 *      and |lo| <= 2^-16 |x|; typical values are half of these bounds).  Of the nine piece products per element pair -- each exact in
 *      fp32 (8 x 8 bits), of relative sizes 1, 2^-8 (two), 2^-16 (three), 2^-24 (two), 2^-32 -- the six of size >= 2^-16 are added
 *      into fp32 accumulators by v_mfma_f32_32x32x16_bf16; the three smallest, together at most 2^-23 |a||b| in the worst case (one
 *      fp32 ulp of the product; 2^-25 for typical pieces), are not formed: a SINGLE product may therefore be off by about one ulp
 *      where an fp32 FMA is exact (tests: <= 2^-22 relative).  What justifies calling this an fp32 GEMM is measured, not this
 *      bound: on sums the error against fp64 is not above the fp32-MFMA kernels' (tests, operands spanning 2^+-20; full-size
 *      training step in four arithmetics against one oracle step).  160-212 TFLOP/s fp32-equivalent on the training step's large
 *      products against 124-135 (one MI355X, stand-alone; the fp32-MFMA pipe's own peak is 157).  Kernels: 9 for unsplit,
 *      unbatched products of at least 192 tiles of 256 x 128 (the split is done once per element while the tile is staged:
 *      186-212 TFLOP/s; 72 KB of LDS, 200 VGPRs -- a caller that runs a product beside a persistent recurrence passes 2), else 2
 *      (128 x 128 tiles; any splitk / batch).
 *      SIGN PHASES: the bf16 MFMA truncates the alignment of its addends towards minus infinity, so a plain split-product result
 *      carries a DC offset (about -2e-11 of the result per K element on all-positive operands: -1.5e-7 at K = 7168) that anything
 *      integrating the result amplifies (r05: the recurrence below a data gradient).  Both split kernels, in every form, therefore
 *      keep -sum instead of +sum in their accumulators over stretches of K (signs + - - +, the B operand negated before it is
 *      split): truncation then pulls down and up in turn and the offsets cancel (tests/test_gpu_signed_error.py: mean signed
 *      error at the fp32-MFMA kernels' level).  The pattern runs over the whole K, in a whole number p = (n + 32) / 64 of periods
 *      of about 64 K steps of 16 (n = K / 16 steps): a stretch is q = ceil(n / 4p) steps, 14 / 16 / 17 at K = 1792 / 7168 /
 *      12800; products of fewer than 48 steps (K < 768) keep the plain form.
 *      Other operands (F = 257 columns, K = 514): the fp32-MFMA kernels as under 8.  Operands
 *      beyond bf16's finite range (|x| > 3.39e38) round to inf.  SEPKERN_GEMM_SPLIT=0 makes 0 mean 8.
 *   1  the register-staged fp32-MFMA kernel (v_mfma_f32_32x32x2_f32), any alignment
 *   2  the 128 x 128-tile split kernel wherever the LDS-DMA conditions hold (else as 8)
 *   3 / 4  the 128 x 128 / 256 x 128-tile fp32-MFMA LDS-DMA kernels wherever they apply (diagnostics)
 *   9  256 x 128 tiles, split once per element while staging (unsplit, unbatched products; else as 2)
 *   6  256 x 256 tiles, one PERSISTENT workgroup per CU with a stream-K cut of the last partial round of tiles, fp32 MFMA:
 *      unsplit, unbatched products; splitk = 1 and ws >= sk_gemm_streamk_workspace_bytes(), zero-filled before its first use and
 *      left with zeroed counters by every launch (without ws: 4).  Tiles of the cut are summed piece by piece in a fixed order:
 *      deterministic.
 *   8  choose among the fp32-MFMA kernels only -- the reference's literal arithmetic (fp32 products, fp32 accumulation rounded to
 *      nearest): LDS-DMA where the operands allow, stream-K (6) for the large unsplit N/T and N/N products when a ws is given, the
 *      register-staged kernel otherwise.  bench.py times the whole step on it as secondary.fp32_mfma.
 *   (5: the 256 x 256 tile without the stream-K cut, retired in r04; 7: the split-product form of 6, retired in r06 -- since the
 *   planes kernel it served no launch of any configuration.  Both are SK_EINVAL.) */
size_t sk_gemm_workspace_bytes(int M, int N, int batch, int splitk);
/* Which kernel the calling thread's LAST sk_gemm_f32[_splitk] / sk_gemm_bf16_splitk launch took (profiling: bench.py prices a
 * launch against the peak of the matrix pipe it ran on; tests/test_gpu_census.py generates DESIGN.md's kernel census from it):
 * 1 register-staged fp32 MFMA, 3 / 4 / 6 the 128 x 128 / 256 x 128 / stream-K fp32-MFMA LDS-DMA kernels, 2 / 10 the 128 x 128 /
 * 256 x 128 split-while-staging SPLIT kernels (bf16 pipe, six piece products), 9 bf16 inputs (fp32 operands rounded on the way
 * in); sk_gemm_bf16_nt / _mm: 11 / 12 the 256 x 128 / 256 x 256-tile bf16-operand kernel, 13 its stream-K form; sk_gemm_pl3_tn: 14;
 * 0 before the first launch.
 * A thread-local read-back: with the error string of sk_last_error() the library's only mutable state that is not a caller's
 * buffer (SURVEY 8b's rule has these exceptions -- sk_lstm_last_launch() is the third --, all thread-local and none read by any
 * kernel or launch decision). */
int sk_gemm_last_kernel(void);
size_t sk_gemm_streamk_workspace_bytes(void);
/* Zero the ticket counters at the head of a split-K workspace (once, before its first use; a buffer that was allocated
 * zero-filled needs no call). */
int sk_gemm_workspace_init(void* ws, sk_stream_t stream);
int sk_gemm_f32_splitk(const float* A, const float* B, float* C, const float* bias, int M, int N, int K,
                       int lda, int ldb, int ldc, int transA, int transB, int accumulate, int act,
                       int batch, int64_t sA, int64_t sB, int64_t sC, int64_t sbias, int splitk, void* ws,
                       int variant, sk_stream_t stream);
/* Same contract, bf16 matrix-core inputs (BASELINE configs[3]: "bf16"): A and B stay fp32 in memory and are
 * rounded to bf16 (round-to-nearest-even) on the way into the matrix cores; products are exact and are
 * accumulated in fp32; C, bias, slabs are fp32.  Equals an fp32 GEMM of the bf16-rounded operands up to
 * summation order. */
int sk_gemm_bf16_splitk(const float* A, const float* B, float* C, const float* bias, int M, int N, int K,
                        int lda, int ldb, int ldc, int transA, int transB, int accumulate, int act,
                        int batch, int64_t sA, int64_t sB, int64_t sC, int64_t sbias, int splitk, void* ws,
                        sk_stream_t stream);

/* bf16 operands IN MEMORY, both K-contiguous ("NT"): C[M,N] = act(A[M,K] B[N,K]^T + bias (+ C)), A and B bf16
 * (row-major, leading dimensions lda, ldb in elements), C / bias / slabs fp32.  The form every product of the bf16
 * configuration is brought to by writing row-major bf16 copies of the operands (sk_cast_bf16_rows; a factor whose rows
 * are the contraction index enters sk_gemm_bf16_mm K-major, so no transposed copy exists).  Requirements: K % 64 == 0 (pad the copies with zero columns), lda, ldb, sA, sB
 * multiples of 8, A and B 16-byte aligned; rows are read up to K.  M and N are arbitrary.  splitk / ws / batch /
 * accumulate / act as sk_gemm_f32_splitk. */
int sk_gemm_bf16_nt(const void* A, const void* B, float* C, const float* bias, int M, int N, int K, int lda, int ldb,
                    int ldc, int accumulate, int act, int batch, int64_t sA, int64_t sB, int64_t sC, int64_t sbias,
                    int splitk, void* ws, sk_stream_t stream);
/* The same product with either operand optionally K-MAJOR in memory: a_kmajor: A is stored [K][M] (element (m, k) at
 * A[k * lda + m], i.e. the TRANSPOSE of an (K, M) row-major matrix is the factor), likewise b_kmajor for B stored [K][N].
 * This is what the weight-gradient products (both factors are activation / gradient matrices whose ROWS are the
 * contraction index) and the data-gradient products (the weight matrix (N, K') is the K-major B of dout (R, N) x W) need:
 * with it they read the same row-major bf16 copies as the forward products and no transposed copy is ever made (the
 * tiles are DMA'd as they lie and the MFMA fragments are gathered by the transposed LDS read ds_read_b64_tr_b16).
 * K-major operand: ld = elements between consecutive k rows, >= its dimension rounded up to 8 and a multiple of 8; the
 * (ld - dim) padding elements of a row must be readable (finite or not: their products are never stored); K % 64 == 0
 * as always -- rows [K', K) of a zero-padded factor must be zeros in at least one of the two factors.
 * splitk = 1 WITH ws != NULL (>= sk_gemm_streamk_workspace_bytes(), zero-filled before its first use; r03): the product
 * may run as the persistent stream-K form of the 256 x 256-tile kernel (unbatched, N % 256 == 0 or N > 1024, K >= 512):
 * one workgroup per CU, the last partial round of tiles cut along K, pieces added in a fixed order (deterministic) --
 * instead of K slabs of the whole matrix and a reduce launch.  Not for products meant to run beside a recurrence. */
int sk_gemm_bf16_mm(const void* A, const void* B, float* C, const float* bias, int M, int N, int K, int lda, int ldb,
                    int ldc, int a_kmajor, int b_kmajor, int accumulate, int act, int batch, int64_t sA, int64_t sB,
                    int64_t sC, int64_t sbias, int splitk, void* ws, sk_stream_t stream);
/* ---------------------------------------------------------------- operands that arrive split (r06)
 * The weight gradients of the training step are T/N products of activation / gradient matrices whose ROWS are the contraction
 * index.  As fp32 split products (sk_gemm_f32_splitk variant 2) every wave of the GEMM cuts the fragments it reads into their
 * three bf16 pieces -- each element twice per workgroup, and beside a persistent recurrence that VALU work and the longer launch
 * are taken from the recurrence too.  Here the PRODUCERS cut each operand once: sk_split_rows (layer inputs, recurrent inputs),
 * sk_lstm_bwd's plane_bf16 (dgx); sk_gemm_pl3_tn multiplies the planes.
 * sk_split_rows: dst plane p (p = 0 hi, 1 mid, 2 lo; `plane` elements apart), row r, column c = piece p of src[r][c] (pieces by
 * rounding to nearest even, exactly the pieces the split kernels make); zeros for C <= c < ld_dst and for rows R .. R_pad - 1.
 * ld_dst % 8 == 0, plane >= R_pad * ld_dst and % 8 == 0, dst 16-byte aligned. */
int sk_split_rows(const float* src, int R, int C, int ld_src, void* dst, int ld_dst, int R_pad, int64_t plane, sk_stream_t stream);
/* C[M,N] (+)= A^T B on operands that arrive split: A = three bf16 planes [K][lda] (element (k, m) of plane p at
 * Apl[p * planeA + k * lda + m]), B likewise [K][ldb]; fp32 accumulation of the six piece products per element pair with the sign
 * phases of the split kernels -- bit for bit sk_gemm_f32_splitk variant 2 on the fp32 matrices the planes were cut from.  K % 16 ==
 * 0 (zero tail rows in the planes), lda / ldb / planeA / planeB / sA / sB multiples of 8 elements, lda >= M rounded up to 8 (+ the
 * batch offset), planes 16-byte aligned; batch, splitk / ws (zero-filled once) as sk_gemm_f32_splitk.  128 x 128 tiles, 120
 * VGPRs, 48 KB of LDS: meant to run beside a persistent recurrence (and alone). */
int sk_gemm_pl3_tn(const void* Apl, const void* Bpl, float* C, int M, int N, int K, int lda, int ldb, int ldc, int64_t planeA,
                   int64_t planeB, int accumulate, int batch, int64_t sA, int64_t sB, int64_t sC, int splitk, void* ws,
                   sk_stream_t stream);
/* dst[r][c] = bf16(src[r][c]) (round to nearest even) for r < R, c < C; 0 for C <= c < ld_dst and for the rows
 * R .. R_pad-1 (R_pad >= R): a copy that also serves as a K-MAJOR factor of sk_gemm_bf16_mm (its rows are then the
 * contraction index, read in whole K steps of 64).  ld_dst % 8 == 0. */
int sk_cast_bf16_rows(const float* src, int R, int C, int ld_src, void* dst, int ld_dst, int R_pad, sk_stream_t stream);

/* ---------------------------------------------------------------- packed rows
 * The reference feeds the network a torch PackedSequence (archs/uPIT.py:46,132,135): of a length-sorted batch only the
 * R = sum(lens) valid frames exist, time-major: row of (t, j) is offs[t] + j for j < n_t, where n_t = offs[t+1] - offs[t]
 * is the number of utterances longer than t (offs has T+1 int32 entries, offs[0] = 0, offs[T] = R; lens[j] sorted
 * descending, lens[0] = T).  Entry points that take `offs` work on that layout; offs = NULL means zero-padded (T, B, C).
 * sk_pack_rows / sk_unpack_rows convert (perm, may be NULL: sorted position j is the caller's utterance perm[j]);
 * unpack writes zeros at the padded positions, or the row `fill` (C floats; may be NULL) -- the value the reference's
 * network shows at a zero-padded frame, sigmoid(lin(bn(0))), archs/uPIT.py:135-144.  ld_packed >= C is the packed
 * matrix's leading dimension. */
int sk_pack_rows(const float* padded, const int32_t* offs, const int32_t* perm, int T, int B, int C, float* packed,
                 int ld_packed, sk_stream_t stream);
int sk_unpack_rows(const float* packed, int ld_packed, const int32_t* offs, const int32_t* perm, int T, int B, int C,
                   const float* fill, float* padded, sk_stream_t stream);
/* The recurrent INPUT of every packed row of one BLSTM layer: out[r][0:H] = forward-direction output of the same
 * utterance one frame earlier (h0[0][j] at t = 0), out[r][H:2H] = reverse-direction output one frame later (h0[1][j] at the
 * utterance's last frame); y (R, ldy >= 2H) is the layer output, h0 (2, B, H).  With it the recurrent weight gradient is a
 * plain product over the packed rows, dW_hh[d] = dG[:, d]^T out[:, d-half] (in the padded layout the shift was a constant
 * B rows; packed it varies with t).  out_bf16 != 0: out is bf16 (the operand copy of the bf16 configuration). */
int sk_hprev_rows(const float* y, int ldy, const float* h0, const int32_t* offs, int T, int B, int H, void* out,
                  int ld_out, int out_bf16, sk_stream_t stream);

/* ---------------------------------------------------------------- BLSTM recurrence
 * One bidirectional LSTM layer's time recurrence (the part of nn.LSTM, reference
 * archs/uPIT.py:115,132, that cannot be batched over time), with packed-sequence semantics:
 * for row b the state is frozen at t >= lens[b]; the reverse direction starts from (h0,c0) at t = lens[b]-1.
 * Sequence tensors below are written (T,B,..) for the padded layout (offs = NULL; y is then 0 at t >= lens[b]); with
 * `offs` they are the R packed rows ("packed rows" above; lens sorted descending) and positions past a row's end do
 * not exist -- nothing is read or written there.
 *   gx    (T,B,2,4H)  input projections x*W_ih^T + b_ih + b_hh for both directions, GATE-INTERLEAVED: within a
 *                     direction's 4H values, element 4u + g is gate g (i,f,g,o) of hidden unit u -- the four gates
 *                     of a cell are one 16-byte access (torch keeps the rows of W_ih gate-major, g H + u:
 *                     sk_gate_rows reorders a weight matrix / bias once so that a plain GEMM produces this layout)
 *   whh   (2,4H,H)    recurrent weights (torch layout, gate rows i,f,g,o)
 *   h0,c0 (2,B,H)     initial state of this layer;  hn,cn (2,B,H) final state (may be NULL)
 *   y     (T,B,2H)    layer output [fwd | bwd]
 *   gates (T,B,2,4H)  post-activation i,f,g,o (gate-interleaved like gx) and cs (T,B,2,H) cell states, saved
 *                     for the backward pass (both NULL for inference)
 *   ws    workspace of sk_lstm_workspace_bytes(); zeroed by the call itself
 * mode: a word of the SK_LSTM_* fields below, the same word for sk_lstm_fwd and sk_lstm_bwd except where noted.  Everything
 * but the launch kind, SK_LSTM_BF16 and SK_LSTM_SPLIT3 / _TAGGED is speed only (never the arithmetic).
 *   launch kind (low byte)  SK_LSTM_AUTO: persistent where the grid is co-resident, else per step; SK_LSTM_PERSISTENT: one launch
 *                           with a flag-synchronised time loop (SK_EINVAL if the grid does not fit); SK_LSTM_PER_STEP
 *   SK_LSTM_GMIN(g)         minimum number of 16-row batch groups a workgroup carries (0/1 = as few as fit, at most 8): a larger
 *                           value shrinks the persistent grid, leaving CUs free for kernels running concurrently on other streams
 *   SK_LSTM_BF16            bf16 matrix-core inputs (this one IS arithmetic: BASELINE configs[3])
 *   SK_LSTM_BWD_EXCLUSIVE   BACKWARD (r06): the instantiation whose LDS footprint (127 KB) leaves no room for a workgroup of
 *                           sk_gemm_pl3_tn beside it, so that products enqueued on other streams take the CUs the grid leaves free
 *                           instead of sharing the recurrence's (without it and with one batch group per workgroup: 113 KB, such a
 *                           workgroup fits).  FORWARD: the same bit was the 8-unit / 256-thread workgroup form, retired in r05
 *                           (slower at every shape); setting it is SK_EINVAL
 *   SK_LSTM_MAP(m)          block id -> stream map, 0..3
 *   SK_LSTM_POLL1           forward: one polling wave per workgroup.  Backward: ignored (one wave polls always)
 *   SK_LSTM_REPFLAGS        forward: flags replicated per XCD; cleared by SK_LSTM_FLAG_PER_LINE.  Backward: ignored
 *   SK_LSTM_FLAG_PER_LINE   one flag per 128-byte line
 *   SK_LSTM_DELAY(d)        hold-back of a step's first poll in units of 0.1 us, 1..30; SK_LSTM_DELAY_NONE (31): none.  0: FORWARD
 *                           the library's choice (by grid size), BACKWARD none
 *   SK_LSTM_SPLIT3, SK_LSTM_TAGGED   forward, fp32 (below); ignored with SK_LSTM_BF16 and by the backward
 *   SK_LSTM_XL8             XCD-local streams (below)
 * SK_LSTM_SPLIT3 (fp32 forward, H <= 896): the product h W_hh^T by the EXACT three-way bf16 split of both fp32
 * operands on the bf16 matrix pipe -- x = hi + mid + lo with three bf16 pieces (24 significand bits = 3 x 8); of the nine piece
 * products per element pair (each exact in fp32) the six of relative size >= 2^-16 are added into fp32 accumulators by
 * v_mfma_f32_16x16x32_bf16, the three of size <= 2^-24 -- together at most 2^-23 of |w||h|, see sk_gemm_f32_splitk variant 0 --
 * are not formed: an fp32 product in another summation order (error against fp64 not above the fp32-MFMA kernel's, results
 * within 2.2e-6 of it, no operand perturbed), 96 instead of 256 matrix-pipe cycles per 32 k.  W_hh is split once per launch,
 * h by its producer (three bf16 images, flags hand-off).  Sign phases (r06): the two K halves of a workgroup accumulate with
 * opposite signs (one on -W_hh), so that the bf16 MFMA's truncation towards minus infinity pulls one partial sum down and the
 * other up -- the cell state integrates over the sequence what is left of it (tests/test_gpu_signed_error.py: 400 steps
 * against an fp64 recurrence).  The engine ships it for the fp32 forward recurrence (bench.py's config.numerics
 * names it);
 * SK_LSTM_TAGGED (fp32 forward; not together with SK_LSTM_SPLIT3): "the data is the flag" -- every exchanged h word carries the step's epoch
 * in its two low mantissa bits, producers publish without drain / barrier / flag, consumers hold back, pull, check every word
 * and pull again what was not complete; the next step's product runs on the tagged words (<= 3 ulp = 3.6e-7 relative),
 * everything stored (y, gates, cs, states) is exact.  The r03 default; still the engine's choice for H > 896;
 * SK_LSTM_XL8 (with SK_LSTM_BF16, both directions, persistent launches, 640 < H <= 896, B <= 32, a device of 8 XCDs x 32 CUs; ignored otherwise;
 * r06): XCD-LOCAL streams of 8 rows -- every (direction, 8-row batch group) stream is 28 workgroups of 32 hidden units on ONE
 * XCD, h_t published with plain stores and a plain flag (within an XCD the L2 is the coherence point; polls and pulls stay sc1),
 * 14 KB instead of 28 KB pulled per workgroup and step.  Same arithmetic bit for bit.  A workgroup joins the stream of the XCD it
 * runs on (HW_REG_XCC_ID + one counter per XCD): no dependence on the order in which blocks are dealt; an XCD that received fewer
 * than 28 workgroups ends in the bounded-spin status word (sk_lstm_status: SK_ETIMEOUT, the step is skipped).
 */
#define SK_LSTM_AUTO 0
#define SK_LSTM_PERSISTENT 1
#define SK_LSTM_PER_STEP 2
#define SK_LSTM_KIND(mode) ((mode) & 0xff)
#define SK_LSTM_GMIN_SHIFT 8 /* bits 8..15 */
#define SK_LSTM_GMIN(g) (((g) & 0xff) << SK_LSTM_GMIN_SHIFT)
#define SK_LSTM_BF16 (1 << 16)
#define SK_LSTM_BWD_EXCLUSIVE (1 << 17)
#define SK_LSTM_MAP_SHIFT 18 /* bits 18..19 */
#define SK_LSTM_MAP(m) (((m) & 3) << SK_LSTM_MAP_SHIFT)
#define SK_LSTM_POLL1 (1 << 20)
#define SK_LSTM_REPFLAGS (1 << 21)
#define SK_LSTM_FLAG_PER_LINE (1 << 22)
#define SK_LSTM_DELAY_SHIFT 23 /* bits 23..27 */
#define SK_LSTM_DELAY(d) (((d) & 31) << SK_LSTM_DELAY_SHIFT)
#define SK_LSTM_DELAY_NONE 31
#define SK_LSTM_SPLIT3 (1 << 28)
#define SK_LSTM_TAGGED (1 << 29)
#define SK_LSTM_XL8 (1 << 30)
size_t sk_lstm_workspace_bytes(int T, int B, int H);
int sk_lstm_fwd(const float* gx, const float* whh, const float* h0, const float* c0, const int32_t* lens,
                const int32_t* offs, float* y, float* gates, float* cs, float* hn, float* cn, void* ws,
                int T, int B, int H, int mode, sk_stream_t stream);
/* Backward of the recurrence.  mode: the SK_LSTM_* word above, read as its BACKWARD notes say.
 * dy (T,B,2H) is the gradient of the layer output, dhn / dcn (2,B,H; either may be NULL = 0)
 * the gradient wrt the final state (the RSH arch carries the hidden state from pass to pass, reference archs/RSH.py:172);
 * produces dgx (T,B,2,4H) = gradient of the gate pre-activations (gate-interleaved like gx; padded layout: zero at padded
 * positions), from which the caller forms dW_ih, dW_hh (with sk_hprev_rows), db and dx with the GEMMs, and dh0/dc0
 * (2,B,H; may be NULL).  gates / cs are what sk_lstm_fwd saved; dgx may alias gates (each cell is read, then
 * overwritten, by the same lane).  Optional by-products that spare the caller a pass over dgx each:
 *   dbias    (ceil(B/16), 2, 4H)  partial sums of dG over (t, b), one row per 16-row batch group block of the
 *            grid (unused rows are 0): their column sum is the gradient of b_ih and of b_hh;
 *   dgx_bf16 (the bf16 configuration) dgx a second time as bf16, dgx_bf16[row ld_bf16 + d 4H + 4u + g]: the row-major
 *            operand copy the layer's data- and weight-gradient products read, so that no cast pass over dgx runs between
 *            the recurrence and those products.  ld_bf16 >= 8H, a multiple of 4; only the rows x 8H entries are written:
 *            padding columns / rows a product expects to be zero are the caller's.
 *            plane_bf16 = 0: that one rounded copy.  plane_bf16 > 0 (the fp32 configuration, r06): dgx_bf16 receives THREE planes
 *            plane_bf16 elements apart -- the exact hi / mid / lo bf16 pieces of every dgx value (x = hi + mid + lo, see
 *            sk_gemm_f32_splitk variant 0), split ONCE here by the lane that computed the value: the operand sk_gemm_pl3_tn reads. */
int sk_lstm_bwd(const float* dy, const float* dhn, const float* dcn, const float* whh, const float* gates,
                const float* cs, const float* c0, const int32_t* lens, const int32_t* offs, float* dgx, float* dh0,
                float* dc0, float* dbias, void* dgx_bf16, int ld_bf16, int64_t plane_bf16, void* ws, int T, int B, int H,
                int mode, sk_stream_t stream);
/* Reorder the rows of a (nblk * 4H, C) matrix between torch's gate-major order (row g H + u inside each block of 4H
 * rows) and the gate-interleaved order of gx / gates / dgx (row 4u + g).  back = 0: dst[4u+g] = src[gH+u] (weights,
 * biases -> interleaved); back = 1: dst[gH+u] (+)= src[4u+g] (weight gradients back to the parameter order,
 * optionally accumulating).  Rows are ld_src / ld_dst floats apart (>= C); without `accumulate`, columns C..ld_dst-1
 * of the destination are zeroed, so a copy with a padded leading dimension (257 -> 260: 16-byte aligned rows for
 * the GEMMs) is made in the same pass.  dbias of sk_lstm_bwd is already gate-major. */
int sk_gate_rows(const float* src, float* dst, int nblk, int H, int C, int ld_src, int ld_dst, int back, int accumulate,
                 sk_stream_t stream);
/* What the calling thread's LAST sk_lstm_fwd / sk_lstm_bwd call launched (tests/test_gpu_lstm_choice.py pins it case by case,
 * tests/test_gpu_census.py generates DESIGN.md's kernel census from it).  Returns the number of kernel launches the call made
 * (1 persistent; T per step, + 1 for the backward's dh0 / dc0 product; 0 before the first call or when the call returned an
 * argument error) and fills out[SK_LSTM_Q_*]; a thread-local read-back like sk_gemm_last_kernel(). */
#define SK_LSTM_Q_FAMILY 0    /* SK_LSTM_K_* below; with KS, BF16, PACKED (and GM) it names the template instantiation */
#define SK_LSTM_Q_KS 1        /* 16-unit groups per direction: 20, 38 (fp32) / 40 (bf16, split3), 56, 64 */
#define SK_LSTM_Q_BF16 2
#define SK_LSTM_Q_PACKED 3    /* the call passed `offs` */
#define SK_LSTM_Q_GM 4        /* lstm_bwd_kernel's batch groups a workgroup MAY carry, 1 or 8 (0 for every other family) */
#define SK_LSTM_Q_EXCLUSIVE 5 /* the call asked for SK_LSTM_BWD_EXCLUSIVE */
#define SK_LSTM_Q_BLOCKS 6    /* workgroups per launch */
#define SK_LSTM_Q_G 7         /* batch groups a workgroup carries */
#define SK_LSTM_K_FWD 1        /* lstm_fwd_kernel<KS, BF16, 8, false, PACKED> */
#define SK_LSTM_K_FWD_SPLIT3 2 /* lstm_fwd_kernel<KS, false, 8, true, PACKED> */
#define SK_LSTM_K_FWD_XL8 3    /* lstm_fwd_xl8_kernel<56, PACKED> */
#define SK_LSTM_K_BWD 4        /* lstm_bwd_kernel<KS, BF16, GM> */
#define SK_LSTM_K_BWD_XL8 5    /* lstm_bwd_xl8_kernel<56> */
int sk_lstm_last_launch(int out[8]);
/* Word 0 of the workspace is a STICKY status word: a launch whose bounded spin gave up sets it (no launch clears
 * it; allocate the workspace zeroed).  Its address can be handed to sk_grad_norm as `guard` (as a float: any
 * non-zero bit pattern counts) so that a failed launch never reaches the weights, without a host sync per step.
 * sk_lstm_status: 0, or SK_ETIMEOUT if a launch since the last call timed out (reads the word back to the host,
 * synchronises the stream, clears the word). */
int sk_lstm_status(void* ws, sk_stream_t stream);
/* dst (R_pad, ld_dst) = src (R, C; rows ld_src floats apart) with columns C..ld_dst-1 and rows R..R_pad-1 zero: the copy of
 * the F = 257 input features with rows padded to 260 floats (16-byte aligned rows for both operands of the layer-0 products)
 * and the row count rounded up to whole K steps of the weight-gradient product. */
int sk_pad_rows(const float* src, int64_t R, int C, int ld_src, float* dst, int ld_dst, int64_t R_pad, sk_stream_t stream);
/* ---------------------------------------------------------------- BatchNorm1d over (rows, C)
 * Replaces nn.BatchNorm1d(2H) on (B, 2H, T) (reference archs/uPIT.py:119,135-138): statistics over
 * ALL count = B*T_max positions, zero-padded frames included.
 * stats: mean[c], var[c] (biased, two-pass) over `count` rows of which the first R are stored in x and the other
 * count - R are zero rows that are not (packed rows: count = B*T_max, R = sum(lens); padded: count = R);
 * ws >= sk_bn_workspace_bytes(R,C). */
size_t sk_bn_workspace_bytes(int R, int C);
int sk_bn_stats(const float* x, int R, int C, int64_t count, float* mean, float* var, void* ws, sk_stream_t stream);
/* running = (1-momentum)*running + momentum*batch (var unbiased, count/(count-1)), as torch does.  guard (may be NULL):
 * a device word, non-zero = leave the running statistics alone (the recurrence's sticky status word, sk_lstm_status:
 * after a timed-out launch the batch statistics are garbage and must not reach a checkpoint). */
int sk_bn_update_running(const float* mean, const float* var, float* running_mean, float* running_var,
                         int64_t count, int C, float momentum, const void* guard, sk_stream_t stream);
/* out = (x - mean) / sqrt(var + eps) * gamma + beta */
int sk_bn_apply(const float* x, const float* mean, const float* var, const float* gamma, const float* beta,
                float* out, int R, int C, float eps, sk_stream_t stream);
/* BatchNorm folded into the Linear layer that follows it (lin(bn(x)), reference archs/uPIT.py:138-141; SURVEY 2.3 K4:
 * "normalize fused into the Linear prologue"): with s = gamma / sqrt(var + eps), t = beta - mean * s,
 *   Wf[o][c] = W[o][c] * s[c]  (leading dimension ldf >= C, extra columns zero),  bf[o] = b[o] + sum_c W[o][c] * t[c],
 * so that lin(bn(x)) = x Wf^T + bf and the normalised activations are never written.  s and t (C each) are returned for
 * sk_bn_unfold_grad: the weight gradient dW (+)= (dz^T x) diag(s) + colsum(dz) t^T from G = dz^T x (O x C, ld ldg). */
int sk_bn_fold(const float* W, const float* b, const float* mean, const float* var, const float* gamma, const float* beta,
               float eps, int O, int C, float* Wf, int ldf, float* bf, float* s, float* t, sk_stream_t stream);
int sk_bn_unfold_grad(const float* G, int ldg, const float* dzsum, const float* s, const float* t, float* dW, int O, int C,
                      int accumulate, sk_stream_t stream);
/* training-mode backward: dgamma, dbeta, dx from dout, x and the batch statistics */
int sk_bn_bwd(const float* dout, const float* x, const float* mean, const float* var, const float* gamma,
              float* dx, float* dgamma, float* dbeta, void* ws, int R, int C, float eps, sk_stream_t stream);
/* The same in two halves, for BatchNorm statistics shared by several devices (data-parallel "sync" option): local
 * column sums dbeta = sum dy, dgamma = sum dy*xhat, then -- after the caller has summed them over the devices --
 * dx from the global sums; `count` = rows that mean / var and the sums cover (all devices). */
int sk_bn_bwd_sums(const float* dout, const float* x, const float* mean, const float* var, float* dgamma,
                   float* dbeta, void* ws, int R, int C, float eps, sk_stream_t stream);
int sk_bn_bwd_apply(const float* dout, const float* x, const float* mean, const float* var, const float* gamma,
                    const float* dgamma, const float* dbeta, float* dx, int R, int C, double count, float eps,
                    sk_stream_t stream);

/* out[c] (+)= sum_r x[r*ld + c]   (bias gradients); ws >= sk_bn_workspace_bytes(R,C) */
int sk_colsum(const float* x, int R, int C, int ld, float* out, int accumulate, void* ws, sk_stream_t stream);
/* dz = dmask * m * (1 - m)   (sigmoid backward, reference archs/uPIT.py:144) */
int sk_sigmoid_bwd(const float* dmask, const float* m, float* dz, int64_t n, sk_stream_t stream);

/* ---------------------------------------------------------------- PIT-MSE loss
 * Replaces the loss body of compute_loss (reference archs/uPIT.py:181-197,206).
 *   mask (T,B,S*F), mix (T,B,F), src_host[s] -> (T,B,F) device pointers (host array of S), lens (B);
 *   with offs != NULL all of them are packed rows (R, .) -- PackedSequence.data as the collator built it
 *   pair_sse (B,S,S): pair[b][s][r] = sum_{t,f} (mask[t,b,s,f]*mix[t,b,f] - src_r[t,b,f])^2
 *   perm_loss (S!,B) in itertools.permutations order; best_perm (B) = argmin (first minimum)
 *   out[0] = loss/norm, out[1] = norm = sum(lens)*F, out[2] = sum_b min loss / S
 * norm_dev (device scalar, may be NULL) replaces norm when given: data-parallel training divides by the
 * GLOBAL norm, all-reduced on the device without a host round trip. */
size_t sk_pit_workspace_bytes(int T, int B, int S);
int sk_pit_mse_fwd(const float* mask, const float* mix, const float* const* src_host, const int32_t* lens,
                   const int32_t* offs, int T, int B, int F, int S, const float* norm_dev, float* pair_sse,
                   float* perm_loss, int32_t* best_perm, float* out, void* ws, sk_stream_t stream);
/* dmask = gscale[0] * 2 * (mask*mix - src_{best_perm[b][s]}) * mix / (S * norm), norm = out[1]; nrows = packed rows R
 * (ignored when offs == NULL) */
int sk_pit_mse_bwd(const float* mask, const float* mix, const float* const* src_host,
                   const int32_t* best_perm, const float* out, const float* gscale, const int32_t* offs, int64_t nrows,
                   int T, int B, int F, int S, float* dmask, sk_stream_t stream);

/* ---------------------------------------------------------------- SI-SDR uPIT loss (waveform domain)
 * A second training loss beside PIT-MSE: utterance-level PIT on the negative SI-SDR of the time-domain estimates
 * e_s = istft(mask_s * STFT(mix)) against the source waveforms.  No counterpart in the reference (its only loss is the
 * magnitude MSE above); the metric is sepkern/sisdr.py's, which also restates the arithmetic below in numpy fp64.
 * Three entry points, all on PACKED rows (offs as under "packed rows": row of (t, j) = offs[t] + j; utterance j has
 * T_j = nframes[j] frames and L_j = hop * (T_j - 1) output samples; n_fft = 512, hop = 128 only; 1 <= S <= 4):
 *
 * sk_mask_istft_rows: sk_mask_istft's arithmetic (same frames, same overlap-add order, same window-sum-square division,
 *   same trim) with the spectra read from rows: mix_rows_c64 (R, 257) complex64, mask (R, ld >= S*257) float32 with source s
 *   in columns s*257 .. s*257+256.  Estimate s of utterance j: L_j float32 samples at wav_out + out_offs[j*S + s].
 *   max_frames >= max_j T_j sizes the grid. */
int sk_mask_istft_rows(const void* mix_rows_c64, const float* mask, int ld, const int32_t* offs, const int32_t* nframes,
                       int B, int S, int n_fft, int hop, float* wav_out, const int64_t* out_offs, int max_frames,
                       sk_stream_t stream);
/* sk_sisdr_pit_fwd: est as sk_mask_istft_rows wrote it (est_offs[j*S + k]); reference i of utterance j = nsamp[j] samples at
 *   ref + ref_offs[j*S + i] (elements; float32, or int16 PCM scaled by 1/32768 when pcm16 != 0 -- sk_stft's convention);
 *   nsamp[j] = L_j samples of both are read.  From the plain sums sum e, sum r, sum e^2, sum r^2, sum e r (fp64, fixed order,
 *   no atomics: bitwise reproducible, and an utterance's numbers do not depend on what else is in the batch) the zero-mean
 *   a = <e~,r~>, b = <r~,r~>, c = <e~,e~> and
 *     pair (B,S,S): pair[j][k][i] = SI-SDR(e_k, r_i) = 10 log10(((a/b) a + eps) / (c - (a/b) a + eps)) dB, eps = 1e-30
 *                   (b <= 0, a silent reference: the projection is 0 and the value the finite 10 log10(eps / (c + eps)))
 *     perm_score (S!,B) in itertools.permutations order: (1/S) sum_k pair[j][k][p(k)];  best_perm (B) = argMAX (first maximum)
 *     out[0] = loss = -(1/count) sum_j best score, out[1] = count, out[2] = sum_j best score;  count = B, or count_dev[0]
 *              (device scalar, may be NULL: the GLOBAL utterance count of a data-parallel step)
 *     coef (B,S,3): A, B, C of d loss / d e_k[n] = A e_k[n] + B r_i[n] + C, i = the best permutation's reference for k
 *              (r in its scaled units), i.e. -(1/(count S)) kappa (2 r~/a - 2 (e~ - (a/b) r~)/(c - a^2/b)), kappa = 10/ln 10;
 *              0, 0, 0 for a pair with b <= 0, a == 0 or c - a^2/b <= 0 (silent source, exact copy): never NaN or Inf.
 *   max_samples >= max_j nsamp[j] sizes the grid; ws >= sk_sisdr_workspace_bytes(B, S, max_samples) (0 for bad arguments). */
size_t sk_sisdr_workspace_bytes(int B, int S, int max_samples);
int sk_sisdr_pit_fwd(const float* est, const int64_t* est_offs, const void* ref, int pcm16, const int64_t* ref_offs,
                     const int32_t* nsamp, int B, int S, int max_samples, const float* count_dev, float* pair,
                     float* perm_score, int32_t* best_perm, float* out, float* coef, void* ws, sk_stream_t stream);
/* sk_sisdr_mask_grad: dmask = gscale[0] * d loss / d mask, the gradient above taken back through the overlap-add, the
 *   inverse FFT and the mask product in ONE kernel.  The adjoint of mask-apply + iSTFT is a forward STFT of another signal:
 *   g_k[p] = (A e_k[n] + B r_i[n] + C) * gscale / wss[p] at p = n + n_fft/2, n in [0, L_j), zero elsewhere (formed by the sample
 *   loader; wss = the forward's window-sum-square), framed WITHOUT reflection, U_k[t][f] = sum_n w[n] g_k[t hop + n] e^(-2 pi i f n / n_fft),
 *     dmask[offs[t] + j][k*257 + f] = (c_f / n_fft) (Re X[t][f] Re U_k[t][f] + Im X[t][f] Im U_k[t][f]),  c_f = 1 for f in {0, 256}, else 2,
 *   X = mix_rows_c64, contracted in the epilogue and stored from registers: neither g nor U exists in memory.
 *   dmask (>= R, ld >= S*257): only rows offs[t] + j, t < T_j, columns < S*257 are written. */
int sk_sisdr_mask_grad(const float* est, const int64_t* est_offs, const void* ref, int pcm16, const int64_t* ref_offs,
                       const int32_t* nframes, const int32_t* best_perm, const float* coef, const float* gscale,
                       const void* mix_rows_c64, const int32_t* offs, int B, int S, int n_fft, int hop, int max_frames,
                       float* dmask, int ld, sk_stream_t stream);

/* ---------------------------------------------------------------- mixture-invariant loss (waveform domain, loss=mixit)
 * Unsupervised training (MixIT, Wisdom et al., NeurIPS 2020): the training mixture is the sum of TWO recordings x_0, x_1, the
 * network emits M masks, 2 <= M <= 4, and the loss asks only that SOME assignment of the M time-domain estimates
 * e_k = istft(mask_k * STFT(mix)) to the two recordings sums to them.  No counterpart in the reference; sepkern/mixit.py states
 * the definition and restates the arithmetic below in numpy fp64.  The estimates are sk_mask_istft_rows' (above, S = M).
 *
 * sk_mixit_fwd: est as sk_mask_istft_rows wrote it (est_offs[j*M + k]); reference n of utterance j = nsamp[j] samples at
 *   ref + ref_offs[j*2 + n] (elements; float32, or int16 PCM scaled by 1/32768 when pcm16 != 0); nsamp[j] = L_j samples of both
 *   are read.  From the plain sums P_n = sum x_n^2, c_nk = sum x_n e_k, G_kl = sum e_k e_l (no mean removal; fp64, fixed order,
 *   no atomics: bitwise reproducible, and an utterance's numbers do not depend on what else is in the batch), for every code
 *   a in [0, 2^M) -- bit k of a = the reference that estimate k is added to; every code is legal, an empty group included --
 *     err_n(a)   = max(P_n - 2 sum_{k in n} c_nk + sum_{k,l in n} G_kl, 0)          (= |x_n - sum_{k in n} e_k|^2)
 *     score_n(a) = 10 log10((P_n + eps) / (err_n(a) + tau P_n + eps)) dB,  eps = 1e-30,  tau = 10^(-snr_max / 10)
 *     assign_score (2^M,B): assign_score[a][j] = (score_0(a) + score_1(a)) / 2;   best_code (B) = argMAX (first maximum)
 *     out[0] = loss = -(1/count) sum_j best score, out[1] = count, out[2] = sum_j best score;  count = B, or count_dev[0]
 *              (device scalar, may be NULL: the GLOBAL utterance count of a data-parallel step)
 *     coef (B,2): D_0, D_1 of d loss / d e_k[t] = D_n (m_n[t] - x_n[t]), n = bit k of the best code, m_n = sum_{l in n} e_l:
 *              D_n = kappa / (count (err_n + tau P_n + eps)), kappa = 10/ln 10; 0 where err_n + tau P_n <= 0 (a silent
 *              reference met exactly): never NaN or Inf.
 *   max_samples >= max_j nsamp[j] sizes the grid; ws >= sk_mixit_workspace_bytes(B, M, max_samples) (0 for bad arguments). */
size_t sk_mixit_workspace_bytes(int B, int M, int max_samples);
int sk_mixit_fwd(const float* est, const int64_t* est_offs, const void* ref, int pcm16, const int64_t* ref_offs,
                 const int32_t* nsamp, int B, int M, int max_samples, const float* count_dev, double tau,
                 float* assign_score, int32_t* best_code, float* out, float* coef, void* ws, sk_stream_t stream);
/* sk_mixit_mask_grad: dmask = gscale[0] * d loss / d mask, as sk_sisdr_mask_grad takes its gradient back (one kernel: the
 *   adjoint of mask-apply + iSTFT is a forward STFT of the gradient signal).  The signal is the SAME for every estimate of a
 *   group, so ONE transform per (utterance, reference n) serves the column blocks of all members:
 *   g_n[p] = D_n gscale (sum_{l in n} e_l[t] - x_n[t]) / wss[p] at p = t + n_fft/2, t in [0, L_j), zero elsewhere (the member
 *   sum in fp32, l ascending from the first member), framed WITHOUT reflection, U_n its windowed transform,
 *     dmask[offs[t] + j][k*257 + f] = (c_f / n_fft) (Re X[t][f] Re U_n[t][f] + Im X[t][f] Im U_n[t][f])  for every k in group n,
 *   c_f = 1 for f in {0, 256}, else 2, X = mix_rows_c64.  An empty group launches no work.  The groups partition the estimates:
 *   every column < M*257 of every row offs[t] + j, t < T_j, is written exactly once, by one lane; nothing else is written
 *   (dmask (>= R, ld >= M*257)).  The column blocks of one group hold the same bits. */
int sk_mixit_mask_grad(const float* est, const int64_t* est_offs, const void* ref, int pcm16, const int64_t* ref_offs,
                       const int32_t* nframes, const int32_t* best_code, const float* coef, const float* gscale,
                       const void* mix_rows_c64, const int32_t* offs, int B, int M, int n_fft, int hop, int max_frames,
                       float* dmask, int ld, sk_stream_t stream);

/* ---------------------------------------------------------------- deep clustering (loss=dpcl; k-means masks)
 * A second way to separate beside uPIT (Hershey et al. 2016; the low-rank objective of Isik et al. 2016; the sigmoid + unit-norm
 * embedding and the magnitude-ratio weights of Wang et al. 2018): the network emits a D-dimensional embedding per
 * time-frequency point, the loss pulls the embeddings of points dominated by the same source together, and k-means on the
 * embeddings gives the masks.  No counterpart in the reference; sepkern/dpcl.py states the definition and restates the
 * arithmetic below in numpy fp64.
 * All three entry points work on PACKED rows ("packed rows" above: row of (t, j) = offs[t] + j, lens sorted descending, lens[0]
 * = T).  z (R, ld >= F*D) float32: dimension d of bin f in column d*F + f (D planes of F columns); mix and the S sources
 * src_host[s] (a host array of device pointers) are (R, F) contiguous.  A point i = (row, bin); utterance j has lens[j] * F
 * points, numbered t*F + f.  v_i = (z[row][d*F + f])_d, u_i = v_i / |v_i| (0 for a zero vector; fp32, d ascending).
 *
 * sk_dpcl_fwd:  y_i = the first maximum of src_s[row][f] over s;  weights before normalisation w'_i = mix_i (weight =
 *   SK_DPCL_MR) or [mix_i > thr_j] (SK_DPCL_VAD), thr_j = vad_ratio * max_{i in j} mix_i, ONE fp32 product;  w_i = w'_i / sum_j w'
 *   (0 for an utterance whose weights are all zero).  With the rows sqrt(w'_i) [u_i | onehot(y_i)] the Gram matrix holds
 *     A = U^T W U (D x D),  Bm = U^T W Y (D x S),  C = Y^T W Y (diagonal),   L_j = |A|_F^2 - 2 |Bm|_F^2 + |C|_F^2
 *   Launch (1) (SK_DPCL_VAD: two launches before it form thr): (utterance, chunk of 8 of ITS frames), tiles of 64 points; the
 *   exact-fp32 MFMA sums four points per instruction (fp32 products, an fp32 chain of four), every such sum is added in fp64;
 *   one fp64 partial per chunk in a fixed slot of ws; (2) per utterance the chunks added in ascending order in fp64, the
 *   normaliser 1 / tr C applied, L_j;  (3) the batch output.
 *     lj (B) fp64 = L_j;  out[0] = loss = (1/count) sum_j L_j, out[1] = count, out[2] = sum_j L_j (j ascending, fp64);  count = B, or
 *     count_dev[0] (device scalar, may be NULL: the GLOBAL utterance count of a data-parallel step)
 *     ab (B, 40*40 + 40*4) float32 = A (pitch 40) and Bm (pitch 4) of every utterance, zero-padded;  stats (B, 2) = 1 / sum w', thr
 * sk_dpcl_bwd:  dz = gscale[0] / out[1] * dL_j/dz on the rows and columns of the batch -- one point per lane,
 *     g_i = 4 w_i (A u_i - Bm[:, y_i]),   dL/dv_i = (g_i - u_i (u_i . g_i)) / |v_i|   (0 for a zero vector or a zero weight)
 *   from ab, stats and out as sk_dpcl_fwd left them; w_i and y_i are recomputed.  Only rows offs[t] + j, t < lens[j], columns
 *   < F*D of dz (>= R, ld) are written, each exactly once.
 * sk_dpcl_kmeans:  per utterance, S clusters on u_i.  A point is ACTIVE when mix_i > thr_j (above) and then weighs mix_i.
 *   Initialisation (skipped with centroids_in (B, S, D) float32): centroid 0 = the active point of largest mix; centroid k = the
 *   active point whose least squared distance to the centroids before k is largest; ties to the lowest point index; with at
 *   most k active points centroid k copies centroid 0 (zeros without any active point).  `iterations` >= 0 Lloyd steps: every
 *   point to the centroid of least squared distance (fp32, d ascending; ties to the lowest k), every centroid to the weighted
 *   mean of its active members (the loss's sums: four points per MFMA in fp32, added in fp64; a cluster without active member
 *   keeps its centroid).  Then one final assignment:  labels (R, F) int32;  mask (R, ld_mask >= S*F): mask[row][k*F + f] = 1.0 where the
 *   label is k, else 0.0 -- the layout of the uPIT masks;  centroids (B, S, D) float32.  Two launches for thr, two per centroid,
 *   two per iteration, one for the assignment; no host synchronisation, no hand-off between workgroups.
 * No atomics, every sum in one fixed order, chunk boundaries a function of the utterance's own length: bitwise reproducible,
 * the bits do not depend on ld, and an utterance's numbers do not depend on the batch around it.  Nothing outside the rows
 * and columns named above is read or written.  SK_EINVAL before anything is launched: D outside 1..40, S outside 1..4 (2..4 for
 * k-means), F, T or B < 1, B > 65535, ld < F*D, ld_mask < S*F, iterations < 0, vad_ratio outside [0, 1], a weight other than
 * the two, a NULL pointer.  ws >= sk_dpcl_workspace_bytes / sk_dpcl_kmeans_workspace_bytes (0 for arguments out of range). */
#define SK_DPCL_MR 0
#define SK_DPCL_VAD 1
size_t sk_dpcl_workspace_bytes(int T, int B, int F, int D, int S);
int sk_dpcl_fwd(const float* z, int ld, const float* mix, const float* const* src_host, const int32_t* lens,
                const int32_t* offs, int T, int B, int F, int D, int S, int weight, float vad_ratio, const float* count_dev,
                double* lj, float* ab, float* stats, float* out, void* ws, sk_stream_t stream);
int sk_dpcl_bwd(const float* z, int ld, const float* mix, const float* const* src_host, const int32_t* lens,
                const int32_t* offs, int T, int B, int F, int D, int S, int weight, const float* ab, const float* stats,
                const float* out, const float* gscale, float* dz, sk_stream_t stream);
size_t sk_dpcl_kmeans_workspace_bytes(int T, int B, int F, int D, int S);
int sk_dpcl_kmeans(const float* z, int ld, const float* mix, const int32_t* lens, const int32_t* offs, int T, int B, int F, int D,
                   int S, int iterations, float vad_ratio, const float* centroids_in, float* mask, int ld_mask, int32_t* labels,
                   float* centroids, void* ws, sk_stream_t stream);

/* ---------------------------------------------------------------- phase-sensitive uPIT targets (loss=psa / tpsa)
 * The targets of the phase-sensitive approximation loss (sepkern/psa.py states the definition and restates it in numpy fp64),
 * made from the batch's waveforms in ONE launch: with Y the mixture's STFT and S_s source s's, both as sk_stft defines them,
 *   mix_rows[row][f]            = |Y[t][f]|                               (the bits sk_stft's magnitude output has)
 *   targets[s*plane + row*ld+f] = (Re S_s Re Y + Im S_s Im Y) / |Y|  = |S_s| cos(theta_s - theta_Y),
 * 0 where the fp32 |Y|^2 < 2^-100; clamp != 0 holds the target to [0, |Y|] (the truncated form).  The PIT-MSE kernels above
 * take these rows in place of the source magnitudes.  The sources' spectra never exist in memory; the mixture's passes through
 * ws (below) on its way from the lane that formed a bin to the same lane's S contractions.
 * Signal q (0 = mixture, 1 + s = source s) of utterance u: nsamp[u] samples at wav + sig_offs[q*B + u] (elements; float32, or
 * int16 PCM scaled by 1/32768 when pcm16 != 0), T_u = 1 + nsamp[u]/hop frames.  Row of frame t of utterance u:
 *   offs != NULL:     offs[t] + u        (packed rows of a length-sorted batch, row_base NULL)
 *   row_base != NULL: row_base[u] + t    (per-utterance blocks of (T_u, ld), offs NULL)
 * Rows are ld >= 257 floats with unit bin stride; mix_rows and every target plane share ld.  Only the rows of existing frames
 * and columns < 257 are written, each element by one lane in a fixed order: bitwise reproducible, and an utterance's numbers
 * do not depend on the batch around it.  ws: work rows, 257 * 8 bytes for every row the launch addresses (rows 0 .. R-1 of the
 * packed batch, or 0 .. sum_u T_u - 1), contents undefined afterwards.  min_samples <= min_u nsamp[u] must exceed n_fft/2 (reflect padding), max_frames >=
 * max_u T_u sizes the grid; n_fft = 512, hop = 128 only; 1 <= S <= 4; B <= 65535. */
int sk_stft_psa(const void* wav, int pcm16, const int64_t* sig_offs, const int32_t* nsamp, int B, int S, int n_fft, int hop,
                int clamp, const int32_t* offs, const int64_t* row_base, float* mix_rows, float* targets, int ld, int64_t plane,
                void* ws, int min_samples, int max_frames, sk_stream_t stream);

/* ---------------------------------------------------------------- inter-channel phase features (conf key ipd_channels)
 * The input rows of a network that sees an array (sepkern/ipd.py states the definition and restates it in numpy fp64): with Y_r
 * the reference channel's STFT and Y_c listed channel c's, both as sk_stft defines them, P = number of listed channels (1..7),
 *   rows[row*ld + f]                  = |Y_r[t][f]|                                  (the bits sk_stft's magnitude output has)
 *   rows[row*ld + 257 (1 + 2p) + f]   = Re(Y_c conj Y_r) / (|Y_c| |Y_r|) = cos(theta_c - theta_r),   c = listed channel p
 *   rows[row*ld + 257 (2 + 2p) + f]   = Im(Y_c conj Y_r) / (|Y_c| |Y_r|) = sin(theta_c - theta_r)
 * cos and sin both 0 where the fp32 |Y_c|^2 or |Y_r|^2 is below 2^-100.  In fp32, with (a, b) = (Re, Im): the numerators are
 * fma(a_c, a_r, b_c b_r) and fma(b_c, a_r, -(a_c b_r)), a squared magnitude is fma(a, a, b b), and the feature is
 * (numerator * rsq(|Y_c|^2)) * rsq(|Y_r|^2): every rounding is fixed, and both entry points give the same bits on the same spectra.
 * Rows are ld >= 257 (1 + 2P) floats; the columns behind the features up to the next multiple of 16 (or to ld, if that is
 * nearer) are stored as zeros and nothing behind those is touched: with ld = the width rounded up to 16 a row is what the
 * engine's first layer reads.  Each element is written by one lane; vector stores only; bitwise reproducible.
 *
 * sk_stft_ipd (training): one launch from the batch's waveforms to the rows.  Signal q (0 = the reference channel, 1 + p =
 * listed channel p) of utterance u: nsamp[u] samples at wav + sig_offs[q*B + u] (elements; float32, or int16 PCM scaled by
 * 1/32768 when pcm16 != 0), T_u = 1 + nsamp[u]/hop frames; C = 1 + P signals per utterance, 2..8.  Row of frame t of
 * utterance u: offs[t] + u (packed rows of a length-sorted batch, row_base NULL) or row_base[u] + t (per-utterance blocks,
 * offs NULL).  Only the rows of existing frames are written; an utterance's numbers depend on neither the batch around it nor
 * the sample format.  mix_rows (may be NULL): a contiguous (rows, 257) copy of the magnitude columns, for the loss kernels,
 * which take the mixture without a row stride.  ws: work rows, 257 * 8 bytes for every row the launch addresses, contents
 * undefined afterwards (the reference's bins on their way from the lane that formed them to the same lane's P contractions).
 * min_samples <= min_u nsamp[u] must exceed n_fft/2, max_frames >= max_u T_u sizes the grid; n_fft = 512, hop = 128; B <= 65535.
 *
 * sk_ipd_rows (inference): the same features from spectra in memory.  Y: complex64, element (c, t, f) at
 * Y[c*y_chan_stride + t*y_row_stride + f] (elements, y_row_stride >= 257), C channels (2..8), T frames; chans_host: host array
 * of the P listed channels, each in [0, C), distinct and not ref.  mag (T, ld_mag >= 257): the magnitude rows of the reference
 * channel as the caller already holds them (sk_stft's magnitude output, sk_wpe's mag_out); they are COPIED into columns
 * 0..256, so an IPD model's first 257 inputs are the bits a single-channel model gets.  Row t of rows is frame t.
 * Both return SK_EINVAL (with a text for sk_last_error) for arguments outside the above. */
int sk_stft_ipd(const void* wav, int pcm16, const int64_t* sig_offs, const int32_t* nsamp, int B, int C, int n_fft, int hop,
                const int32_t* offs, const int64_t* row_base, float* rows, int ld, float* mix_rows, void* ws, int min_samples,
                int max_frames, sk_stream_t stream);
int sk_ipd_rows(const void* Y_c64, int64_t y_chan_stride, int64_t y_row_stride, int T, int C, int ref, const int32_t* chans_host,
                int P, const float* mag, int ld_mag, float* rows, int ld, sk_stream_t stream);

/* ---------------------------------------------------------------- RSH arch (reference archs/RSH.py)
 * One pass of the greedy source-assignment loss (archs/RSH.py:225-244): mask (T,B,F); x (T,B,ldx) whose
 * first F columns are the mixture; src_host[r] -> (T,B,F), r < S (host array of device pointers).
 *   sse (S,B) raw per-source SSE of mask*mix; used (S,B) int32 in/out: sources already assigned to row b are
 *   excluded; sel (B) = chosen source (first minimum), which is then marked used;
 *   out[0] = sum_b min / S (this pass's loss term), out[1] = sum(lens)*F (its norm term). */
size_t sk_rsh_workspace_bytes(int T, int B, int S);
int sk_rsh_loss_fwd(const float* mask, const float* x, int ldx, const float* const* src_host, const int32_t* lens,
                    int T, int B, int F, int S, int32_t* used, float* sse, int32_t* sel, float* out, void* ws,
                    sk_stream_t stream);
/* dmask = gscale[0] * (2/S) * (mask*mix - src_{sel[b]}) * mix */
int sk_rsh_loss_bwd(const float* mask, const float* x, int ldx, const float* const* src_host, const int32_t* sel,
                    const float* gscale, int T, int B, int F, int S, float* dmask, sk_stream_t stream);
/* Attention update between passes (archs/RSH.py:254-257 / :278-281): x_out = act(x_in - [0 | mask]) on rows of
 * 2F = [mixture | attention]; act = relu when relu != 0 (training), identity otherwise (test). */
int sk_att_update(const float* x_in, const float* mask, float* x_out, int64_t rows, int F, int relu, sk_stream_t stream);
/* dx_in = dx_out * gate, dmask = -(dx_out * gate)[attention half], gate = (x_out > 0) with relu, 1 without */
int sk_att_update_bwd(const float* dx_out, const float* x_out, float* dx_in, float* dmask, int64_t rows, int F,
                      int relu, sk_stream_t stream);

/* ---------------------------------------------------------------- clip_grad_norm_ + Adam
 * Replaces torch.nn.utils.clip_grad_norm_(params, max_norm) + torch.optim.Adam.step()
 * (reference steps/train_qsub.py:121-122) on ONE flat fp32 buffer holding every parameter.
 *   scal[0] = total grad L2 norm, scal[1] = clip coefficient min(1, max_norm/(norm+1e-6)),
 *   scal[2] = 1 when this step is skipped, scal[3] = count of skipped steps (caller zeroes scal once).
 * guard (may be NULL): device float; non-zero means "the gradients of this step are not to be trusted" (a
 * persistent recurrence launch timed out, on this rank or -- summed by the data-parallel all-reduce -- on any
 * rank): sk_clip_adam then leaves parameters and moments untouched.
 * step is the 1-based count of sk_clip_adam calls; the bias corrections use step - scal[3], the number of updates
 * actually applied. ws >= sk_optim_workspace_bytes(n). */
size_t sk_optim_workspace_bytes(int64_t n);
int sk_grad_norm(const float* g, int64_t n, float max_norm, const float* guard, float* scal, void* ws,
                 sk_stream_t stream);
int sk_clip_adam(float* p, const float* g, float* m, float* v, int64_t n, const float* scal,
                 float lr, float beta1, float beta2, float eps, int step, sk_stream_t stream);

/* ---------------------------------------------------------------- BSS Eval (scoring)
 * Replaces the per-utterance host computation of sepkern/bsseval.py (mir_eval.separation.bss_eval_sources' SDR /
 * SIR / SAR with a `taps`-long allowed-distortion filter; the reference's steps/evaluate_sources.py:57) for a batch of
 * U utterances of S sources each.  ref / est: packed fp64 rows; utterance u has length lens_host[u] and its source
 * (or estimate) i starts at element offs_host[u] + i*lens_host[u] of ref (est).  offs_host / lens_host are HOST arrays,
 * copied into the workspace on `stream`.  1 <= S <= 4, 1 <= taps <= 512, lengths >= 1; all arithmetic is fp64.
 * ws >= sk_bss_workspace_bytes(U, S, taps) (0 for arguments out of range).
 *
 * sk_bss_xcorr: the lag correlations alone, one record of X = P*(2*taps-1) + S*S*taps + S doubles per utterance at
 *   xc + u*X, P = S*(S+1)/2:  [c_ij[d] for pairs i <= j in order (0,0),(0,1)..(0,S-1),(1,1).., d = -(taps-1)..taps-1]
 *   [c_{r_i,e_k}[t], (i, k) row-major, t = 0..taps-1] [|e_k|^2, k = 0..S-1], with c_xy[d] = sum_m x[m] y[m+d].
 *   Direct sums in a fixed order, no atomics: bitwise reproducible and independent of the batch; exact (every
 *   product and partial sum representable) for 16-bit PCM scaled by 2^-15.
 * sk_bss_eval: correlations, the block-Toeplitz Gram matrix of the delayed references and each source's own block,
 *   their Cholesky factors (blocked, fp64 MFMA trailing update), forward substitution of the estimates' correlations
 *   and the energies |P_all e_k|^2, |P_j e_k|^2, |e_k|^2.  out (U, S, S, 3) fp64: [u][k][j] = SDR, SIR, SAR in dB of
 *   estimate k against true source j (a zero or negative denominator gives +inf).  status (U) int32: 0, or bit w set
 *   when the factorisation of system w (0: all sources, j >= 1: source j alone) met a pivot that is not finite or
 *   not above 2^-40 (~1e-12) times its diagonal entry (rank-deficient references): that utterance's numbers are not valid and
 *   the caller re-scores it on the host (sepkern/bsseval_gpu.py). */
size_t sk_bss_workspace_bytes(int U, int S, int taps);
int sk_bss_xcorr(const double* ref, const double* est, const int64_t* offs_host, const int32_t* lens_host, int U, int S,
                 int taps, void* ws, double* xc, sk_stream_t stream);
int sk_bss_eval(const double* ref, const double* est, const int64_t* offs_host, const int32_t* lens_host, int U, int S,
                int taps, void* ws, double* out, int32_t* status, sk_stream_t stream);

/* ---------------------------------------------------------------- STOI (scoring)
 * Short-time objective intelligibility (Taal et al. 2011) and its extended form ESTOI (Jensen & Taal 2016) as
 * sepkern/stoi.py defines them, for a batch of U utterances of S sources each: silent-frame removal decided by each
 * reference (fp64 frame energies, 40 dB), 15 one-third-octave band envelopes of the rebuilt signals (the 512-point FFT of the
 * STFT front end, fp32), and the correlations over segments of 30 frames (fp64).
 * ref / est: packed fp32 rows at 10 kHz in sk_bss_eval's layout: utterance u has length lens_host[u] and its source (or
 * estimate) i starts at element offs_host[u] + i*lens_host[u] of ref (est).  offs_host / lens_host are HOST arrays, copied into
 * the workspace on `stream`.  1 <= S <= 4, 1 <= lengths <= 2^24, 1 <= U <= 2^20.
 * out (U, S, S, 2) fp64: [u][k][j] = STOI, ESTOI of estimate k against reference j (under reference j's kept frames).
 * frames (U, S) int32: T of reference j, the frames left after silent-frame removal minus one; T < 30 gives 1e-5 for both
 * scores.  A signal without a frame (length <= 256) or an all-zero reference gives T = 0 and 1e-5: no error.
 * Every score is computed in one fixed order of operations by workgroups that see its own utterance alone: no atomics,
 * bitwise reproducible, independent of the batch.
 * ws >= sk_stoi_workspace_bytes(U, S, max_u lens_host[u]) (0 for arguments out of range).  Bad arguments return SK_EINVAL
 * before anything is launched. */
size_t sk_stoi_workspace_bytes(int U, int S, int max_len);
int sk_stoi(const float* ref, const float* est, const int64_t* offs_host, const int32_t* lens_host, int U, int S, void* ws,
            double* out, int32_t* frames, sk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
