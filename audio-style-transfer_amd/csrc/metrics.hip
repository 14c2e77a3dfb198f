// Spectrogram metrics of the reference's evaluation scripts for a padded batch of clips of different lengths:
//   mse_spectrogram (evaluation_reconstruction.py:105-118, after the truncation to a common length at :193-204): n_fft 1024, hop 256
//   instrumentation_similarity (evaluation_style_transfer.py:111-119): n_fft 2048, hop 512, band energies + Pearson's r
//   mfcc_distance (evaluation_style_transfer.py:99-109) and librosa.feature.mfcc itself: n_fft 2048, hop 256 or 512, Slaney mel
//     filter bank, power_to_db with top_db 80, orthonormal DCT-II -- the section "MFCC" below
// The first two are |STFT| (librosa.stft defaults: centred frames, periodic Hann) plus a reduction, so the spectrogram never exists in
// HBM: a workgroup transforms a frame in LDS with the front end's 1024-point network (fft1024.h), reduces what it needs and stores
// one partial per frame (MSE) or per run of frames (band energies) into the caller's workspace with ordinary stores.  A second
// small launch sums a clip's partials in a fixed order in double.  No atomics: every output element has one owner and a fixed
// order of summation, so the results are bit-reproducible.
//
// Per-clip sample counts are read from the device and clamped, as in the ragged front end (fft.hip); samples behind a clip's
// end are never read, and per frame the arithmetic does not depend on the batch around the clip.
#include "spec_common.h"

namespace {
constexpr int MSE_HOP = 256, MSE_BINS = 513;             // N_FFT / HOP_LENGTH of evaluation_reconstruction.py
constexpr int BE_HOP = 512;                              // librosa.stft's default at n_fft 2048
constexpr int BE_RUN = 5;                                // consecutive frames of one clip per workgroup (one partial per run)

// ---- mse_spectrogram: frames 2 blockIdx.x and 2 blockIdx.x + 1 of pair blockIdx.y.  One FFT per frame pair on average: two
// consecutive frames of ONE clip ride in the real and the imaginary part of a transform and are split by Hermitian symmetry,
// X0[k] = (Z[k] + conj Z[N-k]) / 2, X1[k] = (Z[k] - conj Z[N-k]) / 2i; the workgroup does that for `original`, keeps the 513 x 2
// magnitudes in registers, and then for `generated`.  The two clips of a pair so pass through the same arithmetic, and equal
// clips score exactly 0.  (Packing original + i generated into one transform instead leaves 2.5e-12 there, measured: |A| = |G|
// would need the network to commute with a multiplication by i, and the fused multiply-adds of its twiddle products do not.)
// part[b][blockIdx.x] = sum over the two frames and the 513 bins of (|A| - |G|)^2, in a fixed order (thread, DPP wave sum, the
// four waves in turn).
template <bool REFLECT>
__global__ __launch_bounds__(256) void spec_mse_frames_kernel(const float* __restrict__ orig, int n_orig, const float* __restrict__ gen,
                                                               int n_gen, const int32_t* __restrict__ len_orig,
                                                               const int32_t* __restrict__ len_gen, int P_max, float* __restrict__ part) {
  __shared__ float2 buf[2][NFFT];
  __shared__ float red[4];
  const int t0 = 2 * blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int lo = REFLECT ? NFFT / 2 + 1 : 1;
  const int L = min(clip_count(len_orig, b, lo, n_orig), clip_count(len_gen, b, lo, n_gen));
  const int T = 1 + L / MSE_HOP;
  if (t0 >= T) return;                                   // uniform over the workgroup, ahead of the first barrier
  const bool two = t0 + 1 < T;                           // the last frame of an odd count travels alone
  float mag[3][2], acc = 0.f;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const float* x = pass ? gen + (size_t)b * n_gen : orig + (size_t)b * n_orig;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = tid + 256 * k;
      const int idx = t0 * MSE_HOP + j - NFFT / 2;
      const float hann = 0.5f - 0.5f * cospif(2.f * j / NFFT);
      buf[0][j] = make_float2(clip_sample<REFLECT>(x, idx, L) * hann, two ? clip_sample<REFLECT>(x, idx + MSE_HOP, L) * hann : 0.f);
    }
    __syncthreads();
    const int cur = fft1024_stages(buf, tid);            // = 1: the second pass's loads into buf[0] disturb no reader of buf[1]
#pragma unroll
    for (int i = 0; i < 3; ++i) {                        // bins tid, tid + 256, and 512 for thread 0
      const int f = tid + 256 * i;
      if (f < MSE_BINS) {
        const float2 z = buf[cur][f], w = buf[cur][(NFFT - f) & (NFFT - 1)];
        const float m0 = 0.5f * cabs2(z.x + w.x, z.y - w.y), m1 = 0.5f * cabs2(z.y + w.y, z.x - w.x);
        if (pass == 0) { mag[i][0] = m0; mag[i][1] = m1; }
        else {
          const float d0 = mag[i][0] - m0, d1 = two ? mag[i][1] - m1 : 0.f;
          acc += d0 * d0 + d1 * d1;
        }
      }
    }
  }
  acc = wave_sum(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) part[(size_t)b * P_max + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// out[b] = sum of the clip's ceil(T_b / 2) partials / (513 T_b): one wave per pair (wave_partials_sum)
__global__ __launch_bounds__(64) void spec_mse_finish_kernel(const float* __restrict__ part, int n_orig, int n_gen,
                                                             const int32_t* __restrict__ len_orig, const int32_t* __restrict__ len_gen,
                                                             int P_max, int lo, float* __restrict__ out) {
  __shared__ double lane_sum[64];
  const int b = blockIdx.x;
  const int L = min(clip_count(len_orig, b, lo, n_orig), clip_count(len_gen, b, lo, n_gen));
  const int T = 1 + L / MSE_HOP;
  const double tot = wave_partials_sum(part + (size_t)b * P_max, (T + 1) / 2, lane_sum);
  if (threadIdx.x == 0) out[b] = (float)(tot / ((double)MSE_BINS * (double)T));
}

// ---- band energies: run blockIdx.x (frames BE_RUN * run ...) of clip blockIdx.y.  The 2048-point real FFT of a frame
// (frame_fft, spec_common.h); thread tid keeps the window values, the twiddles and the running sums of |X| of its bins
// tid + 256 m, m < 4 (thread 0 of bin 1024 as well) in registers and stores the sums once: part[b][run][1025].
template <bool REFLECT>
__global__ __launch_bounds__(256) void band_energy_runs_kernel(const float* __restrict__ waves, int n, const int32_t* __restrict__ n_samples,
                                                                int n_runs, float* __restrict__ part) {
  __shared__ float2 buf[2][NFFT];
  const int run = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int L = clip_count(n_samples, b, REFLECT ? WIDE_NFFT / 2 + 1 : 1, n);
  const int T = 1 + L / BE_HOP, t0 = run * BE_RUN;
  if (t0 >= T) return;                                   // uniform over the workgroup, ahead of the first barrier
  const int t1 = min(t0 + BE_RUN, T);
  const float* w = waves + (size_t)b * n;
  FrameConsts<true> fc;
  fc.init(tid);
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int t = t0; t < t1; ++t) {
    const int cur = frame_fft<true, REFLECT>(buf, w, t, BE_HOP, L, tid, fc);
#pragma unroll
    for (int m = 0; m < 4; ++m) { const float2 x = own_bin<true>(buf[cur], tid, m, fc); acc[m] += cabs2(x.x, x.y); }
    if (tid == 0) acc[4] += fabsf(last_real(buf[cur]));
  }
  float* p = part + ((size_t)b * n_runs + run) * WIDE_BINS;
#pragma unroll
  for (int m = 0; m < 4; ++m) p[tid + 256 * m] = acc[m];
  if (tid == 0) p[NFFT] = acc[4];
}

// energy[b][f] = sum over the clip's runs, ascending, in double
__global__ __launch_bounds__(256) void band_energy_finish_kernel(const float* __restrict__ part, int n, const int32_t* __restrict__ n_samples,
                                                                 int lo, int n_runs, float* __restrict__ energy) {
  const int f = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (f >= WIDE_BINS) return;
  const int T = 1 + clip_count(n_samples, b, lo, n) / BE_HOP;
  const int runs = (T + BE_RUN - 1) / BE_RUN;
  double s = 0.0;
  for (int r = 0; r < runs; ++r) s += (double)part[((size_t)b * n_runs + r) * WIDE_BINS + f];
  energy[(size_t)b * WIDE_BINS + f] = (float)s;
}

// Pearson's r (pearson_r) of rows a[b], b[b] of n values, exactly 0 where it is not finite
__global__ __launch_bounds__(256) void pearson_rows_kernel(const float* __restrict__ a, const float* __restrict__ b, int n,
                                                           float* __restrict__ out) {
  __shared__ double red[257];
  bool counts;
  const double r = pearson_r(a + (size_t)blockIdx.x * n, b + (size_t)blockIdx.x * n, n, red, counts);
  if (threadIdx.x == 0) out[blockIdx.x] = counts ? (float)r : 0.f;
}

// ---- MFCC: librosa.feature.mfcc(y, sr, n_mfcc, hop_length) with every other argument at its default, restated:
//   S = |STFT|^2 (n_fft 2048), M = W S (Slaney mel filter bank, 128 x 1025), dB = 10 log10(max(1e-10, M)), clamped from below to
//   the clip's own maximum - 80, mfcc = the first n_mfcc rows of the orthonormal DCT-II along the 128 mel bands.
// The clamp needs the maximum over the whole clip, hence two passes: the first stores the unclamped dB rows (B, T_max, 128) and
// one maximum per run of frames, the second takes the clip's maximum, clamps and transforms.
//
// The filter bank travels as a sparse table of MEL_WORDS 32-bit words (ast_mel_table, built on the host in double): the first
// bin of every filter, 129 offsets into the weights, and the weights of the filters one after the other as float bits.  A bin
// lies inside at most two triangles, so there are never more than 2 x 1025 weights.  What the kernel reads from the table is
// clamped, so that a wrong table gives wrong numbers, not reads outside the workgroup's arrays.
constexpr int MEL_W_MAX = 2 * WIDE_BINS, MEL_WORDS = 2 * MEL_N + 1 + MEL_W_MAX;
constexpr int DCT_FRAMES = 32;                           // frames per workgroup of the second pass

// pass 1: run blockIdx.x (frames MF_RUN * run ...) of clip blockIdx.y.  The frame's 2048-point real FFT (frame_fft,
// spec_common.h); the power of the 1025 bins goes to LDS, then thread j < 128 owns mel band j: it sums its filter's
// weights x powers over the filter's own bins, ascending, takes the logarithm, stores db[b][t][j] and keeps its maximum.
// run_max[b][run] = the maximum over the run's frames and the 128 bands (a maximum is exact in any order).
template <bool REFLECT>
__global__ __launch_bounds__(256) void mel_db_runs_kernel(const float* __restrict__ waves, int n, const int32_t* __restrict__ n_samples, int hop,
                                                           const int32_t* __restrict__ mel, int T_max, int n_runs, float* __restrict__ db,
                                                           float* __restrict__ run_max) {
  __shared__ float2 buf[2][NFFT];
  __shared__ float pw[WIDE_BINS], mw[MEL_W_MAX], red[2];
  const int run = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int L = clip_count(n_samples, b, REFLECT ? WIDE_NFFT / 2 + 1 : 1, n);
  const int T = 1 + L / hop, t0 = run * MF_RUN;
  if (t0 >= T) return;                                   // uniform over the workgroup, ahead of the first barrier
  const int t1 = min(t0 + MF_RUN, T);
  const float* w = waves + (size_t)b * n;
  int f_lo = 0, f_off = 0, f_n = 0;                      // mel band tid: its first bin, where its weights start, how many
  if (tid < MEL_N) {
    f_lo = min(max(mel[tid], 0), WIDE_BINS);
    f_off = min(max(mel[MEL_N + tid], 0), MEL_W_MAX);
    f_n = max(min(min(mel[MEL_N + tid + 1], MEL_W_MAX) - f_off, WIDE_BINS - f_lo), 0);
  }
  for (int i = tid; i < MEL_W_MAX; i += 256) mw[i] = __int_as_float(mel[2 * MEL_N + 1 + i]);   // read behind the loop's first barrier
  FrameConsts<true> fc;
  fc.init(tid);
  float vmax = -INFINITY;
  for (int t = t0; t < t1; ++t) {
    const int cur = frame_fft<true, REFLECT>(buf, w, t, hop, L, tid, fc);   // its barriers also stand between the last frame's readers of pw and the writes below
#pragma unroll
    for (int m = 0; m < 4; ++m) pw[tid + 256 * m] = own_power<true>(buf[cur], tid, m, fc);
    if (tid == 0) pw[NFFT] = last_power<true>(buf[cur]);
    __syncthreads();
    if (tid < MEL_N) {
      float s = 0.f;
      for (int i = 0; i < f_n; ++i) s += mw[f_off + i] * pw[f_lo + i];
      const float v = 10.f * log10f(fmaxf(s, AMIN));
      db[((size_t)b * T_max + t) * MEL_N + tid] = v;
      vmax = fmaxf(vmax, v);
    }
  }
  vmax = wave_max(vmax);                                  // waves 2 and 3 hold -inf
  if (tid == 0 || tid == 64) red[tid >> 6] = vmax;
  __syncthreads();
  if (tid == 0) run_max[(size_t)b * n_runs + run] = fmaxf(red[0], red[1]);
}

// cos(pi p / 256), p < 512: every phase of the DCT (dct_phase), so exact to float32 rounding
__device__ __forceinline__ void dct_cos_table(float* ct) {
  for (int p = threadIdx.x; p < 512; p += 256) ct[p] = cospif(p / 256.f);
}
// coefficient k of the orthonormal DCT-II of one row of 128 values, summed over j ascending
__device__ __forceinline__ float dct_row(const float* __restrict__ x, const float* __restrict__ ct, int k) {
  float s = 0.f;
#pragma unroll 8
  for (int j = 0; j < MEL_N; ++j) s += x[j] * ct[dct_phase(k, j)];
  return s * dct_scale<float>(k);
}

// pass 2 of mfcc: frames DCT_FRAMES * blockIdx.x ... of clip blockIdx.y -> out[b][k][t], layout (B, n_mfcc, T_max) as librosa's.
// Thread (tid & 31, tid >> 5) owns frame t0 + (tid & 31) and the coefficients (tid >> 5) + 8 i.  Every element of out is
// written: frames t >= T_b are exactly 0.
__global__ __launch_bounds__(256) void mfcc_dct_kernel(const float* __restrict__ db, const float* __restrict__ run_max, int n,
                                                       const int32_t* __restrict__ n_samples, int lo, int hop, int T_max, int n_runs,
                                                       int n_mfcc, float* __restrict__ out) {
  __shared__ float x[DCT_FRAMES][MEL_N + 1], ct[512], red[4];
  const int t0 = blockIdx.x * DCT_FRAMES, b = blockIdx.y, tid = threadIdx.x;
  const int T = 1 + clip_count(n_samples, b, lo, n) / hop;
  const int tl = tid & 31, t = t0 + tl;
  if (t0 < T) {                                          // uniform over the workgroup
    const float floor_db = clip_max_db<256>(run_max + (size_t)b * n_runs, (T + MF_RUN - 1) / MF_RUN, red) - TOP_DB;
    dct_cos_table(ct);
    for (int i = tid; i < DCT_FRAMES * MEL_N; i += 256) {
      const int r = i >> 7, j = i & (MEL_N - 1);
      x[r][j] = t0 + r < T ? fmaxf(db[((size_t)b * T_max + t0 + r) * MEL_N + j], floor_db) : 0.f;
    }
    __syncthreads();
  }
  if (t >= T_max) return;
  for (int k = tid >> 5; k < n_mfcc; k += 8) out[((size_t)b * n_mfcc + k) * T_max + t] = t < T ? dct_row(x[tl], ct, k) : 0.f;
}

// pass 2 of mfcc_distance: frames DCT_FRAMES * blockIdx.x ... of pair blockIdx.y, T = min of the two clips' frame counts.
// The DCT is linear: one transform of the difference of the two clamped rows (each clamped by its OWN clip's maximum over its
// own full length); both clips pass through the same arithmetic up to there, so equal clips score exactly 0.
// part[b][t] = the norm over k of frame t's coefficients: thread (tid & 31, tid >> 5) squares its coefficients in turn, thread
// (tid & 31, 0) adds the eight sums ascending.
__global__ __launch_bounds__(256) void mfcc_dist_frames_kernel(const float* __restrict__ db_g, const float* __restrict__ max_g, int n_g,
                                                               const int32_t* __restrict__ len_g, int Tmax_g, int runs_g,
                                                               const float* __restrict__ db_r, const float* __restrict__ max_r, int n_r,
                                                               const int32_t* __restrict__ len_r, int Tmax_r, int runs_r, int lo, int hop,
                                                               int n_mfcc, int P_max, float* __restrict__ part) {
  __shared__ float x[DCT_FRAMES][MEL_N + 1], ct[512], red[2][4], sq[8][DCT_FRAMES];
  const int t0 = blockIdx.x * DCT_FRAMES, b = blockIdx.y, tid = threadIdx.x;
  const int T_g = 1 + clip_count(len_g, b, lo, n_g) / hop, T_r = 1 + clip_count(len_r, b, lo, n_r) / hop;
  const int T = min(T_g, T_r);
  if (t0 >= T) return;                                   // uniform over the workgroup, ahead of the first barrier
  const float floor_g = clip_max_db<256>(max_g + (size_t)b * runs_g, (T_g + MF_RUN - 1) / MF_RUN, red[0]) - TOP_DB;
  const float floor_r = clip_max_db<256>(max_r + (size_t)b * runs_r, (T_r + MF_RUN - 1) / MF_RUN, red[1]) - TOP_DB;
  dct_cos_table(ct);
  for (int i = tid; i < DCT_FRAMES * MEL_N; i += 256) {
    const int r = i >> 7, j = i & (MEL_N - 1);
    x[r][j] = t0 + r < T ? fmaxf(db_g[((size_t)b * Tmax_g + t0 + r) * MEL_N + j], floor_g) -
                               fmaxf(db_r[((size_t)b * Tmax_r + t0 + r) * MEL_N + j], floor_r) : 0.f;
  }
  __syncthreads();
  const int tl = tid & 31;
  float s = 0.f;
  for (int k = tid >> 5; k < n_mfcc; k += 8) { const float c = dct_row(x[tl], ct, k); s += c * c; }
  sq[tid >> 5][tl] = s;
  __syncthreads();
  if (tid < DCT_FRAMES && t0 + tid < T) {
    float tot = sq[0][tid];
#pragma unroll
    for (int i = 1; i < 8; ++i) tot += sq[i][tid];
    part[(size_t)b * P_max + t0 + tid] = sqrtf(tot);
  }
}

// out[b] = the mean of the pair's T partials: one wave per pair (wave_partials_sum)
__global__ __launch_bounds__(64) void mfcc_dist_finish_kernel(const float* __restrict__ part, int n_g, int n_r, const int32_t* __restrict__ len_g,
                                                              const int32_t* __restrict__ len_r, int lo, int hop, int P_max,
                                                              float* __restrict__ out) {
  __shared__ double lane_sum[64];
  const int b = blockIdx.x;
  const int T = 1 + min(clip_count(len_g, b, lo, n_g), clip_count(len_r, b, lo, n_r)) / hop;
  const double tot = wave_partials_sum(part + (size_t)b * P_max, T, lane_sum);
  if (threadIdx.x == 0) out[b] = (float)(tot / (double)T);
}

// Slaney's mel scale (librosa.hz_to_mel, htk=False): linear below 1 kHz, logarithmic above
double hz_to_mel(double f) { return f < 1000.0 ? 3.0 * f / 200.0 : 15.0 + log(f / 1000.0) / (log(6.4) / 27.0); }
double mel_to_hz(double m) { return m < 15.0 ? 200.0 * m / 3.0 : 1000.0 * exp((log(6.4) / 27.0) * (m - 15.0)); }
}  // namespace

// the first pass and its sizes, for curation.hip as well (spec_common.h)
int mfcc_runs(int n, int hop) { return runs_of(frames_of(n, hop), MF_RUN); }
long mfcc_pass1_floats(int B, int n, int hop) { return (long)B * ((long)frames_of(n, hop) * MEL_N + mfcc_runs(n, hop)); }
void mel_db_launch(const float* waves, int B, int n, const int32_t* n_samples, int hop, int pad_mode, const int32_t* mel, float* db,
                   float* run_max, hipStream_t s) {
  const int T_max = frames_of(n, hop), n_runs = mfcc_runs(n, hop);
  PAD_LAUNCH(pad_mode, (mel_db_runs_kernel<R>), dim3(n_runs, B), dim3(256), s, waves, n, n_samples, hop, mel, T_max, n_runs, db, run_max);
}

extern "C" long ast_spec_mse_ws_floats(int B, int n_orig, int n_gen) {
  if (B < 1 || n_orig < 1 || n_gen < 1) return 0;
  return (long)B * ((2 + std::min(n_orig, n_gen) / MSE_HOP) / 2);
}

extern "C" int ast_spec_mse_len(const float* original, int n_orig, const float* generated, int n_gen, int B, const int32_t* len_orig,
                                const int32_t* len_gen, int pad_mode, float* ws, long ws_floats, float* out, void* stream) {
  const char* me = "ast_spec_mse_len";
  if (!original || !generated || !out) AST_FAIL("%s: null pointer", me);
  if (rows_check(me, B, n_orig, NFFT, pad_mode) || rows_check(me, B, n_gen, NFFT, pad_mode)) return -1;
  const int P_max = (2 + std::min(n_orig, n_gen) / MSE_HOP) / 2;        // frame pairs of the longest clip: ceil(T / 2)
  if (ws_check(me, ws, ws_floats, (long)B * P_max)) return -1;
  hipStream_t s = (hipStream_t)stream;
  PAD_LAUNCH(pad_mode, (spec_mse_frames_kernel<R>), dim3(P_max, B), dim3(256), s, original, n_orig, generated, n_gen, len_orig, len_gen, P_max, ws);
  hipLaunchKernelGGL(spec_mse_finish_kernel, dim3(B), dim3(64), 0, s, (const float*)ws, n_orig, n_gen, len_orig, len_gen, P_max,
                     min_count(pad_mode, NFFT), out);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" long ast_band_energy_ws_floats(int B, int n) {
  if (B < 1 || n < 1) return 0;
  return (long)B * runs_of(frames_of(n, BE_HOP), BE_RUN) * WIDE_BINS;
}

extern "C" int ast_band_energy_len(const float* waves, int B, int n, const int32_t* n_samples, int pad_mode, float* ws, long ws_floats,
                                   float* energy, void* stream) {
  const char* me = "ast_band_energy_len";
  if (!waves || !energy) AST_FAIL("%s: null pointer", me);
  if (rows_check(me, B, n, WIDE_NFFT, pad_mode)) return -1;
  const int n_runs = runs_of(frames_of(n, BE_HOP), BE_RUN);
  if (ws_check(me, ws, ws_floats, (long)B * n_runs * WIDE_BINS)) return -1;
  hipStream_t s = (hipStream_t)stream;
  PAD_LAUNCH(pad_mode, (band_energy_runs_kernel<R>), dim3(n_runs, B), dim3(256), s, waves, n, n_samples, n_runs, ws);
  hipLaunchKernelGGL(band_energy_finish_kernel, dim3((WIDE_BINS + 255) / 256, B), dim3(256), 0, s, (const float*)ws, n, n_samples,
                     min_count(pad_mode, WIDE_NFFT), n_runs, energy);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" int ast_band_energy_run_frames(void) { return BE_RUN; }

extern "C" int ast_pearson_rows(const float* a, const float* b, int B, int n, float* out, void* stream) {
  if (!a || !b || !out) AST_FAIL("ast_pearson_rows: null pointer");
  if (B < 1 || n < 2 || (long long)B * n > 0x7fffffffll) AST_FAIL("ast_pearson_rows: bad shape (B=%d n=%d)", B, n);
  hipLaunchKernelGGL(pearson_rows_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a, b, n, out);
  AST_CHECK_LAUNCH();
  return 0;
}

// ---- MFCC entries
extern "C" int ast_mfcc_run_frames(void) { return MF_RUN; }
extern "C" int ast_mel_table_words(void) { return MEL_WORDS; }

extern "C" int ast_mel_table(int sample_rate, int32_t* table) {
  if (!table) AST_FAIL("ast_mel_table: null pointer");
  if (sample_rate < 1) AST_FAIL("ast_mel_table: bad sample rate %d", sample_rate);
  const double fmax = 0.5 * sample_rate, mel_max = hz_to_mel(fmax);
  double mel_f[MEL_N + 2];
  for (int i = 0; i < MEL_N + 2; ++i) mel_f[i] = mel_to_hz(mel_max * i / (MEL_N + 1));
  mel_f[MEL_N + 1] = fmax;
  memset(table, 0, sizeof(int32_t) * MEL_WORDS);
  int off = 0;
  for (int i = 0; i < MEL_N; ++i) {
    int first = -1, count = 0;
    for (int k = 0; k < WIDE_BINS; ++k) {
      const double f = k * fmax / (WIDE_BINS - 1);
      const double lower = (f - mel_f[i]) / (mel_f[i + 1] - mel_f[i]), upper = (mel_f[i + 2] - f) / (mel_f[i + 2] - mel_f[i + 1]);
      const double wgt = std::max(0.0, std::min(lower, upper)) * 2.0 / (mel_f[i + 2] - mel_f[i]);
      if (!(wgt > 0.0)) {
        if (first >= 0) break;                           // a triangle: its bins are consecutive
        continue;
      }
      if (first < 0) first = k;
      if (off + count >= MEL_W_MAX) AST_FAIL("ast_mel_table: more than %d weights at %d Hz", MEL_W_MAX, sample_rate);
      const float wf = (float)wgt;
      memcpy(&table[2 * MEL_N + 1 + off + count], &wf, sizeof(float));
      ++count;
    }
    if (count == 0)
      AST_FAIL("ast_mel_table: mel band %d holds no bin of the 2048-point transform at %d Hz (the bands are narrower than a bin)", i, sample_rate);
    table[i] = first;
    table[MEL_N + i] = off;
    off += count;
  }
  table[2 * MEL_N] = off;
  return 0;
}

extern "C" long ast_mfcc_ws_floats(int B, int n, int hop) {
  if (B < 1 || n < 1 || (hop != 256 && hop != 512)) return 0;
  return mfcc_pass1_floats(B, n, hop);
}

extern "C" long ast_mfcc_distance_ws_floats(int B, int n_gen, int n_ref, int hop) {
  if (B < 1 || n_gen < 1 || n_ref < 1 || (hop != 256 && hop != 512)) return 0;
  return mfcc_pass1_floats(B, n_gen, hop) + mfcc_pass1_floats(B, n_ref, hop) + (long)B * frames_of(std::min(n_gen, n_ref), hop);
}

extern "C" int ast_mfcc_len(const float* waves, int B, int n, const int32_t* n_samples, int n_mfcc, int hop, int pad_mode,
                            const int32_t* mel_table, float* ws, long ws_floats, float* out, void* stream) {
  const char* me = "ast_mfcc_len";
  if (!waves || !out) AST_FAIL("%s: null pointer", me);
  if (mfcc_check(me, n_mfcc, MEL_N, hop, mel_table) || rows_check(me, B, n, WIDE_NFFT, pad_mode)) return -1;
  if (ws_check(me, ws, ws_floats, mfcc_pass1_floats(B, n, hop))) return -1;
  hipStream_t s = (hipStream_t)stream;
  const int T_max = frames_of(n, hop), n_runs = mfcc_runs(n, hop);
  float* run_max = ws + (size_t)B * T_max * MEL_N;
  mel_db_launch(waves, B, n, n_samples, hop, pad_mode, mel_table, ws, run_max, s);
  hipLaunchKernelGGL(mfcc_dct_kernel, dim3(runs_of(T_max, DCT_FRAMES), B), dim3(256), 0, s, (const float*)ws, (const float*)run_max, n,
                     n_samples, min_count(pad_mode, WIDE_NFFT), hop, T_max, n_runs, n_mfcc, out);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" int ast_mfcc_distance_len(const float* generated, int n_gen, const float* reference, int n_ref, int B, const int32_t* len_gen,
                                     const int32_t* len_ref, int n_mfcc, int hop, int pad_mode, const int32_t* mel_table, float* ws,
                                     long ws_floats, float* out, void* stream) {
  const char* me = "ast_mfcc_distance_len";
  if (!generated || !reference || !out) AST_FAIL("%s: null pointer", me);
  if (mfcc_check(me, n_mfcc, MEL_N, hop, mel_table) || rows_check(me, B, n_gen, WIDE_NFFT, pad_mode) || rows_check(me, B, n_ref, WIDE_NFFT, pad_mode))
    return -1;
  const int P_max = frames_of(std::min(n_gen, n_ref), hop);
  if (ws_check(me, ws, ws_floats, mfcc_pass1_floats(B, n_gen, hop) + mfcc_pass1_floats(B, n_ref, hop) + (long)B * P_max)) return -1;
  hipStream_t s = (hipStream_t)stream;
  const int Tg = frames_of(n_gen, hop), Tr = frames_of(n_ref, hop), runs_g = mfcc_runs(n_gen, hop), runs_r = mfcc_runs(n_ref, hop);
  float* db_g = ws;
  float* max_g = db_g + (size_t)B * Tg * MEL_N;
  float* db_r = max_g + (size_t)B * runs_g;
  float* max_r = db_r + (size_t)B * Tr * MEL_N;
  float* part = max_r + (size_t)B * runs_r;
  const int lo = min_count(pad_mode, WIDE_NFFT);
  mel_db_launch(generated, B, n_gen, len_gen, hop, pad_mode, mel_table, db_g, max_g, s);
  mel_db_launch(reference, B, n_ref, len_ref, hop, pad_mode, mel_table, db_r, max_r, s);
  hipLaunchKernelGGL(mfcc_dist_frames_kernel, dim3(runs_of(P_max, DCT_FRAMES), B), dim3(256), 0, s, (const float*)db_g,
                     (const float*)max_g, n_gen, len_gen, Tg, runs_g, (const float*)db_r, (const float*)max_r, n_ref, len_ref, Tr, runs_r, lo, hop,
                     n_mfcc, P_max, part);
  hipLaunchKernelGGL(mfcc_dist_finish_kernel, dim3(B), dim3(64), 0, s, (const float*)part, n_gen, n_ref, len_gen, len_ref, lo, hop, P_max, out);
  AST_CHECK_LAUNCH();
  return 0;
}

// ---- onsets and self-similarity: the last two of the evaluation scripts' eight metrics.
//   onset_accuracy (evaluation_reconstruction.py:54-81): librosa.onset.onset_detect(y, sr) with every other argument at its default,
//     restated: the mel dB rows of the MFCC's first pass at hop 512, clamped; onset strength e[t] = mean over the 128 bands of
//     max(0, dB[m][t-2] - dB[m][t-3]) for 3 <= t < T_b (lag 1, max_size 1, centred: shifted by 1 + n_fft / (2 hop) = 3 frames and
//     cut to T_b), 0 before; x = (e - min e) / (max e - min e + float32 tiny); frame n is a detection if x[n] is the maximum of its
//     pre_max / post_max window and x[n] >= the mean of its pre_avg / post_avg window + 0.07, windows cut at the clip's ends; of the
//     detections those further than `wait` behind the last kept one are kept.  Then the F1 score of the two clips' onset sets.
//   self_similarity_distance (evaluation_style_transfer.py:121-133): librosa.segment.recurrence_matrix(mfcc.T) at its defaults.  The
//     reference hands over the transpose, so the matrix's "frames" are the 20 coefficient rows, each a vector over the clip's T_b
//     time frames: 20 x 20 whatever the length.  D[i][j] = ||c_i - c_j||; per column j the 12 nearest other rows, those at
//     distance exactly 0 dropped, of the rest the 10 nearest kept: R[i][j] = 1.  The score is the mean of |R_a - R_b|.
// The rules of the kernels above hold: no atomics, one owner and a fixed order per output, counts clamped on the device.
namespace {
constexpr int ON_SR = 22050, ON_HOP = BE_HOP;            // librosa's defaults: sr, hop_length
constexpr int ON_SHIFT = 1 + WIDE_NFFT / (2 * ON_HOP);     // 3: lag + the frames `center=True` pads on the left
constexpr int ON_PRE_MAX = (3 * ON_SR / 100) / ON_HOP;   // 0.03 sr // hop = 1   \  librosa.onset.onset_detect's peak_pick arguments
constexpr int ON_POST_MAX = (0 * ON_SR) / ON_HOP + 1;    // 0.00 sr // hop + 1 = 1 |  at 22 050 Hz and hop 512; the window of frame n is
constexpr int ON_PRE_AVG = (ON_SR / 10) / ON_HOP;        // 0.10 sr // hop = 4     |  n - pre .. n + post - 1
constexpr int ON_POST_AVG = (ON_SR / 10) / ON_HOP + 1;   // 0.10 sr // hop + 1 = 5 |
constexpr int ON_WAIT = (3 * ON_SR / 100) / ON_HOP;      // 0.03 sr // hop = 1    /
constexpr float ON_DELTA = 0.07f;
static_assert(ON_WAIT == 1, "the pick kernel's greedy pass keeps every second frame of a run of detections: wait = 1");
constexpr int ENV_TILE = 8;                              // frames of one clip per workgroup of the envelope kernel
constexpr int SS_MFCC = 20;                              // librosa.feature.mfcc's default n_mfcc: the rows of the recurrence matrix
constexpr int SS_WIDTH = 1;                              // recurrence_matrix's default width
constexpr int ceil_sqrt(int v) { int r = 0; while (r * r < v) ++r; return r; }
constexpr int SS_K = 2 * ceil_sqrt(SS_MFCC - 2 * SS_WIDTH + 1);                                           // 10 links kept per column
constexpr int SS_NN = SS_MFCC - 1 < SS_K + 2 * SS_WIDTH ? SS_MFCC - 1 : SS_K + 2 * SS_WIDTH;           // 12 neighbours asked for
constexpr int SS_PAIRS = SS_MFCC * (SS_MFCC - 1) / 2, SS_CELLS = SS_MFCC * SS_MFCC;                      // 190, 400
constexpr int CD_CHUNK = 16;                             // frames per workgroup of the coefficient-distance kernel

// L[b] = the common length of pair b (evaluation_reconstruction.py:193-204): the minimum of the two clamped counts.  Both clips of
// the pair then take L as their count; it lies inside both clamps already.
__global__ __launch_bounds__(64) void pair_counts_kernel(const int32_t* __restrict__ len_a, int n_a, const int32_t* __restrict__ len_g, int n_g,
                                                         int lo, int B, int32_t* __restrict__ L) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b < B) L[b] = min(clip_count(len_a, b, lo, n_a), clip_count(len_g, b, lo, n_g));
}

// onset strength: frames ENV_TILE * blockIdx.x ... of clip blockIdx.y.  The tile's dB rows and one halo row go to LDS, clamped by the
// clip's own maximum; thread (tid >> 5, tid & 31) sums frame tid >> 5's rectified differences of the bands l, l + 32, l + 64, l + 96
// in turn, thread (f, 0) the 32 sums ascending.  Every element of env is written: 0 for t < 3 and for t >= T_b.  tile_min / tile_max:
// over the tile's frames t < T_b; the maximum is +inf if one of them is not finite.
__global__ __launch_bounds__(256) void onset_env_kernel(const float* __restrict__ db, const float* __restrict__ run_max, int n,
                                                        const int32_t* __restrict__ n_samples, int lo, int T_max, int n_runs, int n_tiles,
                                                        float* __restrict__ env, float* __restrict__ tile_min, float* __restrict__ tile_max) {
  __shared__ float x[ENV_TILE + 1][MEL_N], ps[ENV_TILE][32], ev[ENV_TILE], red[4];
  const int t0 = blockIdx.x * ENV_TILE, b = blockIdx.y, tid = threadIdx.x;
  const int T = 1 + clip_count(n_samples, b, lo, n) / ON_HOP;
  if (t0 >= T) {                                         // uniform over the workgroup: nothing of the clip is read
    if (tid < ENV_TILE && t0 + tid < T_max) env[(size_t)b * T_max + t0 + tid] = 0.f;
    return;
  }
  const float floor_db = clip_max_db<256>(run_max + (size_t)b * n_runs, (T + MF_RUN - 1) / MF_RUN, red) - TOP_DB;
  for (int i = tid; i < (ENV_TILE + 1) * MEL_N; i += 256) {
    const int r = i >> 7, j = i & (MEL_N - 1), u = t0 - ON_SHIFT + r;          // row r holds dB frame u
    x[r][j] = (u >= 0 && u < T) ? fmaxf(db[((size_t)b * T_max + u) * MEL_N + j], floor_db) : 0.f;
  }
  __syncthreads();
  const int f = tid >> 5, l = tid & 31;
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < MEL_N / 32; ++q) s += fmaxf(x[f + 1][l + 32 * q] - x[f][l + 32 * q], 0.f);
  ps[f][l] = s;
  __syncthreads();
  if (tid < ENV_TILE) {
    float tot = ps[tid][0];
    for (int i = 1; i < 32; ++i) tot += ps[tid][i];
    const int t = t0 + tid;
    const float e = (t >= ON_SHIFT && t < T) ? tot * (1.f / MEL_N) : 0.f;
    ev[tid] = e;
    if (t < T_max) env[(size_t)b * T_max + t] = e;
  }
  __syncthreads();
  if (tid == 0) {
    float mn = INFINITY, mx = -INFINITY;
    for (int i = 0; i < ENV_TILE && t0 + i < T; ++i) {
      mn = fminf(mn, ev[i]);
      mx = ev[i] < INFINITY ? fmaxf(mx, ev[i]) : INFINITY;                      // not finite (NaN as well): +inf
    }
    tile_min[(size_t)b * n_tiles + blockIdx.x] = mn;
    tile_max[(size_t)b * n_tiles + blockIdx.x] = mx;
  }
}

// the first frame of the run of consecutive detections that holds frame c0 + pos; bits: the detections of the 256 frames from
// c0 on; carry: the first frame of the run that reaches frame c0 - 1, or -1
__device__ __forceinline__ int run_start(const unsigned long long* bits, int pos, int c0, int carry) {
  int w = pos >> 6;
  unsigned long long z = ~bits[w] & ((1ull << (pos & 63)) - 1ull);
  for (;;) {
    if (z) return c0 + 64 * w + 64 - __clzll((long long)z);
    if (--w < 0) return carry >= 0 ? carry : c0;
    z = ~bits[w];
  }
}

// peak picking: clip blockIdx.x, one workgroup.  Minimum and maximum over the clip's tiles, then 256 consecutive frames at a time:
// every thread tests its frame's two conditions on the normalised envelope (window sums in ascending order), a ballot turns the
// detections into bit masks, and the greedy pass with wait = 1 needs no walk: inside a run of consecutive detections the frames at
// even distance from the run's first are kept.  Every element of mask is written, 0 for t >= T_b.
__global__ __launch_bounds__(256) void onset_pick_kernel(const float* __restrict__ env, const float* __restrict__ tile_min,
                                                         const float* __restrict__ tile_max, int n, const int32_t* __restrict__ n_samples,
                                                         int lo, int T_max, int n_tiles, int32_t* __restrict__ mask) {
  __shared__ float red[2][4];
  __shared__ unsigned long long bits[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = 1 + clip_count(n_samples, b, lo, n) / ON_HOP;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = tid; i < (T + ENV_TILE - 1) / ENV_TILE; i += 256) {
    mn = fminf(mn, tile_min[(size_t)b * n_tiles + i]);
    mx = fmaxf(mx, tile_max[(size_t)b * n_tiles + i]);
  }
  mn = -wave_max(-mn);
  mx = wave_max(mx);
  if ((tid & 63) == 0) { red[0][tid >> 6] = mn; red[1][tid >> 6] = mx; }
  __syncthreads();
  mn = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
  mx = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  const bool any = mx > 0.f && mx < INFINITY;            // e >= 0: all zero means max e = 0; not all finite means max e = +inf
  const float den = (mx - mn) + F32_TINY;
  const float* e = env + (size_t)b * T_max;
  int carry = -1;
  for (int c0 = 0; c0 < T_max; c0 += 256) {
    const int t = c0 + tid;
    bool det = false;
    if (any && t < T) {
      const float xt = (e[t] - mn) / den;
      bool top = true;
      for (int k = max(t - ON_PRE_MAX, 0); k < min(t + ON_POST_MAX, T); ++k) top = top && xt >= (e[k] - mn) / den;
      const int k0 = max(t - ON_PRE_AVG, 0), k1 = min(t + ON_POST_AVG, T);
      float s = 0.f;
      for (int k = k0; k < k1; ++k) s += (e[k] - mn) / den;
      det = top && xt >= s / (float)(k1 - k0) + ON_DELTA;
    }
    const unsigned long long m = __ballot(det);
    if ((tid & 63) == 0) bits[tid >> 6] = m;
    __syncthreads();
    if (t < T_max) mask[(size_t)b * T_max + t] = det && ((t - run_start(bits, tid, c0, carry)) & 1) == 0;
    carry = (bits[3] >> 63) ? run_start(bits, 255, c0, carry) : -1;
    __syncthreads();
  }
}

// onset_accuracy's F1: pair blockIdx.x over its T(L_b) frames; integer counts, thread 0 adds the 256 partial counts
__global__ __launch_bounds__(256) void onset_f1_kernel(const int32_t* __restrict__ mask_o, int To_max, const int32_t* __restrict__ mask_g, int Tg_max,
                                                       const int32_t* __restrict__ L, float* __restrict__ out) {
  __shared__ int cnt[3][256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = min(1 + L[b] / ON_HOP, min(To_max, Tg_max));
  int o = 0, g = 0, both = 0;
  for (int t = tid; t < T; t += 256) {
    const int mo = mask_o[(size_t)b * To_max + t] != 0, mg = mask_g[(size_t)b * Tg_max + t] != 0;
    o += mo; g += mg; both += mo & mg;
  }
  cnt[0][tid] = o; cnt[1][tid] = g; cnt[2][tid] = both;
  __syncthreads();
  if (tid == 0) {
    int O = 0, G = 0, I = 0;
    for (int i = 0; i < 256; ++i) { O += cnt[0][i]; G += cnt[1][i]; I += cnt[2][i]; }
    out[b] = (O == 0 && G == 0) ? 1.f : (O == 0 || G == 0) ? 0.f : (float)((double)(2 * I) / (double)(O + G));
  }
}

// pair p < 190 of coefficient rows -> (i, j), i < j, counted row by row
__device__ __forceinline__ void ss_pair(int p, int& i, int& j) {
  i = 0;
  while (p >= SS_MFCC - 1 - i) { p -= SS_MFCC - 1 - i; ++i; }
  j = i + 1 + p;
}

// squared distances between the 20 coefficient rows: frames CD_CHUNK * blockIdx.x ... of clip blockIdx.y through an LDS tile;
// thread p < 190 owns pair p and sums (c_i[t] - c_j[t])^2 over the chunk's frames t < T_b ascending -- the differences themselves,
// no Gram matrix: c_0 is near -1000 and the other rows are small.  part[b][chunk][p]
__global__ __launch_bounds__(256) void coef_dist_chunks_kernel(const float* __restrict__ c, int n, const int32_t* __restrict__ n_samples, int lo,
                                                               int T_max, int n_chunks, float* __restrict__ part) {
  __shared__ float x[SS_MFCC][CD_CHUNK + 1];
  const int t0 = blockIdx.x * CD_CHUNK, b = blockIdx.y, tid = threadIdx.x;
  const int T = 1 + clip_count(n_samples, b, lo, n) / ON_HOP;
  if (t0 >= T) return;                                   // uniform over the workgroup, ahead of the barrier
  const int len = min(CD_CHUNK, T - t0);
  for (int i = tid; i < SS_MFCC * CD_CHUNK; i += 256) {
    const int r = i / CD_CHUNK, j = i % CD_CHUNK;
    x[r][j] = j < len ? c[((size_t)b * SS_MFCC + r) * T_max + t0 + j] : 0.f;
  }
  __syncthreads();
  if (tid < SS_PAIRS) {
    int i, j;
    ss_pair(tid, i, j);
    float s = 0.f;
    for (int t = 0; t < len; ++t) { const float d = x[i][t] - x[j][t]; s += d * d; }
    part[((size_t)b * n_chunks + blockIdx.x) * SS_PAIRS + tid] = s;
  }
}

// recurrence matrix of clip blockIdx.x: thread p < 190 sums pair p's chunks ascending in double and rounds the sum to float once (what
// d2_out shows is what is ranked); then thread (i, j) ranks row i among the 19 candidates of column j by squared distance, ties
// to the lower index: i is kept if it is among the SS_NN nearest,
// its distance is not exactly 0, and fewer than SS_K nonzero candidates come before it.  R[b][i][j], diagonal 0, not symmetrised.
// d2_out: NULL, or (B, 20, 20) f32 squared distances (for the tests)
__global__ __launch_bounds__(256) void recurrence_kernel(const float* __restrict__ part, int n, const int32_t* __restrict__ n_samples, int lo,
                                                         int n_chunks, int32_t* __restrict__ R, float* __restrict__ d2_out) {
  __shared__ float d2[SS_MFCC][SS_MFCC];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = 1 + clip_count(n_samples, b, lo, n) / ON_HOP;
  if (tid < SS_PAIRS) {
    int i, j;
    ss_pair(tid, i, j);
    double s = 0.0;
    for (int ch = 0; ch < (T + CD_CHUNK - 1) / CD_CHUNK; ++ch) s += (double)part[((size_t)b * n_chunks + ch) * SS_PAIRS + tid];
    d2[i][j] = (float)s;
    d2[j][i] = (float)s;
  }
  if (tid < SS_MFCC) d2[tid][tid] = 0.f;
  __syncthreads();
  for (int cell = tid; cell < SS_CELLS; cell += 256) {
    const int i = cell / SS_MFCC, j = cell % SS_MFCC;
    const float d = d2[i][j];
    int rank = 0, nonzero_before = 0;
    for (int k = 0; k < SS_MFCC; ++k) {
      if (k == i || k == j) continue;
      const float dk = d2[k][j];
      const bool before = dk < d || (dk == d && k < i);
      rank += before;
      nonzero_before += before && dk != 0.f;
    }
    R[(size_t)b * SS_CELLS + cell] = i != j && rank < SS_NN && d != 0.f && nonzero_before < SS_K;
    if (d2_out) d2_out[(size_t)b * SS_CELLS + cell] = d;
  }
}

// out[b] = the mean over the 400 cells of |R_a - R_b|: one wave per pair, integer counts, lane 0 adds the 64 lanes
__global__ __launch_bounds__(64) void self_sim_finish_kernel(const int32_t* __restrict__ Ra, const int32_t* __restrict__ Rb, float* __restrict__ out) {
  __shared__ int cnt[64];
  const int b = blockIdx.x, l = threadIdx.x;
  int s = 0;
  for (int i = l; i < SS_CELLS; i += 64) s += abs(Ra[(size_t)b * SS_CELLS + i] - Rb[(size_t)b * SS_CELLS + i]);
  cnt[l] = s;
  __syncthreads();
  if (l == 0) {
    int tot = 0;
    for (int i = 0; i < 64; ++i) tot += cnt[i];
    out[b] = (float)((double)tot / (double)SS_CELLS);
  }
}

// host: sizes and launches the onset and recurrence entries share
int on_tiles(int n) { return runs_of(frames_of(n, ON_HOP), ENV_TILE); }
int ss_chunks(int n) { return runs_of(frames_of(n, ON_HOP), CD_CHUNK); }
long on_strength_floats(int B, int n) { return mfcc_pass1_floats(B, n, ON_HOP) + 2L * B * on_tiles(n); }
long on_detect_floats(int B, int n) { return on_strength_floats(B, n) + (long)B * frames_of(n, ON_HOP); }
long ss_rec_floats(int B, int n) {
  return mfcc_pass1_floats(B, n, ON_HOP) + (long)B * SS_MFCC * frames_of(n, ON_HOP) + (long)B * ss_chunks(n) * SS_PAIRS;
}
// mel dB rows -> envelope (-> mask, unless it is null) of one batch; ws: on_strength_floats(B, n)
void onset_launch(const float* waves, int B, int n, const int32_t* counts, int pad_mode, const int32_t* mel, float* ws, float* env,
                  int32_t* mask, hipStream_t s) {
  const int T_max = frames_of(n, ON_HOP), n_runs = mfcc_runs(n, ON_HOP), n_tiles = on_tiles(n);
  const int lo = min_count(pad_mode, WIDE_NFFT);
  float* run_max = ws + (size_t)B * T_max * MEL_N;
  float* tile_min = run_max + (size_t)B * n_runs;
  float* tile_max = tile_min + (size_t)B * n_tiles;
  mel_db_launch(waves, B, n, counts, ON_HOP, pad_mode, mel, ws, run_max, s);
  hipLaunchKernelGGL(onset_env_kernel, dim3(n_tiles, B), dim3(256), 0, s, (const float*)ws, (const float*)run_max, n, counts, lo, T_max, n_runs,
                     n_tiles, env, tile_min, tile_max);
  if (mask)
    hipLaunchKernelGGL(onset_pick_kernel, dim3(B), dim3(256), 0, s, (const float*)env, (const float*)tile_min, (const float*)tile_max, n, counts,
                       lo, T_max, n_tiles, mask);
}
// mel dB rows -> 20 coefficients -> squared distances -> R of one batch; ws: ss_rec_floats(B, n)
void recurrence_launch(const float* waves, int B, int n, const int32_t* counts, int pad_mode, const int32_t* mel, float* ws, int32_t* R,
                       float* d2, hipStream_t s) {
  const int T_max = frames_of(n, ON_HOP), n_runs = mfcc_runs(n, ON_HOP), n_chunks = ss_chunks(n);
  const int lo = min_count(pad_mode, WIDE_NFFT);
  float* run_max = ws + (size_t)B * T_max * MEL_N;
  float* coef = run_max + (size_t)B * n_runs;
  float* part = coef + (size_t)B * SS_MFCC * T_max;
  mel_db_launch(waves, B, n, counts, ON_HOP, pad_mode, mel, ws, run_max, s);
  hipLaunchKernelGGL(mfcc_dct_kernel, dim3(runs_of(T_max, DCT_FRAMES), B), dim3(256), 0, s, (const float*)ws, (const float*)run_max, n,
                     counts, lo, ON_HOP, T_max, n_runs, SS_MFCC, coef);
  hipLaunchKernelGGL(coef_dist_chunks_kernel, dim3(n_chunks, B), dim3(256), 0, s, (const float*)coef, n, counts, lo, T_max, n_chunks, part);
  hipLaunchKernelGGL(recurrence_kernel, dim3(B), dim3(256), 0, s, (const float*)part, n, counts, lo, n_chunks, R, d2);
}
int onset_check(const char* name, const void* a, const void* b, const void* out, const int32_t* mel) {
  if (!a || !b || !out) AST_FAIL("%s: null pointer", name);
  if (!mel) AST_FAIL("%s: null mel table (ast_mel_table fills one)", name);
  return 0;
}
}  // namespace

extern "C" int ast_onset_tile_frames(void) { return ENV_TILE; }
extern "C" int ast_recurrence_chunk_frames(void) { return CD_CHUNK; }

extern "C" long ast_onset_strength_ws_floats(int B, int n) { return (B < 1 || n < 1) ? 0 : on_strength_floats(B, n); }
extern "C" long ast_onset_detect_ws_floats(int B, int n) { return (B < 1 || n < 1) ? 0 : on_detect_floats(B, n); }
extern "C" long ast_onset_accuracy_ws_floats(int B, int n_orig, int n_gen) {
  if (B < 1 || n_orig < 1 || n_gen < 1) return 0;
  return B + on_detect_floats(B, n_orig) + on_detect_floats(B, n_gen) + (long)B * (frames_of(n_orig, ON_HOP) + frames_of(n_gen, ON_HOP));
}
extern "C" long ast_recurrence_ws_floats(int B, int n) { return (B < 1 || n < 1) ? 0 : ss_rec_floats(B, n); }
extern "C" long ast_self_similarity_distance_ws_floats(int B, int n_a, int n_b) {
  if (B < 1 || n_a < 1 || n_b < 1) return 0;
  return ss_rec_floats(B, n_a) + ss_rec_floats(B, n_b) + 2L * B * SS_CELLS;
}

extern "C" int ast_onset_strength_len(const float* waves, int B, int n, const int32_t* n_samples, int pad_mode, const int32_t* mel_table,
                                      float* ws, long ws_floats, float* out, void* stream) {
  const char* me = "ast_onset_strength_len";
  if (onset_check(me, waves, waves, out, mel_table) || rows_check(me, B, n, WIDE_NFFT, pad_mode)) return -1;
  if (ws_check(me, ws, ws_floats, on_strength_floats(B, n))) return -1;
  onset_launch(waves, B, n, n_samples, pad_mode, mel_table, ws, out, nullptr, (hipStream_t)stream);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" int ast_onset_detect_len(const float* waves, int B, int n, const int32_t* n_samples, int pad_mode, const int32_t* mel_table,
                                    float* ws, long ws_floats, int32_t* mask, void* stream) {
  const char* me = "ast_onset_detect_len";
  if (onset_check(me, waves, waves, mask, mel_table) || rows_check(me, B, n, WIDE_NFFT, pad_mode)) return -1;
  if (ws_check(me, ws, ws_floats, on_detect_floats(B, n))) return -1;
  onset_launch(waves, B, n, n_samples, pad_mode, mel_table, ws, ws + on_strength_floats(B, n), mask, (hipStream_t)stream);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" int ast_onset_accuracy_len(const float* original, int n_orig, const float* generated, int n_gen, int B, const int32_t* len_orig,
                                      const int32_t* len_gen, int pad_mode, const int32_t* mel_table, float* ws, long ws_floats, float* out,
                                      void* stream) {
  const char* me = "ast_onset_accuracy_len";
  if (onset_check(me, original, generated, out, mel_table) || rows_check(me, B, n_orig, WIDE_NFFT, pad_mode) ||
      rows_check(me, B, n_gen, WIDE_NFFT, pad_mode))
    return -1;
  if (ws_check(me, ws, ws_floats, ast_onset_accuracy_ws_floats(B, n_orig, n_gen))) return -1;
  hipStream_t s = (hipStream_t)stream;
  const int To = frames_of(n_orig, ON_HOP), Tg = frames_of(n_gen, ON_HOP);
  int32_t* L = (int32_t*)ws;                             // the pair's common counts, then the two clips' chains and masks
  float* ws_o = ws + B;
  float* env_o = ws_o + on_strength_floats(B, n_orig);
  float* ws_g = env_o + (size_t)B * To;
  float* env_g = ws_g + on_strength_floats(B, n_gen);
  int32_t* mask_o = (int32_t*)(env_g + (size_t)B * Tg);
  int32_t* mask_g = mask_o + (size_t)B * To;
  hipLaunchKernelGGL(pair_counts_kernel, dim3((B + 63) / 64), dim3(64), 0, s, len_orig, n_orig, len_gen, n_gen,
                     min_count(pad_mode, WIDE_NFFT), B, L);
  onset_launch(original, B, n_orig, L, pad_mode, mel_table, ws_o, env_o, mask_o, s);
  onset_launch(generated, B, n_gen, L, pad_mode, mel_table, ws_g, env_g, mask_g, s);
  hipLaunchKernelGGL(onset_f1_kernel, dim3(B), dim3(256), 0, s, (const int32_t*)mask_o, To, (const int32_t*)mask_g, Tg, (const int32_t*)L, out);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" int ast_recurrence_len(const float* waves, int B, int n, const int32_t* n_samples, int pad_mode, const int32_t* mel_table, float* ws,
                                  long ws_floats, int32_t* R, float* dist2, void* stream) {
  const char* me = "ast_recurrence_len";
  if (onset_check(me, waves, waves, R, mel_table) || rows_check(me, B, n, WIDE_NFFT, pad_mode)) return -1;
  if (ws_check(me, ws, ws_floats, ss_rec_floats(B, n))) return -1;
  recurrence_launch(waves, B, n, n_samples, pad_mode, mel_table, ws, R, dist2, (hipStream_t)stream);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" int ast_self_similarity_distance_len(const float* a, int n_a, const float* b, int n_b, int B, const int32_t* len_a,
                                                const int32_t* len_b, int pad_mode, const int32_t* mel_table, float* ws, long ws_floats,
                                                float* out, void* stream) {
  const char* me = "ast_self_similarity_distance_len";
  if (onset_check(me, a, b, out, mel_table) || rows_check(me, B, n_a, WIDE_NFFT, pad_mode) || rows_check(me, B, n_b, WIDE_NFFT, pad_mode)) return -1;
  if (ws_check(me, ws, ws_floats, ast_self_similarity_distance_ws_floats(B, n_a, n_b))) return -1;
  hipStream_t s = (hipStream_t)stream;
  float* ws_b = ws + ss_rec_floats(B, n_a);
  int32_t* Ra = (int32_t*)(ws_b + ss_rec_floats(B, n_b));
  int32_t* Rb = Ra + (size_t)B * SS_CELLS;
  recurrence_launch(a, B, n_a, len_a, pad_mode, mel_table, ws, Ra, nullptr, s);
  recurrence_launch(b, B, n_b, len_b, pad_mode, mel_table, ws_b, Rb, nullptr, s);
  hipLaunchKernelGGL(self_sim_finish_kernel, dim3(B), dim3(64), 0, s, (const int32_t*)Ra, (const int32_t*)Rb, out);
  AST_CHECK_LAUNCH();
  return 0;
}
