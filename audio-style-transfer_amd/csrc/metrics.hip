// Spectrogram metrics of the reference's evaluation scripts for a padded batch of clips of different lengths:
//   mse_spectrogram (evaluation_reconstruction.py:105-118, after the truncation to a common length at :193-204): n_fft 1024, hop 256
//   instrumentation_similarity (evaluation_style_transfer.py:111-119): n_fft 2048, hop 512, band energies + Pearson's r
// Both are |STFT| (librosa.stft defaults: centred frames, periodic Hann) plus a reduction, so the spectrogram never exists in
// HBM: a workgroup transforms a frame in LDS with the front end's 1024-point network (fft1024.h), reduces what it needs and stores
// one partial per frame (MSE) or per run of frames (band energies) into the caller's workspace with ordinary stores.  A second
// small launch sums a clip's partials in a fixed order in double.  No atomics: every output element has one owner and a fixed
// order of summation, so the results are bit-reproducible.
//
// Per-clip sample counts are read from the device and clamped, as in the ragged front end (fft.hip); samples behind a clip's
// end are never read, and per frame the arithmetic does not depend on the batch around the clip.
#include "ast_common.h"
#include "fft1024.h"
#include "../../include/ast_hip.h"

namespace {
constexpr int MSE_HOP = 256, MSE_BINS = 513;             // N_FFT / HOP_LENGTH of evaluation_reconstruction.py
constexpr int BE_NFFT = 2048, BE_HOP = 512, BE_BINS = 1025;   // librosa.stft defaults
constexpr int BE_RUN = 5;                                // consecutive frames of one clip per workgroup (one partial per run)

__device__ __forceinline__ int clip_count(const int32_t* __restrict__ n, int b, int lo, int n_max) {
  return n ? min(max(n[b], lo), n_max) : n_max;
}
// sample `idx` of a clip of L samples under the pad mode; reflect needs -L < idx < 2 L - 1, which L > n_fft / 2 gives
template <bool REFLECT>
__device__ __forceinline__ float clip_sample(const float* __restrict__ w, int idx, int L) {
  if (REFLECT) {
    if (idx < 0) idx = -idx;
    if (idx >= L) idx = 2 * (L - 1) - idx;
    return w[idx];
  }
  return (idx >= 0 && idx < L) ? w[idx] : 0.f;
}
__device__ __forceinline__ float cabs2(float x, float y) { return sqrtf(x * x + y * y); }

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

// out[b] = sum of the clip's ceil(T_b / 2) partials / (513 T_b): one wave per pair; lane l sums the partials l, l + 64, ...
// ascending, lane 0 the 64 lanes ascending, all in double
__global__ __launch_bounds__(64) void spec_mse_finish_kernel(const float* __restrict__ part, int n_orig, int n_gen,
                                                             const int32_t* __restrict__ len_orig, const int32_t* __restrict__ len_gen,
                                                             int P_max, int lo, float* __restrict__ out) {
  __shared__ double lane_sum[64];
  const int b = blockIdx.x, l = threadIdx.x;
  const int L = min(clip_count(len_orig, b, lo, n_orig), clip_count(len_gen, b, lo, n_gen));
  const int T = 1 + L / MSE_HOP;
  double s = 0.0;
  for (int p = l; p < (T + 1) / 2; p += 64) s += (double)part[(size_t)b * P_max + p];
  lane_sum[l] = s;
  __syncthreads();
  if (l == 0) {
    double tot = 0.0;
    for (int i = 0; i < 64; ++i) tot += lane_sum[i];
    out[b] = (float)(tot / ((double)MSE_BINS * (double)T));
  }
}

// ---- band energies: run blockIdx.x (frames BE_RUN * run ...) of clip blockIdx.y.  The 2048-point real FFT of a frame through
// the 1024-point network: z[n] = x[2n] + i x[2n+1], then X[k] = E[k] + e^(-i pi k / 1024) O[k] with E, O the Hermitian split of
// Z as above (Z[1024] = Z[0]).  Thread tid owns the bins tid + 256 m, m < 4 (thread 0 bin 1024 as well), keeps their window
// values, twiddles and running sums of |X| in registers and stores them once: part[b][run][1025].
template <bool REFLECT>
__global__ __launch_bounds__(256) void band_energy_runs_kernel(const float* __restrict__ waves, int n, const int32_t* __restrict__ n_samples,
                                                                int n_runs, float* __restrict__ part) {
  __shared__ float2 buf[2][NFFT];
  const int run = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int L = clip_count(n_samples, b, REFLECT ? BE_NFFT / 2 + 1 : 1, n);
  const int T = 1 + L / BE_HOP, t0 = run * BE_RUN;
  if (t0 >= T) return;                                   // uniform over the workgroup, ahead of the first barrier
  const int t1 = min(t0 + BE_RUN, T);
  const float* w = waves + (size_t)b * n;
  float hann[4][2], tc[4], ts[4], acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int j = 2 * (tid + 256 * m);
    hann[m][0] = 0.5f - 0.5f * cospif(2.f * j / BE_NFFT);
    hann[m][1] = 0.5f - 0.5f * cospif(2.f * (j + 1) / BE_NFFT);
    sincospif(-(float)(tid + 256 * m) / NFFT, &ts[m], &tc[m]);
  }
  for (int t = t0; t < t1; ++t) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int q = tid + 256 * m;
      const int idx = t * BE_HOP + 2 * q - BE_NFFT / 2;
      buf[0][q] = make_float2(clip_sample<REFLECT>(w, idx, L) * hann[m][0], clip_sample<REFLECT>(w, idx + 1, L) * hann[m][1]);
    }
    __syncthreads();
    const int cur = fft1024_stages(buf, tid);            // = 1: the next frame's loads into buf[0] disturb no reader of buf[1]
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int k = tid + 256 * m;
      const float2 z = buf[cur][k], c = buf[cur][(NFFT - k) & (NFFT - 1)];
      const float er = 0.5f * (z.x + c.x), ei = 0.5f * (z.y - c.y), orr = 0.5f * (z.y + c.y), oi = -0.5f * (z.x - c.x);
      acc[m] += cabs2(er + (orr * tc[m] - oi * ts[m]), ei + (orr * ts[m] + oi * tc[m]));
    }
    if (tid == 0) { const float2 z = buf[cur][0]; acc[4] += fabsf(z.x - z.y); }
  }
  float* p = part + ((size_t)b * n_runs + run) * BE_BINS;
#pragma unroll
  for (int m = 0; m < 4; ++m) p[tid + 256 * m] = acc[m];
  if (tid == 0) p[NFFT] = acc[4];
}

// energy[b][f] = sum over the clip's runs, ascending, in double
__global__ __launch_bounds__(256) void band_energy_finish_kernel(const float* __restrict__ part, int n, const int32_t* __restrict__ n_samples,
                                                                 int lo, int n_runs, float* __restrict__ energy) {
  const int f = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (f >= BE_BINS) return;
  const int T = 1 + clip_count(n_samples, b, lo, n) / BE_HOP;
  const int runs = (T + BE_RUN - 1) / BE_RUN;
  double s = 0.0;
  for (int r = 0; r < runs; ++r) s += (double)part[((size_t)b * n_runs + r) * BE_BINS + f];
  energy[(size_t)b * BE_BINS + f] = (float)s;
}

// block-wide sum in double in a fixed order: thread-strided partial sums, then thread 0 adds the 256 of them ascending
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  if (threadIdx.x == 0) { double s = 0.0; for (int i = 0; i < 256; ++i) s += red[i]; red[256] = s; }
  __syncthreads();
  return red[256];
}
// Pearson's r of rows a[b], b[b] of n values (scipy.stats.pearsonr: means, centred sums, ratio), exactly 0 where it is not
// finite (the reference's nan -> 0.0)
__global__ __launch_bounds__(256) void pearson_rows_kernel(const float* __restrict__ a, const float* __restrict__ b, int n,
                                                           float* __restrict__ out) {
  __shared__ double red[257];
  const float* x = a + (size_t)blockIdx.x * n;
  const float* y = b + (size_t)blockIdx.x * n;
  double sx = 0.0, sy = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) { sx += (double)x[i]; sy += (double)y[i]; }
  const double mx = block_sum_f64(sx, red) / n, my = block_sum_f64(sy, red) / n;
  double sxy = 0.0, sxx = 0.0, syy = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double dx = (double)x[i] - mx, dy = (double)y[i] - my;
    sxy += dx * dy; sxx += dx * dx; syy += dy * dy;
  }
  sxy = block_sum_f64(sxy, red); sxx = block_sum_f64(sxx, red); syy = block_sum_f64(syy, red);
  if (threadIdx.x == 0) {
    const double r = sxy / (sqrt(sxx) * sqrt(syy));
    out[blockIdx.x] = (r == r && fabs(r) <= 1.7976931348623157e308) ? (float)fmin(fmax(r, -1.0), 1.0) : 0.f;
  }
}

// host: the row checks both transforms share.  0, or -1 with the message of entry `name` set
int rows_check(const char* name, int B, int n, int n_fft, int pad_mode) {
  if (B < 1 || B > 65535) AST_FAIL("%s: bad shape (B=%d, 1 .. 65535)", name, B);
  if (pad_mode != AST_PAD_CONSTANT && pad_mode != AST_PAD_REFLECT) AST_FAIL("%s: bad pad_mode %d (0 constant, 1 reflect)", name, pad_mode);
  if (n < 1) AST_FAIL("%s: bad shape (n=%d)", name, n);
  if (n > 0x7fffffff - 2 * n_fft) AST_FAIL("%s: row too long (n=%d: n + 2 n_fft must stay below 2^31)", name, n);
  if (pad_mode == AST_PAD_REFLECT && n < n_fft / 2 + 1)
    AST_FAIL("%s: reflect padding needs rows of >= %d samples, got %d", name, n_fft / 2 + 1, n);
  return 0;
}
}  // namespace

extern "C" long ast_spec_mse_ws_floats(int B, int n_orig, int n_gen) {
  if (B < 1 || n_orig < 1 || n_gen < 1) return 0;
  return (long)B * ((2 + std::min(n_orig, n_gen) / MSE_HOP) / 2);
}

extern "C" int ast_spec_mse_len(const float* original, int n_orig, const float* generated, int n_gen, int B, const int32_t* len_orig,
                                const int32_t* len_gen, int pad_mode, float* ws, long ws_floats, float* out, void* stream) {
  if (!original || !generated || !out) AST_FAIL("ast_spec_mse_len: null pointer");
  if (rows_check("ast_spec_mse_len", B, n_orig, NFFT, pad_mode) || rows_check("ast_spec_mse_len", B, n_gen, NFFT, pad_mode)) return -1;
  const int P_max = (2 + std::min(n_orig, n_gen) / MSE_HOP) / 2;        // frame pairs of the longest clip: ceil(T / 2)
  if (!ws || ws_floats < (long)B * P_max) AST_FAIL("ast_spec_mse_len: workspace of %ld floats needed, got %ld", (long)B * P_max, ws ? ws_floats : 0L);
  hipStream_t s = (hipStream_t)stream;
  const bool reflect = pad_mode == AST_PAD_REFLECT;
  if (reflect)
    hipLaunchKernelGGL(spec_mse_frames_kernel<true>, dim3(P_max, B), dim3(256), 0, s, original, n_orig, generated, n_gen, len_orig, len_gen, P_max, ws);
  else
    hipLaunchKernelGGL(spec_mse_frames_kernel<false>, dim3(P_max, B), dim3(256), 0, s, original, n_orig, generated, n_gen, len_orig, len_gen, P_max, ws);
  hipLaunchKernelGGL(spec_mse_finish_kernel, dim3(B), dim3(64), 0, s, (const float*)ws, n_orig, n_gen, len_orig, len_gen, P_max,
                     reflect ? NFFT / 2 + 1 : 1, out);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" long ast_band_energy_ws_floats(int B, int n) {
  if (B < 1 || n < 1) return 0;
  return (long)B * ((1 + n / BE_HOP + BE_RUN - 1) / BE_RUN) * BE_BINS;
}

extern "C" int ast_band_energy_len(const float* waves, int B, int n, const int32_t* n_samples, int pad_mode, float* ws, long ws_floats,
                                   float* energy, void* stream) {
  if (!waves || !energy) AST_FAIL("ast_band_energy_len: null pointer");
  if (rows_check("ast_band_energy_len", B, n, BE_NFFT, pad_mode)) return -1;
  const int n_runs = (1 + n / BE_HOP + BE_RUN - 1) / BE_RUN;
  const long need = (long)B * n_runs * BE_BINS;
  if (!ws || ws_floats < need) AST_FAIL("ast_band_energy_len: workspace of %ld floats needed, got %ld", need, ws ? ws_floats : 0L);
  hipStream_t s = (hipStream_t)stream;
  const bool reflect = pad_mode == AST_PAD_REFLECT;
  if (reflect)
    hipLaunchKernelGGL(band_energy_runs_kernel<true>, dim3(n_runs, B), dim3(256), 0, s, waves, n, n_samples, n_runs, ws);
  else
    hipLaunchKernelGGL(band_energy_runs_kernel<false>, dim3(n_runs, B), dim3(256), 0, s, waves, n, n_samples, n_runs, ws);
  hipLaunchKernelGGL(band_energy_finish_kernel, dim3((BE_BINS + 255) / 256, B), dim3(256), 0, s, (const float*)ws, n, n_samples,
                     reflect ? BE_NFFT / 2 + 1 : 1, n_runs, energy);
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
