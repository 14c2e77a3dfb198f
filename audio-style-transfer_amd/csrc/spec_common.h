// What the spectrogram metrics (metrics.hip), the chroma / pitch metrics (chroma.hip) and the dataset screening (curation.hip)
// share: the constants, the clamped per-clip count, a clip's sample under the pad mode, the transform of one windowed frame, the
// fixed-order reducers in double, the clip's dB maximum, the DCT's phase and scale, and the host prelude of the entries.  Everything
// on the device is force-inlined, so a kernel's code is what it would be with the text in its own file (tools/kernel_diff.py).
#pragma once
#include <math.h>

#include "ast_common.h"
#include "fft1024.h"
#include "../../include/ast_hip.h"

namespace {
constexpr int WIDE_NFFT = 2048, WIDE_BINS = 1025;        // librosa's default n_fft and its bins: two real samples per point of the network
constexpr int MEL_N = 128;                               // librosa.feature.mfcc's default n_mels
constexpr int MF_RUN = 5;                                // consecutive frames of one clip per workgroup of the mel pass (one maximum per run)
constexpr float TOP_DB = 80.f, AMIN = 1e-10f;            // librosa.power_to_db defaults
constexpr float F32_TINY = 1.17549435e-38f;

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

// ---- the transform of one windowed frame (librosa.stft: centred frames, periodic Hann) by a 256-thread workgroup.
// WIDE: n_fft 2048 through the 1024-point network: z[n] = x[2n] + i x[2n+1], then X[k] = E[k] + e^(-i pi k / 1024) O[k] with E, O
// the Hermitian split of Z, E[k] = (Z[k] + conj Z[N-k]) / 2, O[k] = (Z[k] - conj Z[N-k]) / 2i (Z[1024] = Z[0]); thread tid owns
// the bins tid + 256 m, m < 4, thread 0 bin 1024 as well.  Otherwise n_fft 1024, one real frame per transform (bins tid + 256 m,
// m < 2, thread 0 bin 512 as well).
template <bool WIDE> struct Bins { static constexpr int N_FFT = WIDE ? WIDE_NFFT : NFFT, HOP = N_FFT / 4, K = N_FFT / 2 + 1, OWN = WIDE ? 4 : 2; };
// the thread's window values and twiddles, computed once per workgroup and kept in registers
template <bool WIDE>
struct FrameConsts {
  float hann[4][2], tc[4], ts[4];
  __device__ __forceinline__ void init(int tid) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int q = tid + 256 * m;
      if (WIDE) {
        hann[m][0] = 0.5f - 0.5f * cospif(2.f * (2 * q) / WIDE_NFFT);
        hann[m][1] = 0.5f - 0.5f * cospif(2.f * (2 * q + 1) / WIDE_NFFT);
        sincospif(-(float)q / NFFT, &ts[m], &tc[m]);
      } else {
        hann[m][0] = 0.5f - 0.5f * cospif(2.f * q / NFFT);
      }
    }
  }
};
// frame t (at `hop` samples a frame) of a clip of L samples into buf[0], transformed; returns the half of buf that holds Z (= 1:
// the next frame's loads into buf[0] disturb no reader of buf[1])
template <bool WIDE, bool REFLECT>
__device__ __forceinline__ int frame_fft(float2 (&buf)[2][NFFT], const float* __restrict__ w, int t, int hop, int L, int tid,
                                         const FrameConsts<WIDE>& fc) {
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int q = tid + 256 * m;
    if (WIDE) {
      const int idx = t * hop + 2 * q - WIDE_NFFT / 2;
      buf[0][q] = make_float2(clip_sample<REFLECT>(w, idx, L) * fc.hann[m][0], clip_sample<REFLECT>(w, idx + 1, L) * fc.hann[m][1]);
    } else {
      buf[0][q] = make_float2(clip_sample<REFLECT>(w, t * hop + q - NFFT / 2, L) * fc.hann[m][0], 0.f);
    }
  }
  __syncthreads();
  return fft1024_stages(buf, tid);
}
// X[k] of the thread's own bin k = tid + 256 m as (re, im); what a caller takes of it (|X|, |X|^2) is its own expression
template <bool WIDE>
__device__ __forceinline__ float2 own_bin(const float2 (&z_)[NFFT], int tid, int m, const FrameConsts<WIDE>& fc) {
  const int k = tid + 256 * m;
  const float2 z = z_[k];
  if (!WIDE) return z;
  const float2 c = z_[(NFFT - k) & (NFFT - 1)];
  const float er = 0.5f * (z.x + c.x), ei = 0.5f * (z.y - c.y), orr = 0.5f * (z.y + c.y), oi = -0.5f * (z.x - c.x);
  return make_float2(er + (orr * fc.tc[m] - oi * fc.ts[m]), ei + (orr * fc.ts[m] + oi * fc.tc[m]));
}
template <bool WIDE>
__device__ __forceinline__ float own_power(const float2 (&z_)[NFFT], int tid, int m, const FrameConsts<WIDE>& fc) {
  const float2 x = own_bin<WIDE>(z_, tid, m, fc);
  return x.x * x.x + x.y * x.y;
}
// the last bin, K - 1 (thread 0 only).  WIDE: X[1024] = Re Z[0] - Im Z[0], a real number
__device__ __forceinline__ float last_real(const float2 (&z_)[NFFT]) { return z_[0].x - z_[0].y; }
template <bool WIDE>
__device__ __forceinline__ float last_power(const float2 (&z_)[NFFT]) {
  if (WIDE) return last_real(z_) * last_real(z_);
  const float2 z = z_[NFFT / 2];
  return z.x * z.x + z.y * z.y;
}

// ---- reducers: every output has one owner and a fixed order of summation
// block-wide sum in double in a fixed order: thread-strided partial sums, then thread 0 adds the 256 of them ascending
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  if (threadIdx.x == 0) { double s = 0.0; for (int i = 0; i < 256; ++i) s += red[i]; red[256] = s; }
  __syncthreads();
  return red[256];
}
// Pearson's r of x[0 .. n) and y[0 .. n) (scipy.stats.pearsonr: means, centred sums, ratio) in double, clamped to [-1, 1], to every
// thread of a 256-thread workgroup (red: 257 doubles of LDS).  counts: whether r is finite (the reference's nan -> 0.0 where not)
__device__ __forceinline__ double pearson_r(const float* __restrict__ x, const float* __restrict__ y, int n, double* red, bool& counts) {
  double sx = 0.0, sy = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) { sx += (double)x[i]; sy += (double)y[i]; }
  const double mx = block_sum_f64(sx, red) / n, my = block_sum_f64(sy, red) / n;
  double sxy = 0.0, sxx = 0.0, syy = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double dx = (double)x[i] - mx, dy = (double)y[i] - my;
    sxy += dx * dy; sxx += dx * dx; syy += dy * dy;
  }
  sxy = block_sum_f64(sxy, red); sxx = block_sum_f64(sxx, red); syy = block_sum_f64(syy, red);
  const double r = sxy / (sqrt(sxx) * sqrt(syy));
  counts = r == r && fabs(r) <= 1.7976931348623157e308;
  return fmin(fmax(r, -1.0), 1.0);
}
// the sum of part[0 .. count) in double by one wave (a 64-thread workgroup; lane_sum: 64 doubles of LDS): lane l sums the partials
// l, l + 64, ... ascending, lane 0 the 64 lanes ascending.  The sum is lane 0's; the other lanes get 0
__device__ __forceinline__ double wave_partials_sum(const float* __restrict__ part, int count, double* lane_sum) {
  double s = 0.0, tot = 0.0;
  for (int p = threadIdx.x; p < count; p += 64) s += (double)part[p];
  lane_sum[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) for (int i = 0; i < 64; ++i) tot += lane_sum[i];
  return tot;
}
// the maximum of a clip's `runs` run maxima of the mel pass, to every thread of a workgroup of THREADS threads (red: THREADS / 64
// floats of LDS of its own); a maximum is exact in any order
template <int THREADS>
__device__ __forceinline__ float clip_max_db(const float* __restrict__ run_max, int runs, float* red) {
  static_assert(THREADS == 128 || THREADS == 256, "two or four waves");
  float m = -INFINITY;
  for (int r = threadIdx.x; r < runs; r += THREADS) m = fmaxf(m, run_max[r]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  return THREADS == 256 ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : fmaxf(red[0], red[1]);
}
// the orthonormal DCT-II along the 128 mel bands: coefficient k = dct_scale(k) sum_j x[j] cos(pi dct_phase(k, j) / 256), the phase
// k (2 j + 1) reduced mod 512 in integers, so exact whatever the precision of the cosine
__device__ __forceinline__ int dct_phase(int k, int j) { return (k * (2 * j + 1)) & 511; }
template <typename T>
__device__ __forceinline__ T dct_scale(int k) { return k ? (T)0.125 : (T)0.08838834764831845; }   // sqrt(2 / 128), sqrt(1 / 128)

// ---- host: the prelude every entry shares
inline int frames_of(int n, int hop) { return 1 + n / hop; }                             // T(n) of centred frames
inline int runs_of(int frames, int run) { return (frames + run - 1) / run; }
inline int min_count(int pad_mode, int n_fft) { return pad_mode == AST_PAD_REFLECT ? n_fft / 2 + 1 : 1; }   // a clip's count is clamped to it
// the row checks every transform shares.  0, or -1 with the message of entry `name` set
inline int rows_check(const char* name, int B, int n, int n_fft, int pad_mode) {
  if (B < 1 || B > 65535) AST_FAIL("%s: bad shape (B=%d, 1 .. 65535)", name, B);
  if (pad_mode != AST_PAD_CONSTANT && pad_mode != AST_PAD_REFLECT) AST_FAIL("%s: bad pad_mode %d (0 constant, 1 reflect)", name, pad_mode);
  if (n < 1) AST_FAIL("%s: bad shape (n=%d)", name, n);
  if (n > 0x7fffffff - 2 * n_fft) AST_FAIL("%s: row too long (n=%d: n + 2 n_fft must stay below 2^31)", name, n);
  if (pad_mode == AST_PAD_REFLECT && n < n_fft / 2 + 1)
    AST_FAIL("%s: reflect padding needs rows of >= %d samples, got %d", name, n_fft / 2 + 1, n);
  return 0;
}
inline int ws_check(const char* name, const float* ws, long have, long need) {
  if (!ws || have < need) AST_FAIL("%s: workspace of %ld floats needed, got %ld", name, need, ws ? have : 0L);
  return 0;
}
// what the MFCC entries refuse: n_mfcc above `max_mfcc`, a hop that is neither of the reference's two, no mel table
inline int mfcc_check(const char* name, int n_mfcc, int max_mfcc, int hop, const int32_t* mel_table) {
  if (!mel_table) AST_FAIL("%s: null mel table (ast_mel_table fills one)", name);
  if (n_mfcc < 1 || n_mfcc > max_mfcc) AST_FAIL("%s: bad n_mfcc %d (1 .. %d)", name, n_mfcc, max_mfcc);
  if (hop != 256 && hop != 512) AST_FAIL("%s: bad hop %d (256 or 512)", name, hop);
  return 0;
}
// launches KERNEL, a parenthesised template-id that names the pad mode's argument R: PAD_LAUNCH(pad_mode, (k<true, R>), grid, ...)
#define PAD_LAUNCH(pad_mode, KERNEL, grid, block, s, ...)                                                                  \
  do {                                                                                                                      \
    if ((pad_mode) == AST_PAD_REFLECT) { constexpr bool R = true; hipLaunchKernelGGL(KERNEL, grid, block, 0, s, __VA_ARGS__); } \
    else { constexpr bool R = false; hipLaunchKernelGGL(KERNEL, grid, block, 0, s, __VA_ARGS__); }                          \
  } while (0)
}  // namespace

// ---- the MFCC's first pass (metrics.hip), which the dataset screening (curation.hip) runs too: the unclamped mel dB rows
// db (B, T_max, 128) and one maximum per run of MF_RUN frames, T_max = frames_of(n, hop).  Host code only, not exported.
AST_HIDDEN int mfcc_runs(int n, int hop);                                      // run maxima per clip
AST_HIDDEN long mfcc_pass1_floats(int B, int n, int hop);                      // floats of db + run_max, run_max behind db
AST_HIDDEN void mel_db_launch(const float* waves, int B, int n, const int32_t* n_samples, int hop, int pad_mode, const int32_t* mel, float* db,
                              float* run_max, hipStream_t s);
