// Chroma and pitch metrics of the reference's evaluation scripts for a padded batch of clips of different lengths:
//   chroma_distance   (evaluation_reconstruction.py:39-52):  librosa.feature.chroma_stft at n_fft 2048, hop 512
//   pitch_correlation (evaluation_reconstruction.py:83-103): librosa.piptrack at n_fft 2048, hop 512
//   chroma_similarity (evaluation_style_transfer.py:80-96):  librosa.feature.chroma_stft at n_fft 1024, hop 256
// librosa's documented chain is restated ("Chroma and pitch"); sr = 22 050 throughout.  As in metrics.hip the
// spectrogram never exists in HBM: a workgroup transforms a run of consecutive frames of one clip in LDS (fft1024.h) and keeps
// what a frame needs.  chroma_stft needs the clip's tuning first, and the tuning needs a median over the whole clip, hence three
// passes:
//   1. peaks:  per frame the parabolic-interpolated peaks of the candidate band (piptrack) -> ws: pitch and mag, [b][t][band],
//              0 where there is no peak; for pitch_correlation only the frame's mean pitch is stored;
//   2. tuning: per clip an exact median of the peaks' mags by radix selection on their bit patterns, then the 100-bin histogram
//              of the kept peaks' deviations from equal temperament and its argmax;
//   3. chroma: the frames again, 12 weighted sums of the power spectrum per frame with the filter bank of the clip's tuning.
// No float atomics: every float output has one owner and a fixed order of summation; the only atomics are integer counters in
// LDS, whose sums do not depend on the order.  Per-clip sample counts are read from the device and clamped; samples behind a
// clip's end are never read, and per frame the arithmetic does not depend on the batch around the clip.
#include "spec_common.h"

namespace {
constexpr int SR = 22050, N_CHROMA = 12;
constexpr int CH_RUN = 16;                               // consecutive frames of one clip per workgroup
constexpr int TN_THREADS = 1024;                         // threads of the tuning pass, one workgroup per clip
constexpr int DBG_WORDS = 103;                           // candidates, kept, thr (float bits), 100 histogram counts

// librosa.piptrack's defaults fmin = 150, fmax = 4000: the bins with 150 <= k sr / n_fft < 4000
__host__ __device__ constexpr int band_lo(int n_fft) { return (150 * n_fft + SR - 1) / SR; }
__host__ __device__ constexpr int band_hi(int n_fft) { return (4000 * n_fft - 1) / SR; }
__host__ __device__ constexpr int band_width(int n_fft) { return band_hi(n_fft) - band_lo(n_fft) + 1; }
static_assert(band_lo(2048) >= 1 && band_hi(2048) < 1024 && band_lo(1024) >= 1 && band_hi(1024) < 512, "the band has both neighbours");
static_assert(band_width(2048) <= 512 && band_width(1024) <= 512, "two candidate bins per thread");

// the clip's sample count: its own, cut to its partner's where there is one (evaluation_reconstruction.py:193-204)
__device__ __forceinline__ int cut_count(const int32_t* __restrict__ n_samples, int n, const int32_t* __restrict__ n_cut, int cut_max,
                                         int b, int lo) {
  return min(clip_count(n_samples, b, lo, n), clip_count(n_cut, b, lo, cut_max));
}

// ---- pass 1, librosa.piptrack with its defaults: run blockIdx.x (frames CH_RUN * run ...) of clip blockIdx.y.  S (the power
// spectrum for the tuning, the magnitudes for pitch_correlation) of the K bins goes to LDS; the frame's maximum is a block
// reduction (exact in any order); thread tid tests the candidate bins band_lo + tid and band_lo + tid + 256 against their
// neighbours in LDS.  TUNE: pitch and mag of the band go to ws[b][t][band], 0 where there is no peak.  Otherwise
// p[b][t] = (1 / K) sum_k pitch[k][t], summed in a fixed order (thread, DPP wave sum, the four waves in turn), and exactly 0 for
// the frames t >= T_b of the row.
template <bool WIDE, bool TUNE, bool REFLECT>
__global__ __launch_bounds__(256) void pitch_runs_kernel(const float* __restrict__ waves, int n, const int32_t* __restrict__ n_samples,
                                                          const int32_t* __restrict__ n_cut, int cut_max, int T_max,
                                                          float* __restrict__ pitch_out, float* __restrict__ mag_out) {
  using G = Bins<WIDE>;
  constexpr int LO = band_lo(G::N_FFT), HI = band_hi(G::N_FFT), BAND = HI - LO + 1;
  __shared__ float2 buf[2][NFFT];
  __shared__ float sp[G::K], red[2][4];
  const int run = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int L = cut_count(n_samples, n, n_cut, cut_max, b, REFLECT ? G::N_FFT / 2 + 1 : 1);
  const int T = 1 + L / G::HOP, t0 = run * CH_RUN;
  if (t0 >= T) {                                         // uniform over the workgroup, ahead of the first barrier
    if (!TUNE && tid < CH_RUN && t0 + tid < T_max) pitch_out[(size_t)b * T_max + t0 + tid] = 0.f;
    return;
  }
  const float* w = waves + (size_t)b * n;
  FrameConsts<WIDE> fc;
  fc.init(tid);
  for (int t = t0; t < min(t0 + CH_RUN, T_max); ++t) {
    if (t >= T) {                                        // uniform: only the row's frames behind the clip are left
      if (!TUNE && tid == 0) pitch_out[(size_t)b * T_max + t] = 0.f;
      continue;
    }
    const int cur = frame_fft<WIDE, REFLECT>(buf, w, t, G::HOP, L, tid, fc);   // its barriers also stand between the last frame's readers of sp and red and the writes below
    float mx = 0.f;
#pragma unroll
    for (int m = 0; m < G::OWN; ++m) {
      const float p = own_power<WIDE>(buf[cur], tid, m, fc), s = TUNE ? p : sqrtf(p);
      sp[tid + 256 * m] = s;
      mx = fmaxf(mx, s);
    }
    if (tid == 0) { const float p = last_power<WIDE>(buf[cur]), s = TUNE ? p : sqrtf(p); sp[G::K - 1] = s; mx = fmaxf(mx, s); }
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[0][tid >> 6] = mx;
    __syncthreads();
    const float ref = 0.1f * fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
    float psum = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int k = LO + tid + 256 * i;
      if (k <= HI) {
        const float s = sp[k], lower = sp[k - 1], upper = sp[k + 1];
        float pitch = 0.f, mag = 0.f;
        if (s > ref && s > lower && s >= upper) {
          const float avg = 0.5f * (upper - lower), den = 2.f * s - upper - lower;
          const float shift = avg / (den + (fabsf(den) < F32_TINY ? 1.f : 0.f));
          pitch = ((float)k + shift) * (float)SR / (float)G::N_FFT;
          mag = s + 0.5f * avg * shift;
        }
        if (TUNE) {
          const size_t at = ((size_t)b * T_max + t) * BAND + (k - LO);
          pitch_out[at] = pitch;
          mag_out[at] = mag;
        }
        psum += pitch;
      }
    }
    if (!TUNE) {
      psum = wave_sum(psum);
      if ((tid & 63) == 0) red[1][tid >> 6] = psum;
      __syncthreads();
      if (tid == 0) pitch_out[(size_t)b * T_max + t] = (((red[1][0] + red[1][1]) + red[1][2]) + red[1][3]) / (float)G::K;
    }
  }
}

// ---- pass 2, librosa.estimate_tuning as chroma_stft calls it (bins_per_octave 12, resolution 0.01): clip blockIdx.x.  The
// clip's T_b x band words of `mag` are one contiguous span; the candidates are the positive ones (a peak's mag is positive, every
// other slot holds 0).  Positive floats order as their bit patterns, so the median is a radix selection on uint32, eight bits a
// sweep, for the two middle ranks (n - 1) / 2 and n / 2 at once: hist[j] counts the next digit of the candidates that agree
// with rank j's prefix so far.  Integer counters in LDS; nothing depends on the order of the adds.
__global__ __launch_bounds__(TN_THREADS) void tuning_kernel(const float* __restrict__ pitch, const float* __restrict__ mag, int n,
                                                            const int32_t* __restrict__ n_samples, const int32_t* __restrict__ n_cut,
                                                            int cut_max, int lo, int hop, int T_max, int band, float* __restrict__ tuning,
                                                            int32_t* __restrict__ debug) {
  __shared__ unsigned hist[2][256], prefix[2], rank[2], total;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = 1 + cut_count(n_samples, n, n_cut, cut_max, b, lo) / hop;
  const size_t N = (size_t)T * band, base = (size_t)b * T_max * band;
  const uint32_t* mg = reinterpret_cast<const uint32_t*>(mag) + base;
  int32_t* dbg = debug ? debug + (size_t)b * DBG_WORDS : nullptr;
  unsigned mask = 0;
  if (tid < 2) prefix[tid] = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 512) hist[tid >> 8][tid & 255] = 0;
    __syncthreads();
    const unsigned p0 = prefix[0], p1 = prefix[1];
    for (size_t i0 = 0; i0 < N; i0 += 4 * TN_THREADS) {
      uint32_t v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { const size_t i = i0 + u * TN_THREADS + tid; v[u] = i < N ? mg[i] : 0u; }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (v[u] != 0u && v[u] < 0x7f800000u) {          // a positive finite float
          if ((v[u] & mask) == p0) atomicAdd(&hist[0][(v[u] >> shift) & 255], 1u);
          if ((v[u] & mask) == p1) atomicAdd(&hist[1][(v[u] >> shift) & 255], 1u);
        }
    }
    __syncthreads();
    if (tid < 2) {
      if (shift == 24) {                                 // the first sweep counts the candidates
        unsigned cnt = 0;
        for (int d = 0; d < 256; ++d) cnt += hist[0][d];
        rank[tid] = tid ? cnt / 2 : (cnt ? (cnt - 1) / 2 : 0);
        if (tid == 0) total = cnt;
      }
      unsigned r = rank[tid], d = 0;
      for (; d < 255 && r >= hist[tid][d]; ++d) r -= hist[tid][d];
      rank[tid] = r;
      prefix[tid] |= d << shift;
    }
    mask |= 255u << shift;
    __syncthreads();
    if (total == 0) {                                    // uniform: no candidate, the tuning is 0
      if (tid == 0) tuning[b] = 0.f;
      if (dbg) for (int i = tid; i < DBG_WORDS; i += TN_THREADS) dbg[i] = 0;
      return;
    }
  }
  // thr = the median: the mean of the two middle values (equal for an odd count), compared in double, so exact
  const double thr = 0.5 * ((double)__uint_as_float(prefix[0]) + (double)__uint_as_float(prefix[1]));
  if (tid < 100) hist[0][tid] = 0;
  __syncthreads();
  const float* pt = pitch + base;
  const float* mf = mag + base;
  for (size_t i0 = 0; i0 < N; i0 += 4 * TN_THREADS) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { const size_t i = i0 + u * TN_THREADS + tid; v[u] = i < N ? mf[i] : 0.f; }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (v[u] > 0.f && v[u] < INFINITY && (double)v[u] >= thr) {
        // the deviation from equal temperament in semitones, in [-0.5, 0.5): frac(12 log2(f / 27.5)), wrapped
        double r = 12.0 * log2((double)pt[i0 + u * TN_THREADS + tid] / 27.5);
        r -= floor(r);
        if (r >= 0.5) r -= 1.0;
        if (r == r) {
          // np.histogram over linspace(-0.5, 0.5, 101): bin i holds edge[i] <= r < edge[i + 1], edge[i] = i * 0.01 - 0.5
          int i = min(max((int)floor((r + 0.5) * 100.0), 0), 99);
          if (i > 0 && r < i * 0.01 + -0.5) --i;
          else if (i < 99 && r >= (i + 1) * 0.01 + -0.5) ++i;
          atomicAdd(&hist[0][i], 1u);
        }
      }
  }
  __syncthreads();
  if (tid == 0) {
    int arg = 0;
    for (int i = 1; i < 100; ++i) if (hist[0][i] > hist[0][arg]) arg = i;            // the lowest index wins ties
    tuning[b] = (float)(arg * 0.01 + -0.5);
  }
  if (dbg) {
    if (tid < 100) dbg[3 + tid] = (int32_t)hist[0][tid];
    if (tid == 0) {
      unsigned kept = 0;
      for (int i = 0; i < 100; ++i) kept += hist[0][i];
      dbg[0] = (int32_t)total;
      dbg[1] = (int32_t)kept;
      dbg[2] = __float_as_int((float)thr);
    }
  }
}

// column k of librosa.filters.chroma(sr, n_fft, tuning) with its defaults (12 rows, ctroct 5, octwidth 2, norm 2, base_c), rows
// already rolled so that w[0] is C.  The positions q come from double logarithms (q reaches 104, where a float's 8e-6 would
// show in the Gaussians); everything behind them is float.  Local to the column and the next.
__device__ __forceinline__ void chroma_column(int k, int n_fft, double tuning, float (&w)[N_CHROMA]) {
  const double hz = (double)SR / n_fft;
  const double q_next = 12.0 * log2((k + 1) * hz / 27.5) - tuning;
  const double q = k ? 12.0 * log2(k * hz / 27.5) - tuning : q_next - 18.0;
  const double width = fmax(q_next - q, 1.0);
  float g[N_CHROMA], s2 = 0.f;
#pragma unroll
  for (int c = 0; c < N_CHROMA; ++c) {
    const float a = (float)(2.0 * (fmod(q - c + 126.0, 12.0) - 6.0) / width);
    g[c] = expf(-0.5f * a * a);
    s2 += g[c] * g[c];
  }
  const float o = (float)((q / 12.0 - 5.0) / 2.0);
  const float scale = expf(-0.5f * o * o) / sqrtf(s2);
#pragma unroll
  for (int c = 0; c < N_CHROMA; ++c) w[c] = g[(c + 3) % N_CHROMA] * scale;
}

// ---- pass 3, librosa.feature.chroma_stft: run blockIdx.x of clip blockIdx.y -> out[b][c][t], layout (B, 12, T_max).  Thread tid
// computes the 12 weights of each bin it owns once, from tuning[b], and keeps them in registers like the window and the twiddles.
// Per frame: the transform again, raw[c] = sum_k w[c][k] |X[k]|^2 (the thread's bins ascending, DPP wave sum, the four waves in
// turn), divided by the frame's maximum over c unless that is below float32 tiny.  The run's 12 x CH_RUN values wait in LDS and
// are stored row by row; every element of out is written: frames t >= T_b are exactly 0.
template <bool WIDE, bool REFLECT>
__global__ __launch_bounds__(256) void chroma_runs_kernel(const float* __restrict__ waves, int n, const int32_t* __restrict__ n_samples,
                                                           const int32_t* __restrict__ n_cut, int cut_max, const float* __restrict__ tuning,
                                                           int T_max, float* __restrict__ out) {
  using G = Bins<WIDE>;
  __shared__ float2 buf[2][NFFT];
  __shared__ float red[4][N_CHROMA], cs[N_CHROMA][CH_RUN];
  const int run = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int L = cut_count(n_samples, n, n_cut, cut_max, b, REFLECT ? G::N_FFT / 2 + 1 : 1);
  const int T = 1 + L / G::HOP, t0 = run * CH_RUN;
  if (t0 < T) {                                          // uniform over the workgroup
    const float* w = waves + (size_t)b * n;
    const double tune = (double)tuning[b];
    FrameConsts<WIDE> fc;
    fc.init(tid);
    float wt[G::OWN][N_CHROMA], wl[N_CHROMA] = {};
#pragma unroll
    for (int m = 0; m < G::OWN; ++m) chroma_column(tid + 256 * m, G::N_FFT, tune, wt[m]);
    if (tid == 0) chroma_column(G::K - 1, G::N_FFT, tune, wl);   // the last bin is thread 0's
    for (int t = t0; t < min(t0 + CH_RUN, T); ++t) {
      const int cur = frame_fft<WIDE, REFLECT>(buf, w, t, G::HOP, L, tid, fc);   // its barriers also stand between the last frame's readers of red and the writes below
      float acc[N_CHROMA];
#pragma unroll
      for (int c = 0; c < N_CHROMA; ++c) acc[c] = 0.f;
#pragma unroll
      for (int m = 0; m < G::OWN; ++m) {
        const float p = own_power<WIDE>(buf[cur], tid, m, fc);
#pragma unroll
        for (int c = 0; c < N_CHROMA; ++c) acc[c] += wt[m][c] * p;
      }
      if (tid == 0) {
        const float p = last_power<WIDE>(buf[cur]);
#pragma unroll
        for (int c = 0; c < N_CHROMA; ++c) acc[c] += wl[c] * p;
      }
#pragma unroll
      for (int c = 0; c < N_CHROMA; ++c) {
        const float s = wave_sum(acc[c]);
        if ((tid & 63) == 0) red[tid >> 6][c] = s;
      }
      __syncthreads();
      if (tid < N_CHROMA) {
        float mine = 0.f, mx = 0.f;
#pragma unroll
        for (int c = 0; c < N_CHROMA; ++c) {
          const float raw = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
          mx = fmaxf(mx, fabsf(raw));
          if (c == tid) mine = raw;
        }
        cs[tid][t - t0] = mx < F32_TINY ? mine : mine / mx;
      }
    }
    __syncthreads();
  }
  for (int i = tid; i < N_CHROMA * CH_RUN; i += 256) {
    const int c = i / CH_RUN, t = t0 + i % CH_RUN;
    if (t < T_max) out[((size_t)b * N_CHROMA + c) * T_max + t] = t < T ? cs[c][t - t0] : 0.f;
  }
}

// ---- finishers.  The frame count of pair b: both clips' own counts give T = min(T_a, T_g); cutting both clips to the shorter
// one's samples first (chroma_distance, pitch_correlation) gives the same T, as T(n) is monotonic.
__device__ __forceinline__ int pair_frames(const int32_t* __restrict__ len_a, int n_a, const int32_t* __restrict__ len_g, int n_g, int b,
                                           int lo, int hop) {
  return 1 + min(clip_count(len_a, b, lo, n_a), clip_count(len_g, b, lo, n_g)) / hop;
}

// chroma_distance: out[b] = mean over t < T of ||a[b][:, t] - g[b][:, t]||_2; thread-strided sums of the frames' distances in
// double, then block_sum_f64.  a (B, 12, Ta), g (B, 12, Tg).
__global__ __launch_bounds__(256) void chroma_dist_kernel(const float* __restrict__ a, int n_a, const int32_t* __restrict__ len_a, int Ta,
                                                          const float* __restrict__ g, int n_g, const int32_t* __restrict__ len_g, int Tg,
                                                          int lo, int hop, float* __restrict__ out) {
  __shared__ double red[257];
  const int b = blockIdx.x;
  const int T = pair_frames(len_a, n_a, len_g, n_g, b, lo, hop);
  double s = 0.0;
  for (int t = threadIdx.x; t < T; t += 256) {
    float d2 = 0.f;
#pragma unroll
    for (int c = 0; c < N_CHROMA; ++c) {
      const float d = a[((size_t)b * N_CHROMA + c) * Ta + t] - g[((size_t)b * N_CHROMA + c) * Tg + t];
      d2 += d * d;
    }
    s += (double)sqrtf(d2);
  }
  s = block_sum_f64(s, red);
  if (threadIdx.x == 0) out[b] = (float)(s / (double)T);
}

// chroma_similarity (R = 12) and pitch_correlation (R = 1): Pearson's r (pearson_r, spec_common.h) of rows
// a[b][r][:T] and g[b][r][:T] for every r < R; out[b] = the mean of the finite ones, exactly 0 if there is none (a constant
// row, T < 2).  a (B, R, Ta), g (B, R, Tg).
__global__ __launch_bounds__(256) void pearson_frames_kernel(const float* __restrict__ a, int n_a, const int32_t* __restrict__ len_a, int Ta,
                                                             const float* __restrict__ g, int n_g, const int32_t* __restrict__ len_g, int Tg,
                                                             int lo, int hop, int R, float* __restrict__ out) {
  __shared__ double red[257];
  const int b = blockIdx.x;
  const int T = pair_frames(len_a, n_a, len_g, n_g, b, lo, hop);
  double tot = 0.0;
  int kept = 0;
  for (int r = 0; r < R; ++r) {
    bool counts;
    const double rr = pearson_r(a + ((size_t)b * R + r) * Ta, g + ((size_t)b * R + r) * Tg, T, red, counts);
    if (counts) { tot += rr; ++kept; }
  }
  if (threadIdx.x == 0) out[b] = kept ? (float)(tot / kept) : 0.f;
}

// ---- host
int ch_runs(int n, int hop) { return runs_of(frames_of(n, hop), CH_RUN); }
// the two settings of the evaluation scripts: 0, or -1 with the message of entry `name` set
int setting_check(const char* name, int n_fft, int hop) {
  if (!((n_fft == 2048 && hop == 512) || (n_fft == 1024 && hop == 256)))
    AST_FAIL("%s: (n_fft, hop) must be (2048, 512) or (1024, 256), got (%d, %d)", name, n_fft, hop);
  return 0;
}
// a clip and the partner it is cut to: the row checks of both widths
int cut_check(const char* name, int B, int n, int cut_max, int n_fft, int pad_mode) {
  return rows_check(name, B, n, n_fft, pad_mode) || rows_check(name, B, cut_max, n_fft, pad_mode) ? -1 : 0;
}
long tuning_floats(int B, int n, int n_fft) { return 2l * B * frames_of(n, n_fft / 4) * band_width(n_fft); }

// passes 1 and 2 (checked arguments): ws holds tuning_floats(B, n, n_fft) floats
void tuning_launch(const float* waves, int B, int n, const int32_t* n_samples, const int32_t* n_cut, int cut_max, int n_fft, int pad_mode,
                   float* ws, float* tuning, int32_t* debug, hipStream_t s) {
  const int hop = n_fft / 4, T_max = frames_of(n, hop), band = band_width(n_fft);
  float* pitch = ws;
  float* mag = ws + (size_t)B * T_max * band;
  const dim3 grid(ch_runs(n, hop), B);
  if (n_fft == 2048) PAD_LAUNCH(pad_mode, (pitch_runs_kernel<true, true, R>), grid, dim3(256), s, waves, n, n_samples, n_cut, cut_max, T_max, pitch, mag);
  else PAD_LAUNCH(pad_mode, (pitch_runs_kernel<false, true, R>), grid, dim3(256), s, waves, n, n_samples, n_cut, cut_max, T_max, pitch, mag);
  hipLaunchKernelGGL(tuning_kernel, dim3(B), dim3(TN_THREADS), 0, s, (const float*)pitch, (const float*)mag, n, n_samples, n_cut, cut_max,
                     min_count(pad_mode, n_fft), hop, T_max, band, tuning, debug);
}
// pass 3 (checked arguments)
void chroma_launch(const float* waves, int B, int n, const int32_t* n_samples, const int32_t* n_cut, int cut_max, int n_fft, int pad_mode,
                   const float* tuning, float* out, hipStream_t s) {
  const int hop = n_fft / 4, T_max = frames_of(n, hop);
  const dim3 grid(ch_runs(n, hop), B);
  if (n_fft == 2048) PAD_LAUNCH(pad_mode, (chroma_runs_kernel<true, R>), grid, dim3(256), s, waves, n, n_samples, n_cut, cut_max, tuning, T_max, out);
  else PAD_LAUNCH(pad_mode, (chroma_runs_kernel<false, R>), grid, dim3(256), s, waves, n, n_samples, n_cut, cut_max, tuning, T_max, out);
}
void pitch_mean_launch(const float* waves, int B, int n, const int32_t* n_samples, const int32_t* n_cut, int cut_max, int pad_mode, float* out,
                       hipStream_t s) {
  PAD_LAUNCH(pad_mode, (pitch_runs_kernel<true, false, R>), dim3(ch_runs(n, 512), B), dim3(256), s, waves, n, n_samples, n_cut, cut_max,
             frames_of(n, 512), out, (float*)nullptr);
}
// floats of a pair's chroma scores: the peaks of the wider batch (the two batches use them in turn), 2 B tunings, both chromas
long chroma_pair_floats(int B, int n_a, int n_g, int n_fft) {
  const int hop = n_fft / 4;
  return tuning_floats(B, std::max(n_a, n_g), n_fft) + 2l * B + (long)B * N_CHROMA * (frames_of(n_a, hop) + frames_of(n_g, hop));
}
// both clips' chromas into ws (checked arguments); cut: each clip is cut to its partner's count first.  Returns where they start.
void chroma_pair_launch(const float* a, int n_a, const int32_t* len_a, const float* g, int n_g, const int32_t* len_g, int B, int n_fft, bool cut,
                        int pad_mode, float* ws, float** chroma_a, float** chroma_g, hipStream_t s) {
  const int hop = n_fft / 4;
  float* tune = ws + tuning_floats(B, std::max(n_a, n_g), n_fft);
  *chroma_a = tune + 2 * (size_t)B;
  *chroma_g = *chroma_a + (size_t)B * N_CHROMA * frames_of(n_a, hop);
  tuning_launch(a, B, n_a, len_a, cut ? len_g : nullptr, cut ? n_g : n_a, n_fft, pad_mode, ws, tune, nullptr, s);
  chroma_launch(a, B, n_a, len_a, cut ? len_g : nullptr, cut ? n_g : n_a, n_fft, pad_mode, tune, *chroma_a, s);
  tuning_launch(g, B, n_g, len_g, cut ? len_a : nullptr, cut ? n_a : n_g, n_fft, pad_mode, ws, tune + B, nullptr, s);
  chroma_launch(g, B, n_g, len_g, cut ? len_a : nullptr, cut ? n_a : n_g, n_fft, pad_mode, tune + B, *chroma_g, s);
}
}  // namespace

extern "C" int ast_chroma_run_frames(void) { return CH_RUN; }
extern "C" int ast_tuning_debug_words(void) { return DBG_WORDS; }

extern "C" int ast_pitch_band(int n_fft, int* k_lo, int* k_hi) {
  if (!k_lo || !k_hi) AST_FAIL("ast_pitch_band: null pointer");
  if (n_fft != 2048 && n_fft != 1024) AST_FAIL("ast_pitch_band: n_fft must be 2048 or 1024, got %d", n_fft);
  *k_lo = band_lo(n_fft);
  *k_hi = band_hi(n_fft);
  return 0;
}

extern "C" long ast_tuning_ws_floats(int B, int n, int n_fft) {
  if (B < 1 || n < 1 || (n_fft != 2048 && n_fft != 1024)) return 0;
  return tuning_floats(B, n, n_fft);
}

extern "C" int ast_tuning_len(const float* waves, int B, int n, const int32_t* n_samples, const int32_t* n_cut, int cut_max, int n_fft, int hop,
                              int pad_mode, float* ws, long ws_floats, float* tuning, int32_t* debug, void* stream) {
  const char* me = "ast_tuning_len";
  if (!waves || !tuning) AST_FAIL("%s: null pointer", me);
  if (setting_check(me, n_fft, hop) || cut_check(me, B, n, cut_max, n_fft, pad_mode)) return -1;
  if (ws_check(me, ws, ws_floats, tuning_floats(B, n, n_fft))) return -1;
  tuning_launch(waves, B, n, n_samples, n_cut, cut_max, n_fft, pad_mode, ws, tuning, debug, (hipStream_t)stream);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" int ast_chroma_len(const float* waves, int B, int n, const int32_t* n_samples, const int32_t* n_cut, int cut_max, int n_fft, int hop,
                              int pad_mode, const float* tuning, float* out, void* stream) {
  const char* me = "ast_chroma_len";
  if (!waves || !tuning || !out) AST_FAIL("%s: null pointer", me);
  if (setting_check(me, n_fft, hop) || cut_check(me, B, n, cut_max, n_fft, pad_mode)) return -1;
  chroma_launch(waves, B, n, n_samples, n_cut, cut_max, n_fft, pad_mode, tuning, out, (hipStream_t)stream);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" long ast_chroma_distance_ws_floats(int B, int n_orig, int n_gen) {
  if (B < 1 || n_orig < 1 || n_gen < 1) return 0;
  return chroma_pair_floats(B, n_orig, n_gen, 2048);
}

extern "C" int ast_chroma_distance_len(const float* original, int n_orig, const float* generated, int n_gen, int B, const int32_t* len_orig,
                                       const int32_t* len_gen, int pad_mode, float* ws, long ws_floats, float* out, void* stream) {
  const char* me = "ast_chroma_distance_len";
  if (!original || !generated || !out) AST_FAIL("%s: null pointer", me);
  if (cut_check(me, B, n_orig, n_gen, 2048, pad_mode)) return -1;
  if (ws_check(me, ws, ws_floats, chroma_pair_floats(B, n_orig, n_gen, 2048))) return -1;
  hipStream_t s = (hipStream_t)stream;
  float *ca, *cg;
  chroma_pair_launch(original, n_orig, len_orig, generated, n_gen, len_gen, B, 2048, true, pad_mode, ws, &ca, &cg, s);
  hipLaunchKernelGGL(chroma_dist_kernel, dim3(B), dim3(256), 0, s, (const float*)ca, n_orig, len_orig, frames_of(n_orig, 512), (const float*)cg,
                     n_gen, len_gen, frames_of(n_gen, 512), min_count(pad_mode, 2048), 512, out);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" long ast_chroma_similarity_ws_floats(int B, int n_gen, int n_orig) {
  if (B < 1 || n_orig < 1 || n_gen < 1) return 0;
  return chroma_pair_floats(B, n_gen, n_orig, 1024);
}

extern "C" int ast_chroma_similarity_len(const float* generated, int n_gen, const float* original, int n_orig, int B, const int32_t* len_gen,
                                         const int32_t* len_orig, int pad_mode, float* ws, long ws_floats, float* out, void* stream) {
  const char* me = "ast_chroma_similarity_len";
  if (!original || !generated || !out) AST_FAIL("%s: null pointer", me);
  if (cut_check(me, B, n_gen, n_orig, 1024, pad_mode)) return -1;
  if (ws_check(me, ws, ws_floats, chroma_pair_floats(B, n_gen, n_orig, 1024))) return -1;
  hipStream_t s = (hipStream_t)stream;
  float *cg, *co;
  chroma_pair_launch(generated, n_gen, len_gen, original, n_orig, len_orig, B, 1024, false, pad_mode, ws, &cg, &co, s);
  hipLaunchKernelGGL(pearson_frames_kernel, dim3(B), dim3(256), 0, s, (const float*)cg, n_gen, len_gen, frames_of(n_gen, 256), (const float*)co,
                     n_orig, len_orig, frames_of(n_orig, 256), min_count(pad_mode, 1024), 256, N_CHROMA, out);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" int ast_pitch_mean_len(const float* waves, int B, int n, const int32_t* n_samples, const int32_t* n_cut, int cut_max, int pad_mode,
                                  float* out, void* stream) {
  const char* me = "ast_pitch_mean_len";
  if (!waves || !out) AST_FAIL("%s: null pointer", me);
  if (cut_check(me, B, n, cut_max, 2048, pad_mode)) return -1;
  pitch_mean_launch(waves, B, n, n_samples, n_cut, cut_max, pad_mode, out, (hipStream_t)stream);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" long ast_pitch_correlation_ws_floats(int B, int n_orig, int n_gen) {
  if (B < 1 || n_orig < 1 || n_gen < 1) return 0;
  return (long)B * (frames_of(n_orig, 512) + frames_of(n_gen, 512));
}

extern "C" int ast_pitch_correlation_len(const float* original, int n_orig, const float* generated, int n_gen, int B, const int32_t* len_orig,
                                         const int32_t* len_gen, int pad_mode, float* ws, long ws_floats, float* out, void* stream) {
  const char* me = "ast_pitch_correlation_len";
  if (!original || !generated || !out) AST_FAIL("%s: null pointer", me);
  if (cut_check(me, B, n_orig, n_gen, 2048, pad_mode)) return -1;
  const int To = frames_of(n_orig, 512), Tg = frames_of(n_gen, 512);
  if (ws_check(me, ws, ws_floats, (long)B * (To + Tg))) return -1;
  hipStream_t s = (hipStream_t)stream;
  float* po = ws;
  float* pg = ws + (size_t)B * To;
  pitch_mean_launch(original, B, n_orig, len_orig, len_gen, n_gen, pad_mode, po, s);
  pitch_mean_launch(generated, B, n_gen, len_gen, len_orig, n_orig, pad_mode, pg, s);
  hipLaunchKernelGGL(pearson_frames_kernel, dim3(B), dim3(256), 0, s, (const float*)po, n_orig, len_orig, To, (const float*)pg, n_gen, len_gen, Tg,
                     min_count(pad_mode, 2048), 512, 1, out);
  AST_CHECK_LAUNCH();
  return 0;
}
