// Dataset screening of the reference's Preprocessing_Dataset scripts for a padded batch of clips of different lengths:
//   silent_tracks_dataset.py:20-27     librosa.feature.rms(y)[0] at its defaults and the share of frames with rms < 0.005
//   dataset_tracks_analysis.py:25-29   the clip level sqrt(mean(y^2)) and mean(librosa.feature.mfcc(y, sr, n_mfcc=13), axis=1)
//   dataset_variety.py:13-16           the same MFCC time-mean as the feature vector of a track
//   unifies_violin_datasets.py:25-30   rms_normalize(y, 0.07): y * target / level, y itself where the level is 0
//   split_BachViolinDataset.py:24-30   is_mostly_sound: the share of 100 ms windows whose level is above -45 dBFS
// The rules of metrics.hip hold: no atomics, one owner and a fixed order of summation per output, per-clip counts clamped on the
// device, samples behind a clip's end never read, no synchronisation and no allocation in an entry.
//
// Frame RMS rests on one identity: with frame_length 2048 = 4 x hop_length 512 and centred frames, frame t covers the padded clip's
// samples [512 t - 1024, 512 t + 1024), which are the four hop blocks t - 2 .. t + 1 (block j = samples [512 j, 512 j + 512)).  So a
// workgroup reads every sample of its span once, forms one sum of squares per block, and a frame is four block sums.
// The MFCC time-mean rests on another: the DCT is linear, so mean_t(mfcc)[k] is the DCT of the time-mean of the clamped dB rows;
// the (B, n_mfcc, T) coefficients never exist.
#include "spec_common.h"

namespace {
constexpr int RMS_FRAME = 2048, RMS_HOP = 512;           // librosa.feature.rms defaults: frame_length, hop_length
constexpr int RMS_TILE = 32;                             // consecutive frames of one clip per workgroup
constexpr int MM_CHUNK = 32;                             // frames per partial of the mel-mean pass
constexpr int MM_MAX_MFCC = 20;                          // librosa's default n_mfcc; the scripts ask for 13

// ---- 1. frame RMS, silent frames, clip level
// The sum of squares of hop block j, wave-wide: lane l owns the samples 4 l .. 4 l + 3 and 256 + 4 l .. 256 + 4 l + 3 of the block,
// squares and adds them as a fixed tree, then the DPP wave sum.  A block that lies inside the clip at a 16-byte aligned address is
// read as two float4 per lane, any other one sample at a time under the pad mode; the values then take the same instructions, so a
// clip's results do not depend on its row's alignment.  padded: under the pad mode (what the frames use); own: the clip's own
// samples alone (what the level uses) -- they differ only under reflect padding in the block that holds the clip's end.
__device__ __forceinline__ float tree8(const float (&v)[8]) {
  return ((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3])) + ((v[4] * v[4] + v[5] * v[5]) + (v[6] * v[6] + v[7] * v[7]));
}
template <bool REFLECT>
__device__ __forceinline__ void hop_block_sums(const float* __restrict__ w, int j, int L, int lane, float& padded, float& own) {
  const int base = RMS_HOP * j + 4 * lane;
  const bool inside = j >= 0 && RMS_HOP * (j + 1) <= L;  // uniform over the wave
  float v[8];
  if (inside && (reinterpret_cast<uintptr_t>(w + RMS_HOP * j) & 15) == 0) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(w + base), c = *reinterpret_cast<const f32x4*>(w + base + 256);
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[i] = a[i]; v[4 + i] = c[i]; }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = clip_sample<REFLECT>(w, base + (i & 3) + 256 * (i >> 2), L);
  }
  padded = wave_sum(tree8(v));
  own = padded;
  if (REFLECT && !inside) {                              // reflected samples are not the clip's own
#pragma unroll
    for (int i = 0; i < 8; ++i) { const int idx = base + (i & 3) + 256 * (i >> 2); v[i] = (idx >= 0 && idx < L) ? v[i] : 0.f; }
    own = wave_sum(tree8(v));
  }
}

// frames RMS_TILE * blockIdx.x ... of clip blockIdx.y.  The tile's RMS_TILE + 3 hop blocks are shared out over the four waves; then
// thread f < RMS_TILE adds frame t0 + f's four block sums in ascending block order.  Every element of rms is written: 0 for
// t >= T_b.  tile_silent: the tile's frames t < T_b with rms < threshold (a ballot's popcount); tile_sum: the sum of squares of the
// clip's own samples in the hop blocks t0 .. t0 + RMS_TILE - 1, the block sums added ascending in double.
template <bool REFLECT>
__global__ __launch_bounds__(256) void frame_rms_tiles_kernel(const float* __restrict__ waves, int n, const int32_t* __restrict__ n_samples,
                                                               float threshold, int T_max, int n_tiles, float* __restrict__ rms,
                                                               int32_t* __restrict__ tile_silent, double* __restrict__ tile_sum) {
  __shared__ float bs[RMS_TILE + 3], us[RMS_TILE];
  const int t0 = blockIdx.x * RMS_TILE, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int L = clip_count(n_samples, b, REFLECT ? RMS_FRAME / 2 + 1 : 1, n);
  const int T = 1 + L / RMS_HOP;
  if (t0 >= T) {                                         // uniform over the workgroup: nothing of the clip is read
    if (tid < RMS_TILE && t0 + tid < T_max) rms[(size_t)b * T_max + t0 + tid] = 0.f;
    return;
  }
  const float* w = waves + (size_t)b * n;
  const int j_last = min(t0 + RMS_TILE + 1, T);          // the last block a frame t < T_b of this tile covers
  for (int i = tid >> 6; i < RMS_TILE + 3; i += 4) {
    const int j = t0 - 2 + i;
    float padded = 0.f, own = 0.f;
    if (j <= j_last && (REFLECT || j >= 0)) hop_block_sums<REFLECT>(w, j, L, lane, padded, own);
    if (lane == 0) {
      bs[i] = padded;
      if (i >= 2 && i < RMS_TILE + 2) us[i - 2] = own;
    }
  }
  __syncthreads();
  if (tid < 64) {
    const int t = t0 + tid;
    bool silent = false;
    if (tid < RMS_TILE && t < T_max) {
      float r = 0.f;
      if (t < T) {
        r = sqrtf((((bs[tid] + bs[tid + 1]) + bs[tid + 2]) + bs[tid + 3]) * (1.f / RMS_FRAME));
        silent = r < threshold;
      }
      rms[(size_t)b * T_max + t] = r;
    }
    const unsigned long long m = __ballot(silent);
    if (tid == 0) {
      double s = 0.0;
      for (int i = 0; i < RMS_TILE; ++i) s += (double)us[i];
      tile_silent[(size_t)b * n_tiles + blockIdx.x] = __popcll(m);
      tile_sum[(size_t)b * n_tiles + blockIdx.x] = s;
    }
  }
}

// clip blockIdx.x: its tiles' partials added in ascending order by one thread; the level is rounded from double once
__global__ __launch_bounds__(64) void frame_rms_finish_kernel(const int32_t* __restrict__ tile_silent, const double* __restrict__ tile_sum, int n,
                                                              const int32_t* __restrict__ n_samples, int lo, int n_tiles,
                                                              int32_t* __restrict__ n_frames, int32_t* __restrict__ silent,
                                                              float* __restrict__ ratio, float* __restrict__ level, double* __restrict__ sumsq) {
  if (threadIdx.x != 0) return;
  const int b = blockIdx.x;
  const int L = clip_count(n_samples, b, lo, n);
  const int T = 1 + L / RMS_HOP;
  int c = 0;
  double s = 0.0;
  for (int i = 0; i < (T + RMS_TILE - 1) / RMS_TILE; ++i) {
    c += tile_silent[(size_t)b * n_tiles + i];
    s += tile_sum[(size_t)b * n_tiles + i];
  }
  n_frames[b] = T;
  silent[b] = c;
  ratio[b] = (float)((double)c / (double)T);
  level[b] = (float)sqrt(s / (double)L);
  if (sumsq) sumsq[b] = s;
}

// ---- 2. window levels: window 4 blockIdx.x + wave of clip blockIdx.y, one wave per window.  Lane l adds the squares of the window's
// samples l, l + 64, ... ascending, then the DPP wave sum.  Every element of mask is written: 0 for w >= W_b = L_b / win.
__global__ __launch_bounds__(256) void window_sound_kernel(const float* __restrict__ waves, int n, const int32_t* __restrict__ n_samples, int win,
                                                           float threshold_db, int W_max, int32_t* __restrict__ mask) {
  const int wi = 4 * blockIdx.x + (threadIdx.x >> 6), b = blockIdx.y, lane = threadIdx.x & 63;
  if (wi >= W_max) return;                               // uniform over the wave; the kernel has no barrier
  const int W = clip_count(n_samples, b, 1, n) / win;
  int sound = 0;
  if (wi < W) {
    const float* x = waves + (size_t)b * n + (size_t)wi * win;
    float s = 0.f;
    for (int i = lane; i < win; i += 64) s += x[i] * x[i];
    const float r = sqrtf(wave_sum(s) / (float)win);
    sound = r > 0.f && 20.f * log10f(r) > threshold_db;
  }
  if (lane == 0) mask[(size_t)b * W_max + wi] = sound;
}

// ratio[b] = the clip's sound windows / W_b, exactly 0 when W_b = 0: integer counts, thread 0 adds the 256 partial counts
__global__ __launch_bounds__(256) void window_ratio_kernel(const int32_t* __restrict__ mask, int n, const int32_t* __restrict__ n_samples, int win,
                                                           int W_max, float* __restrict__ ratio) {
  __shared__ int cnt[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int W = clip_count(n_samples, b, 1, n) / win;
  int c = 0;
  for (int i = tid; i < W; i += 256) c += mask[(size_t)b * W_max + i] != 0;
  cnt[tid] = c;
  __syncthreads();
  if (tid == 0) {
    int tot = 0;
    for (int i = 0; i < 256; ++i) tot += cnt[i];
    ratio[b] = W > 0 ? (float)((double)tot / (double)W) : 0.f;
  }
}

// ---- 3. MFCC time-mean.  Chunk blockIdx.x (frames MM_CHUNK * chunk ...) of clip blockIdx.y: thread j owns mel band j and adds
// max(dB[t][j], clip maximum - 80) over the chunk's frames t < T_b ascending.  part[b][chunk][128]
__global__ __launch_bounds__(128) void mel_mean_chunks_kernel(const float* __restrict__ db, const float* __restrict__ run_max, int n,
                                                              const int32_t* __restrict__ n_samples, int lo, int hop, int T_max, int n_runs,
                                                              int n_chunks, float* __restrict__ part) {
  __shared__ float red[2];
  const int t0 = blockIdx.x * MM_CHUNK, b = blockIdx.y, tid = threadIdx.x;
  const int T = 1 + clip_count(n_samples, b, lo, n) / hop;
  if (t0 >= T) return;                                   // uniform over the workgroup, ahead of the barrier
  const float floor_db = clip_max_db<128>(run_max + (size_t)b * n_runs, (T + MF_RUN - 1) / MF_RUN, red) - TOP_DB;
  const float* row = db + ((size_t)b * T_max + t0) * MEL_N + tid;
  float s = 0.f;
  for (int t = 0; t < min(MM_CHUNK, T - t0); ++t) s += fmaxf(row[(size_t)t * MEL_N], floor_db);
  part[((size_t)b * n_chunks + blockIdx.x) * MEL_N + tid] = s;
}

// clip blockIdx.x: thread j adds band j's chunks ascending in double and divides by T_b; thread k < n_mfcc then takes coefficient k
// of the orthonormal DCT-II of the 128 means in double, summed over j ascending (dct_phase, dct_scale: spec_common.h)
__global__ __launch_bounds__(128) void mfcc_mean_finish_kernel(const float* __restrict__ part, int n, const int32_t* __restrict__ n_samples, int lo,
                                                               int hop, int n_chunks, int n_mfcc, float* __restrict__ out) {
  __shared__ double mean[MEL_N];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = 1 + clip_count(n_samples, b, lo, n) / hop;
  double s = 0.0;
  for (int c = 0; c < (T + MM_CHUNK - 1) / MM_CHUNK; ++c) s += (double)part[((size_t)b * n_chunks + c) * MEL_N + tid];
  mean[tid] = s / (double)T;
  __syncthreads();
  if (tid < n_mfcc) {
    double a = 0.0;
    for (int j = 0; j < MEL_N; ++j) a += mean[j] * cospi((double)dct_phase(tid, j) / 256.0);
    out[(size_t)b * n_mfcc + tid] = (float)(a * dct_scale<double>(tid));
  }
}

// ---- 4. gain: out[b][i] = waves[b][i] * g_b for i < L_b, 0 behind; g_b = target / sqrt(sumsq[b] / L_b) in double, rounded once,
// 1 where the level is 0.  Every element has one thread that reads and then writes it, so out may be waves.
__global__ __launch_bounds__(256) void gain_rows_kernel(const float* waves, int n, const int32_t* __restrict__ n_samples,
                                                        const double* __restrict__ sumsq, double target, float* out) {
  const int b = blockIdx.y;
  const int L = clip_count(n_samples, b, 1, n);
  const double level = sqrt(sumsq[b] / (double)L);
  const float g = level > 0.0 ? (float)(target / level) : 1.f;
  const size_t row = (size_t)b * n;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = blockIdx.x * 1024 + threadIdx.x + 256 * k;             // n + 1024 stays below 2^31 (rows_check)
    if (i < n) out[row + i] = i < L ? waves[row + i] * g : 0.f;
  }
}

// host
int rms_tiles(int n) { return runs_of(frames_of(n, RMS_HOP), RMS_TILE); }
long rms_ws_floats(int B, int n) { return 3L * B * rms_tiles(n); }            // a double and an int32 per tile
int mm_chunks(int n, int hop) { return runs_of(frames_of(n, hop), MM_CHUNK); }
long mm_ws_floats(int B, int n, int hop) { return mfcc_pass1_floats(B, n, hop) + (long)B * mm_chunks(n, hop) * MEL_N; }
}  // namespace

extern "C" int ast_frame_rms_tile_frames(void) { return RMS_TILE; }
extern "C" int ast_mfcc_mean_chunk_frames(void) { return MM_CHUNK; }

extern "C" long ast_frame_rms_ws_floats(int B, int n) { return (B < 1 || n < 1) ? 0 : rms_ws_floats(B, n); }

extern "C" int ast_frame_rms_len(const float* waves, int B, int n, const int32_t* n_samples, float threshold, int pad_mode, float* ws,
                                 long ws_floats, float* rms, int32_t* n_frames, int32_t* silent, float* silence_ratio, float* level,
                                 double* sumsq, void* stream) {
  const char* me = "ast_frame_rms_len";
  if (!waves || !rms || !n_frames || !silent || !silence_ratio || !level) AST_FAIL("%s: null pointer", me);
  if (rows_check(me, B, n, RMS_FRAME, pad_mode)) return -1;
  if (ws_check(me, ws, ws_floats, rms_ws_floats(B, n))) return -1;
  if (reinterpret_cast<uintptr_t>(ws) & 7) AST_FAIL("%s: the workspace must be 8-byte aligned (it holds doubles)", me);
  hipStream_t s = (hipStream_t)stream;
  const int T_max = frames_of(n, RMS_HOP), n_tiles = rms_tiles(n);
  double* tile_sum = reinterpret_cast<double*>(ws);
  int32_t* tile_silent = reinterpret_cast<int32_t*>(tile_sum + (size_t)B * n_tiles);
  PAD_LAUNCH(pad_mode, (frame_rms_tiles_kernel<R>), dim3(n_tiles, B), dim3(256), s, waves, n, n_samples, threshold, T_max, n_tiles, rms, tile_silent,
             tile_sum);
  hipLaunchKernelGGL(frame_rms_finish_kernel, dim3(B), dim3(64), 0, s, (const int32_t*)tile_silent, (const double*)tile_sum, n, n_samples,
                     min_count(pad_mode, RMS_FRAME), n_tiles, n_frames, silent, silence_ratio, level, sumsq);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" int ast_window_sound_len(const float* waves, int B, int n, const int32_t* n_samples, int win, float threshold_db, int32_t* mask,
                                    float* sound_ratio, void* stream) {
  const char* me = "ast_window_sound_len";
  if (!waves || !sound_ratio) AST_FAIL("%s: null pointer", me);
  if (rows_check(me, B, n, RMS_FRAME, AST_PAD_CONSTANT)) return -1;
  if (win < 1) AST_FAIL("%s: bad window of %d samples", me, win);
  const int W_max = n / win;
  if (W_max > 0 && !mask) AST_FAIL("%s: null pointer", me);
  hipStream_t s = (hipStream_t)stream;
  if (W_max > 0)
    hipLaunchKernelGGL(window_sound_kernel, dim3((W_max + 3) / 4, B), dim3(256), 0, s, waves, n, n_samples, win, threshold_db, W_max, mask);
  hipLaunchKernelGGL(window_ratio_kernel, dim3(B), dim3(256), 0, s, (const int32_t*)mask, n, n_samples, win, W_max, sound_ratio);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" long ast_mfcc_mean_ws_floats(int B, int n, int hop) {
  if (B < 1 || n < 1 || (hop != 256 && hop != 512)) return 0;
  return mm_ws_floats(B, n, hop);
}

extern "C" int ast_mfcc_mean_len(const float* waves, int B, int n, const int32_t* n_samples, int n_mfcc, int hop, int pad_mode,
                                 const int32_t* mel_table, float* ws, long ws_floats, float* out, void* stream) {
  const char* me = "ast_mfcc_mean_len";
  if (!waves || !out) AST_FAIL("%s: null pointer", me);
  if (mfcc_check(me, n_mfcc, MM_MAX_MFCC, hop, mel_table) || rows_check(me, B, n, WIDE_NFFT, pad_mode)) return -1;
  if (ws_check(me, ws, ws_floats, mm_ws_floats(B, n, hop))) return -1;
  hipStream_t s = (hipStream_t)stream;
  const int T_max = frames_of(n, hop), n_runs = mfcc_runs(n, hop), n_chunks = mm_chunks(n, hop);
  const int lo = min_count(pad_mode, WIDE_NFFT);
  float* run_max = ws + (size_t)B * T_max * MEL_N;
  float* part = ws + mfcc_pass1_floats(B, n, hop);
  mel_db_launch(waves, B, n, n_samples, hop, pad_mode, mel_table, ws, run_max, s);
  hipLaunchKernelGGL(mel_mean_chunks_kernel, dim3(n_chunks, B), dim3(128), 0, s, (const float*)ws, (const float*)run_max, n, n_samples, lo, hop,
                     T_max, n_runs, n_chunks, part);
  hipLaunchKernelGGL(mfcc_mean_finish_kernel, dim3(B), dim3(128), 0, s, (const float*)part, n, n_samples, lo, hop, n_chunks, n_mfcc, out);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" int ast_gain_rows_len(const float* waves, int B, int n, const int32_t* n_samples, const double* sumsq, double target_rms, float* out,
                                 void* stream) {
  const char* me = "ast_gain_rows_len";
  if (!waves || !sumsq || !out) AST_FAIL("%s: null pointer", me);
  if (rows_check(me, B, n, RMS_FRAME, AST_PAD_CONSTANT)) return -1;
  if (!(target_rms > 0.0) || !(target_rms <= 3.4028234663852886e38)) AST_FAIL("%s: bad target level %g", me, target_rms);
  hipLaunchKernelGGL(gain_rows_kernel, dim3((n + 1023) / 1024, B), dim3(256), 0, (hipStream_t)stream, waves, n, n_samples, sumsq, target_rms, out);
  AST_CHECK_LAUNCH();
  return 0;
}
