// What the spectrogram metrics (metrics.hip), the chroma / pitch metrics (chroma.hip) and the dataset screening (curation.hip)
// share: the clamped per-clip count, a clip's sample under the pad mode, the fixed-order block sum in double and the host's row checks.  Everything on the device is
// force-inlined, so moving it here changes no kernel's code (tools/kernel_diff.py).
#pragma once
#include <math.h>

#include "ast_common.h"
#include "fft1024.h"
#include "../../include/ast_hip.h"

namespace {
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

// block-wide sum in double in a fixed order: thread-strided partial sums, then thread 0 adds the 256 of them ascending
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  if (threadIdx.x == 0) { double s = 0.0; for (int i = 0; i < 256; ++i) s += red[i]; red[256] = s; }
  __syncthreads();
  return red[256];
}

// host: the row checks every transform shares.  0, or -1 with the message of entry `name` set
inline int rows_check(const char* name, int B, int n, int n_fft, int pad_mode) {
  if (B < 1 || B > 65535) AST_FAIL("%s: bad shape (B=%d, 1 .. 65535)", name, B);
  if (pad_mode != AST_PAD_CONSTANT && pad_mode != AST_PAD_REFLECT) AST_FAIL("%s: bad pad_mode %d (0 constant, 1 reflect)", name, pad_mode);
  if (n < 1) AST_FAIL("%s: bad shape (n=%d)", name, n);
  if (n > 0x7fffffff - 2 * n_fft) AST_FAIL("%s: row too long (n=%d: n + 2 n_fft must stay below 2^31)", name, n);
  if (pad_mode == AST_PAD_REFLECT && n < n_fft / 2 + 1)
    AST_FAIL("%s: reflect padding needs rows of >= %d samples, got %d", name, n_fft / 2 + 1, n);
  return 0;
}
}  // namespace

// ---- the MFCC's first pass (metrics.hip) for the dataset screening (curation.hip): the unclamped mel dB rows db (B, T_max, 128) and
// one maximum per run of frames, T_max = 1 + n / hop.  Host code only, not exported.
AST_HIDDEN long mel_db_pass1_floats(int B, int n, int hop);                    // floats of db + run_max, run_max behind db
AST_HIDDEN int mel_db_pass1_runs(int n, int hop);                             // run maxima per clip
AST_HIDDEN void mel_db_pass1_launch(const float* waves, int B, int n, const int32_t* n_samples, int hop, int pad_mode, const int32_t* mel,
                                    float* db, float* run_max, hipStream_t s);
