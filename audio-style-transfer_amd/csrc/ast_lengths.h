// Length arithmetic of the waveform front end for a padded batch (ast_frontend_lengths, ast_stft_sections_len, ast_decimate2_len,
// ast_cqt_octaves_len, ast_cqt_sections_len): the one place that says how many frames and sections a clip of `ns` samples has.
// Host and device compile the same function, so the kernels, the host twin ast_frontend_lengths_host and the Python side agree.
#pragma once
#include "ast_common.h"

#define AST_FE_HOP 256            // the front end's hop (get_STFT / get_CQT, utilityFunctions.py:12-60)
#define AST_FE_MAX_WIN (1 << 20)  // the host refuses longer windows, so that 256 * (win / 2) stays an int

struct AstClipLen {
  int ns;                         // the clip's sample count, clamped to [ast_ns_min(win), nsamp]
  int T;                          // frames: 1 + ns / 256 (torch.stft center=True; librosa trims the CQT to the same count)
  int n_sec;                      // len(section_starts(T)) (utilityFunctions.py:246-262)
  int n_frames;                   // min(T, step * (n_sec - 1) + win): the frames its kept sections cover
};

// the smallest sample count that reflect-pads validly (> 512) and yields one section (T >= win / 2): 36 608 at win = 287
__host__ __device__ inline int ast_ns_min(int win) {
  const int a = AST_FE_HOP * ((win + 1) / 2 - 1);
  return a > 513 ? a : 513;
}

// get_overlap_windows keeps the full windows at 0, step, ... and the last, partly filled one iff it holds at least half a
// window: with k = ceil(max(T - win, 0) / step) full ones, the window at k * step holds T - k * step frames.
__host__ __device__ inline AstClipLen ast_clip_len(int ns_raw, int nsamp, int win, int step) {
  AstClipLen L;
  const int lo = ast_ns_min(win);
  L.ns = ns_raw < lo ? lo : ns_raw;
  if (L.ns > nsamp) L.ns = nsamp;
  L.T = 1 + L.ns / AST_FE_HOP;
  const int over = L.T > win ? L.T - win : 0;
  const int k = (over + step - 1) / step;
  L.n_sec = k + (2 * (L.T - k * step) >= win ? 1 : 0);
  const int covered = step * (L.n_sec - 1) + win;
  L.n_frames = L.T < covered ? L.T : covered;
  return L;
}

// ---- sections of a padded batch of B clips x S sections (the image and token kernels that take n_sections): clip b holds
// n_b = clamp(n_sections[b], 1, S) real sections, clamped where it is read and never on the host; section s of clip b is live iff s < n_b
__host__ __device__ inline int ast_live_sections(int n_raw, int S) { return n_raw < 1 ? 1 : (n_raw > S ? S : n_raw); }
// the most images (B * S) an entry that takes n_sections accepts: counts stay exact in f32 and image indices stay ints
#define AST_LEN_MAX_IMAGES (1 << 24)

// samples of the clip after o ceil-halvings (librosa's audio.resample(2 -> 1) between octaves): ceil(ns / 2^o)
__host__ __device__ inline int ast_halved(int ns, int o) { return (int)(((long long)ns + (1ll << o) - 1) >> o); }

// ---- host: what every entry that takes per-clip lengths checks before ast_clip_len may run on its arguments
inline bool ast_sectioning_ok(int win, int step) { return win >= 1 && win <= AST_FE_MAX_WIN && step >= 1 && step <= win; }
// the padded row must hold one section: 0, or -1 with the message of entry `name` set
inline int ast_row_check(const char* name, int nsamp, int win) {
  if (nsamp < ast_ns_min(win)) AST_FAIL("%s: nsamp %d needs >= %d samples (one section at win %d)", name, nsamp, ast_ns_min(win), win);
  return 0;
}
