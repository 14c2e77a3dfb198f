// Host-side argument checks of the onset and self-similarity entries (ast_onset_strength_len, ast_onset_detect_len,
// ast_onset_accuracy_len, ast_recurrence_len, ast_self_similarity_distance_len and their workspace counts) as a stand-alone
// program, for a sanitizer run of host code only (no GPU needed: every launch entry below is refused before any launch, the
// device pointers are fake and never dereferenced).  Build and run from the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//     tools/onset_args_main.cpp audio-style-transfer_amd/csrc/{metrics.hip,abi.cpp} -o onset_args && ./onset_args
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../include/ast_hip.h"

static int failures = 0;
static void refused(int rc, const char* what, const char* needle) {
  const char* err = ast_last_error();
  if (rc == 0 || !err || !strstr(err, needle)) {
    printf("NOT REFUSED: %s (rc=%d, error \"%s\", wanted \"%s\")\n", what, rc, err ? err : "", needle);
    ++failures;
  }
}
static void equal(long got, long want, const char* what) {
  if (got != want) { printf("COUNT: %s = %ld, wanted %ld\n", what, got, want); ++failures; }
}
static long run, tile, chunk;
static long frames(long n) { return 1 + n / 512; }
static long pass1(long B, long n) { return B * (frames(n) * 128 + (frames(n) + run - 1) / run); }
static long strength(long B, long n) { return pass1(B, n) + 2 * B * ((frames(n) + tile - 1) / tile); }
static long detect(long B, long n) { return strength(B, n) + B * frames(n); }
static long rec(long B, long n) { return pass1(B, n) + B * 20 * frames(n) + B * ((frames(n) + chunk - 1) / chunk) * 190; }

typedef int (*one_fn)(const float*, int, int, const int32_t*, int, const int32_t*, float*, long, void*, void*);
typedef int (*pair_fn)(const float*, int, const float*, int, int, const int32_t*, const int32_t*, int, const int32_t*, float*, long, float*, void*);

static int strength_len(const float* w, int B, int n, const int32_t* ns, int pad, const int32_t* mel, float* ws, long wsn, void* out, void* s) {
  return ast_onset_strength_len(w, B, n, ns, pad, mel, ws, wsn, (float*)out, s);
}
static int detect_len(const float* w, int B, int n, const int32_t* ns, int pad, const int32_t* mel, float* ws, long wsn, void* out, void* s) {
  return ast_onset_detect_len(w, B, n, ns, pad, mel, ws, wsn, (int32_t*)out, s);
}
static int recurrence_len(const float* w, int B, int n, const int32_t* ns, int pad, const int32_t* mel, float* ws, long wsn, void* out, void* s) {
  return ast_recurrence_len(w, B, n, ns, pad, mel, ws, wsn, (int32_t*)out, nullptr, s);
}

int main() {
  float* f = (float*)(uintptr_t)0x10000;
  int32_t* n = (int32_t*)(uintptr_t)0x20000;
  int32_t* mel = (int32_t*)(uintptr_t)0x30000;
  const int N = 12000, M = 11000, B = 4, BIG = 0x7fffffff;
  run = ast_mfcc_run_frames(), tile = ast_onset_tile_frames(), chunk = ast_recurrence_chunk_frames();
  if (run < 1 || tile < 1 || chunk < 1) { printf("frames per run / tile / chunk: %ld %ld %ld\n", run, tile, chunk); return 1; }

  // workspace arithmetic, at ordinary sizes and at the limits (64-bit all the way)
  const int sizes[][3] = {{B, N, M}, {1, 1, 1}, {65535, BIG, BIG}, {65535, BIG, 1}};
  for (const auto& z : sizes) {
    equal(ast_onset_strength_ws_floats(z[0], z[1]), strength(z[0], z[1]), "ast_onset_strength_ws_floats");
    equal(ast_onset_detect_ws_floats(z[0], z[1]), detect(z[0], z[1]), "ast_onset_detect_ws_floats");
    equal(ast_onset_accuracy_ws_floats(z[0], z[1], z[2]), z[0] + detect(z[0], z[1]) + detect(z[0], z[2]) + (long)z[0] * (frames(z[1]) + frames(z[2])),
          "ast_onset_accuracy_ws_floats");
    equal(ast_recurrence_ws_floats(z[0], z[1]), rec(z[0], z[1]), "ast_recurrence_ws_floats");
    equal(ast_self_similarity_distance_ws_floats(z[0], z[1], z[2]), rec(z[0], z[1]) + rec(z[0], z[2]) + 2L * z[0] * 400,
          "ast_self_similarity_distance_ws_floats");
  }
  equal(ast_onset_strength_ws_floats(0, N), 0, "strength workspace, B = 0");
  equal(ast_onset_detect_ws_floats(B, -1), 0, "detect workspace, n < 0");
  equal(ast_onset_accuracy_ws_floats(B, N, 0), 0, "accuracy workspace, n_gen = 0");
  equal(ast_recurrence_ws_floats(-BIG - 1, N), 0, "recurrence workspace, B = INT_MIN");
  equal(ast_self_similarity_distance_ws_floats(B, -BIG - 1, N), 0, "self-similarity workspace, n_a = INT_MIN");

  const struct { const char* name; one_fn fn; long need; } ones[] = {
      {"strength", strength_len, ast_onset_strength_ws_floats(B, N)},
      {"detect", detect_len, ast_onset_detect_ws_floats(B, N)},
      {"recurrence", recurrence_len, ast_recurrence_ws_floats(B, N)}};
  for (const auto& e : ones) {
    const long ws = e.need;
    refused(e.fn(nullptr, B, N, n, 0, mel, f, ws, f, nullptr), e.name, "null");
    refused(e.fn(f, B, N, n, 0, mel, f, ws, nullptr, nullptr), e.name, "null");
    refused(e.fn(f, B, N, n, 0, nullptr, f, ws, f, nullptr), e.name, "mel table");
    refused(e.fn(f, 0, N, n, 0, mel, f, ws, f, nullptr), e.name, "bad shape");
    refused(e.fn(f, 65536, N, n, 0, mel, f, 1L << 50, f, nullptr), e.name, "bad shape");
    refused(e.fn(f, -BIG - 1, N, n, 0, mel, f, ws, f, nullptr), e.name, "bad shape");
    refused(e.fn(f, B, 0, n, 0, mel, f, ws, f, nullptr), e.name, "bad shape");
    refused(e.fn(f, B, -BIG - 1, n, 0, mel, f, ws, f, nullptr), e.name, "bad shape");
    refused(e.fn(f, B, BIG, n, 0, mel, f, 1L << 50, f, nullptr), e.name, "too long");
    refused(e.fn(f, B, BIG - 4095, n, 0, mel, f, 1L << 50, f, nullptr), e.name, "too long");
    refused(e.fn(f, B, N, n, 2, mel, f, ws, f, nullptr), e.name, "pad_mode");
    refused(e.fn(f, B, N, n, -1, mel, f, ws, f, nullptr), e.name, "pad_mode");
    refused(e.fn(f, B, 1024, n, AST_PAD_REFLECT, mel, f, ws, f, nullptr), e.name, "reflect");
    refused(e.fn(f, B, N, n, 0, mel, nullptr, ws, f, nullptr), e.name, "workspace");
    refused(e.fn(f, B, N, n, 0, mel, f, ws - 1, f, nullptr), e.name, "workspace");
    refused(e.fn(f, B, N, n, 0, mel, f, -1, f, nullptr), e.name, "workspace");
    refused(e.fn(f, 65535, BIG - 4096, n, 0, mel, f, 1L << 40, f, nullptr), e.name, "workspace");     // at the limits: 2^40 floats are too few
  }
  const struct { const char* name; pair_fn fn; long need; } pairs[] = {
      {"accuracy", ast_onset_accuracy_len, ast_onset_accuracy_ws_floats(B, N, M)},
      {"self-similarity", ast_self_similarity_distance_len, ast_self_similarity_distance_ws_floats(B, N, M)}};
  for (const auto& e : pairs) {
    const long ws = e.need;
    refused(e.fn(nullptr, N, f, M, B, n, n, 0, mel, f, ws, f, nullptr), e.name, "null");
    refused(e.fn(f, N, nullptr, M, B, n, n, 0, mel, f, ws, f, nullptr), e.name, "null");
    refused(e.fn(f, N, f, M, B, n, n, 0, mel, f, ws, nullptr, nullptr), e.name, "null");
    refused(e.fn(f, N, f, M, B, n, n, 0, nullptr, f, ws, f, nullptr), e.name, "mel table");
    refused(e.fn(f, N, f, M, 0, n, n, 0, mel, f, ws, f, nullptr), e.name, "bad shape");
    refused(e.fn(f, N, f, M, 65536, n, n, 0, mel, f, 1L << 50, f, nullptr), e.name, "bad shape");
    refused(e.fn(f, 0, f, M, B, n, n, 0, mel, f, ws, f, nullptr), e.name, "bad shape");
    refused(e.fn(f, N, f, -BIG - 1, B, n, n, 0, mel, f, ws, f, nullptr), e.name, "bad shape");
    refused(e.fn(f, BIG, f, M, B, n, n, 0, mel, f, 1L << 50, f, nullptr), e.name, "too long");
    refused(e.fn(f, N, f, BIG - 4095, B, n, n, 0, mel, f, 1L << 50, f, nullptr), e.name, "too long");
    refused(e.fn(f, N, f, M, B, n, n, 3, mel, f, ws, f, nullptr), e.name, "pad_mode");
    refused(e.fn(f, 1024, f, M, B, n, n, AST_PAD_REFLECT, mel, f, ws, f, nullptr), e.name, "reflect");
    refused(e.fn(f, N, f, 1024, B, n, n, AST_PAD_REFLECT, mel, f, ws, f, nullptr), e.name, "reflect");
    refused(e.fn(f, N, f, M, B, n, n, 0, mel, nullptr, ws, f, nullptr), e.name, "workspace");
    refused(e.fn(f, N, f, M, B, n, n, 0, mel, f, ws - 1, f, nullptr), e.name, "workspace");
    refused(e.fn(f, N, f, M, B, n, n, 0, mel, f, -1, f, nullptr), e.name, "workspace");
    refused(e.fn(f, BIG - 4096, f, BIG - 4096, 65535, n, n, 0, mel, f, 1L << 40, f, nullptr), e.name, "workspace");
  }
  printf(failures ? "%d check(s) failed\n" : "onset / self-similarity argument checks: all refused before any launch, workspace counts agree\n", failures);
  return failures ? 1 : 0;
}
