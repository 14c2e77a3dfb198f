// Host-side argument checks of the spectrogram-metric entries (ast_spec_mse_len, ast_band_energy_len, ast_pearson_rows and the
// workspace counts) as a stand-alone program, for a sanitizer run of host code only (no GPU needed: every call below is refused
// before any launch, the pointers are fake and never dereferenced).  Build and run from the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//     tools/metrics_args_main.cpp audio-style-transfer_amd/csrc/{metrics.hip,abi.cpp} -o metrics_args && ./metrics_args
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

int main() {
  float* f = (float*)(uintptr_t)0x10000;
  int32_t* n = (int32_t*)(uintptr_t)0x20000;
  const int N = 40000, B = 4, BIG = 0x7fffffff;
  const int run = ast_band_energy_run_frames();
  const long mse_ws = ast_spec_mse_ws_floats(B, N, 39000), be_ws = ast_band_energy_ws_floats(B, N);
  equal(mse_ws, 4L * ((1 + 39000 / 256 + 1) / 2), "ast_spec_mse_ws_floats");
  equal(be_ws, 4L * ((1 + N / 512 + run - 1) / run) * 1025, "ast_band_energy_ws_floats");
  equal(ast_spec_mse_ws_floats(0, N, N), 0, "mse workspace, B = 0");
  equal(ast_spec_mse_ws_floats(B, -1, N), 0, "mse workspace, n < 0");
  equal(ast_band_energy_ws_floats(B, 0), 0, "band workspace, n = 0");
  equal(ast_spec_mse_ws_floats(65535, BIG, BIG), 65535L * ((2 + BIG / 256) / 2), "mse workspace at the limits");
  equal(ast_band_energy_ws_floats(65535, BIG), 65535L * ((1 + BIG / 512 + run - 1) / run) * 1025, "band workspace at the limits");

  refused(ast_spec_mse_len(nullptr, N, f, N, B, n, n, 0, f, mse_ws, f, nullptr), "mse null original", "null");
  refused(ast_spec_mse_len(f, N, nullptr, N, B, n, n, 0, f, mse_ws, f, nullptr), "mse null generated", "null");
  refused(ast_spec_mse_len(f, N, f, N, B, n, n, 0, f, mse_ws, nullptr, nullptr), "mse null out", "null");
  refused(ast_spec_mse_len(f, N, f, N, 0, n, n, 0, f, mse_ws, f, nullptr), "mse B = 0", "bad shape");
  refused(ast_spec_mse_len(f, N, f, N, 65536, n, n, 0, f, 1L << 40, f, nullptr), "mse B past the grid", "bad shape");
  refused(ast_spec_mse_len(f, 0, f, N, B, n, n, 0, f, mse_ws, f, nullptr), "mse n_orig = 0", "bad shape");
  refused(ast_spec_mse_len(f, N, f, -BIG - 1, B, n, n, 0, f, mse_ws, f, nullptr), "mse n_gen = INT_MIN", "bad shape");
  refused(ast_spec_mse_len(f, BIG, f, N, B, n, n, 0, f, 1L << 40, f, nullptr), "mse n_orig = INT_MAX", "too long");
  refused(ast_spec_mse_len(f, N, f, N, B, n, n, 2, f, mse_ws, f, nullptr), "mse pad_mode = 2", "pad_mode");
  refused(ast_spec_mse_len(f, N, f, N, B, n, n, -1, f, mse_ws, f, nullptr), "mse pad_mode = -1", "pad_mode");
  refused(ast_spec_mse_len(f, 512, f, N, B, n, n, AST_PAD_REFLECT, f, mse_ws, f, nullptr), "mse reflect on 512 samples", "reflect");
  refused(ast_spec_mse_len(f, N, f, 512, B, n, n, AST_PAD_REFLECT, f, mse_ws, f, nullptr), "mse reflect on 512 samples (generated)", "reflect");
  refused(ast_spec_mse_len(f, N, f, 39000, B, n, n, 0, nullptr, mse_ws, f, nullptr), "mse null workspace", "workspace");
  refused(ast_spec_mse_len(f, N, f, 39000, B, n, n, 0, f, mse_ws - 1, f, nullptr), "mse short workspace", "workspace");
  refused(ast_spec_mse_len(f, N, f, 39000, B, n, n, 0, f, -1, f, nullptr), "mse negative workspace", "workspace");

  refused(ast_band_energy_len(nullptr, B, N, n, 0, f, be_ws, f, nullptr), "band null waves", "null");
  refused(ast_band_energy_len(f, B, N, n, 0, f, be_ws, nullptr, nullptr), "band null energy", "null");
  refused(ast_band_energy_len(f, 0, N, n, 0, f, be_ws, f, nullptr), "band B = 0", "bad shape");
  refused(ast_band_energy_len(f, 65536, N, n, 0, f, 1L << 40, f, nullptr), "band B past the grid", "bad shape");
  refused(ast_band_energy_len(f, B, 0, n, 0, f, be_ws, f, nullptr), "band n = 0", "bad shape");
  refused(ast_band_energy_len(f, B, BIG - 4095, n, 0, f, 1L << 40, f, nullptr), "band n too long", "too long");
  refused(ast_band_energy_len(f, B, N, n, 3, f, be_ws, f, nullptr), "band pad_mode = 3", "pad_mode");
  refused(ast_band_energy_len(f, B, 1024, n, AST_PAD_REFLECT, f, be_ws, f, nullptr), "band reflect on 1024 samples", "reflect");
  refused(ast_band_energy_len(f, B, N, n, 0, nullptr, be_ws, f, nullptr), "band null workspace", "workspace");
  refused(ast_band_energy_len(f, B, N, n, 0, f, be_ws - 1, f, nullptr), "band short workspace", "workspace");

  refused(ast_pearson_rows(nullptr, f, B, 1025, f, nullptr), "pearson null a", "null");
  refused(ast_pearson_rows(f, nullptr, B, 1025, f, nullptr), "pearson null b", "null");
  refused(ast_pearson_rows(f, f, B, 1025, nullptr, nullptr), "pearson null out", "null");
  refused(ast_pearson_rows(f, f, 0, 1025, f, nullptr), "pearson B = 0", "bad shape");
  refused(ast_pearson_rows(f, f, B, 1, f, nullptr), "pearson n = 1", "bad shape");
  refused(ast_pearson_rows(f, f, BIG, BIG, f, nullptr), "pearson B * n past 2^31", "bad shape");
  printf(failures ? "%d check(s) failed\n" : "spectrogram-metric argument checks: all refused before any launch, workspace counts agree\n", failures);
  return failures ? 1 : 0;
}
