// Host-side argument checks of the ragged-waveform entries (ast_frontend_lengths, ast_stft_sections_len, ast_decimate2_len,
// ast_cqt_octaves_len, ast_cqt_sections_len) and the host twin of the length function as a stand-alone program, for a
// sanitizer run of host code only (no GPU needed: every call below is refused before any launch, the pointers are fake and
// never dereferenced).  Build and run from the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//     tools/frontend_len_args_main.cpp audio-style-transfer_amd/csrc/{fft.hip,cqt.hip,abi.cpp} -o frontend_len_args && ./frontend_len_args
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

// utilityFunctions.section_starts(T): the count of kept sections
static int n_sections(int T, int win, int step) {
  int n = 0;
  for (int s = 0; s < T; s += step) {
    const int e = s + win < T ? s + win : T;
    if (2 * (e - s) < win) break;
    ++n;
    if (e == T) break;
  }
  return n;
}

int main() {
  float* f = (float*)(uintptr_t)0x10000;
  int32_t* n = (int32_t*)(uintptr_t)0x20000;
  const int NS = 85760, MIN = 36608, W = 287, ST = 191;
  int out[4];
  for (int T = 144; T <= 1200; ++T)
    for (int ns : {256 * (T - 1), 256 * (T - 1) + 255}) {
      const int k = n_sections(T, W, ST), cov = ST * (k - 1) + W;
      if (ast_frontend_lengths_host(ns, 256 * 1200, W, ST, out) != 0 || out[0] != ns || out[1] != T || out[2] != k || out[3] != (T < cov ? T : cov)) {
        printf("LENGTHS: ns=%d -> %d %d %d %d, wanted T=%d n_sec=%d\n", ns, out[0], out[1], out[2], out[3], T, k);
        ++failures;
      }
    }
  for (int ns : {-0x7fffffff - 1, -1, 0, MIN - 1, NS + 1, 0x7fffffff})
    if (ast_frontend_lengths_host(ns, NS, W, ST, out) != 0 || out[0] != (ns < MIN ? MIN : NS)) { printf("CLAMP: ns=%d -> %d\n", ns, out[0]); ++failures; }
  refused(ast_frontend_lengths_host(NS, MIN - 1, W, ST, out), "host twin, short row", "needs");
  refused(ast_frontend_lengths_host(NS, NS, W, ST, nullptr), "host twin, null out", "bad args");

  refused(ast_frontend_lengths(nullptr, 3, NS, W, ST, n, n, nullptr), "lengths null n_samples", "n_samples");
  refused(ast_frontend_lengths(n, 3, NS, W, ST, nullptr, n, nullptr), "lengths null out", "null");
  refused(ast_frontend_lengths(n, 0, NS, W, ST, n, n, nullptr), "lengths Bc = 0", "bad shape");
  refused(ast_frontend_lengths(n, 3, MIN - 1, W, ST, n, n, nullptr), "lengths short row", "needs");
  refused(ast_frontend_lengths(n, 3, NS, 0x7fffffff, ST, n, n, nullptr), "lengths win = INT_MAX", "bad shape");

  refused(ast_stft_sections_len(f, 3, NS, f, f, f, 2, W, ST, 597, nullptr, nullptr), "stft null n_samples", "n_samples");
  refused(ast_stft_sections_len(nullptr, 3, NS, f, f, f, 2, W, ST, 597, n, nullptr), "stft null wave", "bad args");
  refused(ast_stft_sections_len(f, 3, NS, f, f, f, 2, W, ST, 512, n, nullptr), "stft F_total = 512", "bad args");
  refused(ast_stft_sections_len(f, 3, NS, f, f, f, 1 << 20, W, ST, 597, n, nullptr), "stft S past the grid", "bad args");
  refused(ast_stft_sections_len(f, 3, MIN - 1, f, f, f, 2, W, ST, 597, n, nullptr), "stft short row", "needs");

  refused(ast_decimate2_len(f, 3, NS, f, 359, 179, f, NS / 2, 1.f, nullptr, NS, W, ST, 0, nullptr), "decimate null n_samples", "n_samples");
  refused(ast_decimate2_len(f, 3, NS, nullptr, 359, 179, f, NS / 2, 1.f, n, NS, W, ST, 0, nullptr), "decimate null taps", "null");
  refused(ast_decimate2_len(f, 3, NS, f, 4097, 179, f, NS / 2, 1.f, n, NS, W, ST, 0, nullptr), "decimate klen", "bad shape");
  refused(ast_decimate2_len(f, 3, NS, f, 359, 179, f, NS / 2, 1.f, n, NS, W, ST, 31, nullptr), "decimate o = 31", "bad shape");
  refused(ast_decimate2_len(f, 3, NS, f, 359, 179, f, NS / 2, 1.f, n, NS, W, ST, 1, nullptr), "decimate wrong level", "halved");
  refused(ast_decimate2_len(f, 3, 0x7fffffff, f, 359, 179, f, 0x7fffffff, 1.f, n, 0x7fffffff, W, ST, 0, nullptr), "decimate too long", "too long");
  refused(ast_decimate2_len(f, 3, MIN - 1, f, 359, 179, f, MIN / 2, 1.f, n, MIN - 1, W, ST, 0, nullptr), "decimate short row", "needs");

  const float* ys[7] = {f, f, f, f, f, f, f};
  int ns[7], hops[7], los[7], nfs[7], row0s[7];
  for (int o = 0; o < 7; ++o) { ns[o] = (NS + (1 << o) - 1) >> o; hops[o] = 256 >> o; los[o] = 72 - 12 * o; nfs[o] = 12; row0s[o] = 0; }
  refused(ast_cqt_octaves_len(ys, ns, hops, los, nfs, row0s, 7, 3, f, f, f, 256, f, 336, 597, 513, nullptr, NS, W, ST, nullptr), "octaves null n_samples", "n_samples");
  refused(ast_cqt_octaves_len(ys, ns, hops, los, nfs, row0s, 13, 3, f, f, f, 256, f, 336, 597, 513, n, NS, W, ST, nullptr), "octaves n_oct = 13", "bad shape");
  refused(ast_cqt_octaves_len(ys, ns, hops, los, nfs, row0s, 7, 3, f, f, f, 256, f, 336, 596, 513, n, NS, W, ST, nullptr), "octaves ld = 596", "bad octave");
  refused(ast_cqt_octaves_len(ys, ns, hops, los, nfs, row0s, 7, 3, f, f, f, 256, f, 336, 597, 513, n, NS + 2, W, ST, nullptr), "octaves wrong widths", "halved");
  refused(ast_cqt_octaves_len(ys, ns, hops, los, nfs, row0s, 7, 3, f, f, f, 256, f, 336, 597, 513, n, NS, W, 0, nullptr), "octaves step = 0", "sectioning");
  hops[0] = 1 << 20;
  refused(ast_cqt_octaves_len(ys, ns, hops, los, nfs, row0s, 7, 3, f, f, f, 256, f, 336, 597, 513, n, NS, W, ST, nullptr), "octaves hop past the LDS span", "LDS");

  refused(ast_cqt_sections_len(f, 3, 336, 84, f, f, f, 2, W, ST, 597, 513, nullptr, NS, nullptr), "sections null n_samples", "n_samples");
  refused(ast_cqt_sections_len(f, 3, 336, 84, f, f, nullptr, 2, W, ST, 597, 513, n, NS, nullptr), "sections null x", "null");
  refused(ast_cqt_sections_len(f, 3, 336, 84, f, f, f, 2, W, ST, 597, 514, n, NS, nullptr), "sections bin0 = 514", "bad shape");
  refused(ast_cqt_sections_len(f, 3, 335, 84, f, f, f, 2, W, ST, 597, 513, n, NS, nullptr), "sections wrong T", "1 + nsamp");
  refused(ast_cqt_sections_len(f, 3, 143, 84, f, f, f, 2, W, ST, 597, 513, n, MIN - 1, nullptr), "sections short row", "needs");
  printf(failures ? "%d check(s) failed\n" : "ragged-waveform argument checks: all refused before any launch, lengths agree\n", failures);
  return failures ? 1 : 0;
}
