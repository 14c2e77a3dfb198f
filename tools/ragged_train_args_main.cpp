// Host-side argument checks of the ragged-training entries -- ast_recon_loss_len_grad and its workspace query, ast_bign_dgrad_len,
// ast_bign_dgrad_len_det and its workspace query, ast_linear_wgrad_len -- as a stand-alone program, for a sanitizer run of host code
// only (no GPU needed: every call below is refused before any launch, the pointers are fake and never dereferenced).  Build and
// run from the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//     tools/ragged_train_args_main.cpp audio-style-transfer_amd/csrc/{misc.hip,attn.hip,losses.hip,skinny.hip,abi.cpp} -o ragged_train_args \
//     && ./ragged_train_args
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../include/ast_hip.h"

static int failures = 0;
static void refused(long rc, const char* what, const char* entry, const char* needle) {
  const char* err = ast_last_error();
  if (rc == 0 || !err || !strstr(err, entry) || !strstr(err, needle)) {
    printf("NOT REFUSED: %s (rc=%ld, error \"%s\", wanted \"%s\" from %s)\n", what, rc, err ? err : "", needle, entry);
    ++failures;
  }
}
static void expect(long got, long want, const char* what) {
  if (got != want) { printf("WRONG: %s = %ld, expected %ld\n", what, got, want); ++failures; }
}

int main() {
  float* f = (float*)(uintptr_t)0x10000;
  float* odd = (float*)(uintptr_t)0x10002;
  const int32_t* n = (const int32_t*)(uintptr_t)0x20000;
  const int32_t* nodd = (const int32_t*)(uintptr_t)0x20001;
  const float c5[5] = {2.f, 0.5f, 0.2f, 0.3f, 0.1f};

  // ---- ast_recon_loss_len_grad ----------------------------------------------------------------------------------------------
  const char* LG = "ast_recon_loss_len_grad";
  expect(ast_recon_loss_len_grad_ws_floats(3, 3, 5, 7), 5 * 3 * 1, "ws_floats small");
  expect(ast_recon_loss_len_grad_ws_floats(2, 2, 287, 513), 5 * 2 * 576, "ws_floats real size");
  expect(ast_recon_loss_len_grad_ws_floats(1, 2, 3, 400000), 5 * 4096, "ws_floats capped");
  const int bad_sizes[][4] = {{0, 2, 287, 513}, {2, 0, 287, 513}, {2, 2, 0, 513}, {2, 2, 287, 0}, {-1, 2, 287, 513}, {65536, 1, 1, 1},
                              {16, 1, 287 * 513, 1024}, {0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff}};
  for (const auto& a : bad_sizes)
    refused(ast_recon_loss_len_grad_ws_floats(a[0], a[1], a[2], a[3]) < 0 ? -1 : 0, "ws_floats bad sizes", "ast_recon_loss_len_grad_ws_floats", "bad sizes");
  const long need = 5 * 2 * 576;
  refused(ast_recon_loss_len_grad(nullptr, f, 597, 2, 2, 287, 513, n, f, c5, f, need, f, f, f, nullptr), "null out", LG, "null");
  refused(ast_recon_loss_len_grad(f, nullptr, 597, 2, 2, 287, 513, n, f, c5, f, need, f, f, f, nullptr), "null tgt", LG, "null");
  refused(ast_recon_loss_len_grad(f, f, 597, 2, 2, 287, 513, n, f, nullptr, f, need, f, f, f, nullptr), "null coef5", LG, "null");
  refused(ast_recon_loss_len_grad(f, f, 597, 2, 2, 287, 513, n, f, c5, nullptr, need, f, f, f, nullptr), "null ws", LG, "null");
  refused(ast_recon_loss_len_grad(f, f, 597, 2, 2, 287, 513, n, f, c5, f, need, nullptr, f, f, nullptr), "null res", LG, "null");
  refused(ast_recon_loss_len_grad(f, f, 597, 2, 2, 287, 513, n, f, c5, f, need, f, nullptr, f, nullptr), "null loss", LG, "null");
  refused(ast_recon_loss_len_grad(f, f, 597, 2, 2, 287, 513, n, f, c5, f, need, f, f, nullptr, nullptr), "null grad", LG, "null");
  for (int z : {0, -2, (int)0x80000000}) {
    refused(ast_recon_loss_len_grad(f, f, 597, z, 2, 287, 513, n, f, c5, f, need, f, f, f, nullptr), "B < 1", LG, ">= 1");
    refused(ast_recon_loss_len_grad(f, f, 597, 2, z, 287, 513, n, f, c5, f, need, f, f, f, nullptr), "S < 1", LG, ">= 1");
    refused(ast_recon_loss_len_grad(f, f, 597, 2, 2, z, 513, n, f, c5, f, need, f, f, f, nullptr), "T < 1", LG, ">= 1");
    refused(ast_recon_loss_len_grad(f, f, 597, 2, 2, 287, z, n, f, c5, f, need, f, f, f, nullptr), "Fq < 1", LG, ">= 1");
  }
  refused(ast_recon_loss_len_grad(f, f, 512, 2, 2, 287, 513, n, f, c5, f, need, f, f, f, nullptr), "tgt_ld < Fq", LG, "tgt_ld");
  refused(ast_recon_loss_len_grad(f, f, -1, 2, 2, 287, 513, n, f, c5, f, need, f, f, f, nullptr), "tgt_ld < 0", LG, "tgt_ld");
  refused(ast_recon_loss_len_grad(f, f, 1024, 16, 1, 287 * 513, 1024, n, f, c5, f, need, f, f, f, nullptr), "2^31 bins", LG, "2^31");
  refused(ast_recon_loss_len_grad(f, f, 0x7fffffff, 0x7fffffff, 1, 0x7fffffff, 0x7fffffff, n, f, c5, f, need, f, f, f, nullptr), "overflowing sizes", LG, "2^31");
  refused(ast_recon_loss_len_grad(f, f, 1, 65536, 1, 1, 1, n, f, c5, f, need, f, f, f, nullptr), "B > 65535", LG, "65535");
  refused(ast_recon_loss_len_grad(f, f, 597, 2, 2, 287, 513, n, f, c5, f, need - 1, f, f, f, nullptr), "short ws", LG, "ws needs");
  refused(ast_recon_loss_len_grad(f, f, 597, 2, 2, 287, 513, nullptr, nullptr, c5, f, -5, f, f, f, nullptr), "negative ws", LG, "ws needs");

  // ---- ast_bign_dgrad_len[_det] -----------------------------------------------------------------------------------------------
  const int N = 294462, K = 256;
  expect(ast_bign_dgrad_len_det_ws_floats(9, 2050, 256), 5L * 9 * 256, "dgrad ws small");
  expect(ast_bign_dgrad_len_det_ws_floats(1024, N, K), 576L * 1024 * 256, "dgrad ws largest");
  const int bad_mnk[][3] = {{0, N, K}, {-3, N, K}, {1025, N, K}, {9, 0, K}, {9, N, 0}, {9, N, 257}, {9, 0x7fffffff, 4}, {0x7fffffff, 0x7fffffff, 256}};
  for (const auto& a : bad_mnk) expect(ast_bign_dgrad_len_det_ws_floats(a[0], a[1], a[2]), -1, "dgrad ws refused sizes");
  const long dneed = 576L * 12 * 256;
  for (int det = 0; det < 2; ++det) {
    const char* E = det ? "ast_bign_dgrad_len_det" : "ast_bign_dgrad_len";
    auto call = [&](const float* dy, const float* w, float* dx, int M, int Nn, int Kk, int lddy, int S, const int32_t* nv) {
      return det ? ast_bign_dgrad_len_det(dy, w, dx, M, Nn, Kk, lddy, S, nv, f, dneed, nullptr) : ast_bign_dgrad_len(dy, w, dx, M, Nn, Kk, lddy, S, nv, nullptr);
    };
    refused(call(nullptr, f, f, 12, N, K, N, 3, n), "null dy", E, "null");
    refused(call(f, nullptr, f, 12, N, K, N, 3, n), "null w", E, "null");
    refused(call(f, f, nullptr, 12, N, K, N, 3, n), "null dx", E, "null");
    for (int M : {0, -12, 1025, 0x7fffffff}) refused(call(f, f, f, M, N, K, N, 1, n), "M out of range", E, "1..1024");
    for (int S : {0, -3, 5, 13, 0x7fffffff}) refused(call(f, f, f, 12, N, K, N, S, n), "S does not divide M", E, "M % S");
    refused(call(f, f, f, 12, 0, K, 0, 3, n), "N = 0", E, "bad args");
    for (int Kk : {0, -1, 257, 0x7fffffff}) refused(call(f, f, f, 12, N, Kk, N, 3, n), "K out of range", E, "K <= 256");
    refused(call(f, f, f, 12, N, K, N - 1, 3, n), "lddy < N", E, "lddy");
    refused(call(odd, f, f, 12, N, K, N, 3, n), "misaligned dy", E, "4-byte");
    refused(call(f, f, odd, 12, N, K, N, 3, n), "misaligned dx", E, "4-byte");
    refused(call(f, f, f, 12, N, K, N, 3, nodd), "misaligned n_valid", E, "4-byte");
  }
  refused(ast_bign_dgrad_len_det(f, f, f, 12, N, K, N, 3, n, nullptr, dneed, nullptr), "det null ws", "ast_bign_dgrad_len_det", "null");
  refused(ast_bign_dgrad_len_det(f, f, f, 12, N, K, N, 3, n, f, dneed - 1, nullptr), "det short ws", "ast_bign_dgrad_len_det", "ws needs");
  refused(ast_bign_dgrad_len_det(f, f, f, 12, N, K, N, 3, nullptr, f, -1, nullptr), "det negative ws", "ast_bign_dgrad_len_det", "ws needs");
  refused(ast_bign_dgrad_len_det(f, f, f, 4, 512 * 65536 + 1, 4, 512 * 65536 + 1, 2, n, f, 1L << 40, nullptr), "det too many slabs", "ast_bign_dgrad_len_det", "ws needs");

  // ---- ast_linear_wgrad_len ---------------------------------------------------------------------------------------------------
  const char* WG = "ast_linear_wgrad_len";
  refused(ast_linear_wgrad_len(nullptr, f, f, f, 12, N, K, N, K, 3, n, nullptr), "null dy", WG, "null");
  refused(ast_linear_wgrad_len(f, nullptr, f, f, 12, N, K, N, K, 3, n, nullptr), "null x", WG, "null");
  refused(ast_linear_wgrad_len(f, f, nullptr, f, 12, N, K, N, K, 3, n, nullptr), "null dW", WG, "null");
  for (int M : {0, -12, 1025, 0x7fffffff}) refused(ast_linear_wgrad_len(f, f, f, f, M, N, K, N, K, 1, n, nullptr), "M out of range", WG, "1..1024");
  for (int S : {0, -3, 5, 13, 0x7fffffff}) refused(ast_linear_wgrad_len(f, f, f, f, 12, N, K, N, K, S, n, nullptr), "S does not divide M", WG, "M % S");
  refused(ast_linear_wgrad_len(f, f, f, f, 12, 0, K, 0, K, 3, n, nullptr), "N = 0", WG, "bad args");
  refused(ast_linear_wgrad_len(f, f, f, f, 12, N, 0, N, 0, 3, n, nullptr), "K = 0", WG, "bad args");
  refused(ast_linear_wgrad_len(f, f, f, f, 12, N, K, N - 1, K, 3, n, nullptr), "lddy < N", WG, "lddy");
  refused(ast_linear_wgrad_len(f, f, f, f, 12, N, K, N, K - 1, 3, n, nullptr), "ldw < K", WG, "ldw");
  refused(ast_linear_wgrad_len(f, f, f, f, 12, 64 * 65535 + 1, K, 64 * 65535 + 1, K, 3, n, nullptr), "N past the grid", WG, "too large");
  refused(ast_linear_wgrad_len(f, f, f, f, 12, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff, 3, n, nullptr), "largest sizes", WG, "too large");
  refused(ast_linear_wgrad_len(f, odd, f, f, 12, N, K, N, K, 3, n, nullptr), "misaligned x", WG, "4-byte");
  refused(ast_linear_wgrad_len(f, f, f, odd, 12, N, K, N, K, 3, n, nullptr), "misaligned db", WG, "4-byte");
  refused(ast_linear_wgrad_len(f, f, f, nullptr, 12, N, K, N, K, 3, nodd, nullptr), "misaligned n_valid", WG, "4-byte");
  printf(failures ? "%d check(s) failed\n" : "ragged training argument checks: all refused before any launch\n", failures);
  return failures ? 1 : 0;
}
