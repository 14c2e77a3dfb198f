// Host-side argument checks of ast_attn_fwd / ast_attn_fwd_p / ast_attn_bwd / ast_attn_bwd_p and of the key-masked training
// entries ast_attn_fwd_len_p / ast_attn_bwd_len_p as a stand-alone program, for a
// sanitizer run of host code only (no GPU needed: every call below is refused before any launch, the pointers are fake and
// never dereferenced).  Build and run from the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//     tools/attn_args_main.cpp audio-style-transfer_amd/csrc/{misc.hip,attn.hip,abi.cpp} -o attn_args && ./attn_args
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

int main() {
  float* f = (float*)(uintptr_t)0x10000;
  float* odd = (float*)(uintptr_t)0x10004;
  const int caps[] = {AST_ATTN_MAX_L + 1, 1 << 30, 0x7fffffff};
  for (int L : caps) {
    refused(ast_attn_fwd(f, f, f, f, f, 2, 4, L, 17, 64, 256, 256, 256, 0, nullptr, nullptr), "fwd Lq past the cap", "1024");
    refused(ast_attn_fwd_p(f, f, f, f, f, 2, 4, 17, L, 64, 256, 256, 256, 1, nullptr, 0.3f, 7, nullptr, nullptr), "fwd_p Lk past the cap", "1024");
    refused(ast_attn_bwd(f, f, f, f, f, f, f, f, 2, 4, L, L, 64, 256, 256, 256, nullptr, nullptr), "bwd L past the cap", "1024");
    refused(ast_attn_bwd_p(f, f, f, f, f, f, f, f, 2, 4, 1, L, 64, 256, 256, 256, nullptr, 0.3f, 7, nullptr, nullptr), "bwd_p Lk past the cap", "1024");
  }
  for (int L : {4, 17}) {
    refused(ast_attn_fwd(f, f, f, f, f, 2, 4, L, L, 65, 260, 260, 260, 0, nullptr, nullptr), "fwd dh = 65", "dh");
    refused(ast_attn_bwd(f, f, f, f, f, f, f, f, 2, 4, L, L, 65, 260, 260, 260, nullptr, nullptr), "bwd dh = 65", "dh");
  }
  refused(ast_attn_fwd_p(f, f, f, f, f, 2, 4, 17, 17, 30, 120, 120, 120, 0, nullptr, 0.f, 0, nullptr, nullptr), "fwd_p dh = 30, L = 17", "dh % 4");
  refused(ast_attn_bwd_p(f, f, f, f, f, f, f, f, 2, 4, 17, 17, 30, 120, 120, 120, nullptr, 0.f, 0, nullptr, nullptr), "bwd_p dh = 30, L = 17", "dh % 4");
  refused(ast_attn_fwd(odd, f, f, f, f, 2, 4, 17, 17, 64, 256, 256, 256, 0, nullptr, nullptr), "fwd misaligned q", "16-byte");
  refused(ast_attn_bwd(f, f, f, f, f, f, f, odd, 2, 4, 17, 17, 64, 256, 256, 256, nullptr, nullptr), "bwd misaligned dv", "16-byte");
  refused(ast_attn_fwd(f, f, f, f, f, 2, 4, 17, 17, 64, 258, 256, 256, 0, nullptr, nullptr), "fwd ldq = 258", "multiple of 4");
  refused(ast_attn_fwd(f, f, f, f, f, 2, 4, 17, 17, 64, 128, 256, 256, 0, nullptr, nullptr), "fwd ldq < H*dh", "row strides");
  refused(ast_attn_fwd(f, f, f, f, f, 1 << 20, 1 << 12, 17, 17, 64, 256, 256, 256, 0, nullptr, nullptr), "fwd B*H overflow", "B*H");
  refused(ast_attn_fwd(f, f, f, f, f, 2, 4, 0, 17, 64, 256, 256, 256, 0, nullptr, nullptr), "fwd Lq = 0", "ast_attn_fwd");
  refused(ast_attn_bwd(f, f, f, f, f, f, f, f, 2, 4, 17, -1, 64, 256, 256, 256, nullptr, nullptr), "bwd Lk = -1", "ast_attn_bwd");
  refused(ast_attn_fwd(nullptr, f, f, f, f, 2, 4, 17, 17, 64, 256, 256, 256, 0, nullptr, nullptr), "fwd null q", "bad args");
  refused(ast_attn_bwd_p(f, f, f, f, f, f, f, f, 2, 4, 17, 17, 64, 256, 256, 256, nullptr, 1.f, 0, nullptr, nullptr), "bwd_p p = 1", "bad args");
  // the key-masked training entries: the mask's checks, p, and everything above on both dispatch paths
  const int32_t* n = (const int32_t*)(uintptr_t)0x20000;
  for (int L : {3, 17}) {
    const int Lk = 2 * L;
    refused(ast_attn_fwd_len_p(f, f, f, f, f, 2, 4, L, Lk, 64, 256, 256, 256, 0, nullptr, L, nullptr, 0.1f, 7, nullptr, nullptr), "fwd_len_p null key_len", "key_len");
    refused(ast_attn_bwd_len_p(f, f, f, f, f, f, f, f, 2, 4, L, Lk, 64, 256, 256, 256, nullptr, L, nullptr, 0.1f, 7, nullptr, nullptr), "bwd_len_p null key_len", "key_len");
    for (int period : {0, -3, Lk + 1, L + 1}) {
      refused(ast_attn_fwd_len_p(f, f, f, f, f, 2, 4, L, Lk, 64, 256, 256, 256, 0, n, period, nullptr, 0.1f, 7, nullptr, nullptr), "fwd_len_p key_period", "key_period");
      refused(ast_attn_bwd_len_p(f, f, f, f, f, f, f, f, 2, 4, L, Lk, 64, 256, 256, 256, n, period, nullptr, 0.1f, 7, nullptr, nullptr), "bwd_len_p key_period", "key_period");
    }
    for (float p : {1.f, -0.5f, 2.f}) {
      refused(ast_attn_fwd_len_p(f, f, f, f, f, 2, 4, L, Lk, 64, 256, 256, 256, 0, n, L, nullptr, p, 7, nullptr, nullptr), "fwd_len_p p", "p <");
      refused(ast_attn_bwd_len_p(f, f, f, f, f, f, f, f, 2, 4, L, Lk, 64, 256, 256, 256, n, L, f, p, 7, nullptr, nullptr), "bwd_len_p p", "p <");
    }
    refused(ast_attn_fwd_len_p(f, f, f, nullptr, f, 2, 4, L, Lk, 64, 256, 256, 256, 0, n, L, nullptr, 0.f, 0, nullptr, nullptr), "fwd_len_p null o", "bad args");
    refused(ast_attn_bwd_len_p(f, f, f, f, f, f, nullptr, f, 2, 4, L, Lk, 64, 256, 256, 256, n, L, nullptr, 0.f, 0, nullptr, nullptr), "bwd_len_p null dk", "bad args");
    refused(ast_attn_fwd_len_p(f, f, f, f, f, 2, 4, L, Lk, 65, 260, 260, 260, 0, n, L, nullptr, 0.f, 0, nullptr, nullptr), "fwd_len_p dh = 65", "dh");
    refused(ast_attn_bwd_len_p(f, f, f, f, f, f, f, f, 2, 4, 0, Lk, 64, 256, 256, 256, n, L, nullptr, 0.f, 0, nullptr, nullptr), "bwd_len_p Lq = 0", "1<=L");
  }
  for (int L : caps) {
    refused(ast_attn_fwd_len_p(f, f, f, f, f, 2, 4, 1, L, 64, 256, 256, 256, 0, n, L, nullptr, 0.f, 0, nullptr, nullptr), "fwd_len_p Lk past the cap", "1024");
    refused(ast_attn_bwd_len_p(f, f, f, f, f, f, f, f, 2, 4, L, L, 64, 256, 256, 256, n, L, nullptr, 0.f, 0, nullptr, nullptr), "bwd_len_p L past the cap", "1024");
  }
  refused(ast_attn_fwd_len_p(f, f, f, f, f, 2, 4, 17, 34, 30, 120, 120, 120, 0, n, 17, nullptr, 0.f, 0, nullptr, nullptr), "fwd_len_p dh = 30, L = 17", "dh % 4");
  refused(ast_attn_bwd_len_p(f, f, f, f, f, f, f, f, 2, 4, 17, 34, 30, 120, 120, 120, n, 17, nullptr, 0.f, 0, nullptr, nullptr), "bwd_len_p dh = 30, L = 17", "dh % 4");
  refused(ast_attn_fwd_len_p(f, odd, f, f, f, 2, 4, 17, 34, 64, 256, 256, 256, 0, n, 17, nullptr, 0.f, 0, nullptr, nullptr), "fwd_len_p misaligned k", "16-byte");
  refused(ast_attn_bwd_len_p(f, f, f, f, f, odd, f, f, 2, 4, 17, 34, 64, 256, 256, 256, n, 17, nullptr, 0.f, 0, nullptr, nullptr), "bwd_len_p misaligned dq", "16-byte");
  refused(ast_attn_fwd_len_p(f, f, f, f, f, 2, 4, 17, 34, 64, 256, 258, 256, 0, n, 17, nullptr, 0.f, 0, nullptr, nullptr), "fwd_len_p ldk = 258", "multiple of 4");
  refused(ast_attn_bwd_len_p(f, f, f, f, f, f, f, f, 2, 4, 17, 34, 64, 256, 256, 128, n, 17, nullptr, 0.f, 0, nullptr, nullptr), "bwd_len_p ldo < H*dh", "row strides");
  refused(ast_attn_fwd_len_p(f, f, f, f, f, 1 << 20, 1 << 12, 17, 34, 64, 256, 256, 256, 0, n, 17, nullptr, 0.f, 0, nullptr, nullptr), "fwd_len_p B*H overflow", "B*H");
  refused(ast_attn_bwd_len_p(f, f, f, f, f, f, f, f, 0, 4, 3, 6, 64, 256, 256, 256, n, 3, nullptr, 0.f, 0, nullptr, nullptr), "bwd_len_p B = 0", "B >= 1");
  printf(failures ? "%d check(s) failed\n" : "attention argument checks: all refused before any launch\n", failures);
  return failures ? 1 : 0;
}
