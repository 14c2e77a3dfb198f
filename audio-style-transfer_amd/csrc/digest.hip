// State digest (ast_state_digest): one 64-bit value over the exact bytes of a list of device tensors, in list order.
//
//   digest = mix64( SEED + sum_e mix64((mix64(e) ^ LEN_KEY) + nbytes_e) + sum_i mix64(mix64(i) ^ w_i) )        (all mod 2^64)
//
// w_i is the i-th little-endian 32-bit word of the list: every entry starts a new word, its last word is padded with zero bytes,
// and i runs on over the entries (entry e starts at word sum_{e' < e} ceil(nbytes_e' / 4)).  mix64 is the splitmix64 finaliser the
// dropout masks use (ast_common.h); it is a bijection, so the term of word i is a one-to-one function of w_i: flipping any bit
// changes exactly one term and therefore the sum.  The word index is inside the term, so moving a word changes it too.  The
// terms are combined by wrap-around INTEGER addition, which is associative and commutative: the workgroups add their partial sums
// into *out with one 64-bit atomic each, in whatever order they finish, and the result does not depend on that order, on the grid
// or on how the loop below cuts an entry into vector and scalar loads.  tests/state_digest_ref.py restates the function.
#include "ast_common.h"
#include "../../include/ast_hip.h"

namespace {
constexpr uint64_t DIGEST_SEED = 0x4153545F44494753ull, DIGEST_LEN_KEY = 0xA5A5A5A5A5A5A5A5ull;
__host__ __device__ __forceinline__ uint64_t dmix64(uint64_t z) {                 // == mix64 (ast_common.h), host side as well
  z += 0x9E3779B97F4A7C15ull; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t word_term(uint64_t i, uint32_t w) { return dmix64(dmix64(i) ^ (uint64_t)w); }

__global__ void digest_set_kernel(unsigned long long* out, const unsigned long long v) {
  if (threadIdx.x == 0) out[0] = v;
}
__global__ void digest_final_kernel(unsigned long long* out) {
  if (threadIdx.x == 0) out[0] = dmix64(out[0]);
}
// One entry: p[0, nbytes), whose first word has list index word0.  Every read stays inside [p, p + nbytes).
__global__ __launch_bounds__(256) void digest_entry_kernel(const uint8_t* __restrict__ p, const uint64_t nbytes, const uint64_t word0,
                                                           unsigned long long* __restrict__ out) {
  __shared__ uint64_t red[4];
  const uint64_t nfull = nbytes >> 2;                       // complete words
  const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x, nthreads = (uint64_t)gridDim.x * 256;
  uint64_t acc = 0;
  if (((uintptr_t)p) & 3) {                                 // a view that starts inside a word (16-bit elements): byte loads
    for (uint64_t i = tid; i < nfull; i += nthreads) {
      const uint8_t* b = p + 4 * i;
      acc += word_term(word0 + i, (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24));
    }
  } else {
    const uint32_t* pw = reinterpret_cast<const uint32_t*>(p);
    // up to 3 words to the first 16-byte boundary, 16-byte loads from there, up to 3 words behind them
    const uint64_t lead = ((16 - (((uintptr_t)p) & 15)) & 15) >> 2, head = lead < nfull ? lead : nfull;
    const uint64_t nvec = (nfull - head) >> 2, tail0 = head + 4 * nvec;
    if (tid < head) acc += word_term(word0 + tid, pw[tid]);
    const uint4* pv = reinterpret_cast<const uint4*>(pw + head);
    for (uint64_t i = tid; i < nvec; i += nthreads) {
      const uint4 v = pv[i];
      const uint64_t b = word0 + head + 4 * i;
      acc += (word_term(b, v.x) + word_term(b + 1, v.y)) + (word_term(b + 2, v.z) + word_term(b + 3, v.w));
    }
    if (tid < nfull - tail0) acc += word_term(word0 + tail0 + tid, pw[tail0 + tid]);
  }
  if (tid == 0 && (nbytes & 3)) {                           // the last, incomplete word: its missing bytes count as zero
    uint32_t w = 0;
    for (uint64_t k = 0; k < (nbytes & 3); ++k) w |= (uint32_t)p[4 * nfull + k] << (8 * k);
    acc += word_term(word0 + nfull, w);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor((unsigned long long)acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, (unsigned long long)((red[0] + red[1]) + (red[2] + red[3])));
}
}  // namespace

extern "C" int ast_state_digest(const void* const* ptrs, const long long* nbytes, int n, unsigned long long* out, void* stream) {
  if (!ptrs || !nbytes || !out || n < 0) AST_FAIL("ast_state_digest: null list or output, or n < 0");
  if (((uintptr_t)out) & 7) AST_FAIL("ast_state_digest: out must be 8-byte aligned");
  uint64_t header = DIGEST_SEED;
  for (int e = 0; e < n; ++e) {                             // every entry is checked before anything is launched
    if (nbytes[e] < 0) AST_FAIL("ast_state_digest: entry %d: negative size", e);
    if (nbytes[e] > 0 && !ptrs[e]) AST_FAIL("ast_state_digest: entry %d: null pointer with %lld bytes", e, nbytes[e]);
    header += dmix64((dmix64((uint64_t)e) ^ DIGEST_LEN_KEY) + (uint64_t)nbytes[e]);
  }
  hipLaunchKernelGGL(digest_set_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, out, (unsigned long long)header);
  AST_CHECK_LAUNCH();
  uint64_t word0 = 0;
  for (int e = 0; e < n; ++e) {
    const uint64_t nb = (uint64_t)nbytes[e], words = (nb + 3) >> 2;
    if (nb == 0) continue;
    // a workgroup takes 4096 words (four 16-byte loads per thread); past 2048 workgroups (8 per CU) they loop instead
    const unsigned grid = (unsigned)std::min<uint64_t>((words + 4095) / 4096, 2048);
    hipLaunchKernelGGL(digest_entry_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)ptrs[e], nb, word0, out);
    AST_CHECK_LAUNCH();
    word0 += words;
  }
  hipLaunchKernelGGL(digest_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, out);
  AST_CHECK_LAUNCH();
  return 0;
}
