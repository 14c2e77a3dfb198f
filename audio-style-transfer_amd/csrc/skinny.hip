// Token-sized GEMMs on f32 MFMA (v_mfma_f32_16x16x4_f32, exact f32): the transformer / projection / discriminator linears with
// the fused-FFN epilogues, the two 294 462 x 256 linears of the simple decoder, and every linear weight gradient.  At <= 64 rows
// (B*(S+1) <= 40 in the benchmark) an MFMA macro tile would be >75 % padding and the launch is latency-bound, so a workgroup
// computes one 16-wide output tile with its waves splitting K (LDS reduce): short dependency chains.
// Every forward / data-gradient kernel is ONE template over RT, the number of 16-row accumulator tiles a wave keeps:
//   RT = 1  the <= 64-row entries: every 16-row tile has its own workgroup, the weight is fetched once per 16 rows;
//   RT = 4  the wide entries (65 .. AST_WIDE_MAX_ROWS rows): a workgroup covers 64 rows, a weight byte is fetched once per 64.
// Fragment layouts, K permutations, masking (clamped addresses, operands selected to zero, never a conditional dereference) and
// the order in which the waves' partials are added do not depend on RT.  The weight gradient + bias gradient are one launch
// that adds straight into the parameter gradient (no packed staging: plain linears have no spectral norm); its tile body
// (linear_wgrad_tile) is written once for the one-batch, the any-rows and the two batched kernels.
#include "ast_common.h"
#include "../../include/ast_hip.h"

namespace {

// the NW partial tiles of row tile t, added in wave order 0 .. NW-1
template <int NW, int RT>
__device__ __forceinline__ f32x4 sum_partials(const f32x4 (&part)[NW][RT][64], int t, int lane) {
  f32x4 r = part[0][t][lane];
#pragma unroll
  for (int q = 1; q < NW; ++q) { const f32x4 p = part[q][t][lane]; r[0] += p[0]; r[1] += p[1]; r[2] += p[2]; r[3] += p[3]; }
  return r;
}

// y[m][n] = act(sum_k x[m][k] * w[n][k] + b[n]).  One workgroup = one 16(n) x 16 RT (m) output tile; its NW waves split K and
// are reduced through LDS, wave t < RT finishing row tile t.  The weight tile is the A operand so each lane ends up with 4
// consecutive n of one token row m -> one 16-byte store.  Lane (i = l&15, g = l>>4) loads 16 B of row i at k = kb + 16 s + 4 g:
// the four MFMAs of a step contract k = 4 g + e over g (e = 0..3), the same k permutation on both operands.  The wave's weight
// slice is loaded once and meets RT x tiles.
// NW = waves per workgroup that split K (4; 8 for K = 1024, the FFN's second linear and the data gradient of its first:
// 16 dependent-free loads + 64 MFMAs per wave made those launches 8.9 us against 4.8 us for the K = 256 ones).
template <int RT, int NS, int NW>
__global__ __launch_bounds__(64 * NW) void skinny_gemm_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ bias, float* __restrict__ y, int M, int N,
                                                           int K, int ldx, int ldw, int ldy, int relu,
                                                           const float* __restrict__ mul_mask, float* __restrict__ drop_mask,
                                                           float p, uint64_t seed, const int64_t* __restrict__ d_offset) {
  __shared__ f32x4 part[NW][RT][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16, m0 = blockIdx.y * 16 * RT;
  constexpr int kslice = NS * 16;                     // k per wave (host: NW * kslice >= K)
  const int kb = wave * kslice;
  const bool nv = n0 + i < N;
  const float* wr = w + (size_t)(nv ? n0 + i : 0) * ldw;
  const float* xr[RT];
  bool mv[RT];
  f32x4 acc[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int m = m0 + 16 * t + i;
    mv[t] = m < M;
    xr[t] = x + (size_t)(mv[t] ? m : 0) * ldx;
    acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // the epilogue's bias values (lane: n = n0 + 4 g .. +3) are fetched with the first loads, not after the reduction
  float bq[4] = {0.f, 0.f, 0.f, 0.f};
  if (bias) {
#pragma unroll
    for (int q = 0; q < 4; ++q) { const int n = n0 + 4 * g + q; bq[q] = bias[n < N ? n : 0]; }
  }
  f32x4 wl[NS], xl[RT][NS];                           // every load of the wave's K slice is issued before the first MFMA
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int k = kb + s * 16 + 4 * g;
    const int kc = k < K ? k : 0;
    wl[s] = *reinterpret_cast<const f32x4*>(wr + kc);
#pragma unroll
    for (int t = 0; t < RT; ++t) xl[t][s] = *reinterpret_cast<const f32x4*>(xr[t] + kc);
  }
  // Without this fence the scheduler interleaves load -> s_waitcnt vmcnt(0) -> MFMA per step: 2*NS dependent round trips
  // (13.5 us per launch at K = 1024 instead of ~4).  The masking selects sit on the far side so they cannot pull
  // the waits forward.
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const bool kv = kb + s * 16 + 4 * g < K;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const f32x4 a = (kv && nv) ? wl[s] : z;
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const f32x4 b = (kv && mv[t]) ? xl[t][s] : z;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], acc[t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < RT; ++t) part[wave][t][lane] = acc[t];
  __syncthreads();
  if (wave >= RT) return;
  const int m = m0 + 16 * wave + i, nb = n0 + 4 * g;  // wave t finishes row tile t: D[row = 4 g + r (n)][col = i (m)]
  if (m >= M) return;
  const f32x4 r = sum_partials(part, wave, lane);
  // optional epilogues of the fused FFN: drop_mask != null draws the dropout mask here and stores the COMBINED
  // mask (0 where ReLU or dropout zeroed the unit, else 1/(1-p)) for the backward pass; mul_mask != null applies
  // such a mask to the result (the backward's dh = (dy W2) * mask).  The draw is indexed by m * ldy + n, so the mask
  // does not depend on the tiling.
  const uint64_t base = drop_mask ? mix64(seed ^ mix64((uint64_t)(d_offset ? *d_offset : 0))) : 0;
  const float keep = 1.f / (1.f - p);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int n = nb + q;
    if (n < N) {
      const size_t o = (size_t)m * ldy + n;
      float v = r[q] + bq[q];
      if (relu) v = fmaxf(v, 0.f);
      if (drop_mask) {
        const float km = dropout_keep(base, o, p, keep);
        drop_mask[o] = (relu && v <= 0.f) ? 0.f : km;
        v *= km;
      }
      if (mul_mask) v *= mul_mask[o];
      y[o] = v;
    }
  }
}

// ---- ast_bign_gemm_len: embedding_to_stft at inference, any row count up to AST_BIGN_MAX_ROWS, per-clip section counts ----------
// skinny_gemm_kernel's tile with a row mask and none of the training epilogues.  Row m = b S + s counts iff
// s < clamp(n_valid[b], 1, S) (n_valid == null: every row counts).  A row that does not count is masked like a row >= M (its x
// row is never read: clamped address, operand selected to zero) and stored as exactly 0; a 16-row tile without a row that counts
// issues no x load and no MFMA, and a workgroup whose RT tiles are all such tiles stores its zeros and leaves before any load.
// Both tests are wave-uniform (a ballot over the tile's rows).  Fragment layout, K slices per wave, MFMA order and the order of
// the partial sums (sum_partials) are skinny_gemm_kernel's, so a row that counts has the same bits from either kernel.  The text
// is a second copy because the existing kernels must compile to the code they had: sharing one inlined body reordered commutative
// operands in all eight of them (profiles/simple_infer/README.md).
// grid = (row blocks of 64, n tiles of 16): the row blocks are the fast index, so the up to 64 workgroups that share a 16 x K
// weight slice are dispatched next to each other and the slice comes from HBM about once; x (<= 4 MB) is re-read by every n tile
// and lives in L2 / Infinity Cache.
template <int NS, int NW>
__global__ __launch_bounds__(64 * NW) void bign_gemm_len_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ y, int M, int N,
                                                             int K, int ldw, int ldy, int S, const int32_t* __restrict__ n_valid) {
  constexpr int RT = 4;
  __shared__ f32x4 part[NW][RT][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.y * 16, m0 = blockIdx.x * 16 * RT;
  const int kb = wave * NS * 16;
  const bool nv = n0 + i < N;
  const float* wr = w + (size_t)(nv ? n0 + i : 0) * ldw;
  const float* xr[RT];
  bool mv[RT], live[RT];                              // lane's row of tile t counts; tile t holds such a row (wave-uniform)
  bool any_live = false;
  f32x4 acc[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int m = m0 + 16 * t + i;
    mv[t] = m < M;
    if (mv[t] && n_valid) {
      const int b = m / S, nb = n_valid[b];
      mv[t] = m - b * S < (nb < 1 ? 1 : nb > S ? S : nb);
    }
    live[t] = __any(mv[t]);
    any_live = any_live || live[t];
    xr[t] = x + (size_t)(mv[t] ? m : 0) * K;
    acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  if (!any_live) {                                    // the same answer in every wave: the whole workgroup leaves
    const int m = m0 + 16 * wave + i;
    if (wave < RT && m < M) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (n0 + 4 * g + q < N) y[(size_t)m * ldy + n0 + 4 * g + q] = 0.f;
    }
    return;
  }
  float bq[4] = {0.f, 0.f, 0.f, 0.f};
  if (bias) {
#pragma unroll
    for (int q = 0; q < 4; ++q) { const int n = n0 + 4 * g + q; bq[q] = bias[n < N ? n : 0]; }
  }
  f32x4 wl[NS], xl[RT][NS];                           // every load of the wave's K slice is issued before the first MFMA
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int k = kb + s * 16 + 4 * g;
    const int kc = k < K ? k : 0;
    wl[s] = *reinterpret_cast<const f32x4*>(wr + kc);
  }
#pragma unroll
  for (int t = 0; t < RT; ++t) {
#pragma unroll
    for (int s = 0; s < NS; ++s) xl[t][s] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!live[t]) continue;                           // one uniform branch per row tile
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int k = kb + s * 16 + 4 * g;
      xl[t][s] = *reinterpret_cast<const f32x4*>(xr[t] + (k < K ? k : 0));
    }
  }
  __builtin_amdgcn_sched_barrier(0);                  // see skinny_gemm_kernel
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const bool kv = kb + s * 16 + 4 * g < K;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const f32x4 a = (kv && nv) ? wl[s] : z;
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      if (!live[t]) continue;
      const f32x4 b = (kv && mv[t]) ? xl[t][s] : z;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], acc[t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < RT; ++t) part[wave][t][lane] = acc[t];
  __syncthreads();
  if (wave >= RT) return;
  const int m = m0 + 16 * wave + i, nb = n0 + 4 * g;  // wave t finishes row tile t: D[row = 4 g + r (n)][col = i (m)]
  if (m >= M) return;
  bool counts = false;
#pragma unroll
  for (int t = 0; t < RT; ++t) counts = counts || (t == wave && mv[t]);
  f32x4 r = {0.f, 0.f, 0.f, 0.f};                     // a row that does not count: exactly 0, no bias
  if (counts) {
    r = sum_partials(part, wave, lane);
#pragma unroll
    for (int q = 0; q < 4; ++q) r[q] += bq[q];
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (nb + q < N) y[(size_t)m * ldy + nb + q] = r[q];
}

// dW[n][k] += sum_m dy[m][n] x[m][k] ; db[n] += sum_m dy[m][n]   (contraction over the token rows).
// One wave = 16 n x 64 k of dW (n tile nt of 64 split over the workgroup's 4 waves, k tile kt): A[i][g] = dy[4s+g][n0+i],
// B[g][j] = x[4s+g][k0+j] (16 lanes read 16 consecutive floats), the A fragment reused by 4 k-tiles.  The rows are walked in
// ascending batches of MS MFMA k-steps (4 MS rows), every load of a batch issued before its first MFMA, accumulating in
// registers; ONE read-add-store of dW at the end.  LOOP = false: the caller guarantees M <= 4 MS and there is no loop; LOOP = true:
// the trip count is unknown and the loop stays rolled (the listings hold one batch of 4 MS MFMAs).  No
// other wave touches the tile and the row order is fixed, so the result is the same bits on every call.
template <int MS, bool LOOP>
__device__ __forceinline__ void linear_wgrad_tile(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dW,
                                                  float* __restrict__ db, int M, int N, int K, int lddy, int ldw, int nt, int kt) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int n0 = (nt * 4 + wave) * 16, k0 = kt * 64;
  if (n0 >= N) return;
  const bool nv = n0 + i < N;
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  for (int st0 = 0; st0 * 4 < (LOOP ? M : 1); st0 += MS) {    // st0 = first MFMA k-step (4 rows each) of the batch
    float av[MS], bv[MS][4];
#pragma unroll
    for (int st = 0; st < MS; ++st) {                      // raw loads first (clamped addresses) ...
      const int m = (st0 + st) * 4 + g;
      const bool mv = m < M;
      av[st] = dy[(size_t)(mv ? m : 0) * lddy + (nv ? n0 + i : 0)];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int k = k0 + t * 16 + i;
        const bool kv = mv && k < K;
        bv[st][t] = x[(size_t)(kv ? m : 0) * K + (kv ? k : 0)];
      }
    }
    __builtin_amdgcn_sched_barrier(0);                     // ... so that the batch's 5 MS loads are in flight together (see skinny_gemm_kernel)
#pragma unroll
    for (int st = 0; st < MS; ++st) {
      const bool mv = (st0 + st) * 4 + g < M;
      const float a = (mv && nv) ? av[st] : 0.f;
      bsum += a;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float b = (mv && k0 + t * 16 + i < K) ? bv[st][t] : 0.f;
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[t], 0, 0, 0);
      }
    }
  }
  // D[row = n0 + 4 g + r][col = k0 + 16 t + i]; the 16 old values are fetched together, then added and stored
  float old[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int k = k0 + t * 16 + i;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + 4 * g + r;
      old[t][r] = (k < K && n < N) ? dW[(size_t)n * ldw + k] : 0.f;
    }
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int k = k0 + t * 16 + i;
    if (k >= K) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + 4 * g + r;
      if (n < N) dW[(size_t)n * ldw + k] = old[t][r] + acc[t][r];
    }
  }
  if (db && kt == 0) {
    bsum += __shfl_xor(bsum, 16, 64);
    bsum += __shfl_xor(bsum, 32, 64);
    if (g == 0 && nv) db[n0 + i] += bsum;
  }
}

// <= 4 MS token rows (MS = 4, 8, 16): all of them are loaded before the first MFMA.  grid = (k tiles of 64, n tiles of 64).
template <int MS>
__global__ __launch_bounds__(256) void linear_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                            float* __restrict__ dW, float* __restrict__ db, int M, int N, int K,
                                                            int lddy, int ldw) {
  linear_wgrad_tile<MS, false>(dy, x, dW, db, M, N, K, lddy, ldw, blockIdx.y, blockIdx.x);
}

// Any number of rows (the wide entry): ascending 64-row chunks.  It serves both modes.
__global__ __launch_bounds__(256) void linear_wgrad_rows_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                 float* __restrict__ dW, float* __restrict__ db, int M, int N, int K,
                                                                 int lddy, int ldw) {
  linear_wgrad_tile<16, true>(dy, x, dW, db, M, N, K, lddy, ldw, blockIdx.y, blockIdx.x);
}

// Batched form: one launch for every deferred linear weight gradient of a model.
// table[e] = {dy, x, dW, db, M, N, K, lddy, ldw}; blockIdx.y = entry, blockIdx.x = (k tile, n tile-of-64) of that entry;
// 16 token rows per batch of loads.
struct LinWg { const float* dy; const float* x; float* dW; float* db; int M, N, K, lddy, ldw, pad0, pad1, pad2; };

__device__ __forceinline__ void linear_wgrad_record(const LinWg& e) {
  const int ktiles = (e.K + 63) / 64, ntiles = (e.N + 63) / 64;
  if ((int)blockIdx.x >= ktiles * ntiles) return;
  linear_wgrad_tile<4, true>(e.dy, e.x, e.dW, e.db, e.M, e.N, e.K, e.lddy, e.ldw, blockIdx.x / ktiles, blockIdx.x % ktiles);
}

// The records travel as a by-value kernel argument (<= 56 x 64 B, under the 4 KB kernarg limit): no device table, no
// host-to-device copy node in the captured step (each such memcpy node cost a 20-75 us bubble in the replay).
constexpr int LINWG_MAX = 56;
struct LinWgArgs { LinWg rec[LINWG_MAX]; };

__global__ __launch_bounds__(256) void linear_wgrad_batched_args_kernel(const LinWgArgs tab) {
  linear_wgrad_record(tab.rec[blockIdx.y]);        // uniform index: scalar loads from the kernarg segment
}

__global__ __launch_bounds__(256) void linear_wgrad_batched_kernel(const LinWg* __restrict__ table) {
  linear_wgrad_record(table[blockIdx.y]);
}

// ---- the two 294 462 x 256 linears of SimpleDecoder_TransformerOnly.py:16-17 ----------------------------------------------------
// Both are streams over a 301 MB weight matrix with a few token rows: HBM-bound, f32 MFMA 16x16x4.
//
// Y[m][n] += sum_k X[m][k] W[n][k]   (stft_to_embedding: N = 256, K = 2*287*513).  K is even but not a multiple of
// 4, so rows are only 8-byte aligned: lane (i, g) loads 2 floats at k = kb + 8 s + 2 g and the two MFMAs of a step
// contract k = 2 g + e over g.  grid = (N/16, M/(16 RT), K chunks of 1024); a workgroup's 4 waves split its chunk (a wave's
// 16 n x 256 k weight slice meets RT x tiles), reduce through LDS (wave t < RT: row tile t) and add the partial tile into Y
// with f32 atomics (Y is pre-zeroed; chunk 0 adds the bias).
// DET (deterministic mode): K chunk z STORES its partial tile into its own [M][N] slab y + z * M * N (an ast_ordered_sum adds the
// slabs in chunk order) instead of adding it into Y with atomics.
template <int RT, bool DET>
__global__ __launch_bounds__(256) void bigk_gemm_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ y, int M, int N, int K,
                                                         int ldy) {
  __shared__ f32x4 part[4][RT][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16, m0 = blockIdx.y * 16 * RT;
  const int kb = blockIdx.z * 1024 + wave * 256;
  const bool nv = n0 + i < N;
  const float* wr = w + (size_t)(nv ? n0 + i : 0) * K;
  const float* xr[RT];
  bool mv[RT];
  f32x4 acc[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int m = m0 + 16 * t + i;
    mv[t] = m < M;
    xr[t] = x + (size_t)(mv[t] ? m : 0) * K;
    acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll 1
  for (int sb = 0; sb < 32; sb += 8) {
    f32x2 wl[8], xl[RT][8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int k = kb + (sb + s) * 8 + 2 * g;
      const int kc = k < K ? k : 0;                            // K even: k and k+1 are valid together
      wl[s] = *reinterpret_cast<const f32x2*>(wr + kc);
#pragma unroll
      for (int t = 0; t < RT; ++t) xl[t][s] = *reinterpret_cast<const f32x2*>(xr[t] + kc);
    }
    __builtin_amdgcn_sched_barrier(0);                         // 8 (1 + RT) loads in flight together (see skinny_gemm_kernel)
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const bool kv = kb + (sb + s) * 8 + 2 * g < K;
      const f32x2 z = {0.f, 0.f};
      const f32x2 a = (kv && nv) ? wl[s] : z;
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        const f32x2 b = (kv && mv[t]) ? xl[t][s] : z;
#pragma unroll
        for (int e = 0; e < 2; ++e) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], acc[t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < RT; ++t) part[wave][t][lane] = acc[t];
  __syncthreads();
  if (wave >= RT) return;
  const int m = m0 + 16 * wave + i, nb = n0 + 4 * g;          // D[row = 4 g + r (n)][col = i (m)]
  if (m >= M) return;
  const f32x4 r = sum_partials(part, wave, lane);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int n = nb + q;
    if (n >= N) continue;
    const float v = r[q] + ((bias && blockIdx.z == 0) ? bias[n] : 0.f);
    if constexpr (DET) y[((size_t)blockIdx.z * M + m) * N + n] = v;
    else unsafeAtomicAdd(y + (size_t)m * ldy + n, v);
  }
}

// dX[m][k] += sum_n dY[m][n] W[n][k]   (data gradient of embedding_to_stft: N = 2*287*513 contracted, K = 256 kept).
// A workgroup owns a chunk of 512 n for ALL k and 16 RT rows: wave w keeps the k tiles 4w..4w+3 for its RT row tiles
// (D[k][m] = sum_n W[n][k] dY[m][n]; lane (i, g): A = W[nb + 4 s + g][k0 + i], 16 lanes = 64 contiguous bytes of a weight row;
// B = dY[m0 + 16 u + i][nb + 4 s + g]); a weight fragment is loaded once and meets RT dY tiles.  grid = (n chunks of 512, M/(16 RT)).
// DET: n chunk blockIdx.x STORES its partial into its own [M][K] slab dx + blockIdx.x * M * K (summed in chunk order afterwards)
template <int RT, bool DET>
__global__ __launch_bounds__(256) void bign_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                          float* __restrict__ dx, int M, int N, int K, int lddy) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int nb0 = blockIdx.x * 512, m0 = blockIdx.y * 16 * RT;
  const int kt0 = wave * 4;                                    // first of this wave's four 16-wide k tiles (K <= 256)
  const float* dr[RT];
  bool mv[RT];
  f32x4 acc[RT][4];                                            // [row tile][k tile]
#pragma unroll
  for (int u = 0; u < RT; ++u) {
    const int m = m0 + 16 * u + i;
    mv[u] = m < M;
    dr[u] = dy + (size_t)(mv[u] ? m : 0) * lddy;
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll 1
  for (int sb = 0; sb < 128; sb += 8) {
    float a[8][4], b[RT][8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int n = nb0 + (sb + s) * 4 + g;
      const int nc = n < N ? n : 0;
#pragma unroll
      for (int u = 0; u < RT; ++u) b[u][s] = dr[u][nc];
      const float* wrow = w + (size_t)nc * K;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int k = (kt0 + t) * 16 + i;
        a[s][t] = wrow[k < K ? k : 0];
      }
    }
    __builtin_amdgcn_sched_barrier(0);                         // 8 (4 + RT) loads in flight together (see skinny_gemm_kernel)
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const bool nvv = nb0 + (sb + s) * 4 + g < N;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float aq = (nvv && (kt0 + t) * 16 + i < K) ? a[s][t] : 0.f;
#pragma unroll
        for (int u = 0; u < RT; ++u) {
          const float bq = (nvv && mv[u]) ? b[u][s] : 0.f;
          acc[u][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq, bq, acc[u][t], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < RT; ++u) {
    const int m = m0 + 16 * u + i;                             // D[row = 4 g + r (k)][col = i (m)]
    if (m >= M) continue;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = (kt0 + t) * 16 + 4 * g + r;
        if (k >= K) continue;
        if constexpr (DET) dx[((size_t)blockIdx.x * M + m) * K + k] = acc[u][t][r];
        else unsafeAtomicAdd(dx + (size_t)m * K + k, acc[u][t][r]);
      }
  }
}

// ---- backward of the length-masked output linear (ast_bign_gemm_len in training) ------------------------------------------------
// Row m = b S + s counts iff s < clamp(n_valid[b], 1, S) (n_valid == null: every row counts); the clamp makes row 0 of every clip
// count, so the clamped address of a masked row (row 0) is always a row that may be read.
__device__ __forceinline__ bool row_counts(int m, int M, int S, const int32_t* __restrict__ n_valid) {
  if (m >= M) return false;
  if (!n_valid) return true;
  const int b = m / S, nb = n_valid[b];
  return m - b * S < (nb < 1 ? 1 : nb > S ? S : nb);
}

// bign_dgrad_kernel with the row mask.  A row that does not count is masked like a row >= M (its dy row is never read: clamped
// address, operand selected to zero) and its dx row is exactly 0; a 16-row tile without a row that counts issues no dy load and no
// MFMA; a workgroup whose RT tiles are all such tiles leaves before any load (DET: after storing the zeros of its slab).  Both
// tests are wave-uniform (a ballot over the tile's rows).  Loop structure and MFMA order are bign_dgrad_kernel's, so with every
// row counting the DET form gives its bits.  A second copy of the text for the reason given at bign_gemm_len_kernel.
template <int RT, bool DET>
__global__ __launch_bounds__(256) void bign_dgrad_len_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                              float* __restrict__ dx, int M, int N, int K, int lddy, int S,
                                                              const int32_t* __restrict__ n_valid) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int nb0 = blockIdx.x * 512, m0 = blockIdx.y * 16 * RT;
  const int kt0 = wave * 4;                                    // first of this wave's four 16-wide k tiles (K <= 256)
  const float* dr[RT];
  bool mv[RT], live[RT];                                       // lane's row of tile u counts; tile u holds such a row (wave-uniform)
  bool any_live = false;
  f32x4 acc[RT][4];                                            // [row tile][k tile]
#pragma unroll
  for (int u = 0; u < RT; ++u) {
    const int m = m0 + 16 * u + i;
    mv[u] = row_counts(m, M, S, n_valid);
    live[u] = __any(mv[u]);
    any_live = any_live || live[u];
    dr[u] = dy + (size_t)(mv[u] ? m : 0) * lddy;
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  if (any_live) {                                              // the same answer in every wave
#pragma unroll 1
    for (int sb = 0; sb < 128; sb += 8) {
      float a[8][4], b[RT][8];
#pragma unroll
      for (int u = 0; u < RT; ++u) {
#pragma unroll
        for (int s = 0; s < 8; ++s) b[u][s] = 0.f;
        if (!live[u]) continue;                                // one uniform branch per row tile
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const int n = nb0 + (sb + s) * 4 + g;
          b[u][s] = dr[u][n < N ? n : 0];
        }
      }
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int n = nb0 + (sb + s) * 4 + g;
        const float* wrow = w + (size_t)(n < N ? n : 0) * K;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int k = (kt0 + t) * 16 + i;
          a[s][t] = wrow[k < K ? k : 0];
        }
      }
      __builtin_amdgcn_sched_barrier(0);                       // the loads of the batch in flight together (see skinny_gemm_kernel)
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const bool nvv = nb0 + (sb + s) * 4 + g < N;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float aq = (nvv && (kt0 + t) * 16 + i < K) ? a[s][t] : 0.f;
#pragma unroll
          for (int u = 0; u < RT; ++u) {
            if (!live[u]) continue;
            const float bq = (nvv && mv[u]) ? b[u][s] : 0.f;
            acc[u][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq, bq, acc[u][t], 0, 0, 0);
          }
        }
      }
    }
  } else if (!DET) {
    return;                                                    // dx was zeroed by the launcher
  }
#pragma unroll
  for (int u = 0; u < RT; ++u) {
    const int m = m0 + 16 * u + i;                             // D[row = 4 g + r (k)][col = i (m)]
    if (m >= M) continue;
    if (!DET && !mv[u]) continue;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = (kt0 + t) * 16 + 4 * g + r;
        if (k >= K) continue;
        if constexpr (DET) dx[((size_t)blockIdx.x * M + m) * K + k] = mv[u] ? acc[u][t][r] : 0.f;
        else unsafeAtomicAdd(dx + (size_t)m * K + k, acc[u][t][r]);
      }
  }
}

// linear_wgrad_tile<MS, LOOP> (MS = 4, 8, 16 without a loop for <= 64 rows, <16, true> = the row-chunked form of
// linear_wgrad_rows_kernel beyond; no atomics, both modes) with the row mask: a row that does not count is read from neither dy nor
// x (clamped addresses, operands selected to zero -- NaN there reaches nothing), and a batch of 4 MS rows without a row that counts
// is skipped.  The mask of a batch is formed ONCE per wave: lane l tests row 4 st0 + l (one division, one n_valid load), a ballot
// makes the 64 answers a wave-uniform 64-bit word, and the row of MFMA step st, lane group g is its bit 4 st + g.  A masked row
// adds exact zeros, so with every row counting the result has the bits of ast_linear_wgrad[_wide].
template <int MS, bool LOOP>
__global__ __launch_bounds__(256) void linear_wgrad_len_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                float* __restrict__ dW, float* __restrict__ db, int M, int N, int K,
                                                                int lddy, int ldw, int S, const int32_t* __restrict__ n_valid) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int n0 = (blockIdx.y * 4 + wave) * 16, k0 = blockIdx.x * 64;
  if (n0 >= N) return;
  const bool nv = n0 + i < N;
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  for (int st0 = 0; st0 * 4 < (LOOP ? M : 1); st0 += MS) {     // st0 = first MFMA k-step (4 rows each) of the batch
    // LOOP = false: M <= 4 MS, so the lanes past 4 MS test rows >= M and answer no
    const unsigned long long rows = __ballot(row_counts(st0 * 4 + lane, M, S, n_valid));
    if (rows == 0) continue;
    const unsigned long long mine = rows >> g;                 // bit 4 st: this lane's row of step st0 + st counts
    unsigned cmask = 0;
#pragma unroll
    for (int st = 0; st < MS; ++st) cmask |= (unsigned)((mine >> (4 * st)) & 1ull) << st;
    float av[MS], bv[MS][4];
#pragma unroll
    for (int st = 0; st < MS; ++st) {                          // raw loads first (clamped addresses) ...
      const int m = (st0 + st) * 4 + g;
      const bool mv = (cmask >> st) & 1u;
      av[st] = dy[(size_t)(mv ? m : 0) * lddy + (nv ? n0 + i : 0)];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int k = k0 + t * 16 + i;
        const bool kv = mv && k < K;
        bv[st][t] = x[(size_t)(kv ? m : 0) * K + (kv ? k : 0)];
      }
    }
    __builtin_amdgcn_sched_barrier(0);                         // ... so that the chunk's loads are in flight together
#pragma unroll
    for (int st = 0; st < MS; ++st) {
      const bool mv = (cmask >> st) & 1u;
      const float a = (mv && nv) ? av[st] : 0.f;
      bsum += a;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float b = (mv && k0 + t * 16 + i < K) ? bv[st][t] : 0.f;
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[t], 0, 0, 0);
      }
    }
  }
  // D[row = n0 + 4 g + r][col = k0 + 16 t + i]; the 16 old values are fetched together, then added and stored
  float old[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int k = k0 + t * 16 + i;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + 4 * g + r;
      old[t][r] = (k < K && n < N) ? dW[(size_t)n * ldw + k] : 0.f;
    }
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int k = k0 + t * 16 + i;
    if (k >= K) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + 4 * g + r;
      if (n < N) dW[(size_t)n * ldw + k] = old[t][r] + acc[t][r];
    }
  }
  if (db && blockIdx.x == 0) {
    bsum += __shfl_xor(bsum, 16, 64);
    bsum += __shfl_xor(bsum, 32, 64);
    if (g == 0 && nv) db[n0 + i] += bsum;
  }
}

// ---- host side: one launcher per operation.  RT also fixes the row range an entry takes: RT = 1 -> 1 .. 64 rows, RT = 4 ->
// 65 .. AST_WIDE_MAX_ROWS rows; only the wide entries check the leading dimensions.  `name` is the entry named in messages.
template <int RT> constexpr int rows_lo() { return RT == 1 ? 1 : 65; }
template <int RT> constexpr int rows_hi() { return RT == 1 ? 64 : AST_WIDE_MAX_ROWS; }
template <int RT> constexpr bool rows_ok(int M) { return M >= rows_lo<RT>() && M <= rows_hi<RT>(); }

template <int RT>
int skinny_gemm_launch(const char* name, const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int ldw,
                       int ldy, int relu, const float* mul_mask, float* drop_mask, float p, uint64_t seed, const int64_t* d_offset,
                       void* stream) {
  if (!x || !w || !y || !rows_ok<RT>(M) || N < 1 || K < 4 || (K & 3) || (ldw & 3) || (RT > 1 && (ldw < K || ldy < N)))
    AST_FAIL("%s: bad args M=%d (%d..%d) N=%d K=%d ldw=%d ldy=%d", name, M, rows_lo<RT>(), rows_hi<RT>(), N, K, ldw, ldy);
  if ((((uintptr_t)x) | ((uintptr_t)w)) & 15) AST_FAIL("%s: operands must be 16-byte aligned", name);
  if (drop_mask && (p <= 0.f || p >= 1.f)) AST_FAIL("%s: dropout epilogue needs 0 < p < 1", name);
  const int steps = (K + 63) / 64;                    // 16-wide K steps per wave when 4 waves split K
  if (steps > 16) AST_FAIL("%s: K=%d too large for the token path (<= 1024)", name, K);
  dim3 grid((N + 15) / 16, (M + 16 * RT - 1) / (16 * RT));
#define AST_SK(NS_, NW_) hipLaunchKernelGGL((skinny_gemm_kernel<RT, NS_, NW_>), grid, dim3(64 * NW_), 0, (hipStream_t)stream, x, w, bias, y, \
                                            M, N, K, K, ldw, ldy, relu, mul_mask, drop_mask, p, seed, d_offset)
  if (steps <= 2) AST_SK(2, 4);
  else if (steps <= 4) AST_SK(4, 4);
  else if (steps <= 8) AST_SK(8, 4);
  else AST_SK(8, 8);                                  // eight waves, 8 steps each
#undef AST_SK
  AST_CHECK_LAUNCH();
  return 0;
}

// any row count up to AST_BIGN_MAX_ROWS, per-clip counts on the device; K / ldw / ldy / alignment rules of the wide entry
int bign_gemm_len_launch(const char* name, const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int ldw,
                         int ldy, int S, const int32_t* n_valid, void* stream) {
  if (!x || !w || !y || M < 1 || M > AST_BIGN_MAX_ROWS || S < 1 || M % S || N < 1 || K < 4 || (K & 3) || (ldw & 3) || ldw < K || ldy < N)
    AST_FAIL("%s: bad args M=%d (1..%d) S=%d (M %% S == 0) N=%d K=%d ldw=%d ldy=%d", name, M, AST_BIGN_MAX_ROWS, S, N, K, ldw, ldy);
  if ((((uintptr_t)x) | ((uintptr_t)w)) & 15) AST_FAIL("%s: operands must be 16-byte aligned", name);
  if ((((uintptr_t)y) | ((uintptr_t)bias) | ((uintptr_t)n_valid)) & 3) AST_FAIL("%s: y, bias and n_valid must be 4-byte aligned", name);
  const int steps = (K + 63) / 64;
  if (steps > 16) AST_FAIL("%s: K=%d too large for the token path (<= 1024)", name, K);
  if ((N + 15) / 16 > 65535) AST_FAIL("%s: N=%d too large (<= %d)", name, N, 65535 * 16);
  dim3 grid((M + 63) / 64, (N + 15) / 16);
#define AST_BL(NS_, NW_) hipLaunchKernelGGL((bign_gemm_len_kernel<NS_, NW_>), grid, dim3(64 * NW_), 0, (hipStream_t)stream, x, w, bias, y, \
                                            M, N, K, ldw, ldy, S, n_valid)
  if (steps <= 2) AST_BL(2, 4);
  else if (steps <= 4) AST_BL(4, 4);
  else if (steps <= 8) AST_BL(8, 4);
  else AST_BL(8, 8);
#undef AST_BL
  AST_CHECK_LAUNCH();
  return 0;
}

template <int RT>
int linear_wgrad_launch(const char* name, const float* dy, const float* x, float* dW, float* db, int M, int N, int K, int lddy, int ldw,
                        void* stream) {
  if (!dy || !x || !dW || !rows_ok<RT>(M) || N < 1 || K < 1 || (RT > 1 && (lddy < N || ldw < K)))
    AST_FAIL("%s: bad args M=%d (%d..%d token rows) N=%d K=%d lddy=%d ldw=%d", name, M, rows_lo<RT>(), rows_hi<RT>(), N, K, lddy, ldw);
  dim3 grid((K + 63) / 64, (N + 63) / 64);
  if (RT > 1 && grid.y > 65535) AST_FAIL("%s: N=%d too large", name, N);
  hipStream_t s = (hipStream_t)stream;
  if (RT > 1) hipLaunchKernelGGL(linear_wgrad_rows_kernel, grid, dim3(256), 0, s, dy, x, dW, db, M, N, K, lddy, ldw);
  else if (M <= 16) hipLaunchKernelGGL(linear_wgrad_kernel<4>, grid, dim3(256), 0, s, dy, x, dW, db, M, N, K, lddy, ldw);
  else if (M <= 32) hipLaunchKernelGGL(linear_wgrad_kernel<8>, grid, dim3(256), 0, s, dy, x, dW, db, M, N, K, lddy, ldw);
  else hipLaunchKernelGGL(linear_wgrad_kernel<16>, grid, dim3(256), 0, s, dy, x, dW, db, M, N, K, lddy, ldw);
  AST_CHECK_LAUNCH();
  return 0;
}

// DET (the deterministic forms of include/ast_hip.h): the K chunks' slabs go to ws and are added into y in chunk order; ldy == N.
template <int RT, bool DET>
int bigk_gemm_launch(const char* name, const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int ldy, float* ws,
                     long ws_floats, void* stream) {
  if (!x || !w || !y || (DET && !ws) || !rows_ok<RT>(M) || N < 1 || K < 2 || (K & 1) || (RT > 1 && ldy < N))
    AST_FAIL("%s: bad args M=%d (%d..%d) N=%d K=%d (K must be even) ldy=%d", name, M, rows_lo<RT>(), rows_hi<RT>(), N, K, ldy);
  if ((((uintptr_t)x) | ((uintptr_t)w)) & 7) AST_FAIL("%s: operands must be 8-byte aligned", name);
  const int nz = (K + 1023) / 1024;
  if ((RT > 1 || DET) && nz > (RT > 1 ? 65535 : AST_DET_MAX_SLOTS)) AST_FAIL("%s: K=%d too large", name, K);
  if (DET && ws_floats < (long)nz * M * N) AST_FAIL("%s: ws needs %ld floats", name, (long)nz * M * N);
  dim3 grid((N + 15) / 16, (M + 16 * RT - 1) / (16 * RT), nz);
  if (!DET) AST_HIP(hipMemsetAsync(y, 0, sizeof(float) * (size_t)M * ldy, (hipStream_t)stream));
  hipLaunchKernelGGL((bigk_gemm_kernel<RT, DET>), grid, dim3(256), 0, (hipStream_t)stream, x, w, bias, DET ? ws : y, M, N, K, ldy);
  AST_CHECK_LAUNCH();
  return DET ? ast_ordered_sum(ws, (int64_t)M * N, nz, 1, y, 0, stream) : 0;
}

// DET: the n chunks' slabs go to ws and are added into dx in chunk order.
template <int RT, bool DET>
int bign_dgrad_launch(const char* name, const float* dy, const float* w, float* dx, int M, int N, int K, int lddy, float* ws, long ws_floats,
                      void* stream) {
  if (!dy || !w || !dx || (DET && !ws) || !rows_ok<RT>(M) || N < 1 || K < 1 || K > 256 || (RT > 1 && lddy < N))
    AST_FAIL("%s: bad args M=%d (%d..%d) N=%d K=%d (K <= 256) lddy=%d", name, M, rows_lo<RT>(), rows_hi<RT>(), N, K, lddy);
  const int nx = (N + 511) / 512;
  if (DET && (nx > AST_DET_MAX_SLOTS || ws_floats < (long)nx * M * K)) AST_FAIL("%s: ws needs %ld floats", name, (long)nx * M * K);
  dim3 grid(nx, (M + 16 * RT - 1) / (16 * RT));
  if (!DET) AST_HIP(hipMemsetAsync(dx, 0, sizeof(float) * (size_t)M * K, (hipStream_t)stream));
  hipLaunchKernelGGL((bign_dgrad_kernel<RT, DET>), grid, dim3(256), 0, (hipStream_t)stream, dy, w, DET ? ws : dx, M, N, K, lddy);
  AST_CHECK_LAUNCH();
  return DET ? ast_ordered_sum(ws, (int64_t)M * K, nx, 1, dx, 0, stream) : 0;
}
// the masked data gradient: 1 .. AST_WIDE_MAX_ROWS rows, the 1- or 4-row-tile form picked here
template <bool DET>
int bign_dgrad_len_launch(const char* name, const float* dy, const float* w, float* dx, int M, int N, int K, int lddy, int S,
                          const int32_t* n_valid, float* ws, long ws_floats, void* stream) {
  if (!dy || !w || !dx || (DET && !ws)) AST_FAIL("%s: bad args (null dy, w, dx%s)", name, DET ? " or ws" : "");
  if (M < 1 || M > AST_WIDE_MAX_ROWS || S < 1 || M % S || N < 1 || K < 1 || K > 256 || lddy < N)
    AST_FAIL("%s: bad args M=%d (1..%d) S=%d (M %% S == 0) N=%d K=%d (K <= 256) lddy=%d", name, M, AST_WIDE_MAX_ROWS, S, N, K, lddy);
  if ((((uintptr_t)dy) | ((uintptr_t)w) | ((uintptr_t)dx) | ((uintptr_t)ws) | ((uintptr_t)n_valid)) & 3)
    AST_FAIL("%s: dy, w, dx, ws and n_valid must be 4-byte aligned", name);
  const int nx = (N - 1) / 512 + 1;                             // N >= 1: no overflow at the largest int
  if (DET && (nx > AST_DET_MAX_SLOTS || ws_floats < (long)nx * M * K)) AST_FAIL("%s: ws needs %ld floats (at most %d slabs)", name, (long)nx * M * K, AST_DET_MAX_SLOTS);
  hipStream_t s = (hipStream_t)stream;
  if (!DET) AST_HIP(hipMemsetAsync(dx, 0, sizeof(float) * (size_t)M * K, s));
  if (M <= 64)
    hipLaunchKernelGGL((bign_dgrad_len_kernel<1, DET>), dim3(nx, (M + 15) / 16), dim3(256), 0, s, dy, w, DET ? ws : dx, M, N, K, lddy, S, n_valid);
  else
    hipLaunchKernelGGL((bign_dgrad_len_kernel<4, DET>), dim3(nx, (M + 63) / 64), dim3(256), 0, s, dy, w, DET ? ws : dx, M, N, K, lddy, S, n_valid);
  AST_CHECK_LAUNCH();
  return DET ? ast_ordered_sum(ws, (int64_t)M * K, nx, 1, dx, 0, stream) : 0;
}
}  // namespace

// ---- backward of the length-masked output linear (include/ast_hip.h) --------------------------------------------------------------
extern "C" int ast_bign_dgrad_len(const float* dy, const float* w, float* dx, int M, int N, int K, int lddy, int S, const int32_t* n_valid,
                                  void* stream) {
  return bign_dgrad_len_launch<false>("ast_bign_dgrad_len", dy, w, dx, M, N, K, lddy, S, n_valid, nullptr, 0, stream);
}

extern "C" long ast_bign_dgrad_len_det_ws_floats(int M, int N, int K) {
  if (M < 1 || M > AST_WIDE_MAX_ROWS || N < 1 || K < 1 || K > 256 || (N - 1) / 512 + 1 > AST_DET_MAX_SLOTS) return -1;
  return (long)((N - 1) / 512 + 1) * M * K;
}

extern "C" int ast_bign_dgrad_len_det(const float* dy, const float* w, float* dx, int M, int N, int K, int lddy, int S,
                                      const int32_t* n_valid, float* ws, long ws_floats, void* stream) {
  return bign_dgrad_len_launch<true>("ast_bign_dgrad_len_det", dy, w, dx, M, N, K, lddy, S, n_valid, ws, ws_floats, stream);
}

extern "C" int ast_linear_wgrad_len(const float* dy, const float* x, float* dW, float* db, int M, int N, int K, int lddy, int ldw, int S,
                                    const int32_t* n_valid, void* stream) {
  if (!dy || !x || !dW) AST_FAIL("ast_linear_wgrad_len: bad args (null dy, x or dW)");
  if (M < 1 || M > AST_WIDE_MAX_ROWS || S < 1 || M % S || N < 1 || K < 1 || lddy < N || ldw < K)
    AST_FAIL("ast_linear_wgrad_len: bad args M=%d (1..%d token rows) S=%d (M %% S == 0) N=%d K=%d lddy=%d ldw=%d", M, AST_WIDE_MAX_ROWS, S, N, K,
             lddy, ldw);
  if ((((uintptr_t)dy) | ((uintptr_t)x) | ((uintptr_t)dW) | ((uintptr_t)db) | ((uintptr_t)n_valid)) & 3)
    AST_FAIL("ast_linear_wgrad_len: dy, x, dW, db and n_valid must be 4-byte aligned");
  dim3 grid((K - 1) / 64 + 1, (N - 1) / 64 + 1);              // N, K >= 1: no overflow at the largest int
  if (grid.y > 65535) AST_FAIL("ast_linear_wgrad_len: N=%d too large (<= %d)", N, 65535 * 64);
  hipStream_t s = (hipStream_t)stream;                         // the row batches of ast_linear_wgrad / ast_linear_wgrad_wide
#define AST_WL(MS_, LOOP_) hipLaunchKernelGGL((linear_wgrad_len_kernel<MS_, LOOP_>), grid, dim3(256), 0, s, dy, x, dW, db, M, N, K, lddy, ldw, S, n_valid)
  if (M <= 16) AST_WL(4, false);
  else if (M <= 32) AST_WL(8, false);
  else if (M <= 64) AST_WL(16, false);
  else AST_WL(16, true);
#undef AST_WL
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" int ast_linear_wgrad_batched_host(const void* host_table, int count, int max_tiles, void* stream) {
  if (!host_table || count <= 0 || max_tiles <= 0) AST_FAIL("ast_linear_wgrad_batched_host: bad args");
  const LinWg* recs = (const LinWg*)host_table;
  for (int c0 = 0; c0 < count; c0 += LINWG_MAX) {
    const int n = std::min(LINWG_MAX, count - c0);
    LinWgArgs args;
    memset(&args, 0, sizeof(args));
    memcpy(args.rec, recs + c0, sizeof(LinWg) * n);
    hipLaunchKernelGGL(linear_wgrad_batched_args_kernel, dim3(max_tiles, n), dim3(256), 0, (hipStream_t)stream, args);
  }
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" int ast_linear_wgrad_batched(const void* table, int count, int max_tiles, void* stream) {
  if (!table || count <= 0 || max_tiles <= 0) AST_FAIL("ast_linear_wgrad_batched: bad args");
  hipLaunchKernelGGL(linear_wgrad_batched_kernel, dim3(max_tiles, count), dim3(256), 0, (hipStream_t)stream, (const LinWg*)table);
  AST_CHECK_LAUNCH();
  return 0;
}

// ---- <= 64 token rows ------------------------------------------------------------------------------------------------------------
extern "C" int ast_skinny_gemm_ex(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int ldw, int ldy,
                                  int relu, const float* mul_mask, float* drop_mask, float p, uint64_t seed, const int64_t* d_offset,
                                  void* stream) {
  return skinny_gemm_launch<1>("ast_skinny_gemm", x, w, bias, y, M, N, K, ldw, ldy, relu, mul_mask, drop_mask, p, seed, d_offset, stream);
}

extern "C" int ast_skinny_gemm(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int ldw, int ldy,
                               int relu, void* stream) {
  return skinny_gemm_launch<1>("ast_skinny_gemm", x, w, bias, y, M, N, K, ldw, ldy, relu, nullptr, nullptr, 0.f, 0, nullptr, stream);
}

extern "C" int ast_linear_wgrad(const float* dy, const float* x, float* dW, float* db, int M, int N, int K, int lddy, int ldw,
                                void* stream) {
  return linear_wgrad_launch<1>("ast_linear_wgrad", dy, x, dW, db, M, N, K, lddy, ldw, stream);
}

extern "C" int ast_bigk_gemm(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int ldy, void* stream) {
  return bigk_gemm_launch<1, false>("ast_bigk_gemm", x, w, bias, y, M, N, K, ldy, nullptr, 0, stream);
}

extern "C" long ast_bigk_gemm_det_ws_floats(int M, int N, int K) {
  if (!rows_ok<1>(M) || N < 1 || K < 2) return -1;
  return (long)((K + 1023) / 1024) * M * N;
}

extern "C" int ast_bigk_gemm_det(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, float* ws, long ws_floats,
                                 void* stream) {
  return bigk_gemm_launch<1, true>("ast_bigk_gemm_det", x, w, bias, y, M, N, K, N, ws, ws_floats, stream);
}

extern "C" int ast_bign_dgrad(const float* dy, const float* w, float* dx, int M, int N, int K, int lddy, void* stream) {
  return bign_dgrad_launch<1, false>("ast_bign_dgrad", dy, w, dx, M, N, K, lddy, nullptr, 0, stream);
}

extern "C" long ast_bign_dgrad_det_ws_floats(int M, int N, int K) {
  if (!rows_ok<1>(M) || N < 1 || K < 1 || K > 256) return -1;
  return (long)((N + 511) / 512) * M * K;
}

extern "C" int ast_bign_dgrad_det(const float* dy, const float* w, float* dx, int M, int N, int K, int lddy, float* ws, long ws_floats,
                                  void* stream) {
  return bign_dgrad_launch<1, true>("ast_bign_dgrad_det", dy, w, dx, M, N, K, lddy, ws, ws_floats, stream);
}

// ---- wide token path (include/ast_hip.h): 65 .. AST_WIDE_MAX_ROWS rows, 64 rows per workgroup ---------------------------------
extern "C" int ast_skinny_gemm_wide_ex(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int ldw, int ldy,
                                       int relu, const float* mul_mask, float* drop_mask, float p, uint64_t seed, const int64_t* d_offset,
                                       void* stream) {
  return skinny_gemm_launch<4>("ast_skinny_gemm_wide", x, w, bias, y, M, N, K, ldw, ldy, relu, mul_mask, drop_mask, p, seed, d_offset, stream);
}

extern "C" int ast_skinny_gemm_wide(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int ldw, int ldy,
                                    int relu, void* stream) {
  return skinny_gemm_launch<4>("ast_skinny_gemm_wide", x, w, bias, y, M, N, K, ldw, ldy, relu, nullptr, nullptr, 0.f, 0, nullptr, stream);
}

extern "C" int ast_linear_wgrad_wide(const float* dy, const float* x, float* dW, float* db, int M, int N, int K, int lddy, int ldw,
                                     void* stream) {
  return linear_wgrad_launch<4>("ast_linear_wgrad_wide", dy, x, dW, db, M, N, K, lddy, ldw, stream);
}

extern "C" int ast_bigk_gemm_wide(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int ldy, void* stream) {
  return bigk_gemm_launch<4, false>("ast_bigk_gemm_wide", x, w, bias, y, M, N, K, ldy, nullptr, 0, stream);
}

extern "C" long ast_bigk_gemm_wide_det_ws_floats(int M, int N, int K) {
  if (!rows_ok<4>(M) || N < 1 || K < 2 || (K & 1) || (K + 1023) / 1024 > 65535) return -1;
  return (long)((K + 1023) / 1024) * M * N;
}

extern "C" int ast_bigk_gemm_wide_det(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, float* ws,
                                      long ws_floats, void* stream) {
  return bigk_gemm_launch<4, true>("ast_bigk_gemm_wide_det", x, w, bias, y, M, N, K, N, ws, ws_floats, stream);
}

extern "C" int ast_bign_dgrad_wide(const float* dy, const float* w, float* dx, int M, int N, int K, int lddy, void* stream) {
  return bign_dgrad_launch<4, false>("ast_bign_dgrad_wide", dy, w, dx, M, N, K, lddy, nullptr, 0, stream);
}

extern "C" long ast_bign_dgrad_wide_det_ws_floats(int M, int N, int K) {
  if (!rows_ok<4>(M) || N < 1 || K < 1 || K > 256 || (N + 511) / 512 > AST_DET_MAX_SLOTS) return -1;
  return (long)((N + 511) / 512) * M * K;
}

extern "C" int ast_bign_dgrad_wide_det(const float* dy, const float* w, float* dx, int M, int N, int K, int lddy, float* ws,
                                       long ws_floats, void* stream) {
  return bign_dgrad_launch<4, true>("ast_bign_dgrad_wide_det", dy, w, dx, M, N, K, lddy, ws, ws_floats, stream);
}

// ---- embedding_to_stft at inference: any row count, per-clip section counts (include/ast_hip.h) ---------------------------------
extern "C" int ast_bign_gemm_len(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int ldw, int ldy, int S,
                                 const int32_t* n_valid, void* stream) {
  return bign_gemm_len_launch("ast_bign_gemm_len", x, w, bias, y, M, N, K, ldw, ldy, S, n_valid, stream);
}
