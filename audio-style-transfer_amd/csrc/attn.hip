// Attention core for 17 .. AST_ATTN_MAX_L tokens (f32): tiles of 16 queries x 16 keys on v_mfma_f32_16x16x4_f32 (exact f32).
// ast_attn_fwd_p / ast_attn_bwd_p (misc.hip) come here when Lq > 16 or Lk > 16; the <= 16-token kernels there are untouched.
// Same semantics as those: scale 1/sqrt(dh), causal masks j > i, probs (B,H,Lq,Lk) written BEFORE dropout, dropout from a
// mask tensor or drawn from (seed, counter, element index ((b*H+h)*Lq+i)*Lk+j), strided q / k / v / o rows.
//
// One wave per workgroup, no LDS.  Every score tile is computed TRANSPOSED, S^T = K Q^T (A operand = the 16 keys, B operand = the
// 16 queries), so that lane (i = l&15, g = l>>4) ends up with the four keys 4g .. 4g+3 of query i in its accumulator.  That is
// already the B-operand layout of the next product (k-slot g of step r <-> key 4g + r), with the other factor's rows
// 4g + r read as the A operand: P V, dS K, (P o M)^T dO and dS^T Q all follow a score tile without a transpose through LDS.
// Contractions over the head dimension load 16 B per lane (row l&15, columns 16 s + 4 g .. + 3) for both operands, the same
// k permutation on both sides as in skinny.hip.  NS = ceil(dh / 16) <= 4 is a template parameter; dh % 4 == 0.
//
// No atomics: a forward workgroup owns 16 query rows of o and probs; the backward is three launches,
//   attn_long_dot_kernel   (query tiles)  dot[i] = sum_j dP[i][j] P[i][j], parked in dq[row i][h*dh] (dq is written last),
//   attn_long_dkdv_kernel  (key tiles)    dk, dv: one wave sums over the query tiles in order,
//   attn_long_dq_kernel    (query tiles)  dq: reads its own rows' dot, then one wave sums over the key tiles in order,
// so every output element has one owner and a fixed summation order: the path is bit-reproducible as it stands.
// Rows past Lq / Lk and columns past dh are predicated: loaded as zero, never stored.
//
// ast_attn_fwd_len (inference with ragged batches) is forward only and has no dropout; the masked forward with dropout and
// the masked backward are ast_attn_fwd_len_p / ast_attn_bwd_len_p (the *_len_kernel templates below).  ast_attn_fwd_len runs the
// instantiations NS + ATTN_MASK of the forward kernel: key j of batch b counts iff (j % key_period) < key_len[b].  key_len is
// read from the device and clamped to [1, key_period], so key 0 stays valid, which is all the merge of the four lane groups
// needs (see there).  Masked K / V rows are treated like the rows past Lk: loaded as zero, scored -inf, probability 0; a key
// tile with no valid key is skipped.  Same template, same signature: `drop` carries key_len and `seed` carries key_period.
#include "ast_common.h"
#include "../../include/ast_hip.h"

namespace {

__device__ __forceinline__ f32x4 ld4(const float* p, bool ok) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  return ok ? *reinterpret_cast<const f32x4*>(p) : z;
}
// sum / max over the four lanes l&15, +16, +32, +48 (xor butterfly: every lane gets the same bits)
__device__ __forceinline__ float g4_sum(float v) { v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64); return v; }
__device__ __forceinline__ float g4_max(float v) { v = fmaxf(v, __shfl_xor(v, 16, 64)); v = fmaxf(v, __shfl_xor(v, 32, 64)); return v; }

// 16-row fragment of a (rows, ld) matrix for a contraction over the head dimension: row r0 + (l&15), columns 16 s + 4 g ..
template <int NS>
__device__ __forceinline__ void load_frag(f32x4 (&f)[NS], const float* base, int ld, int r0, int nrows, int dh, int i, int g,
                                          bool row_ok = true) {
  const bool rv = row_ok && r0 + i < nrows;
#pragma unroll
  for (int s = 0; s < NS; ++s) f[s] = ld4(base + (size_t)(rv ? r0 + i : 0) * ld + 16 * s + 4 * g, rv && 16 * s + 4 * g < dh);
}
// D[a-row 4g + r][b-row l&15] = sum_c A[a-row][c] B[b-row][c]
template <int NS>
__device__ __forceinline__ f32x4 dot_tile(const f32x4 (&a)[NS], const f32x4 (&b)[NS]) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][e], b[s][e], acc, 0, 0, 0);
  return acc;
}
// acc[t][.] += sum_r X[x0 + 4g + r][16 t + (l&15)] * w[r]  as A operand (X rows) x B operand (w: k-slot g of step r <-> row 4g + r).
// D: lane (column l&15 of w's tile, rows 16 t + 4 g + r') -> four consecutive head columns of one output row.
// rows_ok bit r: row x0 + 4g + r may be read (a masked row is loaded as zero).
template <int NS>
__device__ __forceinline__ void rows_mma(f32x4 (&acc)[NS], const float* xbase, int ld, int x0, int nrows, int dh, const f32x4& w,
                                         int i, int g, unsigned rows_ok = 15u) {
  float a[4][NS];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bool rv = (rows_ok >> r & 1u) && x0 + 4 * g + r < nrows;
#pragma unroll
    for (int t = 0; t < NS; ++t) a[r][t] = (rv && 16 * t + i < dh) ? xbase[(size_t)(x0 + 4 * g + r) * ld + 16 * t + i] : 0.f;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int t = 0; t < NS; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r][t], w[r], acc[t], 0, 0, 0);
}
template <int NS>
__device__ __forceinline__ void store_rows(const f32x4 (&acc)[NS], float* base, int ld, int row, bool rv, int dh, int g) {
#pragma unroll
  for (int t = 0; t < NS; ++t)
    if (rv && 16 * t + 4 * g < dh) *reinterpret_cast<f32x4*>(base + (size_t)row * ld + 16 * t + 4 * g) = acc[t];
}

struct Drop {
  const float* mask; float p, keep; uint64_t base;
  __device__ __forceinline__ float at(size_t idx) const { return mask ? mask[idx] : (p > 0.f ? dropout_keep(base, idx, p, keep) : 1.f); }
};
__device__ __forceinline__ Drop make_drop(const float* mask, float p, uint64_t seed, const int64_t* d_offset) {
  Drop d;
  d.mask = mask; d.p = p; d.keep = 1.f / (1.f - p);
  d.base = p > 0.f ? mix64(seed ^ mix64((uint64_t)(d_offset ? *d_offset : 0))) : 0;
  return d;
}

// grid (query tiles, B*H).  Pass 1: running maximum and sum of every query row, kept per lane over its own keys and merged
// across the four lane groups once; pass 2: scores again, probs written, P (after dropout) times V accumulated.
// The key mask of the NS + ATTN_MASK instantiations.  kl = the clamped key_len[b]; tile_live() is uniform over the workgroup
// (b is), so skipping a tile is a scalar branch.
constexpr int ATTN_MASK = 8;
struct KeyMask {
  int kl, period;
  __device__ __forceinline__ bool key(int j) const { return j % period < kl; }
  // does the tile of keys 16 kt .. 16 kt + 15 (< Lk) hold a valid key: its first key, or the start of the next period
  __device__ __forceinline__ bool tile_live(int kt, int Lk) const {
    const int a = (16 * kt) % period;
    return a < kl || 16 * kt + (period - a) < min(16 * kt + 16, Lk);
  }
};
template <int NSM>
__global__ __launch_bounds__(64) void attn_long_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                            const float* __restrict__ v, float* __restrict__ o, float* __restrict__ probs,
                                                            int H, int Lq, int Lk, int dh, int ldq, int ldk, int ldo, int causal,
                                                            const float* __restrict__ drop, float pdrop, uint64_t seed,
                                                            const int64_t* __restrict__ d_offset) {
  constexpr int NS = NSM & (ATTN_MASK - 1);
  constexpr bool MASK = NSM >= ATTN_MASK;
  const Drop dr = make_drop(MASK ? nullptr : drop, pdrop, seed, d_offset);
  const int b = blockIdx.y / H, h = blockIdx.y % H, q0 = blockIdx.x * 16;
  KeyMask km = {1, 1};
  if constexpr (MASK) {
    km.period = (int)seed;
    km.kl = min(max(reinterpret_cast<const int32_t*>(drop)[b], 1), km.period);
  }
  const int lane = threadIdx.x, i = lane & 15, g = lane >> 4;
  const float scale = rsqrtf((float)dh);
  const float* qb = q + (size_t)b * Lq * ldq + h * dh;
  const float* kb = k + (size_t)b * Lk * ldk + h * dh;
  const float* vb = v + (size_t)b * Lk * ldk + h * dh;
  const int nkt = (Lk + 15) / 16;
  const int kt_end = causal ? min(nkt, (q0 + 15) / 16 + 1) : nkt;      // key tiles past the diagonal are all masked
  const int qi = q0 + i;
  f32x4 qf[NS], kf[NS];
  load_frag<NS>(qf, qb, ldq, q0, Lq, dh, i, g);
#pragma unroll
  for (int s = 0; s < NS; ++s) qf[s] *= scale;

  float m = -INFINITY, l = 0.f;
  for (int kt = 0; kt < kt_end; ++kt) {
    if constexpr (MASK) { if (!km.tile_live(kt, Lk)) continue; }
    if constexpr (MASK) load_frag<NS>(kf, kb, ldk, kt * 16, Lk, dh, i, g, km.key(kt * 16 + i));
    else load_frag<NS>(kf, kb, ldk, kt * 16, Lk, dh, i, g);
    f32x4 s = dot_tile<NS>(kf, qf);
    float tm = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = kt * 16 + 4 * g + r;
      if (j >= Lk || (causal && j > qi)) s[r] = -INFINITY;
      if constexpr (MASK) { if (!km.key(j)) s[r] = -INFINITY; }
      tm = fmaxf(tm, s[r]);
    }
    const float mn = fmaxf(m, tm);
    const float mref = mn == -INFINITY ? 0.f : mn;                    // nothing unmasked yet for this lane: every term is 0
    l *= __expf(m - mref);
#pragma unroll
    for (int r = 0; r < 4; ++r) l += __expf(s[r] - mref);
    m = mn;
  }
  // key 0 is never masked, so the row maximum is finite (rows past Lq score 0 everywhere)
  // (MASK too: key_len >= 1.  A lane group that saw no valid key holds m = -inf, l = 0 and adds 0 * exp(-inf - M) = 0: M is
  // finite, so there is no inf - inf.)
  const float M = g4_max(m);
  const float den = g4_sum(l * __expf(m - M));

  f32x4 acc[NS];
#pragma unroll
  for (int t = 0; t < NS; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const size_t prow = (((size_t)b * H + h) * Lq + qi) * Lk;
  const bool qv = qi < Lq;
  for (int kt = 0; kt < nkt; ++kt) {
    f32x4 p = {0.f, 0.f, 0.f, 0.f};
    bool live = kt < kt_end;
    unsigned vok = 15u;                                                // MASK: bit r = V row 16 kt + 4 g + r may be read
    if constexpr (MASK) live = live && km.tile_live(kt, Lk);
    if (live) {
      if constexpr (MASK) load_frag<NS>(kf, kb, ldk, kt * 16, Lk, dh, i, g, km.key(kt * 16 + i));
      else load_frag<NS>(kf, kb, ldk, kt * 16, Lk, dh, i, g);
      const f32x4 s = dot_tile<NS>(kf, qf);
      if constexpr (MASK) vok = 0u;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = kt * 16 + 4 * g + r;
        p[r] = (j >= Lk || (causal && j > qi)) ? 0.f : __expf(s[r] - M) / den;
        if constexpr (MASK) { if (km.key(j)) vok |= 1u << r; else p[r] = 0.f; }
      }
    }
    f32x4 pd = p;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = kt * 16 + 4 * g + r;
      if (qv && j < Lk) {
        probs[prow + j] = p[r];
        pd[r] = p[r] * dr.at(prow + j);
      } else {
        pd[r] = 0.f;
      }
    }
    if constexpr (MASK) { if (live) rows_mma<NS>(acc, vb, ldk, kt * 16, Lk, dh, pd, i, g, vok); }
    else if (live) rows_mma<NS>(acc, vb, ldk, kt * 16, Lk, dh, pd, i, g);
  }
  store_rows<NS>(acc, o + (size_t)b * Lq * ldo + h * dh, ldo, qi, qv, dh, g);
}

// dP^T tile (lane: query q0 + (l&15), keys k0 + 4g + r) -> p, p * mask, dP * mask at the lane's four positions
// keys_ok bit r: key k0 + 4g + r counts (a masked key gets p = 0 and mask 0 without a read of probs or a draw)
template <int NS>
__device__ __forceinline__ void bwd_tile_t(const f32x4 (&vf)[NS], const f32x4 (&dof)[NS], const float* __restrict__ probs, const Drop& dr,
                                           size_t prow, bool qv, int k0, int Lk, int g, f32x4& p, f32x4& pm, f32x4& dpm,
                                           unsigned keys_ok = 15u) {
  const f32x4 dp = dot_tile<NS>(vf, dof);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = k0 + 4 * g + r;
    const bool ok = qv && j < Lk && (keys_ok >> r & 1u);
    const float mk = ok ? dr.at(prow + j) : 0.f;
    p[r] = ok ? probs[prow + j] : 0.f;
    pm[r] = p[r] * mk;
    dpm[r] = dp[r] * mk;
  }
}

// grid (query tiles, B*H): dot[i] = sum_j dP[i][j] P[i][j] -> dq[row i][h*dh], read back by the two kernels below
template <int NS>
__global__ __launch_bounds__(64) void attn_long_dot_kernel(const float* __restrict__ dout, const float* __restrict__ v,
                                                            const float* __restrict__ probs, float* __restrict__ dq, int H, int Lq, int Lk,
                                                            int dh, int ldq, int ldk, int ldo, const float* __restrict__ drop, float pdrop,
                                                            uint64_t seed, const int64_t* __restrict__ d_offset) {
  const Drop dr = make_drop(drop, pdrop, seed, d_offset);
  const int b = blockIdx.y / H, h = blockIdx.y % H, q0 = blockIdx.x * 16;
  const int lane = threadIdx.x, i = lane & 15, g = lane >> 4, qi = q0 + i;
  const float* vb = v + (size_t)b * Lk * ldk + h * dh;
  f32x4 dof[NS], vf[NS];
  load_frag<NS>(dof, dout + (size_t)b * Lq * ldo + h * dh, ldo, q0, Lq, dh, i, g);
  const size_t prow = (((size_t)b * H + h) * Lq + qi) * Lk;
  const bool qv = qi < Lq;
  float dot = 0.f;
  for (int k0 = 0; k0 < Lk; k0 += 16) {
    load_frag<NS>(vf, vb, ldk, k0, Lk, dh, i, g);
    f32x4 p, pm, dpm;
    bwd_tile_t<NS>(vf, dof, probs, dr, prow, qv, k0, Lk, g, p, pm, dpm);
#pragma unroll
    for (int r = 0; r < 4; ++r) dot += dpm[r] * p[r];
  }
  dot = g4_sum(dot);
  if (qv && g == 0) dq[((size_t)b * Lq + qi) * ldq + h * dh] = dot;
}

// grid (query tiles, B*H): dq[i][c] = sum_j dS[i][j] K[j][c], dS = P (dP - dot) / sqrt(dh)
template <int NS>
__global__ __launch_bounds__(64) void attn_long_dq_kernel(const float* __restrict__ dout, const float* __restrict__ k,
                                                           const float* __restrict__ v, const float* __restrict__ probs, float* dq, int H,
                                                           int Lq, int Lk, int dh, int ldq, int ldk, int ldo,
                                                           const float* __restrict__ drop, float pdrop, uint64_t seed,
                                                           const int64_t* __restrict__ d_offset) {
  const Drop dr = make_drop(drop, pdrop, seed, d_offset);
  const int b = blockIdx.y / H, h = blockIdx.y % H, q0 = blockIdx.x * 16;
  const int lane = threadIdx.x, i = lane & 15, g = lane >> 4, qi = q0 + i;
  const float scale = rsqrtf((float)dh);
  const float* kb = k + (size_t)b * Lk * ldk + h * dh;
  const float* vb = v + (size_t)b * Lk * ldk + h * dh;
  float* dqb = dq + (size_t)b * Lq * ldq + h * dh;
  const bool qv = qi < Lq;
  const float dot = qv ? dqb[(size_t)qi * ldq] : 0.f;                  // parked by attn_long_dot_kernel; overwritten below
  f32x4 dof[NS], vf[NS], acc[NS];
  load_frag<NS>(dof, dout + (size_t)b * Lq * ldo + h * dh, ldo, q0, Lq, dh, i, g);
#pragma unroll
  for (int t = 0; t < NS; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const size_t prow = (((size_t)b * H + h) * Lq + qi) * Lk;
  for (int k0 = 0; k0 < Lk; k0 += 16) {
    load_frag<NS>(vf, vb, ldk, k0, Lk, dh, i, g);
    f32x4 p, pm, dpm, ds;
    bwd_tile_t<NS>(vf, dof, probs, dr, prow, qv, k0, Lk, g, p, pm, dpm);
#pragma unroll
    for (int r = 0; r < 4; ++r) ds[r] = p[r] * (dpm[r] - dot) * scale;
    rows_mma<NS>(acc, kb, ldk, k0, Lk, dh, ds, i, g);
  }
  store_rows<NS>(acc, dqb, ldq, qi, qv, dh, g);
}

// grid (key tiles, B*H): dv[j][c] = sum_i (P o M)[i][j] dO[i][c], dk[j][c] = sum_i dS[i][j] Q[i][c].  Here the tile is
// dP = dO V^T untransposed (A operand = 16 queries, B operand = the 16 keys): lane (key k0 + (l&15), queries q0 + 4g + r).
template <int NS>
__global__ __launch_bounds__(64) void attn_long_dkdv_kernel(const float* __restrict__ dout, const float* __restrict__ q,
                                                             const float* __restrict__ v, const float* __restrict__ probs,
                                                             const float* dq, float* __restrict__ dk, float* __restrict__ dv, int H,
                                                             int Lq, int Lk, int dh, int ldq, int ldk, int ldo,
                                                             const float* __restrict__ drop, float pdrop, uint64_t seed,
                                                             const int64_t* __restrict__ d_offset) {
  const Drop dr = make_drop(drop, pdrop, seed, d_offset);
  const int b = blockIdx.y / H, h = blockIdx.y % H, k0 = blockIdx.x * 16;
  const int lane = threadIdx.x, i = lane & 15, g = lane >> 4, kj = k0 + i;
  const float scale = rsqrtf((float)dh);
  const float* qb = q + (size_t)b * Lq * ldq + h * dh;
  const float* dob = dout + (size_t)b * Lq * ldo + h * dh;
  const float* dotb = dq + (size_t)b * Lq * ldq + h * dh;
  const bool kv = kj < Lk;
  f32x4 vf[NS], dof[NS], akv[NS], avv[NS];
  load_frag<NS>(vf, v + (size_t)b * Lk * ldk + h * dh, ldk, k0, Lk, dh, i, g);
#pragma unroll
  for (int t = 0; t < NS; ++t) { akv[t] = f32x4{0.f, 0.f, 0.f, 0.f}; avv[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  for (int q0 = 0; q0 < Lq; q0 += 16) {
    load_frag<NS>(dof, dob, ldo, q0, Lq, dh, i, g);
    const f32x4 dp = dot_tile<NS>(dof, vf);
    f32x4 pm, ds;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qi = q0 + 4 * g + r;
      const bool ok = kv && qi < Lq;
      const size_t idx = (((size_t)b * H + h) * Lq + (ok ? qi : 0)) * Lk + (ok ? kj : 0);
      const float p = ok ? probs[idx] : 0.f;
      const float mk = ok ? dr.at(idx) : 0.f;
      const float dot = ok ? dotb[(size_t)qi * ldq] : 0.f;
      pm[r] = p * mk;
      ds[r] = p * (dp[r] * mk - dot) * scale;
    }
    rows_mma<NS>(avv, dob, ldo, q0, Lq, dh, pm, i, g);
    rows_mma<NS>(akv, qb, ldq, q0, Lq, dh, ds, i, g);
  }
  store_rows<NS>(akv, dk + (size_t)b * Lk * ldk + h * dh, ldk, kj, kv, dh, g);
  store_rows<NS>(avv, dv + (size_t)b * Lk * ldk + h * dh, ldk, kj, kv, dh, g);
}

// ---- the key-masked training kernels (ast_attn_fwd_len_p / ast_attn_bwd_len_p): mask AND dropout, so they take the mask as an
// argument of its own (AttnKeyLen) where the inference instantiations above borrow the dropout slots.  Kernels of their own
// rather than a body shared with the unmasked ones, so that those stay the code they were (tools/kernel_diff.py).  Per element
// they do the arithmetic of the unmasked kernels in the same order over the live keys; with full lengths they are bit-equal.
__device__ __forceinline__ KeyMask make_key_mask(const AttnKeyLen& kl, int b) {
  KeyMask km;
  km.period = kl.period;
  km.kl = min(max(kl.len[b], 1), kl.period);
  return km;
}
// bit r: key k0 + 4g + r counts
__device__ __forceinline__ unsigned keys_ok4(const KeyMask& km, int k0, int g) {
  unsigned ok = 0u;
#pragma unroll
  for (int r = 0; r < 4; ++r) ok |= (km.key(k0 + 4 * g + r) ? 1u : 0u) << r;
  return ok;
}

// attn_long_fwd_kernel<NS + ATTN_MASK> with dropout
template <int NS>
__global__ __launch_bounds__(64) void attn_long_fwd_len_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                const float* __restrict__ v, float* __restrict__ o,
                                                                float* __restrict__ probs, int H, int Lq, int Lk, int dh, int ldq, int ldk,
                                                                int ldo, int causal, AttnKeyLen klen, const float* __restrict__ drop,
                                                                float pdrop, uint64_t seed, const int64_t* __restrict__ d_offset) {
  const Drop dr = make_drop(drop, pdrop, seed, d_offset);
  const int b = blockIdx.y / H, h = blockIdx.y % H, q0 = blockIdx.x * 16;
  const KeyMask km = make_key_mask(klen, b);
  const int lane = threadIdx.x, i = lane & 15, g = lane >> 4;
  const float scale = rsqrtf((float)dh);
  const float* qb = q + (size_t)b * Lq * ldq + h * dh;
  const float* kb = k + (size_t)b * Lk * ldk + h * dh;
  const float* vb = v + (size_t)b * Lk * ldk + h * dh;
  const int nkt = (Lk + 15) / 16;
  const int kt_end = causal ? min(nkt, (q0 + 15) / 16 + 1) : nkt;
  const int qi = q0 + i;
  f32x4 qf[NS], kf[NS];
  load_frag<NS>(qf, qb, ldq, q0, Lq, dh, i, g);
#pragma unroll
  for (int s = 0; s < NS; ++s) qf[s] *= scale;

  float m = -INFINITY, l = 0.f;
  for (int kt = 0; kt < kt_end; ++kt) {
    if (!km.tile_live(kt, Lk)) continue;
    load_frag<NS>(kf, kb, ldk, kt * 16, Lk, dh, i, g, km.key(kt * 16 + i));
    f32x4 s = dot_tile<NS>(kf, qf);
    float tm = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = kt * 16 + 4 * g + r;
      if (j >= Lk || (causal && j > qi) || !km.key(j)) s[r] = -INFINITY;
      tm = fmaxf(tm, s[r]);
    }
    const float mn = fmaxf(m, tm);
    const float mref = mn == -INFINITY ? 0.f : mn;
    l *= __expf(m - mref);
#pragma unroll
    for (int r = 0; r < 4; ++r) l += __expf(s[r] - mref);
    m = mn;
  }
  const float M = g4_max(m);                                           // finite: key 0 is never masked (key_len >= 1)
  const float den = g4_sum(l * __expf(m - M));

  f32x4 acc[NS];
#pragma unroll
  for (int t = 0; t < NS; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const size_t prow = (((size_t)b * H + h) * Lq + qi) * Lk;
  const bool qv = qi < Lq;
  for (int kt = 0; kt < nkt; ++kt) {
    f32x4 p = {0.f, 0.f, 0.f, 0.f};
    const bool live = kt < kt_end && km.tile_live(kt, Lk);
    const unsigned vok = keys_ok4(km, kt * 16, g);
    if (live) {
      load_frag<NS>(kf, kb, ldk, kt * 16, Lk, dh, i, g, km.key(kt * 16 + i));
      const f32x4 s = dot_tile<NS>(kf, qf);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = kt * 16 + 4 * g + r;
        p[r] = (j >= Lk || (causal && j > qi) || !(vok >> r & 1u)) ? 0.f : __expf(s[r] - M) / den;
      }
    }
    f32x4 pd = p;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = kt * 16 + 4 * g + r;
      if (qv && j < Lk) {
        probs[prow + j] = p[r];                                        // a masked key, a skipped tile: exactly 0
        pd[r] = (vok >> r & 1u) ? p[r] * dr.at(prow + j) : 0.f;
      } else {
        pd[r] = 0.f;
      }
    }
    if (live) rows_mma<NS>(acc, vb, ldk, kt * 16, Lk, dh, pd, i, g, vok);
  }
  store_rows<NS>(acc, o + (size_t)b * Lq * ldo + h * dh, ldo, qi, qv, dh, g);
}

// attn_long_dot_kernel under the mask: a key tile with no live key adds nothing and is skipped; a masked V row is not read
template <int NS>
__global__ __launch_bounds__(64) void attn_long_dot_len_kernel(const float* __restrict__ dout, const float* __restrict__ v,
                                                                const float* __restrict__ probs, float* __restrict__ dq, int H, int Lq,
                                                                int Lk, int dh, int ldq, int ldk, int ldo, AttnKeyLen klen,
                                                                const float* __restrict__ drop, float pdrop, uint64_t seed,
                                                                const int64_t* __restrict__ d_offset) {
  const Drop dr = make_drop(drop, pdrop, seed, d_offset);
  const int b = blockIdx.y / H, h = blockIdx.y % H, q0 = blockIdx.x * 16;
  const KeyMask km = make_key_mask(klen, b);
  const int lane = threadIdx.x, i = lane & 15, g = lane >> 4, qi = q0 + i;
  const float* vb = v + (size_t)b * Lk * ldk + h * dh;
  f32x4 dof[NS], vf[NS];
  load_frag<NS>(dof, dout + (size_t)b * Lq * ldo + h * dh, ldo, q0, Lq, dh, i, g);
  const size_t prow = (((size_t)b * H + h) * Lq + qi) * Lk;
  const bool qv = qi < Lq;
  float dot = 0.f;
  for (int k0 = 0; k0 < Lk; k0 += 16) {
    if (!km.tile_live(k0 / 16, Lk)) continue;
    load_frag<NS>(vf, vb, ldk, k0, Lk, dh, i, g, km.key(k0 + i));
    f32x4 p, pm, dpm;
    bwd_tile_t<NS>(vf, dof, probs, dr, prow, qv, k0, Lk, g, p, pm, dpm, keys_ok4(km, k0, g));
#pragma unroll
    for (int r = 0; r < 4; ++r) dot += dpm[r] * p[r];
  }
  dot = g4_sum(dot);
  if (qv && g == 0) dq[((size_t)b * Lq + qi) * ldq + h * dh] = dot;
}

// attn_long_dq_kernel under the mask: dS of a masked key is 0 and its K and V rows are not read; dead tiles are skipped
template <int NS>
__global__ __launch_bounds__(64) void attn_long_dq_len_kernel(const float* __restrict__ dout, const float* __restrict__ k,
                                                               const float* __restrict__ v, const float* __restrict__ probs, float* dq,
                                                               int H, int Lq, int Lk, int dh, int ldq, int ldk, int ldo, AttnKeyLen klen,
                                                               const float* __restrict__ drop, float pdrop, uint64_t seed,
                                                               const int64_t* __restrict__ d_offset) {
  const Drop dr = make_drop(drop, pdrop, seed, d_offset);
  const int b = blockIdx.y / H, h = blockIdx.y % H, q0 = blockIdx.x * 16;
  const KeyMask km = make_key_mask(klen, b);
  const int lane = threadIdx.x, i = lane & 15, g = lane >> 4, qi = q0 + i;
  const float scale = rsqrtf((float)dh);
  const float* kb = k + (size_t)b * Lk * ldk + h * dh;
  const float* vb = v + (size_t)b * Lk * ldk + h * dh;
  float* dqb = dq + (size_t)b * Lq * ldq + h * dh;
  const bool qv = qi < Lq;
  const float dot = qv ? dqb[(size_t)qi * ldq] : 0.f;                  // parked by attn_long_dot_len_kernel; overwritten below
  f32x4 dof[NS], vf[NS], acc[NS];
  load_frag<NS>(dof, dout + (size_t)b * Lq * ldo + h * dh, ldo, q0, Lq, dh, i, g);
#pragma unroll
  for (int t = 0; t < NS; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const size_t prow = (((size_t)b * H + h) * Lq + qi) * Lk;
  for (int k0 = 0; k0 < Lk; k0 += 16) {
    if (!km.tile_live(k0 / 16, Lk)) continue;
    const unsigned kok = keys_ok4(km, k0, g);
    load_frag<NS>(vf, vb, ldk, k0, Lk, dh, i, g, km.key(k0 + i));
    f32x4 p, pm, dpm, ds;
    bwd_tile_t<NS>(vf, dof, probs, dr, prow, qv, k0, Lk, g, p, pm, dpm, kok);
#pragma unroll
    for (int r = 0; r < 4; ++r) ds[r] = p[r] * (dpm[r] - dot) * scale;
    rows_mma<NS>(acc, kb, ldk, k0, Lk, dh, ds, i, g, kok);
  }
  store_rows<NS>(acc, dqb, ldq, qi, qv, dh, g);
}

// attn_long_dkdv_kernel under the mask.  A workgroup whose key tile has no live key stores its zeros and leaves before the query
// loop (uniform: b is).  In a live tile a masked key's V row is not read, its lane takes p = 0 and mask 0 without a read, and its
// dk / dv rows are stored as literal zeros, whatever dout holds.
template <int NS>
__global__ __launch_bounds__(64) void attn_long_dkdv_len_kernel(const float* __restrict__ dout, const float* __restrict__ q,
                                                                 const float* __restrict__ v, const float* __restrict__ probs,
                                                                 const float* dq, float* __restrict__ dk, float* __restrict__ dv, int H,
                                                                 int Lq, int Lk, int dh, int ldq, int ldk, int ldo, AttnKeyLen klen,
                                                                 const float* __restrict__ drop, float pdrop, uint64_t seed,
                                                                 const int64_t* __restrict__ d_offset) {
  const Drop dr = make_drop(drop, pdrop, seed, d_offset);
  const int b = blockIdx.y / H, h = blockIdx.y % H, k0 = blockIdx.x * 16;
  const KeyMask km = make_key_mask(klen, b);
  const int lane = threadIdx.x, i = lane & 15, g = lane >> 4, kj = k0 + i;
  const float scale = rsqrtf((float)dh);
  const float* qb = q + (size_t)b * Lq * ldq + h * dh;
  const float* dob = dout + (size_t)b * Lq * ldo + h * dh;
  const float* dotb = dq + (size_t)b * Lq * ldq + h * dh;
  float* dkb = dk + (size_t)b * Lk * ldk + h * dh;
  float* dvb = dv + (size_t)b * Lk * ldk + h * dh;
  const bool kv = kj < Lk;
  const bool klive = kv && km.key(kj);
  f32x4 vf[NS], dof[NS], akv[NS], avv[NS];
#pragma unroll
  for (int t = 0; t < NS; ++t) { akv[t] = f32x4{0.f, 0.f, 0.f, 0.f}; avv[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  if (!km.tile_live(blockIdx.x, Lk)) {
    store_rows<NS>(akv, dkb, ldk, kj, kv, dh, g);
    store_rows<NS>(avv, dvb, ldk, kj, kv, dh, g);
    return;
  }
  load_frag<NS>(vf, v + (size_t)b * Lk * ldk + h * dh, ldk, k0, Lk, dh, i, g, klive);
  for (int q0 = 0; q0 < Lq; q0 += 16) {
    load_frag<NS>(dof, dob, ldo, q0, Lq, dh, i, g);
    const f32x4 dp = dot_tile<NS>(dof, vf);
    f32x4 pm, ds;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qi = q0 + 4 * g + r;
      const bool ok = klive && qi < Lq;
      const size_t idx = (((size_t)b * H + h) * Lq + (ok ? qi : 0)) * Lk + (ok ? kj : 0);
      const float p = ok ? probs[idx] : 0.f;
      const float mk = ok ? dr.at(idx) : 0.f;
      const float dot = ok ? dotb[(size_t)qi * ldq] : 0.f;
      pm[r] = p * mk;
      ds[r] = p * (dp[r] * mk - dot) * scale;
    }
    rows_mma<NS>(avv, dob, ldo, q0, Lq, dh, pm, i, g);
    rows_mma<NS>(akv, qb, ldq, q0, Lq, dh, ds, i, g);
  }
  if (!klive) {                                                        // 0 * dout is not 0 for a dout that is not finite
#pragma unroll
    for (int t = 0; t < NS; ++t) { akv[t] = f32x4{0.f, 0.f, 0.f, 0.f}; avv[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  }
  store_rows<NS>(akv, dkb, ldk, kj, kv, dh, g);
  store_rows<NS>(avv, dvb, ldk, kj, kv, dh, g);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

#define AST_ATTN_NS(dh, ...)                          \
  do {                                                \
    switch (((dh) + 15) / 16) {                       \
      case 1: { constexpr int NS = 1; __VA_ARGS__; } break; \
      case 2: { constexpr int NS = 2; __VA_ARGS__; } break; \
      case 3: { constexpr int NS = 3; __VA_ARGS__; } break; \
      default: { constexpr int NS = 4; __VA_ARGS__; } break; \
    }                                                 \
  } while (0)

// The argument checks of the long path; the callers have checked the pointers for null and 1 <= L, 1 <= dh <= 64.
int attn_long_check(const char* who, int B, int H, int Lq, int Lk, int dh, int ldq, int ldk, int ldo, const void* const* ptrs,
                        int nptrs) {
  if (Lq > AST_ATTN_MAX_L || Lk > AST_ATTN_MAX_L)
    AST_FAIL("%s: at most AST_ATTN_MAX_L = %d tokens (Lq=%d Lk=%d)", who, AST_ATTN_MAX_L, Lq, Lk);
  if (dh % 4 != 0) AST_FAIL("%s: more than 16 tokens need dh %% 4 == 0 (dh=%d Lq=%d Lk=%d)", who, dh, Lq, Lk);
  if (B < 1 || H < 1 || (long)B * H > 65535) AST_FAIL("%s: needs 1 <= B*H <= 65535 (B=%d H=%d)", who, B, H);
  if (ldq < H * dh || ldk < H * dh || ldo < H * dh || ldq % 4 != 0 || ldk % 4 != 0 || ldo % 4 != 0)
    AST_FAIL("%s: more than 16 tokens need row strides >= H*dh and a multiple of 4 floats (ldq=%d ldk=%d ldo=%d)", who, ldq, ldk, ldo);
  for (int n = 0; n < nptrs; ++n)
    if (!aligned16(ptrs[n])) AST_FAIL("%s: more than 16 tokens need 16-byte aligned q, k, v, o and gradients", who);
  return 0;
}

int attn_long_fwd_launch(const float* q, const float* k, const float* v, float* o, float* probs, int B, int H, int Lq, int Lk, int dh,
                      int ldq, int ldk, int ldo, int causal, const float* drop_mask, float p, uint64_t seed, const int64_t* d_offset,
                      void* stream) {
  const void* ptrs[] = {q, k, v, o};
  if (int rc = attn_long_check("ast_attn_fwd", B, H, Lq, Lk, dh, ldq, ldk, ldo, ptrs, 4)) return rc;
  const dim3 grid((Lq + 15) / 16, B * H);
  AST_ATTN_NS(dh, hipLaunchKernelGGL(attn_long_fwd_kernel<NS>, grid, dim3(64), 0, (hipStream_t)stream, q, k, v, o, probs, H, Lq, Lk, dh,
                                     ldq, ldk, ldo, causal, drop_mask, p, seed, d_offset));
  AST_CHECK_LAUNCH();
  return 0;
}

int attn_long_fwd_len_launch(const float* q, const float* k, const float* v, float* o, float* probs, int B, int H, int Lq, int Lk, int dh,
                             int ldq, int ldk, int ldo, int causal, const int32_t* key_len, int key_period, void* stream) {
  const void* ptrs[] = {q, k, v, o};
  if (int rc = attn_long_check("ast_attn_fwd_len", B, H, Lq, Lk, dh, ldq, ldk, ldo, ptrs, 4)) return rc;
  const dim3 grid((Lq + 15) / 16, B * H);
  // key_len in the `drop` slot, key_period in the `seed` slot (see attn_long_fwd_kernel)
  AST_ATTN_NS(dh, hipLaunchKernelGGL(attn_long_fwd_kernel<NS + ATTN_MASK>, grid, dim3(64), 0, (hipStream_t)stream, q, k, v, o, probs, H,
                                     Lq, Lk, dh, ldq, ldk, ldo, causal, reinterpret_cast<const float*>(key_len), 0.f,
                                     (uint64_t)key_period, (const int64_t*)nullptr));
  AST_CHECK_LAUNCH();
  return 0;
}

int attn_long_bwd_launch(const float* dout, const float* q, const float* k, const float* v, const float* probs, float* dq, float* dk,
                      float* dv, int B, int H, int Lq, int Lk, int dh, int ldq, int ldk, int ldo, const float* drop_mask, float p,
                      uint64_t seed, const int64_t* d_offset, void* stream) {
  const void* ptrs[] = {dout, q, k, v, dq, dk, dv};
  if (int rc = attn_long_check("ast_attn_bwd", B, H, Lq, Lk, dh, ldq, ldk, ldo, ptrs, 7)) return rc;
  const dim3 qgrid((Lq + 15) / 16, B * H), kgrid((Lk + 15) / 16, B * H);
  hipStream_t st = (hipStream_t)stream;
  AST_ATTN_NS(dh, hipLaunchKernelGGL(attn_long_dot_kernel<NS>, qgrid, dim3(64), 0, st, dout, v, probs, dq, H, Lq, Lk, dh, ldq, ldk, ldo,
                                     drop_mask, p, seed, d_offset));
  AST_CHECK_LAUNCH();
  AST_ATTN_NS(dh, hipLaunchKernelGGL(attn_long_dkdv_kernel<NS>, kgrid, dim3(64), 0, st, dout, q, v, probs, (const float*)dq, dk, dv, H,
                                     Lq, Lk, dh, ldq, ldk, ldo, drop_mask, p, seed, d_offset));
  AST_CHECK_LAUNCH();
  AST_ATTN_NS(dh, hipLaunchKernelGGL(attn_long_dq_kernel<NS>, qgrid, dim3(64), 0, st, dout, k, v, probs, dq, H, Lq, Lk, dh, ldq, ldk,
                                     ldo, drop_mask, p, seed, d_offset));
  AST_CHECK_LAUNCH();
  return 0;
}

int attn_long_fwd_len_p_launch(const float* q, const float* k, const float* v, float* o, float* probs, int B, int H, int Lq, int Lk,
                               int dh, int ldq, int ldk, int ldo, int causal, AttnKeyLen kl, const float* drop_mask, float p,
                               uint64_t seed, const int64_t* d_offset, void* stream) {
  const void* ptrs[] = {q, k, v, o};
  if (int rc = attn_long_check("ast_attn_fwd_len_p", B, H, Lq, Lk, dh, ldq, ldk, ldo, ptrs, 4)) return rc;
  const dim3 grid((Lq + 15) / 16, B * H);
  AST_ATTN_NS(dh, hipLaunchKernelGGL(attn_long_fwd_len_kernel<NS>, grid, dim3(64), 0, (hipStream_t)stream, q, k, v, o, probs, H, Lq, Lk,
                                     dh, ldq, ldk, ldo, causal, kl, drop_mask, p, seed, d_offset));
  AST_CHECK_LAUNCH();
  return 0;
}

int attn_long_bwd_len_p_launch(const float* dout, const float* q, const float* k, const float* v, const float* probs, float* dq,
                               float* dk, float* dv, int B, int H, int Lq, int Lk, int dh, int ldq, int ldk, int ldo, AttnKeyLen kl,
                               const float* drop_mask, float p, uint64_t seed, const int64_t* d_offset, void* stream) {
  const void* ptrs[] = {dout, q, k, v, dq, dk, dv};
  if (int rc = attn_long_check("ast_attn_bwd_len_p", B, H, Lq, Lk, dh, ldq, ldk, ldo, ptrs, 7)) return rc;
  const dim3 qgrid((Lq + 15) / 16, B * H), kgrid((Lk + 15) / 16, B * H);
  hipStream_t st = (hipStream_t)stream;
  AST_ATTN_NS(dh, hipLaunchKernelGGL(attn_long_dot_len_kernel<NS>, qgrid, dim3(64), 0, st, dout, v, probs, dq, H, Lq, Lk, dh, ldq, ldk,
                                     ldo, kl, drop_mask, p, seed, d_offset));
  AST_CHECK_LAUNCH();
  AST_ATTN_NS(dh, hipLaunchKernelGGL(attn_long_dkdv_len_kernel<NS>, kgrid, dim3(64), 0, st, dout, q, v, probs, (const float*)dq, dk, dv,
                                     H, Lq, Lk, dh, ldq, ldk, ldo, kl, drop_mask, p, seed, d_offset));
  AST_CHECK_LAUNCH();
  AST_ATTN_NS(dh, hipLaunchKernelGGL(attn_long_dq_len_kernel<NS>, qgrid, dim3(64), 0, st, dout, k, v, probs, dq, H, Lq, Lk, dh, ldq,
                                     ldk, ldo, kl, drop_mask, p, seed, d_offset));
  AST_CHECK_LAUNCH();
  return 0;
}
