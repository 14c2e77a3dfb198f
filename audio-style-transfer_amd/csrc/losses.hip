// Loss kernels: the fused complex-spectrogram reconstruction loss (one streaming
// pass, value + gradient) and the batch-coupled embedding losses of losses.py as
// single-workgroup wavefront-reduction kernels (B <= 64 rows of 256 floats).
#include "ast_common.h"
#include "../../include/ast_hip.h"

namespace {

constexpr float PI_F = 3.14159265358979323846f;

// ---- compute_comprehensive_loss (new_decoder.py:348-420) ---------------------------
// thread = one (b, t, f) complex bin, loops over the S sections so the section
// differences stay in registers; t+-1 neighbours come from L1/L2.
// DET (deterministic mode): workgroup b STORES its five partial sums into sums[b * 5 ..] (one slot per workgroup) instead of adding
// them into slot b % nslots with atomics.
template <bool DET = false>
__global__ __launch_bounds__(1024) void recon_loss_kernel(const float* __restrict__ out, const float* __restrict__ tgt, int64_t tld,
                                                          int B, int S, int T, int Fq, float c_mse, float c_mag, float c_ph,
                                                          float c_tmp, float c_spc, float* __restrict__ sums, float* __restrict__ grad, int nslots) {
  __shared__ float red[17];
  const unsigned total = (unsigned)B * T * Fq;                  // < 2^31 (host check): 32-bit index math, no 64-bit divisions
  const size_t plane_o = (size_t)T * Fq, plane_t = (size_t)T * tld;
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int f = (int)(i % (unsigned)Fq);
    const unsigned r = i / (unsigned)Fq;
    const int t = (int)(r % (unsigned)T);
    const int b = (int)(r / (unsigned)T);
    float eprev[2] = {0.f, 0.f};     // e[s-1] at (t,f)
    for (int s = 0; s < S; ++s) {
      const size_t sec = (size_t)b * S + s;
      float o[2], g[2], e[2], eup[2], edn[2], enext[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float* po = out + (sec * 2 + c) * plane_o + (size_t)t * Fq + f;
        const float* pt = tgt + (sec * 2 + c) * plane_t + (size_t)t * tld + f;
        o[c] = po[0]; g[c] = pt[0]; e[c] = o[c] - g[c];
        eup[c] = t > 0 ? po[-(long)Fq] - pt[-tld] : 0.f;
        edn[c] = t + 1 < T ? po[Fq] - pt[tld] : 0.f;
        enext[c] = s + 1 < S ? po[2 * plane_o] - pt[2 * plane_t] : 0.f;
      }
      const float mo2 = o[0] * o[0] + o[1] * o[1], mt2 = g[0] * g[0] + g[1] * g[1];
      const float mo = sqrtf(mo2 + 1e-8f), mt = sqrtf(mt2 + 1e-8f);
      float dphi = atan2f(o[1], o[0]) - atan2f(g[1], g[0]);
      dphi = dphi + PI_F;
      dphi = dphi - 2.f * PI_F * floorf(dphi / (2.f * PI_F)) - PI_F;      // torch.remainder(., 2pi) - pi
      acc[0] += e[0] * e[0] + e[1] * e[1];
      acc[1] += (mo - mt) * (mo - mt);
      acc[2] += dphi * dphi;
      float gt[2] = {0.f, 0.f}, gs[2] = {0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        if (s + 1 < S) { const float d = enext[c] - e[c]; acc[3] += d * d; gt[c] -= d; }
        if (s > 0) gt[c] += e[c] - eprev[c];
        if (t + 1 < T) { const float d = edn[c] - e[c]; acc[4] += d * d; gs[c] -= d; }
        if (t > 0) gs[c] += e[c] - eup[c];
      }
      if (grad) {
        const float inv2 = 1.f / mo2;   // atan2 backward: (-im, re) / (re^2 + im^2)
        const float gph[2] = {-o[1] * inv2, o[0] * inv2};
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          grad[(sec * 2 + c) * plane_o + (size_t)t * Fq + f] =
              2.f * (c_mse * e[c] + c_mag * (mo - mt) * o[c] / mo + c_ph * dphi * gph[c] + c_tmp * gt[c] + c_spc * gs[c]);
        }
      }
      eprev[0] = e[0]; eprev[1] = e[1];
    }
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const float v = block_sum(acc[k], red);
    if constexpr (DET) {
      if (threadIdx.x == 0) sums[(size_t)blockIdx.x * 5 + k] = v;
    } else {
      if (threadIdx.x == 0) unsafeAtomicAdd(sums + (blockIdx.x % nslots) * 5 + k, v);      // nslots rows of 5: few adders per address
    }
  }
}

// sums[k] = sum over the slots (fixed order), total = sum_k c[k] * sums[k], parts[k] = inv[k] * sums[k]: out = [5 sums][total][5 parts]
struct ReconFin { float c[5], inv[5]; };
__global__ __launch_bounds__(64) void recon_finish_kernel(const float* __restrict__ ws, int nslots, ReconFin a, float* __restrict__ out) {
  __shared__ float sk[5];
  const int k = threadIdx.x;
  if (k < 5) {
    float v = 0.f;
    for (int i = 0; i < nslots; ++i) v += ws[i * 5 + k];
    sk[k] = v;
    out[k] = v;
    out[6 + k] = v * a.inv[k];
  }
  __syncthreads();
  if (k == 0) out[5] = (((a.c[0] * sk[0] + a.c[1] * sk[1]) + a.c[2] * sk[2]) + a.c[3] * sk[3]) + a.c[4] * sk[4];
}

// deterministic finish over thousands of slots: wave k reduces quantity k, lane l the slots l, l + 64, ... in order, then the
// fixed butterfly of wave_sum -- the same order on every run
__global__ __launch_bounds__(320) void recon_finish_det_kernel(const float* __restrict__ ws, int nslots, ReconFin a, float* __restrict__ out) {
  __shared__ float sk[5];
  const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float v = 0.f;
  for (int i = lane; i < nslots; i += 64) v += ws[(size_t)i * 5 + k];
  v = wave_sum(v);
  if (lane == 0) { sk[k] = v; out[k] = v; out[6 + k] = v * a.inv[k]; }
  __syncthreads();
  if (threadIdx.x == 0) out[5] = (((a.c[0] * sk[0] + a.c[1] * sk[1]) + a.c[2] * sk[2]) + a.c[3] * sk[3]) + a.c[4] * sk[4];
}

// ---- compute_comprehensive_loss per clip of a zero-padded batch (values only) --------
// Row b is the loss of clip b alone over its own n_b = clamp(n_sections[b], 1, S) sections.  grid (workgroups per clip, B):
// a workgroup belongs to ONE clip, thread = one (t, f) bin of it, looping over the clip's n_b sections with the section
// difference in registers; sections s >= n_b are never loaded, the last real section has no successor.  Values only, so the
// t - 1 neighbour and e[s-1] of recon_loss_kernel (gradient terms) are not read.  Every workgroup STORES its five partial sums
// into its own slot part[(b * gridDim.x + blockIdx.x) * 5 ..]: no atomics, nothing to zero.
constexpr int RLEN_THREADS = 256;
constexpr int RLEN_MAX_BLOCKS = 4096;           // workgroups per clip; past 4096 * 256 bins a thread strides over several

__device__ __forceinline__ int clip_sections(const int32_t* __restrict__ n_sections, int b, int S) {
  return n_sections ? min(max(n_sections[b], 1), S) : S;
}

__global__ __launch_bounds__(RLEN_THREADS) void recon_len_kernel(const float* __restrict__ out, const float* __restrict__ tgt, int64_t tld,
                                                                  int S, int T, int Fq, const int32_t* __restrict__ n_sections,
                                                                  float* __restrict__ part) {
  __shared__ float red[17];
  const int b = blockIdx.y;
  const int nb = clip_sections(n_sections, b, S);
  const unsigned bins = (unsigned)T * Fq;                       // < 2^31 (host check)
  const size_t plane_o = (size_t)T * Fq, plane_t = (size_t)T * tld;
  const float* ob = out + (size_t)b * S * 2 * plane_o;
  const float* tb = tgt + (size_t)b * S * 2 * plane_t;
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (unsigned i = blockIdx.x * RLEN_THREADS + threadIdx.x; i < bins; i += gridDim.x * RLEN_THREADS) {
    const int f = (int)(i % (unsigned)Fq), t = (int)(i / (unsigned)Fq);
    const bool down = t + 1 < T;
    const float* po = ob + (size_t)t * Fq + f;
    const float* pt = tb + (size_t)t * tld + f;
    float o[2] = {po[0], po[plane_o]}, g[2] = {pt[0], pt[plane_t]};
    for (int s = 0; s < nb; ++s) {
      const bool more = s + 1 < nb;                             // the last REAL section has no successor, whatever lies behind it
      float e[2], edn[2] = {0.f, 0.f}, on[2] = {0.f, 0.f}, gn[2] = {0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float* qo = po + (size_t)(2 * s + c) * plane_o;
        const float* qt = pt + (size_t)(2 * s + c) * plane_t;
        e[c] = o[c] - g[c];
        if (down) edn[c] = qo[Fq] - qt[tld];
        if (more) { on[c] = qo[2 * plane_o]; gn[c] = qt[2 * plane_t]; }
      }
      const float mo = sqrtf(o[0] * o[0] + o[1] * o[1] + 1e-8f), mt = sqrtf(g[0] * g[0] + g[1] * g[1] + 1e-8f);
      float dphi = atan2f(o[1], o[0]) - atan2f(g[1], g[0]);
      dphi = dphi + PI_F;
      dphi = dphi - 2.f * PI_F * floorf(dphi / (2.f * PI_F)) - PI_F;      // torch.remainder(., 2pi) - pi
      acc[0] += e[0] * e[0] + e[1] * e[1];
      acc[1] += (mo - mt) * (mo - mt);
      acc[2] += dphi * dphi;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        if (more) { const float d = (on[c] - gn[c]) - e[c]; acc[3] += d * d; }
        if (down) { const float d = edn[c] - e[c]; acc[4] += d * d; }
        o[c] = on[c]; g[c] = gn[c];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const float v = block_sum(acc[k], red);
    if (threadIdx.x == 0) part[((size_t)b * gridDim.x + blockIdx.x) * 5 + k] = v;
  }
}

// One workgroup per clip, the order of recon_finish_det_kernel: wave k sums quantity k, lane l the slots l, l + 64, ... in order,
// then wave_sum's fixed butterfly.  The counts of new_decoder.py:402-418 for the clip alone and their reciprocals are formed here
// from n_sections (no host read); a term without elements (temporal at n_b == 1, axis-3 difference at T == 1) has sum, mean and
// coefficient exactly 0.  res (B, 11) = [5 sums][total = sum_k (w[k] / count_k) * sums[k]][5 means = sums[k] / count_k].
struct ReconLenW { float w[5]; };
__global__ __launch_bounds__(320) void recon_len_finish_kernel(const float* __restrict__ part, int nslots, int S, int T, int Fq,
                                                                const int32_t* __restrict__ n_sections, ReconLenW a,
                                                                float* __restrict__ res) {
  __shared__ float sk[5];
  const int b = blockIdx.x, k = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* ws = part + (size_t)b * nslots * 5;
  float* out = res + (size_t)b * 11;
  const long long nb = clip_sections(n_sections, b, S);
  const long long bins = (long long)T * Fq;
  const long long count = k == 0 ? 2 * nb * bins : k == 3 ? 2 * (nb - 1) * bins : k == 4 ? 2 * nb * (long long)(T - 1) * Fq : nb * bins;
  float v = 0.f;
  for (int i = lane; i < nslots; i += 64) v += ws[(size_t)i * 5 + k];
  v = wave_sum(v);
  if (lane == 0) {
    out[k] = v;
    out[6 + k] = count > 0 ? v * (float)(1.0 / (double)count) : 0.f;
    sk[k] = count > 0 ? (float)((double)a.w[k] / (double)count) * v : 0.f;
  }
  __syncthreads();
  if (threadIdx.x == 0) out[5] = (((sk[0] + sk[1]) + sk[2]) + sk[3]) + sk[4];
}

// ---- the same per clip WITH the gradient: loss = sum_b w_b total_b and d loss / d out in one pass ----------------------------------
// recon_len_kernel's shape (grid (workgroups per clip, B), thread = one (t, f) bin walking the clip's n_b sections, the next
// section's values carried in registers) plus what the gradient needs: e[s-1] kept in registers and the t - 1 neighbour loaded, as
// recon_loss_kernel does.  The five coefficients cf[k] = w_b * (weight_k / count_k(n_b)) are formed once per workgroup from
// n_sections with recon_len_finish_kernel's counts; a term without elements has coefficient exactly 0 (and its differences are
// never formed), so it contributes gradient exactly 0.  Sections s >= n_b are never loaded; their gradient rows are stored as
// exactly 0 (grad arrives uninitialised).  The value side is recon_len_kernel's, sum for sum: the same slots, the same finish.
__global__ __launch_bounds__(RLEN_THREADS) void recon_len_grad_kernel(const float* __restrict__ out, const float* __restrict__ tgt, int64_t tld,
                                                                       int B, int S, int T, int Fq, const int32_t* __restrict__ n_sections,
                                                                       const float* __restrict__ clip_weights, ReconLenW a,
                                                                       float* __restrict__ part, float* __restrict__ grad) {
  __shared__ float red[17];
  __shared__ float cfs[5];
  const int b = blockIdx.y;
  const int nb = clip_sections(n_sections, b, S);
  const unsigned bins = (unsigned)T * Fq;                       // < 2^31 (host check)
  if (threadIdx.x < 5) {
    const int k = threadIdx.x;
    const long long n = nb, tf = (long long)T * Fq;
    const long long count = k == 0 ? 2 * n * tf : k == 3 ? 2 * (n - 1) * tf : k == 4 ? 2 * n * (long long)(T - 1) * Fq : n * tf;
    const float wb = clip_weights ? clip_weights[b] : 1.f / (float)B;
    cfs[k] = count > 0 ? wb * (float)((double)a.w[k] / (double)count) : 0.f;
  }
  __syncthreads();
  const float c_mse = cfs[0], c_mag = cfs[1], c_ph = cfs[2], c_tmp = cfs[3], c_spc = cfs[4];
  const size_t plane_o = (size_t)T * Fq, plane_t = (size_t)T * tld;
  const float* ob = out + (size_t)b * S * 2 * plane_o;
  const float* tb = tgt + (size_t)b * S * 2 * plane_t;
  float* gb = grad + (size_t)b * S * 2 * plane_o;
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (unsigned i = blockIdx.x * RLEN_THREADS + threadIdx.x; i < bins; i += gridDim.x * RLEN_THREADS) {
    const int f = (int)(i % (unsigned)Fq), t = (int)(i / (unsigned)Fq);
    const bool down = t + 1 < T, up = t > 0;
    const float* po = ob + (size_t)t * Fq + f;
    const float* pt = tb + (size_t)t * tld + f;
    float* pg = gb + (size_t)t * Fq + f;
    float o[2] = {po[0], po[plane_o]}, g[2] = {pt[0], pt[plane_t]};
    float eprev[2] = {0.f, 0.f};                                // e[s-1] at (t, f)
    for (int s = 0; s < nb; ++s) {
      const bool more = s + 1 < nb;                             // the last REAL section has no successor, whatever lies behind it
      float e[2], edn[2] = {0.f, 0.f}, eup[2] = {0.f, 0.f}, on[2] = {0.f, 0.f}, gn[2] = {0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float* qo = po + (size_t)(2 * s + c) * plane_o;
        const float* qt = pt + (size_t)(2 * s + c) * plane_t;
        e[c] = o[c] - g[c];
        if (down) edn[c] = qo[Fq] - qt[tld];
        if (up) eup[c] = qo[-(long)Fq] - qt[-tld];
        if (more) { on[c] = qo[2 * plane_o]; gn[c] = qt[2 * plane_t]; }
      }
      const float mo2 = o[0] * o[0] + o[1] * o[1];
      const float mo = sqrtf(mo2 + 1e-8f), mt = sqrtf(g[0] * g[0] + g[1] * g[1] + 1e-8f);
      float dphi = atan2f(o[1], o[0]) - atan2f(g[1], g[0]);
      dphi = dphi + PI_F;
      dphi = dphi - 2.f * PI_F * floorf(dphi / (2.f * PI_F)) - PI_F;      // torch.remainder(., 2pi) - pi
      acc[0] += e[0] * e[0] + e[1] * e[1];
      acc[1] += (mo - mt) * (mo - mt);
      acc[2] += dphi * dphi;
      const float inv2 = 1.f / mo2;                             // atan2 backward: (-im, re) / (re^2 + im^2)
      const float gph[2] = {-o[1] * inv2, o[0] * inv2};
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        float gt = 0.f, gs = 0.f;
        if (more) { const float d = (on[c] - gn[c]) - e[c]; acc[3] += d * d; gt -= d; }
        if (s > 0) gt += e[c] - eprev[c];
        if (down) { const float d = edn[c] - e[c]; acc[4] += d * d; gs -= d; }
        if (up) gs += e[c] - eup[c];
        pg[(size_t)(2 * s + c) * plane_o] =
            2.f * (c_mse * e[c] + c_mag * (mo - mt) * o[c] / mo + c_ph * dphi * gph[c] + c_tmp * gt + c_spc * gs);
        eprev[c] = e[c];
        o[c] = on[c]; g[c] = gn[c];
      }
    }
    for (int s = nb; s < S; ++s) {                              // padded sections: gradient exactly 0
      pg[(size_t)(2 * s) * plane_o] = 0.f;
      pg[(size_t)(2 * s + 1) * plane_o] = 0.f;
    }
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const float v = block_sum(acc[k], red);
    if (threadIdx.x == 0) part[((size_t)b * gridDim.x + blockIdx.x) * 5 + k] = v;
  }
}

// loss = sum_b w_b * res[b][5]: one wave, lane l adds the clips l, l + 64, ... in order, then wave_sum's fixed butterfly
__global__ __launch_bounds__(64) void recon_len_loss_kernel(const float* __restrict__ res, const float* __restrict__ clip_weights, int B,
                                                             float* __restrict__ loss) {
  float v = 0.f;
  for (int b = threadIdx.x; b < B; b += 64) v += (clip_weights ? clip_weights[b] : 1.f / (float)B) * res[(size_t)b * 11 + 5];
  v = wave_sum(v);
  if (threadIdx.x == 0) loss[0] = v;
}

// ---- InfoNCE (losses.py:9-36), one workgroup of 1024 -------------------------------
__global__ __launch_bounds__(1024) void infonce_kernel(const float* __restrict__ x, const int* __restrict__ labels, int B, int D,
                                                        float temperature, float* __restrict__ loss, float* __restrict__ dx,
                                                        float* __restrict__ ws /* B*B sim + B*B G + B inv */) {
  __shared__ float red[17];
  float* sim = ws; float* G = ws + (size_t)B * B; float* inv = G + (size_t)B * B;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  for (int i = wave; i < B; i += nw) {
    float q = 0.f;
    for (int d = lane; d < D; d += 64) q += x[(size_t)i * D + d] * x[(size_t)i * D + d];
    q = wave_sum(q);
    if (lane == 0) inv[i] = 1.f / fmaxf(sqrtf(q), 1e-12f);
  }
  __syncthreads();
  for (int p = wave; p < B * B; p += nw) {
    const int i = p / B, j = p % B;
    float q = 0.f;
    for (int d = lane; d < D; d += 64) q += x[(size_t)i * D + d] * x[(size_t)j * D + d];
    q = wave_sum(q);
    if (lane == 0) sim[p] = i == j ? -1e9f : q * inv[i] * inv[j];
  }
  __syncthreads();
  float part = 0.f;
  for (int i = tid; i < B; i += blockDim.x) {
    float mx = -INFINITY;
    for (int j = 0; j < B; ++j) mx = fmaxf(mx, sim[i * B + j] / temperature);
    float den = 0.f;
    for (int j = 0; j < B; ++j) den += __expf(sim[i * B + j] / temperature - mx);
    const float lse = mx + __logf(den);
    int cnt = 0; float sp = 0.f;
    for (int j = 0; j < B; ++j) if (j != i && labels[j] == labels[i]) { ++cnt; sp += sim[i * B + j] / temperature - lse; }
    const float cd = (float)max(cnt, 1);
    part += -sp / cd / B;
    for (int j = 0; j < B; ++j) {
      const float pj = j == i ? 0.f : __expf(sim[i * B + j] / temperature - lse);
      const float pos = (j != i && labels[j] == labels[i]) ? 1.f : 0.f;
      G[i * B + j] = ((cnt > 0 ? pj : 0.f) - pos / cd) / (B * temperature);   // d loss / d sim_ij
    }
  }
  part = block_sum(part, red);
  if (tid == 0) loss[0] = part;
  if (!dx) return;
  __syncthreads();
  // de_i = sum_j (G_ij + G_ji) e_j ; dx_i = (de_i - e_i <e_i,de_i>) * inv_i
  for (int i = wave; i < B; i += nw) {
    float de[8];
    float dot = 0.f;
    const int nd = (D + 63) / 64;
    for (int k = 0; k < nd && k < 8; ++k) {
      const int d = lane + 64 * k;
      float a = 0.f;
      if (d < D)
        for (int j = 0; j < B; ++j) a += (G[i * B + j] + G[j * B + i]) * x[(size_t)j * D + d] * inv[j];
      de[k] = a;
      if (d < D) dot += a * x[(size_t)i * D + d] * inv[i];
    }
    dot = wave_sum(dot);
    for (int k = 0; k < nd && k < 8; ++k) {
      const int d = lane + 64 * k;
      if (d < D) dx[(size_t)i * D + d] = (de[k] - x[(size_t)i * D + d] * inv[i] * dot) * inv[i];
    }
  }
}

// ---- margin loss (losses.py:45-57) -------------------------------------------------
__global__ __launch_bounds__(64) void margin_kernel(const float* __restrict__ c, int C, int D, float margin, float* __restrict__ loss,
                                                     float* __restrict__ dc) {
  const int lane = threadIdx.x;
  const int npairs = C * (C - 1) / 2;
  if (dc) for (int i = lane; i < C * D; i += 64) dc[i] = 0.f;
  float total = 0.f;
  for (int i = 0; i < C; ++i)
    for (int j = i + 1; j < C; ++j) {
      float q = 0.f;
      for (int d = lane; d < D; d += 64) { const float v = c[i * D + d] - c[j * D + d]; q += v * v; }
      const float dist = sqrtf(wave_sum(q));
      const float h = fmaxf(margin - dist, 0.f);
      total += h * h / npairs;
      if (dc && h > 0.f && dist > 0.f) {
        const float k = -2.f * h / (dist * npairs);
        for (int d = lane; d < D; d += 64) {
          const float v = c[i * D + d] - c[j * D + d];
          dc[i * D + d] += k * v; dc[j * D + d] -= k * v;
        }
      }
    }
  if (lane == 0) loss[0] = total;
}

// ---- HSIC with the reference's median heuristic (losses.py:138-191) -----------------
// ws: d2[(2B)^2] | K[B^2] | L[B^2] | rmK[B] | rmL[B] | misc[8] ; ihist in LDS.
__global__ __launch_bounds__(1024) void hsic_kernel(const float* __restrict__ s, const float* __restrict__ c, int B, int D,
                                                     float* __restrict__ loss, float* __restrict__ ds, float* __restrict__ dc,
                                                     float* __restrict__ ws) {
  __shared__ float red[17];
  __shared__ unsigned hist[256];
  __shared__ unsigned sel_prefix, sel_rank, sel_index;
  const int M = 2 * B, n = M * M;
  float* d2 = ws; float* K = d2 + n; float* L = K + B * B; float* rmK = L + B * B; float* rmL = rmK + B;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  auto row = [&](int i) { return i < B ? s + (size_t)i * D : c + (size_t)(i - B) * D; };
  for (int p = wave; p < n; p += nw) {
    const int i = p / M, j = p % M;
    const float* a = row(i); const float* b = row(j);
    float q = 0.f;
    for (int d = lane; d < D; d += 64) { const float v = a[d] - b[d]; q += v * v; }
    q = wave_sum(q);
    if (lane == 0) d2[p] = q;
  }
  __syncthreads();
  // radix select of rank n/2-1 (lower median of the full matrix, diagonal included) on the
  // bit pattern of dist = sqrt(d2) (monotone for non-negative floats)
  if (tid == 0) { sel_prefix = 0; sel_rank = (unsigned)(n / 2 - 1); sel_index = 0xffffffffu; }
  __syncthreads();
  for (int pass = 3; pass >= 0; --pass) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    const unsigned shift = pass * 8;
    const unsigned himask = pass == 3 ? 0u : (0xffffffffu << (shift + 8));
    const unsigned pref = sel_prefix;
    for (int p = tid; p < n; p += blockDim.x) {
      const unsigned bits = __float_as_uint(sqrtf(d2[p]));
      if ((bits & himask) == pref) atomicAdd(&hist[(bits >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned r = sel_rank, bsel = 0;
      for (unsigned bkt = 0; bkt < 256; ++bkt) { if (r < hist[bkt]) { bsel = bkt; break; } r -= hist[bkt]; }
      sel_rank = r; sel_prefix = pref | (bsel << shift);
    }
    __syncthreads();
  }
  const unsigned sbits = sel_prefix;
  for (int p = tid; p < n; p += blockDim.x)
    if (__float_as_uint(sqrtf(d2[p])) == sbits) atomicMin(&sel_index, (unsigned)p);
  __syncthreads();
  const float sigma = __uint_as_float(sbits);
  const float i2s2 = 1.f / (2.f * sigma * sigma);
  for (int p = tid; p < B * B; p += blockDim.x) {
    const int i = p / B, j = p % B;
    K[p] = __expf(-d2[i * M + j] * i2s2);
    L[p] = __expf(-d2[(B + i) * M + (B + j)] * i2s2);
  }
  __syncthreads();
  for (int i = tid; i < B; i += blockDim.x) {
    // the centred matrices are small differences of entries near their means (K - rmK_i - rmK_j + mK is ~0.03 where K is ~0.7),
    // and an error of a row mean enters a whole row of them with one sign: the means are summed in double
    double a = 0.0, b = 0.0;
    for (int j = 0; j < B; ++j) { a += (double)K[i * B + j]; b += (double)L[i * B + j]; }
    rmK[i] = (float)(a / B); rmL[i] = (float)(b / B);
  }
  __syncthreads();
  double tk = 0.0, tl = 0.0;
  for (int i = 0; i < B; ++i) { tk += (double)rmK[i]; tl += (double)rmL[i]; }      // every thread the same B <= 128 values, in order
  const float mK = (float)(tk / B);
  const float mL = (float)(tl / B);
  const float nrm = 1.f / ((float)(B - 1) * (B - 1));
  // hsic = sum Kc_ij L_ij * nrm ; gsig = sum (Lc K nS + Kc L nC) * nrm / sigma^3
  float hp = 0.f, gsp = 0.f;
  for (int p = tid; p < B * B; p += blockDim.x) {
    const int i = p / B, j = p % B;
    const float Kc = K[p] - rmK[i] - rmK[j] + mK, Lc = L[p] - rmL[i] - rmL[j] + mL;
    hp += Kc * Lc;                              // = sum Kc L (Kc is doubly centred), without the mean of L multiplying Kc's rounding
    gsp += Lc * K[p] * d2[i * M + j] + Kc * L[p] * d2[(B + i) * M + (B + j)];
  }
  const float hsic = block_sum(hp, red) * nrm;
  const float gsig = block_sum(gsp, red) * nrm / (sigma * sigma * sigma);
  if (tid == 0) loss[0] = hsic;
  if (!ds || !dc) return;
  const unsigned pq = sel_index;
  const int pi = (int)(pq / M), qi = (int)(pq % M);
  const float gd = (pi != qi && sigma > 0.f) ? gsig / sigma : 0.f;
  // dS_i = -(2/sigma^2) sum_j Lc_ij K_ij (S_i - S_j) * nrm  (+ sigma path on rows p, q)
  for (int r = wave; r < M; r += nw) {
    const bool is_s = r < B;
    const int i = is_s ? r : r - B;
    const float* X = is_s ? s : c;
    const float* Aij = is_s ? K : L;
    const float* rmO = is_s ? rmL : rmK;       // centred matrix of the OTHER kernel
    const float* Oij = is_s ? L : K;
    const float mO = is_s ? mL : mK;
    float* dX = is_s ? ds : dc;
    for (int d = lane; d < D; d += 64) {
      float a = 0.f;
      for (int j = 0; j < B; ++j) {
        const float Oc = Oij[i * B + j] - rmO[i] - rmO[j] + mO;
        a += Oc * Aij[i * B + j] * (X[(size_t)i * D + d] - X[(size_t)j * D + d]);
      }
      a *= -4.f * i2s2 * nrm;
      if (r == pi) a += gd * (row(pi)[d] - row(qi)[d]);
      if (r == qi) a -= gd * (row(pi)[d] - row(qi)[d]);
      dX[(size_t)i * D + d] = a;
    }
  }
}

// ---- cross-covariance penalty (losses.py:146-150): ||Sc^T Cc / (B-1)||_F^2 = sum_ij <Sc_i,Sc_j><Cc_i,Cc_j> / (B-1)^2
// ws: mean_s[D] | mean_c[D] | GS[B*B] | GC[B*B]
__global__ __launch_bounds__(1024) void crosscov_kernel(const float* __restrict__ s, const float* __restrict__ c, int B, int D,
                                                         float* __restrict__ loss, float* __restrict__ ds, float* __restrict__ dc,
                                                         float* __restrict__ ws) {
  __shared__ float red[17];
  float* ms = ws; float* mc = ws + D; float* GS = mc + D; float* GC = GS + (size_t)B * B;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  for (int d = tid; d < D; d += blockDim.x) {
    float a = 0.f, b = 0.f;
    for (int i = 0; i < B; ++i) { a += s[(size_t)i * D + d]; b += c[(size_t)i * D + d]; }
    ms[d] = a / B; mc[d] = b / B;
  }
  __syncthreads();
  for (int p = wave; p < B * B; p += nw) {
    const int i = p / B, j = p % B;
    float a = 0.f, b = 0.f;
    for (int d = lane; d < D; d += 64) {
      a += (s[(size_t)i * D + d] - ms[d]) * (s[(size_t)j * D + d] - ms[d]);
      b += (c[(size_t)i * D + d] - mc[d]) * (c[(size_t)j * D + d] - mc[d]);
    }
    a = wave_sum(a); b = wave_sum(b);
    if (lane == 0) { GS[p] = a; GC[p] = b; }
  }
  __syncthreads();
  const float nrm = 1.f / ((float)(B - 1) * (B - 1));
  float part = 0.f;
  for (int p = tid; p < B * B; p += blockDim.x) part += GS[p] * GC[p];
  part = block_sum(part, red) * nrm;
  if (tid == 0) loss[0] = part;
  if (!ds || !dc) return;
  // d/dS_i = 2 nrm sum_j GC_ij Sc_j (centring adds nothing: columns of GC sum to 0), same for C with GS
  for (int idx = tid; idx < B * D; idx += blockDim.x) {
    const int i = idx / D, d = idx % D;
    float a = 0.f, b = 0.f;
    for (int j = 0; j < B; ++j) {
      a += GC[i * B + j] * (s[(size_t)j * D + d] - ms[d]);
      b += GS[i * B + j] * (c[(size_t)j * D + d] - mc[d]);
    }
    ds[idx] = 2.f * nrm * a; dc[idx] = 2.f * nrm * b;
  }
}

__global__ void cross_entropy_kernel(const float* __restrict__ logits, const int* __restrict__ target, int R, int C, float* __restrict__ loss,
                                     float* __restrict__ dl) {
  __shared__ float red[17];
  float part = 0.f;
  for (int r = threadIdx.x; r < R; r += blockDim.x) {
    const float* z = logits + (size_t)r * C;
    float mx = -INFINITY;
    for (int k = 0; k < C; ++k) mx = fmaxf(mx, z[k]);
    float den = 0.f;
    for (int k = 0; k < C; ++k) den += __expf(z[k] - mx);
    const float lse = mx + __logf(den);
    part += (lse - z[target[r]]) / R;
    // softmax as exp(z - max) / den: z - lse would round at the size of the logits (ulp(150) = 1.5e-5 into the exponent)
    if (dl) for (int k = 0; k < C; ++k) dl[(size_t)r * C + k] = (__expf(z[k] - mx) / den - (k == target[r] ? 1.f : 0.f)) / R;
  }
  part = block_sum(part, red);
  if (threadIdx.x == 0) loss[0] = part;
}

__global__ void softmax_entropy_kernel(const float* __restrict__ logits, int R, int C, float* __restrict__ loss, float* __restrict__ dl) {
  __shared__ float red[17];
  float part = 0.f;
  for (int r = threadIdx.x; r < R; r += blockDim.x) {
    const float* z = logits + (size_t)r * C;
    float mx = -INFINITY;
    for (int k = 0; k < C; ++k) mx = fmaxf(mx, z[k]);
    float den = 0.f;
    for (int k = 0; k < C; ++k) den += __expf(z[k] - mx);
    float H = 0.f, gp = 0.f;
    for (int k = 0; k < C; ++k) {
      const float p = __expf(z[k] - mx) / den;
      H -= p * __logf(p + 1e-8f);
      gp += -(__logf(p + 1e-8f) + p / (p + 1e-8f)) * p;
    }
    part += H / R;
    if (dl) for (int k = 0; k < C; ++k) {
      const float p = __expf(z[k] - mx) / den;
      const float g = -(__logf(p + 1e-8f) + p / (p + 1e-8f));
      dl[(size_t)r * C + k] = p * (g - gp) / R;
    }
  }
  part = block_sum(part, red);
  if (threadIdx.x == 0) loss[0] = part;
}

__global__ void scale_kernel(const float* __restrict__ x, const float* __restrict__ dscale, float hscale, float* __restrict__ y, size_t n, int accumulate) {
  const float sc = hscale * (dscale ? dscale[0] : 1.f);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    y[i] = accumulate ? y[i] + sc * x[i] : sc * x[i];
}

}  // namespace

extern "C" int ast_recon_loss(const float* out, const float* tgt, int64_t tgt_ld, int B, int S, int T, int Fq, float c_mse, float c_mag,
                              float c_phase, float c_temporal, float c_spectral, float* sums, float* grad, void* stream) {
  if (!out || !tgt || !sums || B <= 0 || S <= 0 || T <= 0 || Fq <= 0 || tgt_ld < Fq) AST_FAIL("ast_recon_loss: bad args");
  hipStream_t s = (hipStream_t)stream;
  AST_HIP(hipMemsetAsync(sums, 0, 5 * sizeof(float), s));
  const size_t total = (size_t)B * T * Fq;
  if (total >= (1ull << 31)) AST_FAIL("ast_recon_loss: more than 2^31 bins per section");
  // every workgroup ends in 5 same-address f32 atomics, which serialise at ~10 ns each (1024 workgroups of 256: ~50 of the
  // kernel's 95 us; 4608: +250 us): the same 256 K threads as 256 workgroups of 1024
  static const int max_blocks = env_int("AST_RECON_BLOCKS", 256);
  const int grid = (int)std::min<size_t>((total + 1023) / 1024, (size_t)std::max(1, max_blocks));
  hipLaunchKernelGGL(recon_loss_kernel<false>, dim3(grid), dim3(1024), 0, s, out, tgt, tgt_ld, B, S, T, Fq, c_mse, c_mag, c_phase, c_temporal,
                     c_spectral, sums, grad, 1);
  AST_CHECK_LAUNCH();
  return 0;
}

// One thread per (b, t, f) bin (256-thread workgroups: every load of the pass in flight at once instead of 4-5 dependent trips per
// thread), the workgroups' five partial sums added into AST_RECON_SLOTS rows (72 adders per address instead of 4 608), and a
// finishing launch that reduces the rows in a fixed order and forms the weighted total and the five reported means -- which took
// three element-wise launches behind the 256-workgroup pass (47.9 us on the step's chain).
extern "C" int ast_recon_loss_total(const float* out, const float* tgt, int64_t tgt_ld, int B, int S, int T, int Fq, const float* coef5,
                                    const float* inv5, float* ws, float* res11, float* grad, void* stream) {
  if (!out || !tgt || !coef5 || !inv5 || !ws || !res11 || B <= 0 || S <= 0 || T <= 0 || Fq <= 0 || tgt_ld < Fq) AST_FAIL("ast_recon_loss_total: bad args");
  hipStream_t s = (hipStream_t)stream;
  AST_HIP(hipMemsetAsync(ws, 0, AST_RECON_SLOTS * 5 * sizeof(float), s));
  const size_t total = (size_t)B * T * Fq;
  if (total >= (1ull << 31)) AST_FAIL("ast_recon_loss_total: more than 2^31 bins per section");
  const int grid = (int)std::min<size_t>((total + 255) / 256, 65536);
  hipLaunchKernelGGL(recon_loss_kernel<false>, dim3(grid), dim3(256), 0, s, out, tgt, tgt_ld, B, S, T, Fq, coef5[0], coef5[1], coef5[2], coef5[3],
                     coef5[4], ws, grad, AST_RECON_SLOTS);
  ReconFin a;
  for (int k = 0; k < 5; ++k) { a.c[k] = coef5[k]; a.inv[k] = inv5[k]; }
  hipLaunchKernelGGL(recon_finish_kernel, dim3(1), dim3(64), 0, s, ws, AST_RECON_SLOTS, a, res11);
  AST_CHECK_LAUNCH();
  return 0;
}

// deterministic form: one slot per workgroup (ws >= 5 * ceil(B*T*Fq / 256) floats, written completely, never zeroed), fixed-order finish
extern "C" int ast_recon_loss_total_det(const float* out, const float* tgt, int64_t tgt_ld, int B, int S, int T, int Fq, const float* coef5,
                                        const float* inv5, float* ws, long ws_floats, float* res11, float* grad, void* stream) {
  if (!out || !tgt || !coef5 || !inv5 || !ws || !res11 || B <= 0 || S <= 0 || T <= 0 || Fq <= 0 || tgt_ld < Fq)
    AST_FAIL("ast_recon_loss_total_det: bad args");
  hipStream_t s = (hipStream_t)stream;
  const size_t total = (size_t)B * T * Fq;
  if (total >= (1ull << 31)) AST_FAIL("ast_recon_loss_total_det: more than 2^31 bins per section");
  const size_t grid = (total + 255) / 256;
  if (grid > 65536 || ws_floats < (long)(grid * 5)) AST_FAIL("ast_recon_loss_total_det: ws needs %ld floats (at most 65536 slots)", (long)(grid * 5));
  hipLaunchKernelGGL(recon_loss_kernel<true>, dim3((unsigned)grid), dim3(256), 0, s, out, tgt, tgt_ld, B, S, T, Fq, coef5[0], coef5[1], coef5[2],
                     coef5[3], coef5[4], ws, grad, (int)grid);
  ReconFin a;
  for (int k = 0; k < 5; ++k) { a.c[k] = coef5[k]; a.inv[k] = inv5[k]; }
  hipLaunchKernelGGL(recon_finish_det_kernel, dim3(1), dim3(320), 0, s, ws, (int)grid, a, res11);
  AST_CHECK_LAUNCH();
  return 0;
}

// workgroups per clip of recon_len_kernel (one bin per thread up to RLEN_MAX_BLOCKS), or 0 for sizes the entry refuses
static long recon_len_blocks(int B, int S, int T, int Fq) {
  if (B <= 0 || B > 65535 || S <= 0 || T <= 0 || Fq <= 0) return 0;
  const size_t bins = (size_t)T * Fq;
  if ((size_t)B * bins >= (1ull << 31)) return 0;
  return (long)std::min<size_t>((bins + RLEN_THREADS - 1) / RLEN_THREADS, RLEN_MAX_BLOCKS);
}

extern "C" long ast_recon_loss_len_ws_floats(int B, int S, int T, int Fq) {
  const long nblk = recon_len_blocks(B, S, T, Fq);
  if (nblk <= 0) AST_FAIL("ast_recon_loss_len_ws_floats: bad sizes (1 <= B <= 65535, S, T, Fq >= 1, B*T*Fq < 2^31)");
  return 5 * nblk * B;
}

// The per-clip form of ast_recon_loss_total for a padded batch: one pass of stores, one finishing launch, no atomics and no host
// read of n_sections, so the pair is capturable and bit-reproducible as it stands (default and deterministic mode alike).
extern "C" int ast_recon_loss_len(const float* out, const float* tgt, int64_t tgt_ld, int B, int S, int T, int Fq, const int32_t* n_sections,
                                  const float* coef5, float* ws, long ws_floats, float* res, void* stream) {
  if (!out || !tgt || !coef5 || !ws || !res) AST_FAIL("ast_recon_loss_len: bad args (null out, tgt, coef5, ws or res)");
  if (B <= 0 || S <= 0 || T <= 0 || Fq <= 0) AST_FAIL("ast_recon_loss_len: bad args (B=%d S=%d T=%d Fq=%d must all be >= 1)", B, S, T, Fq);
  if (tgt_ld < Fq) AST_FAIL("ast_recon_loss_len: bad args (tgt_ld %lld < Fq %d)", (long long)tgt_ld, Fq);
  if ((size_t)B * T * Fq >= (1ull << 31)) AST_FAIL("ast_recon_loss_len: more than 2^31 bins per section");
  const long nblk = recon_len_blocks(B, S, T, Fq);
  if (nblk <= 0) AST_FAIL("ast_recon_loss_len: bad args (B %d > 65535)", B);
  if (ws_floats < 5 * nblk * B) AST_FAIL("ast_recon_loss_len: ws needs %ld floats, got %ld", 5 * nblk * B, ws_floats);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(recon_len_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(RLEN_THREADS), 0, s, out, tgt, tgt_ld, S, T, Fq, n_sections, ws);
  ReconLenW a;
  for (int k = 0; k < 5; ++k) a.w[k] = coef5[k];
  hipLaunchKernelGGL(recon_len_finish_kernel, dim3((unsigned)B), dim3(320), 0, s, ws, (int)nblk, S, T, Fq, n_sections, a, res);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" long ast_recon_loss_len_grad_ws_floats(int B, int S, int T, int Fq) {
  const long nblk = recon_len_blocks(B, S, T, Fq);
  if (nblk <= 0) AST_FAIL("ast_recon_loss_len_grad_ws_floats: bad sizes (1 <= B <= 65535, S, T, Fq >= 1, B*T*Fq < 2^31)");
  return 5 * nblk * B;
}

// ast_recon_loss_len plus the scalar loss = sum_b w_b total_b and its gradient: the pass (stores only), ast_recon_loss_len's finish
// and a one-wave launch for the scalar.  No atomics, no memset, no host read: capturable, bit-reproducible in both modes.
extern "C" int ast_recon_loss_len_grad(const float* out, const float* tgt, int64_t tgt_ld, int B, int S, int T, int Fq,
                                       const int32_t* n_sections, const float* clip_weights, const float* coef5, float* ws, long ws_floats,
                                       float* res, float* loss, float* grad, void* stream) {
  if (!out || !tgt || !coef5 || !ws || !res || !loss || !grad)
    AST_FAIL("ast_recon_loss_len_grad: bad args (null out, tgt, coef5, ws, res, loss or grad)");
  if (B <= 0 || S <= 0 || T <= 0 || Fq <= 0) AST_FAIL("ast_recon_loss_len_grad: bad args (B=%d S=%d T=%d Fq=%d must all be >= 1)", B, S, T, Fq);
  if (tgt_ld < Fq) AST_FAIL("ast_recon_loss_len_grad: bad args (tgt_ld %lld < Fq %d)", (long long)tgt_ld, Fq);
  const size_t bins = (size_t)T * Fq;                           // < 2^62: the product below cannot wrap once bins < 2^31
  if (bins >= (1ull << 31) || (size_t)B * bins >= (1ull << 31)) AST_FAIL("ast_recon_loss_len_grad: B*T*Fq = %d*%d*%d must be < 2^31", B, T, Fq);
  const long nblk = recon_len_blocks(B, S, T, Fq);
  if (nblk <= 0) AST_FAIL("ast_recon_loss_len_grad: bad args (B %d > 65535)", B);
  if (ws_floats < 5 * nblk * B) AST_FAIL("ast_recon_loss_len_grad: ws needs %ld floats, got %ld", 5 * nblk * B, ws_floats);
  hipStream_t s = (hipStream_t)stream;
  ReconLenW a;
  for (int k = 0; k < 5; ++k) a.w[k] = coef5[k];
  hipLaunchKernelGGL(recon_len_grad_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(RLEN_THREADS), 0, s, out, tgt, tgt_ld, B, S, T, Fq, n_sections,
                     clip_weights, a, ws, grad);
  hipLaunchKernelGGL(recon_len_finish_kernel, dim3((unsigned)B), dim3(320), 0, s, ws, (int)nblk, S, T, Fq, n_sections, a, res);
  hipLaunchKernelGGL(recon_len_loss_kernel, dim3(1), dim3(64), 0, s, res, clip_weights, B, loss);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" int ast_infonce(const float* emb, const int32_t* labels, int B, int D, float temperature, float* loss, float* demb, float* ws,
                           void* stream) {
  if (!emb || !labels || !loss || !ws || B < 1 || B > 256 || D < 1 || D > 512) AST_FAIL("ast_infonce: bad args (B<=256, D<=512)");
  hipLaunchKernelGGL(infonce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, emb, labels, B, D, temperature, loss, demb, ws);
  AST_CHECK_LAUNCH();
  return 0;
}
extern "C" int ast_margin(const float* cls, int C, int D, float margin, float* loss, float* dcls, void* stream) {
  if (!cls || !loss || C < 2 || D < 1) AST_FAIL("ast_margin: bad args (C >= 2 rows of D >= 1 floats)");
  hipLaunchKernelGGL(margin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, cls, C, D, margin, loss, dcls);
  AST_CHECK_LAUNCH();
  return 0;
}
extern "C" int ast_hsic(const float* s, const float* c, int B, int D, float* loss, float* ds, float* dc, float* ws, void* stream) {
  if (!s || !c || !loss || !ws || B < 2 || B > 128) AST_FAIL("ast_hsic: bad args (2<=B<=128)");
  if (D < 1) AST_FAIL("ast_hsic: bad args (D >= 1)");
  if (!ds != !dc) AST_FAIL("ast_hsic: ds and dc come together (both gradients or neither)");
  hipLaunchKernelGGL(hsic_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, s, c, B, D, loss, ds, dc, ws);
  AST_CHECK_LAUNCH();
  return 0;
}
extern "C" int ast_crosscov(const float* s, const float* c, int B, int D, float* loss, float* ds, float* dc, float* ws, void* stream) {
  if (!s || !c || !loss || !ws || B < 2 || B > 256) AST_FAIL("ast_crosscov: bad args (2<=B<=256)");
  if (D < 1) AST_FAIL("ast_crosscov: bad args (D >= 1)");
  if (!ds != !dc) AST_FAIL("ast_crosscov: ds and dc come together (both gradients or neither)");
  hipLaunchKernelGGL(crosscov_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, s, c, B, D, loss, ds, dc, ws);
  AST_CHECK_LAUNCH();
  return 0;
}
extern "C" int ast_cross_entropy(const float* logits, const int32_t* target, int R, int C, float* loss, float* dlogits, void* stream) {
  if (!logits || !target || !loss || R < 1 || C < 1) AST_FAIL("ast_cross_entropy: bad args");
  hipLaunchKernelGGL(cross_entropy_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, target, R, C, loss, dlogits);
  AST_CHECK_LAUNCH();
  return 0;
}
extern "C" int ast_softmax_entropy(const float* logits, int R, int C, float* loss, float* dlogits, void* stream) {
  if (!logits || !loss || R < 1 || C < 1) AST_FAIL("ast_softmax_entropy: bad args");
  hipLaunchKernelGGL(softmax_entropy_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, R, C, loss, dlogits);
  AST_CHECK_LAUNCH();
  return 0;
}
extern "C" int ast_scale(const float* x, const float* dscale, float hscale, float* y, int64_t n, int accumulate, void* stream) {
  if (!x || !y || n < 0) AST_FAIL("ast_scale: bad args");
  if (n == 0) return 0;
  const int grid = (int)std::min<size_t>(((size_t)n + 255) / 256, 4096);
  hipLaunchKernelGGL(scale_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, dscale, hscale, y, (size_t)n, accumulate);
  AST_CHECK_LAUNCH();
  return 0;
}
