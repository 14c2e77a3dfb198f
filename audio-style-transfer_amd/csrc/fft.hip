// STFT front-end (utilityFunctions.py:12-37): 1024-point Hann-windowed frames,
// hop 256, reflect padding, as an LDS-staged radix-4 Stockham FFT -- one
// 256-thread workgroup per frame, one radix-4 butterfly per thread per stage
// (5 stages).  The epilogue z-scores each bin (dataloader.py:9-13) and writes the
// frame straight into its row of the (B,S,2,287,F) section tensor
// (utilityFunctions.py:240-263), so the spectrogram never exists in HBM in
// (freq,time) order and no separate normalise / window / collate pass runs.
#include "ast_common.h"
#include "../../include/ast_hip.h"

namespace {
constexpr int NFFT = 1024, HOP = 256, NBIN = 513;

__global__ __launch_bounds__(256) void stft_sections_kernel(const float* __restrict__ wave, int nsamp, int T, const float* __restrict__ mean,
                                                             const float* __restrict__ stdv, float* __restrict__ x, int S, int win, int step,
                                                             int Ftot) {
  __shared__ float2 buf[2][NFFT];
  const int row = blockIdx.x, s = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int t = s * step + row;
  float* xr = x + ((((size_t)b * S + s) * 2 + 0) * win + row) * Ftot;
  float* xi = x + ((((size_t)b * S + s) * 2 + 1) * win + row) * Ftot;
  if (t >= T) {            // zero padded tail rows of the last section
    for (int f = tid; f < NBIN; f += 256) { xr[f] = 0.f; xi[f] = 0.f; }
    return;
  }
  const float* w = wave + (size_t)b * nsamp;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = tid + 256 * k;
    int idx = t * HOP + j - NFFT / 2;
    if (idx < 0) idx = -idx;
    if (idx >= nsamp) idx = 2 * (nsamp - 1) - idx;
    const float hann = 0.5f - 0.5f * cospif(2.f * j / NFFT);
    buf[0][j] = make_float2(w[idx] * hann, 0.f);
  }
  __syncthreads();
  int cur = 0;
#pragma unroll
  for (int p = 1; p < NFFT; p *= 4) {
    const int k = tid & (p - 1);
    const int j = ((tid - k) << 2) + k;
    const float alpha = -(float)k / (2.f * p);          // in units of pi
    float s1, c1, s2, c2, s3, c3;
    sincospif(alpha, &s1, &c1); sincospif(2.f * alpha, &s2, &c2); sincospif(3.f * alpha, &s3, &c3);
    const float2 a0 = buf[cur][tid], a1 = buf[cur][tid + 256], a2 = buf[cur][tid + 512], a3 = buf[cur][tid + 768];
    const float2 u0 = a0;
    const float2 u1 = make_float2(a1.x * c1 - a1.y * s1, a1.x * s1 + a1.y * c1);
    const float2 u2 = make_float2(a2.x * c2 - a2.y * s2, a2.x * s2 + a2.y * c2);
    const float2 u3 = make_float2(a3.x * c3 - a3.y * s3, a3.x * s3 + a3.y * c3);
    const float2 v0 = make_float2(u0.x + u2.x, u0.y + u2.y), v1 = make_float2(u0.x - u2.x, u0.y - u2.y);
    const float2 v2 = make_float2(u1.x + u3.x, u1.y + u3.y);
    const float2 d = make_float2(u1.x - u3.x, u1.y - u3.y);
    const float2 v3 = make_float2(d.y, -d.x);            // -i * (u1 - u3)
    buf[cur ^ 1][j] = make_float2(v0.x + v2.x, v0.y + v2.y);
    buf[cur ^ 1][j + p] = make_float2(v1.x + v3.x, v1.y + v3.y);
    buf[cur ^ 1][j + 2 * p] = make_float2(v0.x - v2.x, v0.y - v2.y);
    buf[cur ^ 1][j + 3 * p] = make_float2(v1.x - v3.x, v1.y - v3.y);
    cur ^= 1;
    __syncthreads();
  }
  for (int f = tid; f < NBIN; f += 256) {
    const float2 z = buf[cur][f];
    xr[f] = (z.x - mean[f]) / (stdv[f] + 1e-8f);
    xi[f] = (z.y - mean[NBIN + f]) / (stdv[NBIN + f] + 1e-8f);
  }
}
// ---- inverse STFT (utilityFunctions.py:62-82, torch.istft defaults) -------------------
// frame kernel: Hermitian extension of the one-sided bins, inverse 1024-point FFT (same Stockham
// network on the conjugated spectrum), periodic Hann window -> frames[t][1024].
__global__ __launch_bounds__(256) void istft_frames_kernel(const float* __restrict__ spec, int T, float* __restrict__ frames) {
  __shared__ float2 buf[2][NFFT];
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const float* re = spec + ((size_t)b * 2 + 0) * T * NBIN + (size_t)t * NBIN;
  const float* im = spec + ((size_t)b * 2 + 1) * T * NBIN + (size_t)t * NBIN;
#pragma unroll
  for (int k4 = 0; k4 < 4; ++k4) {
    const int k = tid + 256 * k4;
    float xr, xi;
    if (k <= NFFT / 2) { xr = re[k]; xi = (k == 0 || k == NFFT / 2) ? 0.f : im[k]; }     // c2r ignores imag of DC / Nyquist
    else { xr = re[NFFT - k]; xi = -im[NFFT - k]; }
    buf[0][k] = make_float2(xr, -xi);                  // conj(X): x = conj(FFT(conj(X))) / N
  }
  __syncthreads();
  int cur = 0;
#pragma unroll
  for (int p = 1; p < NFFT; p *= 4) {
    const int k = tid & (p - 1);
    const int j = ((tid - k) << 2) + k;
    const float alpha = -(float)k / (2.f * p);
    float s1, c1, s2, c2, s3, c3;
    sincospif(alpha, &s1, &c1); sincospif(2.f * alpha, &s2, &c2); sincospif(3.f * alpha, &s3, &c3);
    const float2 a0 = buf[cur][tid], a1 = buf[cur][tid + 256], a2 = buf[cur][tid + 512], a3 = buf[cur][tid + 768];
    const float2 u0 = a0;
    const float2 u1 = make_float2(a1.x * c1 - a1.y * s1, a1.x * s1 + a1.y * c1);
    const float2 u2 = make_float2(a2.x * c2 - a2.y * s2, a2.x * s2 + a2.y * c2);
    const float2 u3 = make_float2(a3.x * c3 - a3.y * s3, a3.x * s3 + a3.y * c3);
    const float2 v0 = make_float2(u0.x + u2.x, u0.y + u2.y), v1 = make_float2(u0.x - u2.x, u0.y - u2.y);
    const float2 v2 = make_float2(u1.x + u3.x, u1.y + u3.y);
    const float2 d = make_float2(u1.x - u3.x, u1.y - u3.y);
    const float2 v3 = make_float2(d.y, -d.x);
    buf[cur ^ 1][j] = make_float2(v0.x + v2.x, v0.y + v2.y);
    buf[cur ^ 1][j + p] = make_float2(v1.x + v3.x, v1.y + v3.y);
    buf[cur ^ 1][j + 2 * p] = make_float2(v0.x - v2.x, v0.y - v2.y);
    buf[cur ^ 1][j + 3 * p] = make_float2(v1.x - v3.x, v1.y - v3.y);
    cur ^= 1;
    __syncthreads();
  }
  float* fr = frames + ((size_t)b * T + t) * NFFT;
#pragma unroll
  for (int k4 = 0; k4 < 4; ++k4) {
    const int j = tid + 256 * k4;
    const float hann = 0.5f - 0.5f * cospif(2.f * j / NFFT);
    fr[j] = buf[cur][j].x * (1.f / NFFT) * hann;       // real part of conj(...) = real part
  }
}
// overlap-add of the 4 frames that cover each sample, divided by the window^2 envelope, centre trimmed
__global__ void istft_ola_kernel(const float* __restrict__ frames, int T, int nout, float* __restrict__ wave) {
  const int b = blockIdx.y;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nout; i += gridDim.x * blockDim.x) {
    const int j = i + NFFT / 2;                        // position in the padded signal
    float acc = 0.f, env = 0.f;
    const int t_hi = min(T - 1, j / HOP), t_lo = max(0, (j - NFFT + HOP) / HOP);
    for (int t = t_lo; t <= t_hi; ++t) {
      const int o = j - t * HOP;
      if (o < 0 || o >= NFFT) continue;
      const float hann = 0.5f - 0.5f * cospif(2.f * o / NFFT);
      acc += frames[((size_t)b * T + t) * NFFT + o];
      env += hann * hann;
    }
    wave[(size_t)b * nout + i] = env > 1e-11f ? acc / env : acc;
  }
}

// ---- the same pair for a batch of clips of different lengths (ast_istft_len; evaluation_style_transfer.py:135-159 run on a
// padded batch): clip b holds Tb = n_frames[b] frames, read from the device and clamped to [2, T], inside rows of T frames.
// They are kernels of their own, so that the code of the two above does not move; the arithmetic per frame and per sample is
// the same, in the same order, so a clip comes out as it does alone through ast_istft at T = Tb.
__device__ __forceinline__ int clip_frames(const int32_t* __restrict__ n_frames, int b, int T) { return min(max(n_frames[b], 2), T); }

// the 5 radix-4 Stockham stages of istft_frames_kernel / stft_sections_kernel on buf[0] (filled, barrier passed); returns the
// index of the half of buf that holds the result
__device__ __forceinline__ int fft1024_stages(float2 (&buf)[2][NFFT], int tid) {
  int cur = 0;
#pragma unroll
  for (int p = 1; p < NFFT; p *= 4) {
    const int k = tid & (p - 1);
    const int j = ((tid - k) << 2) + k;
    const float alpha = -(float)k / (2.f * p);
    float s1, c1, s2, c2, s3, c3;
    sincospif(alpha, &s1, &c1); sincospif(2.f * alpha, &s2, &c2); sincospif(3.f * alpha, &s3, &c3);
    const float2 a0 = buf[cur][tid], a1 = buf[cur][tid + 256], a2 = buf[cur][tid + 512], a3 = buf[cur][tid + 768];
    const float2 u0 = a0;
    const float2 u1 = make_float2(a1.x * c1 - a1.y * s1, a1.x * s1 + a1.y * c1);
    const float2 u2 = make_float2(a2.x * c2 - a2.y * s2, a2.x * s2 + a2.y * c2);
    const float2 u3 = make_float2(a3.x * c3 - a3.y * s3, a3.x * s3 + a3.y * c3);
    const float2 v0 = make_float2(u0.x + u2.x, u0.y + u2.y), v1 = make_float2(u0.x - u2.x, u0.y - u2.y);
    const float2 v2 = make_float2(u1.x + u3.x, u1.y + u3.y);
    const float2 d = make_float2(u1.x - u3.x, u1.y - u3.y);
    const float2 v3 = make_float2(d.y, -d.x);
    buf[cur ^ 1][j] = make_float2(v0.x + v2.x, v0.y + v2.y);
    buf[cur ^ 1][j + p] = make_float2(v1.x + v3.x, v1.y + v3.y);
    buf[cur ^ 1][j + 2 * p] = make_float2(v0.x - v2.x, v0.y - v2.y);
    buf[cur ^ 1][j + 3 * p] = make_float2(v1.x - v3.x, v1.y - v3.y);
    cur ^= 1;
    __syncthreads();
  }
  return cur;
}
__global__ __launch_bounds__(256) void istft_frames_len_kernel(const float* __restrict__ spec, int T, float* __restrict__ frames,
                                                                const int32_t* __restrict__ n_frames) {
  __shared__ float2 buf[2][NFFT];
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  if (t >= clip_frames(n_frames, b, T)) return;        // uniform over the workgroup, ahead of the first barrier
  const float* re = spec + ((size_t)b * 2 + 0) * T * NBIN + (size_t)t * NBIN;
  const float* im = spec + ((size_t)b * 2 + 1) * T * NBIN + (size_t)t * NBIN;
#pragma unroll
  for (int k4 = 0; k4 < 4; ++k4) {
    const int k = tid + 256 * k4;
    float xr, xi;
    if (k <= NFFT / 2) { xr = re[k]; xi = (k == 0 || k == NFFT / 2) ? 0.f : im[k]; }
    else { xr = re[NFFT - k]; xi = -im[NFFT - k]; }
    buf[0][k] = make_float2(xr, -xi);
  }
  __syncthreads();
  const int cur = fft1024_stages(buf, tid);
  float* fr = frames + ((size_t)b * T + t) * NFFT;
#pragma unroll
  for (int k4 = 0; k4 < 4; ++k4) {
    const int j = tid + 256 * k4;
    const float hann = 0.5f - 0.5f * cospif(2.f * j / NFFT);
    fr[j] = buf[cur][j].x * (1.f / NFFT) * hann;
  }
}
// overlap-add and envelope over the frames t < Tb only; samples i >= HOP * (Tb - 1) are written as 0
__global__ void istft_ola_len_kernel(const float* __restrict__ frames, int T, int nout, float* __restrict__ wave,
                                     const int32_t* __restrict__ n_frames) {
  const int b = blockIdx.y, Tb = clip_frames(n_frames, b, T);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nout; i += gridDim.x * blockDim.x) {
    float acc = 0.f, env = 0.f;
    if (i < HOP * (Tb - 1)) {
      const int j = i + NFFT / 2;
      const int t_hi = min(Tb - 1, j / HOP), t_lo = max(0, (j - NFFT + HOP) / HOP);
      for (int t = t_lo; t <= t_hi; ++t) {
        const int o = j - t * HOP;
        if (o < 0 || o >= NFFT) continue;
        const float hann = 0.5f - 0.5f * cospif(2.f * o / NFFT);
        acc += frames[((size_t)b * T + t) * NFFT + o];
        env += hann * hann;
      }
    }
    wave[(size_t)b * nout + i] = env > 1e-11f ? acc / env : acc;
  }
}
}  // namespace

namespace {
// sections2spectrogram (utilityFunctions.py:265-283): count-normalised overlap-average of S windows of `wind` frames at
// step `hop` back to one (2, n_time, F) spectrogram per clip, truncated to `out_T` frames.  One thread per 4 bins.
__global__ __launch_bounds__(256) void overlap_avg_kernel(const float* __restrict__ sec, float* __restrict__ out, int S, int wind,
                                                          int hop, int F_in, int F_out, int out_T, size_t total4) {
  const int f4n = (F_out + 3) >> 2;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (size_t)gridDim.x * 256) {
    const int f = (int)(i % f4n) * 4;
    size_t r = i / f4n;
    const int t = (int)(r % out_T); r /= out_T;
    const int c = (int)(r % 2);
    const size_t b = r / 2;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int cnt = 0;
    const int i_hi = min(S - 1, t / hop), i_lo = max(0, (t - wind + hop) / hop);
    for (int k = i_lo; k <= i_hi; ++k) {
      const int tt = t - k * hop;
      if (tt < 0 || tt >= wind) continue;
      const float* p = sec + ((((b * S + k) * 2 + c) * wind + tt) * (size_t)F_in) + f;
#pragma unroll
      for (int q = 0; q < 4; ++q) if (f + q < F_out) acc[q] += p[q];
      ++cnt;
    }
    const float inv = 1.f / (float)max(cnt, 1);
    float* o = out + ((b * 2 + c) * (size_t)out_T + t) * F_out + f;
#pragma unroll
    for (int q = 0; q < 4; ++q) if (f + q < F_out) o[q] = acc[q] * inv;
  }
}
// The same for clips of different section counts in one padded batch (ast_sections_overlap_avg_len): clip b averages its
// sections k < n_sec[b] only, in the sum and in the count (later sections are never read), and frames t >= n_frames[b] are
// written as 0.  Both are read from the device and clamped to [1, S] / [1, out_T].  A kernel of its own, so that the code of
// the one above does not move; same sum order per element, so a clip comes out as it does alone at S = n_sec[b].
__global__ __launch_bounds__(256) void overlap_avg_len_kernel(const float* __restrict__ sec, float* __restrict__ out, int S, int wind,
                                                              int hop, int F_in, int F_out, int out_T, size_t total4,
                                                              const int32_t* __restrict__ n_sec, const int32_t* __restrict__ n_frames) {
  const int f4n = (F_out + 3) >> 2;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (size_t)gridDim.x * 256) {
    const int f = (int)(i % f4n) * 4;
    size_t r = i / f4n;
    const int t = (int)(r % out_T); r /= out_T;
    const int c = (int)(r % 2);
    const size_t b = r / 2;
    const int Sb = min(max(n_sec[b], 1), S), Tb = min(max(n_frames[b], 1), out_T);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int cnt = 0;
    const int i_hi = t < Tb ? min(Sb - 1, t / hop) : -1, i_lo = max(0, (t - wind + hop) / hop);
    for (int k = i_lo; k <= i_hi; ++k) {
      const int tt = t - k * hop;
      if (tt < 0 || tt >= wind) continue;
      const float* p = sec + ((((b * S + k) * 2 + c) * wind + tt) * (size_t)F_in) + f;
#pragma unroll
      for (int q = 0; q < 4; ++q) if (f + q < F_out) acc[q] += p[q];
      ++cnt;
    }
    const float inv = 1.f / (float)max(cnt, 1);
    float* o = out + ((b * 2 + c) * (size_t)out_T + t) * F_out + f;
#pragma unroll
    for (int q = 0; q < 4; ++q) if (f + q < F_out) o[q] = acc[q] * inv;
  }
}
}  // namespace

namespace {
// dataloader.py:9-13 normalize: (x - mean[c][f]) / (std[c][f] + eps) over a (C, T, F) spectrogram
__global__ __launch_bounds__(256) void zscore_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                     const float* __restrict__ std_, float* __restrict__ out, int T, int F, float eps,
                                                     size_t total) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int f = (int)(i % F);
    const int c = (int)(i / ((size_t)T * F));
    out[i] = (x[i] - mean[(size_t)c * F + f]) / (std_[(size_t)c * F + f] + eps);
  }
}
}  // namespace

namespace {
// Preprocessing_Dataset/compute_unified_stats.py:34-44 for one clip: per (channel, bin) mean over the T frames and the
// unbiased variance (torch.std(dim=1)**2), ADDED into running sums (the caller divides by the clip count at the end).
// One thread per (channel, bin); consecutive threads read consecutive bins of a frame (coalesced).
__global__ __launch_bounds__(256) void bin_stats_kernel(const float* __restrict__ x, float* __restrict__ mean_acc,
                                                        float* __restrict__ var_acc, int T, int F) {
  const int f = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
  if (f >= F) return;
  const float* p = x + (size_t)c * T * F + f;
  double s = 0.0, q = 0.0;
  for (int t = 0; t < T; ++t) { const double v = p[(size_t)t * F]; s += v; q += v * v; }
  const double m = s / T;
  const double var = T > 1 ? fmax((q - s * m) / (T - 1), 0.0) : 0.0;
  mean_acc[(size_t)c * F + f] += (float)m;
  var_acc[(size_t)c * F + f] += (float)var;
}
}  // namespace

extern "C" int ast_bin_stats_acc(const float* x, float* mean_acc, float* var_acc, int C, int T, int F, void* stream) {
  if (!x || !mean_acc || !var_acc || C < 1 || T < 1 || F < 1) AST_FAIL("ast_bin_stats_acc: bad args");
  hipLaunchKernelGGL(bin_stats_kernel, dim3((F + 255) / 256, C), dim3(256), 0, (hipStream_t)stream, x, mean_acc, var_acc, T, F);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" int ast_zscore(const float* x, const float* mean, const float* std_, float* out, int C, int T, int F, float eps, void* stream) {
  if (!x || !mean || !std_ || !out || C < 1 || T < 1 || F < 1) AST_FAIL("ast_zscore: bad args");
  const size_t total = (size_t)C * T * F;
  hipLaunchKernelGGL(zscore_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)stream, x, mean,
                     std_, out, T, F, eps, total);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" int ast_sections_overlap_avg(const float* sections, float* out, int Bc, int S, int wind, int hop, int F_in, int F_out,
                                        int out_T, void* stream) {
  if (!sections || !out || Bc < 1 || S < 1 || wind < 1 || hop < 1 || hop > wind || F_out < 1 || F_out > F_in || out_T < 1 ||
      out_T > hop * (S - 1) + wind)
    AST_FAIL("ast_sections_overlap_avg: bad args");
  const size_t total4 = (size_t)Bc * 2 * out_T * ((F_out + 3) / 4);
  const unsigned grid = (unsigned)std::min<size_t>((total4 + 255) / 256, 4096);
  hipLaunchKernelGGL(overlap_avg_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, sections, out, S, wind, hop, F_in, F_out, out_T,
                     total4);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" int ast_sections_overlap_avg_len(const float* sections, float* out, int Bc, int S, int wind, int hop, int F_in, int F_out,
                                            int out_T, const int32_t* n_sec, const int32_t* n_frames, void* stream) {
  if (!sections || !out || Bc < 1 || S < 1 || wind < 1 || hop < 1 || hop > wind || F_out < 1 || F_out > F_in || out_T < 1 ||
      out_T > hop * (S - 1) + wind)
    AST_FAIL("ast_sections_overlap_avg_len: bad args");
  if (!n_sec || !n_frames) AST_FAIL("ast_sections_overlap_avg_len: n_sec / n_frames is NULL (equal clips: ast_sections_overlap_avg)");
  const size_t total4 = (size_t)Bc * 2 * out_T * ((F_out + 3) / 4);
  const unsigned grid = (unsigned)std::min<size_t>((total4 + 255) / 256, 4096);
  hipLaunchKernelGGL(overlap_avg_len_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, sections, out, S, wind, hop, F_in, F_out,
                     out_T, total4, n_sec, n_frames);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" int ast_istft_len(const float* spec, int Bc, int T, float* frames_ws, float* wave, const int32_t* n_frames, void* stream) {
  if (!spec || !frames_ws || !wave || Bc <= 0 || T <= 1) AST_FAIL("ast_istft_len: bad args");
  if (!n_frames) AST_FAIL("ast_istft_len: n_frames is NULL (equal clips: ast_istft)");
  hipStream_t s = (hipStream_t)stream;
  const int nout = HOP * (T - 1);
  hipLaunchKernelGGL(istft_frames_len_kernel, dim3(T, Bc), dim3(256), 0, s, spec, T, frames_ws, n_frames);
  hipLaunchKernelGGL(istft_ola_len_kernel, dim3((nout + 255) / 256, Bc), dim3(256), 0, s, frames_ws, T, nout, wave, n_frames);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" int ast_istft(const float* spec, int Bc, int T, float* frames_ws, float* wave, void* stream) {
  if (!spec || !frames_ws || !wave || Bc <= 0 || T <= 1) AST_FAIL("ast_istft: bad args");
  hipStream_t s = (hipStream_t)stream;
  const int nout = HOP * (T - 1);
  hipLaunchKernelGGL(istft_frames_kernel, dim3(T, Bc), dim3(256), 0, s, spec, T, frames_ws);
  hipLaunchKernelGGL(istft_ola_kernel, dim3((nout + 255) / 256, Bc), dim3(256), 0, s, frames_ws, T, nout, wave);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" int ast_stft_sections(const float* wave, int Bc, int nsamp, const float* mean, const float* std_, float* x, int S, int win,
                                 int step, int F_total, void* stream) {
  if (!wave || !mean || !std_ || !x || Bc <= 0 || nsamp <= NFFT / 2 || S <= 0 || win <= 0 || step <= 0 || F_total < NBIN)
    AST_FAIL("ast_stft_sections: bad args");
  const int T = 1 + nsamp / HOP;
  hipLaunchKernelGGL(stft_sections_kernel, dim3(win, S, Bc), dim3(256), 0, (hipStream_t)stream, wave, nsamp, T, mean, std_, x, S, win, step,
                     F_total);
  AST_CHECK_LAUNCH();
  return 0;
}

// ---- the STFT front end for a batch of clips of different sample counts (ast_stft_sections_len, ast_frontend_lengths;
// evaluation_style_transfer.py:135-159 starts from one waveform per clip).  Clip b holds n_samples[b] samples (read from the
// device, clamped to [ast_ns_min(win), nsamp]) inside a zero-padded row of nsamp: it is reflected at its own end, and its
// rows t >= T_b and every row of its sections s >= n_sec_b (the dropped tail included) are written as 0.  Kernels of their
// own, so that the code of stft_sections_kernel does not move; per frame the arithmetic is the same, in the same order, so
// a clip's sections come out as they do alone through ast_stft_sections at nsamp = n_samples[b].
#include "ast_lengths.h"
namespace {
__global__ __launch_bounds__(256) void stft_sections_len_kernel(const float* __restrict__ wave, int nsamp, const float* __restrict__ mean,
                                                                 const float* __restrict__ stdv, float* __restrict__ x, int S, int win,
                                                                 int step, int Ftot, const int32_t* __restrict__ n_samples) {
  __shared__ float2 buf[2][NFFT];
  const int row = blockIdx.x, s = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int t = s * step + row;
  const AstClipLen L = ast_clip_len(n_samples[b], nsamp, win, step);
  float* xr = x + ((((size_t)b * S + s) * 2 + 0) * win + row) * Ftot;
  float* xi = x + ((((size_t)b * S + s) * 2 + 1) * win + row) * Ftot;
  if (t >= L.T || s >= L.n_sec) {      // uniform over the workgroup, ahead of the first barrier
    for (int f = tid; f < NBIN; f += 256) { xr[f] = 0.f; xi[f] = 0.f; }
    return;
  }
  const int ns = L.ns;
  const float* w = wave + (size_t)b * nsamp;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = tid + 256 * k;
    int idx = t * HOP + j - NFFT / 2;
    if (idx < 0) idx = -idx;
    if (idx >= ns) idx = 2 * (ns - 1) - idx;           // t < T_b and ns > 512: 0 <= idx < ns
    const float hann = 0.5f - 0.5f * cospif(2.f * j / NFFT);
    buf[0][j] = make_float2(w[idx] * hann, 0.f);
  }
  __syncthreads();
  const int cur = fft1024_stages(buf, tid);
  for (int f = tid; f < NBIN; f += 256) {
    const float2 z = buf[cur][f];
    xr[f] = (z.x - mean[f]) / (stdv[f] + 1e-8f);
    xi[f] = (z.y - mean[NBIN + f]) / (stdv[NBIN + f] + 1e-8f);
  }
}
// n_sections[b], n_frames[b] of every clip: one thread per clip, ordinary stores
__global__ void frontend_lengths_kernel(const int32_t* __restrict__ n_samples, int Bc, int nsamp, int win, int step,
                                        int32_t* __restrict__ n_sections, int32_t* __restrict__ n_frames) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= Bc) return;
  const AstClipLen L = ast_clip_len(n_samples[b], nsamp, win, step);
  n_sections[b] = L.n_sec;
  n_frames[b] = L.n_frames;
}
}  // namespace

extern "C" int ast_frontend_lengths_host(int ns, int nsamp, int win, int step, int* out4) {
  if (!out4 || win < 1 || win > AST_FE_MAX_WIN || step < 1 || step > win) AST_FAIL("ast_frontend_lengths_host: bad args (win=%d step=%d)", win, step);
  if (nsamp < ast_ns_min(win)) AST_FAIL("ast_frontend_lengths_host: nsamp %d needs >= %d samples (one section at win %d)", nsamp, ast_ns_min(win), win);
  const AstClipLen L = ast_clip_len(ns, nsamp, win, step);
  out4[0] = L.ns; out4[1] = L.T; out4[2] = L.n_sec; out4[3] = L.n_frames;
  return 0;
}

extern "C" int ast_frontend_lengths(const int32_t* n_samples, int Bc, int nsamp, int win, int step, int32_t* n_sections_out,
                                    int32_t* n_frames_out, void* stream) {
  if (!n_samples) AST_FAIL("ast_frontend_lengths: n_samples is NULL");
  if (!n_sections_out || !n_frames_out) AST_FAIL("ast_frontend_lengths: null pointer");
  if (Bc < 1 || win < 1 || win > AST_FE_MAX_WIN || step < 1 || step > win) AST_FAIL("ast_frontend_lengths: bad shape (Bc=%d win=%d step=%d)", Bc, win, step);
  if (nsamp < ast_ns_min(win)) AST_FAIL("ast_frontend_lengths: nsamp %d needs >= %d samples (one section at win %d)", nsamp, ast_ns_min(win), win);
  hipLaunchKernelGGL(frontend_lengths_kernel, dim3((Bc + 63) / 64), dim3(64), 0, (hipStream_t)stream, n_samples, Bc, nsamp, win, step,
                     n_sections_out, n_frames_out);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" int ast_stft_sections_len(const float* wave, int Bc, int nsamp, const float* mean, const float* std_, float* x, int S, int win,
                                     int step, int F_total, const int32_t* n_samples, void* stream) {
  if (!wave || !mean || !std_ || !x || Bc <= 0 || Bc > 65535 || nsamp <= NFFT / 2 || S <= 0 || S > 65535 || win <= 0 || win > AST_FE_MAX_WIN ||
      step <= 0 || step > win || F_total < NBIN)
    AST_FAIL("ast_stft_sections_len: bad args");
  if (!n_samples) AST_FAIL("ast_stft_sections_len: n_samples is NULL (equal clips: ast_stft_sections)");
  if (nsamp < ast_ns_min(win)) AST_FAIL("ast_stft_sections_len: nsamp %d needs >= %d samples (one section at win %d)", nsamp, ast_ns_min(win), win);
  hipLaunchKernelGGL(stft_sections_len_kernel, dim3(win, S, Bc), dim3(256), 0, (hipStream_t)stream, wave, nsamp, mean, std_, x, S, win, step,
                     F_total, n_samples);
  AST_CHECK_LAUNCH();
  return 0;
}
