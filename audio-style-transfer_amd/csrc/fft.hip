// STFT front-end (utilityFunctions.py:12-37): 1024-point Hann-windowed frames,
// hop 256, reflect padding, as an LDS-staged radix-4 Stockham FFT -- one
// 256-thread workgroup per frame, one radix-4 butterfly per thread per stage
// (5 stages).  The epilogue z-scores each bin (dataloader.py:9-13) and writes the
// frame straight into its row of the (B,S,2,287,F) section tensor
// (utilityFunctions.py:240-263), so the spectrogram never exists in HBM in
// (freq,time) order and no separate normalise / window / collate pass runs.
//
// A batch of clips of different lengths (the _len entries; evaluation_style_transfer.py:135-159 run on a padded batch): the
// per-clip counts are read from the device and clamped.  Each operation has one device body; its two kernels differ only in
// the counts they hand it, so per frame and per sample the arithmetic is the same, in the same order, and a clip of a padded
// batch comes out as it does alone.
#include "ast_common.h"
#include "ast_lengths.h"
#include "fft1024.h"                                     // NFFT and the Stockham network fft1024_stages (shared with metrics.hip)
#include "../../include/ast_hip.h"

namespace {
constexpr int HOP = 256, NBIN = 513;

// One frame (blockIdx.x = row of section blockIdx.y of clip blockIdx.z) of a clip of `ns` samples, `Tb` frames and, with LEN,
// `Sb` sections inside a row of nsamp: reflected at the clip's own end; rows t >= Tb and every row of the sections s >= Sb (the
// dropped tail included) are written as 0 -- a choice that is uniform over the workgroup, ahead of the first barrier.
// stft_sections_kernel passes nsamp and T = 1 + nsamp / 256, stft_sections_len_kernel ast_clip_len of the device count.
template <bool LEN>
__device__ __forceinline__ void stft_sections_body(const float* __restrict__ wave, int nsamp, const float* __restrict__ mean,
                                                   const float* __restrict__ stdv, float* __restrict__ x, int S, int win, int step, int Ftot,
                                                   int ns, int Tb, int Sb) {
  __shared__ float2 buf[2][NFFT];
  const int row = blockIdx.x, s = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int t = s * step + row;
  float* xr = x + ((((size_t)b * S + s) * 2 + 0) * win + row) * Ftot;
  float* xi = x + ((((size_t)b * S + s) * 2 + 1) * win + row) * Ftot;
  if (t >= Tb || (LEN && s >= Sb)) {
    for (int f = tid; f < NBIN; f += 256) { xr[f] = 0.f; xi[f] = 0.f; }
    return;
  }
  const float* w = wave + (size_t)b * nsamp;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = tid + 256 * k;
    int idx = t * HOP + j - NFFT / 2;
    if (idx < 0) idx = -idx;
    if (idx >= ns) idx = 2 * (ns - 1) - idx;             // t < Tb and ns > 512: 0 <= idx < ns
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
__global__ __launch_bounds__(256) void stft_sections_kernel(const float* __restrict__ wave, int nsamp, int T, const float* __restrict__ mean,
                                                             const float* __restrict__ stdv, float* __restrict__ x, int S, int win, int step,
                                                             int Ftot) {
  stft_sections_body<false>(wave, nsamp, mean, stdv, x, S, win, step, Ftot, nsamp, T, S);
}
__global__ __launch_bounds__(256) void stft_sections_len_kernel(const float* __restrict__ wave, int nsamp, const float* __restrict__ mean,
                                                                 const float* __restrict__ stdv, float* __restrict__ x, int S, int win,
                                                                 int step, int Ftot, const int32_t* __restrict__ n_samples) {
  const AstClipLen L = ast_clip_len(n_samples[blockIdx.z], nsamp, win, step);
  stft_sections_body<true>(wave, nsamp, mean, stdv, x, S, win, step, Ftot, L.ns, L.T, L.n_sec);
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

// ---- inverse STFT (utilityFunctions.py:62-82, torch.istft defaults) -------------------
// Clip b of a padded batch holds Tb = n_frames[b] frames, clamped to [2, T], inside rows of T frames.
__device__ __forceinline__ int clip_frames(const int32_t* __restrict__ n_frames, int b, int T) { return min(max(n_frames[b], 2), T); }

// frame blockIdx.x of clip blockIdx.y: Hermitian extension of the one-sided bins, inverse 1024-point FFT (the Stockham network
// on the conjugated spectrum), periodic Hann window -> frames[t][1024].  istft_frames_kernel runs every frame of the row,
// istft_frames_len_kernel leaves before it for the frames t >= Tb.
__device__ __forceinline__ void istft_frames_body(const float* __restrict__ spec, int T, float* __restrict__ frames) {
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
  const int cur = fft1024_stages(buf, tid);
  float* fr = frames + ((size_t)b * T + t) * NFFT;
#pragma unroll
  for (int k4 = 0; k4 < 4; ++k4) {
    const int j = tid + 256 * k4;
    const float hann = 0.5f - 0.5f * cospif(2.f * j / NFFT);
    fr[j] = buf[cur][j].x * (1.f / NFFT) * hann;       // real part of conj(...) = real part
  }
}
__global__ __launch_bounds__(256) void istft_frames_kernel(const float* __restrict__ spec, int T, float* __restrict__ frames) {
  istft_frames_body(spec, T, frames);
}
__global__ __launch_bounds__(256) void istft_frames_len_kernel(const float* __restrict__ spec, int T, float* __restrict__ frames,
                                                                const int32_t* __restrict__ n_frames) {
  if ((int)blockIdx.x >= clip_frames(n_frames, blockIdx.y, T)) return;        // uniform over the workgroup, ahead of the first barrier
  istft_frames_body(spec, T, frames);
}
// overlap-add of the (up to 4) frames t < Tb that cover each sample, divided by the window^2 envelope, centre trimmed.
// istft_ola_kernel passes Tb = T; with LEN (istft_ola_len_kernel, the clip's clamped count) samples i >= HOP * (Tb - 1) are
// written as 0.  The grid-stride loop over the samples (`i0`, `stride`) is the kernels' own.
template <bool LEN>
__device__ __forceinline__ void istft_ola_body(const float* __restrict__ frames, int T, int nout, float* __restrict__ wave, int Tb, int i0,
                                               int stride) {
  const int b = blockIdx.y;
  for (int i = i0; i < nout; i += stride) {
    float acc = 0.f, env = 0.f;
    if (!LEN || i < HOP * (Tb - 1)) {
      const int j = i + NFFT / 2;                        // position in the padded signal
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
__global__ void istft_ola_kernel(const float* __restrict__ frames, int T, int nout, float* __restrict__ wave) {
  istft_ola_body<false>(frames, T, nout, wave, T, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}
__global__ void istft_ola_len_kernel(const float* __restrict__ frames, int T, int nout, float* __restrict__ wave,
                                     const int32_t* __restrict__ n_frames) {
  istft_ola_body<true>(frames, T, nout, wave, clip_frames(n_frames, blockIdx.y, T), blockIdx.x * blockDim.x + threadIdx.x,
                       gridDim.x * blockDim.x);
}

// sections2spectrogram (utilityFunctions.py:265-283): count-normalised overlap-average of S windows of `wind` frames at
// step `hop` back to one (2, n_time, F) spectrogram per clip, truncated to `out_T` frames.  One thread per 4 bins.
// LEN (overlap_avg_len_kernel): clip b averages its sections k < n_sec[b] only, in the sum and in the count (later sections
// are never read), and frames t >= n_frames[b] are written as 0; both are clamped to [1, S] / [1, out_T].  overlap_avg_kernel
// passes no lengths: every clip has S sections and out_T frames.
template <bool LEN>
__device__ __forceinline__ void overlap_avg_body(const float* __restrict__ sec, float* __restrict__ out, int S, int wind, int hop, int F_in,
                                                 int F_out, int out_T, size_t total4, const int32_t* __restrict__ n_sec,
                                                 const int32_t* __restrict__ n_frames) {
  const int f4n = (F_out + 3) >> 2;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (size_t)gridDim.x * 256) {
    const int f = (int)(i % f4n) * 4;
    size_t r = i / f4n;
    const int t = (int)(r % out_T); r /= out_T;
    const int c = (int)(r % 2);
    const size_t b = r / 2;
    int Sb = S, Tb = out_T;
    if (LEN) { Sb = min(max(n_sec[b], 1), S); Tb = min(max(n_frames[b], 1), out_T); }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int cnt = 0;
    const int i_hi = (!LEN || t < Tb) ? min(Sb - 1, t / hop) : -1, i_lo = max(0, (t - wind + hop) / hop);
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
__global__ __launch_bounds__(256) void overlap_avg_kernel(const float* __restrict__ sec, float* __restrict__ out, int S, int wind,
                                                          int hop, int F_in, int F_out, int out_T, size_t total4) {
  overlap_avg_body<false>(sec, out, S, wind, hop, F_in, F_out, out_T, total4, nullptr, nullptr);
}
__global__ __launch_bounds__(256) void overlap_avg_len_kernel(const float* __restrict__ sec, float* __restrict__ out, int S, int wind,
                                                              int hop, int F_in, int F_out, int out_T, size_t total4,
                                                              const int32_t* __restrict__ n_sec, const int32_t* __restrict__ n_frames) {
  overlap_avg_body<true>(sec, out, S, wind, hop, F_in, F_out, out_T, total4, n_sec, n_frames);
}

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

// ---- host side: one launcher per operation.  `equal` is nullptr behind the entry for equal clips; behind its _len twin it is
// that entry's name (for the message that sends a caller without lengths there) and the length arguments are required.
int overlap_avg_launch(const char* name, const char* equal, const float* sections, float* out, int Bc, int S, int wind, int hop, int F_in,
                       int F_out, int out_T, const int32_t* n_sec, const int32_t* n_frames, void* stream) {
  if (!sections || !out || Bc < 1 || S < 1 || wind < 1 || hop < 1 || hop > wind || F_out < 1 || F_out > F_in || out_T < 1 ||
      out_T > hop * (S - 1) + wind)
    AST_FAIL("%s: bad args", name);
  if (equal && (!n_sec || !n_frames)) AST_FAIL("%s: n_sec / n_frames is NULL (equal clips: %s)", name, equal);
  const size_t total4 = (size_t)Bc * 2 * out_T * ((F_out + 3) / 4);
  const dim3 grid((unsigned)std::min<size_t>((total4 + 255) / 256, 4096));
  if (equal)
    hipLaunchKernelGGL(overlap_avg_len_kernel, grid, dim3(256), 0, (hipStream_t)stream, sections, out, S, wind, hop, F_in, F_out, out_T, total4,
                       n_sec, n_frames);
  else
    hipLaunchKernelGGL(overlap_avg_kernel, grid, dim3(256), 0, (hipStream_t)stream, sections, out, S, wind, hop, F_in, F_out, out_T, total4);
  AST_CHECK_LAUNCH();
  return 0;
}

int istft_launch(const char* name, const char* equal, const float* spec, int Bc, int T, float* frames_ws, float* wave, const int32_t* n_frames,
                 void* stream) {
  if (!spec || !frames_ws || !wave || Bc <= 0 || T <= 1) AST_FAIL("%s: bad args", name);
  if (equal && !n_frames) AST_FAIL("%s: n_frames is NULL (equal clips: %s)", name, equal);
  hipStream_t s = (hipStream_t)stream;
  const int nout = HOP * (T - 1);
  const dim3 ola_grid((nout + 255) / 256, Bc);
  if (equal) {
    hipLaunchKernelGGL(istft_frames_len_kernel, dim3(T, Bc), dim3(256), 0, s, spec, T, frames_ws, n_frames);
    hipLaunchKernelGGL(istft_ola_len_kernel, ola_grid, dim3(256), 0, s, frames_ws, T, nout, wave, n_frames);
  } else {
    hipLaunchKernelGGL(istft_frames_kernel, dim3(T, Bc), dim3(256), 0, s, spec, T, frames_ws);
    hipLaunchKernelGGL(istft_ola_kernel, ola_grid, dim3(256), 0, s, frames_ws, T, nout, wave);
  }
  AST_CHECK_LAUNCH();
  return 0;
}

int stft_sections_launch(const char* name, const char* equal, const float* wave, int Bc, int nsamp, const float* mean, const float* std_,
                         float* x, int S, int win, int step, int F_total, const int32_t* n_samples, void* stream) {
  if (!wave || !mean || !std_ || !x || Bc <= 0 || nsamp <= NFFT / 2 || S <= 0 || win <= 0 || step <= 0 || F_total < NBIN ||
      (equal && (Bc > 65535 || S > 65535 || !ast_sectioning_ok(win, step))))
    AST_FAIL("%s: bad args", name);
  if (equal) {
    if (!n_samples) AST_FAIL("%s: n_samples is NULL (equal clips: %s)", name, equal);
    if (ast_row_check(name, nsamp, win)) return -1;
    hipLaunchKernelGGL(stft_sections_len_kernel, dim3(win, S, Bc), dim3(256), 0, (hipStream_t)stream, wave, nsamp, mean, std_, x, S, win, step,
                       F_total, n_samples);
  } else {
    hipLaunchKernelGGL(stft_sections_kernel, dim3(win, S, Bc), dim3(256), 0, (hipStream_t)stream, wave, nsamp, 1 + nsamp / HOP, mean, std_, x,
                       S, win, step, F_total);
  }
  AST_CHECK_LAUNCH();
  return 0;
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
  return overlap_avg_launch("ast_sections_overlap_avg", nullptr, sections, out, Bc, S, wind, hop, F_in, F_out, out_T, nullptr, nullptr, stream);
}

extern "C" int ast_sections_overlap_avg_len(const float* sections, float* out, int Bc, int S, int wind, int hop, int F_in, int F_out,
                                            int out_T, const int32_t* n_sec, const int32_t* n_frames, void* stream) {
  return overlap_avg_launch("ast_sections_overlap_avg_len", "ast_sections_overlap_avg", sections, out, Bc, S, wind, hop, F_in, F_out, out_T,
                            n_sec, n_frames, stream);
}

extern "C" int ast_istft(const float* spec, int Bc, int T, float* frames_ws, float* wave, void* stream) {
  return istft_launch("ast_istft", nullptr, spec, Bc, T, frames_ws, wave, nullptr, stream);
}

extern "C" int ast_istft_len(const float* spec, int Bc, int T, float* frames_ws, float* wave, const int32_t* n_frames, void* stream) {
  return istft_launch("ast_istft_len", "ast_istft", spec, Bc, T, frames_ws, wave, n_frames, stream);
}

extern "C" int ast_stft_sections(const float* wave, int Bc, int nsamp, const float* mean, const float* std_, float* x, int S, int win,
                                 int step, int F_total, void* stream) {
  return stft_sections_launch("ast_stft_sections", nullptr, wave, Bc, nsamp, mean, std_, x, S, win, step, F_total, nullptr, stream);
}

extern "C" int ast_stft_sections_len(const float* wave, int Bc, int nsamp, const float* mean, const float* std_, float* x, int S, int win,
                                     int step, int F_total, const int32_t* n_samples, void* stream) {
  return stft_sections_launch("ast_stft_sections_len", "ast_stft_sections", wave, Bc, nsamp, mean, std_, x, S, win, step, F_total, n_samples,
                              stream);
}

extern "C" int ast_frontend_lengths_host(int ns, int nsamp, int win, int step, int* out4) {
  if (!out4 || !ast_sectioning_ok(win, step)) AST_FAIL("ast_frontend_lengths_host: bad args (win=%d step=%d)", win, step);
  if (ast_row_check("ast_frontend_lengths_host", nsamp, win)) return -1;
  const AstClipLen L = ast_clip_len(ns, nsamp, win, step);
  out4[0] = L.ns; out4[1] = L.T; out4[2] = L.n_sec; out4[3] = L.n_frames;
  return 0;
}

extern "C" int ast_frontend_lengths(const int32_t* n_samples, int Bc, int nsamp, int win, int step, int32_t* n_sections_out,
                                    int32_t* n_frames_out, void* stream) {
  if (!n_samples) AST_FAIL("ast_frontend_lengths: n_samples is NULL");
  if (!n_sections_out || !n_frames_out) AST_FAIL("ast_frontend_lengths: null pointer");
  if (Bc < 1 || !ast_sectioning_ok(win, step)) AST_FAIL("ast_frontend_lengths: bad shape (Bc=%d win=%d step=%d)", Bc, win, step);
  if (ast_row_check("ast_frontend_lengths", nsamp, win)) return -1;
  hipLaunchKernelGGL(frontend_lengths_kernel, dim3((Bc + 63) / 64), dim3(64), 0, (hipStream_t)stream, n_samples, Bc, nsamp, win, step,
                     n_sections_out, n_frames_out);
  AST_CHECK_LAUNCH();
  return 0;
}
