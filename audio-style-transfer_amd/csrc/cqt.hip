// Constant-Q front end (utilityFunctions.py:39-60, `librosa.cqt(y, sr=22050, n_bins=84, hop_length=256)`) and the
// polyphase resampler of `load_audio` (utilityFunctions.py:105-122, `torchaudio.functional.resample`).
//
// librosa's recursive CQT is, per octave o (top octave first): a rectangular-window STFT of the o-times-halved signal
// at hop 256 >> o, multiplied by the sparsified FFT of 12 wavelets.  Both steps are linear in the frame, so the host
// folds them into 12 complex time-domain kernels W[k][n] (ast_amd/cqt.py) and one octave is a strided correlation:
//     C[k][t] = sum_n y_o[t * hop_o - nfft/2 + n] * W[k][n]           (zero outside the signal: pad_mode="constant")
// 345 frames x 12 filters x 256 taps per octave per clip: HBM/latency-bound byte work, no MFMA.  Between octaves the
// signal is halved by a linear-phase FIR (ast_resample_poly with orig=2, new=1), which is also the kernel behind
// load_audio's 44.1/48 kHz -> 22.05 kHz conversion.
//
// A batch of clips of different sample counts (ast_decimate2_len, ast_cqt_octaves_len, ast_cqt_sections_len;
// evaluation_style_transfer.py:135-159 starts from one waveform per clip): clip b holds n_samples[b] samples (read from the
// device, clamped to [ast_ns_min(win), nsamp]) inside a zero-padded row of nsamp.  After o ceil-halvings it holds
// ceil(ns_b / 2^o) samples; whatever lies behind them in its row (the FIR's ringing into the padding) is read as 0 by the next
// halving and by the octave kernel, as the clip alone ends there.  Each operation has one device body; its two kernels differ
// only in the counts they hand it, so a clip's samples, frames and sections come out as they do alone.
#include "ast_common.h"
#include "ast_lengths.h"

#define AST_CQT_MAX_OCTAVES 12
#define AST_CQT_FR 8                     // frames per workgroup of the octave kernel

namespace {

// one workgroup per (8 frames, clip, octave); their sample span is staged in LDS once and read by the 4 waves, 3 filters
// each.  NPL > 0: nfft == 64 * NPL and nf <= 12 -- every lane's kernel taps are fetched into registers once, before the
// span barrier, and reused for the 8 frames (one frame per workgroup spent ~4 us of latency per 256-tap dot product).
struct CqtOctaves {                     // one entry per octave of the launch (blockIdx.z)
  const float* y[AST_CQT_MAX_OCTAVES];  // the octave's (halved) signals, B rows of n[o] floats
  int n[AST_CQT_MAX_OCTAVES], hop[AST_CQT_MAX_OCTAVES], lo[AST_CQT_MAX_OCTAVES], nf[AST_CQT_MAX_OCTAVES], row0[AST_CQT_MAX_OCTAVES];
};

// `n_row`: the width of the rows at octave blockIdx.z, oc.n[o]; `n`: the samples of row blockIdx.y that count.
// cqt_octave_kernel passes the row's width for both, cqt_octave_len_kernel the clip's own count after o halvings for `n`.
template <int NPL>
__device__ __forceinline__ void cqt_octave_body(const CqtOctaves& oc, const float* __restrict__ w_re_all,
                                                const float* __restrict__ w_im_all, const float* __restrict__ scale_all, const int nfft,
                                                float* __restrict__ out, const int T, const int ld, const int bin_off, const int n_row,
                                                const int n) {
  const int o = blockIdx.z;
  const float* __restrict__ y = oc.y[o];
  const int hop = oc.hop[o], nf = oc.nf[o], bin0 = bin_off + oc.lo[o];
  const long y_stride = n_row;
  const float* __restrict__ w_re = w_re_all + (size_t)oc.row0[o] * nfft;
  const float* __restrict__ w_im = w_im_all + (size_t)oc.row0[o] * nfft;
  const float* __restrict__ scale = scale_all + oc.lo[o];
  extern __shared__ float span[];                                // the samples of FR consecutive frames
  const int t0 = blockIdx.x * AST_CQT_FR, b = blockIdx.y;
  const float* yb = y + (size_t)b * y_stride;
  const int start = t0 * hop - nfft / 2;
  const int nfr = min(AST_CQT_FR, T - t0);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  constexpr int NR = NPL > 0 ? NPL : 1;
  float wr[3][NR], wi[3][NR];
  if (NPL > 0) {
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      const int k = min(wave + 4 * f, nf - 1);
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        wr[f][i] = w_re[(size_t)k * nfft + lane + 64 * i];
        wi[f][i] = w_im[(size_t)k * nfft + lane + 64 * i];
      }
    }
  }
  const int nspan = (nfr - 1) * hop + nfft;
  for (int i = threadIdx.x; i < nspan; i += 256) {
    const int s = start + i;
    span[i] = (s >= 0 && s < n) ? yb[s] : 0.0f;
  }
  __syncthreads();
  if constexpr (NPL > 0) {
    // 8 frames x 3 filters x (re, im) = 48 per-lane partial sums.  Three transposed reductions of 16 values each
    // (row16_transpose_sum: lane l of a 16-lane row ends with the row's sum of value l), two cross-row exchanges, and
    // lanes 0..15 store one result each -- instead of 48 separate wave sums (which made the kernel VALU-issue bound).
    static_assert(AST_CQT_FR * 6 == 48, "three groups of sixteen");
    float part[AST_CQT_FR * 6];
#pragma unroll
    for (int fr = 0; fr < AST_CQT_FR; ++fr) {
      const float* frame = span + fr * hop;                            // frames past nfr read stale LDS: never stored
      float fv[NR];
#pragma unroll
      for (int i = 0; i < NR; ++i) fv[i] = frame[lane + 64 * i];
#pragma unroll
      for (int f = 0; f < 3; ++f) {
        float re = 0.0f, im = 0.0f;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          re = __builtin_fmaf(fv[i], wr[f][i], re);
          im = __builtin_fmaf(fv[i], wi[f][i], im);
        }
        part[fr * 6 + f * 2] = re;
        part[fr * 6 + f * 2 + 1] = im;
      }
    }
    const int l = lane & 15;
#pragma unroll
    for (int grp = 0; grp < 3; ++grp) {
      float v[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) v[q] = part[grp * 16 + q];
      float val = row16_transpose_sum(v, l);
      val += __shfl_xor(val, 16);
      val += __shfl_xor(val, 32);
      const int q = grp * 16 + l, fr = q / 6, f = (q - fr * 6) >> 1, c = q & 1;
      const int k = wave + 4 * f, t = t0 + fr;
      if (lane < 16 && fr < nfr && k < nf)
        out[((size_t)b * 2 * T + (size_t)c * T + t) * ld + bin0 + k] = val * scale[k];   // (B, 2, T, ld): real plane, then imaginary
    }
  } else {
    for (int fr = 0; fr < nfr; ++fr) {
      const float* frame = span + fr * hop;
      const int t = t0 + fr;
      for (int k = wave; k < nf; k += 4) {
        float re = 0.0f, im = 0.0f;
        const float* pr = w_re + (size_t)k * nfft;
        const float* pi = w_im + (size_t)k * nfft;
        for (int i = lane; i < nfft; i += 64) {
          const float v = frame[i];
          re = __builtin_fmaf(v, pr[i], re);
          im = __builtin_fmaf(v, pi[i], im);
        }
        re = wave_sum_dpp(re);
        im = wave_sum_dpp(im);
        if (lane == 0) {
          float* op = out + ((size_t)b * 2 * T + t) * ld + bin0 + k;
          op[0] = re * scale[k];
          op[(size_t)T * ld] = im * scale[k];
        }
      }
    }
  }
}
template <int NPL>
__global__ __launch_bounds__(256) void cqt_octave_kernel(const CqtOctaves oc, const float* __restrict__ w_re_all,
                                                         const float* __restrict__ w_im_all, const float* __restrict__ scale_all,
                                                         const int nfft, float* __restrict__ out, const int T, const int ld, const int bin_off) {
  const int n = oc.n[blockIdx.z];
  cqt_octave_body<NPL>(oc, w_re_all, w_im_all, scale_all, nfft, out, T, ld, bin_off, n, n);
}
template <int NPL>
__global__ __launch_bounds__(256) void cqt_octave_len_kernel(const CqtOctaves oc, const float* __restrict__ w_re_all,
                                                             const float* __restrict__ w_im_all, const float* __restrict__ scale_all,
                                                             const int nfft, float* __restrict__ out, const int T, const int ld, const int bin_off,
                                                             const int32_t* __restrict__ n_samples, const int nsamp, const int win,
                                                             const int step) {
  const int o = blockIdx.z, n = oc.n[o];
  cqt_octave_body<NPL>(oc, w_re_all, w_im_all, scale_all, nfft, out, T, ld, bin_off, n,
                       min(n, ast_halved(ast_clip_len(n_samples[blockIdx.y], nsamp, win, step).ns, o)));
}

// y[b][i*nnew + p] = gain * sum_k kern[p][k] * x[b][i*orig + k - width]   (x = 0 outside [0, n)); any ratio.
// One thread per output; its taps are a serial chain of load pairs, so eight independent accumulators keep eight
// pairs in flight.  (Splitting one output's taps over 8 lanes was 3x slower: it turns the broadcast tap loads and the
// stride-`orig` signal loads into scattered ones and the kernel becomes L1-throughput bound.)
__global__ __launch_bounds__(256) void resample_poly_kernel(const float* __restrict__ x, const int n, const float* __restrict__ kern,
                                                            const int orig, const int nnew, const int klen, const int width,
                                                            float* __restrict__ y, const int m, const float gain) {
  const int b = blockIdx.y;
  const float* xb = x + (size_t)b * n;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < m; j += gridDim.x * 256) {
    const int i = j / nnew, p = j - i * nnew;
    const float* kp = kern + (size_t)p * klen;
    const int s0 = i * orig - width;
    const int k0 = s0 < 0 ? -s0 : 0, k1 = min(klen, n - s0);
    const float* xs = xb + s0;
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int k = k0;
    for (; k + 8 <= k1; k += 8) {
      float kv[8], xv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { kv[u] = kp[k + u]; xv[u] = xs[k + u]; }
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] = __builtin_fmaf(kv[u], xv[u], a[u]);
    }
    for (; k < k1; ++k) a[0] = __builtin_fmaf(kp[k], xs[k], a[0]);
    y[(size_t)b * m + j] = (((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))) * gain;
  }
}

// The 2:1 case (the six halvings of a CQT, 44.1 -> 22.05 kHz in load_audio): y[j] = gain * sum_k h[k] x[2j + k - width].
// A workgroup stages its input span in LDS split into even and odd samples, so that for a fixed tap the 64 lanes of
// a wave (64 consecutive outputs) read 64 consecutive words -- conflict-free -- and the tap itself is wave-uniform
// (an LDS broadcast).  R outputs per thread (j, j+256, ...) share each tap.  8 x 44100 outputs x 359 taps: 151 -> ~10 us.
// `nb`: input sample s of row blockIdx.y counts iff s < nb.  decimate2_kernel passes the row's width n, decimate2_len_kernel
// (halving level o) the clip's ceil(ns_b / 2^o).
// EPI (decimate2_clip_kernel): 1 writes 0 for j >= mb, the clip's own output count; 2 also replaces what y holds (the first
// channel) by the mean of that and this channel.  Neither touches the sum itself.
template <int R, int EPI = 0>
__device__ __forceinline__ void decimate2_body(const float* __restrict__ x, const int n, const float* __restrict__ h, const int klen,
                                               const int width, float* __restrict__ y, const int m, const float gain, const int nb,
                                               const int mb = 0) {
  extern __shared__ float sm[];
  const int b = blockIdx.y, t = threadIdx.x;
  const float* xb = x + (size_t)b * n;
  const int j0 = blockIdx.x * (256 * R);
  const int ne = 256 * R + (klen + 1) / 2;                    // even (and odd) samples the tile needs
  float* xe = sm;
  float* xo = sm + ne;
  float* hs = sm + 2 * ne;                                     // taps: LDS broadcast reads, one latency class with the samples
  for (int i = t; i < klen; i += 256) hs[i] = h[i];
  const int base = 2 * j0 - width;
  for (int i = t; i < 2 * ne; i += 256) {
    const int s = base + i;
    const float v = (s >= 0 && s < nb) ? xb[s] : 0.0f;
    ((i & 1) ? xo : xe)[i >> 1] = v;
  }
  __syncthreads();
  float acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.0f;
  const int pairs = klen >> 1;
#pragma unroll 8
  for (int k2 = 0; k2 < pairs; ++k2) {
    const float h0 = hs[2 * k2], h1 = hs[2 * k2 + 1];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      acc[r] = __builtin_fmaf(h0, xe[t + 256 * r + k2], acc[r]);
      acc[r] = __builtin_fmaf(h1, xo[t + 256 * r + k2], acc[r]);
    }
  }
  if (klen & 1) {
    const float h0 = hs[klen - 1];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = __builtin_fmaf(h0, xe[t + 256 * r + pairs], acc[r]);
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int j = j0 + t + 256 * r;
    if (EPI == 0) {
      if (j < m) y[(size_t)b * m + j] = acc[r] * gain;
    } else if (j < m) {
#pragma clang fp contract(off)                                  // the mean adds two rounded products: no fma
      float v = acc[r] * gain;
      if (EPI == 2) v = (y[(size_t)b * m + j] + v) * 0.5f;
      y[(size_t)b * m + j] = j < mb ? v : 0.0f;
    }
  }
}
template <int R>
__global__ __launch_bounds__(256) void decimate2_kernel(const float* __restrict__ x, const int n, const float* __restrict__ h, const int klen,
                                                        const int width, float* __restrict__ y, const int m, const float gain) {
  decimate2_body<R>(x, n, h, klen, width, y, m, gain, n);
}
template <int R>
__global__ __launch_bounds__(256) void decimate2_len_kernel(const float* __restrict__ x, const int n, const float* __restrict__ h,
                                                            const int klen, const int width, float* __restrict__ y, const int m,
                                                            const float gain, const int32_t* __restrict__ n_samples, const int nsamp,
                                                            const int win, const int step, const int o) {
  decimate2_body<R>(x, n, h, klen, width, y, m, gain, min(n, ast_halved(ast_clip_len(n_samples[blockIdx.y], nsamp, win, step).ns, o)));
}

// ---- load_audio's resample + stereo mean for a padded batch of clips at their native rate (ast_resample_poly_len):
// x (B, C, n), clip b holds nb = n_in[b] samples per channel (clamped to [1, n]; all n without n_in) and comes out as the
// mb = ceil(nb * nnew / orig) samples it gives alone, 0 behind them.  Samples s >= nb are never read.
#define AST_RS_THREADS 512                // 8 waves: two per SIMD
#define AST_RS_P 4                        // phases a wave runs per pass over its rows' samples
#define AST_RS_MAX_PITCH 640              // 64 rows x 640 floats = the 160 KiB of LDS

__device__ __forceinline__ int resample_clip_n(const int32_t* __restrict__ n_in, const int b, const int n) {
  return n_in ? min(max(n_in[b], 1), n) : n;
}
__device__ __forceinline__ int resample_clip_m(const int nb, const int orig, const int nnew) {
  return (int)(((long long)nb * nnew + orig - 1) / orig);
}

// The 2:1 case: decimate2_body on channel `x` of every clip (row pitch `ld` = C * n), its outputs past mb zeroed.  AVG: the
// second channel's launch, y becomes the mean of what the first wrote and this one.  A tile wholly past mb leaves before the
// body's barrier (the first launch stores its zeros, the second finds them).
template <int R, bool AVG>
__global__ __launch_bounds__(256) void decimate2_clip_kernel(const float* __restrict__ x, const int ld, const int n,
                                                             const float* __restrict__ h, const int klen, const int width,
                                                             float* __restrict__ y, const int m, const float gain,
                                                             const int32_t* __restrict__ n_in, int32_t* __restrict__ n_out) {
  const int b = blockIdx.y;
  const int nb = resample_clip_n(n_in, b, n), mb = resample_clip_m(nb, 2, 1);
  if (!AVG && n_out && blockIdx.x == 0 && threadIdx.x == 0) n_out[b] = mb;
  const int j0 = blockIdx.x * (256 * R);
  if (j0 >= mb) {
    if (!AVG) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int j = j0 + threadIdx.x + 256 * r;
        if (j < m) y[(size_t)b * m + j] = 0.0f;
      }
    }
    return;
  }
  decimate2_body<R, AVG ? 2 : 1>(x, ld, h, klen, width, y, m, gain, nb, mb);
}

// resample_poly_kernel's sum for P phases of one polyphase row i: a[q][(k - k0) mod 8] over k0 <= k < k1, the scalar tail into
// a[q][0], the same tree.  xs[k] = x[i * orig - width + k] (LDS, or global in the unstaged kernel), kp = kern + p0 * klen.
// UNI: k0 = 0 and k1 = klen for the whole wave, so k and the tap addresses are wave-uniform (scalar loads) and xs, a row of
// even pitch, is read as 8-byte pairs.
template <bool UNI, int P, typename XP>
__device__ __forceinline__ void resample_rows(XP xs, const float* __restrict__ kp, const int klen, const int k0, const int k1,
                                              float (&out)[P]) {
  const int kb = UNI ? 0 : k0, ke = UNI ? klen : k1;
  float a[P][8];
#pragma unroll
  for (int q = 0; q < P; ++q)
#pragma unroll
    for (int u = 0; u < 8; ++u) a[q][u] = 0.f;
  int k = kb;
  for (; k + 8 <= ke; k += 8) {
    float xv[8];
    if (UNI) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const f32x2 v = *reinterpret_cast<const f32x2*>(&xs[k + 2 * u]);
        xv[2 * u] = v[0]; xv[2 * u + 1] = v[1];
      }
    } else {
#pragma unroll
      for (int u = 0; u < 8; ++u) xv[u] = xs[k + u];
    }
#pragma unroll
    for (int q = 0; q < P; ++q) {
      float kv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) kv[u] = kp[(size_t)q * klen + k + u];
#pragma unroll
      for (int u = 0; u < 8; ++u) a[q][u] = __builtin_fmaf(kv[u], xv[u], a[q][u]);
    }
  }
  for (; k < ke; ++k) {
    const float xv = xs[k];
#pragma unroll
    for (int q = 0; q < P; ++q) a[q][0] = __builtin_fmaf(kp[(size_t)q * klen + k], xv, a[q][0]);
  }
#pragma unroll
  for (int q = 0; q < P; ++q) out[q] = ((a[q][0] + a[q][1]) + (a[q][2] + a[q][3])) + ((a[q][4] + a[q][5]) + (a[q][6] + a[q][7]));
}

// Any other ratio, staged.  A workgroup owns TI = 64 / C consecutive polyphase rows i of one clip, i.e. the TI * nnew
// consecutive outputs j = i * nnew + p.  Output (i, p) reads x[i * orig - width + k], k < klen, whatever p is: lane l of every
// wave keeps row l of an LDS image -- its own klen samples, zero-filled outside [0, nb) -- at a pitch of 2 mod 4 floats (8-byte
// aligned rows on 32 distinct bank pairs per half wave: conflict-free ds_read_b64).  C = 2: rows 0..31 are channel 0 and rows
// 32..63 channel 1 of the same 32 i, and the two halves of the wave swap their results for the mean.  The waves share out the
// phases, AST_RS_P at a time: all 64 lanes of a wave are at one phase, so a tap is one scalar load for the wave (the bank,
// 147 x 348 floats at 48 kHz, stays in L2), and a sample pair read from LDS serves AST_RS_P phases.
template <int C>
__global__ __launch_bounds__(AST_RS_THREADS) void resample_poly_len_kernel(const float* __restrict__ x, const int n,
                                                                           const float* __restrict__ kern, const int orig, const int nnew,
                                                                           const int klen, const int width, const int pitch,
                                                                           float* __restrict__ y, const int m, const float gain,
                                                                           const int32_t* __restrict__ n_in, int32_t* __restrict__ n_out) {
#pragma clang fp contract(off)                                  // the sums are explicit fmas; the mean adds two rounded products
  extern __shared__ f32x2 rs_sm[];                              // 8-byte aligned: the rows are read as pairs
  float* sm = reinterpret_cast<float*>(rs_sm);
  constexpr int TI = 64 / C;
  const int b = blockIdx.y, t = threadIdx.x, lane = t & 63;
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int nb = resample_clip_n(n_in, b, n), mb = resample_clip_m(nb, orig, nnew);
  if (n_out && blockIdx.x == 0 && t == 0) n_out[b] = mb;
  const int i0 = blockIdx.x * TI;
  const long long j0 = (long long)i0 * nnew;
  float* yb = y + (size_t)b * m;
  if (j0 >= mb) {                                               // workgroup-uniform: a tile behind the clip's end stores zeros
    const int je = (int)min((long long)m - j0, (long long)TI * nnew);
    for (int j = t; j < je; j += AST_RS_THREADS) yb[j0 + j] = 0.0f;
    return;
  }
  for (int r = wv; r < 64; r += AST_RS_THREADS / 64) {
    const int c = C == 2 ? r >> 5 : 0;
    const int s0 = (i0 + (C == 2 ? r & 31 : r)) * orig - width;
    const float* xr = x + ((size_t)b * C + c) * n;
    float* row = sm + r * pitch;
    for (int k = lane; k < klen; k += 64) {
      const int s = s0 + k;
      row[k] = (s >= 0 && s < nb) ? xr[s] : 0.0f;
    }
  }
  __syncthreads();
  const int i = i0 + (C == 2 ? lane & 31 : lane);
  const long long jb = (long long)i * nnew;
  const int s0 = i * orig - width;
  const bool live = jb < mb;
  const int k0 = live ? max(-s0, 0) : 0, k1 = live ? min(klen, nb - s0) : 0;
  const bool uni = __all(k0 == 0 && k1 == klen);
  const float* row = sm + lane * pitch;
  auto store = [&](const int p, const float sum) {
#pragma clang fp contract(off)
    float v = sum * gain;
    if (C == 2) v = (v + __shfl_xor(v, 32)) * 0.5f;
    const long long j = jb + p;
    if ((C == 1 || lane < 32) && j < m) yb[j] = j < mb ? v : 0.0f;
  };
  const int ngroups = nnew / AST_RS_P;
  for (int g = wv; g < ngroups; g += AST_RS_THREADS / 64) {
    const float* kp = kern + (size_t)g * AST_RS_P * klen;
    float r[AST_RS_P];
    if (uni)
      resample_rows<true, AST_RS_P>(row, kp, klen, 0, klen, r);
    else
      resample_rows<false, AST_RS_P>(row, kp, klen, k0, k1, r);
#pragma unroll
    for (int q = 0; q < AST_RS_P; ++q) store(g * AST_RS_P + q, r[q]);
  }
  for (int p = ngroups * AST_RS_P + wv; p < nnew; p += AST_RS_THREADS / 64) {
    float r[1];
    if (uni)
      resample_rows<true, 1>(row, kern + (size_t)p * klen, klen, 0, klen, r);
    else
      resample_rows<false, 1>(row, kern + (size_t)p * klen, klen, k0, k1, r);
    store(p, r[0]);
  }
}

// The same entry where a row of klen samples per lane does not fit in LDS (klen > AST_RS_MAX_PITCH: 96 kHz -> 22.05 kHz has
// 694 taps): resample_poly_kernel's one thread per output on the clip's own counts.
template <int C>
__global__ __launch_bounds__(256) void resample_poly_len_direct_kernel(const float* __restrict__ x, const int n,
                                                                       const float* __restrict__ kern, const int orig, const int nnew,
                                                                       const int klen, const int width, float* __restrict__ y, const int m,
                                                                       const float gain, const int32_t* __restrict__ n_in,
                                                                       int32_t* __restrict__ n_out) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const int nb = resample_clip_n(n_in, b, n), mb = resample_clip_m(nb, orig, nnew);
  if (n_out && blockIdx.x == 0 && threadIdx.x == 0) n_out[b] = mb;
  const float* xb = x + (size_t)b * C * n;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < m; j += gridDim.x * 256) {
    float v = 0.0f;
    if (j < mb) {
      const int i = j / nnew, p = j - i * nnew;
      const int s0 = i * orig - width;
      const int k0 = s0 < 0 ? -s0 : 0, k1 = min(klen, nb - s0);
      float r[1];
      resample_rows<false, 1>(xb + s0, kern + (size_t)p * klen, klen, k0, k1, r);
      v = r[0] * gain;
      if (C == 2) {
        resample_rows<false, 1>(xb + n + s0, kern + (size_t)p * klen, klen, k0, k1, r);
        v = (v + r[0] * gain) * 0.5f;
      }
    }
    y[(size_t)b * m + j] = v;
  }
}

// z-score + overlap windows of the CQT planes into the bins behind the STFT's (dataloader.py:9-18,
// utilityFunctions.py:240-263): x[b][s][c][w][bin0 + k] = (cqt[b][c][s*step + w][k] - mean[c][k]) / (std[c][k] + 1e-8),
// 0 past the last frame (the zero-padded tail window).  LEN (cqt_sections_len_kernel): 0 as well for t >= T_b and for
// s >= n_sec_b, the clip's own frame and section counts; cqt_sections_kernel passes no lengths.
template <bool LEN>
__device__ __forceinline__ void cqt_sections_body(const float* __restrict__ cqt, const int T, const int nb, const float* __restrict__ mean,
                                                  const float* __restrict__ std_, float* __restrict__ x, const int S, const int win,
                                                  const int step, const int F_total, const int bin0, const size_t total,
                                                  const int32_t* __restrict__ n_samples, const int nsamp) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int k = (int)(i % nb);
    size_t r = i / nb;
    const int w = (int)(r % win); r /= win;
    const int c = (int)(r & 1); r >>= 1;
    const int s = (int)(r % S);
    const size_t b = r / S;
    const int t = s * step + w;
    bool live = t < T;
    if (LEN) {
      const AstClipLen L = ast_clip_len(n_samples[b], nsamp, win, step);
      live = t < min(T, L.T) && s < L.n_sec;
    }
    float v = 0.0f;
    if (live) v = (cqt[((b * 2 + c) * T + t) * nb + k] - mean[c * nb + k]) / (std_[c * nb + k] + 1e-8f);
    x[((((b * S + s) * 2 + c) * win + w) * (size_t)F_total) + bin0 + k] = v;
  }
}
__global__ __launch_bounds__(256) void cqt_sections_kernel(const float* __restrict__ cqt, const int T, const int nb,
                                                           const float* __restrict__ mean, const float* __restrict__ std_,
                                                           float* __restrict__ x, const int S, const int win, const int step,
                                                           const int F_total, const int bin0, const size_t total) {
  cqt_sections_body<false>(cqt, T, nb, mean, std_, x, S, win, step, F_total, bin0, total, nullptr, 0);
}
__global__ __launch_bounds__(256) void cqt_sections_len_kernel(const float* __restrict__ cqt, const int T, const int nb,
                                                               const float* __restrict__ mean, const float* __restrict__ std_,
                                                               float* __restrict__ x, const int S, const int win, const int step,
                                                               const int F_total, const int bin0, const size_t total,
                                                               const int32_t* __restrict__ n_samples, const int nsamp) {
  cqt_sections_body<true>(cqt, T, nb, mean, std_, x, S, win, step, F_total, bin0, total, n_samples, nsamp);
}

// ---- host side: one launcher per operation, behind the entry for equal clips (len == nullptr) and its _len twin
struct LenArgs {                       // what a _len entry adds: the device lengths and the padded row they are clamped to
  const int32_t* n_samples;
  int nsamp, win, step;
};

int len_args_check(const char* name, const LenArgs& a) {
  if (!a.n_samples) AST_FAIL("%s: n_samples is NULL (equal clips: the entry without _len)", name);
  if (!ast_sectioning_ok(a.win, a.step)) AST_FAIL("%s: bad sectioning (win=%d step=%d)", name, a.win, a.step);
  return ast_row_check(name, a.nsamp, a.win);
}

int cqt_sections_launch(const char* name, const float* cqt, int Bc, int T, int nb, const float* mean, const float* std_, float* x, int S,
                        int win, int step, int F_total, int bin0, const LenArgs* len, void* stream) {
  if (!cqt || !mean || !std_ || !x) AST_FAIL("%s: null pointer", name);
  if (Bc < 1 || T < 1 || nb < 1 || S < 1 || win < 1 || step < 1 || bin0 < 0 || bin0 + nb > F_total)
    AST_FAIL("%s: bad shape (Bc=%d T=%d nb=%d S=%d win=%d step=%d F=%d bin0=%d)", name, Bc, T, nb, S, win, step, F_total, bin0);
  if (len) {
    if (len_args_check(name, *len)) return -1;
    if (T != 1 + len->nsamp / AST_FE_HOP) AST_FAIL("%s: bad shape (T=%d is not 1 + nsamp / 256 at nsamp=%d)", name, T, len->nsamp);
  }
  const size_t total = (size_t)Bc * S * 2 * win * nb;
  const dim3 grid((unsigned)std::min<size_t>((total + 255) / 256, 4096));
  if (len)
    hipLaunchKernelGGL(cqt_sections_len_kernel, grid, dim3(256), 0, (hipStream_t)stream, cqt, T, nb, mean, std_, x, S, win, step, F_total, bin0,
                       total, len->n_samples, len->nsamp);
  else
    hipLaunchKernelGGL(cqt_sections_kernel, grid, dim3(256), 0, (hipStream_t)stream, cqt, T, nb, mean, std_, x, S, win, step, F_total, bin0, total);
  AST_CHECK_LAUNCH();
  return 0;
}

int cqt_octaves_launch(const char* name, const float* const* ys, const int* ns, const int* hops, const int* los, const int* nfs,
                       const int* row0s, int n_oct, int B, const float* w_re, const float* w_im, const float* scale, int nfft, float* out, int T,
                       int ld, int bin_off, const LenArgs* len, void* stream) {
  if (!ys || !ns || !hops || !los || !nfs || !row0s || !w_re || !w_im || !scale || !out) AST_FAIL("%s: null pointer", name);
  if (n_oct < 1 || n_oct > AST_CQT_MAX_OCTAVES || B < 1 || B > 65535 || nfft < 2 || nfft > 8192 || (nfft & 1) || T < 1 || bin_off < 0)
    AST_FAIL("%s: bad shape (n_oct=%d B=%d nfft=%d T=%d)", name, n_oct, B, nfft, T);
  if (len && len_args_check(name, *len)) return -1;
  CqtOctaves oc;
  bool fast = nfft == 256;
  int hop_max = 1;
  for (int o = 0; o < n_oct; ++o) {
    if (!ys[o] || ns[o] < 1 || hops[o] < 1 || los[o] < 0 || nfs[o] < 1 || row0s[o] < 0 || bin_off + los[o] + nfs[o] > ld)
      AST_FAIL("%s: bad octave %d (n=%d hop=%d lo=%d nf=%d row0=%d ld=%d)", name, o, ns[o], hops[o], los[o], nfs[o], row0s[o], ld);
    if (len && ns[o] != ast_halved(len->nsamp, o))
      AST_FAIL("%s: bad octave %d (n=%d is not nsamp=%d halved %d times)", name, o, ns[o], len->nsamp, o);
    oc.y[o] = ys[o]; oc.n[o] = ns[o]; oc.hop[o] = hops[o]; oc.lo[o] = los[o]; oc.nf[o] = nfs[o]; oc.row0[o] = row0s[o];
    fast = fast && nfs[o] <= 12;
    hop_max = std::max(hop_max, hops[o]);
  }
  const size_t lds = ((size_t)(AST_CQT_FR - 1) * hop_max + nfft) * sizeof(float);
  if (lds > 64 * 1024) AST_FAIL("%s: hop %d x %d frames + nfft %d exceeds the LDS span", name, hop_max, AST_CQT_FR, nfft);
  const dim3 grid((T + AST_CQT_FR - 1) / AST_CQT_FR, B, n_oct);
  const hipStream_t s = (hipStream_t)stream;
  if (len) {
    const auto kern = fast ? cqt_octave_len_kernel<4> : cqt_octave_len_kernel<0>;
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, oc, w_re, w_im, scale, nfft, out, T, ld, bin_off, len->n_samples, len->nsamp, len->win,
                       len->step);
  } else {
    const auto kern = fast ? cqt_octave_kernel<4> : cqt_octave_kernel<0>;
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, oc, w_re, w_im, scale, nfft, out, T, ld, bin_off);
  }
  AST_CHECK_LAUNCH();
  return 0;
}

// the 2:1 FIR on checked arguments (klen <= 4096): R = 4 outputs per thread from 256 Ki outputs on, else 1
template <int R>
void decimate2_launch_r(const float* x, int B, int n, const float* h, int klen, int width, float* y, int m, float gain, const LenArgs* len, int o,
                        hipStream_t s) {
  const size_t lds = (2 * (size_t)(256 * R + (klen + 1) / 2) + klen) * sizeof(float);
  const dim3 grid((m + 256 * R - 1) / (256 * R), B);
  if (len)
    hipLaunchKernelGGL(decimate2_len_kernel<R>, grid, dim3(256), lds, s, x, n, h, klen, width, y, m, gain, len->n_samples, len->nsamp, len->win,
                       len->step, o);
  else
    hipLaunchKernelGGL(decimate2_kernel<R>, grid, dim3(256), lds, s, x, n, h, klen, width, y, m, gain);
}
int decimate2_launch(const float* x, int B, int n, const float* h, int klen, int width, float* y, int m, float gain, const LenArgs* len, int o,
                     void* stream) {
  if ((long)m * B >= 256 * 1024)
    decimate2_launch_r<4>(x, B, n, h, klen, width, y, m, gain, len, o, (hipStream_t)stream);
  else
    decimate2_launch_r<1>(x, B, n, h, klen, width, y, m, gain, len, o, (hipStream_t)stream);
  AST_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int ast_cqt_sections(const float* cqt, int Bc, int T, int nb, const float* mean, const float* std_, float* x, int S, int win,
                                int step, int F_total, int bin0, void* stream) {
  return cqt_sections_launch("ast_cqt_sections", cqt, Bc, T, nb, mean, std_, x, S, win, step, F_total, bin0, nullptr, stream);
}

extern "C" int ast_cqt_sections_len(const float* cqt, int Bc, int T, int nb, const float* mean, const float* std_, float* x, int S, int win,
                                    int step, int F_total, int bin0, const int32_t* n_samples, int nsamp, void* stream) {
  const LenArgs len = {n_samples, nsamp, win, step};
  return cqt_sections_launch("ast_cqt_sections_len", cqt, Bc, T, nb, mean, std_, x, S, win, step, F_total, bin0, &len, stream);
}

extern "C" int ast_cqt_octaves(const float* const* ys, const int* ns, const int* hops, const int* los, const int* nfs, const int* row0s,
                               int n_oct, int B, const float* w_re, const float* w_im, const float* scale, int nfft, float* out, int T,
                               int ld, int bin_off, void* stream) {
  return cqt_octaves_launch("ast_cqt_octaves", ys, ns, hops, los, nfs, row0s, n_oct, B, w_re, w_im, scale, nfft, out, T, ld, bin_off, nullptr,
                            stream);
}

extern "C" int ast_cqt_octaves_len(const float* const* ys, const int* ns, const int* hops, const int* los, const int* nfs, const int* row0s,
                                   int n_oct, int B, const float* w_re, const float* w_im, const float* scale, int nfft, float* out, int T,
                                   int ld, int bin_off, const int32_t* n_samples, int nsamp, int win, int step, void* stream) {
  const LenArgs len = {n_samples, nsamp, win, step};
  return cqt_octaves_launch("ast_cqt_octaves_len", ys, ns, hops, los, nfs, row0s, n_oct, B, w_re, w_im, scale, nfft, out, T, ld, bin_off, &len,
                            stream);
}

extern "C" int ast_resample_poly(const float* x, int B, int n, const float* kern, int orig, int nnew, int klen, int width, float* y, int m,
                                 float gain, void* stream) {
  if (!x || !kern || !y) AST_FAIL("ast_resample_poly: null pointer");
  if (B < 1 || B > 65535 || n < 1 || orig < 1 || nnew < 1 || klen < 1 || width < 0 || m < 1)
    AST_FAIL("ast_resample_poly: bad shape (B=%d n=%d orig=%d new=%d klen=%d width=%d m=%d)", B, n, orig, nnew, klen, width, m);
  // every output must come from a polyphase row that exists: j/nnew*orig stays an int
  if ((long)((m - 1) / nnew) * orig + klen >= (1L << 31)) AST_FAIL("ast_resample_poly: signal too long");
  if (orig == 2 && nnew == 1 && klen <= 4096) return decimate2_launch(x, B, n, kern, klen, width, y, m, gain, nullptr, 0, stream);
  hipLaunchKernelGGL(resample_poly_kernel, dim3(std::min((m + 255) / 256, 4096), B), dim3(256), 0, (hipStream_t)stream, x, n, kern, orig, nnew,
                     klen, width, y, m, gain);
  AST_CHECK_LAUNCH();
  return 0;
}

namespace {
template <int R>
void decimate2_clip_launch(const float* x, int B, int C, int n, const float* h, int klen, int width, float* y, int m, float gain,
                           const int32_t* n_in, int32_t* n_out, hipStream_t s) {
  const size_t lds = (2 * (size_t)(256 * R + (klen + 1) / 2) + klen) * sizeof(float);
  const dim3 grid((m + 256 * R - 1) / (256 * R), B);
  hipLaunchKernelGGL((decimate2_clip_kernel<R, false>), grid, dim3(256), lds, s, x, C * n, n, h, klen, width, y, m, gain, n_in, n_out);
  if (C == 2)
    hipLaunchKernelGGL((decimate2_clip_kernel<R, true>), grid, dim3(256), lds, s, x + n, C * n, n, h, klen, width, y, m, gain, n_in, n_out);
}
}  // namespace

extern "C" int ast_resample_poly_len(const float* x, int B, int C, int n, const float* kern, int orig, int nnew, int klen, int width,
                                     float* y, int m, float gain, const int32_t* n_in, int32_t* n_out, void* stream) {
  if (!x || !kern || !y) AST_FAIL("ast_resample_poly_len: null pointer");
  if (B < 1 || B > 65535 || n < 1 || orig < 1 || nnew < 1 || klen < 1 || width < 0 || m < 1)
    AST_FAIL("ast_resample_poly_len: bad shape (B=%d n=%d orig=%d new=%d klen=%d width=%d m=%d)", B, n, orig, nnew, klen, width, m);
  if (C != 1 && C != 2) AST_FAIL("ast_resample_poly_len: bad shape (C=%d: one or two channels)", C);
  // n * nnew is the numerator of every clip's output count, C * n the pitch of a clip; row i starts at i * orig - width and
  // the last tile's rows run up to 64 past the last output's
  if ((long)n * nnew >= (1L << 31) || (long)C * n >= (1L << 31) || (long)n + 66L * orig + klen >= (1L << 31))
    AST_FAIL("ast_resample_poly_len: signal too long (n=%d orig=%d new=%d)", n, orig, nnew);
  if ((long)m != ((long)n * nnew + orig - 1) / orig)
    AST_FAIL("ast_resample_poly_len: bad shape (m=%d is not ceil(n * new / orig) at n=%d orig=%d new=%d)", m, n, orig, nnew);
  if ((long)((m - 1) / nnew) * orig + klen >= (1L << 31)) AST_FAIL("ast_resample_poly_len: signal too long");
  const hipStream_t s = (hipStream_t)stream;
  if (orig == 2 && nnew == 1 && klen <= 4096) {
    if ((long)m * B >= 256 * 1024)
      decimate2_clip_launch<4>(x, B, C, n, kern, klen, width, y, m, gain, n_in, n_out, s);
    else
      decimate2_clip_launch<1>(x, B, C, n, kern, klen, width, y, m, gain, n_in, n_out, s);
    AST_CHECK_LAUNCH();
    return 0;
  }
  const int pitch = ((klen + 1) & ~3) + 2;                      // the smallest count >= klen that is 2 mod 4
  if (pitch > AST_RS_MAX_PITCH) {
    const dim3 grid(std::min((m + 255) / 256, 4096), B);
    if (C == 2)
      hipLaunchKernelGGL(resample_poly_len_direct_kernel<2>, grid, dim3(256), 0, s, x, n, kern, orig, nnew, klen, width, y, m, gain, n_in, n_out);
    else
      hipLaunchKernelGGL(resample_poly_len_direct_kernel<1>, grid, dim3(256), 0, s, x, n, kern, orig, nnew, klen, width, y, m, gain, n_in, n_out);
    AST_CHECK_LAUNCH();
    return 0;
  }
  const int lds = 64 * pitch * (int)sizeof(float);
  static LdsAttrOnce attr;
  if (attr.set(64 * AST_RS_MAX_PITCH * (int)sizeof(float),
               {(const void*)resample_poly_len_kernel<1>, (const void*)resample_poly_len_kernel<2>}))
    return -3;
  const int tile = (64 / C) * nnew;                             // outputs per workgroup
  const dim3 grid((unsigned)(((long)m + tile - 1) / tile), B);
  if (C == 2)
    hipLaunchKernelGGL(resample_poly_len_kernel<2>, grid, dim3(AST_RS_THREADS), lds, s, x, n, kern, orig, nnew, klen, width, pitch, y, m, gain,
                       n_in, n_out);
  else
    hipLaunchKernelGGL(resample_poly_len_kernel<1>, grid, dim3(AST_RS_THREADS), lds, s, x, n, kern, orig, nnew, klen, width, pitch, y, m, gain,
                       n_in, n_out);
  AST_CHECK_LAUNCH();
  return 0;
}

extern "C" int ast_decimate2_len(const float* x, int B, int n, const float* h, int klen, int width, float* y, int m, float gain,
                                 const int32_t* n_samples, int nsamp, int win, int step, int o, void* stream) {
  if (!x || !h || !y) AST_FAIL("ast_decimate2_len: null pointer");
  if (B < 1 || B > 65535 || n < 1 || klen < 1 || klen > 4096 || width < 0 || m < 1 || o < 0 || o > 30)
    AST_FAIL("ast_decimate2_len: bad shape (B=%d n=%d klen=%d width=%d m=%d o=%d)", B, n, klen, width, m, o);
  if ((long)(m - 1) * 2 + klen >= (1L << 31)) AST_FAIL("ast_decimate2_len: signal too long");
  const LenArgs len = {n_samples, nsamp, win, step};
  if (len_args_check("ast_decimate2_len", len)) return -1;
  if (n != ast_halved(nsamp, o)) AST_FAIL("ast_decimate2_len: bad shape (n=%d is not nsamp=%d halved %d times)", n, nsamp, o);
  return decimate2_launch(x, B, n, h, klen, width, y, m, gain, &len, o, stream);
}

