// The 1024-point radix-4 Stockham network that fft.hip (STFT front end, inverse STFT) and metrics.hip (spectrogram metrics) share.
// It is force-inlined into every kernel that uses it, so moving it here changes no kernel's code (tools/kernel_diff.py).
#pragma once
#include "ast_common.h"

namespace {
constexpr int NFFT = 1024;

// the 5 radix-4 Stockham stages on buf[0] (filled, barrier passed), one butterfly per thread per stage; returns the index of
// the half of buf that holds the result
__device__ __forceinline__ int fft1024_stages(float2 (&buf)[2][NFFT], int tid) {
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
  return cur;
}
}  // namespace
