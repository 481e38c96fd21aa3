// fp32 helpers of the per-frame (continual inference) kernels: rt_fused.hip and co_frame.hip.
#pragma once
#include "common.h"

// 8 lanes per dot product of length 4 * K4 (float4 k = kk + 8j: one contiguous 128-B piece per step),
// butterfly-summed; w from global (L2), x from LDS
DEV float dot8(const float* __restrict__ w, const float* x, int K4, int kk) {
  const float4* w4 = reinterpret_cast<const float4*>(w);
  const float4* x4 = reinterpret_cast<const float4*>(x);
  float s = 0.f;
  for (int k = kk; k < K4; k += 8) {
    const float4 a = w4[k], b = x4[k];
    s = fmaf(a.x, b.x, s);
    s = fmaf(a.y, b.y, s);
    s = fmaf(a.z, b.z, s);
    s = fmaf(a.w, b.w, s);
  }
#pragma unroll
  for (int m = 1; m < 8; m <<= 1) s += __shfl_xor(s, m);
  return s;
}

// LayerNorm passes over a float4 unit: its sum, and its sum of squared distances from the mean m
DEV float sum4(float4 v) { return (v.x + v.y) + (v.z + v.w); }
DEV float sq4(float4 v, float m) {
  const float a = v.x - m, b = v.y - m, c = v.z - m, d = v.w - m;
  return fmaf(a, a, fmaf(b, b, fmaf(c, c, d * d)));
}
