// Helpers of the per-frame (continual inference) kernels: rt_fused.hip, co_frame.hip and rt_streams.hip.
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

// 4 consecutive elements (16 B of fp32, 8 B of bf16) into f[0..3]
DEV void load4(const float* p, float* f) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  f[0] = v.x, f[1] = v.y, f[2] = v.z, f[3] = v.w;
}
DEV void load4(const bf16* p, bf16* f) {
  const bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
  f[0] = v[0], f[1] = v[1], f[2] = v[2], f[3] = v[3];
}

// MFMA B fragment of k-step ks from a packed weight panel [k-step][lane][8] (co_pack_kernel's image): lane l's 8
// contiguous elements at (ks * 64 + l) * 8; zeros beyond ks1
template <typename T>
DEV typename Tr<T>::frag load_b(const T* __restrict__ panel, int ks, int ks1, int lane) {
  T f[8];
  if (ks < ks1) {
    const T* p = panel + ((long)ks * 64 + lane) * 8;
    load4(p, f);
    load4(p + 4, f + 4);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (T)0.f;
  }
  typename Tr<T>::frag b;
#pragma unroll
  for (int j = 0; j < 8; ++j) b[j] = f[j];
  return b;
}
