// Helpers of the per-frame (continual inference) kernels: rt_fused.hip, co_frame.hip, rt_streams.hip and co_streams.hip.
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

// two-pass LayerNorm statistics (mean, 1 / sqrt(unbiased var + eps)) of the n = 4 * n4 values a block of NTH threads
// holds in registers (unit e4 = tid + NTH * j), fixed-order sums through red[NTH / 64]
template <int NTH, int U>
DEV float2 ln_stats_units(const float4 (&v)[U], int n4, float* red) {
  const int tid = threadIdx.x;
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < U; ++j) s += tid + NTH * j < n4 ? sum4(v[j]) : 0.f;
  const float n = 4.f * (float)n4;
  const float mean = block_sum(s, red) / n;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < U; ++j) q += tid + NTH * j < n4 ? sq4(v[j], mean) : 0.f;
  const float var = block_sum(q, red) / (n - 1.f);
  return make_float2(mean, 1.f / sqrtf(var + 1e-5f));
}

DEV float4 relu4(float4 v) { return make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)); }
DEV float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
// w * (a - mean) * rstd + b per element
DEV float4 affine4(float4 a, float mean, float rstd, float4 w, float4 b) {
  return make_float4(fmaf(w.x, (a.x - mean) * rstd, b.x), fmaf(w.y, (a.y - mean) * rstd, b.y),
                     fmaf(w.z, (a.z - mean) * rstd, b.z), fmaf(w.w, (a.w - mean) * rstd, b.w));
}

// The 4 parameter elements of a LayerNorm([C,1,V]) tensor (element c*V + v) that meet unit e4 of the rows [V][C]
DEV float4 ln_param4(const float* __restrict__ p, int e4, int V, int C) {
  const int e = e4 * 4, v = e / C, c = e - v * C;  // C % 4 == 0: one row
  const int gi = c * V + v;
  return make_float4(p[gi], p[gi + V], p[gi + 2 * V], p[gi + 3 * V]);
}

// LayerNorm([C,1,V]) affine of the 4 elements of unit e4 of the rows [V][C]: parameter element c*V + v
DEV float4 ln_apply4(float4 a, float2 st, const float* __restrict__ g, const float* __restrict__ b, int e4, int V,
                     int C) {
  const int e = e4 * 4, v = e / C, c = e - v * C;  // C % 4 == 0: one row
  const int gi = c * V + v;
  return make_float4(fmaf(g[gi], (a.x - st.x) * st.y, b[gi]), fmaf(g[gi + V], (a.y - st.x) * st.y, b[gi + V]),
                     fmaf(g[gi + 2 * V], (a.z - st.x) * st.y, b[gi + 2 * V]),
                     fmaf(g[gi + 3 * V], (a.w - st.x) * st.y, b[gi + 3 * V]));
}

DEV void store4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
DEV void store4(bf16* p, float4 v) {
  bf16x4 o;
  o[0] = (bf16)v.x, o[1] = (bf16)v.y, o[2] = (bf16)v.z, o[3] = (bf16)v.w;
  *reinterpret_cast<bf16x4*>(p) = o;
}

// A fragment of k-step ks from fp32 rows in LDS (row stride ld): lane (row = l & 31, h = l >> 5) holds
// x[row][16 ks + 8 h + j], j < 8; zero rows beyond V, zero beyond nks and Cin
DEV f32x8 load_a(const float* xs, int ld, int ks, int nks, int row, int h, int V, int Cin) {
  float f[8];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int kk = ks * 16 + 8 * h + 4 * u;
    if (ks < nks && row < V && kk < Cin) {
      load4(xs + row * ld + kk, f + 4 * u);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) f[4 * u + i] = 0.f;
    }
  }
  f32x8 a;
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = f[j];
  return a;
}

// The same fragment as the MFMA operand type T: fp32 as read; bf16 rounded to nearest even here, once per staged
// element, so the rows in LDS stay fp32 for whoever else reads them
template <typename T>
DEV typename Tr<T>::frag load_a_as(const float* xs, int ld, int ks, int nks, int row, int h, int V, int Cin) {
  const f32x8 f = load_a(xs, ld, ks, nks, row, h, V, Cin);
  if constexpr (sizeof(T) == 4) {
    return f;
  } else {
    bf16x8 a;
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = (bf16)f[j];
    return a;
  }
}
