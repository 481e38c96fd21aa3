// Shared device helpers for the MI355X (gfx950, CDNA4) ST-GCN kernels.
//
// Layout convention: every activation tensor is the reference's logical
// (N, C, T, V) tensor stored CHANNELS-LAST, i.e. physically [N][T][V][C] ("rows" of C
// contiguous channels, row index m = (n*T + t)*V + v).  Element types: fp32 (parity path)
// and bf16 (perf path); accumulation is always fp32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef __bf16 bf16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
// bf16 bit patterns as the transposed LDS reads return them (lds_ops.h)
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

#define DEV __device__ __forceinline__

// ------------------------------------------------------------------------------------------
// Element traits.  A "fragment" is the 8 consecutive-k values one lane contributes to one
// 32x32 MFMA k-step of 16 (lane l: row/col l&31, k = 8*(l>>5) + j, j = 0..7).
//   bf16: one v_mfma_f32_32x32x16_bf16.
//   fp32: eight v_mfma_f32_32x32x2_f32, instruction j consuming element j of both operands
//         (a relabelling of the k axis that keeps the bf16 lane map: exact fp32 products).
// ------------------------------------------------------------------------------------------
template <typename T> struct Tr;

template <> struct Tr<float> {
  typedef f32x8 frag;
  static constexpr int VEC = 4;  // elements per 16-byte unit
  static DEV float to_f(float v) { return v; }
  static DEV float from_f(float v) { return v; }
  static DEV void mma(f32x16& acc, const frag& a, const frag& b) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
  }
};

template <> struct Tr<bf16> {
  typedef bf16x8 frag;
  static constexpr int VEC = 8;
  static DEV float to_f(bf16 v) { return (float)v; }
  static DEV bf16 from_f(float v) { return (bf16)v; }
  static DEV void mma(f32x16& acc, const frag& a, const frag& b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
  }
};

// 16-byte unit <-> 8 floats (bf16) or 4 floats (fp32)
// Channel of block b in a one-block-per-channel reduction over [nb][C] partial rows (grid = C): workgroups
// are dealt round-robin to the 8 XCDs, so with c = b every 128-B line of partials (8 float4 channels) was
// fetched into all eight L2s; this mapping gives each XCD a contiguous channel range (C % 64 == 0), so each
// line goes to one L2.
DEV int xcd_channel(int b, int C) { return (C & 63) ? b : (b & 7) * (C >> 3) + (b >> 3); }

DEV void unpack16(const uint4& u, float* f, bf16*) {
  const bf16x8 v = __builtin_bit_cast(bf16x8, u);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = (float)v[j];
}
DEV void unpack16(const uint4& u, float* f, float*) {
  const f32x4 v = __builtin_bit_cast(f32x4, u);
#pragma unroll
  for (int j = 0; j < 4; ++j) f[j] = v[j];
}
DEV uint4 pack16(const float* f, bf16*) {
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (bf16)f[j];
  return __builtin_bit_cast(uint4, v);
}
DEV uint4 pack16(const float* f, float*) {
  f32x4 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = f[j];
  return __builtin_bit_cast(uint4, v);
}

// MFMA fragment from LDS rows that hold consecutive k: bf16 = the 16 B at p0; fp32 = the 16 B at p0 (elements
// 0..3) and at p1 (4..7)
template <typename T>
DEV typename Tr<T>::frag frag2(const char* p0, const char* p1) {
  if constexpr (sizeof(T) == 2) {
    (void)p1;
    return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(p0));
  } else {
    const f32x4 a = __builtin_bit_cast(f32x4, *reinterpret_cast<const uint4*>(p0));
    const f32x4 b = __builtin_bit_cast(f32x4, *reinterpret_cast<const uint4*>(p1));
    f32x8 f;
    f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3];
    f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
    return f;
  }
}

// LDS pointer -> its 32-bit LDS offset (what M0 and the asm DMA of lds_ops.h take)
DEV unsigned lds_u32(const void* p) { return (unsigned)(size_t)(const __attribute__((address_space(3))) char*)p; }

// Workgroup barrier for LDS hand-offs only: waits for this wave's LDS ops (lgkmcnt) but NOT for its outstanding
// global loads, DMA and stores -- __syncthreads() would drain vmcnt, i.e. every prefetch ring, at each hand-off.
// The "memory" clobber keeps the compiler from moving memory ops across it.
DEV void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// s_waitcnt vmcnt(n) for a wave-uniform run-time n (clamped to 63, the counter's range: waiting for fewer
// outstanding operations is always safe)
template <int N>
DEV void wait_vm_upto(int n) {
  if constexpr (N < 63) {
    if (n <= N) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
      return;
    }
    wait_vm_upto<N + 1>(n);
  } else {
    asm volatile("s_waitcnt vmcnt(63)" ::: "memory");
  }
}
DEV void wait_vm(int n) { wait_vm_upto<0>(n < 0 ? 0 : n); }

// C/D map of the 32x32 MFMAs (dtype independent on gfx950): col = lane&31,
// row = (r&3) + 8*(r>>2) + 4*(lane>>5), r = accumulator register 0..15.
DEV int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// Chan's parallel combination of (count, mean, M2) triples (numerically robust variance).
struct Welford {
  float n, mean, m2;
};
DEV Welford welford_merge(Welford a, Welford b) {
  const float n = a.n + b.n;
  if (n == 0.f) return a;
  const float d = b.mean - a.mean;
  const float fb = b.n / n;
  Welford r;
  r.n = n;
  r.mean = a.mean + d * fb;
  r.m2 = a.m2 + b.m2 + d * d * a.n * fb;
  return r;
}

DEV float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// fixed-order block sum through red[blockDim.x / 64]: every thread gets the total
DEV float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
  return t;
}

// status codes of the C-ABI (include/stgcn_amd.h)
#define STGCN_OK 0
#define STGCN_EBADSHAPE 1
#define STGCN_EDTYPE 2
#define STGCN_EHIP 3

// Per-device launcher state (runtime.cpp): the CU count of the stream's device, and a one-time (per kernel
// and device) raise of a kernel's dynamic LDS limit.  Thread-safe; no other mutable state in the launchers.
int stgcn_cu_count(hipStream_t s);
int stgcn_lds_attr(const void* kernel, int bytes, hipStream_t s);
