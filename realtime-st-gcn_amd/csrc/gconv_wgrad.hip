// Weight gradient of the graph convolution (the maths is in gconv.hip's header):
//   dWeff[w][j][co][ci] = sum_i dg[(i,w)][co] * x[(i, S(w)_j)][ci]
// in bf16 by one of four kernels (per pair; joint-grouped register-staged; joint-grouped DMA ring; wide) and an
// fp32 parity kernel, with the slab reductions of the plans that split the rows.  plan_wgrad() chooses the kernel,
// its geometry and the workspace layout once, for gconv_wgrad_workspace and gconv_wgrad_launch alike.
#include "common.h"
#include "launchers.h"
#include "lds_ops.h"
#include "../../include/stgcn_amd.h"

namespace {

// ------------------------------------------------------------------ weight gradient (bf16 + fp32)
// dWeff[w][j][co][ci] += sum_i dy[(i,w)][co] * x[(i, nbr[w][j])][ci].  Block = (pair (w,j), 64-co x
// 64-ci block, row range); the 4 waves split the k-steps of each 128-row tile and are summed in LDS
// at the end; per-block partials go to a slab and are reduced deterministically.
constexpr int WKM = 128;  // rows per tile
constexpr int WPR = 64;   // bytes per bf16 panel row (32 channels): the packed panel trfrag reads

struct WGG {
  int ntile, tpb, R, nco, nci;
  float* slab;     // [R][V*J][Cout][Cin]
  float* rowpart;  // joint-grouped kernel: [R][V][Cout] partial row sums of dy per joint, or NULL
  int zero_unused;  // direct plan (slab = dWeff): also write zeros into the slots j in [deg, J)
  // direct plan, degree-balanced: the joints whose ring is shallow (deg >= W3_SPLIT_DEG) run as two half-row-range
  // blocks that merge in-kernel; part = [V][ngrp][2][J*4096 + 64] half partials, cnt = [V*ngrp] arrival counters
  // (zeroed ahead of every launch)
  float* part;
  unsigned* cnt;
};
constexpr int W3_SPLIT_DEG = 4;  // at 80 KB: ring depth 4 (deg 4) / 3 (deg 5) vs 5 at deg 3 (w3d)

__global__ __launch_bounds__(256, 2) void gconv_wgrad_kernel(const stgcn_gconv_wgrad_desc a, const WGG g) {
  constexpr int PANEL = WKM * WPR;   // one 32-channel panel of a tile
  constexpr int STAGE = 4 * PANEL;   // dy: 2 panels, x: 2 panels
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = a.V;
  const int ngrp = g.nco * g.nci;
  const int pair = blockIdx.x / (ngrp * g.R);
  const int rem = blockIdx.x % (ngrp * g.R);
  const int rr = rem / ngrp, grp = rem % ngrp;
  const int w = pair / a.J, j = pair % a.J;
  if (j >= a.deg[w]) return;  // unused (joint, neighbour) slot: block-uniform exit before any barrier
  const int src = a.nbr[pair];
  const int co0 = (grp % g.nco) * 64, ci0 = (grp / g.nco) * 64;
  const int t0 = rr * g.tpb, t1 = min(g.ntile, t0 + g.tpb);

  const bf16* __restrict__ dy = reinterpret_cast<const bf16*>(a.dy);
  const bf16* __restrict__ x = reinterpret_cast<const bf16*>(a.x);
  // staging: 128 rows x 8 units (64 channels) per operand -> 4 units per thread per operand
  const int uc = tid & 7;
  const int co = co0 + uc * 8, ci = ci0 + uc * 8;
  uint4 ry[4], rx[4];
  auto load = [&](int t) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = (tid >> 3) + u * 32;
      const int i = t * WKM + row;
      ry[u] = make_uint4(0, 0, 0, 0);
      rx[u] = make_uint4(0, 0, 0, 0);
      if (i < a.NT) {
        if (co < a.Cout) ry[u] = *reinterpret_cast<const uint4*>(dy + ((long)i * V + w) * a.dy_ld + co);
        if (ci < a.Cin) rx[u] = *reinterpret_cast<const uint4*>(x + ((long)i * V + src) * a.x_ld + ci);
      }
    }
  };
  auto store = [&](int buf) {
    char* base = smem + buf * STAGE;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = (tid >> 3) + u * 32;
      const int off = (uc >> 2) * PANEL + row * WPR + (uc & 3) * 16;
      *reinterpret_cast<uint4*>(base + off) = ry[u];
      *reinterpret_cast<uint4*>(base + 2 * PANEL + off) = rx[u];
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int a2 = 0; a2 < 2; ++a2)
#pragma unroll
    for (int b2 = 0; b2 < 2; ++b2)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a2][b2][r] = 0.f;

  int cur = 0;
  if (t0 < t1) {
    load(t0);
    store(0);
  }
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    const bool more = t + 1 < t1;
    if (more) load(t + 1);
    const char* base = smem + cur * STAGE;
#pragma unroll
    for (int kk = 0; kk < WKM / 16 / 4; ++kk) {  // this wave's k-steps: ks = wave + 4*kk
      const int ks = wave + 4 * kk;
      bf16x8 fa[2], fb[2];
#pragma unroll
      for (int a2 = 0; a2 < 2; ++a2) fa[a2] = trfrag(base + a2 * PANEL, ks * 16, lane);
#pragma unroll
      for (int b2 = 0; b2 < 2; ++b2) fb[b2] = trfrag(base + (2 + b2) * PANEL, ks * 16, lane);
#pragma unroll
      for (int a2 = 0; a2 < 2; ++a2)
#pragma unroll
        for (int b2 = 0; b2 < 2; ++b2)
          acc[a2][b2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[a2], fb[b2], acc[a2][b2], 0, 0, 0);
    }
    if (more) store(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

  // sum the 4 waves' accumulators (LDS), wave 0 writes this block's partial
  float* red = reinterpret_cast<float*>(smem);  // [3][4 tiles][16][64]
  if (wave > 0) {
#pragma unroll
    for (int a2 = 0; a2 < 2; ++a2)
#pragma unroll
      for (int b2 = 0; b2 < 2; ++b2)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[(((wave - 1) * 4 + a2 * 2 + b2) * 16 + r) * 64 + lane] = acc[a2][b2][r];
  }
  __syncthreads();
  if (wave == 0) {
    float* slab = g.slab + ((long)rr * V * a.J + pair) * a.Cout * a.Cin;
#pragma unroll
    for (int a2 = 0; a2 < 2; ++a2)
#pragma unroll
      for (int b2 = 0; b2 < 2; ++b2) {
        const int cc = ci0 + b2 * 32 + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v = acc[a2][b2][r];
          for (int k = 0; k < 3; ++k) v += red[((k * 4 + a2 * 2 + b2) * 16 + r) * 64 + lane];
          const int oc = co0 + a2 * 32 + acc_row(r, lane);
          if (oc < a.Cout && cc < a.Cin) slab[(long)oc * a.Cin + cc] = v;
        }
      }
  }
}

// Joint-grouped variant: block = (output joint w, COB = 64 output channels, 64 input channels, row range).
// Every pair (w, j < deg[w]) shares the dy[:, w] panel, so a 32-row tile stages dy once plus deg x
// panels (one per neighbour) instead of deg (dy, x) pairs: (1 + deg) / (2 deg) of the L2 -> LDS traffic.
// Waves = (32-co half, 32-ci half);
// each keeps one 32x32 accumulator per neighbour (J2 <= 5) and per k-step reads one dy fragment and
// deg x fragments (ds_read_b64_tr_b16) for deg MFMAs.  Partials go to the same slab as above.
// COB = 64: 32-row tiles, 48 KB of LDS double-buffered, three 4-wave blocks per CU.  Measured against COB = 128
// (64-row tiles, 112 KB, one 8-wave block per CU), not kept: C=128 78 vs 85 us, C=256 143 vs 153 us, equal at
// 64 -> 128; and 56 vs 72 us (per-pair kernel) at C = 64.
constexpr int W2_COB = 64;  // output channels per block
constexpr int W2M = 32;     // rows per tile
constexpr int J2 = 5;       // max neighbours per joint
constexpr int W2_LDS = 2 * (W2_COB / 32 + 2 * J2) * W2M * WPR;  // two stages of (dy panels + 2 x panels per neighbour)
__global__ __launch_bounds__(W2_COB / 16 * 64, 3) void gconv_wgrad2_kernel(const stgcn_gconv_wgrad_desc a, const WGG g) {
  constexpr int COB = W2_COB;
  constexpr int NW = COB / 16, NT = NW * 64;
  constexpr int PANEL = W2M * WPR;           // 32 channels x W2M rows
  constexpr int DYP = COB / 32;              // dy panels
  constexpr int STAGE = (DYP + 2 * J2) * PANEL;
  constexpr int DYU = COB * W2M / 8 / NT;    // dy 16-B units per thread (2)
  constexpr int XU = 64 * W2M / 8 / NT;      // x units per thread per neighbour (2)
  static_assert(DYU >= 1 && XU >= 1, "units");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cq = wave % DYP, ch = wave / DYP;  // co quarter (32), ci half (32)
  const int V = a.V;
  const int ngrp = g.nco * g.nci;
  const int w = blockIdx.x / (ngrp * g.R);
  const int rem = blockIdx.x % (ngrp * g.R);
  const int rr = rem / ngrp, grp = rem % ngrp;
  const int deg = a.deg[w];
  const int co0 = (grp % g.nco) * COB, ci0 = (grp / g.nco) * 64;
  const int t0 = rr * g.tpb, t1 = min(g.ntile, t0 + g.tpb);
  int src[J2];
#pragma unroll
  for (int j = 0; j < J2; ++j) src[j] = j < deg ? a.nbr[w * a.J + j] : 0;

  const bf16* __restrict__ dy = reinterpret_cast<const bf16*>(a.dy);
  const bf16* __restrict__ x = reinterpret_cast<const bf16*>(a.x);
  uint4 ry[DYU], rx[J2][XU];
  // dy unit e = tid + NT*u: row e / (COB/8), 8 channels at (e % (COB/8)) * 8; x unit: row e / 8, ch (e % 8) * 8
  auto load = [&](int t) {
#pragma unroll
    for (int u = 0; u < DYU; ++u) {
      const int e = tid + NT * u, row = e / (COB / 8), cu = e % (COB / 8);
      const int i = t * W2M + row;
      ry[u] = make_uint4(0, 0, 0, 0);
      if (i < a.NT && co0 + cu * 8 < a.Cout) ry[u] = *reinterpret_cast<const uint4*>(dy + ((long)i * V + w) * a.dy_ld + co0 + cu * 8);
    }
#pragma unroll
    for (int j = 0; j < J2; ++j)
#pragma unroll
      for (int u = 0; u < XU; ++u) {
        const int e = tid + NT * u, row = e >> 3, cu = e & 7;
        const int i = t * W2M + row;
        rx[j][u] = make_uint4(0, 0, 0, 0);
        if (j < deg && i < a.NT && ci0 + cu * 8 < a.Cin)
          rx[j][u] = *reinterpret_cast<const uint4*>(x + ((long)i * V + src[j]) * a.x_ld + ci0 + cu * 8);
      }
  };
  auto store = [&](int buf) {
    char* base = smem + buf * STAGE;
#pragma unroll
    for (int u = 0; u < DYU; ++u) {
      const int e = tid + NT * u, row = e / (COB / 8), cu = e % (COB / 8);
      *reinterpret_cast<uint4*>(base + (cu >> 2) * PANEL + row * WPR + (cu & 3) * 16) = ry[u];
    }
#pragma unroll
    for (int j = 0; j < J2; ++j)
#pragma unroll
      for (int u = 0; u < XU; ++u) {
        const int e = tid + NT * u, row = e >> 3, cu = e & 7;
        if (j < deg)
          *reinterpret_cast<uint4*>(base + (DYP + 2 * j + (cu >> 2)) * PANEL + row * WPR + (cu & 3) * 16) = rx[j][u];
      }
  };

  f32x16 acc[J2];
#pragma unroll
  for (int j = 0; j < J2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  // per-joint row sums of dy (the bias-through-A gradient) ride along in the first ci-group's blocks
  const bool rsum = g.rowpart != nullptr && grp / g.nco == 0;
  float sacc[DYU][8];
#pragma unroll
  for (int u = 0; u < DYU; ++u)
#pragma unroll
    for (int e = 0; e < 8; ++e) sacc[u][e] = 0.f;
  auto add_rows = [&]() {
    if (rsum) {
#pragma unroll
      for (int u = 0; u < DYU; ++u) {
        float f[8];
        unpack16(ry[u], f, (bf16*)nullptr);
#pragma unroll
        for (int e = 0; e < 8; ++e) sacc[u][e] += f[e];
      }
    }
  };

  int cur = 0;
  if (t0 < t1) {
    load(t0);
    add_rows();
    store(0);
  }
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    const bool more = t + 1 < t1;
    if (more) load(t + 1);
    const char* base = smem + cur * STAGE;
#pragma unroll
    for (int ks = 0; ks < W2M / 16; ++ks) {
      const bf16x8 fa = trfrag(base + cq * PANEL, ks * 16, lane);
#pragma unroll
      for (int j = 0; j < J2; ++j)
        if (j < deg) {
          const bf16x8 fb = trfrag(base + (DYP + 2 * j + ch) * PANEL, ks * 16, lane);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[j], 0, 0, 0);
        }
    }
    if (more) {
      add_rows();
      store(cur ^ 1);
    }
    __syncthreads();
    cur ^= 1;
  }
  if (rsum) {  // [row slot][COB] in LDS (the stages are free after the last barrier), fixed-order sum
    float* red = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int u = 0; u < DYU; ++u) {
      const int e = tid + NT * u, row = e / (COB / 8), cu = e % (COB / 8);
#pragma unroll
      for (int k = 0; k < 8; ++k) red[row * COB + cu * 8 + k] = sacc[u][k];
    }
    __syncthreads();
    if (tid < COB && co0 + tid < a.Cout) {
      float t = 0.f;
      for (int r = 0; r < W2M; ++r) t += red[r * COB + tid];
      g.rowpart[((long)rr * V + w) * a.Cout + co0 + tid] = t;
    }
  }

  // block partial of each pair (w, j) -> slab[rr][w*J + j][co][ci]
  const int cc = ci0 + ch * 32 + (lane & 31);
#pragma unroll
  for (int j = 0; j < J2; ++j) {
    if (j >= deg) continue;
    float* slab = g.slab + ((long)rr * V * a.J + w * a.J + j) * a.Cout * a.Cin;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int oc = co0 + cq * 32 + acc_row(r, lane);
      if (oc < a.Cout && cc < a.Cin) slab[(long)oc * a.Cin + cc] = acc[j][r];
    }
  }
}

// DMA-ring variant of gconv_wgrad2_kernel (the default): the same block = (joint w, 64 co, 64 ci,
// row range) and wave split, but the 32-row tiles go global -> LDS with global_load_lds (no register
// staging) into a ring of W3D(DEG) slots sized by the joint's degree, so D - 1 tiles are in flight
// while one is consumed instead of one.  The register-staged kernel kept at most one tile (~16 KB)
// per block in flight and sat at ~13 % of the MFMA peak, latency-bound on L2/MALL.  Body per degree
// (DEG = deg[w], a block-uniform value) so the vmcnt counts are immediates.
// LDS per block: 80 KB (two blocks per CU).  160 KB for the direct plans (R = 1: fewer, longer blocks; one block
// per CU and a deeper ring) measured slower in the step (8.09 vs 8.01 ms, 3 interleaved runs), not kept.
constexpr int W3_LDS = 80 * 1024;
constexpr int w3_stage(int deg) { return (2 + 2 * deg) * 32 * WPR; }
constexpr int w3d(int deg) { return W3_LDS / w3_stage(deg) > 8 ? 8 : W3_LDS / w3_stage(deg); }

// half: -1 = a whole (joint, group, row range) block; 0 / 1 = one half of a split direct-plan block (tiles t0..t1)
template <int DEG>
DEV void wgrad3_body(const stgcn_gconv_wgrad_desc& a, const WGG& g, char* smem, int w, int rr, int grp, int t0,
                     int t1, int half) {
  constexpr int D = w3d(DEG), PANEL = 32 * WPR, STAGE = w3_stage(DEG), NU = 1 + DEG;
  static_assert(D >= 3 && (D - 2) * NU <= 63, "ring");
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cq = wave & 1, ch = wave >> 1;  // co half (32), ci half (32)
  const int V = a.V;
  const int co0 = (grp % g.nco) * 64, ci0 = (grp / g.nco) * 64;
  const bf16* __restrict__ dy = reinterpret_cast<const bf16*>(a.dy);
  const bf16* __restrict__ x = reinterpret_cast<const bf16*>(a.x);
  // this wave's DMA share of a tile: dy panel (wave >> 1) rows 16 (wave & 1) .. +15, and the same
  // (panel, half) of every neighbour's x; lane -> (row lane / 4, 16-B unit lane % 4)
  const int prow = 16 * (wave & 1) + (lane >> 2), pu = lane & 3, pp = wave >> 1;
  const bf16* ysrc = dy + (long)w * a.dy_ld + co0 + pp * 32 + pu * 8;
  const bf16* xsrc[DEG];
#pragma unroll
  for (int j = 0; j < DEG; ++j) xsrc[j] = x + (long)a.nbr[w * a.J + j] * a.x_ld + ci0 + pp * 32 + pu * 8;
  const long ystep = (long)V * a.dy_ld, xstep = (long)V * a.x_ld;
  const unsigned ring = lds_u32(smem);
  const unsigned woff = (unsigned)(pp * PANEL + (wave & 1) * 1024);
  auto issue = [&](int t) {
    const int i = min(t * 32 + prow, a.NT - 1);  // rows past NT: clamped here, zeroed in LDS below
    const unsigned slot = ring + (unsigned)(((t - t0) % D) * STAGE) + woff;
    glds16(ysrc + i * ystep, slot);
#pragma unroll
    for (int j = 0; j < DEG; ++j) glds16(xsrc[j] + i * xstep, slot + (unsigned)((2 + 2 * j) * PANEL));
  };
#pragma unroll
  for (int k = 0; k < D - 1; ++k)
    if (t0 + k < t1) issue(t0 + k);

  f32x16 acc[DEG];
#pragma unroll
  for (int j = 0; j < DEG; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  const bool rsum = g.rowpart != nullptr && grp / g.nco == 0;
  float sacc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) sacc[e] = 0.f;
  // row-sum unit of this thread: row tid / 8, 8 channels at (tid % 8) * 8
  const int srow = tid >> 3, scu = tid & 7;
  const int soff = (scu >> 2) * PANEL + srow * WPR + (scu & 3) * 16;

  for (int t = t0; t < t1; ++t) {
    const int after = min(D - 2, t1 - 1 - t);  // tiles issued after t
    static_for<D - 1>([&]<int m>() {
      if (after == m) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(m * NU) : "memory");
    });
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (t + D - 1 < t1) issue(t + D - 1);  // into the slot of tile t - 1, free after the barrier
    char* base = smem + ((t - t0) % D) * STAGE;
    if (t * 32 + 32 > a.NT) {  // last, partial tile: zero dy rows >= NT (block-uniform branch)
      if (t * 32 + srow >= a.NT) *reinterpret_cast<uint4*>(base + soff) = make_uint4(0, 0, 0, 0);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    if (rsum) {
      float f[8];
      unpack16(*reinterpret_cast<const uint4*>(base + soff), f, (bf16*)nullptr);
#pragma unroll
      for (int e = 0; e < 8; ++e) sacc[e] += f[e];
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 fa = trfrag(base + cq * PANEL, ks * 16, lane);
#pragma unroll
      for (int j = 0; j < DEG; ++j) {
        const bf16x8 fb = trfrag(base + (2 + 2 * j + ch) * PANEL, ks * 16, lane);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[j], 0, 0, 0);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  float rs = 0.f;  // this block's row sum of column co0 + tid (tid < 64)
  if (rsum) {  // [row][64] in LDS, fixed-order column sums
    float* red = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int k = 0; k < 8; ++k) red[srow * 64 + scu * 8 + k] = sacc[k];
    __syncthreads();
    if (tid < 64)
      for (int r = 0; r < 32; ++r) rs += red[r * 64 + tid];
  }
  if (half >= 0) {
    // split block: publish this half's partial write-through (sc1), drain, one arrival; the second arriver reads the
    // other half (sc1) and adds it (a + b == b + a: the result does not depend on which half came last) and writes
    // the outputs (MI355X_MICROARCH "Valid forms" row 1: sc1 stores and loads on both sides, no fences)
    constexpr int PSZ_J = 4096;
    const int ngrp = g.nco * g.nci;
    const long PSZ = (long)a.J * PSZ_J + 64;
    float* mine = g.part + (((long)w * ngrp + grp) * 2 + half) * PSZ;
    const float* other = g.part + (((long)w * ngrp + grp) * 2 + (1 - half)) * PSZ;
    const int el = (cq * 32) * 64 + ch * 32 + (lane & 31);  // + acc_row(r, lane) * 64
#pragma unroll
    for (int j = 0; j < DEG; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        __hip_atomic_store(mine + j * PSZ_J + el + acc_row(r, lane) * 64, acc[j][r], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    if (rsum && tid < 64) __hip_atomic_store(mine + a.J * PSZ_J + tid, rs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int* flag = reinterpret_cast<int*>(smem);
    if (tid == 0)
      *flag = (int)__hip_atomic_fetch_add(g.cnt + (long)w * ngrp + grp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (*flag == 0) return;  // first arriver: the partner merges
#pragma unroll
    for (int j = 0; j < DEG; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        acc[j][r] += __hip_atomic_load(const_cast<float*>(other) + j * PSZ_J + el + acc_row(r, lane) * 64,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (rsum && tid < 64)
      rs += __hip_atomic_load(const_cast<float*>(other) + a.J * PSZ_J + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (rsum && tid < 64) g.rowpart[((long)rr * V + w) * a.Cout + co0 + tid] = rs;
  const int cc = ci0 + ch * 32 + (lane & 31);
#pragma unroll
  for (int j = 0; j < DEG; ++j) {
    float* slab = g.slab + ((long)rr * V * a.J + w * a.J + j) * a.Cout * a.Cin;
#pragma unroll
    for (int r = 0; r < 16; ++r) slab[(long)(co0 + cq * 32 + acc_row(r, lane)) * a.Cin + cc] = acc[j][r];
  }
  if (g.zero_unused)
    for (int j = DEG; j < a.J; ++j) {
      float* slab = g.slab + ((long)w * a.J + j) * a.Cout * a.Cin;
#pragma unroll
      for (int r = 0; r < 16; ++r) slab[(long)(co0 + cq * 32 + acc_row(r, lane)) * a.Cin + cc] = 0.f;
    }
}

// Blocks run joint-major.  A row-range-major order remapped so that consecutive logical blocks share an XCD (all
// joints of one row range on one XCD: the x rows a joint's neighbours also read stay in that XCD's L2) was an A/B
// build, not kept.  The direct plan (R = 1) is always the degree-balanced one (W3_SPLIT_DEG).
__global__ __launch_bounds__(256, 2) void gconv_wgrad3_kernel(const stgcn_gconv_wgrad_desc a, const WGG g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int ngrp = g.nco * g.nci;
  const int bid = g.part ? (int)(blockIdx.x % (a.V * ngrp)) : (int)blockIdx.x;  // split plan: slot 1 repeats slot 0
  const int w = bid / (ngrp * g.R);
  const int rem = bid % (ngrp * g.R);
  const int rr = rem / ngrp, grp = rem % ngrp;
  // joints in decreasing-degree order (ties by index): the heaviest blocks are dispatched first and the
  // light ones fill the tail.  Scratch in the ring's first bytes, before any DMA is issued.
  int* sdeg = reinterpret_cast<int*>(smem);
  int* order = sdeg + 64;
  int wj = w;
  if (a.V <= 64) {
    const int tid = threadIdx.x;
    if (tid < a.V) sdeg[tid] = a.deg[tid];
    __syncthreads();
    if (tid < a.V) {
      const int d = sdeg[tid];
      int r = 0;
      for (int u = 0; u < a.V; ++u) r += (sdeg[u] > d) | ((sdeg[u] == d) & (u < tid));
      order[r] = tid;
    }
    __syncthreads();
    wj = order[w];
    __syncthreads();
  }
  int t0 = rr * g.tpb, t1 = min(g.ntile, t0 + g.tpb), half = -1;
  if (g.part) {  // degree-balanced direct plan: grid = 2 x V x ngrp, slot 1 only for the split joints
    const int slot = blockIdx.x / (a.V * ngrp);
    const bool split = a.deg[wj] >= W3_SPLIT_DEG;
    if (slot == 1 && !split) return;  // block-uniform exit before any barrier
    if (split) {
      half = slot;
      const int tm = g.ntile / 2;
      t0 = half ? tm : 0;
      t1 = half ? g.ntile : tm;
    }
  }
  switch (a.deg[wj]) {
    case 1: wgrad3_body<1>(a, g, smem, wj, rr, grp, t0, t1, half); break;
    case 2: wgrad3_body<2>(a, g, smem, wj, rr, grp, t0, t1, half); break;
    case 3: wgrad3_body<3>(a, g, smem, wj, rr, grp, t0, t1, half); break;
    case 4: wgrad3_body<4>(a, g, smem, wj, rr, grp, t0, t1, half); break;
    case 5: wgrad3_body<5>(a, g, smem, wj, rr, grp, t0, t1, half); break;
    default:  // deg 0: no pairs (the reduction skips j >= deg); the row sums still come from here
      if (g.rowpart != nullptr && grp / g.nco == 0 && threadIdx.x < 64) {
        const int co = (grp % g.nco) * 64 + threadIdx.x;
        const int i1 = min(a.NT, min(g.ntile, (rr + 1) * g.tpb) * 32);
        const bf16* dy = reinterpret_cast<const bf16*>(a.dy);
        float s = 0.f;
        for (int i = rr * g.tpb * 32; i < i1; ++i) s += (float)dy[((long)i * a.V + wj) * a.dy_ld + co];
        g.rowpart[((long)rr * a.V + wj) * a.Cout + co] = s;
      }
      if (g.zero_unused) {  // direct plan: this joint's J slots of the (64 co, 64 ci) group are zero
        const int co0 = (grp % g.nco) * 64, ci0 = (grp / g.nco) * 64;
        for (int i = threadIdx.x; i < a.J * 64 * 64; i += blockDim.x) {
          const int j = i >> 12, co = (i >> 6) & 63, ci = i & 63;
          g.slab[(((long)wj * a.J + j) * a.Cout + co0 + co) * a.Cin + ci0 + ci] = 0.f;
        }
      }
      break;
  }
}

// ---- wide plan (Cin, Cout % 128 == 0): block = (joint, 128 co x 128 ci group, row part), 4 waves (one per SIMD, 2 x 2
// output tiles per neighbour each: 64*DEG accumulators, up to 512 registers per lane) and a 160 KB ring.  Against the 64 x 64 blocks above it halves the panels every block stages per MFMA (dy read by
// Cin/128 instead of Cin/64 blocks, x by Cout/128) and gives each barrier twice the matrix work per SIMD.  Row
// parts of one group merge in-kernel: every part publishes its partial write-through (sc1), takes a ticket, and
// the last arriver sums the R partials in part-index order (a fixed order: the result does not depend on
// arrival), then writes dWeff, the zero slots and the row sums.
constexpr int W3W_LDS = 160 * 1024;
constexpr int W3W_PSZ_J = 128 * 128;
constexpr int W3W_JE = 3;  // neighbours per entry at most: joints of degree >= 4 run as two entries
constexpr int w3w_stage(int deg) { return (4 + 4 * deg) * 32 * WPR; }
constexpr int w3w_d(int deg) { return W3W_LDS / w3w_stage(deg) > 8 ? 8 : W3W_LDS / w3w_stage(deg); }

template <int DEG>
DEV void wgrad3w_body(const stgcn_gconv_wgrad_desc& a, const WGG& g, char* smem, int w, int e, int j0, int dtot, int rr,
                      int grp, int t0, int t1) {
  constexpr int D = w3w_d(DEG), PANEL = 32 * WPR, STAGE = w3w_stage(DEG), NU = 2 * (1 + DEG);
  static_assert(D >= 3 && (D - 2) * NU <= 63, "ring");
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cp = wave & 1, ip = wave >> 1;  // co tiles 2cp, 2cp+1 and ci tiles 2ip, 2ip+1 (32 each) of the group
  const int V = a.V;
  const int co0 = (grp % g.nco) * 128, ci0 = (grp / g.nco) * 128;
  const bf16* __restrict__ dy = reinterpret_cast<const bf16*>(a.dy);
  const bf16* __restrict__ x = reinterpret_cast<const bf16*>(a.x);
  // DMA share of a tile: panel `wave` of dy and of every neighbour's x, both 16-row halves;
  // lane -> (row lane / 4 (+16), 16-B unit lane % 4)
  const int prow = lane >> 2, pu = lane & 3;
  const bf16* ysrc = dy + (long)w * a.dy_ld + co0 + wave * 32 + pu * 8;
  const bf16* xsrc[DEG];
#pragma unroll
  for (int j = 0; j < DEG; ++j) xsrc[j] = x + (long)a.nbr[w * a.J + j0 + j] * a.x_ld + ci0 + wave * 32 + pu * 8;
  const long ystep = (long)V * a.dy_ld, xstep = (long)V * a.x_ld;
  const unsigned ring = lds_u32(smem);
  const unsigned woff = (unsigned)(wave * PANEL);
  auto issue = [&](int t) {
    const unsigned slot = ring + (unsigned)(((t - t0) % D) * STAGE) + woff;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = min(t * 32 + 16 * h + prow, a.NT - 1);  // rows past NT: clamped here, dy zeroed in LDS below
      glds16(ysrc + i * ystep, slot + (unsigned)(h * 1024));
#pragma unroll
      for (int j = 0; j < DEG; ++j) glds16(xsrc[j] + i * xstep, slot + (unsigned)((4 + 4 * j) * PANEL + h * 1024));
    }
  };
#pragma unroll
  for (int k = 0; k < D - 1; ++k)
    if (t0 + k < t1) issue(t0 + k);

  f32x16 acc[DEG][2][2];
#pragma unroll
  for (int j = 0; j < DEG; ++j)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][u][c][r] = 0.f;
  const bool rsum = g.rowpart != nullptr && grp / g.nco == 0 && j0 == 0;  // an entry's first neighbour slot: row sums
  float sacc[2][8];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int e = 0; e < 8; ++e) sacc[h][e] = 0.f;
  // dy units of this thread (row sums, zeroing past NT): unit tid + 256 h -> row (unit / 16), channels (unit % 16) * 8
  auto soff = [&](int h) {
    const int u = tid + 256 * h, sr = u >> 4, sc = u & 15;
    return (sc >> 2) * PANEL + sr * WPR + (sc & 3) * 16;
  };

  for (int t = t0; t < t1; ++t) {
    const int after = min(D - 2, t1 - 1 - t);  // tiles issued after t
    static_for<D - 1>([&]<int m>() {
      if (after == m) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(m * NU) : "memory");
    });
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (t + D - 1 < t1) issue(t + D - 1);  // into the slot of tile t - 1, free after the barrier
    char* base = smem + ((t - t0) % D) * STAGE;
    if (t * 32 + 32 > a.NT) {  // last, partial tile: zero dy rows >= NT (block-uniform branch)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        if (t * 32 + ((tid + 256 * h) >> 4) >= a.NT) *reinterpret_cast<uint4*>(base + soff(h)) = make_uint4(0, 0, 0, 0);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    if (rsum) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float f[8];
        unpack16(*reinterpret_cast<const uint4*>(base + soff(h)), f, (bf16*)nullptr);
#pragma unroll
        for (int e = 0; e < 8; ++e) sacc[h][e] += f[e];
      }
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 fa[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) fa[u] = trfrag(base + (2 * cp + u) * PANEL, ks * 16, lane);
#pragma unroll
      for (int j = 0; j < DEG; ++j) {
        bf16x8 fb[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) fb[c] = trfrag(base + (4 + 4 * j + 2 * ip + c) * PANEL, ks * 16, lane);
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int c = 0; c < 2; ++c)
            acc[j][u][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[u], fb[c], acc[j][u][c], 0, 0, 0);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  float rs = 0.f;  // this block's row sum of column co0 + tid (tid < 128)
  if (rsum) {      // [row][128] in LDS (first 16 KB), fixed-order column sums
    float* red = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int u = tid + 256 * h;
#pragma unroll
      for (int k = 0; k < 8; ++k) red[(u >> 4) * 128 + (u & 15) * 8 + k] = sacc[h][k];
    }
    __syncthreads();
    if (tid < 128)
      for (int r = 0; r < 32; ++r) rs += red[r * 128 + tid];
  }
  // Epilogue through LDS, one neighbour at a time: the 128 x 128 tile staged as fp32 rows [co][132], then whole
  // 512-B rows leave as 16-B stores (every address an LDS immediate or one running pointer: no per-element
  // address registers next to the 64*DEG accumulators)
  constexpr int SRS = 132;
  float* stg = reinterpret_cast<float*>(smem + 20 * 1024);  // after the row sums and the ticket word
  int* flag = reinterpret_cast<int*>(smem + 16 * 1024);
  const bool merged = g.R > 1;
  const int ngrp = g.nco * g.nci;
  const long PSZ = (long)W3W_JE * W3W_PSZ_J + 128;
  float* gp = merged ? g.part + ((long)e * ngrp + grp) * g.R * PSZ : nullptr;
  const __amdgpu_buffer_rsrc_t prs =
      __builtin_amdgcn_make_buffer_rsrc(merged ? gp : g.slab, 0, merged ? (int)(g.R * PSZ * 4) : 0, 0x00020000);
  float* o0 = g.slab + (long)w * a.J * a.Cout * a.Cin + (long)co0 * a.Cin + ci0;  // dWeff[w][0][co0][ci0]
  const long ojs = (long)a.Cout * a.Cin;
#pragma unroll
  for (int j = 0; j < DEG; ++j) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          stg[(cp * 64 + u * 32 + acc_row(r, lane)) * SRS + ip * 64 + c * 32 + (lane & 31)] = acc[j][u][c][r];
    __syncthreads();
    for (int e = tid; e < 128 * 32; e += 256) {
      const int row = e >> 5, q4 = e & 31;
      const float4 v = *reinterpret_cast<const float4*>(stg + row * SRS + q4 * 4);
      if (!merged)
        *reinterpret_cast<float4*>(o0 + (j0 + j) * ojs + (long)row * a.Cin + q4 * 4) = v;
      else  // this part's partial, write-through (sc1): the last arriver reads it from another CU / XCD
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v), prs,
                                               (int)(((long)rr * PSZ + j * W3W_PSZ_J + row * 128 + q4 * 4) * 4), 0, 16);
    }
  }
  if (merged) {
    if (rsum && tid < 128)
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, rs), prs,
                                            (int)(((long)rr * PSZ + W3W_JE * W3W_PSZ_J + tid) * 4), 0, 16);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0)
      *flag = (int)__hip_atomic_fetch_add(g.cnt + (long)e * ngrp + grp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (*flag != g.R - 1) return;  // not the last part: the last arriver merges
    // the R partials summed in part-index order (a fixed order: the result does not depend on arrival)
    for (int j = 0; j < DEG; ++j)
      for (int e = tid; e < 128 * 32; e += 256) {
        const int row = e >> 5, q4 = e & 31;
        const int off = (j * W3W_PSZ_J + row * 128 + q4 * 4) * 4;
        float4 sum = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(prs, off, 0, 16));
        for (int k = 1; k < g.R; ++k) {
          const float4 v =
              __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(prs, (int)(off + k * PSZ * 4), 0, 16));
          sum.x += v.x;
          sum.y += v.y;
          sum.z += v.z;
          sum.w += v.w;
        }
        *reinterpret_cast<float4*>(o0 + (j0 + j) * ojs + (long)row * a.Cin + q4 * 4) = sum;
      }
    if (rsum && tid < 128) {
      rs = 0.f;
      for (int k = 0; k < g.R; ++k) {
        const float v = __builtin_bit_cast(
            float, __builtin_amdgcn_raw_buffer_load_b32(prs, (int)((k * PSZ + W3W_JE * W3W_PSZ_J + tid) * 4), 0, 16));
        rs = k == 0 ? v : rs + v;
      }
    }
  }
  if (rsum && tid < 128) g.rowpart[(long)w * a.Cout + co0 + tid] = rs;
  if (j0 == 0)
  for (int j = dtot; j < a.J; ++j)  // the unused slots of this joint and group: zero (by the joint's first entry)
    for (int e = tid; e < 128 * 32; e += 256)
      *reinterpret_cast<float4*>(o0 + j * ojs + (long)(e >> 5) * a.Cin + (e & 31) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ __launch_bounds__(256, 1) void gconv_wgrad3w_kernel(const stgcn_gconv_wgrad_desc a, const WGG g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int ngrp = g.nco * g.nci;
  const int bid = blockIdx.x;
  const int e = bid / (ngrp * g.R), rem = bid % (ngrp * g.R);
  const int rr = rem / ngrp, grp = rem % ngrp;
  // entries (joint, first neighbour slot, neighbour count) in decreasing-degree joint order (the heaviest blocks
  // are dispatched first); a joint of degree >= 4 runs as two entries of <= 3 neighbours (its dy panels are staged
  // twice, but 64*deg accumulators would exceed the register file and its ring would be shallow).  Scratch in the
  // ring's first bytes, read before any DMA is issued.  Grid: 2V entries (the ones past the count exit at once).
  int* sdeg = reinterpret_cast<int*>(smem);
  int* order = sdeg + 64;
  int* ent = order + 64;  // [0] = count, then (joint, j0, n) triples
  const int tid = threadIdx.x;
  if (tid < a.V) sdeg[tid] = a.deg[tid];
  __syncthreads();
  if (tid < a.V) {
    const int d = sdeg[tid];
    int r = 0;
    for (int u = 0; u < a.V; ++u) r += (sdeg[u] > d) | ((sdeg[u] == d) & (u < tid));
    order[r] = tid;
  }
  __syncthreads();
  if (tid == 0) {
    int E = 0;
    for (int r = 0; r < a.V; ++r) {
      const int w = order[r], d = sdeg[w];
      if (d > W3W_JE) {
        const int h = (d + 1) / 2;
        ent[1 + 3 * E] = w, ent[2 + 3 * E] = 0, ent[3 + 3 * E] = h, ++E;
        ent[1 + 3 * E] = w, ent[2 + 3 * E] = h, ent[3 + 3 * E] = d - h, ++E;
      } else {
        ent[1 + 3 * E] = w, ent[2 + 3 * E] = 0, ent[3 + 3 * E] = d, ++E;
      }
    }
    ent[0] = E;
  }
  __syncthreads();
  const int E = ent[0];
  const int wj = e < E ? ent[1 + 3 * e] : 0, j0 = e < E ? ent[2 + 3 * e] : 0, n = e < E ? ent[3 + 3 * e] : 0;
  const int dtot = e < E ? sdeg[wj] : 0;
  __syncthreads();  // every thread has its entry: the ring may overwrite the scratch
  if (e >= E) return;
  const int t0 = rr * g.tpb, t1 = min(g.ntile, t0 + g.tpb);
  switch (n) {
    case 1: wgrad3w_body<1>(a, g, smem, wj, e, j0, dtot, rr, grp, t0, t1); break;
    case 2: wgrad3w_body<2>(a, g, smem, wj, e, j0, dtot, rr, grp, t0, t1); break;
    case 3: wgrad3w_body<3>(a, g, smem, wj, e, j0, dtot, rr, grp, t0, t1); break;
    default:  // deg 0: no pairs; part 0 writes the zero slots and the row sums
      if (rr != 0) break;
      const int co0 = (grp % g.nco) * 128, ci0 = (grp / g.nco) * 128;
      if (g.rowpart != nullptr && grp / g.nco == 0 && tid < 128) {
        const bf16* dy = reinterpret_cast<const bf16*>(a.dy);
        float s = 0.f;
        for (int i = 0; i < a.NT; ++i) s += (float)dy[((long)i * a.V + wj) * a.dy_ld + co0 + tid];
        g.rowpart[(long)wj * a.Cout + co0 + tid] = s;
      }
      for (int i = tid; i < a.J * 128 * 128; i += blockDim.x) {
        const int j = i >> 14, co = (i >> 7) & 127, ci = i & 127;
        g.slab[(((long)wj * a.J + j) * a.Cout + co0 + co) * a.Cin + ci0 + ci] = 0.f;
      }
      break;
  }
}

// fp32 parity path of the gather wgrad: one thread per (pair, co, ci), loop over rows (small sizes)
__global__ void gconv_wgrad_f32_kernel(const stgcn_gconv_wgrad_desc a) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)a.V * a.J * a.Cout * a.Cin;
  if (idx >= total) return;
  const int ci = (int)(idx % a.Cin);
  const int co = (int)((idx / a.Cin) % a.Cout);
  const int pair = (int)(idx / ((long)a.Cin * a.Cout));
  const int w = pair / a.J, j = pair % a.J;
  if (j >= a.deg[w]) {
    a.dweff[idx] = 0.f;
    return;
  }
  const int src = a.nbr[pair];
  const float* dy = reinterpret_cast<const float*>(a.dy);
  const float* x = reinterpret_cast<const float*>(a.x);
  float s = 0.f;
  for (int i = 0; i < a.NT; ++i)
    s += dy[((long)i * a.V + w) * a.dy_ld + co] * x[((long)i * a.V + src) * a.x_ld + ci];
  a.dweff[idx] = s;
}

// out[e] = sum_r part[r][e] in fixed order (per-joint row-sum partials of the joint-grouped kernel)
__global__ void rowpart_sum_kernel(const float* __restrict__ part, int R, long E, float* __restrict__ out) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  float s = 0.f;
  for (int r = 0; r < R; ++r) s += part[(long)r * E + e];
  out[e] = s;
}

// gslab_reduce (blocks [0, nb1)) and rowpart_sum (the rest) of one joint-grouped wgrad in one launch
__global__ void gslab_rowpart_kernel(const float* __restrict__ slab, int R, long E, long EC, const int* deg, int J,
                                     float* __restrict__ dweff, int nb1, const float* __restrict__ rpart, long ER,
                                     float* __restrict__ rowsum) {
  if ((int)blockIdx.x < nb1) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int pair = (int)(e / EC);
    float s = 0.f;
    if (pair % J < deg[pair / J])
      for (int r = 0; r < R; ++r) s += slab[(long)r * E + e];
    dweff[e] = s;
    return;
  }
  const long e = (long)(blockIdx.x - nb1) * blockDim.x + threadIdx.x;
  if (e >= ER) return;
  float s = 0.f;
  for (int r = 0; r < R; ++r) s += rpart[(long)r * ER + e];
  rowsum[e] = s;
}

// slab reduction (rows of the slab are whole [V*J][Cout][Cin] images): dweff[e] = sum_r slab[r][e]
__global__ void gslab_reduce_kernel(const float* __restrict__ slab, int R, long E, long EC, const int* deg, int J,
                                    float* __restrict__ out) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int pair = (int)(e / EC);
  float s = 0.f;
  if (pair % J < deg[pair / J])  // slab slots of unused pairs are never written (nor read)
    for (int r = 0; r < R; ++r) s += slab[(long)r * E + e];
  out[e] = s;
}

// ------------------------------------------------------------------ the plan
// Which kernel computes dWeff for a shape, its geometry, and where its partials live in the caller's workspace.
// plan_wgrad() is the only place that decides; gconv_wgrad_workspace() reports the plan's size and
// gconv_wgrad_launch() validates the buffer against the same size and carves it at the same offsets.
enum WgradKernel {
  WG_F32,   // gconv_wgrad_f32_kernel: fp32 parity path, no workspace
  WG_PAIR,  // gconv_wgrad_kernel: block per (pair, 64 x 64 group, row range), any channel counts
  WG_REG,   // gconv_wgrad2_kernel: joint-grouped, register-staged
  WG_RING,  // gconv_wgrad3_kernel: joint-grouped, DMA ring
  WG_WIDE,  // gconv_wgrad3w_kernel: 128 x 128 groups, row parts merged in-kernel
};
struct WgradPlan {
  WgradKernel kernel;
  WGG g;        // geometry; the launch sets the pointers
  bool direct;  // the kernel writes dWeff, the zero slots and the row sums itself: no slab, no reduction launch
  bool split;   // ring kernel, direct: joints of degree >= W3_SPLIT_DEG run as two half-row-range blocks
  // workspace, laid out in this order (0 = absent)
  long slab_floats;     // [R][V*J][Cout][Cin] block partials
  long rowpart_floats;  // [R][V][Cout] partial row sums of dy (joint-grouped kernels, when row sums are asked for)
  long part_floats;     // partials merged in-kernel: split [V][ngrp][2][J*4096 + 64], wide [2V][ngrp][R][3*16384 + 128]
  long cnt_bytes;       // their arrival counters (split [V*ngrp], wide [2V*ngrp]; 16-B padded), zeroed per launch
  long slab_off, rowpart_off, part_off, cnt_off, total;  // bytes
  long grid;
  int block;
  size_t lds;
};

// at most `want` row parts, none empty
void set_row_parts(WGG& g, long want) {
  long R = want;
  if (R > g.ntile) R = g.ntile;
  if (R < 1) R = 1;
  g.tpb = (int)((g.ntile + R - 1) / R);
  g.R = (g.ntile + g.tpb - 1) / g.tpb;
}

// DMA-ring block target once a joint has several channel groups: 512 at C = 128 (100 groups: R = 6, 67 + 12 us
// with the slab reduction, against 87 + 9 at R = 3), 256 from 200 groups up (128 -> 256: R = 2, 114 + 13 us vs
// 127 + 15 at R = 3; C = 256: R = 1).  A plan with R = 1 (one row range per block) writes dWeff and the row
// sums directly, with no slab and no reduction launch (C = 256: 114-123 us vs 117 + 25 us at R = 2)
constexpr long W3_WIDE_TARGET = 256;
// DMA ring: block target by the group count, measured per layer (targets 512 / 1024 / 2048): C = 64
// (25 groups) 49 / 40 / 56 us, C = 128 64 / 81 / 75 us, C = 256 108 / 113 / 130 us
constexpr long W3_NARROW_TARGET = 1024;
constexpr long W2_TARGET = 512;   // register-staged kernel: three blocks fit a CU
constexpr long W3W_TARGET = 256;  // wide kernel: one block per CU

WgradPlan plan_wgrad(const stgcn_gconv_wgrad_desc& a, int dtype) {
  WgradPlan p{};
  WGG& g = p.g;
  const long E = (long)a.V * a.J * a.Cout * a.Cin;
  p.block = 256;
  if (dtype != 1) {
    p.kernel = WG_F32;  // one thread per element of dWeff
    p.direct = true;
    p.grid = (E + 255) / 256;
    return p;
  }
  const bool grouped = a.J <= J2 && a.Cin % 64 == 0 && a.Cout % 64 == 0;  // the joint-grouped kernels' shapes
  // wide: taken where the machine fills with at most 2 row parts (C = 256: 100 groups; tools/bench_conv.py, us, wide
  // vs the 64 x 64 plans: C = 256 98.7 vs 101.5; with more parts the last arriver's serial merge of R partials
  // dominates: C = 128 (R = 8) 162 vs 73.5, 128 -> 256 (R = 4) 156 vs 126)
  const bool wide = grouped && a.Cin % 128 == 0 && a.Cout % 128 == 0 && a.V <= 64 && a.J <= 2 * W3W_JE &&
                    W3W_TARGET / ((long)a.V * (a.Cout / 128) * (a.Cin / 128)) <= 2;
  if (wide) {
    p.kernel = WG_WIDE;
    g.ntile = (a.NT + 31) / 32;
    g.nco = a.Cout / 128;
    g.nci = a.Cin / 128;
    const long groups = (long)a.V * g.nco * g.nci;
    set_row_parts(g, W3W_TARGET / groups);
    p.direct = true;
    if (g.R > 1) {  // 2V entries: a joint of degree > W3W_JE runs as two
      p.part_floats = 2 * groups * g.R * ((long)W3W_JE * W3W_PSZ_J + 128);
      p.cnt_bytes = (2 * groups * 4 + 15) / 16 * 16;
    }
    p.grid = 2 * groups * g.R;
    p.lds = W3W_LDS;
  } else if (grouped) {
    // the DMA-ring kernel, except 64 -> 128 channels, where the register-staged kernel measured 74 vs 82 us
    const bool ring = !(a.Cin == 64 && a.Cout == 128);
    p.kernel = ring ? WG_RING : WG_REG;
    g.ntile = (a.NT + W2M - 1) / W2M;
    g.nco = a.Cout / W2_COB;
    g.nci = a.Cin / 64;
    const long groups = (long)a.V * g.nco * g.nci;
    const long target = !ring ? W2_TARGET : groups <= 32 ? W3_NARROW_TARGET : groups < 200 ? 512 : W3_WIDE_TARGET;
    set_row_parts(g, (target + groups - 1) / groups);
    p.direct = p.split = ring && g.R == 1;  // the only row range: partials are the result
    if (p.split) {
      p.part_floats = groups * 2 * ((long)a.J * 4096 + 64);
      p.cnt_bytes = (groups * 4 + 15) / 16 * 16;
    } else {
      p.slab_floats = (long)g.R * E;
      p.rowpart_floats = a.rowsum ? (long)g.R * a.V * a.Cout : 0;
    }
    p.grid = groups * g.R * (p.split ? 2 : 1);  // split: slot 1 only for the split joints
    p.lds = ring ? W3_LDS : W2_LDS;
  } else {
    p.kernel = WG_PAIR;
    g.ntile = (a.NT + WKM - 1) / WKM;
    g.nco = (a.Cout + 63) / 64;
    g.nci = (a.Cin + 63) / 64;
    // blocks of unused pairs exit at once; size R by all V*J pairs
    const long groups = (long)a.V * a.J * g.nco * g.nci;
    set_row_parts(g, (1024 + groups - 1) / groups);
    p.slab_floats = (long)g.R * E;
    p.grid = groups * g.R;
    p.lds = 2 * 4 * WKM * WPR;  // >= the 48 KB cross-wave reduction buffer
  }
  p.rowpart_off = p.slab_off + p.slab_floats * (long)sizeof(float);  // slab_off = 0
  p.part_off = p.rowpart_off + p.rowpart_floats * (long)sizeof(float);
  p.cnt_off = p.part_off + p.part_floats * (long)sizeof(float);
  p.total = p.cnt_off + p.cnt_bytes;
  return p;
}

}  // namespace

long gconv_wgrad_workspace(const stgcn_gconv_wgrad_desc& a, int dtype) { return plan_wgrad(a, dtype).total; }

int gconv_wgrad_launch(const stgcn_gconv_wgrad_desc& a, int dtype, hipStream_t s) {
  const long E = (long)a.V * a.J * a.Cout * a.Cin;
  if (a.phase < 0 || a.phase > 2) return STGCN_EBADSHAPE;
  if (dtype == 1 && (a.Cin % 8 || a.Cout % 8 || a.x_ld % 8 || a.dy_ld % 8)) return STGCN_EBADSHAPE;
  const WgradPlan p = plan_wgrad(a, dtype);
  if (p.kernel == WG_F32) {
    if (a.phase == 2) return STGCN_OK;  // one kernel, run in phase 1
    hipLaunchKernelGGL(gconv_wgrad_f32_kernel, dim3((unsigned)p.grid), dim3(p.block), 0, s, a);
    return hipGetLastError() == hipSuccess ? STGCN_OK : STGCN_EHIP;
  }
  if (p.kernel == WG_WIDE && a.phase == 2) return STGCN_OK;  // one kernel, run in phase 1
  if (p.kernel == WG_PAIR && a.rowsum) return STGCN_EBADSHAPE;  // row sums ride only on the joint-grouped kernels
  if (p.total && (!a.work || a.work_bytes < p.total)) return STGCN_EBADSHAPE;
  char* const work = reinterpret_cast<char*>(a.work);
  WGG g = p.g;
  if (p.direct) {
    g.slab = a.dweff;
    g.rowpart = a.rowsum;
    g.zero_unused = 1;
  } else {
    g.slab = reinterpret_cast<float*>(work + p.slab_off);
    g.rowpart = p.rowpart_floats ? reinterpret_cast<float*>(work + p.rowpart_off) : nullptr;
  }
  if (p.part_floats) {  // partials merged in-kernel: the arrival counters are zeroed ahead of every kernel launch
    g.part = reinterpret_cast<float*>(work + p.part_off);
    g.cnt = reinterpret_cast<unsigned*>(work + p.cnt_off);
    if (a.phase != 2 && hipMemsetAsync(g.cnt, 0, (size_t)p.cnt_bytes, s) != hipSuccess) return STGCN_EHIP;
  }
  void (*const k)(const stgcn_gconv_wgrad_desc, const WGG) = p.kernel == WG_WIDE   ? gconv_wgrad3w_kernel
                                                             : p.kernel == WG_RING ? gconv_wgrad3_kernel
                                                             : p.kernel == WG_REG  ? gconv_wgrad2_kernel
                                                                                   : gconv_wgrad_kernel;
  if (stgcn_lds_attr((const void*)k, 160 * 1024, s)) return STGCN_EHIP;
  if (a.phase != 2) hipLaunchKernelGGL(k, dim3((unsigned)p.grid), dim3(p.block), p.lds, s, a, g);
  if (p.direct || a.phase == 1) return hipGetLastError() == hipSuccess ? STGCN_OK : STGCN_EHIP;
  if (p.rowpart_floats) {  // slab reduction and row sums in one launch
    const long ER = (long)a.V * a.Cout;
    const int nb1 = (int)((E + 255) / 256);
    hipLaunchKernelGGL(gslab_rowpart_kernel, dim3((unsigned)(nb1 + (ER + 255) / 256)), dim3(256), 0, s,
                       (const float*)g.slab, g.R, E, (long)a.Cout * a.Cin, a.deg, a.J, a.dweff, nb1,
                       (const float*)g.rowpart, ER, a.rowsum);
  } else {
    hipLaunchKernelGGL(gslab_reduce_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, (const float*)g.slab,
                       g.R, E, (long)a.Cout * a.Cin, a.deg, a.J, a.dweff);
  }
  return hipGetLastError() == hipSuccess ? STGCN_OK : STGCN_EHIP;
}

