// The stages of a co-st-gcn clip (T consecutive frames of one stream, every layer's temporal conv as one causal GEMM) as
// __device__ functions on ONE stream's buffers.  co_streams_clip.hip (B streams per call, one stream's clip as B = 1:
// the pointers offset to stream b, the frame count n_b and the restart flag read on the device) sets up the pointers,
// calls these and keeps the launch order; the arithmetic and the order of every sum live here.
//
// D is stgcn_co_clip_layer.  n is the number of frames the stream consumes in this call.  hist / resq are the stream's
// linear clip buffers of co_streams_clip.hip's header comment.
#pragma once
#include "common.h"
#include "frame_ops.h"

namespace clip_ops {

constexpr int HNT = 256;   // in / out block
constexpr int GNT = 512;   // gcn block
constexpr int GNW = GNT / 64;
constexpr int FNT = 1024;  // push / finish / state block: V * C <= 8192 in 2 float4 units per thread
constexpr int TNT = 512;   // taps block
constexpr int TNW = TNT / 64;
constexpr int G = 4;       // 32-row tiles per tap block: 4 x 16 accumulator registers per wave
constexpr int GTU = 4;     // k-steps in flight per wave in the gcn stage
constexpr int MAX_SPLITS = 8;

// K splits of a layer's tap stage: co_streams_num_splits' rule (16 k-steps per wave, at most 8), a function of
// (Cout, Kt) and the forced count alone, never of B, T, t0 or the device, so that a frame's sums have one order
inline int num_splits(int Cout, int Kt, int forced) {
  const int nks = num_ksteps(Cout, Kt), ntile = (Cout + 31) / 32;
  const int nsub = ntile >= TNW ? 1 : TNW / ntile;
  int n = forced;
  if (n <= 0) {
    n = nks / (16 * nsub);
    if (n > MAX_SPLITS) n = MAX_SPLITS;
  }
  if (n > nks) n = nks;
  return n < 1 ? 1 : n;
}

// ---------------------------------------------------------------------------------------------------- heads
// x: channel c of the frame at x[c * x_stride + v]; xf / xi: F * V floats of LDS each, red: HNT / 64
DEV void in_frame(const float* __restrict__ x, long x_stride, int F, int V, int C0, const float* __restrict__ ln_w,
                  const float* __restrict__ ln_b, const float* __restrict__ w_in, const float* __restrict__ b_in,
                  float* xf, float* xi, float* red, float* __restrict__ h0) {
  for (int i = threadIdx.x; i < F * V; i += HNT) {
    const int c = i / V, v = i - c * V;
    xf[i] = x[c * x_stride + v];
  }
  __syncthreads();
  frame_head_in<HNT>(xf, F, V, C0, ln_w, ln_b, w_in, b_in, xi, red, h0, C0);
}

// ---------------------------------------------------------------------------------------------------- gcn
// cs_gcn_kernel's body for one frame: x [V][Cin] -> z [V][Cout], r [V][Cout] (res_mode 2); xs: VMAX * (CMAX + XPAD)
template <typename D>
DEV void gcn_frame(const D& ly, int V, const float* __restrict__ x, float* __restrict__ zdst, float* __restrict__ rdst,
                   float* xs) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, row = lane & 31, h = lane >> 5;
  const int Cin = ly.Cin, Cout = ly.Cout, P = ly.P, ldx = Cin + XPAD, K4 = Cin / 4;
  const float4* xb = reinterpret_cast<const float4*>(x);
  for (int i = tid; i < V * K4; i += GNT) {
    const int v = i / K4, k = i - v * K4;
    *reinterpret_cast<float4*>(xs + v * ldx + 4 * k) = xb[i];
  }
  __syncthreads();
  const int ntile = (Cout + 31) / 32, nks = (Cin + 15) / 16;
  const int ntask = ntile * (ly.res_mode == 2 ? 2 : 1);
  for (int task = w; task < ntask; task += GNW) {
    const bool res = task >= ntile;
    const int tile = res ? task - ntile : task;
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    for (int p = 0; p < (res ? 1 : P); ++p) {
      const float* panel = (res ? ly.wrp : ly.wp + (long)p * ntile * nks * 512) + (long)tile * nks * 512;
      const f32x16 acc = conv_tile_acc<float, GTU>(panel, xs, ldx, nks, row, h, V, Cin, lane);
      if (res) {
        z = acc;
      } else {  // z[v][co] += sum_u A_p[u][v] Y_p[u][co]
        float am[16];
        amix_coeffs(ly.A, p, V, lane, true, am);
        amix_mma(am, acc, z);
      }
    }
    const int co = tile * 32 + row;
    if (co < Cout) {
      const float add = res && ly.br ? ly.br[co] : 0.f;
      float* dst = res ? rdst : zdst;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int v = acc_row(r, lane);
        if (v < V) dst[v * Cout + co] = z[r] + (res ? add : (ly.bias2d ? ly.bias2d[v * Cout + co] : 0.f));
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------- push + carry
// co_push_stage of frame t: z, res = the frame's rows -> hist[fifo-1+t], resq[Kt/2+t]
template <typename T, typename D>
DEV void push_frame(const D& ly, int V, int t, const float* z, const float* res, T* hist, float* resq, float* red) {
  CoView d;
  d.V = V, d.C = ly.Cout, d.Kt = ly.Kt, d.S = ly.S, d.res_mode = ly.res_mode;
  d.z = z;
  d.res = res;
  d.res_ring = resq;
  d.idx = nullptr;
  d.ln1_w = ly.ln1_w, d.ln1_b = ly.ln1_b, d.ln2_w = ly.ln2_w, d.ln2_b = ly.ln2_b;
  d.lnr_w = ly.lnr_w, d.lnr_b = ly.lnr_b;
  d.bt = ly.bt;
  d.y = nullptr;
  co_push_stage<T, FNT>(d, hist, ring_slots(ly.S, ly.Kt) - 1 + t, res_slots(ly.Kt) - 1 + t, red);
}

// one [V][C] row block copied as it is
template <typename T>
DEV void copy_rows(const T* __restrict__ src, T* __restrict__ dst, int n4) {
  for (int e4 = threadIdx.x; e4 < n4; e4 += FNT) {
    T f[4];
    load4(src + e4 * 4, f);
    if constexpr (sizeof(T) == 4) {
      *reinterpret_cast<float4*>(dst + e4 * 4) = make_float4(f[0], f[1], f[2], f[3]);
    } else {
      bf16x4 o;
      o[0] = f[0], o[1] = f[1], o[2] = f[2], o[3] = f[3];
      *reinterpret_cast<bf16x4*>(dst + e4 * 4) = o;
    }
  }
}

// the empty FIFO's activation row, ReLU(LN1(0)) = ReLU(ln1_b), as cs_push_kernel writes it on a restart
template <typename T>
DEV void empty_rows(const float* __restrict__ ln1_b, T* __restrict__ dst, int V, int C) {
  for (int e4 = threadIdx.x; e4 < V * C / 4; e4 += FNT) store4(dst + e4 * 4, relu4(ln_param4(ln1_b, e4, V, C)));
}
DEV void zero_rows(float* __restrict__ dst, int n4) {
  for (int e4 = threadIdx.x; e4 < n4; e4 += FNT) store4(dst + e4 * 4, make_float4(0.f, 0.f, 0.f, 0.f));
}

// Carry block p of fifo-1 + Kt/2: p < fifo-1 is hist position p, the frame of age fifo-2-p (age 0 = the newest carried
// frame, ring slot idx[0]); the others resq position q = p - (fifo-1), the residual of age Kt/2-1-q (slot idx[1]).  A
// restarting stream carries the empty FIFO: nothing of ring, res_ring or idx is read.
template <typename T, typename D>
DEV void carry_block(const D& ly, int V, int p, bool restart, const T* ring, const float* res_ring, const int* idx,
                     T* hist, float* resq) {
  const int C = ly.Cout, n4 = V * C / 4;
  const long E = (long)V * C;
  const int fifo = ring_slots(ly.S, ly.Kt), R = res_slots(ly.Kt), Hh = fifo - 1, Hr = R - 1;
  if (p < Hh) {
    if (restart) {
      empty_rows<T>(ly.ln1_b, hist + p * E, V, C);
    } else {
      const int slot = (idx[0] + (Hh - 1 - p)) % fifo;
      copy_rows<T>(ring + slot * E, hist + p * E, n4);
    }
  } else if (ly.res_mode) {
    const int q = p - Hh;
    if (restart) {
      zero_rows(resq + q * E, n4);
    } else {
      const int slot = (idx[1] + (Hr - 1 - q)) % R;
      copy_rows<float>(res_ring + slot * E, resq + q * E, n4);
    }
  }
}

// ---------------------------------------------------------------------------------------------------- taps
// The 8 waves of a block over the layer's column tiles, as in cs_taps_kernel: nsub = max(1, 8 / ntile) waves share a
// tile and interleave its k-steps.  A function of Cout alone.
DEV int taps_nsub(int ntile) { return ntile >= TNW ? 1 : TNW / ntile; }

// A fragment of row m (the clip's dense row t*V + v) for one k-step: 8 consecutive kk = tap * C + ci, two 4-element
// units; tap k of row m is hist row (fifo-1)*V + m - k*S*V (>= 0: k*S <= fifo-1)
template <typename T>
DEV typename Tr<T>::frag load_hist(const T* __restrict__ hrow, bool ok, int C, int SV, const int (&tap)[2],
                                   const int (&ci)[2], const bool (&in)[2]) {
  T f[8];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (ok && in[u]) {
      load4(hrow - (long)tap[u] * SV * C + ci[u], f + 4 * u);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) f[4 * u + i] = (T)0.f;
    }
  }
  typename Tr<T>::frag a;
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = f[j];
  return a;
}

// K split s of the rows [m0, m0 + G*32) of a stream's M = n*V dense rows: partial[t][s][v][co].  red: [TNW][16][64].
template <typename T, int TU, typename D>
DEV void taps_block(const D& ly, int V, int M, int nks, int nsplit, int s, int m0, const T* __restrict__ hist,
                    float* __restrict__ partial, float (*red)[16][64]) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, row = lane & 31, h = lane >> 5;
  const int C = ly.Cout, Kt = ly.Kt, S = ly.S, Hh = ring_slots(S, Kt) - 1, Ktot = Kt * C;
  const int ntile = (C + 31) / 32, nsub = taps_nsub(ntile);
  const int tile = w / nsub, sub = w - tile * nsub;
  const bool work = tile < ntile;  // uniform over the wave
  const int ng = min(G, (M - m0 + 31) / 32);  // row tiles of this block that hold rows: uniform over the block
  const int ks0 = (int)((long)s * nks / nsplit), ks1 = (int)((long)(s + 1) * nks / nsplit);
  const T* hrow[G];
  bool ok[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int m = m0 + g * 32 + row;
    ok[g] = m < M;
    hrow[g] = hist + ((long)Hh * V + (ok[g] ? m : 0)) * C;
  }
  f32x16 acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[g][r] = 0.f;
  if (work) {
    const T* panel = reinterpret_cast<const T*>(ly.wt) + (long)tile * nks * 512;
    for (int kb = ks0 + sub; kb < ks1; kb += nsub * TU) {
      typename Tr<T>::frag bf[TU], af[TU][G];
#pragma unroll
      for (int u = 0; u < TU; ++u) bf[u] = load_b<T>(panel, kb + u * nsub, ks1, lane);
#pragma unroll
      for (int u = 0; u < TU; ++u) {
        int tap[2], ci[2];
        bool in[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) in[q] = ring_unit(kb + u * nsub, ks1, h, q, C, Ktot, tap[q], ci[q]);
#pragma unroll
        for (int g = 0; g < G; ++g) af[u][g] = load_hist<T>(hrow[g], g < ng && ok[g], C, S * V, tap, ci, in);
      }
#pragma unroll
      for (int u = 0; u < TU; ++u)
#pragma unroll
        for (int g = 0; g < G; ++g)
          if (g < ng) Tr<T>::mma(acc[g], af[u][g], bf[u]);
    }
  }
  // per row tile: the nsub interleaves of every column tile summed in index order -> partial[t][s][v][co]
  const long E = (long)V * C;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (g < ng) {  // uniform over the block
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 16; ++r) red[w][r][lane] = acc[g][r];
      __syncthreads();
      for (int o = tid; o < ntile * 16 * 64; o += TNT) {
        const int tl = o >> 10, r = (o >> 6) & 15, l = o & 63;
        float sum = 0.f;
        for (int i = 0; i < nsub; ++i) sum += red[tl * nsub + i][r][l];
        const int m = m0 + g * 32 + acc_row(r, l), co = tl * 32 + (l & 31);
        if (m < M && co < C) {
          const int t = m / V, v = m - t * V;
          partial[((long)t * nsplit + s) * E + (long)v * C + co] = sum;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------- finish
// co_finish_stage's arithmetic for one frame: partial = the frame's [nsplit][V][C], rrow = resq[t] (the residual row of
// frame t - Kt/2), y = the frame's output rows; no ring head to store.  red: FNT / 64.  ly by value: through a reference
// the compiler kept u[] in 32 bytes of scratch.
template <typename D>
DEV void finish_frame(const D ly, int V, int nsplit, const float* __restrict__ partial, const float* __restrict__ rrow,
                      float* __restrict__ yrow, float* red) {
  constexpr int U = co_units(FNT);
  const int tid = threadIdx.x, C = ly.Cout, n4 = V * C / 4;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 u[U];
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const int e4 = tid + FNT * j;
    u[j] = zero;
    if (e4 < n4) {
      const int c = (e4 * 4) % C;
      float4 a = ly.bt ? *reinterpret_cast<const float4*>(ly.bt + c) : zero;
      const float4* p = reinterpret_cast<const float4*>(partial) + e4;
#pragma unroll 4
      for (int s = 0; s < nsplit; ++s) a = add4(a, p[(long)s * n4]);
      u[j] = a;
    }
  }
  const float2 st = ln_stats_units<FNT>(u, n4, red);
  const float4* r4 = reinterpret_cast<const float4*>(rrow);
  float4* y = reinterpret_cast<float4*>(yrow);
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const int e4 = tid + FNT * j;
    if (e4 < n4) {
      float4 o = ln_apply4(u[j], st, ly.ln2_w, ly.ln2_b, e4, V, C);
      if (ly.res_mode) o = add4(o, r4[e4]);
      y[e4] = relu4(o);
    }
  }
}

// both indices moved by n frames, from (0, 0) on a restart; for one thread of the launch
DEV void advance_idx(int* idx, int S, int Kt, int n, bool restart) {
  const int fifo = ring_slots(S, Kt), R = res_slots(Kt);
  idx[0] = (((restart ? 0 : idx[0]) - n) % fifo + fifo) % fifo;
  idx[1] = (((restart ? 0 : idx[1]) - n) % R + R) % R;
}

// ---------------------------------------------------------------------------------------------------- state
// Ring slot block j of the activation ring (res = false, j < fifo) or of the residual ring (res = true, j < Kt/2+1),
// idx already advanced: the j-th newest frame of the clip (t = n-1-j) -> slot (idx + j) % slots while j < n; on a
// restart the slots the clip did not reach get the empty FIFO's row.
template <typename T, typename D>
DEV void state_block(const D& ly, int V, int n, bool res, int j, bool restart, T* ring, float* res_ring, const int* idx,
                     const T* hist, const float* resq) {
  const int C = ly.Cout, n4 = V * C / 4;
  const long E = (long)V * C;
  const int fifo = ring_slots(ly.S, ly.Kt), R = res_slots(ly.Kt);
  if (!res) {
    T* dst = ring + (long)((idx[0] + j) % fifo) * E;
    if (j < n) copy_rows<T>(hist + (long)(fifo - 1 + n - 1 - j) * E, dst, n4);
    else if (restart) empty_rows<T>(ly.ln1_b, dst, V, C);
  } else {  // res_mode 0 pushes no residual rows: only a restart writes its ring
    float* dst = res_ring + (long)((idx[1] + j) % R) * E;
    if (ly.res_mode && j < n) copy_rows<float>(resq + (long)(R - 1 + n - 1 - j) * E, dst, n4);
    else if (restart) zero_rows(dst, n4);
  }
}

}  // namespace clip_ops
