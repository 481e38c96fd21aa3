// The stages of the per-frame (continual inference) routes: each stage has ONE body here; the __global__ kernels of
// rt_fused.hip, co_frame.hip, rt_streams.hip, co_streams.hip and co_streams_clip.hip set up pointers, call the stages and
// place the barriers between them.  A stage that reduces over the block is a template on the block size NTH (tid-stride loops and
// block_sum fix the order of its sums), and every kernel instantiates it with its own block size:
//
//   stage                          kernel (NTH)
//   frame_head_in<NTH>             rt_in_kernel (256), cs_in_kernel (256), rt_streams_kernel (512)
//   frame_head_out<NTH>            rt_out_kernel (1024), cs_out_kernel (256), rt_streams_kernel (512)
//   conv_tile_acc<T, TU>           rt_streams_kernel (T, 4), cs_gcn_kernel (float, 4)
//   amix_coeffs / amix_mma         rt_streams_kernel (coefficients ahead of the k-loop), cs_gcn_kernel (inside the mix)
//   co_push_stage<T, NTH>          cs_push_kernel<T> (1024, stream b); co_push_kernel<T> keeps the same body of its own
//   co_finish_stage<NTH>           co_finish_kernel (1024, stream 0), cs_finish_kernel (1024, stream b)
//   ring_unit / load_ring<T>       cs_taps_kernel<T, TU>; co_taps_kernel<T> keeps its load_a<T>(ring, ...)
//   ln_stats_units<NTH, U>         rt_streams_kernel (512), the push / finish stages (1024)
// The co-st-gcn clip route (co_streams_clip.hip: frame t of a clip in the place of stream b) goes through
// clip_ops.h, which instantiates the heads, conv_tile_acc / amix_*, co_push_stage and ring_unit like co_streams.hip;
// its finish_frame restates co_finish_stage's arithmetic with the residual row taken from the clip's linear buffer (no
// ring head to read or store).
//
// rt_frame_kernel (the one-launch persistent kernel of rt_fused.hip) keeps its own bodies: its sums go through DPP
// reductions in another fixed order.  It shares the constants below only.  The dot8 graph conv of rt_gcn_kernel and
// co_gcn_kernel is not a stage here: shared, rt_gcn_kernel measured 0.27 us per launch slower.
#pragma once
#include "common.h"

// shape limits of every per-frame route
constexpr int VMAX = 32;    // joints: the 32-row MFMA operand
constexpr int CMAX = 256;   // channels per layer
constexpr int PMAX = 3;     // graph partitions
constexpr int FMAX = 16;    // input features per joint (the input head's in_feat)
constexpr int KTMAX = 69;   // temporal taps (co-st-gcn)
constexpr int MAXE = 7680;  // V * C of the routes that keep a frame in one workgroup's LDS / registers
constexpr int XPAD = 4;     // LDS row stride = C + XPAD floats: the 32 rows of a fragment read spread over the banks
constexpr int GCN_CB = 2;   // output channels per rt_gcn / co_gcn block (Cout / 2 blocks stream the weight rows)

// 16-k steps of the packed [tile][k-step][lane][8] weight image of a Kt-tap conv over C channels
constexpr int num_ksteps(int C, int Kt) { return (Kt * C + 15) / 16; }
// co-st-gcn rings: activation slots of a Kt-tap, dilation-S conv; slots of the residual delayed by Kt / 2 frames
constexpr int ring_slots(int S, int Kt) { return S * (Kt - 1) + 1; }
constexpr int res_slots(int Kt) { return Kt / 2 + 1; }
// slot of the newest frame, from the stored index of the previous one: the rings advance downwards
DEV int ring_head(int i, int n) { return (i + n - 1) % n; }

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

// ------------------------------------------------------------------------------------------- heads
// The descriptors' F field: 0 (a descriptor filled before the field existed) reads as 3
__host__ __device__ inline int head_feats(int F) { return F == 0 ? 3 : F; }
// F as given in a descriptor is usable: 0 or 1 .. FMAX, and the unbiased variance over F * V values exists
inline bool head_feats_ok(int F, int V) { return F >= 0 && F <= FMAX && head_feats(F) * V >= 2; }

// fcn_in of one output: b + sum over c < F of w[c] * xn[c * V], the fmaf chain in ascending c from the bias.  FC > 0
// is F at compile time (the chain unrolled); both forms give the same bits.
template <int FC>
DEV float head_dot(const float* __restrict__ w, const float* xn, int F, int V, float b) {
  if constexpr (FC > 0) {
#pragma unroll
    for (int c = 0; c < FC; ++c) b = fmaf(w[c], xn[c * V], b);
  } else {
    for (int c = 0; c < F; ++c) b = fmaf(w[c], xn[c * V], b);
  }
  return b;
}

// Input head: LayerNorm([F,1,V]) (per frame, two-pass, unbiased variance) + fcn_in (1x1 conv + bias) of the frame x
// (element c*V + v) -> rows out[v * ld + co].  xi: F * V floats of LDS, red: NTH / 64.  No trailing barrier.
template <int NTH>
DEV void frame_head_in(const float* __restrict__ x, int F, int V, int C0, const float* __restrict__ ln_w,
                       const float* __restrict__ ln_b, const float* __restrict__ w_in, const float* __restrict__ b_in,
                       float* xi, float* red, float* out, int ld) {
  const int tid = threadIdx.x, n = F * V;
  for (int i = tid; i < n; i += NTH) xi[i] = x[i];
  __syncthreads();
  float s = 0.f;
  for (int i = tid; i < n; i += NTH) s += xi[i];
  const float mean = block_sum(s, red) / (float)n;
  float q = 0.f;
  for (int i = tid; i < n; i += NTH) {
    const float t = xi[i] - mean;
    q = fmaf(t, t, q);
  }
  const float rstd = 1.f / sqrtf(block_sum(q, red) / (float)(n - 1) + 1e-5f);
  __syncthreads();
  for (int i = tid; i < n; i += NTH) xi[i] = fmaf(ln_w[i], (xi[i] - mean) * rstd, ln_b[i]);
  __syncthreads();
  // F == 3 (skeleton coordinates) keeps the unrolled chain it had before F became a runtime value: with the runtime
  // loop alone the bf16 stream-batch tick measured 1.4 - 1.6 % slower
  if (F == 3) {
    for (int i = tid; i < V * C0; i += NTH) {
      const int v = i / C0, co = i - v * C0;
      out[v * ld + co] = head_dot<3>(w_in + co * 3, xi + v, 3, V, b_in[co]);
    }
  } else {
    for (int i = tid; i < V * C0; i += NTH) {
      const int v = i / C0, co = i - v * C0;
      out[v * ld + co] = head_dot<0>(w_in + co * F, xi + v, F, V, b_in[co]);
    }
  }
}

// Output head: mean over the V joints of the rows y[v * ld + c] -> fcn_out (+ bias) -> out[K]; one wave per class, the
// channels over the lanes.  pool: C floats of LDS.
template <int NTH>
DEV void frame_head_out(const float* y, int ld, int V, int C, const float* __restrict__ w_out,
                        const float* __restrict__ b_out, int K, float* pool, float* out) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int c = tid; c < C; c += NTH) {
    float s = 0.f;
    for (int v = 0; v < V; ++v) s += y[v * ld + c];
    pool[c] = s / (float)V;
  }
  __syncthreads();
  for (int k = w; k < K; k += NTH / 64) {
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s = fmaf(w_out[(long)k * C + c], pool[c], s);
    s = wave_sum(s);
    if (lane == 0) out[k] = s + (b_out ? b_out[k] : 0.f);
  }
}

// ------------------------------------------------------------------------------------------- graph conv, MFMA form
// Y[u][co] = sum_ci x[u][ci] W[co][ci] of one 32-channel tile: the k-loop over the tile's packed panel, TU k-steps in
// flight; A operand = the fp32 rows xs (row stride ldx) as T, B operand = the panel
template <typename T, int TU>
DEV f32x16 conv_tile_acc(const T* panel, const float* xs, int ldx, int nks, int row, int h, int V, int Cin,
                         int lane) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int kb = 0; kb < nks; kb += TU) {
    typename Tr<T>::frag fa[TU], fb[TU];
#pragma unroll
    for (int u = 0; u < TU; ++u) fb[u] = load_b<T>(panel, kb + u, nks, lane);
#pragma unroll
    for (int u = 0; u < TU; ++u) fa[u] = load_a_as<T>(xs, ldx, kb + u, nks, row, h, V, Cin);
#pragma unroll
    for (int u = 0; u < TU; ++u) Tr<T>::mma(acc, fa[u], fb[u]);
  }
  return acc;
}

// The A-mix on the accumulators where they are: accumulator register r of lane l holds Y_p[acc_row(r, l)][co], which IS
// the B operand (k = l >> 5, n = l & 31) of an MFMA whose two k are u = acc_row(r, 0) and acc_row(r, 32); with A operand
// am[r] = A[p][u = acc_row(r, lane)][v = lane & 31] sixteen MFMAs give z[v][co] += sum_u A[p][u][v] Y_p[u][co].
// A stays the uniform base pointer (p goes into the 32-bit offset: a pointer A + p*V*V with p derived from the wave index
// would cost a 64-bit address register pair per load); !on: zeros (a task that mixes nothing).
DEV void amix_coeffs(const float* __restrict__ A, int p, int V, int lane, bool on, float (&am)[16]) {
  const int row = lane & 31;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int u = acc_row(r, lane);
    am[r] = (on && u < V && row < V) ? A[(p * V + u) * V + row] : 0.f;
  }
}
DEV void amix_mma(const float (&am)[16], const f32x16& acc, f32x16& z) {
#pragma unroll
  for (int r = 0; r < 16; ++r) z = __builtin_amdgcn_mfma_f32_32x32x2f32(am[r], acc[r], z, 0, 0, 0);
}

// ------------------------------------------------------------------------------------------- co-st-gcn push / finish
constexpr int co_units(int nth) { return (VMAX * CMAX / 4 + nth - 1) / nth; }  // float4 units of a frame per thread
// One stream's slice of a co-st-gcn layer (stgcn_co_layer: stream 0 of 1; stgcn_co_streams_layer: stream b): every
// pointer already offset to the stream
struct CoView {
  int V, C, Kt, S, res_mode;
  const float* z;    // [V][C] graph conv
  const float* res;  // [V][C] residual source: the layer's input (res_mode 1) | the residual conv (res_mode 2)
  float* res_ring;   // [res_slots][V][C]
  int* idx;          // int[2]
  const float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *lnr_w, *lnr_b;
  const float* bt;
  float* y;
};
// d: either layer descriptor (the same field names); x: the layer's input rows.  The activation ring has the compute
// dtype's elements: co_push_stage takes the stream's slots as a typed pointer.
template <typename D>
DEV CoView co_view(const D& d, int V, const float* x, long b) {
  const long E = (long)V * d.Cout;
  CoView v;
  v.V = V, v.C = d.Cout, v.Kt = d.Kt, v.S = d.S, v.res_mode = d.res_mode;
  v.z = d.z_buf + b * E;
  v.res = d.res_mode == 2 ? d.r_buf + b * E : x ? x + b * E : nullptr;  // read by the push stage; mode 1: Cin == Cout
  v.res_ring = d.res_ring + b * res_slots(d.Kt) * E;
  v.idx = d.idx + b * 2;
  v.ln1_w = d.ln1_w, v.ln1_b = d.ln1_b, v.ln2_w = d.ln2_w, v.ln2_b = d.ln2_b, v.lnr_w = d.lnr_w, v.lnr_b = d.lnr_b;
  v.bt = d.bt;
  v.y = d.y + b * E;
  return v;
}

// ring[head] = ReLU(LN1(z)) in T; res_ring[rhead] = x | LN_r(r).  ring: the stream's slots as T.  red: NTH / 64.
template <typename T, int NTH>
DEV void co_push_stage(const CoView d, T* ring, int head, int rhead, float* red) {
  constexpr int U = co_units(NTH);
  const int tid = threadIdx.x, V = d.V, C = d.C, n4 = V * C / 4;
  const long E = (long)V * C;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 z[U], r[U];
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const int e4 = tid + NTH * j;
    z[j] = e4 < n4 ? reinterpret_cast<const float4*>(d.z)[e4] : zero;
    r[j] = e4 < n4 && d.res_mode ? reinterpret_cast<const float4*>(d.res)[e4] : zero;
  }
  const float2 st = ln_stats_units<NTH>(z, n4, red);
  float2 sr = make_float2(0.f, 1.f);
  if (d.res_mode == 2) sr = ln_stats_units<NTH>(r, n4, red);
  T* slot = ring + head * E;
  float* rslot = d.res_ring + rhead * E;
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const int e4 = tid + NTH * j;
    if (e4 < n4) {
      store4(slot + e4 * 4, relu4(ln_apply4(z[j], st, d.ln1_w, d.ln1_b, e4, V, C)));
      if (d.res_mode == 1) store4(rslot + e4 * 4, r[j]);
      if (d.res_mode == 2) store4(rslot + e4 * 4, ln_apply4(r[j], sr, d.lnr_w, d.lnr_b, e4, V, C));
    }
  }
}

// u = bt + sum_s partial[s] (index order; partial: the stream's [nsplit][V][C]), y = relu(LN2(u) + res_ring[(rhead +
// Kt/2) % R]); stores both ring heads
template <int NTH>
DEV void co_finish_stage(const CoView d, const float* __restrict__ partial, int nsplit, float* red) {
  constexpr int U = co_units(NTH);
  const int tid = threadIdx.x, V = d.V, C = d.C, n4 = V * C / 4;
  const long E = (long)V * C;
  const int R = res_slots(d.Kt);
  const int head = ring_head(d.idx[0], ring_slots(d.S, d.Kt)), rhead = ring_head(d.idx[1], R);
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 u[U];
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const int e4 = tid + NTH * j;
    u[j] = zero;
    if (e4 < n4) {
      const int c = (e4 * 4) % C;
      float4 t = d.bt ? *reinterpret_cast<const float4*>(d.bt + c) : zero;
      const float4* p = reinterpret_cast<const float4*>(partial) + e4;
#pragma unroll 4
      for (int s = 0; s < nsplit; ++s) t = add4(t, p[(long)s * n4]);
      u[j] = t;
    }
  }
  const float2 st = ln_stats_units<NTH>(u, n4, red);
  const float* rslot = d.res_ring + ((rhead + d.Kt / 2) % R) * E;
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const int e4 = tid + NTH * j;
    if (e4 < n4) {
      float4 o = ln_apply4(u[j], st, d.ln2_w, d.ln2_b, e4, V, C);
      if (d.res_mode) o = add4(o, reinterpret_cast<const float4*>(rslot)[e4]);
      reinterpret_cast<float4*>(d.y)[e4] = relu4(o);
    }
  }
  __syncthreads();  // every read of idx precedes the update
  if (tid == 0) {
    d.idx[0] = head;
    d.idx[1] = rhead;
  }
}

// ------------------------------------------------------------------------------------------- co-st-gcn tap GEMM
// Unit q (4 elements) of k-step ks that wave half h reads: kk = 16 ks + 8 h + 4 q = tap * C + ci (C % 4 == 0: one ring
// slot); false (and tap = ci = 0) beyond ks1 and Ktot = Kt * C
DEV bool ring_unit(int ks, int ks1, int h, int q, int C, int Ktot, int& tap, int& ci) {
  const int kk = ks * 16 + 8 * h + 4 * q;
  const bool in = ks < ks1 && kk < Ktot;
  tap = in ? kk / C : 0;
  ci = in ? kk - tap * C : 0;
  return in;
}

// A fragment of one stream: 8 consecutive kk = tap * C + ci from slot (head + tap * S) % fifo, row `row`
template <typename T>
DEV typename Tr<T>::frag load_ring(const T* __restrict__ ring, bool ok, int row, int V, int C, int S, int fifo, int head,
                                   const int (&tap)[2], const int (&ci)[2], const bool (&in)[2]) {
  T f[8];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (ok && in[u]) {
      int slot = head + tap[u] * S;  // head < fifo, tap * S <= fifo - 1
      if (slot >= fifo) slot -= fifo;
      load4(ring + ((long)slot * V + row) * C + ci[u], f + 4 * u);
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
