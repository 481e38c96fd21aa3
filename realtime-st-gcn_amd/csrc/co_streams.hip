// CoST-GCN per-frame inference for a batch of B independent skeleton streams (stgcn_co_streams): the four per-layer
// stages of co_frame.hip with a leading stream axis, plus the heads.  State is stream-major (ring [B][fifo][V][C] in
// the compute dtype, res_ring [B][Kt/2+1][V][C] fp32, idx [B][2]); active [B] is read on the device (0 skip, 2 restart
// then step, anything else step).  One tick = these launches on one stream, every hand-off a kernel boundary:
//
//   cs_order  : order[0] = number of active streams, order[1..] = their slots (the tap stage's groups)       (1 block)
//   cs_in     : h0[b] = fcn_in(LayerNorm([F,1,V])(x[b])): frame_head_in                           (1 block per stream)
//   per layer:
//   cs_gcn    : z[b] = gcn(x[b], A), r[b] = Wr x[b] + br.  One block per stream, x[b] in LDS; a wave owns a 32-channel
//               tile: per partition p, Y_p = x W_p^T on v_mfma_f32_32x32x2_f32 with the packed weight image (the B
//               operand: conv_tile_acc), then the A-mix on the accumulators where they are (amix_coeffs / amix_mma),
//               summed over p in the same accumulator: z never passes through LDS.
//   cs_push   : co_push_stage per stream.  Code 2 first makes every other ring slot ReLU(ln1_b), every other residual
//               slot zero and takes idx as (0, 0).
//   cs_taps   : the tap GEMM.  Grid (K splits) x (groups of G = 4 active streams); the 8 waves of a block share out the
//               layer's column tiles (taps_nsub), so one block covers every column tile of its (split, group): a weight
//               B fragment is loaded once and meets the G streams' A fragments (G MFMAs), and the column tiles'
//               re-reads of a ring element come from the same CU: HBM sees the element once.
//   cs_finish : co_finish_stage per stream.
//   cs_out    : out[b] = fcn_out(mean_v y_last[b]): frame_head_out; zeros for a skipped stream.
// The stages, the ring fragment loads (ring_unit / load_ring) and the shape limits are frame_ops.h's.
//
// Order of every sum: k-steps in sequence within a wave, the nsub K-interleaves of a tile in index order, the splits
// in index order, LayerNorm statistics as in co_frame.hip.  nsub and the default split count are functions of the
// layer's shape alone, each stream has its own accumulators, and no atomics touch floating-point data: a stream's
// outputs do not depend on B, its slot, its group, the other streams' masks or the device.
#include "common.h"
#include "launchers.h"
#include "frame_ops.h"
#include "../../include/stgcn_amd.h"

namespace {

constexpr int HNT = 256;   // cs_order / cs_in / cs_out block
constexpr int GNT = 512;   // cs_gcn block
constexpr int GNW = GNT / 64;
constexpr int FNT = 1024;  // cs_push / cs_finish block: V * C <= 8192 in 2 float4 units per thread
constexpr int TNT = 512;   // cs_taps block
constexpr int TNW = TNT / 64;
constexpr int G = 4;       // streams per tap block: 4 x 16 accumulator registers per wave
constexpr int GTU = 4;     // k-steps in flight per wave in cs_gcn
constexpr int MAX_SPLITS = 8;

using layer_t = stgcn_co_streams_layer;

// ---------------------------------------------------------------------------------------------------- heads
__global__ __launch_bounds__(HNT) void cs_order_kernel(const int* __restrict__ active, int B, int* __restrict__ order) {
  __shared__ int cnt[HNT];
  const int tid = threadIdx.x, per = (B + HNT - 1) / HNT;
  const int b0 = tid * per, b1 = min(B, b0 + per);
  int n = 0;
  for (int b = b0; b < b1; ++b) n += active[b] != 0;
  cnt[tid] = n;
  __syncthreads();
  int at = 0;
  for (int i = 0; i < tid; ++i) at += cnt[i];
  for (int b = b0; b < b1; ++b)
    if (active[b] != 0) order[1 + at++] = b;
  if (tid == HNT - 1) order[0] = at;
}

// frame_head_in of one stream's frame -> h0[b] rows [V][C0]
__global__ __launch_bounds__(HNT) void cs_in_kernel(const float* __restrict__ x, const int* __restrict__ active, int F,
                                                    int V, int C0, const float* __restrict__ ln_w,
                                                    const float* __restrict__ ln_b, const float* __restrict__ w_in,
                                                    const float* __restrict__ b_in, float* __restrict__ h0) {
  __shared__ float xi[FMAX * VMAX];
  __shared__ float red[HNT / 64];
  const long b = blockIdx.x;
  if (active[b] == 0) return;
  frame_head_in<HNT>(x + b * F * V, F, V, C0, ln_w, ln_b, w_in, b_in, xi, red, h0 + b * V * C0, C0);
}

// frame_head_out of one stream's last rows; a zero row for a skipped stream
__global__ __launch_bounds__(HNT) void cs_out_kernel(const float* __restrict__ y, const int* __restrict__ active, int V,
                                                     int C, const float* __restrict__ w_out,
                                                     const float* __restrict__ b_out, int K, float* __restrict__ out) {
  __shared__ float pool[CMAX];
  const long b = blockIdx.x;
  float* o = out + b * K;
  if (active[b] == 0) {
    for (int k = threadIdx.x; k < K; k += HNT) o[k] = 0.f;
    return;
  }
  frame_head_out<HNT>(y + b * V * C, C, V, C, w_out, b_out, K, pool, o);
}

// ---------------------------------------------------------------------------------------------------- gcn
__global__ __launch_bounds__(GNT) void cs_gcn_kernel(const layer_t ly, int V, const float* __restrict__ x,
                                                     const int* __restrict__ active) {
  __shared__ __attribute__((aligned(16))) float xs[VMAX * (CMAX + XPAD)];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, row = lane & 31, h = lane >> 5;
  const long b = blockIdx.x;
  if (active[b] == 0) return;
  const int Cin = ly.Cin, Cout = ly.Cout, P = ly.P, ldx = Cin + XPAD, K4 = Cin / 4;
  const float4* xb = reinterpret_cast<const float4*>(x + b * V * Cin);
  for (int i = tid; i < V * K4; i += GNT) {
    const int v = i / K4, k = i - v * K4;
    *reinterpret_cast<float4*>(xs + v * ldx + 4 * k) = xb[i];
  }
  __syncthreads();
  const int ntile = (Cout + 31) / 32, nks = (Cin + 15) / 16;
  const int ntask = ntile * (ly.res_mode == 2 ? 2 : 1);
  float* zb = ly.z_buf + b * V * Cout;
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
      float* dst = res ? ly.r_buf + b * V * Cout : zb;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int v = acc_row(r, lane);
        if (v < V) dst[v * Cout + co] = z[r] + (res ? add : (ly.bias2d ? ly.bias2d[v * Cout + co] : 0.f));
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------- push
template <typename T>
__global__ __launch_bounds__(FNT) void cs_push_kernel(const layer_t ly, int V, const float* __restrict__ x,
                                                      const int* __restrict__ active) {
  __shared__ float red[FNT / 64];
  const int tid = threadIdx.x, C = ly.Cout, n4 = V * C / 4;
  const long b = blockIdx.x, E = (long)V * C;
  const int code = active[b];
  if (code == 0) return;
  const bool restart = code == 2;
  const int fifo = ring_slots(ly.S, ly.Kt), R = res_slots(ly.Kt);
  const int head = ring_head(restart ? 0 : ly.idx[b * 2], fifo), rhead = ring_head(restart ? 0 : ly.idx[b * 2 + 1], R);
  const CoView d = co_view(ly, V, x, b);
  T* ring = reinterpret_cast<T*>(ly.ring) + b * fifo * E;
  if (restart) {  // an empty FIFO: ReLU(LN1(0)) = ReLU(ln1_b) in every slot but the one written below; residuals zero
#pragma unroll
    for (int j = 0; j < co_units(FNT); ++j) {
      const int e4 = tid + FNT * j;
      if (e4 < n4) {
        const float4 f = relu4(ln_param4(ly.ln1_b, e4, V, C));
        for (int s = 0; s < fifo; ++s)
          if (s != head) store4(ring + s * E + e4 * 4, f);
        for (int s = 0; s < R; ++s)
          if (s != rhead) store4(d.res_ring + s * E + e4 * 4, make_float4(0.f, 0.f, 0.f, 0.f));
      }
    }
    if (tid == 0) ly.idx[b * 2] = 0, ly.idx[b * 2 + 1] = 0;  // what cs_taps and cs_finish read; nobody else reads them here
  }
  co_push_stage<T, FNT>(d, ring, head, rhead, red);
}

// ---------------------------------------------------------------------------------------------------- taps
// The 8 waves of a block over the layer's column tiles: nsub = max(1, 8 / ntile) waves share a tile and interleave its
// k-steps (wave (tile, sub) takes ks0 + sub, ks0 + sub + nsub, ...); with more than 8 tiles a wave would loop, but
// Cout <= 256 gives at most 8.  A function of Cout alone.
DEV int taps_nsub(int ntile) { return ntile >= TNW ? 1 : TNW / ntile; }

template <typename T, int TU>
__global__ __launch_bounds__(TNT) void cs_taps_kernel(const layer_t ly, int V, int nks, int nsplit,
                                                      const int* __restrict__ order) {
  __shared__ float red[TNW][16][64];
  const int nact = order[0], g0 = blockIdx.y * G;
  if (g0 >= nact) return;  // uniform over the block
  const int ng = min(G, nact - g0);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, row = lane & 31, h = lane >> 5;
  const int C = ly.Cout, Kt = ly.Kt, S = ly.S, fifo = ring_slots(S, Kt), Ktot = Kt * C;
  const int ntile = (C + 31) / 32, nsub = taps_nsub(ntile);
  const int tile = w / nsub, sub = w - tile * nsub;
  const bool work = tile < ntile;  // uniform over the wave
  const int s = blockIdx.x;
  const int ks0 = (int)((long)s * nks / nsplit), ks1 = (int)((long)(s + 1) * nks / nsplit);
  const long E = (long)V * C;
  int sb[G], head[G];
  const T* ring[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    sb[g] = g < ng ? order[1 + g0 + g] : 0;
    head[g] = g < ng ? ring_head(ly.idx[sb[g] * 2], fifo) : 0;
    ring[g] = reinterpret_cast<const T*>(ly.ring) + (long)sb[g] * fifo * E;
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
        for (int g = 0; g < G; ++g)
          af[u][g] = load_ring<T>(ring[g], g < ng && row < V, row, V, C, S, fifo, head[g], tap, ci, in);
      }
#pragma unroll
      for (int u = 0; u < TU; ++u)
#pragma unroll
        for (int g = 0; g < G; ++g)
          if (g < ng) Tr<T>::mma(acc[g], af[u][g], bf[u]);
    }
  }
  // per stream: the nsub interleaves of every tile summed in index order -> partial[b][s][v][co]
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (g < ng) {  // uniform over the block
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 16; ++r) red[w][r][lane] = acc[g][r];
      __syncthreads();
      float* out = ly.partial + ((long)sb[g] * nsplit + s) * E;
      for (int o = tid; o < ntile * 16 * 64; o += TNT) {
        const int t = o >> 10, r = (o >> 6) & 15, l = o & 63;
        float sum = 0.f;
        for (int i = 0; i < nsub; ++i) sum += red[t * nsub + i][r][l];
        const int v = acc_row(r, l), co = t * 32 + (l & 31);
        if (v < V && co < C) out[(long)v * C + co] = sum;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------- finish
__global__ __launch_bounds__(FNT) void cs_finish_kernel(const layer_t ly, int V, int nsplit,
                                                        const int* __restrict__ active) {
  __shared__ float red[FNT / 64];
  const long b = blockIdx.x;
  if (active[b] == 0) return;
  co_finish_stage<FNT>(co_view(ly, V, nullptr, b), ly.partial + b * nsplit * V * ly.Cout, nsplit, red);
}

// the single-stream descriptor that carries the same shape: co_check's limits are this route's limits
stgcn_co_layer as_co_layer(const stgcn_co_streams_desc& d, const layer_t& y) {
  stgcn_co_layer c = {};
  c.V = d.V, c.Cin = y.Cin, c.Cout = y.Cout, c.P = y.P, c.Kt = y.Kt, c.S = y.S;
  c.res_mode = y.res_mode, c.dtype = d.dtype, c.splits = y.splits;
  return c;
}

template <typename T>
void launch_taps(const layer_t& y, int V, int nks, int nsplit, const int* order, int B, hipStream_t s) {
  const dim3 grid((unsigned)nsplit, (unsigned)((B + G - 1) / G));
  constexpr int TU = sizeof(T) == 2 ? 4 : 2;
  hipLaunchKernelGGL((cs_taps_kernel<T, TU>), grid, dim3(TNT), 0, s, y, V, nks, nsplit, order);
}

}  // namespace

// 0 when the descriptor's shapes, dtype and (unless shapes_only) pointers are usable
int co_streams_check(const stgcn_co_streams_desc& d, bool shapes_only) {
  if (d.B < 1 || d.L < 1 || d.L > STGCN_RT_MAX_LAYERS || d.K < 1 || d.C0 < 4 || d.C0 > CMAX || d.C0 % 4 ||
      !head_feats_ok(d.F, d.V))
    return STGCN_EBADSHAPE;
  int cin = d.C0;
  for (int l = 0; l < d.L; ++l) {
    const layer_t& y = d.layers[l];
    if (y.Cin != cin) return STGCN_EBADSHAPE;
    const int rc = co_check(as_co_layer(d, y), true);  // shapes first, then the dtype
    if (rc != STGCN_OK) return rc;
    cin = y.Cout;
  }
  if (shapes_only) return STGCN_OK;
  if (!d.x || !d.active || !d.ln_w || !d.ln_b || !d.w_in || !d.b_in || !d.w_out || !d.h0 || !d.order || !d.out)
    return STGCN_EBADSHAPE;
  for (int l = 0; l < d.L; ++l) {
    const layer_t& y = d.layers[l];
    if (!y.A || !y.wp || !y.ln1_w || !y.ln1_b || !y.ln2_w || !y.ln2_b || !y.wt || !y.ring || !y.res_ring || !y.idx ||
        !y.z_buf || !y.partial || !y.y || (y.res_mode == 2 && (!y.wrp || !y.lnr_w || !y.lnr_b || !y.r_buf)))
      return STGCN_EBADSHAPE;
  }
  return STGCN_OK;
}

// K splits of layer l's tap stage.  The default aims at 16 k-steps per wave and caps at 8 (every split writes and
// re-reads one [V][C] fp32 partial per stream; 8 of them are 23 % of the bf16 ring bytes at Kt = 69): a function of
// (Cout, Kt) alone, never of B or of the device, so that a stream's sums have one order everywhere.
int co_streams_num_splits(const stgcn_co_streams_desc& d, int l) {
  const layer_t& y = d.layers[l];
  const int nks = num_ksteps(y.Cout, y.Kt), ntile = (y.Cout + 31) / 32;
  const int nsub = ntile >= TNW ? 1 : TNW / ntile;
  int n = y.splits;
  if (n <= 0) {
    n = nks / (16 * nsub);
    if (n > MAX_SPLITS) n = MAX_SPLITS;
  }
  if (n > nks) n = nks;
  return n < 1 ? 1 : n;
}

int co_streams_launch(const stgcn_co_streams_desc& d, hipStream_t s) {
  const int B = d.B, V = d.V;
  hipLaunchKernelGGL(cs_order_kernel, dim3(1), dim3(HNT), 0, s, d.active, B, d.order);
  hipLaunchKernelGGL(cs_in_kernel, dim3((unsigned)B), dim3(HNT), 0, s, d.x, d.active, head_feats(d.F), V, d.C0, d.ln_w, d.ln_b, d.w_in,
                     d.b_in, d.h0);
  const float* x = d.h0;
  for (int l = 0; l < d.L; ++l) {
    const layer_t& y = d.layers[l];
    const int nks = num_ksteps(y.Cout, y.Kt), nsplit = co_streams_num_splits(d, l);
    hipLaunchKernelGGL(cs_gcn_kernel, dim3((unsigned)B), dim3(GNT), 0, s, y, V, x, d.active);
    if (d.dtype == 0) {
      hipLaunchKernelGGL(cs_push_kernel<float>, dim3((unsigned)B), dim3(FNT), 0, s, y, V, x, d.active);
      launch_taps<float>(y, V, nks, nsplit, d.order, B, s);
    } else {
      hipLaunchKernelGGL(cs_push_kernel<bf16>, dim3((unsigned)B), dim3(FNT), 0, s, y, V, x, d.active);
      launch_taps<bf16>(y, V, nks, nsplit, d.order, B, s);
    }
    hipLaunchKernelGGL(cs_finish_kernel, dim3((unsigned)B), dim3(FNT), 0, s, y, V, nsplit, d.active);
    x = y.y;
  }
  const layer_t& last = d.layers[d.L - 1];
  hipLaunchKernelGGL(cs_out_kernel, dim3((unsigned)B), dim3(HNT), 0, s, x, d.active, V, last.Cout, d.w_out, d.b_out, d.K,
                     d.out);
  return hipGetLastError() == hipSuccess ? STGCN_OK : STGCN_EHIP;
}
