// CoST-GCN per-frame inference (models/costgcn/costgcn.py StgcnLayer.forward, :192-211), batch 1, one frame per
// call.  A layer keeps the last fifo = S*(Kt-1)+1 graph-conv frames and runs the full learned Kt-tap temporal
// convolution (dilation S) over them every frame: a V-row GEMM with K = Kt*C whose cost is reading the weights.
// Four launches per layer, every hand-off a kernel boundary (no workgroup waits on another):
//
//   co_gcn    : z = gcn(x, A) (conv1x1 + bias, A-mix summed over partitions; rt_gcn_kernel's first half) and the
//               residual 1x1 conv WITH its bias (costgcn.py:178-181) -> z_buf, r_buf             (Cout / 2 blocks)
//   co_push   : ring[head] = ReLU(LN1(z)) in the compute dtype; res_ring[rhead] = x | LN_r(r)        (1 block)
//               LN1 is per frame, so the ring caches its result instead of re-normalising the FIFO each frame;
//               an empty FIFO (zeros) normalises to ReLU(LN1.bias): the host initialises every slot to that.
//   co_taps   : partial[s][v][co] = sum_{kk in split s} Wp[co][kk] * ring[(head + tap*S) % fifo][v][ci],
//               kk = tap*C + ci (tap 0 meets the newest frame).  Grid (Cout/32 column tiles) x (K splits); the
//               frame's V <= 32 rows are the 32-row MFMA operand, 32x32x16 bf16 or 8 x 32x32x2 fp32 per 16 kk.
//               Weights are packed once [tile][k-step][lane][8] (co_pack_kernel): lane l's B fragment of a k-step
//               is 8 contiguous elements, a workgroup's k-step range one contiguous panel read exactly once.
//   co_finish : co_finish_stage: u = bias + sum_s partial[s] (fixed order), y = relu(LN2(u) + res_ring[(rhead +
//               Kt/2) % R]); advances both ring heads.                                               (1 block)
// co_finish_stage and the shape limits are frame_ops.h's, shared with co_streams.hip (one stream here is its stream 0
// of 1).  co_gcn, co_push and the ring fragment load of co_taps keep their own bodies: shared with rt_gcn_kernel /
// cs_push / cs_taps they measured slower or took more registers here.
// head' = (head + fifo - 1) % fifo is the slot of the newest frame: co_push / co_taps / co_finish all derive it
// from the stored head, co_finish stores it.  Entry of age j lives in slot (head' + j) % fifo.
// No floating-point atomics anywhere: a stream replays bit-identically.
#include "common.h"
#include "launchers.h"
#include "frame_ops.h"
#include "../../include/stgcn_amd.h"

namespace {

constexpr int NT = 256;
constexpr int FNT = 1024;  // co_push / co_finish block: V * C <= 8192 in 2 float4 units per thread

// y_p[u][co] = W_p[co] . x[u] for the block's GCN_CB channels, then z[v][co] = bias2d[v][co] + sum_{p,u} A[p][u][v] y_p[u][co];
// r[v][co] = br[co] + Wr[co] . x[v]
__global__ __launch_bounds__(NT) void co_gcn_kernel(const float* __restrict__ x, int V, int Cin, int Cout, int P,
                                                    const float* __restrict__ A, const float* __restrict__ W,
                                                    const float* __restrict__ bias2d, const float* __restrict__ Wr,
                                                    const float* __restrict__ br, float* __restrict__ z_out,
                                                    float* __restrict__ r_out) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* xs = sm;               // [V][Cin]
  float* ys = xs + V * Cin;     // [P][V][GCN_CB]
  float* As = ys + P * V * GCN_CB;  // [P][V][V]
  const int tid = threadIdx.x, kk = tid & 7, K4 = Cin / 4;
  for (int i = tid; i < V * Cin / 4; i += NT) reinterpret_cast<float4*>(xs)[i] = reinterpret_cast<const float4*>(x)[i];
  for (int i = tid; i < P * V * V; i += NT) As[i] = A[i];
  __syncthreads();
  const int co0 = blockIdx.x * GCN_CB;
  for (int t0 = 0; t0 < P * V * GCN_CB; t0 += NT / 8) {
    const int t = t0 + (tid >> 3);
    const int cl = t % GCN_CB, pu = t / GCN_CB, u = pu % V, p = pu / V;
    const bool ok = t < P * V * GCN_CB && co0 + cl < Cout;
    const int co = ok ? co0 + cl : co0;
    const float y = dot8(W + ((long)(ok ? p : 0) * Cout + co) * Cin, xs + (ok ? u : 0) * Cin, K4, kk);
    if (ok && kk == 0) ys[t] = y;  // t = (p * V + u) * GCN_CB + cl
  }
  __syncthreads();
  for (int t0 = 0; t0 < V * GCN_CB; t0 += NT / 8) {
    const int tr = t0 + (tid >> 3);
    const int cl = tr % GCN_CB, v = tr / GCN_CB, co = co0 + cl;
    const bool ok = v < V && co < Cout;
    float r = 0.f;
    if (Wr) r = dot8(Wr + (long)(ok ? co : co0) * Cin, xs + (ok ? v : 0) * Cin, K4, kk);
    if (ok && kk == 0) {
      float s = bias2d ? bias2d[v * Cout + co] : 0.f;
      for (int p = 0; p < P; ++p)
        for (int u = 0; u < V; ++u) s = fmaf(As[(p * V + u) * V + v], ys[(p * V + u) * GCN_CB + cl], s);
      const long e = (long)v * Cout + co;
      z_out[e] = s;
      if (Wr) r_out[e] = r + (br ? br[co] : 0.f);
    }
  }
}

// the body co_push_stage restates for co_streams.hip: kept apart, the shared stage measured 0.3 us slower here
template <typename T>
__global__ __launch_bounds__(FNT) void co_push_kernel(const stgcn_co_layer d) {
  __shared__ float red[FNT / 64];
  const int tid = threadIdx.x, V = d.V, C = d.Cout, n4 = V * C / 4;
  const int head = ring_head(d.idx[0], ring_slots(d.S, d.Kt)), rhead = ring_head(d.idx[1], res_slots(d.Kt));
  float4 z[co_units(FNT)], r[co_units(FNT)];
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int j = 0; j < co_units(FNT); ++j) {
    const int e4 = tid + FNT * j;
    z[j] = e4 < n4 ? reinterpret_cast<const float4*>(d.z_buf)[e4] : zero;
    r[j] = zero;
    if (e4 < n4 && d.res_mode == 1) r[j] = reinterpret_cast<const float4*>(d.x)[e4];
    if (e4 < n4 && d.res_mode == 2) r[j] = reinterpret_cast<const float4*>(d.r_buf)[e4];
  }
  const float2 st = ln_stats_units<FNT>(z, n4, red);
  float2 sr = make_float2(0.f, 1.f);
  if (d.res_mode == 2) sr = ln_stats_units<FNT>(r, n4, red);
  T* slot = reinterpret_cast<T*>(d.ring) + (long)head * V * C;
  float* rslot = d.res_ring + (long)rhead * V * C;
#pragma unroll
  for (int j = 0; j < co_units(FNT); ++j) {
    const int e4 = tid + FNT * j;
    if (e4 < n4) {
      float4 o = ln_apply4(z[j], st, d.ln1_w, d.ln1_b, e4, V, C);
      o = make_float4(fmaxf(o.x, 0.f), fmaxf(o.y, 0.f), fmaxf(o.z, 0.f), fmaxf(o.w, 0.f));
      store4(slot + e4 * 4, o);
      if (d.res_mode == 1) store4(rslot + e4 * 4, r[j]);
      if (d.res_mode == 2) store4(rslot + e4 * 4, ln_apply4(r[j], sr, d.lnr_w, d.lnr_b, e4, V, C));
    }
  }
}

// ------------------------------------------------------------------------------------------- the tap GEMM
// A fragment of k-step ks: lane (row = l & 31, h = l >> 5) holds kk = 16 ks + 8 h + j, j < 8, of frame row `row`,
// kk = tap * C + ci read from ring slot (head + tap * S) % fifo.  Two 4-element units (C % 4 == 0: one slot each).
template <typename T>
DEV typename Tr<T>::frag load_a(const T* __restrict__ ring, int ks, int ks1, int row, int h, int V, int C, int Ktot,
                                int S, int fifo, int head) {
  T f[8];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int kk = ks * 16 + 8 * h + 4 * u;
    if (ks < ks1 && row < V && kk < Ktot) {
      const int tap = kk / C, ci = kk - tap * C;
      const int slot = (head + tap * S) % fifo;
      load4(ring + ((long)slot * V + row) * C + ci, f + 4 * u);
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

constexpr int TW = NT / 64;  // waves per co_taps block; wave w takes k-steps ks0 + w, ks0 + w + TW, ...
constexpr int TU = 4;        // k-steps in flight per wave

template <typename T>
__global__ __launch_bounds__(NT) void co_taps_kernel(const T* __restrict__ wt, const T* __restrict__ ring,
                                                     const int* __restrict__ idx, int V, int C, int Cout, int Kt, int S,
                                                     int nks, int nsplit, float* __restrict__ partial) {
  __shared__ float red[TW][16][64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, row = lane & 31, h = lane >> 5;
  const int tile = blockIdx.x, s = blockIdx.y;
  const int fifo = ring_slots(S, Kt), head = ring_head(idx[0], fifo), Ktot = Kt * C;
  const int ks0 = (int)((long)s * nks / nsplit), ks1 = (int)((long)(s + 1) * nks / nsplit);
  const T* panel = wt + (long)tile * nks * 512;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int kb = ks0 + w; kb < ks1; kb += TW * TU) {
    typename Tr<T>::frag a[TU], b[TU];
#pragma unroll
    for (int u = 0; u < TU; ++u) b[u] = load_b<T>(panel, kb + u * TW, ks1, lane);
#pragma unroll
    for (int u = 0; u < TU; ++u) a[u] = load_a<T>(ring, kb + u * TW, ks1, row, h, V, C, Ktot, S, fifo, head);
#pragma unroll
    for (int u = 0; u < TU; ++u) Tr<T>::mma(acc, a[u], b[u]);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) red[w][r][lane] = acc[r];
  __syncthreads();
  float* out = partial + (long)s * V * Cout;
  for (int o = tid; o < 16 * 64; o += NT) {
    const int r = o >> 6, l = o & 63;
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < TW; ++i) t += red[i][r][l];
    const int v = acc_row(r, l), co = tile * 32 + (l & 31);
    if (v < V && co < Cout) out[(long)v * Cout + co] = t;
  }
}

// element (tile, ks, l, j) of the pack: co = 32 tile + (l & 31), kk = 16 ks + 8 (l >> 5) + j = tap * C + ci;
// w is the Conv2d weight [Cout][C][Kt] (the trailing 1 dropped); zero beyond Cout and Kt * C
template <typename T>
__global__ __launch_bounds__(NT) void co_pack_kernel(const float* __restrict__ w, int Cout, int C, int Kt, int nks,
                                                     long total, T* __restrict__ dst) {
  const long i = (long)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i & 7), l = (int)((i >> 3) & 63);
  const long tk = i >> 9;
  const int ks = (int)(tk % nks), tile = (int)(tk / nks);
  const int co = tile * 32 + (l & 31), kk = ks * 16 + 8 * (l >> 5) + j;
  float v = 0.f;
  if (co < Cout && kk < Kt * C) {
    const int tap = kk / C, ci = kk - tap * C;
    v = w[((long)co * C + ci) * Kt + tap];
  }
  dst[i] = (T)v;
}

__global__ __launch_bounds__(FNT) void co_finish_kernel(const stgcn_co_layer d, int nsplit) {
  __shared__ float red[FNT / 64];
  co_finish_stage<FNT>(co_view(d, d.V, d.x, 0), d.partial, nsplit, red);
}

bool shape_ok(int V, int Cin, int Cout, int P, int Kt, int S) {
  return V >= 2 && V <= VMAX && Cin >= 4 && Cin <= CMAX && Cin % 4 == 0 && Cout >= 4 && Cout <= CMAX &&
         Cout % 4 == 0 && P >= 1 && P <= PMAX && Kt >= 1 && Kt <= KTMAX && (Kt & 1) && (S == 1 || S == 2);
}

}  // namespace

// 0 when the descriptor's shapes, dtype and (unless shapes_only) pointers are usable
int co_check(const stgcn_co_layer& d, bool shapes_only) {
  if (!shape_ok(d.V, d.Cin, d.Cout, d.P, d.Kt, d.S) || d.res_mode < 0 || d.res_mode > 2 || d.splits < 0 ||
      (d.res_mode == 1 && d.Cin != d.Cout))
    return STGCN_EBADSHAPE;
  if (d.dtype != 0 && d.dtype != 1) return STGCN_EDTYPE;
  if (shapes_only) return STGCN_OK;
  if (!d.x || !d.A || !d.w || !d.ln1_w || !d.ln1_b || !d.ln2_w || !d.ln2_b || !d.wt || !d.ring || !d.res_ring ||
      !d.idx || !d.z_buf || !d.partial || !d.y || (d.res_mode == 2 && (!d.wr || !d.lnr_w || !d.lnr_b || !d.r_buf)))
    return STGCN_EBADSHAPE;
  return STGCN_OK;
}

// K splits: enough that (column tiles) x (splits) covers every CU, at least TW k-steps (one per wave) each
int co_num_splits(const stgcn_co_layer& d, hipStream_t s) {
  const int nks = num_ksteps(d.Cout, d.Kt), ntiles = (d.Cout + 31) / 32;
  int n = d.splits;
  if (n <= 0) {
    const int cus = stgcn_cu_count(s);
    n = ((cus > 0 ? cus : 256) + ntiles - 1) / ntiles;
    const int cap = (nks + TW - 1) / TW;
    if (n > cap) n = cap;
  }
  if (n > nks) n = nks;
  return n < 1 ? 1 : n;
}

long co_pack_elems(int Cout, int C, int Kt) {
  if (!shape_ok(2, C, Cout, 1, Kt, 1)) return -1;
  return (long)((Cout + 31) / 32) * num_ksteps(C, Kt) * 512;
}

int co_pack_launch(const float* w, int Cout, int C, int Kt, void* dst, int dtype, hipStream_t s) {
  if (!w || !dst || !shape_ok(2, C, Cout, 1, Kt, 1) || Cout != C) return STGCN_EBADSHAPE;
  if (dtype != 0 && dtype != 1) return STGCN_EDTYPE;
  const long total = co_pack_elems(Cout, C, Kt);
  const unsigned nb = (unsigned)((total + NT - 1) / NT);
  if (dtype == 0)
    hipLaunchKernelGGL(co_pack_kernel<float>, dim3(nb), dim3(NT), 0, s, w, Cout, C, Kt, num_ksteps(C, Kt), total,
                       (float*)dst);
  else
    hipLaunchKernelGGL(co_pack_kernel<bf16>, dim3(nb), dim3(NT), 0, s, w, Cout, C, Kt, num_ksteps(C, Kt), total,
                       (bf16*)dst);
  return hipGetLastError() == hipSuccess ? STGCN_OK : STGCN_EHIP;
}

// The same [tile][k-step][lane][8] image for `groups` consecutive row-major fp32 matrices [rows][C] (a 1x1 conv weight,
// one group per partition; Kt = 1, so kk = ci): each group is packed on its own, so no 32-row tile straddles two groups.
// dtype 0 fp32 | 1 bf16 (rounded to nearest even), the element count is the same.
long co_pack_rows_elems(int rows, int C) {
  if (rows < 1 || rows > CMAX || C < 4 || C > CMAX || C % 4) return -1;
  return (long)((rows + 31) / 32) * num_ksteps(C, 1) * 512;
}

int co_pack_rows_launch(const float* w, int groups, int rows, int C, void* dst, int dtype, hipStream_t s) {
  const long total = co_pack_rows_elems(rows, C);
  if (!w || !dst || total < 0 || groups < 1 || groups > PMAX) return STGCN_EBADSHAPE;
  if (dtype != 0 && dtype != 1) return STGCN_EDTYPE;
  const unsigned nb = (unsigned)((total + NT - 1) / NT);
  for (int g = 0; g < groups; ++g) {
    if (dtype == 0)
      hipLaunchKernelGGL(co_pack_kernel<float>, dim3(nb), dim3(NT), 0, s, w + (long)g * rows * C, rows, C, 1,
                         num_ksteps(C, 1), total, (float*)dst + g * total);
    else
      hipLaunchKernelGGL(co_pack_kernel<bf16>, dim3(nb), dim3(NT), 0, s, w + (long)g * rows * C, rows, C, 1,
                         num_ksteps(C, 1), total, (bf16*)dst + g * total);
  }
  return hipGetLastError() == hipSuccess ? STGCN_OK : STGCN_EHIP;
}

int co_gcn_launch(const stgcn_co_layer& d, hipStream_t s) {
  const size_t lds = ((size_t)d.V * d.Cin + (size_t)d.P * d.V * GCN_CB + (size_t)d.P * d.V * d.V) * sizeof(float);
  hipLaunchKernelGGL(co_gcn_kernel, dim3((unsigned)((d.Cout + GCN_CB - 1) / GCN_CB)), dim3(NT), lds, s, d.x, d.V, d.Cin,
                     d.Cout, d.P, d.A, d.w, d.bias2d, d.res_mode == 2 ? d.wr : nullptr, d.br, d.z_buf, d.r_buf);
  return hipGetLastError() == hipSuccess ? STGCN_OK : STGCN_EHIP;
}

int co_push_launch(const stgcn_co_layer& d, hipStream_t s) {
  if (d.dtype == 0) hipLaunchKernelGGL(co_push_kernel<float>, dim3(1), dim3(FNT), 0, s, d);
  else hipLaunchKernelGGL(co_push_kernel<bf16>, dim3(1), dim3(FNT), 0, s, d);
  return hipGetLastError() == hipSuccess ? STGCN_OK : STGCN_EHIP;
}

int co_taps_launch(const stgcn_co_layer& d, hipStream_t s) {
  const int nks = num_ksteps(d.Cout, d.Kt), ntiles = (d.Cout + 31) / 32, nsplit = co_num_splits(d, s);
  const dim3 grid((unsigned)ntiles, (unsigned)nsplit);
  if (d.dtype == 0)
    hipLaunchKernelGGL(co_taps_kernel<float>, grid, dim3(NT), 0, s, (const float*)d.wt, (const float*)d.ring, d.idx, d.V,
                       d.Cout, d.Cout, d.Kt, d.S, nks, nsplit, d.partial);
  else
    hipLaunchKernelGGL(co_taps_kernel<bf16>, grid, dim3(NT), 0, s, (const bf16*)d.wt, (const bf16*)d.ring, d.idx, d.V,
                       d.Cout, d.Cout, d.Kt, d.S, nks, nsplit, d.partial);
  return hipGetLastError() == hipSuccess ? STGCN_OK : STGCN_EHIP;
}

int co_finish_launch(const stgcn_co_layer& d, hipStream_t s) {
  hipLaunchKernelGGL(co_finish_kernel, dim3(1), dim3(FNT), 0, s, d, co_num_splits(d, s));
  return hipGetLastError() == hipSuccess ? STGCN_OK : STGCN_EHIP;
}
