// CoST-GCN clip inference (stgcn_co_clip): T consecutive frames of ONE stream per call, on the stream's own rings.
// Column t of the output is what the per-frame route would give for frame t from the stream's current state, and the
// rings and indices end where T per-frame calls would have left them.  Frame t of the clip takes the place of stream b
// of co_streams.hip, so the heads, the graph conv, the push arithmetic and the LayerNorm statistics are frame_ops.h's;
// the temporal conv of a layer becomes ONE causal dilated GEMM with T*V rows that reads the tap weights once per clip.
//
// A layer works on linear clip buffers, time ascending, the carried history in front of the new frames:
//   hist [fifo-1 + T][V][C]  compute dtype: ReLU(LN1(z)) of the fifo-1 frames the ring carried in, then of frame 0..T-1
//   resq [Kt/2   + T][V][C]  fp32: the residual rows of the Kt/2 frames the residual ring carried in, then the new ones
// so frame t's tap k is hist row block fifo-1 + t - k*S and its residual is resq row block t: no ring arithmetic in
// the hot kernel.  Launches per clip, every hand-off a kernel boundary, no workgroup waits on another:
//
//   cc_in     : h0[t] = fcn_in(LayerNorm([3,1,V])(x[:, t])): frame_head_in                         (1 block per frame)
//   per layer:
//   cc_gcn    : z[t] = gcn(x[t], A), r[t] = Wr x[t] + br: cs_gcn_kernel's body (conv_tile_acc + amix)   (1 per frame)
//   cc_push   : blocks 0..T-1: co_push_stage of frame t into hist[fifo-1+t] and resq[Kt/2+t];
//               further blocks: one carried ring slot each copied into the front of hist / resq.  The ONLY launch of
//               the layer that reads the rings, and it writes none of them.
//   cc_taps   : partial[t][s][v][co] = sum over K split s of Wp . hist.  Rows are m = t*V + v, dense over the clip
//               (no padding of a frame to 32 rows); a block takes G = 4 consecutive 32-row tiles (about 5 frames at
//               V = 25) and one K split; its 8 waves share out the column tiles (taps_nsub), so a weight B fragment is
//               loaded once for the G row tiles and the tiles' overlapping history rows are re-read on one CU.
//   cc_finish : per frame u = bt + sum_s partial[t][s] (index order), y[t] = relu(LN2(u) + resq[t]); one thread of the
//               launch advances idx by T (nobody else reads idx in this launch).
//   cc_state  : the last min(T, fifo) hist frames and min(T, Kt/2+1) resq rows into the ring slots the per-frame route
//               would have used (new frame t: slot (idx0 - 1 - t) mod fifo, derived from the advanced idx).  The ONLY
//               launch that writes the rings.
//   cc_out    : out[t] = fcn_out(mean_v y_last[t]): frame_head_out                                      (1 per frame)
//
// The hazard of a clip (new frame t = fifo-1-j takes the slot of the carried frame of age j, which earlier clip frames
// still need) is designed out: cc_push copies the carried frames out before anything writes a ring, cc_state writes the
// rings after cc_taps and cc_finish have run, and two kernel boundaries lie between the two.
//
// Order of every sum, none of which depends on T, on the frame's position in the clip or on the device: k-steps in
// sequence within a wave (an MFMA row's result does not depend on which of the 32 rows it is), the nsub K-interleaves
// of a column tile in index order, the splits in index order (cc_splits: a function of (Cout, Kt) alone), LayerNorm
// statistics through ln_stats_units<1024>.  No atomics.  So any split of a clip into consecutive clips gives the same
// bits, outputs and state.
#include "common.h"
#include "launchers.h"
#include "frame_ops.h"
#include "../../include/stgcn_amd.h"

namespace {

constexpr int HNT = 256;   // cc_in / cc_out block
constexpr int GNT = 512;   // cc_gcn block
constexpr int GNW = GNT / 64;
constexpr int FNT = 1024;  // cc_push / cc_finish / cc_state block: V * C <= 8192 in 2 float4 units per thread
constexpr int TNT = 512;   // cc_taps block
constexpr int TNW = TNT / 64;
constexpr int G = 4;       // 32-row tiles per tap block: 4 x 16 accumulator registers per wave
constexpr int GTU = 4;     // k-steps in flight per wave in cc_gcn
constexpr int MAX_SPLITS = 8;

using layer_t = stgcn_co_clip_layer;

// ---------------------------------------------------------------------------------------------------- heads
// x is the (3, T, V) clip as given: channel c of frame t at x[c * x_stride + t * V]
__global__ __launch_bounds__(HNT) void cc_in_kernel(const float* __restrict__ x, long x_stride, int V, int C0,
                                                    const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                    const float* __restrict__ w_in, const float* __restrict__ b_in,
                                                    float* __restrict__ h0) {
  __shared__ float xf[3 * VMAX];
  __shared__ float xi[3 * VMAX];
  __shared__ float red[HNT / 64];
  const long t = blockIdx.x;
  for (int i = threadIdx.x; i < 3 * V; i += HNT) {
    const int c = i / V, v = i - c * V;
    xf[i] = x[c * x_stride + t * V + v];
  }
  __syncthreads();
  frame_head_in<HNT>(xf, V, C0, ln_w, ln_b, w_in, b_in, xi, red, h0 + t * V * C0, C0);
}

__global__ __launch_bounds__(HNT) void cc_out_kernel(const float* __restrict__ y, int V, int C,
                                                     const float* __restrict__ w_out, const float* __restrict__ b_out,
                                                     int K, float* __restrict__ out) {
  __shared__ float pool[CMAX];
  const long t = blockIdx.x;
  frame_head_out<HNT>(y + t * V * C, C, V, C, w_out, b_out, K, pool, out + t * K);
}

// ---------------------------------------------------------------------------------------------------- gcn
// cs_gcn_kernel with frame t in the place of stream b
__global__ __launch_bounds__(GNT) void cc_gcn_kernel(const layer_t ly, int V, const float* __restrict__ x) {
  __shared__ __attribute__((aligned(16))) float xs[VMAX * (CMAX + XPAD)];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, row = lane & 31, h = lane >> 5;
  const long t = blockIdx.x;
  const int Cin = ly.Cin, Cout = ly.Cout, P = ly.P, ldx = Cin + XPAD, K4 = Cin / 4;
  const float4* xb = reinterpret_cast<const float4*>(x + t * V * Cin);
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
      float* dst = (res ? ly.r_buf : ly.z_buf) + t * V * Cout;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int v = acc_row(r, lane);
        if (v < V) dst[v * Cout + co] = z[r] + (res ? add : (ly.bias2d ? ly.bias2d[v * Cout + co] : 0.f));
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------- push + carry
// blocks [0, T): frame t's push; [T, T + fifo-1): carried activation frame of hist position p; then Kt/2 blocks: the
// carried residual row of resq position q.  Position p holds the frame of age fifo-2-p (age 0 = the newest carried
// frame, ring slot idx[0]); position q the residual of age Kt/2-1-q (slot idx[1]).
template <typename T>
__global__ __launch_bounds__(FNT) void cc_push_kernel(const layer_t ly, int V, int Tn, const float* __restrict__ x) {
  __shared__ float red[FNT / 64];
  const int tid = threadIdx.x, C = ly.Cout, n4 = V * C / 4;
  const long E = (long)V * C;
  const int fifo = ring_slots(ly.S, ly.Kt), R = res_slots(ly.Kt), Hh = fifo - 1, Hr = R - 1;
  T* hist = reinterpret_cast<T*>(ly.hist);
  const int b = blockIdx.x;
  if (b < Tn) {
    CoView d;
    d.V = V, d.C = C, d.Kt = ly.Kt, d.S = ly.S, d.res_mode = ly.res_mode;
    d.z = ly.z_buf + b * E;
    d.res = ly.res_mode == 2 ? ly.r_buf + b * E : x + b * E;  // mode 1: Cin == Cout
    d.res_ring = ly.resq;
    d.idx = nullptr;
    d.ln1_w = ly.ln1_w, d.ln1_b = ly.ln1_b, d.ln2_w = ly.ln2_w, d.ln2_b = ly.ln2_b;
    d.lnr_w = ly.lnr_w, d.lnr_b = ly.lnr_b;
    d.bt = ly.bt;
    d.y = nullptr;
    co_push_stage<T, FNT>(d, hist, Hh + b, Hr + b, red);
    return;
  }
  const int p = b - Tn;
  if (p < Hh) {
    const int slot = (ly.idx[0] + (Hh - 1 - p)) % fifo;
    const T* src = reinterpret_cast<const T*>(ly.ring) + slot * E;
    T* dst = hist + p * E;
    for (int e4 = tid; e4 < n4; e4 += FNT) {
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
  } else if (ly.res_mode) {
    const int q = p - Hh;
    const int slot = (ly.idx[1] + (Hr - 1 - q)) % R;
    const float4* src = reinterpret_cast<const float4*>(ly.res_ring + slot * E);
    float4* dst = reinterpret_cast<float4*>(ly.resq + q * E);
    for (int e4 = tid; e4 < n4; e4 += FNT) dst[e4] = src[e4];
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

template <typename T, int TU>
__global__ __launch_bounds__(TNT) void cc_taps_kernel(const layer_t ly, int V, int M, int nks, int nsplit) {
  __shared__ float red[TNW][16][64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, row = lane & 31, h = lane >> 5;
  const int C = ly.Cout, Kt = ly.Kt, S = ly.S, Hh = ring_slots(S, Kt) - 1, Ktot = Kt * C;
  const int ntile = (C + 31) / 32, nsub = taps_nsub(ntile);
  const int tile = w / nsub, sub = w - tile * nsub;
  const bool work = tile < ntile;  // uniform over the wave
  const int s = blockIdx.x, m0 = blockIdx.y * (G * 32);
  const int ng = min(G, (M - m0 + 31) / 32);  // row tiles of this block that hold rows: uniform over the block
  const int ks0 = (int)((long)s * nks / nsplit), ks1 = (int)((long)(s + 1) * nks / nsplit);
  const T* hist = reinterpret_cast<const T*>(ly.hist);
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
          ly.partial[((long)t * nsplit + s) * E + (long)v * C + co] = sum;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------- finish
// co_finish_stage's arithmetic for frame t, the residual taken from resq[t] (the row of frame t - Kt/2) and no ring
// head to store.  Block 0's thread 0 advances both indices by T: no other thread of this launch reads them.
__global__ __launch_bounds__(FNT) void cc_finish_kernel(const layer_t ly, int V, int Tn, int nsplit) {
  __shared__ float red[FNT / 64];
  constexpr int U = co_units(FNT);
  const int tid = threadIdx.x, C = ly.Cout, n4 = V * C / 4;
  const long E = (long)V * C, t = blockIdx.x;
  const float* partial = ly.partial + t * nsplit * E;
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
  const float4* rrow = reinterpret_cast<const float4*>(ly.resq + t * E);
  float4* y = reinterpret_cast<float4*>(ly.y + t * E);
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const int e4 = tid + FNT * j;
    if (e4 < n4) {
      float4 o = ln_apply4(u[j], st, ly.ln2_w, ly.ln2_b, e4, V, C);
      if (ly.res_mode) o = add4(o, rrow[e4]);
      y[e4] = relu4(o);
    }
  }
  if (t == 0 && tid == 0) {
    const int fifo = ring_slots(ly.S, ly.Kt), R = res_slots(ly.Kt);
    ly.idx[0] = ((ly.idx[0] - Tn) % fifo + fifo) % fifo;
    ly.idx[1] = ((ly.idx[1] - Tn) % R + R) % R;
  }
}

// ---------------------------------------------------------------------------------------------------- state
// blocks [0, na): the j-th newest activation frame (t = T-1-j) -> ring slot (idx[0] + j) % fifo, idx already advanced;
// blocks [na, na + nr): the j-th newest residual row -> res_ring slot (idx[1] + j) % R
template <typename T>
__global__ __launch_bounds__(FNT) void cc_state_kernel(const layer_t ly, int V, int Tn, int na) {
  const int tid = threadIdx.x, C = ly.Cout, n4 = V * C / 4;
  const long E = (long)V * C;
  const int fifo = ring_slots(ly.S, ly.Kt), R = res_slots(ly.Kt);
  int j = blockIdx.x;
  if (j < na) {
    const T* src = reinterpret_cast<const T*>(ly.hist) + (long)(fifo - 1 + Tn - 1 - j) * E;
    T* dst = reinterpret_cast<T*>(ly.ring) + (long)((ly.idx[0] + j) % fifo) * E;
    for (int e4 = tid; e4 < n4; e4 += FNT) {
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
  } else {
    j -= na;
    const float4* src = reinterpret_cast<const float4*>(ly.resq + (long)(R - 1 + Tn - 1 - j) * E);
    float4* dst = reinterpret_cast<float4*>(ly.res_ring + (long)((ly.idx[1] + j) % R) * E);
    for (int e4 = tid; e4 < n4; e4 += FNT) dst[e4] = src[e4];
  }
}

// the single-frame descriptor that carries the same shape: co_check's limits are this route's limits
stgcn_co_layer as_co_layer(const stgcn_co_clip_desc& d, const layer_t& y) {
  stgcn_co_layer c = {};
  c.V = d.V, c.Cin = y.Cin, c.Cout = y.Cout, c.P = y.P, c.Kt = y.Kt, c.S = y.S;
  c.res_mode = y.res_mode, c.dtype = d.dtype, c.splits = y.splits;
  return c;
}

template <typename T>
void launch_layer(const layer_t& y, int V, int Tn, int nsplit, const float* x, hipStream_t s) {
  const int fifo = ring_slots(y.S, y.Kt), R = res_slots(y.Kt), nks = num_ksteps(y.Cout, y.Kt), M = Tn * V;
  hipLaunchKernelGGL(cc_gcn_kernel, dim3((unsigned)Tn), dim3(GNT), 0, s, y, V, x);
  hipLaunchKernelGGL(cc_push_kernel<T>, dim3((unsigned)(Tn + fifo - 1 + R - 1)), dim3(FNT), 0, s, y, V, Tn, x);
  const dim3 grid((unsigned)nsplit, (unsigned)((M + G * 32 - 1) / (G * 32)));
  constexpr int TU = sizeof(T) == 2 ? 4 : 2;
  hipLaunchKernelGGL((cc_taps_kernel<T, TU>), grid, dim3(TNT), 0, s, y, V, M, nks, nsplit);
  hipLaunchKernelGGL(cc_finish_kernel, dim3((unsigned)Tn), dim3(FNT), 0, s, y, V, Tn, nsplit);
  const int na = Tn < fifo ? Tn : fifo, nr = y.res_mode ? (Tn < R ? Tn : R) : 0;
  hipLaunchKernelGGL(cc_state_kernel<T>, dim3((unsigned)(na + nr)), dim3(FNT), 0, s, y, V, Tn, na);
}

}  // namespace

// 0 when the descriptor's shapes, dtype and (unless shapes_only) pointers are usable
int co_clip_check(const stgcn_co_clip_desc& d, bool shapes_only) {
  if (d.T < 1 || d.T > STGCN_CO_CLIP_MAX_T || d.L < 1 || d.L > STGCN_RT_MAX_LAYERS || d.K < 1 || d.C0 < 4 ||
      d.C0 > CMAX || d.C0 % 4)
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
  if (!d.x || d.x_stride < (long)d.T * d.V || !d.ln_w || !d.ln_b || !d.w_in || !d.b_in || !d.w_out || !d.h0 || !d.out)
    return STGCN_EBADSHAPE;
  for (int l = 0; l < d.L; ++l) {
    const layer_t& y = d.layers[l];
    if (!y.A || !y.wp || !y.ln1_w || !y.ln1_b || !y.ln2_w || !y.ln2_b || !y.wt || !y.ring || !y.res_ring || !y.idx ||
        !y.z_buf || !y.hist || !y.resq || !y.partial || !y.y ||
        (y.res_mode == 2 && (!y.wrp || !y.lnr_w || !y.lnr_b || !y.r_buf)))
      return STGCN_EBADSHAPE;
  }
  return STGCN_OK;
}

// K splits of layer l's tap stage: co_streams_num_splits' rule (16 k-steps per wave, at most 8), a function of
// (Cout, Kt) alone and never of T or the device, so that a frame's sums have one order in every clip
int co_clip_num_splits(const stgcn_co_clip_desc& d, int l) {
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

int co_clip_launch(const stgcn_co_clip_desc& d, hipStream_t s) {
  const int T = d.T, V = d.V;
  hipLaunchKernelGGL(cc_in_kernel, dim3((unsigned)T), dim3(HNT), 0, s, d.x, d.x_stride, V, d.C0, d.ln_w, d.ln_b, d.w_in,
                     d.b_in, d.h0);
  const float* x = d.h0;
  for (int l = 0; l < d.L; ++l) {
    const layer_t& y = d.layers[l];
    const int nsplit = co_clip_num_splits(d, l);
    if (d.dtype == 0) launch_layer<float>(y, V, T, nsplit, x, s);
    else launch_layer<bf16>(y, V, T, nsplit, x, s);
    x = y.y;
  }
  const layer_t& last = d.layers[d.L - 1];
  hipLaunchKernelGGL(cc_out_kernel, dim3((unsigned)T), dim3(HNT), 0, s, x, V, last.Cout, d.w_out, d.b_out, d.K, d.out);
  return hipGetLastError() == hipSuccess ? STGCN_OK : STGCN_EHIP;
}
