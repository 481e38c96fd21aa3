// RT-ST-GCN clip inference for a batch of B independent streams (stgcn_rt_streams_clip): stream b advances by n_b
// frames per call on the stream-major state of rt_streams.hip.  A frame's arithmetic is rt_streams_kernel's, stage by
// stage (frame_ops.h's frame_head_in, conv_tile_acc + amix_coeffs / amix_mma, ln_stats_units, frame_head_out, the same
// 512-thread block and the same unit-to-thread map, so the same order of every sum); what changes is where the frame
// boundary lies.  The FIFO step is a recurrence over the frames of one stream and everything else is per frame, so a
// layer is cut at the recurrence:
//
//   rtc_frame<T>(l), one workgroup per (stream b, frame t < n_b), l = 0 .. L:
//     l = 0     : input head -> xs (LDS) and xb[b][t]
//     l >= 1    : layer l-1's second half: y = relu(relu(LN(a[b][t])) + res), res = xb[b][t] | LN_r(r[b][t]) | none
//                 -> xs and, in place, xb[b][t]; thread 0 of the stream's frame 0 advances layer l-1's idx[b] by n_b
//                 (from 0 on a restart): no workgroup of this launch reads it
//     l < L     : layer l's first half: conv (A operand = xs as T, B operand = the packed image) + A-mix per
//                 (partition, tile) -> zs (LDS); z[b][t] = bias2d + Z_0 + Z_1 + Z_2; the residual conv -> r[b][t]
//     l = L     : output head -> out[b][t]; zero rows for frames not processed
//   rtc_scan(l), one thread per float4 unit of (stream b, V * Cout), l = 0 .. L-1:
//     for t < n_b, in order: a = acc[ai] + z_t - fifo[fi]; acc[ai] = a; fifo[fi] = z_t; a[b][t] = a; fi, ai advance.
//     The thread owns its 4 elements' whole history in the launch.  The S accumulator slots are S independent
//     chains (slot (ai + t) % S takes frames t = s, s + S, ...), each run in frame order with its value in registers;
//     the subtracted value is the stream's old fifo slot for t < fifo_size and z_{t - fifo_size} of this clip after
//     that, both loads that do not wait for the chain.  Every read of an old fifo slot precedes, in this thread, the
//     stores of the min(n_b, fifo_size) newest z into the slots the per-frame ticks would have left them in.  On a
//     restart nothing of fifo, acc or idx is read and the slots the clip does not reach are cleared.
// 2 L + 1 launches whatever B and T are.  Every workgroup reads what earlier launches wrote and writes rows of its own:
// no grid barrier, no spin, no cooperative launch, no atomics.  active [B] and lengths [B] are read on the device by
// every workgroup (stream_frames), so a captured call replays with other codes and lengths.
#include "common.h"
#include "launchers.h"
#include "frame_ops.h"
#include "../../include/stgcn_amd.h"

#include <algorithm>

namespace {

using desc_t = stgcn_rt_streams_clip_desc;
using layer_t = stgcn_rt_streams_layer;

constexpr int NT = 512;  // rt_streams_kernel's block: the same unit-to-thread map, the same order of the LN sums
constexpr int NW = NT / 64;
constexpr int U4 = (MAXE / 4 + NT - 1) / NT;  // float4 units of a frame per thread
constexpr int TU = 4;                         // k-steps in flight per wave
constexpr int SNT = 256;                      // scan block
constexpr int SU = 4;                         // frames of a scan chain whose operands are loaded ahead

// n_b = clamp(lengths[b] - t0, 0, T), or -1 for a skipped stream (no frame index is below it); restart: code 2 on the
// first call of the caller's clip
DEV int stream_frames(const desc_t& d, long b, bool& restart) {
  const int code = d.active[b], len = d.lengths[b];
  restart = code == 2 && d.t0 == 0;
  if (code == 0) return -1;
  return len <= d.t0 ? 0 : min(len - d.t0, d.T);
}

DEV int wrap(int i, int n) {  // an index read from device memory, into [0, n)
  i %= n;
  return i < 0 ? i + n : i;
}

// dynamic LDS (floats): xs [xsf] | zs [PMAX][ef] | red [16], sized per layer on the host (frame_lds)
template <typename T>
__global__ __launch_bounds__(NT) void rtc_frame_kernel(const desc_t d, const int l, const int xsf, const int ef) {
  extern __shared__ __attribute__((aligned(16))) float rc_sm[];
  float* xs = rc_sm;          // [V][C + XPAD] layer l's input
  float* zs = xs + xsf;       // [P][V][Cout] A-mixed conv per partition; the heads' scratch
  float* red = zs + PMAX * ef;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, V = d.V;
  const long b = blockIdx.x / d.T;
  const int t = (int)(blockIdx.x - b * d.T);
  bool restart;
  const int n = stream_frames(d, b, restart);
  if (t >= n) {  // uniform over the workgroup
    if (l == d.L) {
      float* o = d.out + b * d.out_bstride + (long)t * d.K;
      for (int k = tid; k < d.K; k += NT) o[k] = 0.f;
    }
    if (l > 0 && t == 0 && tid == 0 && n == 0 && restart) {  // a restart that consumes nothing: layer l-1's idx
      int* idx = d.layers[l - 1].idx + b * 2;
      idx[0] = 0, idx[1] = 0;
    }
    return;
  }
  const long f = (b * d.T + t) * d.fstride;
  float* xb = d.xb + f;

  if (l == 0) {
    const int F = head_feats(d.F);
    float* xf = zs + F * VMAX;  // the frame [F][V], gathered from the clip's strides
    const float* x = d.x + b * d.x_bstride + (long)t * V;
    for (int i = tid; i < F * V; i += NT) {
      const int c = i / V;
      xf[i] = x[c * d.x_stride + (i - c * V)];
    }
    __syncthreads();
    frame_head_in<NT>(xf, F, V, d.C0, d.ln_w, d.ln_b, d.w_in, d.b_in, zs, red, xs, d.C0 + XPAD);
    __syncthreads();
    for (int i = tid; i < V * d.C0 / 4; i += NT) {
      const int v = i * 4 / d.C0, c = i * 4 - v * d.C0;
      reinterpret_cast<float4*>(xb)[i] = *reinterpret_cast<const float4*>(xs + v * (d.C0 + XPAD) + c);
    }
  } else {
    // layer l-1's norms and residual (rt_streams_kernel's step (2) after the FIFO step)
    const layer_t ly = d.layers[l - 1];
    const int Cout = ly.Cout, n4 = V * Cout / 4, ldy = Cout + XPAD;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 va[U4], vr[U4];
#pragma unroll
    for (int j = 0; j < U4; ++j) {
      const int e4 = tid + NT * j;
      va[j] = vr[j] = zero;
      if (e4 < n4) {
        va[j] = reinterpret_cast<const float4*>(d.a + f)[e4];
        if (ly.res_mode == 1) vr[j] = reinterpret_cast<const float4*>(xb)[e4];  // Cin == Cout: the same rows
        if (ly.res_mode == 2) vr[j] = reinterpret_cast<const float4*>(d.r + f)[e4];
      }
    }
    const float2 st = ln_stats_units<NT>(va, n4, red);
    float2 sr = make_float2(0.f, 1.f);
    if (ly.res_mode == 2) sr = ln_stats_units<NT>(vr, n4, red);
#pragma unroll
    for (int j = 0; j < U4; ++j) {
      const int e4 = tid + NT * j;
      if (e4 < n4) {
        float4 o = relu4(affine4(va[j], st.x, st.y, reinterpret_cast<const float4*>(ly.ln_w)[e4],
                                 reinterpret_cast<const float4*>(ly.ln_b)[e4]));
        if (ly.res_mode == 1) o = relu4(add4(o, vr[j]));
        if (ly.res_mode == 2)
          o = relu4(add4(o, affine4(vr[j], sr.x, sr.y, reinterpret_cast<const float4*>(ly.lnr_w)[e4],
                                    reinterpret_cast<const float4*>(ly.lnr_b)[e4])));
        const int v = e4 * 4 / Cout, c = e4 * 4 - v * Cout;
        *reinterpret_cast<float4*>(xs + v * ldy + c) = o;
        if (l < d.L) reinterpret_cast<float4*>(xb)[e4] = o;  // the unit this thread read: in place
      }
    }
    if (t == 0 && tid == 0) {
      const int fi = restart ? 0 : wrap(ly.idx[b * 2], ly.fifo_size), ai = restart ? 0 : wrap(ly.idx[b * 2 + 1], ly.S);
      ly.idx[b * 2] = (fi + n % ly.fifo_size) % ly.fifo_size;
      ly.idx[b * 2 + 1] = (ai + n % ly.S) % ly.S;
    }
  }
  __syncthreads();

  if (l == d.L) {
    const int C = d.layers[d.L - 1].Cout;
    frame_head_out<NT>(xs, C + XPAD, V, C, d.w_out, d.b_out, d.K, zs, d.out + b * d.out_bstride + (long)t * d.K);
    return;
  }

  // layer l's conv + A-mix per (partition, tile), residual conv per tile (rt_streams_kernel's step (1))
  const layer_t ly = d.layers[l];
  const int Cin = ly.Cin, Cout = ly.Cout, P = ly.P, ldx = Cin + XPAD;
  const int E = V * Cout, n4 = E / 4;
  {
    const int ntile = (Cout + 31) / 32, nks = (Cin + 15) / 16, nconv = ntile * P;
    const int ntask = nconv + (ly.res_mode == 2 ? ntile : 0);
    const int row = lane & 31, h = lane >> 5;
    for (int task = w; task < ntask; task += NW) {
      const bool res = task >= nconv;
      const int t2 = res ? task - nconv : task;
      const int p = res ? 0 : t2 / ntile, tile = res ? t2 : t2 - p * ntile;
      const T* panel = res ? static_cast<const T*>(ly.wrp) : static_cast<const T*>(ly.wp) + (long)p * ntile * nks * 512;
      panel += (long)tile * nks * 512;
      float am[16];  // loaded ahead of the k-loop: in flight under it
      amix_coeffs(ly.A, p, V, lane, !res, am);
      f32x16 acc = conv_tile_acc<T, TU>(panel, xs, ldx, nks, row, h, V, Cin, lane);
      float* dst = d.r + f;  // the residual conv goes straight to its rows: 32 consecutive channels per store
      if (!res) {
        f32x16 z;
#pragma unroll
        for (int r = 0; r < 16; ++r) z[r] = 0.f;
        amix_mma(am, acc, z);
        acc = z;
        dst = zs + p * E;
      }
      const int co = tile * 32 + row;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int v = acc_row(r, lane);
        if (v < V && co < Cout) dst[v * Cout + co] = acc[r];
      }
    }
  }
  __syncthreads();
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int e4 = tid; e4 < n4; e4 += NT) {
    float4 s = ly.bias2d ? reinterpret_cast<const float4*>(ly.bias2d)[e4] : zero;
    for (int p = 0; p < P; ++p) s = add4(s, reinterpret_cast<const float4*>(zs + p * E)[e4]);
    reinterpret_cast<float4*>(d.z + f)[e4] = s;
  }
}

DEV float4 box4(float4 oa, float4 s, float4 of) {  // acc + z - fifo, in this association
  return make_float4(oa.x + s.x - of.x, oa.y + s.y - of.y, oa.z + s.z - of.z, oa.w + s.w - of.w);
}

// per: blocks per stream, ceil(V * Cout / 4 / SNT)
__global__ __launch_bounds__(SNT) void rtc_scan_kernel(const desc_t d, const int l, const int per) {
  const layer_t ly = d.layers[l];
  const long b = blockIdx.x / per;
  const int e4 = (int)(blockIdx.x - b * per) * SNT + threadIdx.x;
  const int n4 = d.V * ly.Cout / 4, F = ly.fifo_size, S = ly.S;
  bool restart;
  const int n = stream_frames(d, b, restart);
  if (n < 0 || (n == 0 && !restart) || e4 >= n4) return;
  const int fi = restart ? 0 : wrap(ly.idx[b * 2], F), ai = restart ? 0 : wrap(ly.idx[b * 2 + 1], S);
  const long fs4 = d.fstride / 4;
  float4* fifo = reinterpret_cast<float4*>(ly.fifo) + b * F * n4 + e4;  // slot stride n4
  float4* accu = reinterpret_cast<float4*>(ly.acc) + b * S * n4 + e4;
  const float4* __restrict__ z = reinterpret_cast<const float4*>(d.z) + b * d.T * fs4 + e4;  // frame stride fs4
  float4* __restrict__ a = reinterpret_cast<float4*>(d.a) + b * d.T * fs4 + e4;

  for (int s = 0; s < S; ++s) {  // accumulator slot (ai + s) % S: frames s, s + S, ...
    const int slot = (ai + s) % S;
    float4 va = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!restart) va = accu[(long)slot * n4];
    for (int t0 = s; t0 < n; t0 += SU * S) {
      float4 zt[SU], of[SU];
#pragma unroll
      for (int u = 0; u < SU; ++u) {
        const int t = t0 + u * S;
        zt[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        of[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < n) {
          zt[u] = z[t * fs4];
          if (t >= F) of[u] = z[(t - F) * fs4];
          else if (!restart) of[u] = fifo[(long)((fi + t) % F) * n4];
        }
      }
#pragma unroll
      for (int u = 0; u < SU; ++u) {
        const int t = t0 + u * S;
        if (t < n) {
          va = box4(va, zt[u], of[u]);
          a[t * fs4] = va;
        }
      }
    }
    if (restart || s < n) accu[(long)slot * n4] = va;
  }
  // every read of an old fifo slot is above; the newest min(n, F) z go where the ticks would have left them
  for (int t = max(0, n - F); t < n; ++t) fifo[(long)((fi + t) % F) * n4] = z[t * fs4];
  if (restart)
    for (int j = n; j < F; ++j) fifo[(long)j * n4] = make_float4(0.f, 0.f, 0.f, 0.f);  // fi = 0: frames t < n < F wrote slots 0 .. n-1
}

int max_e(const desc_t& d) {
  int e = d.V * d.C0;
  for (int l = 0; l < d.L; ++l) e = std::max(e, d.V * d.layers[l].Cout);
  return e;
}

// dynamic LDS of frame kernel l, from the network alone: xsf = its input rows, ef = its output rows (at least the
// heads' scratch: 2 * F * VMAX floats of the input head (frame kernel 0: up to 1024, more than three narrow output
// rows hold), CMAX of the output head's pool, both within PMAX * ef)
void frame_lds(const desc_t& d, int l, int& xsf, int& ef) {
  xsf = d.V * ((l == 0 ? d.C0 : d.layers[l - 1].Cout) + XPAD);
  ef = std::max(96, l < d.L ? d.V * d.layers[l].Cout : 0);
  if (l == 0) ef = std::max(ef, ((2 * head_feats(d.F) * VMAX + PMAX - 1) / PMAX + 3) / 4 * 4);
}

template <typename T>
int launch_as(const desc_t& d, hipStream_t s) {
  int most = 0, xsf, ef;
  for (int l = 0; l <= d.L; ++l) {
    frame_lds(d, l, xsf, ef);
    most = std::max(most, xsf + PMAX * ef + 16);
  }
  if (stgcn_lds_attr((const void*)rtc_frame_kernel<T>, most * (int)sizeof(float), s)) return STGCN_EHIP;
  const unsigned nbt = (unsigned)d.B * (unsigned)d.T;
  for (int l = 0; l <= d.L; ++l) {
    frame_lds(d, l, xsf, ef);
    const int lds = (xsf + PMAX * ef + 16) * (int)sizeof(float);
    hipLaunchKernelGGL(rtc_frame_kernel<T>, dim3(nbt), dim3(NT), lds, s, d, l, xsf, ef);
    if (l < d.L) {
      const int per = (d.V * d.layers[l].Cout / 4 + SNT - 1) / SNT;
      hipLaunchKernelGGL(rtc_scan_kernel, dim3((unsigned)d.B * per), dim3(SNT), 0, s, d, l, per);
    }
  }
  return hipGetLastError() == hipSuccess ? STGCN_OK : STGCN_EHIP;
}

}  // namespace

int rt_streams_clip_launch(const stgcn_rt_streams_clip_desc& d, hipStream_t s) {
  // stgcn_rt_streams's limits
  if (d.V < 2 || d.V > VMAX || d.L < 1 || d.L > STGCN_RT_MAX_LAYERS || d.C0 < 4 || d.C0 > CMAX || d.C0 % 4 ||
      d.V * d.C0 > MAXE || d.K < 1 || d.B < 1)
    return STGCN_EBADSHAPE;
  if (d.T < 1 || d.T > STGCN_RT_CLIP_MAX_T || d.t0 < 0 || (long)d.B * d.T > 0x7fffffffL || !head_feats_ok(d.F, d.V))
    return STGCN_EBADSHAPE;
  int cin = d.C0;
  bool resconv = false;
  for (int l = 0; l < d.L; ++l) {
    const layer_t& y = d.layers[l];
    if (y.Cin != cin || y.Cout < 4 || y.Cout > CMAX || y.Cout % 4 || d.V * y.Cout > MAXE || y.P < 1 || y.P > PMAX ||
        y.fifo_size < 1 || y.S < 1 || y.res_mode < 0 || y.res_mode > 2 || (y.res_mode == 1 && y.Cin != y.Cout))
      return STGCN_EBADSHAPE;
    resconv |= y.res_mode == 2;
    cin = y.Cout;
  }
  if (d.dtype != 0 && d.dtype != 1) return STGCN_EDTYPE;
  if ((long)d.B * ((MAXE / 4 + SNT - 1) / SNT) > 0x7fffffffL) return STGCN_EBADSHAPE;  // blockIdx.x: (stream, block)
  if (!d.x || !d.active || !d.lengths || !d.ln_w || !d.ln_b || !d.w_in || !d.b_in || !d.w_out || !d.out || !d.xb ||
      !d.z || !d.a || (resconv && !d.r))
    return STGCN_EBADSHAPE;
  if (d.fstride < max_e(d) || d.fstride % 4 || d.x_stride < (long)d.T * d.V || d.out_bstride < (long)d.T * d.K ||
      (d.B > 1 && d.x_bstride < head_feats(d.F) * d.x_stride))
    return STGCN_EBADSHAPE;
  for (int l = 0; l < d.L; ++l) {
    const layer_t& y = d.layers[l];
    if (!y.A || !y.wp || !y.ln_w || !y.ln_b || !y.fifo || !y.acc || !y.idx ||
        (y.res_mode == 2 && (!y.wrp || !y.lnr_w || !y.lnr_b)))
      return STGCN_EBADSHAPE;
  }
  return d.dtype == 0 ? launch_as<float>(d, s) : launch_as<bf16>(d, s);
}
