// RT-ST-GCN per-frame inference for a batch of B independent skeleton streams (stgcn_rt_streams), LayerNorm online
// layers, conv operands fp32 or bf16 (template parameter T; all that follows the conv accumulators is fp32 in both):
// one workgroup per stream runs the whole network for its stream's frame (frame_ops.h's stages: frame_head_in, per
// layer conv_tile_acc + amix_coeffs / amix_mma and the FIFO step + norms below, frame_head_out) with the layer input
// and output in LDS, the weights streamed from L2 (shared by every workgroup) and the stream's FIFO state updated in
// place.  No workgroup waits on another: no grid barrier, no spin, no atomics.  B may exceed the CU count; the
// workgroups queue.
//
// Per layer (V <= 32 joint rows, zero-padded to the 32-row MFMA operand by the fragment loads):
//   (1) tasks over the 8 waves: (partition p, 32-channel tile) of the conv, and (tile) of the residual conv.
//       Y_p[u][co] = sum_ci x[u][ci] W[p*Cout+co][ci]: v_mfma_f32_32x32x2_f32 (T = float) or v_mfma_f32_32x32x16_bf16
//       (T = bf16), A operand = x rows from LDS, B operand = the packed weight image in T (co_frame.hip's
//       [tile][k-step][lane][8]: one contiguous piece per lane per 16-k step, read once).  LDS keeps the rows in fp32
//       only; the bf16 A fragment is rounded (nearest even) from them as it is loaded, so the identity residual and
//       every later step read the unrounded values.
//       The A-mix runs on the accumulators where they are (amix_mma): Z_p[v][co] = sum_u A_p[u][v] Y_p[u][co].
//       Z_p -> LDS zs[p], the residual conv -> LDS rs.
//   (2) z = bias2d + Z_0 + Z_1 + Z_2; a = acc[ai] + z - fifo[fi]; acc[ai] = a; fifo[fi] = z (rtstgcn.py:591-627);
//       y = relu(relu(LN(a)) + res) (rt_fused.hip's rt_norm math; two-pass statistics ln_stats_units, fixed-order sums) -> LDS xs.
// Every sum has a fixed order that depends on the network only: a stream's frames are bit-identical whatever B, its
// slot and the other streams' masks are.
#include "common.h"
#include "launchers.h"
#include "frame_ops.h"
#include "../../include/stgcn_amd.h"

namespace {

constexpr int NT = 512;
constexpr int NW = NT / 64;
constexpr int U4 = (MAXE / 4 + NT - 1) / NT;  // float4 units of a frame per thread
constexpr int TU = 4;                         // k-steps in flight per wave
constexpr int XS_FLOATS = MAXE + VMAX * XPAD;
// dynamic LDS (floats): xs | rs | zs[PMAX] | red
constexpr int LDS_FLOATS = XS_FLOATS + MAXE + PMAX * MAXE + 16;

template <typename T>
__global__ __launch_bounds__(NT) void rt_streams_kernel(const stgcn_rt_streams_desc d) {
  extern __shared__ __attribute__((aligned(16))) float rs_sm[];
  float* xs = rs_sm;            // [V][C + XPAD] the current layer's input
  float* rs = xs + XS_FLOATS;   // [V][Cout] residual conv
  float* zs = rs + MAXE;        // [P][V][Cout] A-mixed conv per partition; the heads' scratch
  float* red = zs + PMAX * MAXE;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, V = d.V;
  const long b = blockIdx.x;
  const int code = d.active[b];
  float* out = d.out + b * d.K;
  if (code == 0) {  // skip: state untouched, a zero row (uniform over the workgroup)
    for (int k = tid; k < d.K; k += NT) out[k] = 0.f;
    return;
  }
  const bool restart = code == 2;
  if (restart) {  // clear this stream's FIFOs and accumulators; every later write of them follows a barrier
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int l = 0; l < d.L; ++l) {
      const stgcn_rt_streams_layer ly = d.layers[l];
      const long E4 = (long)V * ly.Cout / 4;
      float4* f = reinterpret_cast<float4*>(ly.fifo) + b * ly.fifo_size * E4;
      float4* a = reinterpret_cast<float4*>(ly.acc) + b * ly.S * E4;
      for (long i = tid; i < ly.fifo_size * E4; i += NT) f[i] = z4;
      for (long i = tid; i < ly.S * E4; i += NT) a[i] = z4;
    }
  }

  const int F = head_feats(d.F);
  frame_head_in<NT>(d.x + b * F * V, F, V, d.C0, d.ln_w, d.ln_b, d.w_in, d.b_in, zs, red, xs, d.C0 + XPAD);
  __syncthreads();

  for (int l = 0; l < d.L; ++l) {
    const stgcn_rt_streams_layer ly = d.layers[l];
    const int Cin = ly.Cin, Cout = ly.Cout, P = ly.P, ldx = Cin + XPAD;
    const int E = V * Cout, n4 = E / 4;
    const int fi = restart ? 0 : ly.idx[b * 2], ai = restart ? 0 : ly.idx[b * 2 + 1];
    // (1) conv + A-mix per (partition, tile), residual conv per tile
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
        float* dst = rs;
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
    // (2) FIFO step, norms, residual
    {
      float* fifo = ly.fifo + (b * ly.fifo_size + fi) * E;
      float* accu = ly.acc + (b * ly.S + ai) * E;
      const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
      float4 va[U4], vr[U4];
#pragma unroll
      for (int j = 0; j < U4; ++j) {
        const int e4 = tid + NT * j;
        va[j] = vr[j] = zero;
        if (e4 < n4) {
          float4 s = ly.bias2d ? reinterpret_cast<const float4*>(ly.bias2d)[e4] : zero;
          for (int p = 0; p < P; ++p) s = add4(s, reinterpret_cast<const float4*>(zs + p * E)[e4]);
          const float4 oa = restart ? zero : reinterpret_cast<const float4*>(accu)[e4];
          const float4 of = restart ? zero : reinterpret_cast<const float4*>(fifo)[e4];
          const float4 a = make_float4(oa.x + s.x - of.x, oa.y + s.y - of.y, oa.z + s.z - of.z, oa.w + s.w - of.w);
          reinterpret_cast<float4*>(accu)[e4] = a;
          reinterpret_cast<float4*>(fifo)[e4] = s;
          va[j] = a;
          if (ly.res_mode == 1) {
            const int v = e4 * 4 / Cout, c = e4 * 4 - v * Cout;  // Cin == Cout
            vr[j] = *reinterpret_cast<const float4*>(xs + v * ldx + c);
          }
          if (ly.res_mode == 2) vr[j] = reinterpret_cast<const float4*>(rs)[e4];
        }
      }
      const float2 st = ln_stats_units<NT>(va, n4, red);
      float2 sr = make_float2(0.f, 1.f);
      if (ly.res_mode == 2) sr = ln_stats_units<NT>(vr, n4, red);
      __syncthreads();  // every read of xs (the identity residual) before the overwrite
      const int ldy = Cout + XPAD;
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
        }
      }
      if (tid == 0) {
        ly.idx[b * 2] = (fi + 1) % ly.fifo_size;
        ly.idx[b * 2 + 1] = (ai + 1) % ly.S;
      }
      __syncthreads();
    }
  }

  const int C = d.layers[d.L - 1].Cout;
  frame_head_out<NT>(xs, C + XPAD, V, C, d.w_out, d.b_out, d.K, zs, out);
}

template <typename T>
int launch_as(const stgcn_rt_streams_desc& d, hipStream_t s) {
  constexpr int lds = LDS_FLOATS * (int)sizeof(float);
  if (stgcn_lds_attr((const void*)rt_streams_kernel<T>, lds, s)) return STGCN_EHIP;
  hipLaunchKernelGGL(rt_streams_kernel<T>, dim3((unsigned)d.B), dim3(NT), lds, s, d);
  return hipGetLastError() == hipSuccess ? STGCN_OK : STGCN_EHIP;
}

}  // namespace

int rt_streams_launch(const stgcn_rt_streams_desc& d, hipStream_t s) {
  if (!d.x || !d.active || !d.ln_w || !d.ln_b || !d.w_in || !d.b_in || !d.w_out || !d.out) return STGCN_EBADSHAPE;
  if (d.V < 2 || d.V > VMAX || d.L < 1 || d.L > STGCN_RT_MAX_LAYERS || d.C0 < 4 || d.C0 > CMAX || d.C0 % 4 ||
      d.V * d.C0 > MAXE || d.K < 1 || d.B < 1 || !head_feats_ok(d.F, d.V))
    return STGCN_EBADSHAPE;
  if (d.dtype != 0 && d.dtype != 1) return STGCN_EDTYPE;
  int cin = d.C0;
  for (int l = 0; l < d.L; ++l) {
    const stgcn_rt_streams_layer& y = d.layers[l];
    if (y.Cin != cin || y.Cout < 4 || y.Cout > CMAX || y.Cout % 4 || d.V * y.Cout > MAXE || y.P < 1 || y.P > PMAX ||
        y.fifo_size < 1 || y.S < 1 || y.res_mode < 0 || y.res_mode > 2 || (y.res_mode == 1 && y.Cin != y.Cout))
      return STGCN_EBADSHAPE;
    if (!y.A || !y.wp || !y.ln_w || !y.ln_b || !y.fifo || !y.acc || !y.idx ||
        (y.res_mode == 2 && (!y.wrp || !y.lnr_w || !y.lnr_b)))
      return STGCN_EBADSHAPE;
    cin = y.Cout;
  }
  return d.dtype == 0 ? launch_as<float>(d, s) : launch_as<bf16>(d, s);
}
