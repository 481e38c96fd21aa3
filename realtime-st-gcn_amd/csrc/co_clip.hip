// CoST-GCN clip inference (stgcn_co_clip): T consecutive frames of ONE stream per call, on the stream's own rings.
// Column t of the output is what the per-frame route would give for frame t from the stream's current state, and the
// rings and indices end where T per-frame calls would have left them.  Frame t of the clip takes the place of stream b
// of co_streams.hip, so the heads, the graph conv, the push arithmetic and the LayerNorm statistics are frame_ops.h's;
// the temporal conv of a layer becomes ONE causal dilated GEMM with T*V rows that reads the tap weights once per clip.
// The stage bodies are clip_ops.h's, shared with co_streams_clip.hip (B streams per call); the kernels here pass the
// descriptor's pointers as they are.
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
#include "clip_ops.h"
#include "../../include/stgcn_amd.h"

namespace {
using namespace clip_ops;  // the block sizes, G, and the stages themselves: shared with co_streams_clip.hip
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
  in_frame(x + t * V, x_stride, V, C0, ln_w, ln_b, w_in, b_in, xf, xi, red, h0 + t * V * C0);
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
  const long t = blockIdx.x, E = (long)V * ly.Cout;
  gcn_frame(ly, V, x + t * V * ly.Cin, ly.z_buf + t * E, ly.r_buf + t * E, xs);
}

// ---------------------------------------------------------------------------------------------------- push + carry
// blocks [0, T): frame t's push; then fifo-1 + Kt/2 carry blocks (carry_block)
template <typename T>
__global__ __launch_bounds__(FNT) void cc_push_kernel(const layer_t ly, int V, int Tn, const float* __restrict__ x) {
  __shared__ float red[FNT / 64];
  const long E = (long)V * ly.Cout;
  T* hist = reinterpret_cast<T*>(ly.hist);
  const int b = blockIdx.x;
  if (b < Tn) {
    const float* res = ly.res_mode == 2 ? ly.r_buf + b * E : x + b * E;  // mode 1: Cin == Cout
    push_frame<T>(ly, V, b, ly.z_buf + b * E, res, hist, ly.resq, red);
    return;
  }
  carry_block<T>(ly, V, b - Tn, false, reinterpret_cast<const T*>(ly.ring), ly.res_ring, ly.idx, hist, ly.resq);
}

// ---------------------------------------------------------------------------------------------------- taps
template <typename T, int TU>
__global__ __launch_bounds__(TNT) void cc_taps_kernel(const layer_t ly, int V, int M, int nks, int nsplit) {
  __shared__ float red[TNW][16][64];
  taps_block<T, TU>(ly, V, M, nks, nsplit, blockIdx.x, blockIdx.y * (G * 32), reinterpret_cast<const T*>(ly.hist),
                    ly.partial, red);
}

// ---------------------------------------------------------------------------------------------------- finish
// Block 0's thread 0 advances both indices by T: no other thread of this launch reads them.
__global__ __launch_bounds__(FNT) void cc_finish_kernel(const layer_t ly, int V, int Tn, int nsplit) {
  __shared__ float red[FNT / 64];
  const long E = (long)V * ly.Cout, t = blockIdx.x;
  finish_frame(ly, V, nsplit, ly.partial + t * nsplit * E, ly.resq + t * E, ly.y + t * E, red);
  if (t == 0 && threadIdx.x == 0) advance_idx(ly.idx, ly.S, ly.Kt, Tn, false);
}

// ---------------------------------------------------------------------------------------------------- state
// blocks [0, na): the j-th newest activation frame (t = T-1-j) -> ring slot (idx[0] + j) % fifo, idx already advanced;
// blocks [na, na + nr): the j-th newest residual row -> res_ring slot (idx[1] + j) % R
template <typename T>
__global__ __launch_bounds__(FNT) void cc_state_kernel(const layer_t ly, int V, int Tn, int na) {
  const int j = blockIdx.x;
  const bool res = j >= na;
  state_block<T>(ly, V, Tn, res, res ? j - na : j, false, reinterpret_cast<T*>(ly.ring), ly.res_ring, ly.idx,
                 reinterpret_cast<const T*>(ly.hist), ly.resq);
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
  return num_splits(y.Cout, y.Kt, y.splits);
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
