// CoST-GCN clip inference: stream b of B independent streams advances by n_b consecutive frames per call, on the
// stream-major state of co_streams.hip (stgcn_co_streams_clip); stgcn_co_clip, one stream on its own rings, is the
// B = 1 case of the same kernels.  Column t of a stream's output is what the per-frame route would give for frame t
// from the stream's current state, and its rings and indices end where n_b per-frame calls would have left them.
// Frame t of a clip takes the place of stream b of co_streams.hip, so the heads, the graph conv, the push arithmetic and
// the LayerNorm statistics are frame_ops.h's; the temporal conv of a layer becomes ONE causal dilated GEMM with n_b*V
// rows per stream that reads the tap weights once per clip.  The stage bodies are clip_ops.h's, called on pointers
// offset to stream b.
//
// A layer works on linear clip buffers per stream, time ascending, the carried history in front of the new frames:
//   hist [fifo-1 + T][V][C]  compute dtype: ReLU(LN1(z)) of the fifo-1 frames the ring carried in, then of frame 0..T-1
//   resq [Kt/2   + T][V][C]  fp32: the residual rows of the Kt/2 frames the residual ring carried in, then the new ones
// so frame t's tap k is hist row block fifo-1 + t - k*S and its residual is resq row block t: no ring arithmetic in
// the hot kernel.
//
// active [B] and lengths [B] are read on the device by every block (stream_frames), so a captured call replays with
// other codes and lengths, and nothing is compacted on the host: a block whose frame, row tile or ring slot lies beyond
// n_b, or whose stream has code 0, returns after those two loads (co_streams.hip's skip).  stgcn_co_clip passes neither
// (Call's null form): its one stream has code 1 and consumes all T frames.
//
// Launches per call, 2 + 5 L whatever B and T are, every hand-off a kernel boundary, no workgroup waits on another;
// blockIdx.x = b * (blocks per stream) + i:
//   csc_in     : T blocks per stream: h0[b][t] = fcn_in(LayerNorm([F,1,V])(x[b][:, t])): frame_head_in          (i < n_b)
//   per layer:
//   csc_gcn    : T per stream: z[b][t] = gcn(x[t], A), r[b][t] = Wr x[t] + br: cs_gcn_kernel's body            (i < n_b)
//   csc_push   : T + fifo-1 + Kt/2 per stream: co_push_stage of frame i into hist[b][fifo-1+i] / resq[b][Kt/2+i]
//                (i < n_b), then the carry blocks (n_b > 0), one carried ring slot each copied into the front of hist /
//                resq: the stream's ring frames, or on a restart the empty FIFO's rows (ReLU(ln1_b) / zero) without a
//                read of ring, res_ring or idx.  The ONLY launch that reads rings, and it writes none.
//   csc_taps   : splits x ceil(T*V / 128) per stream: partial[b][t][s][v][co] = sum over K split s of Wp . hist.  Rows
//                are m = t*V + v < n_b*V, dense per stream (no padding of a frame to 32 rows); a row tile never spans
//                two streams, whose histories are different buffers.  A block takes G = 4 consecutive 32-row tiles
//                (about 5 frames at V = 25) and one K split; its 8 waves share out the column tiles (taps_nsub), so a
//                weight B fragment is loaded once for the G row tiles and the tiles' overlapping history rows are
//                re-read on one CU.
//   csc_finish : T per stream: u = bt + sum_s partial[b][t][s] (index order), y[b][t] = relu(LN2(u) + resq[b][t])
//                (i < n_b); thread 0 of the stream's block 0 advances idx[b] by n_b, from 0 on a restart; no other
//                thread of the launch reads idx
//   csc_state  : fifo + Kt/2+1 per stream, one ring slot each: the min(n_b, slots) newest clip frames into the slots the
//                per-frame route would have used (new frame t: slot (idx0 - 1 - t) mod fifo, derived from the advanced
//                idx); on a restart the other slots get the empty rows; otherwise the blocks beyond n_b return.  The
//                ONLY launch that writes rings.
//   csc_out    : T per stream: out[b][t] = fcn_out(mean_v y_last[b][t]): frame_head_out; zero rows for t >= n_b and for
//                skipped streams
// The hazard of a clip (new frame t = fifo-1-j takes the slot of the carried frame of age j, which earlier clip frames
// still need) is designed out: csc_push copies the carried frames out before anything writes a ring, csc_state writes
// the rings after csc_taps and csc_finish have run, and those two kernel boundaries lie between the last ring read and
// the first ring write.  Nothing depends on the order of blocks inside a launch: every block reads what earlier
// launches wrote and writes rows of its own.
//
// Order of every sum, none of which depends on B, T, the frame's position in the clip or the device: k-steps in
// sequence within a wave (an MFMA row's result does not depend on which of the 32 rows it is), the nsub K-interleaves
// of a column tile in index order, the splits in index order (num_splits: a function of (Cout, Kt) alone), LayerNorm
// statistics through ln_stats_units<1024>.  No atomics, no cooperative launch, no spin.  So a stream's outputs and state
// do not depend on B, its slot, T, t0 chunking or the other streams, and any split of a clip into consecutive clips
// gives the same bits.
#include "common.h"
#include "launchers.h"
#include "frame_ops.h"
#include "clip_ops.h"
#include "../../include/stgcn_amd.h"

namespace {
using namespace clip_ops;
using layer_t = stgcn_co_clip_layer;  // stgcn_co_streams_clip_layer is the same type

// what every block needs of the call besides its layer
struct Call {
  const int* active;  // nullptr (stgcn_co_clip): every stream has code 1 and consumes all T frames
  const int* lengths;
  int T, t0;
};

// n_b = clamp(lengths[b] - t0, 0, T), or -1 for a skipped stream (no frame, carry or slot index is below it);
// restart: code 2 on the first call of the caller's clip
DEV int stream_frames(const Call c, long b, bool& restart) {
  restart = false;
  if (!c.active) return c.T;  // uniform over the launch
  const int code = c.active[b], len = c.lengths[b];
  restart = code == 2 && c.t0 == 0;
  if (code == 0) return -1;
  return len <= c.t0 ? 0 : min(len - c.t0, c.T);
}

// ---------------------------------------------------------------------------------------------------- heads
// x is the (F, T, V) clip of stream b as given: channel c of frame t at x[b * x_bstride + c * x_stride + t * V]
__global__ __launch_bounds__(HNT) void csc_in_kernel(const Call c, const float* __restrict__ x, long x_stride,
                                                     long x_bstride, int F, int V, int C0, const float* __restrict__ ln_w,
                                                     const float* __restrict__ ln_b, const float* __restrict__ w_in,
                                                     const float* __restrict__ b_in, float* __restrict__ h0) {
  __shared__ float xf[FMAX * VMAX];
  __shared__ float xi[FMAX * VMAX];
  __shared__ float red[HNT / 64];
  const long b = blockIdx.x / c.T, t = blockIdx.x - b * c.T;
  bool restart;
  if (t >= stream_frames(c, b, restart)) return;
  in_frame(x + b * x_bstride + t * V, x_stride, F, V, C0, ln_w, ln_b, w_in, b_in, xf, xi, red, h0 + (b * c.T + t) * V * C0);
}

__global__ __launch_bounds__(HNT) void csc_out_kernel(const Call c, const float* __restrict__ y, int V, int C,
                                                      const float* __restrict__ w_out, const float* __restrict__ b_out,
                                                      int K, float* __restrict__ out, long out_bstride) {
  __shared__ float pool[CMAX];
  const long b = blockIdx.x / c.T, t = blockIdx.x - b * c.T;
  float* o = out + b * out_bstride + t * K;
  bool restart;
  if (t >= stream_frames(c, b, restart)) {
    for (int k = threadIdx.x; k < K; k += HNT) o[k] = 0.f;
    return;
  }
  frame_head_out<HNT>(y + (b * c.T + t) * V * C, C, V, C, w_out, b_out, K, pool, o);
}

// ---------------------------------------------------------------------------------------------------- per layer
// x: the layer's input rows [B][T][V][Cin]
__global__ __launch_bounds__(GNT) void csc_gcn_kernel(const layer_t ly, const Call c, int V, const float* __restrict__ x) {
  __shared__ __attribute__((aligned(16))) float xs[VMAX * (CMAX + XPAD)];
  const long b = blockIdx.x / c.T, t = blockIdx.x - b * c.T, E = (long)V * ly.Cout, f = b * c.T + t;
  bool restart;
  if (t >= stream_frames(c, b, restart)) return;
  gcn_frame(ly, V, x + f * V * ly.Cin, ly.z_buf + f * E, ly.r_buf + f * E, xs);
}

template <typename T>
__global__ __launch_bounds__(FNT) void csc_push_kernel(const layer_t ly, const Call c, int V, const float* __restrict__ x) {
  __shared__ float red[FNT / 64];
  const long E = (long)V * ly.Cout;
  const int fifo = ring_slots(ly.S, ly.Kt), R = res_slots(ly.Kt), per = c.T + fifo - 1 + R - 1;
  const long b = blockIdx.x / per;
  const int i = (int)(blockIdx.x - b * per);
  bool restart;
  const int n = stream_frames(c, b, restart);
  T* hist = reinterpret_cast<T*>(ly.hist) + b * (fifo - 1 + c.T) * E;
  float* resq = ly.resq + b * (R - 1 + c.T) * E;
  if (i < c.T) {
    if (i >= n) return;
    const long f = b * c.T + i;
    const float* res = ly.res_mode == 2 ? ly.r_buf + f * E : x + f * E;  // mode 1: Cin == Cout
    push_frame<T>(ly, V, i, ly.z_buf + f * E, res, hist, resq, red);
    return;
  }
  if (n <= 0) return;  // no frame of this call reads the stream's history
  carry_block<T>(ly, V, i - c.T, restart, reinterpret_cast<const T*>(ly.ring) + b * fifo * E, ly.res_ring + b * R * E,
                 ly.idx + b * 2, hist, resq);
}

template <typename T, int TU>
__global__ __launch_bounds__(TNT) void csc_taps_kernel(const layer_t ly, const Call c, int V, int nks, int nsplit,
                                                       int ngroup) {
  __shared__ float red[TNW][16][64];
  const int per = nsplit * ngroup;
  const long b = blockIdx.x / per;
  const int i = (int)(blockIdx.x - b * per), grp = i / nsplit, s = i - grp * nsplit, m0 = grp * (G * 32);
  bool restart;
  const int M = stream_frames(c, b, restart) * V;
  if (m0 >= M) return;  // uniform over the block
  const long E = (long)V * ly.Cout;
  const int Hh = ring_slots(ly.S, ly.Kt) - 1;
  taps_block<T, TU>(ly, V, M, nks, nsplit, s, m0, reinterpret_cast<const T*>(ly.hist) + b * (Hh + c.T) * E,
                    ly.partial + b * c.T * nsplit * E, red);
}

__global__ __launch_bounds__(FNT) void csc_finish_kernel(const layer_t ly, const Call c, int V, int nsplit) {
  __shared__ float red[FNT / 64];
  const long b = blockIdx.x / c.T, t = blockIdx.x - b * c.T, E = (long)V * ly.Cout, f = b * c.T + t;
  bool restart;
  const int n = stream_frames(c, b, restart);
  if (t < n)
    finish_frame(ly, V, nsplit, ly.partial + f * nsplit * E, ly.resq + (b * (res_slots(ly.Kt) - 1 + c.T) + t) * E,
                 ly.y + f * E, red);
  if (t == 0 && threadIdx.x == 0 && (n > 0 || (n == 0 && restart)))  // code 1 with no frame: idx stays as it is
    advance_idx(ly.idx + b * 2, ly.S, ly.Kt, n, restart);
}

template <typename T>
__global__ __launch_bounds__(FNT) void csc_state_kernel(const layer_t ly, const Call c, int V) {
  const long E = (long)V * ly.Cout;
  const int fifo = ring_slots(ly.S, ly.Kt), R = res_slots(ly.Kt), per = fifo + R;
  const long b = blockIdx.x / per;
  const int i = (int)(blockIdx.x - b * per);
  const bool res = i >= fifo;
  const int j = res ? i - fifo : i;
  bool restart;
  const int n = stream_frames(c, b, restart);
  if (n < 0 || (j >= n && !restart)) return;
  state_block<T>(ly, V, n, res, j, restart, reinterpret_cast<T*>(ly.ring) + b * fifo * E, ly.res_ring + b * R * E,
                 ly.idx + b * 2, reinterpret_cast<const T*>(ly.hist) + b * (fifo - 1 + c.T) * E,
                 ly.resq + b * (R - 1 + c.T) * E);
}

template <typename T>
void launch_layer(const layer_t& y, const Call& c, int B, int V, int nsplit, const float* x, hipStream_t s) {
  const unsigned fifo = ring_slots(y.S, y.Kt), R = res_slots(y.Kt), Tn = c.T, nb = B;
  const int nks = num_ksteps(y.Cout, y.Kt), ngroup = (c.T * V + G * 32 - 1) / (G * 32);
  hipLaunchKernelGGL(csc_gcn_kernel, dim3(nb * Tn), dim3(GNT), 0, s, y, c, V, x);
  hipLaunchKernelGGL(csc_push_kernel<T>, dim3(nb * (Tn + fifo - 1 + R - 1)), dim3(FNT), 0, s, y, c, V, x);
  constexpr int TU = sizeof(T) == 2 ? 4 : 2;
  hipLaunchKernelGGL((csc_taps_kernel<T, TU>), dim3(nb * nsplit * ngroup), dim3(TNT), 0, s, y, c, V, nks, nsplit, ngroup);
  hipLaunchKernelGGL(csc_finish_kernel, dim3(nb * Tn), dim3(FNT), 0, s, y, c, V, nsplit);
  hipLaunchKernelGGL(csc_state_kernel<T>, dim3(nb * (fifo + R)), dim3(FNT), 0, s, y, c, V);
}

// The checks and the launch sequence of both entries, on the fields their descriptors D have in common (neither has
// the other's B, t0, active, lengths or stream strides).
// shapes, then the dtype: co_check's limits per layer are this route's limits
template <typename D>
int check_shapes(const D& d) {
  if (d.T < 1 || d.T > STGCN_CO_CLIP_MAX_T || d.L < 1 || d.L > STGCN_RT_MAX_LAYERS || d.K < 1 || d.C0 < 4 ||
      d.C0 > CMAX || d.C0 % 4 || !head_feats_ok(d.F, d.V))
    return STGCN_EBADSHAPE;
  int cin = d.C0;
  for (int l = 0; l < d.L; ++l) {
    const layer_t& y = d.layers[l];
    if (y.Cin != cin) return STGCN_EBADSHAPE;
    stgcn_co_layer c = {};  // the single-frame descriptor that carries the same shape
    c.V = d.V, c.Cin = y.Cin, c.Cout = y.Cout, c.P = y.P, c.Kt = y.Kt, c.S = y.S;
    c.res_mode = y.res_mode, c.dtype = d.dtype, c.splits = y.splits;
    const int rc = co_check(c, true);
    if (rc != STGCN_OK) return rc;
    cin = y.Cout;
  }
  return STGCN_OK;
}

template <typename D>
int check_pointers(const D& d) {
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

template <typename D>
int launch(const D& d, const Call& c, int B, long x_bstride, long out_bstride, hipStream_t s) {
  const int V = d.V;
  const unsigned nbt = (unsigned)B * (unsigned)d.T;
  hipLaunchKernelGGL(csc_in_kernel, dim3(nbt), dim3(HNT), 0, s, c, d.x, d.x_stride, x_bstride, head_feats(d.F), V, d.C0, d.ln_w,
                     d.ln_b,
                     d.w_in, d.b_in, d.h0);
  const float* x = d.h0;
  for (int l = 0; l < d.L; ++l) {
    const layer_t& y = d.layers[l];
    const int nsplit = co_clip_num_splits(y);
    if (d.dtype == 0) launch_layer<float>(y, c, B, V, nsplit, x, s);
    else launch_layer<bf16>(y, c, B, V, nsplit, x, s);
    x = y.y;
  }
  const layer_t& last = d.layers[d.L - 1];
  hipLaunchKernelGGL(csc_out_kernel, dim3(nbt), dim3(HNT), 0, s, c, x, V, last.Cout, d.w_out, d.b_out, d.K, d.out,
                     out_bstride);
  return hipGetLastError() == hipSuccess ? STGCN_OK : STGCN_EHIP;
}

// the largest grid of a call, per stream: a layer's push, state or tap blocks (shapes already checked)
long max_blocks_per_stream(const stgcn_co_streams_clip_desc& d) {
  const long groups = ((long)d.T * d.V + G * 32 - 1) / (G * 32);
  long n = d.T;
  for (int l = 0; l < d.L; ++l) {
    const layer_t& y = d.layers[l];
    const long slots = ring_slots(y.S, y.Kt) + res_slots(y.Kt);
    n = std::max(n, std::max(d.T + slots, co_clip_num_splits(y) * groups));
  }
  return n;
}

}  // namespace

// K splits of a layer's tap stage: a function of (Cout, Kt) and the forced count alone (clip_ops::num_splits)
int co_clip_num_splits(const stgcn_co_clip_layer& y) { return num_splits(y.Cout, y.Kt, y.splits); }

// 0 when the descriptor's shapes, dtype and (unless shapes_only) pointers are usable
int co_clip_check(const stgcn_co_clip_desc& d, bool shapes_only) {
  const int rc = check_shapes(d);
  return rc != STGCN_OK || shapes_only ? rc : check_pointers(d);
}

int co_streams_clip_check(const stgcn_co_streams_clip_desc& d, bool shapes_only) {
  if (d.B < 1 || d.t0 < 0) return STGCN_EBADSHAPE;
  const int rc = check_shapes(d);
  if (rc != STGCN_OK) return rc;
  if ((long)d.B * max_blocks_per_stream(d) > 0x7fffffffL) return STGCN_EBADSHAPE;  // blockIdx.x carries (stream, block)
  if (shapes_only) return STGCN_OK;
  if (!d.active || !d.lengths || d.out_bstride < (long)d.T * d.K || (d.B > 1 && d.x_bstride < head_feats(d.F) * d.x_stride))
    return STGCN_EBADSHAPE;
  return check_pointers(d);
}

// one stream on the descriptor's own pointers: B = 1, no stream strides, no codes and no lengths
int co_clip_launch(const stgcn_co_clip_desc& d, hipStream_t s) {
  return launch(d, Call{nullptr, nullptr, d.T, 0}, 1, 0, 0, s);
}

int co_streams_clip_launch(const stgcn_co_streams_clip_desc& d, hipStream_t s) {
  return launch(d, Call{d.active, d.lengths, d.T, d.t0}, d.B, d.x_bstride, d.out_bstride, s);
}
