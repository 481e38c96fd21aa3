// Snapshot and restore of live streams of the stream batches (stgcn_stream_state_export / _import): the per-layer state
// of rt_streams.hip (fifo [B][fifo_size][V][C], acc [B][S][V][C], idx [B][2]) and of co_streams.hip (ring
// [B][S*(Kt-1)+1][V][C] in the compute dtype, res_ring [B][Kt/2+1][V][C], idx [B][2]) to and from the canonical image:
// per selected stream one fp32 row [E] of the snapshot, layer-major, each state tensor rotated along its slot axis so
// that it is the original with both stored indices 0:
//
//   image[off_t + k * V*C + e] = tensor_t[slot][(idx_t + k) % n_t][e],   k < n_t, e < V*C.
//
// Every kernel of both families addresses a slot only relative to the stored index (rt: fifo[(fi + t) % F],
// acc[(ai + s) % S]; co: ring_head(idx, n) = (idx + n - 1) % n for the push and (head + tap * S) % n, (rhead + Kt/2) % R for the
// reads, advance_idx / state_block / carry_block of clip_ops.h likewise), so the rotated state with indices (0, 0)
// gives the same bits from every later step or step_clip.  No value is recomputed: the rt accumulators are copied as
// they are.
//
// One launch for all layers and all selected streams.  The work is cut into chunks of NT * U units of W elements (one
// 16-byte access on the fp32 side, two for W = 8); blockIdx.x = selected stream * (chunks of a stream) + chunk, and a
// workgroup finds its (layer tensor, chunk within it) by walking the at most 2 * L chunk counts.  It reads slots[i] and
// the stream's index on the device; a slot outside [0, B) returns before any other access.  Export folds the rotation
// into the source address; import writes the image at rotation 0 (a linear copy with the cast to the ring's dtype,
// nearest even) and idx = (0, 0).  Plain vector loads and stores: no atomics, no LDS, no barrier, nothing waits on
// another workgroup.
#include "common.h"
#include "launchers.h"
#include "frame_ops.h"
#include "../../include/stgcn_amd.h"

namespace {

using desc_t = stgcn_stream_state_desc;
using layer_t = stgcn_stream_state_layer;

constexpr int NT = 256;
constexpr int U = 4;  // units per thread, loaded ahead of the stores

constexpr long chunk_units = (long)NT * U;

// elements per unit of a tensor with E = V * C elements per slot: 8 bf16 (one 16-byte load) when a slot holds whole
// units of 8, else 4 (C % 4 == 0: a unit never straddles two slots)
__host__ __device__ inline int unit_width(bool half, long E) { return half && E % 8 == 0 ? 8 : 4; }
__host__ __device__ inline long tensor_chunks(int slots, long E, int W) {
  return ((long)slots * E / W + chunk_units - 1) / chunk_units;
}
// s0 holds bf16 only for a co-st-gcn batch in bf16: the rt-st-gcn state is fp32 in both of its dtypes
__host__ __device__ inline bool s0_half(const desc_t& d) { return d.kind == STGCN_STREAM_STATE_CO && d.dtype == 1; }

__host__ __device__ inline long stream_chunks(const desc_t& d) {
  long n = 0;
  for (int l = 0; l < d.L; ++l) {
    const long E = (long)d.V * d.layers[l].C;
    n += tensor_chunks(d.layers[l].n0, E, unit_width(s0_half(d), E)) + tensor_chunks(d.layers[l].n1, E, 4);
  }
  return n;
}

DEV int wrap(int i, int n) {  // an index read from device memory, into [0, n)
  i %= n;
  return i < 0 ? i + n : i;
}

template <int W>
struct Unit {
  float v[W];
};
template <typename T, int W>
DEV Unit<W> load_unit(const T* p) {
  Unit<W> u;
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int i = 0; i < W; i += 4) load4(p + i, u.v + i);
  } else if constexpr (W == 8) {
    const bf16x8 q = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) u.v[i] = (float)q[i];
  } else {
    const bf16x4 q = *reinterpret_cast<const bf16x4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) u.v[i] = (float)q[i];
  }
  return u;
}
template <typename T, int W>
DEV void store_unit(T* p, const Unit<W>& u) {
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int i = 0; i < W; i += 4) store4(p + i, make_float4(u.v[i], u.v[i + 1], u.v[i + 2], u.v[i + 3]));
  } else if constexpr (W == 8) {
    bf16x8 q;
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i] = (bf16)u.v[i];  // nearest even
    *reinterpret_cast<bf16x8*>(p) = q;
  } else {
    store4(p, make_float4(u.v[0], u.v[1], u.v[2], u.v[3]));
  }
}

// One chunk of one state tensor of one stream.  st: the stream's [slots][E] elements of T; img: its image, fp32.
// Export: img[k * E + e] = st[(head + k) % slots][e]; import: st[k * E + e] = (T)img[k * E + e].
template <typename T, int W, bool IMPORT>
DEV void copy_chunk(T* st, float* img, int slots, long E, int head, long chunk) {
  const long units = (long)slots * E / W;
  Unit<W> u[U];
  long at[U];
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const long i = chunk * chunk_units + (long)j * NT + threadIdx.x;
    at[j] = i < units ? i * W : -1;
    if (at[j] < 0) continue;
    if constexpr (IMPORT) {
      u[j] = load_unit<float, W>(img + at[j]);
    } else {
      const int k = (int)(at[j] / E);
      int slot = head + k;  // head < slots, k < slots
      if (slot >= slots) slot -= slots;
      u[j] = load_unit<T, W>(st + (long)slot * E + (at[j] - (long)k * E));
    }
  }
#pragma unroll
  for (int j = 0; j < U; ++j) {
    if (at[j] < 0) continue;
    if constexpr (IMPORT) store_unit<T, W>(st + at[j], u[j]);
    else store_unit<float, W>(img + at[j], u[j]);
  }
}

template <typename T, bool IMPORT>
__global__ __launch_bounds__(NT) void stream_state_kernel(const desc_t d, const long per_stream) {
  const long i = blockIdx.x / per_stream;
  long c = blockIdx.x - i * per_stream;
  const int slot = d.slots[i];
  if (slot < 0 || slot >= d.B) return;  // uniform over the workgroup: nothing is touched
  // (layer, tensor, chunk within the tensor) of flat chunk c
  int l = 0, which = 0;
  long E = 0;
  for (; l < d.L; ++l) {
    E = (long)d.V * d.layers[l].C;
    const long c0 = tensor_chunks(d.layers[l].n0, E, unit_width(sizeof(T) == 2, E));
    if (c < c0) break;
    c -= c0;
    const long c1 = tensor_chunks(d.layers[l].n1, E, 4);
    if (c < c1) {
      which = 1;
      break;
    }
    c -= c1;
  }
  if (l >= d.L) return;
  const layer_t ly = d.layers[l];
  int* idx = ly.idx + (long)slot * 2;
  float* img = d.snap + i * d.E + (which ? ly.off1 : ly.off0);
  const int slots = which ? ly.n1 : ly.n0;
  const int head = IMPORT ? 0 : wrap(idx[which], slots);
  if (IMPORT && c == 0 && threadIdx.x == 0) idx[which] = 0;
  if (which) {
    copy_chunk<float, 4, IMPORT>(ly.s1 + (long)slot * slots * E, img, slots, E, head, c);
  } else {
    T* st = reinterpret_cast<T*>(ly.s0) + (long)slot * slots * E;
    if (unit_width(sizeof(T) == 2, E) == 8) copy_chunk<T, 8, IMPORT>(st, img, slots, E, head, c);
    else copy_chunk<T, 4, IMPORT>(st, img, slots, E, head, c);
  }
}

template <bool IMPORT>
int launch(const desc_t& d, hipStream_t s) {
  const long per = stream_chunks(d);
  const dim3 grid((unsigned)(per * d.n));
  if (s0_half(d)) hipLaunchKernelGGL((stream_state_kernel<bf16, IMPORT>), grid, dim3(NT), 0, s, d, per);
  else hipLaunchKernelGGL((stream_state_kernel<float, IMPORT>), grid, dim3(NT), 0, s, d, per);
  return hipGetLastError() == hipSuccess ? STGCN_OK : STGCN_EHIP;
}

}  // namespace

// 0 when the descriptor's shapes, offsets, kind, dtype and pointers are usable
int stream_state_check(const stgcn_stream_state_desc& d) {
  if (d.L < 1 || d.L > STGCN_RT_MAX_LAYERS || d.V < 2 || d.V > VMAX || d.B < 1 || d.n < 1) return STGCN_EBADSHAPE;
  if (d.kind != STGCN_STREAM_STATE_RT && d.kind != STGCN_STREAM_STATE_CO) return STGCN_EBADSHAPE;
  long at = 0;
  for (int l = 0; l < d.L; ++l) {
    const stgcn_stream_state_layer& y = d.layers[l];
    if (y.C < 4 || y.C % 4 || y.n0 < 1 || y.n1 < 1) return STGCN_EBADSHAPE;
    const long E = (long)d.V * y.C;
    if (y.off0 != at) return STGCN_EBADSHAPE;  // the image is dense, layer-major, s0 before s1
    at += y.n0 * E;
    if (y.off1 != at) return STGCN_EBADSHAPE;
    at += y.n1 * E;
  }
  if (d.E != at) return STGCN_EBADSHAPE;
  if (d.dtype != 0 && d.dtype != 1) return STGCN_EDTYPE;
  if (stream_chunks(d) * d.n > 0x7fffffffL) return STGCN_EBADSHAPE;  // blockIdx.x: (stream, chunk)
  if (!d.slots || !d.snap) return STGCN_EBADSHAPE;
  for (int l = 0; l < d.L; ++l)
    if (!d.layers[l].s0 || !d.layers[l].s1 || !d.layers[l].idx) return STGCN_EBADSHAPE;
  return STGCN_OK;
}

int stream_state_export_launch(const stgcn_stream_state_desc& d, hipStream_t s) { return launch<false>(d, s); }
int stream_state_import_launch(const stgcn_stream_state_desc& d, hipStream_t s) { return launch<true>(d, s); }
