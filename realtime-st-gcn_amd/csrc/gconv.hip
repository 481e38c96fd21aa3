// Graph convolution of ST-GCN (ConvTemporalGraphical, models/utils/tgcn.py:58-79) as a
// joint-gathered GEMM, for a graph shared by the batch.
//
// The reference computes  y = conv1x1(x) (P*Cout channels) ; g = einsum('nkctv,kvw->nctw', y, A).
// Writing W_p = conv weight rows [p*Cout, (p+1)*Cout) and S(w) = {v : A_p[v][w] != 0 for some p}
// (the joints feeding output joint w; <= 5 for the skeleton graphs), the same thing is
//
//   g[(i,w)][co] = sum_{j < |S(w)|} sum_ci x[(i, S(w)_j)][ci] * Weff[w][j][co][ci] + bias2d[w][co]
//   Weff[w][j][co][ci] = sum_p A_p[S(w)_j][w] * W_p[co][ci]            (i = n*T + t)
//
// i.e. for every output joint w a GEMM over the frame rows i whose K axis gathers the |S(w)|
// neighbour rows of the same frame.  Total MFMA work = sum_w |S(w)| * Cin * Cout per frame
// (73 * Cin * Cout for the 25-joint graphs, vs P*V = 75 for the A-first form) and no A-mixed
// intermediate ever touches HBM: the old path wrote and re-read an M x P*Cin tensor three times
// (forward, data grad, weight grad).  The data gradient is the same kernel on dg with the
// transposed effective weights  WeffT[v][j][ci][co] = sum_p A_p[v][R(v)_j] W_p[co][ci]  over the
// reverse lists R(v) = {w : v in S(w)}; the weight/adjacency gradients come from
//   dWeff[w][j][co][ci] = sum_i dg[(i,w)][co] * x[(i, S(w)_j)][ci]          (gconv_wgrad)
//   dW_p[co][ci] = sum_{w,j} A_p[S(w)_j][w] dWeff[w][j][co][ci],
//   dA_p[S(w)_j][w] = sum_{co,ci} W_p[co][ci] dWeff[w][j][co][ci]            (gconv_wgrad_finish)
//
// Kernel layout follows conv_tile.hip (flat mode): block = (row tile of BM frames, joint a, column
// tile); A rows staged through registers into padded LDS rows, B (packed Weff) by LDS-DMA with the
// XOR swizzle on the source, fragment double-buffering, BN partial statistics in the epilogue.
//
// This file holds the gather GEMM (forward and data gradient) and the effective-weight pack; the weight
// gradient dWeff and its slab reductions are in gconv_wgrad.hip, the dW / dA / db finish in gconv_finish.hip.
#include "common.h"
#include "lds_ops.h"
#include "pack.h"
#include "launchers.h"
#include "../../include/stgcn_amd.h"

namespace {

// DMA K loop: LDS stages of the ring at Cout <= 64 (N), at Cin < 256 (M) and at Cin >= 256 (W); these and the two
// TM below were A/B build flags, settled at these values
constexpr int GCONV_NSTG_N = 2, GCONV_NSTG_M = 2, GCONV_NSTG_W = 2;
// row tiles of the wide DMA forms: BM = 4 * TM * 32 rows; a taller tile re-reads each joint's effective weights
// (deg x 64-channel chunks x 128 columns) fewer times per launch
constexpr int GCONV_TM_W = 2, GCONV_TM_M = 1;

template <typename T, int KC>
struct GL {
  static constexpr int RB = KC * (int)sizeof(T);
  static constexpr int UPR = RB / 16;
  static constexpr int RPB = RB >= 256 ? 1 : 256 / RB;
  static constexpr int RS = RB + 16;
  static DEV int swz(int row) { return (row / RPB) & (UPR - 1); }
};

// s_waitcnt vmcnt(n) for the counts the DMA K loop uses (n = steps in flight x instructions per step)
DEV void gwait_vm(int n) {
  switch (n) {
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
    case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}

struct GGeom {
  int ntile;  // row tiles
  int ncol;   // column tiles
  int nblk;
};

// ------------------------------------------------------------------ gather GEMM (fwd and data grad)
// ACCV: stores (and accumulate, out +=) through the vectorised LDS-scratch epilogue; a separate instantiation so
// the plain-store kernel keeps its register budget (<= 128 VGPRs: 2 blocks per CU)
// NSTG > 0 (bf16, KC = 64): the K loop DMAs both operands (gathered x rows and the effective weights,
// XOR-swizzled 128-B rows) into an NSTG-deep LDS ring, NSTG - 1 K steps ahead, with counted vmcnt waits
// (every wave issues the same number of DMA instructions per step) and one LDS-only barrier per step;
// NSTG = 0: rows staged through registers, double-buffered.
template <typename T, int WM, int WN, int TM, int TN, int KC, bool ACCV, int NSTG = 0>
__global__ __launch_bounds__(WM * WN * 64, (NSTG && (WM * TM + WN * TN) * 32 * 128 * NSTG > 80 * 1024) ? 1 : 2) void gconv_kernel(const stgcn_gconv_desc a, const GGeom g) {
  typedef GL<T, KC> L;
  constexpr int NW = WM * WN, NT = NW * 64;
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  constexpr int VEC = 16 / (int)sizeof(T);
  constexpr int KS = KC / 16;
  constexpr int A_UNITS = BM * L::UPR / NT;
  constexpr int A_BYTES = BM * L::RS;
  constexpr int B_BYTES = BN * L::RB;
  constexpr int B_PIECES = (B_BYTES + 1023) / 1024;
  constexpr int STAGE = ((A_BYTES + B_BYTES) + 1023) & ~1023;
  static_assert(BM * L::UPR % NT == 0, "A units");
  static_assert(B_BYTES % 1024 == 0, "B pieces");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int lr = lane & 31, lh = lane >> 5;
  const int V = a.V;

  // XCD-aware order: consecutive ids (column tile fastest, then joint) share the row tile's x rows
  int wg;
  {
    const int id = blockIdx.x, x = id & 7, q = g.nblk >> 3, r = g.nblk & 7;
    wg = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (id >> 3);
  }
  const int ct = wg % g.ncol;
  const int jt = (wg / g.ncol) % V;  // output joint
  const int it = wg / (g.ncol * V);
  const int n0 = ct * BN;
  const int i0 = it * BM;
  const int rows_valid = min(BM, a.NT - i0);
  const int deg = a.deg[jt];

  const T* __restrict__ in = reinterpret_cast<const T*>(a.in);
  const T* __restrict__ wp = reinterpret_cast<const T*>(a.w);
  const int ucol = tid % L::UPR;
  long a_row[A_UNITS];  // element offset of frame row (i, joint 0) ; -1 = zero row
  int a_lds[A_UNITS];
#pragma unroll
  for (int u = 0; u < A_UNITS; ++u) {
    const int row = (tid + u * NT) / L::UPR;
    a_lds[u] = row * L::RS + ucol * 16;
    a_row[u] = row < rows_valid ? (long)(i0 + row) * V * a.in_ld + ucol * VEC : -1;
  }
  const bool fast_ld = (a.in_ld % VEC) == 0 && (a.Cin % KC) == 0;

  int a_off[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) a_off[i] = ((wm * TM + i) * 32 + lr) * L::RS + lh * 16 * (int)(sizeof(T) / 2);
  int b_off[KS][2];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int f = L::swz(lr);
    if constexpr (sizeof(T) == 2) {
      b_off[ks][0] = lr * L::RB + (((2 * ks + lh) ^ f) << 4);
      b_off[ks][1] = b_off[ks][0];
    } else {
      b_off[ks][0] = lr * L::RB + (((4 * ks + 2 * lh) ^ f) << 4);
      b_off[ks][1] = lr * L::RB + (((4 * ks + 2 * lh + 1) ^ f) << 4);
    }
  }

  const int nch = a.Cin_pad / KC;
  const int nk = deg * nch;  // K chunks: (neighbour j, channel chunk c)
  uint4 ra[A_UNITS];

  auto load = [&](int k, int buf) {
    const int j = k / nch, c = k - j * nch;
    const int src = a.nbr[jt * a.J + j];
    const long joff = (long)src * a.in_ld + c * KC;
    const int ci = c * KC + ucol * VEC;
#pragma unroll
    for (int u = 0; u < A_UNITS; ++u) {
      ra[u] = make_uint4(0, 0, 0, 0);
      if (a_row[u] >= 0) {
        const T* p = in + a_row[u] + joff;
        if (fast_ld) {
          ra[u] = *reinterpret_cast<const uint4*>(p);
        } else if (ci < a.Cin) {
          float f[VEC];
#pragma unroll
          for (int e = 0; e < VEC; ++e) f[e] = ci + e < a.Cin ? Tr<T>::to_f(p[e]) : 0.f;
          ra[u] = pack16(f, (T*)nullptr);
        }
      }
    }
    char* B_ = smem + buf * STAGE + A_BYTES;
    const T* wsrc = wp + ((long)(jt * a.J + j) * a.Cout_pad + n0) * a.Cin_pad + c * KC;
#pragma unroll
    for (int kk = 0; kk < (B_PIECES + NW - 1) / NW; ++kk) {
      const int piece = wave + kk * NW;
      if (piece < B_PIECES) {
        const int byte = piece * 1024 + lane * 16;
        const int br = byte / L::RB, pu = (byte % L::RB) >> 4;
        glds16(wsrc + (long)br * a.Cin_pad + (pu ^ L::swz(br)) * VEC, B_ + piece * 1024);
      }
    }
  };
  auto store = [&](int buf) {
    char* A_ = smem + buf * STAGE;
#pragma unroll
    for (int u = 0; u < A_UNITS; ++u) *reinterpret_cast<uint4*>(A_ + a_lds[u]) = ra[u];
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  typedef typename Tr<T>::frag Frag;
  if constexpr (NSTG > 0) {
    static_assert(sizeof(T) == 2 && KC == 64, "DMA K loop: bf16, 64-channel chunks");
    constexpr int RBD = 128, A_B = BM * RBD, STG = A_B + BN * RBD;
    constexpr int AI = BM / 8 / NW, BI = BN / 8 / NW, OPS = AI + BI;  // DMA instructions per wave and step
    static_assert(BM % (8 * NW) == 0 && BN % (8 * NW) == 0, "DMA rows");
    int* const snbr = reinterpret_cast<int*>(smem + NSTG * STG);  // this joint's neighbour list
    if (tid < a.J) snbr[tid] = a.nbr[jt * a.J + tid];
    __syncthreads();
    // lane -> (row rr of the instruction's 8 rows, 16-B slot); the slot holds unit slot ^ swz(row)
    const int rr = lane >> 3, slot = lane & 7;
    long a_src[AI];
    int b_src[BI];
#pragma unroll
    for (int q = 0; q < AI; ++q) {
      const int r = (wave * AI + q) * 8 + rr;
      const int rc = min(r, max(rows_valid, 1) - 1);  // rows past the tile's end read a valid row (discarded)
      a_src[q] = (long)(i0 + rc) * V * a.in_ld + (slot ^ ((r >> 1) & 7)) * 8;
    }
#pragma unroll
    for (int q = 0; q < BI; ++q) {
      const int r = (wave * BI + q) * 8 + rr;
      b_src[q] = (n0 + r) * a.Cin_pad + (slot ^ ((r >> 1) & 7)) * 8;
    }
    auto issue = [&](int k, int stage) {
      const int j = k / nch, c = k - j * nch;
      const long joff = (long)snbr[j] * a.in_ld + c * KC;
      const T* wsrc = wp + (long)(jt * a.J + j) * a.Cout_pad * a.Cin_pad + c * KC;
      char* base = smem + stage * STG;
#pragma unroll
      for (int q = 0; q < AI; ++q) glds16(in + a_src[q] + joff, lds_u32(base + (wave * AI + q) * 1024));
#pragma unroll
      for (int q = 0; q < BI; ++q) glds16(wsrc + b_src[q], lds_u32(base + A_B + (wave * BI + q) * 1024));
    };
#pragma unroll
    for (int sidx = 0; sidx < NSTG - 1; ++sidx)
      if (sidx < nk) issue(sidx, sidx);
    for (int k = 0; k < nk; ++k) {
      const int younger = min(NSTG - 2, nk - 1 - k);  // own DMA steps allowed to stay in flight
      gwait_vm(younger * OPS);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // every wave's DMAs of step k landed
      if (k + NSTG - 1 < nk) issue(k + NSTG - 1, (k + NSTG - 1) % NSTG);  // that stage was read in step k-1
      const char* A_ = smem + (k % NSTG) * STG;
      const char* B_ = A_ + A_B;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        Frag fa[TM], fb[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int r = (wm * TM + i) * 32 + lr;
          fa[i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(A_ + r * RBD + (((2 * ks + lh) ^ ((r >> 1) & 7)) << 4)));
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int r = (wn * TN + j) * 32 + lr;
          fb[j] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(B_ + r * RBD + (((2 * ks + lh) ^ ((r >> 1) & 7)) << 4)));
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) Tr<T>::mma(acc[i][j], fa[i], fb[j]);
      }
    }
    __syncthreads();  // every wave is done with the ring before the epilogue reuses it
  } else {
  int cur = 0;
  if (nk > 0) {
    load(0, 0);
    store(0);
  }
  __syncthreads();
  for (int k = 0; k < nk; ++k) {
    const bool more = k + 1 < nk;
    if (more) load(k + 1, cur ^ 1);
    const char* A_ = smem + cur * STAGE;
    const char* B_ = A_ + A_BYTES;
    Frag fa[2][TM], fb[2][TN];
    auto rd = [&](int ks, int b) {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const char* p = A_ + a_off[i] + ks * 16 * (int)sizeof(T);
        fa[b][i] = frag2<T>(p, p + 16);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const char* p = B_ + ((wn * TN + j) * 32) * L::RB;
        fb[b][j] = frag2<T>(p + b_off[ks][0], p + b_off[ks][1]);
      }
    };
    rd(0, 0);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if (ks + 1 < KS) rd(ks + 1, (ks + 1) & 1);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) Tr<T>::mma(acc[i][j], fa[ks & 1][i], fb[ks & 1][j]);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (more) store(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }
  }  // NSTG == 0

  // ---------------------------------------------------------------- epilogue
  // bias + BN partials on the fp32 accumulators.  accumulate: the values go through a per-wave LDS
  // scratch (one 32x32 tile at a time) so that every lane read-modify-writes 16-B units of an output
  // row instead of scattered 2/4-byte elements (a dependent load per element before its store).  The main loop's last barrier
  // retired every read of the stage buffers, which the scratch reuses.
  T* __restrict__ out = reinterpret_cast<T*>(a.out);
  const long ldv = (long)a.out_ld * V;  // row stride between consecutive frames of joint jt
  constexpr int SROW = 32 * (int)sizeof(T) + 16;  // padded scratch row (bytes)
  constexpr int UR = 32 * (int)sizeof(T) / 16;     // 16-B units per 32-column row
  char* scratch = smem + wave * 32 * SROW;
  constexpr bool vec_out = ACCV;  // launcher: ACCV when rows are 16-B aligned
  Welford ws[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int c0 = n0 + (wn * TN + j) * 32;
    const int col = c0 + lr;
    const bool cok = col < a.Cout;
    const float b1 = (a.bias && cok) ? a.bias[jt * a.Cout + col] : 0.f;
    float s = 0.f, cnt = 0.f;
    if constexpr (!vec_out) {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int lb = (wm * TM + i) * 32 + 4 * lh;
        T* pb = out + ((long)(i0 + lb) * V + jt) * a.out_ld + col;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ro = (r & 3) + 8 * (r >> 2);
          const bool ok = cok && lb + ro < rows_valid;
          float v = acc[i][j][r] + b1;
          if (ok) {
            T* p = pb + ro * ldv;
            if (a.accumulate) v += Tr<T>::to_f(*p);
            *p = Tr<T>::from_f(v);
            s += v;
            cnt += 1.f;
          }
          acc[i][j][r] = v;
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int rb = (wm * TM + i) * 32;  // tile's first row (frame index within the row tile)
        const int lb = rb + 4 * lh;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ro = (r & 3) + 8 * (r >> 2);
          const float v = acc[i][j][r] + b1;
          acc[i][j][r] = v;
          if (cok && lb + ro < rows_valid) {
            s += v;
            cnt += 1.f;
          }
          *reinterpret_cast<T*>(scratch + (4 * lh + ro) * SROW + lr * (int)sizeof(T)) = Tr<T>::from_f(v);
        }
        // 32 rows x UR units, lane -> (row, unit): 16-B read-modify-write of the output (wave-private
        // scratch: no block barrier needed)
#pragma unroll
        for (int q = 0; q < 32 * UR / 64; ++q) {
          const int idx = q * 64 + lane, row = idx / UR, u = idx % UR;
          if (rb + row < rows_valid && c0 + u * VEC < a.Cout) {
            T* p = out + ((long)(i0 + rb + row) * V + jt) * a.out_ld + c0 + u * VEC;
            float f[VEC], o[VEC];
            if (a.accumulate) {
              unpack16(*reinterpret_cast<const uint4*>(scratch + row * SROW + u * 16), f, (T*)nullptr);
              unpack16(*reinterpret_cast<const uint4*>(p), o, (T*)nullptr);
#pragma unroll
              for (int e = 0; e < VEC; ++e) f[e] += o[e];
              *reinterpret_cast<uint4*>(p) = pack16(f, (T*)nullptr);
            } else if (sizeof(T) == 2 && a.res) {  // masked residual (launcher: bf16, VEC = 8 = one mask byte)
              const long grow = (long)(i0 + rb + row) * V + jt;
              const int cc = c0 + u * VEC;
              unpack16(*reinterpret_cast<const uint4*>(scratch + row * SROW + u * 16), f, (T*)nullptr);
              unpack16(*reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(a.res) + grow * a.res_ld + cc), o,
                       (T*)nullptr);
              const unsigned mb = reinterpret_cast<const unsigned char*>(a.res_bits)[grow * (a.Cout / 8) + cc / 8];
#pragma unroll
              for (int e = 0; e < VEC; ++e) f[e] += ((mb >> e) & 1u) ? o[e] : 0.f;
              *reinterpret_cast<uint4*>(p) = pack16(f, (T*)nullptr);
            } else {
              *reinterpret_cast<uint4*>(p) = *reinterpret_cast<const uint4*>(scratch + row * SROW + u * 16);
            }
          }
        }
      }
    }
    Welford w;
    w.n = cnt;
    w.mean = cnt > 0.f ? s / cnt : 0.f;
    float m2 = 0.f;
    if (a.stats) {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int lb = (wm * TM + i) * 32 + 4 * lh;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float d = acc[i][j][r] - w.mean;
          if (cok && lb + (r & 3) + 8 * (r >> 2) < rows_valid) m2 += d * d;
        }
      }
    }
    w.m2 = m2;
    ws[j] = w;
  }
  if (a.stats) {
    __syncthreads();
    float4* red = reinterpret_cast<float4*>(smem);  // [WM][BN]
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      Welford o;
      o.n = __shfl_xor(ws[j].n, 32);
      o.mean = __shfl_xor(ws[j].mean, 32);
      o.m2 = __shfl_xor(ws[j].m2, 32);
      const Welford w = welford_merge(ws[j], o);
      if (lh == 0) red[wm * BN + (wn * TN + j) * 32 + lr] = make_float4(w.n, w.mean, w.m2, 0.f);
    }
    __syncthreads();
    for (int c = tid; c < BN; c += NT) {
      const float4 f = red[c];
      Welford w = {f.x, f.y, f.z};
      for (int k = 1; k < WM; ++k) {
        const float4 h = red[k * BN + c];
        w = welford_merge(w, Welford{h.x, h.y, h.z});
      }
      if (n0 + c < a.Cout_pad)
        reinterpret_cast<float4*>(a.stats)[((long)it * V + jt) * a.Cout_pad + n0 + c] =
            make_float4(w.n, w.mean, w.m2, 0.f);
    }
  }
}

template <typename T, int WM, int WN, int TM, int TN, int KC, int NSTG = 0>
int launch_gconv(const stgcn_gconv_desc& a, hipStream_t s) {
  constexpr int VEC = 16 / (int)sizeof(T);
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  typedef GL<T, KC> L;
  if (a.Cout_pad % BN || a.Cin_pad % KC) return STGCN_EBADSHAPE;
  if (NSTG && (a.in_ld % VEC || a.Cin != a.Cin_pad || a.J > 64)) return STGCN_EBADSHAPE;
  GGeom g;
  g.ntile = (a.NT + BM - 1) / BM;
  g.ncol = a.Cout_pad / BN;
  const long nblk = (long)g.ntile * a.V * g.ncol;
  if (nblk <= 0 || nblk > 0x7fffffffL) return STGCN_EBADSHAPE;
  g.nblk = (int)nblk;
  const int STAGE = ((BM * L::RS + BN * L::RB) + 1023) & ~1023;
  size_t lds = NSTG ? (size_t)NSTG * (BM + BN) * 128 + 256 : 2 * (size_t)STAGE;
  const size_t red = a.stats ? (size_t)WM * BN * 16 : 0;
  if (red > lds) lds = red;
  if (stgcn_lds_attr((const void*)gconv_kernel<T, WM, WN, TM, TN, KC, false, NSTG>, 160 * 1024, s) ||
      stgcn_lds_attr((const void*)gconv_kernel<T, WM, WN, TM, TN, KC, true, NSTG>, 160 * 1024, s))
    return STGCN_EHIP;
  // 16-B row stores through the LDS scratch whenever rows are 16-B aligned (per-element stores otherwise)
  const bool accv = (a.out_ld % VEC) == 0 && (a.Cout % VEC) == 0;
  if (a.res && (!accv || sizeof(T) != 2 || a.accumulate || !a.res_bits || a.Cout % 8 || a.res_ld % 8))
    return STGCN_EBADSHAPE;  // the masked residual rides on the 16-B bf16 epilogue only
  if (accv)
    hipLaunchKernelGGL((gconv_kernel<T, WM, WN, TM, TN, KC, true, NSTG>), dim3((unsigned)nblk), dim3(WM * WN * 64),
                       lds, s, a, g);
  else
    hipLaunchKernelGGL((gconv_kernel<T, WM, WN, TM, TN, KC, false, NSTG>), dim3((unsigned)nblk), dim3(WM * WN * 64),
                       lds, s, a, g);
  return hipGetLastError() == hipSuccess ? STGCN_OK : STGCN_EHIP;
}

// ------------------------------------------------------------------ effective weights (pack.h)
template <typename T>
__global__ void gconv_weights_kernel(const float* __restrict__ A, const float* __restrict__ W, const int* nbr,
                                     const int* deg, int P, int V, int J, int Cout, int Cin, int trans, T* out,
                                     int R_pad, int C_pad, const float* __restrict__ bconv, float* __restrict__ bias2d) {
  __shared__ float colsum[GW_COLSUM_MAX];
  if (bias2d) gconv_colsum_block(A, nullptr, P, V, colsum);  // block-uniform
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < (long)V * R_pad * (C_pad / 8))
    gconv_weights_elem<T>(A, nullptr, W, nbr, deg, P, V, J, Cout, Cin, trans, out, R_pad, C_pad, bconv, bias2d, colsum,
                          idx);
}

}  // namespace

long gconv_row_blocks(int NT, int V) { return (long)((NT + 127) / 128) * V; }

int gconv_launch(const stgcn_gconv_desc& a, int dtype, hipStream_t s) {
  // column tile: 64 for Cout <= 64, else 128 (weights padded accordingly by stgcn_gconv_weights)
  const bool wide = a.Cout > 64;
  // bf16, Cout <= 64: 128-row tiles (TM = 1, TN = 2) — twice the blocks of the 256-row tile, measured
  // 46 vs 54 us (C=64 fwd), 42 vs 47 us (dgrad), 68 vs 72 us (128 -> 64 dgrad); wider outputs keep
  // 256 x 128 tiles (128-row variants measured 5-10 % slower there)
  // K chunk of 64 channels (one barrier per 64 instead of 32) once Cin >= 128, with 128-row tiles at the
  // wide outputs (tools/bench_conv.py gconv, us, 32-chunk -> 64-chunk: fwd C=128 63 -> 56.5, C=256 96.5 ->
  // 92; dgrad 128 -> 64 67 -> 55; at Cin = 64 the 32-chunk tiles stay ahead or even)
  if (dtype == 1) {
    // DMA K loop (two LDS stages, 64-channel chunks) whenever rows allow it: tools/bench_conv.py gconv, us,
    // register-staged -> DMA: C=64 fwd 44.7 -> 42.7, dgrad 40.7 -> 36.6; C=128 59.8 -> 56.0 / 51.8 -> 48.9;
    // 64->128 69.8 -> 67.2 / 58.2 -> 49.8; C=256 (256-row tiles) 95.7 -> 85.2 / 88.1 -> 75.2
    const bool dma = a.Cin % 64 == 0 && a.Cin == a.Cin_pad && a.in_ld % 8 == 0;
    if (dma) {
      if (!wide) return launch_gconv<bf16, 4, 1, 1, 2, 64, GCONV_NSTG_N>(a, s);
      return a.Cin >= 256 ? launch_gconv<bf16, 4, 2, GCONV_TM_W, 2, 64, GCONV_NSTG_W>(a, s)
                          : launch_gconv<bf16, 4, 2, GCONV_TM_M, 2, 64, GCONV_NSTG_M>(a, s);
    }
    const bool k64 = a.Cin >= 128 && a.Cin_pad % 64 == 0;
    if (wide) return k64 ? launch_gconv<bf16, 4, 2, 1, 2, 64>(a, s) : launch_gconv<bf16, 4, 2, 2, 2, 32>(a, s);
    return k64 ? launch_gconv<bf16, 4, 1, 1, 2, 64>(a, s) : launch_gconv<bf16, 4, 1, 1, 2, 32>(a, s);
  }
  return wide ? launch_gconv<float, 4, 2, 2, 2, 16>(a, s) : launch_gconv<float, 4, 1, 2, 2, 16>(a, s);
}

int gconv_weights_launch(const float* A, const float* W, const int* nbr, const int* deg, int P, int V, int J, int Cout,
                         int Cin, int trans, void* out, int R_pad, int C_pad, int dtype, hipStream_t s,
                         const float* bconv, float* bias2d) {
  if (C_pad % 8 || P > GW_PMAX || (bconv && P * V > GW_COLSUM_MAX)) return STGCN_EBADSHAPE;
  const long total = (long)V * R_pad * (C_pad / 8);
  const unsigned blocks = (unsigned)((total + 255) / 256);
  if (dtype == 1)
    hipLaunchKernelGGL(gconv_weights_kernel<bf16>, dim3(blocks), dim3(256), 0, s, A, W, nbr, deg, P, V, J, Cout, Cin,
                       trans, (bf16*)out, R_pad, C_pad, bconv, bias2d);
  else
    hipLaunchKernelGGL(gconv_weights_kernel<float>, dim3(blocks), dim3(256), 0, s, A, W, nbr, deg, P, V, J, Cout,
                       Cin, trans, (float*)out, R_pad, C_pad, bconv, bias2d);
  return hipGetLastError() == hipSuccess ? STGCN_OK : STGCN_EHIP;
}
