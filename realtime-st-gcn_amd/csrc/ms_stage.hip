// MS-TCN stage (models/mstcn/mstcn.py:68-116): conv_in 1x1, num_layers dilated residual layers, conv_out 1x1,
// forward and backward, on rows [L][V][F] (row r = t*V + v, F channels contiguous).  A layer with dilation d is
//   h = ReLU(b1 + sum_k W1_k x[r + (k-1) d V]),   y = x + b2 + W2 h          (mstcn.py:108-116, kernel 3)
// and a tap whose row falls outside [0, L V) is zero: with this row order that is exactly the time padding.
// The residual stream x / y and every gradient of it stay fp32 in HBM; MFMA operands are rounded to the compute
// type T (fp32 | bf16) while they are staged, accumulation is fp32; the saved hidden activation h and its gradient
// g are T.  Every hand-off is a kernel boundary, there are no atomics, and every reduction runs in a fixed order.
//
//   ms_pack      : W1 (F,F,3), W2 (F,F) -> four [tile][k-step][lane][8] MFMA B images (co_frame.hip's layout):
//                  W1 tap-major (K = 3F), W2 (K = F), and their transposes for the data gradient
//   ms_layer_fwd : a workgroup owns 128 rows, a wave 32 of them.  A fragments of the tile and of its two dilated
//                  neighbour tiles come from x, the K = 3F tap GEMM runs on 32x32 MFMAs, + b1, ReLU; the hidden tile
//                  goes through LDS (accumulator layout -> A layout) into the K = F GEMM; + b2 + x; h saved in training
//   ms_layer_g   : g = (W2^T dy) . [h > 0]
//   ms_layer_dx  : dx = dy + sum_k W1_k^T g[r - (k-1) d V]    (the forward tap GEMM with the shift negated)
//   ms_layer_wgrad : split-M partials per workgroup: wave k < 3 forms dW1_k = sum_r g[r] (x) x[r + (k-1) d V],
//                  wave 3 dW2 = sum_r dy[r] (x) h[r] (rows are the MFMA k axis); waves 1 and 3 also sum db1 / db2
//   ms_reduce    : grads[e] = sum_b partial[b][e], b ascending
//   ms_lin_fwd / ms_lin_bwd : the small-width ends of a stage in plain FMA code.  conv_in with the `refine` prologue
//                  (none | log-softmax | softmax over the Cin values of a row) fused, and conv_out with the mean over
//                  the V joints fused in front of it (the mean commutes with the 1x1 convolution); the backward
//                  gives per-workgroup dW / db partials (ms_reduce sums them) and the input gradient through the
//                  prologue's Jacobian, or broadcast over the joints
//   ms_prob      : the model's `out` selector (log-softmax | softmax over the classes) and its backward
#include "common.h"
#include "launchers.h"
#include "../../include/stgcn_amd.h"

namespace {

constexpr int NT = 256;
constexpr int TM = 128;       // rows per workgroup of the layer kernels: 4 waves x 32
constexpr int FMIN = 16;
constexpr int FMAX = 64;
constexpr int HS = FMAX + 8;  // LDS row stride of the hidden tile (elements; keeps 16-B alignment)
constexpr int WG_MAX = 256;   // most wgrad workgroups
constexpr int LR = 32;        // rows per chunk of the lin kernels
constexpr int CM = 64;        // most channels on either side of a lin kernel
constexpr int LIN_MAX = 128;  // most lin-backward workgroups
constexpr int LACC = (CM * CM + CM + NT - 1) / NT;  // dW + db elements per thread there

DEV void load8(const float* p, float* f) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  f[0] = a.x, f[1] = a.y, f[2] = a.z, f[3] = a.w, f[4] = b.x, f[5] = b.y, f[6] = b.z, f[7] = b.w;
}
DEV void load8(const bf16* p, float* f) {
  const bf16x8 v = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = (float)v[j];
}
// 8 values -> an MFMA fragment of T (the rounding to the compute type)
template <typename T> DEV typename Tr<T>::frag make_frag(const float* f) {
  typename Tr<T>::frag a;
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = (T)f[j];
  return a;
}
template <typename T> DEV typename Tr<T>::frag load_frag(const T* p) {
  float f[8];
  load8(p, f);
  return make_frag<T>(f);
}

// acc[t] += sum over taps and channels of src[row + (tap - 1) * D][c] * B_t[kk = tap * F + c] for the column tiles
// t < ntile; taps == 1 reads the row itself.  Lane (row = lane & 31, h = lane >> 5) holds 8 consecutive channels
// of its row per k-step; F % 16 == 0, so a k-step never straddles two taps.
template <typename T, typename TI>
DEV void tap_gemm(f32x16 (&acc)[2], const TI* __restrict__ src, const T* __restrict__ wp, long row, long R, int F,
                  int taps, long D, int ntile, int lane) {
  const int h = lane >> 5, kpt = F >> 4, nks = taps * kpt;
  for (int tap = 0; tap < taps; ++tap) {
    const long rr = taps == 3 ? row + (tap - 1) * D : row;
    const bool ok = row < R && rr >= 0 && rr < R;
    for (int kc = 0; kc < kpt; ++kc) {
      float f[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = 0.f;
      if (ok) load8(src + rr * F + kc * 16 + 8 * h, f);
      const typename Tr<T>::frag a = make_frag<T>(f);
      const int ks = tap * kpt + kc;
#pragma unroll
      for (int t = 0; t < 2; ++t)
        if (t < ntile) Tr<T>::mma(acc[t], a, load_frag<T>(wp + (((long)t * nks + ks) * 64 + lane) * 8));
    }
  }
}

DEV void zero_acc(f32x16& a) {
#pragma unroll
  for (int r = 0; r < 16; ++r) a[r] = 0.f;
}

template <typename T>
__global__ __launch_bounds__(NT) void ms_layer_fwd_kernel(const float* __restrict__ x, const T* __restrict__ w1p,
                                                          const T* __restrict__ w2p, const float* __restrict__ b1,
                                                          const float* __restrict__ b2, float* __restrict__ y,
                                                          T* __restrict__ hout, long R, int F, long D) {
  __shared__ __attribute__((aligned(16))) T hs[TM / 32][32][HS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, m = lane & 31, ntile = (F + 31) >> 5;
  const long row0 = (long)blockIdx.x * TM + w * 32;
  f32x16 acc[2];
  zero_acc(acc[0]);
  zero_acc(acc[1]);
  tap_gemm<T, float>(acc, x, w1p, row0 + m, R, F, 3, D, ntile, lane);
  // columns >= F of a tile meet zero weights and no bias: they stay 0
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if (t < ntile) {
      const int col = t * 32 + m;
      const float bias = col < F ? b1[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rl = acc_row(r, lane);
        const T hv = (T)fmaxf(acc[t][r] + bias, 0.f);
        hs[w][rl][col] = hv;
        if (hout && col < F && row0 + rl < R) hout[(row0 + rl) * F + col] = hv;
      }
    }
  }
  __syncthreads();
  f32x16 acc2[2];
  zero_acc(acc2[0]);
  zero_acc(acc2[1]);
  const int kpt = F >> 4;
  for (int kc = 0; kc < kpt; ++kc) {
    const typename Tr<T>::frag a = load_frag<T>(&hs[w][m][kc * 16 + 8 * (lane >> 5)]);
#pragma unroll
    for (int t = 0; t < 2; ++t)
      if (t < ntile) Tr<T>::mma(acc2[t], a, load_frag<T>(w2p + (((long)t * kpt + kc) * 64 + lane) * 8));
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int col = t * 32 + m;
    if (t < ntile && col < F) {
      const float bias = b2[col];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long rg = row0 + acc_row(r, lane);
        if (rg < R) y[rg * F + col] = acc2[t][r] + bias + x[rg * F + col];
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(NT) void ms_layer_g_kernel(const float* __restrict__ dy, const T* __restrict__ w2tp,
                                                        const T* __restrict__ hsave, T* __restrict__ g, long R, int F) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, m = lane & 31, ntile = (F + 31) >> 5;
  const long row0 = (long)blockIdx.x * TM + w * 32;
  f32x16 acc[2];
  zero_acc(acc[0]);
  zero_acc(acc[1]);
  tap_gemm<T, float>(acc, dy, w2tp, row0 + m, R, F, 1, 0, ntile, lane);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int col = t * 32 + m;
    if (t < ntile && col < F) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long rg = row0 + acc_row(r, lane);
        if (rg < R) g[rg * F + col] = (float)hsave[rg * F + col] > 0.f ? (T)acc[t][r] : (T)0.f;
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(NT) void ms_layer_dx_kernel(const T* __restrict__ g, const T* __restrict__ w1tp,
                                                         const float* __restrict__ dy, float* __restrict__ dx, long R,
                                                         int F, long D) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, m = lane & 31, ntile = (F + 31) >> 5;
  const long row0 = (long)blockIdx.x * TM + w * 32;
  f32x16 acc[2];
  zero_acc(acc[0]);
  zero_acc(acc[1]);
  tap_gemm<T, T>(acc, g, w1tp, row0 + m, R, F, 3, -D, ntile, lane);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int col = t * 32 + m;
    if (t < ntile && col < F) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long rg = row0 + acc_row(r, lane);
        if (rg < R) dx[rg * F + col] = acc[t][r] + dy[rg * F + col];
      }
    }
  }
}

// images (see the header comment): [W1 | W2 | W1^T | W2^T]; element (tile, ks, l, j) of an image is
// B[n = 32 tile + (l & 31)][kk = 16 ks + 8 (l >> 5) + j], kk = tap * F + c, zero for n >= F
template <typename T>
__global__ __launch_bounds__(NT) void ms_pack_kernel(const float* __restrict__ w1, const float* __restrict__ w2, int F,
                                                     T* __restrict__ dst) {
  const int ntile = (F + 31) >> 5, nks1 = 3 * F / 16, nks2 = F / 16;
  const long n1 = (long)ntile * nks1 * 512, n2 = (long)ntile * nks2 * 512;
  long i = (long)blockIdx.x * NT + threadIdx.x;
  if (i >= 2 * (n1 + n2)) return;
  T* out = dst + i;
  const bool trans = i >= n1 + n2;
  if (trans) i -= n1 + n2;
  const bool second = i >= n1;
  if (second) i -= n1;
  const int nks = second ? nks2 : nks1;
  const int j = (int)(i & 7), l = (int)((i >> 3) & 63);
  const long tk = i >> 9;
  const int ks = (int)(tk % nks), tile = (int)(tk / nks);
  const int n = tile * 32 + (l & 31), kk = ks * 16 + 8 * (l >> 5) + j;
  const int tap = kk / F, c = kk - tap * F;
  float v = 0.f;
  if (n < F) {
    const int co = trans ? c : n, ci = trans ? n : c;
    v = second ? w2[co * F + ci] : w1[(co * F + ci) * 3 + tap];
  }
  *out = (T)v;
}

// acc[mt][nt] += sum_r a[r][32 mt + .] (x) b[r + shift][32 nt + .] over rows [r_begin, r_end): rows are the MFMA
// k axis, lane (m, h) reads rows r0 + 8 h + j of column 32 t + m.  bs[t]: the lane's share of the column sums of a.
template <typename T, typename TA, typename TB>
DEV void wgrad_accum(f32x16 (&acc)[2][2], float (&bs)[2], const TA* __restrict__ a, const TB* __restrict__ b,
                     long shift, long r_begin, long r_end, long R, int F, int lane) {
  const int m = lane & 31, h = lane >> 5, ntile = (F + 31) >> 5;
  for (long r0 = r_begin; r0 < r_end; r0 += 16) {
    typename Tr<T>::frag af[2], bf[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int col = t * 32 + m;
      float fa[8], fb[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const long rr = r0 + 8 * h + j, rb = rr + shift;
        const bool oka = rr < r_end && col < F;
        fa[j] = oka ? (float)a[rr * F + col] : 0.f;
        fb[j] = oka && rb >= 0 && rb < R ? (float)b[rb * F + col] : 0.f;
        bs[t] += fa[j];
      }
      af[t] = make_frag<T>(fa);
      bf[t] = make_frag<T>(fb);
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
        if (mt < ntile && nt < ntile) Tr<T>::mma(acc[mt][nt], af[mt], bf[nt]);
  }
}

// partial[b] = [dW1 (F,F,3) | db1 (F) | dW2 (F,F) | db2 (F)] of rows [b * rows_per, (b + 1) * rows_per)
template <typename T>
__global__ __launch_bounds__(NT) void ms_layer_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                            const T* __restrict__ hsave, const T* __restrict__ g,
                                                            long R, int F, long D, long rows_per,
                                                            float* __restrict__ part) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, m = lane & 31, ntile = (F + 31) >> 5;
  const long r_begin = (long)blockIdx.x * rows_per;
  const long r_end = r_begin + rows_per < R ? r_begin + rows_per : R;
  f32x16 acc[2][2];
  float bs[2] = {0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i) zero_acc(acc[i >> 1][i & 1]);
  if (w < 3) wgrad_accum<T, T, float>(acc, bs, g, x, (w - 1) * D, r_begin, r_end, R, F, lane);
  else wgrad_accum<T, float, T>(acc, bs, dy, hsave, 0, r_begin, r_end, R, F, lane);
  const int FF = F * F;
  float* P = part + (long)blockIdx.x * (4 * FF + 2 * F);
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
      if (mt < ntile && nt < ntile) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int co = mt * 32 + acc_row(r, lane), ci = nt * 32 + m;
          if (co < F && ci < F) {
            if (w < 3) P[(co * F + ci) * 3 + w] = acc[mt][nt][r];
            else P[3 * FF + F + co * F + ci] = acc[mt][nt][r];
          }
        }
      }
  if (w == 1 || w == 3) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const float s = bs[t] + __shfl_xor(bs[t], 32);
      const int col = t * 32 + m;
      if (lane < 32 && col < F) P[(w == 1 ? 3 * FF : 4 * FF + F) + col] = s;
    }
  }
}

__global__ __launch_bounds__(NT) void ms_reduce_kernel(const float* __restrict__ part, int nb, int E,
                                                       float* __restrict__ out) {
  const int e = blockIdx.x * NT + threadIdx.x;
  if (e >= E) return;
  float s = 0.f;
  for (int b = 0; b < nb; ++b) s += part[(long)b * E + e];
  out[e] = s;
}

// the `refine` / `out` selectors over the n values of an LDS or register row; mode 1 log-softmax, 2 softmax
DEV void prob_row(float* p, int n, int stride, int mode) {
  float mx = p[0];
  for (int i = 1; i < n; ++i) mx = fmaxf(mx, p[i * stride]);
  float s = 0.f;
  for (int i = 0; i < n; ++i) s += expf(p[i * stride] - mx);
  if (mode == 1) {
    const float ls = mx + logf(s);
    for (int i = 0; i < n; ++i) p[i * stride] -= ls;
  } else {
    const float inv = 1.f / s;
    for (int i = 0; i < n; ++i) p[i * stride] = expf(p[i * stride] - mx) * inv;
  }
}
// q (the gradient w.r.t. p = selector(x)) -> the gradient w.r.t. x, in place
DEV void prob_row_bwd(const float* p, float* q, int n, int stride, int mode) {
  float t = 0.f;
  if (mode == 1) {
    for (int i = 0; i < n; ++i) t += q[i * stride];
    for (int i = 0; i < n; ++i) q[i * stride] -= expf(p[i * stride]) * t;
  } else {
    for (int i = 0; i < n; ++i) t = fmaf(p[i * stride], q[i * stride], t);
    for (int i = 0; i < n; ++i) q[i * stride] = p[i * stride] * (q[i * stride] - t);
  }
}

// out[r][o] = b[o] + sum_i W[o][i] p[r][i],  p[r] = selector(mean_v in[r * pool + v])
__global__ __launch_bounds__(NT) void ms_lin_fwd_kernel(const float* __restrict__ in, const float* __restrict__ W,
                                                        const float* __restrict__ b, float* __restrict__ out,
                                                        float* __restrict__ psave, long rows, int pool, int I, int O,
                                                        int mode) {
  __shared__ float ws[CM][CM + 1];  // [i][o]
  __shared__ float ps[LR][CM + 1];
  const int tid = threadIdx.x;
  const long r0 = (long)blockIdx.x * LR;
  for (int e = tid; e < O * I; e += NT) ws[e % I][e / I] = W[e];
  const float inv = 1.f / (float)pool;
  for (int e = tid; e < LR * I; e += NT) {
    const int rr = e / I, i = e - rr * I;
    const long r = r0 + rr;
    float s = 0.f;
    if (r < rows)
      for (int v = 0; v < pool; ++v) s += in[(r * pool + v) * I + i];
    ps[rr][i] = pool > 1 ? s * inv : s;
  }
  __syncthreads();
  if (mode && tid < LR) prob_row(ps[tid], I, 1, mode);
  __syncthreads();
  if (psave)
    for (int e = tid; e < LR * I; e += NT) {
      const int rr = e / I, i = e - rr * I;
      if (r0 + rr < rows) psave[(r0 + rr) * I + i] = ps[rr][i];
    }
  for (int e = tid; e < LR * O; e += NT) {
    const int rr = e / O, o = e - rr * O;
    if (r0 + rr < rows) {
      float acc = b[o];
      for (int i = 0; i < I; ++i) acc = fmaf(ws[i][o], ps[rr][i], acc);
      out[(r0 + rr) * O + o] = acc;
    }
  }
}

// partial[b] = [dW (O,I) | db (O)] of the block's row chunks (b, b + grid, ...);
// din[r * pool + v] = Jacobian(W^T d[r]) / pool for every v, when din is given
__global__ __launch_bounds__(NT) void ms_lin_bwd_kernel(const float* __restrict__ d, const float* __restrict__ p,
                                                        const float* __restrict__ W, float* __restrict__ din,
                                                        float* __restrict__ part, long rows, int pool, int I, int O,
                                                        int mode) {
  __shared__ float ws[CM][CM + 1];  // [o][i]
  __shared__ float ds[LR][CM + 1], ps[LR][CM + 1], qs[LR][CM + 1];
  const int tid = threadIdx.x, E = O * I + O;
  for (int e = tid; e < O * I; e += NT) ws[e / I][e % I] = W[e];
  float acc[LACC];
#pragma unroll
  for (int j = 0; j < LACC; ++j) acc[j] = 0.f;
  const float inv = 1.f / (float)pool;
  for (long r0 = (long)blockIdx.x * LR; r0 < rows; r0 += (long)gridDim.x * LR) {
    __syncthreads();
    for (int e = tid; e < LR * O; e += NT) {
      const int rr = e / O, o = e - rr * O;
      ds[rr][o] = r0 + rr < rows ? d[(r0 + rr) * O + o] : 0.f;
    }
    for (int e = tid; e < LR * I; e += NT) {
      const int rr = e / I, i = e - rr * I;
      ps[rr][i] = r0 + rr < rows ? p[(r0 + rr) * I + i] : 0.f;
    }
    __syncthreads();
    if (din) {
      for (int e = tid; e < LR * I; e += NT) {
        const int rr = e / I, i = e - rr * I;
        float s = 0.f;
        for (int o = 0; o < O; ++o) s = fmaf(ws[o][i], ds[rr][o], s);
        qs[rr][i] = s;
      }
      __syncthreads();
      if (mode && tid < LR) prob_row_bwd(ps[tid], qs[tid], I, 1, mode);
      __syncthreads();
      const int PI = pool * I;
      for (int e = tid; e < LR * PI; e += NT) {
        const int rr = e / PI, rem = e - rr * PI;
        if (r0 + rr < rows) din[(r0 + rr) * PI + rem] = pool > 1 ? qs[rr][rem % I] * inv : qs[rr][rem];
      }
    }
#pragma unroll
    for (int j = 0; j < LACC; ++j) {
      const int e = tid + NT * j;
      if (e < O * I) {
        const int o = e / I, i = e - o * I;
        float s = acc[j];
        for (int rr = 0; rr < LR; ++rr) s = fmaf(ds[rr][o], ps[rr][i], s);
        acc[j] = s;
      } else if (e < E) {
        float s = acc[j];
        for (int rr = 0; rr < LR; ++rr) s += ds[rr][e - O * I];
        acc[j] = s;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < LACC; ++j) {
    const int e = tid + NT * j;
    if (e < E) part[(long)blockIdx.x * E + e] = acc[j];
  }
}

__global__ __launch_bounds__(NT) void ms_prob_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long rows,
                                                         int C, int mode) {
  const long r = (long)blockIdx.x * NT + threadIdx.x;
  if (r >= rows) return;
  float p[CM];
  for (int i = 0; i < C; ++i) p[i] = x[r * C + i];
  prob_row(p, C, 1, mode);
  for (int i = 0; i < C; ++i) y[r * C + i] = p[i];
}

__global__ __launch_bounds__(NT) void ms_prob_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy,
                                                         float* __restrict__ dx, long rows, int C, int mode) {
  const long r = (long)blockIdx.x * NT + threadIdx.x;
  if (r >= rows) return;
  float p[CM], q[CM];
  for (int i = 0; i < C; ++i) p[i] = y[r * C + i], q[i] = dy[r * C + i];
  prob_row_bwd(p, q, C, 1, mode);
  for (int i = 0; i < C; ++i) dx[r * C + i] = q[i];
}

bool filters_ok(int F) { return F >= FMIN && F <= FMAX && F % 16 == 0; }
int launched() { return hipGetLastError() == hipSuccess ? STGCN_OK : STGCN_EHIP; }
long pack_n1(int F) { return (long)((F + 31) / 32) * (3 * F / 16) * 512; }
long pack_n2(int F) { return (long)((F + 31) / 32) * (F / 16) * 512; }

}  // namespace

long ms_pack_elems(int F) { return filters_ok(F) ? 2 * (pack_n1(F) + pack_n2(F)) : -1; }

int ms_pack_launch(const float* w1, const float* w2, int F, int kernel, void* dst, int dtype, hipStream_t s) {
  if (!w1 || !w2 || !dst || !filters_ok(F) || kernel != 3) return STGCN_EBADSHAPE;
  if (dtype != 0 && dtype != 1) return STGCN_EDTYPE;
  const unsigned nb = (unsigned)((ms_pack_elems(F) + NT - 1) / NT);
  if (dtype == 0) hipLaunchKernelGGL(ms_pack_kernel<float>, dim3(nb), dim3(NT), 0, s, w1, w2, F, (float*)dst);
  else hipLaunchKernelGGL(ms_pack_kernel<bf16>, dim3(nb), dim3(NT), 0, s, w1, w2, F, (bf16*)dst);
  return launched();
}

// shapes of a layer descriptor; R * dil (= L V d, the farthest tap offset) has to stay in int range
int ms_layer_check(const stgcn_ms_layer& d) {
  if (d.R < 1 || d.V < 1 || d.R % d.V || !filters_ok(d.F) || d.dil < 1 || (long)d.R * d.dil > 2147483647L)
    return STGCN_EBADSHAPE;
  if (d.dtype != 0 && d.dtype != 1) return STGCN_EDTYPE;
  return STGCN_OK;
}

int ms_wgrad_blocks(int R) {
  if (R < 1) return -1;
  const long n = ((long)R + TM - 1) / TM;
  return (int)(n < WG_MAX ? n : WG_MAX);
}

int ms_layer_fwd_launch(const stgcn_ms_layer& d, hipStream_t s) {
  const int rc = ms_layer_check(d);
  if (rc != STGCN_OK) return rc;
  if (!d.x || !d.wp || !d.b1 || !d.b2 || !d.y) return STGCN_EBADSHAPE;
  const dim3 grid((unsigned)(((long)d.R + TM - 1) / TM));
  const long D = (long)d.dil * d.V, n1 = pack_n1(d.F);
  if (d.dtype == 0)
    hipLaunchKernelGGL(ms_layer_fwd_kernel<float>, grid, dim3(NT), 0, s, d.x, (const float*)d.wp,
                       (const float*)d.wp + n1, d.b1, d.b2, d.y, (float*)d.h, (long)d.R, d.F, D);
  else
    hipLaunchKernelGGL(ms_layer_fwd_kernel<bf16>, grid, dim3(NT), 0, s, d.x, (const bf16*)d.wp, (const bf16*)d.wp + n1,
                       d.b1, d.b2, d.y, (bf16*)d.h, (long)d.R, d.F, D);
  return launched();
}

template <typename T> static int ms_layer_bwd_typed(const stgcn_ms_layer& d, hipStream_t s) {
  const long R = d.R, D = (long)d.dil * d.V, n1 = pack_n1(d.F), n2 = pack_n2(d.F);
  const T* wp = (const T*)d.wp;
  const T* w1t = wp + n1 + n2;
  const T* w2t = w1t + n1;
  const dim3 grid((unsigned)((R + TM - 1) / TM));
  hipLaunchKernelGGL(ms_layer_g_kernel<T>, grid, dim3(NT), 0, s, d.dy, w2t, (const T*)d.h, (T*)d.g, R, d.F);
  if (d.dx) hipLaunchKernelGGL(ms_layer_dx_kernel<T>, grid, dim3(NT), 0, s, (const T*)d.g, w1t, d.dy, d.dx, R, d.F, D);
  const int nb = ms_wgrad_blocks(d.R), E = 4 * d.F * d.F + 2 * d.F;
  long rows_per = (R + nb - 1) / nb;
  rows_per = (rows_per + 15) / 16 * 16;
  hipLaunchKernelGGL(ms_layer_wgrad_kernel<T>, dim3((unsigned)nb), dim3(NT), 0, s, d.x, d.dy, (const T*)d.h,
                     (const T*)d.g, R, d.F, D, rows_per, d.part);
  hipLaunchKernelGGL(ms_reduce_kernel, dim3((unsigned)((E + NT - 1) / NT)), dim3(NT), 0, s, d.part, nb, E, d.grads);
  return launched();
}

int ms_layer_bwd_launch(const stgcn_ms_layer& d, hipStream_t s) {
  const int rc = ms_layer_check(d);
  if (rc != STGCN_OK) return rc;
  if (!d.x || !d.wp || !d.h || !d.dy || !d.g || !d.part || !d.grads) return STGCN_EBADSHAPE;
  return d.dtype == 0 ? ms_layer_bwd_typed<float>(d, s) : ms_layer_bwd_typed<bf16>(d, s);
}

// which: 0 = ms_in (a selector prologue, no pooling, O = the stage's filters), 1 = ms_out (the joint mean, I = filters)
int ms_lin_check(const stgcn_ms_lin& d, int which) {
  if (d.rows < 1 || d.I < 1 || d.I > CM || d.O < 1 || d.O > CM || d.pool < 1 || d.pool > 32 ||
      (long)d.rows * d.pool > 2147483647L)
    return STGCN_EBADSHAPE;
  if (which == 0 ? (d.pool != 1 || !filters_ok(d.O) || d.mode < 0 || d.mode > 2) : (d.mode != 0 || !filters_ok(d.I)))
    return STGCN_EBADSHAPE;
  return STGCN_OK;
}

int ms_lin_blocks(int rows) {
  if (rows < 1) return -1;
  const long n = ((long)rows + LR - 1) / LR;
  return (int)(n < LIN_MAX ? n : LIN_MAX);
}

int ms_lin_fwd_launch(const stgcn_ms_lin& d, int which, hipStream_t s) {
  const int rc = ms_lin_check(d, which);
  if (rc != STGCN_OK) return rc;
  if (!d.in || !d.w || !d.b || !d.out) return STGCN_EBADSHAPE;
  hipLaunchKernelGGL(ms_lin_fwd_kernel, dim3((unsigned)(((long)d.rows + LR - 1) / LR)), dim3(NT), 0, s, d.in, d.w, d.b,
                     d.out, d.p, (long)d.rows, d.pool, d.I, d.O, d.mode);
  return launched();
}

int ms_lin_bwd_launch(const stgcn_ms_lin& d, int which, hipStream_t s) {
  const int rc = ms_lin_check(d, which);
  if (rc != STGCN_OK) return rc;
  if (!d.d || !d.p || !d.w || !d.part || !d.grads) return STGCN_EBADSHAPE;
  const int nb = ms_lin_blocks(d.rows), E = d.O * d.I + d.O;
  hipLaunchKernelGGL(ms_lin_bwd_kernel, dim3((unsigned)nb), dim3(NT), 0, s, d.d, d.p, d.w, d.din, d.part, (long)d.rows,
                     d.pool, d.I, d.O, d.mode);
  hipLaunchKernelGGL(ms_reduce_kernel, dim3((unsigned)((E + NT - 1) / NT)), dim3(NT), 0, s, d.part, nb, E, d.grads);
  return launched();
}

int ms_prob_launch(const float* y, const float* dy, float* out, int rows, int C, int mode, hipStream_t s) {
  if (!y || !out || rows < 1 || C < 1 || C > CM || (mode != 1 && mode != 2)) return STGCN_EBADSHAPE;
  const dim3 grid((unsigned)(((long)rows + NT - 1) / NT));
  if (dy) hipLaunchKernelGGL(ms_prob_bwd_kernel, grid, dim3(NT), 0, s, y, dy, out, (long)rows, C, mode);
  else hipLaunchKernelGGL(ms_prob_fwd_kernel, grid, dim3(NT), 0, s, y, out, (long)rows, C, mode);
  return launched();
}
