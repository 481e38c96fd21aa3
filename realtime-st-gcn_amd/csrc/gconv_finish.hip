// Finish of the graph-conv weight gradient (the maths is in gconv.hip's header): from dWeff (gconv_wgrad.hip) to
//   dW_p[co][ci]       = sum_{w,j} A_p[S(w)_j][w] dWeff[w][j][co][ci]
//   dA_p[S(w)_j][w]    = sum_{co,ci} W_p[co][ci] dWeff[w][j][co][ci]
// and, in the merged form, the gradient of the conv bias pushed through A (dA's bias term and db).
#include "common.h"
#include "launchers.h"

namespace {

// dW[p*Cout+co][ci] (+)= sum_{w, j<deg} A[p][nbr[w][j]][w] * dWeff[w][j][co][ci]
__global__ void gconv_dw_kernel(const float* __restrict__ dweff, const float* __restrict__ A, const int* nbr,
                                const int* deg, int P, int V, int J, int Cout, int Cin, float* dW) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long E = (long)Cout * Cin;
  if (idx >= (long)P * E) return;
  const int p = (int)(idx / E);
  const long e = idx % E;
  float s = 0.f;
  for (int w = 0; w < V; ++w)
    for (int j = 0; j < deg[w]; ++j) s += A[((long)p * V + nbr[w * J + j]) * V + w] * dweff[(long)(w * J + j) * E + e];
  dW[idx] += s;
}

// dA[p][nbr[w][j]][w] (+)= sum_{co,ci} W[p*Cout+co][ci] * dWeff[w][j][co][ci]; block per (pair, p)
__global__ void gconv_dA_kernel(const float* __restrict__ dweff, const float* __restrict__ W, const int* nbr,
                                const int* deg, int P, int V, int J, int Cout, int Cin, float* dA) {
  const int pair = blockIdx.x, p = blockIdx.y;
  const int w = pair / J, j = pair % J;
  if (j >= deg[w]) return;
  const long E = (long)Cout * Cin;
  const float* d = dweff + (long)pair * E;
  const float* wp = W + (long)p * E;
  float s = 0.f;
  for (long e = threadIdx.x; e < E; e += blockDim.x) s += wp[e] * d[e];
  s = wave_sum(s);
  __shared__ float part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float t = part[0] + part[1] + part[2] + part[3];
    dA[((long)p * V + nbr[w * J + j]) * V + w] += t;
  }
}

constexpr int PMAX = 4;
// dW[p][e] += sum_{pairs} A[p][v][w] dWeff[pair][e] for all p in one pass (dWeff read once).
// Block = 256 e-columns (4 per lane) x 4 groups over the used (w, j) pairs (pair list and coefficients A[p][S(w)_j][w]
// staged in LDS first: the per-pair deg -> nbr -> A chain of dependent global loads was this kernel's
// cost); fixed-order LDS combine.
constexpr int DW_PAIRS = 32 * 8;  // V * J upper bound for the LDS tables
// one block's work (block index bb of ceil(E / 64)); ``acc_out``: dW += (else dW =, the caller's buffer
// needs no zero fill)
DEV void gconv_dw_all_body(const float* __restrict__ dweff, const float* __restrict__ A, const int* nbr,
                           const int* deg, int P, int V, int J, long E, float* dW, long bb, bool acc_out) {
  __shared__ int spair[DW_PAIRS];
  __shared__ float scoef[DW_PAIRS][PMAX];
  __shared__ int snp;
  if (threadIdx.x == 0) {  // compacted list of used pairs, in (w, j) order
    int n = 0;
    for (int w = 0; w < V; ++w)
      for (int j = 0; j < deg[w]; ++j) spair[n++] = w * J + j;
    snp = n;
  }
  __syncthreads();
  const int np = snp;
  for (int i = threadIdx.x; i < np * PMAX; i += 256) {
    const int k = i / PMAX, p = i % PMAX;
    const int pr = spair[k], w = pr / J;
    scoef[k][p] = p < P ? A[((long)p * V + nbr[pr]) * V + w] : 0.f;
  }
  __syncthreads();
  const int g = threadIdx.x >> 6;
  // 4 consecutive e per lane (16-B loads of dWeff): a block covers 256 columns of E (E % 4 == 0)
  const long e = (bb * 64 + (threadIdx.x & 63)) * 4;
  float4 acc[PMAX];
#pragma unroll
  for (int p = 0; p < PMAX; ++p) acc[p] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (e < E) {
#pragma unroll 4
    for (int k = g; k < np; k += 4) {
      const float4 d = *reinterpret_cast<const float4*>(dweff + (long)spair[k] * E + e);
#pragma unroll
      for (int p = 0; p < PMAX; ++p) {
        const float c = scoef[k][p];
        acc[p].x += c * d.x; acc[p].y += c * d.y; acc[p].z += c * d.z; acc[p].w += c * d.w;
      }
    }
  }
  __shared__ float4 part[4][PMAX][64];
#pragma unroll
  for (int p = 0; p < PMAX; ++p) part[g][p][threadIdx.x & 63] = acc[p];
  __syncthreads();
  if (threadIdx.x < 64 && e < E) {
    const int l = threadIdx.x;
#pragma unroll
    for (int p = 0; p < PMAX; ++p)
      if (p < P) {
        const float4 a0 = part[0][p][l], a1 = part[1][p][l], a2 = part[2][p][l], a3 = part[3][p][l];
        float4 t = make_float4(((a0.x + a1.x) + a2.x) + a3.x, ((a0.y + a1.y) + a2.y) + a3.y,
                               ((a0.z + a1.z) + a2.z) + a3.z, ((a0.w + a1.w) + a2.w) + a3.w);
        float4* o = reinterpret_cast<float4*>(dW + (long)p * E + e);
        if (acc_out) {
          const float4 q = *o;
          t.x += q.x; t.y += q.y; t.z += q.z; t.w += q.w;
        }
        *o = t;
      }
  }
}
__global__ __launch_bounds__(256) void gconv_dw_all_kernel(const float* __restrict__ dweff, const float* __restrict__ A,
                                                           const int* nbr, const int* deg, int P, int V, int J, long E,
                                                           float* dW) {
  gconv_dw_all_body(dweff, A, nbr, deg, P, V, J, E, dW, blockIdx.x, true);
}

// dA[p][v][w] += <W_p, dWeff[pair]> for all p, in two deterministic steps: block (pair, chunk) writes the
// P partial dots of its DA_CHUNK-element slice to part[pair][chunk][p]; gconv_dA_reduce sums the chunks in
// order.  (pair, chunk) grid keeps >= ~1000 blocks in flight even for C = 64.
constexpr int DA_CHUNK = 2048;
DEV void gconv_dA_part_body(const float* __restrict__ dweff, const float* __restrict__ W, const int* deg, int P, int J,
                           long E, float* part, int pair, int c, int nch) {
  if (pair % J >= deg[pair / J]) return;  // block-uniform, no barrier after it
  const float* d = dweff + (long)pair * E;
  float acc[PMAX] = {0.f, 0.f, 0.f, 0.f};
  const long e1 = min(E, (long)(c + 1) * DA_CHUNK);
  for (long e = (long)c * DA_CHUNK + threadIdx.x * 4; e < e1; e += 1024) {  // 16-B loads (E % 4 == 0)
    const float4 dv = *reinterpret_cast<const float4*>(d + e);
#pragma unroll
    for (int p = 0; p < PMAX; ++p)
      if (p < P) {
        const float4 w = *reinterpret_cast<const float4*>(W + (long)p * E + e);
        acc[p] += ((w.x * dv.x + w.y * dv.y) + w.z * dv.z) + w.w * dv.w;
      }
  }
  __shared__ float red[4][PMAX];
#pragma unroll
  for (int p = 0; p < PMAX; ++p) {
    const float t = wave_sum(acc[p]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][p] = t;
  }
  __syncthreads();
  if (threadIdx.x < P)
    part[((long)pair * nch + c) * PMAX + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}
__global__ __launch_bounds__(256) void gconv_dA_part_kernel(const float* __restrict__ dweff, const float* __restrict__ W,
                                                            const int* deg, int P, int J, long E, float* part) {
  gconv_dA_part_body(dweff, W, deg, P, J, E, part, blockIdx.x, blockIdx.y, gridDim.y);
}

// The finish of the graph-conv weight / adjacency gradient with the conv bias pushed through A folded in, two
// launches instead of four (stgcn_gconv_wgrad_finish_bias).  Launch 1: blocks [0, nb_dw) the dW pass
// (overwriting), the rest the dA partial dots of (pair, chunk) = (b' / nch, b' % nch).
__global__ __launch_bounds__(256) void gconv_finish1_kernel(const float* __restrict__ dweff, const float* __restrict__ A,
                                                            const float* __restrict__ W, const int* nbr, const int* deg,
                                                            int P, int V, int J, long E, float* dW, int nb_dw, int nch,
                                                            float* part) {
  const int b = blockIdx.x;
  if (b < nb_dw) {
    gconv_dw_all_body(dweff, A, nbr, deg, P, V, J, E, dW, b, false);
  } else {
    const int b2 = b - nb_dw;
    gconv_dA_part_body(dweff, W, deg, P, J, E, part, b2 / nch, b2 % nch, nch);
  }
}

// Launch 2: blocks [0, P*V): (p, w) — every dA[p][v][w] written once: the support entries' chunk sums
// (fixed order) plus the bias term sum_c b[p][c] S[w][c] (v-independent; gcn_bias_bwd's value and order);
// blocks [P*V, ...): db[p*C + c] = sum_w colsum_p(A)[w] S[w][c] (gcn_bias_bwd's).
constexpr int FV_MAX = 32;
__global__ __launch_bounds__(256) void gconv_finish2_kernel(const float* __restrict__ part, const float* __restrict__ A,
                                                            const float* __restrict__ b, const float* __restrict__ S,
                                                            const int* nbr, const int* deg, int P, int V, int J, int C,
                                                            int nch, float* dA, float* db) {
  const int bx = blockIdx.x;
  if (bx < P * V) {
    const int p = bx / V, w = bx % V;
    float t = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) t += b[p * C + c] * S[w * C + c];
    t = wave_sum(t);
    __shared__ float red[4];
    __shared__ float sup[FV_MAX];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
    if (threadIdx.x < V) sup[threadIdx.x] = 0.f;
    __syncthreads();
    const float tot = ((red[0] + red[1]) + red[2]) + red[3];
    if (threadIdx.x < deg[w]) {  // the support entries of column w: chunk sums in order
      const int j = threadIdx.x, pair = w * J + j;
      float s = 0.f;
      for (int c = 0; c < nch; ++c) s += part[((long)pair * nch + c) * PMAX + p];
      sup[nbr[pair]] = s;
    }
    __syncthreads();
    for (int v = threadIdx.x; v < V; v += 256) dA[(p * V + v) * V + w] = sup[v] + tot;
    return;
  }
  __shared__ float cs[PMAX * FV_MAX];
  for (int i = threadIdx.x; i < P * V; i += 256) {
    const int p = i / V, w = i % V;
    float t = 0.f;
    for (int v = 0; v < V; ++v) t += A[(p * V + v) * V + w];
    cs[i] = t;
  }
  __syncthreads();
  const int i = (bx - P * V) * 256 + threadIdx.x;  // (p, c)
  if (i >= P * C) return;
  const int p = i / C, c = i % C;
  float t = 0.f;
  for (int w = 0; w < V; ++w) t += cs[p * V + w] * S[w * C + c];
  db[i] = t;
}

__global__ void gconv_dA_reduce_kernel(const float* __restrict__ part, const int* nbr, const int* deg, int P, int V,
                                       int J, int nch, float* dA) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // (pair, p)
  if (i >= V * J * P) return;
  const int pair = i / P, p = i % P, w = pair / J, j = pair % J;
  if (j >= deg[w]) return;
  float s = 0.f;
  for (int c = 0; c < nch; ++c) s += part[((long)pair * nch + c) * PMAX + p];
  dA[((long)p * V + nbr[w * J + j]) * V + w] += s;
}

}  // namespace

long gconv_wgrad_finish_workspace(int P, int V, int J, int Cout, int Cin) {
  const long E = (long)Cout * Cin;
  return P > PMAX ? 0 : (long)V * J * ((E + DA_CHUNK - 1) / DA_CHUNK) * PMAX * (long)sizeof(float);
}

bool gconv_finish_bias_ok(int P, int V, int J) { return P <= PMAX && V <= FV_MAX && V * J <= DW_PAIRS; }
// the one-pass dW and the chunked dA read dWeff / W as float4 (Cout * Cin % 4 == 0)

int gconv_wgrad_finish_bias_launch(const float* dweff, const float* A, const float* W, const int* nbr, const int* deg,
                                   int P, int V, int J, int Cout, int Cin, const float* bconv, const float* S, float* dW,
                                   float* dA, float* db, void* work, hipStream_t s) {
  if (!gconv_finish_bias_ok(P, V, J) || !work || ((long)Cout * Cin) % 4) return STGCN_EBADSHAPE;
  const long E = (long)Cout * Cin;
  const int nch = (int)((E + DA_CHUNK - 1) / DA_CHUNK);
  const int nb_dw = (int)((E + 255) / 256);  // 256 columns per dW block
  float* part = reinterpret_cast<float*>(work);
  hipLaunchKernelGGL(gconv_finish1_kernel, dim3((unsigned)(nb_dw + V * J * nch)), dim3(256), 0, s, dweff, A, W, nbr,
                     deg, P, V, J, E, dW, nb_dw, nch, part);
  hipLaunchKernelGGL(gconv_finish2_kernel, dim3((unsigned)(P * V + (P * Cout + 255) / 256)), dim3(256), 0, s,
                     (const float*)part, A, bconv, S, nbr, deg, P, V, J, Cout, nch, dA, db);
  return hipGetLastError() == hipSuccess ? STGCN_OK : STGCN_EHIP;
}

int gconv_wgrad_finish_launch(const float* dweff, const float* A, const float* W, const int* nbr, const int* deg,
                              int P, int V, int J, int Cout, int Cin, float* dW, float* dA, void* work, hipStream_t s) {
  const long E = (long)Cout * Cin;
  if (P > PMAX || (dA && !work) || V * J > DW_PAIRS || E % 4) {  // generic per-partition path (dA per (pair,p) block)
    const long n = (long)P * E;
    if (dW)
      hipLaunchKernelGGL(gconv_dw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dweff, A, nbr, deg, P,
                         V, J, Cout, Cin, dW);
    if (dA)
      hipLaunchKernelGGL(gconv_dA_kernel, dim3((unsigned)(V * J), (unsigned)P), dim3(256), 0, s, dweff, W, nbr, deg,
                         P, V, J, Cout, Cin, dA);
  } else {  // one pass over dWeff per output, all partitions at once
    if (dW)
      hipLaunchKernelGGL(gconv_dw_all_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, dweff, A, nbr, deg,
                         P, V, J, E, dW);
    if (dA) {
      const int nch = (int)((E + DA_CHUNK - 1) / DA_CHUNK);
      float* part = reinterpret_cast<float*>(work);
      hipLaunchKernelGGL(gconv_dA_part_kernel, dim3((unsigned)(V * J), (unsigned)nch), dim3(256), 0, s, dweff, W,
                         deg, P, J, E, part);
      hipLaunchKernelGGL(gconv_dA_reduce_kernel, dim3((unsigned)((V * J * P + 255) / 256)), dim3(256), 0, s, part,
                         nbr, deg, P, V, J, nch, dA);
    }
  }
  return hipGetLastError() == hipSuccess ? STGCN_OK : STGCN_EHIP;
}
