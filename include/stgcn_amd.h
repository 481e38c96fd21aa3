/*
 * stgcn_amd.h — C-ABI of the MI355X-native ST-GCN hot path (libstgcn_amd.so).
 *
 * The reference (maximyudayev/Realtime-ST-GCN) has no native code and no FFI: its hot path is
 * a stack of PyTorch aten ops inside nn.Modules.  Each entry point below replaces one or more of
 * those aten calls; the reference call site it replaces is cited (file:line, relative to the
 * reference root).  The Python package realtime-st-gcn_amd/ binds these with ctypes underneath
 * modules that keep the reference's nn.Module API and state_dict names.
 *
 * Conventions
 *   - Plain pointers and sizes only; device pointers unless noted; no framework types.
 *   - Activations are the reference's logical (N, C, T, V) tensors stored channels-last:
 *     element (n, c, t, v) at ((n*T + t)*V + v)*ld + c  ("rows" of ld >= C elements).
 *   - dtype: 0 = fp32 (parity path), 1 = bf16 (perf path).  Accumulation is fp32.
 *   - stream: a hipStream_t (NULL = default stream).  Every call is asynchronous.
 *   - Return: 0 ok, 1 bad shape/arguments, 2 unsupported dtype, 3 HIP launch error.
 *   - Thread-safety: no global mutable state; calls on different streams/devices are independent
 *     (the reference runs replicas from nn.DataParallel threads, processor.py:32-33).
 */
#ifndef STGCN_AMD_H
#define STGCN_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped on every change of a descriptor's layout or of an entry point's signature; realtime-st-gcn_amd/_lib.py
 * refuses a library whose stgcn_abi_version() differs from the version it was written against.
 *   1: rounds 1-4;  2: round 5 (stgcn_gconv_desc gained res / res_bits / res_ld);
 *   3: round 6 (stgcn_gcn_tile removed; stgcn_layer_fused_desc is the LayerNorm layer only: the BatchNorm
 *      fields n1_scale / n1_shift / stats / ln / g_in / g_in_ld and stgcn_layer_fused_row_blocks removed);
 *   4: round 6 (stgcn_rt_frame + stgcn_rt_layer / stgcn_rt_frame_desc: the RT per-frame step in one launch;
 *      stgcn_gconv_wgrad_desc gained phase);
 *   5: round 6 (stgcn_bn_merge: one (count, mean, M2) entry per channel, the SyncBatchNorm exchange unit);
 *   6: stgcn_co_* + stgcn_co_layer: CoST-GCN per-frame inference (co_frame.hip);
 *   7: stgcn_ms_* + stgcn_ms_layer / stgcn_ms_lin: MS-TCN stages, forward and backward (ms_stage.hip);
 *      still 7: stgcn_rt_streams* added (rt_streams.hip) — additive, no existing struct or entry point changed;
 *      still 7: stgcn_co_streams* added (co_streams.hip) — additive likewise;
 *      still 7: stgcn_rt_streams_desc.pad_ became dtype (0 = fp32, what a zero-filled descriptor always passed; 1 = bf16
 *      conv operands), stgcn_rt_streams_layer.wp / wrp became const void* of that element type, and
 *      stgcn_rt_streams_pack_weight_as was added — no size, offset or existing entry point changed;
 *      still 7: stgcn_co_clip* added — additive likewise;
 *      still 7: stgcn_co_streams_clip* added (co_streams_clip.hip) — additive likewise; stgcn_co_clip* are since
 *      served by the same file as its B = 1 case and the two layer structs are one type — no layout changed;
 *      still 7: stgcn_rt_streams_clip* added (rt_streams_clip.hip) — additive likewise;
 *      still 7: stgcn_stream_state* added (stream_state.hip) — additive likewise. */
#define STGCN_ABI_VERSION 7

/* Implicit-GEMM (Kt x 1) row convolution; see conv_rows.hip for the exact contract.
 * Replaces: nn.Conv2d tcn.2 (models/stgcn/stgcn.py:154-159), residual.0 (stgcn.py:165-170),
 * gcn.conv (models/utils/tgcn.py:48-55,71), fcn_in/fcn_out (stgcn.py:49,74,85,95), OfflineLayer
 * conv/residual (models/rtstgcn/rtstgcn.py:316,330) and their input-gradients (trans = 1). */
typedef struct {
  const void* in;
  void* out;
  const void* w;          /* packed [Kt][Cout_pad][Cin_pad], element type = dtype */
  const float* bias;      /* [Cout] (bias_mode 1) | [V][Cout] (2) | [N][V][Cout] (3) | NULL */
  const float* pro_a;     /* prologue scale [Cin] (pro 1) | LN gamma [Cin][V] (pro 2) */
  const float* pro_b;     /* prologue shift [Cin] | LN beta [Cin][V] */
  const float* pro_stats; /* pro 2: float2 (mean, rstd) per input frame [N*T_in] */
  float* stats;           /* optional BN partials: float4 (count, mean, M2, 0) [row_blocks][Cout_pad] */
  int N, T_in, T_out, V, Cin, Cout, Cin_pad, Cout_pad;
  int Kt, stride, pad, trans, pro, bias_mode, accumulate;
  int in_ld, out_ld;
  const void* w_frag;     /* optional MFMA-fragment image of the weights for the wide-channel Kt = 9 kernel
                           * (NULL: other kernels): stride 1 -> stgcn_pack_weight_frag's image of w;
                           * stride 2 -> stgcn_pack_weight_s2frag's parity-folded image (trans to match) */
} stgcn_conv_desc;

int stgcn_conv_rows(const stgcn_conv_desc* d, int dtype, void* stream);
/* The 64-channel Kt = 9 stride-1 temporal conv (stgcn.py:151-159) forward (trans 0, pro 0 or 1: BN1 scale /
 * shift + ReLU on the input, bias_mode 0/1, optional BN partial statistics [stgcn_tconv_frame_row_blocks(N, T)]
 * [Cout_pad]) and data gradient (trans 1, pro 0), bf16, on the row-streaming kernel (tconv_frame.hip): the same
 * arithmetic as stgcn_conv_rows for these shapes; w_frag = the MFMA-fragment image of the packed weight
 * (stgcn_pack_weight_frag, Kt = 9), Cin = Cout = 64, pad = 4, 16 < V <= 25, in_ld % 8 == 0, out_ld % 8 == 0 (16-B
 * row stores), no accumulate; other shapes return STGCN_EBADSHAPE (use stgcn_conv_rows). */
int stgcn_tconv_frame(const stgcn_conv_desc* d, void* stream);
long stgcn_tconv_frame_row_blocks(int N, int T);
/* Pack an fp32 weight given as any strided [Kt][Cout][Cin] view (element (k,co,ci) at src[k*s0+co*s1+ci*s2])
 * into the zero-padded contiguous [Kt][Cout_pad][Cin_pad] dtype image stgcn_conv_rows reads. */
int stgcn_pack_weight(const float* src, long s0, long s1, long s2, int Kt, int Cout, int Cin, void* dst, int Cout_pad,
                      int Cin_pad, int dtype, void* stream);
/* stgcn_pack_weight plus the MFMA-fragment image dst_frag (same element count; Cout_pad % 32 == 0,
 * Cin_pad % 16 == 0): 1-KiB blocks [k][co/32][ci/16], lane (ci%16)/8*32 + co%32 holding 8 consecutive ci,
 * so one 32x32x16 B fragment is one contiguous wave load (conv_wide.hip). */
int stgcn_pack_weight_frag(const float* src, long s0, long s1, long s2, int Kt, int Cout, int Cin, void* dst,
                           void* dst_frag, int Cout_pad, int Cin_pad, int dtype, void* stream);
/* Parity-folded MFMA-fragment image of a stride-2 Kt = 9 weight src [9][Cout][Cin] (fp32, element
 * (k,co,ci) at src[k*s0+co*s1+ci*s2]) — the w_frag a stride-2 stgcn_conv_rows call takes: the 5-tap
 * conv over frame pairs (forward: W'[t][co][par*Cin+ci] = W[2t+par][co][ci]; trans = 1, the data grad:
 * W'[t][par*Cout+co][ci] = W[8-2t+par][co][ci]), dst_frag holding 5 * 2 * Cout * Cin bf16.
 * Replaces: the strided tcn.2 of layers with stride 2 (models/stgcn/stgcn.py:154-159) and its input grad. */
int stgcn_pack_weight_s2frag(const float* src, long s0, long s1, long s2, int Cout, int Cin, void* dst_frag, int trans,
                             int dtype, void* stream);
/* column tile the packed weights must be padded to (Cout_pad % tile == 0) */
int stgcn_conv_rows_col_tile(int cout);
/* upper bound on row blocks (first dim of the BN partial-stat buffer, which the caller zero-fills) */
long stgcn_conv_rows_row_blocks(long M, int cout);

/* Weight gradient of stgcn_conv_rows (trans = 0): dw[Kt][Cout][Cin] += ... (fp32, zeroed by caller).
 * Replaces: convolution_backward weight path of the convs above (autograd of stgcn.py:154-170). */
typedef struct {
  const void* in;
  const void* dy;
  float* dw;
  const float* pro_a;
  const float* pro_b;
  const float* pro_stats;
  int N, T_in, T_out, V, Cin, Cout, Kt, stride, pad, pro;
  int in_ld, dy_ld;
  long rows_per_block; /* filled by the library */
  void* work;          /* optional workspace (bf16 frame-tiled path: per-block fp32 partials) */
  long work_bytes;     /* its size; stgcn_conv_wgrad_workspace() tells how much the fast path needs */
  int out_mode;        /* 0: dw[Kt][Cout][Cin] += gradient; 1: dw OVERWRITTEN in nn.Conv2d weight order
                        * [Cout][Cin][Kt] (no zero fill, no permute copy) — the workspace paths only
                        * (stgcn_conv_wgrad_workspace() > 0), else STGCN_EBADSHAPE */
  int pad_;
} stgcn_wgrad_desc;

int stgcn_conv_wgrad(const stgcn_wgrad_desc* d, int dtype, void* stream);
/* workspace bytes for the deterministic frame-tiled path (0: shape/dtype served without one) */
long stgcn_conv_wgrad_workspace(const stgcn_wgrad_desc* d, int dtype);

/* Graph (joint-axis) mixing of ConvTemporalGraphical (models/utils/tgcn.py:58-79), A applied first.
 *   fwd  : XA[(n,t,w)][p*Cin+ci] = sum_v A[(n),p,v,w] x[(n,t,v)][ci]             (tgcn.py:76)
 *   trans: dx[(n,t,v)][ci] (+)= sum_{p,w} A[(n),p,v,w] DW[(n,t,w)][p*Cin+ci]       (autograd of :76)
 *   dA   : dA[(n),p,v,w] += sum_{t,ci} x[(n,t,v)][ci] DW[(n,t,w)][p*Cin+ci]          (grad of A)
 *   bias : bias2d[(n),w,c] = sum_p b[p*C+c] sum_v A[(n),p,v,w]   (the conv bias pushed through A)
 * A is fp32 [P][V][V] (shared) or [N][P][V][V] (per_sample, AAGCN models/aagcn/aagcn.py:148). */
typedef struct {
  const void* x;
  void* out;
  const float* A;
  int N, T, V, P, Cin, per_sample, accumulate;
  int x_ld, out_ld;
} stgcn_amix_desc;

int stgcn_amix_fwd(const stgcn_amix_desc* d, int dtype, void* stream);
int stgcn_amix_trans(const stgcn_amix_desc* d, int dtype, void* stream);
/* dA (+)= sum over frames of x (x) DW.  work: stgcn_amix_dA_workspace() bytes -> per-block partials summed
   in a fixed order (bit-reproducible); NULL -> fp32 atomics (run-to-run order noise). */
long stgcn_amix_dA_workspace(const stgcn_amix_desc* d);
int stgcn_amix_dA(const stgcn_amix_desc* d, const void* dw, float* dA, void* work, int dtype, void* stream);
/* Shared-A gradients of the graph-conv bias (autograd of tgcn.py:71-79 through the bias), from
 * S[w][c] = sum of dg over the rows of joint w (stgcn_rowgroup_sum):
 *   dA[p][v][w] += sum_c b[p*C+c] S[w][c];   db[p*C+c] = sum_w (sum_v A[p][v][w]) S[w][c] */
int stgcn_gcn_bias_bwd(const float* A, const float* b, const float* S, int P, int V, int C, float* dA, float* db,
                       void* stream);
int stgcn_gcn_bias(const float* A, const float* b, float* out, int N, int P, int V, int C, int per_sample,
                   void* stream);

/* Graph convolution as a joint-gathered GEMM for a batch-shared A (ConvTemporalGraphical,
 * models/utils/tgcn.py:58-79; replaces the conv1x1 + einsum pair):
 *   out[(i,a)][r] (+)= sum_{j<deg[a]} sum_c in[(i, nbr[a*J+j])][c] * w[a][j][r][c]  (+ bias[a][r]),
 * i = n*T + t in [0, NT).  w = effective weights from stgcn_gconv_weights ([V][J][Cout_pad][Cin_pad]):
 *   trans 0 (forward):   w[w][j][co][ci] = sum_p A[p][S(w)_j][w] * W[p*Cout+co][ci]
 *   trans 1 (data grad): w[v][j][ci][co] = sum_p A[p][v][R(v)_j] * W[p*Cout+co][ci]
 * with nbr = the support lists S (forward) or the reverse lists R (data grad).  Optional BN partial
 * statistics per (row block, channel) as stgcn_conv_rows, row blocks <= stgcn_gconv_row_blocks. */
typedef struct {
  const void* in;
  void* out;
  const void* w;
  const int* nbr;   /* [V][J] */
  const int* deg;   /* [V] */
  const float* bias; /* [V][Cout] or NULL */
  float* stats;
  int NT, V, J, Cin, Cout, Cin_pad, Cout_pad, in_ld, out_ld, accumulate;
  /* optional masked residual (bf16, accumulate = 0, 16-B aligned rows): out = result + res * mask with mask bit
   * c % 8 of byte res_bits[row * (Cout / 8) + c / 8] (stgcn_bn_apply_bits' layout) — the identity residual's
   * gradient dz = dy * [y > 0] of stgcn.py:191-193 added in the data gradient's epilogue instead of being
   * written by the BatchNorm backward and read back here.  res rows: ld res_ld, rows as out. */
  const void* res;
  const void* res_bits;
  int res_ld;
} stgcn_gconv_desc;

int stgcn_gconv(const stgcn_gconv_desc* d, int dtype, void* stream);

long stgcn_gconv_row_blocks(int NT, int V);
int stgcn_gconv_weights(const float* A, const float* W, const int* nbr, const int* deg, int P, int V, int J, int Cout,
                        int Cin, int trans, void* out, int rows_pad, int cols_pad, int dtype, void* stream);
/* stgcn_gconv_weights (forward form, trans = 0) and stgcn_gcn_bias for a shared A in ONE launch:
 * bias2d[w][co] = sum_p b[p*Cout + co] * sum_v A[p][v][w]  (fp32 [V][Cout]; replaces the separate
 * bias-through-A launch of ConvTemporalGraphical.forward, tgcn.py:71-79, conv bias then einsum with A) */
int stgcn_gconv_weights_bias(const float* A, const float* W, const float* b, const int* nbr, const int* deg, int P,
                             int V, int J, int Cout, int Cin, void* out, int rows_pad, int cols_pad, float* bias2d,
                             int dtype, void* stream);
/* dweff[w][j][co][ci] = sum_i dy[(i,w)][co] * x[(i, nbr[w][j])][ci]   (fp32 [V][J][Cout][Cin], written
 * whole: 0 for the unused slots j >= deg[w]) */
typedef struct {
  const void* x;
  const void* dy;
  const int* nbr;
  const int* deg;
  float* dweff;
  int NT, V, J, Cin, Cout, x_ld, dy_ld;
  void* work;
  long work_bytes;
  float* rowsum; /* optional [V][Cout]: rowsum[w][co] = sum_i dy[(i,w)][co] (bias through A), or NULL */
  int phase;     /* 0: the whole gradient; 1: the accumulation kernel only (row-range partials left in work);
                  * 2: the slab reduction only (work holds phase 1's partials of the same desc) — so a caller can
                  * time the accumulation kernel alone; plans without a slab do everything in phase 1 */
  int pad_;
} stgcn_gconv_wgrad_desc;

int stgcn_gconv_wgrad(const stgcn_gconv_wgrad_desc* d, int dtype, void* stream);
long stgcn_gconv_wgrad_workspace(const stgcn_gconv_wgrad_desc* d, int dtype);
/* dW[p*Cout+co][ci] += sum_{w,j} A[p][S(w)_j][w] dweff[w][j][co][ci]  (dW may be NULL);
 * dA[p][S(w)_j][w] += sum_{co,ci} W[p*Cout+co][ci] dweff[w][j][co][ci]  (dA may be NULL)
 * work: stgcn_gconv_wgrad_finish_workspace() bytes (chunked dA partials, fixed-order reduce) or NULL
 * (slower per-partition path).  Deterministic either way. */
long stgcn_gconv_wgrad_finish_workspace(int P, int V, int J, int Cout, int Cin);
/* The same finish with the conv bias pushed through A folded in (stgcn_gcn_bias_bwd), in two launches, every
 * output OVERWRITTEN (no zero fill needed):
 *   dW[p*Cout+co][ci] = sum_{w,j} A[p][S(w)_j][w] dweff[w][j][co][ci]
 *   dA[p][v][w]       = [v in S(w)] sum_{co,ci} W[p*Cout+co][ci] dweff[pair(v,w)][co][ci] + sum_c bconv[p*Cout+c] S[w][c]
 *   db[p*Cout+c]      = sum_w colsum_p(A)[w] S[w][c]
 * S = the per-joint row sums of dy [V][Cout] (stgcn_gconv_wgrad's rowsum); work as above (required);
 * P <= 4, V <= 32.  Bit-identical to stgcn_gconv_wgrad_finish into zeros followed by stgcn_gcn_bias_bwd. */
int stgcn_gconv_wgrad_finish_bias(const float* dweff, const float* A, const float* W, const int* nbr, const int* deg,
                                  int P, int V, int J, int Cout, int Cin, const float* bconv, const float* S, float* dW,
                                  float* dA, float* db, void* work, void* stream);
int stgcn_gconv_wgrad_finish(const float* dweff, const float* A, const float* W, const int* nbr, const int* deg, int P,
                             int V, int J, int Cout, int Cin, float* dW, float* dA, void* work, void* stream);

/* BatchNorm with batch statistics (nn.BatchNorm2d(track_running_stats=False), stgcn.py:152,160,171;
 * BatchNorm1d input norm, models/utils/batchnorm.py:13-23 viewed as [N*T][V*C]).
 * Partials are float4 (count, mean, M2, 0) per (row block, channel); finalize merges them (fp64).
 * Row views (stgcn_bn_stats_partial, stgcn_bn_apply, stgcn_bn_bwd_reduce / _apply, stgcn_rowgroup_sum): 16-B
 * units (8 bf16 / 4 fp32 channels) when C, every row stride and every base pointer are multiples of the unit,
 * else one element at a time; STGCN_EBADSHAPE when a row does not fit 256 threads (C > 256 element-wise,
 * C / unit > 256 otherwise).  stgcn_bn_apply_bits and the fused backward have no element-wise route: a view
 * that rules out the 16-B units (stride or pointer) is STGCN_EBADSHAPE. */
long stgcn_bn_stat_blocks(long M);
int stgcn_bn_stats_partial(const void* x, int ld, long M, int C, void* part_f4, int dtype, void* stream);
int stgcn_bn_finalize(const void* part_f4, int nblocks, int ld_part, int C, const float* gamma, const float* beta,
                      float eps, void* mean_rstd_f2, float* scale, float* shift, void* stream);
/* merged_f4[c] = the nblocks partials of channel c merged (fp64) into ONE (count, mean, M2, 0) entry: a rank's
 * contribution to SyncBatchNorm (torch.nn.SyncBatchNorm's batch_norm_gather_stats_with_counts role, the
 * north_star's optional SyncBN); the gathered [ranks][C] entries go back through stgcn_bn_finalize
 * (nblocks = ranks, ld_part = C).  No reference counterpart: the reference's DataParallel keeps per-replica
 * statistics (processor.py:32-33). */
int stgcn_bn_merge(const void* part_f4, int nblocks, int ld_part, int C, void* merged_f4, void* stream);
/* Fused BatchNorm backward (two row passes), see bn_fused.hip:
 *   reduce: dz = dy*mask; sums[c] = (sum dz, sum dz*xhat1, sum dz*xhat2, 0)
 *   apply : out1 = g1*rstd1*(dz - S0/M - xhat1*S1/M) (or dz when x1 == NULL);
 *           out2 (+)= g2*rstd2*(dz - S0/M - xhat2*S2/M) (or dz when x2 == NULL);  osum[c] = (sum out1,
 *           sum out2) — the conv-bias gradients.  mask: 0 none | 1 mref > 0 | 2 mref*msc + msh > 0 |
 *           3 (bf16, C % 8 == 0) mref = the bit mask stgcn_bn_apply_bits wrote: byte [m * ldm + c / 8], bit c % 8
 *           set where the stored output was > 0 (ldm = bytes per row, >= C / 8) — 1/16 of the bytes of mask 1.
 * Replaces: autograd of stgcn.py:160,171,191-193 (BN2 / residual BN / ReLU / add) and :152-153. */
typedef struct {
  const void* dy;
  const void* mref;
  const void* x1;
  const void* x2;
  const float* msc;
  const float* msh;
  const float* mean_rstd1; /* float2 [C] */
  const float* mean_rstd2;
  const float* gamma1;
  const float* gamma2;
  float* sums;  /* float4 [C], then the same planar: float [3][C] (7*C floats) */
  void* out1;
  void* out2;
  float* osum;  /* optional, layout as sums */
  float* work;  /* float4 [blocks][C], stgcn_bn_bwd_fused_workspace() floats */
  long M;
  int C, mask, lddy, ldm, ldx1, ldx2, ldo1, ldo2, acc2;
} stgcn_bn_bwd_desc;

long stgcn_bn_bwd_fused_workspace(long M, int C, int dtype);
int stgcn_bn_bwd_fused_reduce(const stgcn_bn_bwd_desc* d, int dtype, void* stream);
int stgcn_bn_bwd_fused_apply(const stgcn_bn_bwd_desc* d, int dtype, void* stream);
/* y = act(u*sc + sh + res), res_mode 0 none | 1 r | 2 r*rsc + rsh  (stgcn.py:191-193, rtstgcn.py:386-389);
 * relu bit 0: ReLU after the residual add; bit 1: ReLU on the normalised branch before the add. */
int stgcn_bn_apply(const void* u, int ldu, const float* sc, const float* sh, int res_mode, const void* r, int ldr,
                   const float* rsc, const float* rsh, int relu, void* y, int ldy, long M, int C, int dtype,
                   void* stream);
/* stgcn_bn_apply (bf16, C % 8 == 0) that also writes the output's sign bits for the backward's ReLU mask:
 * bits[m * (C / 8) + c / 8] bit c % 8 = (stored y[m][c] > 0) — what the fused backward reads as mask 3
 * instead of re-reading y (1/16 of the bytes). */
int stgcn_bn_apply_bits(const void* u, int ldu, const float* sc, const float* sh, int res_mode, const void* r, int ldr,
                        const float* rsc, const float* rsh, int relu, void* y, int ldy, long M, int C, void* bits,
                        void* stream);
/* sums_f2[c] = (sum dz, sum dz*xhat) with dz = dy * mask (mask 0 none | 1 mref>0 | 2 mref*msc+msh>0);
 * x may be NULL (then only sum dz).  part_f2 scratch: [stgcn_bn_stat_blocks(M)][C] float2. */
int stgcn_bn_bwd_reduce(const void* dy, int lddy, int mask, const void* mref, int ldm, const float* msc,
                        const float* msh, const void* x, int ldx, const void* mean_rstd_f2, long M, int C,
                        void* part_f2, void* sums_f2, int dtype, void* stream);
/* dx (+)= gamma*rstd*(dz - S1/M - xhat*S2/M); x == NULL: dx (+)= dz */
int stgcn_bn_bwd_apply(const void* dy, int lddy, int mask, const void* mref, int ldm, const float* msc,
                       const float* msh, const void* x, int ldx, const void* mean_rstd_f2, const float* gamma,
                       const void* sums_f2, long M, int C, void* dx, int lddx, int accumulate, int dtype,
                       void* stream);
/* S[g][c] += sum_{m % G == g} x[m][c]  (per-joint column sums: GCN bias gradient);
 * period > 0: per-sample S[n][g][c] over rows [n*period, (n+1)*period) (per-sample A, AAGCN). */
int stgcn_rowgroup_sum(const void* x, int ld, long M, int C, int G, long period, float* S, float* work, int dtype,
                       void* stream);
/* floats of scratch `work` stgcn_rowgroup_sum needs (per-block partial slabs, reduced deterministically) */
long stgcn_rowgroup_sum_workspace(long M, int C, int G, long period);

/* Custom LayerNorm([C,1,V]) (models/utils/layernorm.py:4-28): per (n,t) frame over (C,V),
 * unbiased variance, per-(c,v) affine. */
int stgcn_ln_stats(const void* x, int ld, long frames, int V, int C, float eps, void* stats_f2, int dtype,
                   void* stream);
int stgcn_ln_apply(const void* u, int ldu, const void* st_f2, const float* g, const float* b, int res_mode,
                   const void* r, int ldr, const void* rst_f2, const float* rg, const float* rb, int relu, void* y,
                   int ldy, long M, int V, int C, int dtype, void* stream);
/* dx (+)= rstd*(gz - mean(gz) - xhat*sum(gz*xhat)/(E-1)), gz = dz*g, dz = dy*mask (0 none | 1 mref > 0 |
 * 2 relu(LN(x)) > 0); dgb (optional, [2][C*V]) += (sum dz*xhat, sum dz) over all frames, reduced in a fixed
 * order through `work` (stgcn_ln_bwd_workspace bytes; unused when dgb is NULL). */
int stgcn_ln_bwd(const void* dy, int lddy, int mask, const void* mref, int ldm, const void* x, int ldx,
                 const void* st_f2, const float* g, const float* b, long frames, int V, int C, void* dx, int lddx,
                 int accumulate, float* dgb, void* work, long work_bytes, int dtype, void* stream);
long stgcn_ln_bwd_workspace(long frames, int V, int C, int dtype);

/* out_bf16[m][c] = bf16(x[m][c]) and colsum[c] = sum_m x[m][c] (fp32, fixed order) from one read of the fp32
 * rows: the attention projections' backward (models/aagcn/aagcn.py:139-141 autograd; the bf16 GEMM operand
 * and the bias gradients).  C % 4 == 0, C <= 1024; work: stgcn_cast_colsum_workspace floats. */
int stgcn_cast_colsum(const float* x, int ldx, long M, int C, void* out_bf16, int ldo, float* colsum, float* work,
                      void* stream);
long stgcn_cast_colsum_workspace(long M, int C);

/* Head: F.avg_pool2d over (T,V) (stgcn.py:92) and its gradient. */
int stgcn_pool_rows(const void* x, int ld, int N, int R, int C, void* out, int ldo, int dtype, void* stream);
int stgcn_unpool_rows(const void* dp, int ldp, int R, int C, long M, void* dx, int ldx, int dtype, void* stream);

/* RT-ST-GCN temporal aggregation (models/rtstgcn/rtstgcn.py):
 *   box_sum : y[...,t] = sum_{i < K/S} x[..., t - i*S]  on rows (Toeplitz matmul rtstgcn.py:366-379),
 *             trans = 1 gives its adjoint (gradient).
 *   online  : one frame of AggregateStgcn.forward (rtstgcn.py:591-627) with device-resident FIFO. */
int stgcn_box_sum(const void* x, int ldx, void* y, int ldy, int N, int T, int V, int C, int K, int S, int trans,
                  int accumulate, int dtype, void* stream);
int stgcn_rt_online_step(const void* z_f32, float* fifo, float* acc, int* idx, int C, int V, int fifo_size, int S,
                         float* out, void* stream);

/* AAGCN attention adjacency (models/aagcn/aagcn.py:142-145): C[n,p] = softmax_w(theta_p^T phi_p) over
 * K = T*ce, theta/phi rows [N][T][V][ld] (channel p*ce+c).  C: fp32 [N][P][V][V].  Backward writes
 * dS (scratch, fp32 like C) and dtheta/dphi (rows like theta/phi). */
/* AgcnLayer's theta / phi projections for a bf16 model (aagcn.py:139-141): out[r][o] = bias[o] +
 * sum_c w[o][c] x[r][c], x bf16 rows [M][ldx] (Cin % 16 == 0, <= 256), w fp32 [Nout][Cin] (theta and phi
 * stacked), out fp32 rows [M][ldo]: fp32-accurate outputs (w split into two bf16 parts on the matrix cores)
 * without converting x; the attention logits need fp32 theta/phi. */
int stgcn_attn_proj(const void* x, int ldx, long M, int Cin, const float* w, const float* bias, int Nout, float* out,
                    int ldo, void* stream);
/* work: stgcn_attn_scores_workspace() bytes (deterministic T-chunk reduction) or NULL (atomics). */
long stgcn_attn_scores_workspace(int N, int T, int V, int P);
int stgcn_attn_scores(const void* theta, const void* phi, int ld, int N, int T, int V, int P, int ce, float* C,
                      void* work, int dtype, void* stream);
int stgcn_attn_bwd(const void* theta, const void* phi, int ld, int N, int T, int V, int P, int ce, const float* C,
                   const float* dC, float* dS, void* dtheta, void* dphi, int dtype, void* stream);

int stgcn_abi_version(void);

/* Segmentation loss + statistics of a prediction series (replaces utils/loss.py:25-41 Loss.__call__ and
 * utils/statistics.py:5-16 Statistics.__call__ on the (1, C, L) output of segment_generator.mask_segment).
 *   p: fp32 [L][ldp] predictions (frame w, class c); labels: int64 [L - first]; wt: fp32 [C] class weights
 *   (1 - class_dist / sum, loss.py:20); mode: 0 'logits', 1 'logsoftmax', 2 'softmax' output_type;
 *   first: 1 drops frame 0 from the CE and statistics (subsegment i > 0).
 *   Data-parallel shards: prev = predictions of the frame before this shard (its MSE pair) or NULL,
 *   den = the global CE weight sum (device fp32 scalar; NULL: this call's own), pairs = the global MSE
 *   pair count (<= 0: this call's own).
 *   Outputs: out[0] ce, out[1] mse (this call's share of the trial's loss), out[2] top-1 hits,
 *   out[3] top-5 hits, out[4] this call's CE weight sum (out: fp32 [8]); dce / dmse [L][C] the gradients
 *   of ce and mse w.r.t. p (NULL: skipped); top5 int32 [L][5] class indices (NULL: skipped).
 *   work: stgcn_seg_loss_workspace(L) bytes.  Deterministic (fixed-order sums). */
long stgcn_seg_loss_workspace(int L);
int stgcn_seg_loss(const float* p, int ldp, const long* labels, const float* wt, const float* prev, int L, int C,
                   int first, int mode, const float* den, float pairs, float* dce, float* dmse, int* top5, float* work,
                   float* out, void* stream);
/* dp[i] = (*gce) * dce[i] + (*gmse) * dmse[i]  (gce/gmse: device fp32 scalars, NULL = 0) — the backward of
 * the two loss terms given the upstream gradients, without a host round trip. */
int stgcn_seg_loss_bwd(const float* dce, const float* dmse, const float* gce, const float* gmse, long n, float* dp,
                       void* stream);

/* The fused ST-GCN layer (layer_fused.hip; BASELINE north_star) of a LayerNorm StgcnLayer, 64 -> 64 channels,
 * stride 1, Kt = 9, identity or no residual, as ONE kernel:
 *   g = ConvTemporalGraphical(x) (tgcn.py:58-79; graph conv recomputed per frame on the matrix cores, never stored),
 *   h = relu(LN1(g)), u = tcn(h) + tbias (stgcn.py:151-159), y = relu(LN2(u) + residual * x) (stgcn.py:181-193),
 * with LayerNorm([64,1,V]) per frame over C x V, unbiased variance (layernorm.py:22-28); y is written to z.
 * bf16; P <= 3; 16 < V <= 25.  wg_frag: the Kt = 1 MFMA-fragment image of W'[co][p*64+ci] = W[p*64+co][ci] with
 * the columns of every 16-wide group permuted (realtime-st-gcn_amd/native.py pack_gcn_weight):
 * W''[c][16m + 8h + j] = W'[c][16m + 8(j/4) + 4h + j%4] (h < 2, j < 8); wt_frag: the stgcn_pack_weight_frag image
 * of the temporal weight [9][64][64]; gbias: the conv bias through A [V][64] (or NULL); ln*_g / ln*_b: the
 * LayerNorm([64,1,V]) parameters TRANSPOSED to [V][64] fp32.
 * Replaces: StgcnLayer.forward (models/stgcn/stgcn.py:181-193) of a LayerNorm layer. */
typedef struct {
  const void* x;         /* bf16 rows [N][T][V][x_ld], 64 channels */
  void* z;               /* bf16 rows [N][T][V][z_ld]: the layer output y */
  const void* wg_frag;
  const float* A;        /* [P][V][V] fp32 (A * edge importance) */
  const float* gbias;    /* [V][64] or NULL */
  const void* wt_frag;
  const float* tbias;    /* [64] or NULL */
  int N, T, V, P, x_ld, z_ld;
  const float* ln1_g;
  const float* ln1_b;
  const float* ln2_g;
  const float* ln2_b;
  int residual, pad_;
  /* training forward (all four set, or all NULL for inference): what the layer's backward (StgcnLayerFunction's
   * unfused LN backward) reads besides y — g_out: the graph-conv output incl. its bias (pre-LN1) rows
   * [N][T][V][g_ld]; u_out: the temporal-conv output incl. its bias (pre-LN2) rows, u_ld; st1_out / st2_out:
   * per-frame LayerNorm statistics (mean, 1/sqrt(unbiased var + 1e-5)) of g and u, float2 [N*T] —
   * stgcn_ln_stats's layout, computed here from the fp32 values before their bf16 rounding. */
  void* g_out;
  void* u_out;
  float* st1_out;
  float* st2_out;
  int g_ld, u_ld;
  /* optional with the training outputs (NULL otherwise): h = relu(LN1(g)) rows, h_ld — the temporal conv's input,
   * which the layer's weight gradient reads (saves recomputing it in the backward) */
  void* h_out;
  int h_ld, pad2_;
} stgcn_layer_fused_desc;

int stgcn_layer_fused_fwd(const stgcn_layer_fused_desc* d, void* stream);

/* Segment metrics of one trial (evaluation): labels / pred int64 [L] framewise classes (device).
 * out fp32 [K + 1]: F1@overlap[k] (utils/metrics/f1.py:14-52; NaN when the trial has no hit, as the
 * reference) and the segmental edit score out[K] (utils/metrics/edit.py:10-33); confusion (int64 [C][C],
 * [predicted][label], or NULL) += the framewise counts (utils/metrics/confusion.py:10-29).  overlap: fp32
 * [K] device, K <= 8; work: stgcn_segment_metrics_workspace(L) bytes; status (device int): 0 ok, 1 more than
 * 8192 segments in both sequences (edit score not computed).  One wave; bit-identical to the reference. */
long stgcn_segment_metrics_workspace(int L);
int stgcn_segment_metrics(const long* labels, const long* pred, int L, int C, const float* overlap, int K, void* work,
                          long long* confusion, float* out, int* status, void* stream);

/* RT-ST-GCN per-frame inference (config 3; rt_fused.hip), fp32, batch 1, rows [V][C] of one frame:
 *   stgcn_rt_frame_in_f: x (1,F,1,V) -> LayerNorm([F,1,V]) (ln_w/ln_b [F*V], element c*V+v) -> fcn_in
 *                        (w [C0][F], b [C0]) -> out [V][C0], 1 <= F <= 16           (rtstgcn.py:103,140-143)
 *   stgcn_rt_frame_in  : the same with F = 3
 *   stgcn_rt_frame_gcn : OnlineLayer's conv1x1 + A-mix (A [P][V][V] = graph * importance, w [P*Cout][Cin],
 *                        bias2d [V][Cout] = the conv bias through A) and AggregateStgcn's FIFO step
 *                        (fifo [S*(K-1)+1][V][Cout], acc [S][V][Cout], idx int[2] = (fifo, acc) indices,
 *                        read only) -> a_out [V][Cout]; wr [Cout][Cin] (or NULL): the residual 1x1 conv
 *                        (no bias) -> r_out                                    (rtstgcn.py:528-537,591-627)
 *   stgcn_rt_frame_norm: y = relu(relu(LN(a)) + res) (res_mode 1: res = x, 2: res = LN_r(r)) or relu(LN(a))
 *                        (res_mode 0); LN per frame over C*V, unbiased; advances idx   (rtstgcn.py:538-553)
 *   stgcn_rt_frame_out : mean over V -> fcn_out (w [K][C], b [K]) -> out [K]          (rtstgcn.py:149-153) */
int stgcn_rt_frame_in(const float* x, int V, const float* ln_w, const float* ln_b, const float* w, const float* b, int C0,
                      float* out, void* stream);
int stgcn_rt_frame_in_f(const float* x, int F, int V, const float* ln_w, const float* ln_b, const float* w, const float* b,
                        int C0, float* out, void* stream);
int stgcn_rt_frame_gcn(const float* x, int V, int Cin, int Cout, int P, const float* A, const float* w, const float* bias2d,
                       float* fifo, float* acc, const int* idx, const float* wr, float* a_out, float* r_out,
                       void* stream);
int stgcn_rt_frame_norm(const float* a, const float* ln_w, const float* ln_b, int res_mode, const float* res,
                        const float* lnr_w, const float* lnr_b, int V, int C, int* idx, int fifo_size, int S, float* y,
                        void* stream);
int stgcn_rt_frame_out(const float* x, int V, int C, const float* w, const float* b, int K, float* out, void* stream);

/* The whole per-frame step of a LayerNorm RT-ST-GCN (Model.forward after prepare_benchmark, rtstgcn.py:130-153
 * with every OnlineLayer, rtstgcn.py:528-553 + 591-627) as ONE persistent launch (rt_fused.hip): stgcn_rt_frame_in,
 * then per layer stgcn_rt_frame_gcn's arithmetic spread over `blocks` workgroups (channel pairs), an in-launch grid
 * barrier (agent-scope release / acquire on a counter), stgcn_rt_frame_norm's arithmetic redundantly in every
 * workgroup (the next layer's input stays in LDS), the FIFO indices advanced, and stgcn_rt_frame_out.  Same math as
 * the four entry points above (LN sums in another fixed order).  Per layer: a_buf / r_buf [V][Cout] device scratch
 * (r_buf only when res_mode == 2), wr NULL unless res_mode == 2; lnr_w / lnr_b only for res_mode 2.
 * sync: 16 device bytes, zeroed by this call (a memset on the stream ahead of the launch) — the barrier counter;
 * status: a device int the kernel sets to 1 if a barrier wait gave up (bounded spin; never reset here).
 * Workgroups of 1024 threads; the hand-off of a / r between workgroups is write-through (sc1) stores and loads.
 * V <= 32, 4 <= C <= 256 (C % 4 == 0), V * C <= 7680, P <= 3, L <= STGCN_RT_MAX_LAYERS, blocks in [1, 256] (0 = 64). */
/* F, in every descriptor that carries an input head (stgcn_rt_frame_desc, stgcn_rt_streams_desc, stgcn_co_streams_desc,
 * stgcn_co_clip_desc, stgcn_co_streams_clip_desc, stgcn_rt_streams_clip_desc; additive to ABI 7): the input features per
 * joint, in_feat of LayerNorm([F,1,V]) and fcn_in.  0 is read as 3, so a zero-initialised descriptor filled as before
 * the field existed behaves as before; otherwise 1 <= F <= STGCN_MAX_IN_FEAT and F * V >= 2 (the variance is unbiased).
 * Anything else returns 1 before any launch. */
#define STGCN_MAX_IN_FEAT 16
#define STGCN_RT_MAX_LAYERS 12
typedef struct {
  int Cin, Cout, P, fifo_size, S, res_mode;
  const float* A;       /* [P][V][V] graph * importance */
  const float* w;       /* [P*Cout][Cin] */
  const float* bias2d;  /* [V][Cout] or NULL */
  const float* wr;      /* [Cout][Cin] residual conv (res_mode 2) or NULL */
  const float* ln_w;    /* [V][Cout]: the LayerNorm([Cout,1,V]) affine in the rows' layout (transposed) */
  const float* ln_b;
  const float* lnr_w;   /* residual LN (res_mode 2), [V][Cout] */
  const float* lnr_b;
  float* fifo;          /* [fifo_size][V][Cout] */
  float* acc;           /* [S][V][Cout] */
  int* idx;             /* int[2] (fifo, acc) */
  float* a_buf;         /* [V][Cout] hand-off scratch */
  float* r_buf;         /* [V][Cout] (res_mode 2) */
} stgcn_rt_layer;
typedef struct {
  int V, L, C0, K, blocks;
  int F;                /* input features per joint; 0 = 3 */
  const float* x;       /* (1,F,1,V) frame, element c*V+v */
  const float* ln_w;    /* [F*V] */
  const float* ln_b;
  const float* w_in;    /* [C0][F] */
  const float* b_in;    /* [C0] */
  const float* w_out;   /* [K][C_last] */
  const float* b_out;   /* [K] or NULL */
  float* out;           /* [K] */
  unsigned* sync;       /* 16 B, zeroed per call */
  int* status;
  stgcn_rt_layer layers[STGCN_RT_MAX_LAYERS];
} stgcn_rt_frame_desc;
int stgcn_rt_frame(const stgcn_rt_frame_desc* d, void* stream);

/* A batch of B independent skeleton streams of the same LayerNorm RT-ST-GCN, each advanced by one frame in ONE launch
 * (rt_streams.hip; additive to ABI 7).  One workgroup of 512 threads per stream runs stgcn_rt_frame's arithmetic for
 * its stream (input LayerNorm + fcn_in; per layer conv1x1, A-mix over P, FIFO step, residual, LayerNorm, ReLU, index
 * advance; pool + fcn_out) with the layer input / output in LDS: no workgroup waits on another (no grid barrier, no
 * atomics, no cooperative launch), so B may exceed the CU count.  The conv and the A-mix run on the fp32 matrix cores
 * (v_mfma_f32_32x32x2_f32, exact fp32 products, fixed summation order; LayerNorm statistics two-pass in a fixed
 * order): a stream's result does not depend on B, on its slot or on the other streams.
 * dtype 1 (bf16 operands): the conv and the residual conv run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; the
 * layer's input rows are rounded to bf16 (nearest even) as the A fragments are loaded and wp / wrp are bf16 images.
 * Everything after the conv accumulators (A-mix, bias2d, FIFO step and state, LayerNorm, residual add, ReLU, the heads)
 * is fp32 as with dtype 0, the identity residual reads the unrounded input, and the state buffers are the same.  Any
 * other dtype returns 2 (unsupported dtype) before any launch.
 * State is stream-major and updated in place: fifo [B][fifo_size][V][Cout], acc [B][S][V][Cout], idx [B][2].
 * active [B] (device int32, read by the kernel): 0 = skip (state untouched, the out row written as zeros), 2 = restart
 * then step (FIFO, accumulators and indices taken as zero before this frame; the kernel clears them), any other
 * value = step.
 * wp: stgcn_rt_streams_pack_weight(w [P*Cout][Cin], groups = P, rows = Cout) — per partition the MFMA B-fragment image
 * [Cout/32 tiles][Cin/16 k-steps][64 lanes][8] of stgcn_co_pack_weight; wrp: the same of wr [Cout][Cin] (groups = 1),
 * res_mode 2 only.  stgcn_rt_streams_pack_weight_as(..., dtype, ...) writes the same image in dtype (0: fp32, identical
 * to stgcn_rt_streams_pack_weight; 1: bf16, rounded to nearest even); the element count is
 * stgcn_rt_streams_pack_elems(rows, Cin) per group for both.  The unpacked weights are not read.
 * Limits of stgcn_rt_frame: 2 <= V <= 32, 4 <= C <= 256 (C % 4 == 0), V * C <= 7680, P <= 3, L <= STGCN_RT_MAX_LAYERS,
 * res_mode 1 needs Cin == Cout; B >= 1.  A NULL required pointer or a shape outside the limits returns 1 before any
 * launch. */
typedef struct {
  int Cin, Cout, P, fifo_size, S, res_mode;
  const float* A;       /* [P][V][V] graph * importance */
  const void* wp;       /* packed conv weight, P * stgcn_rt_streams_pack_elems(Cout, Cin) elements of desc.dtype */
  const float* bias2d;  /* [V][Cout] or NULL */
  const void* wrp;      /* packed residual conv weight (res_mode 2) of desc.dtype, or NULL */
  const float* ln_w;    /* [V][Cout], as stgcn_rt_layer */
  const float* ln_b;
  const float* lnr_w;   /* residual LN (res_mode 2), [V][Cout] */
  const float* lnr_b;
  float* fifo;          /* [B][fifo_size][V][Cout] */
  float* acc;           /* [B][S][V][Cout] */
  int* idx;             /* [B][2] (fifo, acc) */
} stgcn_rt_streams_layer;
typedef struct {
  int V, L, C0, K, B;
  int dtype;            /* conv operand type: 0 fp32, 1 bf16 (element type of every layer's wp / wrp) */
  int F;                /* input features per joint; 0 = 3 */
  const float* x;       /* [B][F][V] */
  const int* active;    /* [B] */
  const float* ln_w;    /* [F*V] */
  const float* ln_b;
  const float* w_in;    /* [C0][F] */
  const float* b_in;    /* [C0] */
  const float* w_out;   /* [K][C_last] */
  const float* b_out;   /* [K] or NULL */
  float* out;           /* [B][K] */
  stgcn_rt_streams_layer layers[STGCN_RT_MAX_LAYERS];
} stgcn_rt_streams_desc;
long stgcn_rt_streams_pack_elems(int rows, int Cin);
int stgcn_rt_streams_pack_weight(const float* w, int groups, int rows, int Cin, float* dst, void* stream);
int stgcn_rt_streams_pack_weight_as(const float* w, int groups, int rows, int Cin, void* dst, int dtype, void* stream);
int stgcn_rt_streams(const stgcn_rt_streams_desc* d, void* stream);

/* CoST-GCN per-frame inference (models/costgcn/costgcn.py:192-211; co_frame.hip), batch 1, one frame per call,
 * LayerNorm layers.  A layer keeps a ring of the last fifo = S*(Kt-1)+1 frames of ReLU(LN1(gcn(x))) (tcn.0 is per
 * frame, so its result is cached; an empty FIFO normalises to ReLU(tcn.0.bias), which the CALLER writes into every
 * slot before the first frame) and a ring of the last R = Kt/2+1 residual frames (zeros at the start), and every
 * frame evaluates the Kt-tap temporal convolution with dilation S over the ring: tap k meets the frame of age k*S.
 * One frame of one layer is the four calls, in this order, on one stream:
 *   stgcn_co_gcn    : z_buf = gcn(x, A) (w [P*Cout][Cin], bias2d [V][Cout] = the conv bias through A, or NULL),
 *                     r_buf = wr x + br (res_mode 2: the residual conv has a bias, costgcn.py:178-181)
 *   stgcn_co_push   : ring[head'] = ReLU(LN1(z_buf)) (dtype elements), res_ring[rhead'] = x (res_mode 1) |
 *                     LN_r(r_buf) (2), head' = (idx[0] + fifo - 1) % fifo, rhead' = (idx[1] + R - 1) % R
 *   stgcn_co_taps   : partial[s][v][co] = sum over K split s of wt . ring, K = Kt*Cout split into `splits` ranges of
 *                     16-element steps, grid (Cout/32 column tiles) x (splits); MFMA, fp32 accumulation
 *   stgcn_co_finish : y = relu(LN2(bt + sum_s partial[s]) + res_ring[(rhead' + Kt/2) % R]) (no residual term for
 *                     res_mode 0); idx = (head', rhead')
 * Hand-offs are kernel boundaries; no atomics: a stream replays bit-identically from the same ring state.
 * Rows are [V][C] fp32; LayerNorm affines are the (C,1,V) parameters as stored (element c*V + v); statistics per
 * frame over C*V values, unbiased variance, eps 1e-5.  dtype (0 fp32 | 1 bf16) is the element type of ring and wt
 * only.  wt: stgcn_co_pack_weight's image of the Conv2d weight [Cout][Cout][Kt] (stgcn_co_pack_elems elements).
 * splits: 0 = chosen so that the grid covers every CU (stgcn_co_splits returns the count used);
 * partial: stgcn_co_workspace bytes.
 * 2 <= V <= 32, P <= 3, channels % 4 == 0 and <= 256, odd Kt <= 69, S in {1, 2}, res_mode 1 needs Cin == Cout;
 * anything else (or a NULL required pointer) returns 1 before any launch. */
typedef struct {
  int V, Cin, Cout, P, Kt, S, res_mode, dtype, splits, pad_;
  const float* x;       /* [V][Cin] the layer's input frame */
  const float* A;       /* [P][V][V] graph * importance */
  const float* w;       /* [P*Cout][Cin] gcn.conv */
  const float* bias2d;  /* [V][Cout] or NULL */
  const float* wr;      /* [Cout][Cin] residual.0 (res_mode 2) */
  const float* br;      /* [Cout] or NULL */
  const float* ln1_w;   /* tcn.0 */
  const float* ln1_b;
  const float* ln2_w;   /* tcn.3 */
  const float* ln2_b;
  const float* lnr_w;   /* residual.1 (res_mode 2) */
  const float* lnr_b;
  const void* wt;       /* packed tcn.2 weight, dtype elements */
  const float* bt;      /* [Cout] tcn.2 bias or NULL */
  void* ring;           /* [fifo][V][Cout] dtype elements */
  float* res_ring;      /* [Kt/2+1][V][Cout] */
  int* idx;             /* int[2]: slot of the newest frame in ring, res_ring */
  float* z_buf;         /* [V][Cout] */
  float* r_buf;         /* [V][Cout] (res_mode 2) */
  float* partial;       /* [splits][V][Cout] */
  float* y;             /* [V][Cout] */
} stgcn_co_layer;
long stgcn_co_pack_elems(int Cout, int C, int Kt);
int stgcn_co_pack_weight(const float* w, int Cout, int C, int Kt, void* dst, int dtype, void* stream);
int stgcn_co_splits(const stgcn_co_layer* d, void* stream);
long stgcn_co_workspace(const stgcn_co_layer* d, void* stream);
int stgcn_co_gcn(const stgcn_co_layer* d, void* stream);
int stgcn_co_push(const stgcn_co_layer* d, void* stream);
int stgcn_co_taps(const stgcn_co_layer* d, void* stream);
int stgcn_co_finish(const stgcn_co_layer* d, void* stream);

/* CoST-GCN per-frame inference for B independent streams (co_streams.hip): one call advances every active stream by one
 * frame through the whole network.  Per stream the arithmetic is stgcn_co_layer's four stages (gcn, push, taps,
 * finish) between an input head (LayerNorm([F,1,V]) + fcn_in) and an output head (mean over V + fcn_out); every
 * hand-off is a kernel boundary, no atomics on floating-point data, no cooperative launch.
 * State is stream-major and updated in place: ring [B][fifo][V][Cout] (dtype elements, fifo = S*(Kt-1)+1), res_ring
 * [B][Kt/2+1][V][Cout] fp32, idx [B][2].  active [B] (device int32, read by the kernels): 0 = skip (the stream's state
 * untouched, no ring reads, its out row written as zeros), 2 = restart then step (the kernels make every ring slot
 * ReLU(ln1_b), the residual ring and idx zero, then push this frame: the caller need not initialise a stream it
 * restarts), any other value = step.
 * The tap stage runs groups of 4 active streams against one read of the weight panel (stgcn_co_pack_weight's image,
 * unchanged); wp / wrp are stgcn_rt_streams_pack_weight's images of gcn.conv (groups = P, rows = Cout) and residual.0
 * (groups = 1).  splits: 0 = the default, a function of (Cout, Kt) alone; stgcn_co_streams_splits returns the count
 * used for layer l, stgcn_co_streams_workspace the bytes of that layer's `partial`.  With the same split counts a
 * stream's outputs are bit-identical whatever B, its slot and the other streams' codes are.
 * Limits per layer are stgcn_co_layer's (2 <= V <= 32, P <= 3, channels % 4 == 0 and <= 256, odd Kt <= 69, S in
 * {1, 2}, res_mode 1 needs Cin == Cout), layers[l].Cin == layers[l-1].Cout (C0 for l = 0), 1 <= L <=
 * STGCN_RT_MAX_LAYERS, B >= 1, K >= 1; dtype 0 fp32 | 1 bf16 (ring and wt only).  Anything else, or a NULL required
 * pointer, returns 1 (2 for the dtype) before any launch; the two queries return -1. */
typedef struct {
  int Cin, Cout, P, Kt, S, res_mode, splits, pad_;
  const float* A;       /* [P][V][V] graph * importance */
  const float* wp;      /* packed gcn.conv weight, P * stgcn_rt_streams_pack_elems(Cout, Cin) floats */
  const float* bias2d;  /* [V][Cout] or NULL */
  const float* wrp;     /* packed residual.0 weight (res_mode 2) */
  const float* br;      /* [Cout] or NULL */
  const float* ln1_w;   /* tcn.0, (C,1,V) as stored */
  const float* ln1_b;
  const float* ln2_w;   /* tcn.3 */
  const float* ln2_b;
  const float* lnr_w;   /* residual.1 (res_mode 2) */
  const float* lnr_b;
  const void* wt;       /* packed tcn.2 weight, dtype elements */
  const float* bt;      /* [Cout] tcn.2 bias or NULL */
  void* ring;           /* [B][fifo][V][Cout] dtype elements */
  float* res_ring;      /* [B][Kt/2+1][V][Cout] */
  int* idx;             /* [B][2] */
  float* z_buf;         /* [B][V][Cout] scratch */
  float* r_buf;         /* [B][V][Cout] scratch (res_mode 2) */
  float* partial;       /* [B][splits][V][Cout] scratch */
  float* y;             /* [B][V][Cout] the layer's output rows */
} stgcn_co_streams_layer;
typedef struct {
  int B, V, L, C0, K, dtype;
  int F;                /* input features per joint; 0 = 3 */
  const float* x;       /* [B][F][V] */
  const int* active;    /* [B] */
  const float* ln_w;    /* [F*V] */
  const float* ln_b;
  const float* w_in;    /* [C0][F] */
  const float* b_in;    /* [C0] */
  const float* w_out;   /* [K][C_last] */
  const float* b_out;   /* [K] or NULL */
  float* h0;            /* [B][V][C0] scratch: the first layer's input rows */
  int* order;           /* [B + 1] scratch: the active count, then the active streams' slots */
  float* out;           /* [B][K] */
  stgcn_co_streams_layer layers[STGCN_RT_MAX_LAYERS];
} stgcn_co_streams_desc;
int stgcn_co_streams_splits(const stgcn_co_streams_desc* d, int layer);
long stgcn_co_streams_workspace(const stgcn_co_streams_desc* d, int layer);
int stgcn_co_streams(const stgcn_co_streams_desc* d, void* stream);

/* CoST-GCN clip inference: T consecutive frames of ONE stream per call, on the rings stgcn_co_layer's calls use
 * (ring, res_ring, idx: the same buffers, the same layout).  The contract:
 *   1. out[t] is what the per-frame calls would give for frame t, the T frames fed one at a time from the state the
 *      rings hold on entry (equal within rounding: the sums below have an order of their own);
 *   2. on return the rings and idx are what those T calls would have left: new frame t in ring slot
 *      (idx0 - 1 - t) mod fifo, its residual row in res_ring slot (idx1 - 1 - t) mod R, idx moved by -T (mod fifo, R);
 *   3. per-frame calls, clips of any T and a re-initialisation of the rings by the caller can be mixed on one stream.
 * It is the B = 1 case of stgcn_co_streams_clip (below, co_streams_clip.hip): the same launches, 2 + 5 L of them, on
 * this descriptor's pointers, with no codes and no lengths: the stream advances by all T frames from the state as it
 * is.  The stages, the order of every sum and the split count (stgcn_co_clip_splits) are described there.  Hence
 * chunk invariance: a clip of T frames and any split of it into consecutive clips (T = 1 included) give the same bits
 * in out, ring, res_ring and idx; a captured graph of a clip replays bit-identically.
 * x: the (F, T, V) fp32 clip, channel c of frame t at x[c * x_stride + t * V] (x_stride >= T * V: a dense clip has
 * x_stride = T * V, a chunk of a longer clip keeps the whole clip's stride).  out: [T][K].
 * wt: stgcn_co_pack_weight's image; wp / wrp: stgcn_rt_streams_pack_weight's (groups = P / 1), fp32.
 * dtype 0 fp32 | 1 bf16: the element type of wt, ring and hist only.
 * Limits per layer are stgcn_co_layer's, layers[l].Cin == layers[l-1].Cout (C0 for l = 0), 1 <= L <=
 * STGCN_RT_MAX_LAYERS, K >= 1, 1 <= T <= STGCN_CO_CLIP_MAX_T (longer clips: consecutive calls).  Anything else, or a
 * NULL required pointer, returns 1 (2 for the dtype) before any launch; the two queries return -1.  The scratch
 * buffers of different layers may alias each other (each is dead once its layer's state launch has run), except y of
 * neighbouring layers. */
#define STGCN_CO_CLIP_MAX_T 256
/* A layer of either clip descriptor; B = 1 for stgcn_co_clip. */
typedef struct {
  int Cin, Cout, P, Kt, S, res_mode, splits, pad_;
  const float* A;       /* [P][V][V] graph * importance */
  const float* wp;      /* packed gcn.conv weight, P * stgcn_rt_streams_pack_elems(Cout, Cin) floats */
  const float* bias2d;  /* [V][Cout] or NULL */
  const float* wrp;     /* packed residual.0 weight (res_mode 2) */
  const float* br;      /* [Cout] or NULL */
  const float* ln1_w;   /* tcn.0, (C,1,V) as stored */
  const float* ln1_b;
  const float* ln2_w;   /* tcn.3 */
  const float* ln2_b;
  const float* lnr_w;   /* residual.1 (res_mode 2) */
  const float* lnr_b;
  const void* wt;       /* packed tcn.2 weight, dtype elements */
  const float* bt;      /* [Cout] tcn.2 bias or NULL */
  void* ring;           /* [B][fifo][V][Cout] dtype elements: the state, as in stgcn_co_layer / _co_streams_layer */
  float* res_ring;      /* [B][Kt/2+1][V][Cout] */
  int* idx;             /* [B][2] */
  float* z_buf;         /* [B][T][V][Cout] scratch */
  float* r_buf;         /* [B][T][V][Cout] scratch (res_mode 2) */
  void* hist;           /* [B][fifo-1 + T][V][Cout] scratch, dtype elements */
  float* resq;          /* [B][Kt/2 + T][V][Cout] scratch */
  float* partial;       /* [B][T][splits][V][Cout] scratch */
  float* y;             /* [B][T][V][Cout] the layer's output rows */
} stgcn_co_clip_layer;
typedef stgcn_co_clip_layer stgcn_co_streams_clip_layer;
typedef struct {
  int T, V, L, C0, K, dtype;
  int F;                /* input features per joint; 0 = 3 */
  long x_stride;        /* elements between two channels of x */
  const float* x;       /* the clip, see above */
  const float* ln_w;    /* [F*V] */
  const float* ln_b;
  const float* w_in;    /* [C0][F] */
  const float* b_in;    /* [C0] */
  const float* w_out;   /* [K][C_last] */
  const float* b_out;   /* [K] or NULL */
  float* h0;            /* [T][V][C0] scratch: the first layer's input rows */
  float* out;           /* [T][K] */
  stgcn_co_clip_layer layers[STGCN_RT_MAX_LAYERS];
} stgcn_co_clip_desc;
int stgcn_co_clip_splits(const stgcn_co_clip_desc* d, int layer);
long stgcn_co_clip_workspace(const stgcn_co_clip_desc* d, int layer);  /* bytes of layers[layer].partial */
int stgcn_co_clip(const stgcn_co_clip_desc* d, void* stream);

/* CoST-GCN clip inference for B independent streams (co_streams_clip.hip): one call advances stream b by n_b frames,
 * on the stream-major state of stgcn_co_streams (ring [B][fifo][V][Cout], res_ring [B][Kt/2+1][V][Cout], idx [B][2]:
 * the same buffers, so per-frame ticks and clips mix on one batch).  Per stream the contract is stgcn_co_clip's, with
 * n_b in the place of T.  Per call: an input head and an output head per frame, and per layer five launches, every
 * hand-off a kernel boundary, no atomics, no workgroup waiting on another:
 *   gcn    : z_buf[b][t], r_buf[b][t] as stgcn_co_streams computes them for a stream (packed wp / wrp)
 *   push   : hist[b][fifo-1+t] = ReLU(LN1(z_buf[b][t])) (dtype elements), resq[b][Kt/2+t] = the residual row of frame
 *            t; the same launch copies the fifo-1 newest ring frames and the Kt/2 newest res_ring rows, oldest first,
 *            into hist[b][0 .. fifo-1) and resq[b][0 .. Kt/2).  It is the only launch that reads the rings and writes
 *            none.
 *   taps   : partial[b][t][s][v][co] = sum over K split s of wt . hist, tap k of frame t = hist[b][fifo-1 + t - k*S]:
 *            one GEMM with n_b*V dense rows per stream; a workgroup holds 4 row tiles of 32 against one load of each
 *            weight fragment
 *   finish : y[b][t] = relu(LN2(bt + sum_s partial[b][t][s]) + resq[b][t]); idx[b] advanced
 *   state  : the last min(n_b, fifo) hist frames and min(n_b, Kt/2+1) resq rows into their ring slots.  It is the only
 *            launch that writes the rings, and it runs after the taps and finish launches: a new frame never replaces
 *            a carried frame that an earlier frame of the clip still has to read.
 * Order of every sum: the 16-element k-steps of a K split in sequence within a wave (with Cout < 256 the 8 / (Cout/32)
 * waves of a column tile interleave the split's k-steps and are summed in index order), then the splits in index
 * order, then bt; LayerNorm statistics as in the per-frame calls (two passes, 1024 threads, fixed order).  The split
 * count (stgcn_co_streams_clip_splits, stgcn_co_clip_splits) is a function of (Cout, Kt) and layers[l].splits (> 0
 * forces it) alone, never of B, T, t0 or the device.  So a stream's out, ring, res_ring and idx are bit-identical to
 * stgcn_co_clip's on the same frames from the same state, whatever B, its slot, T, the other streams' codes, lengths
 * and contents, and however the frames are split into consecutive calls.
 * active [B] and lengths [B] are device int32, read by the kernels (a captured call replays with other values):
 *   n_b = clamp(lengths[b] - t0, 0, T) frames are consumed, frames 0 .. n_b-1 of this call's T;
 *   code 0: skip — state untouched, no ring reads, every out row of the stream zero;
 *   code 2 and t0 == 0: restart, then advance — the carried history is the empty FIFO (ReLU(ln1_b) rows, zero residual
 *     rows, idx taken as 0), nothing of the old state is read, and the ring slots the clip does not reach are written
 *     with the empty rows (n_b = 0 leaves exactly a re-initialised stream);
 *   any other code (and code 2 with t0 > 0): advance from the state as it is; n_b = 0 leaves it untouched.
 * t0 is the position of this call's first frame in the caller's clip: a clip longer than T runs as consecutive calls
 * with t0 = 0, T, 2T, ..., x and out moved on by the caller, lengths and active unchanged.
 * out rows t >= n_b are written as zeros.  Launches: 2 + 5 L whatever B and T are, grids sized from (B, T); a workgroup
 * whose frame, row tile or ring slot lies beyond n_b returns after reading the code and the length.
 * x: stream b's channel c of frame t at x[b * x_bstride + c * x_stride + t * V]; out: stream b's row t at
 * out[b * out_bstride + t * K].  Scratch is stream-major; different layers' scratch may alias as in stgcn_co_clip.
 * Limits are stgcn_co_clip's plus B >= 1; anything else, or a NULL required pointer (active and lengths included),
 * returns 1 (2 for the dtype) before any launch; the two queries return -1. */
typedef struct {
  int B, T, t0, V, L, C0, K, dtype;
  int F;                /* input features per joint; 0 = 3 */
  long x_stride;        /* elements between two channels of x */
  long x_bstride;       /* elements between two streams of x */
  long out_bstride;     /* elements between two streams of out */
  const float* x;       /* this call's first frame of stream 0, see above */
  const int* active;    /* [B] */
  const int* lengths;   /* [B] */
  const float* ln_w;    /* [F*V] */
  const float* ln_b;
  const float* w_in;    /* [C0][F] */
  const float* b_in;    /* [C0] */
  const float* w_out;   /* [K][C_last] */
  const float* b_out;   /* [K] or NULL */
  float* h0;            /* [B][T][V][C0] scratch: the first layer's input rows */
  float* out;           /* stream b's [T][K] at out + b * out_bstride */
  stgcn_co_streams_clip_layer layers[STGCN_RT_MAX_LAYERS];
} stgcn_co_streams_clip_desc;
int stgcn_co_streams_clip_splits(const stgcn_co_streams_clip_desc* d, int layer);
long stgcn_co_streams_clip_workspace(const stgcn_co_streams_clip_desc* d, int layer);  /* bytes of layers[layer].partial */
int stgcn_co_streams_clip(const stgcn_co_streams_clip_desc* d, void* stream);

/* RT-ST-GCN clip inference for B independent streams (rt_streams_clip.hip): one call advances stream b by n_b frames
 * on the stream-major state of stgcn_rt_streams (fifo [B][fifo_size][V][Cout], acc [B][S][V][Cout], idx [B][2]: the
 * same buffers, so per-frame ticks and clips mix on one batch).  layers[] are stgcn_rt_streams_layer as that call takes
 * them (the same packed weight images of desc.dtype, the same [V][Cout] norm rows).
 * active [B] and lengths [B] are device int32, read by the kernels (a captured call replays with other values):
 *   n_b = clamp(lengths[b] - t0, 0, T) frames are consumed, frames 0 .. n_b-1 of this call's T;
 *   code 0: skip — state untouched and unread, every out row of the stream zero;
 *   code 2 and t0 == 0: restart, then advance — fifo, acc and idx are taken as zero, nothing of the old state is read,
 *     and the slots the clip does not reach are cleared (n_b = 0 leaves exactly a reset stream);
 *   any other code (and code 2 with t0 > 0): advance from the state as it is; n_b = 0 leaves it untouched.
 * t0 is the position of this call's first frame in the caller's clip: a clip longer than T runs as consecutive calls
 * with t0 = 0, T, 2T, ..., x and out moved on by the caller, lengths and active unchanged.
 * Per frame the arithmetic is stgcn_rt_streams's (the conv, A-mix, bias2d, LayerNorm, residual and head stages are the
 * same device functions with the same block size); the FIFO step a = acc[ai] + z - fifo[fi]; acc[ai] = a; fifo[fi] = z
 * runs in exactly this association frame after frame, one thread per 4 elements of a stream for the whole call.  The
 * order of every sum depends on the network only: a stream's out, fifo, acc and idx are bit-identical whatever B, its
 * slot, T, t0 chunking and the other streams' codes, lengths and contents are.
 * Launches: 2 L + 1 whatever B and T are (frame kernel 0: input head + layer 0's conv; scan of layer l; frame kernel
 * l + 1: layer l's norms and residual + layer l+1's conv, the last one the output head), grids sized from (B, T); a
 * workgroup whose stream is skipped or whose frame lies beyond n_b returns after reading the code and the length.
 * out rows t >= n_b are written as zeros.  x: stream b's channel c of frame t at x[b * x_bstride + c * x_stride + t * V];
 * out: stream b's row t at out[b * out_bstride + t * K].  Scratch: xb, z, r, a, each [B][T][fstride] floats with
 * fstride >= the largest V * C of the network (C0 included) and fstride % 4 == 0; shared by all layers.
 * Limits are stgcn_rt_streams's, plus 1 <= T <= STGCN_RT_CLIP_MAX_T, t0 >= 0 and B * T < 2^31.  A NULL required pointer
 * (active and lengths included; r only with a res_mode 2 layer) or a shape outside the limits returns 1 (2 for the
 * dtype) before any launch. */
#define STGCN_RT_CLIP_MAX_T 256
typedef struct {
  int B, T, t0, V, L, C0, K, dtype;
  int F;                /* input features per joint; 0 = 3 */
  long x_stride;        /* elements between two channels of x */
  long x_bstride;       /* elements between two streams of x */
  long out_bstride;     /* elements between two streams of out */
  long fstride;         /* elements between two frames of the scratch buffers */
  const float* x;       /* this call's first frame of stream 0, see above */
  const int* active;    /* [B] */
  const int* lengths;   /* [B] */
  const float* ln_w;    /* [F*V] */
  const float* ln_b;
  const float* w_in;    /* [C0][F] */
  const float* b_in;    /* [C0] */
  const float* w_out;   /* [K][C_last] */
  const float* b_out;   /* [K] or NULL */
  float* xb;            /* [B][T][fstride] scratch: the current layer's input rows [V][C] */
  float* z;             /* [B][T][fstride] scratch: bias2d + the A-mixed conv */
  float* r;             /* [B][T][fstride] scratch: the residual conv (res_mode 2 layers), or NULL */
  float* a;             /* [B][T][fstride] scratch: the running box sum per frame */
  float* out;           /* stream b's [T][K] at out + b * out_bstride */
  stgcn_rt_streams_layer layers[STGCN_RT_MAX_LAYERS];
} stgcn_rt_streams_clip_desc;
int stgcn_rt_streams_clip(const stgcn_rt_streams_clip_desc* d, void* stream);

/* Snapshot and restore of live streams of the stream batches (stream_state.hip; additive to ABI 7): the per-layer state
 * of stgcn_rt_streams (kind 0: s0 = fifo [B][n0 = fifo_size][V][C], s1 = acc [B][n1 = S][V][C]) or of stgcn_co_streams
 * (kind 1: s0 = ring [B][n0 = S*(Kt-1)+1][V][C] in dtype elements, s1 = res_ring [B][n1 = Kt/2+1][V][C]) and idx [B][2],
 * to and from the canonical image.  A snapshot is snap [n][E] fp32: row i is stream slots[i], layer-major, and each
 * state tensor t of a layer is stored rotated along its slot axis so that it is the original with stored index 0:
 *   snap[i][off_t + k * V*C + e] = tensor_t[slots[i]][(idx[slots[i]][t] + k) % n_t][e],   k < n_t, e < V*C.
 * Every per-frame and clip kernel addresses a slot only relative to the stored index, so a stream continued from its
 * canonical image with idx = (0, 0) returns the same bits.  No value is recomputed (the rt accumulators are copied).
 * The element type of s0 is bf16 for kind 1 with dtype 1 and fp32 otherwise (the rt-st-gcn state is fp32 in both of its
 * dtypes); a bf16 value is widened exactly on export and an image value is rounded to nearest even on import.
 *   stgcn_stream_state_export: snap[i] = the canonical image of stream slots[i]; state and idx are not written.
 *   stgcn_stream_state_import: stream slots[i] = snap[i] at rotation 0, idx[slots[i]] = (0, 0); other streams are not
 *                              touched.  Two entries of slots naming one stream make that stream's content undefined.
 * One launch each for all layers and all n streams, 256 threads per workgroup, 16-byte accesses on the [V][C] rows, no
 * atomics, no barrier between workgroups, no host synchronisation: slots (device int32 [n]) and idx are read by the
 * kernel, so a captured call replays with other slots.  An entry of slots outside [0, B) is skipped: its workgroups
 * return without touching memory (its export row stays as it was).
 * The image is dense: layers[0].off0 = 0, off1 = off0 + n0*V*C, the next layer's off0 = off1 + n1*V*C, E = the end.
 * Limits: 1 <= L <= STGCN_RT_MAX_LAYERS, 2 <= V <= 32, C >= 4 and C % 4 == 0, n0, n1 >= 1, B >= 1, n >= 1, kind 0 | 1;
 * an offset or E that disagrees with the above, or a NULL pointer, returns 1 and a dtype other than 0 | 1 returns 2,
 * before any launch. */
#define STGCN_STREAM_STATE_RT 0
#define STGCN_STREAM_STATE_CO 1
typedef struct {
  void* s0;             /* fifo (kind 0, fp32) | ring (kind 1, dtype elements): [B][n0][V][C] */
  float* s1;            /* acc (kind 0) | res_ring (kind 1): [B][n1][V][C] */
  int* idx;             /* [B][2] */
  int C, n0, n1, pad_;
  long off0, off1;      /* first element of s0's / s1's part in a snapshot row */
} stgcn_stream_state_layer;
typedef struct {
  int kind, V, L, B, n, dtype;
  const int* slots;     /* [n] device: the streams, in snapshot row order */
  float* snap;          /* [n][E] device */
  long E;               /* elements per snapshot row */
  stgcn_stream_state_layer layers[STGCN_RT_MAX_LAYERS];
} stgcn_stream_state_desc;
int stgcn_stream_state_check(const stgcn_stream_state_desc* d);  /* the code either call would return, no launch */
int stgcn_stream_state_export(const stgcn_stream_state_desc* d, void* stream);
int stgcn_stream_state_import(const stgcn_stream_state_desc* d, void* stream);

/* MS-TCN stage (models/mstcn/mstcn.py:68-116; ms_stage.hip): SingleStage = conv_in 1x1, num_layers
 * DilatedResidualLayers (dilation 2^i), conv_out 1x1, forward and backward, batch 1.  Activations are fp32 rows
 * [L][V][F] (row r = t*V + v); dtype (0 fp32 | 1 bf16) is the type MFMA operands are rounded to and the element type
 * of the packed weights, of the saved hidden activation h and of its gradient g; accumulation is fp32 and the
 * residual stream stays fp32.  Every hand-off is a kernel boundary, no atomics: results are run-to-run identical.
 *
 * One layer with dilation dil (kernel 3, padding dil: nn.Conv2d(F, F, (3,1), padding=(dil,0), dilation=(dil,1)),
 * ReLU, nn.Conv2d(F, F, 1); dropout must be 0), R = L*V rows:
 *   stgcn_ms_layer_fwd : h = ReLU(b1 + sum_k W1_k x[r + (k-1)*dil*V]) (rows outside [0, R) are the zero padding),
 *                        y = x + b2 + W2 h; h is stored when h != NULL (training)
 *   stgcn_ms_layer_bwd : g = (W2^T dy) . [h > 0];  dx = dy + sum_k W1_k^T g[r - (k-1)*dil*V] (skipped when
 *                        dx == NULL);  grads = [dW1 (F,F,3) | db1 (F) | dW2 (F,F) | db2 (F)] summed in a fixed
 *                        order from stgcn_ms_wgrad_blocks(R) per-workgroup partials (part: that many times
 *                        4*F*F + 2*F floats)
 * wp: stgcn_ms_pack_layer's image of W1 (F,F,3,1) and W2 (F,F,1,1): four MFMA fragment-order panels (W1 tap-major,
 * W2, and both transposed), stgcn_ms_pack_elems(F) dtype elements; kernel != 3 is refused there.
 * F in {16, 32, 48, 64}; R % V == 0; R * dil <= INT_MAX; anything else returns 1 before any launch. */
typedef struct {
  int R, V, F, dil, dtype, pad_;
  const float* x;   /* [R][F] layer input */
  const void* wp;   /* packed weights */
  const float* b1;  /* [F] conv.0.bias */
  const float* b2;  /* [F] conv.2.bias */
  float* y;         /* [R][F] (forward) */
  void* h;          /* [R][F] dtype elements: written by the forward (or NULL), read by the backward */
  const float* dy;  /* [R][F] (backward) */
  void* g;          /* [R][F] dtype elements, backward workspace */
  float* dx;        /* [R][F] or NULL */
  float* part;      /* backward workspace */
  float* grads;     /* [4*F*F + 2*F] */
} stgcn_ms_layer;
long stgcn_ms_pack_elems(int F);
int stgcn_ms_pack_layer(const float* w1, const float* w2, int F, int kernel, void* dst, int dtype, void* stream);
int stgcn_ms_wgrad_blocks(int R);
int stgcn_ms_layer_fwd(const stgcn_ms_layer* d, void* stream);
int stgcn_ms_layer_bwd(const stgcn_ms_layer* d, void* stream);

/* The two ends of a stage, fp32, plain FMA code (widths <= 64):
 *   out[r][o] = b[o] + sum_i w[o][i] p[r][i],   p[r] = selector(mean_v in[r*pool + v]),   r < rows
 * stgcn_ms_in_*  : conv_in with the model's `refine` selector fused in front (mstcn.py:63): mode 0 none | 1 log-softmax
 *                  | 2 softmax over the I values of a row; pool == 1; O = filters.
 * stgcn_ms_out_* : conv_out with the mean over the V = pool <= 32 joints fused in front (mstcn.py:58; the mean
 *                  commutes with a 1x1 convolution); mode == 0; I = filters.
 * The forward stores p when p != NULL (the backward reads it).  The backward writes grads = [dw (O,I) | db (O)],
 * summed in a fixed order from stgcn_ms_lin_blocks(rows) partials (part: that many times O*I + O floats), and, when
 * din != NULL, din[r*pool + v] = J^T (w^T d[r]) / pool (J: the selector's Jacobian at p). */
typedef struct {
  int rows, pool, I, O, mode, pad_;
  const float* in;  /* [rows*pool][I] */
  const float* w;   /* [O][I] */
  const float* b;   /* [O] */
  float* out;       /* [rows][O] */
  float* p;         /* [rows][I] */
  const float* d;   /* [rows][O] gradient of out (backward) */
  float* din;       /* [rows*pool][I] or NULL */
  float* part;
  float* grads;     /* [O*I + O] */
} stgcn_ms_lin;
int stgcn_ms_lin_blocks(int rows);
int stgcn_ms_in_fwd(const stgcn_ms_lin* d, void* stream);
int stgcn_ms_in_bwd(const stgcn_ms_lin* d, void* stream);
int stgcn_ms_out_fwd(const stgcn_ms_lin* d, void* stream);
int stgcn_ms_out_bwd(const stgcn_ms_lin* d, void* stream);
/* The model's `out` selector on [rows][C] fp32 rows, C <= 64 (mstcn.py:40-45): y = log-softmax (mode 1) | softmax
 * (mode 2) of x, and dx from y and dy. */
int stgcn_ms_prob_fwd(const float* x, int rows, int C, int mode, float* y, void* stream);
int stgcn_ms_prob_bwd(const float* y, const float* dy, int rows, int C, int mode, float* dx, void* stream);

/* Window staging (window.hip): the first activation of a batch of sliding windows
 * (WindowSegment, utils/segment_generator.py:132-145) computed from the padded capture without forming the
 * windows.  x: fp32 [Cin][Lp][V] (the reference's padded (1, Cin, Lp, V) capture, processor.py:372-374),
 * Cin in {1,2,3,4,6,8}; windows n in [n0, n0+nw) hold frames [n, n+W) (n0 + nw + W - 1 <= Lp).
 *   stgcn_window_stats : norm_in statistics of the windowed batch.  mode 0, BatchNorm1d(V*Cin) (batchnorm.py:
 *       13-23): out = float4 (count, mean, M2, 0) partials [stgcn_window_stat_blocks(nw, W)][V*Cin], each
 *       frame weighted by the number of windows holding it -> stgcn_bn_finalize(nb, ld = C = V*Cin);
 *       mode 1, LayerNorm([Cin,1,V]) (layernorm.py:22-28): out = float2 (mean, rstd) per frame [nw+W-1],
 *       unbiased variance.
 *   stgcn_window_expand: out rows (n, t, v) [nw][W][V], ld ldo, dtype: fcn_in(norm_in(x[:, n+t, v]))
 *       (stgcn.py:82-85) with w [Cout][Cin], bias [Cout] (or NULL).  mode 0: g/b = the folded affine
 *       (scale, shift) [V*Cin] of stgcn_bn_finalize, fst NULL; mode 1: g/b = gamma/beta [Cin*V] (element
 *       c*V+v), fst = the frame statistics.  Cout % (16 / element size) == 0.
 *   stgcn_window_grad  : from dy rows (the gradient of expand's output, ld ldd): dw [Cout][Cin], db [Cout],
 *       dgamma / dbeta (mode 0 [V*Cin] v*Cin+c with st = (mean, rstd) [V*Cin] of stgcn_bn_finalize; mode 1
 *       [Cin*V] with st = the frame statistics); any output may be NULL.  One pass over dy (windows folded
 *       onto frames); work: stgcn_window_grad_workspace bytes, no initialisation needed. */
int stgcn_window_stat_blocks(int nw, int W);
int stgcn_window_stats(const float* x, int Cin, int Lp, int V, int W, int n0, int nw, int mode, float eps, float* out,
                       void* stream);
int stgcn_window_expand(const float* x, int Cin, int Lp, int V, int W, int n0, int nw, int mode, const float* g,
                        const float* b, const float* fst, const float* w, const float* bias, int Cout, void* out,
                        int ldo, int dtype, void* stream);
long stgcn_window_grad_workspace(int nw, int W, int V, int Cin, int Cout);
int stgcn_window_grad(const void* dy, int ldd, int dtype, const float* x, int Cin, int Lp, int V, int W, int n0, int nw,
                      int mode, const float* st, const float* gamma, const float* beta, const float* w, int Cout,
                      void* work, float* dgamma, float* dbeta, float* dw, float* db, void* stream);

/* Batched weight preparation (prep.hip): every packed operand a model's layers read in one training step —
 * the GEMM packs and MFMA-fragment images of the temporal / residual / head 1x1 convs (stgcn_pack_weight,
 * _frag, _s2frag) and the graph conv's per-joint effective weights with the bias pushed through A
 * (stgcn_gconv_weights_bias), for the forward and the data gradient — in ONE launch instead of ~50
 * (stgcn.py:80-97 as a whole; replaces the per-layer packing of the reference's nn.Conv2d weights, which
 * PyTorch's own kernels read in place).  A job is one of those single-job entry points with the same
 * argument meaning:
 *   kind 0 (pack): src + strides (s0, s1, s2), Kt, Co, Ci -> dst [Kt][cp][kp] (dtype), and the fragment
 *                  image into dst_frag when non-NULL (cp % 32 == 0, kp % 16 == 0);
 *   kind 1 (stride-2 fold, bf16): src + strides, Co, Ci, trans -> dst (stgcn_pack_weight_s2frag);
 *   kind 2 (graph conv): A [P][V][V] (times the edge importance M [P][V][V] when non-NULL: the product the
 *                  model feeds the layer, formed here exactly as a rounded fp32 product), W = src
 *                  [P*Cout][Cin] (Co = Cout, Ci = Cin), nbr / deg support lists, trans, dst [V][J][R_pad]
 *                  [C_pad] (dtype), and for trans 0 with bconv non-NULL bias2d [V][Cout];
 *   kind 3 (graph-conv bias through A alone, the frame-kernel route): A (times M when non-NULL), bconv
 *                  [P*Cout] (Co = Cout) -> bias2d [V][Cout] = sum_p bconv[p*Cout+c] sum_v (A*M)[p][v][w]
 *                  (src = bconv, dst = bias2d, Ci = 1).
 * stgcn_prep_check validates a host-side job array and fills each job's thread count (threads);
 * stgcn_prep_run launches the jobs from a DEVICE copy of that array with block_start [njobs + 1] (device,
 * block_start[j] = first 256-thread block of job j, block_start[njobs] = nblocks). */
typedef struct {
  int kind, dtype, trans, Kt, Co, Ci, cp, kp;
  long s0, s1, s2, threads;
  const float* src;
  void* dst;
  void* dst_frag;
  const float* A;
  const float* M;
  const int* nbr;
  const int* deg;
  int P, V, J, R_pad, C_pad, pad_;
  const float* bconv;
  float* bias2d;
} stgcn_prep_job;
int stgcn_prep_check(stgcn_prep_job* jobs, int njobs);
int stgcn_prep_run(const stgcn_prep_job* jobs_dev, const long* block_start_dev, int njobs, long nblocks,
                   void* stream);

/* Adam over every parameter tensor of a model in one launch (adam.hip).
 * Replaces: the reference's optimizer step, torch.optim.Adam (processor.py:561, built at processor.py:579; optimizer
 * config learning_rate 5e-4, default betas / eps), with torch's update rule:
 *   g' = g + weight_decay * p;  m = lerp(m, g', 1 - b1);  v = b2 v + (1 - b2) g'^2;
 *   p += (-lr / (1 - b1^t)) * (m / (sqrt(v) / sqrt(1 - b2^t) + eps)),   t = the tensor's step count
 * (the default foreach implementation's operation order; hyper-parameters in double, as Python floats).
 * table_dev: device array of stgcn_adam_entry (p: the fp32 parameter, m / v: its moment slices, n elements,
 * b0 = first block of the tensor, b0 increasing, block counts from stgcn_adam_blocks(n); vec = 1 when p, m
 * and v are 16-B aligned).  grads: HOST array of ntensors device gradient pointers (NULL = no gradient:
 * the tensor is skipped, its step count unchanged).  steps: device float [nblocks], every block's copy of
 * its tensor's step count (zero-initialised; the caller reads a tensor's count at its first block). */
#define STGCN_ADAM_MAXT 256
typedef struct {
  float* p;
  float* m;
  float* v;
  long n, b0;
  int vec, pad_;
} stgcn_adam_entry;
long stgcn_adam_blocks(long n);
int stgcn_adam_step(const stgcn_adam_entry* table_dev, int ntensors, long nblocks, const float* const* grads,
                    float* steps, double lr, double beta1, double beta2, double eps, double weight_decay,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STGCN_AMD_H */
