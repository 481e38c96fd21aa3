// Host launchers of the kernel translation units, declared once: capi.cpp calls them and every .hip that
// defines one includes this header, so a prototype that drifts from its definition is a compile error.
// Grouped by the file that defines them.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/stgcn_amd.h"

// conv_rows.hip
int conv_rows_launch(const stgcn_conv_desc& a, int dtype, hipStream_t s);
int conv_rows_bn_tile(int cout);
int pack_weight_launch(const float* src, long s0, long s1, long s2, int Kt, int Co, int Ci, void* dst, int cp, int kp,
                       int dtype, hipStream_t s, void* dst_frag);
long conv_rows_num_row_blocks(long M, int cout);
// conv_wide.hip
int pack_s2frag_launch(const float* src, long s0, long s1, long s2, int Co, int Ci, void* dst, int trans,
                       hipStream_t s);
// tconv_frame.hip
int tconv_frame_launch(const stgcn_conv_desc& a, hipStream_t s);
long tconv_frame_row_blocks(int N, int T);
// conv_wgrad.hip, wgrad_tile.hip, wgrad_wide.hip, wgrad_ring.hip, wgrad1x1.hip
int conv_wgrad_launch(stgcn_wgrad_desc a, int dtype, hipStream_t s);
long wgrad_tile_workspace(const stgcn_wgrad_desc& a, int dtype);
int wgrad_tile_launch(const stgcn_wgrad_desc& a, int dtype, hipStream_t s);
long wgrad_wide_workspace(const stgcn_wgrad_desc& a, int dtype);
int wgrad_wide_launch(const stgcn_wgrad_desc& a, int dtype, hipStream_t s);
long wgrad_ring_workspace(const stgcn_wgrad_desc& a, int dtype);
int wgrad_ring_launch(const stgcn_wgrad_desc& a, int dtype, hipStream_t s);
long wgrad1x1_workspace(const stgcn_wgrad_desc& a, int dtype);
int wgrad1x1_launch(const stgcn_wgrad_desc& a, int dtype, hipStream_t s);
// gconv.hip
long gconv_row_blocks(int NT, int V);
int gconv_launch(const stgcn_gconv_desc& a, int dtype, hipStream_t s);
int gconv_weights_launch(const float* A, const float* W, const int* nbr, const int* deg, int P, int V, int J, int Cout,
                         int Cin, int trans, void* out, int R_pad, int C_pad, int dtype, hipStream_t s,
                         const float* bconv = nullptr, float* bias2d = nullptr);
// gconv_wgrad.hip
long gconv_wgrad_workspace(const stgcn_gconv_wgrad_desc& a, int dtype);
int gconv_wgrad_launch(const stgcn_gconv_wgrad_desc& a, int dtype, hipStream_t s);
// gconv_finish.hip
int gconv_wgrad_finish_launch(const float* dweff, const float* A, const float* W, const int* nbr, const int* deg,
                              int P, int V, int J, int Cout, int Cin, float* dW, float* dA, void* work, hipStream_t s);
long gconv_wgrad_finish_workspace(int P, int V, int J, int Cout, int Cin);
int gconv_wgrad_finish_bias_launch(const float* dweff, const float* A, const float* W, const int* nbr, const int* deg,
                                   int P, int V, int J, int Cout, int Cin, const float* bconv, const float* S, float* dW,
                                   float* dA, float* db, void* work, hipStream_t s);
// gcn_amix.hip
int amix_fwd_launch(const stgcn_amix_desc& a, int dtype, hipStream_t s);
int amix_trans_launch(const stgcn_amix_desc& a, int dtype, hipStream_t s);
int amix_dA_launch(const stgcn_amix_desc& a, const void* dw, float* dA, void* work, int dtype, hipStream_t s);
long amix_dA_workspace(const stgcn_amix_desc& a);
int gcn_bias_bwd_launch(const float* A, const float* b, const float* S, int P, int V, int C, float* dA, float* db,
                        hipStream_t s);
int gcn_bias_launch(const float* A, const float* b, float* out, int N, int P, int V, int C, int per_sample,
                    hipStream_t s);
// bn_fused.hip
long bn_bwd_fused_work_floats(long M, int C, int dtype);
int bn_bwd_fused_reduce_launch(const stgcn_bn_bwd_desc& a, int dtype, hipStream_t s);
int bn_bwd_fused_apply_launch(const stgcn_bn_bwd_desc& a, int dtype, hipStream_t s);
// norm.hip
long norm_stats_num_blocks(long M);
int bn_stats_partial_launch(const void* x, int ld, long M, int C, float4* part, int dtype, hipStream_t s);
int bn_finalize_launch(const float4* part, int nb, int ldp, int C, const float* gamma, const float* beta, float eps,
                       float2* mean_rstd, float* scale, float* shift, hipStream_t s);
int bn_merge_launch(const float4* part, int nb, int ldp, int C, float4* merged, hipStream_t s);
int bn_apply_launch(const void* u, int ldu, const float* sc, const float* sh, int res_mode, const void* r, int ldr,
                    const float* rsc, const float* rsh, int relu, void* y, int ldy, long M, int C, int dtype,
                    hipStream_t s, unsigned char* bits = nullptr);
int bn_bwd_reduce_launch(const void* dy, int lddy, int mask, const void* mref, int ldm, const float* msc,
                         const float* msh, const void* x, int ldx, const float2* mean_rstd, long M, int C,
                         float2* part, float2* out, int dtype, hipStream_t s);
int bn_bwd_apply_launch(const void* dy, int lddy, int mask, const void* mref, int ldm, const float* msc,
                        const float* msh, const void* x, int ldx, const float2* mean_rstd, const float* gamma,
                        const float2* sums, long M, int C, void* dx, int lddx, int accumulate, int dtype,
                        hipStream_t s);
int rowgroup_sum_launch(const void* x, int ld, long M, int C, int G, long period, float* S, float* work, int dtype,
                        hipStream_t s);
long rowgroup_sum_workspace(long M, int C, int G, long period);
long cast_colsum_workspace(long M, int C);
int cast_colsum_launch(const float* x, int ldx, long M, int C, void* out16, int ldo, float* colsum, float* work,
                       hipStream_t s);
int pool_rows_launch(const void* x, int ld, int N, int R, int C, void* out, int ldo, int dtype, hipStream_t s);
int unpool_rows_launch(const void* dp, int ldp, int R, int C, long M, void* dx, int ldx, int dtype, hipStream_t s);
// ln.hip
int ln_stats_launch(const void* x, int ld, long F, int V, int C, float eps, float2* stats, int dtype, hipStream_t s);
int ln_apply_launch(const void* u, int ldu, const float2* st, const float* g, const float* b, int res_mode,
                    const void* r, int ldr, const float2* rst, const float* rg, const float* rb, int relu, void* y,
                    int ldy, long M, int V, int C, int dtype, hipStream_t s);
long ln_bwd_workspace(long F, int V, int C, int dtype);
int ln_bwd_launch(const void* dy, int lddy, int mask, const void* mref, int ldm, const void* x, int ldx,
                  const float2* st, const float* g, const float* b, long F, int V, int C, void* dx, int lddx,
                  int accumulate, float* dgb, void* work, long work_bytes, int dtype, hipStream_t s);
// rt.hip
int box_sum_launch(const void* x, int ldx, void* y, int ldy, int N, int T_, int V, int C, int K, int S, int trans,
                   int accumulate, int dtype, hipStream_t s);
int rt_online_launch(const float* z, float* fifo, float* acc, int* idx, int C, int V, int fifo_size, int S,
                     float* out, hipStream_t s);
// attn.hip
int attn_scores_launch(const void* th, const void* ph, int ld, int N, int T_, int V, int P, int ce, float* S,
                       void* work, int dtype, hipStream_t s);
long attn_scores_workspace(int N, int T_, int V, int P);
int attn_proj_launch(const void* x, int ldx, long M, int Cin, const float* W, const float* bias, int Nout, float* out,
                     int ldo, hipStream_t s);
int attn_bwd_launch(const void* th, const void* ph, int ld, int N, int T_, int V, int P, int ce, const float* C,
                    const float* dC, float* dS, void* dth, void* dph, int dtype, hipStream_t s);
// layer_fused.hip
int layer_fused_launch(const stgcn_layer_fused_desc& a, hipStream_t s);
// rt_fused.hip
int rt_in_launch(const float* x, int V, const float* g, const float* b, const float* W, const float* bias, int C0,
                 float* out, int F, hipStream_t s);
int rt_gcn_launch(const float* x, int V, int Cin, int Cout, int P, const float* A, const float* W, const float* bias2d,
                  float* fifo, float* acc, const int* idx, const float* Wr, float* a_out, float* r_out,
                  hipStream_t s);
int rt_norm_launch(const float* a, const float* g, const float* b, int res_mode, const float* res, const float* gr,
                   const float* br, int V, int C, int* idx, int fifo_size, int S, float* y, hipStream_t s);
int rt_out_launch(const float* x, int V, int C, const float* W, const float* bias, int K, float* out, hipStream_t s);
int rt_frame_launch(const stgcn_rt_frame_desc& d, hipStream_t s);
// rt_streams.hip
int rt_streams_launch(const stgcn_rt_streams_desc& d, hipStream_t s);
// co_frame.hip
int co_check(const stgcn_co_layer& d, bool shapes_only);
int co_num_splits(const stgcn_co_layer& d, hipStream_t s);
long co_pack_elems(int Cout, int C, int Kt);
int co_pack_launch(const float* w, int Cout, int C, int Kt, void* dst, int dtype, hipStream_t s);
long co_pack_rows_elems(int rows, int C);
int co_pack_rows_launch(const float* w, int groups, int rows, int C, void* dst, int dtype, hipStream_t s);
int co_gcn_launch(const stgcn_co_layer& d, hipStream_t s);
int co_push_launch(const stgcn_co_layer& d, hipStream_t s);
int co_taps_launch(const stgcn_co_layer& d, hipStream_t s);
int co_finish_launch(const stgcn_co_layer& d, hipStream_t s);
// co_streams.hip
int co_streams_check(const stgcn_co_streams_desc& d, bool shapes_only);
int co_streams_num_splits(const stgcn_co_streams_desc& d, int layer);
int co_streams_launch(const stgcn_co_streams_desc& d, hipStream_t s);
// co_streams_clip.hip: the stream batch's clip, and one stream's as its B = 1 case
int co_clip_num_splits(const stgcn_co_clip_layer& y);
int co_clip_check(const stgcn_co_clip_desc& d, bool shapes_only);
int co_clip_launch(const stgcn_co_clip_desc& d, hipStream_t s);
int co_streams_clip_check(const stgcn_co_streams_clip_desc& d, bool shapes_only);
int co_streams_clip_launch(const stgcn_co_streams_clip_desc& d, hipStream_t s);
// rt_streams_clip.hip
int rt_streams_clip_launch(const stgcn_rt_streams_clip_desc& d, hipStream_t s);
// stream_state.hip
int stream_state_check(const stgcn_stream_state_desc& d);
int stream_state_export_launch(const stgcn_stream_state_desc& d, hipStream_t s);
int stream_state_import_launch(const stgcn_stream_state_desc& d, hipStream_t s);
// ms_stage.hip
long ms_pack_elems(int F);
int ms_pack_launch(const float* w1, const float* w2, int F, int kernel, void* dst, int dtype, hipStream_t s);
int ms_wgrad_blocks(int R);
int ms_layer_fwd_launch(const stgcn_ms_layer& d, hipStream_t s);
int ms_layer_bwd_launch(const stgcn_ms_layer& d, hipStream_t s);
int ms_lin_blocks(int rows);
int ms_lin_fwd_launch(const stgcn_ms_lin& d, int which, hipStream_t s);
int ms_lin_bwd_launch(const stgcn_ms_lin& d, int which, hipStream_t s);
int ms_prob_launch(const float* y, const float* dy, float* out, int rows, int C, int mode, hipStream_t s);
// window.hip
int window_stat_blocks_launch(int nw, int W);
int window_stats_launch(const float* x, int Cin, int Lp, int V, int W, int n0, int nw, int mode, float eps, float* out,
                        hipStream_t s);
int window_expand_launch(const float* x, int Cin, int Lp, int V, int W, int n0, int nw, int mode, const float* g,
                         const float* b, const float* fst, const float* w, const float* bias, int Cout, void* out,
                         int ldo, int dtype, hipStream_t s);
long window_grad_workspace_launch(int nw, int W, int V, int Cin, int Cout);
int window_grad_launch(const void* dy, int ldd, int dtype, const float* x, int Cin, int Lp, int V, int W, int n0, int nw,
                       int mode, const float* st, const float* g, const float* b, const float* w, int Cout, float* work,
                       float* dg, float* dbeta, float* dw, float* db, hipStream_t s);
// metrics.hip
long seg_metrics_workspace_launch(int L);
int seg_metrics_launch(const long* lab, const long* pred, int L, int C, const float* ov, int K, int* ws,
                       unsigned long long* cm, float* out, int* status, hipStream_t s);
// loss.hip
long seg_loss_workspace_launch(int L);
int seg_loss_launch(const float* p, int ldp, const long* labels, const float* wt, const float* prev, int L, int C,
                    int first, int mode, const float* den, float pairs, float* dce, float* dmse, int* top5, float* work,
                    float* out, hipStream_t s);
int seg_loss_bwd_launch(const float* dce, const float* dmse, const float* gce, const float* gmse, long n, float* dp,
                        hipStream_t s);
