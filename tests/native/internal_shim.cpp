// Test-only forwarders to the INTERNAL launchers of the residual-network programs (resblock.hip, dwconv.hip, gemm.hip), of the
// classifier tails (tail.hip, gconv.hip kws_flat_tail_launch), of the shared BatchNorm bookkeeping (bncols.hip kws_gbn_*) and of
// the raw-waveform net's first convolution (conv1.hip kws_conv1_*; tests/test_conv1_cpu.py, tests/test_conv1_kernels_gpu.py).
// libkws_hip.so builds them with hidden visibility; tests/internal_shim.py links this file with the library's own objects into a
// separate libkws_internal_test.so (-Wl,-Bsymbolic) so that Python can call them (tests/test_resblock_kernels_gpu.py,
// tests/test_gemm_pair_gpu.py, tests/test_tail_kernels_gpu.py, tests/test_bn_cols_kernels_gpu.py) - and to the two batch launchers
// of bn.hip that only the network programs call (tests/test_dw3_kernels_gpu.py).  No kernels live here.
//
// Every forwarder has exactly the parameter list of the declaration it forwards to: KWST_FORWARD static_asserts that the two
// function types are the same, so a changed declaration fails this build instead of being cast into a wrong call.
#include <cstddef>
#include <type_traits>

#include "net_internal.h"

#define KWST_API extern "C" __attribute__((visibility("default")))
#define KWST_FORWARD(RET, NAME, PARAMS, ARGS)                                                                        \
  KWST_API RET kwst_##NAME PARAMS { return kws_##NAME ARGS; }                                                         \
  static_assert(std::is_same<decltype(kwst_##NAME), decltype(kws_##NAME)>::value,                                     \
                "kwst_" #NAME " does not match the declaration of kws_" #NAME)

// ---- residual-block joins (resblock.hip) ----
KWST_FORWARD(int, block_out_fwd,
             (const float* y, const float* bn, const float* res, const float* res_bn, float* o, int B, int L, int C, int pool,
              hipStream_t st),
             (y, bn, res, res_bn, o, B, L, C, pool, st));
KWST_FORWARD(int, block_out_dw_fwd,
             (const float* y, const float* bn, const float* res, const float* res_bn, const float* w, float* o, float* z, int B,
              int L, int C, int pool, hipStream_t st),
             (y, bn, res, res_bn, w, o, z, B, L, C, pool, st));
KWST_FORWARD(int64_t, block_out_bwd_part_floats, (int B, int L, int C, int pool), (B, L, C, pool));
KWST_FORWARD(int, block_out_bwd,
             (const float* dO, const float* y, const float* bn, float* g, float* part, int B, int L, int C, int pool, int relu,
              hipStream_t st),
             (dO, y, bn, g, part, B, L, C, pool, relu, st));
KWST_FORWARD(int, block_join_bwd_parts, (int B, int L, int C, int pool), (B, L, C, pool));
KWST_FORWARD(int, block_join_bwd,
             (const float* dO, const float* y, const float* bn, const float* gamma, const float* coef, float* out, float* part,
              int pass, int B, int L, int C, int pool, int relu, hipStream_t st),
             (dO, y, bn, gamma, coef, out, part, pass, B, L, C, pool, relu, st));
KWST_FORWARD(int, block_out3_fwd,
             (const float* y, const float* bn, const float* res, const float* res_bn, float* o, int B, int L, int Lo, int C,
              int stride, int pad_l, hipStream_t st),
             (y, bn, res, res_bn, o, B, L, Lo, C, stride, pad_l, st));
KWST_FORWARD(int64_t, block_out3_bwd_part_floats, (int B, int L, int C), (B, L, C));
KWST_FORWARD(int, block_out3_bwd,
             (const float* dO, const float* y, const float* bn, float* g, float* part, int B, int L, int Lo, int C, int stride,
              int pad_l, hipStream_t st),
             (dO, y, bn, g, part, B, L, Lo, C, stride, pad_l, st));

// ---- adds and the depthwise backward with an added gradient (resblock.hip, dwconv.hip) ----
KWST_FORWARD(int, add_f32, (const float* a, const float* b, float* out, int64_t n, hipStream_t st), (a, b, out, n, st));
KWST_FORWARD(int, add_strided_f32, (float* out, const float* in, int B, int L_out, int L_in, int C, int stride, hipStream_t st),
             (out, in, B, L_out, L_in, C, stride, st));
KWST_FORWARD(int, dwconv_bwd_acc_f32,
             (const float* dz, const float* y, const float* w, const float* add, float* g, float* part, int B, int L_in,
              int L_out, int C, int stride, int pad_l, hipStream_t st),
             (dz, y, w, add, g, part, B, L_in, L_out, C, stride, pad_l, st));
KWST_FORWARD(int, dwconv_bwd_acc_strided_f32,
             (const float* dz, const float* y, const float* w, const float* add, int add_stride, int add_len, float* g,
              float* part, int B, int L_in, int L_out, int C, int stride, int pad_l, hipStream_t st),
             (dz, y, w, add, add_stride, add_len, g, part, B, L_in, L_out, C, stride, pad_l, st));

// ---- strided GEMMs and slab sums (gemm.hip) ----
KWST_FORWARD(bool, gather_strided_rows, (const kws_gather_t* g, int* lda), (g, lda));
KWST_FORWARD(int, gemm_nn_strided_f32,
             (const float* A, int lda, const float* W, float* C, int64_t M, int K, int N, float* stats_part, hipStream_t stream),
             (A, lda, W, C, M, K, N, stats_part, stream));
KWST_FORWARD(int, gemm_tn_slabs_strided_f32,
             (const float* A, int lda, const float* G, int64_t M, int K, int N, float* workspace, int* S, hipStream_t stream),
             (A, lda, G, M, K, N, workspace, S, stream));
KWST_FORWARD(int, gemm_tn_slabs_f32,
             (const float* A, const float* G, int64_t M, int K, int N, float* workspace, int* S, hipStream_t stream),
             (A, G, M, K, N, workspace, S, stream));
KWST_FORWARD(int, gemm_dgrad_wgrad_f32,
             (const float* dY, const float* WT, float* dZ, const float* Z, int64_t M, int cin, int cout, float* workspace, int* S,
              hipStream_t stream),
             (dY, WT, dZ, Z, M, cin, cout, workspace, S, stream));
KWST_FORWARD(int, reduce_slabs_batch,
             (const float* const* ws, float* const* out, const int64_t* n, const int* S, int count, hipStream_t stream),
             (ws, out, n, S, count, stream));

// ---- classifier tails (tail.hip, gconv.hip) and the slab sum kws_small_wgrad_launch uses (gemm.hip) ----
KWST_FORWARD(int, ts_tail_launch, (const kws_ts_tail_args* p, hipStream_t st), (p, st));
KWST_FORWARD(int, small_wgrad_launch,
             (const float* X, const float* D, float* out, float* out_bias, int B, int K, int N, float* scratch, hipStream_t st),
             (X, D, out, out_bias, B, K, N, scratch, st));
KWST_FORWARD(int, metrics_launch, (const float* per_loss, const float* per_correct, int B, float* metrics, hipStream_t st),
             (per_loss, per_correct, B, metrics, st));
KWST_FORWARD(int, tail_post_launch, (const kws_tail_post_args* a, int* S_out, hipStream_t st), (a, S_out, st));
KWST_FORWARD(int, flat_tail_launch, (const kws_flat_tail_args* a, int training, hipStream_t st), (a, training, st));
KWST_FORWARD(int, reduce_slabs_f32, (const float* ws, float* out, int64_t n, int S, hipStream_t st), (ws, out, n, S, st));

// ---- the raw-waveform net's first convolution (conv1.hip) and the first stage of its two-stage slab sum (gemm.hip) ----
KWST_FORWARD(bool, conv1_supported, (const kws_gather_t* g, const kws_gather_t* unfolded, int N), (g, unfolded, N));
KWST_FORWARD(int, conv1_stats_rows, (int64_t M), (M));
KWST_FORWARD(int64_t, conv1_wgrad_workspace_floats, (int64_t M), (M));
KWST_FORWARD(int, conv1_fwd,
             (const float* x, const kws_gather_t* g, const kws_gather_t* unfolded, const float* W, float* y, int B, int N,
              float* stats, hipStream_t st),
             (x, g, unfolded, W, y, B, N, stats, st));
KWST_FORWARD(int, conv1_wgrad,
             (const float* x, const kws_gather_t* g, const kws_gather_t* unfolded, const float* G, float* dW, int B, int N,
              float* workspace, hipStream_t st),
             (x, g, unfolded, G, dW, B, N, workspace, st));
KWST_FORWARD(int, conv1_wgrad_slabs,
             (const float* x, const kws_gather_t* g, const kws_gather_t* unfolded, const float* G, float* dW, int B, int N,
              float* workspace, const float* const* sl_ws, float* const* sl_out, const int64_t* sl_n, const int* sl_S, int n_sl,
              hipStream_t st),
             (x, g, unfolded, G, dW, B, N, workspace, sl_ws, sl_out, sl_n, sl_S, n_sl, st));
KWST_FORWARD(int, reduce_slab_groups_f32, (float* ws, int64_t n, int S, int per_group, hipStream_t st), (ws, n, S, per_group, st));

// ---- BatchNorm bookkeeping over grouped columns or a column window (bncols.hip) ----
KWST_FORWARD(int, gbn_finalize,
             (const float* part, int rows, int64_t count, const kws_gbn_cols* c, const kws_gbn_refs* r, float eps, float momentum,
              float* bn, hipStream_t st),
             (part, rows, count, c, r, eps, momentum, bn, st));
KWST_FORWARD(int, gbn_infer, (const kws_gbn_cols* c, const kws_gbn_refs* r, float eps, float* bn, hipStream_t st), (c, r, eps, bn, st));
KWST_FORWARD(int, gbn_bwd_rows, (int64_t M), (M));
KWST_FORWARD(int, gbn_bwd,
             (float* dA, const float* y, const float* bn, const float* add, int64_t M, const kws_gbn_cols* c, float* part, float* coef,
              float* dgamma0, int64_t pstride, int64_t boff, hipStream_t st),
             (dA, y, bn, add, M, c, part, coef, dgamma0, pstride, boff, st));
KWST_FORWARD(int, gbn_bwd_finish,
             (float* g, const float* y, const float* bn, int64_t M, const kws_gbn_cols* c, const float* part, int rows, float* coef,
              float* dgamma0, int64_t pstride, int64_t boff, hipStream_t st),
             (g, y, bn, M, c, part, rows, coef, dgamma0, pstride, boff, st));
// ---- the batch launchers of bn.hip: depthwise weight gradients / inference BatchNorm tables of several layers in one launch ----
KWST_FORWARD(int, dw_grad_finalize_batch,
             (const float* const* part, const int* n_parts, const int* C, float* const* dw, int count, hipStream_t stream),
             (part, n_parts, C, dw, count, stream));
KWST_FORWARD(int, bn_infer_prepare_batch,
             (const float* const* gamma, const float* const* beta, const float* const* mm, const float* const* mv, float eps,
              const int* C, float* const* bn, int count, hipStream_t stream),
             (gamma, beta, mm, mv, eps, C, bn, count, stream));

// sizeof and the offset of the last member of kws_gbn_cols and kws_gbn_refs, for their ctypes mirrors
KWST_API void kwst_gbn_struct_layout(int64_t* out4) {
  out4[0] = (int64_t)sizeof(kws_gbn_cols);
  out4[1] = (int64_t)offsetof(kws_gbn_cols, c0);
  out4[2] = (int64_t)sizeof(kws_gbn_refs);
  out4[3] = (int64_t)offsetof(kws_gbn_refs, voff);
}

// sizeof and the offset of the last member of the three argument structs, in the order ts_tail, tail_post, flat_tail: the ctypes
// mirrors of tests/internal_shim.py are compared with these on the build machine (tests/test_internal_shim_cpu.py), so that a
// changed struct fails there instead of becoming a wrong call on the GPU
KWST_API void kwst_tail_struct_layout(int64_t* out6) {
  out6[0] = (int64_t)sizeof(kws_ts_tail_args);
  out6[1] = (int64_t)offsetof(kws_ts_tail_args, train);
  out6[2] = (int64_t)sizeof(kws_tail_post_args);
  out6[3] = (int64_t)offsetof(kws_tail_post_args, B);
  out6[4] = (int64_t)sizeof(kws_flat_tail_args);
  out6[5] = (int64_t)offsetof(kws_flat_tail_args, raw);
}
