// The k-wide depthwise-separable block (SepBlock, net_internal.h) that the ladders of net_dwk.hip and net_mts.hip are made of.
// Data flow (training), as in net.hip:
//   z = dwk( relu6(bn_prev(y_prev)) )     kws_dwconvk_fwd_f32, BN + ReLU6 applied on load (or a materialised activation as it is)
//   y = z W                               f32 MFMA GEMM with the BN statistics in its epilogue
// The backward is the two-kernel form: kws_dwconvk_bwd_f32 materialises the gated gradient g, kws_dwconvk_bwd_finalize folds its
// partial rows, kws_bn_bwd_apply turns g into the producer's dy in place.  A program's first block keeps a pointwise kernel of its
// own (K = 1 / the stems) and calls that beside these.
#include "net_internal.h"

int kws_sep_fwd(const SepBlock& b, const float* params, const float* in, const float* bn_in, float* z, float* y, float* stats, int B,
                hipStream_t st) {
  const int64_t M = (int64_t)B * b.Lout;
  KWS_TRY(kws_dwconvk_fwd_f32(in, bn_in, params + b.dw, z, B, b.Lin, b.Lout, b.cin, b.k, b.stride, b.pad_l, st));
  KWS_TRY(kws_gemm_nn_f32(z, params + b.pw, y, M, b.cin, b.cout, stats, st));
  return kws_gemm_nn_stats_rows(M, b.cin, b.cout);
}

int kws_sep_bn_table(const SepBlock& b, const float* params, float* state, const float* stats, int rows, int64_t M, bool training,
                     float* bn, float* red, hipStream_t st) {
  if (training)
    return kws_bn_stats_finalize(stats, rows, M, b.cout, params + b.bn.gamma, params + b.bn.beta, KWS_BN_EPS, KWS_BN_MOMENTUM,
                                 state + b.bn.mm, state + b.bn.mv, bn, red, st);
  return kws_bn_infer_prepare(params + b.bn.gamma, params + b.bn.beta, state + b.bn.mm, state + b.bn.mv, KWS_BN_EPS, b.cout, bn, st);
}

int kws_sep_dw_bwd(const SepBlock& b, const float* params, float* grads, const float* in, const float* bn_in, const BnRef* prod,
                   float* out, const SepBwdScratch& s, int B, hipStream_t st) {
  KWS_TRY(kws_dwconvk_bwd_f32(s.DZ, in, bn_in, params + b.dw, out, s.part, B, b.Lin, b.Lout, b.cin, b.k, b.stride, b.pad_l, st));
  const int prows = kws_dwconvk_bwd_part_rows(B, b.Lin, b.cin, b.k, b.stride);
  if (!prod) return kws_dwconvk_bwd_finalize(s.part, prows, (int64_t)B * b.Lin, b.cin, b.k, grads + b.dw, nullptr, nullptr, nullptr, st);
  KWS_TRY(kws_dwconvk_bwd_finalize(s.part, prows, (int64_t)B * b.Lin, b.cin, b.k, grads + b.dw, grads + prod->gamma, grads + prod->beta,
                                   s.coef, st));
  return kws_bn_bwd_apply(out, in, bn_in, params + prod->gamma, s.coef, (int64_t)B * b.Lin, b.cin, st);
}

int kws_sep_bwd(const SepBlock& b, const float* params, float* grads, const float* dy, const float* z, const float* in,
                const float* bn_in, const BnRef* prod, float* out, const SepBwdScratch& s, int B, hipStream_t st) {
  const int64_t M = (int64_t)B * b.Lout;
  KWS_TRY(kws_transpose_f32(params + b.pw, s.WT, b.cin, b.cout, st));
  KWS_TRY(kws_gemm_nn_f32(dy, s.WT, s.DZ, M, b.cout, b.cin, nullptr, st));
  KWS_TRY(kws_gemm_tn_f32(z, dy, grads + b.pw, M, b.cin, b.cout, s.tn, st));
  return kws_sep_dw_bwd(b, params, grads, in, bn_in, prod, out, s, B, st);
}
