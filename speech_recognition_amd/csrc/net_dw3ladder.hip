// The 3-tap depthwise ladder (Dw3Ladder, net_internal.h) under conv_1d_time_sliced_with_attention (net.hip) and
// conv_1d_time_sliced (net_time_sliced.hip): the block table, its share of the workspace, and the launch steps of a block.
// Backward of block i, from r.DZ = the gradient wrt z[i] (the caller's input-gradient GEMM): kws_dwconv_bwd_bn_f32 pass 1 leaves
// partial rows, kws_dw_bwd_finalize folds them into the depthwise kernel's gradient, the producing BatchNorm's dgamma / dbeta and
// its coefficients, pass 2 recomputes the gated gradient and writes dy of the producer - the masked gradient is never materialised.
// Nothing here asks which net calls or which arithmetic its GEMMs run in: a program branches around these steps.
#include "net_internal.h"

int Dw3Ladder::build(KerasNames& kn, const int (*spec)[2], int n, int fm, int input_size) {
  int L = L1, cin = C1;
  for (int i = 0; i < n; ++i) {
    Dw3Block b;
    b.stride = spec[i][0];
    b.cin = cin;
    b.cout = spec[i][1] * fm;
    b.Lin = L;
    if (b.stride == 2) {
      kws_same_pad(L, 3, 2, &b.Lout, &b.pad_l);  // _reduce_conv: padding='same'
    } else {
      b.Lout = L - 2;  // _context_conv: padding='valid'
      b.pad_l = 0;
    }
    KWS_REQUIRE(b.Lout >= 1, "net: input_size %d is too short: block %d keeps no row", input_size, i);
    b.dw = kn.dw(cin);
    b.pw = kn.conv(1, cin, b.cout, KWS_L2_COEF);
    b.bn = kn.bn(b.cout);
    blocks.push_back(b);
    L = b.Lout;
    cin = b.cout;
  }
  return KWS_OK;
}

Dw3Sizes Dw3Ladder::sizes(int B) const {
  Dw3Sizes s;
  s.max_y = (int64_t)B * L1 * C1;
  s.maxC = C1;
  for (const Dw3Block& b : blocks) {
    const int64_t M = (int64_t)B * b.Lout;
    s.max_y = std::max(s.max_y, M * b.cout);
    s.max_z = std::max(s.max_z, M * b.cin);
    s.max_part = std::max(s.max_part, (int64_t)kws_gemm_num_row_tiles(M) * 2 * b.cout);
    s.max_dwpart = std::max(s.max_dwpart, kws_dwconv_bwd_part_floats(B, b.Lin, b.cin));
    s.maxC = std::max(s.maxC, b.cout);
  }
  return s;
}

void Dw3Ladder::take_acts(Bump& bp, int B, bool training, const Dw3Sizes& s, Dw3Offsets* o) const {
  o->y.assign(nb() + 1, 0);
  o->z.assign(nb(), 0);
  if (training) {
    o->y[0] = bp.take((int64_t)B * L1 * C1);
    for (int i = 0; i < nb(); ++i) {
      o->z[i] = bp.take((int64_t)B * blocks[i].Lout * blocks[i].cin);
      o->y[i + 1] = bp.take((int64_t)B * blocks[i].Lout * blocks[i].cout);
    }
  } else {
    const int64_t ya = bp.take(s.max_y), yb = bp.take(s.max_y), zz = bp.take(s.max_z);
    o->y[0] = ya;
    for (int i = 0; i < nb(); ++i) {
      o->z[i] = zz;
      o->y[i + 1] = (i % 2 == 0) ? yb : ya;
    }
  }
}

void Dw3Ladder::take_bn(Bump& bp, int maxC, Dw3Offsets* o) const {
  o->bn_stride = (4 * maxC + 63) / 64 * 64;
  o->bn = bp.take(o->bn_stride * (nb() + 1));
}

void Dw3Ladder::take_WT(Bump& bp, Dw3Offsets* o) const {
  o->WT.assign(nb(), 0);
  for (int i = 0; i < nb(); ++i) o->WT[i] = bp.take((int64_t)blocks[i].cin * blocks[i].cout);
}

int Dw3Ladder::debug_view(const Dw3Offsets& o, int B, int what, int index, int64_t* offset_floats, int64_t* count) const {
  if (what == 0) {          // pre-BN output y[index]: 0 = the first convolution, i + 1 = block i
    KWS_REQUIRE(index >= 0 && index <= nb(), "net_debug_view: y index %d", index);
    *offset_floats = o.y[index];
    *count = index == 0 ? (int64_t)B * L1 * C1 : (int64_t)B * blocks[index - 1].Lout * blocks[index - 1].cout;
  } else if (what == 1) {   // depthwise output z[index]
    KWS_REQUIRE(index >= 0 && index < nb(), "net_debug_view: z index %d", index);
    *offset_floats = o.z[index];
    *count = (int64_t)B * blocks[index].Lout * blocks[index].cin;
  } else {                  // table (scale|shift|mean|rstd) of batch_normalization_{index+1}
    KWS_REQUIRE(what == 2 && index >= 0 && index <= nb(), "net_debug_view: bn index %d", index);
    *offset_floats = o.bn + o.bn_stride * index;
    *count = 4 * (index == 0 ? C1 : blocks[index - 1].cout);
  }
  return KWS_OK;
}

int Dw3Ladder::infer_tables(const Dw3Run& r) const {
  KWS_REQUIRE(nb() + 1 <= KWS_BN_INFER_BATCH, "net: %d blocks exceed the BatchNorm table batch", nb());
  const float *ga[KWS_BN_INFER_BATCH], *be[KWS_BN_INFER_BATCH], *mm[KWS_BN_INFER_BATCH], *mv[KWS_BN_INFER_BATCH];
  float* tb[KWS_BN_INFER_BATCH];
  int Cs[KWS_BN_INFER_BATCH];
  for (int l = 0; l <= nb(); ++l) {
    const BnRef& b = l == 0 ? bn1 : blocks[l - 1].bn;
    ga[l] = r.params + b.gamma; be[l] = r.params + b.beta; mm[l] = r.state + b.mm; mv[l] = r.state + b.mv; tb[l] = r.bn_at(l); Cs[l] = b.C;
  }
  return kws_bn_infer_prepare_batch(ga, be, mm, mv, KWS_BN_EPS, Cs, tb, nb() + 1, r.st);
}

int Dw3Ladder::transpose_all(const Dw3Run& r) const {
  KWS_REQUIRE(nb() <= KWS_TRANSPOSE_BATCH, "net: %d blocks exceed the transpose batch", nb());
  const float* tin[KWS_TRANSPOSE_BATCH];
  float* tout[KWS_TRANSPOSE_BATCH];
  int trows[KWS_TRANSPOSE_BATCH], tcols[KWS_TRANSPOSE_BATCH];
  for (int i = 0; i < nb(); ++i) {
    tin[i] = r.params + blocks[i].pw; tout[i] = r.WT(i);
    trows[i] = blocks[i].cin; tcols[i] = blocks[i].cout;
  }
  return kws_transpose_batch_f32(tin, tout, trows, tcols, nb(), r.st);
}

int Dw3Ladder::fwd_dw(int i, const Dw3Run& r, unsigned* amax) const {
  const Dw3Block& b = blocks[i];
  return kws_dwconv_fwd_amax_f32(r.y(i), r.bn_at(i), r.params + b.dw, r.z(i), r.B, b.Lin, b.Lout, b.cin, b.stride, b.pad_l, amax, r.st);
}

int Dw3Ladder::stats_finalize(int i, const Dw3Run& r, const float* stats, int rows) const {
  const Dw3Block& b = blocks[i];
  return kws_bn_stats_finalize(stats, rows, (int64_t)r.B * b.Lout, b.cout, r.params + b.bn.gamma, r.params + b.bn.beta, KWS_BN_EPS,
                               KWS_BN_MOMENTUM, r.state + b.bn.mm, r.state + b.bn.mv, r.bn_at(i + 1), r.red, r.st);
}

int Dw3Ladder::fwd_block_f32(int i, const Dw3Run& r, float* stats, unsigned* amax) const {
  const Dw3Block& b = blocks[i];
  const int64_t M = (int64_t)r.B * b.Lout;
  KWS_TRY(fwd_dw(i, r, amax));
  KWS_TRY(kws_gemm_nn_f32(r.z(i), r.params + b.pw, r.y(i + 1), M, b.cin, b.cout, stats, r.st));
  return stats ? stats_finalize(i, r, stats, kws_gemm_nn_stats_rows(M, b.cin, b.cout)) : KWS_OK;
}

int Dw3Ladder::bwd_block_input(int i, const Dw3Run& r, float* dy, unsigned* amax) const {
  const Dw3Block& b = blocks[i];
  const BnRef& prev = (i == 0) ? bn1 : blocks[i - 1].bn;
  KWS_TRY(kws_dwconv_bwd_bn_f32(r.DZ, r.y(i), r.bn_at(i), r.params + b.dw, nullptr, nullptr, r.part, 1, r.B, b.Lin, b.Lout, b.cin,
                                b.stride, b.pad_l, r.st));
  const int n_parts = (int)(kws_dwconv_bwd_part_floats(r.B, b.Lin, b.cin) / (5 * b.cin));
  KWS_TRY(kws_dw_bwd_finalize(r.part, n_parts, (int64_t)r.B * b.Lin, b.cin, r.grads + b.dw, r.grads + prev.gamma, r.grads + prev.beta,
                              r.coef, r.red, r.st));
  return kws_dwconv_bwd_bn_amax_f32(r.DZ, r.y(i), r.bn_at(i), r.params + b.dw, r.coef, dy, nullptr, 2, r.B, b.Lin, b.Lout, b.cin, b.stride,
                                    b.pad_l, amax, r.st);
}
