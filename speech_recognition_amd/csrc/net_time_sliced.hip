// Network program of
//
//   KWS_NET_CONV_1D_TIME_SLICED  conv_1d_time_sliced_model   reference model.py:716-772
//
// the model the raw-waveform attention net (net.hip) grew out of.  The same front end - overlapping_time_slice_stack(x, 40, 20)
// + Conv1D(3, strides=2) and the 3-tap depthwise / pointwise / BatchNormalization / relu6 blocks - but it starts at
// 32 * filter_mult filters, has one more reduce block and ends in
//   GlobalAveragePooling1D -> Dropout(.4) -> Dense(256 * fm, no bias) -> relu6 -> Dropout(.3) -> Dense(softmax, no bias, l2 1e-5)
// with keras categorical_crossentropy.
//   first convolution   kws_frame_conv_* (frame_conv.hip: N = 32 / 64 is outside conv1.hip)
//   blocks              the 3-tap depthwise ladder it shares with net.hip (Dw3Ladder, net_dw3ladder.hip); the input- and weight-
//                       gradient GEMMs of a layer as one launch where the fused kernel takes the shape (KwsSlabQueue::pair; K = 32
//                       is below its granule: two launches)
//   head                kws_gap_drop_* (gap.hip) -> the hidden Dense product as a GEMM over the dropped features -> relu6, the second
//                       Dropout, Dense + softmax, the loss and their backward in the flat tail over (h, table 1 | 0 | 0 | 1), as
//                       conv_1d_gru's head (net_dwk.hip) without its biases
// Dropout layer ids: 1 = Dropout(.4), 2 = Dropout(.3).
#include "net_internal.h"

namespace {

constexpr float TSL_KEEP1 = 0.6f;   // Dropout(0.4), model.py:760
constexpr float TSL_KEEP2 = 0.7f;   // Dropout(0.3), model.py:763
constexpr int TSL_FRAME = 40, TSL_HOP = 20, TSL_TAPS = 3, TSL_STRIDE = 2;   // model.py:745-747

struct TslLayout {
  int64_t total = 0;             // bytes
  Dw3Offsets a;                  // the ladder's activations, BatchNorm tables and transposed pointwise kernels
  int64_t part = 0, red = 0, feat = 0, fd1 = 0, h = 0, tab = 0;
  int64_t G[2] = {0, 0}, DZ = 0, coef = 0, tn = 0, tns = 0, tns_cap = 0, WTd = 0, fcws = 0;
  FlatTailWs tail;
  int64_t bpart = 0;
};

struct TslProgram : FlatTailProgram<TslLayout> {
  int L_in = 0, pad1 = 0;
  int64_t conv1 = 0;
  Dw3Ladder lad;   // L1, C1, bn1: the first convolution's output
  int T = 0, C = 0, H = 0;
  int64_t d1k = 0;

  kws_frame_conv_t frame(int B) const {
    kws_frame_conv_t d;
    d.B = B; d.L = L_in; d.Lout = lad.L1; d.ksize = TSL_FRAME; d.hop = TSL_HOP; d.pad_l = pad1; d.taps = TSL_TAPS; d.stride = TSL_STRIDE;
    d.N = lad.C1; d.x_batch_stride = L_in;
    return d;
  }
  // the ladder's view of one call; the backward scratch (pass-1 rows = the forward statistics rows, coefficients, DZ) in training only
  Dw3Run run(const TslLayout& lo, const NetCall& c) const {
    float* ws = c.ws;
    return Dw3Run{&lo.a, c.params, c.state, c.grads, ws, c.B, ws + lo.red, c.training ? ws + lo.part : nullptr,
                  c.training ? ws + lo.coef : nullptr, c.training ? ws + lo.DZ : nullptr, c.st};
  }
  void layout(int B, bool training, TslLayout* lo) const override;
  int forward(const TslLayout& lo, const NetCall& c) const override;
  kws_flat_tail_args tail_args(const TslLayout& lo, const NetCall& c, float* probs) const override;
  int64_t tail_grad(const TslLayout& lo) const override { return lo.G[0]; }
  int backward(const TslLayout& lo, const NetCall& c) const override;
  int debug_view(int B, int training, int what, int index, int64_t* offset_floats, int64_t* count) const override;
};

void TslProgram::layout(int B, bool training, TslLayout* lo) const {
  Bump bp;
  const kws_frame_conv_t fc = frame(B);
  const Dw3Sizes s = lad.sizes(B);
  const int maxC = std::max(s.maxC, H);
  const int64_t max_part = std::max(std::max(s.max_part, (int64_t)kws_frame_conv_stats_rows(&fc) * 2 * lad.C1),
                                    (int64_t)kws_gap_drop_bwd_part_rows(B, T, C) * 2 * C);
  lad.take_acts(bp, B, training, s, &lo->a);
  lad.take_bn(bp, maxC, &lo->a);
  lo->part = bp.take(std::max(max_part, s.max_dwpart));
  lo->red = bp.take((int64_t)KWS_REDUCE_SLICES * 5 * maxC);
  lo->feat = bp.take((int64_t)B * C);
  lo->fd1 = bp.take((int64_t)B * C);
  lo->h = bp.take((int64_t)B * H);
  lo->tab = bp.take((int64_t)4 * H);
  if (training) {
    const int64_t max_g = std::max(s.max_y, (int64_t)B * std::max(C, H));
    lo->G[0] = bp.take(max_g);
    lo->G[1] = bp.take(max_g);
    lo->DZ = bp.take(s.max_z);
    lo->coef = bp.take((int64_t)2 * maxC);
    lad.take_WT(bp, &lo->a);
    lo->WTd = bp.take((int64_t)C * H);
    lo->tn = bp.take(kws_gemm_tn_workspace_floats(B, C, H));
    lo->tns_cap = 0;   // the blocks' weight-gradient slabs: one region, summed in batches (KwsSlabQueue)
    for (const Dw3Block& b : lad.blocks) lo->tns_cap += (kws_gemm_tn_workspace_floats((int64_t)B * b.Lout, b.cin, b.cout) + 63) / 64 * 64;
    lo->tns = bp.take(lo->tns_cap);
    lo->fcws = bp.take(kws_frame_conv_wgrad_workspace_floats(&fc));
    lo->tail.take(bp, B, H, dense.NC);
    lo->bpart = bp.take((int64_t)DK_BIAS_SLICES * H);
  }
  lo->total = bp.cur * 4;
}

int TslProgram::debug_view(int B, int training, int what, int index, int64_t* offset_floats, int64_t* count) const {
  TslLayout lo;
  layout(B, training != 0, &lo);
  if (what >= 0 && what <= 2) return lad.debug_view(lo.a, B, what, index, offset_floats, count);
  if (what == 4) {   // the hidden Dense layer's output before relu6 [B, H]
    *offset_floats = lo.h;
    *count = (int64_t)B * H;
  } else {
    kws_set_error("net_debug_view: unknown view %d", what);
    return KWS_E_INVALID;
  }
  return KWS_OK;
}

// first convolution, blocks, pool + Dropout(.4) and the hidden Dense product; training: batch statistics (moving averages updated)
// and the masks
int TslProgram::forward(const TslLayout& lo, const NetCall& c) const {
  const Dw3Run r = run(lo, c);
  const int nb = lad.nb(), B = c.B;
  const float* params = c.params;
  float* ws = c.ws;
  hipStream_t st = c.st;
  const bool training = c.training;
  float* stats = r.part;   // NULL in inference
  if (!training) KWS_TRY(lad.infer_tables(r));
  {
    const kws_frame_conv_t fc = frame(B);
    const BnRef& bn1 = lad.bn1;
    KWS_TRY(kws_frame_conv_fwd_f32(c.x, params + conv1, r.y(0), stats, &fc, st));
    if (training)
      KWS_TRY(kws_bn_stats_finalize(stats, kws_frame_conv_stats_rows(&fc), (int64_t)B * lad.L1, lad.C1, params + bn1.gamma,
                                    params + bn1.beta, KWS_BN_EPS, KWS_BN_MOMENTUM, r.state + bn1.mm, r.state + bn1.mv, r.bn_at(0), r.red, st));
  }
  for (int i = 0; i < nb; ++i) KWS_TRY(lad.fwd_block_f32(i, r, stats, nullptr));
  KWS_TRY(kws_gap_drop_fwd_f32(r.y(nb), r.bn_at(nb), ws + lo.feat, ws + lo.fd1, B, T, C, training ? TSL_KEEP1 : 1.f, c.seed, c.step, 1,
                               c.row_offset, st));
  KWS_TRY(kws_gemm_nn_f32(ws + lo.fd1, params + d1k, ws + lo.h, B, C, H, nullptr, st));
  return dk_bias_table(nullptr, H, ws + lo.tab, st);
}

// relu6 + Dropout(.3) of the hidden layer, Dense + softmax (+ loss and its backward): the flat tail over (h, table 1 | 0 | 0 | 1)
kws_flat_tail_args TslProgram::tail_args(const TslLayout& lo, const NetCall& c, float* probs) const {
  kws_flat_tail_args t;
  memset(&t, 0, sizeof(t));
  t.y = c.ws + lo.h; t.bn = c.ws + lo.tab; t.Ng = H;
  t.Wd = c.params + dense.kernel; t.bd = nullptr;
  t.probs = probs;
  t.B = c.B; t.D = H; t.F = H; t.NC = dense.NC;
  t.keep_prob = TSL_KEEP2;
  t.layer_id = 2;
  return t;
}

// G[0] = gradient wrt relu6(h) [B, H] -> wrt h; dense_1's gradients; back through Dropout(.4) and the pool; then the blocks
int TslProgram::backward(const TslLayout& lo, const NetCall& c) const {
  const Dw3Run r = run(lo, c);
  const int nb = lad.nb(), B = c.B;
  const float* params = c.params;
  float* grads = c.grads;
  float* ws = c.ws;
  hipStream_t st = c.st;
  float* part = r.part;
  float* coef = r.coef;
  float* DZ = r.DZ;
  float* G[2] = {ws + lo.G[0], ws + lo.G[1]};
  KWS_TRY(dk_dense_bwd(G[0], ws + lo.h, ws + lo.fd1, params + d1k, nullptr, grads + d1k, nullptr, DZ, B, C, H,
                       {ws + lo.WTd, ws + lo.tn, ws + lo.bpart}, st));
  {   // DZ = gradient wrt the dropped features [B, C] (DZ holds B * T * C floats for the last block) -> G[nb % 2] = gated gradient
      // wrt relu6(bn(y)) [B, T, C] -> dy of the last block's pointwise output, in place
    const Dw3Block& b = lad.blocks[nb - 1];
    float* g = G[nb % 2];
    KWS_TRY(kws_gap_drop_bwd_f32(DZ, r.y(nb), r.bn_at(nb), g, part, B, T, C, TSL_KEEP1, c.seed, c.step, 1, c.row_offset, st));
    KWS_TRY(kws_gbn_layer_bwd_finish(g, r.y(nb), r.bn_at(nb), (int64_t)B * T, kws_gbn_grouped(1, b.cout), part,
                                     kws_gap_drop_bwd_part_rows(B, T, C), coef, grads, b.bn, st));
  }
  // ---- blocks: G[(i + 1) % 2] = dy of block i's pointwise output
  KWS_TRY(lad.transpose_all(r));
  KwsSlabQueue q;
  q.base = ws + lo.tns;
  q.cap = lo.tns_cap;
  q.allow_pair = kws_net_get_gemm_mode(net) != 1;   // mode 1: separate input- / weight-gradient launches; mode 2 is ignored
  for (int i = nb - 1; i >= 0; --i) {
    const Dw3Block& b = lad.blocks[i];
    KWS_TRY(q.pair(G[(i + 1) % 2], r.WT(i), DZ, r.z(i), grads + b.pw, (int64_t)B * b.Lout, b.cin, b.cout, st));
    KWS_TRY(lad.bwd_block_input(i, r, G[i % 2], nullptr));
  }
  KWS_TRY(q.flush(st));
  // G[0] = dy of the first convolution; its input is the waveform: no input gradient
  const kws_frame_conv_t fc = frame(B);
  return kws_frame_conv_wgrad_f32(c.x, G[0], grads + conv1, ws + lo.fcws, &fc, st);
}

}  // namespace

int tsl_build(kws_net* n) {
  TslProgram* p = new TslProgram();
  n->program.reset(p);
  p->net = n;
  const kws_net_config_t& c = n->cfg;
  KWS_REQUIRE(c.filter_mult >= 1 && c.filter_mult <= 2, "net: filter_mult %d unsupported", c.filter_mult);
  KWS_REQUIRE(c.input_size >= TSL_FRAME && c.input_size % 4 == 0, "net: input_size %d unsupported", c.input_size);
  const int fm = c.filter_mult;
  p->L_in = c.input_size;
  // overlapping_time_slice_stack(x, 40, 20) SAME (model.py:745) fused with Conv1D(32 fm, 3, strides=2) (model.py:747)
  int Lf;
  kws_same_pad(p->L_in, TSL_FRAME, TSL_HOP, &Lf, &p->pad1);
  KWS_REQUIRE(Lf >= TSL_TAPS, "net: input_size %d is too short for the first convolution", c.input_size);
  Dw3Ladder& lad = p->lad;
  lad.L1 = (Lf - TSL_TAPS) / TSL_STRIDE + 1;
  lad.C1 = 32 * fm;
  KerasNames kn{n};
  p->conv1 = kn.conv(TSL_TAPS, TSL_FRAME, lad.C1, KWS_L2_COEF);
  lad.bn1 = kn.bn(lad.C1);
  {
    const kws_frame_conv_t fc = p->frame(1);
    KWS_REQUIRE(kws_frame_conv_stats_rows(&fc) > 0, "net: input_size %d is outside the first convolution's domain", c.input_size);
  }
  // _context_conv(64), then six _reduce_block = _reduce_conv (stride 2, SAME) + _context_conv (VALID) (model.py:752-758)
  static const int spec[13][2] = {{1, 64},  {2, 128}, {1, 128}, {2, 192}, {1, 192}, {2, 256}, {1, 256},
                                  {2, 320}, {1, 320}, {2, 384}, {1, 384}, {2, 512}, {1, 512}};
  KWS_TRY(lad.build(kn, spec, 13, fm, c.input_size));
  p->T = lad.blocks.back().Lout;
  p->C = lad.blocks.back().cout;
  p->H = 256 * fm;
  p->dense.NC = c.num_classes;
  p->dense.D = p->H;
  p->zero_grads = true;
  KWS_REQUIRE(p->T <= 16, "net: %d time steps at the pool (max 16)", p->T);
  p->d1k = kws_net_add_tensor(n, "dense_1/kernel", {p->C, p->H}, false, 0.f, p->C, p->H, 0.f);
  p->dense.kernel = kws_net_add_tensor(n, "dense_2/kernel", {p->H, p->dense.NC}, false, KWS_L2_COEF, p->H, p->dense.NC, 0.f);
  return KWS_OK;
}
