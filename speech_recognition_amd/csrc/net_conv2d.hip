// Network programs of the reference's MFCC-image CNNs: ONE table-driven 2-D ladder, instantiated twice.
//   KWS_NET_CONV_2D_MOBILE  conv_2d_mobile_model (reference model.py:547-594): [98 * 40] mfcc -> Reshape [98, 40, 1] -> Preprocess ->
//                           eight Conv2D(F, 3 x 3, SAME, bias) -> BatchNormalization -> relu6 with F = 32, 32, 64, 64, 128, 128, 256, 256,
//                           the odd-numbered ones at stride 2 (49 x 20, 25 x 10, 13 x 5, 7 x 3), Dropout(.05) behind every pair ->
//                           GlobalAveragePooling2D -> Dropout(.1) -> Dense + softmax; SGD(1e-3, momentum .95), categorical CE
//   KWS_NET_CONV_2D_FAST    conv_2d_fast_model (model.py:597-639): four Conv2D(SAME, bias, dilation) -> BatchNormalization -> relu ->
//                           MaxPool2D(): 16 x (11, 5) dilation (2, 1), 32 x (5, 3) dilation (2, 1), 64 x (3, 3), 128 x (3, 3); images
//                           98 x 40 -> 49 x 20 -> 24 x 10 -> 12 x 5 -> 6 x 2 -> GlobalAveragePooling2D -> Dense + softmax; SGD(1e-3, .9)
// A ladder step is kws_conv2d_fwd_f32 (BN partial sums in its epilogue) and one BatchNorm finalise; the normalise + activation is
// applied on load by the next convolution (the project's convention) unless something stands between the two: a pool
// (kws_pool2x2_*, the pooled tensor is materialised ACTIVATED) or, in training, a Dropout, which is a small pass of its own
// (kws_bn_relu6_apply, then kws_dropout_fwd) - the next convolution then reads a materialised tensor without a table.  The tail is the
// residual family's global-average tail (kws_gp_tail_launch) over the last materialised tensor.
//
// The convolution bias stands in front of a BatchNormalization.  In training it cancels in the normalisation and its gradient is the
// BatchNorm backward's sum of dy, zero up to rounding: the device leaves it out of the GEMM, writes an exact-zero gradient, and adds
// it where it does matter - to the batch mean that updates moving_mean, and to the shift of the inference table (bias_fix_kernel).
#include "net_internal.h"

namespace {

struct C2Layer {
  kws_conv2d_t d;      // B filled in per call
  int64_t w, bias;     // conv2d_<n>/kernel [kh, kw, Cin, F], conv2d_<n>/bias [F]
  BnRef bn;
  int bn_idx;          // 1-based Keras index
  bool pool;           // MaxPool2D() behind the activation
  int Ho, Wo;          // what leaves the layer
  float drop_keep;     // 1: no Dropout behind the activation
  uint32_t drop_id;    // its layer id for the counter RNG
};

struct C2Program : NetProgram {
  const kws_net* net = nullptr;
  int H0 = 98, W0 = 40;
  int act = KWS_ACT_RELU6;
  std::vector<C2Layer> layers;
  int64_t dk = 0, db = 0;
  int T = 0, C = 0, NC = 0;   // the tail averages [T, C]
  float tail_keep = 1.f;

  int64_t workspace_bytes(int B, int training) const override;
  int debug_view(int B, int training, int what, int index, int64_t* offset_floats, int64_t* count) const override;
  int predict(const float* params, const float* state, const float* x, int B, float* probs, float* ws, int64_t ws_bytes,
              hipStream_t st) const override;
  int train(const float* params, float* state, const float* x, const float* y_onehot, int B, float* grads, float* probs, float* metrics,
            uint64_t seed, uint32_t step, int64_t row_offset, int loss_batch, float* ws, int64_t ws_bytes, hipStream_t st) const override;
};

constexpr float C2_MOBILE_KEEP = 0.95f;       // Dropout(0.05), model.py:574-583
constexpr float C2_MOBILE_TAIL_KEEP = 0.9f;   // Dropout(0.1), model.py:586
constexpr uint32_t C2_DROP_ID0 = 2;           // the ladder's Dropout layers draw with ids 2, 3, ...; the tail's with id 1

// Preprocess (model.py:13-16): clip((x + 0.8) / 7, -5, 5); no gradient flows to the input
__global__ __launch_bounds__(256) void preprocess_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t n) {
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    out[i] = fminf(fmaxf((x[i] + 0.8f) / 7.0f, -5.f), 5.f);
}

// The bias the GEMM leaves out.  training: the batch mean of y + b is mean(y) + b, so moving_mean += (1 - momentum) * b on top of
// the finalise's update.  inference: bn(y + b) = scale * y + (shift + scale * b).
__global__ __launch_bounds__(256) void bias_fix_kernel(const float* __restrict__ bias, float* __restrict__ mm, float* __restrict__ bn,
                                                       int C, float one_minus_momentum, int training) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  if (training) mm[c] = fmaf(one_minus_momentum, bias[c], mm[c]);
  else bn[C + c] = fmaf(bn[c], bias[c], bn[C + c]);
}

struct C2Layout {
  int64_t total = 0;
  int64_t xp = 0;
  std::vector<int64_t> y, bn, o;   // o: the materialised output of a layer (pooled, dropped, or the last activation), 0 = none
  int64_t act = 0;                 // activated tensor in front of a Dropout
  int64_t stats = 0, dA[2] = {0, 0}, part = 0, coef = 0, wws = 0;
  int64_t fd = 0, dl = 0, per_loss = 0, per_correct = 0, swg = 0;
};

// does layer i leave a materialised tensor behind?
bool c2_materialised(const C2Program& p, int i, bool training) {
  const C2Layer& l = p.layers[i];
  return l.pool || (training && l.drop_keep < 1.f) || i + 1 == (int)p.layers.size();
}

void c2_layout(const C2Program& p, int B, bool training, C2Layout* lo) {
  Bump bp;
  const int n = (int)p.layers.size();
  lo->xp = bp.take((int64_t)B * p.H0 * p.W0);
  lo->y.assign(n, 0);
  lo->bn.assign(n, 0);
  lo->o.assign(n, 0);
  int64_t max_act = 64, max_stats = 64, max_part = 64, max_coef = 64, max_wws = 64, max_drop = 64;
  for (int i = 0; i < n; ++i) {
    kws_conv2d_t d = p.layers[i].d;
    d.B = B;
    const int F = d.F;
    const int64_t M = (int64_t)B * d.Hout * d.Wout;
    lo->y[i] = bp.take(M * F);
    lo->bn[i] = bp.take((int64_t)4 * F);
    if (c2_materialised(p, i, training)) lo->o[i] = bp.take((int64_t)B * p.layers[i].Ho * p.layers[i].Wo * F);
    if (p.layers[i].pool) max_part = std::max(max_part, kws_pool2x2_bwd_part_floats(B, d.Hout, d.Wout, F));
    if (p.layers[i].drop_keep < 1.f) max_drop = std::max(max_drop, M * F);
    max_act = std::max(max_act, std::max(M * F, (int64_t)B * d.H * d.W * d.Cin));
    max_stats = std::max(max_stats, (int64_t)kws_conv2d_stats_rows(&d) * 2 * F);
    max_part = std::max(max_part, (int64_t)kws_gbn_bwd_rows(M) * 2 * F);
    max_coef = std::max(max_coef, (int64_t)2 * F);
    max_wws = std::max(max_wws, kws_conv2d_wgrad_workspace_floats(&d));
  }
  lo->stats = bp.take(max_stats);
  if (training) {
    lo->act = bp.take(max_drop);
    lo->dA[0] = bp.take(max_act);
    lo->dA[1] = bp.take(max_act);
    lo->part = bp.take(max_part);
    lo->coef = bp.take(max_coef);
    lo->wws = bp.take(max_wws);
    lo->fd = bp.take((int64_t)B * p.C);
    lo->dl = bp.take((int64_t)B * p.NC);
    lo->per_loss = bp.take(B);
    lo->per_correct = bp.take(B);
    lo->swg = bp.take((int64_t)KWS_SMALL_WGRAD_SLICES * p.C * p.NC);
  }
  lo->total = bp.cur * 4;
}

// what layer i convolves: the preprocessed input, the materialised output of the layer before it, or that layer's raw output
// with its table (applied on load)
struct C2Input {
  const float* in;
  const float* bn;
};
C2Input c2_input(const C2Program& p, const C2Layout& lo, int i, const float* ws, bool training) {
  if (i == 0) return {ws + lo.xp, nullptr};
  if (c2_materialised(p, i - 1, training)) return {ws + lo.o[i - 1], nullptr};
  return {ws + lo.y[i - 1], ws + lo.bn[i - 1]};
}

int c2_forward(const C2Program& p, const C2Layout& lo, const float* params, float* state, const float* x, int B, bool training, float* ws,
               uint64_t seed, uint32_t step, int64_t row_offset, hipStream_t st) {
  const int64_t n_in = (int64_t)B * p.H0 * p.W0;
  hipLaunchKernelGGL(preprocess_kernel, dim3((unsigned)std::min<int64_t>(ceil_div64(n_in, 256), 4096)), dim3(256), 0, st, x, ws + lo.xp,
                     n_in);
  KWS_LAUNCH_CHECK("preprocess_kernel");
  for (int i = 0; i < (int)p.layers.size(); ++i) {
    const C2Layer& l = p.layers[i];
    kws_conv2d_t d = l.d;
    d.B = B;
    const int F = d.F;
    const int64_t M = (int64_t)B * d.Hout * d.Wout;
    const C2Input in = c2_input(p, lo, i, ws, training);
    const kws_gbn_refs r = kws_gbn_layer_refs(l.bn, params, state);
    const kws_gbn_cols cols = kws_gbn_grouped(1, F);
    KWS_TRY(kws_conv2d_fwd_f32(in.in, in.bn, params + l.w, ws + lo.y[i], training ? ws + lo.stats : nullptr, &d, st));
    if (training)
      KWS_TRY(kws_gbn_finalize(ws + lo.stats, kws_conv2d_stats_rows(&d), M, &cols, &r, KWS_BN_EPS, KWS_BN_MOMENTUM, ws + lo.bn[i], st));
    else
      KWS_TRY(kws_gbn_infer(&cols, &r, KWS_BN_EPS, ws + lo.bn[i], st));
    hipLaunchKernelGGL(bias_fix_kernel, dim3((unsigned)ceil_div(F, 256)), dim3(256), 0, st, params + l.bias, state + l.bn.mm,
                       ws + lo.bn[i], F, 1.f - KWS_BN_MOMENTUM, training ? 1 : 0);
    KWS_LAUNCH_CHECK("bias_fix_kernel");
    if (l.pool) {
      KWS_TRY(kws_pool2x2_fwd_f32(ws + lo.y[i], ws + lo.bn[i], ws + lo.o[i], B, d.Hout, d.Wout, F, p.act, st));
    } else if (training && l.drop_keep < 1.f) {
      KWS_TRY(kws_bn_relu6_apply(ws + lo.y[i], ws + lo.bn[i], ws + lo.act, M, F, 1, st));
      KWS_TRY(kws_dropout_fwd(ws + lo.act, ws + lo.o[i], B, d.Hout * d.Wout * F, l.drop_keep, seed, step, l.drop_id, row_offset, st));
    } else if (lo.o[i]) {   // the last activation, for the tail
      KWS_TRY(kws_bn_relu6_apply(ws + lo.y[i], ws + lo.bn[i], ws + lo.o[i], M, F, 1, st));
    }
  }
  return KWS_OK;
}

kws_gp_tail_args c2_tail_args(const C2Program& p, const C2Layout& lo, const float* params, const float* ws, int B, float* probs) {
  kws_gp_tail_args g;
  memset(&g, 0, sizeof(g));
  g.x = ws + lo.o.back(); g.Wd = params + p.dk; g.bd = params + p.db; g.probs = probs;
  g.B = B; g.T = p.T; g.C = p.C; g.NC = p.NC;
  g.pool_max = 0; g.loss_kind = 1;   // GlobalAveragePooling2D; keras categorical_crossentropy
  g.keep_prob = 1.f; g.loss_batch = 1;
  return g;
}

struct C2Spec {
  int F, kh, kw, stride, dh, dw;
  bool pool, drop;
};

int c2_add_layer(kws_net* n, C2Program* p, int idx, int H, int W, int Cin, const C2Spec& s, uint32_t* next_drop_id) {
  C2Layer l;
  memset(&l, 0, sizeof(l));
  kws_conv2d_t& d = l.d;
  d.B = 1; d.H = H; d.W = W; d.kh = s.kh; d.kw = s.kw; d.sh = s.stride; d.sw = s.stride; d.dh = s.dh; d.dw = s.dw;
  d.Cin = Cin; d.F = s.F; d.act = p->act;
  // TensorFlow SAME per axis with the dilated window d * (k - 1) + 1
  kws_same_pad(H, s.dh * (s.kh - 1) + 1, s.stride, &d.Hout, &d.pad_t);
  kws_same_pad(W, s.dw * (s.kw - 1) + 1, s.stride, &d.Wout, &d.pad_l);
  const std::string base = "conv2d_" + std::to_string(idx) + "/";
  l.w = kws_net_add_tensor(n, base + "kernel", {s.kh, s.kw, Cin, s.F}, false, 0.f, s.kh * s.kw * Cin, s.kh * s.kw * s.F, 0.f);
  l.bias = kws_net_add_tensor(n, base + "bias", {s.F}, false, 0.f, 0, 0, 0.f);
  l.bn = kws_net_add_bn(n, idx, s.F);
  l.bn_idx = idx;
  l.pool = s.pool;
  KWS_REQUIRE(!s.pool || (d.Hout >= 2 && d.Wout >= 2 && s.F % 4 == 0), "net: pooled 2-D layer %d x %d x %d", d.Hout, d.Wout, s.F);
  KWS_REQUIRE(p->act == KWS_ACT_RELU6 || s.pool, "net: a relu layer without a pool has no activation pass");
  l.Ho = s.pool ? d.Hout / 2 : d.Hout;
  l.Wo = s.pool ? d.Wout / 2 : d.Wout;
  l.drop_keep = s.drop ? C2_MOBILE_KEEP : 1.f;
  l.drop_id = s.drop ? (*next_drop_id)++ : 0;
  p->layers.push_back(l);
  return KWS_OK;
}

}  // namespace

int c2n_build(kws_net* n) {
  const kws_net_config_t& c = n->cfg;
  KWS_REQUIRE(c.input_size == 98 * 40, "net: conv_2d_%s input_size %d (the reference reshapes 98 x 40 mfcc features)",
              c.kind == KWS_NET_CONV_2D_MOBILE ? "mobile" : "fast", c.input_size);
  C2Program* p = new C2Program();
  n->program.reset(p);
  p->net = n;
  p->NC = c.num_classes;
  static const C2Spec mobile[8] = {{32, 3, 3, 2, 1, 1, false, false},  {32, 3, 3, 1, 1, 1, false, true},
                                   {64, 3, 3, 2, 1, 1, false, false},  {64, 3, 3, 1, 1, 1, false, true},
                                   {128, 3, 3, 2, 1, 1, false, false}, {128, 3, 3, 1, 1, 1, false, true},
                                   {256, 3, 3, 2, 1, 1, false, false}, {256, 3, 3, 1, 1, 1, false, true}};
  static const C2Spec fast[4] = {{16, 11, 5, 1, 2, 1, true, false}, {32, 5, 3, 1, 2, 1, true, false}, {64, 3, 3, 1, 1, 1, true, false},
                                 {128, 3, 3, 1, 1, 1, true, false}};
  const bool is_mobile = c.kind == KWS_NET_CONV_2D_MOBILE;
  p->act = is_mobile ? KWS_ACT_RELU6 : KWS_ACT_RELU;
  p->tail_keep = is_mobile ? C2_MOBILE_TAIL_KEEP : 1.f;
  const C2Spec* spec = is_mobile ? mobile : fast;
  int H = p->H0, W = p->W0, Cin = 1;
  uint32_t drop_id = C2_DROP_ID0;
  for (int i = 0; i < (is_mobile ? 8 : 4); ++i) {
    KWS_TRY(c2_add_layer(n, p, i + 1, H, W, Cin, spec[i], &drop_id));
    H = p->layers.back().Ho;
    W = p->layers.back().Wo;
    Cin = spec[i].F;
  }
  p->T = H * W;
  p->C = Cin;
  p->dk = kws_net_add_tensor(n, "dense_1/kernel", {p->C, p->NC}, false, 0.f, p->C, p->NC, 0.f);
  p->db = kws_net_add_tensor(n, "dense_1/bias", {p->NC}, false, 0.f, 0, 0, 0.f);
  return KWS_OK;
}

namespace {

int64_t C2Program::workspace_bytes(int B, int training) const {
  C2Layout lo;
  c2_layout(*this, B, training != 0, &lo);
  return lo.total;
}

int C2Program::debug_view(int B, int training, int what, int index, int64_t* offset_floats, int64_t* count) const {
  C2Layout lo;
  c2_layout(*this, B, training != 0, &lo);
  KWS_REQUIRE(index >= 0 && index < (int)layers.size(), "net_debug_view: layer index %d", index);
  const C2Layer& l = layers[index];
  if (what == 0) {          // raw output of conv2d_{index+1} (no bias): [B, Hout, Wout, F]
    *offset_floats = lo.y[index];
    *count = (int64_t)B * l.d.Hout * l.d.Wout * l.d.F;
  } else if (what == 1) {   // what the layer hands on: pooled / dropped / last activation [B, Ho, Wo, F] (count 0: read on load)
    *offset_floats = lo.o[index];
    *count = c2_materialised(*this, index, training != 0) ? (int64_t)B * l.Ho * l.Wo * l.d.F : 0;
  } else if (what == 2) {   // table of batch_normalization_{index+1}: scale|shift|mean|rstd [4][F]
    *offset_floats = lo.bn[index];
    *count = 4 * l.d.F;
  } else if (what == 3) {   // the preprocessed input [B, 98, 40, 1]
    *offset_floats = lo.xp;
    *count = (int64_t)B * H0 * W0;
  } else {
    kws_set_error("net_debug_view: unknown view %d", what);
    return KWS_E_INVALID;
  }
  return KWS_OK;
}

int C2Program::predict(const float* params, const float* state, const float* x, int B, float* probs, float* ws, int64_t ws_bytes,
                       hipStream_t st) const {
  C2Layout lo;
  c2_layout(*this, B, false, &lo);
  KWS_TRY(kws_workspace_check("net_predict", lo.total, ws_bytes, B));
  KWS_TRY(c2_forward(*this, lo, params, const_cast<float*>(state), x, B, false, ws, 0, 0, 0, st));
  const kws_gp_tail_args g = c2_tail_args(*this, lo, params, ws, B, probs);
  return kws_gp_tail_launch(&g, 0, st);
}

int C2Program::train(const float* params, float* state, const float* x, const float* y_onehot, int B, float* grads, float* probs,
                     float* metrics, uint64_t seed, uint32_t step, int64_t row_offset, int loss_batch, float* ws, int64_t ws_bytes,
                     hipStream_t st) const {
  const C2Program& p = *this;
  C2Layout lo;
  c2_layout(p, B, true, &lo);
  KWS_TRY(kws_workspace_check("net_train_fwd_bwd", lo.total, ws_bytes, B));
  KWS_HIP(hipMemsetAsync(grads, 0, (size_t)net->n_params * 4, st));   // the convolution biases' gradients stay exact zeros
  KWS_TRY(c2_forward(p, lo, params, state, x, B, true, ws, seed, step, row_offset, st));
  int cur = 0;
  kws_gp_tail_args g = c2_tail_args(p, lo, params, ws, B, probs);
  g.labels = y_onehot; g.dX = ws + lo.dA[cur]; g.fd = ws + lo.fd; g.dl = ws + lo.dl;
  g.per_loss = ws + lo.per_loss; g.per_correct = ws + lo.per_correct;
  g.seed = seed; g.step = step; g.keep_prob = p.tail_keep; g.loss_batch = loss_batch; g.row_offset = row_offset;
  KWS_TRY(kws_gp_tail_launch(&g, 1, st));
  KWS_TRY(kws_metrics_launch(g.per_loss, g.per_correct, B, metrics, st));
  KWS_TRY(kws_small_wgrad_launch(g.fd, g.dl, grads + p.dk, grads + p.db, B, p.C, p.NC, ws + lo.swg, st));
  for (int i = (int)p.layers.size() - 1; i >= 0; --i) {
    const C2Layer& l = p.layers[i];
    kws_conv2d_t d = l.d;
    d.B = B;
    const int F = d.F;
    const int64_t M = (int64_t)B * d.Hout * d.Wout;
    const kws_gbn_cols cols = kws_gbn_grouped(1, F);
    const int64_t boff = l.bn.beta - l.bn.gamma;
    if (l.pool) {   // dA[cur] = gradient wrt the pooled output: route it to the winners, gate it, BN sums in the same pass
      KWS_TRY(kws_pool2x2_bwd_f32(ws + lo.dA[cur], ws + lo.y[i], ws + lo.bn[i], ws + lo.dA[cur ^ 1], ws + lo.part, B, d.Hout, d.Wout, F,
                                  p.act, st));
      cur ^= 1;
      KWS_TRY(kws_gbn_bwd_finish(ws + lo.dA[cur], ws + lo.y[i], ws + lo.bn[i], M, &cols, ws + lo.part,
                                 kws_pool2x2_bwd_part_rows(B, d.Hout, d.Wout, F), ws + lo.coef, grads + l.bn.gamma, 0, boff, st));
    } else {
      if (l.drop_keep < 1.f) {   // back through the Dropout: the gradient wrt the activation
        KWS_TRY(kws_dropout_bwd(ws + lo.dA[cur], ws + lo.dA[cur ^ 1], B, d.Hout * d.Wout * F, l.drop_keep, seed, step, l.drop_id,
                                row_offset, st));
        cur ^= 1;
      }
      KWS_TRY(kws_gbn_bwd(ws + lo.dA[cur], ws + lo.y[i], ws + lo.bn[i], nullptr, M, &cols, ws + lo.part, ws + lo.coef, grads + l.bn.gamma,
                          0, boff, st));
    }
    const float* dy = ws + lo.dA[cur];
    const C2Input in = c2_input(p, lo, i, ws, true);
    KWS_TRY(kws_conv2d_wgrad_f32(in.in, in.bn, dy, grads + l.w, ws + lo.wws, &d, st));
    if (i > 0) {   // (the input has no gradient)
      KWS_TRY(kws_conv2d_dgrad_f32(dy, params + l.w, ws + lo.dA[cur ^ 1], &d, st));
      cur ^= 1;
    }
  }
  return KWS_OK;
}

}  // namespace
