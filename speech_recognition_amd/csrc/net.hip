// Network programs: the forward / forward+backward of one model as a native sequence of kernel
// launches on one HIP stream (no Python between layers, so the step can also be captured into a
// hipGraph by the caller).  SURVEY 8a rows a7-a15.  This file holds the public net entry points, the
// pieces every program shares, and the program of
//
//   KWS_NET_TS_ATTENTION  conv_1d_time_sliced_with_attention_model   reference model.py:775-838
//
// Data flow per depthwise block l (training; the blocks are the ladder of net_dw3ladder.hip, shared with net_time_sliced.hip):
//   z_l = dw_l( relu6(bn_{l-1}(y_{l-1})) )      BN+ReLU6 applied on load, never materialised
//   y_l = z_l W_l                                f32 MFMA GEMM, BN statistics in the epilogue
// Backward keeps two scratch tensors (G: gradient wrt a BN output / pre-BN tensor, DZ: gradient wrt
// a depthwise output) and walks the blocks in reverse.
#include "net_internal.h"
#include <math.h>
#include <stdlib.h>

int64_t kws_net_add_tensor(kws_net* n, const std::string& name, std::vector<int64_t> shape, bool is_state, float l2,
                           int fan_in, int fan_out, float init) {
  kws_tensor_info_t t;
  memset(&t, 0, sizeof(t));
  snprintf(t.name, sizeof(t.name), "%s", name.c_str());
  int64_t size = 1;
  t.ndim = (int)shape.size();
  for (int i = 0; i < t.ndim; ++i) {
    t.shape[i] = shape[i];
    size *= shape[i];
  }
  t.size = size;
  t.is_state = is_state ? 1 : 0;
  t.l2 = l2;
  t.fan_in = fan_in;
  t.fan_out = fan_out;
  t.init = init;
  int64_t& cursor = is_state ? n->n_state : n->n_params;
  t.offset = cursor;
  cursor += (size + 3) / 4 * 4;  // keep every tensor 16-B aligned inside the flat buffer
  n->tensors.push_back(t);
  return t.offset;
}

BnRef kws_net_add_bn(kws_net* n, int idx, int C) {
  BnRef r;
  const std::string base = "batch_normalization_" + std::to_string(idx) + "/";
  r.gamma = kws_net_add_tensor(n, base + "gamma", {C}, false, 0.f, 0, 0, 1.f);
  r.beta = kws_net_add_tensor(n, base + "beta", {C}, false, 0.f, 0, 0, 0.f);
  r.mm = kws_net_add_tensor(n, base + "moving_mean", {C}, true, 0.f, 0, 0, 0.f);
  r.mv = kws_net_add_tensor(n, base + "moving_variance", {C}, true, 0.f, 0, 0, 1.f);
  r.C = C;
  return r;
}

void kws_same_pad(int L, int k, int s, int* Lout, int* pl) {
  *Lout = (L + s - 1) / s;
  int p = (*Lout - 1) * s + k - L;
  if (p < 0) p = 0;
  *pl = p / 2;  // TF: extra padding goes to the right
}

int64_t KerasNames::conv(int k, int cin, int cout, float l2) {
  return kws_net_add_tensor(n, "conv1d_" + std::to_string(++n_conv) + "/kernel", {k, cin, cout}, false, l2, k * cin, k * cout,
                            0.f);
}
BnRef KerasNames::bn(int C, int* idx) {
  ++n_bn;
  if (idx) *idx = n_bn;
  return kws_net_add_bn(n, n_bn, C);
}
int64_t KerasNames::dw(int C) { return dwk(3, C); }
int64_t KerasNames::dwk(int k, int C) {
  return kws_net_add_tensor(n, "depthwise_conv2d_" + std::to_string(++n_dw) + "/depthwise_kernel", {1, k, C, 1}, false, KWS_L2_COEF,
                            k * C, k, 0.f);
}

int kws_workspace_check(const char* who, int64_t need_bytes, int64_t ws_bytes, int B) {
  if (need_bytes <= ws_bytes) return KWS_OK;
  kws_set_error("%s: workspace %lld B < %lld B needed for batch %d", who, (long long)ws_bytes, (long long)need_bytes, B);
  return KWS_E_WORKSPACE;
}

int kws_flat_tail_train(kws_flat_tail_args* t, const float* labels, float* fd, float* dl, float* dA, float* per_loss,
                        float* per_correct, uint64_t seed, uint32_t step, int loss_batch, int64_t row_offset, float* metrics,
                        hipStream_t st) {
  t->labels = labels; t->fd = fd; t->dl = dl; t->dA = dA;
  t->per_loss = per_loss; t->per_correct = per_correct;
  t->seed = seed; t->step = step; t->loss_batch = loss_batch; t->row_offset = row_offset;
  KWS_TRY(kws_flat_tail_launch(t, 1, st));
  return kws_metrics_launch(per_loss, per_correct, t->B, metrics, st);
}

namespace {

constexpr float DROP_KEEP = 0.6f;     // Dropout(0.4), model.py:819,828
constexpr float LABEL_SMOOTH = 0.1f;  // model.py:835-836

// ---- first convolution with overlapping taps, folded -------------------------------------------------
// Weff[s, n] = sum over taps j (ascending) with 0 <= s - hop*j < cin of W[j, s - hop*j, n]
__global__ __launch_bounds__(256) void fold_taps_kernel(const float* __restrict__ W, float* __restrict__ Weff, int taps,
                                                        int cin, int hop, int Kf, int N) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Kf * N) return;
  const int s = i / N, n = i - s * N;
  float acc = 0.f;
  for (int j = 0; j < taps; ++j) {
    const int c = s - hop * j;
    if (c >= 0 && c < cin) acc += W[((int64_t)j * cin + c) * N + n];
  }
  Weff[i] = acc;
}
// dW[j, c, n] = dWeff[hop*j + c, n]: every tap row reads the gradient of the sample it multiplies - the same sum
// over (clip, frame) as the unfolded weight-gradient GEMM, not a regrouping
__global__ __launch_bounds__(256) void unfold_taps_kernel(const float* __restrict__ dWeff, float* __restrict__ dW, int taps,
                                                          int cin, int hop, int N) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= taps * cin * N) return;
  const int n = i % N, jc = i / N;
  const int j = jc / cin, c = jc - j * cin;
  dW[i] = dWeff[(int64_t)(hop * j + c) * N + n];
}
// ---- workspace layout ------------------------------------------------------------------------------
struct Layout {
  int64_t total = 0;  // bytes
  Dw3Offsets a;             // the ladder's activations, BatchNorm tables and transposed pointwise kernels (float offsets)
  int64_t G = 0, G2 = 0, DZ = 0, part = 0, coef = 0, tn = 0, red = 0, swg = 0, swg1 = 0;
  int64_t tns = 0, tns_cap = 0;   // the blocks' weight-gradient slabs: one region, summed in ONE launch (KwsSlabQueue)
  std::vector<int64_t> WPf, WPd;  // fp16 x 2 arm: fp16 planes [2][cout][cin] (forward) / [2][cin][cout] (input gradient)
  int64_t amax = 0;               // fp16 x 2 arm: 3 nb slot groups of |x| maxima: W[i] | z[i] | dy[i + 1]
  int64_t xd = 0, fd = 0, dl1 = 0, dl2 = 0, per_loss = 0, per_correct = 0, att = 0;
  int64_t w1f = 0, g1f = 0;  // folded first-convolution kernel and its gradient [K1f, C1]
};

// The layer table of the raw-waveform attention net and its launch sequences
struct TsProgram : NetProgram {
  const kws_net* net = nullptr;   // n_params, gemm_mode
  int L_in = 0;        // samples per clip
  int64_t conv1 = 0;
  Dw3Ladder lad;       // L1, C1, bn1: the first convolution's output
  int T = 0, C = 0, NC = 0;
  int64_t d1k = 0, d1b = 0, d2k = 0;
  kws_gather_t gather1;   // the reference's view: 3 taps of 40 samples, taps 20 samples apart (K = 120)
  kws_gather_t gather1f;  // folded view used by the GEMMs: ONE tap of 80 contiguous samples (see fold_taps_kernel)
  int K1f = 0;            // folded K

  void make_layout(int B, bool training, Layout* lo) const;
  int fold_conv1(const float* params, float* w1f, hipStream_t st) const;
  int unfold_conv1(const float* g1f, float* grads, hipStream_t st) const;
  // fp16 x 2 arm: the slot groups of |x| maxima of W[i] / z[i] / dy of block i's output
  unsigned* slots(const Layout& lo, float* ws, int group, int i) const {
    return reinterpret_cast<unsigned*>(ws + lo.amax) + (int64_t)(group * lad.nb() + i) * KWS_ABSMAX_WORDS;
  }
  int split_kernels(const Layout& lo, const float* params, float* ws, bool training, hipStream_t st) const;
  int blocks_fwd(const Layout& lo, const Dw3Run& r, bool h2, float* stats) const;
  int64_t workspace_bytes(int B, int training) const override;
  int debug_view(int B, int training, int what, int index, int64_t* offset_floats, int64_t* count) const override;
  int predict(const float* params, const float* state, const float* x, int B, float* probs, float* ws, int64_t ws_bytes,
              hipStream_t st) const override;
  int train(const float* params, float* state, const float* x, const float* y_onehot, int B, float* grads, float* probs, float* metrics,
            uint64_t seed, uint32_t step, int64_t row_offset, int loss_batch, float* ws, int64_t ws_bytes, hipStream_t st) const override {
    return train_part(params, state, x, y_onehot, B, grads, probs, metrics, seed, step, row_offset, loss_batch, ws, ws_bytes, st, 0, 0);
  }
  int train_part(const float* params, float* state, const float* x, const float* y_onehot, int B, float* grads, float* probs,
                 float* metrics, uint64_t seed, uint32_t step, int64_t row_offset, int loss_batch, float* ws, int64_t ws_bytes,
                 hipStream_t st, int phase, int split) const;
};

int ts_build(kws_net* n) {
  TsProgram* p = new TsProgram();
  n->program.reset(p);
  p->net = n;
  const kws_net_config_t& c = n->cfg;
  KWS_REQUIRE(c.filter_mult >= 1 && c.filter_mult <= 2, "net: filter_mult %d unsupported", c.filter_mult);
  KWS_REQUIRE(c.input_size >= 1600 && c.input_size % 4 == 0, "net: input_size %d unsupported", c.input_size);
  const int fm = c.filter_mult;
  p->L_in = c.input_size;
  // overlapping_time_slice_stack(x, 40, 20) SAME (model.py:805) fused with Conv1D(128,3,strides=2) (model.py:807)
  int Lf, plf;
  kws_same_pad(p->L_in, 40, 20, &Lf, &plf);
  Dw3Ladder& lad = p->lad;
  lad.L1 = (Lf - 3) / 2 + 1;
  lad.C1 = 128 * fm;
  KerasNames kn{n};
  p->conv1 = kn.conv(3, 40, lad.C1, KWS_L2_COEF);
  lad.bn1 = kn.bn(lad.C1);
  kws_gather_t g;
  g.L_out = lad.L1; g.cin = 40; g.taps = 3; g.stride_t = 2 * 20; g.stride_j = 20; g.base_off = -plf;
  g.x_len = p->L_in; g.x_batch_stride = p->L_in;
  p->gather1 = g;
  // The three taps overlap (tap j covers samples 20 j .. 20 j + 39 of an 80-sample span): the convolution is a GEMM
  // over the 80 DISTINCT samples with the kernel rows that hit the same sample added up front - 2/3 of the FLOPs.
  p->K1f = g.stride_j * (g.taps - 1) + g.cin;
  kws_gather_t gf = g;
  gf.cin = p->K1f; gf.taps = 1; gf.stride_j = 0;
  p->gather1f = gf;
  static const int spec[11][2] = {{1, 128}, {2, 192}, {1, 192}, {2, 256}, {1, 256}, {2, 320},
                                  {1, 320}, {2, 384}, {1, 384}, {2, 512}, {1, 512}};  // model.py:812-817
  KWS_TRY(lad.build(kn, spec, 11, fm, c.input_size));
  p->T = lad.blocks.back().Lout;
  p->C = lad.blocks.back().cout;
  p->NC = c.num_classes;
  KWS_REQUIRE(p->T <= 16, "net: %d time steps at the tail (max 16)", p->T);
  p->d1k = kws_net_add_tensor(n, "dense_1/kernel", {(int64_t)p->T * p->C, p->T}, false, KWS_L2_COEF, p->T * p->C, p->T, 0.f);
  p->d1b = kws_net_add_tensor(n, "dense_1/bias", {p->T}, false, 0.f, 0, 0, 0.f);
  p->d2k = kws_net_add_tensor(n, "dense_2/kernel", {2 * p->C, p->NC}, false, KWS_L2_COEF, 2 * p->C, p->NC, 0.f);
  return KWS_OK;
}

int TsProgram::fold_conv1(const float* params, float* w1f, hipStream_t st) const {
  const kws_gather_t& g = gather1;
  const int n = K1f * lad.C1;
  hipLaunchKernelGGL(fold_taps_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, params + conv1, w1f, g.taps, g.cin,
                     g.stride_j, K1f, lad.C1);
  KWS_LAUNCH_CHECK("fold_taps_kernel");
  return KWS_OK;
}
int TsProgram::unfold_conv1(const float* g1f, float* grads, hipStream_t st) const {
  const kws_gather_t& g = gather1;
  const int n = g.taps * g.cin * lad.C1;
  hipLaunchKernelGGL(unfold_taps_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, g1f, grads + conv1, g.taps, g.cin,
                     g.stride_j, lad.C1);
  KWS_LAUNCH_CHECK("unfold_taps_kernel");
  return KWS_OK;
}

void TsProgram::make_layout(int B, bool training, Layout* lo) const {
  Bump bp;
  const int nb = lad.nb(), C1 = lad.C1;
  const std::vector<Dw3Block>& blocks = lad.blocks;
  const int64_t M1 = (int64_t)B * lad.L1;
  const Dw3Sizes s = lad.sizes(B);
  // statistics rows of either first-convolution kernel
  const int64_t max_part =
      std::max(s.max_part, std::max((int64_t)kws_gemm_num_row_tiles(M1), (int64_t)kws_conv1_stats_rows(M1)) * 2 * C1);
  int64_t max_tn = std::max(kws_gemm_tn_workspace_floats(M1, K1f, C1), kws_conv1_wgrad_workspace_floats(M1));
  lo->tns_cap = 0;
  for (const Dw3Block& b : blocks) {
    const int64_t M = (int64_t)B * b.Lout, t = kws_gemm_tn_workspace_floats(M, b.cin, b.cout);
    max_tn = std::max(max_tn, std::max(t, kws_gemm_tn_f16x2_workspace_floats(M, b.cin, b.cout)));   // either arithmetic (run-time switch)
    lo->tns_cap += (t + 63) / 64 * 64;
  }
  lad.take_acts(bp, B, training, s, &lo->a);
  if (training) {
    lo->G = bp.take(s.max_y);
    lo->G2 = bp.take(s.max_y);
    lo->DZ = bp.take(s.max_z);
    const int64_t tail_part = (int64_t)B * 5 * C;
    lo->part = bp.take(std::max(std::max(max_part, s.max_dwpart), tail_part));
    lo->coef = bp.take(2 * s.maxC);
    lo->red = bp.take((int64_t)KWS_REDUCE_SLICES * 5 * s.maxC);
    lo->swg = bp.take((int64_t)KWS_SMALL_WGRAD_SLICES *
                      std::max((int64_t)T * C * T, (int64_t)2 * C * NC));
    // the attention dense layer's slices keep a region of their own (both dense layers' slices wait for the call's slab sum)
    lo->swg1 = bp.take((int64_t)KWS_SMALL_WGRAD_SLICES * T * C * T);
    lad.take_WT(bp, &lo->a);
    lo->WPf.assign(nb, 0);
    lo->WPd.assign(nb, 0);
    for (int i = 0; i < nb; ++i) {                  // 2 fp16 per weight = 1 float; taken in every mode (1.2 M weights in all)
      lo->WPf[i] = bp.take((int64_t)blocks[i].cin * blocks[i].cout);
      lo->WPd[i] = bp.take((int64_t)blocks[i].cin * blocks[i].cout);
    }
    lo->amax = bp.take((int64_t)3 * nb * KWS_ABSMAX_WORDS);
    lo->tn = bp.take(max_tn);
    lo->tns = bp.take(lo->tns_cap);
    lo->xd = bp.take((int64_t)B * T * C);
    lo->fd = bp.take((int64_t)B * 2 * C);
    lo->dl1 = bp.take((int64_t)B * T);
    lo->dl2 = bp.take((int64_t)B * NC);
    lo->per_loss = bp.take(B);
    lo->per_correct = bp.take(B);
    lo->att = bp.take((int64_t)B * 16);
    lo->g1f = bp.take((int64_t)K1f * C1);
  } else {
    lo->part = bp.take(64);
    lo->WPf.assign(nb, 0);                          // the split-GEMM arms in inference: forward planes and |x| maxima (W | z)
    for (int i = 0; i < nb; ++i) lo->WPf[i] = bp.take((int64_t)blocks[i].cin * blocks[i].cout);
    lo->amax = bp.take((int64_t)2 * nb * KWS_ABSMAX_WORDS);
  }
  lo->w1f = bp.take((int64_t)K1f * C1);
  lad.take_bn(bp, s.maxC, &lo->a);
  lo->total = bp.cur * 4;
}

int64_t TsProgram::workspace_bytes(int B, int training) const {
  Layout lo;
  make_layout(B, training != 0, &lo);
  return lo.total;
}

int TsProgram::debug_view(int batch, int training, int what, int index, int64_t* offset_floats, int64_t* count) const {
  Layout lo;
  make_layout(batch, training != 0, &lo);
  if (what >= 0 && what <= 2) return lad.debug_view(lo.a, batch, what, index, offset_floats, count);
  if (what == 3) {  // attention weights [B, T] (training only)
    KWS_REQUIRE(training, "net_debug_view: att is a training-only view");
    *offset_floats = lo.att;
    *count = (int64_t)batch * T;
  } else {
    kws_set_error("net_debug_view: unknown view %d", what);
    return KWS_E_INVALID;
  }
  return KWS_OK;
}

// fp16 x 2 arm (kws_net_set_gemm_mode(net, 2), gemm_f16x2.hip): maxima of the pointwise kernels (this also zeroes their slot
// groups), zero the activations' groups, then the kernels as fp16 planes: the forward form and, in training, the input-gradient form
int TsProgram::split_kernels(const Layout& lo, const float* params, float* ws, bool training, hipStream_t st) const {
  const int nb = lad.nb(), per = training ? 2 : 1;
  const float *win[24], *sin_[24];
  int64_t wn[24];
  void* sout[24];
  const unsigned* ssl[24];
  int srows[24], scols[24], str[24];
  KWS_REQUIRE(per * nb <= 24, "net: %d blocks exceed the split batch", nb);
  for (int i = 0; i < nb; ++i) {
    const Dw3Block& b = lad.blocks[i];
    win[i] = params + b.pw;
    wn[i] = (int64_t)b.cin * b.cout;
    for (int k = 0; k < per; ++k) {
      const int j = per * i + k;
      sin_[j] = win[i]; srows[j] = b.cin; scols[j] = b.cout; ssl[j] = slots(lo, ws, 0, i);
      sout[j] = ws + (k ? lo.WPd[i] : lo.WPf[i]); str[j] = k ? 0 : 1;
    }
  }
  KWS_TRY(kws_absmax_batch_f32(win, wn, slots(lo, ws, 0, 0), nb, st));
  KWS_HIP(hipMemsetAsync(slots(lo, ws, 1, 0), 0, (size_t)per * nb * KWS_ABSMAX_WORDS * sizeof(unsigned), st));
  return kws_f16x2_split_batch(sin_, sout, srows, scols, str, ssl, per * nb, st);
}

// The blocks' forward: the ladder's f32 step, or under the fp16 x 2 arm (h2) the split-product GEMM between the ladder's depthwise
// step and its statistics step for every layer the arm's kernels take.  stats: the statistics rows, NULL in inference
int TsProgram::blocks_fwd(const Layout& lo, const Dw3Run& r, bool h2, float* stats) const {
  for (int i = 0; i < lad.nb(); ++i) {
    const Dw3Block& b = lad.blocks[i];
    const int64_t M = (int64_t)r.B * b.Lout;
    unsigned* zs = h2 ? slots(lo, r.ws, 1, i) : nullptr;
    if (h2 && kws_gemm_nn_f16x2_supported(M, b.cin, b.cout)) {
      KWS_TRY(lad.fwd_dw(i, r, zs));
      KWS_TRY(kws_gemm_nn_f16x2_f32(r.z(i), r.ws + lo.WPf[i], r.y(i + 1), M, b.cin, b.cout, zs, slots(lo, r.ws, 0, i), stats, r.st));
      if (stats) KWS_TRY(lad.stats_finalize(i, r, stats, kws_gemm_nn_f16x2_stats_rows(M)));
    } else {
      KWS_TRY(lad.fwd_block_f32(i, r, stats, zs));
    }
  }
  return KWS_OK;
}

int TsProgram::predict(const float* params, const float* state, const float* x, int B, float* probs, float* ws, int64_t ws_bytes,
                       hipStream_t st) const {
  Layout lo;
  make_layout(B, false, &lo);
  KWS_TRY(kws_workspace_check("net_predict", lo.total, ws_bytes, B));
  const int nb = lad.nb(), C1 = lad.C1;
  const Dw3Run r{&lo.a, params, const_cast<float*>(state), nullptr, ws, B, nullptr, nullptr, nullptr, nullptr, st};   // state is only read
  KWS_TRY(lad.infer_tables(r));
  if (kws_conv1_supported(&gather1f, &gather1, C1)) {
    KWS_TRY(kws_conv1_fwd(x, &gather1f, &gather1, params + conv1, r.y(0), B, C1, nullptr, st));
  } else {
    KWS_TRY(fold_conv1(params, ws + lo.w1f, st));
    KWS_TRY(kws_gemm_gather_f32(x, &gather1f, ws + lo.w1f, r.y(0), B, C1, nullptr, st));
  }
  const bool h2 = kws_net_get_gemm_mode(net) == 2;
  if (h2) KWS_TRY(split_kernels(lo, params, ws, false, st));
  KWS_TRY(blocks_fwd(lo, r, h2, nullptr));
  kws_ts_tail_args t;
  memset(&t, 0, sizeof(t));
  t.y = r.y(nb); t.bn = r.bn_at(nb); t.W1 = params + d1k; t.b1 = params + d1b;
  t.W2 = params + d2k; t.probs = probs; t.B = B; t.T = T; t.C = C; t.NC = NC;
  t.keep_prob = 1.f; t.loss_batch = 1; t.train = 0;
  return kws_ts_tail_launch(&t, st);
}

// part 0: the whole step.  part 1: forward, tail and the backward pass down to block `split` (inclusive); part 2: the rest
// of the backward pass (blocks split-1 .. 0 and the first convolution).  Parts 1 + 2 enqueue exactly the launches of
// part 0 in the same order - every intermediate lives in the caller's workspace - so the gradients are bit-identical.
int TsProgram::train_part(const float* params, float* state, const float* x, const float* y_onehot, int B, float* grads, float* probs,
                          float* metrics, uint64_t seed, uint32_t step, int64_t row_offset, int loss_batch, float* ws, int64_t ws_bytes,
                          hipStream_t st, int phase, int split) const {
  Layout lo;
  make_layout(B, true, &lo);
  KWS_TRY(kws_workspace_check("net_train_fwd_bwd", lo.total, ws_bytes, B));
  const int nb = lad.nb(), C1 = lad.C1;
  float* part = ws + lo.part;
  float* DZ = ws + lo.DZ;
  float* coef = ws + lo.coef;
  float* red = ws + lo.red;
  const Dw3Run r{&lo.a, params, state, grads, ws, B, red, part, coef, DZ, st};
  const bool conv1_direct = kws_conv1_supported(&gather1f, &gather1, C1);   // conv1.hip takes the shape; else the gathered GEMMs
  const bool run_head = phase != 2;                   // forward + tail + the late blocks' backward
  // Gemm mode 0: f32 MFMA, a layer's input- and weight-gradient GEMMs as one launch.  Mode 1: the same arithmetic with separate
  // launches (the A/B reference).  Mode 2, the fp16 x 2 arm: the pointwise forward, input-gradient and weight-gradient GEMMs run as
  // three f16 MFMA products of scaled two-way operand splits; the first convolution stays f32, and so does any GEMM whose shape
  // the arm's kernels cannot take (kws_gemm_*_f16x2_supported: K granule, 2 GB buffer views)
  const int gmode = kws_net_get_gemm_mode(net);
  const bool h2 = gmode == 2;
  auto w_slots = [&](int i) { return slots(lo, ws, 0, i); };
  auto z_slots = [&](int i) { return slots(lo, ws, 1, i); };
  auto g_slots = [&](int i) { return slots(lo, ws, 2, i); };
  float* Gb[2] = {ws + lo.G, ws + lo.G2};          // gradient wrt y[l] lives in Gb[l % 2]; the tail writes Gb[nb % 2]
  // the f32 weight-gradient GEMMs leave their slabs in lo.tns; ONE launch sums them when this call's blocks are done.  The queue
  // cannot flush before: lo.tns_cap is the sum of the blocks' needs, and the tail's two entries + nb blocks fit one batch
  KwsSlabQueue q;
  q.base = ws + lo.tns;
  q.cap = lo.tns_cap;
  q.allow_pair = gmode == 0;
  KWS_REQUIRE(nb + 2 <= KWS_SLAB_BATCH, "net: %d blocks exceed the slab batch", nb);
  if (run_head) {
    KWS_HIP(hipMemsetAsync(grads, 0, (size_t)net->n_params * 4, st));
    if (h2) KWS_TRY(split_kernels(lo, params, ws, true, st));
    // ---------------- forward ----------------
    {
      const int64_t M = (int64_t)B * lad.L1;
      const BnRef& bn1 = lad.bn1;
      if (conv1_direct) {
        KWS_TRY(kws_conv1_fwd(x, &gather1f, &gather1, params + conv1, r.y(0), B, C1, part, st));
      } else {
        KWS_TRY(fold_conv1(params, ws + lo.w1f, st));
        KWS_TRY(kws_gemm_gather_f32(x, &gather1f, ws + lo.w1f, r.y(0), B, C1, part, st));
      }
      const int rows1 = conv1_direct ? kws_conv1_stats_rows(M) : kws_gemm_gather_stats_rows(M);
      KWS_TRY(kws_bn_stats_finalize(part, rows1, M, C1, params + bn1.gamma, params + bn1.beta, KWS_BN_EPS, KWS_BN_MOMENTUM,
                                    state + bn1.mm, state + bn1.mv, r.bn_at(0), red, st));
    }
    KWS_TRY(blocks_fwd(lo, r, h2, part));
    // ---------------- tail forward + backward ----------------
    kws_ts_tail_args t;
    memset(&t, 0, sizeof(t));
    t.y = r.y(nb); t.bn = r.bn_at(nb); t.W1 = params + d1k; t.b1 = params + d1b;
    t.W2 = params + d2k; t.labels = y_onehot; t.probs = probs; t.g = Gb[nb % 2]; t.part = part; t.xd = ws + lo.xd;
    t.fd = ws + lo.fd; t.dl1 = ws + lo.dl1; t.dl2 = ws + lo.dl2; t.per_loss = ws + lo.per_loss;
    t.per_correct = ws + lo.per_correct; t.att = ws + lo.att; t.B = B; t.T = T; t.C = C; t.NC = NC; t.seed = seed;
    t.step = step; t.keep_prob = DROP_KEEP; t.label_smoothing = LABEL_SMOOTH; t.loss_batch = loss_batch;
    t.row_offset = row_offset; t.train = 1;
    KWS_TRY(kws_ts_tail_launch(&t, st));
    // off the dependency chain: metrics, the two dense layers' weight gradients, the attention bias gradient.  Gemm mode 0: ONE
    // launch writes the metrics, the bias gradient and the weight gradients' SLICES (tail.hip tail_post_kernel); the slices are
    // queued in front of the pointwise layers' slabs and summed with them (in kws_small_wgrad_launch's own order, the negative
    // count: bit-identical).  Mode 1 / shapes the fused kernel does not take: metrics and the two small weight-gradient launches.
    bool tail_fused = false;
    if (gmode == 0) {
      kws_tail_post_args tp;
      tp.X2 = t.fd; tp.D2 = t.dl2; tp.ws2 = ws + lo.swg; tp.K2 = 2 * C; tp.N2 = NC;
      tp.X1 = t.xd; tp.D1 = t.dl1; tp.ws1 = ws + lo.swg1; tp.K1 = T * C; tp.N1 = T;
      tp.bias1 = grads + d1b; tp.per_loss = t.per_loss; tp.per_correct = t.per_correct; tp.metrics = metrics; tp.B = B;
      int S_tail = 0;
      const int rc = kws_tail_post_launch(&tp, &S_tail, st);
      if (rc < 0) return rc;
      tail_fused = rc == 0;
      if (tail_fused && S_tail > 0) {
        KWS_TRY(q.push(ws + lo.swg, grads + d2k, (int64_t)2 * C * NC, -S_tail, st));
        KWS_TRY(q.push(ws + lo.swg1, grads + d1k, (int64_t)T * C * T, -S_tail, st));
      }
    }
    if (!tail_fused) {
      KWS_TRY(kws_metrics_launch(t.per_loss, t.per_correct, B, metrics, st));
      KWS_TRY(kws_small_wgrad_launch(t.fd, t.dl2, grads + d2k, nullptr, B, 2 * C, NC, ws + lo.swg, st));
      KWS_TRY(kws_small_wgrad_launch(t.xd, t.dl1, grads + d1k, grads + d1b, B, T * C, T, ws + lo.swg, st));
    }
    const BnRef& last = lad.blocks[nb - 1].bn;
    KWS_TRY(kws_dw_bwd_finalize(part, B, (int64_t)B * T, last.C, nullptr, grads + last.gamma, grads + last.beta, coef, red, st));
    // ---------------- backward through the blocks ----------------
    // One stream: the weight-gradient GEMM of a block depends only on dy and z and COULD run beside the HBM-bound depthwise /
    // BN kernels, but the early-layer GEMMs (32 FLOP/B) draw 3.7 TB/s themselves - with the fused two-pass depthwise
    // backward a side-stream program took the same 5.14 - 5.20 ms (measured, then removed).
    // The f32 dgrad GEMMs read the pointwise kernels transposed (the fp16 arm too, for the layers it hands back)
    KWS_TRY(lad.transpose_all(r));
  }
  const int i_hi = phase == 2 ? split - 1 : nb - 1, i_lo = phase == 1 ? split : 0;
  for (int i = i_hi; i >= i_lo; --i) {
    const Dw3Block& b = lad.blocks[i];
    const int64_t M = (int64_t)B * b.Lout;
    float* Gcur = Gb[(i + 1) % 2];
    // Gcur holds dy of this block's pointwise output: written by the depthwise backward of block i+1 (pass 2); only the tail
    // hands over a masked gradient that still needs its BatchNorm backward
    if (i == nb - 1)
      KWS_TRY(kws_bn_bwd_apply_amax(Gcur, r.y(i + 1), r.bn_at(i + 1), params + b.bn.gamma, coef, M, b.cout, h2 ? g_slots(i) : nullptr, st));
    // DZ = Gcur WT and the slabs of dW = z^T Gcur.  The two are independent: in mode 0 they go out as ONE launch whose weight-
    // gradient workgroups start on a CU as soon as its input-gradient workgroup has ended (gemm.hip gemm_dgrad_wgrad_kernel; same
    // code, bit-identical dZ and slabs); mode 1, and any shape the fused kernel does not take, makes the two launches
    if (!h2) {
      KWS_TRY(q.pair(Gcur, r.WT(i), DZ, r.z(i), grads + b.pw, M, b.cin, b.cout, st));
    } else {
      if (kws_gemm_nn_f16x2_supported(M, b.cout, b.cin))
        KWS_TRY(kws_gemm_nn_f16x2_f32(Gcur, ws + lo.WPd[i], DZ, M, b.cout, b.cin, g_slots(i), w_slots(i), nullptr, st));
      else
        KWS_TRY(kws_gemm_nn_f32(Gcur, r.WT(i), DZ, M, b.cout, b.cin, nullptr, st));
      if (kws_gemm_tn_f16x2_supported(M, b.cin, b.cout))
        KWS_TRY(kws_gemm_tn_f16x2_f32(r.z(i), Gcur, grads + b.pw, M, b.cin, b.cout, z_slots(i), g_slots(i), ws + lo.tn, st));
      else
        KWS_TRY(q.gemm(r.z(i), Gcur, grads + b.pw, M, b.cin, b.cout, st));
    }
    KWS_TRY(lad.bwd_block_input(i, r, Gb[i % 2], (h2 && i > 0) ? g_slots(i - 1) : nullptr));
  }
  // the slab sums of this call's pointwise weight gradients: beside the first convolution's weight gradient in ONE launch when
  // that kernel runs in this call (conv1_wgrad_slabsum_kernel - the two are independent, one is MFMA / memory bound, the
  // other HBM bound), their own launch otherwise (a part's gradients are final when it returns)
  const bool sum_with_conv1 = q.count > 0 && phase != 1 && conv1_direct && gmode != 1;
  if (!sum_with_conv1) KWS_TRY(q.flush(st));
  if (phase != 1) {                                   // Gb[0] holds dy of the first convolution
    if (conv1_direct) {
      KWS_TRY(kws_conv1_wgrad_slabs(x, &gather1f, &gather1, Gb[0], grads + conv1, B, C1, ws + lo.tn, q.ws, q.out, q.n, q.S,
                                    q.hand_over(), st));
    } else {
      KWS_TRY(kws_gemm_tn_gather_f32(x, &gather1f, Gb[0], ws + lo.g1f, B, C1, ws + lo.tn, st));
      KWS_TRY(unfold_conv1(ws + lo.g1f, grads, st));
    }
  }
  return KWS_OK;
}

}  // namespace

extern "C" {

int kws_net_create(const kws_net_config_t* cfg, kws_net_t** out) {
  KWS_REQUIRE(cfg && out, "net_create: NULL pointer");
  KWS_REQUIRE(cfg->num_classes >= 2 && cfg->num_classes <= 64, "net: num_classes %d out of range", cfg->num_classes);
  kws_net* n = new kws_net();
  n->cfg = *cfg;
  int rc;
  switch (cfg->kind) {   // the one place that knows which program a kind runs on: its builder installs it as n->program
    case KWS_NET_TS_ATTENTION: rc = ts_build(n); break;
    case KWS_NET_LOG_MFCC: rc = lm_build(n); break;
    case KWS_NET_STEFFE: rc = steffe_build(n); break;
    case KWS_NET_RESIDUAL: rc = residual_build(n); break;
    case KWS_NET_MFCC_AND_RAW: rc = mfcc_raw_build(n); break;
    case KWS_NET_CONV_1D_FAST:
    case KWS_NET_CONV_1D_SPEC:
    case KWS_NET_CONV_1D_TIME_STACKED:
    case KWS_NET_CONV_1D_HEAVY:
    case KWS_NET_CONV_1D_LEARNED_SPEC:
    case KWS_NET_CONV_1D_TOP_DOWN: rc = gc_build(n); break;
    case KWS_NET_CONV_1D_GRU:
    case KWS_NET_CONV_1D_SIMPLE: rc = dk_build(n); break;
    case KWS_NET_XCEPTION_ATTENTION: rc = xception_build(n); break;
    case KWS_NET_CONV_1D_MULTI_TIME_SLICED: rc = mt_build(n); break;
    case KWS_NET_INCEPTION_D1: rc = inc_build(n); break;
    case KWS_NET_CONV_2D_MOBILE:
    case KWS_NET_CONV_2D_FAST: rc = c2n_build(n); break;
    case KWS_NET_CONV_1D_TIME_SLICED: rc = tsl_build(n); break;
    default:
      kws_set_error("net_create: kind %d not supported", cfg->kind);
      rc = KWS_E_INVALID;
  }
  if (rc != KWS_OK) {
    delete n;
    return rc;
  }
  *out = n;
  return KWS_OK;
}

int kws_net_destroy(kws_net_t* net) {
  delete net;
  return KWS_OK;
}

int64_t kws_net_num_params(const kws_net_t* net) { return net ? net->n_params : 0; }
int64_t kws_net_num_state(const kws_net_t* net) { return net ? net->n_state : 0; }
int kws_net_num_tensors(const kws_net_t* net) { return net ? (int)net->tensors.size() : 0; }

int kws_net_tensor_info(const kws_net_t* net, int idx, kws_tensor_info_t* info) {
  KWS_REQUIRE(net && info && idx >= 0 && idx < (int)net->tensors.size(), "net_tensor_info: bad index %d", idx);
  *info = net->tensors[idx];
  return KWS_OK;
}

int64_t kws_net_workspace_bytes(const kws_net_t* net, int max_batch, int training) {
  if (!net || max_batch <= 0) return 0;
  return net->program->workspace_bytes(max_batch, training);
}

int kws_net_debug_view(const kws_net_t* net, int batch, int training, int what, int index, int64_t* offset_floats,
                       int64_t* count) {
  KWS_REQUIRE(net && offset_floats && count && batch > 0, "net_debug_view: bad arguments");
  return net->program->debug_view(batch, training, what, index, offset_floats, count);
}

int kws_net_predict(const kws_net_t* net, const float* params, const float* state, const float* x, int B,
                    float* probs, void* workspace, int64_t workspace_bytes, void* stream) {
  KWS_REQUIRE(net && params && state && x && probs && workspace && B > 0, "net_predict: bad arguments");
  return net->program->predict(params, state, x, B, probs, (float*)workspace, workspace_bytes, (hipStream_t)stream);
}

// Arithmetic of the pointwise GEMMs of ONE net handle: 0 = f32 MFMA (the product path), 2 = power-of-two scaled fp16 x 2 split
// products (A/B arm, gemm_f16x2.hip).  Kept on the handle (no process-wide switch); bench.py's A/B leg flips it between steps.
extern "C" int kws_net_get_gemm_mode(const kws_net_t* net) { return net ? net->gemm_mode.load(std::memory_order_relaxed) : 0; }
extern "C" int kws_net_set_gemm_mode(kws_net_t* net, int mode) {
  KWS_REQUIRE(net != nullptr, "net_set_gemm_mode: NULL net");
  KWS_REQUIRE(mode >= 0 && mode <= 2,
              "net_set_gemm_mode: mode %d (0 = f32 MFMA, 1 = f32 MFMA with separate input- / weight-gradient launches, 2 = fp16 x 2 split)", mode);
  net->gemm_mode.store(mode, std::memory_order_relaxed);
  return KWS_OK;
}

int kws_net_train_fwd_bwd(const kws_net_t* net, const float* params, float* state, const float* x,
                          const float* y_onehot, int B, float* grads, float* probs, float* metrics, uint64_t seed,
                          uint32_t step, int64_t row_offset, int loss_batch, void* workspace, int64_t workspace_bytes,
                          void* stream) {
  KWS_REQUIRE(net && params && state && x && y_onehot && grads && probs && metrics && workspace && B > 0,
              "net_train_fwd_bwd: bad arguments");
  KWS_REQUIRE(loss_batch >= B, "net_train_fwd_bwd: loss_batch %d < B %d", loss_batch, B);
  return net->program->train(params, state, x, y_onehot, B, grads, probs, metrics, seed, step, row_offset, loss_batch, (float*)workspace,
                             workspace_bytes, (hipStream_t)stream);
}

// the raw-waveform attention net's program, NULL for every other kind (the split step exists for it alone)
static const TsProgram* ts_program(const kws_net_t* net) {
  return (net && net->cfg.kind == KWS_NET_TS_ATTENTION) ? static_cast<const TsProgram*>(net->program.get()) : nullptr;
}

int kws_net_num_blocks(const kws_net_t* net) {
  const TsProgram* ts = ts_program(net);
  return ts ? ts->lad.nb() : 0;
}

int64_t kws_net_grad_ready_offset(const kws_net_t* net, int split_block) {
  const TsProgram* ts = ts_program(net);
  if (!ts || split_block < 1 || split_block >= ts->lad.nb()) return -1;
  // block `split_block`'s backward writes the gradients of the BatchNorm in front of it; everything from there to the end
  // of the flat buffer (Keras layer order) is final once part 1 has run
  return ts->lad.blocks[split_block - 1].bn.gamma;
}

int kws_net_train_fwd_bwd_part(const kws_net_t* net, const float* params, float* state, const float* x,
                               const float* y_onehot, int B, float* grads, float* probs, float* metrics, uint64_t seed,
                               uint32_t step, int64_t row_offset, int loss_batch, void* workspace,
                               int64_t workspace_bytes, int part, int split_block, void* stream) {
  KWS_REQUIRE(net && params && state && x && y_onehot && grads && probs && metrics && workspace && B > 0,
              "net_train_fwd_bwd_part: bad arguments");
  KWS_REQUIRE(loss_batch >= B, "net_train_fwd_bwd_part: loss_batch %d < B %d", loss_batch, B);
  KWS_REQUIRE(net->cfg.kind == KWS_NET_TS_ATTENTION, "net_train_fwd_bwd_part: only the raw-waveform attention net is split");
  const TsProgram* ts = ts_program(net);
  KWS_REQUIRE((part == 1 || part == 2) && split_block >= 1 && split_block < ts->lad.nb(),
              "net_train_fwd_bwd_part: part %d split_block %d", part, split_block);
  return ts->train_part(params, state, x, y_onehot, B, grads, probs, metrics, seed, step, row_offset, loss_batch, (float*)workspace,
                        workspace_bytes, (hipStream_t)stream, part, split_block);
}

}  // extern "C"
