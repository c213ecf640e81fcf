// Network programs of the general depthwise ladder:
//   KWS_NET_CONV_1D_GRU  conv_1d_gru_model (reference model.py:470-512; Keras model name 'conv_1d_bigru', no recurrent layer):
//                        raw waveform as [16000, 1] -> six _depthwise_conv_block (DepthwiseConv2D((1, k), strides=s, l2 1e-5) ->
//                        Conv1D(F, 1, l2 1e-5) -> BatchNormalization -> relu6) with k 63 / 31 / 15 / 7 / 5 SAME at strides
//                        16 / 4 / 4 / 4 / 2 and k 8 VALID, F = 128 / 256 / 384 / 448 / 512 / 512 -> Flatten (one time step) ->
//                        Dropout(.3) -> Dense(256) -> relu6 -> Dropout(.3) -> Dense + softmax; RMSprop(1e-3), categorical CE
//   KWS_NET_CONV_1D_SIMPLE  conv_1d_simple_model (reference model.py:116-156; Keras model name 'conv_1d_time_stacked'): raw waveform as
//                        [16000, 1] -> fourteen such blocks, all VALID: k 31 at stride 16, then k 3 at strides 1, 2, 1, 2, 1, ...;
//                        F = 32, 32, 64, 64, 96, 96 .. 224, 224; ends at [B, 10, 224] -> Bidirectional(GRU(128, dropout=.2,
//                        recurrent_dropout=.2)) (gru.hip) -> Dense + softmax; Adam(1e-3), categorical CE.  No l2 on the GRU or the Dense
//                        layer.  The activated ladder output is materialised for the GRU's GEMMs (kws_bn_relu6_apply), its masked
//                        views by kws_gru_fwd_f32; the head is the flat tail's raw arm over the signed [B, 256] GRU output.
// The blocks and their data flow are net_sepblock.hip's.  Block 1 has one input channel: its depthwise layer is the C = 1 arm and
// its pointwise layer the outer product kws_dwconvk_pw1_* (K = 1 is outside the GEMM).
// The hidden Dense layer is a GEMM over the materialised dropped features; its bias, relu6 and Dropout run inside the flat tail,
// which reads (h, table) with the table scale = 1 | shift = bias (fmaf(h, 1, b) = h + b exactly).
#include "net_internal.h"

namespace {

struct DkLayout {
  int64_t total = 0;
  std::vector<int64_t> z, y, bn;
  int64_t stats = 0, red = 0, fa = 0, fd1 = 0, h = 0, tab = 0;
  int64_t G[2] = {0, 0}, DZ = 0, part = 0, coef = 0, tn = 0, WT = 0, pw1ws = 0;
  FlatTailWs tail;
  int64_t bpart = 0;
  int64_t gmx = 0, gmh = 0, gout = 0, gsave = 0, gws = 0, gdout = 0;   // KWS_NET_CONV_1D_SIMPLE
};

struct DkProgram : FlatTailProgram<DkLayout> {
  std::vector<SepBlock> blocks;
  int D = 0, H = 0;                  // features into the head, hidden width
  int64_t d1k = 0, d1b = -1;
  float keep = 0.7f;
  // KWS_NET_CONV_1D_SIMPLE: the ladder ends in gT steps of D channels, a bidirectional GRU of gH units follows (H = 0: no hidden Dense)
  bool gru = false;
  int gT = 0, gH = 0;
  int64_t gW[2] = {0, 0}, gU[2] = {0, 0}, gb[2] = {0, 0};

  void layout(int B, bool training, DkLayout* lo) const override;
  int forward(const DkLayout& lo, const NetCall& c) const override;
  kws_flat_tail_args tail_args(const DkLayout& lo, const NetCall& c, float* probs) const override;
  int64_t tail_grad(const DkLayout& lo) const override { return gru ? lo.gdout : lo.G[0]; }
  int backward(const DkLayout& lo, const NetCall& c) const override;
  int debug_view(int B, int training, int what, int index, int64_t* offset_floats, int64_t* count) const override;
};

constexpr float DK_DROP_KEEP = 0.7f;   // Dropout(0.3), model.py:502, 504
constexpr int DK_HIDDEN = 256;         // Dense(256), model.py:503
constexpr int DK_GRU_UNITS = 128;      // GRU(128, ...), model.py:148
constexpr float DK_GRU_KEEP = 0.8f;    // dropout=0.2, recurrent_dropout=0.2

// tab [4][n] = 1 | bias (0 without one) | 0 | 1: what the flat tail reads as a BatchNorm table
__global__ __launch_bounds__(256) void dk_bias_table_kernel(const float* __restrict__ bias, int n, float* __restrict__ tab) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  tab[i] = 1.f;
  tab[n + i] = bias ? bias[i] : 0.f;
  tab[2 * n + i] = 0.f;
  tab[3 * n + i] = 1.f;
}

// d[b, i] *= relu6'(h[b, i] + bias[i]) in place; slice blockIdx.y adds its rows of the result, ascending, into part[slice][n]
__global__ __launch_bounds__(256) void dk_bias_relu6_bwd_kernel(float* __restrict__ d, const float* __restrict__ h,
                                                                const float* __restrict__ bias, int B, int n, int rows_per,
                                                                float* __restrict__ part) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float bi = bias ? bias[i] : 0.f;
  const int b0 = blockIdx.y * rows_per;
  const int b1 = b0 + rows_per < B ? b0 + rows_per : B;
  float sum = 0.f;
  for (int b = b0; b < b1; ++b) {
    const float pre = h[(int64_t)b * n + i] + bi;
    const float v = (pre > 0.f && pre <= 6.f) ? d[(int64_t)b * n + i] : 0.f;
    d[(int64_t)b * n + i] = v;
    sum += v;
  }
  part[(int64_t)blockIdx.y * n + i] = sum;
}

__global__ __launch_bounds__(256) void dk_bias_grad_fold_kernel(const float* __restrict__ part, int slices, int n,
                                                                float* __restrict__ dbias) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float sum = 0.f;
  for (int s = 0; s < slices; ++s) sum += part[(int64_t)s * n + i];
  dbias[i] = sum;
}

}  // namespace

// (declared in net_internal.h: net_time_sliced.hip's head is this one without the bias)
int dk_bias_table(const float* bias, int n, float* tab, hipStream_t st) {
  hipLaunchKernelGGL(dk_bias_table_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, bias, n, tab);
  KWS_LAUNCH_CHECK("dk_bias_table_kernel");
  return KWS_OK;
}

// the hidden layer's backward through bias + relu6: gradient wrt relu6(h + bias) -> gradient wrt h, in place; dbias may be NULL
// (a hidden layer without bias: conv_1d_time_sliced has this head with use_bias=False)
int dk_bias_relu6_bwd(float* d, const float* h, const float* bias, float* dbias, int B, int n, float* part, hipStream_t st) {
  const int rows_per = ceil_div(B, DK_BIAS_SLICES);
  const int slices = ceil_div(B, rows_per);
  hipLaunchKernelGGL(dk_bias_relu6_bwd_kernel, dim3((unsigned)ceil_div(n, 256), (unsigned)slices), dim3(256), 0, st, d, h, bias, B, n,
                     rows_per, part);
  KWS_LAUNCH_CHECK("dk_bias_relu6_bwd_kernel");
  if (dbias) {
    hipLaunchKernelGGL(dk_bias_grad_fold_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, part, slices, n, dbias);
    KWS_LAUNCH_CHECK("dk_bias_grad_fold_kernel");
  }
  return KWS_OK;
}

int dk_dense_bwd(float* d, const float* h, const float* in, const float* W, const float* bias, float* dW, float* dbias, float* out, int B,
                 int D, int H, const DkDenseBwdScratch& s, hipStream_t st) {
  KWS_TRY(dk_bias_relu6_bwd(d, h, bias, dbias, B, H, s.part, st));
  KWS_TRY(kws_gemm_tn_f32(in, d, dW, B, D, H, s.tn, st));
  KWS_TRY(kws_transpose_f32(W, s.WT, D, H, st));
  return kws_gemm_nn_f32(d, s.WT, out, B, H, D, nullptr, st);
}

namespace {

void DkProgram::layout(int B, bool training, DkLayout* lo) const {
  const DkProgram& p = *this;
  Bump bp;
  const int nb = (int)p.blocks.size();
  int64_t max_y = 64, max_z = 64, max_stats = 64, max_part = 64, max_tn = 64, max_w = 64;
  int maxC = 4;
  lo->z.assign(nb, 0);
  lo->y.assign(nb, 0);
  lo->bn.assign(nb, 0);
  for (int i = 0; i < nb; ++i) {
    const SepBlock& b = p.blocks[i];
    const int64_t M = (int64_t)B * b.Lout;
    lo->z[i] = bp.take(M * b.cin);
    lo->y[i] = bp.take(M * b.cout);
    lo->bn[i] = bp.take((int64_t)4 * b.cout);
    max_y = std::max(max_y, std::max(M * b.cout, (int64_t)B * b.Lin * b.cin));
    max_z = std::max(max_z, M * b.cin);
    maxC = std::max(maxC, b.cout);
    max_stats = std::max(max_stats, (int64_t)2 * b.cout * (i == 0 ? kws_dwconvk_pw1_stats_rows(M) : kws_gemm_num_row_tiles(M)));
    max_part = std::max(max_part, kws_dwconvk_bwd_part_floats(B, b.Lin, b.cin, b.k, b.stride));
    if (i > 0) {
      max_tn = std::max(max_tn, kws_gemm_tn_workspace_floats(M, b.cin, b.cout));
      max_w = std::max(max_w, (int64_t)b.cin * b.cout);
    }
  }
  if (p.gru) {
    const int T = p.gT, I = p.D, H = p.gH;
    max_part = std::max(max_part, (int64_t)kws_gbn_bwd_rows((int64_t)B * T) * 2 * I);
    lo->stats = bp.take(max_stats);
    lo->red = bp.take((int64_t)KWS_REDUCE_SLICES * 2 * maxC);
    lo->fa = bp.take((int64_t)B * T * I);
    lo->gout = bp.take((int64_t)B * 2 * H);
    lo->gws = bp.take(kws_gru_workspace_floats(B, T, I, H, training ? 1 : 0));
    if (training) {
      lo->gmx = bp.take((int64_t)6 * B * I);
      lo->gmh = bp.take((int64_t)6 * B * H);
      lo->gsave = bp.take(kws_gru_save_floats(B, T, H));
      lo->gdout = bp.take((int64_t)B * 2 * H);
      lo->G[0] = bp.take(max_y);
      lo->G[1] = bp.take(max_y);
      lo->DZ = bp.take(max_z);
      lo->part = bp.take(max_part);
      lo->coef = bp.take((int64_t)2 * maxC);
      lo->tn = bp.take(max_tn);
      lo->WT = bp.take(max_w);
      lo->pw1ws = bp.take(kws_dwconvk_pw1_bwd_workspace_floats((int64_t)B * p.blocks[0].Lout, p.blocks[0].cout));
      lo->tail.take(bp, B, dense.D, dense.NC);
    }
    lo->total = bp.cur * 4;
    return;
  }
  max_stats = std::max(max_stats, (int64_t)2 * p.H * kws_gemm_num_row_tiles(B));
  max_part = std::max(max_part, (int64_t)kws_gbn_bwd_rows(B) * 2 * p.D);
  max_tn = std::max(max_tn, kws_gemm_tn_workspace_floats(B, p.D, p.H));
  max_w = std::max(max_w, (int64_t)p.D * p.H);
  lo->stats = bp.take(max_stats);
  lo->red = bp.take((int64_t)KWS_REDUCE_SLICES * 2 * maxC);
  lo->fa = bp.take((int64_t)B * p.D);
  lo->h = bp.take((int64_t)B * p.H);
  lo->tab = bp.take((int64_t)4 * p.H);
  if (training) {
    lo->fd1 = bp.take((int64_t)B * p.D);
    lo->G[0] = bp.take(max_y);
    lo->G[1] = bp.take(max_y);
    lo->DZ = bp.take(max_z);
    lo->part = bp.take(max_part);
    lo->coef = bp.take((int64_t)2 * maxC);
    lo->tn = bp.take(max_tn);
    lo->WT = bp.take(max_w);
    lo->pw1ws = bp.take(kws_dwconvk_pw1_bwd_workspace_floats((int64_t)B * p.blocks[0].Lout, p.blocks[0].cout));
    lo->tail.take(bp, B, dense.D, dense.NC);
    lo->bpart = bp.take((int64_t)DK_BIAS_SLICES * p.H);
  }
  lo->total = bp.cur * 4;
}

// forward through the blocks and the hidden Dense product; training: batch statistics (moving averages updated) and dropout
int DkProgram::forward(const DkLayout& lo, const NetCall& c) const {
  const DkProgram& p = *this;
  const float* params = c.params;
  float* state = c.state;
  const float* x = c.x;
  float* ws = c.ws;
  const int B = c.B;
  const bool training = c.training;
  hipStream_t st = c.st;
  const int nb = (int)p.blocks.size();
  for (int i = 0; i < nb; ++i) {
    const SepBlock& b = p.blocks[i];
    const int64_t M = (int64_t)B * b.Lout;
    const float* in = i == 0 ? x : ws + lo.y[i - 1];
    const float* bn_in = i == 0 ? nullptr : ws + lo.bn[i - 1];
    float* stats = training ? ws + lo.stats : nullptr;
    int rows;
    if (i == 0) {
      KWS_TRY(kws_dwconvk_fwd_f32(in, bn_in, params + b.dw, ws + lo.z[i], B, b.Lin, b.Lout, b.cin, b.k, b.stride, b.pad_l, st));
      KWS_TRY(kws_dwconvk_pw1_fwd_f32(ws + lo.z[i], params + b.pw, ws + lo.y[i], M, b.cout, stats, st));
      rows = kws_dwconvk_pw1_stats_rows(M);
    } else {
      rows = kws_sep_fwd(b, params, in, bn_in, ws + lo.z[i], ws + lo.y[i], stats, B, st);
      if (rows < 0) return rows;
    }
    KWS_TRY(kws_sep_bn_table(b, params, state, stats, rows, M, training, ws + lo.bn[i], ws + lo.red, st));
  }
  if (p.gru) {   // the activated ladder output [B, T, I] is materialised for the GRU's GEMMs; masks only in training
    const int T = p.gT, I = p.D, H = p.gH;
    KWS_TRY(kws_bn_relu6_apply(ws + lo.y[nb - 1], ws + lo.bn[nb - 1], ws + lo.fa, (int64_t)B * T, I, 1, st));
    if (training) KWS_TRY(kws_gru_masks(ws + lo.gmx, ws + lo.gmh, B, I, H, DK_GRU_KEEP, c.seed, c.step, c.row_offset, st));
    return kws_gru_fwd_f32(ws + lo.fa, params + p.gW[0], params + p.gU[0], params + p.gb[0], params + p.gW[1], params + p.gU[1],
                           params + p.gb[1], training ? ws + lo.gmx : nullptr, training ? ws + lo.gmh : nullptr, ws + lo.gout,
                           training ? ws + lo.gsave : nullptr, ws + lo.gws, B, T, I, H, st);
  }
  // Flatten (one time step) -> Dropout -> Dense(H): the features are materialised for the GEMMs
  KWS_TRY(kws_bn_relu6_apply(ws + lo.y[nb - 1], ws + lo.bn[nb - 1], ws + lo.fa, B, p.D, 1, st));
  const float* feat = ws + lo.fa;
  if (training) {
    KWS_TRY(kws_dropout_fwd(ws + lo.fa, ws + lo.fd1, B, p.D, p.keep, c.seed, c.step, 1, c.row_offset, st));
    feat = ws + lo.fd1;
  }
  KWS_TRY(kws_gemm_nn_f32(feat, params + p.d1k, ws + lo.h, B, p.D, p.H, nullptr, st));
  return dk_bias_table(p.d1b >= 0 ? params + p.d1b : nullptr, p.H, ws + lo.tab, st);
}

// bias + relu6 + Dropout (layer 2) of the hidden layer, Dense + softmax (+ loss and its backward): the flat tail over (h, table)
kws_flat_tail_args DkProgram::tail_args(const DkLayout& lo, const NetCall& c, float* probs) const {
  const DkProgram& p = *this;
  float* ws = c.ws;
  kws_flat_tail_args t;
  memset(&t, 0, sizeof(t));
  t.Wd = c.params + dense.kernel; t.bd = c.params + dense.bias;
  t.probs = probs;
  t.B = c.B; t.D = dense.D; t.F = dense.D; t.NC = dense.NC; t.Ng = dense.D;
  if (p.gru) {   // Dense + softmax over the signed GRU output: the raw arm
    t.y = ws + lo.gout; t.raw = 1;
    t.keep_prob = 1.f;
    return t;
  }
  t.y = ws + lo.h; t.bn = ws + lo.tab;
  t.keep_prob = p.keep;
  t.layer_id = 2;
  return t;
}

// conv_1d_simple: _reduce_conv(x, 32, 31, strides=16), _context_conv(x, 32, 3), then for F in 64 .. 224: _reduce_conv(x, F, 3) (stride 2),
// _context_conv(x, F, 3), all padding='valid' (model.py:142-146) -> Bidirectional(GRU(128)) -> Dense
int dk_build_simple(kws_net* n) {
  const kws_net_config_t& c = n->cfg;
  KWS_REQUIRE(c.input_size == 16000, "net: conv_1d_simple input_size %d (the reference's ladder ends in 10 time steps for 16000 samples)",
              c.input_size);
  DkProgram* p = new DkProgram();
  n->program.reset(p);
  p->net = n;
  p->dense.NC = c.num_classes;
  p->zero_grads = true;   // the padding behind a tensor of 63 taps stays zero
  p->gru = true;
  KerasNames kn{n};
  int L = c.input_size, cin = 1;
  for (int i = 0; i < 14; ++i) {
    SepBlock b;
    b.Lin = L; b.k = i == 0 ? 31 : 3; b.stride = i == 0 ? 16 : (i % 2 == 0 ? 2 : 1); b.cin = cin; b.cout = i < 2 ? 32 : 32 * (i / 2 + 1);
    KWS_REQUIRE(L >= b.k, "net: block %d input length %d < %d taps", i, L, b.k);
    b.Lout = (L - b.k) / b.stride + 1;
    b.pad_l = 0;
    b.dw = kn.dwk(b.k, cin);
    b.pw = kn.conv(1, cin, b.cout, KWS_L2_COEF);
    b.bn = kn.bn(b.cout);
    p->blocks.push_back(b);
    L = b.Lout;
    cin = b.cout;
  }
  KWS_REQUIRE(L == 10 && cin == 224, "net: conv_1d_simple ladder ends at [%d, %d], the GRU reads [10, 224]", L, cin);
  p->D = cin;
  p->gT = L;
  p->gH = DK_GRU_UNITS;
  const int H = p->gH;
  for (int d = 0; d < 2; ++d) {   // recurrent_kernel: Keras's Orthogonal initialiser, drawn by the host (fan_in = 0 here)
    const std::string base = std::string("bidirectional_1/") + (d ? "backward" : "forward") + "_gru_1/";
    p->gW[d] = kws_net_add_tensor(n, base + "kernel", {p->D, 3 * H}, false, 0.f, p->D, 3 * H, 0.f);
    p->gU[d] = kws_net_add_tensor(n, base + "recurrent_kernel", {H, 3 * H}, false, 0.f, 0, 0, 0.f);
    p->gb[d] = kws_net_add_tensor(n, base + "bias", {3 * H}, false, 0.f, 0, 0, 0.f);
  }
  p->dense.D = 2 * H;
  p->dense.kernel = kws_net_add_tensor(n, "dense_1/kernel", {2 * H, c.num_classes}, false, 0.f, 2 * H, c.num_classes, 0.f);
  p->dense.bias = kws_net_add_tensor(n, "dense_1/bias", {c.num_classes}, false, 0.f, 0, 0, 0.f);
  return KWS_OK;
}

}  // namespace

int dk_build(kws_net* n) {
  const kws_net_config_t& c = n->cfg;
  if (c.kind == KWS_NET_CONV_1D_SIMPLE) return dk_build_simple(n);
  KWS_REQUIRE(c.input_size == 16000, "net: conv_1d_gru input_size %d (the reference's ladder ends in one time step for 16000 samples)",
              c.input_size);
  DkProgram* p = new DkProgram();
  n->program.reset(p);
  p->net = n;
  p->dense.NC = c.num_classes;
  p->zero_grads = true;   // the padding behind a tensor of 63 taps stays zero
  p->keep = DK_DROP_KEEP;
  KerasNames kn{n};
  // _reduce_conv(x, F, k, strides) padding='same' x 5, _context_conv(x, 512, 8) padding='valid' (model.py:495-500)
  static const struct { int F, k, s; bool same; } spec[6] = {{128, 63, 16, true}, {256, 31, 4, true}, {384, 15, 4, true},
                                                             {448, 7, 4, true},   {512, 5, 2, true},  {512, 8, 1, false}};
  int L = c.input_size, cin = 1;
  for (int i = 0; i < 6; ++i) {
    SepBlock b;
    b.Lin = L; b.k = spec[i].k; b.stride = spec[i].s; b.cin = cin; b.cout = spec[i].F;
    if (spec[i].same) {
      kws_same_pad(L, b.k, b.stride, &b.Lout, &b.pad_l);
    } else {
      KWS_REQUIRE(L >= b.k, "net: block %d input length %d < %d taps", i, L, b.k);
      b.Lout = (L - b.k) / b.stride + 1;
      b.pad_l = 0;
    }
    b.dw = kn.dwk(b.k, cin);
    b.pw = kn.conv(1, cin, b.cout, KWS_L2_COEF);
    b.bn = kn.bn(b.cout);
    p->blocks.push_back(b);
    L = b.Lout;
    cin = b.cout;
  }
  KWS_REQUIRE(L == 1, "net: conv_1d_gru ladder ends with %d time steps, the head flattens 1", L);
  p->D = cin;
  p->H = DK_HIDDEN;
  p->d1k = kws_net_add_tensor(n, "dense_1/kernel", {p->D, p->H}, false, 0.f, p->D, p->H, 0.f);
  p->d1b = kws_net_add_tensor(n, "dense_1/bias", {p->H}, false, 0.f, 0, 0, 0.f);
  p->dense.D = p->H;
  p->dense.kernel = kws_net_add_tensor(n, "dense_2/kernel", {p->H, c.num_classes}, false, 0.f, p->H, c.num_classes, 0.f);
  p->dense.bias = kws_net_add_tensor(n, "dense_2/bias", {c.num_classes}, false, 0.f, 0, 0, 0.f);
  return KWS_OK;
}

namespace {

int DkProgram::debug_view(int B, int training, int what, int index, int64_t* offset_floats, int64_t* count) const {
  const DkProgram& p = *this;
  DkLayout lo;
  layout(B, training != 0, &lo);
  const int nb = (int)p.blocks.size();
  if (p.gru && what == 5) {   // the GRU's saved steps [2][4: z, r, c, h][B, T, H] (training)
    KWS_REQUIRE(training, "net_debug_view: view 5 exists in training only");
    *offset_floats = lo.gsave;
    *count = kws_gru_save_floats(B, p.gT, p.gH);
    return KWS_OK;
  }
  if (p.gru && what == 6) {   // the GRU output [B, 2H]
    *offset_floats = lo.gout;
    *count = (int64_t)B * 2 * p.gH;
    return KWS_OK;
  }
  if (what == 4 && !p.gru) {   // the hidden Dense layer's output before its bias [B, H]
    *offset_floats = lo.h;
    *count = (int64_t)B * p.H;
    return KWS_OK;
  }
  KWS_REQUIRE(index >= 0 && index < nb, "net_debug_view: block index %d", index);
  const SepBlock& b = p.blocks[index];
  if (what == 0) {          // raw pointwise output of block `index`
    *offset_floats = lo.y[index];
    *count = (int64_t)B * b.Lout * b.cout;
  } else if (what == 1) {   // depthwise output of block `index`
    *offset_floats = lo.z[index];
    *count = (int64_t)B * b.Lout * b.cin;
  } else if (what == 2) {   // table of batch_normalization_{index+1}
    *offset_floats = lo.bn[index];
    *count = (int64_t)4 * b.cout;
  } else {
    kws_set_error("net_debug_view: unknown view %d", what);
    return KWS_E_INVALID;
  }
  return KWS_OK;
}

// everything behind the Dense + softmax layer's weight gradient: the GRU or the hidden Dense layer, then the blocks
int DkProgram::backward(const DkLayout& lo, const NetCall& c) const {
  const DkProgram& p = *this;
  const float* params = c.params;
  const float* x = c.x;
  float* grads = c.grads;
  float* ws = c.ws;
  const int B = c.B;
  hipStream_t st = c.st;
  const int nb = (int)p.blocks.size();
  float* G[2] = {ws + lo.G[0], ws + lo.G[1]};
  float* part = ws + lo.part;
  float* coef = ws + lo.coef;
  const SepBwdScratch scratch = {ws + lo.WT, ws + lo.DZ, ws + lo.tn, part, coef};
  int cur = 0;   // G[cur] = gradient wrt the activated output of the last block [B, T, D]
  if (p.gru) {
    const int T = p.gT, I = p.D, H = p.gH;
    const SepBlock& b = p.blocks[nb - 1];
    KWS_TRY(kws_gru_bwd_f32(ws + lo.gdout, ws + lo.fa, params + p.gW[0], params + p.gU[0], params + p.gW[1], params + p.gU[1], ws + lo.gmx,
                            ws + lo.gmh, ws + lo.gsave, G[0], grads + p.gW[0], grads + p.gU[0], grads + p.gb[0], grads + p.gW[1],
                            grads + p.gU[1], grads + p.gb[1], ws + lo.gws, B, T, I, H, st));
    KWS_TRY(kws_gbn_layer_bwd(G[cur], ws + lo.y[nb - 1], ws + lo.bn[nb - 1], nullptr, (int64_t)B * T, kws_gbn_grouped(1, b.cout), part,
                              coef, grads, b.bn, st));
  } else {
    // G[0] = gradient wrt relu6(h + b1) [B, H] -> wrt h; dense_1's gradients; back through Dropout(.3) onto the activated features
    KWS_TRY(dk_dense_bwd(G[0], ws + lo.h, ws + lo.fd1, params + p.d1k, p.d1b >= 0 ? params + p.d1b : nullptr, grads + p.d1k,
                         p.d1b >= 0 ? grads + p.d1b : nullptr, G[1], B, p.D, p.H, {ws + lo.WT, ws + lo.tn, ws + lo.bpart}, st));
    KWS_TRY(kws_dropout_bwd(G[1], G[0], B, p.D, p.keep, c.seed, c.step, 1, c.row_offset, st));
    const SepBlock& b = p.blocks[nb - 1];
    KWS_TRY(kws_gbn_layer_bwd(G[cur], ws + lo.y[nb - 1], ws + lo.bn[nb - 1], nullptr, B, kws_gbn_grouped(1, b.cout), part, coef, grads,
                              b.bn, st));
  }
  // ---- blocks: G[cur] = dy of block i's pointwise output ----
  for (int i = nb - 1; i >= 1; --i) {
    const SepBlock& b = p.blocks[i];
    KWS_TRY(kws_sep_bwd(b, params, grads, G[cur], ws + lo.z[i], ws + lo.y[i - 1], ws + lo.bn[i - 1], &p.blocks[i - 1].bn, G[cur ^ 1],
                        scratch, B, st));
    cur ^= 1;
  }
  {   // block 1: the outer product's backward, then the taps of the one-channel depthwise layer (no gradient leaves the input)
    const SepBlock& b = p.blocks[0];
    const int64_t M = (int64_t)B * b.Lout;
    KWS_TRY(kws_dwconvk_pw1_bwd_f32(G[cur], ws + lo.z[0], params + b.pw, scratch.DZ, grads + b.pw, M, b.cout, ws + lo.pw1ws, st));
    KWS_TRY(kws_sep_dw_bwd(b, params, grads, x, nullptr, nullptr, G[cur ^ 1], scratch, B, st));
  }
  return KWS_OK;
}

}  // namespace
